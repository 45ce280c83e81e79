"""
Every route of the general sparse product (csrc/spgemm.hip: sixteen- and thirty-two-lane hash tables, the workgroup hash
table, column strips in one and two passes, expand-sort-compress, LDS tiles, the 8192-slot hash table, HBM work rows; FAST
and general form; csrc/spgemm_order.hip's tiers) with rows on both sides of every threshold between them, through the public
entries K.mult_ab / K.mult_abt.  The cases, their preconditions and the restated routing come from tests/spgemm_cases.py
(tests/test_spgemm_cases_host.py checks them, and the module's NumPy product against the oracle, without a GPU).

No case can pass on another route than the one it was written for: after every product csrk_spgemm_last_stats -- what the
driver did with the rows -- must equal the module's census field by field.  The result is compared with the oracle's
sequential loop: row pointers and column indices exactly, in ascending and in the reference's order; the values' bits exactly
whenever no row of the right operand as multiplied holds a column twice, within 1e-12 of sum |a| |b| otherwise; and two runs
give the same bits.

Not covered (no small input reaches them): the memory-budget fallbacks SGE_BUDGET_PRODUCTS, the hipMemGetInfo check,
SGS_TABLE_BUDGET, SGS_TEMP_BUDGET and nrows * strips > 2^30 -- their arithmetic (csrc/spgemm_plan.h) is checked on the
host, tests/test_spgemm_plan_host.py.  The dense-panel route of mult_ab has its own tests.
"""
import numpy as np
import pytest

import spgemm_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture
def order():
    "set_spgemm_order for the duration of a test; the environment's order afterwards"
    from csr_amd.kernels import hip as K
    yield K.set_spgemm_order
    K.set_spgemm_order(None)


def _multiply(K, c):
    from csr_amd import CSR
    ah = K.to_handle(CSR(c.a.nrows, c.a.ncols, c.a.nnz, c.a.rowptrs, c.a.colinds, c.a.values, _cast=False))
    bh = K.to_handle(CSR(c.b.nrows, c.b.ncols, c.b.nnz, c.b.rowptrs, c.b.colinds, c.b.values, _cast=False))
    try:
        ch = K.mult_abt(ah, bh) if c.abt else K.mult_ab(ah, bh)
        stats, route = K.spgemm_last_stats(), K.spgemm_last_route()
        try:
            return K.from_handle(ch), stats, route
        finally:
            K.release_handle(ch)
    finally:
        K.release_handle(ah)
        K.release_handle(bh)


def _check_census(K, c, stats, route):
    assert route == 'general', c.name
    wrong = {k: (stats[k], c.census[k]) for k in S.STATS if stats[k] != c.census[k]}
    assert not wrong, f'{c.name}: csrk_spgemm_last_stats against the census (got, expected): {wrong}'
    # the rows of route 0 by kernel, from the module's product counts and the LIBRARY's limits
    lim = K.spgemm_limits()
    n16, n32, n256 = S.small_classes(c.census['u'], c.census['route'], lim)
    kinds = list(c.census['small'].values())
    assert (n16, n32, n256) == (kinds.count(16), kinds.count(32), kinds.count(256)), c.name
    assert (not n32 or stats['mid_rows']) and (not n256 or stats['hash_rows']), c.name      # the kernels they need did run


@pytest.mark.parametrize('name', S.names())
def test_route(name, order, monkeypatch):
    from oracle import oracle as O
    from csr_amd.kernels import hip as K
    c = S.build(name)
    assert not S.failed_preconditions(c), (name, S.failed_preconditions(c))
    for k in S.ENV_KEYS.values():
        monkeypatch.delenv(k, raising=False)
    monkeypatch.delenv('CSRK_SPGEMM_DENSE', raising=False)
    for k, v in c.env().items():
        monkeypatch.setenv(k, v)
    r = O.transpose(*c.b.tup()) if c.abt else c.b.tup()
    _, _, crp, cci, cvs = O.mult_ab(c.a.tup(), r)
    _, _, _, _, cabs = O.mult_ab((c.a.nrows, c.a.ncols, c.a.rowptrs, c.a.colinds, np.abs(c.a.values)),
                                 (r[0], r[1], r[2], r[3], np.abs(r[4])))
    asc = np.lexsort((cci, np.repeat(np.arange(c.a.nrows), np.diff(crp))))
    for which in ('ascending', 'reference'):
        order(which)
        assert K.spgemm_order() == which
        rci, rvs, rabs = (cci[asc], cvs[asc], cabs[asc]) if which == 'ascending' else (cci, cvs, cabs)
        runs = []
        for _ in range(2):
            C, stats, route = _multiply(K, c)
            _check_census(K, c, stats, route)
            assert (C.nrows, C.ncols) == (c.a.nrows, c.r.ncols), (name, which)
            assert C.rowptrs.dtype == np.int32 and np.array_equal(C.rowptrs, crp), (name, which)
            assert C.colinds.dtype == np.int32 and np.array_equal(C.colinds, rci), (name, which)
            assert C.values.dtype == np.float64
            err = np.abs(C.values - rvs)
            print(f'{name} {which}: max |err| / sum|a||b| = {float(np.max(err / (rabs + 1e-300))) if len(err) else 0.0:.3e}, '
                  f'bit-equal {bool(np.array_equal(C.values.view(np.int64), rvs.view(np.int64)))}')
            if c.exact:
                bad = np.flatnonzero(C.values.view(np.int64) != rvs.view(np.int64))
                assert not len(bad), f'{name} {which}: {len(bad)} values differ in their bits, first at entry {bad[0]}: ' \
                                     f'{C.values[bad[0]]!r} instead of {rvs[bad[0]]!r}'
            else:
                assert np.all(err <= 1e-12 * rabs + 1e-300), (name, which)
            runs.append(C.values.view(np.int64).copy())
        assert np.array_equal(runs[0], runs[1]), f'{name} {which}: two runs differ in their bits'


def test_stats_are_zeroed_by_a_call_that_does_not_reach_the_product(order):
    "a dense-panel product and a failing call leave all-zero stats, not the previous product's"
    import ctypes as C
    from csr_amd import CSR, _lib
    from csr_amd.kernels import hip as K
    c = S.build('ladder')
    order('ascending')
    _, stats, _ = _multiply(K, c)
    assert stats['general'] == 1
    rng = np.random.default_rng(5)
    B = CSR(c.a.ncols, 3, c.a.ncols * 3, np.arange(0, c.a.ncols * 3 + 1, 3, dtype=np.int32),
            np.tile(np.arange(3, dtype=np.int32), c.a.ncols), rng.uniform(-1, 1, c.a.ncols * 3), _cast=False)
    ah = K.to_handle(CSR(c.a.nrows, c.a.ncols, c.a.nnz, c.a.rowptrs, c.a.colinds, c.a.values, _cast=False))
    bh = K.to_handle(B)
    try:
        K.release_handle(K.mult_ab(ah, bh))
        assert K.spgemm_last_route() == 'dense-panel' and K.spgemm_last_stats() == dict.fromkeys(S.STATS, 0)
        _multiply(K, c)
        out = _lib.handle_t(0)                    # (the C entry itself: 250 x 3 times 250 x 3 does not fit)
        assert _lib.lib.csrk_spgemm_ab(K._live(bh), K._live(bh), C.byref(out)) == _lib.ERR_INVALID and out.value == 0
        assert K.spgemm_last_stats() == dict.fromkeys(S.STATS, 0)
    finally:
        K.release_handle(ah)
        K.release_handle(bh)
