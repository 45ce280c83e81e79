"""
tests/spgemm_cases.py without a GPU: every case sits on the edge it is named for (its preconditions hold), the constants the
module routes by are the library's (csrk_spgemm_limits: the library loads without a device), the union of the censuses
covers every accumulator of csrc/spgemm.hip in both of its forms, and the module's plain NumPy product agrees with the
oracle's on every case -- row pointers and column sets exactly, values within 1e-12 of sum |a| |b|.
tests/test_gpu_spgemm_routes.py runs the library on the same cases.
"""
import numpy as np
import pytest

import spgemm_cases as S

ALL = S.names()


def test_names_are_unique_and_seeded_by_name():
    assert len(set(ALL)) == len(ALL) and len(S.CASES) >= 25
    a, b = S.build('ladder'), S.build('ladder')
    assert np.array_equal(a.a.colinds, b.a.colinds) and np.array_equal(a.b.values.view(np.int64), b.b.values.view(np.int64))
    assert not np.array_equal(S.build('ladder-two-pass').b.values, a.b.values)


def test_constants_are_the_librarys():
    from csr_amd.kernels import hip as K
    assert K.SPGEMM_LIMITS == tuple(S.LIMITS) and K.SPGEMM_STATS == S.STATS
    assert K.spgemm_limits() == S.LIMITS
    # what the module relies on between them: a 16-lane row's 32 products are ESC's threshold and lie below a 32-lane row's
    assert S.SG_QUAD_CAP == S.LIMITS['SGE_MIN'] < S.LIMITS['SG_WAVE_CAP'] < S.LIMITS['SG_CAP'] == S.LIMITS['SGE_TILE']


def test_stats_before_any_product_are_zero():
    "thread-local and zero until a product ran (nothing here needs a device)"
    import threading
    from csr_amd.kernels import hip as K
    got = []
    t = threading.Thread(target=lambda: got.append(K.spgemm_last_stats()))
    t.start()
    t.join()
    assert got == [dict.fromkeys(S.STATS, 0)]


@pytest.mark.parametrize('name', ALL)
def test_preconditions(name):
    c = S.build(name)
    assert not S.failed_preconditions(c), S.failed_preconditions(c)
    assert c.name == name and set(c.off) <= set(S.ENV_KEYS)
    assert c.r.ncols <= (1 << 20) + 1 and c.a.nrows <= 4096


def test_census_by_hand():
    "the routing restated once more on a matrix small enough to do by hand: one row per route"
    bld = S.Builder('by-hand', 832)
    bld.target(5, 5)                                   # 16 lanes
    bld.target(33, 11, disjoint=False)                 # ESC (32 lanes with ESC off)
    bld.target(1025, 205, disjoint=False)              # 5 entries, one strip: strip-dense
    bld.target(1028, 4, disjoint=False)                # 257 entries: 4 per entry, strip-dense at the limit
    bld.target(1027, 4, disjoint=False)                # 257 entries: under 4 per entry
    a, b = bld.finish()
    p = S.Products(a, b)
    assert list(p.u) == [5, 33, 1025, 1028, 1027] and list(p.J) == [1, 3, 5, 257, 257]
    cs = S.census(a, b, fast=True, b_sorted=True, p=p)
    assert list(cs['route']) == [0, 2, 1, 1, 2] and cs['strip_entries'] == 262 and cs['esc_products'] == 33 + 1027
    cs = S.census(a, b, fast=True, b_sorted=False, p=p)            # no strips: the dense rows are large rows
    assert list(cs['route']) == [0, 2, 3, 3, 2] and cs['strips'] == 0 and cs['large'] == {2: 'lds', 3: 'lds'}      # (8 cnt >= 832)
    cs = S.census(a, b, fast=False, b_sorted=True, esc=False, p=p)
    assert list(cs['route']) == [0, 0, 3, 3, 3] and cs['small'] == {0: 16, 1: 32} and (cs['mid_rows'], cs['hash_rows']) == (1, 1)
    assert S.small_classes(p.u, cs['route'], S.LIMITS) == (1, 1, 0)


def test_union_of_censuses_covers_every_accumulator_in_both_forms():
    """
    Every one of the nine accumulators takes a row of some case, FAST and -- but for the strips, which are FAST only -- in
    the general form; both strip forms, both small-row forms and both strip-table builders occur.
    """
    seen = set()
    for name in ALL:
        c = S.build(name)
        cs, form = c.census, 'fast' if c.census['fast'] else 'general'
        for lanes in set(cs['small'].values()):
            seen.add((f'small-{lanes}', form))
        for kind in set(cs['large'].values()):
            seen.add((kind, form))
        if cs['esc_rows']:
            seen.add(('esc', form))
        if cs['strip_rows']:
            seen.add(('strips-one-pass' if cs['strip_fused'] else 'strips-two-pass', form))
            seen.add(('table by row starts' if c.r.nrows <= 2 * cs['strip_entries'] else 'table by bisection', form))
        if cs['small']:
            seen.add(('small-one-pass' if cs['small_fused'] or not any(v < 256 for v in cs['small'].values()) else 'small-two-pass', form))
    both = ('small-16', 'small-32', 'small-256', 'esc', 'lds', 'hash')
    want = {(k, f) for k in both for f in ('fast', 'general')}
    want |= {(k, 'fast') for k in ('hbm', 'strips-one-pass', 'strips-two-pass', 'table by row starts', 'table by bisection',
                                   'small-one-pass', 'small-two-pass')}
    assert want <= seen, sorted(want - seen)


@pytest.mark.parametrize('name', ALL)
def test_numpy_product_against_the_oracle(name):
    from oracle import oracle as O
    c = S.build(name)
    rp, ci, vs, bound = S.ref_product(c.a, c.r, c.p)
    if c.abt:      # the module's transpose is the oracle's
        _, _, trp, tci, tvs = O.transpose(*c.b.tup())
        assert np.array_equal(trp, c.r.rowptrs) and np.array_equal(tci, c.r.colinds) and np.array_equal(tvs, c.r.values)
    _, _, orp, oci, ovs = O.mult_ab(c.a.tup(), c.r.tup())
    assert orp.dtype == np.int32 and np.array_equal(orp, rp)
    rows = np.repeat(np.arange(c.a.nrows), np.diff(orp))
    o = np.lexsort((oci, rows))
    assert np.array_equal(oci[o], ci)
    assert np.all(np.abs(ovs[o] - vs) <= 1e-12 * bound + 1e-300)
    # the census's distinct-output counts are the product's row lengths
    assert np.array_equal(np.diff(orp), c.census['cnt'])
