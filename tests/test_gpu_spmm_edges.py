"""
The dense-panel SpMM (csrc/spmm_dense.hip) on the cases of tests/spmm_cases.py, each under its own CSRK_SPMM_HEAVY /
CSRK_SPMM_HEAVY_GROUPS (the `unforced` family under neither) and with the handle cache off.  Per case and panel width, on a
fresh handle:
  1. two products: the bits repeat;
  2. the nine fields of csrk_spmm_plan_stats equal the module's model of the plan for this device's CU count, field by field,
     R equals the model's formula and the range table (csrk_spmm_plan_ranges) equals the model's -- before any value is
     looked at;
  3. on the exact-product inputs (24-bit integers times powers of two: fused and unfused multiply-adds agree) EVERY value of C
     equals spmm_cases.product -- the sums in the order DESIGN.md section 7 documents -- bit for bit;
  4. on full-mantissa uniform values, where fused and unfused may differ, |C - ref| <= 1e-12 * sum |a||b| + 1e-300 against the
     oracle's spmm_dense.
`widths` and `widths-heavy` also go through csrk_spmm_dense_device (C pre-filled with NaN); `widths` takes one handle through
ascending widths and back (the partial buffer grows on a live handle); `few-tiles` and `split` go through mult_ab(A, CSR(B))
under both column orders; `types` runs with int64 row pointers, float32 values and no values.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import spmm_cases as T

pytestmark = pytest.mark.gpu

ALL = T.names()
_RUNS, _MODELS = {}, {}


@contextlib.contextmanager
def _environ(env):
    old = {k: os.environ.get(k) for k in T.ENV_KEYS + ('CSRK_HANDLE_CACHE',)}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _bits(a):
    return (a + 0.0).view(np.int64)      # (-0.0 compares as 0.0)


def _values(c, variant, exact):
    v = c.values if exact else c.uniform_values()
    return {'f4': v.astype(np.float32), 'none': None}.get(variant, v)


def _matrix(c, variant='f8', exact=True):
    from csr_amd import CSR
    rp = c.rowptrs.astype(np.int64) if variant == 'ptr64' else c.rowptrs
    return CSR(c.nrows, c.ncols, c.nnz, rp, c.colinds, _values(c, variant, exact), _cast=False)


def _plan_of(h):
    "(the nine statistics, the range table) of a live handle"
    from csr_amd._lib import lib, check
    st = (C.c_int64 * 9)()
    check(lib.csrk_spmm_plan_stats(h.H, st, 9))
    st = [int(v) for v in st]
    rt = np.full(st[4] + 1, -1, dtype=np.int32)
    check(lib.csrk_spmm_plan_ranges(h.H, rt.ctypes.data_as(C.c_void_p), len(rt)))
    return st, (rt.tolist() if st[0] else [])


def _device_product(h, B, nrows):
    "csrk_spmm_dense_device into a C filled with NaN"
    import torch
    from csr_amd._lib import lib, check
    dB = torch.from_numpy(B).to('cuda')
    dC = torch.full((nrows, B.shape[1]), float('nan'), dtype=torch.float64, device='cuda')
    check(lib.csrk_spmm_dense_device(h.H, dB.data_ptr(), B.shape[1], B.shape[1], dC.data_ptr(), B.shape[1], None))
    torch.cuda.synchronize()
    return dC.cpu().numpy()


def _run(name, k, variant='f8', exact=True, entry='host'):
    "two products of (case, width) on a fresh handle, the plan's statistics and its range table (memoised)"
    key = (name, k, variant, exact, entry)
    if key not in _RUNS:
        from csr_amd.kernels import hip as K
        c = T.build(name)
        B = c.panel(k, exact)
        with _environ(dict(c.env(), CSRK_HANDLE_CACHE='0')):
            h = K.to_handle(_matrix(c, variant, exact))
            try:
                out = [K.mult_dense(h, B) if entry == 'host' else _device_product(h, B, c.nrows) for _ in range(2)]
                stats, ranges = _plan_of(h)
            finally:
                K.release_handle(h)
        _RUNS[key] = dict(C=out, stats=stats, ranges=ranges)
    return _RUNS[key]


def _model(name, k, variant='f8'):
    "spmm_cases.product of the exact inputs under the plan this device builds at width k"
    key = (name, k, 'f8' if variant in ('ptr64', 'f4') else variant)      # (the exact values are float32 numbers)
    if key not in _MODELS:
        c = T.build(name)
        m = T.product(c.plan(_cus(), k), _values(c, key[2], True), c.panel(k))
        m.flags.writeable = False
        _MODELS[key] = m
    return _MODELS[key]


def _check_plan(name, k, r, what):
    p = T.build(name).plan(_cus(), k)
    want = p.stats()
    got = r['stats']
    assert got == want, (what, {f: (got[i], want[i]) for i, f in enumerate(T.STAT_KEYS) if got[i] != want[i]})
    if p.on:
        n_tiles = T.cdiv(p.ncols, T.TILE)
        R = min(max(_cus(), got[3]) // got[3], n_tiles)
        assert got[4] == (R // 8 * 8 if R >= 8 else R), (what, 'R', got[4], R)
        assert r['ranges'] == p.range.tolist(), (what, 'range table', r['ranges'], p.range.tolist())
    else:
        assert r['ranges'] == [], what


def _check_bits(name, k, variant, Cm, what):
    want = _model(name, k, variant)
    assert Cm.dtype == np.float64 and Cm.shape == want.shape and not np.isnan(Cm).any(), what
    bad = np.argwhere(_bits(Cm) != _bits(want))
    assert bad.size == 0, (what, 'not the sums in the documented order', len(bad), bad[:6].tolist(),
                           [(float(Cm[i, j]), float(want[i, j])) for i, j in bad[:6]])


def _check_exact(name, k, variant='f8', entry='host'):
    what = (name, k, variant, entry)
    r = _run(name, k, variant, True, entry)
    assert np.array_equal(r['C'][0].view(np.int64), r['C'][1].view(np.int64)), (what, 'the second product differs')
    _check_plan(name, k, r, what)
    _check_bits(name, k, variant, r['C'][0], what)
    return r


def _check_uniform(name, k, entry='host'):
    from oracle import oracle as O
    c = T.build(name)
    what = (name, k, 'uniform', entry)
    r = _run(name, k, 'f8', False, entry)
    assert np.array_equal(r['C'][0].view(np.int64), r['C'][1].view(np.int64)), (what, 'the second product differs')
    _check_plan(name, k, r, what)
    v, B = c.uniform_values(), c.panel(k, False)
    ref = O.spmm_dense(c.nrows, c.rowptrs, c.colinds, v, B)
    bound = O.spmm_dense(c.nrows, c.rowptrs, c.colinds, np.abs(v), np.abs(B))
    err = np.abs(r['C'][0] - ref)
    print(f'{what}: max |C - ref| / bar = {float(np.max(err / (1e-12 * bound + 1e-300))) if err.size else 0.0:.3e}')
    bad = np.argwhere(~(err <= 1e-12 * bound + 1e-300))
    assert bad.size == 0, (what, bad[:6].tolist())


@pytest.mark.parametrize('name', ALL)
def test_plan_is_the_models(name):
    "a case whose plan differs from the model fails here, before any value is compared"
    c = T.build(name)
    assert not c.failed_claims(), c.failed_claims()
    k = c.ks[0]
    _check_plan(name, k, _run(name, k), (name, k))


@pytest.mark.parametrize('name', ALL)
def test_sums_in_the_documented_order(name):
    "census, then every value bit for bit, at every width of the case"
    for k in T.build(name).ks:
        _check_exact(name, k)


@pytest.mark.parametrize('name', ALL)
def test_full_mantissa_values_meet_the_bar(name):
    for k in T.build(name).ks:
        _check_uniform(name, k)


@pytest.mark.parametrize('name', ['widths', 'widths-heavy'])
def test_widths_through_the_device_entry(name):
    for k in T.build(name).ks:
        r = _check_exact(name, k, entry='device')
        assert np.array_equal(r['C'][0].view(np.int64), _run(name, k)['C'][0].view(np.int64)), (name, k)
    _check_uniform(name, T.build(name).ks[-1], entry='device')


def test_one_handle_through_growing_widths():
    """
    the partial buffer of the split rows grows with k on a live handle (grow_p, part_k) and is kept when k shrinks again:
    every product has the bits a fresh handle gives
    """
    from csr_amd.kernels import hip as K
    c = T.build('widths')
    assert c.plan().n_multi > 0
    seq = list(c.ks) + [3, 129, 1, 64]
    with _environ(dict(c.env(), CSRK_HANDLE_CACHE='0')):
        h = K.to_handle(_matrix(c))
        try:
            got = [(k, K.mult_dense(h, c.panel(k))) for k in seq]
            got += [(k, _device_product(h, c.panel(k), c.nrows)) for k in (132, 5)]
        finally:
            K.release_handle(h)
    for k, Cm in got:
        _check_bits('widths', k, 'f8', Cm, ('widths', 'one handle', k))
        assert np.array_equal(Cm.view(np.int64), _run('widths', k)['C'][0].view(np.int64)), k


@pytest.mark.parametrize('variant', ['ptr64', 'f4', 'none'])
def test_types(variant):
    "int64 row pointers, float32 values, no values: the same plan; the same bits where the numbers are the same"
    k = T.build('types').ks[0]
    r = _check_exact('types', k, variant)
    same = np.array_equal(r['C'][0].view(np.int64), _check_exact('types', k)['C'][0].view(np.int64))
    assert same == (variant != 'none'), variant


def _panel_csr(B):
    from csr_amd import CSR
    n, k = B.shape
    return CSR(n, k, n * k, np.arange(n + 1, dtype=np.int32) * k, np.tile(np.arange(k, dtype=np.int32), n), B.reshape(-1).copy(), _cast=False)


@pytest.mark.parametrize('order', ['reference', 'ascending'])
@pytest.mark.parametrize('name', T.names('few-tiles', 'split'))
def test_through_mult_ab(name, order):
    """
    mult_ab(A, CSR(B)) with B fully populated takes the same kernels through SpmmOut: the rows of A that hold entries, k
    values each, at the reversed (the reference's order) or the ascending positions -- the same bits as the panel product
    """
    from csr_amd.kernels import hip as K
    c = T.build(name)
    k = c.ks[-1]
    with _environ(dict(c.env(), CSRK_HANDLE_CACHE='0')):
        K.set_spgemm_order(order)
        ah, bh = K.to_handle(_matrix(c)), K.to_handle(_panel_csr(c.panel(k)))
        try:
            ch = K.mult_ab(ah, bh)
            route = K.spgemm_last_route()
            stats, ranges = _plan_of(ah)
            Cm = K.from_handle(ch)
            K.release_handle(ch)
        finally:
            K.release_handle(ah)
            K.release_handle(bh)
            K.set_spgemm_order(None)
    assert route == 'dense-panel', (name, route)
    _check_plan(name, k, dict(stats=stats, ranges=ranges), (name, order, 'mult_ab'))
    live = np.flatnonzero(c.lens > 0)
    assert np.array_equal(np.diff(Cm.rowptrs), np.where(c.lens > 0, k, 0)) and Cm.nnz == len(live) * k
    cols = np.arange(k - 1, -1, -1) if order == 'reference' else np.arange(k)
    assert np.array_equal(Cm.colinds.reshape(len(live), k), np.tile(cols, (len(live), 1)))
    dense = np.empty((len(live), k))
    dense[:, cols] = Cm.values.reshape(len(live), k)
    want = _model(name, k)[live]
    bad = np.argwhere(_bits(dense) != _bits(want))
    assert bad.size == 0, (name, order, len(bad), bad[:6].tolist())


def test_union_of_plans():
    "what the runs above reported, taken together: every edge of the plan the cases are named for was built on this device"
    st = {n: _run(n, T.build(n).ks[0])['stats'] for n in ALL}
    if _cus() >= 16:
        assert [st[n][4] for n in T.names('few-tiles')] == [1, 1, 2, 2, 3, 7, 8, 8, 8]
    assert [st[f'places:{n}'][2] for n in (1, 15, 16, 17, 511, 512)] == [1, 15, 16, 17, 511, 512]
    assert st['places:513-g2'][2:4] == [513, 2] and st['places:1025-g4'][2:4] == [1025, 3]
    assert st['places:ties-fit'][1:3] == [300, 512] and st['places:ties-move'][1:3] == [301, 505]
    assert st['places:ties-off'][:7] == [0] * 7 and st['places:shrink'][1:4] == [301, 400, 1]
    assert st['all-heavy'][7] == 0 and all(st[n][0] == 0 for n in T.names(*T.LIGHT_FAMILIES))
    assert [st[n][0] for n in T.names('unforced')] == [0, 1, 0, 1, 1, 0]
    assert {st[n][7] % 16 for n in T.names('seg-lengths')} == set(range(1, 16))
    for n in T.names('ranges'):
        w = np.diff(_run(n, 64)['ranges'])
        assert st[n][6] == 300 and st[n][4] < 300 and w.min() >= 1 and w.max() > 1, n
