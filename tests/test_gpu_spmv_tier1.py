"""
The SpMV pair-form tier (tier 1: build_panel and its plan kernels, spmv_panel_kernel, the tier's reduce in
spmv_epilogue_kernel) on the cases of tests/tier1_cases.py, each under its own CSRK_HEAVY_MIN / CSRK_TIERB_MIN with the split
forced, the merge algorithm, the light stream on and no pack unless a test says otherwise.  Per case and variant, on each of
three products into a y filled with NaN:
  1. csrk_spmv_plan_stats equals the module's model of the layout field by field (cut rows, tier sizes, pairs, entries and the
     tier's blocks, tiles, carry rows, listed carries, groups and padding groups) -- before any value is looked at;
  2. EVERY row -- light and tier-0 rows too: a tier-1 bug that writes outside its rows must show -- meets the bar of
     tests/test_gpu_spmv.py, |y - ref| <= 1e-12 * sum |a_ij x_j| + 1e-300, against the oracle's mult_vec, and nothing is NaN.
     (float32 values times a float32 x: the reference's products are float32, and so are the oracle's and the kernels'.)
  3. every tier-1 row the model places whole inside one pair of one tile (Layout.exact_rows) equals tier1_cases.pair_sum of its
     products BIT FOR BIT: the sequential loop's order below 64 entries, the wavefront's order (lane-strided sums, then the
     shuffle tree) from 64 on -- the order spmv_panel_kernel has, written down in tier1_cases.py; every other addend of the
     row's reduce is a zero;
  4. the second and third product equal the first bit for bit, and so does a fresh handle's.
Variants: float64, float32 and no values; int32 and int64 row pointers; a float32 x on the float64 and float32 values.  The
block-edge, tile-edge and rider cases also run with the light stream off (CSRK_SPMV_STREAM=0) and with the pack forced
(CSRK_SPMV_HOT=1: cold staging, under which the pair kernel gathers a float32 x itself), where the tiers' rows must keep
their bits; the block-edge and tile-edge cases run with inf and NaN in x.
"""
import contextlib
import os

import numpy as np
import pytest

import tier1_cases as T

pytestmark = pytest.mark.gpu

ALL = T.names()
EDGE = T.names(*T.EDGE_FAMILIES)
VARIANTS = ('f8', 'f4', 'none', 'ptr64', 'f32x', 'f4f32x')
_RUNS, _REFS, _EXACT = {}, {}, {}


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


def _typed(c, variant, x=None):
    "(row pointers, values, x) of a variant: the case's own arrays retyped"
    x = c.x if x is None else x
    rp = c.rowptrs.astype(np.int64) if variant == 'ptr64' else c.rowptrs
    vals = {'f4': c.values.astype(np.float32), 'f4f32x': c.values.astype(np.float32), 'none': None}.get(variant, c.values)
    return rp, vals, (x.astype(np.float32) if variant in ('f32x', 'f4f32x') else x)


def _ref(c, variant, x=None, tag=None):
    "(oracle's product, sum |a_ij x_j| per row): computed once per case, variant and x"
    key = (c.name, 'f8' if variant == 'ptr64' else variant, tag)
    if key not in _REFS:
        from oracle import oracle as O
        rp, vals, xx = _typed(c, key[1], x)
        with np.errstate(all='ignore'):
            ref = O.mult_vec(c.nrows, c.ncols, rp, c.colinds, vals, xx)
            bound = O.mult_vec(c.nrows, c.ncols, rp, c.colinds, None if vals is None else np.abs(vals), np.abs(xx))
        ref.flags.writeable = bound.flags.writeable = False
        _REFS[key] = (ref, bound)
    return _REFS[key]


def _exact(c, variant):
    "(rows, pair_sum of each row's products) for the bit-for-bit check"
    key = (c.name, 'f8' if variant == 'ptr64' else variant)
    if key not in _EXACT:
        rp, vals, x = _typed(c, key[1])
        rows, _ = c.layout.exact_rows()
        out = np.zeros(len(rows))
        for k, r in enumerate(rows):
            s, e = int(rp[r]), int(rp[r + 1])
            xs = x[c.colinds[s:e]]
            if vals is None:
                p = xs.astype(np.float64)
            elif vals.dtype == np.float32 and x.dtype == np.float32:
                p = (vals[s:e] * xs).astype(np.float64)                    # one float32 rounding, as the reference's loop has
            else:
                p = vals[s:e].astype(np.float64) * xs.astype(np.float64)
            out[k] = T.pair_sum(p)
        _EXACT[key] = (rows, out)
    return _EXACT[key]


def _run(name, variant='f8', stream=True, hot=False, x=None, tag=None):
    "three products of (case, variant) on a fresh handle, each into a NaN-filled y, and the plan's statistics (memoised)"
    key = (name, variant, stream, hot, tag)
    if key in _RUNS:
        return _RUNS[key]
    import torch
    from csr_amd import CSR
    from csr_amd._lib import lib, check
    from csr_amd.kernels import hip as K
    c = T.build(name)
    rp, vals, xx = _typed(c, variant, x)
    dev = torch.device('cuda', 0)
    with _environ(dict(c.env(stream, hot), CSRK_HANDLE_CACHE='0')):
        h = K.to_handle(CSR(c.nrows, c.ncols, c.nnz, rp, c.colinds, vals, _cast=False))
        try:
            K.set_spmv_algo(h, 'merge')
            dx = torch.tensor(xx).to(dev)
            dy = torch.empty(c.nrows, dtype=torch.float64, device=dev)
            out = []
            for _ in range(3):
                dy.fill_(float('nan'))
                if xx.dtype == np.float32:
                    check(lib.csrk_spmv_f32x_device(h.H, dx.data_ptr(), dy.data_ptr(), None))
                else:
                    check(lib.csrk_spmv_device(h.H, dx.data_ptr(), dy.data_ptr(), None))
                torch.cuda.synchronize()
                out.append(dy.cpu().numpy())
            stats = K.spmv_plan_stats(h)
        finally:
            K.release_handle(h)
    _RUNS[key] = dict(y=out, stats=stats)
    return _RUNS[key]


def _bits(a):
    return (a + 0.0).view(np.int64)      # (-0.0 compares as 0.0)


def _check_plan(c, r, what):
    want = c.layout.stats()
    got = {k: r['stats'][k] for k in want}
    assert got == want, (what, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
    assert r['stats']['split_mode'] == (2 if want['cut_rows'] else 0), what


def _check_product(c, variant, y, what):
    "checks 2 and 3 of the module docstring on one product"
    ref, bound = _ref(c, variant)
    assert y.dtype == np.float64 and y.shape == ref.shape and not np.isnan(y).any(), (what, np.flatnonzero(np.isnan(y))[:8])
    err = np.abs(y - ref)
    worst = float(np.max(err / (1e-12 * bound + 1e-300))) if len(y) else 0.0
    print(f'{what}: max |y - ref| / bar = {worst:.3e}')
    bad = np.flatnonzero(~(err <= 1e-12 * bound + 1e-300))
    assert bad.size == 0, (what, bad[:8], y[bad[:8]], ref[bad[:8]])
    rows, want = _exact(c, variant)
    diff = rows[_bits(y[rows]) != _bits(want)]
    assert diff.size == 0, (what, 'rows held by one pair of one tile differ from the order the kernel is said to have', diff[:8],
                            y[diff[:8]], want[np.isin(rows, diff[:8])])


def _check_run(name, variant='f8', **kw):
    c = T.build(name)
    r = _run(name, variant, **kw)
    what = (name, variant) + tuple(f'{k}={v}' for k, v in kw.items())
    _check_plan(c, r, what)
    for i, y in enumerate(r['y']):
        _check_product(c, variant, y, what + (f'product {i}',))
        assert np.array_equal(y.view(np.int64), r['y'][0].view(np.int64)), (what, 'repeat', i)
    return c, r


@pytest.mark.parametrize('name', ALL)
def test_plan_is_the_models(name):
    "a case whose plan differs from the model fails here, before any value is compared"
    c = T.build(name)
    assert not c.failed_claims(), c.failed_claims()
    _check_plan(c, _run(name), (name, 'f8'))


@pytest.mark.parametrize('name', ALL)
def test_case_in_every_type(name):
    c = T.build(name)
    base = _check_run(name)[1]['y'][0]
    for variant in VARIANTS[1:]:
        y = _check_run(name, variant)[1]['y'][0]
        if variant == 'ptr64':                      # the same numbers through other pointers: the same plan, the same bits
            assert np.array_equal(y.view(np.int64), base.view(np.int64)), name
    fresh = _check_run(name, tag='fresh')[1]['y'][0]
    assert np.array_equal(fresh.view(np.int64), base.view(np.int64)), (name, 'a fresh handle')
    if c.layout.n:                                  # float32 products are not the float64 ones: the variant is a check of its own
        assert np.max(np.abs(_ref(c, 'f4f32x')[0] - _ref(c, 'f4')[0])) > 1e-10


@pytest.mark.parametrize('name', EDGE)
def test_stream_off_and_pack_on(name):
    """
    CSRK_SPMV_STREAM=0 (the merge-path tile kernel beside the tiers) and CSRK_SPMV_HOT=1 (the pack and cold staging; a float32
    x then reaches the pair kernel's gathers as float32): the same plan for the tiers, the same bar for every row, and the
    tiers' rows -- which read x themselves in every form -- keep the bits of the default run.
    """
    c = T.build(name)
    cut = c.layout.cut
    for variant in ('f8', 'f4'):
        y = _check_run(name, variant, stream=False)[1]['y'][0]
        assert np.array_equal(y[cut].view(np.int64), _run(name, variant)['y'][0][cut].view(np.int64)), (name, variant, 'stream off')
    for variant in ('f8', 'f32x', 'f4f32x'):
        y = _check_run(name, variant, hot=True)[1]['y'][0]
        assert np.array_equal(y[cut].view(np.int64), _run(name, variant)['y'][0][cut].view(np.int64)), (name, variant, 'pack on')


def _poisoned(c, tier1_too):
    """
    x with inf and NaN at columns no tier-1 row holds: every block's first and last column where free, columns only light (or
    tier-0) rows hold, a few more.  tier1_too: also inf at the largest column of the panel's last tile -- the pair the lanes
    past the tile's end re-read -- and NaN at the largest column of its first tile.
    """
    a = c.layout
    held = np.zeros(c.ncols, dtype=bool)
    held[a.ecol] = True
    lens = np.diff(c.rowptrs.astype(np.int64))
    other = np.ones(c.nrows, dtype=bool)
    other[a.t1] = False
    other_cols = np.unique(c.colinds[np.repeat(other, lens)])
    edge = [b * T.BLOCK for b in range(a.nb)] + [min((b + 1) * T.BLOCK, c.ncols) - 1 for b in range(a.nb)]
    rng = np.random.default_rng(11)
    cand = np.concatenate([edge, other_cols[~held[other_cols]][::3], rng.integers(0, c.ncols, size=40)]).astype(np.int64)
    cand = np.unique(cand[~held[cand]])
    x = c.x.copy()
    x[cand[0::3]] = np.inf
    x[cand[1::3]] = -np.inf
    x[cand[2::3]] = np.nan
    assert len(cand) >= 6 and np.any(np.isin(cand, other_cols))
    if tier1_too:
        last = a.mcol[a.t_j0[-1]:a.t_j0[-1] + a.t_nn[-1]]
        x[int(last.max()) if len(last) else int(a.mcol[-1])] = np.inf
        x[int(a.mcol[:a.t_nn[0]].max())] = np.nan
    return x


@pytest.mark.parametrize('name', T.names('blocks', 'tiles'))
def test_nonfinite_x(name):
    """
    inf and NaN in x where no tier-1 row has an entry: every tier-1 row stays finite and within the bar (the pair loads clamp
    to the tile's own entries and the products are masked after the multiply), every other row is what the oracle gives --
    finite and within the bar, or the same inf / NaN.  Then inf and NaN at columns tier-1 rows do hold: those rows give the
    oracle's non-finite result and the other tier-1 rows stay finite.
    """
    c = T.build(name)
    for tier1_too in (False, True):
        tag = 'poison-t1' if tier1_too else 'poison'
        x = _poisoned(c, tier1_too)
        r = _run(name, x=x, tag=tag)
        _check_plan(c, r, (name, tag))
        ref, bound = _ref(c, 'f8', x, tag)
        fin = np.isfinite(ref)
        assert (not np.all(fin)) and (tier1_too or np.all(fin[c.layout.t1])), (name, tag)
        if tier1_too:
            assert 1 <= np.sum(~fin[c.layout.t1]) < c.layout.n or c.layout.n == 1, (name, tag)
        for i, y in enumerate(r['y']):
            assert np.array_equal(np.isnan(y), np.isnan(ref)), (name, tag, i, np.flatnonzero(np.isnan(y) != np.isnan(ref))[:8])
            inf = np.isinf(ref)
            assert np.array_equal(y[inf], ref[inf]) and np.array_equal(np.isinf(y), inf), (name, tag, i)
            err = np.abs(y[fin] - ref[fin])
            assert np.all(err <= 1e-12 * bound[fin] + 1e-300), (name, tag, i, np.flatnonzero(fin)[~(err <= 1e-12 * bound[fin] + 1e-300)][:8])
            assert np.array_equal(y.view(np.int64), r['y'][0].view(np.int64)), (name, tag, 'repeat', i)


def test_union_of_plans():
    "what the runs above reported, taken together: every edge of the plan the issue lists was built on this device"
    st = {n: _run(n)['stats'] for n in ALL}
    assert {st[n]['t1_pad_groups'] for n in T.names('groups')} == {0, 13, 14}
    assert sorted(st[n]['t1_listed_carries'] for n in T.names('carry', 'listed')) == [0, 1, 1, 2, 64, 65, 65, 66]
    assert all(st[n]['t1_carry_rows'] == 4 for n in T.names('carry', 'listed'))
    assert st['fallback']['t1_rows'] == 0 and st['fallback']['cut_rows'] == 0
    assert max(s['t1_rows'] for s in st.values()) == 2100 and max(s['t1_blocks'] for s in st.values()) == 17
    assert {st[n]['t0_rows'] for n in T.names('rider')} == {0, 1, 64, 65, 130}
