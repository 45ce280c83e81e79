"""
The long-row class of csrk_als_rows_cg on the card (include/csrk.h, rule C11): a row of at least L entries is solved by a
whole workgroup, and no output bit may depend on that.  With L = 1 every row with an entry takes the class and is held to
the exact restatement of rules C2 - C7 (tests/als_cg_ref.py) at every edge of the chunked LDS image; at every k and several
L the results equal those with the class off (the one-team kernel, itself held to the exact chain by test_gpu_als_cg.py),
for every variant of a request; the census counts the rows the class took; the row scan is tried at its slice edges; NaN,
Inf, the stop rule and the empty cases go through the workgroup-uniform loop.

Shapes come from csrk_als_cg_long_limits.  The exact reference makes about 10^5 fused steps per second, an entry costs
about 2 k of them per product: the exact cases are sized so that the whole file's reference work stays under a minute.
"""
import ctypes as C
import math

import numpy as np
import pytest

import als_cg_ref as R
import test_gpu_als_cg as G

pytestmark = pytest.mark.gpu

RHS = G.RHS
_same, _same3, _csr, _pattern, _panel, _sym_base = G._same, G._same3, G._csr, G._pattern, G._panel, G._sym_base


@pytest.fixture(scope='module')
def limits():
    from csr_amd.kernels import hip as K
    return K.als_cg_limits()


@pytest.fixture(scope='module')
def llim():
    from csr_amd.kernels import hip as K
    return K.als_cg_long_limits()


def _chunk(llim, k, pdt):
    "C for the panel type and k"
    return int(llim[3 + 2 * (pdt == np.float32) + (k > 64)])


class _long:
    "the process-wide switch set for a block, and put back to following the environment"

    def __init__(self, L):
        self.L = L

    def __enter__(self):
        from csr_amd.kernels import hip as K
        K.als_cg_set_long(self.L)

    def __exit__(self, *a):
        from csr_amd.kernels import hip as K
        K.als_cg_set_long(None)


def _run(h, L, V, scale, rhs, base, lam, lam_n, rows, steps, x0, tol=0.0):
    "the host form under L: ((x, resid, taken), census)"
    from csr_amd.kernels import hip as K
    with _long(L):
        got = K.als_rows_cg(h, V, scale, rhs, base, lam, lam_n, rows, steps, x0, tol)
        return got, K.als_cg_last_stats()


def _check_census(st, L, lens, S):
    "test 3: what the host form reports against NumPy's counts from the row lengths"
    lens = np.asarray(lens)
    n = len(lens)
    issued = int(L > 0 and n > 0 and lens.sum() > 0)
    assert st[0] == int(n > 0) and st[1] == L and st[2] == issued, (st, L)
    assert st[3] == (math.ceil(n / S) if issued else 0), (st, L)
    long_rows = lens >= L if L > 0 else np.zeros(n, bool)
    assert st[4] == int(long_rows.sum()) and st[5] == int(lens[long_rows].sum()), (st, L)


# ---- 1. every row long: the exact chain -------------------------------------------------------------------------

def _exact_calls(k, Cn):
    "(scale, rhs, with a base, with an x0, row lengths) per call: three chunks with and without x0, every rhs mode once"
    every = [0, 1, 2, Cn - 1, Cn, Cn + 1, 2 * Cn, 2 * Cn + 1, 3 * Cn + 5]
    few = every if k <= 33 else [0, 1, 2, Cn + 1]           # (the reference's cost: two chunks where k is large)
    calls = [(True, RHS[k % 3], False, False, every),
             (False, RHS[(k + 1) % 3], k <= 33, True, few),
             (k % 2 == 0, RHS[(k + 2) % 3], False, True, [1, Cn])]
    if k == 64:
        calls.append((True, 'values', True, True, [0, Cn + 1]))          # the dense base once at k = 64
    return calls


@pytest.mark.parametrize('k', [1, 17, 33, 64, 65, 128])
@pytest.mark.parametrize('pdt', [np.float64, np.float32])
def test_long_rows_are_the_exact_chain(k, pdt, llim):
    from csr_amd.kernels import hip as K
    steps = 2 if k <= 64 else 1
    Cn = _chunk(llim, k, pdt)
    V = _panel(k, pdt, k)
    base = _sym_base(k, k)
    vdt = np.float64 if pdt == np.float64 else np.float32
    for n, (scale, rhs, with_base, with_x0, lens) in enumerate(_exact_calls(k, Cn)):
        nr, nc, rp, ci, vs = _pattern(lens, seed=200 * k + n, vdt=vdt)
        x0 = np.random.default_rng(n).standard_normal((nr, k)) if with_x0 else None
        b = base if with_base else None
        want = R.cg_exact(rp, ci, vs, V, scale, rhs, b, 0.125, 0.0625, steps, 0.0, x0)
        h = K.to_handle(_csr(nr, nc, rp, ci, vs))
        try:
            got, st = _run(h, 1, V, scale, rhs, b, 0.125, 0.0625, None, steps, x0)
        finally:
            K.release_handle(h)
        _check_census(st, 1, lens, int(llim[2]))
        assert st[4] == sum(1 for x in lens if x)            # every row with an entry took the class
        assert _same(got[0], want[0]), (scale, rhs, with_base, with_x0)
        assert _same(got[1], want[1]) and np.array_equal(got[2], want[2]), (scale, rhs, with_base, with_x0)


# ---- 2 and 3. no bit depends on the class; the census -----------------------------------------------------------

def _mixed_long_lens(limits, Cn):
    "_mixed_lens' 300 rows (the longest 700 entries) plus a row of 7 C + 3 and one of 5000"
    return np.concatenate([G._mixed_lens(limits), [7 * Cn + 3, 5000]]).astype(np.int64)


def _Ls(Cn):
    return (1, Cn, 701, 5000, 5001)


@pytest.mark.parametrize('k', G.KS)
@pytest.mark.parametrize('pdt', [np.float64, np.float32])
def test_no_bit_depends_on_the_class(k, pdt, limits, llim):
    from csr_amd.kernels import hip as K
    Cn, S = _chunk(llim, k, pdt), int(llim[2])
    lens = _mixed_long_lens(limits, Cn)
    nr, nc, rp, ci, vs = _pattern(lens, seed=k)
    assert (lens == 700).sum() == 1 and (lens == 5000).sum() == 1          # 701 and 5001 sit one above a row's length
    V = _panel(k, pdt, k)
    base = _sym_base(k, k)
    x0 = np.random.default_rng(k).standard_normal((nr, k)) * 0.1
    h = K.to_handle(_csr(nr, nc, rp, ci, vs))
    try:
        for scale, rhs, b, xx in ((False, 'values', None, None), (True, 'one_plus_values', base, x0), (True, 'ones', None, x0)):
            off, st = _run(h, 0, V, scale, rhs, b, 0.125, 0.0625, None, 3, xx)
            _check_census(st, 0, lens, S)
            assert np.isfinite(off[0]).all() and off[2].max() == 3
            for L in _Ls(Cn):
                on, st = _run(h, L, V, scale, rhs, b, 0.125, 0.0625, None, 3, xx)
                assert _same3(on, off), (L, rhs)
                _check_census(st, L, lens, S)
            # a row of L - 1 entries is not counted and one of L is: at L = 701 the 700-entry row stays with its team
            assert _run(h, 700, V, scale, rhs, b, 0.125, 0.0625, None, 3, xx)[1][4] == _run(h, 701, V, scale, rhs, b, 0.125, 0.0625, None,
                                                                                            3, xx)[1][4] + 1
    finally:
        K.release_handle(h)


@pytest.mark.parametrize('k', [3, 17, 33, 64, 90])
@pytest.mark.parametrize('pdt', [np.float64, np.float32])
def test_variants_give_the_same_bits_at_every_L(k, pdt, limits, llim):
    """
    test_variants_give_the_same_bits' variants, each under every L, against the class off: int64 row pointers, float32 and
    absent values, V misaligned (element loads), ldv / ldo / ldx0 above k, x0 == out in place, a side stream, a row
    sub-range that starts and ends on a long row, NULL resid and taken; and the device form's census.
    """
    import torch
    from csr_amd.kernels import hip as K
    from csr_amd._lib import VAL_F32, VAL_F64
    Cn, S = _chunk(llim, k, pdt), int(llim[2])
    lens = _mixed_long_lens(limits, Cn)
    nr, nc, rp, ci, vs = _pattern(lens, seed=k)
    V = _panel(k, pdt, k)
    base = _sym_base(k, k)
    lam, lam_n, steps = 0.125, 0.0625, 3
    code = VAL_F64 if pdt == np.float64 else VAL_F32
    x0 = np.random.default_rng(k).standard_normal((nr, k)) * 0.1
    # the sub-range: from the 700-entry row (long at L <= 700) to the 5000-entry row, the last
    first_long = int(np.flatnonzero(lens == 700)[0])
    sub = (first_long, nr)
    assert lens[sub[0]] == 700 and lens[sub[1] - 1] == 5000
    h32, h64, hf32 = K.to_handle(_csr(nr, nc, rp, ci, vs)), K.to_handle(_csr(nr, nc, rp, ci, vs, ptr64=True)), \
        K.to_handle(_csr(nr, nc, rp, ci, vs.astype(np.float32)))
    hnone, hones = K.to_handle(_csr(nr, nc, rp, ci, None)), K.to_handle(_csr(nr, nc, rp, ci, np.ones(len(ci))))
    try:
        for scale, rhs, b, xx in ((True, 'one_plus_values', base, x0), (False, 'values', None, None)):
            rcode = RHS.index(rhs)
            off = _run(h32, 0, V, scale, rhs, b, lam, lam_n, None, steps, xx)[0]
            ones_off = _run(hones, 0, V, scale, rhs, b, lam, lam_n, None, steps, xx)[0]
            dbase = None if b is None else torch.from_numpy(b).cuda()
            for L in _Ls(Cn):
                for hh in (h64, hf32):
                    assert _same3(_run(hh, L, V, scale, rhs, b, lam, lam_n, None, steps, xx)[0], off), L
                assert _same3(_run(hnone, L, V, scale, rhs, b, lam, lam_n, None, steps, xx)[0], ones_off), L
                part, st = _run(h32, L, V, scale, rhs, b, lam, lam_n, sub, steps, None if xx is None else xx[sub[0]:sub[1]])
                assert _same3(part, tuple(a[sub[0]:sub[1]] for a in off)), L
                _check_census(st, L, lens[sub[0]:sub[1]], S)
                with _long(L):
                    for n, (voff, ld) in enumerate(((0, k), (1, k + 3))):
                        dV = torch.zeros(nc, ld + voff, dtype=torch.from_numpy(V).dtype, device='cuda')
                        dV[:, voff:voff + k] = torch.from_numpy(V).cuda()
                        pv = dV[:, voff:].data_ptr()
                        assert (pv % 16 != 0) == (voff != 0)
                        st_ = torch.cuda.Stream() if n == 0 else None
                        pad = (0, 5)[n]
                        dx0, ldx0 = None, 0
                        if xx is not None:
                            dx0 = torch.full((nr, k + 1 + n), 9.0, dtype=torch.float64, device='cuda')
                            dx0[:, :k] = torch.from_numpy(xx).cuda()
                            ldx0 = k + 1 + n
                        got = G._device_call(h32 if n else h64, pv, dV.stride(0), k, code, scale, rcode, 0, nr, dbase, lam, lam_n, steps,
                                             0.0, dx0, ldx0, st_, pad)
                        dst = K.als_cg_last_stats()
                        assert _same3((got[0][:, :k],) + got[1:], off) and np.all(got[0][:, k:] == -7.0), (L, voff)
                        assert dst[:4] == (1, L, 1, math.ceil(nr / S)) and dst[4] == dst[5] == -1        # the device form never reads back
                        sub0 = None if dx0 is None else dx0[sub[0]:]
                        got = G._device_call(h32, pv, dV.stride(0), k, code, scale, rcode, sub[0], sub[1], dbase, lam, lam_n, steps, 0.0,
                                             sub0, ldx0, st_, pad, info=False)
                        assert _same(got[0][:, :k], off[0][sub[0]:sub[1]]) and np.all(got[0][:, k:] == -7.0), (L, voff)
                        assert np.all(got[1] == -7.0) and np.all(got[2] == -7)
                        if dx0 is not None:
                            got = G._device_call(h32, pv, dV.stride(0), k, code, scale, rcode, 0, nr, dbase, lam, lam_n, steps, 0.0, dx0,
                                                 ldx0, st_, inplace=True)
                            assert _same3((got[0][:, :k],) + got[1:], off) and np.all(got[0][:, k:] == 9.0), (L, voff)
    finally:
        for h in (h32, h64, hf32, hnone, hones):
            K.release_handle(h)


# ---- 4. the scan's slices ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('pdt', [np.float64, np.float32])
def test_scan_slices(pdt, llim):
    from csr_amd.kernels import hip as K
    k = 5
    S, Cn = int(llim[2]), _chunk(llim, k, pdt)
    lens = np.zeros(2 * S + 3, np.int64)
    at = [0, S - 1, S, S + 1, 2 * S + 2, S + S // 2, S + S // 2 + 1]      # slice edges, and two adjacent rows mid-slice
    lens[at] = Cn + 1
    nr, nc, rp, ci, vs = _pattern(lens, seed=41)
    V = _panel(k, pdt, 41)
    x0 = np.random.default_rng(41).standard_normal((nr, k))
    h = K.to_handle(_csr(nr, nc, rp, ci, vs))
    try:
        for rows in (None, (S - 1, 2 * S + 3)):
            rb, re_ = rows or (0, nr)
            xx = x0[rb:re_]
            off = _run(h, 0, V, True, 'values', None, 0.25, 0.0, rows, 3, xx)[0]
            on, st = _run(h, 2, V, True, 'values', None, 0.25, 0.0, rows, 3, xx)
            assert _same3(on, off), rows
            _check_census(st, 2, lens[rb:re_], S)
            assert st[4] == (7 if rows is None else 6) and st[3] == math.ceil((re_ - rb) / S)
            # the empty rows are the teams': from x0 they solve rho x = 0 by the same rule
            assert np.isfinite(on[0]).all()
    finally:
        K.release_handle(h)


# ---- 5. special values, stops and the empty cases ---------------------------------------------------------------

@pytest.mark.parametrize('pdt', [np.float64, np.float32])
def test_nan_and_inf_reach_only_the_long_rows_that_hold_them(pdt, llim):
    from csr_amd.kernels import hip as K
    k = 3
    Cn = _chunk(llim, k, pdt)
    lens = [0, 4, Cn + 2, 9, 1, 2 * Cn + 1, 3, 0, 6]
    nr, nc, rp, ci, vs = _pattern(lens, seed=9)
    # one column that only rows 2 and 3 hold
    col = G.NCOLS - 1
    ci[ci == col] = 0
    ci[rp[2] + Cn], ci[rp[3] + 1] = col, col
    holds = np.array([bool(np.any(ci[rp[i]:rp[i + 1]] == col)) for i in range(nr)])
    assert holds.tolist() == [False, False, True, True] + [False] * 5
    V = _panel(k, pdt, 9)
    base = _sym_base(k, 9)
    x0 = np.random.default_rng(9).standard_normal((nr, k))
    h = K.to_handle(_csr(nr, nc, rp, ci, vs))
    try:
        for bad in (np.nan, np.inf, -np.inf):
            Vb = V.copy()
            Vb[col, 1] = bad
            for xx, b in ((None, None), (x0, base)):
                clean = _run(h, 1, V, True, 'values', b, 0.5, 0.0, None, 3, xx)[0]
                off = _run(h, 0, Vb, True, 'values', b, 0.5, 0.0, None, 3, xx)[0]
                for L in (1, 5, Cn + 2):
                    got = _run(h, L, Vb, True, 'values', b, 0.5, 0.0, None, 3, xx)[0]
                    assert _same3(got, off), (bad, L)
                    assert _same3(tuple(a[~holds] for a in got), tuple(a[~holds] for a in clean)), (bad, L)
                    assert not np.isfinite(got[1][holds]).any()
    finally:
        K.release_handle(h)


def test_stops(llim):
    "steps = 0; a tol2 that stops different long rows after different step counts; a NaN rs stops (the uniform stop)"
    from csr_amd.kernels import hip as K
    k = 5
    Cn = _chunk(llim, k, np.float64)
    lens = [0, 1, 2, 3, Cn + 1, 9, 2 * Cn + 3, 2]
    nr, nc, rp, ci, vs = _pattern(lens, seed=3)
    V = _panel(k, np.float64, 3)
    x0 = np.random.default_rng(3).standard_normal((nr, k))
    h = K.to_handle(_csr(nr, nc, rp, ci, vs))
    try:
        for xx in (None, x0):
            off = _run(h, 0, V, False, 'values', None, 0.25, 0.0, None, 0, xx)[0]
            on = _run(h, 1, V, False, 'values', None, 0.25, 0.0, None, 0, xx)[0]
            assert _same3(on, off) and not on[2].any()
            if xx is not None:
                assert _same(on[0], x0)                      # no step: x0's bits come back
        first = _run(h, 0, V, False, 'values', None, 0.25, 0.0, None, 0, x0)[0][1]
        seen = set()
        for tol2 in (0.0, 1e-20, 1e-6, float(np.median(first)), float(first.max()), float(first.max()) * 2, float('inf')):
            tol = math.sqrt(tol2) if math.isfinite(tol2) else tol2
            off = _run(h, 0, V, False, 'values', None, 0.25, 0.0, None, 8, x0, tol)[0]
            on = _run(h, 1, V, False, 'values', None, 0.25, 0.0, None, 8, x0, tol)[0]
            assert _same3(on, off), tol2
            seen |= {tuple(on[2])}
        assert any(len(set(t[1:])) >= 3 for t in seen)       # some tolerance stopped the long rows after three different counts
        # the exact reference once, at a tolerance that splits the rows (the C entry's tol2 is tol * tol, as the wrapper squares it)
        tol = 1e-3
        want = R.cg_exact(rp, ci, vs, V, False, 'values', None, 0.25, 0.0, 8, tol * tol, x0)
        assert _same3(_run(h, 1, V, False, 'values', None, 0.25, 0.0, None, 8, x0, tol)[0], want)
        # a NaN in a V row that rows 4 and 6 hold: their rs is NaN, no step is made, and the rows beside them run on
        Vn = V.copy()
        col = G.NCOLS - 1
        ci2 = ci.copy()
        ci2[ci2 == col] = 0
        ci2[rp[4] + Cn], ci2[rp[6] + 1] = col, col
        Vn[col, 1] = np.nan
        hn = K.to_handle(_csr(nr, nc, rp, ci2, vs))
        try:
            for xx in (None, x0):
                off = _run(hn, 0, Vn, False, 'values', None, 0.25, 0.0, None, 8, xx)[0]
                on = _run(hn, 1, Vn, False, 'values', None, 0.25, 0.0, None, 8, xx)[0]
                assert _same3(on, off)
                assert np.isnan(on[1][[4, 6]]).all() and not on[2][[4, 6]].any() and on[2][[3, 5, 7]].min() >= 1
        finally:
            K.release_handle(hn)
    finally:
        K.release_handle(h)


def test_empty_cases_launch_nothing():
    "an empty range and a matrix without entries: the long rows' launch is not issued"
    from csr_amd import CSR
    from csr_amd.kernels import hip as K
    k = 5
    V = _panel(k, np.float64, 1)
    none = CSR(4, G.NCOLS, 0, np.zeros(5, np.int32), np.zeros(0, np.int32), np.zeros(0))
    x0 = np.random.default_rng(1).standard_normal((4, k))
    h = K.to_handle(none)
    try:
        off = _run(h, 0, V, False, 'values', None, 0.5, 0.0, None, 2, x0)[0]
        on, st = _run(h, 1, V, False, 'values', None, 0.5, 0.0, None, 2, x0)
        assert _same3(on, off) and st == (1, 1, 0, 0, 0, 0)
        on, st = _run(h, 1, V, False, 'values', None, 0.5, 0.0, (2, 2), 2, None)
        assert on[0].shape == (0, k) and st == (0, 1, 0, 0, 0, 0)
    finally:
        K.release_handle(h)
