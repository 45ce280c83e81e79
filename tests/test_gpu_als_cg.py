"""
csrk_als_rows_cg on the card (include/csrk.h, rule C): x, resid and taken bit for bit against the exact restatement of rules
C2 - C7 (tests/als_cg_ref.py) at every edge of DOT's ownership (pieces, half chunks, chunks, the largest k) for both panel
types, at every edge of the entry loop, with every option; the same bits from every variant of one request; the stop rule;
long rows and full runs against float64 NumPy and against the exact route (csrk_als_rows); NaN / Inf, empty rows and an
indefinite base by position; every refusal with the outputs untouched.

The exact reference makes about 10^5 fused steps per second: a dense base costs k^2 of them per product and row, an entry
2 k.  Every exact case is sized by that (a few seconds at most), so at k >= 63 a dense base goes with two short rows.
"""
import ctypes as C

import numpy as np
import pytest

import als_cg_ref as R

pytestmark = pytest.mark.gpu

NCOLS = 200
RHS = ('ones', 'values', 'one_plus_values')


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same(a, b):
    "equal bits, a NaN matching any NaN (a created NaN has its position specified, not its sign or payload)"
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _same3(got, want):
    return _same(got[0], want[0]) and _same(got[1], want[1]) and np.array_equal(got[2], want[2])


def _csr(nr, nc, rp, ci, vs, ptr64=False):
    from csr_amd import CSR
    return CSR(nr, nc, int(rp[-1]), np.asarray(rp).astype(np.int64 if ptr64 else np.int32), np.asarray(ci, np.int32).copy(),
               None if vs is None else vs.copy(), _cast=False)


def _pattern(lens, seed, vdt=np.float64):
    "rows of the given lengths over NCOLS columns: unsorted, a column repeated in every row of three or more entries; values in (0.1, 1.1), exact in float32"
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    rp = np.zeros(len(lens) + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    nnz = int(rp[-1])
    ci = rng.integers(0, NCOLS, nnz).astype(np.int32)
    for r in range(len(lens)):
        if lens[r] >= 3:
            ci[rp[r] + 2] = ci[rp[r]]
    vs = None if vdt is None else (rng.random(nnz) + 0.1).astype(np.float32).astype(vdt)
    return len(lens), NCOLS, rp, ci, vs


def _panel(k, pdt, seed):
    rng = np.random.default_rng(1000 + seed)
    return (rng.standard_normal((NCOLS, k)) * (1.0 + np.arange(k) / 7.0) / np.sqrt(k)).astype(pdt)


def _sym_base(k, seed, lam=0.5):
    "symmetric positive definite: lam I + a small Gram"
    rng = np.random.default_rng(3000 + seed)
    A = rng.standard_normal((k + 2, k)) * 0.3
    b = A.T @ A + lam * np.eye(k)
    return np.ascontiguousarray((b + b.T) / 2)


@pytest.fixture(scope='module')
def limits():
    from csr_amd.kernels import hip as K
    return K.als_cg_limits()


def _edge_lens(limits):
    E = int(limits[2])
    return [0, 1, 2, E - 1, E, E + 1, 2 * E + 1]


def _mixed_lens(limits):
    "300 rows, at most 5000 entries: empty runs at both ends, the entry loop's edges, a long row, short rows"
    E = int(limits[2])
    rng = np.random.default_rng(7)
    lens = np.concatenate([np.zeros(5, np.int64), [1, E - 1, E, E + 1, 2 * E - 1, 2 * E, 2 * E + 1, 700], rng.integers(0, 28, 280),
                           np.zeros(7, np.int64)]).astype(np.int64)
    assert len(lens) == 300 and lens.sum() <= 5000
    return lens


# ---- 1. bit for bit against the exact restatement ---------------------------------------------------------------

KS = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128]


def _cg_ks(limits):
    "DOT's edges from the limits: the first pieces, the lanes' columns (a quarter chunk), half a chunk, a chunk, the largest k"
    L, kmax = int(limits[1]), int(limits[0])
    ks = {1, 2, 3, kmax - 1, kmax}
    for m in (1, 2, 4):
        ks |= {m * L - 1, m * L, m * L + 1}
    return sorted(k for k in ks if k <= kmax)


def test_every_k_edge_is_parametrised(limits):
    assert KS == _cg_ks(limits), 'the parametrisation is out of date with csrk_als_cg_limits'
    assert int(limits[2]) >= 1 and len(set(_edge_lens(limits))) >= 5


def _combos(k, limits):
    "(scale, rhs, with a base, with an x0, steps, row lengths) per library call"
    lens = _edge_lens(limits)
    short = [0, lens[-2]]                                       # with a dense base at k >= 63: an empty row and one of E + 1 entries
    if k in (17, 64):                                           # every option, and every pair of (scale, rhs) with (base, x0)
        out, n = [], 0
        for scale in (False, True):
            for rhs in RHS:
                for with_base in (False, True):
                    for with_x0 in (False, True):
                        out.append((scale, rhs, with_base, with_x0, (0, 1, 3)[n % 3], short if (with_base and k > 33) else lens))
                        n += 1
        assert {c[4] for c in out if c[2]} == {0, 1, 3} == {c[4] for c in out if c[3]}
        return out
    return [(True, 'one_plus_values', False, False, 3, lens),
            (False, 'values', True, True, 1, lens if k <= 33 else short),
            (k % 2 == 0, 'ones', False, True, 3, lens)]


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('pdt', [np.float64, np.float32])
def test_rows_are_the_exact_chain(k, pdt, limits):
    from csr_amd.kernels import hip as K
    V = _panel(k, pdt, k)
    base = _sym_base(k, k)
    vdt = np.float64 if pdt == np.float64 else np.float32
    for n, (scale, rhs, with_base, with_x0, steps, lens) in enumerate(_combos(k, limits)):
        nr, nc, rp, ci, vs = _pattern(lens, seed=100 * k + n, vdt=vdt)
        x0 = np.random.default_rng(n).standard_normal((nr, k)) if with_x0 else None
        b = base if with_base else None
        want = R.cg_exact(rp, ci, vs, V, scale, rhs, b, 0.125, 0.0625, steps, 0.0, x0)
        h = K.to_handle(_csr(nr, nc, rp, ci, vs))
        try:
            got = K.als_rows_cg(h, V, scale, rhs, b, 0.125, 0.0625, None, steps, x0, 0.0)
        finally:
            K.release_handle(h)
        assert got[0].dtype == np.float64 and got[1].dtype == np.float64 and got[2].dtype == np.int32
        assert _same(got[0], want[0]), (scale, rhs, with_base, with_x0, steps)
        assert _same(got[1], want[1]) and np.array_equal(got[2], want[2]), (scale, rhs, with_base, with_x0, steps)


def test_the_exact_reference_tells_a_kernel_without_fma_apart(limits):
    from csr_amd.kernels import hip as K
    k = 17
    nr, nc, rp, ci, vs = _pattern(_edge_lens(limits), seed=5)
    V = _panel(k, np.float64, 5)
    h = K.to_handle(_csr(nr, nc, rp, ci, vs))
    try:
        got = K.als_rows_cg(h, V, True, 'values', None, 0.125, 0.0, None, 3, None, 0.0)
    finally:
        K.release_handle(h)
    two = R.cg_two_rounding(rp, ci, vs, V, True, 'values', None, 0.125, 0.0, 3)
    assert np.count_nonzero(got[0] != two[0]) >= k and np.allclose(got[0], two[0], rtol=1e-9, atol=1e-12)


# ---- 2. variants of one request ---------------------------------------------------------------------------------

def _device_call(h, pv, ldv, k, code, scale, rcode, rb, re_, dbase, lam, lam_n, steps, tol2, dx0, ldx0, stream=None, pad=0, info=True,
                 inplace=False):
    "the device entry: (out [n, k + pad] with -7.0 around the result, resid, taken) as NumPy; inplace: out is x0's buffer"
    import torch
    from csr_amd._lib import lib, check
    n = re_ - rb
    if inplace:
        out, ldo = dx0, ldx0
    else:
        out = torch.full((n, k + pad), -7.0, dtype=torch.float64, device='cuda')
        ldo = k + pad
    resid = torch.full((n,), -7.0, dtype=torch.float64, device='cuda')
    taken = torch.full((n,), -7, dtype=torch.int32, device='cuda')
    args = (h.H, rb, re_, pv, ldv, k, code, int(scale), rcode, None if dbase is None else dbase.data_ptr(), lam, lam_n, steps, tol2,
            None if dx0 is None else dx0.data_ptr(), ldx0, out.data_ptr(), ldo, resid.data_ptr() if info else None,
            taken.data_ptr() if info else None)
    if stream is None:
        check(lib.csrk_als_rows_cg_device(*args, None))
        torch.cuda.synchronize()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            check(lib.csrk_als_rows_cg_device(*args, C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
    return out.cpu().numpy(), resid.cpu().numpy(), taken.cpu().numpy()


@pytest.mark.parametrize('k', [3, 17, 33, 64, 90])
@pytest.mark.parametrize('pdt', [np.float64, np.float32])
def test_variants_give_the_same_bits(k, pdt, limits):
    import torch
    from csr_amd.kernels import hip as K
    from csr_amd._lib import VAL_F32, VAL_F64
    nr, nc, rp, ci, vs = _pattern(_mixed_lens(limits), seed=k)
    V = _panel(k, pdt, k)
    base = _sym_base(k, k)
    lam, lam_n, steps = 0.125, 0.0625, 3
    code = VAL_F64 if pdt == np.float64 else VAL_F32
    x0 = np.random.default_rng(k).standard_normal((nr, k)) * 0.1
    A32 = _csr(nr, nc, rp, ci, vs)
    h32, h64, hf32 = K.to_handle(A32), K.to_handle(_csr(nr, nc, rp, ci, vs, ptr64=True)), K.to_handle(_csr(nr, nc, rp, ci, vs.astype(np.float32)))
    hnone, hones = K.to_handle(_csr(nr, nc, rp, ci, None)), K.to_handle(_csr(nr, nc, rp, ci, np.ones(len(ci))))
    try:
        assert K._info(h32.H)[3] == 0 and K._info(h64.H)[3] == 1
        for scale, rhs, b, xx in ((False, 'values', None, None), (True, 'one_plus_values', base, x0), (True, 'ones', None, x0)):
            rcode = RHS.index(rhs)
            full = K.als_rows_cg(h32, V, scale, rhs, b, lam, lam_n, None, steps, xx, 0.0)
            if b is not None:
                by_handle = full
            assert np.isfinite(full[0]).all() and full[2].max() == steps
            # int64 row pointers, float32 values, and a second call
            for hh in (h64, hf32, h32):
                assert _same3(K.als_rows_cg(hh, V, scale, rhs, b, lam, lam_n, None, steps, xx, 0.0), full)
            # absent values count as 1.0
            assert _same3(K.als_rows_cg(hnone, V, scale, rhs, b, lam, lam_n, None, steps, xx, 0.0),
                          K.als_rows_cg(hones, V, scale, rhs, b, lam, lam_n, None, steps, xx, 0.0))
            # the same rows asked for in ranges: an empty range, single rows, the rest
            for rb, re_ in ((0, 0), (0, 1), (1, 140), (140, 141), (141, 299), (299, 300), (300, 300)):
                part = K.als_rows_cg(h32, V, scale, rhs, b, lam, lam_n, (rb, re_), steps, None if xx is None else xx[rb:re_], 0.0)
                assert part[0].shape == (re_ - rb, k) and part[1].shape == (re_ - rb,) and part[2].shape == (re_ - rb,)
                assert _same3(part, tuple(a[rb:re_] for a in full)), (rb, re_)
            # the host entry with strided views of V and x0 (it packs them on the way)
            Vw = np.zeros((nc, k + 3), pdt)
            Vw[:, 1:1 + k] = V
            xw = None
            if xx is not None:
                xw = np.zeros((nr, k + 2))
                xw[:, 2:] = xx
                xw = xw[:, 2:]
            assert _same3(K.als_rows_cg(h64, Vw[:, 1:1 + k], scale, rhs, b, lam, lam_n, None, steps, xw, 0.0), full)
            # the device entry: V packed (16-B loads where k allows), in a panel whose row stride is padded, and one element
            # into a wider panel (element loads); x0 padded; out inside a wider panel whose other columns stay; the default
            # stream and a side stream; resid and taken wanted and NULL; a row sub-range; x0 == out in place
            dbase = None if b is None else torch.from_numpy(b).cuda()
            wide = (k // 4 + 1) * 4
            for n, (off, ld) in enumerate(((0, k), (0, wide), (1, k + 3))):
                dV = torch.zeros(nc, ld + off, dtype=torch.from_numpy(V).dtype, device='cuda')
                dV[:, off:off + k] = torch.from_numpy(V).cuda()
                pv = dV[:, off:].data_ptr()
                assert (pv % 16 != 0) == (off != 0)
                st = torch.cuda.Stream() if n != 1 else None
                pad = (0, 5, 1)[n]
                dx0, ldx0 = None, 0
                if xx is not None:
                    dx0 = torch.full((nr, k + n), 9.0, dtype=torch.float64, device='cuda')
                    dx0[:, :k] = torch.from_numpy(xx).cuda()
                    ldx0 = k + n
                got = _device_call(h32 if n else h64, pv, dV.stride(0), k, code, scale, rcode, 0, nr, dbase, lam, lam_n, steps, 0.0, dx0,
                                   ldx0, st, pad)
                assert _same3((got[0][:, :k],) + got[1:], full) and np.all(got[0][:, k:] == -7.0), (off, ld)
                sub0 = None if dx0 is None else dx0[137:]
                got = _device_call(h32, pv, dV.stride(0), k, code, scale, rcode, 137, 150, dbase, lam, lam_n, steps, 0.0, sub0, ldx0, st,
                                   pad, info=False)
                assert _same(got[0][:, :k], full[0][137:150]) and np.all(got[0][:, k:] == -7.0), (off, ld)
                assert np.all(got[1] == -7.0) and np.all(got[2] == -7)
                if dx0 is not None:
                    got = _device_call(h32, pv, dV.stride(0), k, code, scale, rcode, 0, nr, dbase, lam, lam_n, steps, 0.0, dx0, ldx0, st,
                                       inplace=True)
                    assert _same3((got[0][:, :k],) + got[1:], full) and np.all(got[0][:, k:] == 9.0), (off, ld)
    finally:
        for h in (h32, h64, hf32, hnone, hones):
            K.release_handle(h)
    # the method: of base the lower triangle is read and mirrored, reg and reg_per_entry are lam and lam_n
    low = np.tril(base) + np.triu(np.full((k, k), -777.0), 1)
    got = A32.als_rows_cg(V, x0=x0, weighted=True, rhs='one_plus_values', base=low, reg=lam, reg_per_entry=lam_n, return_info=True)
    assert _same3(got, by_handle)
    assert _same(got[0], A32.als_rows_cg(V, x0=x0, weighted=True, rhs='one_plus_values', base=base, reg=lam, reg_per_entry=lam_n))
    perm = np.random.default_rng(k).permutation(nr)
    assert _same(A32.pick_rows(perm).als_rows_cg(V, x0=x0[perm], weighted=True, rhs='one_plus_values', base=base, reg=lam),
                 A32.als_rows_cg(V, x0=x0, weighted=True, rhs='one_plus_values', base=base, reg=lam)[perm])


# ---- 3. the stop rule -------------------------------------------------------------------------------------------

def _host_call(A, V, scale, rcode, lam, lam_n, steps, tol2, x0):
    "the host C entry on float64 panels without a base: (x, resid, taken)"
    from csr_amd.kernels import hip as K
    from csr_amd._lib import lib, check, VAL_F64
    nr, k = A.nrows, V.shape[1]
    out, resid, taken = np.zeros((nr, k)), np.zeros(nr), np.zeros(nr, np.int32)
    h = K.to_handle(A)
    try:
        check(lib.csrk_als_rows_cg(h.H, 0, nr, V.ctypes.data, k, k, VAL_F64, scale, rcode, None, lam, lam_n, steps, tol2,
                                   None if x0 is None else x0.ctypes.data, k, out.ctypes.data, k, resid.ctypes.data, taken.ctypes.data))
    finally:
        K.release_handle(h)
    return out, resid, taken


def test_stop_rule(limits):
    from csr_amd import CSR
    # the hand case: k = 1, V = [[2]], c = 4, lam = 4: one step of five, resid +0.0
    for pdt in (np.float64, np.float32):
        hand = CSR(1, 1, 1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([4.0]))
        x, rs, taken = hand.als_rows_cg(np.array([[2.0]], pdt), steps=5, reg=4.0, return_info=True)
        assert x.tolist() == [[1.0]] and rs.tolist() == [0.0] and not np.signbit(rs[0]) and taken.tolist() == [1]
    # rows that stop at different steps: resid is the rs the reference holds at the stop, bit for bit
    k = 5
    nr, nc, rp, ci, vs = _pattern([0, 1, 2, 3, 5, 9, 4, 2], seed=3)
    V = _panel(k, np.float64, 3)
    A = _csr(nr, nc, rp, ci, vs)
    x0 = np.random.default_rng(3).standard_normal((nr, k))
    first = R.cg_exact(rp, ci, vs, V, False, 'values', None, 0.25, 0.0, 0, 0.0, x0)[1]
    for tol2 in (0.0, 1e-20, 1e-6, float(np.median(first)), float(first.max()), float(first.max()) * 2, float('inf')):
        want = R.cg_exact(rp, ci, vs, V, False, 'values', None, 0.25, 0.0, 8, tol2, x0)
        got = _host_call(A, V, 0, 1, 0.25, 0.0, 8, tol2, x0)          # (the C entry: it takes tol2 itself, the method squares a tol)
        assert _same3(got, want), tol2
        assert np.all((got[1] <= tol2) | (got[2] == 8))
    # a tol2 at or above the first rs: no step, x is x0's bits, resid that first rs
    got = A.als_rows_cg(V, x0=x0, steps=8, reg=0.25, tol=float('inf'), return_info=True)
    assert _same(got[0], x0) and _same(got[1], first) and not got[2].any()
    # a NaN rs stops: a NaN in one V row that rows 4 and 5 reference
    Vn = V.copy()
    Vn[ci[rp[4]], 1] = np.nan
    holds = np.array([bool(np.any(ci[rp[i]:rp[i + 1]] == ci[rp[4]])) for i in range(nr)])
    assert holds[4] and not holds.all()
    for xx in (None, x0):
        got = A.als_rows_cg(Vn, x0=xx, steps=8, reg=0.25, return_info=True)
        assert np.isnan(got[1][holds]).all() and not got[2][holds].any() and np.isfinite(got[1][~holds]).all()
        clean = A.als_rows_cg(V, x0=xx, steps=8, reg=0.25, return_info=True)
        assert _same3(tuple(a[~holds] for a in got), tuple(a[~holds] for a in clean))
        if xx is None:
            assert np.all(got[0][holds] == 0.0)          # cold: x stays +0.0, the NaN shows in resid


# ---- 4. long rows and convergence -------------------------------------------------------------------------------

def _rel(a, b):
    "the largest relative distance of two sets of rows: max_i |a_i - b_i|_inf / |b_i|_inf (rows that are zero in both: 0)"
    a, b = np.asarray(a), np.asarray(b)
    num, den = np.abs(a - b).max(axis=1), np.abs(b).max(axis=1)
    assert np.all(num[den == 0.0] == 0.0)
    return float(np.max(num[den > 0.0] / den[den > 0.0])) if np.any(den > 0.0) else 0.0


def _long_case(which, limits):
    if which == 'one long row':
        k, lens, base = 64, [5000], None
    else:
        k, lens, base = 33, _mixed_lens(limits), _sym_base(33, 33, lam=0.25)
    nr, nc, rp, ci, vs = _pattern(lens, seed=k)
    return k, nr, nc, rp, ci, vs, _panel(k, np.float64, k), base


@pytest.fixture(scope='module')
def long_refs(limits):
    "per case: the inputs, the direct solution, and cg_numpy in both orders for both runs -- computed once"
    out = {}
    for which in ('one long row', 'mixed rows'):
        k, nr, nc, rp, ci, vs, V, base = _long_case(which, limits)
        lam = 0.1
        args = (rp, ci, vs, V, True, 'one_plus_values', base, lam, 0.0)
        bb = R.cg_numpy(*args, 0)[1]                                          # steps = 0 from zero: resid = DOT(b, b)
        tol2 = 2.0 ** -96 * float(bb.max())
        # the systems themselves, for the direct solve
        direct = np.zeros((nr, k))
        for i in range(nr):
            Vr, w = V[ci[rp[i]:rp[i + 1]]], vs[rp[i]:rp[i + 1]]
            M = (np.zeros((k, k)) if base is None else base) + lam * np.eye(k) + (Vr * w[:, None]).T @ Vr
            direct[i] = np.linalg.solve(M, (1.0 + w) @ Vr)
        warm = direct * (1.0 + 0.01 * np.random.default_rng(1).standard_normal(direct.shape))
        runs = {}
        for name, steps, x0 in (('warm', 3, warm), ('cold', 2 * k, None)):
            runs[name] = (steps, x0, R.cg_numpy(*args, steps, tol2, x0, order=1), R.cg_numpy(*args, steps, tol2, x0, order=-1))
        out[which] = dict(k=k, csr=(nr, nc, rp, ci, vs), V=V, base=base, lam=lam, tol2=tol2, direct=direct, runs=runs)
    return out


@pytest.mark.parametrize('which', ['one long row', 'mixed rows'])
@pytest.mark.parametrize('run', ['warm', 'cold'])
def test_long_rows_against_numpy(which, run, long_refs):
    """
    Against cg_numpy(order=+1).  The tolerance is computed here: 4 x the largest relative distance between cg_numpy(+1) and
    cg_numpy(-1) on the same inputs.  The two references differ only in their order of addition, which is all that
    separates the kernel from either; the factor 4 covers the kernel's two further reorderings (DOT's tree, fused steps).
    tol2 = 2^-96 max_i DOT(b_i, b_i) keeps the runs out of rule C10's hazard; it is a condition, not a measurement.
    """
    from csr_amd.kernels import hip as K
    c = long_refs[which]
    steps, x0, up, down = c['runs'][run]
    h = K.to_handle(_csr(*c['csr']))
    try:
        got = K.als_rows_cg(h, c['V'], True, 'one_plus_values', c['base'], c['lam'], 0.0, None, steps, x0, np.sqrt(c['tol2']))
    finally:
        K.release_handle(h)
    tol = 4.0 * _rel(up[0], down[0])
    dist = _rel(got[0], up[0])
    print(f'{which}, {run}: kernel to numpy(+1) {dist:.3e}, numpy(+1) to numpy(-1) {tol / 4:.3e}, bound {tol:.3e}, '
          f'taken {got[2].min()}..{got[2].max()} (numpy {up[2].min()}..{up[2].max()})')
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert dist <= tol


@pytest.mark.parametrize('which', ['one long row', 'mixed rows'])
def test_full_runs_meet_the_exact_route(which, long_refs):
    """
    At steps = 2 k from zero the result is also held to CSR.als_rows on the same systems, within the tolerance above plus
    cg_numpy's own distance to numpy.linalg.solve.  (A NumPy CG reaches about 6e-14 relative of the direct solve at k = 128
    on such systems; that figure is a record, not the bound.)
    """
    c = long_refs[which]
    steps, x0, up, down = c['runs']['cold']
    A = _csr(*c['csr'])
    base = c['base']
    ridge = c['lam'] * np.eye(c['k']) + (0.0 if base is None else base)
    exact = A.als_rows(c['V'], weighted=True, rhs='one_plus_values', base=ridge)
    got = A.als_rows_cg(c['V'], steps=steps, weighted=True, rhs='one_plus_values', base=base, reg=c['lam'], tol=np.sqrt(c['tol2']))
    tol = 4.0 * _rel(up[0], down[0]) + _rel(up[0], c['direct'])
    dist = _rel(got, exact)
    print(f'{which}: kernel CG to als_rows {dist:.3e}, bound {tol:.3e} (numpy CG to numpy solve {_rel(up[0], c["direct"]):.3e})')
    assert dist <= tol


# ---- 5. other cases ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('pdt', [np.float64, np.float32])
def test_nan_and_inf_touch_only_the_rows_that_hold_them(pdt, limits):
    k = 3
    nr, nc, rp, ci, vs = _pattern([0, 4, 2, 9, 1, 5, 3, 0, 6], seed=9)
    V = _panel(k, pdt, 9)
    A = _csr(nr, nc, rp, ci, vs)
    base = _sym_base(k, 9)
    x0 = np.random.default_rng(9).standard_normal((nr, k))
    for bad in (np.nan, np.inf, -np.inf):
        col = int(ci[rp[3] + 1])
        Vb = V.copy()
        Vb[col, 1] = bad
        holds = np.array([bool(np.any(ci[rp[i]:rp[i + 1]] == col)) for i in range(nr)])
        assert holds.any() and not holds.all()
        for xx, b in ((None, None), (x0, base)):
            clean = A.als_rows_cg(V, x0=xx, weighted=True, base=b, reg=0.5, return_info=True)
            got = A.als_rows_cg(Vb, x0=xx, weighted=True, base=b, reg=0.5, return_info=True)
            assert _same3(tuple(a[~holds] for a in got), tuple(a[~holds] for a in clean)), bad
            assert _same3(got, R.cg_exact(rp, ci, vs, Vb, True, 'values', b, 0.5, 0.0, 3, 0.0, xx)), bad
            assert not np.isfinite(got[1][holds]).any()


def test_empty_rows_and_an_indefinite_base(limits):
    k = 3
    nr, nc, rp, ci, vs = _pattern([0, 2, 0, 0, 5, 0], seed=4)
    V = _panel(k, np.float64, 4)
    A = _csr(nr, nc, rp, ci, vs)
    empty = np.diff(rp) == 0
    # rule C8: cold, an empty row gives x = +0.0, resid +0.0, taken 0 -- with any base
    for b in (None, _sym_base(k, 4), np.array([[1.0, 2.0, 0.0], [2.0, -3.0, 0.5], [0.0, 0.5, 0.25]])):
        x, rs, taken = A.als_rows_cg(V, base=b, reg=0.5, steps=4, return_info=True)
        assert np.all(_bits(x[empty]) == 0) and np.all(_bits(rs[empty]) == 0) and not taken[empty].any()
        assert _same3((x, rs, taken), R.cg_exact(rp, ci, vs, V, False, 'values', b, 0.5, 0.0, 4))
    # warm, an empty row solves (base + lam I) x = 0 from x0: the reference's bits, an indefinite base included
    x0 = np.random.default_rng(4).standard_normal((nr, k))
    indef = np.array([[1.0, 2.0, 0.0], [2.0, -3.0, 0.5], [0.0, 0.5, 0.25]])
    assert np.linalg.eigvalsh(indef + 0.5 * np.eye(k)).min() < 0
    for b in (None, _sym_base(k, 4), indef):
        for steps in (1, 3, 6):
            got = A.als_rows_cg(V, x0=x0, base=b, reg=0.5, steps=steps, return_info=True)
            assert _same3(got, R.cg_exact(rp, ci, vs, V, False, 'values', b, 0.5, 0.0, steps, 0.0, x0)), steps


def test_refusals_leave_the_outputs_untouched(limits):
    import torch
    from csr_amd._lib import lib, ERR_INVALID, ERR_UNSUPPORTED, VAL_F64
    from csr_amd.kernels import hip as K
    k = 4
    nr, nc, rp, ci, vs = _pattern([3, 0, 5, 2], seed=6)
    h = K.to_handle(_csr(nr, nc, rp, ci, vs))
    try:
        V = torch.ones(nc, k + 1, dtype=torch.float64, device='cuda')
        base = torch.eye(k, dtype=torch.float64, device='cuda')
        x0 = torch.ones(nr, k + 1, dtype=torch.float64, device='cuda')
        out = torch.full((nr, k), -7.0, dtype=torch.float64, device='cuda')
        resid = torch.full((nr + 1,), -7.0, dtype=torch.float64, device='cuda')
        taken = torch.full((nr + 2,), -7, dtype=torch.int32, device='cuda')
        g = dict(rb=0, re=nr, V=V.data_ptr(), ldv=k + 1, k=k, pt=VAL_F64, scale=1, rhs=1, base=base.data_ptr(), lam=0.5, lam_n=0.0, steps=3,
                 tol2=0.0, x0=x0.data_ptr(), ldx0=k + 1, out=out.data_ptr(), ldo=k, resid=resid.data_ptr(), taken=taken.data_ptr())
        order = ('rb', 're', 'V', 'ldv', 'k', 'pt', 'scale', 'rhs', 'base', 'lam', 'lam_n', 'steps', 'tol2', 'x0', 'ldx0', 'out', 'ldo',
                 'resid', 'taken')
        cases = {
            'k = 0': dict(k=0), 'ldv < k': dict(ldv=k - 1), 'ldo < k': dict(ldo=k - 1), 'panel type': dict(pt=0), 'scale': dict(scale=-1),
            'rhs_mode': dict(rhs=-1), 'steps < 0': dict(steps=-1), 'tol2 < 0': dict(tol2=-1e-300), 'tol2 NaN': dict(tol2=float('nan')),
            'ldx0 < k': dict(ldx0=k - 1), 'rows reversed': dict(rb=2, re=1), 'rows negative': dict(rb=-1), 'rows past the end': dict(re=nr + 1),
            'NULL out': dict(out=None), 'NULL V': dict(V=None), 'V misaligned': dict(V=V.data_ptr() + 4),
            'base misaligned': dict(base=base.data_ptr() + 4), 'x0 misaligned': dict(x0=x0.data_ptr() + 4),
            'out misaligned': dict(out=out.data_ptr() + 4), 'resid misaligned': dict(resid=resid.data_ptr() + 4),
            'taken misaligned': dict(taken=taken.data_ptr() + 2),
        }
        for name, change in cases.items():
            a = dict(g, **change)
            assert lib.csrk_als_rows_cg_device(h.H, *[a[n] for n in order], None) == ERR_INVALID, name
            assert lib.csrk_last_error(), name
        kk = int(limits[0]) + 1
        Vb = torch.ones(nc, kk, dtype=torch.float64, device='cuda')
        ob = torch.full((nr, kk), -7.0, dtype=torch.float64, device='cuda')
        assert lib.csrk_als_rows_cg_device(h.H, 0, nr, Vb.data_ptr(), kk, kk, VAL_F64, 0, 1, None, 0.5, 0.0, 3, 0.0, None, kk, ob.data_ptr(),
                                           kk, resid.data_ptr(), taken.data_ptr(), None) == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((ob == -7.0).all()) and bool((resid == -7.0).all()) and bool((taken == -7).all())
        # the host entry: the same refusals with host buffers
        hV, hout, hres, htak = np.ones((nc, k)), np.full((nr, k), -7.0), np.full(nr, -7.0), np.full(nr, -7, np.int32)
        for name, args in {'rows past the end': (0, nr + 1, hV.ctypes.data, k, k, VAL_F64, 0, 1, None, 0.5, 0.0, 3, 0.0, None, k),
                           'steps < 0': (0, nr, hV.ctypes.data, k, k, VAL_F64, 0, 1, None, 0.5, 0.0, -1, 0.0, None, k),
                           'NULL V': (0, nr, None, k, k, VAL_F64, 0, 1, None, 0.5, 0.0, 3, 0.0, None, k)}.items():
            assert lib.csrk_als_rows_cg(h.H, *args, hout.ctypes.data, k, hres.ctypes.data, htak.ctypes.data) == ERR_INVALID, name
        assert lib.csrk_als_rows_cg(h.H, 0, nr, hV.ctypes.data, k, k, VAL_F64, 0, 1, None, 0.5, 0.0, 3, 0.0, None, k, None, k, None,
                                    None) == ERR_INVALID
        assert np.all(hout == -7.0) and np.all(hres == -7.0) and np.all(htak == -7)
        # no rows: fine, NULL pointers and all
        assert lib.csrk_als_rows_cg_device(h.H, 1, 1, None, k, k, VAL_F64, 0, 1, None, 0.5, 0.0, 3, 0.0, None, 0, None, k, None, None, None) == 0
        assert lib.csrk_als_rows_cg(h.H, nr, nr, None, k, k, VAL_F64, 0, 1, None, 0.5, 0.0, 3, 0.0, None, 0, None, k, None, None) == 0
    finally:
        K.release_handle(h)


def test_no_rows_and_no_entries(limits):
    from csr_amd import CSR
    k = 5
    V = _panel(k, np.float64, 1)
    none = CSR(4, NCOLS, 0, np.zeros(5, np.int32), np.zeros(0, np.int32), np.zeros(0))
    x, rs, taken = none.als_rows_cg(V, reg=0.5, return_info=True)
    assert x.shape == (4, k) and np.all(_bits(x) == 0) and np.all(_bits(rs) == 0) and not taken.any()
    x0 = np.random.default_rng(1).standard_normal((4, k))
    got = none.als_rows_cg(V, x0=x0, reg=0.5, steps=2, return_info=True)
    assert _same3(got, R.cg_exact(none.rowptrs, none.colinds, none.values, V, False, 'values', None, 0.5, 0.0, 2, 0.0, x0))
    x, rs, taken = none.als_rows_cg(V, rows=(2, 2), return_info=True)
    assert x.shape == (0, k) and rs.shape == (0,) and taken.shape == (0,)
    norows = CSR(0, NCOLS, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    assert norows.als_rows_cg(V).shape == (0, k)
