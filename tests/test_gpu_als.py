"""
csrk_solve_blocks and csrk_als_rows on the card (include/csrk.h, rules S and A): the solve bit for bit against the exact
restatement of rule S (tests/als_ref.py) at every k class threshold that csrk_als_limits names -- which is also the check
that the card's 1.0 / d is correctly rounded --; the fused row bit for bit against the composed path (csrk_gram_rows, the
ridge and the right-hand side restated exactly, csrk_solve_blocks) at every class and staging boundary; the same bits
from every variant of one request; the textbook residual bound on rows too long for the exact reference; NaN / Inf, empty
rows and indefinite systems by position; every refusal with the outputs untouched.

Matrices have at most 300 rows, 200 columns and 5000 entries.  The exact solve costs about 0.6 s at k = 64, 1.5 s at
k = 88 and 5 s at k = 128 per system, the exact chains about 10^5 element-steps per second: every exact case is sized by
those figures.
"""
import ctypes as C

import numpy as np
import pytest

import als_ref as R
import gram_ref

pytestmark = pytest.mark.gpu

NCOLS = 200


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same(a, b):
    "equal bits, a NaN matching any NaN (a created NaN has its position specified, not its sign or payload)"
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _csr(nr, nc, rp, ci, vs, ptr64=False):
    from csr_amd import CSR
    return CSR(nr, nc, int(rp[-1]), np.asarray(rp).astype(np.int64 if ptr64 else np.int32), np.asarray(ci, np.int32).copy(),
               None if vs is None else vs.copy(), _cast=False)


def _pattern(lens, seed, vdt=np.float64, positive=False):
    "rows of the given lengths over NCOLS columns: unsorted, columns repeated within rows"
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    rp = np.zeros(len(lens) + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    nnz = int(rp[-1])
    ci = rng.integers(0, NCOLS, nnz).astype(np.int32)
    for r in range(len(lens)):                                  # a repeated column in every row of three or more entries
        if lens[r] >= 3:
            ci[rp[r] + 2] = ci[rp[r]]
    vs = None
    if vdt is not None:
        vs = rng.standard_normal(nnz)
        vs = (np.abs(vs) + 0.1 if positive else vs).astype(vdt)
    return len(lens), NCOLS, rp, ci, vs


def _panel(k, pdt, seed):
    "asymmetric in every sense: no two columns alike, so a p <-> q swap shows"
    rng = np.random.default_rng(1000 + seed)
    return (rng.standard_normal((NCOLS, k)) * (1.0 + np.arange(k) / 7.0)).astype(pdt)


def _base(k, seed):
    "asymmetric: the upper triangle holds other numbers than the lower, so reading it shows"
    rng = np.random.default_rng(2000 + seed)
    b = rng.standard_normal((k, k))
    b[np.triu_indices(k, 1)] += 1000.0
    return b


def _pd_base(k, seed, lam=0.5):
    "positive definite in its lower triangle (lam I + a small Gram), other numbers above the diagonal"
    rng = np.random.default_rng(3000 + seed)
    A = rng.standard_normal((k + 2, k)) * 0.1
    b = A.T @ A + lam * np.eye(k)
    b[np.triu_indices(k, 1)] = -777.0
    return b


@pytest.fixture(scope='module')
def limits():
    from csr_amd.kernels import hip as K
    lim = K.als_limits()
    assert tuple(lim) == tuple(K.gram_limits())          # one set of constants (csrc/gram_tile.h)
    return lim


def _mixed_lens(limits):
    "300 rows, at most 5000 entries: empty runs at both ends, every staging boundary, a long row, short rows"
    S = int(limits[1])
    rng = np.random.default_rng(7)
    lens = np.concatenate([np.zeros(5, np.int64), [1, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 700], rng.integers(0, 28, 280),
                           np.zeros(7, np.int64)]).astype(np.int64)
    assert len(lens) == 300 and lens.sum() <= 5000
    return lens


# ---- 1. the solve against the exact restatement -----------------------------------------------------------------

def _systems(k, counts, seed):
    "V^T V + lam I from n random rows each, n in counts; the upper triangles hold other numbers; b random"
    rng = np.random.default_rng(seed)
    G = np.zeros((len(counts), k, k))
    for s, n in enumerate(counts):
        A = rng.standard_normal((n, k))
        G[s] = A.T @ A + (0.05 + 0.3 * rng.random()) * np.eye(k)
        G[s][np.triu_indices(k, 1)] = 1000.0 + rng.standard_normal(k * (k - 1) // 2)
    return G, rng.standard_normal((len(counts), k))


def _solve_ks(limits):
    ks = {1, 2, 3, 4, 5, int(limits[0])}
    for t in limits[2:]:
        ks |= {int(t) - 1, int(t), int(t) + 1}
    return sorted(ks)


@pytest.mark.parametrize('k', [1, 2, 3, 4, 5, 15, 16, 17, 39, 40, 41, 87, 88, 89, 128])
def test_solve_blocks_is_the_exact_chain(k, limits):
    "this is also the check that 1.0 / d is correctly rounded on the card: one wrong quotient changes an L and an x"
    from csr_amd.kernels import hip as K
    assert k in _solve_ks(limits), 'the parametrisation is out of date with csrk_als_limits'
    if k <= 17:
        counts = [0, 1, k // 2, 3 * k] * 5                       # 20 systems: two workgroups of the 16-lane class
    elif k <= 41:
        counts = [0, 1, k // 2, 3 * k, k // 2, 3 * k]             # 6 systems: two workgroups of the wavefront class
    else:
        counts = [3 * k if k != 88 else k // 2]                   # one system: 1.5 s of exact reference at k = 88, 5 s at 128
    G, b = _systems(k, counts, seed=k)
    x, info = K.solve_blocks(G, b)
    want, winfo = R.ldl_exact_batch(G, b)
    assert x.shape == (len(counts), k) and x.dtype == np.float64 and info.dtype == np.int32
    assert np.all(winfo == 0) and np.array_equal(info, winfo)
    bad = np.argwhere(_bits(x) != _bits(want))
    assert len(bad) == 0, (k, len(bad), bad[:4].tolist())


def test_every_solve_k_is_parametrised(limits):
    assert _solve_ks(limits) == [1, 2, 3, 4, 5, 15, 16, 17, 39, 40, 41, 87, 88, 89, 128]


def test_solve_blocks_hand_cases():
    from csr_amd.kernels import hip as K
    a = 1.0 + 2.0 ** -30
    # by hand; where fusing matters; where round(c round(1 / d)) differs from c / d
    G = np.array([[[4.0, 99.0], [2.0, 3.0]], [[1.0, 7.0], [a, 1.0 + 2.0 ** -29 + 2.0 ** -52]], [[38.0, 0.0], [39.0, 50.0]]])
    b = np.array([[2.0, 5.0], [0.0, 1.0], [1.0, 1.0]])
    x, info = K.solve_blocks(G, b)
    assert info.tolist() == [0, 0, 0]
    assert np.array_equal(x[0], [-0.5, 2.0])
    assert x[1][1] == 1.0 / (2.0 ** -52 - 2.0 ** -60) and x[1][1] != 2.0 ** 52            # fused: d1 = 2^-52 - 2^-60
    assert np.array_equal(_bits(x), _bits(R.ldl_exact_batch(G, b)[0]))
    L = 39.0 * (1.0 / 38.0)
    d1 = R.fnma(L, 39.0, 50.0)
    assert L != 39.0 / 38.0 and x[2][1] == R.fnma(L, 1.0, 1.0) * (1.0 / d1)                # x1 = round(z1 r1), z1 = 1 - L
    # every pair of integers below 40: 291 of the 1521 quotients differ from the product with the rounded reciprocal
    pairs = [(c, d) for c in range(1, 40) for d in range(1, 40)]
    Gp = np.array([[[float(d), 0.0], [float(c), 1e6]] for c, d in pairs])
    bp = np.tile([1.0, 0.0], (len(pairs), 1))
    xp, ip = K.solve_blocks(Gp, bp)
    wp, _ = R.ldl_exact_batch(Gp, bp)
    assert np.array_equal(_bits(xp), _bits(wp)) and not ip.any()
    # info: the first pivot that is not positive, a NaN pivot, a pivot the elimination makes negative, all zero
    Gi = np.array([np.diag([1.0, 2.0, -1.0, 4.0]), np.diag([1.0, np.nan, 3.0, 4.0]), np.diag([1.0, 2.0, 3.0, 0.0]), np.zeros((4, 4)),
                   np.diag([1.0, 2.0, 3.0, 4.0])])
    Gi[4][1, 0] = 2.0                                            # d1 = 2 - 2 * 2 = -2
    xi, ii = K.solve_blocks(Gi, np.ones((5, 4)))
    wi, wii = R.ldl_exact_batch(Gi, np.ones((5, 4)))
    assert ii.tolist() == [3, 2, 4, 1, 2] and wii.tolist() == [3, 2, 4, 1, 2]
    assert np.array_equal(gram_ref.classify(xi), gram_ref.classify(wi))
    fin = np.isfinite(wi)
    assert np.array_equal(_bits(xi)[fin], _bits(wi)[fin])
    # the upper triangle is never read
    Gn = G.copy()
    Gn[:, 0, 1] = np.nan
    assert np.array_equal(_bits(K.solve_blocks(Gn, b)[0]), _bits(x))


def test_solve_blocks_device_entry_strides_and_null_info(limits):
    import torch
    from csr_amd.kernels import hip as K
    from csr_amd._lib import lib, check
    for k in (3, 17, 41, 90):
        n = 37
        G, b = _systems(k, [2 * k] * n, seed=100 + k)
        x, info = K.solve_blocks(G, b)
        assert not info.any()
        assert np.array_equal(_bits(x), _bits(K.solve_blocks(G, b)[0]))                    # a second call
        dG = torch.from_numpy(G).cuda()
        db = torch.full((n, k + 3), 5.0, dtype=torch.float64, device='cuda')
        db[:, 1:1 + k] = torch.from_numpy(b).cuda()
        dx = torch.full((n, k + 2), -7.0, dtype=torch.float64, device='cuda')
        di = torch.full((n,), -7, dtype=torch.int32, device='cuda')
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            check(lib.csrk_solve_blocks_device(n, k, dG.data_ptr(), db[:, 1:].data_ptr(), k + 3, dx.data_ptr(), k + 2, di.data_ptr(),
                                               C.c_void_p(st.cuda_stream)))
        st.synchronize()
        got = dx.cpu().numpy()
        assert np.array_equal(_bits(got[:, :k]), _bits(x)) and np.all(got[:, k:] == -7.0) and not di.cpu().numpy().any()
        # part of the batch, info NULL
        dx.fill_(-7.0)
        check(lib.csrk_solve_blocks_device(5, k, dG[20:].data_ptr(), db[20:, 1:].data_ptr(), k + 3, dx.data_ptr(), k + 2, None, None))
        torch.cuda.synchronize()
        got = dx.cpu().numpy()
        assert np.array_equal(_bits(got[:5, :k]), _bits(x[20:25])) and np.all(got[5:] == -7.0) and np.all(got[:, k:] == -7.0)


# ---- 2. the fused row against the composed path -------------------------------------------------------------------

# scale, value dtype (None: structure-only), panel dtype, with base
COMBOS = [(False, np.float64, np.float64, False), (True, np.float64, np.float64, True), (True, np.float32, np.float32, False),
          (True, None, np.float64, True), (False, np.float32, np.float32, True), (True, np.float64, np.float32, False)]


@pytest.mark.parametrize('k', [3, 16, 17, 40, 41, 88, 89, 128])
def test_als_rows_equals_gram_ridge_and_solve(k, limits):
    """
    rows of 0, 1 and S - 1, S, S + 1, 2S - 1, 2S, 2S + 1 entries (S staged per step) at a k of every class: als_rows must be
    solve_blocks(gram_rows + the ridge restated exactly, the right-hand side restated exactly), bit for bit; the six value /
    panel / base combinations, the three right-hand sides and a zero and a nonzero ridge all meet over the ks
    """
    from csr_amd.kernels import hip as K
    assert set(limits[2:]) | {limits[0]} <= {16, 40, 88, 128} and set(K.gram_limits()[2:]) <= {16, 40, 88, 128}
    S = int(limits[1])
    lens = [0, 0, 1, S - 1, S, S + 1, 0, 2 * S - 1, 2 * S, 2 * S + 1, 0, 0]
    first = [3, 16, 17, 40, 41, 88, 89, 128].index(k)
    for c in range(6):
        scale, vdt, pdt, with_base = COMBOS[c]
        rhs = R.RHS[(c + first) % 3]
        lam = (0.0, 0.375)[(c // 3 + first) % 2]
        nr, nc, rp, ci, vs = _pattern(lens, 10 * k + c, vdt)
        V = _panel(k, pdt, k + c)
        base = _base(k, k + c) if with_base else None
        h = K.to_handle(_csr(nr, nc, rp, ci, vs))
        try:
            got, info = K.als_rows(h, V, scale, rhs, base, lam)
            G = K.gram_rows(h, V, scale, None, base)
        finally:
            K.release_handle(h)
        G = R.ridge_exact(G, rp, lam)
        b = R.rhs_exact(rp, ci, vs, V, rhs)
        want, winfo = K.solve_blocks(G, b)
        assert got.shape == (nr, k) and got.dtype == np.float64 and info.dtype == np.int32
        assert _same(got, want), (k, c, rhs, lam, np.argwhere(_bits(got) != _bits(want))[:4].tolist())
        assert np.array_equal(info, winfo), (k, c, info.tolist(), winfo.tolist())
        assert (info[np.diff(rp) == 0] == info[0]).all()          # every empty row alike (row 0 is one)
        if base is None:
            assert (info[np.diff(rp) == 0] == 1).all() and np.isnan(got[np.diff(rp) == 0]).all()
        if k <= 17 and c in (first % 6, (first + 3) % 6):
            assert sum(lens) * k * (k + 1) // 2 <= 100000
            ex, einfo, _, _ = R.als_exact(rp, ci, vs, V, scale, rhs, base, lam)
            assert _same(got, ex) and np.array_equal(info, einfo), (k, c)


# ---- 3. equal bits among the variants of one request ----------------------------------------------------------------

def _device_call(h, dV, ldv, k, code, scale, rcode, rb, re_, dbase, lam, stream=None, pad=0, with_info=True):
    import torch
    from csr_amd._lib import lib, check
    out = torch.full(((re_ - rb), k + pad), -7.0, dtype=torch.float64, device='cuda')
    info = torch.full(((re_ - rb),), -7, dtype=torch.int32, device='cuda')
    pb = None if dbase is None else dbase.data_ptr()
    pi = info.data_ptr() if with_info else None
    if stream is None:
        check(lib.csrk_als_rows_device(h.H, rb, re_, dV, ldv, k, code, int(scale), rcode, pb, lam, out.data_ptr(), k + pad, pi, None))
        torch.cuda.synchronize()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            check(lib.csrk_als_rows_device(h.H, rb, re_, dV, ldv, k, code, int(scale), rcode, pb, lam, out.data_ptr(), k + pad, pi,
                                           C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
    return out.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize('k', [3, 17, 33, 64, 90])
@pytest.mark.parametrize('pdt', [np.float64, np.float32])
def test_variants_give_the_same_bits(k, pdt, limits):
    import torch
    from csr_amd.kernels import hip as K
    from csr_amd._lib import VAL_F32, VAL_F64
    nr, nc, rp, ci, vs = _pattern(_mixed_lens(limits), seed=k, positive=True)
    V = _panel(k, pdt, k)
    base = _pd_base(k, k)
    lam = 0.0625
    code = VAL_F64 if pdt == np.float64 else VAL_F32
    A32, A64 = _csr(nr, nc, rp, ci, vs), _csr(nr, nc, rp, ci, vs, ptr64=True)
    h32, h64 = K.to_handle(A32), K.to_handle(A64)
    try:
        assert K._info(h32.H)[3] == 0 and K._info(h64.H)[3] == 1
        for scale, rhs in ((False, 'values'), (True, 'one_plus_values'), (True, 'ones')):
            rcode = R.RHS.index(rhs)
            for b in (None, base):
                full, finfo = K.als_rows(h32, V, scale, rhs, b, lam)
                assert b is None or not finfo.any()
                # the int64 twin, and a second call
                for hh in (h64, h32):
                    again, ainfo = K.als_rows(hh, V, scale, rhs, b, lam)
                    assert _same(full, again) and np.array_equal(finfo, ainfo)
                # the same rows asked for in ranges: an empty range, single rows, the rest
                for rb, re_ in ((0, 0), (0, 1), (1, 1), (1, 140), (140, 141), (141, 299), (299, 300), (300, 300)):
                    part, pinfo = K.als_rows(h32, V, scale, rhs, b, lam, (rb, re_))
                    assert part.shape == (re_ - rb, k) and pinfo.shape == (re_ - rb,)
                    assert _same(part, full[rb:re_]) and np.array_equal(pinfo, finfo[rb:re_]), (rb, re_)
            # (full, finfo: with base)  the host entry with a strided view (it packs the panel on the way)
            Vw = np.zeros((nc, k + 3), pdt)
            Vw[:, 1:1 + k] = V
            assert _same(full, K.als_rows(h64, Vw[:, 1:1 + k], scale, rhs, base, lam)[0])
            # the device entry, default stream and a side stream; V packed, at column 0 of a panel whose row stride is a
            # multiple of 16 B, and 8 B but not 16 B into a wider panel (element loads); out packed and inside a wider panel
            # whose other columns stay; info wanted and NULL
            dbase = torch.from_numpy(base).cuda()
            wide = (k // 4 + 1) * 4
            off8 = 8 // np.dtype(pdt).itemsize
            for n, (off, ld) in enumerate(((0, k), (0, wide), (off8, k + 3))):
                dV = torch.zeros(nc, ld + (off8 if off else 0), dtype=torch.from_numpy(V).dtype, device='cuda')
                dV[:, off:off + k] = torch.from_numpy(V).cuda()
                pv = dV[:, off:].data_ptr()
                assert pv % 8 == 0 and (pv % 16 != 0) == (off != 0)
                st = torch.cuda.Stream() if n != 1 else None
                pad = (0, 5, 1)[n]
                got, ginfo = _device_call(h32 if n else h64, pv, dV.stride(0), k, code, scale, rcode, 0, nr, dbase, lam, st, pad)
                assert _same(full, got[:, :k]) and np.array_equal(ginfo, finfo) and np.all(got[:, k:] == -7.0), (off, ld)
                got, ginfo = _device_call(h32, pv, dV.stride(0), k, code, scale, rcode, 137, 150, dbase, lam, st, pad, with_info=False)
                assert _same(full[137:150], got[:, :k]) and np.all(ginfo == -7) and np.all(got[:, k:] == -7.0), (off, ld)
    finally:
        K.release_handle(h32)
        K.release_handle(h64)
    # a permutation of the rows: the solutions are permuted
    perm = np.random.default_rng(k).permutation(nr)
    got = A32.pick_rows(perm).als_rows(V, weighted=True, rhs='one_plus_values', base=base, reg_per_entry=lam)
    assert _same(got, A32.als_rows(V, weighted=True, rhs='one_plus_values', base=base, reg_per_entry=lam)[perm])


# ---- 4. accuracy on rows too long for the exact reference ---------------------------------------------------------

def _check_residual(K, lens, k, seed, scale, rhs, pdt=np.float64):
    """
    The systems are formed by float64 NumPy, not by the library, and the computed x must leave a residual within
        k (3 k + 2) 2^-53 (|G|_inf |x|_inf + |b|_inf)
    the textbook backward-error bound of an unpivoted LDL^T solve, plus the accumulation chains' own (len + 2) 2^-52 M
    bound (tests/test_gpu_gram.py) carried through the same way: als_ref.residual_bound states the sum.  Positive
    weights and a positive definite base: every system is positive definite, which is what the bound is about.
    """
    nr, nc, rp, ci, vs = _pattern(lens, seed, positive=True)
    V = _panel(k, pdt, seed)
    base = _pd_base(k, seed)
    lam = 0.01
    h = K.to_handle(_csr(nr, nc, rp, ci, vs))
    try:
        x, info = K.als_rows(h, V, scale, rhs, base, lam)
    finally:
        K.release_handle(h)
    assert not info.any() and np.isfinite(x).all()
    G, M, b, Mb = R.als_numpy(rp, ci, vs, V, scale, rhs, base, lam)
    res, bound = R.residual_bound(G, M, b, Mb, np.diff(rp), x)
    ratio = res / np.maximum(bound, 1e-300)                      # (an empty row: 0 <= 0)
    print('k', k, 'rows', nr, 'largest residual / bound', float(ratio.max()))
    assert np.all(res <= bound), (float(ratio.max()), np.argwhere(res > bound)[:4].tolist())
    # and the solution itself, loosely: these systems are well conditioned
    xs = R.solve_numpy(G, b)[0]
    assert np.allclose(x, xs, rtol=1e-9, atol=1e-11)


def test_one_row_of_5000_entries_at_k_64():
    from csr_amd.kernels import hip as K
    _check_residual(K, [5000], 64, seed=64, scale=True, rhs='one_plus_values')


def test_300_mixed_rows_at_k_33(limits):
    from csr_amd.kernels import hip as K
    _check_residual(K, _mixed_lens(limits), 33, seed=33, scale=True, rhs='values')
    _check_residual(K, _mixed_lens(limits), 33, seed=34, scale=False, rhs='ones', pdt=np.float32)


# ---- 5. special values by position ------------------------------------------------------------------------------

def _als(K, nr, nc, rp, ci, vs, V, scale, rhs='values', base=None, lam=0.0):
    h = K.to_handle(_csr(nr, nc, rp, ci, vs))
    try:
        return K.als_rows(h, V, scale, rhs, base, lam)
    finally:
        K.release_handle(h)


@pytest.mark.parametrize('k', [5, 20, 64])
def test_nan_and_inf_in_one_v_row_touch_only_the_rows_that_hold_it(k, limits):
    from csr_amd.kernels import hip as K
    nr, nc, rp, ci, vs = _pattern(_mixed_lens(limits), seed=50 + k, positive=True)
    V = _panel(k, np.float64, k)
    base = _pd_base(k, k)
    clean, cinfo = _als(K, nr, nc, rp, ci, vs, V, True, 'values', base, 0.125)
    assert not cinfo.any() and np.isfinite(clean).all()
    Vs = V.copy()
    col = int(ci[rp[20]])                                       # a column some rows hold
    Vs[col, 0], Vs[col, 1], Vs[col, k - 1] = np.nan, np.inf, -np.inf
    got, info = _als(K, nr, nc, rp, ci, vs, Vs, True, 'values', base, 0.125)
    holds = np.array([col in ci[rp[r]:rp[r + 1]] for r in range(nr)])
    assert holds.any() and not holds.all()
    assert np.array_equal(_bits(got[~holds]), _bits(clean[~holds])) and not info[~holds].any()
    assert (info[holds] == 1).all()                             # G[0][0] is NaN: the first pivot fails
    assert not np.isfinite(got[holds]).all(axis=1).any()
    # an infinite element alone: d0 stays finite, L10 is infinite, d1 = Inf - Inf * Inf is NaN
    Vs = V.copy()
    Vs[col, 1] = np.inf
    got, info = _als(K, nr, nc, rp, ci, vs, Vs, True, 'values', base, 0.125)
    assert np.array_equal(_bits(got[~holds]), _bits(clean[~holds])) and not info[~holds].any()
    assert (info[holds] == 2).all()


def test_empty_rows_indefinite_base_and_an_infinite_ridge(limits):
    from csr_amd.kernels import hip as K
    k = 6
    nr, nc, rp, ci, vs = _pattern([0, 3, 0, 9, 1], 77, positive=True)
    V = _panel(k, np.float64, 5)
    empty = np.diff(rp) == 0
    # rule A5: with a positive definite base an empty row is +0.0 everywhere, info 0
    x, info = _als(K, nr, nc, rp, ci, vs, V, True, 'values', _pd_base(k, 1), 0.5)
    assert not info.any() and np.array_equal(_bits(x[empty]), _bits(np.zeros((2, k))))
    ex, einfo, _, _ = R.als_exact(rp, ci, vs, V, True, 'values', _pd_base(k, 1), 0.5)
    assert np.array_equal(_bits(x), _bits(ex)) and np.array_equal(info, einfo)
    # without base: the first pivot is +0.0, info 1 and every x NaN; the other rows are as before without the base
    x, info = _als(K, nr, nc, rp, ci, vs, V, True, 'values', None, 0.5)
    assert (info[empty] == 1).all() and np.isnan(x[empty]).all()
    ex, einfo, _, _ = R.als_exact(rp, ci, vs, V, True, 'values', None, 0.5)
    assert _same(x, ex) and np.array_equal(info, einfo) and not info[~empty].any()
    # an indefinite base: diag(1, 1, -50, 1, ...) fails at pivot 2 in the empty rows; the exact restatement names the rest
    bad = np.eye(k)
    bad[2, 2] = -50.0
    x, info = _als(K, nr, nc, rp, ci, vs, V, False, 'ones', bad, 0.0)
    ex, einfo, _, _ = R.als_exact(rp, ci, vs, V, False, 'ones', bad, 0.0)
    assert (info[empty] == 3).all() and np.array_equal(info, einfo) and _same(x, ex)
    # CSR.als_rows raises on a nonzero info unless asked for the codes
    A = _csr(nr, nc, rp, ci, vs)
    with pytest.raises(ValueError, match='row 0, at pivot 2'):
        A.als_rows(V, rhs='ones', base=bad)
    U, codes = A.als_rows(V, rhs='ones', base=bad, return_info=True)
    assert np.array_equal(codes, info) and _same(U, x)
    # lam_n = Inf: n_i > 0 makes every diagonal element +Inf (r = 0, x = 0); n_i = 0 makes it fma(Inf, 0, g) = NaN
    x, info = _als(K, nr, nc, rp, ci, vs, V, True, 'values', _pd_base(k, 1), np.inf)
    assert (info[empty] == 1).all() and np.isnan(x[empty]).all()
    assert not info[~empty].any() and np.all(x[~empty] == 0.0)


# ---- 6. refusals and the cases without entries -----------------------------------------------------------------

def test_every_refusal_leaves_the_outputs_untouched(limits):
    import torch
    from csr_amd.kernels import hip as K
    from csr_amd._lib import lib, ERR_INVALID, ERR_UNSUPPORTED, VAL_F64, VAL_F32
    nr, nc, rp, ci, vs = _pattern([2, 0, 3], 9)
    k = 4
    h = K.to_handle(_csr(nr, nc, rp, ci, vs))
    try:
        V = torch.ones(nc, k, dtype=torch.float64, device='cuda')
        out = torch.full((nr, k), -7.0, dtype=torch.float64, device='cuda')
        info = torch.full((nr,), -7, dtype=torch.int32, device='cuda')
        v, o, ii = V.data_ptr(), out.data_ptr(), info.data_ptr()
        # row_begin, row_end, V, ldv, k, panel_type, scale, rhs_mode, base, lam_n, out, ldo, info
        bad = {
            'k = 0': (0, nr, v, k, 0, VAL_F64, 0, 1, None, 0.0, o, k, ii),
            'k < 0': (0, nr, v, k, -1, VAL_F64, 0, 1, None, 0.0, o, k, ii),
            'ldv < k': (0, nr, v, k - 1, k, VAL_F64, 0, 1, None, 0.0, o, k, ii),
            'ldo < k': (0, nr, v, k, k, VAL_F64, 0, 1, None, 0.0, o, k - 1, ii),
            'panel_type none': (0, nr, v, k, k, 0, 0, 1, None, 0.0, o, k, ii),
            'panel_type 7': (0, nr, v, k, k, 7, 0, 1, None, 0.0, o, k, ii),
            'scale 2': (0, nr, v, k, k, VAL_F64, 2, 1, None, 0.0, o, k, ii),
            'scale -1': (0, nr, v, k, k, VAL_F32, -1, 1, None, 0.0, o, k, ii),
            'rhs_mode 3': (0, nr, v, k, k, VAL_F64, 0, 3, None, 0.0, o, k, ii),
            'rhs_mode -1': (0, nr, v, k, k, VAL_F64, 0, -1, None, 0.0, o, k, ii),
            'row_begin < 0': (-1, nr, v, k, k, VAL_F64, 0, 1, None, 0.0, o, k, ii),
            'row_end > nrows': (0, nr + 1, v, k, k, VAL_F64, 0, 1, None, 0.0, o, k, ii),
            'row_begin > row_end': (2, 1, v, k, k, VAL_F64, 0, 1, None, 0.0, o, k, ii),
            'NULL V': (0, nr, None, k, k, VAL_F64, 0, 1, None, 0.0, o, k, ii),
            'NULL out': (0, nr, v, k, k, VAL_F64, 0, 1, None, 0.0, None, k, ii),
        }
        for name, args in bad.items():
            assert lib.csrk_als_rows_device(h.H, *args, None) == ERR_INVALID, name
            assert lib.csrk_last_error(), name
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((info == -7).all())
        # the host entry refuses the same way
        Vh, oh, ih = np.ones((nc, k)), np.full((nr, k), -7.0), np.full(nr, -7, np.int32)
        for name, args in bad.items():
            a = list(args)
            a[2] = None if args[2] is None else Vh.ctypes.data
            a[10] = None if args[10] is None else oh.ctypes.data
            a[12] = ih.ctypes.data
            assert lib.csrk_als_rows(h.H, *a) == ERR_INVALID, name
        assert np.all(oh == -7.0) and np.all(ih == -7)
        # k above the limit is unsupported, on both entries
        kk = int(limits[0]) + 1
        Vb = torch.ones(nc, kk, dtype=torch.float64, device='cuda')
        ob = torch.full((nr, kk), -7.0, dtype=torch.float64, device='cuda')
        assert lib.csrk_als_rows_device(h.H, 0, nr, Vb.data_ptr(), kk, kk, VAL_F64, 0, 1, None, 0.0, ob.data_ptr(), kk, ii,
                                        None) == ERR_UNSUPPORTED
        Vbh, obh = np.ones((nc, kk)), np.full((nr, kk), -7.0)
        assert lib.csrk_als_rows(h.H, 0, nr, Vbh.ctypes.data, kk, kk, VAL_F64, 0, 1, None, 0.0, obh.ctypes.data, kk,
                                 ih.ctypes.data) == ERR_UNSUPPORTED
        Gb, bb, xb = torch.ones(1, kk, kk, dtype=torch.float64, device='cuda'), torch.ones(1, kk, dtype=torch.float64, device='cuda'), ob
        assert lib.csrk_solve_blocks_device(1, kk, Gb.data_ptr(), bb.data_ptr(), kk, xb.data_ptr(), kk, ii, None) == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((ob == -7.0).all()) and bool((info == -7).all()) and np.all(obh == -7.0) and np.all(ih == -7)
        # an empty range is fine and writes nothing, NULL pointers and all
        assert lib.csrk_als_rows_device(h.H, 1, 1, None, k, k, VAL_F64, 0, 1, None, 0.0, None, k, None, None) == 0
        assert lib.csrk_als_rows(h.H, 3, 3, None, k, k, VAL_F64, 0, 1, None, 0.0, None, k, None) == 0
        # the handle still computes
        U, codes = K.als_rows(h, np.ones((nc, k)), False, 'values', np.eye(k))
        assert np.array_equal(U[1], np.zeros(k)) and not codes.any()
    finally:
        K.release_handle(h)


def test_no_rows_and_no_entries():
    from csr_amd.kernels import hip as K
    k = 5
    V = _panel(k, np.float64, 1)
    base = _pd_base(k, 1)
    # nrows = 0: nothing to write
    x, info = _als(K, 0, NCOLS, np.zeros(1, np.int64), np.zeros(0, np.int32), None, V, False, 'values', base)
    assert x.shape == (0, k) and info.shape == (0,)
    x, info = K.solve_blocks(np.zeros((0, k, k)), np.zeros((0, k)))
    assert x.shape == (0, k) and info.shape == (0,)
    # nnz = 0: every row is empty -- base x = 0, or (no base) the all-zero system
    rp = np.zeros(4, np.int64)
    for vs in (None, np.zeros(0)):
        for rhs in R.RHS:
            x, info = _als(K, 3, NCOLS, rp, np.zeros(0, np.int32), vs, V, True, rhs, base, 0.25)
            assert np.array_equal(_bits(x), _bits(np.zeros((3, k)))) and not info.any()
            x, info = _als(K, 3, NCOLS, rp, np.zeros(0, np.int32), vs, V, True, rhs, None, 0.25)
            assert np.isnan(x).all() and (info == 1).all()
