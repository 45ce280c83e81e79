"""
csrk_als_fit on the card (include/csrk.h, rule F): U, V and bad bit for bit against the caller's own loop over the public
host entries panel_gram, als_rows / als_rows_cg and als_objective (tests/als_fit_ref.py, fit_by_parts) for both solvers,
explicit and implicit, at three k and 0, 1 and 3 sweeps, on a matrix with an empty row and an empty column; the objective
after every sweep; the CSR method, the handle form and the device form on a side stream against one another; the long-row
class on and off; descent of the exact solver; bad pivots counted and raised; refusals with U and V untouched.
"""
import ctypes as C

import numpy as np
import pytest

import als_fit_ref as R

pytestmark = pytest.mark.gpu

NROWS, NCOLS = 60, 45
EXPLICIT = dict(scale=False, rhs='values', implicit=False, lam=0.1, lam_n=0.05)
IMPLICIT = dict(scale=True, rhs='one_plus_values', implicit=True, lam=0.1, lam_n=0.0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


@pytest.fixture(scope='module')
def K():
    from csr_amd.kernels import hip
    return hip


@pytest.fixture(scope='module')
def matrix():
    "60 x 45, about 400 entries without repeated pairs, columns unsorted; row 7 and column 11 are empty"
    from csr_amd import CSR
    rng = np.random.default_rng(17)
    flat = rng.choice(NROWS * NCOLS, size=420, replace=False)
    rows, cols = flat // NCOLS, flat % NCOLS
    keep = (rows != 7) & (cols != 11)
    rows, cols = rows[keep], cols[keep]
    o = np.argsort(rows, kind='stable')
    rows, cols = rows[o], cols[o].astype(np.int32)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=NROWS))]).astype(np.int32)
    vs = rng.random(len(cols)) + 0.1
    return CSR(NROWS, NCOLS, len(cols), rp, cols, vs, _cast=False)


@pytest.fixture(scope='module')
def handles(K, matrix):
    h = K.to_handle(matrix)
    th = K.transpose(h, True)
    yield h, th
    K.release_handle(th)
    K.release_handle(h)


def _start(k, seed=0):
    rng = np.random.default_rng(200 + seed)
    return rng.standard_normal((NROWS, k)) * 0.3, rng.standard_normal((NCOLS, k)) * 0.3


def _fit_equals_parts(K, handles, k, sweeps, solver, cfg, steps=3):
    h, th = handles
    U0, V0 = _start(k)
    U0c, V0c = U0.copy(), V0.copy()
    U, V, obj, bad = K.als_fit(h, th, U0, V0, sweeps, solver, steps, cfg['scale'], cfg['rhs'], cfg['implicit'], cfg['lam'], cfg['lam_n'], 0.0,
                               True)
    pU, pV, pobj, pbad = R.fit_by_parts(K, h, th, U0, V0, sweeps, solver, steps, cfg['scale'], cfg['rhs'], cfg['implicit'], cfg['lam'],
                                        cfg['lam_n'], 0.0, True)
    assert np.array_equal(U0, U0c) and np.array_equal(V0, V0c)                     # the start factors are the caller's
    assert _same(U, pU) and _same(V, pV)
    assert bad.dtype == np.int64 and list(bad) == pbad and len(bad) == 2 * sweeps
    assert len(obj) == sweeps + 1 and _same(obj, pobj)
    if sweeps == 0:
        assert _same(U, U0) and _same(V, V0)
    else:
        assert not _same(U, U0) and not _same(V, V0)
    return U, V, obj, bad


@pytest.mark.parametrize('sweeps', [0, 1, 3])
@pytest.mark.parametrize('k', [3, 16, 33])
@pytest.mark.parametrize('cfg', [EXPLICIT, IMPLICIT], ids=['explicit', 'implicit'])
@pytest.mark.parametrize('solver', ['exact', 'cg'])
def test_fit_is_the_loop_over_its_parts(K, handles, solver, cfg, k, sweeps):
    U, V, obj, bad = _fit_equals_parts(K, handles, k, sweeps, solver, cfg)
    assert not bad.any() and np.all(np.isfinite(U)) and np.all(np.isfinite(V))


def test_lower_level_forms_agree(K, matrix, handles):
    "CSR.als_fit = hip.als_fit on handles = the device form on a side stream with the exact workspace and strided panels"
    import torch
    from csr_amd._lib import lib
    h, th = handles
    k, sweeps = 16, 2
    U0, V0 = _start(k, 1)
    cfg = IMPLICIT
    U, V, obj, bad = K.als_fit(h, th, U0, V0, sweeps, 'cg', 3, True, 'one_plus_values', True, cfg['lam'], 0.0, 0.0, True)
    cU, cV, cobj, cbad = matrix.als_fit(U0, V0, sweeps=sweeps, solver='cg', steps=3, weighted=True, rhs='one_plus_values', implicit=True,
                                        reg=cfg['lam'], return_objective=True, return_info=True)
    assert _same(cU, U) and _same(cV, V) and _same(cobj, obj) and np.array_equal(cbad, bad)
    two = matrix.als_fit(U0, V0, sweeps=sweeps, weighted=True, rhs='one_plus_values', implicit=True, reg=cfg['lam'])
    assert len(two) == 2 and _same(two[0], U) and _same(two[1], V)

    need = C.c_int64(0)
    assert lib.csrk_als_fit_workspace(NROWS, NCOLS, k, 1, 1, 1, C.byref(need)) == 0
    dU = torch.zeros((NROWS, k + 2), dtype=torch.float64, device='cuda')
    dU[:, :k] = torch.from_numpy(U0).cuda()
    dV = torch.from_numpy(V0).cuda()
    dW = torch.empty(need.value, dtype=torch.uint8, device='cuda')
    dJ = torch.full((sweeps + 1,), -7.0, dtype=torch.float64, device='cuda')
    dB = torch.full((2 * sweeps,), -7, dtype=torch.int64, device='cuda')
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    args = (h.H, th.H, k, sweeps, 1, 3, 0.0, 1, 2, 1, cfg['lam'], 0.0, dU.data_ptr(), k + 2, dV.data_ptr(), k, dJ.data_ptr(), dB.data_ptr(),
            dW.data_ptr())
    assert lib.csrk_als_fit_device(*args, need.value - 1, s.cuda_stream) != 0          # one byte short: refused
    torch.cuda.synchronize()
    assert _same(dU[:, :k].cpu().numpy(), U0) and dJ.cpu().numpy()[0] == -7.0
    assert lib.csrk_als_fit_device(*args, need.value, s.cuda_stream) == 0
    torch.cuda.synchronize()
    assert _same(dU[:, :k].cpu().numpy(), U) and _same(dV.cpu().numpy(), V) and _same(dJ.cpu().numpy(), obj)
    assert np.array_equal(dB.cpu().numpy(), bad) and np.all(dU[:, k:].cpu().numpy() == 0.0)


def test_long_row_class_changes_no_bit(K, handles):
    h, th = handles
    U0, V0 = _start(16, 2)
    out = []
    try:
        for L in (1, 0):
            K.als_cg_set_long(L)
            out.append(K.als_fit(h, th, U0, V0, 2, 'cg', 3, True, 'one_plus_values', True, 0.1, 0.0, 0.0, True))
    finally:
        K.als_cg_set_long(None)
    assert _same(out[0][0], out[1][0]) and _same(out[0][1], out[1][1]) and _same(out[0][2], out[1][2])


def test_exact_sweeps_descend(K, matrix, handles):
    "solver exact, explicit, reg 0.1: the objective does not increase from sweep to sweep, under the host test's bound"
    h, th = handles
    U, V = _start(8, 3)
    rp, ci, vs = matrix.rowptrs, matrix.colinds, matrix.values
    objs, mags = [], []
    for _ in range(4):
        loss, const, mag, adds = R.loss_numpy(rp, ci, vs, U, V, 'explicit', 0.1, 0.0)
        mags.append(mag)
        U, V, obj, bad = K.als_fit(h, th, U, V, 1, 'exact', 3, False, 'values', False, 0.1, 0.0, 0.0, True)
        objs.append(obj)
        assert not bad.any()
    mags.append(R.loss_numpy(rp, ci, vs, U, V, 'explicit', 0.1, 0.0)[2])
    for s in range(4):
        mag = max(mags[s], mags[s + 1])
        assert objs[s][1] <= objs[s][0] + adds * 2.0 ** -52 * (mag + const)
        if s:
            assert _same([objs[s][0]], [objs[s - 1][1]])
    assert objs[0][1] < objs[0][0] and objs[3][1] < objs[0][1]


def test_bad_pivots_are_counted_and_raised(K, matrix, handles):
    """
    exact, reg 0, not implicit: the empty row's system is 0 x = 0 (rule A5): one bad row in half-step 0, the empty column in 1.
    (k = 1: without a ridge a row of fewer than k entries is singular too, and this matrix has rows of one entry.)
    """
    h, th = handles
    U0, V0 = _start(1, 4)
    U, V, obj, bad = K.als_fit(h, th, U0, V0, 1, 'exact', 3, False, 'values', False, 0.0, 0.0, 0.0, False)
    assert list(bad) == [1, 1] and obj is None
    assert np.all(np.isnan(U[7])) and np.all(np.isnan(V[11])) and np.isfinite(np.delete(U, 7, 0)).all()
    pU, pV, _, pbad = R.fit_by_parts(K, h, th, U0, V0, 1, 'exact', 3, False, 'values', False, 0.0, 0.0, 0.0, False)
    assert _same(U, pU) and _same(V, pV) and pbad == [1, 1]
    with pytest.raises(ValueError, match='half-step 0'):
        matrix.als_fit(U0, V0, sweeps=1, solver='exact')
    rU, rV, rbad = matrix.als_fit(U0, V0, sweeps=1, solver='exact', return_info=True)
    assert _same(rU, U) and _same(rV, V) and list(rbad) == [1, 1]


def test_refused_fits_leave_the_factors_untouched(K, handles):
    from csr_amd import _lib
    lib = _lib.lib
    h, th = handles
    k = 4
    U0, V0 = _start(k, 5)
    U, V = U0.copy(), V0.copy()
    obj, bad = np.full(3, -7.0), np.full(4, -7, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def call(hA=h.H, hAt=th.H, k=k, sweeps=2, solver=1, steps=3, tol2=0.0, scale=0, rhs=1, implicit=0, ldu=k, ldv=k, Up=p(U), Vp=p(V)):
        return lib.csrk_als_fit(hA, hAt, k, sweeps, solver, steps, tol2, scale, rhs, implicit, 0.1, 0.0, Up, ldu, Vp, ldv, p(obj), p(bad))

    for kw in (dict(sweeps=-1), dict(solver=2), dict(solver=-1), dict(hAt=h.H), dict(k=0), dict(ldu=k - 1), dict(ldv=k - 1), dict(steps=-1),
               dict(tol2=-1.0), dict(tol2=float('nan')), dict(scale=2), dict(rhs=3), dict(implicit=2), dict(Vp=p(U)), dict(Up=None)):
        assert call(**kw) == _lib.ERR_INVALID, kw
    assert call(k=129, ldu=200, ldv=200) == _lib.ERR_UNSUPPORTED
    assert _same(U, U0) and _same(V, V0) and np.all(obj == -7.0) and np.all(bad == -7)
    assert call() == 0 and not _same(U, U0) and obj[0] != -7.0 and list(bad) == [0, 0, 0, 0]
