"""
csrk_als_objective_rows and csrk_als_objective on the card (include/csrk.h, rules J and T): the rows bit for bit against the
exact restatement of rule J1 (tests/als_fit_ref.py) on csrk_als_rows_cg's kind of pattern -- unsorted, a repeated column,
empty rows at both ends, row lengths at the entry loop's edges -- with every option, at DOT's k edges, for both pointer
widths; the total bit for bit against rule J2 with and without the all-pairs term, with one, three and more than 32 chunks in
rule T's tree; the device forms on a side stream; refusals with the outputs untouched.
"""
import ctypes as C

import numpy as np
import pytest

import als_fit_ref as R

pytestmark = pytest.mark.gpu

RHS = ('ones', 'values', 'one_plus_values')
NCOLS = 50


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
def limits(K):
    return K.als_objective_limits()


def _csr(nr, nc, rp, ci, vs, ptr64=False):
    from csr_amd import CSR
    return CSR(nr, nc, int(rp[-1]), np.asarray(rp).astype(np.int64 if ptr64 else np.int32), np.asarray(ci, np.int32).copy(),
               None if vs is None else vs.copy(), _cast=False)


def _pattern(lens, seed, ncols=NCOLS, values=True):
    "rows of the given lengths: unsorted, a column repeated in every row of three or more entries; values in (0.1, 1.1)"
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    rp = np.zeros(len(lens) + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    ci = rng.integers(0, ncols, int(rp[-1])).astype(np.int32)
    for r in range(len(lens)):
        if lens[r] >= 3:
            ci[rp[r] + 2] = ci[rp[r]]
    vs = (rng.random(int(rp[-1])) + 0.1) if values else None
    return rp, ci, vs


def _factors(nrows, ncols, k, seed):
    rng = np.random.default_rng(100 + seed)
    return rng.standard_normal((nrows, k)) * 0.7, rng.standard_normal((ncols, k)) * 0.7


def _edge_lens(limits):
    E = int(limits[3])
    return [0, 0, 1, 2, E - 1, E, E + 1, 2 * E + 1, 0]


# ---- rows ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [1, 16, 17, 33, 64])
def test_rows_at_every_k_edge(K, limits, k):
    lens = _edge_lens(limits)
    rp, ci, vs = _pattern(lens, k)
    U, V = _factors(len(lens), NCOLS, k, k)
    with_h = K.to_handle(_csr(len(lens), NCOLS, rp, ci, vs))
    try:
        got = K.als_objective_rows(with_h, U, V, scale=True, rhs='one_plus_values', lam=0.25, lam_n=0.125)
    finally:
        K.release_handle(with_h)
    assert _same(got, R.objective_rows_exact(rp, ci, vs, U, V, True, 'one_plus_values', 0.25, 0.125))


@pytest.mark.parametrize('values', [True, False], ids=['values', 'structure'])
@pytest.mark.parametrize('scale', [False, True])
@pytest.mark.parametrize('rhs', RHS)
def test_rows_with_every_option(K, limits, rhs, scale, values):
    "every (rhs, scale) on a matrix with and without values; data = 0; a row range; int64 row pointers; a strided V"
    lens, k = _edge_lens(limits), 17
    rp, ci, vs = _pattern(lens, 9, values=values)
    U, V = _factors(len(lens), NCOLS, k, 9)
    want = R.objective_rows_exact(rp, ci, vs, U, V, scale, rhs, 0.5, 0.0625)
    reg = R.objective_rows_exact(rp, None, None, U, None, scale, rhs, 0.5, 0.0625, data=False)
    wide = np.zeros((NCOLS, k + 3))
    wide[:, 1:1 + k] = V
    for ptr64 in (False, True):
        h = K.to_handle(_csr(len(lens), NCOLS, rp, ci, vs, ptr64))
        try:
            assert _same(K.als_objective_rows(h, U, V, scale, rhs, 0.5, 0.0625), want)
            assert _same(K.als_objective_rows(h, U, wide[:, 1:1 + k], scale, rhs, 0.5, 0.0625), want)
            assert _same(K.als_objective_rows(h, U, V, scale, rhs, 0.5, 0.0625, rows=(3, 8)), want[3:8])
            assert _same(K.als_objective_rows(h, U, V, scale, rhs, 0.5, 0.0625, data=False), reg)
            assert len(K.als_objective_rows(h, U, V, scale, rhs, rows=(4, 4))) == 0
        finally:
            K.release_handle(h)
    assert not _same(want, reg)


def test_rows_nan_by_position(K, limits):
    lens, k = [3, 2, 0, 4], 5
    rp, ci, vs = _pattern(lens, 21)
    U, V = _factors(4, NCOLS, k, 21)
    V[ci[rp[1]], 2] = np.nan                                     # a V row that row 1 names (others may too)
    want = R.objective_rows_exact(rp, ci, vs, U, V, False, 'values', 0.1, 0.0)
    h = K.to_handle(_csr(4, NCOLS, rp, ci, vs))
    try:
        got = K.als_objective_rows(h, U, V, lam=0.1)
    finally:
        K.release_handle(h)
    assert np.isnan(want[1]) and np.isfinite(want[2]) and _same(got, want)


# ---- the total ------------------------------------------------------------------------------------------------------

def _matrix(nrows, ncols, nnz, seed):
    "a random pattern without repeated pairs, in row order with unsorted columns; (rp, ci, vs, row pointers of the transpose)"
    rng = np.random.default_rng(seed)
    flat = rng.choice(nrows * ncols, size=nnz, replace=False)
    rows, cols = flat // ncols, flat % ncols
    o = np.argsort(rows, kind='stable')
    rows, cols = rows[o], cols[o].astype(np.int32)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nrows))])
    atrp = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=ncols))])
    return rp, cols, rng.random(nnz) + 0.1, atrp


def _handles(K, nrows, ncols, rp, ci, vs):
    h = K.to_handle(_csr(nrows, ncols, rp, ci, vs))
    return h, K.transpose(h, True)


CASES = {'40x30': (40, 30, 150, 5), '700x30': (700, 30, 900, 3), '8500x20': (8500, 20, 2500, 2)}


@pytest.mark.parametrize('implicit', [False, True], ids=['explicit', 'implicit'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_total_bit_for_bit(K, limits, case, implicit):
    "40 rows: one chunk of rule T; 700: three (an odd count); 8500: more than 32, so the tree takes two launches"
    nrows, ncols, nnz, k = CASES[case]
    rp, ci, vs, atrp = _matrix(nrows, ncols, nnz, 3)
    U, V = _factors(nrows, ncols, k, 3)
    scale, rhs = (True, 'one_plus_values') if implicit else (False, 'values')
    Rr, L = int(K.panel_gram_limits()[1]), int(limits[1])
    assert (nrows + L - 1) // L > 32 or case != '8500x20'
    h, th = _handles(K, nrows, ncols, rp, ci, vs)
    try:
        got = K.als_objective(h, th, U, V, scale, rhs, implicit, 0.3, 0.05)
        again = K.als_objective(h, th, U, V, scale, rhs, implicit, 0.3, 0.05)
    finally:
        K.release_handle(th)
        K.release_handle(h)
    want = R.objective_exact((rp, ci, vs), atrp, U, V, scale, rhs, implicit, 0.3, 0.05, Rr, L)
    assert _same([got], [want]) and _same([got], [again])


def test_csr_method_and_the_plain_loss(K):
    "CSR.als_objective is the kernel entry on the CSR's own transpose, and the plain NumPy loss minus its constant"
    rp, ci, vs, atrp = _matrix(40, 30, 150, 4)
    U, V = _factors(40, 30, 4, 4)
    a = _csr(40, 30, rp, ci, vs)
    for config, kw in (('explicit', dict(weighted=False, rhs='values', implicit=False)),
                       ('implicit', dict(weighted=True, rhs='one_plus_values', implicit=True))):
        J = a.als_objective(U, V, reg=0.3, reg_per_entry=0.05, **kw)
        h, th = _handles(K, 40, 30, rp, ci, vs)
        try:
            assert _same([J], [K.als_objective(h, th, U, V, kw['weighted'], kw['rhs'], kw['implicit'], 0.3, 0.05)])
        finally:
            K.release_handle(th)
            K.release_handle(h)
        loss, const, mag, adds = R.loss_numpy(rp, ci, vs, U, V, config, 0.3, 0.05)
        assert abs(J - (loss - const)) <= adds * 2.0 ** -52 * (mag + const)


def test_device_form_on_a_side_stream(K):
    "the exact workspace size, a side stream, strided panels: the host form's bits"
    import torch
    from csr_amd._lib import lib
    nrows, ncols, nnz, k = CASES['700x30']
    rp, ci, vs, _ = _matrix(nrows, ncols, nnz, 5)
    U, V = _factors(nrows, ncols, k, 5)
    h, th = _handles(K, nrows, ncols, rp, ci, vs)
    try:
        want = K.als_objective(h, th, U, V, True, 'one_plus_values', True, 0.3, 0.05)
        need = C.c_int64(0)
        assert lib.csrk_als_objective_workspace(nrows, ncols, k, 1, C.byref(need)) == 0
        dU, dV = torch.zeros((nrows, k + 1), dtype=torch.float64, device='cuda'), torch.from_numpy(V).cuda()
        dU[:, :k] = torch.from_numpy(U).cuda()
        dW = torch.empty(need.value, dtype=torch.uint8, device='cuda')
        dJ = torch.full((2,), -7.0, dtype=torch.float64, device='cuda')
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        args = (h.H, th.H, dU.data_ptr(), k + 1, dV.data_ptr(), k, k, 1, 2, 1, 0.3, 0.05, dJ.data_ptr(), dW.data_ptr())
        assert lib.csrk_als_objective_device(*args, need.value - 1, s.cuda_stream) != 0
        torch.cuda.synchronize()
        assert dJ.cpu().numpy()[0] == -7.0                      # one byte short: refused, untouched
        assert lib.csrk_als_objective_device(*args, need.value, s.cuda_stream) == 0
        torch.cuda.synchronize()
        got = dJ.cpu().numpy()
        assert _same([got[0]], [want]) and got[1] == -7.0
    finally:
        K.release_handle(th)
        K.release_handle(h)


# ---- refusals -------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(K):
    from csr_amd import _lib
    lib = _lib.lib
    rp, ci, vs, _ = _matrix(40, 30, 150, 6)
    U, V = _factors(40, 30, 4, 6)
    h, th = _handles(K, 40, 30, rp, ci, vs)
    try:
        with pytest.raises(ValueError):
            K.als_objective(h, h, U, V)                               # not the transpose's shape
        with pytest.raises(ValueError):
            K.als_objective(h, th, U.astype(np.float32), V.astype(np.float32))
        with pytest.raises(ValueError):
            K.als_objective_rows(h, U.astype(np.float32), V.astype(np.float32))
        out = np.full(40, -7.0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        assert lib.csrk_als_objective(h.H, h.H, p(U), 4, p(V), 4, 4, 0, 1, 0, 0.0, 0.0, p(out)) == _lib.ERR_INVALID
        assert 'transpose' in _lib.last_error()
        for args in ((h.H, 0, 40, p(U), 3, p(V), 4, 4, 0, 1, 1, 0.0, 0.0, p(out)), (h.H, 0, 41, p(U), 4, p(V), 4, 4, 0, 1, 1, 0.0, 0.0, p(out)),
                     (h.H, 0, 40, p(U), 4, p(V), 4, 4, 2, 1, 1, 0.0, 0.0, p(out)), (h.H, 0, 40, p(U), 4, p(V), 4, 4, 0, 3, 1, 0.0, 0.0, p(out)),
                     (h.H, 0, 40, p(U), 4, p(V), 4, 4, 0, 1, 2, 0.0, 0.0, p(out)), (h.H, 0, 40, p(U), 4, None, 4, 4, 0, 1, 1, 0.0, 0.0, p(out)),
                     (h.H, 0, 40, p(U), 4, p(V), 4, 0, 0, 1, 1, 0.0, 0.0, p(out))):
            assert lib.csrk_als_objective_rows(*args) == _lib.ERR_INVALID, args
        assert lib.csrk_als_objective_rows(h.H, 0, 40, p(U), 200, p(V), 200, 129, 0, 1, 1, 0.0, 0.0, p(out)) == _lib.ERR_UNSUPPORTED
        assert np.all(out == -7.0)
    finally:
        K.release_handle(th)
        K.release_handle(h)
