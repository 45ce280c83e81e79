"""
panel_gram, als_objective and als_fit without a device (CPU suite): every argument refusal is raised before the library is
touched (on a box without a GPU a library call would raise CsrkError instead), the limits answer without a device, and the
references of tests/als_fit_ref.py are checked against hand-written trees, against the plain NumPy losses with their
documented constants, and against each other (fused against two roundings) -- which guards the formulas of rules P, J and T
before any kernel runs.
"""
import types

import numpy as np
import pytest

import als_fit_ref as R


@pytest.fixture(scope='module')
def K():
    from csr_amd.kernels import hip
    return hip


def _shape(nrows, ncols, nnz):
    "what the *_args functions look at in a handle or a CSR"
    return types.SimpleNamespace(nrows=nrows, ncols=ncols, nnz=nnz, H=0)


# ---- argument refusals ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('V,ridge', [(np.ones(3), 0.0), (np.ones((2, 2, 2)), 0.0), (np.ones((3, 2), np.int32), 0.0),
                                     (np.ones((3, 2), np.float16), 0.0), (np.ones((3, 0)), 0.0), (np.ones((3, 2)), float('nan')),
                                     (np.ones((3, 2)), 'x'), (np.ones((3, 2)), None), (np.ones((3, 2)), True), (np.ones((3, 2)), 1j)])
def test_panel_gram_refusals(K, V, ridge):
    with pytest.raises(ValueError):
        K.panel_gram(V, ridge)


def _objective_refusals():
    a, at = _shape(4, 3, 5), _shape(3, 4, 5)
    U, V = np.ones((4, 2)), np.ones((3, 2))
    return [
        (a, at, U.astype(np.float32), V.astype(np.float32), {}),          # float32 panels
        (a, at, U, V.astype(np.float32), {}),
        (a, at, U[:3], V, {}), (a, at, U, V[:2], {}), (a, at, U, np.ones((3, 3)), {}), (a, at, U[:, :0], V[:, :0], {}),
        (a, at, U[0], V, {}),
        (a, _shape(4, 3, 5), U, V, {}), (a, _shape(3, 4, 6), U, V, {}), (a, _shape(3, 5, 5), U, V, {}),      # not the transpose's shape
        (a, at, U, V, {'rhs': 'value'}), (a, at, U, V, {'rhs': 1}), (a, at, U, V, {'lam': 'x'}), (a, at, U, V, {'lam_n': None}),
    ]


@pytest.mark.parametrize('case', range(len(_objective_refusals())))
def test_als_objective_refusals(K, case):
    a, at, U, V, kw = _objective_refusals()[case]
    with pytest.raises(ValueError):
        K.als_objective(a, at, U, V, **kw)
    with pytest.raises(ValueError):
        K.als_fit_args(a, at, U, V, **kw)


@pytest.mark.parametrize('kw', [{'sweeps': -1}, {'sweeps': 1.5}, {'sweeps': True}, {'solver': 'lu'}, {'solver': 0}, {'steps': -1},
                                {'steps': 2.0}, {'tol': -1.0}, {'tol': float('nan')}, {'tol': 'x'}, {'rhs': 'one'}, {'lam': 1j}])
def test_als_fit_args_refusals(K, kw):
    a, at = _shape(4, 3, 5), _shape(3, 4, 5)
    with pytest.raises(ValueError):
        K.als_fit_args(a, at, np.ones((4, 2)), np.ones((3, 2)), **kw)
    with pytest.raises(ValueError):
        K.als_fit(a, at, np.ones((4, 2)), np.ones((3, 2)), **kw)


def test_als_fit_args_accepts_and_copies(K):
    a, at = _shape(4, 3, 5), _shape(3, 4, 5)
    U0, V0 = np.arange(8.0).reshape(4, 2), np.arange(12.0).reshape(3, 4)[:, 1:3]
    U, V, k, sweeps, scode, steps, tol2, rcode, lam, lam_n = K.als_fit_args(a, at, U0, V0, 2, 'exact', 5, 'ones', 0.5, 0.25, 3.0)
    assert (k, sweeps, scode, steps, tol2, rcode, lam, lam_n) == (2, 2, 0, 5, 9.0, 0, 0.5, 0.25)
    assert U is not U0 and np.array_equal(U, U0) and V.flags.c_contiguous and np.array_equal(V, V0)


def test_csr_methods_refuse_before_the_library():
    from csr_amd import CSR
    a = CSR.from_coo(np.array([0, 1]), np.array([1, 0]), np.array([1.0, 2.0]))
    with pytest.raises(ValueError):
        a.als_fit(np.ones((2, 2)), np.ones((2, 2)), solver='qr')
    with pytest.raises(ValueError):
        a.als_fit(np.ones((2, 2), np.float32), np.ones((2, 2), np.float32))
    with pytest.raises(ValueError):
        a.als_objective(np.ones((3, 2)), np.ones((2, 2)))


# ---- limits -------------------------------------------------------------------------------------------------------

def test_limits_answer_without_a_device(K):
    kmax, Rr = K.panel_gram_limits()
    assert kmax >= 128 and Rr >= 1
    lim = K.als_objective_limits()
    assert lim[0] >= 128 and lim[1] >= 1 and lim[2] == 16 and lim[3] >= 1


def test_workspace_sizes_answer_without_a_device(K):
    import ctypes as C
    from csr_amd import _lib
    lib, b = _lib.lib, C.c_int64(-1)
    Rr = int(K.panel_gram_limits()[1])
    assert lib.csrk_panel_gram_workspace(0, 4, C.byref(b)) == 0 and b.value == 0
    assert lib.csrk_panel_gram_workspace(Rr + 1, 4, C.byref(b)) == 0 and b.value == 2 * 16 * 8
    assert lib.csrk_panel_gram_workspace(33 * Rr, 4, C.byref(b)) == 0 and b.value == (33 + 2) * 16 * 8
    assert lib.csrk_panel_gram_workspace(5, 129, C.byref(b)) == _lib.ERR_UNSUPPORTED
    assert lib.csrk_panel_gram_workspace(-1, 4, C.byref(b)) == _lib.ERR_INVALID
    small, big = C.c_int64(0), C.c_int64(0)
    assert lib.csrk_als_objective_workspace(10, 7, 4, 0, C.byref(small)) == 0 and lib.csrk_als_objective_workspace(10, 7, 4, 1, C.byref(big)) == 0
    assert 0 < small.value < big.value
    for solver in (0, 1):
        assert lib.csrk_als_fit_workspace(10, 7, 4, solver, 1, 1, C.byref(b)) == 0 and b.value >= big.value and b.value % 16 == 0
    assert lib.csrk_als_fit_workspace(10, 7, 4, 2, 1, 1, C.byref(b)) == _lib.ERR_INVALID


# ---- the tree -------------------------------------------------------------------------------------------------------

def test_tree_sum_against_hand_written_trees():
    "values whose sum depends on the parenthesisation"
    p = [1e16, 1.0, -1e16, 1.0, 3.0, 1e-3, 2.0 ** 53, 1.0]
    assert R.tree_sum([]) == 0.0 and not np.signbit(R.tree_sum([]))
    assert R.tree_sum(p[:1]) == p[0]
    assert R.tree_sum([-0.0]) == 0.0 and np.signbit(R.tree_sum([-0.0]))          # carried unchanged, no + 0.0
    assert R.tree_sum(p[:2]) == p[0] + p[1]
    assert R.tree_sum(p[:3]) == (p[0] + p[1]) + p[2]
    assert R.tree_sum(p[:5]) == ((p[0] + p[1]) + (p[2] + p[3])) + p[4]
    assert R.tree_sum(p[:8]) == ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))
    assert R.tree_sum(p[:3]) != p[0] + (p[1] + p[2]) or R.tree_sum(p[:5]) != sum(p[:5])      # ... and the order shows
    a = [np.array([x, -x]) for x in p[:5]]
    assert np.array_equal(R.tree_sum(a), [R.tree_sum(p[:5]), -R.tree_sum(p[:5])])


def test_chunk_sum_is_serial_inside_a_chunk_and_a_tree_across():
    x = [1e16, 1.0, 1.0, -1e16, 1.0]
    assert R.chunk_sum(x, 2) == ((1e16 + 1.0) + (1.0 + -1e16)) + 1.0
    assert R.chunk_sum(x, 8) == (((1e16 + 1.0) + 1.0) + -1e16) + 1.0
    assert R.chunk_sum([], 4) == 0.0


# ---- rounding mode ------------------------------------------------------------------------------------------------

def test_the_references_tell_fused_from_two_roundings():
    "S[1][0] = fma(x, x, -1) with x = 1 + 2^-30: exactly 2^-29 + 2^-60 fused, 2^-29 when the product is rounded first"
    x = 1.0 + 2.0 ** -30
    V = np.array([[1.0, -1.0], [x, x]])
    assert R.panel_gram_exact(V, 0.0, 8)[1, 0] == 2.0 ** -29 + 2.0 ** -60
    assert R.panel_gram_two_rounding(V, 0.0, 8)[1, 0] == 2.0 ** -29
    # J = fma(h, s, 0) then fma(rho, |u|^2, J): u = (x), v = (x), a = 1: s = round(x^2), h = s - 2, J1 = round(h s);
    # rho = 1, |u|^2 = s: fused round(s + J1) from the exact product rho s, two roundings the same here; so take rho = x
    rp, ci, vs = np.array([0, 1]), np.array([0]), np.array([1.0])
    f = R.objective_rows_exact(rp, ci, vs, [[x]], [[x]], lam=x, fused=True)
    t = R.objective_rows_exact(rp, ci, vs, [[x]], [[x]], lam=x, fused=False)
    assert f[0] != t[0]


# ---- the objective against the plain losses ---------------------------------------------------------------------------

def _small(seed=5, nrows=12, ncols=9, k=3):
    "no repeated column in a row (the plain loss counts a pair once), an empty row, an empty column"
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for i in range(nrows):
        if i == 4:
            continue
        c = rng.choice(ncols - 1, size=rng.integers(1, 5), replace=False)          # (the last column stays empty)
        rows += [i] * len(c)
        cols += list(c)
    rp = np.zeros(nrows + 1, np.int64)
    np.add.at(rp, np.asarray(rows) + 1, 1)
    rp = np.cumsum(rp)
    ci = np.asarray(cols, np.int32)
    vs = rng.random(len(ci)) + 0.1
    atrp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=ncols))])
    U, V = rng.standard_normal((nrows, k)) * 0.5, rng.standard_normal((ncols, k)) * 0.5
    return rp, ci, vs, atrp, U, V


CONFIGS = {'explicit': dict(scale=False, rhs='values', implicit=False), 'implicit': dict(scale=True, rhs='one_plus_values', implicit=True)}


def _bound(adds, mag, const):
    """
    J and NumPy's loss - const are two roundings of one exact number.  J's sums have `adds` additions over terms of total
    magnitude mag: its error is at most adds 2^-53 mag.  NumPy's loss sums the same products expanded differently, plus the
    constant twice (in the loss and in the subtraction): at most adds 2^-53 (mag + 2 const).  Together adds 2^-52 (mag + const).
    """
    return adds * 2.0 ** -52 * (mag + const)


@pytest.mark.parametrize('config', sorted(CONFIGS))
def test_objective_is_the_plain_loss_minus_the_documented_constant(config):
    rp, ci, vs, atrp, U, V = _small()
    lam, lam_n = 0.3, 0.05
    cfg = CONFIGS[config]
    J = R.objective_exact((rp, ci, vs), atrp, U, V, cfg['scale'], cfg['rhs'], cfg['implicit'], lam, lam_n, R=5, L=4)
    loss, const, mag, adds = R.loss_numpy(rp, ci, vs, U, V, config, lam, lam_n)
    assert const > 1.0 and abs(J - (loss - const)) <= _bound(adds, mag, const)
    assert abs(J - loss) > 100 * _bound(adds, mag, const)          # (the constant is not noise)


def _numpy_half_step(rp, ci, vs, V, config, lam, lam_n):
    "the exact minimiser over the rows' factors, per row, in NumPy"
    k = V.shape[1]
    out = np.zeros((len(rp) - 1, k))
    G = V.T @ V if config == 'implicit' else np.zeros((k, k))
    for i in range(len(rp) - 1):
        e0, e1 = rp[i], rp[i + 1]
        Vr, a = V[ci[e0:e1]], vs[e0:e1]
        w = a if config == 'implicit' else np.ones(e1 - e0)
        c = 1 + a if config == 'implicit' else a
        M = G + (Vr * w[:, None]).T @ Vr + (lam + lam_n * (e1 - e0)) * np.eye(k)
        out[i] = np.linalg.solve(M, c @ Vr)
    return out


@pytest.mark.parametrize('config', sorted(CONFIGS))
def test_an_exact_half_step_does_not_increase_the_objective(config):
    rp, ci, vs, atrp, U, V = _small(seed=6)
    lam, lam_n = 0.3, 0.05
    before, const, mag, adds = R.loss_numpy(rp, ci, vs, U, V, config, lam, lam_n)
    U1 = _numpy_half_step(rp, ci, vs, V, config, lam, lam_n)
    after, _, mag1, _ = R.loss_numpy(rp, ci, vs, U1, V, config, lam, lam_n)
    assert after <= before + _bound(adds, max(mag, mag1), const) and after < before
