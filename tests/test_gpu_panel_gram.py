"""
csrk_panel_gram on the card (include/csrk.h, rule P): G = V^T V + ridge I bit for bit against the exact restatement
(tests/als_fit_ref.py, panel_gram_exact) at every edge of the chunks and of the tree, at every edge of the k classes and
their tiles, with every option; NaN / Inf by position; exact symmetry and repeatability; the device form on a side stream
with the exact workspace; the limit and workspace refusals; a large case against float64 NumPy.

The exact reference makes about 10^5 fused steps per second and a row of V costs k (k + 1) / 2 of them: the chunk edges run
at k = 3, the k edges at 12 rows or fewer.
"""
import ctypes as C

import numpy as np
import pytest

import als_fit_ref as R

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same(a, b):
    "equal bits, a NaN matching any NaN (a created NaN has its position specified, not its sign or payload)"
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _panel(n, k, pdt, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, k)) * (1.0 + np.arange(k) / 7.0)).astype(pdt)


@pytest.fixture(scope='module')
def K():
    from csr_amd.kernels import hip
    return hip


@pytest.fixture(scope='module')
def limits(K):
    return K.panel_gram_limits()


def test_limits(limits):
    assert limits[0] >= 128 and limits[1] >= 1


# ---- 1. chunk edges: the tree sees odd counts at two levels (3 R + 1 -> 4 -> 2 -> 1 is even; 5 R -> 5 -> 3 -> 2 -> 1) ----

CHUNK_NS = [(0, 0), (0, 1), (1, -1), (1, 0), (1, 1), (2, 0), (2, 1), (3, 1), (5, 0)]      # n = a R + b


@pytest.fixture(scope='module')
def chunk_panel(limits):
    return _panel(5 * int(limits[1]), 3, np.float64, 11)


@pytest.mark.parametrize('a,b', CHUNK_NS, ids=[f'{a}R{b:+d}' for a, b in CHUNK_NS])
def test_chunk_edges(K, limits, chunk_panel, a, b):
    Rr = int(limits[1])
    V = chunk_panel[:a * Rr + b]
    assert _same(K.panel_gram(V, 0.25), R.panel_gram_exact(V, 0.25, Rr))


# ---- 2. k edges: tiles (4), the classes (40, 88), pieces, the largest k ----

KS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128]


@pytest.mark.parametrize('pdt', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('k', KS)
def test_k_edges(K, limits, k, pdt):
    n = 12 if k <= 33 else (5 if k <= 65 else 2)
    V = _panel(n, k, pdt, 100 + k)
    assert _same(K.panel_gram(V, 0.0), R.panel_gram_exact(V, 0.0, int(limits[1])))


@pytest.mark.parametrize('k', [39, 40, 41, 87, 88, 89])
def test_class_edges(K, limits, k):
    V = _panel(3, k, np.float64, 200 + k)
    assert _same(K.panel_gram(V, 0.0), R.panel_gram_exact(V, 0.0, int(limits[1])))


# ---- 3. options ----

@pytest.mark.parametrize('pdt', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('ridge', [0.0, 0.5, -0.0])
def test_options(K, limits, pdt, ridge):
    "ldv > k, a view offset by one element (no 16-B alignment: element loads), every ridge: one result"
    Rr = int(limits[1])
    k = 8
    wide = _panel(40, k + 5, pdt, 7)
    want = R.panel_gram_exact(wide[:, 1:1 + k], ridge, Rr)
    for V in (np.ascontiguousarray(wide[:, 1:1 + k]), wide[:, 1:1 + k], wide[:, 0:k + 1][:, 1:]):
        assert _same(K.panel_gram(V, ridge), want)


def test_negative_zero_sum_becomes_positive_zero(K):
    "P4: the ridge is always added, so a -0.0 sum on the diagonal cannot survive; off the diagonal it does"
    V = np.array([[0.0, -0.0], [0.0, 0.0]])
    G = K.panel_gram(V, -0.0)
    assert not np.signbit(G[0, 0]) and not np.signbit(G[1, 1])
    assert _same(G, R.panel_gram_exact(V, -0.0, 4))


def test_fused_on_the_card(K):
    "the input on which the fused and the two-rounding restatements differ (tests/test_als_fit_host.py): the card fuses"
    x = 1.0 + 2.0 ** -30
    G = K.panel_gram(np.array([[1.0, -1.0], [x, x]]), 0.0)
    assert G[1, 0] == 2.0 ** -29 + 2.0 ** -60


# ---- 4. special values ----

def test_nan_and_inf_rows_by_position(K, limits):
    Rr = int(limits[1])
    V = _panel(Rr + 3, 5, np.float64, 21)
    V[2, 1] = np.nan
    V[Rr + 1, 3] = np.inf
    got, want = K.panel_gram(V, 0.5), R.panel_gram_exact(V, 0.5, Rr)
    assert np.isnan(want[1, 0]) and np.isposinf(want[3, 3]) and np.isfinite(want[4, 0])
    assert _same(got, want)


# ---- 5. symmetry and repeatability ----

def test_symmetric_and_repeatable(K, limits):
    V = _panel(3 * int(limits[1]) + 17, 37, np.float32, 31)
    a, b = K.panel_gram(V, 0.1), K.panel_gram(V, 0.1)
    assert np.array_equal(_bits(a), _bits(a.T.copy())) and np.array_equal(_bits(a), _bits(b))


# ---- 6. the device form ----

def _device_gram(V, ridge, short=0, stream=True, prefill=None):
    "csrk_panel_gram_device on torch buffers with a workspace of exactly the reported size minus `short` bytes: (rc, out)"
    import torch
    from csr_amd._lib import lib
    n, k = V.shape
    need = C.c_int64(-1)
    assert lib.csrk_panel_gram_workspace(n, k, C.byref(need)) == 0
    dV = torch.from_numpy(np.ascontiguousarray(V)).cuda()
    dO = torch.from_numpy(np.full((k, k), -7.0) if prefill is None else prefill).cuda()
    dW = torch.empty(max(need.value, 8), dtype=torch.uint8, device='cuda')
    s = torch.cuda.Stream() if stream else None
    code = {np.dtype('f4'): 1, np.dtype('f8'): 2}[V.dtype]
    torch.cuda.synchronize()
    rc = lib.csrk_panel_gram_device(n, k, dV.data_ptr(), k, code, ridge, dO.data_ptr(), dW.data_ptr(), need.value - short,
                                    s.cuda_stream if s else None)
    torch.cuda.synchronize()
    return rc, dO.cpu().numpy(), need.value


@pytest.mark.parametrize('nR', [0, 1, 3, 40])
def test_device_form_on_a_side_stream(K, limits, nR):
    "the exact workspace size; 40 chunks take two tree launches"
    Rr = int(limits[1])
    V = _panel(nR * Rr + (5 if nR else 0), 6, np.float64, 41)
    rc, got, need = _device_gram(V, 0.5)
    assert rc == 0 and (need > 0) == (nR > 0)
    assert _same(got, K.panel_gram(V, 0.5))
    if nR == 40:
        assert np.all(np.abs(got - (V.T @ V + 0.5 * np.eye(6))) <= len(V) * 2.0 ** -52 * (np.abs(V).T @ np.abs(V) + 0.5))


def test_workspace_one_byte_short_is_refused_untouched(limits):
    from csr_amd import _lib
    V = _panel(int(limits[1]) + 1, 4, np.float64, 51)
    rc, out, _ = _device_gram(V, 0.0, short=1)
    assert rc == _lib.ERR_INVALID and np.all(out == -7.0)
    assert 'workspace' in _lib.last_error()


def test_k_above_the_limit_is_unsupported(K, limits):
    from csr_amd import _lib
    k = int(limits[0]) + 1
    with pytest.raises(_lib.CsrkError) as ei:
        K.panel_gram(np.ones((2, k)), 0.0)
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    need = C.c_int64(-1)
    assert _lib.lib.csrk_panel_gram_workspace(2, k, C.byref(need)) == _lib.ERR_UNSUPPORTED and need.value == -1


def test_library_refusals_write_nothing(limits):
    "what the Python wrapper never lets through: refused by the library itself, out untouched"
    from csr_amd import _lib
    lib = _lib.lib
    V, out = np.ones((4, 3)), np.full((3, 3), -7.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    for args in ((-1, 3, p(V), 3, 2, 0.0, p(out)), (4, 0, p(V), 3, 2, 0.0, p(out)), (4, 3, p(V), 2, 2, 0.0, p(out)),
                 (4, 3, p(V), 3, 7, 0.0, p(out)), (4, 3, p(V), 3, 2, float('nan'), p(out)), (4, 3, None, 3, 2, 0.0, p(out)),
                 (4, 3, p(V), 3, 2, 0.0, None), (4, 3, C.c_void_p(V.ctypes.data + 4), 3, 2, 0.0, p(out))):
        assert lib.csrk_panel_gram(*args) == _lib.ERR_INVALID, args
    assert np.all(out == -7.0)


# ---- 7. a large case against float64 NumPy ----

def test_large_against_numpy(K):
    V = _panel(20000, 64, np.float64, 61)
    G = K.panel_gram(V, 0.0)
    bound = len(V) * 2.0 ** -52 * (np.abs(V).T @ np.abs(V))
    assert np.all(np.abs(G - V.T @ V) <= bound)
    assert np.array_equal(_bits(G), _bits(G.T.copy()))
