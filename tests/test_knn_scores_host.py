"""
csrk_knn_scores on the host side, without a GPU: the entries are declared in include/csrk.h, exported and in the ctypes
table, the enum values are right; the limits need no device; every malformed argument is refused with ValueError before any
library call; the C entry refuses a bad handle with an error code; without a device CSR.knn_scores fails loudly.  The
restatement the GPU tests compare against (tests/knn_scores_ref.py) is checked here against hand-written rows and against a
dense brute-force form of the same rule.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from knn_scores_ref import knn_scores_ref, knn_scores_dense, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i4 = np.int32


def _ratings():
    from csr_amd import CSR
    return CSR(3, 4, 5, np.array([0, 2, 2, 5], i4), np.array([0, 3, 0, 1, 2], i4), np.array([4.0, 2.0, 5.0, 3.0, 1.0]))


def _model(ncols=4):
    from csr_amd import CSR
    return CSR(4, ncols, 4, np.array([0, 1, 2, 3, 4], i4), np.array([1, 0, 3, 2], i4), np.array([0.5, 0.5, 0.25, 0.25]))


def test_entries_declared_and_exported():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'csrk.h')).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, 'csr_amd', 'libcsrk.so'))
    from csr_amd import _lib
    from csr_amd.kernels import raw
    for name in ('csrk_knn_scores', 'csrk_knn_scores_limits'):
        assert re.search(r'CSRK_API\s+int\s+' + name + r'\s*\(', text), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
        assert name in raw.table()
    for i, name in enumerate(('WEIGHTED_AVERAGE', 'SUM')):
        assert re.search(r'CSRK_KNN_%s\s*=\s*%d\b' % (name, i), text), name
        assert getattr(_lib, 'KNN_' + name) == i


def test_limits_need_no_device():
    from csr_amd.kernels import hip as K
    lanes, tile, lds_row, bits, tiles_max, fill = K.knn_scores_limits()
    assert tiles_max >= 1 and fill >= 1
    assert lanes >= 1 and 64 % lanes == 0                       # whole groups in a wavefront
    assert tile >= lanes and tile % lanes == 0
    assert bits >= 32 and bits & (bits - 1) == 0                # a power of two: the residue is a mask
    assert lds_row >= 1 and (lds_row * 12 + bits // 8) * 2 <= 160 * 1024      # two workgroups' staged rows and filters fit the LDS of a CU
    from csr_amd._lib import lib, ERR_INVALID
    assert lib.csrk_knn_scores_limits(None, 3) == ERR_INVALID
    out = (ctypes.c_int64 * 3)(-1, -1, -1)
    assert lib.csrk_knn_scores_limits(out, 1) == 0 and list(out) == [lanes, -1, -1]


def _forbid(monkeypatch):
    from csr_amd.kernels import hip as K
    from csr_amd import _lib

    def forbidden(*a, **kw):
        raise AssertionError('library called')
    for name in ('csrk_knn_scores', 'csrk_create', 'csrk_combine', 'csrk_export', 'csrk_topk_rows', 'csrk_pick_rows'):
        monkeypatch.setattr(_lib.lib, name, forbidden)
    monkeypatch.setattr(K, 'to_handle', forbidden)
    return K


BAD = {
    'unknown aggregate': dict(aggregate='mean'),
    'aggregate code': dict(aggregate=0),
    'aggregate None': dict(aggregate=None),
    'float max_nbrs': dict(max_nbrs=2.0),
    'negative max_nbrs': dict(max_nbrs=-1),
    'bool max_nbrs': dict(max_nbrs=True),
    'zero min_nbrs': dict(min_nbrs=0),
    'float min_nbrs': dict(min_nbrs=1.5),
    '2-D users': dict(users=np.zeros((2, 2), i4)),
    'float users': dict(users=np.array([0.0, 1.0])),
    'bool users': dict(users=np.array([True, False])),
    'user too large': dict(users=np.array([0, 3])),
    'negative user': dict(users=np.array([-1])),
    'short offsets': dict(users=np.array([0, 1]), offsets=np.zeros(1)),
    'long offsets': dict(users=np.array([0, 1]), offsets=np.zeros(3)),
    '2-D offsets': dict(users=np.array([0, 1]), offsets=np.zeros((2, 1))),
    'string offsets': dict(users=np.array([0]), offsets=np.array(['a'])),
}


@pytest.mark.parametrize('case', sorted(BAD))
def test_bad_arguments_raise_before_any_library_call(case, monkeypatch):
    K = _forbid(monkeypatch)
    kw = dict(BAD[case])
    users = kw.pop('users', np.array([0, 2]))
    with pytest.raises(ValueError):
        K.knn_scores(K.hip_h(12345, 4, 4, 4), K.hip_h(12346, 3, 4, 5), users, **kw)
    with pytest.raises(ValueError):
        _ratings().knn_scores(_model(), users, **kw)
    with pytest.raises(ValueError):
        _ratings().knn_topk(_model(), users, 2, **kw)


def test_shapes_and_topk_arguments_raise_before_any_library_call(monkeypatch):
    K = _forbid(monkeypatch)
    with pytest.raises(ValueError):
        K.knn_scores(K.hip_h(12345, 4, 5, 4), K.hip_h(12346, 3, 4, 5), np.array([0]))
    with pytest.raises(ValueError):
        _ratings().knn_scores(_model(5))
    with pytest.raises(ValueError):
        _ratings().knn_scores(np.zeros((4, 4)))
    with pytest.raises(ValueError):
        _ratings().knn_topk(_model(), [0], 0)
    with pytest.raises(ValueError):
        _ratings().knn_topk(_model(), [0], 2, min_value=float('nan'))
    from csr_amd import CSR
    tall = CSR(5, 4, 0, np.zeros(6, i4), np.zeros(0, i4), np.zeros(0))
    with pytest.raises(ValueError):                       # exclude needs a model over the rated items
        _ratings().knn_topk(tall, [0], 2)
    with pytest.raises(TypeError):
        _ratings().knn_topk(_model(), [0], 2, neighbours=3)
    # the good arguments come back as the library takes them
    users, mx, mn, code, off = K.knn_scores_args(_model(), _ratings(), [2, 0, 2], 20, 2, 'sum', [1, 2, 3])
    assert users.dtype == np.int32 and list(users) == [2, 0, 2] and (mx, mn, code) == (20, 2, 1)
    assert off.dtype == np.float64 and list(off) == [1.0, 2.0, 3.0]
    users, mx, mn, code, off = K.knn_scores_args(_model(), _ratings(), [])
    assert len(users) == 0 and users.dtype == np.int32 and (mx, mn, code, off) == (0, 1, 0, None)


def test_bad_handle_is_an_error_code():
    from csr_amd._lib import lib, ERR_INVALID, handle_t
    rows = np.array([0], i4)
    for H in (0, 12345):
        for agg in (0, 1):
            out = handle_t(77)
            assert lib.csrk_knn_scores(H, H, rows.ctypes.data, 1, 0, 1, agg, None, ctypes.byref(out)) == ERR_INVALID
            assert b'invalid csrk handle' in lib.csrk_last_error()
            assert out.value == 0
    assert lib.csrk_knn_scores(12345, 12345, rows.ctypes.data, 1, 0, 1, 0, None, None) == ERR_INVALID
    assert b'out is NULL' in lib.csrk_last_error()


def test_no_cpu_fallback():
    "without a device the CSR methods raise CsrkError; with one they compute (they never fall back to the CPU)"
    import torch
    from csr_amd._lib import CsrkError
    r, m = _ratings(), _model()
    if torch.cuda.device_count() > 0:
        got = r.knn_scores(m)
        assert same((got.rowptrs, got.colinds, got.values), knn_scores_ref(_t(m), _t(r), range(3)))
        return
    for call in (lambda: r.knn_scores(m), lambda: r.knn_topk(m, [0, 2], 2)):
        with pytest.raises(CsrkError) as ei:
            call()
        assert 'hip' in str(ei.value).lower()


def _t(m):
    return m.rowptrs, m.colinds, m.values


# ---- the restatement itself ---------------------------------------------------------------------------------------------
def test_restatement_on_hand_written_rows():
    # one user who rated items 0, 2, 3, 5 with 4, 1, 5, 2
    R = (np.array([0, 4], i4), np.array([0, 2, 3, 5], i4), np.array([4.0, 1.0, 5.0, 2.0]))
    # target 0: neighbours by descending similarity, columns NOT ascending; item 4 is unrated
    M = (np.array([0, 4, 4, 7], i4), np.array([5, 4, 0, 2, 3, 3, 1], i4), np.array([0.5, 0.4, 0.25, 0.125, 1.0, 0.5, 2.0]))
    rp, ci, vs = knn_scores_ref(M, R, [0])
    assert rp.dtype == np.int32 and ci.dtype == np.int32 and vs.dtype == np.float64
    assert list(rp) == [0, 2] and list(ci) == [0, 2]              # the empty model row stores nothing
    assert vs[0] == (2 * 0.5 + 4 * 0.25 + 1 * 0.125) / 0.875
    # a repeated model column is counted twice: (5 * 1.0 + 5 * 0.5) / 1.5, the unrated item 1 does not count
    assert vs[1] == 5.0
    assert list(knn_scores_ref(M, R, [0], aggregate='sum')[2]) == [0.875, 1.5]
    # the cut at max_nbrs = 2 takes the first two RATED neighbours (items 5, 0), skipping the unrated item 4 ...
    cut = knn_scores_ref(M, R, [0], max_nbrs=2)
    assert cut[2][0] == (2 * 0.5 + 4 * 0.25) / 0.75
    # ... which differs from pruning the model to its first two entries (items 5, 4: one hit only)
    pruned = (np.array([0, 2, 2, 4], i4), np.array([5, 4, 3, 3], i4), np.array([0.5, 0.4, 1.0, 0.5]))
    assert knn_scores_ref(pruned, R, [0])[2][0] == 2.0 != cut[2][0]
    # ... and from a cut by column order (items 0, 2)
    assert cut[2][0] != (4 * 0.25 + 1 * 0.125) / 0.375
    # min_nbrs: target 0 has 3 hits, target 2 has 2
    assert list(knn_scores_ref(M, R, [0], min_nbrs=2)[1]) == [0, 2]
    assert list(knn_scores_ref(M, R, [0], min_nbrs=3)[1]) == [0]
    assert list(knn_scores_ref(M, R, [0], min_nbrs=4)[0]) == [0, 0]
    # max_nbrs caps nn, so min_nbrs above it stores nothing
    assert list(knn_scores_ref(M, R, [0], max_nbrs=1, min_nbrs=2)[0]) == [0, 0]
    # offsets are added last; a repeated user gives the same row twice
    rp, ci, vs = knn_scores_ref(M, R, [0, 0], offsets=[0.0, 10.0])
    assert list(rp) == [0, 2, 4] and list(ci) == [0, 2, 0, 2] and vs[2] == vs[0] + 10.0 and vs[3] == 15.0
    # structure-only operands count as 1.0, float32 is widened exactly
    assert list(knn_scores_ref((M[0], M[1], None), R, [0])[2]) == [7.0 / 3.0, 5.0]
    assert list(knn_scores_ref(M, (R[0], R[1], None), [0])[2]) == [1.0, 1.0]
    m32 = (M[0], M[1], np.array([0.1] * 7, np.float32))
    assert knn_scores_ref(m32, R, [0], aggregate='sum')[2][1] == float(np.float32(0.1)) + float(np.float32(0.1))
    # a zero similarity is a hit: it counts toward max_nbrs; den = 0 stores NaN
    z = (np.array([0, 3], i4), np.array([0, 2, 3], i4), np.array([0.0, -0.0, 1.0]))
    assert np.isnan(knn_scores_ref(z, R, [0], max_nbrs=2)[2][0]) and knn_scores_ref(z, R, [0])[2][0] == 5.0
    # no users, no targets
    assert list(knn_scores_ref(M, R, [])[0]) == [0]
    assert list(knn_scores_ref((np.array([0], i4), np.zeros(0, i4), np.zeros(0)), R, [0])[0]) == [0, 0]


@pytest.mark.parametrize('seed', range(4))
def test_restatement_against_dense_brute_force(seed):
    rng = np.random.default_rng(seed)
    nu, nt, ni = 7, 9, 12
    has_m, has_r = rng.random((nt, ni)) < 0.4, rng.random((nu, ni)) < 0.5
    Md, Rd = rng.normal(size=(nt, ni)), rng.integers(1, 6, (nu, ni)).astype(np.float64)

    def tup(has, D):
        rp = np.concatenate(([0], np.cumsum(has.sum(1)))).astype(i4)
        r, c = np.nonzero(has)
        return rp, c.astype(i4), D[r, c]
    M, R = tup(has_m, Md), tup(has_r, Rd)
    users = rng.integers(0, nu, 10)
    off = rng.normal(size=10)
    for agg in ('weighted-average', 'sum'):
        for mx in (0, 1, 2, 5):
            for mn in (1, 2, 3):
                for o in (None, off):
                    rp, ci, vs = knn_scores_ref(M, R, users, mx, mn, agg, o)
                    stored, value = knn_scores_dense(Md, has_m, Rd, has_r, users, mx, mn, agg, o)
                    r, c = np.nonzero(stored)
                    assert list(rp) == [0] + list(np.cumsum(stored.sum(1))) and list(ci) == list(c)
                    assert same((rp, ci, vs), (rp, c.astype(i4), value[r, c]))
