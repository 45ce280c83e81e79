"""
The reach route of knn_scores on the host side, without a GPU: csrk_knn_scores_reach, csrk_knn_reach_index,
csrk_knn_scores_reach_limits and csrk_knn_scores_last_stats are declared in include/csrk.h, exported, in the ctypes table and in
the raw-address table; the limits need no device and are sane; a bad `route` is refused with ValueError before any library
call; the C entries refuse a bad handle and NULL pointers with an error code; without a device route='reach' fails loudly.
The last test covers the argument the route rests on: the targets reached through a transpose of the model's pattern are, per
user, exactly the targets the restatement (tests/knn_scores_ref.py) stores at min_nbrs = 1, and a superset of them otherwise.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from knn_scores_ref import knn_scores_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i4 = np.int32
NEW = ('csrk_knn_scores_reach', 'csrk_knn_reach_index', 'csrk_knn_scores_reach_limits', 'csrk_knn_scores_last_stats')


def _ratings():
    from csr_amd import CSR
    return CSR(3, 4, 5, np.array([0, 2, 2, 5], i4), np.array([0, 3, 0, 1, 2], i4), np.array([4.0, 2.0, 5.0, 3.0, 1.0]))


def _model():
    from csr_amd import CSR
    return CSR(4, 4, 4, np.array([0, 1, 2, 3, 4], i4), np.array([1, 0, 3, 2], i4), np.array([0.5, 0.5, 0.25, 0.25]))


def test_entries_declared_and_exported():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'csrk.h')).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, 'csr_amd', 'libcsrk.so'))
    from csr_amd import _lib
    from csr_amd.kernels import raw
    for name in NEW:
        assert re.search(r'CSRK_API\s+int\s+' + name + r'\s*\(', text), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
        assert name in raw.table() and raw.address(name)
    # the two scoring entries take the same arguments
    assert _lib.SIGNATURES['csrk_knn_scores_reach'] == _lib.SIGNATURES['csrk_knn_scores']


def test_limits_need_no_device():
    from csr_amd.kernels import hip as K
    from csr_amd._lib import lib, ERR_INVALID
    lim = K.knn_scores_reach_limits()
    assert len(lim) == len(K.KNN_REACH_LIMITS) >= 6
    R, lanes, lds_row, bits, per_round, chunk = lim[:6]
    assert R >= 32 and R & (R - 1) == 0 and R % 32 == 0            # a power of two, whole 32-bit words
    walk = K.knn_scores_limits()
    assert (lanes, lds_row, bits) == (walk[0], walk[2], walk[3])    # the walk is the walk-all route's
    # two workgroups' staged row, filter and bitmap fit the LDS of a CU
    assert (lds_row * 12 + bits // 8 + R // 8) * 2 <= 160 * 1024
    assert per_round >= 1 and per_round % (64 // lanes) == 0
    assert 1 <= chunk <= R and R % chunk == 0
    if len(lim) > 6:
        assert lim[6] >= lanes                                       # the long-reach-row threshold
    assert lib.csrk_knn_scores_reach_limits(None, 3) == ERR_INVALID
    out = (ctypes.c_int64 * 3)(-1, -1, -1)
    assert lib.csrk_knn_scores_reach_limits(out, 1) == 0 and list(out) == [R, -1, -1]


def _forbid(monkeypatch):
    from csr_amd.kernels import hip as K
    from csr_amd import _lib

    def forbidden(*a, **kw):
        raise AssertionError('library called')
    for name in ('csrk_knn_scores', 'csrk_knn_scores_reach', 'csrk_knn_reach_index', 'csrk_create', 'csrk_combine', 'csrk_export',
                 'csrk_topk_rows', 'csrk_pick_rows'):
        monkeypatch.setattr(_lib.lib, name, forbidden)
    monkeypatch.setattr(K, 'to_handle', forbidden)
    return K


@pytest.mark.parametrize('route', ['Reach', 'all', '', None, 1, True, b'reach'])
def test_bad_route_raises_before_any_library_call(route, monkeypatch):
    K = _forbid(monkeypatch)
    users = np.array([0, 2])
    with pytest.raises(ValueError) as ei:
        K.knn_scores(K.hip_h(12345, 4, 4, 4), K.hip_h(12346, 3, 4, 5), users, route=route)
    assert 'route' in str(ei.value)
    with pytest.raises(ValueError):
        _ratings().knn_scores(_model(), users, route=route)
    with pytest.raises(ValueError):
        _ratings().knn_topk(_model(), users, 2, route=route)


@pytest.mark.parametrize('route', ['walk', 'reach'])
def test_other_bad_arguments_still_raise_first(route, monkeypatch):
    K = _forbid(monkeypatch)
    for kw in (dict(aggregate='mean'), dict(min_nbrs=0), dict(max_nbrs=-1), dict(users=np.array([0, 3]))):
        kw = dict(kw)
        users = kw.pop('users', np.array([0, 2]))
        with pytest.raises(ValueError):
            K.knn_scores(K.hip_h(12345, 4, 4, 4), K.hip_h(12346, 3, 4, 5), users, route=route, **kw)
        with pytest.raises(ValueError):
            _ratings().knn_scores(_model(), users, route=route, **kw)
        with pytest.raises(ValueError):
            _ratings().knn_topk(_model(), users, 2, route=route, **kw)
    # knn_scores_args keeps its signature and its 5-tuple
    assert len(K.knn_scores_args(_model(), _ratings(), [0])) == 5


def test_bad_handles_and_null_pointers_are_error_codes():
    from csr_amd._lib import lib, ERR_INVALID, OK, handle_t
    rows = np.array([0], i4)
    for H in (0, 12345):
        for agg in (0, 1):
            out = handle_t(77)
            assert lib.csrk_knn_scores_reach(H, H, rows.ctypes.data, 1, 0, 1, agg, None, ctypes.byref(out)) == ERR_INVALID
            assert b'invalid csrk handle' in lib.csrk_last_error()
            assert out.value == 0
        e, b = ctypes.c_int64(7), ctypes.c_int64(7)
        for build in (0, 1):
            assert lib.csrk_knn_reach_index(H, build, ctypes.byref(e), ctypes.byref(b)) == ERR_INVALID
            assert b'invalid csrk handle' in lib.csrk_last_error() and (e.value, b.value) == (0, 0)
    assert lib.csrk_knn_scores_reach(12345, 12345, rows.ctypes.data, 1, 0, 1, 0, None, None) == ERR_INVALID
    assert lib.csrk_last_error().startswith(b'knn_scores_reach: out is NULL')
    assert lib.csrk_knn_scores(12345, 12345, rows.ctypes.data, 1, 0, 1, 0, None, None) == ERR_INVALID
    assert lib.csrk_last_error().startswith(b'knn_scores: out is NULL')            # the walk-all entry keeps its own name
    e = ctypes.c_int64(7)
    assert lib.csrk_knn_reach_index(12345, 0, None, ctypes.byref(e)) == ERR_INVALID
    assert lib.csrk_knn_reach_index(12345, 0, ctypes.byref(e), None) == ERR_INVALID
    assert lib.csrk_knn_scores_last_stats(None, 6) == ERR_INVALID
    # after failed calls the census is all zero
    st = (ctypes.c_int64 * 6)(*[-1] * 6)
    assert lib.csrk_knn_scores_last_stats(st, 6) == OK and list(st) == [0] * 6
    st = (ctypes.c_int64 * 3)(-1, -1, -1)
    assert lib.csrk_knn_scores_last_stats(st, 1) == OK and list(st) == [0, -1, -1]


def test_no_cpu_fallback():
    "without a device route='reach' raises CsrkError (it never falls back to the CPU or to the other route)"
    import torch
    from csr_amd._lib import CsrkError
    from csr_amd.kernels import hip as K
    r, m = _ratings(), _model()
    if torch.cuda.device_count() > 0:
        got, exp = r.knn_scores(m, route='reach'), r.knn_scores(m)
        assert np.array_equal(got.rowptrs, exp.rowptrs) and np.array_equal(got.colinds, exp.colinds)
        assert got.values.tobytes() == exp.values.tobytes()
        return
    for call in (lambda: r.knn_scores(m, route='reach'), lambda: r.knn_topk(m, [0, 2], 2, route='reach')):
        with pytest.raises(CsrkError) as ei:
            call()
        assert 'hip' in str(ei.value).lower()
    assert K.knn_scores_last_stats() == (0,) * len(K.KNN_STATS)


# ---- the argument the route rests on ------------------------------------------------------------------------------------------
def _reached(M, R, users, n_items):
    "per user, the sorted targets found through a NumPy transpose of the model's pattern: row j = the targets that store column j"
    mrp, mci, _ = M
    rrp, rci, _ = R
    target_of = np.repeat(np.arange(len(mrp) - 1), np.diff(mrp))
    order = np.argsort(mci, kind='stable')                       # a counting sort by column: ascending targets inside a row
    tp = np.concatenate(([0], np.cumsum(np.bincount(mci, minlength=n_items))))
    ti = target_of[order]
    assert len(ti) == len(mci)                                   # one entry per stored occurrence: repeats are kept
    for j in range(n_items):
        assert np.all(np.diff(ti[tp[j]:tp[j + 1]]) >= 0)
    out = []
    for u in users:
        rated = rci[rrp[u]:rrp[u + 1]]
        out.append(np.unique(np.concatenate([np.zeros(0, np.int64)] + [ti[tp[j]:tp[j + 1]] for j in rated])))
    return out


@pytest.mark.parametrize('seed', range(6))
def test_reached_targets_are_the_stored_ones_at_min_nbrs_1(seed):
    rng = np.random.default_rng(seed)
    n_users, n_targets, n_items = 6, 11, 9
    # model rows in any order WITH repeated columns; some empty; ratings canonical, some users without ratings
    lens = rng.integers(0, 7, n_targets)
    mci = np.concatenate([np.zeros(0, np.int64)] + [rng.integers(0, n_items, n) for n in lens]).astype(i4)
    M = (np.concatenate(([0], np.cumsum(lens))).astype(i4), mci, rng.normal(size=len(mci)))
    if seed == 0:
        assert any(len(set(mci[a:b])) < b - a for a, b in zip(M[0][:-1], M[0][1:]))       # a repeat is present
    has = rng.random((n_users, n_items)) < 0.3
    has[0] = False
    r, c = np.nonzero(has)
    R = (np.concatenate(([0], np.cumsum(has.sum(1)))).astype(i4), c.astype(i4), rng.integers(1, 6, len(c)).astype(np.float64))
    users = list(rng.permutation(n_users)) + [0, 3]
    reached = _reached(M, R, users, n_items)
    for agg in ('weighted-average', 'sum'):
        for mx in (0, 1, 2):
            for mn in (1, 2, 3):
                rp, ci, _ = knn_scores_ref(M, R, users, mx, mn, agg)
                for k in range(len(users)):
                    stored = ci[rp[k]:rp[k + 1]]
                    if mn == 1:
                        assert np.array_equal(stored, reached[k]), (agg, mx, k)
                    else:
                        assert np.all(np.isin(stored, reached[k])), (agg, mx, mn, k)
