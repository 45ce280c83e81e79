"""
csrk_combine on the host side, without a GPU: the entries are declared in include/csrk.h, exported and in the ctypes table;
the row-class bounds need no device; every malformed argument is refused with ValueError before any library call; the C
entry refuses a null handle with an error code (no crash); without a device the CSR methods fail loudly instead of
computing on the CPU.  The NumPy restatement the GPU tests compare against (tests/combine_ref.py) is checked here against
scipy.sparse and against hand-written rows.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from combine_ref import combine_ref, same, OPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mat(ncols=4):
    from csr_amd import CSR
    return CSR(3, ncols, 4, np.array([0, 2, 2, 4], np.int32), np.array([0, 3, 1, 2], np.int32), np.array([1.0, -2.0, 0.5, 4.0]))


def _square():
    from csr_amd import CSR
    return CSR(2, 2, 2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.array([1.0, 2.0]))


def test_entries_declared_and_exported():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'csrk.h')).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, 'csr_amd', 'libcsrk.so'))
    from csr_amd import _lib
    for name in ('csrk_combine', 'csrk_combine_limits'):
        assert re.search(r'CSRK_API\s+int\s+' + name + r'\s*\(', text), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    for i, name in enumerate(('ADD', 'MUL', 'KEEP', 'DROP')):
        assert re.search(r'CSRK_COMBINE_%s\s*=\s*%d\b' % (name, i), text), name
        assert getattr(_lib, 'COMBINE_' + name) == i


def test_limits_need_no_device_and_ascend():
    from csr_amd.kernels import hip as K
    lim = K.combine_limits()
    assert len(lim) == 3 and lim[0] == 64
    assert all(a <= b for a, b in zip(lim, lim[1:])), lim
    assert lim[1] % 64 == 0


def _forbid(monkeypatch):
    from csr_amd.kernels import hip as K
    from csr_amd import _lib

    def forbidden(*a, **kw):
        raise AssertionError('library called')
    for name in ('csrk_combine', 'csrk_create', 'csrk_spgemm_ab', 'csrk_spgemm_abt', 'csrk_filter_zeros', 'csrk_export',
                 'csrk_topk_rows', 'csrk_pick_rows'):
        monkeypatch.setattr(_lib.lib, name, forbidden)
    monkeypatch.setattr(K, 'to_handle', forbidden)
    return K


BAD = {
    'unknown op': dict(op='subtract'),
    'op code': dict(op=0),
    'op None': dict(op=None),
    'string alpha': dict(op='add', alpha='1'),
    'string beta': dict(op='add', beta='x'),
    'complex alpha': dict(op='add', alpha=1j),
    'None beta': dict(op='add', beta=None),
}


@pytest.mark.parametrize('case', sorted(BAD))
def test_bad_arguments_raise_before_any_library_call(case, monkeypatch):
    K = _forbid(monkeypatch)
    h = K.hip_h(12345, 3, 4, 4)
    with pytest.raises(ValueError):
        K.combine(h, h, **BAD[case])
    kw = dict(BAD[case])
    op = kw.pop('op')
    if op == 'add':
        with pytest.raises(ValueError):
            _mat().add(_mat(), **kw)
    else:
        with pytest.raises(ValueError):
            _mat()._combine(_mat(), op)


def test_shape_mismatch_raises_before_any_library_call(monkeypatch):
    K = _forbid(monkeypatch)
    with pytest.raises(ValueError):
        K.combine(K.hip_h(12345, 3, 4, 4), K.hip_h(12346, 3, 5, 4), 'add')
    with pytest.raises(ValueError):
        K.combine(K.hip_h(12345, 3, 4, 4), K.hip_h(12346, 2, 4, 4), 'keep')
    a, b = _mat(4), _mat(5)
    for call in (lambda: a.add(b), lambda: a.subtract(b), lambda: a.multiply_entries(b), lambda: a.keep_entries(b),
                 lambda: a.drop_entries(b)):
        with pytest.raises(ValueError):
            call()


def test_exclude_of_the_wrong_shape_raises_before_any_library_call(monkeypatch):
    _forbid(monkeypatch)
    s = _square()
    for tr in (False, True):
        with pytest.raises(ValueError):
            s.multiply_topk(s, 1, transpose=tr, exclude=_mat())
    with pytest.raises(ValueError):                       # the top-k arguments are still checked first
        s.multiply_topk(s, 0, exclude=s)


def test_null_handle_is_an_error_code():
    from csr_amd._lib import lib, ERR_INVALID, handle_t
    for H in (0, 12345):
        for op in range(4):
            out = handle_t(77)
            assert lib.csrk_combine(H, H, op, 1.0, 1.0, ctypes.byref(out)) == ERR_INVALID
            assert b'invalid csrk handle' in lib.csrk_last_error()
            assert out.value == 0
    assert lib.csrk_combine(12345, 12345, 0, 1.0, 1.0, None) == ERR_INVALID
    assert lib.csrk_combine_limits(None, 3) == ERR_INVALID


def test_no_cpu_fallback():
    "without a device the CSR methods raise CsrkError; with one they compute (they never fall back to the CPU)"
    import torch
    from csr_amd._lib import CsrkError
    a, b = _mat(), _mat()
    calls = (lambda: a.add(b), lambda: a.subtract(b), lambda: a.multiply_entries(b), lambda: a.keep_entries(b),
             lambda: a.drop_entries(b), lambda: _square().multiply_topk(_square(), 1, exclude=_square()))
    if torch.cuda.device_count() > 0:
        t = a.subtract(b)
        assert list(t.rowptrs) == [0, 2, 2, 4] and list(t.colinds) == [0, 3, 1, 2] and list(t.values) == [0.0] * 4
        return
    for call in calls:
        with pytest.raises(CsrkError) as ei:
            call()
        assert 'hip' in str(ei.value).lower()


def test_shard_cuts_are_the_boundaries_of_shard_rows():
    "the cuts _combine takes the union of, for two operands that must be cut at the same rows"
    from csr_amd import CSR
    lens = np.array([3, 0, 4, 1, 1, 5, 2], np.int64)
    rp = np.concatenate(([0], np.cumsum(lens)))
    m = CSR(7, 9, int(rp[-1]), rp, np.zeros(int(rp[-1]), np.int32), None)
    cuts = m._shard_cuts(5)
    assert cuts[0] == 0 and cuts[-1] == 7 and all(rp[b] - rp[a] <= 5 for a, b in zip(cuts[:-1], cuts[1:]))
    assert [s.nrows for s in m._shard_rows(5)] == list(np.diff(cuts))


# ---- the restatement itself ---------------------------------------------------------------------------------------------
def _tuple(m, dtype=np.float64):
    "a canonical scipy matrix as (rowptrs, colinds, values)"
    m = m.tocsr()
    m.sort_indices()
    return m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.astype(dtype)


def _no_zeros(t):
    rp, ci, vs = t
    keep = vs != 0
    cum = np.concatenate(([0], np.cumsum(keep)))
    return cum[rp].astype(np.int32), ci[keep], vs[keep]


def _random_int_matrix(rng, nr, nc, density):
    import scipy.sparse as sps
    d = (rng.random((nr, nc)) < density) * rng.integers(1, 6, (nr, nc)) * rng.choice([-1, 1], (nr, nc))
    return sps.csr_matrix(d.astype(np.float64))


def test_restatement_against_scipy():
    import scipy.sparse as sps
    rng = np.random.default_rng(11)
    hand = [(sps.csr_matrix(np.array([[1., 0, 2, 0], [0, 0, 0, 0], [0, 3, 0, 4]])),
             sps.csr_matrix(np.array([[0., 5, -2, 0], [0, 0, 0, 0], [7, 3, 0, 0]])))]
    for nr, nc, da, db in ((1, 1, 1.0, 1.0), (5, 7, 0.5, 0.5), (40, 30, 0.1, 0.6), (30, 40, 0.6, 0.1), (17, 64, 0.3, 0.3), (6, 9, 0.0, 0.5)):
        hand.append((_random_int_matrix(rng, nr, nc, da), _random_int_matrix(rng, nr, nc, db)))
    for A, B in hand:
        a, b = _tuple(A), _tuple(B)
        # SciPy drops the zeros a sum or a product makes; the contract keeps them: compare without them on both sides
        assert same(_no_zeros(combine_ref(a, b, 'add')), _no_zeros(_tuple(A + B)), 'add')
        assert same(_no_zeros(combine_ref(a, b, 'add', 2.0, -3.0)), _no_zeros(_tuple(2.0 * A - 3.0 * B)), 'add')
        assert same(_no_zeros(combine_ref(a, b, 'multiply')), _no_zeros(_tuple(A.multiply(B))), 'multiply')
        pattern = sps.csr_matrix((np.ones(B.nnz), B.indices, B.indptr), shape=B.shape)
        assert same(combine_ref(a, b, 'keep'), _tuple(A.multiply(pattern)), 'keep')
        assert same(combine_ref(a, b, 'drop'), _tuple(A - A.multiply(pattern)), 'drop')
        # the union keeps exact zeros: its size is |A| + |B| - |A and B|
        n_both = int(A.astype(bool).multiply(B.astype(bool)).nnz)
        assert len(combine_ref(a, b, 'add', 1.0, -1.0)[1]) == A.nnz + B.nnz - n_both


def test_restatement_on_hand_written_rows():
    i4 = np.int32
    # an unsorted A that repeats columns, against a canonical B: storage order and bits stay
    A = (np.array([0, 6, 6, 8], i4), np.array([9, 2, 9, 0, 2, 5, 1, 1], i4), np.array([1, 2, 3, 4, 5, 6, 7, 8], np.float32))
    B = (np.array([0, 2, 3, 4], i4), np.array([2, 9, 4, 0], i4), None)
    rp, ci, vs = combine_ref(A, B, 'keep')
    assert list(rp) == [0, 5, 5, 5] and list(ci) == [9, 2, 9, 2, 5][:4] + [2] or True
    assert list(rp) == [0, 4, 4, 4] and list(ci) == [9, 2, 9, 2] and list(vs) == [1, 2, 3, 5] and vs.dtype == np.float32
    rp, ci, vs = combine_ref(A, B, 'drop')
    assert list(rp) == [0, 2, 2, 4] and list(ci) == [0, 5, 1, 1] and list(vs) == [4, 6, 7, 8] and vs.dtype == np.float32
    # a structure-only A stays structure-only
    rp, ci, vs = combine_ref((A[0], A[1], None), B, 'keep')
    assert vs is None and list(ci) == [9, 2, 9, 2]
    # add and multiply refuse that A; every op refuses an unsorted or repeating B
    for op in ('add', 'multiply'):
        with pytest.raises(ValueError):
            combine_ref(A, B, op)
    for op in OPS:
        with pytest.raises(ValueError):
            combine_ref(B, A, op)
    # add: the three kinds of entry, float32 widened, structure-only = 1.0, an exact zero stays
    A = (np.array([0, 3], i4), np.array([1, 4, 6], i4), np.array([0.1, 2.0, -1.0], np.float32))
    B = (np.array([0, 3], i4), np.array([0, 4, 6], i4), None)
    rp, ci, vs = combine_ref(A, B, 'add', 3.0, 1.0)
    assert rp.dtype == np.int32 and list(rp) == [0, 4] and list(ci) == [0, 1, 4, 6] and vs.dtype == np.float64
    assert list(vs) == [1.0, 3.0 * float(np.float32(0.1)), 7.0, -2.0]
    _, ci, vs = combine_ref(A, B, 'add', 1.0, 1.0)
    assert list(ci) == [0, 1, 4, 6] and vs[3] == 0.0
    _, ci, vs = combine_ref(A, B, 'multiply')
    assert list(ci) == [4, 6] and list(vs) == [2.0, -1.0]
    # IEEE: Inf - Inf and 0 * Inf are NaN, and same() lets any NaN stand for a NaN under add only
    A = (np.array([0, 2], i4), np.array([0, 1], i4), np.array([np.inf, np.inf]))
    B = (np.array([0, 2], i4), np.array([0, 1], i4), np.array([np.inf, 1.0]))
    r = combine_ref(A, B, 'add', 1.0, -1.0)
    assert np.isnan(r[2][0]) and r[2][1] == np.inf
    r0 = combine_ref(A, B, 'add', 0.0, 1.0)
    assert np.isnan(r0[2]).all()                                # 0 * Inf
    other = (r[0], r[1], r[2].copy())
    other[2].view(np.uint64)[0] ^= np.uint64(0x8000000000000001)    # another NaN
    assert same(other, r, 'add') and not same(other, r, 'keep')
    # no rows at all
    e = (np.array([0], i4), np.zeros(0, i4), np.zeros(0))
    for op in OPS:
        rp, ci, vs = combine_ref(e, e, op)
        assert list(rp) == [0] and len(ci) == 0 and len(vs) == 0
