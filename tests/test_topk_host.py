"""
Row top-k on the host side, without a GPU: the entries are declared in include/csrk.h, exported and in the ctypes table;
every malformed argument is refused with ValueError before any library call; the C entry refuses a null handle with an
error code (no crash); without a device CSR.topk_rows fails loudly instead of computing on the CPU.  The NumPy
restatement the GPU tests compare against (tests/topk_ref.py) is checked here on hand-written rows.
"""
import ctypes
import os

import numpy as np
import pytest

from topk_ref import topk_rows_ref, topk_rows_vec, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float('nan'), float('inf')


def _mat():
    from csr_amd import CSR
    return CSR(3, 4, 4, np.array([0, 2, 2, 4], np.int32), np.array([3, 0, 1, 1], np.int32), np.array([1.0, -2.0, 0.5, 4.0]))


def test_entries_declared_and_exported():
    import re
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'csrk.h')).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, 'csr_amd', 'libcsrk.so'))
    from csr_amd import _lib
    for name in ('csrk_topk_rows', 'csrk_topk_limits'):
        assert re.search(r'CSRK_API\s+int\s+' + name + r'\s*\(', text), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert re.search(r'CSRK_TOPK_BY_VALUE\s*=\s*0\b', text) and re.search(r'CSRK_TOPK_STORAGE\s*=\s*1\b', text)
    assert (_lib.TOPK_BY_VALUE, _lib.TOPK_STORAGE) == (0, 1)


def test_limits_need_no_device():
    from csr_amd.kernels import hip as K
    short, cap, threads, mid = K.topk_limits()
    assert 1 <= short <= mid <= cap and threads >= 64


BAD = {
    'k = 0': dict(k=0),
    'k < 0': dict(k=-3),
    'k float': dict(k=2.5),
    'k integral float': dict(k=2.0),
    'k bool': dict(k=True),
    'k None': dict(k=None),
    'NaN min_value': dict(k=2, min_value=NAN),
    'unknown order': dict(k=2, order='ascending'),
    'order code': dict(k=2, order=0),
}


@pytest.mark.parametrize('case', sorted(BAD))
def test_bad_arguments_raise_before_any_library_call(case, monkeypatch):
    from csr_amd.kernels import hip as K
    from csr_amd import _lib

    def forbidden(*a, **kw):
        raise AssertionError('library called')
    for name in ('csrk_topk_rows', 'csrk_create', 'csrk_spgemm_ab', 'csrk_spgemm_abt', 'csrk_filter_zeros', 'csrk_export'):
        monkeypatch.setattr(_lib.lib, name, forbidden)
    monkeypatch.setattr(K, 'to_handle', forbidden)
    kw = BAD[case]
    h = K.hip_h(12345, 3, 4, 4)
    with pytest.raises(ValueError):
        K.topk_rows(h, **kw)
    with pytest.raises(ValueError):
        _mat().topk_rows(**kw)
    for tr in (False, True):
        with pytest.raises(ValueError):
            _square().multiply_topk(_square(), transpose=tr, **kw)


def _square():
    from csr_amd import CSR
    return CSR(2, 2, 2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.array([1.0, 2.0]))


def test_structure_only_matrix_is_refused_before_any_library_call(monkeypatch):
    from csr_amd import CSR
    from csr_amd.kernels import hip as K
    monkeypatch.setattr(K, 'to_handle', lambda *a: (_ for _ in ()).throw(AssertionError('library called')))
    s = CSR(2, 2, 2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), None)
    with pytest.raises(ValueError):
        s.topk_rows(1)


def test_null_handle_is_an_error_code():
    from csr_amd._lib import lib, ERR_INVALID, handle_t
    for H in (0, 12345):
        out = handle_t(77)
        assert lib.csrk_topk_rows(H, 3, -INF, 0, ctypes.byref(out)) == ERR_INVALID
        assert b'invalid csrk handle' in lib.csrk_last_error()
        assert out.value == 0
    assert lib.csrk_topk_rows(12345, 3, 0.0, 0, None) == ERR_INVALID


def test_no_cpu_fallback():
    "without a device CSR.topk_rows raises CsrkError naming hip; with one it computes (it never falls back to the CPU)"
    import torch
    from csr_amd._lib import CsrkError
    if torch.cuda.device_count() > 0:
        t = _mat().topk_rows(1)
        assert list(t.rowptrs) == [0, 1, 1, 2] and list(t.colinds) == [3, 1] and list(t.values) == [1.0, 4.0]
        return
    with pytest.raises(CsrkError) as ei:
        _mat().topk_rows(1)
    assert 'hip' in str(ei.value).lower()
    with pytest.raises(CsrkError):
        _square().multiply_topk(_square(), 1)


# ---- the restatement itself ---------------------------------------------------------------------------------------------
NEG_NAN = np.frombuffer(np.array([0xfff8000000000123], np.uint64).tobytes(), np.float64)[0]
ROW = np.array([1, NAN, -0.0, 0.0, INF, -INF, 1, 5, NEG_NAN, 3], np.float64)


def _one_row(v):
    return np.array([0, len(v)], np.int64), np.arange(len(v), dtype=np.int32) * 7, v


def test_restatement_on_hand_written_rows():
    rp, ci, vs = _one_row(ROW)
    orp, oci, ovs = topk_rows_ref(rp, ci, vs, 4)
    assert list(orp) == [0, 4] and list(oci // 7) == [1, 8, 4, 7]            # nan, nan, inf, 5: NaNs tie, the earlier first
    assert ovs.view(np.int64)[1] == NEG_NAN.view(np.int64)                   # the payload travels
    _, oci, ovs = topk_rows_ref(rp, ci, vs, 20)
    assert list(oci // 7) == [1, 8, 4, 7, 9, 0, 6, 2, 3, 5]                   # ... 1 (pos 0), 1 (pos 6), -0.0, 0.0, -inf
    assert np.signbit(ovs[7]) and not np.signbit(ovs[8])
    _, oci, _ = topk_rows_ref(rp, ci, vs, 20, min_value=0.0)
    assert list(oci // 7) == [1, 8, 4, 7, 9, 0, 6, 2, 3]                      # only -inf is dropped; -0.0 passes 0.0
    _, oci, _ = topk_rows_ref(rp, ci, vs, 4, order='storage')
    assert list(oci // 7) == [1, 4, 7, 8]
    _, oci, _ = topk_rows_ref(rp, ci, vs, 20, min_value=INF)
    assert list(oci // 7) == [1, 8, 4]                                        # +inf keeps +Inf and the NaNs
    _, oci, _ = topk_rows_ref(rp, ci, vs, 3, min_value=2.0, order='storage')
    assert list(oci // 7) == [1, 4, 8]
    # ties go to the entry stored earlier
    rp, ci, vs = _one_row(np.array([2.0, 3.0, 2.0, 3.0, 2.0, 3.0], np.float32))
    orp, oci, ovs = topk_rows_ref(rp, ci, vs, 4)
    assert list(oci // 7) == [1, 3, 5, 0] and ovs.dtype == np.float32
    # empty rows, a row shorter than k, and no rows at all
    rp = np.array([0, 0, 2, 2, 3], np.int64)
    orp, oci, ovs = topk_rows_ref(rp, np.array([5, 1, 2], np.int32), np.array([1.0, 2.0, -1.0]), 2, min_value=0.0)
    assert list(orp) == [0, 0, 2, 2, 2] and list(oci) == [1, 5] and list(ovs) == [2.0, 1.0]
    orp, oci, ovs = topk_rows_ref(np.array([0], np.int64), np.zeros(0, np.int32), np.zeros(0), 3)
    assert list(orp) == [0] and len(oci) == 0 and len(ovs) == 0


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_vectorised_restatement_equals_the_row_loop(dtype):
    rng = np.random.default_rng(5)
    lens = np.concatenate([[0, 0, 1, 2, 17, 0, 64, 65, 300], rng.integers(0, 12, 40), [0]])
    rp = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    n = int(rp[-1])
    ci = rng.integers(0, 50, n).astype(np.int32)
    for pattern in ('distinct', 'ties', 'special'):
        if pattern == 'distinct':
            vs = rng.uniform(-1, 1, n)
        elif pattern == 'ties':
            vs = rng.integers(-2, 3, n).astype(np.float64)
        else:
            vs = rng.uniform(-1, 1, n)
            sp = np.array([NAN, NEG_NAN, INF, -INF, 0.0, -0.0, 1e-40, -1e-45])
            at = rng.choice(n, n // 3, replace=False)
            vs[at] = sp[rng.integers(0, len(sp), len(at))]
        vs = vs.astype(dtype)
        for k in (1, 2, 5, 64, 1000):
            for mv in (-INF, 0.0, 0.25, INF):
                for order in ('descending', 'storage'):
                    assert same(topk_rows_vec(rp, ci, vs, k, mv, order), topk_rows_ref(rp, ci, vs, k, mv, order)), \
                        (pattern, k, mv, order)
