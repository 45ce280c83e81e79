"""
SDDMM on the host side, without a GPU: both entries are declared in include/csrk.h and exported, every malformed panel
is refused with ValueError before any library call, the C entries refuse a null handle with an error code (no crash),
and without a device CSR.sddmm fails loudly instead of computing on the CPU.
"""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mat():
    from csr_amd import CSR
    return CSR(3, 4, 4, np.array([0, 2, 2, 4], np.int32), np.array([3, 0, 1, 1], np.int32), np.array([1.0, -2.0, 0.5, 4.0]))


def test_entries_declared_and_exported():
    import re
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'csrk.h')).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, 'csr_amd', 'libcsrk.so'))
    for name in ('csrk_sddmm', 'csrk_sddmm_device'):
        assert re.search(r'CSRK_API\s+int\s+' + name + r'\s*\(', text), name
        assert hasattr(lib, name), name
    from csr_amd import _lib
    assert 'csrk_sddmm' in _lib.SIGNATURES and 'csrk_sddmm_device' in _lib.SIGNATURES


def _bad_cases():
    U, V = np.ones((3, 5)), np.ones((4, 5))
    return {
        'U rows': (np.ones((2, 5)), V),
        'V rows': (U, np.ones((5, 5))),
        'k mismatch': (U, np.ones((4, 6))),
        'mixed f32/f64': (U.astype(np.float32), V),
        '1-D panel': (np.ones(3), V),
        'k = 0': (np.ones((3, 0)), np.ones((4, 0))),
    }


@pytest.mark.parametrize('case', sorted(_bad_cases()))
def test_bad_panels_raise_before_any_library_call(case, monkeypatch):
    from csr_amd.kernels import hip as K
    from csr_amd import _lib

    def forbidden(*a, **kw):
        raise AssertionError('library called')
    # a handle that never touched the device, and every library entry the two paths could reach stubbed out
    for name in ('csrk_sddmm', 'csrk_create', 'csrk_sddmm_device'):
        monkeypatch.setattr(_lib.lib, name, forbidden)
    monkeypatch.setattr(K, 'to_handle', forbidden)
    U, V = _bad_cases()[case]
    h = K.hip_h(12345, 3, 4, 4)
    with pytest.raises(ValueError):
        K.sddmm(h, U, V)
    with pytest.raises(ValueError):
        _mat().sddmm(U, V)


def test_null_handle_is_an_error_code():
    from csr_amd._lib import lib, ERR_INVALID, VAL_F64
    U = np.ones((3, 2))
    out = np.zeros(4)
    for H in (0, 12345):
        assert lib.csrk_sddmm(H, U.ctypes.data, 2, U.ctypes.data, 2, 2, VAL_F64, 0, out.ctypes.data) == ERR_INVALID
        assert b'invalid csrk handle' in lib.csrk_last_error()
        assert lib.csrk_sddmm_device(H, None, 2, None, 2, 2, VAL_F64, 0, None, None) == ERR_INVALID
        assert b'invalid csrk handle' in lib.csrk_last_error()


def test_no_cpu_fallback():
    "without a device CSR.sddmm raises CsrkError naming hip; with one it computes (it never falls back to the CPU)"
    import torch
    from csr_amd._lib import CsrkError
    U, V = np.arange(6.0).reshape(3, 2), np.arange(8.0).reshape(4, 2)
    if torch.cuda.device_count() > 0:
        got = _mat().sddmm(U, V).values
        assert np.array_equal(got, np.array([U[0] @ V[3], U[0] @ V[0], U[2] @ V[1], U[2] @ V[1]]))
        return
    with pytest.raises(CsrkError) as ei:
        _mat().sddmm(U, V)
    assert 'hip' in str(ei.value).lower()
