"""
Per-row Gram matrices on the host side, without a GPU: the three entries are declared in include/csrk.h, exported and in
the ctypes table; every malformed request is refused with ValueError before any library call; the C entries refuse a
null handle with an error code (no crash); without a device CSR.gram_rows fails loudly instead of computing on the CPU;
and the references of tests/gram_ref.py check themselves.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import gram_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('csrk_gram_rows', 'csrk_gram_rows_device', 'csrk_gram_limits')


def _mat():
    from csr_amd import CSR
    return CSR(3, 4, 4, np.array([0, 2, 2, 4], np.int32), np.array([3, 0, 1, 1], np.int32), np.array([1.0, -2.0, 0.5, 4.0]))


def test_entries_declared_exported_and_in_the_table():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'csrk.h')).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, 'csr_amd', 'libcsrk.so'))
    from csr_amd import _lib
    from csr_amd.kernels import raw
    for name in NAMES:
        assert re.search(r'CSRK_API\s+int\s+' + name + r'\s*\(', text), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert raw.address(name)


def test_limits_need_no_device():
    from csr_amd.kernels import hip as K
    lim = K.gram_limits()
    assert len(lim) == 5 and lim[0] >= 128 and lim[1] >= 1
    assert 1 <= lim[2] < lim[3] < lim[4] <= lim[0]          # the k classes, ascending
    from csr_amd._lib import lib, ERR_INVALID
    assert lib.csrk_gram_limits(None, 1) == ERR_INVALID
    two = (ctypes.c_int64 * 2)(-1, -1)
    assert lib.csrk_gram_limits(two, 1) == 0 and two[0] == lim[0] and two[1] == -1


def _bad_cases():
    V = np.ones((4, 5))
    return {
        'V rows': dict(V=np.ones((5, 5))),
        '1-D V': dict(V=np.ones(4)),
        'k = 0': dict(V=np.ones((4, 0))),
        'integer V': dict(V=np.ones((4, 5), np.int64)),
        'float16 V': dict(V=np.ones((4, 5), np.float16)),
        'base shape': dict(V=V, base=np.ones((5, 4))),
        'base 1-D': dict(V=V, base=np.ones(25)),
        'base dtype': dict(V=V, base=np.ones((5, 5), np.float32)),
        'rows past the end': dict(V=V, rows=(0, 4)),
        'rows negative': dict(V=V, rows=(-1, 2)),
        'rows reversed': dict(V=V, rows=(2, 1)),
        'rows not a pair': dict(V=V, rows=(1,)),
        'rows not integers': dict(V=V, rows=(0.0, 2.0)),
    }


@pytest.mark.parametrize('case', sorted(_bad_cases()))
def test_bad_requests_raise_before_any_library_call(case, monkeypatch):
    from csr_amd.kernels import hip as K
    from csr_amd import _lib

    def forbidden(*a, **kw):
        raise AssertionError('library called')
    for name in ('csrk_gram_rows', 'csrk_gram_rows_device', 'csrk_create'):
        monkeypatch.setattr(_lib.lib, name, forbidden)
    monkeypatch.setattr(K, 'to_handle', forbidden)
    kw = dict(_bad_cases()[case])
    V = kw.pop('V')
    h = K.hip_h(12345, 3, 4, 4)
    with pytest.raises(ValueError):
        K.gram_rows(h, V, **kw)
    with pytest.raises(ValueError):
        _mat().gram_rows(V, **kw)


def test_output_over_budget_names_the_rows_that_fit(monkeypatch):
    from csr_amd.kernels import hip as K
    from csr_amd import _lib

    def forbidden(*a, **kw):
        raise AssertionError('library called')
    for name in ('csrk_gram_rows', 'csrk_create'):
        monkeypatch.setattr(_lib.lib, name, forbidden)
    monkeypatch.setattr(K, 'to_handle', forbidden)
    V = np.ones((4, 5))
    with pytest.raises(ValueError, match=r'at most 2 rows fit'):
        _mat().gram_rows(V, max_bytes=2 * 5 * 5 * 8 + 199)       # 3 rows asked for, 2 fit
    with pytest.raises(ValueError, match=r'at most 0 rows fit'):
        _mat().gram_rows(V, rows=(1, 2), max_bytes=199)
    # the default budget is 4 GiB: 2^20 rows at k = 64 are 32 GiB
    from csr_amd import CSR
    big = CSR(1 << 20, 4, 0, np.zeros((1 << 20) + 1, np.int32), np.zeros(0, np.int32), None)
    with pytest.raises(ValueError, match=r'at most 131072 rows fit'):
        big.gram_rows(np.ones((4, 64)))


def test_null_handle_is_an_error_code():
    from csr_amd._lib import lib, ERR_INVALID, VAL_F64
    V = np.ones((4, 2))
    out = np.full(12, 7.0)
    for H in (0, 12345):
        assert lib.csrk_gram_rows(H, 0, 3, V.ctypes.data, 2, 2, VAL_F64, 0, None, out.ctypes.data) == ERR_INVALID
        assert b'invalid csrk handle' in lib.csrk_last_error()
        assert lib.csrk_gram_rows_device(H, 0, 3, None, 2, 2, VAL_F64, 0, None, None, None) == ERR_INVALID
        assert b'invalid csrk handle' in lib.csrk_last_error()
    assert np.all(out == 7.0)


def test_no_cpu_fallback():
    "without a device CSR.gram_rows raises CsrkError naming hip; with one it computes (it never falls back to the CPU)"
    import torch
    from csr_amd._lib import CsrkError
    V = np.arange(8.0).reshape(4, 2) + 1.0
    m = _mat()
    if torch.cuda.device_count() > 0:
        got = m.gram_rows(V, weighted=True)
        assert np.array_equal(got, R.gram_exact(m.rowptrs, m.colinds, m.values, V, True))
        return
    with pytest.raises(CsrkError) as ei:
        m.gram_rows(V)
    assert 'hip' in str(ei.value).lower()


# ---- the references check themselves ----------------------------------------------------------------------

def _small():
    rng = np.random.default_rng(5)
    rp = np.array([0, 3, 3, 7, 8], np.int64)
    ci = np.array([2, 0, 2, 5, 1, 1, 4, 3], np.int32)          # unsorted, column 2 and column 1 repeated
    vs = rng.standard_normal(8)
    V = rng.standard_normal((6, 3))
    return rp, ci, vs, V


def test_ref_symmetry_empty_row_and_base():
    rp, ci, vs, V = _small()
    base = np.arange(9.0).reshape(3, 3) + 0.25                  # asymmetric: only its lower triangle counts
    for scale in (False, True):
        G = R.gram_exact(rp, ci, vs, V, scale, base)
        assert np.array_equal(G, G.transpose(0, 2, 1))
        want = np.tril(base) + np.tril(base, -1).T
        assert np.array_equal(G[1], want)                       # the empty row: base mirrored
        G0 = R.gram_exact(rp, ci, vs, V, scale)
        assert np.array_equal(G0[1], np.zeros((3, 3))) and not np.signbit(G0[1]).any()
        Gn, M = R.gram_numpy(rp, ci, vs, V, scale, base)
        lens = np.diff(rp)[:, None, None]
        assert np.all(np.abs(G - Gn) <= (lens + 2) * 2.0 ** -52 * M)
        assert np.array_equal(R.gram_exact(rp, ci, vs, V, scale, base, rows=(2, 4)), G[2:4])
    # a row of one entry with scale = 0 and no base: fma(v_p, v_q, +0.0) = round(v_p v_q)
    G = R.gram_exact(rp, ci, None, V, True)
    v = V[3]
    assert np.array_equal(G[3], np.tril(np.outer(v, v)) + np.tril(np.outer(v, v), -1).T)


def test_ref_hand_computed_case_where_fusing_matters():
    """
    k = 2, one row of one entry, V[0] = [a, 3] with a = 1 + 2^-30, so a a = 1 + 2^-29 + 2^-60 exactly, and
    base[0][0] = -(1 + 2^-29).  Fused: fma(a, a, base[0][0]) = 2^-60, exactly.  Two roundings: round(a a) = 1 + 2^-29
    (2^-60 is far below half an ulp of 1), plus base[0][0] = 0.0.
    """
    a = 1.0 + 2.0 ** -30
    rp, ci = np.array([0, 1], np.int32), np.array([0], np.int32)
    V = np.array([[a, 3.0]])
    base = np.array([[-(1.0 + 2.0 ** -29), 99.0], [0.5, 0.25]])
    G = R.gram_exact(rp, ci, None, V, False, base)
    assert G[0, 0, 0] == 2.0 ** -60
    assert G[0, 1, 0] == G[0, 0, 1] == 3.0 * a + 0.5            # exact in float64; base[0][1] = 99 is never read
    assert G[0, 1, 1] == 9.25
    G2 = R.gram_two_rounding(rp, ci, None, V, False, base)
    assert G2[0, 0, 0] == 0.0
    # with a weight: t = round(w a) first.  w = 3: 3 a = 3 + 3 * 2^-30 is exact; fma(3 a, a, -3 (1 + 2^-29)) = 3 * 2^-60
    vs = np.array([3.0])
    base3 = np.array([[-3.0 * (1.0 + 2.0 ** -29), 0.0], [0.0, 0.0]])
    assert R.gram_exact(rp, ci, vs, V, True, base3)[0, 0, 0] == 3.0 * 2.0 ** -60
    assert R.gram_two_rounding(rp, ci, vs, V, True, base3)[0, 0, 0] == 0.0


def test_ref_tells_a_fused_chain_from_a_two_rounding_one():
    rng = np.random.default_rng(11)
    n, k = 40, 5
    rp = np.array([0, n], np.int64)
    ci = rng.integers(0, 30, n).astype(np.int32)
    V = rng.standard_normal((30, k))
    vs = rng.standard_normal(n)
    a, b = R.gram_exact(rp, ci, vs, V, True), R.gram_two_rounding(rp, ci, vs, V, True)
    assert np.count_nonzero(a != b) >= k                       # most elements differ in the last place
    assert np.allclose(a, b, rtol=1e-12, atol=1e-13)


def test_ref_positions():
    rp, ci, vs, V = _small()
    V = V.copy()
    V[5] = [np.nan, np.inf, -np.inf]                            # column 5: row 2 alone holds it
    c = R.gram_positions(rp, ci, vs, V, False)
    assert not c[0].any() and not c[1].any() and not c[3].any()
    # row 2: outer products with NaN in position 0, +Inf^2 = +Inf at (1,1), +Inf * -Inf = -Inf at (2,1), -Inf^2 = +Inf at (2,2)
    assert c[2][0, 0] == R.NAN and c[2][1, 0] == R.NAN and c[2][2, 0] == R.NAN
    assert c[2][1, 1] == R.PINF and c[2][2, 1] == R.NINF and c[2][1, 2] == R.NINF and c[2][2, 2] == R.PINF
