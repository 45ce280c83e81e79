"""
csrk_coalesce and csrk_is_canonical on the host side, without a GPU: the entries are declared in include/csrk.h, exported and
in the ctypes table; a malformed `duplicates` is refused with ValueError before any library call; the C entries refuse a null
handle with an error code (no crash) and leave *out = 0; without a device the CSR methods fail loudly instead of computing
on the CPU; from_coo(duplicates=None) is what it was.  The NumPy restatement the GPU tests compare against
(tests/coalesce_ref.py) is checked here against scipy.sparse and against hand-written rows.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from coalesce_ref import coalesce_ref, same, first_difference, is_canonical, route, bits, DUPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i4 = np.int32


def _mat():
    "row 0 repeats column 3"
    from csr_amd import CSR
    return CSR(3, 4, 5, np.array([0, 3, 3, 5], i4), np.array([3, 0, 3, 1, 2], i4), np.array([1.0, -2.0, 0.5, 4.0, 8.0]))


def test_entries_declared_and_exported():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'csrk.h')).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, 'csr_amd', 'libcsrk.so'))
    from csr_amd import _lib
    for name in ('csrk_coalesce', 'csrk_coalesce_last_route', 'csrk_is_canonical'):
        assert re.search(r'CSRK_API\s+int\s+' + name + r'\s*\(', text), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    for i, name in enumerate(('SUM', 'FIRST', 'LAST', 'MAX', 'MIN')):
        assert re.search(r'CSRK_DUP_%s\s*=\s*%d\b' % (name, i), text), name
        assert getattr(_lib, 'DUP_' + name) == i


def test_python_names_and_codes():
    from csr_amd.kernels import hip as K
    from csr_amd import CSR
    assert [K.coalesce_args(d) for d in DUPS] == [0, 1, 2, 3, 4]
    for name in ('coalesce', 'coalesce_last_route', 'is_canonical'):
        assert callable(getattr(K, name))
    for name in ('coalesce', 'sum_duplicates', 'is_canonical'):
        assert callable(getattr(CSR, name))


def _forbid(monkeypatch):
    from csr_amd.kernels import hip as K
    from csr_amd import _lib

    def forbidden(*a, **kw):
        raise AssertionError('library called')
    for name in ('csrk_coalesce', 'csrk_is_canonical', 'csrk_create', 'csrk_export', 'csrk_from_coo', 'csrk_combine'):
        monkeypatch.setattr(_lib.lib, name, forbidden)
    monkeypatch.setattr(K, 'to_handle', forbidden)
    return K


BAD = {
    'unknown word': 'mean',
    'upper case': 'SUM',
    'code': 0,
    'None': None,
    'bytes': b'sum',
    'bool': True,
    'list': ['sum'],
    'empty': '',
}


@pytest.mark.parametrize('case', sorted(BAD))
def test_bad_duplicates_raise_before_any_library_call(case, monkeypatch):
    K = _forbid(monkeypatch)
    bad = BAD[case]
    with pytest.raises(ValueError):
        K.coalesce(K.hip_h(12345, 3, 4, 5), bad)
    with pytest.raises(ValueError):
        _mat().coalesce(bad)
    if bad is not None:                     # from_coo: None is "keep the repeats", the default
        from csr_amd import CSR
        with pytest.raises(ValueError):
            CSR.from_coo(np.array([0, 0]), np.array([1, 1]), np.array([1.0, 2.0]), duplicates=bad)


def test_null_handle_is_an_error_code():
    from csr_amd._lib import lib, ERR_INVALID, OK, handle_t
    for H in (0, 12345):
        for dup in range(5):
            out = handle_t(77)
            assert lib.csrk_coalesce(H, dup, ctypes.byref(out)) == ERR_INVALID
            assert b'invalid csrk handle' in lib.csrk_last_error()
            assert out.value == 0
        ok, row = ctypes.c_int(7), ctypes.c_int32(7)
        assert lib.csrk_is_canonical(H, ctypes.byref(ok), ctypes.byref(row)) == ERR_INVALID
        assert b'invalid csrk handle' in lib.csrk_last_error()
    assert lib.csrk_coalesce(12345, 0, None) == ERR_INVALID
    assert lib.csrk_is_canonical(12345, None, None) == ERR_INVALID
    assert lib.csrk_coalesce_last_route(None) == ERR_INVALID
    r = ctypes.c_int(9)
    assert lib.csrk_coalesce_last_route(ctypes.byref(r)) == OK and r.value == 0      # after the failures above


def test_no_cpu_fallback():
    "without a device the CSR methods raise CsrkError; with one they compute (they never fall back to the CPU)"
    import torch
    from csr_amd import CSR
    from csr_amd._lib import CsrkError
    a = _mat()
    coo = (np.array([0, 0, 1]), np.array([1, 1, 0]), np.array([1.0, 2.0, 4.0]))
    calls = (lambda: a.coalesce(), lambda: a.coalesce('max'), lambda: a.sum_duplicates(), lambda: a.is_canonical(),
             lambda: CSR.from_coo(*coo, duplicates='sum'))
    if torch.cuda.device_count() > 0:
        t = a.coalesce()
        assert list(t.rowptrs) == [0, 2, 2, 4] and list(t.colinds) == [0, 3, 1, 2] and list(t.values) == [-2.0, 1.5, 4.0, 8.0]
        assert a.is_canonical(with_row=True) == (False, 0) and t.is_canonical()
        return
    for call in calls:
        with pytest.raises(CsrkError) as ei:
            call()
        assert 'hip' in str(ei.value).lower()


def test_from_coo_without_duplicates_is_what_it_was():
    "duplicates=None: the stable counting sort by row, every repeated pair kept, no device needed"
    from csr_amd import CSR
    rng = np.random.default_rng(5)
    rows, cols = rng.integers(0, 9, 200), rng.integers(0, 7, 200)
    vals = rng.standard_normal(200).astype(np.float32)
    order = np.argsort(rows, kind='stable')
    rp = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=9))))
    for kw in ({}, {'duplicates': None}):
        for v in (vals, None):
            m = CSR.from_coo(rows, cols, v, shape=(9, 7), **kw)
            assert (m.nrows, m.ncols, m.nnz) == (9, 7, 200)
            assert m.rowptrs.dtype == np.int32 and np.array_equal(m.rowptrs, rp)
            assert m.colinds.dtype == np.int32 and np.array_equal(m.colinds, cols[order])
            if v is None:
                assert m.values is None
            else:
                assert m.values.dtype == np.float32 and np.array_equal(bits(m.values), bits(vals[order]))
    m = CSR.from_coo(np.array([0, 1]), np.array([1, 0]), np.array([1.0, 2.0]))       # positional, as ever
    assert (m.nrows, m.ncols) == (2, 2)


# ---- the restatement itself ---------------------------------------------------------------------------------------------
def test_restatement_against_scipy():
    "integer-valued matrices: the sums are exact in any order, so SciPy's sum_duplicates is the same numbers"
    import scipy.sparse as sps
    rng = np.random.default_rng(23)
    for nr, nc, n in ((1, 1, 5), (5, 7, 60), (40, 30, 500), (30, 3, 400), (17, 64, 100), (6, 9, 0)):
        rows, cols = rng.integers(0, nr, n), rng.integers(0, nc, n)
        vals = (rng.integers(1, 6, n) * rng.choice([-1, 1], n)).astype(np.float64)
        order = np.argsort(rows, kind='stable')
        rp = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=nr)))).astype(i4)
        for dt in (np.float64, np.float32):
            A = (rp, cols[order].astype(i4), vals[order].astype(dt))
            got = coalesce_ref(A, 'sum')
            S = sps.csr_matrix((A[2].copy(), A[1].copy(), A[0].copy()), shape=(nr, nc))
            S.sum_duplicates()                                  # sorts and merges in place, keeps the exact zeros
            exp = (S.indptr.astype(i4), S.indices.astype(i4), S.data.astype(dt))
            assert same(got, exp, 'sum'), first_difference(got, exp, 'sum')
            T = sps.coo_matrix((vals, (rows, cols)), shape=(nr, nc)).tocsr()
            T.sort_indices()
            assert np.array_equal(got[0], T.indptr) and np.array_equal(got[1], T.indices) and np.array_equal(got[2], T.data)
            # every other rule has the same pattern, and a structure-only matrix just that pattern
            for dup in DUPS:
                r = coalesce_ref(A, dup)
                assert np.array_equal(r[0], exp[0]) and np.array_equal(r[1], exp[1]) and r[2].dtype == dt
                assert is_canonical(r[0], r[1]) == (True, None)
                s = coalesce_ref((A[0], A[1], None), dup)
                assert s[2] is None and np.array_equal(s[1], exp[1])


def test_restatement_on_hand_written_rows():
    nan = np.nan
    # row 0: 9 2 9 0 2 9 (unsorted, repeats), row 1 empty, row 2 ends with column 1 and row 3 starts with it
    rp = np.array([0, 6, 6, 8, 10], i4)
    ci = np.array([9, 2, 9, 0, 2, 9, 1, 1, 1, 5], i4)
    vs = np.array([1, 2, 3, 4, 5, 7, 8, 16, 32, 64], np.float32)
    exp = {
        'sum': [4, 7, 11, 24, 32, 64], 'first': [4, 2, 1, 8, 32, 64], 'last': [4, 5, 7, 16, 32, 64],
        'max': [4, 5, 7, 16, 32, 64], 'min': [4, 2, 1, 8, 32, 64],
    }
    assert is_canonical(rp, ci) == (False, 0) and route(rp, ci) == 2
    for dup in DUPS:
        r = coalesce_ref((rp, ci, vs), dup)
        assert r[0].dtype == i4 and list(r[0]) == [0, 3, 3, 4, 6], dup           # rows 2 and 3 never merge
        assert r[1].dtype == i4 and list(r[1]) == [0, 2, 9, 1, 1, 5], dup
        assert r[2].dtype == np.float32 and list(r[2]) == exp[dup], dup
        s = coalesce_ref((rp, ci, None), dup)
        assert s[2] is None and list(s[1]) == [0, 2, 9, 1, 1, 5]
    assert route(np.array([0, 3, 4], i4), np.array([1, 1, 2, 1], i4)) == 1
    assert route(np.array([0, 2, 3], i4), np.array([1, 2, 1], i4)) == 0
    assert is_canonical(np.array([0, 2, 4], i4), np.array([0, 1, 3, 3], i4)) == (False, 1)

    def one(vals, dup, dt=np.float64):
        "one group: a single row, a single column"
        v = np.array(vals, dt)
        r = coalesce_ref((np.array([0, len(v)], i4), np.zeros(len(v), i4), v), dup)
        assert list(r[0]) == [0, 1] and list(r[1]) == [0] and r[2].dtype == dt
        return r[2][0]
    # the order of addition is the storage order, rounded at every step in the values' dtype
    assert one([1e16, 1.0, 1.0], 'sum') == 1e16 and one([1.0, 1.0, 1e16], 'sum') == 1e16 + 2
    assert one([2.0 ** 24, 1, 1], 'sum', np.float32) == 2.0 ** 24 and one([1, 1, 2.0 ** 24], 'sum', np.float32) == 2.0 ** 24 + 2
    # signed zeros: the sum does not start at +0.0
    assert np.signbit(one([-0.0], 'sum')) and np.signbit(one([-0.0, -0.0], 'sum')) and not np.signbit(one([0.0, -0.0], 'sum'))
    assert np.isnan(one([np.inf, -np.inf], 'sum')) and one([3.0, -3.0], 'sum') == 0.0
    # max: the earliest of the largest; NaN above +Inf; +-0 tie
    assert np.isnan(one([1.0, nan, np.inf], 'max')) and one([1.0, np.inf, 2.0], 'max') == np.inf
    assert np.signbit(one([-0.0, 0.0], 'max')) and not np.signbit(one([0.0, -0.0], 'max'))
    # min: the latest of the smallest; a NaN only when every member is one
    assert one([nan, 2.0, nan, 5.0], 'min') == 2.0 and np.isnan(one([nan, nan], 'min'))
    assert not np.signbit(one([-0.0, 0.0], 'min')) and np.signbit(one([0.0, -0.0], 'min'))
    # bits: quiet-NaN payloads and a float32 subnormal come through first / last / max / min and a group of one
    p1, p2 = np.array([0x7ff8000000000123, 0xfff800000000beef], np.uint64).view(np.float64)
    for dup, want in (('first', p1), ('last', p2), ('max', p1), ('min', p2)):
        got = coalesce_ref((np.array([0, 2], i4), np.zeros(2, i4), np.array([p1, p2])), dup)[2]
        assert bits(got)[0] == bits(np.array([want]))[0], dup
    q = np.array([0x7fc00abc, 0x00000001], np.uint32).view(np.float32)
    for dup in DUPS:
        got = coalesce_ref((np.array([0, 1, 2], i4), np.zeros(2, i4), q), dup)[2]
        assert list(bits(got)) == list(bits(q)), dup
    # same(): any NaN for a NaN under 'sum' only
    a = (np.array([0, 1], i4), np.zeros(1, i4), np.array([nan]))
    b = (a[0], a[1], a[2].copy())
    b[2].view(np.uint64)[0] ^= np.uint64(0x8000000000000001)        # another NaN
    assert same(a, b, 'sum') and not same(a, b, 'max') and 'value 0' in first_difference(a, b, 'max')
    # no rows, no entries
    e = (np.array([0], i4), np.zeros(0, i4), np.zeros(0, np.float32))
    for dup in DUPS:
        r = coalesce_ref(e, dup)
        assert list(r[0]) == [0] and len(r[1]) == 0 and r[2].dtype == np.float32 and len(r[2]) == 0
        r = coalesce_ref((np.zeros(4, i4), np.zeros(0, i4), None), dup)
        assert list(r[0]) == [0, 0, 0, 0] and r[2] is None
