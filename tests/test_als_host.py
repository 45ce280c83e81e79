"""
The ALS half-step on the host side, without a GPU: the five entries are declared in include/csrk.h, exported and in the
ctypes table; every malformed request is refused with ValueError before any library call; the C entries refuse a null
handle with an error code (no crash, nothing written); without a device CSR.als_rows and solve_blocks fail loudly instead
of computing on the CPU; and the references of tests/als_ref.py check themselves.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import als_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('csrk_solve_blocks', 'csrk_solve_blocks_device', 'csrk_als_rows', 'csrk_als_rows_device', 'csrk_als_limits')


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
    for n, name in enumerate(('CSRK_ALS_RHS_ONES', 'CSRK_ALS_RHS_VALUES', 'CSRK_ALS_RHS_ONE_PLUS')):
        assert re.search(name + r'\s*=\s*%d\b' % n, text), name
    assert (_lib.ALS_RHS_ONES, _lib.ALS_RHS_VALUES, _lib.ALS_RHS_ONE_PLUS) == (0, 1, 2)


def test_limits_need_no_device():
    from csr_amd.kernels import hip as K
    lim = K.als_limits()
    assert len(lim) == 5 and lim[0] >= 128 and lim[1] >= 1
    assert 1 <= lim[2] < lim[3] < lim[4] <= lim[0]          # the k classes, ascending
    assert lim[0] <= K.gram_limits()[0]                     # never above the Gram limit
    from csr_amd._lib import lib, ERR_INVALID
    assert lib.csrk_als_limits(None, 1) == ERR_INVALID
    two = (ctypes.c_int64 * 2)(-1, -1)
    assert lib.csrk_als_limits(two, 1) == 0 and two[0] == lim[0] and two[1] == -1


def _bad_als():
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
        'rhs unknown': dict(V=V, rhs='value'),
        'rhs a code': dict(V=V, rhs=1),
        'rhs None': dict(V=V, rhs=None),
        'ridge per row': dict(V=V, reg=np.ones(3)),
        'ridge a string': dict(V=V, reg='0.1'),
        'ridge None': dict(V=V, reg=None),
        'ridge complex': dict(V=V, reg=1j),
    }


def _forbid(monkeypatch, names):
    from csr_amd.kernels import hip as K
    from csr_amd import _lib

    def forbidden(*a, **kw):
        raise AssertionError('library called')
    for name in names:
        monkeypatch.setattr(_lib.lib, name, forbidden)
    monkeypatch.setattr(K, 'to_handle', forbidden)
    return K


@pytest.mark.parametrize('case', sorted(_bad_als()))
def test_bad_als_requests_raise_before_any_library_call(case, monkeypatch):
    K = _forbid(monkeypatch, ('csrk_als_rows', 'csrk_als_rows_device', 'csrk_gram_rows', 'csrk_create'))
    kw = dict(_bad_als()[case])
    V = kw.pop('V')
    h = K.hip_h(12345, 3, 4, 4)
    with pytest.raises(ValueError):
        K.als_rows(h, V, False, kw.get('rhs', 'values'), kw.get('base'), kw.get('reg', 0.0), kw.get('rows'))
    ckw = {a: b for a, b in kw.items() if a != 'reg'}
    if 'reg' in kw:
        ckw['reg_per_entry'] = kw['reg']
    with pytest.raises(ValueError):
        _mat().als_rows(V, **ckw)


def _bad_solve():
    G, b = np.ones((3, 4, 4)), np.ones((3, 4))
    return {
        'G 2-D': (np.ones((4, 4)), np.ones(4)),
        'G not square': (np.ones((3, 4, 5)), b),
        'G float32': (G.astype(np.float32), b),
        'G integer': (G.astype(np.int64), b),
        'k = 0': (np.ones((3, 0, 0)), np.ones((3, 0))),
        'b 1-D': (G, np.ones(12)),
        'b rows': (G, np.ones((2, 4))),
        'b columns': (G, np.ones((3, 5))),
        'b float32': (G, b.astype(np.float32)),
        'b 3-D': (G, np.ones((3, 4, 1))),
    }


@pytest.mark.parametrize('case', sorted(_bad_solve()))
def test_bad_solve_requests_raise_before_any_library_call(case, monkeypatch):
    K = _forbid(monkeypatch, ('csrk_solve_blocks', 'csrk_solve_blocks_device'))
    G, b = _bad_solve()[case]
    with pytest.raises(ValueError):
        K.solve_blocks(G, b)


def test_null_handle_is_an_error_code():
    from csr_amd._lib import lib, ERR_INVALID, VAL_F64, ALS_RHS_VALUES
    V = np.ones((4, 2))
    out, info = np.full(6, 7.0), np.full(3, 7, np.int32)
    for H in (0, 12345):
        assert lib.csrk_als_rows(H, 0, 3, V.ctypes.data, 2, 2, VAL_F64, 0, ALS_RHS_VALUES, None, 0.0, out.ctypes.data, 2,
                                 info.ctypes.data) == ERR_INVALID
        assert b'invalid csrk handle' in lib.csrk_last_error()
        assert lib.csrk_als_rows_device(H, 0, 3, None, 2, 2, VAL_F64, 0, ALS_RHS_VALUES, None, 0.0, None, 2, None, None) == ERR_INVALID
        assert b'invalid csrk handle' in lib.csrk_last_error()
    assert np.all(out == 7.0) and np.all(info == 7)


def test_solve_blocks_refuses_without_touching_anything():
    "the argument checks of csrk_solve_blocks come before any device work: they need no GPU"
    from csr_amd._lib import lib, ERR_INVALID, ERR_UNSUPPORTED
    from csr_amd.kernels import hip as K
    G, b = np.ones((2, 3, 3)), np.ones((2, 3))
    x, info = np.full((2, 3), 7.0), np.full(2, 7, np.int32)
    g, bb, xx, ii = G.ctypes.data, b.ctypes.data, x.ctypes.data, info.ctypes.data
    for name, args in {'n < 0': (-1, 3, g, bb, 3, xx, 3, ii), 'k = 0': (2, 0, g, bb, 3, xx, 3, ii), 'ldb < k': (2, 3, g, bb, 2, xx, 3, ii),
                       'ldx < k': (2, 3, g, bb, 3, xx, 2, ii), 'NULL G': (2, 3, None, bb, 3, xx, 3, ii),
                       'NULL b': (2, 3, g, None, 3, xx, 3, ii), 'NULL x': (2, 3, g, bb, 3, None, 3, ii)}.items():
        assert lib.csrk_solve_blocks(*args) == ERR_INVALID, name
        assert lib.csrk_solve_blocks_device(*args, None) == ERR_INVALID, name
        assert lib.csrk_last_error(), name
    k = K.als_limits()[0] + 1
    assert lib.csrk_solve_blocks(2, k, g, bb, k, xx, k, ii) == ERR_UNSUPPORTED
    assert lib.csrk_solve_blocks_device(2, k, g, bb, k, xx, k, ii, None) == ERR_UNSUPPORTED
    assert lib.csrk_solve_blocks(0, 3, None, None, 3, None, 3, None) == 0          # no systems: fine, NULL pointers and all
    assert lib.csrk_solve_blocks_device(0, 3, None, None, 3, None, 3, None, None) == 0
    assert np.all(x == 7.0) and np.all(info == 7)


def test_no_cpu_fallback():
    "without a device als_rows and solve_blocks raise CsrkError naming hip; with one they compute (never on the CPU)"
    import torch
    from csr_amd._lib import CsrkError
    from csr_amd.kernels import hip as K
    V = np.arange(8.0).reshape(4, 2) + 1.0
    base = np.eye(2)
    m = _mat()
    G, b = np.array([[[4.0, 0.0], [2.0, 3.0]]]), np.array([[2.0, 5.0]])
    if torch.cuda.device_count() > 0:
        got = m.als_rows(V, base=base)
        want = R.als_exact(m.rowptrs, m.colinds, m.values, V, False, 'values', base)[0]
        assert np.array_equal(got, want)
        x, info = K.solve_blocks(G, b)
        assert np.array_equal(x, [[-0.5, 2.0]]) and info[0] == 0
        return
    with pytest.raises(CsrkError) as ei:
        m.als_rows(V, base=base)
    assert 'hip' in str(ei.value).lower()
    with pytest.raises(CsrkError) as ei:
        K.solve_blocks(G, b)
    assert 'hip' in str(ei.value).lower()


# ---- the references check themselves ----------------------------------------------------------------------

def test_ref_two_by_two_by_hand():
    """
    G = [[4, .], [2, 3]], b = [2, 5]:  d0 = 4, r0 = 1/4, L10 = 1/2, d1 = 3 - 1/2 * 2 = 2, r1 = 1/2;  z = [2, 5 - 1/2 * 2] =
    [2, 4];  y = [1/2, 2];  x1 = 2, x0 = 1/2 - 1/2 * 2 = -1/2.  (4 * -1/2 + 2 * 2 = 2, 2 * -1/2 + 3 * 2 = 5.)
    """
    x, info, L, d = R.ldl_exact([[4.0, 99.0], [2.0, 3.0]], [2.0, 5.0], factors=True)
    assert info == 0 and d == [4.0, 2.0] and L[1][0] == 0.5
    assert np.array_equal(x, [-0.5, 2.0])
    assert np.array_equal(R.ldl_two_rounding([[4.0, 99.0], [2.0, 3.0]], [2.0, 5.0])[0], [-0.5, 2.0])
    x1, i1 = R.ldl_exact([[0.5]], [3.0])
    assert x1[0] == 6.0 and i1 == 0


def test_ref_hand_computed_case_where_fusing_matters():
    """
    a = 1 + 2^-30, G = [[1, .], [a, 1 + 2^-29 + 2^-52]]:  L10 = a, a a = 1 + 2^-29 + 2^-60 exactly, so the fused
    d1 = fma(-a, a, G11) = 2^-52 - 2^-60, while round(a a) = 1 + 2^-29 and the two-rounding d1 = 2^-52.
    """
    a = 1.0 + 2.0 ** -30
    G = [[1.0, 7.0], [a, 1.0 + 2.0 ** -29 + 2.0 ** -52]]
    x, info, L, d = R.ldl_exact(G, [0.0, 1.0], factors=True)
    assert L[1][0] == a and d[1] == 2.0 ** -52 - 2.0 ** -60 and info == 0
    x2, info2, L2, d2 = R.ldl_two_rounding(G, [0.0, 1.0], factors=True)
    assert d2[1] == 2.0 ** -52 and info2 == 0
    assert x[1] == 1.0 / (2.0 ** -52 - 2.0 ** -60) and x2[1] == 2.0 ** 52 and x[1] != x2[1]


def test_ref_multiplies_by_the_rounded_reciprocal():
    "L = round(C * round(1 / d)), not C / d: 39 and 38 tell them apart, as do 291 of the 1521 pairs of integers below 40"
    x, info, L, d = R.ldl_exact([[38.0, 0.0], [39.0, 50.0]], [1.0, 1.0], factors=True)
    assert L[1][0] == 39.0 * (1.0 / 38.0) and L[1][0] != 39.0 / 38.0
    n = sum(1 for a in range(1, 40) for dd in range(1, 40) if float(a) * (1.0 / float(dd)) != float(a) / float(dd))
    assert n == 291


def test_ref_never_reads_the_upper_triangle():
    rng = np.random.default_rng(3)
    k = 6
    A = rng.standard_normal((9, k))
    G = A.T @ A + 0.5 * np.eye(k)
    b = rng.standard_normal(k)
    x, info = R.ldl_exact(G, b)
    Gn = G.copy()
    Gn[np.triu_indices(k, 1)] = np.nan
    xn, infon = R.ldl_exact(Gn, b)
    assert info == 0 and infon == 0 and np.array_equal(x, xn)
    xs = R.solve_numpy(Gn[None], b[None])[0][0]
    assert np.allclose(x, xs, rtol=1e-10, atol=1e-12)
    # most elements differ in the last place from the two-rounding chain: the exact reference tells them apart
    big = rng.standard_normal((60, 12))
    Gb, bb = big.T @ big + np.eye(12), rng.standard_normal(12)
    assert np.count_nonzero(R.ldl_exact(Gb, bb)[0] != R.ldl_two_rounding(Gb, bb)[0]) >= 3


def test_ref_info_names_the_first_pivot_that_is_not_positive():
    assert R.ldl_exact(np.diag([1.0, 2.0, -1.0, 4.0]), np.ones(4))[1] == 3
    assert R.ldl_exact(np.diag([1.0, 2.0, 3.0, 4.0]), np.ones(4))[1] == 0
    x, info = R.ldl_exact(np.diag([1.0, 0.0, -1.0]), np.ones(3))
    assert info == 2 and np.isnan(x).all()          # L21 = round(0.0 * Inf) is NaN: no zero is skipped, x is lost
    x, info = R.ldl_exact(np.diag([1.0, 3.0, 0.0]), np.ones(3))
    assert info == 3 and np.isinf(x[2]) and np.isnan(x[0]) and np.isnan(x[1])          # x1 = fma(-0.0, Inf, 1/3)
    G = np.diag([1.0, np.nan, 3.0])
    x, info = R.ldl_exact(G, np.ones(3))
    assert info == 2 and np.isnan(x).all()          # a NaN pivot: r1 is NaN and so is every L below it
    # a pivot that the elimination makes negative: [[1, .], [2, 1]] has d1 = 1 - 4 = -3
    assert R.ldl_exact([[1.0, 0.0], [2.0, 1.0]], [1.0, 1.0])[1] == 2
    # the empty row of rule A5: no base, every pivot +0.0, info 1 and every x NaN; with a definite base, +0.0 everywhere
    x, info = R.ldl_exact(np.zeros((3, 3)), np.zeros(3))
    assert info == 1 and np.isnan(x).all()
    x, info = R.ldl_exact([[2.0, 0.0], [-1.0, 2.0]], [0.0, 0.0])
    assert info == 0 and np.all(x == 0.0) and not np.signbit(x).any()


def test_ref_als_pieces():
    rng = np.random.default_rng(5)
    rp = np.array([0, 3, 3, 7, 8], np.int64)
    ci = np.array([2, 0, 2, 5, 1, 1, 4, 3], np.int32)          # unsorted, column 2 and column 1 repeated
    vs = rng.standard_normal(8).astype(np.float32)
    V = rng.standard_normal((6, 3))
    base = np.eye(3) + 0.1
    x, info, G, b = R.als_exact(rp, ci, vs, V, False, 'one_plus_values', base, 0.25)
    assert info.tolist() == [0, 0, 0, 0] and np.all(x[1] == 0.0)
    Gn, M, bn, Mb = R.als_numpy(rp, ci, vs, V, False, 'one_plus_values', base, 0.25)
    assert np.allclose(G, Gn, rtol=1e-13, atol=1e-14) and np.allclose(b, bn, rtol=1e-13, atol=1e-14)
    assert G[0][0, 0] == Gn[0][0, 0] or abs(G[0][0, 0] - Gn[0][0, 0]) < 1e-14
    assert np.array_equal(b[3], (1.0 + np.float64(vs[7])) * V[3])           # one entry: fma(c, v, +0.0) = round(c v)
    assert np.array_equal(R.rhs_exact(rp, ci, None, V, 'values'), R.rhs_exact(rp, ci, vs, V, 'ones'))
    assert np.array_equal(R.rhs_exact(rp, ci, None, V, 'one_plus_values')[3], 2.0 * V[3])
    res, bound = R.residual_bound(Gn, M, bn, Mb, np.diff(rp), x)
    assert np.all(res <= 0.05 * bound)
    part = R.als_exact(rp, ci, vs, V, False, 'one_plus_values', base, 0.25, rows=(2, 4))
    assert np.array_equal(part[0], x[2:4]) and np.array_equal(part[2], G[2:4])
