"""
The conjugate-gradient ALS half-step on the host side, without a GPU: the three entries are declared in include/csrk.h,
exported and in the ctypes table; the limits need no device; every malformed request is refused with ValueError before any
library call; the C entries refuse a null handle and every argument they check before device work with an error code
(no crash, nothing written); without a device CSR.als_rows_cg fails loudly instead of computing on the CPU; and the
references of tests/als_cg_ref.py check themselves.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import als_cg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('csrk_als_rows_cg', 'csrk_als_rows_cg_device', 'csrk_als_cg_limits')


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
    # the device form is the host form plus a stream
    assert _lib.SIGNATURES['csrk_als_rows_cg_device'][1][:-1] == _lib.SIGNATURES['csrk_als_rows_cg'][1]


def test_limits_need_no_device():
    from csr_amd.kernels import hip as K
    lim = K.als_cg_limits()
    assert len(lim) == 3 and lim[0] >= 128 and lim[1] == 16 and lim[2] >= 1
    assert lim[0] <= K.als_limits()[0]                      # never above what the exact route takes
    from csr_amd._lib import lib, ERR_INVALID
    assert lib.csrk_als_cg_limits(None, 1) == ERR_INVALID
    two = (ctypes.c_int64 * 2)(-1, -1)
    assert lib.csrk_als_cg_limits(two, 1) == 0 and two[0] == lim[0] and two[1] == -1


def _bad():
    V = np.ones((4, 5))
    return {
        # als_args' cases
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
        'ridge per row': dict(V=V, lam_n=np.ones(3)),
        'ridge a string': dict(V=V, lam_n='0.1'),
        'ridge None': dict(V=V, lam_n=None),
        'ridge complex': dict(V=V, lam_n=1j),
        # the new ones
        'lam a string': dict(V=V, lam='0.1'),
        'lam None': dict(V=V, lam=None),
        'lam complex': dict(V=V, lam=1j),
        'lam per row': dict(V=V, lam=np.ones(3)),
        'steps negative': dict(V=V, steps=-1),
        'steps a float': dict(V=V, steps=3.0),
        'steps None': dict(V=V, steps=None),
        'steps a bool': dict(V=V, steps=True),
        'tol negative': dict(V=V, tol=-1e-9),
        'tol NaN': dict(V=V, tol=float('nan')),
        'tol a string': dict(V=V, tol='0'),
        'tol None': dict(V=V, tol=None),
        'x0 rows': dict(V=V, x0=np.ones((2, 5))),
        'x0 columns': dict(V=V, x0=np.ones((3, 4))),
        'x0 1-D': dict(V=V, x0=np.ones(15)),
        'x0 float32': dict(V=V, x0=np.ones((3, 5), np.float32)),
        'x0 integer': dict(V=V, x0=np.ones((3, 5), np.int64)),
        'x0 for the whole matrix with a row range': dict(V=V, rows=(1, 3), x0=np.ones((3, 5))),
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


@pytest.mark.parametrize('case', sorted(_bad()))
def test_bad_requests_raise_before_any_library_call(case, monkeypatch):
    K = _forbid(monkeypatch, ('csrk_als_rows_cg', 'csrk_als_rows_cg_device', 'csrk_als_rows', 'csrk_als_rows_device', 'csrk_create'))
    kw = dict(_bad()[case])
    V = kw.pop('V')
    h = K.hip_h(12345, 3, 4, 4)
    with pytest.raises(ValueError):
        K.als_rows_cg(h, V, False, kw.get('rhs', 'values'), kw.get('base'), kw.get('lam', 0.0), kw.get('lam_n', 0.0), kw.get('rows'),
                      kw.get('steps', 3), kw.get('x0'), kw.get('tol', 0.0))
    ckw = {{'lam': 'reg', 'lam_n': 'reg_per_entry'}.get(a, a): b for a, b in kw.items()}
    with pytest.raises(ValueError):
        _mat().als_rows_cg(V, **ckw)


def test_good_arguments_come_back_as_the_library_takes_them():
    from csr_amd.kernels import hip as K
    from csr_amd import _lib
    h = K.hip_h(12345, 3, 4, 4)
    V = np.ones((4, 5), np.float32)
    x0 = np.arange(10.0).reshape(2, 5)
    got = K.als_cg_args(h, V, 'one_plus_values', np.eye(5), 0.5, 0.25, (1, 3), 7, x0, 0.5)
    assert got[1:6] == (5, 5, _lib.VAL_F32, 1, 3) and got[7:12] == (_lib.ALS_RHS_ONE_PLUS, 0.5, 0.25, 7, 0.25)      # tol squared
    assert np.array_equal(got[12], x0) and got[12].flags.c_contiguous
    assert K.als_cg_args(h, V)[10:] == (3, 0.0, None)          # the defaults: three steps, no tolerance, a cold start


def test_null_handle_is_an_error_code():
    from csr_amd._lib import lib, ERR_INVALID, VAL_F64, ALS_RHS_VALUES
    V = np.ones((4, 2))
    out, resid, taken = np.full(6, 7.0), np.full(3, 7.0), np.full(3, 7, np.int32)
    for H in (0, 12345):
        assert lib.csrk_als_rows_cg(H, 0, 3, V.ctypes.data, 2, 2, VAL_F64, 0, ALS_RHS_VALUES, None, 0.1, 0.0, 3, 0.0, None, 2,
                                    out.ctypes.data, 2, resid.ctypes.data, taken.ctypes.data) == ERR_INVALID
        assert b'invalid csrk handle' in lib.csrk_last_error()
        assert lib.csrk_als_rows_cg_device(H, 0, 3, None, 2, 2, VAL_F64, 0, ALS_RHS_VALUES, None, 0.1, 0.0, 3, 0.0, None, 2, None, 2,
                                           None, None, None) == ERR_INVALID
        assert b'invalid csrk handle' in lib.csrk_last_error()
    assert np.all(out == 7.0) and np.all(resid == 7.0) and np.all(taken == 7)


def test_scalar_refusals_come_before_the_handle_and_need_no_device():
    "rule C9: what the scalars alone decide is refused before the handle is looked at -- with its own words, not the handle's"
    from csr_amd._lib import lib, ERR_INVALID, ERR_UNSUPPORTED, VAL_F64, ALS_RHS_VALUES
    from csr_amd.kernels import hip as K
    V, x0 = np.ones((4, 2)), np.ones((3, 2))
    out, resid, taken = np.full(6, 7.0), np.full(3, 7.0), np.full(3, 7, np.int32)
    kmax = K.als_cg_limits()[0]
    good = dict(rb=0, re=3, ldv=2, k=2, pt=VAL_F64, scale=0, rhs=ALS_RHS_VALUES, lam=0.1, lam_n=0.0, steps=3, tol2=0.0, ldx0=2, ldo=2)
    cases = {
        'k = 0': (dict(k=0), ERR_INVALID, b'k must be at least 1'),
        'ldv < k': (dict(ldv=1), ERR_INVALID, b'bad panel geometry'),
        'ldo < k': (dict(ldo=1), ERR_INVALID, b'bad output geometry'),
        'panel type': (dict(pt=7), ERR_INVALID, b'panel_type must be'),
        'scale': (dict(scale=2), ERR_INVALID, b'scale must be 0 or 1'),
        'rhs_mode': (dict(rhs=3), ERR_INVALID, b'rhs_mode must be'),
        'steps < 0': (dict(steps=-1), ERR_INVALID, b'steps must not be negative'),
        'tol2 < 0': (dict(tol2=-1.0), ERR_INVALID, b'tol2 must be'),
        'tol2 NaN': (dict(tol2=float('nan')), ERR_INVALID, b'tol2 must be'),
        'ldx0 < k': (dict(ldx0=1), ERR_INVALID, b'bad x0 geometry'),
        'rows reversed': (dict(rb=2, re=1), ERR_INVALID, b'bad row range'),
        'rows negative': (dict(rb=-1), ERR_INVALID, b'bad row range'),
        'k too large': (dict(k=kmax + 1, ldv=kmax + 1, ldo=kmax + 1, ldx0=kmax + 1), ERR_UNSUPPORTED, b'csrk_als_cg_limits'),
    }
    for name, (change, code, words) in cases.items():
        a = dict(good, **change)
        for H in (0, 12345):
            args = (H, a['rb'], a['re'], V.ctypes.data, a['ldv'], a['k'], a['pt'], a['scale'], a['rhs'], None, a['lam'], a['lam_n'],
                    a['steps'], a['tol2'], x0.ctypes.data, a['ldx0'], out.ctypes.data, a['ldo'], resid.ctypes.data, taken.ctypes.data)
            assert lib.csrk_als_rows_cg(*args) == code, name
            assert words in lib.csrk_last_error(), (name, lib.csrk_last_error())
            assert lib.csrk_als_rows_cg_device(*args, None) == code, name
            assert words in lib.csrk_last_error(), (name, lib.csrk_last_error())
    # ldx0 is not looked at without an x0
    args = (0, 0, 3, V.ctypes.data, 2, 2, VAL_F64, 0, ALS_RHS_VALUES, None, 0.1, 0.0, 3, 0.0, None, 0, out.ctypes.data, 2, None, None)
    assert lib.csrk_als_rows_cg(*args) == ERR_INVALID and b'invalid csrk handle' in lib.csrk_last_error()
    assert np.all(out == 7.0) and np.all(resid == 7.0) and np.all(taken == 7)


def test_a_stale_handle_is_an_error_code():
    "a handle that was freed is refused like a null one (this needs a device to make a handle at all: without one, nothing to check)"
    import torch
    if torch.cuda.device_count() == 0:
        return
    from csr_amd._lib import lib, ERR_INVALID, VAL_F64, ALS_RHS_VALUES
    from csr_amd.kernels import hip as K
    h = K.to_handle(_mat())
    H = h.H
    K.release_handle(h)
    lib.csrk_trim_cache()
    V, out = np.ones((4, 2)), np.full(6, 7.0)
    rc = lib.csrk_als_rows_cg(H, 0, 3, V.ctypes.data, 2, 2, VAL_F64, 0, ALS_RHS_VALUES, None, 0.1, 0.0, 3, 0.0, None, 2, out.ctypes.data,
                              2, None, None)
    assert rc == ERR_INVALID and b'invalid csrk handle' in lib.csrk_last_error()      # (four entries: too small for the handle cache)
    assert np.all(out == 7.0)


def test_no_cpu_fallback():
    "without a device als_rows_cg raises CsrkError naming hip; with one it computes (never on the CPU)"
    import torch
    from csr_amd._lib import CsrkError
    V = np.arange(8.0).reshape(4, 2) + 1.0
    base = np.eye(2)
    m = _mat()
    if torch.cuda.device_count() > 0:
        got = m.als_rows_cg(V, base=base, reg=0.5, return_info=True)
        want = R.cg_exact(m.rowptrs, m.colinds, m.values, V, False, 'values', base, 0.5, 0.0, 3)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        return
    with pytest.raises(CsrkError) as ei:
        m.als_rows_cg(V, base=base)
    assert 'hip' in str(ei.value).lower()


# ---- the references check themselves ----------------------------------------------------------------------

def test_ref_hand_case():
    """
    k = 1, V = [[2]], no scaling, c = 4, lam = 4: b = 4 * 2 = 8, M = 2 * 2 + 4 = 8.  Cold: r = p = 8, rs = 64, q = M p = 64,
    pq = 512, alpha = 0.125, x = 1, r = 8 - 0.125 * 64 = 0, rn = 0: one step of the five allowed, resid +0.0.
    """
    for V in (np.array([[2.0]]), np.array([[2.0]], np.float32)):
        x, rs, taken = R.cg_exact([0, 1], [0], np.array([4.0]), V, False, 'values', None, 4.0, 0.0, 5)
        assert x.tolist() == [[1.0]] and rs.tolist() == [0.0] and not np.signbit(rs[0]) and taken.tolist() == [1]
    x, rs, taken = R.cg_numpy([0, 1], [0], np.array([4.0]), np.array([[2.0]]), False, 'values', None, 4.0, 0.0, 5)
    assert x.tolist() == [[1.0]] and rs.tolist() == [0.0] and taken.tolist() == [1]


def test_ref_the_documented_hazard_stays_finite_for_five_steps():
    "rule C10: k = 1, M = 12.75, b = 8 never reaches rs = 0; after 5 steps rs is about 1.7e-167"
    # V = [[0.5]], one entry with c = 16: b = 8; M = 0.25 + 12.5
    x, rs, taken = R.cg_exact([0, 1], [0], np.array([16.0]), np.array([[0.5]]), False, 'values', None, 12.5, 0.0, 5)
    assert taken[0] == 5 and 1e-168 < rs[0] < 1e-166
    assert abs(x[0, 0] - 8.0 / 12.75) < 1e-15


def test_ref_exact_differs_from_two_rounding():
    "a = 1 + 2^-30: DOT(a, a) = fma(a, a, +0.0) = round(1 + 2^-29 + 2^-60) either way, but b = fma(c, v, b) over two entries tells them apart"
    a = 1.0 + 2.0 ** -30
    # b = fma(a, a, fma(-1, 1 + 2^-29, 0)) = a a - (1 + 2^-29) = 2^-60 exactly when fused; round(a a) - (1 + 2^-29) = 0 when not
    V = np.array([[1.0 + 2.0 ** -29], [a]])
    args = ([0, 2], [0, 1], np.array([-1.0, a]), V, False, 'values', None, 1.0, 0.0, 0)
    assert R.cg_exact(*args)[1][0] == (2.0 ** -60) ** 2
    assert R.cg_two_rounding(*args)[1][0] == 0.0
    # and on an ordinary input most elements differ in the last place
    rng = np.random.default_rng(11)
    V = rng.standard_normal((9, 12))
    rp, ci, vs = [0, 6], [3, 1, 8, 3, 0, 5], rng.random(6)
    xe = R.cg_exact(rp, ci, vs, V, True, 'one_plus_values', None, 0.1, 0.0, 3)[0]
    x2 = R.cg_two_rounding(rp, ci, vs, V, True, 'one_plus_values', None, 0.1, 0.0, 3)[0]
    assert np.count_nonzero(xe != x2) >= 3 and np.allclose(xe, x2, rtol=1e-12)


@pytest.mark.parametrize('k', [1, 31, 32, 33, 63, 64, 65, 128])
@pytest.mark.parametrize('f32', [False, True])
def test_ref_dot_ownership(k, f32):
    "C2 against a direct enumeration of csrk_sddmm's lanes: lane l, in each 64-column chunk, its 16-B pieces"
    lanes = [[] for _ in range(16)]
    for c in range(0, k, 64):
        for l in range(16):
            cols = [4 * l + i for i in range(4)] if f32 else [2 * l, 2 * l + 1, 32 + 2 * l, 33 + 2 * l]
            lanes[l] += [c + t for t in cols if c + t < k]
    assert sorted(t for ln in lanes for t in ln) == list(range(k))
    for l, ln in enumerate(lanes):
        assert ln == sorted(ln) and all(R.owner(t, f32) == l for t in ln)
    # the value: partials over a lane's columns ascending, then the balanced tree in index order
    rng = np.random.default_rng(k)
    a, b = rng.standard_normal(k), rng.standard_normal(k)
    s = []
    for ln in lanes:
        acc = 0.0
        for t in ln:
            acc = R._fma(a[t], b[t], acc)
        s.append(acc)
    want = (((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))) + \
           (((s[8] + s[9]) + (s[10] + s[11])) + ((s[12] + s[13]) + (s[14] + s[15])))
    assert R.dot(list(a), list(b), f32) == want
    assert abs(want - float(a @ b)) <= 1e-13 * float(np.abs(a) @ np.abs(b))


def test_ref_no_steps_returns_x0s_bits():
    rng = np.random.default_rng(2)
    V = rng.standard_normal((5, 7))
    x0 = rng.standard_normal((2, 7))
    x0[0, 3], x0[1, 0] = -0.0, 5e-324
    x, rs, taken = R.cg_exact([0, 2, 5], [1, 4, 0, 0, 2], None, V, False, 'ones', None, 0.5, 0.0, 0, 0.0, x0)
    assert np.array_equal(x.view(np.int64), x0.view(np.int64)) and taken.tolist() == [0, 0] and np.all(rs > 0)
    # rs is DOT(r, r) of r = b - M x0 all the same
    xn, rsn, _ = R.cg_numpy([0, 2, 5], [1, 4, 0, 0, 2], None, V, False, 'ones', None, 0.5, 0.0, 0, 0.0, x0)
    assert np.allclose(rs, rsn, rtol=1e-12)


def test_ref_a_tolerance_above_the_first_residual_takes_no_step_and_nan_stops():
    V = np.array([[2.0, 1.0]])
    x, rs, taken = R.cg_exact([0, 1], [0], None, V, False, 'ones', None, 1.0, 0.0, 5, 5.0 + 1e-9)
    assert taken[0] == 0 and rs[0] == 5.0 and np.all(x == 0.0)
    assert R.cg_exact([0, 1], [0], None, V, False, 'ones', None, 1.0, 0.0, 5, 5.0 - 1e-9)[2][0] >= 1
    Vn = np.array([[np.nan, 1.0]])
    x, rs, taken = R.cg_exact([0, 1], [0], None, Vn, False, 'ones', None, 1.0, 0.0, 5)
    assert taken[0] == 0 and np.isnan(rs[0])


def test_ref_full_run_meets_the_direct_solve():
    "steps = 2 k from zero: CG has converged (k steps in exact arithmetic) and meets numpy.linalg.solve"
    rng = np.random.default_rng(7)
    k = 6
    V = rng.standard_normal((9, k))
    rp, ci = [0, 8], [3, 1, 8, 3, 0, 5, 7, 2]
    vs = rng.random(8).astype(np.float32)
    A = rng.standard_normal((k, k))
    base = A.T @ A / k
    b = ((1.0 + vs.astype(np.float64)) @ V[ci])
    M = base + 0.25 * np.eye(k) + (V[ci] * vs[:, None].astype(np.float64)).T @ V[ci]
    want = np.linalg.solve(M, b)
    tol2 = 2.0 ** -96 * float(b @ b)
    for ref in (R.cg_exact, R.cg_numpy):
        x, rs, taken = ref(rp, ci, vs, V, True, 'one_plus_values', base, 0.25, 0.0, 2 * k, tol2)
        assert np.allclose(x[0], want, rtol=1e-12, atol=1e-14) and k <= taken[0] <= 2 * k and rs[0] <= tol2
    # a row sub-range and an empty row
    x, rs, taken = R.cg_exact([0, 0, 8], ci, vs, V, True, 'one_plus_values', base, 0.25, 0.0, 3, rows=(0, 1))
    assert np.all(x == 0.0) and not np.signbit(x).any() and rs[0] == 0.0 and taken[0] == 0
    up = R.cg_numpy(rp, ci, vs, V, True, 'one_plus_values', base, 0.25, 0.0, 3, order=1)[0]
    down = R.cg_numpy(rp, ci, vs, V, True, 'one_plus_values', base, 0.25, 0.0, 3, order=-1)[0]
    assert np.allclose(up, down, rtol=1e-12) and np.allclose(up, R.cg_exact(rp, ci, vs, V, True, 'one_plus_values', base, 0.25, 0.0, 3)[0], rtol=1e-12)


def test_the_method_mirrors_the_lower_triangle_of_base(monkeypatch):
    "CSR.als_rows_cg hands the kernel the matrix CSR.als_rows would solve with: base's lower triangle, mirrored"
    from csr_amd.kernels import hip as K
    seen = {}

    class H:
        pass

    def fake(h, V, scale, rhs, base, lam, lam_n, rows, steps, x0, tol):
        seen.update(base=base, lam=lam, lam_n=lam_n, steps=steps, tol=tol, rows=rows)
        return np.zeros((3, 2)), np.zeros(3), np.zeros(3, np.int32)
    monkeypatch.setattr(K, 'als_rows_cg', fake)
    monkeypatch.setattr(K, 'to_handle', lambda m: H())
    monkeypatch.setattr(K, 'release_handle', lambda h: None)
    base = np.array([[2.0, np.nan], [0.5, 3.0]])
    out = _mat().als_rows_cg(np.ones((4, 2)), base=base, reg=0.5, reg_per_entry=0.25, tol=0.5)
    assert out.shape == (3, 2)
    assert np.array_equal(seen['base'], [[2.0, 0.5], [0.5, 3.0]])
    assert (seen['lam'], seen['lam_n'], seen['steps'], seen['tol'], seen['rows']) == (0.5, 0.25, 3, 0.5, (0, 3))
