"""
csrk_topk_scores on the host side, without a GPU: the three entries are declared in include/csrk.h, exported and in the
ctypes table; the limits need no device; every malformed request is refused with ValueError before any library call; the C
entries refuse a bad handle and every bad argument with an error code (no crash, nothing written); without a device
CSR.topk_scores fails loudly instead of computing on the CPU; and the references of tests/topk_scores_ref.py check
themselves.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import topk_scores_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('csrk_topk_scores', 'csrk_topk_scores_device', 'csrk_topk_scores_limits')
INF = np.inf


def _mat():
    from csr_amd import CSR
    return CSR(3, 4, 4, np.array([0, 2, 2, 4], np.int32), np.array([0, 3, 1, 2], np.int32), np.array([1.0, -2.0, 0.5, 4.0]))


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
    from csr_amd._lib import lib, ERR_INVALID
    lim = K.topk_scores_limits()
    assert len(lim) == 6 and lim[0] >= 256 and lim[1] >= 128
    assert lim[2] >= 1 and lim[3] >= 1 and 1 <= lim[4] <= lim[0] and lim[5] >= 1
    assert lib.csrk_topk_scores_limits(None, 1) == ERR_INVALID
    two = (ctypes.c_int64 * 2)(-1, -1)
    assert lib.csrk_topk_scores_limits(two, 1) == 0 and two[0] == lim[0] and two[1] == -1


def _bad():
    U, V = np.ones((3, 5)), np.ones((4, 5))
    return {
        'U rows': dict(U=np.ones((4, 5)), V=V),
        'V rows': dict(U=U, V=np.ones((5, 5))),
        '1-D U': dict(U=np.ones(3), V=V),
        '1-D V': dict(U=U, V=np.ones(4)),
        'k differs': dict(U=U, V=np.ones((4, 4))),
        'k = 0': dict(U=np.ones((3, 0)), V=np.ones((4, 0))),
        'mixed dtypes': dict(U=U, V=V.astype(np.float32)),
        'integer panels': dict(U=U.astype(np.int64), V=V.astype(np.int64)),
        'float16 panels': dict(U=U.astype(np.float16), V=V.astype(np.float16)),
        'n = 0': dict(U=U, V=V, n=0),
        'n negative': dict(U=U, V=V, n=-3),
        'n a float': dict(U=U, V=V, n=2.0),
        'n a bool': dict(U=U, V=V, n=True),
        'n None': dict(U=U, V=V, n=None),
        'min_score NaN': dict(U=U, V=V, min_score=float('nan')),
        'min_score a string': dict(U=U, V=V, min_score='0'),
        'min_score per row': dict(U=U, V=V, min_score=np.zeros(3)),
        'rows past the end': dict(U=U, V=V, rows=(0, 4)),
        'rows negative': dict(U=U, V=V, rows=(-1, 2)),
        'rows reversed': dict(U=U, V=V, rows=(2, 1)),
        'rows not a pair': dict(U=U, V=V, rows=(1,)),
        'rows not integers': dict(U=U, V=V, rows=(0.0, 2.0)),
    }


@pytest.mark.parametrize('case', sorted(_bad()))
def test_bad_requests_raise_before_any_library_call(case, monkeypatch):
    from csr_amd.kernels import hip as K
    from csr_amd import _lib

    def forbidden(*a, **kw):
        raise AssertionError('library called')
    for name in ('csrk_topk_scores', 'csrk_topk_scores_device', 'csrk_create'):
        monkeypatch.setattr(_lib.lib, name, forbidden)
    monkeypatch.setattr(K, 'to_handle', forbidden)
    kw = dict(_bad()[case])
    U, V, n = kw.pop('U'), kw.pop('V'), kw.pop('n', 2)
    h = K.hip_h(12345, 3, 4, 4)
    with pytest.raises(ValueError):
        K.topk_scores(h, U, V, n, kw.get('min_score'), kw.get('rows'))
    with pytest.raises(ValueError):
        K.topk_scores_args(h, U, V, n, kw.get('min_score'), kw.get('rows'))
    with pytest.raises(ValueError):
        _mat().topk_scores(U, V, n, **kw)
    with pytest.raises(ValueError):
        _mat().topk_scores(U, V, n, exclude=False, **kw)


def test_args_without_a_handle_take_the_shape_from_the_panels():
    from csr_amd.kernels import hip as K
    U, V = np.ones((3, 5), np.float32), np.ones((7, 5), np.float32)[:, :]
    a = K.topk_scores_args(None, U, V, 4, None, (1, 3))
    assert a[1] == 5 and a[3] == 5 and a[4] == 7 and a[5] == 5 and a[7] == 4 and a[8] == -INF and a[9:] == (1, 3)
    wide = np.ones((7, 9))
    a = K.topk_scores_args(None, np.ones((3, 5)), wide[:, 2:7], 1, 0.5)
    assert a[3] == 9 and a[8] == 0.5 and a[9:] == (0, 3)          # a row-major view keeps its stride


def test_bad_handles_and_arguments_are_error_codes():
    "the argument checks of both C entries come before any device work: they need no GPU, and nothing is written"
    from csr_amd._lib import lib, ERR_INVALID, ERR_UNSUPPORTED, VAL_F64
    from csr_amd.kernels import hip as K
    U, V = np.ones((3, 2)), np.ones((4, 2))
    items, scores, counts = np.full((3, 2), 7, np.int32), np.full((3, 2), 7.0), np.full(3, 7, np.int32)
    u, v, it, sc, cn = U.ctypes.data, V.ctypes.data, items.ctypes.data, scores.ctypes.data, counts.ctypes.data
    for H in (12345, 777):
        assert lib.csrk_topk_scores(H, 0, 3, u, 2, v, 2, 4, 2, VAL_F64, 2, -INF, it, 2, sc, 2, cn) == ERR_INVALID
        assert b'invalid csrk handle' in lib.csrk_last_error()
        assert lib.csrk_topk_scores_device(H, 0, 3, u, 2, v, 2, 4, 2, VAL_F64, 2, -INF, it, 2, sc, 2, cn, None) == ERR_INVALID
        assert b'invalid csrk handle' in lib.csrk_last_error()
    good = dict(rb=0, re=3, u=u, ldu=2, v=v, ldv=2, ni=4, k=2, pt=VAL_F64, nt=2, ms=-INF, it=it, ldi=2, sc=sc, lds=2, cn=cn)
    bad = {'k = 0': dict(k=0), 'n_top = 0': dict(nt=0), 'n_items < 0': dict(ni=-1), 'ldu < k': dict(ldu=1), 'ldv < k': dict(ldv=1),
           'ldi < n_top': dict(ldi=1), 'lds < n_top': dict(lds=1), 'panel type': dict(pt=7), 'panel none': dict(pt=0),
           'NaN min_score': dict(ms=float('nan')), 'row_begin < 0': dict(rb=-1), 'row_begin > row_end': dict(rb=3, re=2),
           'NULL items': dict(it=None), 'NULL scores': dict(sc=None), 'NULL U': dict(u=None), 'NULL V': dict(v=None)}
    for name, change in bad.items():
        a = dict(good, **change)
        args = (0, a['rb'], a['re'], a['u'], a['ldu'], a['v'], a['ldv'], a['ni'], a['k'], a['pt'], a['nt'], a['ms'], a['it'], a['ldi'],
                a['sc'], a['lds'], a['cn'])
        assert lib.csrk_topk_scores(*args) == ERR_INVALID, name
        assert lib.csrk_topk_scores_device(*args, None) == ERR_INVALID, name
        assert lib.csrk_last_error(), name
    lim = K.topk_scores_limits()
    for change in (dict(k=lim[0] + 1, ldu=lim[0] + 1, ldv=lim[0] + 1), dict(nt=lim[1] + 1, ldi=lim[1] + 1, lds=lim[1] + 1)):
        a = dict(good, **change)
        args = (0, a['rb'], a['re'], a['u'], a['ldu'], a['v'], a['ldv'], a['ni'], a['k'], a['pt'], a['nt'], a['ms'], a['it'], a['ldi'],
                a['sc'], a['lds'], a['cn'])
        assert lib.csrk_topk_scores(*args) == ERR_UNSUPPORTED, change
        assert lib.csrk_topk_scores_device(*args, None) == ERR_UNSUPPORTED, change
    # no rows: fine, NULL pointers and all
    assert lib.csrk_topk_scores(0, 2, 2, None, 2, None, 2, 4, 2, VAL_F64, 2, -INF, None, 2, None, 2, None) == 0
    assert lib.csrk_topk_scores_device(0, 2, 2, None, 2, None, 2, 4, 2, VAL_F64, 2, -INF, None, 2, None, 2, None, None) == 0
    assert np.all(items == 7) and np.all(scores == 7.0) and np.all(counts == 7)


def test_no_cpu_fallback():
    "without a device topk_scores raises CsrkError naming hip; with one it computes (never on the CPU)"
    import torch
    from csr_amd._lib import CsrkError
    m = _mat()
    U = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    V = np.array([[4.0, 1.0], [3.0, 2.0], [2.0, 3.0], [1.0, 4.0]])
    if torch.cuda.device_count() > 0:
        for ex in (True, False):
            got = m.topk_scores(U, V, 2, exclude=ex)
            want = R.select(R.scores_plain(U, V), m.rowptrs if ex else None, m.colinds, 2)
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
        return
    for ex in (True, False):
        with pytest.raises(CsrkError) as ei:
            m.topk_scores(U, V, 2, exclude=ex)
        assert 'hip' in str(ei.value).lower()


# ---- the references check themselves ----------------------------------------------------------------------

def _sel(row, n, seen=None, min_score=None):
    S = np.array([row], np.float64)
    rp = None if seen is None else np.array([0, len(seen)])
    it, sc, cn = R.select(S, rp, None if seen is None else np.array(seen, np.int32), n, min_score)
    return it[0].tolist(), sc[0], int(cn[0])


def test_select_ties_go_to_the_smaller_item():
    it, sc, cn = _sel([1.0, 3.0, 3.0, 2.0, 3.0], 2)
    assert it == [1, 2] and cn == 2 and sc.tolist() == [3.0, 3.0]
    it, sc, cn = _sel([1.0, 3.0, 3.0, 2.0, 3.0], 4)
    assert it == [1, 2, 4, 3] and cn == 4
    it, sc, cn = _sel([5.0, 5.0, 5.0], 2, seen=[0])
    assert it == [1, 2]


def test_select_nan_above_inf_and_all_nans_tied():
    nan2 = np.array([0x7ff8000000000001, 0xfff8000000000000], np.uint64).view(np.float64)
    it, sc, cn = _sel([INF, nan2[0], 1.0, nan2[1], -INF], 5)
    assert it == [1, 3, 0, 2, 4] and cn == 5
    assert sc.view(np.uint64)[:2].tolist() == [0x7ff8000000000001, 0xfff8000000000000]          # the bits are kept


def test_select_signed_zeros_tie_and_keep_their_bits():
    it, sc, cn = _sel([-1.0, -0.0, 0.0, -0.0], 3)
    assert it == [1, 2, 3] and np.signbit(sc[:3]).tolist() == [True, False, True]
    it, sc, cn = _sel([0.0, -0.0], 1)
    assert it == [0] and not np.signbit(sc[0])


def test_select_threshold_padding_and_counts():
    row = [0.5, 2.0, -1.0, 1.0, float('nan')]
    it, sc, cn = _sel(row, 4, min_score=1.0)          # a score equal to min_score passes, and so does NaN
    assert it == [4, 1, 3, -1] and cn == 3 and sc[3] == -INF and np.isnan(sc[0])
    it, sc, cn = _sel(row, 2, min_score=-INF)
    assert it == [4, 1] and cn == 2
    it, sc, cn = _sel([-0.0, -1.0], 2, min_score=0.0)          # -0.0 passes 0.0
    assert it == [0, -1] and cn == 1
    it, sc, cn = _sel(row, 3, seen=[0, 1, 2, 3, 4])          # a fully seen row
    assert it == [-1, -1, -1] and cn == 0 and np.all(sc == -INF)
    it, sc, cn = _sel([1.0, 2.0], 5)          # n_top > n_items
    assert it == [1, 0, -1, -1, -1] and cn == 2
    it, sc, cn = R.select(np.zeros((2, 0)), None, None, 3)          # no items at all
    assert it.tolist() == [[-1] * 3] * 2 and cn.tolist() == [0, 0] and np.all(sc == -INF)


def test_key_orders_like_the_contract():
    xs = np.array([-INF, -2.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, INF, float('nan')])
    k = R.key(xs)
    assert k[3] == k[4] and np.all(np.diff(k[[0, 1, 2, 3, 5, 6, 7, 8]].astype(object)) > 0) and k[0] > 0


def test_plain_equals_exact_on_a_grid_and_on_float32():
    rng = np.random.default_rng(11)
    U = rng.integers(-512, 512, (3, 9)) / 64.0
    V = rng.integers(-512, 512, (17, 9)) / 64.0
    assert np.array_equal(R.scores_plain(U, V), R.scores_exact(U, V))
    U32, V32 = rng.standard_normal((3, 9)).astype(np.float32), rng.standard_normal((17, 9)).astype(np.float32)
    assert np.array_equal(R.scores_plain(U32, V32), R.scores_exact(U32, V32))
    assert np.array_equal(R.scores_two_rounding(U32, V32), R.scores_exact(U32, V32))


def test_exact_tells_a_fused_chain_from_two_roundings():
    "a = 1 + 2^-30: a a = 1 + 2^-29 + 2^-60 exactly; fma(a, a, -(1 + 2^-29)) = 2^-60, multiply-then-add gives 0"
    a = 1.0 + 2.0 ** -30
    U, V = np.array([[1.0, a]]), np.array([[-(1.0 + 2.0 ** -29), a]])
    assert R.scores_exact(U, V)[0, 0] == 2.0 ** -60
    assert R.scores_two_rounding(U, V)[0, 0] == 0.0 and R.scores_plain(U, V)[0, 0] == 0.0
    rng = np.random.default_rng(7)
    Ur, Vr = rng.standard_normal((2, 8)), rng.standard_normal((40, 8))
    assert np.count_nonzero(R.scores_exact(Ur, Vr) != R.scores_two_rounding(Ur, Vr)) >= 10


def test_positions_of_special_values():
    U = np.array([[1.0, 0.0], [INF, 1.0], [0.0, 0.0]])
    V = np.array([[1.0, 1.0], [-INF, 1.0], [float('nan'), 0.0], [0.0, INF]])
    nan, pinf, ninf = R.scores_positions(U, V)
    assert nan.tolist() == [[False, False, True, True], [False, False, True, True], [False, True, True, True]]
    assert pinf.tolist() == [[False, False, False, False], [True, False, False, False], [False] * 4]
    assert ninf.tolist() == [[False, True, False, False], [False, True, False, False], [False] * 4]
