"""
csrk_rank_entries on the host side, without a GPU: the three entries are declared in include/csrk.h, exported and in the
ctypes table; the limits need no device; every malformed request is refused with ValueError before any library call; the C
entries refuse a bad handle and every bad scalar argument with an error code (no crash, nothing written); without a device
CSR.rank_entries fails loudly instead of computing on the CPU; and the reference of tests/rank_entries_ref.py checks itself.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import rank_entries_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('csrk_rank_entries', 'csrk_rank_entries_device', 'csrk_rank_entries_limits')
INF = np.inf


def _mat():
    from csr_amd import CSR
    return CSR(3, 4, 4, np.array([0, 2, 2, 4], np.int32), np.array([0, 3, 1, 2], np.int32), np.array([1.0, -2.0, 0.5, 4.0]))


def _test_mat(nrows=3, ncols=4):
    from csr_amd import CSR
    return CSR(nrows, ncols, 3, np.array([0, 1] + [3] * (nrows - 1), np.int32), np.array([1, 2, 0], np.int32), None)


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
    lim = K.rank_entries_limits()
    assert len(lim) == 5 and lim[0] >= 256 and all(v >= 1 for v in lim[1:])
    assert lib.csrk_rank_entries_limits(None, 1) == ERR_INVALID
    two = (ctypes.c_int64 * 2)(-1, -1)
    assert lib.csrk_rank_entries_limits(two, 1) == 0 and two[0] == lim[0] and two[1] == -1


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
        'test of more columns': dict(U=U, V=V, test=(3, 5)),
        'test of fewer rows': dict(U=U, V=V, test=(2, 4)),
        'test an array': dict(U=U, V=V, test=np.zeros((3, 4))),
        'test None': dict(U=U, V=V, test=None),
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
    for name in ('csrk_rank_entries', 'csrk_rank_entries_device', 'csrk_create', 'csrk_row_extent'):
        monkeypatch.setattr(_lib.lib, name, forbidden)
    monkeypatch.setattr(K, 'to_handle', forbidden)
    kw = dict(_bad()[case])
    U, V, rows, test = kw['U'], kw['V'], kw.get('rows'), kw.get('test', (3, 4))
    seen_h = K.hip_h(12345, 3, 4, 4)
    test_h = K.hip_h(777, test[0], test[1], 3) if isinstance(test, tuple) else test
    test_m = _test_mat(*test) if isinstance(test, tuple) else test
    with pytest.raises(ValueError):
        K.rank_entries(seen_h, test_h, U, V, rows)
    with pytest.raises(ValueError):
        K.rank_entries_args(seen_h, test_h, U, V, rows)
    with pytest.raises(ValueError):
        _mat().rank_entries(U, V, test_m, rows=rows)
    with pytest.raises(ValueError):
        _mat().rank_entries(U, V, test_m, rows=rows, exclude=False, return_scores=True)
    if 'test' not in kw:          # without seen the panels are still checked against test
        with pytest.raises(ValueError):
            K.rank_entries(None, test_h, U, V, rows)


def test_args_keep_strides_and_default_rows():
    from csr_amd.kernels import hip as K
    t = K.hip_h(777, 3, 7, 2)
    wide = np.ones((7, 9), np.float32)
    a = K.rank_entries_args(None, t, np.ones((3, 5), np.float32), wide[:, 2:7], (1, 3))
    assert a[1] == 5 and a[3] == 9 and a[4] == 5 and a[6:] == (1, 3)          # a row-major view keeps its stride
    a = K.rank_entries_args(K.hip_h(1, 3, 7, 0), t, np.ones((3, 5)), np.ones((7, 5)))
    assert a[6:] == (0, 3)


def test_bad_handles_and_arguments_are_error_codes():
    "the handle and scalar checks of both C entries come before any device work: they need no GPU, and nothing is written"
    from csr_amd._lib import lib, ERR_INVALID, ERR_UNSUPPORTED, VAL_F64
    from csr_amd.kernels import hip as K
    U, V = np.ones((3, 2)), np.ones((4, 2))
    ranks, scores = np.full(6, 7, np.int32), np.full(6, 7.0)
    u, v, rk, sc = U.ctypes.data, V.ctypes.data, ranks.ctypes.data, scores.ctypes.data
    for seen, test in ((0, 12345), (12345, 777), (777, 0)):
        assert lib.csrk_rank_entries(seen, test, 0, 3, u, 2, v, 2, 2, VAL_F64, rk, sc) == ERR_INVALID
        assert b'invalid csrk handle' in lib.csrk_last_error()
        assert lib.csrk_rank_entries_device(seen, test, 0, 3, u, 2, v, 2, 2, VAL_F64, rk, sc, None) == ERR_INVALID
        assert b'invalid csrk handle' in lib.csrk_last_error()
    # the scalar arguments are looked at before the handles (rule 9), so no live handle is needed to see them refused
    good = dict(rb=0, re=3, ldu=2, ldv=2, k=2, pt=VAL_F64)
    bad = {'k = 0': dict(k=0), 'k < 0': dict(k=-1), 'ldu < k': dict(ldu=1), 'ldv < k': dict(ldv=1), 'panel type': dict(pt=7),
           'panel none': dict(pt=0), 'row_begin < 0': dict(rb=-1), 'row_begin > row_end': dict(rb=3, re=2)}
    for name, change in bad.items():
        a = dict(good, **change)
        args = (0, 12345, a['rb'], a['re'], u, a['ldu'], v, a['ldv'], a['k'], a['pt'], rk, sc)
        for fn, more in ((lib.csrk_rank_entries, ()), (lib.csrk_rank_entries_device, (None,))):
            assert fn(*args, *more) == ERR_INVALID, name
            err = lib.csrk_last_error()
            assert b'rank_entries' in err and b'invalid csrk handle' not in err, (name, err)
    lim = K.rank_entries_limits()
    args = (0, 12345, 0, 3, u, lim[0] + 1, v, lim[0] + 1, lim[0] + 1, VAL_F64, rk, sc)
    assert lib.csrk_rank_entries(*args) == ERR_UNSUPPORTED
    assert lib.csrk_rank_entries_device(*args, None) == ERR_UNSUPPORTED
    assert b'csrk_rank_entries_limits' in lib.csrk_last_error()
    assert np.all(ranks == 7) and np.all(scores == 7.0)


def test_no_cpu_fallback():
    "without a device rank_entries raises CsrkError naming hip; with one it computes (never on the CPU)"
    import torch
    from csr_amd._lib import CsrkError
    m, t = _mat(), _test_mat()
    U = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    V = np.array([[4.0, 1.0], [3.0, 2.0], [2.0, 3.0], [1.0, 4.0]])
    if torch.cuda.device_count() > 0:
        S = R.scores_plain(U, V)
        for ex in (True, False):
            got = m.rank_entries(U, V, t, exclude=ex, return_scores=True)
            assert np.array_equal(got[0], R.ranks(S, m.rowptrs if ex else None, m.colinds, t.rowptrs, t.colinds))
            assert np.array_equal(got[1], R.entry_scores(S, t.rowptrs, t.colinds))
        return
    for ex in (True, False):
        with pytest.raises(CsrkError) as ei:
            m.rank_entries(U, V, t, exclude=ex)
        assert 'hip' in str(ei.value).lower()


# ---- the reference checks itself --------------------------------------------------------------------------------

def _rk(row, test, seen=None):
    S = np.array([row], np.float64)
    rp = None if seen is None else np.array([0, len(seen)])
    return R.ranks(S, rp, None if seen is None else np.array(seen, np.int32), np.array([0, len(test)]), np.array(test, np.int32)).tolist()


def test_ref_ties_go_to_the_smaller_item():
    assert _rk([1.0, 3.0, 3.0, 2.0, 3.0], [0, 1, 2, 3, 4]) == [4, 0, 1, 3, 2]
    assert _rk([5.0, 5.0, 5.0], [2, 1], seen=[0]) == [1, 0]


def test_ref_nan_above_inf_and_all_nans_tied():
    nan2 = np.array([0x7ff8000000000001, 0xfff8000000000000], np.uint64).view(np.float64)
    assert _rk([INF, nan2[0], 1.0, nan2[1], -INF], [0, 1, 2, 3, 4]) == [2, 0, 3, 1, 4]


def test_ref_signed_zeros_tie():
    assert _rk([-1.0, -0.0, 0.0, -0.0], [3, 2, 1, 0]) == [2, 1, 0, 3]
    assert _rk([0.0, -0.0], [1]) == [1]


def test_ref_seen_entries_repeats_and_full_rows():
    row = [0.5, 2.0, -1.0, 1.0, 3.0]
    assert _rk(row, [3]) == [2]
    assert _rk(row, [3], seen=[4]) == [1]
    assert _rk(row, [3], seen=[3, 4]) == [1]                       # an entry that seen stores is still ranked
    assert _rk(row, [0, 3, 0, 0]) == [3, 2, 3, 3]                  # a repeated test column: equal ranks
    assert _rk(row, [2, 0, 4, 1, 3], seen=[0, 1, 2, 3, 4]) == [0] * 5          # a fully seen row
    assert _rk(row, [2, 0], seen=[1]) == [3, 2]                    # the other test entry is an ordinary competitor
    assert R.ranks(np.zeros((2, 3)), None, None, np.array([0, 0, 0]), np.zeros(0, np.int32)).tolist() == []
    assert R.entry_scores(np.array([row]), np.array([0, 2]), np.array([3, 0])).tolist() == [1.0, 0.5]


def test_ref_tells_a_fused_chain_from_two_roundings_at_the_level_of_ranks():
    "a = 1 + 2^-30: the exact chain scores item 1 at 2^-60 and item 0 at +0.0; multiply-then-add scores both at 0"
    a = 1.0 + 2.0 ** -30
    U, V = np.array([[1.0, a]]), np.array([[0.0, 0.0], [-(1.0 + 2.0 ** -29), a]])
    rp, ci = np.array([0, 2]), np.array([0, 1], np.int32)
    Se, S2 = R.scores_exact(U, V), R.scores_two_rounding(U, V)
    assert Se[0].tolist() == [0.0, 2.0 ** -60] and S2[0].tolist() == [0.0, 0.0]
    assert R.ranks(Se, None, None, rp, ci).tolist() == [1, 0]
    assert R.ranks(S2, None, None, rp, ci).tolist() == [0, 1]
