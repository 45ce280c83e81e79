"""
csrk_rank_entries_for on the host side, without a GPU: the four entries are declared, exported, in the ctypes table and
reachable by raw address; the limits and the number of splits need no device and follow rule 11 of include/csrk.h, restated
here from the limits; every malformed request is refused with ValueError before any library call; the C entries refuse every
bad scalar and bad handle with its code and its exact text, and write nothing; without a device CSR.rank_entries_for fails
loudly.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import rank_entries_ref as R
import score_rules as RULES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('csrk_rank_entries_for', 'csrk_rank_entries_for_device', 'csrk_rank_entries_for_splits', 'csrk_rank_entries_for_limits')


def _mat(cols=((0, 3), (), (1, 2))):
    from csr_amd import CSR
    rp = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    ci = np.array([j for c in cols for j in c], np.int32)
    return CSR(3, 4, len(ci), rp, ci, None)


def test_entries_declared_exported_and_in_the_table():
    whole = open(os.path.join(ROOT, 'include', 'csrk.h')).read()
    text = re.sub(r'/\*.*?\*/', '', whole, flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, 'csr_amd', 'libcsrk.so'))
    from csr_amd import _lib
    from csr_amd.kernels import raw
    for name in NAMES:
        assert re.search(r'CSRK_API\s+int\s+' + name + r'\s*\(', text), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert raw.address(name)
    assert '(csrk_rank_entries_for splits them)' in whole


def test_limits_need_no_device():
    from csr_amd.kernels import hip as K
    from csr_amd._lib import lib, ERR_INVALID
    lim = K.rank_entries_for_limits()
    assert lim == (64, 512)                        # S_max, and two workgroups on each of 256 CUs
    assert lib.csrk_rank_entries_for_limits(None, 1) == ERR_INVALID
    two = (ctypes.c_int64 * 2)(-1, -1)
    assert lib.csrk_rank_entries_for_limits(two, 1) == 0 and two[0] == lim[0] and two[1] == -1


def test_splits_follow_rule_11():
    "(the restatement of rule 11 and the grid of requests: tests/score_rules.py, shared with test_score_plan_host.py)"
    from csr_amd.kernels import hip as K
    (s_max, W), rlim = K.rank_entries_for_limits(), K.rank_entries_limits()
    block, tile = rlim[1], rlim[2]
    assert (block, tile) == (64, 64)
    seen = set()
    for n_rows, n_items, splits, T in RULES.rule11_grid(s_max, W, tile):
        got = K.rank_entries_for_splits(n_rows, n_items, splits)
        assert got == RULES.rule11(n_rows, n_items, splits, s_max, W, block, tile), (n_rows, n_items, splits, got)
        assert 1 <= got <= max(1, min(T, s_max))          # forced splits above T and above S_max are clamped
        seen.add(got)
    assert {1, 2, 3, 5, s_max} <= seen
    # the cases the automatic choice is made for
    assert K.rank_entries_for_splits(1, 2_000_000) == 64 and K.rank_entries_for_splits(64, 2_000_000) == 64
    assert K.rank_entries_for_splits(65, 2_000_000) == 64 and K.rank_entries_for_splits(1024, 2_000_000) == 32
    assert K.rank_entries_for_splits(64 * W, 2_000_000) == 1 and K.rank_entries_for_splits(64 * W - 64, 2_000_000) == 2
    assert K.rank_entries_for_splits(64 * W + 1, 2_000_000) == 1 and K.rank_entries_for_splits(65536, 2_000_000) == 1
    assert K.rank_entries_for_splits(1, 65 * 64 + 3, 1000) == 64


def test_splits_refusals():
    from csr_amd.kernels import hip as K
    from csr_amd._lib import lib, ERR_INVALID
    s = ctypes.c_int32(7)
    rs = ctypes.byref(s)
    for args, text in (((-1, 5, 0), 'rank_entries_for: n_rows must not be negative (n_rows=-1)'),
                       ((1, -5, 0), 'rank_entries_for: n_items must not be negative (n_items=-5)'),
                       ((1, 5, -1), 'rank_entries_for: splits must not be negative (splits=-1)')):
        assert lib.csrk_rank_entries_for_splits(*args, rs) == ERR_INVALID, args
        assert lib.csrk_last_error().decode() == text
        assert s.value == 7
    assert lib.csrk_rank_entries_for_splits(1, 5, 0, None) == ERR_INVALID
    for bad in (dict(n_rows=1.0), dict(n_items=True), dict(splits=0), dict(splits=-2), dict(splits=2.0), dict(splits=True),
                dict(n_rows=-1), dict(n_items=2 ** 31)):
        kw = dict(dict(n_rows=4, n_items=100, splits=None), **bad)
        with pytest.raises(ValueError):
            K.rank_entries_for_splits(kw['n_rows'], kw['n_items'], kw['splits'])


def _bad():
    U, V = np.ones((3, 5)), np.ones((4, 5))
    return {
        'U rows': dict(U=np.ones((4, 5)), V=V),
        'V rows': dict(U=U, V=np.ones((5, 5))),
        '1-D U': dict(U=np.ones(3), V=V),
        'k differs': dict(U=U, V=np.ones((4, 4))),
        'k = 0': dict(U=np.ones((3, 0)), V=np.ones((4, 0))),
        'mixed dtypes': dict(U=U, V=V.astype(np.float32)),
        'integer panels': dict(U=U.astype(np.int64), V=V.astype(np.int64)),
        'users 2-D': dict(U=U, V=V, users=np.zeros((2, 2), np.int32)),
        'users a scalar': dict(U=U, V=V, users=1),
        'users float': dict(U=U, V=V, users=np.array([0.0, 1.0])),
        'users bool': dict(U=U, V=V, users=np.array([True, False])),
        'users strings': dict(U=U, V=V, users=np.array(['0'])),
        'users past the end': dict(U=U, V=V, users=np.array([0, 3, 1]), says='users[1] = 3 is outside [0, 3)'),
        'users negative': dict(U=U, V=V, users=np.array([1, 1, -1], np.int64), says='users[2] = -1 is outside [0, 3)'),
        'users beyond int32': dict(U=U, V=V, users=np.array([2 ** 32]), says=f'users[0] = {2 ** 32} is outside [0, 3)'),
        'splits = 0': dict(U=U, V=V, splits=0),
        'splits negative': dict(U=U, V=V, splits=-1),
        'splits a float': dict(U=U, V=V, splits=2.0),
        'splits a bool': dict(U=U, V=V, splits=True),
        'splits a string': dict(U=U, V=V, splits='auto'),
        'test an array': dict(U=U, V=V, test=np.ones((3, 4))),
        'test None': dict(U=U, V=V, test=None),
        'seen of another shape': dict(U=U, V=V, seen_shape=(3, 5)),
    }


@pytest.mark.parametrize('case', sorted(_bad()))
def test_bad_requests_raise_before_any_library_call(case, monkeypatch):
    from csr_amd.kernels import hip as K
    from csr_amd import _lib

    def forbidden(*a, **kw):
        raise AssertionError('library called')
    for name in NAMES + ('csrk_rank_entries', 'csrk_rank_entries_limits', 'csrk_row_nnzs', 'csrk_create'):
        monkeypatch.setattr(_lib.lib, name, forbidden)
    monkeypatch.setattr(K, 'to_handle', forbidden)
    kw = dict(_bad()[case])
    U, V, users, says = kw.pop('U'), kw.pop('V'), kw.pop('users', np.array([2, 0, 2])), kw.pop('says', None)
    t = K.hip_h(12345, 3, 4, 4)
    s = K.hip_h(12346, *kw.pop('seen_shape', (3, 4)), 4)
    test_h = kw.pop('test', t)
    for seen_h in (s, None):
        if seen_h is None and case == 'seen of another shape':
            continue
        with pytest.raises(ValueError) as ei:
            K.rank_entries_for_args(seen_h, test_h, users, U, V, kw.get('splits'))
        assert says is None or says in str(ei.value)
        with pytest.raises(ValueError):
            K.rank_entries_for(seen_h, test_h, users, U, V, kw.get('splits'))
    if case == 'seen of another shape':
        return
    test = _mat() if test_h is t else test_h
    for ex in (True, False):
        with pytest.raises(ValueError):
            _mat().rank_entries_for(users, U, V, test, exclude=ex, **kw)


def test_args_and_the_empty_list(monkeypatch):
    from csr_amd.kernels import hip as K
    from csr_amd import _lib
    U, V = np.ones((3, 5), np.float32), np.ones((4, 5), np.float32)
    t = K.hip_h(12345, 3, 4, 4)
    a = K.rank_entries_for_args(None, t, [2, 0, 2], U, V, 3)
    assert a[0].dtype == np.int32 and a[0].tolist() == [2, 0, 2] and a[2] == 5 and a[4] == 5 and a[5:] == (5, _lib.VAL_F32, 3, 3)
    assert K.rank_entries_for_args(t, t, np.array([1], np.uint8), U, V)[7:] == (0, 3)          # automatic is 0
    for name in NAMES + ('csrk_row_nnzs', 'csrk_create'):
        monkeypatch.setattr(_lib.lib, name, lambda *a, **kw: (_ for _ in ()).throw(AssertionError('library called')))
    for users in ([], np.zeros(0, np.int64)):
        rk, sc = K.rank_entries_for(None, t, users, U, V)
        assert rk.shape == (0,) and rk.dtype == np.int32 and sc.shape == (0,) and sc.dtype == np.float64


def _call(form, p, **ch):
    "the C entry on host arrays; every default but the handles is a valid request"
    from csr_amd._lib import lib, VAL_F64
    a = dict(dict(s=0, t=12345, rows=p['rows'], nr=3, ur=3, u=p['u'], ldu=2, v=p['v'], ldv=2, k=2, pt=VAL_F64, off=p['off'], no=4,
                  rk=p['rk'], sc=p['sc'], sp=0), **ch)
    head = (a['s'], a['t'], a['rows'], a['nr'], a['ur'], a['u'], a['ldu'], a['v'], a['ldv'], a['k'], a['pt'])
    if form == 'host':
        return lib.csrk_rank_entries_for(*head, a['rk'], a['sc'], a['no'], a['sp'])
    return lib.csrk_rank_entries_for_device(*head, a['off'], a['no'], a['rk'], a['sc'], a['sp'], None)


def test_scalar_and_handle_refusals_have_their_code_and_exact_text():
    "the scalars are answered whatever the handles are, in csrk_rank_entries' order; then the handles: no GPU, nothing written"
    from csr_amd._lib import lib, ERR_INVALID, ERR_UNSUPPORTED
    from csr_amd.kernels import hip as K
    U, V, rows, off = np.ones((3, 2)), np.ones((4, 2)), np.array([2, 0, 2], np.int32), np.array([0, 2, 2, 4], np.int64)
    ranks, scores = np.full(4, 7, np.int32), np.full(4, 7.0)
    p = dict(rows=rows.ctypes.data, u=U.ctypes.data, v=V.ctypes.data, off=off.ctypes.data, rk=ranks.ctypes.data, sc=scores.ctypes.data)
    kmax = K.rank_entries_limits()[0]
    P = 'rank_entries_for: '
    both = [
        (dict(k=0), ERR_INVALID, P + 'k must be at least 1 (k=0)'),
        (dict(ldu=1), ERR_INVALID, P + 'bad panel geometry k=2 ldu=1 ldv=2'),
        (dict(ldv=1), ERR_INVALID, P + 'bad panel geometry k=2 ldu=2 ldv=1'),
        (dict(pt=7), ERR_INVALID, P + 'panel_type must be CSRK_VAL_F32 or CSRK_VAL_F64, not 7'),
        (dict(nr=-1), ERR_INVALID, P + 'n_rows must not be negative (n_rows=-1)'),
        (dict(ur=-1), ERR_INVALID, P + 'u_rows must not be negative (u_rows=-1)'),
        (dict(sp=-1), ERR_INVALID, P + 'splits must not be negative (splits=-1)'),
        (dict(no=-1), ERR_INVALID, P + 'n_out must not be negative (n_out=-1)'),
        (dict(k=kmax + 1, ldu=kmax + 1, ldv=kmax + 1), ERR_UNSUPPORTED,
         P + f'k={kmax + 1} is above the largest supported k={kmax} (csrk_rank_entries_limits)'),
        # the first of two faults is the one named; an invalid scalar comes before the unsupported k
        (dict(k=0, pt=7), ERR_INVALID, P + 'k must be at least 1 (k=0)'),
        (dict(pt=7, nr=-1), ERR_INVALID, P + 'panel_type must be CSRK_VAL_F32 or CSRK_VAL_F64, not 7'),
        (dict(nr=-1, sp=-1), ERR_INVALID, P + 'n_rows must not be negative (n_rows=-1)'),
        (dict(sp=-1, k=kmax + 1, ldu=kmax + 1, ldv=kmax + 1), ERR_INVALID, P + 'splits must not be negative (splits=-1)'),
    ]
    for form in ('host', 'device'):
        for ch, code, text in both:
            for t in (12345, 0):                   # whatever the handles are
                assert _call(form, p, t=t, **ch) == code, (form, ch)
                assert lib.csrk_last_error().decode() == text, (form, ch)
        for ch in (dict(t=12345), dict(t=777), dict(t=0), dict(s=12345)):
            assert _call(form, p, **ch) == ERR_INVALID and b'invalid csrk handle' in lib.csrk_last_error(), (form, ch)
        assert _call(form, p, nr=0, no=0, rows=None, u=None, v=None, rk=None, sc=None, off=None) == ERR_INVALID      # (no handle: still refused)
    assert np.all(ranks == 7) and np.all(scores == 7.0)


def test_no_cpu_fallback():
    "without a device rank_entries_for raises CsrkError naming hip; with one it computes (never on the CPU)"
    import torch
    from csr_amd._lib import CsrkError
    seen, test = _mat(), _mat(((1, 2), (0,), (3, 0, 3)))
    U = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    V = np.array([[4.0, 1.0], [3.0, 2.0], [2.0, 3.0], [1.0, 4.0]])
    users = np.array([2, 0, 2, 1])
    if torch.cuda.device_count() > 0:
        S = R.scores_plain(U, V)[users]
        trp = np.concatenate([[0], np.cumsum(np.diff(test.rowptrs)[users])])
        tci = np.concatenate([test.colinds[test.rowptrs[u]:test.rowptrs[u + 1]] for u in users])
        srp = np.concatenate([[0], np.cumsum(np.diff(seen.rowptrs)[users])])
        sci = np.concatenate([seen.colinds[seen.rowptrs[u]:seen.rowptrs[u + 1]] for u in users])
        for ex in (True, False):
            rk, sc, off = seen.rank_entries_for(users, U, V, test, exclude=ex, return_scores=True, return_offsets=True)
            assert np.array_equal(rk, R.ranks(S, srp if ex else None, sci, trp, tci))
            assert np.array_equal(sc, R.entry_scores(S, trp, tci)) and np.array_equal(off, trp) and off.dtype == np.int64
        return
    for ex in (True, False):
        with pytest.raises(CsrkError) as ei:
            seen.rank_entries_for(users, U, V, test, exclude=ex)
        assert 'hip' in str(ei.value).lower()
