"""
csrk_topk_scores_for on the host side, without a GPU: the four entries are declared, exported and in the ctypes table; the
limits and the workspace size need no device and follow rule 4 of include/csrk.h, restated here from the limits; every
malformed request is refused with ValueError before any library call; the C entries refuse every bad argument that needs no
handle with its code and its exact text, and write nothing; without a device CSR.topk_scores_for fails loudly.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import score_rules as RULES
import topk_scores_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('csrk_topk_scores_for', 'csrk_topk_scores_for_device', 'csrk_topk_scores_for_workspace', 'csrk_topk_scores_for_limits')
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
    assert '(csrk_topk_scores_for splits them)' in open(os.path.join(ROOT, 'include', 'csrk.h')).read()


def test_limits_need_no_device():
    from csr_amd.kernels import hip as K
    from csr_amd._lib import lib, ERR_INVALID
    lim = K.topk_scores_for_limits()
    assert lim == (64, 512, 256, 16, 12)          # rule 4's constants, and slots of 8 + 4 bytes per entry and 4 per count
    assert lib.csrk_topk_scores_for_limits(None, 1) == ERR_INVALID
    two = (ctypes.c_int64 * 2)(-1, -1)
    assert lib.csrk_topk_scores_for_limits(two, 1) == 0 and two[0] == lim[0] and two[1] == -1


def test_workspace_follows_rule_4():
    "(the restatement of rule 4 and the grid of requests: tests/score_rules.py, shared with test_score_plan_host.py)"
    from csr_amd.kernels import hip as K
    lim, tlim = K.topk_scores_for_limits(), K.topk_scores_limits()
    s_max, tile = lim[0], tlim[3]
    seen = set()
    for n in RULES.RULE4_NS:
        W = lim[1] if n <= 32 else lim[2]
        for n_rows, n_items, splits in RULES.rule4_grid(n, lim):
            got = K.topk_scores_for_workspace(n_rows, n_items, n, splits)
            assert got == RULES.rule4(n_rows, n_items, n, splits, lim, tlim), (n_rows, n_items, n, splits, got)
            assert (got[1] == 0) == (got[0] == 1) and got[1] % 16 == 0
            T = -(-n_items // tile)
            assert 1 <= got[0] <= max(1, min(T, s_max))          # forced splits above T and above S_max are clamped
            seen.add(got[0])
        assert K.topk_scores_for_workspace(64 * W, 2_000_000, n)[0] == 1          # as many row blocks as fill the card: no split
        assert K.topk_scores_for_workspace(65536, 2_000_000, n)[0] == 1
    assert {1, 2, 3, 5, s_max} <= seen
    # the cases the automatic choice is made for: one block of rows takes S_max ranges, 1 024 rows of n = 20 take 32
    assert K.topk_scores_for_workspace(1, 2_000_000, 20) == (64, 64 * (16 + 19 * 12))
    assert K.topk_scores_for_workspace(1024, 2_000_000, 20) == (32, 1024 * 32 * (16 + 19 * 12))
    assert K.topk_scores_for_workspace(1024, 2_000_000, 33) == (16, 1024 * 16 * (16 + 32 * 12))
    # linear in n_rows, S and n by [3] and [4]; an odd product is rounded up to 16
    assert K.topk_scores_for_workspace(3, 1000, 2, 3) == (3, 256)          # 3 * 3 * 28 = 252


def test_workspace_refusals():
    from csr_amd.kernels import hip as K
    from csr_amd._lib import lib, ERR_INVALID, ERR_UNSUPPORTED
    s, b = ctypes.c_int32(7), ctypes.c_int64(7)
    rs, rb = ctypes.byref(s), ctypes.byref(b)
    cases = [((-1, 5, 2, 0), ERR_INVALID, 'topk_scores_for: n_rows must not be negative (n_rows=-1)'),
             ((1, -5, 2, 0), ERR_INVALID, 'topk_scores_for: n_items must not be negative (n_items=-5)'),
             ((1, 5, 0, 0), ERR_INVALID, 'topk_scores_for: n_top must be at least 1 (n_top=0)'),
             ((1, 5, 2, -1), ERR_INVALID, 'topk_scores_for: splits must not be negative (splits=-1)'),
             ((1, 5, 129, 0), ERR_UNSUPPORTED,
              'topk_scores_for: n_top=129 is above the largest supported n_top=128 (csrk_topk_scores_limits)'),
             ((64 * 2 ** 31, 5, 2, 0), ERR_UNSUPPORTED,
              f'topk_scores_for: n_rows={64 * 2 ** 31} makes more row blocks than a grid holds ({2 ** 31 - 1})')]
    for args, code, text in cases:
        assert lib.csrk_topk_scores_for_workspace(*args, rs, rb) == code, args
        assert lib.csrk_last_error().decode() == text
        assert s.value == 7 and b.value == 7
    assert lib.csrk_topk_scores_for_workspace(1, 5, 2, 0, None, rb) == ERR_INVALID
    assert lib.csrk_topk_scores_for_workspace(64 * (2 ** 31 - 1), 5, 2, 0, rs, rb) == 0 and s.value == 1 and b.value == 0
    for bad in (dict(n_rows=1.0), dict(n=None), dict(n_items=True), dict(splits=0), dict(splits=-2), dict(splits=2.0), dict(splits=True),
                dict(n_rows=-1), dict(n=0), dict(n_items=2 ** 31)):
        kw = dict(dict(n_rows=4, n_items=100, n=3, splits=None), **bad)
        with pytest.raises(ValueError):
            K.topk_scores_for_workspace(kw['n_rows'], kw['n_items'], kw['n'], kw['splits'])


def _bad():
    U, V, users = np.ones((3, 5)), np.ones((4, 5)), np.array([2, 0, 2])
    return {
        'U rows': dict(U=np.ones((4, 5)), V=V),
        'V rows': dict(U=U, V=np.ones((5, 5))),
        '1-D U': dict(U=np.ones(3), V=V),
        'k differs': dict(U=U, V=np.ones((4, 4))),
        'k = 0': dict(U=np.ones((3, 0)), V=np.ones((4, 0))),
        'mixed dtypes': dict(U=U, V=V.astype(np.float32)),
        'integer panels': dict(U=U.astype(np.int64), V=V.astype(np.int64)),
        'n = 0': dict(U=U, V=V, n=0),
        'n a float': dict(U=U, V=V, n=2.0),
        'n a bool': dict(U=U, V=V, n=True),
        'min_score NaN': dict(U=U, V=V, min_score=float('nan')),
        'min_score a string': dict(U=U, V=V, min_score='0'),
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
    }


@pytest.mark.parametrize('case', sorted(_bad()))
def test_bad_requests_raise_before_any_library_call(case, monkeypatch):
    from csr_amd.kernels import hip as K
    from csr_amd import _lib

    def forbidden(*a, **kw):
        raise AssertionError('library called')
    for name in NAMES + ('csrk_topk_scores', 'csrk_topk_scores_limits', 'csrk_create'):
        monkeypatch.setattr(_lib.lib, name, forbidden)
    monkeypatch.setattr(K, 'to_handle', forbidden)
    kw = dict(_bad()[case])
    U, V, n, users, says = kw.pop('U'), kw.pop('V'), kw.pop('n', 2), kw.pop('users', np.array([2, 0, 2])), kw.pop('says', None)
    h = K.hip_h(12345, 3, 4, 4)
    with pytest.raises(ValueError) as ei:
        K.topk_scores_for_args(h, users, U, V, n, kw.get('min_score'), kw.get('splits'))
    assert says is None or says in str(ei.value)
    with pytest.raises(ValueError):
        K.topk_scores_for(h, users, U, V, n, kw.get('min_score'), kw.get('splits'))
    with pytest.raises(ValueError):
        _mat().topk_scores_for(users, U, V, n, **kw)
    with pytest.raises(ValueError):
        _mat().topk_scores_for(users, U, V, n, exclude=False, **kw)


def test_args_and_the_empty_list(monkeypatch):
    from csr_amd.kernels import hip as K
    from csr_amd import _lib
    U, V = np.ones((3, 5), np.float32), np.ones((7, 5), np.float32)
    a = K.topk_scores_for_args(None, [2, 0, 2], U, V, 4, None, 3)
    assert a[0].dtype == np.int32 and a[0].tolist() == [2, 0, 2] and a[2] == 5 and a[4] == 5 and a[5] == 7 and a[6] == 5
    assert a[8:] == (4, -INF, 3, 3)
    assert K.topk_scores_for_args(None, np.array([1], np.uint8), U, V, 1, 0.5)[9:] == (0.5, 0, 3)          # automatic is 0
    for name in ('csrk_topk_scores_for', 'csrk_topk_scores_for_device', 'csrk_create'):
        monkeypatch.setattr(_lib.lib, name, lambda *a, **kw: (_ for _ in ()).throw(AssertionError('library called')))
    for users in ([], np.zeros(0, np.int64)):
        it, sc, cn = K.topk_scores_for(None, users, U, V, 4)
        assert it.shape == (0, 4) and it.dtype == np.int32 and sc.shape == (0, 4) and sc.dtype == np.float64
        assert cn.shape == (0,) and cn.dtype == np.int32


def _call(form, **ch):
    "the C entry without a handle on host arrays; every default is a valid request"
    from csr_amd._lib import lib, VAL_F64
    a = dict(dict(h=0, rows=ch['_p']['rows'], nr=3, ur=3, u=ch['_p']['u'], ldu=2, v=ch['_p']['v'], ldv=2, ni=4, k=2, pt=VAL_F64, nt=2,
                  ms=-INF, it=ch['_p']['it'], ldi=2, sc=ch['_p']['sc'], lds=2, cn=ch['_p']['cn'], sp=0, wk=None, wb=0), **ch)
    args = (a['h'], a['rows'], a['nr'], a['ur'], a['u'], a['ldu'], a['v'], a['ldv'], a['ni'], a['k'], a['pt'], a['nt'], a['ms'], a['it'],
            a['ldi'], a['sc'], a['lds'], a['cn'], a['sp'])
    return lib.csrk_topk_scores_for(*args) if form == 'host' else lib.csrk_topk_scores_for_device(*args, a['wk'], a['wb'], None)


def test_handle_free_refusals_have_their_code_and_exact_text():
    "the argument checks of both C entries come before any device work: they need no GPU, and nothing is written"
    from csr_amd._lib import lib, ERR_INVALID, ERR_UNSUPPORTED
    from csr_amd.kernels import hip as K
    U, V, rows = np.ones((3, 2)), np.ones((4, 2)), np.array([2, 0, 2], np.int32)
    items, scores, counts = np.full((3, 2), 7, np.int32), np.full((3, 2), 7.0), np.full(3, 7, np.int32)
    work = np.full(64, 7, np.uint8)
    p = dict(rows=rows.ctypes.data, u=U.ctypes.data, v=V.ctypes.data, it=items.ctypes.data, sc=scores.ctypes.data, cn=counts.ctypes.data)
    lim = K.topk_scores_limits()
    P = 'topk_scores_for: '
    both = [
        (dict(k=0), ERR_INVALID, P + 'k must be at least 1 (k=0)'),
        (dict(nt=0), ERR_INVALID, P + 'n_top must be at least 1 (n_top=0)'),
        (dict(ni=-1), ERR_INVALID, P + 'n_items must not be negative (n_items=-1)'),
        (dict(ldu=1), ERR_INVALID, P + 'bad panel geometry k=2 ldu=1 ldv=2'),
        (dict(ldv=1), ERR_INVALID, P + 'bad panel geometry k=2 ldu=2 ldv=1'),
        (dict(ldi=1), ERR_INVALID, P + 'bad output geometry n_top=2 ldi=1 lds=2'),
        (dict(lds=1), ERR_INVALID, P + 'bad output geometry n_top=2 ldi=2 lds=1'),
        (dict(pt=7), ERR_INVALID, P + 'panel_type must be CSRK_VAL_F32 or CSRK_VAL_F64, not 7'),
        (dict(ms=float('nan')), ERR_INVALID, P + 'min_score is NaN'),
        (dict(nr=-1), ERR_INVALID, P + 'n_rows must not be negative (n_rows=-1)'),
        (dict(ur=-1), ERR_INVALID, P + 'u_rows must not be negative (u_rows=-1)'),
        (dict(sp=-1), ERR_INVALID, P + 'splits must not be negative (splits=-1)'),
        (dict(k=lim[0] + 1, ldu=lim[0] + 1, ldv=lim[0] + 1), ERR_UNSUPPORTED,
         P + f'k={lim[0] + 1} is above the largest supported k={lim[0]} (csrk_topk_scores_limits)'),
        (dict(nt=lim[1] + 1, ldi=lim[1] + 1, lds=lim[1] + 1), ERR_UNSUPPORTED,
         P + f'n_top={lim[1] + 1} is above the largest supported n_top={lim[1]} (csrk_topk_scores_limits)'),
        (dict(nr=64 * 2 ** 31), ERR_UNSUPPORTED, P + f'n_rows={64 * 2 ** 31} makes more row blocks than a grid holds ({2 ** 31 - 1})'),
        (dict(it=None), ERR_INVALID, P + 'items or scores is NULL'),
        (dict(sc=None), ERR_INVALID, P + 'items or scores is NULL'),
        (dict(rows=None), ERR_INVALID, P + 'rows is NULL'),
        (dict(u=None), ERR_INVALID, P + 'U is NULL'),
        (dict(v=None), ERR_INVALID, P + 'V is NULL'),
        # the order of the checks is csrk_topk_scores': the first of two faults is the one named
        (dict(k=0, nt=0), ERR_INVALID, P + 'k must be at least 1 (k=0)'),
        (dict(ms=float('nan'), nr=-1), ERR_INVALID, P + 'min_score is NaN'),
        (dict(sp=-1, nt=lim[1] + 1, ldi=lim[1] + 1, lds=lim[1] + 1), ERR_INVALID, P + 'splits must not be negative (splits=-1)'),
    ]
    for form in ('host', 'device'):
        for ch, code, text in both:
            assert _call(form, _p=p, **ch) == code, (form, ch)
            assert lib.csrk_last_error().decode() == text, (form, ch)
        for H in (12345, 777):
            assert _call(form, _p=p, h=H) == ERR_INVALID and b'invalid csrk handle' in lib.csrk_last_error()
        assert _call(form, _p=p, nr=0, rows=None, u=None, v=None, it=None, sc=None, cn=None) == 0          # no rows: nothing launched
    # the host form looks at the list before anything is sent: the first bad position and its value
    for bad, text in ((np.array([2, 3, 5], np.int32), 'rows[1]=3 is outside [0, 3)'), (np.array([0, 1, -4], np.int32), 'rows[2]=-4 is outside [0, 3)')):
        assert _call('host', _p=p, rows=bad.ctypes.data) == ERR_INVALID
        assert lib.csrk_last_error().decode() == P + text
    # the device form and its workspace: 130 items are 3 tiles, so splits = 2 needs 3 * 2 * 28 = 168 -> 176 bytes
    assert K.topk_scores_for_workspace(3, 130, 2, 2) == (2, 176)
    wk = work.ctypes.data + (-work.ctypes.data % 16)
    for ch, text in ((dict(wk=None, wb=176), 'the workspace is NULL but 176 bytes are needed (splits_used=2)'),
                     (dict(wk=wk + 8, wb=176), 'the workspace is not aligned to 16 bytes'),
                     (dict(wk=wk, wb=175), 'work_bytes=175 but 176 bytes are needed (splits_used=2)')):
        assert _call('device', _p=p, ni=130, sp=2, **ch) == ERR_INVALID, ch
        assert lib.csrk_last_error().decode() == P + text
    assert np.all(items == 7) and np.all(scores == 7.0) and np.all(counts == 7) and np.all(work == 7)


def test_no_cpu_fallback():
    "without a device topk_scores_for raises CsrkError naming hip; with one it computes (never on the CPU)"
    import torch
    from csr_amd._lib import CsrkError
    m = _mat()
    U = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    V = np.array([[4.0, 1.0], [3.0, 2.0], [2.0, 3.0], [1.0, 4.0]])
    users = np.array([2, 0, 2, 1])
    if torch.cuda.device_count() > 0:
        for ex in (True, False):
            got = m.topk_scores_for(users, U, V, 2, exclude=ex)
            rp = np.concatenate([[0], np.cumsum(np.diff(m.rowptrs)[users])])
            ci = np.concatenate([m.colinds[m.rowptrs[u]:m.rowptrs[u + 1]] for u in users])
            want = R.select(R.scores_plain(U, V)[users], rp if ex else None, ci, 2)
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
        return
    for ex in (True, False):
        with pytest.raises(CsrkError) as ei:
            m.topk_scores_for(users, U, V, 2, exclude=ex)
        assert 'hip' in str(ei.value).lower()
