"""
csrk_rank_entries_for on the card (include/csrk.h), every output bit against the restatement of tests/rank_entries_ref.py
applied to the listed rows gathered in list order, and against csrk_rank_entries itself: a range as a list; shuffled lists
with repeats; every number of splits on one request, with rows of several sweeps; more tiles than S_max; `seen` across the
range boundaries; ties across ranges; special values and test columns that are no item; the variants of the device form,
with the traps of a missing clear and of -1 added once per split; agreement with csrk_topk_scores_for; every refusal with
the outputs untouched.

Panels lie on a grid (integers / 64) so that every product is exact and scores_plain is the chain; one small case runs
random float64 panels against exact rational arithmetic.  k is 1, 3, chunk, chunk + 1 and 2 * chunk + 5 on float64 and
float32 panels through both forms, so that all four instantiations of the kernel run.  At most 2 * block + 8 listed rows,
5 * tile + 5 items (six tiles; one case has 65 tiles + 3 items), 2 * T + 3 test entries in a row (block, tile, chunk and T
from csrk_rank_entries_limits).
"""
import ctypes as C

import numpy as np
import pytest

import rank_entries_ref as R
import topk_scores_ref as TR

pytestmark = pytest.mark.gpu

INF = np.inf
SPLITS = (1, 2, 3, 5, 6, 64, None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same(a, b):
    "equal bits, a NaN matching any NaN (a created NaN has its position specified, not its sign or payload)"
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _eq(got, want):
    return got[0].dtype == np.int32 and np.array_equal(got[0], want[0]) and _same(got[1], want[1])


@pytest.fixture(scope='module')
def lim():
    from csr_amd.kernels import hip as K
    return tuple(int(v) for v in K.rank_entries_limits())


def _grid(shape, rng):
    "float64 on a grid coarse enough that every product is exact"
    return rng.integers(-512, 512, shape) / 64.0


def _csr(nrows, ncols, cols, ptr64=False):
    "a pattern from one array of columns per row, kept in the order given"
    from csr_amd import CSR
    rp = np.zeros(nrows + 1, np.int64)
    rp[1:] = np.cumsum([len(c) for c in cols])
    ci = np.concatenate([np.asarray(c, np.int32) for c in cols] + [np.zeros(0, np.int32)]).astype(np.int32)
    return CSR(nrows, ncols, int(rp[-1]), rp.astype(np.int64 if ptr64 else np.int32), ci, None, _cast=False)


def _test_cols(m, ni, counts, rng):
    "counts[r] columns for row r, unsorted; distinct while they fit, then with repeats"
    cols = []
    for r in range(m):
        c = int(counts[r % len(counts)])
        own = rng.permutation(ni)[:c]
        if c > ni:
            own = rng.permutation(np.concatenate([own, rng.integers(0, ni, c - ni)]))
        cols.append(own.astype(np.int32))
    return cols


def _seen(tcols, ni, seed, ptr64=False):
    "row r: r % 4 = 0 empty, 1 full, 2 exactly the row's test items, 3 a random third"
    rng = np.random.default_rng(seed)
    cols = []
    for r, t in enumerate(tcols):
        kind = r % 4
        c = (np.zeros(0, np.int32), np.arange(ni), np.unique(t), np.flatnonzero(rng.random(ni) < 0.33))[kind]
        cols.append(np.asarray(c, np.int32))
    return _csr(len(tcols), ni, cols, ptr64)


def _gather(mat, users):
    "(rowptrs, colinds) of the listed rows, in list order"
    lens = np.diff(mat.rowptrs)[users]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ci = np.concatenate([mat.colinds[mat.rowptrs[u]:mat.rowptrs[u + 1]] for u in users] + [np.zeros(0, np.int32)])
    return rp, ci.astype(np.int32)


def _want(seen, test, U, V, users, S=None):
    "the restatement on the gathered rows; a test column that is no item: rank -1 and a NaN score (rule 1)"
    users = np.asarray(users, np.int64)
    S = (R.scores_plain(U, V) if S is None else S)[users]
    trp, tci = _gather(test, users)
    srp, sci = (None, None) if seen is None else _gather(seen, users)
    if srp is not None:                              # (a seen column that is no item excludes nothing)
        ok = (sci >= 0) & (sci < S.shape[1])
        srp = np.concatenate([[0], np.cumsum(ok)])[srp]
        sci = sci[ok]
    bad = (tci < 0) | (tci >= S.shape[1])
    rk = R.ranks(S, srp, sci, trp, np.where(bad, 0, tci))
    sc = R.entry_scores(S, trp, np.where(bad, 0, tci))
    rk[bad], sc[bad] = -1, np.nan
    return rk, sc


def _host(seen, test, users, U, V, splits=None):
    from csr_amd.kernels import hip as K, releasing
    with releasing(K.to_handle(test), K) as t:
        if seen is None:
            return K.rank_entries_for(None, t, users, U, V, splits)
        with releasing(K.to_handle(seen), K) as s:
            return K.rank_entries_for(s, t, users, U, V, splits)


def _range(seen, test, U, V, rows):
    from csr_amd.kernels import hip as K, releasing
    with releasing(K.to_handle(test), K) as t:
        if seen is None:
            return K.rank_entries(None, t, U, V, rows)
        with releasing(K.to_handle(seen), K) as s:
            return K.rank_entries(s, t, U, V, rows)


def _device(seen, test, users, U, V, splits=None, *, pad=0, shift=0, stream=False, repeat=1, scores=True, offsets=None, odd=False):
    """
    The device entry on torch tensors: panels with `pad` extra elements per row (NaN: reading them would show) starting
    `shift` elements into their allocation; rows and offsets 4 and 8 bytes into theirs with odd=True (aligned to the element
    only); ranks and scores are filled with garbage first and have three sentinels behind n_out, checked here.  Returns
    (ranks, scores) after the first call and asserts that every further call leaves the same bits.
    """
    import torch
    from csr_amd._lib import lib, check
    from csr_amd.kernels import hip as K
    code = K._PANEL_CODES[U.dtype]
    k = U.shape[1]
    users = np.asarray(users, np.int32)
    if offsets is None:
        ok = (users >= 0) & (users < test.nrows)
        offsets = np.concatenate([[0], np.cumsum(np.where(ok, np.diff(test.rowptrs)[np.where(ok, users, 0)], 0))])
    offsets = np.asarray(offsets, np.int64)
    ne = int(offsets[-1])
    keep = []

    def put(P):
        r, ld = P.shape[0], k + pad
        buf = torch.full((r * ld + shift + 1,), float('nan'), dtype=torch.from_numpy(P[:0]).dtype, device='cuda')
        if r:
            buf[shift:shift + r * ld].view(r, ld)[:, :k] = torch.from_numpy(np.ascontiguousarray(P)).cuda()
        keep.append(buf)
        return buf.data_ptr() + shift * P.dtype.itemsize, ld
    up, ldu = put(U)
    vp, ldv = put(V)
    rows_t = torch.from_numpy(np.concatenate([[-5] * odd, users]).astype(np.int32)).cuda()
    off_t = torch.from_numpy(np.concatenate([[-5] * odd, offsets]).astype(np.int64)).cuda()
    ranks = torch.full((ne + 3,), -77, dtype=torch.int32, device='cuda')
    sc = torch.full((ne + 3,), 77.0, dtype=torch.float64, device='cuda')
    t = K.to_handle(test)
    h = None if seen is None else K.to_handle(seen)
    outs = []
    try:
        s = torch.cuda.Stream() if stream else None
        torch.cuda.synchronize()
        for _ in range(repeat):
            check(lib.csrk_rank_entries_for_device(0 if h is None else h.H, t.H, rows_t.data_ptr() + 4 * odd, len(users), U.shape[0], up,
                                                   ldu, vp, ldv, k, code, off_t.data_ptr() + 8 * odd, ne, ranks.data_ptr(),
                                                   sc.data_ptr() if scores else None, K._splits(splits),
                                                   C.c_void_p(s.cuda_stream) if s else None))
            torch.cuda.synchronize()
            outs.append((ranks.cpu().numpy(), sc.cpu().numpy()))
    finally:
        K.release_handle(t)
        if h is not None:
            K.release_handle(h)
    for rk, ss in outs:
        assert np.all(rk[ne:] == -77) and np.all(ss[ne:] == 77.0)          # nothing behind n_out is written
        assert np.array_equal(rk, outs[0][0]) and np.array_equal(_bits(ss), _bits(outs[0][1]))
        if not scores:
            assert np.all(ss == 77.0)
    return outs[0][0][:ne], outs[0][1][:ne]


@pytest.fixture(scope='module')
def case(lim):
    "one request shared by the tests that need no shape of their own; the reference is computed once and left unchanged"
    B, T, TT = lim[1], lim[2], lim[4]
    rng = np.random.default_rng(1)
    m, ni, k = 2 * B + 8, 5 * T + 5, 2 * lim[3] + 5
    U, V = _grid((m, k), rng), _grid((ni, k), rng)
    V[T + 1] = V[3]                                                # ties across ranges
    V[4 * T + 2] = V[3]
    tcols = _test_cols(m, ni, [3, 0, TT + 2, 1, 2 * TT + 3, 0, 0, 6], rng)
    test = _csr(m, ni, tcols)
    seen = _seen(tcols, ni, 2)
    S = R.scores_plain(U, V)
    S.setflags(write=False)
    return dict(m=m, ni=ni, k=k, U=U, V=V, test=test, seen=seen, S=S)


# ---- 1. a range as a list ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('splits', SPLITS)
def test_a_range_as_a_list_is_rank_entries(case, lim, splits):
    B = lim[1]
    c = case
    for x, (b, e) in enumerate(((0, c['m']), (5, 9), (B - 2, B + 3), (1, 2 * B + 1), (7, 7))):
        users = np.arange(b, e)
        seen = c['seen'] if x % 2 == 0 else None
        want = _range(seen, c['test'], c['U'], c['V'], (b, e))
        got = _host(seen, c['test'], users, c['U'], c['V'], splits)
        assert _eq(got, want), (b, e, splits)
        if x < 2:
            assert _eq(got, _want(seen, c['test'], c['U'], c['V'], users, S=c['S'])), (b, e, splits)


# ---- 2. shuffled lists with repeats -----------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 63, 64, 65, 130])
def test_shuffled_lists_with_repeats(case, n):
    c = case
    rng = np.random.default_rng(20 + n)
    users = rng.integers(0, c['m'], n)
    if n > 2:
        users[n // 2] = users[0]                                   # a repeat for certain
        users[-1] = users[0]
    want = _want(c['seen'], c['test'], c['U'], c['V'], users, S=c['S'])
    for splits in (None, 1, 3):
        assert _eq(_host(c['seen'], c['test'], users, c['U'], c['V'], splits), want), (n, splits)
    # each occurrence has its own positions and the bits the row gets alone
    whole = _range(c['seen'], c['test'], c['U'], c['V'], None)
    rp = c['test'].rowptrs
    got = _host(c['seen'], c['test'], users, c['U'], c['V'], 2)
    at = 0
    for u in users:
        a, b = int(rp[u]), int(rp[u + 1])
        assert _eq((got[0][at:at + b - a], got[1][at:at + b - a]), (whole[0][a:b], whole[1][a:b])), u
        at += b - a
    assert at == len(got[0])


# ---- 3. every S gives the same bits ----------------------------------------------------------------------------------

def test_every_number_of_splits_gives_the_same_bits(case, lim):
    "rows of one, two and three sweeps (more than T and more than 2 T test entries) and empty test rows between full ones"
    c = case
    TT = lim[4]
    lens = np.diff(c['test'].rowptrs)
    users = np.concatenate([np.arange(0, 24), [c['m'] - 1, 4, 2, 4], np.arange(60, 70)])
    assert (lens[users] > TT).any() and (lens[users] > 2 * TT).any() and (lens[users] == 0).any()
    want = _want(c['seen'], c['test'], c['U'], c['V'], users, S=c['S'])
    for splits in (1, 2, 3, 4, 5, 6, 7, 64, None):
        assert _eq(_host(c['seen'], c['test'], users, c['U'], c['V'], splits), want), splits
        assert _eq(_device(c['seen'], c['test'], users, c['U'], c['V'], splits), want), splits
    f32 = (c['U'].astype(np.float32), c['V'].astype(np.float32))   # (the grid is exact in float32 too)
    assert np.array_equal(f32[0].astype(np.float64), c['U'])
    for splits in (1, 4, None):
        assert _eq(_host(c['seen'], c['test'], users, *f32, splits), want), splits


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('kk', ['1', '3', 'chunk', 'chunk + 1', '2 chunk + 5'])
def test_every_k_on_every_panel_path(lim, kk, dtype):
    """
    k = 1, 3, one full chunk (no tail, no further chunk within a tile), a chunk and a one-factor tail, two chunks and a tail,
    on float64 and float32 panels (the grid is exact in both), with and without `seen`, at S = 1 and S > 1.  The host form
    sends packed panels (16-B pieces when k is a whole number of them: k = chunk); the device form runs the same request with
    rows that start 16-B aligned (ld = k and ld = k + 4: pieces at k = chunk), and with rows that do not (element loads).
    """
    B, T, KC, TT = lim[1], lim[2], lim[3], lim[4]
    k = {'1': 1, '3': 3, 'chunk': KC, 'chunk + 1': KC + 1, '2 chunk + 5': 2 * KC + 5}[kk]
    rng = np.random.default_rng(300 + k)
    m, ni = B + 6, 5 * T + 5
    U, V = _grid((m, k), rng).astype(dtype), _grid((ni, k), rng).astype(dtype)
    assert np.array_equal(U.astype(np.float64).astype(dtype), U)
    tcols = _test_cols(m, ni, [2, 0, TT + 1, 5], rng)
    test = _csr(m, ni, tcols)
    seen = _seen(tcols, ni, 30 + k)
    S = R.scores_plain(U, V)
    users = np.concatenate([rng.permutation(m), [3, 3, m - 1]])                # two blocks of list rows, with repeats
    for sn in (seen, None):
        want = _want(sn, test, U, V, users, S=S)
        for splits in SPLITS:
            assert _eq(_host(sn, test, users, U, V, splits), want), (k, splits, sn is None)
        for kw in (dict(), dict(pad=4), dict(shift=1), dict(pad=1)):
            for splits in (1, 3):
                assert _eq(_device(sn, test, users, U, V, splits, **kw), want), (k, splits, kw, sn is None)
    assert _eq(_range(seen, test, U, V, (2, B + 3)), _want(seen, test, U, V, np.arange(2, B + 3), S=S))


def test_exact_random_float64(lim):
    "random float64 panels against exact rational arithmetic, every split"
    T = lim[2]
    rng = np.random.default_rng(3)
    m, ni, k = 3, 2 * T + 5, 5
    U, V = rng.standard_normal((m, k)), rng.standard_normal((ni, k))
    S = R.scores_exact(U, V)
    tcols = [rng.permutation(ni)[:9].astype(np.int32) for _ in range(m)]
    test, seen = _csr(m, ni, tcols), _seen(tcols, ni, 4)
    users = np.array([2, 0, 1, 2])
    want = _want(seen, test, U, V, users, S=S)
    for splits in (1, 2, 3, None):
        assert _eq(_host(seen, test, users, U, V, splits), want), splits


# ---- 4. more tiles than S_max ----------------------------------------------------------------------------------------

def test_more_tiles_than_s_max(lim):
    from csr_amd.kernels import hip as K
    T = lim[2]
    rng = np.random.default_rng(4)
    ni, k = 65 * T + 3, 3
    U, V = _grid((3, k), rng), _grid((ni, k), rng)
    tcols = [np.array([0, ni - 1, 64 * T, 7], np.int32), rng.integers(0, ni, 5).astype(np.int32), np.array([ni - 2], np.int32)]
    test = _csr(3, ni, tcols)
    seen = _csr(3, ni, [np.arange(0, ni, 3, dtype=np.int32), np.zeros(0, np.int32), np.arange(ni, dtype=np.int32)])
    users = np.array([0, 1, 2])
    want = _want(seen, test, U, V, users)
    assert K.rank_entries_for_splits(3, ni) == 64 and K.rank_entries_for_splits(3, ni, 1000) == 64
    for splits in (None, 64, 1000):
        assert _eq(_host(seen, test, users, U, V, splits), want), splits
    assert _eq(_range(seen, test, U, V, None), want)


# ---- 5. seen across the range boundaries -----------------------------------------------------------------------------

@pytest.mark.parametrize('s64,t64', [(False, False), (True, False), (False, True)])
def test_seen_across_range_boundaries(lim, s64, t64):
    T = lim[2]
    rng = np.random.default_rng(5)
    ni, k = 5 * T + 5, 4
    edges = sorted({j for q in range(1, 6) for j in (T * q - 1, T * q, T * q + 1)})
    tcols = [rng.permutation(ni)[:7].astype(np.int32) for _ in range(8)]
    scols = [np.array(edges),                                      # tile q - 1's last item, tile q's first two, for every q
             np.arange(ni),                                        # everything
             np.arange(2 * T, 4 * T),                              # exactly range 1 of three (and ranges 2, 3 of six)
             np.unique(tcols[3]),                                  # exactly its test items
             np.zeros(0),
             np.arange(0, 2 * T),                                  # exactly range 0 of three
             np.arange(4 * T, ni),                                 # exactly the last range of three
             np.array([0, ni - 1])]
    test = _csr(8, ni, tcols, ptr64=t64)
    seen = _csr(8, ni, [np.asarray(c, np.int32) for c in scols], ptr64=s64)
    U, V = _grid((8, k), rng), _grid((ni, k), rng)
    users = np.array([7, 0, 1, 2, 3, 4, 5, 6, 0])
    want = _want(seen, test, U, V, users)
    rp = np.concatenate([[0], np.cumsum(np.diff(test.rowptrs)[users])])
    assert np.all(want[0][rp[2]:rp[3]] == 0)                       # the row that has seen everything
    for splits in (1, 2, 3, 6, None):
        assert _eq(_host(seen, test, users, U, V, splits), want), splits


# ---- 6. ties across ranges -------------------------------------------------------------------------------------------

def test_ties_across_ranges(lim):
    T = lim[2]
    rng = np.random.default_rng(6)
    ni, m = 5 * T + 5, 5
    # V repeats five rows over and over: equal keys in every range, the smaller item first
    base = _grid((5, 3), rng)
    V = base[np.arange(ni) % 5]
    U = _grid((m, 3), rng)
    tcols = [np.array([0, ni - 1, T, T - 1, 3 * T + 2, 5, ni - 5], np.int32)] * m          # the first and the last tile among them
    test = _csr(m, ni, tcols)
    seen = _seen(tcols, ni, 7)
    users = np.array([4, 3, 2, 1, 0])
    want = _want(seen, test, U, V, users)
    for splits in (1, 2, 6, None):
        assert _eq(_host(seen, test, users, U, V, splits), want), splits
    # all scores equal: the rank is the number of unseen items below j
    Z = np.zeros((m, 3))
    got = _host(None, test, users, Z, V, 6)
    assert np.array_equal(got[0], np.tile(tcols[0], m)) and np.all(got[1] == 0.0) and not np.signbit(got[1]).any()
    assert _eq(_host(seen, test, users, Z, V, 5), _want(seen, test, Z, V, users))
    # ascending and descending scores
    up = np.arange(ni, dtype=np.float64)[:, None]
    one = np.arange(1, m + 1, dtype=np.float64)[:, None]
    j = np.tile(tcols[0], m).astype(np.int64)
    for name, Vx in (('ascending', up), ('descending', -up)):
        for splits in (1, 3, 6):
            got = _host(None, test, users, one, Vx, splits)
            assert np.array_equal(got[0], ni - 1 - j if name == 'ascending' else j), (name, splits)
        assert _eq(_host(seen, test, users, one, Vx, 6), _want(seen, test, one, Vx, users)), name


# ---- 7. special values -----------------------------------------------------------------------------------------------

def test_special_values_in_chosen_ranges(lim):
    T = lim[2]
    rng = np.random.default_rng(8)
    ni, m, k = 5 * T + 5, 6, 3
    U, V = _grid((m, k), rng), _grid((ni, k), rng)
    U[:, 0] = np.abs(U[:, 0]) + 1.0
    V[2, 1] = np.nan                                               # a NaN score in range 0 ...
    V[4 * T + 3, 2] = np.nan                                       # ... and one in the last
    V[T + 1, 0] = INF
    V[3 * T, 0] = INF
    V[2 * T + 5, 0] = -INF
    V[5 * T + 4, 0] = -INF
    tcols = [np.array([2, 4 * T + 3, T + 1, 3 * T, 2 * T + 5, 5 * T + 4, 0, ni - 2, T], np.int32)] * m
    test = _csr(m, ni, tcols)
    seen = _csr(m, ni, [np.array([2, 3 * T] if r % 2 else [], np.int32) for r in range(m)])
    users = np.array([5, 0, 3, 3, 1])
    want = _want(seen, test, U, V, users)
    assert np.isnan(want[1]).any() and np.isposinf(want[1]).any() and np.isneginf(want[1]).any()
    for splits in (1, 2, 6, None):
        assert _eq(_host(seen, test, users, U, V, splits), want), splits
    Un = U.copy()
    Un[3] = np.nan                                                 # all scores of a row NaN: all tied, the item decides
    got = _host(None, test, users, Un, V, 6)
    assert _eq(got, _want(None, test, Un, V, users)) and got[0][18:27].tolist() == tcols[0].tolist()


def test_signed_zeros_across_ranges(lim):
    T = lim[2]
    rng = np.random.default_rng(9)
    ni = 5 * T + 5
    Uz = np.array([[1e-200], [-1e-200]])
    Vz = rng.choice(np.array([-1e-200, 0.0, 1e-200, -3.0, 2.0]), ni)[:, None]
    Sz = R.scores_exact(Uz, Vz)
    assert np.signbit(Sz[Sz == 0.0]).any() and not np.signbit(Sz[Sz == 0.0]).all()
    test = _csr(2, ni, [np.arange(0, ni, 7, dtype=np.int32)[::-1]] * 2)
    users = np.array([1, 0, 1])
    want = _want(None, test, Uz, Vz, users, S=Sz)
    for splits in (1, 3, 6):
        got = _host(None, test, users, Uz, Vz, splits)
        assert _eq(got, want) and np.array_equal(np.signbit(got[1]), np.signbit(want[1])), splits


def test_bad_test_columns_get_minus_one_once_and_test_need_not_be_canonical(lim):
    "the trap of adding -1 once per split; unsorted and repeated test columns are just more entries"
    T = lim[2]
    rng = np.random.default_rng(10)
    ni, m, k = 5 * T + 5, 4, 5
    U, V = _grid((m, k), rng), _grid((ni, k), rng)
    tcols = [np.array([5, ni, 2, -1, 5, 2 ** 31 - 1, T + 2, 5, -2 ** 31], np.int32),
             np.array([ni + 7], np.int32),
             np.concatenate([rng.integers(0, ni, 40), [-3, ni], rng.integers(0, ni, 30)]).astype(np.int32),      # several sweeps
             np.array([3, 3, 1, 0, 1], np.int32)]
    test = _csr(m, ni, tcols)
    seen = _csr(m, ni, [np.array([5, T + 2], np.int32), np.arange(ni, dtype=np.int32), np.zeros(0, np.int32), np.array([1], np.int32)])
    users = np.array([3, 0, 1, 2, 0])
    want = _want(seen, test, U, V, users)
    assert np.count_nonzero(want[0] == -1) == 2 * 4 + 1 + 2
    for splits in (1, 6):
        for got in (_host(seen, test, users, U, V, splits), _device(seen, test, users, U, V, splits, repeat=2)):
            assert _eq(got, want), splits
            assert np.all(got[0][want[0] == -1] == -1) and np.isnan(got[1][want[0] == -1]).all()
    r0 = _host(seen, test, users, U, V, 3)[0][5:14]
    assert r0[0] == r0[4] == r0[7] >= 0 and r0[[1, 3, 5, 8]].tolist() == [-1] * 4


# ---- 8. the device form ----------------------------------------------------------------------------------------------

def test_device_form_variants(case, lim):
    c = case
    rng = np.random.default_rng(11)
    users = rng.integers(0, c['m'], 70)
    want = _want(c['seen'], c['test'], c['U'], c['V'], users, S=c['S'])
    for x, kw in enumerate((dict(), dict(pad=3), dict(shift=1), dict(pad=1, shift=1), dict(pad=4), dict(stream=True), dict(odd=True),
                            dict(pad=2, shift=3, stream=True, odd=True))):
        for splits in ((1, 6) if x < 2 else ((1, 3, None)[x % 3],)):
            assert _eq(_device(c['seen'], c['test'], users, c['U'], c['V'], splits, **kw), want), (kw, splits)
    # two calls into the same buffers, garbage in them before the first: the second equals the first (_device asserts it)
    for splits in (1, 2, 6):
        assert _eq(_device(c['seen'], c['test'], users, c['U'], c['V'], splits, repeat=2), want), splits
        got = _device(c['seen'], c['test'], users, c['U'], c['V'], splits, scores=False)              # scores may be NULL
        assert np.array_equal(got[0], want[0])
    f32 = (c['U'].astype(np.float32), c['V'].astype(np.float32))
    for kw in (dict(), dict(shift=1), dict(pad=4, shift=4)):
        assert _eq(_device(None, c['test'], users, *f32, 6, **kw), _want(None, c['test'], c['U'], c['V'], users, S=c['S'])), kw


def test_a_bad_row_index_in_the_device_list(case):
    "it is not dereferenced: nothing is written at its position and no neighbour changes"
    c = case
    good = np.array([9, 2, 70, 2, 4, 131])
    want = _want(c['seen'], c['test'], c['U'], c['V'], good, S=c['S'])
    lens = np.diff(c['test'].rowptrs)[good]
    users = np.array([9, -1, 2, 70, c['m'], 2, 4, 2 ** 31 - 1, 131, -2 ** 31])
    isbad = (users < 0) | (users >= c['m'])
    for splits in (1, 2, 6):
        got = _device(c['seen'], c['test'], users, c['U'], c['V'], splits)          # (a bad position has no entries)
        assert _eq(got, want), splits
    # S = 1 touches nothing else of ranks: two places reserved for every bad position keep the garbage
    gaps = np.zeros(len(users), np.int64)
    gaps[isbad] = 2
    gaps[~isbad] = lens
    off = np.concatenate([[0], np.cumsum(gaps)])
    rk, sc = _device(c['seen'], c['test'], users, c['U'], c['V'], 1, offsets=off)
    mine = np.concatenate([np.arange(off[r], off[r + 1]) for r in np.flatnonzero(~isbad)])
    hole = np.concatenate([np.arange(off[r], off[r + 1]) for r in np.flatnonzero(isbad)])
    assert _eq((rk[mine], sc[mine]), want) and np.all(rk[hole] == -77) and np.all(sc[hole] == 77.0)
    # offsets that are no prefix sum (every row wants to start near the end): unspecified ranks, nothing outside [0, n_out)
    ne = int(lens.sum())
    wild = np.concatenate([np.full(len(good), ne - 2), [ne]])
    _device(c['seen'], c['test'], good, c['U'], c['V'], 1, offsets=wild)            # (_device checks the sentinels)
    _device(c['seen'], c['test'], good, c['U'], c['V'], 6, offsets=np.concatenate([[-4], wild[1:]]))


# ---- 9. agreement with csrk_topk_scores_for --------------------------------------------------------------------------

def test_agrees_with_topk_scores_for(case):
    from csr_amd.kernels import hip as K, releasing
    c = case
    rng = np.random.default_rng(12)
    users = rng.integers(0, c['m'], 40)
    ranks, scores = _host(c['seen'], c['test'], users, c['U'], c['V'], 3)
    with releasing(K.to_handle(c['seen']), K) as h:
        tops = {n: K.topk_scores_for(h, users, c['U'], c['V'], n, None, 2) for n in (1, 20, 128)}
    trp = np.concatenate([[0], np.cumsum(np.diff(c['test'].rowptrs)[users])])
    tci = _gather(c['test'], users)[1]
    for n, (items, tsc, counts) in tops.items():
        hits = 0
        for r, u in enumerate(users):
            stored = set(c['seen'].colinds[c['seen'].rowptrs[u]:c['seen'].rowptrs[u + 1]].tolist())
            for e in range(trp[r], trp[r + 1]):
                j = int(tci[e])
                if j in stored or ranks[e] >= n:
                    continue
                assert items[r, ranks[e]] == j and _bits(tsc[r, ranks[e]]) == _bits(scores[e]), (n, r, j)
                hits += 1
        assert hits > 0 or n < 20, n


# ---- 10. refusals ----------------------------------------------------------------------------------------------------

def test_refusals_write_nothing(lim):
    import torch
    from csr_amd._lib import lib, ERR_INVALID, ERR_UNSUPPORTED, VAL_F64
    from csr_amd.kernels import hip as K
    m, ni, k = 5, 9, 3
    rng = np.random.default_rng(13)
    U, V = _grid((m, k), rng), _grid((ni, k), rng)
    test = _csr(m, ni, [np.array([3, 1], np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.array([8, 8, 0], np.int32),
                        np.array([2], np.int32)])
    good = _csr(m, ni, [np.array([1, 4], np.int32)] * m)
    bad = _csr(m, ni, [np.array([1, 4], np.int32), np.array([2, 7], np.int32), np.array([4, 4], np.int32), np.array([5, 2], np.int32),
                       np.zeros(0, np.int32)])
    wider, taller = _csr(m, ni + 1, [np.zeros(0, np.int32)] * m), _csr(m + 1, ni, [np.zeros(0, np.int32)] * (m + 1))
    ht, hg, hb, hw, hl = (K.to_handle(x) for x in (test, good, bad, wider, taller))
    rows = np.array([3, 0, 3, 1], np.int32)
    off = np.array([0, 3, 5, 8, 8], np.int64)
    ne = 8
    P = b'rank_entries_for: '
    try:
        for form in ('host', 'device'):
            if form == 'host':
                ranks, scores = np.full(ne, 7, np.int32), np.full(ne, 7.0)
                p = dict(rows=rows.ctypes.data, off=off.ctypes.data, u=U.ctypes.data, v=V.ctypes.data, rk=ranks.ctypes.data,
                         sc=scores.ctypes.data)
            else:
                tU, tV = torch.from_numpy(U).cuda(), torch.from_numpy(V).cuda()
                tr, to = torch.from_numpy(np.concatenate([rows, [0]])).cuda(), torch.from_numpy(np.concatenate([off, [0]])).cuda()
                ranks = torch.full((ne,), 7, dtype=torch.int32, device='cuda')
                scores = torch.full((ne,), 7.0, dtype=torch.float64, device='cuda')
                p = dict(rows=tr.data_ptr(), off=to.data_ptr(), u=tU.data_ptr(), v=tV.data_ptr(), rk=ranks.data_ptr(), sc=scores.data_ptr())

            def call(**ch):
                a = dict(dict(s=hg.H, t=ht.H, nr=4, ur=m, ldu=k, ldv=k, k=k, pt=VAL_F64, no=ne, sp=0, **p), **ch)
                head = (a['s'], a['t'], a['rows'], a['nr'], a['ur'], a['u'], a['ldu'], a['v'], a['ldv'], a['k'], a['pt'])
                if form == 'host':
                    return lib.csrk_rank_entries_for(*head, a['rk'], a['sc'], a['no'], a['sp'])
                return lib.csrk_rank_entries_for_device(*head, a['off'], a['no'], a['rk'], a['sc'], a['sp'], None)
            invalid = {'k < 1': dict(k=0), 'ldu < k': dict(ldu=k - 1), 'ldv < k': dict(ldv=k - 1), 'panel type': dict(pt=9),
                       'n_rows < 0': dict(nr=-1), 'u_rows < 0': dict(ur=-1), 'splits < 0': dict(sp=-1), 'n_out < 0': dict(no=-1),
                       'u_rows != nrows': dict(ur=m + 1), 'u_rows short': dict(ur=m - 1),
                       'seen wider': dict(s=hw.H), 'seen taller': dict(s=hl.H), 'not canonical': dict(s=hb.H),
                       'seen not a handle': dict(s=12345), 'test not a handle': dict(t=12345), 'test 0': dict(t=0),
                       'NULL rows': dict(rows=None), 'NULL ranks': dict(rk=None), 'NULL U': dict(u=None), 'NULL V': dict(v=None),
                       'misaligned rows': dict(rows=p['rows'] + 2), 'misaligned U': dict(u=p['u'] + 4),
                       'misaligned ranks': dict(rk=p['rk'] + 2), 'misaligned scores': dict(sc=p['sc'] + 4)}
            if form == 'device':
                invalid.update({'NULL offsets': dict(off=None), 'misaligned offsets': dict(off=p['off'] + 4)})
            for name, ch in invalid.items():
                assert call(**ch) == ERR_INVALID, (form, name)
                if 'handle' not in name and name != 'test 0':
                    assert lib.csrk_last_error().startswith(P), (form, name)
                if name == 'not canonical':
                    assert b'row 2' in lib.csrk_last_error()          # the first bad row, as csrk_rank_entries names it
            assert call(k=lim[0] + 1, ldu=lim[0] + 1, ldv=lim[0] + 1) == ERR_UNSUPPORTED
            assert call(k=lim[0] + 1, ldu=lim[0] + 1, ldv=lim[0] + 1, t=12345) == ERR_UNSUPPORTED      # scalars first
            assert call(nr=64 * (2 ** 31 - 1) + 1, rows=None) == ERR_UNSUPPORTED
            assert b'more workgroups than a grid holds' in lib.csrk_last_error()
            if form == 'host':
                for lst, text in ((np.array([3, 5, 9, 1], np.int32), b'rows[1]=5 is outside [0, 5)'),
                                  (np.array([3, 0, 3, -4], np.int32), b'rows[3]=-4 is outside [0, 5)')):
                    assert call(rows=lst.ctypes.data) == ERR_INVALID and lib.csrk_last_error() == P + text
                for no in (7, 9, 0):
                    assert call(no=no) == ERR_INVALID
                    assert lib.csrk_last_error() == P + b'n_out=%d but the listed rows hold 8 test entries' % no
                assert call(nr=0, no=3, rows=None) == ERR_INVALID
                two = np.array([1, 2], np.int32)                   # rows without test entries: nothing launched
                assert call(rows=two.ctypes.data, nr=2, no=0, u=None, v=None, rk=None, sc=None) == 0
            else:
                assert call(no=0, u=None, v=None, rk=None, sc=None, rows=None, off=None) == 0       # nothing launched, nothing cleared
                torch.cuda.synchronize()
            assert call(nr=0, no=0, rows=None, off=None, u=None, v=None, rk=None, sc=None) == 0     # no rows: nothing launched
            if form == 'device':
                torch.cuda.synchronize()
                ranks, scores = ranks.cpu().numpy(), scores.cpu().numpy()
            assert np.all(ranks == 7) and np.all(scores == 7.0), form
        # the seen that was refused is fine as test; and the request the refusals were made of succeeds
        with pytest.raises(ValueError):
            K.rank_entries_for(hb, ht, rows, U, V)
        assert _eq(K.rank_entries_for(hg, hb, rows, U, V, 2), _want(good, bad, U, V, rows))
        assert _eq(K.rank_entries_for(hg, ht, rows, U, V), _want(good, test, U, V, rows))
    finally:
        for h in (ht, hg, hb, hw, hl):
            K.release_handle(h)
    # success at the largest k, and CSR.rank_entries_for with its offsets
    Uk, Vk = _grid((2, lim[0]), rng), _grid((70, lim[0]), rng)
    full = _csr(2, 70, [np.arange(70, dtype=np.int32)[::-1]] * 2)
    assert _eq(_host(None, full, [1, 0], Uk, Vk, 2), _want(None, full, Uk, Vk, [1, 0]))
    rk, sc, offs = good.rank_entries_for(rows, U, V, test, return_scores=True, return_offsets=True, splits=2)
    assert _eq((rk, sc), _want(good, test, U, V, rows)) and offs.dtype == np.int64 and offs.tolist() == off.tolist()
    assert np.array_equal(good.rank_entries_for(rows, U, V, test, exclude=False), _want(None, test, U, V, rows)[0])
    assert np.array_equal(good.rank_entries_for(rows, U, V, good), _want(good, good, U, V, rows)[0])      # one device copy for both
    assert TR.key(np.array([0.0]))[0] == TR.key(np.array([-0.0]))[0]
