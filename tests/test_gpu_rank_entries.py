"""
csrk_rank_entries on the card (include/csrk.h), every output bit against the restatement of tests/rank_entries_ref.py: the
chain against exact rational arithmetic on random float64 panels (where multiply-then-add is shown to give other scores, and
other ranks on the a = 1 + 2^-30 case); against the vectorised loop on panels whose products are exact at every row-block,
tile, chunk and list boundary that csrk_rank_entries_limits names; every kind of seen row; ascending, descending, equal and
special scores; a test matrix that is not canonical; agreement with csrk_topk_scores; the same bits from every variant of
one request; every refusal with the outputs untouched.

Matrices have at most 2 * block + 8 rows, 3 * tile + 5 items and 2 * T + 3 test entries in a row (block, tile and T from the
limits).  The exact chain costs about 10^5 steps (rows x items x k) a second: the exact cases are sized by that.
"""
import ctypes as C

import numpy as np
import pytest

import rank_entries_ref as R
import topk_scores_ref as TR

pytestmark = pytest.mark.gpu

INF = np.inf


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


def _f32(shape, rng):
    return rng.standard_normal(shape).astype(np.float32)


def _csr(nrows, ncols, cols, ptr64=False, values=False):
    "a pattern from one array of columns per row, kept in the order given"
    from csr_amd import CSR
    rp = np.zeros(nrows + 1, np.int64)
    rp[1:] = np.cumsum([len(c) for c in cols])
    ci = np.concatenate([np.asarray(c, np.int32) for c in cols] + [np.zeros(0, np.int32)]).astype(np.int32)
    vs = np.full(len(ci), np.nan) if values else None          # never read: NaN would show
    return CSR(nrows, ncols, int(rp[-1]), rp.astype(np.int64 if ptr64 else np.int32), ci, vs, _cast=False)


def _test_cols(m, ni, counts, rng):
    "counts[r] columns for row r, unsorted; distinct while they fit, then with repeats"
    cols = []
    for r in range(m):
        c = int(counts[r % len(counts)])
        if ni == 0:
            c = 0
        own = rng.permutation(ni)[:c]
        if c > ni:
            own = rng.permutation(np.concatenate([own, rng.integers(0, ni, c - ni)]))
        cols.append(own.astype(np.int32))
    return cols


def _seen(tcols, ni, seed, ptr64=False, values=False):
    "row r: r % 4 = 0 empty, 1 full, 2 exactly the row's test items, 3 a random third"
    rng = np.random.default_rng(seed)
    cols = []
    for r, t in enumerate(tcols):
        kind = r % 4
        if kind == 0:
            c = np.zeros(0, np.int32)
        elif kind == 1:
            c = np.arange(ni, dtype=np.int32)
        elif kind == 2:
            c = np.unique(t)
        else:
            c = np.flatnonzero(rng.random(ni) < 0.33)
        cols.append(c.astype(np.int32))
    return _csr(len(tcols), ni, cols, ptr64, values)


def _host(seen, test, U, V, rows=None):
    from csr_amd.kernels import hip as K, releasing
    with releasing(K.to_handle(test), K) as t:
        if seen is None:
            return K.rank_entries(None, t, U, V, rows)
        with releasing(K.to_handle(seen), K) as s:
            return K.rank_entries(s, t, U, V, rows)


def _want(seen, test, U, V, rows=None, S=None):
    S = R.scores_plain(U, V) if S is None else S
    rb, re_ = (0, S.shape[0]) if rows is None else rows
    trp = test.rowptrs[rb:re_ + 1]
    rk = R.ranks(S[rb:re_], None if seen is None else seen.rowptrs[rb:re_ + 1], None if seen is None else seen.colinds, trp, test.colinds)
    return rk, R.entry_scores(S[rb:re_], trp, test.colinds)


def _device(seen, test, U, V, rows=None, *, pad=0, shift=0, stream=False, repeat=1, scores=True):
    """
    The device entry on torch tensors: panels with `pad` extra elements per row (NaN: reading them would show) starting
    `shift` elements into their allocation; the outputs have three sentinels behind the last entry, checked here.
    """
    import torch
    from csr_amd._lib import lib, check
    from csr_amd.kernels import hip as K
    code = K._PANEL_CODES[U.dtype]
    rb, re_ = (0, U.shape[0]) if rows is None else rows
    k = U.shape[1]
    ne = int(test.rowptrs[re_]) - int(test.rowptrs[rb])
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
    ranks = torch.full((ne + 3,), -77, dtype=torch.int32, device='cuda')
    sc = torch.full((ne + 3,), 77.0, dtype=torch.float64, device='cuda')
    t = K.to_handle(test)
    h = None if seen is None else K.to_handle(seen)
    try:
        s = torch.cuda.Stream() if stream else None
        torch.cuda.synchronize()
        for _ in range(repeat):
            check(lib.csrk_rank_entries_device(0 if h is None else h.H, t.H, rb, re_, up, ldu, vp, ldv, k, code, ranks.data_ptr(),
                                               sc.data_ptr() if scores else None, C.c_void_p(s.cuda_stream) if s else None))
        torch.cuda.synchronize()
    finally:
        K.release_handle(t)
        if h is not None:
            K.release_handle(h)
    ranks, sc = ranks.cpu().numpy(), sc.cpu().numpy()
    assert np.all(ranks[ne:] == -77) and np.all(sc[ne:] == 77.0)          # nothing else is written
    if not scores:
        assert np.all(sc == 77.0)
    return ranks[:ne], sc[:ne]


def _full(m, ni):
    return _csr(m, ni, [np.arange(ni, dtype=np.int32)] * m)


# ---- 1. the chain against exact arithmetic ------------------------------------------------------------------------

def test_exact_random_float64_where_two_roundings_fail():
    rng = np.random.default_rng(7)
    U, V = rng.standard_normal((2, 8)), rng.standard_normal((40, 8))
    S, S2 = R.scores_exact(U, V), R.scores_two_rounding(U, V)
    test = _full(2, 40)
    want = _want(None, test, U, V, S=S)
    other = _want(None, test, U, V, S=S2)
    print('scores that differ', np.count_nonzero(S2 != S), 'of', S.size, '; ranks that differ', np.count_nonzero(want[0] != other[0]))
    for got in (_host(None, test, U, V), _device(None, test, U, V)):
        assert _eq(got, want)
        assert not _eq(got, other)          # a kernel that multiplies and then adds would not have passed
    seen = _seen([np.arange(40)] * 2, 40, 1)
    assert _eq(_host(seen, test, U, V), _want(seen, test, U, V, S=S))


def test_exact_fused_chain_decides_a_rank():
    "a = 1 + 2^-30: item 1 scores 2^-60 under the fused chain and wins; multiply-then-add ties both at 0 and item 0 wins"
    a = 1.0 + 2.0 ** -30
    U, V = np.array([[1.0, a]]), np.array([[0.0, 0.0], [-(1.0 + 2.0 ** -29), a]])
    test = _full(1, 2)
    assert R.ranks(R.scores_two_rounding(U, V), None, None, test.rowptrs, test.colinds).tolist() == [0, 1]
    for got in (_host(None, test, U, V), _device(None, test, U, V)):
        assert got[0].tolist() == [1, 0] and got[1].tolist() == [0.0, 2.0 ** -60]


@pytest.mark.parametrize('k', [1, 7, 16, 17, 33])
def test_exact_random_float64_every_k(k):
    rng = np.random.default_rng(70 + k)
    U, V = rng.standard_normal((5, k)), rng.standard_normal((70, k))
    S = R.scores_exact(U, V)
    test = _full(5, 70)
    seen = _seen([np.arange(3 * r, 3 * r + 9) for r in range(5)], 70, k)
    assert _eq(_host(seen, test, U, V), _want(seen, test, U, V, S=S))
    assert _eq(_device(None, test, U, V, rows=(1, 4)), _want(None, test, U, V, rows=(1, 4), S=S))


# ---- 2. every boundary, on panels whose products are exact ---------------------------------------------------------

def _check(m, ni, k, counts, seed, lim, first=3):
    "one case on both kinds of panel, rows [first, first + m) of a taller U, through both forms"
    for y, gen in enumerate((_grid, _f32)):
        rng = np.random.default_rng(100 * seed + y)
        U, V = gen((m + first + 2, k), rng), gen((ni, k), rng)
        tcols = _test_cols(m + first + 2, ni, counts, rng)
        test = _csr(m + first + 2, ni, tcols, ptr64=bool((seed + y) % 2))
        seen = _seen(tcols, ni, seed, ptr64=bool(seed % 3 == 0))
        S = R.scores_plain(U, V)
        rr = (first, first + m)
        form = _host if (seed + y) % 2 else _device
        assert _eq(form(seen, test, U, V, rr), _want(seen, test, U, V, rr, S=S)), (gen.__name__, m, ni, k, counts)


def test_every_row_count(lim):
    B = lim[1]
    for x, m in enumerate(sorted({1, B - 1, B, B + 1, 2 * B + 8} - {0})):
        _check(m, 70, 5, [2, 0, 5, 1, 3], x, lim)


def test_every_item_count(lim):
    T = lim[2]
    for x, ni in enumerate(sorted({1, T - 1, T, T + 1, 3 * T + 5} - {0})):
        _check(6, ni, 5, [2, 0, 5, 1, 3], 10 + x, lim)


def test_every_k(lim):
    KC = lim[3]
    for x, k in enumerate(sorted({1, KC - 1, KC, KC + 1, 4 * KC + 3} - {0})):
        _check(6, 70, k, [2, 0, 5, 1, 3], 20 + x, lim)


def test_every_number_of_test_entries_in_a_row(lim):
    T = lim[4]
    for x, c in enumerate(sorted({0, 1, T - 1, T, T + 1, 2 * T + 3})):
        _check(6, T + 9, 5, [2, c, 0, T + 2, 1], 30 + x, lim, first=0)          # (2 T + 3 > T + 9 items: repeats)


def test_long_rows_in_two_blocks(lim):
    "every row longer than a list, across a block border: each workgroup decides its own number of sweeps"
    B, T = lim[1], lim[4]
    _check(B + 3, 2 * T + 1, 17, [2 * T + 3, T + 1, 2 * T], 40, lim)


# ---- 3. the kinds of seen row ----------------------------------------------------------------------------------------

def test_seen_kinds_pointer_widths_and_values_never_read(lim):
    B, T = lim[1], lim[2]
    rng = np.random.default_rng(50)
    m, ni, k = B + 5, 2 * T + 5, 6
    U, V = _grid((m, k), rng), _grid((ni, k), rng)
    S = R.scores_plain(U, V)
    tcols = _test_cols(m, ni, [3, 1, 7, 0, 12], rng)
    test = _csr(m, ni, tcols)
    seen = _seen(tcols, ni, 5)
    want = _want(seen, test, U, V, S=S)
    assert all(np.all(want[0][test.rowptrs[r]:test.rowptrs[r + 1]] == 0) for r in range(1, m, 4))          # a fully seen row: rank 0
    assert _eq(_host(seen, test, U, V), want)
    assert _eq(_host(None, test, U, V), _want(None, test, U, V, S=S))
    for s64, t64 in ((True, False), (False, True), (True, True)):
        assert _eq(_host(_seen(tcols, ni, 5, ptr64=s64), _csr(m, ni, tcols, ptr64=t64), U, V), want), (s64, t64)
    assert _eq(_device(_seen(tcols, ni, 5, values=True), _csr(m, ni, tcols, values=True), U, V), want)
    # CSR.rank_entries: self is seen; exclude=False ranks among all items
    assert np.array_equal(seen.rank_entries(U, V, test), want[0])
    assert _eq(seen.rank_entries(U, V, test, exclude=False, return_scores=True), _want(None, test, U, V, S=S))
    assert _eq(seen.rank_entries(U, V, test, rows=(2, B + 1), return_scores=True), _want(seen, test, U, V, (2, B + 1), S=S))


# ---- 4. order --------------------------------------------------------------------------------------------------------

def test_ascending_descending_and_equal_scores(lim):
    B, T = lim[1], lim[2]
    m, ni = B + 1, 3 * T + 5
    rng = np.random.default_rng(60)
    U = (np.arange(m, dtype=np.float64) + 1.0)[:, None]
    up = np.arange(ni, dtype=np.float64)[:, None]
    tcols = _test_cols(m, ni, [4, 1, 9, 2], rng)
    test = _csr(m, ni, tcols)
    seen = _seen(tcols, ni, 6)
    for name, V in (('ascending', up), ('descending', -up)):
        got = _host(None, test, U, V)
        assert _eq(got, _want(None, test, U, V)), name
        j = test.colinds.astype(np.int64)
        assert np.array_equal(got[0], ni - 1 - j if name == 'ascending' else j)
        assert _eq(_host(seen, test, U, V), _want(seen, test, U, V)), name
    # U = 0: every score is +0.0 and the rank is the number of unseen items below j
    V = _grid((ni, 4), rng)
    Z = np.zeros((m, 4))
    got = _host(seen, test, Z, V)
    assert _eq(got, _want(seen, test, Z, V)) and np.all(got[1] == 0.0) and not np.signbit(got[1]).any()
    for r in range(m):
        unseen = np.ones(ni, bool)
        unseen[seen.colinds[seen.rowptrs[r]:seen.rowptrs[r + 1]]] = False
        for e in range(test.rowptrs[r], test.rowptrs[r + 1]):
            assert got[0][e] == np.count_nonzero(unseen[:test.colinds[e]])


def test_signed_zeros_tie_and_keep_their_sign():
    Uz, Vz = np.array([[1e-200], [-1e-200]]), np.array([[-1e-200], [0.0], [1e-200], [-3.0], [-1e-200]])
    Sz = R.scores_exact(Uz, Vz)
    assert np.signbit(Sz).tolist() == [[True, False, False, True, True], [False, False, True, False, False]]
    test = _csr(2, 5, [np.array([4, 3, 2, 1, 0], np.int32)] * 2)
    got = _host(None, test, Uz, Vz)
    assert _eq(got, _want(None, test, Uz, Vz, S=Sz))
    assert got[0].tolist() == [3, 4, 2, 1, 0, 4, 0, 3, 2, 1] and np.signbit(got[1][:5]).tolist() == [True, True, False, False, True]


def test_special_values(lim):
    T = lim[2]
    rng = np.random.default_rng(61)
    m, ni, j = 8, T + 7, T + 2
    U, V = _grid((m, 5), rng), _grid((ni, 5), rng)
    tcols = [np.array([j, 1, ni - 1, 5], np.int32)] * m
    test = _csr(m, ni, tcols)
    seen = _csr(m, ni, [np.array([j] if r % 2 else [], np.int32) for r in range(m)])
    base = _host(seen, test, U, V)
    Vn = V.copy()
    Vn[j, 3] = np.nan                                              # a NaN row of V: rank 0 for j; one more ahead of the others where unseen
    got = _host(seen, test, U, Vn)
    assert _eq(got, _want(seen, test, U, Vn))
    assert np.all(got[0][0::4] == 0) and np.isnan(got[1][0::4]).all()
    for r in range(0, m, 2):
        assert np.all(got[0][4 * r + 1:4 * r + 4] >= 1)
    for bad in (np.nan, INF, -INF):                                # a NaN or Inf in a row of U reaches that row only
        Ub = U.copy()
        Ub[2, 1] = bad
        got = _host(seen, test, Ub, V)
        assert _eq(got, _want(seen, test, Ub, V))
        keep = np.repeat(np.arange(m) != 2, 4)
        assert np.array_equal(got[0][keep], base[0][keep]) and np.array_equal(_bits(got[1][keep]), _bits(base[1][keep]))
    Un = U.copy()
    Un[2] = np.nan                                                 # all scores of the row NaN: all tied, the item decides
    got = _host(None, test, Un, V)
    assert _eq(got, _want(None, test, Un, V)) and got[0][8:12].tolist() == [j, 1, ni - 1, 5]
    # Inf - Inf inside a chain; 0 * Inf; no zero is skipped
    Ui = np.array([[INF, INF, 1.0], [0.0, 1.0, 1.0], [1.0, 1.0, 1.0]])
    Vi = np.array([[1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [INF, 0.0, 0.0], [0.0, 0.0, 2.0], [-INF, 1.0, 1.0]])
    ti = _full(3, 5)
    for si in (None, _csr(3, 5, [np.array([0, 2], np.int32)] * 3)):
        got = _host(si, ti, Ui, Vi)
        assert _eq(got, _want(si, ti, Ui, Vi))
        assert np.isnan(got[1]).reshape(3, 5).tolist() == TR.scores_positions(Ui, Vi)[0].tolist()
    assert _host(None, ti, Ui, Vi)[0].reshape(3, 5).tolist()[0] == [0, 4, 1, 2, 3]          # four NaNs by item, then +Inf


# ---- 5. a test matrix that is not canonical ------------------------------------------------------------------------

def test_unsorted_and_repeated_test_columns_in_storage_order(lim):
    T = lim[2]
    rng = np.random.default_rng(62)
    m, ni = 7, T + 3
    U, V = _f32((m, 9), rng), _f32((ni, 9), rng)
    S = R.scores_plain(U, V)
    rows = [np.array([5, 2, 5, 9, 2, 0, T + 2, 5], np.int32)] + [rng.integers(0, ni, 11).astype(np.int32) for _ in range(m - 1)]
    test = _csr(m, ni, rows)
    seen = _seen(rows, ni, 7)
    got = _host(seen, test, U, V)
    assert _eq(got, _want(seen, test, U, V, S=S))
    r0 = got[0][:8]
    assert r0[0] == r0[2] == r0[7] and r0[1] == r0[4] and len(set(r0.tolist())) == 5
    # the same rows in another order: the outputs move with their entries
    perm = [rng.permutation(len(c)) for c in rows]
    moved = _host(seen, _csr(m, ni, [c[p] for c, p in zip(rows, perm)]), U, V)
    at = 0
    for c, p in zip(rows, perm):
        assert np.array_equal(moved[0][at:at + len(c)], got[0][at:at + len(c)][p])
        assert np.array_equal(_bits(moved[1][at:at + len(c)]), _bits(got[1][at:at + len(c)][p]))
        at += len(c)


# ---- 6. agreement with csrk_topk_scores (rule 5) -------------------------------------------------------------------

def test_agrees_with_topk_scores(lim):
    from csr_amd.kernels import hip as K, releasing
    B, T = lim[1], lim[2]
    rng = np.random.default_rng(63)
    m, ni, k = 2 * B + 8, 3 * T + 5, 12
    U, V = _f32((m, k), rng), _f32((ni, k), rng)
    V[7] = V[3]                                                    # ties, so that the tie rules have to agree too
    tcols = _test_cols(m, ni, [10, 3, 25, 1, 0, 40], rng)
    test = _csr(m, ni, tcols)
    seen = _seen(tcols, ni, 8)
    ranks, scores = _host(seen, test, U, V)
    assert _eq((ranks, scores), _want(seen, test, U, V))
    with releasing(K.to_handle(seen), K) as h:
        tops = {n: K.topk_scores(h, U, V, n) for n in (1, 20, 128)}
    for n, (items, tsc, counts) in tops.items():
        hits = 0
        for r in range(m):
            stored = set(seen.colinds[seen.rowptrs[r]:seen.rowptrs[r + 1]].tolist())
            found = set()
            for e in range(test.rowptrs[r], test.rowptrs[r + 1]):
                j = int(test.colinds[e])
                if j in stored or ranks[e] >= n:
                    continue
                assert items[r, ranks[e]] == j and _bits(tsc[r, ranks[e]]) == _bits(scores[e]), (n, r, j)
                found.add(j)
            assert found == set(items[r, :counts[r]].tolist()) & set(tcols[r].tolist()), (n, r)
            hits += len(found)
        assert hits > 0 or n < 20, n


# ---- 7. invariance -----------------------------------------------------------------------------------------------------

def test_same_bits_from_every_variant(lim):
    B, T, TT = lim[1], lim[2], lim[4]
    rng = np.random.default_rng(64)
    m, ni = 2 * B + 3, 2 * T + 5
    for gen, k in ((_f32, 20), (_grid, 18), (_f32, 7)):
        U, V = gen((m, k), rng), gen((ni, k), rng)
        S = R.scores_plain(U, V)
        tcols = _test_cols(m, ni, [3, 0, TT + 2, 1, 6], rng)
        test = _csr(m, ni, tcols)
        seen = _seen(tcols, ni, 9)
        whole = _want(seen, test, U, V, S=S)
        assert _eq(_host(seen, test, U, V), whole)
        cuts = [0, 1, B - 2, B + 7, B + 7, 2 * B, m]                # pieces, one of them empty
        parts = [_host(seen, test, U, V, rows=(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
        assert _eq(tuple(np.concatenate([p[x] for p in parts]) for x in range(2)), whole)
        for kw in (dict(), dict(pad=3), dict(shift=1), dict(pad=1, shift=1), dict(pad=4), dict(stream=True), dict(repeat=2),
                   dict(pad=2, shift=3, stream=True)):
            assert _eq(_device(seen, test, U, V, **kw), whole), (gen.__name__, k, kw)
        got = _device(seen, test, U, V, scores=False)              # scores may be NULL
        assert np.array_equal(got[0], whole[0])
        a, b = int(test.rowptrs[B - 1]), int(test.rowptrs[B + 9])
        assert _eq(_device(seen, test, U, V, rows=(B - 1, B + 9), shift=1), (whole[0][a:b], whole[1][a:b]))
        # the other entries of test decide nothing: one entry per row alone gets what it got among the others
        one = _csr(m, ni, [c[:1] for c in tcols])
        first = np.array([int(test.rowptrs[r]) for r in range(m) if len(tcols[r])])
        assert _eq(_host(seen, one, U, V), (whole[0][first], whole[1][first]))


# ---- 8. refusals -------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing_and_limits_hold(lim):
    import torch
    from csr_amd._lib import lib, ERR_INVALID, ERR_UNSUPPORTED, VAL_F64
    from csr_amd.kernels import hip as K
    m, ni, k = 5, 9, 3
    rng = np.random.default_rng(65)
    U, V = _grid((m, k), rng), _grid((ni, k), rng)
    tU, tV = torch.from_numpy(U).cuda(), torch.from_numpy(V).cuda()
    test = _csr(m, ni, [np.array([3, 1], np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.array([8, 8, 0], np.int32),
                        np.array([2], np.int32)])
    good = _csr(m, ni, [np.array([1, 4], np.int32)] * m)
    bad = _csr(m, ni, [np.array([1, 4], np.int32), np.array([2, 7], np.int32), np.array([4, 4], np.int32), np.array([5, 2], np.int32),
                       np.zeros(0, np.int32)])
    wider, taller = _csr(m, ni + 1, [np.zeros(0, np.int32)] * m), _csr(m + 1, ni, [np.zeros(0, np.int32)] * (m + 1))
    empty = _csr(m, ni, [np.zeros(0, np.int32)] * m)
    ht, hg, hb, hw, hl, he = (K.to_handle(x) for x in (test, good, bad, wider, taller, empty))
    ne = test.nnz
    try:
        for form in ('host', 'device'):
            if form == 'host':
                ranks, scores = np.full(ne, 7, np.int32), np.full(ne, 7.0)
                p = dict(u=U.ctypes.data, v=V.ctypes.data, rk=ranks.ctypes.data, sc=scores.ctypes.data)
            else:
                ranks = torch.full((ne,), 7, dtype=torch.int32, device='cuda')
                scores = torch.full((ne,), 7.0, dtype=torch.float64, device='cuda')
                p = dict(u=tU.data_ptr(), v=tV.data_ptr(), rk=ranks.data_ptr(), sc=scores.data_ptr())

            def call(**ch):
                a = dict(dict(s=hg.H, t=ht.H, rb=0, re=m, ldu=k, ldv=k, k=k, pt=VAL_F64, **p), **ch)
                args = (a['s'], a['t'], a['rb'], a['re'], a['u'], a['ldu'], a['v'], a['ldv'], a['k'], a['pt'], a['rk'], a['sc'])
                return lib.csrk_rank_entries(*args) if form == 'host' else lib.csrk_rank_entries_device(*args, None)
            invalid = {'k < 1': dict(k=0), 'ldu < k': dict(ldu=k - 1), 'ldv < k': dict(ldv=k - 1), 'panel type': dict(pt=9),
                       'row_begin < 0': dict(rb=-1), 'row_begin > row_end': dict(rb=3, re=2), 'row_end > nrows': dict(re=m + 1),
                       'seen wider': dict(s=hw.H), 'seen taller': dict(s=hl.H), 'not canonical': dict(s=hb.H),
                       'seen not a handle': dict(s=12345), 'test not a handle': dict(t=12345), 'test 0': dict(t=0),
                       'NULL ranks': dict(rk=None), 'NULL U': dict(u=None), 'NULL V': dict(v=None),
                       'misaligned U': dict(u=p['u'] + 4), 'misaligned ranks': dict(rk=p['rk'] + 2)}
            for name, ch in invalid.items():
                assert call(**ch) == ERR_INVALID, (form, name)
                if name == 'not canonical':
                    assert b'row 2' in lib.csrk_last_error()          # the first bad row, as csrk_topk_scores names it
            assert call(k=lim[0] + 1, ldu=lim[0] + 1, ldv=lim[0] + 1) == ERR_UNSUPPORTED
            assert call(rb=2, re=2, u=None, v=None, rk=None, sc=None) == 0          # no rows: nothing launched
            assert call(t=he.H, u=None, v=None, rk=None, sc=None) == 0              # a test without entries: nothing launched
            if form == 'host':
                assert call(rb=1, re=3, u=None, v=None, rk=None, sc=None) == 0      # a range without test entries
            else:
                assert call(rb=1, re=3) == 0                                        # (the device form launches; nothing is written)
                torch.cuda.synchronize()
                ranks, scores = ranks.cpu().numpy(), scores.cpu().numpy()
            assert np.all(ranks == 7) and np.all(scores == 7.0), form
            assert K.is_canonical(hg) == (True, None) and K.is_canonical(hb) == (False, 2)
        # the seen that was refused is fine as test: rows out of order and a repeat are just entries
        with pytest.raises(Exception):
            K.rank_entries(hb, ht, U, V)
        assert _eq(K.rank_entries(hg, hb, U, V), _want(good, bad, U, V))
        assert _eq(K.rank_entries(hg, ht, U, V), _want(good, test, U, V))
    finally:
        for h in (ht, hg, hb, hw, hl, he):
            K.release_handle(h)
    # success at the largest k
    Uk, Vk = _grid((2, lim[0]), rng), _grid((5, lim[0]), rng)
    assert _eq(_host(None, _full(2, 5), Uk, Vk), _want(None, _full(2, 5), Uk, Vk))
