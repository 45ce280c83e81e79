"""
knn_scores(route='reach') on the card (csrc/knn_scores.hip: mark, enumerate, walk) against the plain-Python restatement of the
contract (tests/knn_scores_ref.py) AND against route='walk'.  Every comparison is bit for bit -- row pointers, columns and
values (a NaN stands for any NaN) -- and every call is held to its census (knn_scores_last_stats): the reach route ran, with
ceil(n_targets / R) ranges per listed row, counting from the marks exactly when min_nbrs == 1.  The limits are read from
knn_scores_reach_limits(); the models of the range cases are almost entirely empty rows, so the restatement stays fast.
"""
import ctypes

import numpy as np
import pytest

from knn_scores_ref import knn_scores_ref, same, first_difference

pytestmark = pytest.mark.gpu

i4 = np.int32
INF, NAN = float('inf'), float('nan')
AGG = ('weighted-average', 'sum')


def _K():
    from csr_amd.kernels import hip as K
    return K


def _lim():
    return _K().knn_scores_reach_limits()


def _csr(t, ncols, ptr=np.int32):
    from csr_amd import CSR
    rp, ci, vs = t
    return CSR(len(rp) - 1, ncols, int(rp[-1]), np.ascontiguousarray(rp, dtype=ptr), np.ascontiguousarray(ci, dtype=np.int32),
               None if vs is None else np.ascontiguousarray(vs), _cast=False)


def _tup(m):
    return m.rowptrs, m.colinds, m.values


def _rows(cols, vals=None):
    "a list of column arrays (and of value arrays) -> (rowptrs, colinds, values)"
    rp = np.concatenate(([0], np.cumsum([len(c) for c in cols]))).astype(np.int64)
    ci = np.concatenate([np.zeros(0, np.int64)] + [np.asarray(c, np.int64) for c in cols]).astype(i4)
    vs = None if vals is None else np.concatenate([np.zeros(0)] + [np.asarray(v, np.float64) for v in vals])
    return rp, ci, vs


def _sparse_model(n_targets, rows, seed=0):
    "a model of n_targets rows, all empty but rows = {target: columns}; similarities descending inside a row"
    rng = np.random.default_rng(seed)
    cols = [rows.get(i, ()) for i in range(n_targets)]
    return _rows(cols, [np.sort(rng.uniform(0.05, 1.0, len(c)))[::-1] for c in cols])


def _census(st, M, R, users, got, kw):
    K = _K()
    n_targets, n_rows = len(M[0]) - 1, len(users)
    if n_rows == 0 or n_targets == 0 or M[0][-1] == 0 or R[0][-1] == 0:
        assert st == (0,) * len(K.KNN_STATS), st                  # an empty result: nothing ran
        return
    ranges = -(-n_targets // _lim()[0])
    assert st[0] == 1 and st[1] == ranges and st[2] == n_rows * ranges, st
    assert st[3] == (1 if kw.get('min_nbrs', 1) == 1 else 0), st
    assert st[5] == len(got[1]), st


def _check(M, R, n_items, users, what='', mcsr=None, rcsr=None, exp=None, **kw):
    "route='reach' against the restatement and against route='walk', and its census; the operands' CSR objects may be reused"
    K = _K()
    mcsr = _csr(M, n_items) if mcsr is None else mcsr
    rcsr = _csr(R, n_items) if rcsr is None else rcsr
    got = _tup(rcsr.knn_scores(mcsr, users, route='reach', **kw))
    st = K.knn_scores_last_stats()
    walk = _tup(rcsr.knn_scores(mcsr, users, route='walk', **kw))
    assert K.knn_scores_last_stats() == (0,) * len(K.KNN_STATS)   # the walk-all entry reports nothing
    exp = knn_scores_ref(M, R, users, **kw) if exp is None else exp
    assert same(got, exp), (what, kw, first_difference(got, exp))
    assert same(got, walk), (what, kw, first_difference(got, walk))
    _census(st, M, R, users, got, kw)
    return got


def _descending_model(rng, lengths, n_items):
    "rows of the given lengths: distinct columns in random (not ascending) order, similarities descending"
    cols = [rng.permutation(n_items)[:n] for n in lengths]
    vals = [np.sort(rng.uniform(0.05, 1.0, n))[::-1] for n in lengths]
    return _rows(cols, vals)


# ---- ranges of targets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['one', 'below', 'exact', 'above', 'three ranges'])
def test_ranges(which):
    """
    Model rows only at targets 0, R - 1, R, R + 1, 2 R - 1, 2 R and the last.  Item 0 is stored by all of them: its reach row
    spans every range (the lower bound and the stop).  Item 1 is stored only by the middle range's rows, item 2 only by the
    first and the last range's: a user of item 1 reaches the middle range alone, a user of item 2 leaves it empty (PLACE skips
    it), and with min_nbrs = 2 a user of items 0 and 1 reaches every range but stores in the middle one only.
    """
    R_ = _lim()[0]
    n_targets = {'one': 1, 'below': R_ - 1, 'exact': R_, 'above': R_ + 1, 'three ranges': 2 * R_ + 1}[which]
    n_items = 12
    rows = {}
    for k, i in enumerate(sorted({0, R_ - 1, R_, R_ + 1, 2 * R_ - 1, 2 * R_, n_targets - 1})):
        if i < n_targets:
            middle = R_ <= i < 2 * R_
            rows[i] = [3 + k, 1 if middle else 2, 0, 11]           # (unsorted columns)
    M = _sparse_model(n_targets, rows)
    R = _rows([[0], [1], [2], [0, 1, 2, 5], [], [0, 1], [4, 5]], [[4.0], [3.0], [2.0], [1.0, 2.0, 3.0, 4.0], [], [5.0, 1.0], [2.0, 2.0]])
    mc, rc = _csr(M, n_items), _csr(R, n_items)
    users = [3, 0, 1, 2, 4, 5, 6, 1]
    got = _check(M, R, n_items, users, which, mc, rc)
    if which == 'three ranges':
        # user 1 (item 1): the middle range only; user 2 (item 2): the first and the last
        assert list(got[1][got[0][2]:got[0][3]]) == [R_, R_ + 1, 2 * R_ - 1]
        assert list(got[1][got[0][3]:got[0][4]]) == [0, R_ - 1, 2 * R_]
        assert list(got[1][got[0][1]:got[0][2]]) == [0, R_ - 1, R_, R_ + 1, 2 * R_ - 1, 2 * R_]
    got = _check(M, R, n_items, users, which, mc, rc, min_nbrs=2, aggregate='sum')
    if which == 'three ranges':
        assert list(got[1][got[0][5]:got[0][6]]) == [R_, R_ + 1, 2 * R_ - 1]      # items 0 and 1: reached everywhere, stored in the middle
        assert got[0][2] == got[0][4]                                             # one hit each: reached, none stored
    _check(M, R, n_items, users, which, mc, rc, min_nbrs=2, max_nbrs=2, offsets=np.arange(8.0))


# ---- the bitmap -------------------------------------------------------------------------------------------------------------------
def test_bitmap_words_repeats_and_several_items():
    n_items, n_targets = 10, 100
    rows = {0: [4], 31: [4, 7], 32: [7], 63: [4], 64: [7, 4],
            70: [5, 4, 7, 6],              # reached from several rated items
            71: [4, 9, 4],                 # repeats a column: the index holds target 71 twice; stored once, column 4 counted twice
            72: [9, 9],                    # repeats an unrated column
            99: [8]}
    M = _sparse_model(n_targets, rows, 3)
    R = _rows([[4, 5, 6, 7], [7], [9], [4]], [[1.0, 2.0, 3.0, 4.0], [5.0], [2.5], [3.5]])
    mc, rc = _csr(M, n_items), _csr(R, n_items)
    for agg in AGG:
        got = _check(M, R, n_items, [0, 1, 2, 3], 'bitmap', mc, rc, aggregate=agg)
        assert list(got[1][:got[0][1]]) == [0, 31, 32, 63, 64, 70, 71]
        assert list(got[1][got[0][3]:]) == [0, 31, 63, 64, 70, 71]
        for mn in (2, 3):
            _check(M, R, n_items, [0, 1, 2, 3], 'bitmap', mc, rc, aggregate=agg, min_nbrs=mn)
        _check(M, R, n_items, [0, 1, 2, 3], 'bitmap', mc, rc, aggregate=agg, max_nbrs=1)
    got = _check(M, R, n_items, [3], 'repeat', mc, rc, aggregate='sum', min_nbrs=2)
    assert list(got[1]) == [71]                                    # two hits, both on column 4
    # the index: one entry per stored occurrence
    K = _K()
    from csr_amd.kernels import releasing
    with releasing(K.to_handle(mc), K) as mh:
        assert K.knn_reach_index(mh)[0] == M[0][-1]


# ---- rounds of candidates ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('extra', [-1, 0, 1])
@pytest.mark.parametrize('rounds', [1, 2])
def test_candidates_around_a_round(rounds, extra):
    per_round, chunk, R_ = _lim()[4], _lim()[5], _lim()[0]
    assert chunk == R_                                              # a range is enumerated in one piece: no chunk edge to test
    n_cand = rounds * per_round + extra
    n_items, n_targets = 8, 3 * n_cand + 7
    rng = np.random.default_rng(n_cand)
    at = np.sort(rng.choice(n_targets, n_cand, replace=False))
    # every candidate stores item 0; every other one stores item 1 too (min_nbrs = 2 keeps those)
    rows = {int(i): ([1, 5, 0] if k % 2 else [5, 0, 3]) for k, i in enumerate(at)}
    M = _sparse_model(n_targets, rows, 1)
    R = _rows([[0, 1], [0]], [[2.0, 4.0], [3.0]])
    mc, rc = _csr(M, n_items), _csr(R, n_items)
    got = _check(M, R, n_items, [0, 1], n_cand, mc, rc)
    assert list(got[1][:got[0][1]]) == list(at) and got[0][2] == 2 * n_cand
    got = _check(M, R, n_items, [0, 1], n_cand, mc, rc, min_nbrs=2)
    assert list(got[1]) == list(at[1::2])
    _check(M, R, n_items, [0, 1], n_cand, mc, rc, min_nbrs=2, aggregate='sum', max_nbrs=2)


# ---- reach-row classes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('extra', [-1, 0, 1])
def test_reach_rows_around_the_wavefront_threshold(extra):
    "a reach row of T - 1, T and T + 1 entries (T = the most a group of lanes marks), beside a short one, in one range"
    lim = _lim()
    assert len(lim) > 6
    T = lim[6]
    n = T + extra
    n_items, n_targets = 6, n + 40
    rng = np.random.default_rng(n)
    at = np.sort(rng.choice(n_targets, n, replace=False))
    rows = {int(i): [0, 2] for i in at}
    for i in range(0, n_targets, 9):
        rows[i] = rows.get(i, []) + [1]
    M = _sparse_model(n_targets, rows, 2)
    R = _rows([[0], [0, 1], [1]], [[2.0], [4.0, 1.0], [3.0]])
    mc, rc = _csr(M, n_items), _csr(R, n_items)
    got = _check(M, R, n_items, [0, 1, 2], n, mc, rc)
    assert list(got[1][:got[0][1]]) == list(at)
    _check(M, R, n_items, [0, 1, 2], n, mc, rc, min_nbrs=2, aggregate='sum')


def test_long_reach_row_across_a_range_edge():
    "a popular item whose reach row begins in one range and ends in the next: long on both sides of the edge, stopped at the first"
    lim = _lim()
    R_, T = lim[0], lim[6]
    n_items, n_targets = 6, R_ + 2 * T
    rows = {i: [0] for i in range(R_ - T - 3, R_ + T + 5)}
    rows[5] = [1, 0]
    rows[R_ + 2 * T - 1] = [0, 1]
    M = _sparse_model(n_targets, rows, 4)
    R = _rows([[0], [1]], [[2.0], [3.0]])
    mc, rc = _csr(M, n_items), _csr(R, n_items)
    got = _check(M, R, n_items, [0, 1, 0], 'edge', mc, rc)
    assert list(got[1][:got[0][1]]) == sorted(rows)
    _check(M, R, n_items, [0, 1, 0], 'edge', mc, rc, min_nbrs=2)


# ---- no candidates ----------------------------------------------------------------------------------------------------------------
def test_users_without_candidates():
    n_items, n_targets = 9, 70
    M = _sparse_model(n_targets, {3: [1, 2], 40: [2], 69: [1]}, 5)
    R = _rows([[], [0, 5, 8], [1], [4]], [[], [1.0, 2.0, 3.0], [4.0], [5.0]])      # user 0: no rating; users 1, 3: nothing stores their items
    mc, rc = _csr(M, n_items), _csr(R, n_items)
    for mn in (1, 2):
        got = _check(M, R, n_items, [0, 1, 3, 1, 0], 'none', mc, rc, min_nbrs=mn)
        assert list(got[0]) == [0] * 6 and got[0].dtype == np.int32                 # total 0, row pointers complete
        got = _check(M, R, n_items, [0, 2, 1, 3], 'one', mc, rc, min_nbrs=mn)
        assert list(got[0]) == ([0, 0, 2, 2, 2] if mn == 1 else [0] * 5)


# ---- the walk on this route -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def walk_case():
    L = _lim()[1]
    rng = np.random.default_rng(5)
    n_items = 3 * L
    lengths = [0, 1, L - 1, L, L + 1, 2 * L + 1] * 2
    M = _descending_model(rng, lengths, n_items)
    # user 0 rated everything (hits = the row's length: the cut at every place of a step), user 1 nothing, user 2 about half
    half = np.sort(rng.choice(n_items, n_items // 2, replace=False))
    R = _rows([np.arange(n_items), [], half], [rng.integers(1, 6, n_items), [], rng.integers(1, 6, len(half))])
    return L, n_items, M, R, _csr(M, n_items), _csr(R, n_items)


@pytest.mark.parametrize('aggregate', AGG)
def test_model_row_lengths_and_the_cut(walk_case, aggregate):
    L, n_items, M, R, mc, rc = walk_case
    users = [0, 1, 2]
    off = np.array([0.5, -1.25, 3.0])
    for mx in (0, 1, L // 2, L - 2, L - 1, L, L + 1, L + 2, 2 * L, 2 * L + 1, 2 * L + 2):
        _check(M, R, n_items, users, 'cut', mc, rc, max_nbrs=mx, aggregate=aggregate)
    _check(M, R, n_items, users, 'offsets', mc, rc, max_nbrs=L, aggregate=aggregate, offsets=off)
    _check(M, R, n_items, users, 'offsets', mc, rc, aggregate=aggregate, offsets=off)


@pytest.mark.parametrize('aggregate', AGG)
def test_min_nbrs(walk_case, aggregate):
    L, n_items, M, R, mc, rc = walk_case
    for mn in (1, 2, L - 1, L, L + 1, L + 2, 2 * L + 1, 2 * L + 2):       # hits, hits + 1 of every row length: present, absent
        got = _check(M, R, n_items, [0, 1, 2], 'min', mc, rc, min_nbrs=mn, aggregate=aggregate)
    assert got[0][-1] == 0 and len(got[0]) == 4                            # reached, none stored: the pointers are complete
    got = _check(M, R, n_items, [0, 2], 'min above max', mc, rc, max_nbrs=2, min_nbrs=3, aggregate=aggregate)
    assert list(got[0]) == [0, 0, 0]
    _check(M, R, n_items, [0, 2], 'min = max', mc, rc, max_nbrs=3, min_nbrs=3, aggregate=aggregate, offsets=np.array([1.5, -2.0]))


# ---- rating rows ------------------------------------------------------------------------------------------------------------------
def test_rating_row_lengths():
    "rows staged in LDS and rows searched in device memory: the same bits, and the marks come from either"
    D = _lim()[2]
    rng = np.random.default_rng(7)
    n_items = D + 9
    lens = [0, 1, D - 1, D, D + 1]
    R = _rows([np.sort(rng.choice(n_items, n, replace=False)) for n in lens], [rng.integers(1, 6, n) for n in lens])
    cols = [np.concatenate(([0, n_items - 1], rng.permutation(np.arange(1, n_items - 1))[:18])) for _ in range(24)]
    cols = [rng.permutation(c) for c in cols]
    M = _rows(cols, [np.sort(rng.uniform(0.05, 1.0, 20))[::-1] for _ in cols])
    mc, rc = _csr(M, n_items), _csr(R, n_items)
    for agg in AGG:
        _check(M, R, n_items, [4, 0, 3, 1, 2], 'ratings', mc, rc, aggregate=agg)
        _check(M, R, n_items, [4, 0, 3, 1, 2], 'ratings', mc, rc, aggregate=agg, max_nbrs=5, min_nbrs=2, offsets=np.arange(5.0))


def test_columns_that_share_a_filter_bit():
    "unrated neighbours whose column equals a rated column modulo the filter's size are searched for and not found"
    L, B = _lim()[1], _lim()[3]
    n_items = 2 * B + 9
    rated = [3, 40, B + 7, 2 * B + 1]
    R = _rows([rated, []], [[4.0, 2.0, 5.0, 3.0], []])
    alias = [B + 3, 2 * B + 3, 7, 2 * B + 7, 1, B + 1, B + 40]           # none is rated, every one shares a rated column's bit
    cols = [alias,                                                        # only aliases: not even a candidate
            [B + 3, 3, 7, B + 7, 1, 2 * B + 1],                           # an alias in front of every hit
            alias + rated,
            (alias * 3)[:L - 1] + [40] + alias[:2] + [3],                 # hits on both sides of a step boundary
            rated[::-1]]
    M = _rows(cols, [np.linspace(1.0, 0.1, len(c)) for c in cols])
    mc, rc = _csr(M, n_items), _csr(R, n_items)
    for agg in AGG:
        for mx in (0, 1, 2):
            got = _check(M, R, n_items, [0, 1, 0], 'aliases', mc, rc, max_nbrs=mx, aggregate=agg)
        assert list(got[1][:got[0][1]]) == [1, 2, 3, 4] and got[0][2] == got[0][1]
        _check(M, R, n_items, [0, 1, 0], 'aliases', mc, rc, min_nbrs=3, aggregate=agg)


# ---- value types, pointer widths --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small_case():
    rng = np.random.default_rng(21)
    n_items, n_targets, n_users = 50, 37, 9
    M = _descending_model(rng, rng.integers(0, 25, n_targets), n_items)
    lens = rng.integers(0, 30, n_users)
    R = _rows([np.sort(rng.choice(n_items, n, replace=False)) for n in lens], [rng.integers(1, 11, n) / 2 for n in lens])
    return n_items, M, R


@pytest.mark.parametrize('rtype', ['f8', 'f4', None])
@pytest.mark.parametrize('mtype', ['f8', 'f4', None])
def test_value_types_and_pointer_widths(small_case, mtype, rtype):
    n_items, M, R = small_case
    cast = lambda t, d: (t[0], t[1], None if d is None else t[2].astype(d))      # noqa: E731
    M, R = cast(M, mtype), cast(R, rtype)
    users = np.arange(len(R[0]) - 1)
    exp = {(agg, mn): knn_scores_ref(M, R, users, aggregate=agg, max_nbrs=4, min_nbrs=mn) for agg in AGG for mn in (1, 2)}
    for pm in (np.int32, np.int64):
        for pr in (np.int32, np.int64):
            mc, rc = _csr(M, n_items, pm), _csr(R, n_items, pr)
            for agg in AGG:
                for mn in (1, 2):
                    _check(M, R, n_items, users, (pm, pr), mc, rc, exp=exp[agg, mn], aggregate=agg, max_nbrs=4, min_nbrs=mn)


# ---- the list of rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mn', [1, 2])
def test_the_list_of_rows(small_case, mn):
    n_items, M, R = small_case
    mc, rc = _csr(M, n_items), _csr(R, n_items)
    n_users = len(R[0]) - 1
    rng = np.random.default_rng(3)
    kw = dict(max_nbrs=5, min_nbrs=mn)
    full = _check(M, R, n_items, np.arange(n_users), 'all', mc, rc, **kw)
    none = _tup(rc.knn_scores(mc, route='reach', **kw))                       # users=None: all rows
    assert same(none, full)
    again = _tup(rc.knn_scores(mc, np.arange(n_users), route='reach', **kw))  # a second call: the same bits
    assert same(again, full) and again[2].tobytes() == full[2].tobytes()
    _check(M, R, n_items, rng.permutation(n_users), 'shuffled', mc, rc, **kw)
    rep = np.array([4, 4, 1, 4, 8, 1])
    got = _check(M, R, n_items, rep, 'repeated', mc, rc, **kw)
    for r, u in enumerate(rep):                                               # a row alone equals the same row inside a batch
        alone = _tup(rc.knn_scores(mc, [u], route='reach', **kw))
        b, e = got[0][r], got[0][r + 1]
        assert np.array_equal(alone[1], got[1][b:e]) and alone[2].tobytes() == got[2][b:e].tobytes(), (r, u)
        fb, fe = full[0][u], full[0][u + 1]
        assert np.array_equal(alone[1], full[1][fb:fe]) and alone[2].tobytes() == full[2][fb:fe].tobytes(), (r, u)
    empty = _check(M, R, n_items, np.zeros(0, np.int64), 'empty', mc, rc, **kw)
    assert list(empty[0]) == [0]


def test_empty_operands():
    n_items = 6
    M = _rows([[1, 2], [0]], [[0.5, 0.25], [1.0]])
    R = _rows([[0, 2], [1]], [[3.0, 4.0], [5.0]])
    E_m, E_r, no_targets = _rows([[], []], [[], []]), _rows([[], []], [[], []]), _rows([], [])
    K = _K()
    from csr_amd.kernels import releasing
    for m, r, what in ((E_m, R, 'model.nnz = 0'), (M, E_r, 'ratings.nnz = 0'), (no_targets, R, 'n_targets = 0')):
        got = _check(m, r, n_items, [1, 0, 1], what)
        assert got[0].dtype == np.int32 and list(got[0]) == [0, 0, 0, 0] and got[2].dtype == np.float64
    # nothing is built for an empty result
    with releasing(K.to_handle(_csr(M, n_items)), K) as mh, releasing(K.to_handle(_csr(E_r, n_items)), K) as rh:
        K.release_handle(K.knn_scores(mh, rh, [0], route='reach'))
        K.release_handle(K.knn_scores(mh, rh, [], route='reach'))
        assert K.knn_reach_index(mh, build=False) == (0, 0)


# ---- special values ---------------------------------------------------------------------------------------------------------------
def test_zero_similarities_are_hits():
    n_items = 8
    R = _rows([[0, 1, 2, 3, 4]], [[1.0, 2.0, 3.0, 4.0, 5.0]])
    M = _rows([[0, 1, 2], [3, 2, 1], [5, 0, 1], [0, 1], [5, 3]], [[0.0, -0.0, 1.0], [-0.0, 0.0, 0.5], [9.0, 0.0, 0.0], [0.0, 0.0], [1.0, 0.0]])
    for agg in AGG:
        for mx in (0, 1, 2, 3):
            _check(M, R, n_items, [0], 'zeros', max_nbrs=mx, aggregate=agg)
        _check(M, R, n_items, [0], 'zeros', min_nbrs=3, aggregate=agg)
    got = _check(M, R, n_items, [0], 'zeros', max_nbrs=2)
    assert list(got[1]) == [0, 1, 2, 3, 4] and np.isnan(got[2]).all()          # den = 0 stores NaN
    got = _check(M, R, n_items, [0], 'zeros')
    assert list(got[2][:2]) == [3.0, 2.0] and np.isnan(got[2][2:]).all()
    assert got[1][-1] == 4                                                      # its only hit has s = 0.0: a candidate, and stored
    Rz = _rows([[0, 1, 2]], [[0.0, -0.0, 0.0]])                                 # explicit zero ratings are hits too
    got = _check(M, Rz, n_items, [0], 'zero ratings', min_nbrs=2)
    assert list(got[1]) == [0, 1, 2, 3]


@pytest.mark.parametrize('bad', [NAN, INF, -INF])
def test_nan_and_inf_reach_only_the_walks_that_use_them(bad):
    L = _lim()[1]
    n_items = 2 * L + 4
    rng = np.random.default_rng(9)
    n = 2 * L + 1
    cols = [rng.permutation(n_items)[:n] for _ in range(4)]
    vals = [np.sort(rng.uniform(0.05, 1.0, n))[::-1] for _ in range(4)]
    vals[1][L + 2] = bad                                 # a similarity in the second step of target 1
    vals[3][0] = bad
    R = _rows([np.arange(n_items), np.arange(n_items)], [rng.integers(1, 6, n_items).astype(float), rng.integers(1, 6, n_items).astype(float)])
    R[2][cols[2][1]] = bad                               # user 0's rating of target 2's second neighbour (and of others' too)
    M = _rows(cols, vals)
    mc, rc = _csr(M, n_items), _csr(R, n_items)
    for agg in AGG:
        full = _check(M, R, n_items, [0, 1], bad, mc, rc, aggregate=agg)
        assert np.isfinite(full[2][full[0][1]:][[0, 2]]).all()          # user 1, targets 0 and 2: untouched
        assert not np.isfinite(full[2][full[0][1]:][[1, 3]]).any()
        clean = (M[0], M[1], np.where(np.isfinite(M[2]), M[2], 0.25))
        for mx in (L + 2, L + 3):                                        # the cut before the bad similarity
            got = _check(M, R, n_items, [1], bad, mc, rc, aggregate=agg, max_nbrs=mx, min_nbrs=2)
            ref = knn_scores_ref(clean, R, [1], max_nbrs=mx, aggregate=agg)
            assert (got[2][1].tobytes() == ref[2][1].tobytes()) == (mx == L + 2)


# ---- the index and its lifetime ---------------------------------------------------------------------------------------------------
def _device_bytes(h):
    from csr_amd import _lib
    nb = ctypes.c_int64(0)
    _lib.check(_lib.lib.csrk_device_bytes(h.H, ctypes.byref(nb)))
    return nb.value


def _score(K, mh, rh, users, **kw):
    from csr_amd.kernels import releasing
    with releasing(K.knn_scores(mh, rh, users, route='reach', **kw), K) as sh:
        st = K.knn_scores_last_stats()
        return _tup(K.from_handle(sh)), st


def test_index_lifetime(small_case):
    K = _K()
    from csr_amd.kernels import releasing
    n_items, M, R = small_case
    users = np.arange(len(R[0]) - 1)
    exp = knn_scores_ref(M, R, users, max_nbrs=4)
    nnz = int(M[0][-1])
    with releasing(K.to_handle(_csr(M, n_items)), K) as mh, releasing(K.to_handle(_csr(R, n_items)), K) as rh:
        assert K.knn_reach_index(mh, build=False) == (0, 0)                     # a fresh handle holds none
        before = _device_bytes(mh)
        got, st = _score(K, mh, rh, users, max_nbrs=4)
        assert same(got, exp) and st[0] == 1 and st[4] == 1                     # the first call built it
        entries, nbytes = K.knn_reach_index(mh, build=False)
        assert entries == nnz and nbytes == (n_items + 1) * 4 + nnz * 4
        assert _device_bytes(mh) == before + nbytes
        assert _device_bytes(rh) == _device_bytes(rh) and K.knn_reach_index(rh, build=False) == (0, 0)      # the model's, not the ratings'
        got, st = _score(K, mh, rh, users, max_nbrs=4)
        assert same(got, exp) and st[4] == 0                                    # a second call finds it
        # order_columns rewrites the columns: the index goes, the next call builds it again and equals the restatement of
        # the model as it now lies
        K.order_columns(mh)
        assert K.knn_reach_index(mh, build=False) == (0, 0) and _device_bytes(mh) == before
        sorted_model = _tup(K.from_handle(mh))
        got, st = _score(K, mh, rh, users, max_nbrs=4)
        assert st[4] == 1 and same(got, knn_scores_ref(sorted_model, R, users, max_nbrs=4))
        assert K.knn_reach_index(mh, build=False) == (nnz, nbytes)
    with releasing(K.to_handle(_csr(M, n_items)), K) as mh, releasing(K.to_handle(_csr(R, n_items)), K) as rh:
        assert K.knn_reach_index(mh) == (nnz, (n_items + 1) * 4 + nnz * 4)      # built beforehand ...
        got, st = _score(K, mh, rh, users, max_nbrs=4, min_nbrs=2)
        assert st[4] == 0 and st[3] == 0                                        # ... the first call does not build
        assert same(got, knn_scores_ref(M, R, users, max_nbrs=4, min_nbrs=2))


def test_model_may_be_the_ratings():
    "one handle as both operands: allowed, locked once, and it keeps the index"
    K = _K()
    from csr_amd.kernels import releasing
    S = _rows([[0, 2], [1], [0, 1, 2]], [[1.0, 2.0], [3.0], [0.5, 0.25, 4.0]])
    with releasing(K.to_handle(_csr(S, 3)), K) as h:
        for mn in (1, 2):
            got, st = _score(K, h, h, [2, 0], min_nbrs=mn)
            assert same(got, knn_scores_ref(S, S, [2, 0], min_nbrs=mn)) and st[0] == 1 and st[4] == (mn == 1)
        assert K.knn_reach_index(h, build=False)[0] == 6


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(small_case):
    "every CSRK_ERR_INVALID of csrk_knn_scores' rule 7 that one card can show, under the new entry's name"
    K = _K()
    from csr_amd import _lib
    from csr_amd.kernels import releasing
    lib = _lib.lib
    n_items, M, R = small_case
    n_users = len(R[0]) - 1
    unsorted = _rows([[1, 3], [2, 2]], [[1.0, 2.0], [3.0, 4.0]])             # row 1 repeats a column
    rows = np.array([0, 1, n_users, -1], i4)
    one = np.array([0], i4)

    def call(mh, rh, rows, n, mx=0, mn=1, agg=0, out=True):
        o = _lib.handle_t(77)
        rc = lib.csrk_knn_scores_reach(mh, rh, None if rows is None else rows.ctypes.data, n, mx, mn, agg, None,
                                       ctypes.byref(o) if out else None)
        msg = _lib.last_error()
        if out:
            assert (o.value == 0) == (rc != _lib.OK), (rc, msg)
            if rc == _lib.OK:
                lib.csrk_free(o.value)
        if rc != _lib.OK:
            assert K.knn_scores_last_stats() == (0,) * len(K.KNN_STATS)
        return rc, msg

    with releasing(K.to_handle(_csr(M, n_items)), K) as mh, releasing(K.to_handle(_csr(R, n_items)), K) as rh, \
            releasing(K.to_handle(_csr(M, n_items + 1)), K) as wide, releasing(K.to_handle(_csr(unsorted, n_items)), K) as bad:
        INV = _lib.ERR_INVALID
        P = 'knn_scores_reach: '
        for args, words in (((mh.H, rh.H, one, 1, 0, 1, 0, False), (P, 'out', 'NULL')),
                            ((0, rh.H, one, 1), ('invalid csrk handle',)),
                            ((mh.H, 12345, one, 1), ('invalid csrk handle',)),
                            ((wide.H, rh.H, one, 1), (P, 'columns', str(n_items + 1))),
                            ((mh.H, rh.H, one, -1), (P, 'n_rows',)),
                            ((mh.H, rh.H, None, 1), (P, 'rows is NULL',)),
                            ((mh.H, rh.H, one, 1, -1), (P, 'max_nbrs',)),
                            ((mh.H, rh.H, one, 1, 0, 0), (P, 'min_nbrs',)),
                            ((mh.H, rh.H, one, 1, 0, 1, 2), (P, 'aggregate',)),
                            ((mh.H, rh.H, one, 1, 0, 1, -1), (P, 'aggregate',)),
                            ((mh.H, bad.H, one, 1), ('ratings', 'not canonical', 'row 1')),
                            ((mh.H, rh.H, rows, 3), (P, 'rows[2]', str(n_users))),
                            ((mh.H, rh.H, rows[3:], 1), (P, 'rows[0]', '-1'))):
            rc, msg = call(*args)
            assert rc == INV and all(w in msg for w in words), (args[2:], rc, msg)
            if P in words:
                assert msg.startswith(P), msg
        assert K.knn_reach_index(mh, build=False) == (0, 0)                  # a refused call builds nothing
        assert call(mh.H, rh.H, rows, 2)[0] == _lib.OK                       # the good part of the same list
        assert call(bad.H, rh.H, one, 1)[0] == _lib.OK                       # a non-canonical MODEL is taken
        assert call(mh.H, rh.H, None, 0)[0] == _lib.OK                       # NULL rows with n_rows = 0
        assert call(mh.H, bad.H, None, 0)[0] == _lib.OK                      # an empty list: nothing launched, not even the look at ratings
        assert call(mh.H, bad.H, one, 1, -1)[0] == INV                       # ... but the scalar arguments are still checked
        assert call(rh.H, rh.H, one, 1)[0] == _lib.OK                        # model == ratings is allowed ...
        rc, msg = call(bad.H, bad.H, one, 1)                                 # ... and checked as ratings: this one is unsorted
        assert rc == INV and 'not canonical' in msg
    with pytest.raises(ValueError) as ei:                                    # the Python layer: ValueError
        _csr(unsorted, n_items).knn_scores(_csr(M, n_items), route='reach')
    assert 'not canonical' in str(ei.value)


# ---- knn_topk ---------------------------------------------------------------------------------------------------------------------
def test_knn_topk_by_either_route(small_case):
    n_items, M, R = small_case
    rng = np.random.default_rng(12)
    Msq = _descending_model(rng, rng.integers(0, 25, n_items), n_items)       # a square model for exclude
    mc, rc = _csr(Msq, n_items), _csr(R, n_items)
    users = np.array([3, 0, 7, 3])
    for kw in (dict(max_nbrs=6), dict(max_nbrs=6, min_nbrs=2, aggregate='sum'), dict(exclude=False, min_value=2.5, max_nbrs=6)):
        for n in (1, 5, 100):
            walk = _tup(rc.knn_topk(mc, users, n, **kw))
            got = _tup(rc.knn_topk(mc, users, n, route='reach', **kw))
            assert same(got, walk), (n, kw, first_difference(got, walk))
            assert got[2].tobytes() == walk[2].tobytes()
