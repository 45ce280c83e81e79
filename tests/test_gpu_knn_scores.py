"""
csrk_knn_scores on the card (csrc/knn_scores.hip) against the plain-Python restatement of its contract
(tests/knn_scores_ref.py).  Every comparison is bit for bit -- row pointers, columns and values (a NaN stands for any NaN) --
except the cross-check against the existing product, whose sums are taken in another order.  The shapes are the smallest
that reach each branch; the limits are read from knn_scores_limits().
"""
import ctypes

import numpy as np
import pytest

from combine_ref import combine_ref
from knn_scores_ref import knn_scores_ref, same, first_difference
from topk_ref import topk_rows_ref

pytestmark = pytest.mark.gpu

i4 = np.int32
INF, NAN = float('inf'), float('nan')
AGG = ('weighted-average', 'sum')


def _K():
    from csr_amd.kernels import hip as K
    return K


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


def _check(M, R, n_items, users, what='', mcsr=None, rcsr=None, **kw):
    "CSR.knn_scores against the restatement; mcsr / rcsr: the operands' CSR objects when a caller reuses them"
    mcsr = _csr(M, n_items) if mcsr is None else mcsr
    rcsr = _csr(R, n_items) if rcsr is None else rcsr
    got = _tup(rcsr.knn_scores(mcsr, users, **kw))
    exp = knn_scores_ref(M, R, users, **kw)
    assert same(got, exp), (what, kw, first_difference(got, exp))
    return got


def _descending_model(rng, lengths, n_items):
    "rows of the given lengths: distinct columns in random (not ascending) order, similarities descending"
    cols = [rng.permutation(n_items)[:n] for n in lengths]
    vals = [np.sort(rng.uniform(0.05, 1.0, n))[::-1] for n in lengths]
    return _rows(cols, vals)


# ---- the walk: model row lengths, the cut, the minimum -----------------------------------------------------------------------
@pytest.fixture(scope='module')
def walk_case():
    L = _K().knn_scores_limits()[0]
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
    # 0: no limit; 1; inside a step; hits - 1, hits, hits + 1 for rows of L - 1, L, L + 1 and 2 L + 1 entries (user 0), which
    # also puts the cut on a step boundary (L, 2 L) and one past it
    for mx in (0, 1, L // 2, L - 2, L - 1, L, L + 1, L + 2, 2 * L, 2 * L + 1, 2 * L + 2):
        _check(M, R, n_items, users, 'cut', mc, rc, max_nbrs=mx, aggregate=aggregate)
    _check(M, R, n_items, users, 'offsets', mc, rc, max_nbrs=L, aggregate=aggregate, offsets=off)
    _check(M, R, n_items, users, 'offsets', mc, rc, aggregate=aggregate, offsets=off)


def test_a_cut_by_column_order_would_be_caught(walk_case):
    L, n_items, M, R, mc, rc = walk_case
    got = _check(M, R, n_items, [0], 'cut', mc, rc, max_nbrs=2, aggregate='sum')
    rp, ci, vs = M
    i = 5                                              # a row of 2 L + 1 entries, all of them hits for user 0
    c, s = ci[rp[i]:rp[i + 1]], vs[rp[i]:rp[i + 1]]
    o = np.argsort(c)
    by_storage, by_column = s[0] + s[1], s[o[0]] + s[o[1]]      # the two best neighbours / the two of the smallest columns
    at = list(got[1][:got[0][1]]).index(i)
    assert got[2][at] == by_storage != by_column


@pytest.mark.parametrize('aggregate', AGG)
def test_min_nbrs(walk_case, aggregate):
    L, n_items, M, R, mc, rc = walk_case
    for mn in (1, 2, L - 1, L, L + 1, L + 2, 2 * L + 1, 2 * L + 2):       # hits, hits + 1 of every row length: present, absent
        got = _check(M, R, n_items, [0, 1, 2], 'min', mc, rc, min_nbrs=mn, aggregate=aggregate)
    assert got[0][-1] == 0 and len(got[0]) == 4                            # rows that store nothing: the pointers are complete
    got = _check(M, R, n_items, [0, 2], 'min above max', mc, rc, max_nbrs=2, min_nbrs=3, aggregate=aggregate)
    assert list(got[0]) == [0, 0, 0]
    _check(M, R, n_items, [0, 2], 'min = max', mc, rc, max_nbrs=3, min_nbrs=3, aggregate=aggregate)


# ---- tiles of targets, rating row lengths ---------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['below', 'exact', 'above', 'empty tile'])
def test_target_counts(which):
    T = _K().knn_scores_limits()[1]
    n_targets = {'below': T - 1, 'exact': T, 'above': T + 1, 'empty tile': 2 * T + 1}[which]
    rng = np.random.default_rng(len(which))
    n_items = 40
    lengths = rng.integers(0, 4, n_targets)
    if which == 'empty tile':
        lengths[T:2 * T] = 0                          # the middle tile stores nothing; the row goes on in the last one
        lengths[2 * T] = 3
    M = _descending_model(rng, lengths, n_items)
    R = _rows([np.sort(rng.choice(n_items, n, replace=False)) for n in (n_items, 0, 12)], [rng.integers(1, 6, n) for n in (n_items, 0, 12)])
    mc, rc = _csr(M, n_items), _csr(R, n_items)
    for agg in AGG:
        got = _check(M, R, n_items, [2, 0, 1, 0], which, mc, rc, aggregate=agg)
        _check(M, R, n_items, [2, 0, 1, 0], which, mc, rc, aggregate=agg, min_nbrs=2, max_nbrs=2)
    if which == 'empty tile':
        assert got[1][got[0][1]:got[0][2]].max() == 2 * T       # user 0 rated everything: the last target, beyond the empty tile, is stored


@pytest.mark.parametrize('tiles', [2, 3])
def test_several_tiles_per_workgroup(tiles):
    "enough (row, tile) pairs that a workgroup takes 2 of a row's 3 tiles (a short last run) or all 3: the same bits as one each"
    lim = _K().knn_scores_limits()
    T, tiles_max, fill = lim[1], lim[4], lim[5]
    assert tiles_max >= 3
    rng = np.random.default_rng(17)
    n_items, n_targets = 40, 2 * T + 1
    M = _descending_model(rng, rng.integers(0, 4, n_targets), n_items)
    R = _rows([np.sort(rng.choice(n_items, n, replace=False)) for n in (n_items, 0, 12)], [rng.integers(1, 6, n) for n in (n_items, 0, 12)])
    mc, rc = _csr(M, n_items), _csr(R, n_items)
    one = _check(M, R, n_items, [0, 1, 2], 'one tile each', mc, rc, max_nbrs=2)
    n_rows = -(-tiles * fill // 3)                       # n_rows x 3 tiles / fill == tiles
    assert n_rows * 3 // fill == tiles
    users = np.resize([2, 0, 1, 0], n_rows)
    got = _tup(rc.knn_scores(mc, users, max_nbrs=2))
    lens = np.diff(one[0])[users]                         # a repeated row is the same row: the expected result from `one`
    exp_rp = np.concatenate(([0], np.cumsum(lens)))
    take = np.concatenate([np.arange(one[0][u], one[0][u + 1]) for u in users])
    exp = (exp_rp, one[1][take], one[2][take])
    assert same(got, exp), first_difference(got, exp)


def test_rating_row_lengths():
    "rows staged in LDS and rows searched in device memory: the same bits"
    D = _K().knn_scores_limits()[2]
    rng = np.random.default_rng(7)
    n_items = D + 9
    lens = [0, 1, D - 1, D, D + 1]
    R = _rows([np.sort(rng.choice(n_items, n, replace=False)) for n in lens], [rng.integers(1, 6, n) for n in lens])
    # neighbours at both ends of the item range, so that the search reaches the first and the last entry of a row
    cols = [np.concatenate(([0, n_items - 1], rng.permutation(np.arange(1, n_items - 1))[:18])) for _ in range(24)]
    cols = [rng.permutation(c) for c in cols]
    M = _rows(cols, [np.sort(rng.uniform(0.05, 1.0, 20))[::-1] for _ in cols])
    mc, rc = _csr(M, n_items), _csr(R, n_items)
    for agg in AGG:
        _check(M, R, n_items, [4, 0, 3, 1, 2], 'ratings', mc, rc, aggregate=agg)
        _check(M, R, n_items, [4, 0, 3, 1, 2], 'ratings', mc, rc, aggregate=agg, max_nbrs=5, min_nbrs=2, offsets=np.arange(5.0))
    # the longest row in both regimes gives what the restatement gives: user 3 (D entries, LDS) and user 4 (D + 1, memory)
    # on a model row that only holds items both rated must agree bit for bit
    both = np.intersect1d(R[1][R[0][3]:R[0][4]], R[1][R[0][4]:R[0][5]])[:17]
    r2 = R[2].copy()
    for c in both:                                    # the same ratings for the shared items
        a = R[0][3] + np.searchsorted(R[1][R[0][3]:R[0][4]], c)
        b = R[0][4] + np.searchsorted(R[1][R[0][4]:R[0][5]], c)
        r2[b] = r2[a]
    M1 = _rows([rng.permutation(both)], [np.sort(rng.uniform(0.05, 1.0, len(both)))[::-1]])
    got = _check(M1, (R[0], R[1], r2), n_items, [3, 4], 'both regimes')
    assert got[2][0].tobytes() == got[2][1].tobytes()


def test_columns_that_share_a_filter_bit():
    "unrated neighbours whose column equals a rated column modulo the filter's size are searched for and not found"
    L, B = _K().knn_scores_limits()[0], _K().knn_scores_limits()[3]
    n_items = 2 * B + 9
    rated = [3, 40, B + 7, 2 * B + 1]
    R = _rows([rated, []], [[4.0, 2.0, 5.0, 3.0], []])
    alias = [B + 3, 2 * B + 3, 7, 2 * B + 7, 1, B + 1, B + 40]           # none is rated, every one shares a rated column's bit
    cols = [alias,                                                        # only aliases: the target is absent
            [B + 3, 3, 7, B + 7, 1, 2 * B + 1],                           # an alias in front of every hit
            alias + rated,
            (alias * 3)[:L - 1] + [40] + alias[:2] + [3],                 # hits on both sides of a step boundary
            rated[::-1]]
    M = _rows(cols, [np.linspace(1.0, 0.1, len(c)) for c in cols])
    for agg in AGG:
        for mx in (0, 1, 2):
            got = _check(M, R, n_items, [0, 1, 0], 'aliases', max_nbrs=mx, aggregate=agg)
        assert list(got[1][:got[0][1]]) == [1, 2, 3, 4] and got[0][2] == got[0][1]


# ---- value types, pointer widths ------------------------------------------------------------------------------------------
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
    for pm in (np.int32, np.int64):
        for pr in (np.int32, np.int64):
            mc, rc = _csr(M, n_items, pm), _csr(R, n_items, pr)
            for agg in AGG:
                _check(M, R, n_items, users, (pm, pr), mc, rc, aggregate=agg, max_nbrs=4)


# ---- the list of rows -------------------------------------------------------------------------------------------------------
def test_the_list_of_rows(small_case):
    n_items, M, R = small_case
    mc, rc = _csr(M, n_items), _csr(R, n_items)
    n_users = len(R[0]) - 1
    rng = np.random.default_rng(3)
    full = _check(M, R, n_items, np.arange(n_users), 'all', mc, rc, max_nbrs=5)
    none = _tup(rc.knn_scores(mc, max_nbrs=5))                                # users=None: all rows
    assert same(none, full)
    again = _tup(rc.knn_scores(mc, np.arange(n_users), max_nbrs=5))           # a second call: the same bits
    assert same(again, full) and again[2].tobytes() == full[2].tobytes()
    shuffled = rng.permutation(n_users)
    _check(M, R, n_items, shuffled, 'shuffled', mc, rc, max_nbrs=5)
    rep = np.array([4, 4, 1, 4, 8, 1])
    got = _check(M, R, n_items, rep, 'repeated', mc, rc, max_nbrs=5)
    for r, u in enumerate(rep):                                               # a row alone equals the same row inside a batch
        alone = _tup(rc.knn_scores(mc, [u], max_nbrs=5))
        b, e = got[0][r], got[0][r + 1]
        assert np.array_equal(alone[1], got[1][b:e]) and alone[2].tobytes() == got[2][b:e].tobytes(), (r, u)
        fb, fe = full[0][u], full[0][u + 1]
        assert np.array_equal(alone[1], full[1][fb:fe]) and alone[2].tobytes() == full[2][fb:fe].tobytes(), (r, u)
    empty = rc.knn_scores(mc, np.zeros(0, np.int64))
    assert (empty.nrows, empty.ncols, empty.nnz) == (0, len(M[0]) - 1, 0) and list(empty.rowptrs) == [0]


def test_empty_operands():
    n_items = 6
    M = _rows([[1, 2], [0]], [[0.5, 0.25], [1.0]])
    R = _rows([[0, 2], [1]], [[3.0, 4.0], [5.0]])
    E_m, E_r, no_targets = _rows([[], []], [[], []]), _rows([[], []], [[], []]), _rows([], [])
    for m, r, what in ((E_m, R, 'model.nnz = 0'), (M, E_r, 'ratings.nnz = 0'), (no_targets, R, 'n_targets = 0')):
        got = _check(m, r, n_items, [1, 0, 1], what)
        assert got[0].dtype == np.int32 and list(got[0]) == [0, 0, 0, 0] and got[2].dtype == np.float64
    out = _csr(R, n_items).knn_scores(_csr(no_targets, n_items), [0])
    assert (out.nrows, out.ncols) == (1, 0)


# ---- special values -------------------------------------------------------------------------------------------------------------
def test_zero_similarities_are_hits():
    n_items = 8
    R = _rows([[0, 1, 2, 3, 4]], [[1.0, 2.0, 3.0, 4.0, 5.0]])
    M = _rows([[0, 1, 2], [3, 2, 1], [5, 0, 1], [0, 1]], [[0.0, -0.0, 1.0], [-0.0, 0.0, 0.5], [9.0, 0.0, 0.0], [0.0, 0.0]])
    for agg in AGG:
        for mx in (0, 1, 2, 3):
            _check(M, R, n_items, [0], 'zeros', max_nbrs=mx, aggregate=agg)
        _check(M, R, n_items, [0], 'zeros', min_nbrs=3, aggregate=agg)
    got = _check(M, R, n_items, [0], 'zeros', max_nbrs=2)
    # the zeros used up the two neighbours: den = 0 stores NaN at targets 0 and 1; target 2 skipped the unrated item 5
    assert list(got[1]) == [0, 1, 2, 3] and np.isnan(got[2][[0, 1, 2, 3]]).all()
    got = _check(M, R, n_items, [0], 'zeros')
    assert list(got[2][:2]) == [3.0, 2.0] and np.isnan(got[2][2:]).all()
    # explicit zero ratings are hits too
    Rz = _rows([[0, 1, 2]], [[0.0, -0.0, 0.0]])
    got = _check(M, Rz, n_items, [0], 'zero ratings', min_nbrs=2)
    assert list(got[1]) == [0, 1, 2, 3]


@pytest.mark.parametrize('bad', [NAN, INF, -INF])
def test_nan_and_inf_reach_only_the_walks_that_use_them(bad):
    L = _K().knn_scores_limits()[0]
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
        # the cut before the bad similarity: a NaN in an entry after the cut changes nothing
        clean = (M[0], M[1], np.where(np.isfinite(M[2]), M[2], 0.25))
        for mx in (L + 2, L + 3):
            got = _check(M, R, n_items, [1], bad, mc, rc, aggregate=agg, max_nbrs=mx)
            ref = knn_scores_ref(clean, R, [1], max_nbrs=mx, aggregate=agg)
            assert (got[2][1].tobytes() == ref[2][1].tobytes()) == (mx == L + 2)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(small_case):
    """
    Every CSRK_ERR_INVALID of rule 7 that one card can show, with its status and the key words of its text; the long model
    row (CSRK_ERR_UNSUPPORTED) is the next test.  NOT tested: "operands on different devices", which needs a second card,
    and a RATINGS row of more than 2^31 - 1 entries, which cannot be built -- ratings has to be canonical, and a strictly
    ascending row holds at most ncols <= 2^31 - 1 entries, so that refusal is reachable for the model only.
    """
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
        rc = lib.csrk_knn_scores(mh, rh, None if rows is None else rows.ctypes.data, n, mx, mn, agg, None, ctypes.byref(o) if out else None)
        msg = _lib.last_error()
        if out:
            assert (o.value == 0) == (rc != _lib.OK), (rc, msg)
            if rc == _lib.OK:
                lib.csrk_free(o.value)
        return rc, msg

    with releasing(K.to_handle(_csr(M, n_items)), K) as mh, releasing(K.to_handle(_csr(R, n_items)), K) as rh, \
            releasing(K.to_handle(_csr(M, n_items + 1)), K) as wide, releasing(K.to_handle(_csr(unsorted, n_items)), K) as bad:
        INV = _lib.ERR_INVALID
        for args, words in (((mh.H, rh.H, one, 1, 0, 1, 0, False), ('out', 'NULL')),
                            ((0, rh.H, one, 1), ('invalid csrk handle',)),
                            ((mh.H, 12345, one, 1), ('invalid csrk handle',)),
                            ((wide.H, rh.H, one, 1), ('columns', str(n_items + 1))),
                            ((mh.H, rh.H, one, -1), ('n_rows',)),
                            ((mh.H, rh.H, None, 1), ('rows is NULL',)),
                            ((mh.H, rh.H, one, 1, -1), ('max_nbrs',)),
                            ((mh.H, rh.H, one, 1, 0, 0), ('min_nbrs',)),
                            ((mh.H, rh.H, one, 1, 0, 1, 2), ('aggregate',)),
                            ((mh.H, rh.H, one, 1, 0, 1, -1), ('aggregate',)),
                            ((mh.H, bad.H, one, 1), ('ratings', 'not canonical', 'row 1')),
                            ((mh.H, rh.H, rows, 3), ('rows[2]', str(n_users))),
                            ((mh.H, rh.H, rows[3:], 1), ('rows[0]', '-1'))):
            rc, msg = call(*args)
            assert rc == INV and all(w in msg for w in words), (args[2:], rc, msg)
        assert call(mh.H, rh.H, rows, 2)[0] == _lib.OK                       # the good part of the same list
        assert call(bad.H, rh.H, one, 1)[0] == _lib.OK                       # a non-canonical MODEL is taken
        assert call(mh.H, rh.H, None, 0)[0] == _lib.OK                       # NULL rows with n_rows = 0
        assert call(mh.H, bad.H, None, 0)[0] == _lib.OK                      # an empty list: nothing launched, not even the look at ratings
        assert call(mh.H, bad.H, one, 1, -1)[0] == INV                       # ... but the scalar arguments are still checked
        assert call(rh.H, rh.H, one, 1)[0] == _lib.OK                        # model == ratings is allowed ...
        rc, msg = call(mh.H, mh.H, one, 1)                                   # ... and checked as ratings: this one is unsorted
        assert rc == INV and 'not canonical' in msg
    # the Python layer turns the library's refusal of a non-canonical ratings into ValueError
    with pytest.raises(ValueError) as ei:
        _csr(unsorted, n_items).knn_scores(_csr(M, n_items))
    assert 'not canonical' in str(ei.value)


def test_a_model_row_above_int32_is_unsupported():
    """
    One structure-only model row of 2^31 entries (column 0 over and over: the model need not be canonical), int64 row
    pointers [0, 2^31], in HBM through csrk_create_device (8 GiB, not copied): CSRK_ERR_UNSUPPORTED with its words, *out = 0,
    no walk launched.  A row of 2^31 - 1 entries is not built: it would be taken, and walked.
    """
    import torch
    from csr_amd import _lib
    from csr_amd.kernels import releasing
    K, lib = _K(), _lib.lib
    free, total = torch.cuda.mem_get_info()
    if total < 64 * 2**30 or free < 16 * 2**30:
        pytest.skip('needs 8 GiB of HBM for one model row')
    n_items, nnz = 8, 2**31
    R = _rows([[0, 3]], [[4.0, 2.0]])
    ci = torch.zeros(nnz, dtype=torch.int32, device='cuda')
    rp = torch.tensor([0, nnz], dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    mh, out = _lib.handle_t(0), _lib.handle_t(77)
    _lib.check(lib.csrk_create_device(1, n_items, nnz, rp.data_ptr(), 1, ci.data_ptr(), None, _lib.VAL_NONE, ctypes.byref(mh)))
    try:
        one = np.array([0], i4)
        with releasing(K.to_handle(_csr(R, n_items)), K) as rh:
            for agg in (0, 1):
                rc = lib.csrk_knn_scores(mh.value, rh.H, one.ctypes.data, 1, 20, 1, agg, None, ctypes.byref(out))
                msg = _lib.last_error()
                assert rc == _lib.ERR_UNSUPPORTED and out.value == 0, (rc, msg)
                assert 'knn_scores' in msg and 'a row of model' in msg and '2^31 - 1' in msg, msg
            # the refusals that need no look at the device still come first, and an empty list is still an empty result
            assert lib.csrk_knn_scores(mh.value, rh.H, one.ctypes.data, 1, 20, 0, 0, None, ctypes.byref(out)) == _lib.ERR_INVALID
            assert lib.csrk_knn_scores(mh.value, rh.H, None, 0, 20, 1, 0, None, ctypes.byref(out)) == _lib.OK and out.value != 0
            _lib.check(lib.csrk_free(out.value))
    finally:
        _lib.check(lib.csrk_free(mh.value))
        del ci, rp
        torch.cuda.empty_cache()


def test_model_may_be_the_ratings():
    "one handle as both operands (item-item co-occurrence of a square matrix): allowed, locked once"
    K = _K()
    from csr_amd.kernels import releasing
    S = _rows([[0, 2], [1], [0, 1, 2]], [[1.0, 2.0], [3.0], [0.5, 0.25, 4.0]])
    with releasing(K.to_handle(_csr(S, 3)), K) as h:
        with releasing(K.knn_scores(h, h, [2, 0]), K) as o:
            got = _tup(K.from_handle(o))
    assert same(got, knn_scores_ref(S, S, [2, 0]))


# ---- the result is canonical and feeds the existing operations --------------------------------------------------------------------
def test_canonical_result_and_knn_topk(small_case):
    K = _K()
    from csr_amd.kernels import releasing
    n_items, M, R = small_case
    rng = np.random.default_rng(12)
    # a square model for exclude: n_items targets
    Msq = _descending_model(rng, rng.integers(0, 25, n_items), n_items)
    mc, rc = _csr(Msq, n_items), _csr(R, n_items)
    users = np.array([3, 0, 7, 3])
    ref = knn_scores_ref(Msq, R, users, max_nbrs=6)
    with releasing(K.to_handle(mc), K) as mh, releasing(K.to_handle(rc), K) as rh:
        with releasing(K.knn_scores(mh, rh, users, 6), K) as sh:
            assert K.is_canonical(sh) == (True, None)
            with releasing(K.pick_rows(rh, users, False), K) as xh, releasing(K.combine(sh, xh, 'drop'), K) as dh:
                dropped = _tup(K.from_handle(dh))
    X = _rows([R[1][R[0][u]:R[0][u + 1]] for u in users])
    exp_drop = combine_ref(ref, (X[0].astype(i4), X[1], None), 'drop')
    assert same(dropped, exp_drop), first_difference(dropped, exp_drop)
    for n in (1, 5, 100):
        exp = topk_rows_ref(exp_drop[0], exp_drop[1], exp_drop[2], n)
        got = _tup(rc.knn_topk(mc, users, n, max_nbrs=6))
        assert same(got, exp), (n, first_difference(got, exp))
        exp = topk_rows_ref(ref[0], ref[1], ref[2], n, 2.5)
        got = _tup(rc.knn_topk(mc, users, n, exclude=False, min_value=2.5, max_nbrs=6))
        assert same(got, exp), (n, first_difference(got, exp))


# ---- against the existing product ---------------------------------------------------------------------------------------------------
def test_unlimited_sum_against_the_existing_product(small_case):
    n_items, M, R = small_case
    rng = np.random.default_rng(13)
    users = rng.permutation(len(R[0]) - 1)
    mc, rc = _csr(M, n_items), _csr(R, n_items)
    got = _check(M, R, n_items, users, 'sum', mc, rc, aggregate='sum')
    ones = _csr((R[0], R[1], np.ones(len(R[1]))), n_items)
    prod = ones.pick_rows(users).multiply(mc, transpose=True)
    prod.sort_rows()
    assert np.array_equal(prod.rowptrs, got[0]) and np.array_equal(prod.colinds, got[1])      # the pattern, exactly
    abs_model = _csr((M[0], M[1], np.abs(M[2])), n_items)
    bound = ones.pick_rows(users).multiply(abs_model, transpose=True)
    bound.sort_rows()
    assert np.array_equal(bound.colinds, got[1])
    assert np.all(np.abs(prod.values - got[2]) <= 1e-12 * bound.values)                      # sums taken in another order
