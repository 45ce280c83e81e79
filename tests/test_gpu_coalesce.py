"""
csrk_coalesce and csrk_is_canonical on the card (csrc/coalesce.hip) against the NumPy restatement of the contract
(tests/coalesce_ref.py).  Every comparison goes through coalesce_ref.same: pointer dtype and values, column indices and
value dtype exactly, values bit for bit (under 'sum' a NaN stands for any NaN).  No tolerance anywhere.
"""
import numpy as np
import pytest

from coalesce_ref import coalesce_ref, same, first_difference, is_canonical, route, bits, DUPS
from combine_ref import combine_ref, same as combine_same

pytestmark = pytest.mark.gpu

INF, NAN = float('inf'), float('nan')
i4 = np.int32


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


def _run(A, ncols, dup, ptr=np.int32):
    "coalesce through the handle layer: (result tuple, route)"
    K = _K()
    h = K.to_handle(_csr(A, ncols, ptr))
    try:
        c = K.coalesce(h, dup)
        try:
            return _tup(K.from_handle(c)), K.coalesce_last_route()
        finally:
            K.release_handle(c)
    finally:
        K.release_handle(h)


def _check(A, ncols, dup, ptr=np.int32, exp=None, want_route=None, what=''):
    got, rt = _run(A, ncols, dup, ptr)
    exp = coalesce_ref(A, dup) if exp is None else exp
    assert same(got, exp, dup), (what, dup, first_difference(got, exp, dup))
    assert rt == (route(A[0], A[1]) if want_route is None else want_route), (what, dup, rt)
    return got


def _rows(rows, vals=None, dtype=np.float64, seed=0):
    "rows: a list of column lists -> (rowptrs, colinds, values); vals: a flat list, else random values of `dtype` (None: no values)"
    rp = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    ci = np.concatenate([np.zeros(0, np.int64)] + [np.asarray(r, np.int64) for r in rows]).astype(np.int32)
    if vals is not None:
        vs = np.asarray(vals, dtype=dtype)
        assert len(vs) == len(ci)
    elif dtype is None:
        vs = None
    else:
        vs = np.random.default_rng(seed).uniform(-2, 2, len(ci)).astype(dtype)
    return rp, ci, vs


def _shuffled(A, seed):
    "the same matrix with the entries of every row in a random storage order"
    rp, ci, vs = A
    rng = np.random.default_rng(seed)
    perm = np.concatenate([np.zeros(0, np.int64)] + [int(rp[i]) + rng.permutation(int(rp[i + 1] - rp[i])) for i in range(len(rp) - 1)])
    return rp, ci[perm], None if vs is None else vs[perm]


# ---- routes -----------------------------------------------------------------------------------------------------------------
def test_three_routes_one_matrix():
    rng = np.random.default_rng(1)
    ncols = 900
    lens = rng.integers(0, 40, 150)
    canon = _rows([np.sort(rng.choice(ncols, n, replace=False)) for n in lens], seed=2)
    # the same pattern with some entries stored two or three times (sorted: side by side), then every row shuffled
    rep = rng.integers(1, 4, len(canon[1]))
    rep[rng.random(len(rep)) < 0.7] = 1
    rows = [np.repeat(canon[1][int(canon[0][i]):int(canon[0][i + 1])], rep[int(canon[0][i]):int(canon[0][i + 1])]) for i in range(150)]
    sorted_rep = _rows(rows, seed=3)
    shuffled = _shuffled(sorted_rep, 4)
    assert (route(*canon[:2]), route(*sorted_rep[:2]), route(*shuffled[:2])) == (0, 1, 2)
    for dup in DUPS:
        got = _check(canon, ncols, dup, want_route=0, what='canonical')
        assert same(got, (canon[0].astype(i4), canon[1], canon[2]), 'first')          # a copy, bit for bit
        a = _check(sorted_rep, ncols, dup, want_route=1, what='sorted with repeats')
        b = _check(shuffled, ncols, dup, want_route=2, what='shuffled')
        assert np.array_equal(a[0], got[0]) and np.array_equal(a[1], got[1])          # one pattern from all three
        assert np.array_equal(b[0], got[0]) and np.array_equal(b[1], got[1])


# ---- row boundaries ---------------------------------------------------------------------------------------------------------
def _boundary_rows():
    "row r ends and the next non-empty row starts with the same column: adjacent, 1 and 3 empty rows between, first / last rows, single-entry rows"
    return [
        [5],                        # the matrix's first row: a single entry ...
        [5, 5, 7],                  # ... and its neighbour starts with the same column (and repeats it)
        [7],                        # single-entry row between two rows that end / start with 7
        [7, 9],
        [],
        [9, 9, 11, 11],             # one empty row between
        [], [], [],
        [11, 12],                   # three empty rows between
        [12],
        [12],                       # two single-entry rows side by side
        [3, 12, 12],                # ends with a repeat ...
        [12, 12],                   # ... and the matrix's last row is that column only
    ]


@pytest.mark.parametrize('form', ['sorted', 'shuffled'])
@pytest.mark.parametrize('dup', DUPS)
def test_groups_never_cross_a_row_boundary(dup, form):
    rows = _boundary_rows()
    if form == 'shuffled':
        rows = [r[::-1] for r in rows]                    # descending where a row has two columns: route 2
    n = sum(len(r) for r in rows)
    A = _rows(rows, vals=2.0 ** np.arange(n))             # every sum names its members
    exp_rp = [0, 1, 3, 4, 6, 6, 8, 8, 8, 8, 10, 11, 12, 14, 15]
    for ptr in (np.int32, np.int64):
        got = _check(A, 13, dup, ptr, want_route=1 if form == 'sorted' else 2, what=form)
        assert list(got[0]) == exp_rp
    # empty rows at both ends, and the same column on both sides of them
    B = _rows([[], [], [4, 4], [], [4], [4, 4, 4], [], []], vals=[1, 2, 4, 8, 16, 32])
    got = _check(B, 5, dup, want_route=1)
    assert list(got[0]) == [0, 0, 0, 1, 1, 2, 3, 3, 3] and list(got[1]) == [4, 4, 4]


# ---- group and block edges --------------------------------------------------------------------------------------------------
GROUP_LENGTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000)


def _edge_matrix():
    """
    One long row and a few short ones: groups of every length in GROUP_LENGTHS, each placed once so that it STARTS at an entry
    index one below a multiple of M and once so that it ENDS one past a multiple of M, for M = 64 (a wavefront), 256 (a
    workgroup of the flat kernels) and 2048 (a chunk of the scan); single entries fill the gaps; the last group ends at nnz - 1.
    """
    cols, col = [], 0

    def put(n):
        nonlocal col
        cols.extend([col] * n)
        col += 1

    def fill_to(residue, M):
        while len(cols) % M != residue:
            put(1)
    for M in (64, 256, 2048):
        for L in GROUP_LENGTHS:
            fill_to(M - 1, M)                 # the head is the last entry before a multiple of M
            put(L)
            fill_to((1 - L) % M, M)           # the last member is the first entry after a multiple of M
            put(L)
    put(257)                                  # the last group ends at nnz - 1
    n = len(cols)
    cols = np.array(cols)

    def boundary(k):
        "the first entry at or after k that starts a group"
        while cols[k] == cols[k - 1]:
            k += 1
        return k
    c2 = boundary(700)                        # rows are cut where no group is cut: [0, 1), an empty row, a long row,
    c3 = boundary(c2 + 1)                     # one whole group as a row of its own, and the rest
    cuts = [0, 1, 1, c2, c3, n]
    return [cols[a:b] for a, b in zip(cuts[:-1], cuts[1:])], col


@pytest.fixture(scope='module')
def edge_cases():
    rows, ncols = _edge_matrix()
    out = {}
    for dtype in (np.float64, np.float32):
        s = _rows(rows, dtype=dtype, seed=7)
        out[dtype, 'sorted'] = s
        out[dtype, 'shuffled'] = _shuffled(s, 8)
    return out, ncols


@pytest.mark.parametrize('form', ['sorted', 'shuffled'])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_group_and_block_edges(edge_cases, dtype, form):
    cases, ncols = edge_cases
    A = cases[dtype, form]
    assert A[1][-1] == A[1][-257] or form == 'shuffled'
    for dup in DUPS:
        got = _check(A, ncols, dup, want_route=1 if form == 'sorted' else 2, what=f'{dtype.__name__} {form}')
        assert len(got[1]) == ncols and got[2].dtype == dtype


# ---- every dup x dtype x pointer width --------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dense_repeats():
    "200 rows, 50 columns, row lengths 0 .. 300: repeats are dense"
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 301, 200)
    lens[[0, 17, 199]] = 0
    rows = [np.sort(rng.integers(0, 50, n)) for n in lens]
    out = {}
    for dtype in (np.float64, np.float32, None):
        s = _rows(rows, dtype=dtype, seed=12)
        out[dtype, 'sorted'] = s
        out[dtype, 'shuffled'] = _shuffled(s, 13)
    return out


@pytest.mark.parametrize('dtype', [np.float64, np.float32, None], ids=['f64', 'f32', 'structure'])
@pytest.mark.parametrize('dup', DUPS)
def test_every_rule_dtype_and_pointer_width(dense_repeats, dup, dtype):
    for form, rt in (('sorted', 1), ('shuffled', 2)):
        A = dense_repeats[dtype, form]
        exp = coalesce_ref(A, dup)
        assert exp[0].dtype == i4 and (exp[2] is None) == (dtype is None)
        for ptr in (np.int32, np.int64):
            _check(A, 50, dup, ptr, exp=exp, want_route=rt, what=f'{form} {ptr.__name__}')


# ---- order of addition ------------------------------------------------------------------------------------------------------
def test_sums_run_left_to_right_in_the_values_dtype():
    one = lambda vals, dt: _check(_rows([[3] * len(vals)], vals=vals, dtype=dt), 4, 'sum', want_route=1)[2]      # noqa: E731
    assert list(one([1e16, 1.0, 1.0], np.float64)) == [1e16]
    assert list(one([1.0, 1.0, 1e16], np.float64)) == [1e16 + 2]
    assert list(one([2.0 ** 24, 1, 1], np.float32)) == [2.0 ** 24]                   # not 2^24 + 2
    assert list(one([1, 1, 2.0 ** 24], np.float32)) == [2.0 ** 24 + 2]
    # the same members unsorted among other columns: the storage order is what counts (route 2)
    for dt, big, small_first in ((np.float64, 1e16, 1e16 + 2), (np.float32, 2.0 ** 24, 2.0 ** 24 + 2)):
        cols = [9, 3, 7, 3, 1, 3, 9]
        for vals, want in (([5, big, 6, 1, 7, 1, 8], big), ([5, 1, 6, 1, 7, big, 8], small_first)):
            got = _check(_rows([[2], cols, [3]], vals=[4] + vals + [2], dtype=dt), 10, 'sum', want_route=2)
            assert list(got[1]) == [2, 1, 3, 7, 9, 3] and list(got[2]) == [4, 7, want, 6, 13, 2]


# ---- special values ---------------------------------------------------------------------------------------------------------
def _f64(*words):
    return np.array(words, np.uint64).view(np.float64)


def _f32(*words):
    return np.array(words, np.uint32).view(np.float32)


@pytest.mark.parametrize('form', ['sorted', 'unsorted'])
def test_special_values(form):
    """
    Row 0 holds lone values (groups of one), rows 1 .. hold one case each as a group of column 2 -- alone in the row
    ('sorted', route 1) or between a larger and a smaller column ('unsorted', route 2).
    """
    for dt, mk, qnan, qnan2, sub in ((np.float64, _f64, 0x7ff8000000000123, 0xfff800000000beef, 0x0000000000000001),
                                     (np.float32, _f32, 0x7fc00abc, 0xffc00def, 0x00000001)):
        P, Q, S = mk(qnan)[0], mk(qnan2)[0], mk(sub)[0]
        groups = [[-0.0, -0.0], [0.0, -0.0], [-0.0, 0.0], [INF, -INF], [1.0, P, INF], [P, Q], [Q, P], [P, 2.0, Q, 5.0],
                  [S, S], [S], [3.0, -3.0], [-0.0, 0.0, -0.0], [2.0, P], [INF, 1.0, INF]]
        lone = [-0.0, P, S, Q]
        rows, vals = [list(range(10, 10 + len(lone)))], list(lone)
        for g in groups:
            if form == 'sorted':
                rows.append([2] * len(g))
                vals += g
            else:
                rows.append([7] + [2] * len(g) + [0])
                vals += [1.0] + g + [1.0]
        A = _rows(rows, vals=np.array(vals, dt), dtype=dt)
        for dup in DUPS:
            got = _check(A, 20, dup, what=f'{dt.__name__} {form}')
            v = got[2]
            at = (lambda k: v[len(lone) + k]) if form == 'sorted' else (lambda k: v[len(lone) + 3 * k + 1])      # noqa: E731
            assert list(bits(v[:len(lone)])) == list(bits(np.array(lone, dt))), dup       # lone values: bit for bit, every rule
            word = lambda x: int(bits(np.array([x], dt))[0]) & (2 ** (8 * dt().itemsize) - 1)     # noqa: E731
            if dup == 'sum':
                assert np.signbit(at(0)) and at(0) == 0 and not np.signbit(at(1)) and not np.signbit(at(2))
                assert np.isnan(at(3)) and np.isnan(at(4)) and at(10) == 0 and not np.signbit(at(10))
                assert word(at(9)) == sub and word(at(8)) == 2 * sub                      # subnormal adds are exact
            elif dup == 'first':
                assert np.signbit(at(2)) and word(at(5)) == qnan and word(at(6)) == qnan2 and word(at(9)) == sub
            elif dup == 'last':
                assert not np.signbit(at(2)) and word(at(5)) == qnan2 and word(at(6)) == qnan and word(at(12)) == qnan
            elif dup == 'max':
                assert word(at(4)) == qnan                                                # NaN above +Inf
                assert word(at(5)) == qnan and word(at(6)) == qnan2                       # NaNs tie: the earlier
                assert not np.signbit(at(1)) and np.signbit(at(2)) and np.signbit(at(11))  # +-0 tie: the earlier
                assert word(at(7)) == qnan and at(13) == INF
            else:
                assert at(7) == 2.0 and at(4) == 1.0                                      # a NaN only when every member is one
                assert word(at(5)) == qnan2 and word(at(6)) == qnan                       # all NaN: the last of the order
                assert np.signbit(at(1)) and not np.signbit(at(2)) and np.signbit(at(11))  # +-0 tie: the later
                assert at(12) == 2.0 and at(13) == 1.0


# ---- shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32, None], ids=['f64', 'f32', 'structure'])
def test_degenerate_shapes(dtype):
    for dup in DUPS:
        for ptr in (np.int32, np.int64):
            for nrows in (0, 1, 5):                       # nrows = 0; nnz = 0; all rows empty
                got = _check(_rows([[]] * nrows, dtype=dtype), 7, dup, ptr, want_route=0)
                assert got[0].dtype == i4 and list(got[0]) == [0] * (nrows + 1) and len(got[1]) == 0
                assert (got[2] is None) == (dtype is None) and (dtype is None or (got[2].dtype == dtype and len(got[2]) == 0))
            _check(_rows([[], [4], []], dtype=dtype), 7, dup, ptr, want_route=0)                      # one entry
            got = _check(_rows([[6] * 500], dtype=dtype, seed=3), 7, dup, ptr, want_route=1)          # one column 500 times
            assert list(got[0]) == [0, 1] and list(got[1]) == [6]


# ---- determinism ------------------------------------------------------------------------------------------------------------
def test_two_calls_and_both_pointer_widths_give_the_same_bytes(dense_repeats):
    for dtype in (np.float64, np.float32):
        A = dense_repeats[dtype, 'shuffled']
        for dup in DUPS:
            runs = [_run(A, 50, dup, ptr)[0] for ptr in (np.int32, np.int32, np.int64, np.int64)]
            for r in runs[1:]:
                for x, y in zip(r, runs[0]):
                    assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (dtype, dup)


# ---- h untouched ------------------------------------------------------------------------------------------------------------
def test_the_operand_is_not_modified_and_still_multiplies():
    import scipy.sparse as sps
    K = _K()
    rng = np.random.default_rng(21)
    rows = [rng.integers(0, 40, n) for n in rng.integers(0, 60, 300)]
    n = sum(len(r) for r in rows)
    A = _rows(rows, vals=rng.integers(-8, 9, n).astype(np.float64))        # integers: every product and sum is exact
    x = rng.integers(-4, 5, 40).astype(np.float64)
    y_exp = sps.csr_matrix((A[2], A[1], A[0]), shape=(300, 40)) @ x
    h = K.to_handle(_csr(A, 40))
    try:
        y0 = K.mult_vec(h, x)
        assert np.array_equal(y0, y_exp)
        for dup in DUPS:
            c = K.coalesce(h, dup)
            assert K.coalesce_last_route() == 2
            K.release_handle(c)
            got = _tup(K.from_handle(h))
            assert same(got, (A[0].astype(i4), A[1], A[2]), 'first'), dup
            assert K.is_canonical(h) == (False, is_canonical(A[0], A[1])[1])
            assert np.array_equal(K.mult_vec(h, x), y_exp)
    finally:
        K.release_handle(h)


# ---- the dead end is open ---------------------------------------------------------------------------------------------------
def test_a_repeating_matrix_reaches_combine_through_coalesce():
    from csr_amd._lib import CsrkError
    K = _K()
    rng = np.random.default_rng(31)
    rows = [[2, 5, 9], [1, 4, 4, 8], [0, 3], [7, 7, 7]] + [np.sort(rng.integers(0, 30, n)) for n in rng.integers(0, 25, 60)]
    A = _rows(rows, seed=32)
    B = _rows([np.sort(rng.choice(30, n, replace=False)) for n in rng.integers(0, 12, 64)], seed=33)
    a, b = _csr(A, 30), _csr(B, 30)
    assert a.is_canonical() is False and a.is_canonical(with_row=True) == (False, 1)
    with pytest.raises(CsrkError) as ei:
        a.add(b)
    assert 'operand A is not canonical: row 1 ' in str(ei.value)
    for dup in DUPS:
        c = a.coalesce(dup)
        assert c.is_canonical() is True and c.is_canonical(with_row=True) == (True, None)
        exp = combine_ref(coalesce_ref(A, dup), B, 'add', 2.0, -1.0)
        got = _tup(c.add(b, 2.0, -1.0))
        assert combine_same(got, exp, 'add'), dup
    assert same(_tup(a.sum_duplicates()), coalesce_ref(A, 'sum'), 'sum')
    # on one handle: the result is known to be canonical -- a second coalesce copies, combine accepts it
    h, bh = K.to_handle(a), K.to_handle(b)
    try:
        assert K.is_canonical(h) == (False, 1)
        c = K.coalesce(h, 'sum')
        assert K.coalesce_last_route() == 1
        assert K.is_canonical(c) == (True, None)
        c2 = K.coalesce(c, 'min')
        assert K.coalesce_last_route() == 0
        s = K.combine(c2, bh, 'multiply')
        assert combine_same(_tup(K.from_handle(s)), combine_ref(coalesce_ref(A, 'sum'), B, 'multiply'), 'multiply')
        for x in (s, c2, c):
            K.release_handle(x)
        K.order_columns(h)                                  # sorts only: the repeats stay, and the handle looks again
        assert K.is_canonical(h) == (False, 1)
    finally:
        K.release_handle(h)
        K.release_handle(bh)


def test_from_coo_with_duplicates():
    import scipy.sparse as sps
    from csr_amd import CSR
    rng = np.random.default_rng(41)
    n, shape = 5000, (90, 40)
    rows, cols = rng.integers(0, shape[0], n), rng.integers(0, shape[1], n)
    vals = rng.integers(-5, 6, n).astype(np.float64)
    S = sps.coo_matrix((vals, (rows, cols)), shape=shape).tocsr()
    S.sort_indices()
    m = CSR.from_coo(rows, cols, vals, shape=shape, duplicates='sum')
    assert same(_tup(m), (S.indptr.astype(i4), S.indices.astype(i4), S.data), 'first')
    kept = CSR.from_coo(rows, cols, vals, shape=shape)
    assert kept.nnz == n
    for dup in DUPS:
        m = CSR.from_coo(rows, cols, vals.astype(np.float32), shape=shape, duplicates=dup)
        exp = coalesce_ref((kept.rowptrs, kept.colinds, kept.values.astype(np.float32)), dup)
        assert same(_tup(m), exp, dup), dup
