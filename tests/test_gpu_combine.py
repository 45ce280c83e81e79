"""
csrk_combine on the card (csrc/combine.hip) against the NumPy restatement of its contract (tests/combine_ref.py).  Every
comparison goes through combine_ref.same: pointer dtype and values, column indices and value dtype exactly, values bit for
bit (under add and multiply a NaN stands for any NaN).  No tolerance anywhere.
"""
from fractions import Fraction

import numpy as np
import pytest

from combine_ref import combine_ref, same, first_difference, OPS
from special_values import raw_bits_equal
from topk_ref import topk_rows_ref

pytestmark = pytest.mark.gpu

INF, NAN = float('inf'), float('nan')
METHOD = {'add': 'add', 'multiply': 'multiply_entries', 'keep': 'keep_entries', 'drop': 'drop_entries'}


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


def _run(A, B, ncols, op, alpha=1.0, beta=1.0, ptr=(np.int32, np.int32)):
    a, b = _csr(A, ncols, ptr[0]), _csr(B, ncols, ptr[1])
    if op == 'add':
        return _tup(a.add(b, alpha, beta))
    return _tup(getattr(a, METHOD[op])(b))


def _check(A, B, ncols, op, alpha=1.0, beta=1.0, ptr=(np.int32, np.int32), exp=None, what=''):
    got = _run(A, B, ncols, op, alpha, beta, ptr)
    exp = combine_ref(A, B, op, alpha, beta) if exp is None else exp
    assert same(got, exp, op), (what, op, alpha, beta, first_difference(got, exp, op))
    return got


def _rows_to_tuple(rows, dtype=np.float64, seed=0):
    "rows: a list of column arrays -> (rowptrs, colinds, values) with values that are not symmetric in A and B"
    rng = np.random.default_rng(seed)
    rp = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    ci = np.concatenate([np.zeros(0, np.int64)] + [np.asarray(r, np.int64) for r in rows]).astype(np.int32)
    vs = None if dtype is None else rng.uniform(-2, 2, len(ci)).astype(dtype)
    return rp, ci, vs


RELATIONS = ('disjoint', 'equal', 'a_in_b', 'b_in_a', 'interleaved', 'b_before_a', 'b_after_a')


def _pair(rng, rel, T, universe):
    "column sets of one row of A and of B with len_a + len_b == T (as near as the relation allows) out of range(universe)"
    pick = lambda n: np.sort(rng.choice(universe, n, replace=False))      # noqa: E731
    if rel == 'equal':
        c = pick(T // 2)
        return c, c.copy()
    if rel in ('a_in_b', 'b_in_a'):
        big = pick(T - T // 3)
        small = np.sort(rng.choice(big, T // 3, replace=False)) if T // 3 else big[:0]
        return (small, big) if rel == 'a_in_b' else (big, small)
    la = T // 2
    if rel == 'interleaved':                        # independent draws: dense matches in a small universe, rare in a large one
        return pick(la), pick(T - la)
    c = pick(T)
    if rel == 'disjoint':
        sel = np.zeros(T, bool)
        sel[rng.choice(T, la, replace=False)] = True
        return c[sel], c[~sel]
    return (c[T - la:], c[:T - la]) if rel == 'b_before_a' else (c[:la], c[la:])


@pytest.mark.parametrize('universe', ['dense', 'sparse'])
@pytest.mark.parametrize('which', [0, 1, 2])
def test_row_class_boundaries(which, universe):
    lim = _K().combine_limits()
    L, Lmax = lim[which], max(lim)
    rng = np.random.default_rng(100 + which)
    lengths = [0, 1, 2, L - 1, L, L + 1, 3 * Lmax + 7]
    ra, rb = [[]] * 3, [[]] * 3                                             # empty rows at the start ...
    for rel in RELATIONS:
        for T in lengths:
            u = 2 * T + 2 if universe == 'dense' else 2 ** 30
            a, b = _pair(rng, rel, T, u)
            ra.append(a)
            rb.append(b)
        ra += [[], []]                                                     # ... in the middle ...
        rb += [[], []]
    ra += [[]] * 2                                                         # ... and at the end
    rb += [[]] * 2
    ncols = 2 ** 30 + 1
    A, B = _rows_to_tuple(ra, seed=1), _rows_to_tuple(rb, seed=2)
    for op in OPS:
        _check(A, B, ncols, op, 0.75, -1.5, what=f'L={L} {universe}')


@pytest.mark.parametrize('nrows', [1, 63, 64, 65, 257, 1030])
def test_row_counts(nrows):
    "one wavefront per row, four rows per workgroup, 256 rows per workgroup of the classifying kernels: every edge of those"
    rng = np.random.default_rng(nrows)
    lens = rng.integers(0, 14, (2, nrows))
    if nrows >= 63:
        lens[0][nrows // 2] = 700                                          # one row of the workgroup class in the middle
        lens[1][nrows - 1] = 300
    ncols = 1500
    rows = [[np.sort(rng.choice(ncols, n, replace=False)) for n in lens[s]] for s in (0, 1)]
    A, B = _rows_to_tuple(rows[0], seed=3), _rows_to_tuple(rows[1], seed=4)
    for op in OPS:
        _check(A, B, ncols, op, 2.0, 0.5, what=f'nrows={nrows}')


# ---- pointer widths x value types ---------------------------------------------------------------------------------------
_TYPE_CACHE = {}


def _type_case(vt):
    if 'rows' not in _TYPE_CACHE:
        rng = np.random.default_rng(7)
        lens = rng.integers(0, 90, (2, 300))
        lens[0][17], lens[1][17] = 400, 350                                # a workgroup-class row
        lens[0][200], lens[1][200] = 0, 600
        ncols = 900
        _TYPE_CACHE['rows'] = [[np.sort(rng.choice(ncols, n, replace=False)) for n in lens[s]] for s in (0, 1)]
        _TYPE_CACHE['ncols'] = ncols
    key = ('m', vt)
    if key not in _TYPE_CACHE:
        _TYPE_CACHE[key] = tuple(_rows_to_tuple(_TYPE_CACHE['rows'][s], vt[s], seed=5 + s) for s in (0, 1))
    return _TYPE_CACHE[key] + (_TYPE_CACHE['ncols'],)


def _type_ref(vt, op):
    key = ('ref', vt, op)
    if key not in _TYPE_CACHE:
        A, B, _ = _type_case(vt)
        _TYPE_CACHE[key] = combine_ref(A, B, op, 1.25, -0.3)
    return _TYPE_CACHE[key]


@pytest.mark.parametrize('pb', [np.int32, np.int64])
@pytest.mark.parametrize('pa', [np.int32, np.int64])
def test_type_matrix(pa, pb):
    for va in (np.float64, np.float32, None):
        for vb in (np.float64, np.float32, None):
            A, B, ncols = _type_case((va, vb))
            assert A[0][-1] <= 20000 and B[0][-1] <= 20000
            for op in OPS:
                rp, ci, vs = _check(A, B, ncols, op, 1.25, -0.3, ptr=(pa, pb), exp=_type_ref((va, vb), op), what=f'{pa} {pb} {va} {vb}')
                assert rp.dtype == np.int32                               # whatever the inputs' widths
                if op in ('add', 'multiply'):
                    assert vs.dtype == np.float64
                elif va is None:
                    assert vs is None
                else:
                    assert vs.dtype == va


# ---- no fused multiply-add -----------------------------------------------------------------------------------------------
def _rn(q):
    "a rational rounded to the nearest float64 (int / int true division is correctly rounded)"
    return q.numerator / q.denominator


def _fma_pairs(n, alpha, beta):
    "pairs (a, b) for which fusing either product into the add changes the sum's last bits"
    rng = np.random.default_rng(42)
    out = []
    while len(out) < n:
        a, b = float(rng.uniform(1, 2)), float(rng.uniform(1, 2))
        pa, pb = alpha * a, beta * b
        want = pa + pb
        fused_a = _rn(Fraction(alpha) * Fraction(a) + Fraction(pb))        # fma(alpha, a, round(beta b))
        fused_b = _rn(Fraction(beta) * Fraction(b) + Fraction(pa))         # fma(beta, b, round(alpha a))
        if fused_a != want and fused_b != want:
            out.append((a, b))
    return out


def test_no_fused_multiply_add():
    alpha, beta = 1.0 / 3.0, 3.0
    lim = _K().combine_limits()
    n_long = lim[2] // 2 + 40                                              # len_a + len_b above the wavefront class
    pairs = _fma_pairs(n_long, alpha, beta)
    # the assertion that keeps this test from passing vacuously: on every chosen pair both fused forms differ
    for a, b in pairs:
        want = alpha * a + beta * b
        assert _rn(Fraction(alpha) * Fraction(a) + Fraction(beta * b)) != want
        assert _rn(Fraction(beta) * Fraction(b) + Fraction(alpha * a)) != want
    av = np.array([p[0] for p in pairs])
    bv = np.array([p[1] for p in pairs])
    n_short = 20
    cols_s, cols_l = np.arange(n_short) * 3, np.arange(n_long) * 2
    rp = np.array([0, n_short, n_short + n_long], np.int64)
    A = (rp, np.concatenate([cols_s, cols_l]).astype(np.int32), np.concatenate([av[:n_short], av]))
    B = (rp, A[1].copy(), np.concatenate([bv[:n_short], bv]))
    assert 2 * n_short <= lim[0] and 2 * n_long > lim[2]
    got = _check(A, B, 3 * n_long, 'add', alpha, beta)
    assert np.array_equal(got[2][:n_short], alpha * av[:n_short] + beta * bv[:n_short])


# ---- special values ------------------------------------------------------------------------------------------------------
def _specials(dtype):
    f32 = np.array([1e-45, -1e-45, 1e-40, 3.4028235e38, -3.4028235e38, 1.17549435e-38], np.float32)
    sp = [NAN, -NAN, INF, -INF, 0.0, -0.0, 1.0, -1.0, 2.5] + [float(x) for x in f32]
    if dtype == np.float64:
        sp += [5e-324, 1.7976931348623157e308, -1.7976931348623157e308]
    v = np.array(sp, dtype)
    if dtype == np.float64:                                               # NaNs with payloads
        v.view(np.uint64)[0] = 0x7ff8000000000123
        v.view(np.uint64)[1] = 0xfff4000000000456
    else:
        v.view(np.uint32)[0] = 0x7fc00123
        v.view(np.uint32)[1] = 0xffa00456
    return v


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_special_values(dtype):
    sp = _specials(dtype)
    n = len(sp)
    # row 0: every pair (a, b) on a shared column; row 1: A alone; row 2: B alone; row 3: the pairs again, long enough for a workgroup
    pa, pb = np.repeat(sp, n), np.tile(sp, n)
    cols = np.arange(n * n) * 5
    reps = 3
    long_cols = np.arange(n * n * reps) * 2
    rp_a = np.cumsum([0, n * n, n, 0, n * n * reps])
    rp_b = np.cumsum([0, n * n, 0, n, n * n * reps])
    assert 2 * n * n * reps > _K().combine_limits()[2]
    A = (rp_a, np.concatenate([cols, np.arange(n), long_cols]).astype(np.int32), np.concatenate([pa, sp, np.tile(pa, reps)]))
    B = (rp_b, np.concatenate([cols, np.arange(n), long_cols]).astype(np.int32), np.concatenate([pb, sp, np.tile(pb, reps)]))
    ncols = int(long_cols[-1]) + 1
    for alpha in (1.0, -1.0, 0.0, INF):
        for beta in (1.0, -1.0, 0.0, INF):
            rp, ci, vs = _check(A, B, ncols, 'add', alpha, beta, what=str(dtype))
            assert rp[-1] == n * n + 2 * n + n * n * reps                 # nothing is dropped: exact zeros stay stored
    _check(A, B, ncols, 'multiply', what=str(dtype))
    # Inf - Inf and 0 * Inf are NaN, 1 - 1 is a stored +0.0
    rp, ci, vs = _run(A, B, ncols, 'add', 1.0, -1.0)
    i_inf, i_one = 2, 6
    assert np.isnan(vs[i_inf * n + i_inf]) and np.isnan(vs[(i_inf + 1) * n + i_inf + 1])
    z = vs[i_one * n + i_one]
    assert z == 0.0 and not np.signbit(z)
    rp, ci, vs = _run(A, B, ncols, 'add', 0.0, 1.0)
    assert np.isnan(vs[i_inf * n + i_one])                                 # 0 * Inf + 1
    # the masks move bits: NaN payloads, -0.0 and subnormals come back as they went in
    for op in ('keep', 'drop'):
        _check(A, B, ncols, op, what=str(dtype))
    got = _run(A, B, ncols, 'keep')
    assert raw_bits_equal(got[2][:n * n], pa)
    got = _run(A, B, ncols, 'drop')
    assert raw_bits_equal(got[2], sp)


# ---- masks on an unsorted A ----------------------------------------------------------------------------------------------
def test_masks_on_unsorted_and_repeating_a():
    rng = np.random.default_rng(9)
    ncols = 800
    lens = np.concatenate([[0, 1, 70, 300, 900, 0], rng.integers(0, 50, 120)])
    rows_a = [rng.integers(0, ncols, n) for n in lens]                     # unsorted, with repeats
    rows_b = [np.sort(rng.choice(ncols, int(rng.integers(0, 400)), replace=False)) for _ in lens]
    for dtype in (np.float64, np.float32, None):
        A, B = _rows_to_tuple(rows_a, dtype, seed=1), _rows_to_tuple(rows_b, None, seed=2)
        assert any(len(np.unique(r)) < len(r) for r in rows_a)
        for op in ('keep', 'drop'):
            _check(A, B, ncols, op, what=f'unsorted {dtype}')


def test_mask_on_a_product_in_reference_order():
    "the main caller: mult_ab's rows come in reverse order of first discovery, and stay so through drop / keep"
    from csr_amd import CSR
    from csr_amd.kernels import releasing
    K = _K()
    rng = np.random.default_rng(10)
    n = 150
    m = (rng.random((n, n)) < 0.06) * rng.integers(1, 5, (n, n))
    R = CSR.from_coo(*np.nonzero(m), m[np.nonzero(m)].astype(np.float64), shape=(n, n))
    seen = _rows_to_tuple([np.sort(rng.choice(n, int(rng.integers(0, 40)), replace=False)) for _ in range(n)], None)
    assert K.spgemm_order() == 'reference'
    with releasing(K.to_handle(R), K) as r_h, releasing(K.to_handle(_csr(seen, n)), K) as s_h:
        with releasing(K.mult_ab(r_h, r_h), K) as p_h:
            P = K.from_handle(p_h)
            assert any(np.any(np.diff(P.row_cs(i)) < 0) for i in range(n))    # really unsorted
            for op in ('keep', 'drop'):
                with releasing(K.combine(p_h, s_h, op), K) as c_h:
                    got = _tup(K.from_handle(c_h))
                exp = combine_ref(_tup(P), seen, op)
                assert same(got, exp, op), (op, first_difference(got, exp, op))


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _canonical_pair():
    rng = np.random.default_rng(12)
    lens = rng.integers(0, 20, (2, 50))
    lens[:, 31] = 10                                                       # the row _spoil edits
    rows = [[np.sort(rng.choice(60, int(n), replace=False)) for n in lens[s]] for s in (0, 1)]
    return _rows_to_tuple(rows[0], seed=1), _rows_to_tuple(rows[1], seed=2), 60


def _spoil(t, how):
    "row 31 gets two entries swapped (unsorted) or a column written twice (repeated)"
    rp, ci, vs = t[0], t[1].copy(), t[2]
    s, e = int(rp[31]), int(rp[32])
    assert e - s >= 2
    if how == 'unsorted':
        ci[s], ci[s + 1] = ci[s + 1], ci[s]
    else:
        ci[s + 1] = ci[s]
    return rp, ci, vs


@pytest.mark.parametrize('how', ['unsorted', 'repeated'])
def test_non_canonical_operands_are_refused(how):
    from csr_amd._lib import CsrkError
    A, B, ncols = _canonical_pair()
    bad_b, bad_a = _spoil(B, how), _spoil(A, how)
    for op in OPS:
        with pytest.raises(CsrkError) as ei:
            _run(A, bad_b, ncols, op)
        assert 'operand B' in str(ei.value) and 'row 31' in str(ei.value)
    for op in ('add', 'multiply'):
        with pytest.raises(CsrkError) as ei:
            _run(bad_a, B, ncols, op)
        assert 'operand A' in str(ei.value) and 'row 31' in str(ei.value)
    for op in ('keep', 'drop'):                                            # the masks take that A as it is
        _check(bad_a, B, ncols, op)
    if how == 'unsorted':                                                  # sorted, the same operands are accepted
        b, a = _csr(bad_b, ncols), _csr(bad_a, ncols)
        b.sort_rows()
        a.sort_rows()
        for op in OPS:
            got = _tup(getattr(a, METHOD[op])(b))
            exp = combine_ref(_tup(a), _tup(b), op)
            assert same(got, exp, op), (op, first_difference(got, exp, op))


def test_the_remembered_answer_is_dropped_by_order_columns():
    "one handle: refused while unsorted, accepted after order_columns on that same handle, and no handle comes back from a refusal"
    from csr_amd._lib import CsrkError
    from csr_amd.kernels import releasing
    K = _K()
    A, B, ncols = _canonical_pair()
    bad_b = _spoil(B, 'unsorted')
    with releasing(K.to_handle(_csr(A, ncols)), K) as a_h, releasing(K.to_handle(_csr(bad_b, ncols)), K) as b_h:
        for _ in range(2):                                                 # the second refusal comes from the remembered answer
            got = None
            with pytest.raises(CsrkError):
                got = K.combine(a_h, b_h, 'add')
            assert got is None
        K.order_columns(b_h)
        b_sorted = _tup(K.from_handle(b_h))                                # (the values followed their columns)
        assert np.array_equal(b_sorted[1], B[1])
        for op in OPS:
            with releasing(K.combine(a_h, b_h, op), K) as c_h:
                got = _tup(K.from_handle(c_h))
            exp = combine_ref(A, b_sorted, op)
            assert same(got, exp, op), (op, first_difference(got, exp, op))


# ---- the same handle on both sides, empty inputs, repeatability --------------------------------------------------------
def test_same_matrix_on_both_sides():
    from csr_amd.kernels import releasing
    K = _K()
    A, _, ncols = _canonical_pair()
    a = _csr(A, ncols)
    z = a.add(a, 1, -1)
    assert np.array_equal(z.rowptrs, A[0]) and np.array_equal(z.colinds, A[1]) and not z.values.any() and not np.signbit(z.values).any()
    k = a.keep_entries(a)
    assert same(_tup(k), (A[0].astype(np.int32), A[1], A[2]), 'keep')
    d = a.drop_entries(a)
    assert d.nnz == 0 and np.array_equal(d.rowptrs, np.zeros(len(A[0]), np.int32)) and d.rowptrs.dtype == np.int32
    with releasing(K.to_handle(a), K) as h:                                # and literally one handle
        for op in OPS:
            with releasing(K.combine(h, h, op, 1.0, -1.0), K) as c_h:
                got = _tup(K.from_handle(c_h))
            exp = combine_ref(A, A, op, 1.0, -1.0)
            assert same(got, exp, op), (op, first_difference(got, exp, op))


def test_empty_inputs():
    i4 = np.int32
    some = _rows_to_tuple([[1, 4], [], [0, 2, 3]], seed=1)
    none3 = (np.zeros(4, np.int64), np.zeros(0, i4), np.zeros(0))
    none0 = (np.zeros(1, np.int64), np.zeros(0, i4), np.zeros(0))
    for op in OPS:
        _check(none3, none3, 5, op, what='both empty')
        _check(none0, none0, 5, op, what='no rows')
        _check(some, none3, 5, op, what='B empty')
        _check(none3, some, 5, op, what='A empty')
        _check((none3[0], none3[1], None), some, 5, op, what='A empty, structure only')


def test_repeatable_and_inputs_untouched():
    from csr_amd.kernels import releasing
    K = _K()
    A, B, ncols = _type_case((np.float64, np.float32))
    a, b = _csr(A, ncols), _csr(B, ncols)
    x = np.random.default_rng(1).uniform(-1, 1, ncols)
    with releasing(K.to_handle(a), K) as a_h, releasing(K.to_handle(b), K) as b_h:
        ya, yb = K.mult_vec(a_h, x), K.mult_vec(b_h, x)
        for op in OPS:
            res = []
            for _ in range(2):
                with releasing(K.combine(a_h, b_h, op, 0.5, 2.0), K) as c_h:
                    res.append(_tup(K.from_handle(c_h)))
            assert same(res[0], res[1], 'keep'), op                       # all bits, NaN payloads too
        for h, t, y in ((a_h, A, ya), (b_h, B, yb)):
            back = K.from_handle(h)
            assert np.array_equal(back.rowptrs, t[0]) and np.array_equal(back.colinds, t[1]) and raw_bits_equal(back.values, t[2])
            assert np.array_equal(K.mult_vec(h, x), y)


# ---- multiply_topk(exclude=) -------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ratings():
    from csr_amd import CSR
    rng = np.random.default_rng(21)
    nr, nc = 400, 300
    pop = 1.0 / np.arange(1, nc + 1) ** 0.7
    m = (rng.random((nr, nc)) < 0.25 * pop / pop.mean() * 0.2) * rng.integers(1, 6, (nr, nc))
    r, c = np.nonzero(m)
    return CSR.from_coo(r, c, m[r, c].astype(np.float64), shape=(nr, nc))


@pytest.mark.parametrize('order', ['descending', 'storage'])
@pytest.mark.parametrize('transpose', [True, False])
def test_multiply_topk_exclude(ratings, transpose, order):
    R = ratings
    other = R if transpose else R.transpose()                              # both give the 400 x 400 user-user product
    rng = np.random.default_rng(22)
    seen = _csr(_rows_to_tuple([np.sort(rng.choice(R.nrows, int(rng.integers(0, 120)), replace=False)) for _ in range(R.nrows)], None),
                R.nrows)
    k, mv = 7, 2.0
    got = R.multiply_topk(other, k, transpose=transpose, min_value=mv, order=order, exclude=seen)
    P = R.multiply(other, transpose=transpose)
    D = combine_ref(_tup(P), _tup(seen), 'drop')
    assert 0 < D[0][-1] < P.nnz
    erp, eci, evs = topk_rows_ref(D[0], D[1], D[2], k, mv, order)
    assert np.array_equal(got.rowptrs, erp) and np.array_equal(got.colinds, eci) and raw_bits_equal(got.values, evs)
    # without exclude: the old call, array for array
    old = R.multiply_topk(other, k, transpose=transpose, min_value=mv, order=order)
    exp = P.topk_rows(k, min_value=mv, order=order)
    again = R.multiply_topk(other, k, transpose=transpose, min_value=mv, order=order, exclude=None)
    for m in (old, again):
        assert np.array_equal(m.rowptrs, exp.rowptrs) and np.array_equal(m.colinds, exp.colinds) and raw_bits_equal(m.values, exp.values)
