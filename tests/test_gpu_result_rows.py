"""
What the shared host steps of a NEW result matrix own (csrc/result.h: scan_total, write_rowptrs, write_rowptrs_through,
empty_matrix, finish_result), pinned across the five operations that use them -- csrk_combine, csrk_coalesce,
csrk_topk_rows, csrk_filter_zeros, csrk_pick_rows -- against the references the other modules use (combine_ref,
coalesce_ref, topk_ref; NumPy for filter and pick).  Row pointers, columns and values bit for bit; the result's pointer
width int32 whatever the input's (filter_zeros: the input's); every input once with int32 and once with int64 row pointers.

Two inputs: a 9 x 11 matrix with empty rows first, last and doubled in the middle, and one row of 600 entries among empty
ones, which combine and top-k hand to their workgroup kernels through a row list (the class bounds come from
csrk_combine_limits / csrk_topk_limits).

The empty results asserted elsewhere are not repeated here: nrows == 0 and nnz == 0 for top-k in
test_gpu_topk.py::test_empty_matrices, for coalesce in test_gpu_coalesce.py::test_degenerate_shapes (both widths each), and
for combine with int32 pointers in test_gpu_combine.py::test_empty_inputs.
"""
import numpy as np
import pytest

from coalesce_ref import DUPS, coalesce_ref
from coalesce_ref import same as coalesce_same
from combine_ref import OPS, combine_ref
from combine_ref import same as combine_same
from topk_ref import bits, topk_rows_ref
from topk_ref import same as topk_same

pytestmark = pytest.mark.gpu

i4, i8 = np.int32, np.int64
PTRS = pytest.mark.parametrize('ptr', [i4, i8], ids=['ptr32', 'ptr64'])
LENS = (0, 1, 0, 5, 0, 0, 3, 1, 0)
NCOLS = 11
LONG = 600                  # the one long row (above combine's wavefront class and top-k's, checked in _inputs)
LONG_ROWS, LONG_NCOLS = 5, 1500


def _K():
    from csr_amd.kernels import hip as K
    return K


def _matrix(rows, vals=None, seed=0, dtype=np.float64):
    "rows: a list of column lists -> (int64 rowptrs, colinds, values)"
    rp = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(i8)
    ci = np.concatenate([np.zeros(0, i8)] + [np.asarray(r, i8) for r in rows]).astype(i4)
    if vals is None:
        vals = np.random.default_rng(seed).uniform(-2, 2, len(ci))
    return rp, ci, np.asarray(vals).astype(dtype)


_CACHE = {}


def _inputs():
    "the inputs and their expected results, made once and never written to"
    if _CACHE:
        return _CACHE
    K = _K()
    assert LONG > K.combine_limits()[2] and K.topk_limits()[0] < LONG, (K.combine_limits(), K.topk_limits())
    rng = np.random.default_rng(11)
    small = _matrix([np.sort(rng.choice(NCOLS, n, replace=False)) for n in LENS], seed=1)
    small_b = _matrix([np.sort(rng.choice(NCOLS, n, replace=False)) for n in LENS[::-1]], seed=2)
    # the same rows with repeated columns, sorted (coalesce's route 1) and in a shuffled order (route 2)
    rep = _matrix([np.sort(rng.integers(0, 4, n)) for n in LENS], seed=3)
    shuf = (rep[0], np.concatenate([rng.permutation(rep[1][s:e]) for s, e in zip(rep[0][:-1], rep[0][1:])]).astype(i4), rep[2])
    # some exact zeros, a -0.0 and a NaN for filter_zeros
    zv = small[2].copy()
    zv[[0, 2, 3, 9]] = [0.0, -0.0, np.nan, 0.0]
    zeros = (small[0], small[1], zv)
    long_rows = [[]] * LONG_ROWS
    long_rows[2] = np.sort(rng.choice(LONG_NCOLS, LONG, replace=False))
    long_a = _matrix(long_rows, seed=4)
    long_rows[2] = np.sort(rng.choice(LONG_NCOLS, LONG, replace=False))
    long_b = _matrix(long_rows, seed=5)
    long_rows[2] = np.sort(rng.integers(0, 200, LONG))
    long_rep = _matrix(long_rows, seed=6)
    lz = long_a[2].copy()
    lz[::3] = 0.0
    _CACHE.update(small=small, small_b=small_b, rep=rep, shuf=shuf, zeros=zeros, long_a=long_a, long_b=long_b, long_rep=long_rep,
                  long_zeros=(long_a[0], long_a[1], lz))
    for v in _CACHE.values():
        for a in v:
            a.setflags(write=False)
    return _CACHE


def _csr(t, ncols, ptr):
    from csr_amd import CSR
    rp, ci, vs = t
    return CSR(len(rp) - 1, ncols, int(rp[-1]), np.ascontiguousarray(rp, dtype=ptr), np.ascontiguousarray(ci, dtype=i4),
               None if vs is None else np.ascontiguousarray(vs), _cast=False)


def _on_device(fn, ptr, ncols, *mats):
    "fn(handles...) -> a new handle; its arrays as they come back from the card"
    K = _K()
    hs, out = [], None
    try:
        for t in mats:
            hs.append(K.to_handle(_csr(t, ncols, ptr)))
        out = fn(*hs)
        c = K.from_handle(out)
        return c.rowptrs, c.colinds, c.values
    finally:
        if out is not None:
            K.release_handle(out)
        for h in hs:
            K.release_handle(h)


def _ncols(name):
    return LONG_NCOLS if name.startswith('long') else NCOLS


# ---- the five operations ------------------------------------------------------------------------------------------------------
@PTRS
@pytest.mark.parametrize('pair', [('small', 'small_b'), ('long_a', 'long_b')], ids=['small', 'long'])
def test_combine(pair, ptr):
    K, m = _K(), _inputs()
    A, B = m[pair[0]], m[pair[1]]
    for op in OPS:
        got = _on_device(lambda a, b: K.combine(a, b, op, 0.75, -1.5), ptr, _ncols(pair[0]), A, B)
        assert got[0].dtype == i4, op
        assert combine_same(got, combine_ref(A, B, op, 0.75, -1.5), op), op


@PTRS
@pytest.mark.parametrize('name', ['small', 'rep', 'shuf', 'long_rep'])
def test_coalesce(name, ptr):
    K, m = _K(), _inputs()
    for dup in DUPS:
        got = _on_device(lambda h: K.coalesce(h, dup), ptr, _ncols(name), m[name])
        assert got[0].dtype == i4, dup
        assert coalesce_same(got, coalesce_ref(m[name], dup), dup), dup


@PTRS
@pytest.mark.parametrize('name, k, min_value', [('small', 2, None),        # every row keeps min(k, length): the bounded arrays are the result
                                                ('small', 3, 0.25),        # rows keep fewer: the result is closed up
                                                ('long_a', 40, None), ('long_a', 700, 1.0)])
def test_topk_rows(name, k, min_value, ptr):
    K, m = _K(), _inputs()
    for order in ('descending', 'storage'):
        got = _on_device(lambda h: K.topk_rows(h, k, min_value, order), ptr, _ncols(name), m[name])
        assert got[0].dtype == i4, order
        exp = topk_rows_ref(*m[name], k, -np.inf if min_value is None else min_value, order)
        assert topk_same(got, exp), order


def _filter_ref(t):
    rp, ci, vs = t
    keep = vs != 0                                          # a NaN stays
    cum = np.concatenate(([0], np.cumsum(keep))).astype(i8)
    return cum[rp], ci[keep], vs[keep]


@PTRS
@pytest.mark.parametrize('name', ['zeros', 'small', 'long_zeros'])
def test_filter_zeros(name, ptr):
    K, m = _K(), _inputs()
    got = _on_device(K.filter_zeros, ptr, _ncols(name), m[name])
    assert got[0].dtype == ptr                              # the input's width, not the narrowest
    assert topk_same(got, _filter_ref(m[name]))


def _pick_ref(t, rows, values=True):
    rp, ci, vs = t
    idx = np.concatenate([np.zeros(0, i8)] + [np.arange(rp[r], rp[r + 1]) for r in rows]).astype(i8)
    orp = np.concatenate(([0], np.cumsum([rp[r + 1] - rp[r] for r in rows]))).astype(i8)
    return orp, ci[idx], vs[idx] if values else None


@PTRS
@pytest.mark.parametrize('name, rows', [('small', [3, 0, 3, 8, 6, 1, 1, 2, 7]), ('small', [8, 0]), ('long_a', [2, 4, 2, 0])])
def test_pick_rows(name, rows, ptr):
    K, m = _K(), _inputs()
    for values in (True, False):
        got = _on_device(lambda h: K.pick_rows(h, np.array(rows), values), ptr, _ncols(name), m[name])
        exp = _pick_ref(m[name], rows, values)
        assert got[0].dtype == i4
        assert np.array_equal(got[0], exp[0]) and got[1].dtype == i4 and np.array_equal(got[1], exp[1])
        if values:
            assert got[2].dtype == np.float64 and np.array_equal(bits(got[2]), bits(exp[2]))
        else:
            assert got[2] is None


# ---- empty results ------------------------------------------------------------------------------------------------------------
def _assert_empty(got, nrows, rp_dtype, val_dtype):
    rp, ci, vs = got
    assert rp.dtype == rp_dtype and rp.shape == (nrows + 1,) and not rp.any()
    assert ci.dtype == i4 and len(ci) == 0
    if val_dtype is None:
        assert vs is None
    else:
        assert vs is not None and vs.dtype == val_dtype and len(vs) == 0


def _none(nrows, dtype=np.float64):
    return np.zeros(nrows + 1, i8), np.zeros(0, i4), None if dtype is None else np.zeros(0, dtype)


@PTRS
def test_combine_empty_results(ptr):
    K, m = _K(), _inputs()
    A = m['small']
    cols_a = set(A[1].tolist())
    free = [c for c in range(NCOLS) if c not in cols_a]
    assert free                                              # columns A never uses: a pattern disjoint from A's in every row
    disjoint = _matrix([free[:1] if n else [] for n in LENS], seed=7)
    f4 = (A[0], A[1], A[2].astype(np.float32))
    for op in OPS:
        out_dtype = np.float64 if op in ('add', 'multiply') else np.float32
        if ptr == i8:                                        # (int32 pointers: test_gpu_combine.py::test_empty_inputs)
            got = _on_device(lambda a, b: K.combine(a, b, op), ptr, NCOLS, _none(0, np.float32), _none(0))
            _assert_empty(got, 0, i4, out_dtype)
            got = _on_device(lambda a, b: K.combine(a, b, op), ptr, NCOLS, _none(9, np.float32), _none(9))
            _assert_empty(got, 9, i4, out_dtype)
    got = _on_device(lambda a, b: K.combine(a, b, 'multiply'), ptr, NCOLS, A, disjoint)
    _assert_empty(got, 9, i4, np.float64)
    got = _on_device(lambda a, b: K.combine(a, b, 'keep'), ptr, NCOLS, f4, _none(9))
    _assert_empty(got, 9, i4, np.float32)
    got = _on_device(lambda a, b: K.combine(a, b, 'keep'), ptr, NCOLS, (A[0], A[1], None), disjoint)
    _assert_empty(got, 9, i4, None)


@PTRS
def test_topk_rows_empty_result(ptr):
    K, m = _K(), _inputs()
    for name in ('small', 'long_a'):
        above = float(m[name][2].max()) + 1.0
        for order in ('descending', 'storage'):
            got = _on_device(lambda h: K.topk_rows(h, 3, above, order), ptr, _ncols(name), m[name])
            _assert_empty(got, len(m[name][0]) - 1, i4, np.float64)


@PTRS
def test_filter_zeros_empty_results(ptr):
    K, m = _K(), _inputs()
    for nrows in (0, 9):
        _assert_empty(_on_device(K.filter_zeros, ptr, NCOLS, _none(nrows)), nrows, ptr, np.float64)
    A = m['small']
    all_zero = (A[0], A[1], np.where(np.arange(len(A[1])) % 2 == 0, 0.0, -0.0))
    _assert_empty(_on_device(K.filter_zeros, ptr, NCOLS, all_zero), 9, ptr, np.float64)


@PTRS
def test_pick_rows_empty_results(ptr):
    K, m = _K(), _inputs()
    A = m['small']
    none = np.zeros(0, i4)
    for values, dt in ((True, np.float64), (False, None)):
        _assert_empty(_on_device(lambda h: K.pick_rows(h, none, values), ptr, NCOLS, _none(0)), 0, i4, dt)       # no rows to pick from
        _assert_empty(_on_device(lambda h: K.pick_rows(h, np.array([4, 0, 4]), values), ptr, NCOLS, _none(9)), 3, i4, dt)      # nnz == 0
        _assert_empty(_on_device(lambda h: K.pick_rows(h, none, values), ptr, NCOLS, A), 0, i4, dt)               # no rows picked
        _assert_empty(_on_device(lambda h: K.pick_rows(h, np.array([0, 4, 5, 8, 2, 4]), values), ptr, NCOLS, A), 6, i4, dt)    # only empty rows
