#!/usr/bin/env python3
"""
Generate tests/golden/*.npz by running the REFERENCE's own code.

Container-only tool: it imports lenskit/csr from /root/reference in the reference's
NUMBA_DISABLE_JIT mode (csr/csr.py:20-43) with the stand-in `numba` package in
oracle/gen/numba_stub (real Numba is not installable in this image),
feeds it seeded inputs, and stores inputs + the reference's outputs.  The fixtures are
data only; neither this script nor the fixtures contain reference source.  Nothing on the
GPU box needs /root/reference: tests read the committed .npz files.

Run:  python oracle/gen/gen_golden.py              (writes every fixture under tests/golden/)
      python oracle/gen/gen_golden.py special ...  (writes only the fixtures named, e.g. special.npz)

Input distributions restate csr/test_utils.py:30-101 (`csrs`, `mm_pairs`): shapes 1..80
(mm: 1..100), density <= 0.5, unique COO coordinates, values in +-1e3 of dtype f4/f8 with
exact zeros dropped, or structure-only.
"""
import os
import sys

os.environ['PYTHONDONTWRITEBYTECODE'] = '1'
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('CSR_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(HERE, 'numba_stub'))

import numpy as np  # noqa: E402

import csr  # noqa: E402
from csr import CSR  # noqa: E402
from csr.kernels import get_kernel  # noqa: E402

assert csr.__file__.startswith(REF), csr.__file__
K = get_kernel()
assert K.__name__ == 'csr.kernels.numba', K.__name__

OUT = os.path.join(ROOT, 'tests', 'golden')
os.makedirs(OUT, exist_ok=True)


def draw_csr(rng, nrows=None, ncols=None, values=None, dtype=None, max_density=0.5, max_dim=80):
    "restates csr/test_utils.py:30-74"
    if nrows is None:
        nrows = int(rng.integers(1, max_dim + 1))
    if ncols is None:
        ncols = int(rng.integers(1, max_dim + 1))
    nnz_ub = int(np.ceil(nrows * ncols * max_density))
    nnz = int(rng.integers(0, nnz_ub + 1))
    coords = rng.choice(nrows * ncols, size=nnz, replace=False).astype(np.int32)
    rows = np.mod(coords, nrows).astype(np.int32)
    cols = np.floor_divide(coords, nrows).astype(np.int32)
    if dtype is None:
        dtype = rng.choice(['f4', 'f8'])
    dtype = np.dtype(dtype)
    if values is None:
        values = bool(rng.integers(0, 2))
    if values:
        vals = rng.uniform(-1.0e3, 1.0e3, size=nnz).astype(dtype)
        # sprinkle exact zeros (they must be dropped) and tiny magnitudes
        if nnz > 3:
            vals[rng.integers(0, nnz)] = 0.0
            vals[rng.integers(0, nnz)] *= dtype.type(1e-30)
        nz = vals != 0.0
        rows, cols, vals = rows[nz], cols[nz], vals[nz]
    else:
        vals = None
    return CSR.from_coo(rows, cols, vals, (nrows, ncols))


def put(d, prefix, m):
    d[prefix + 'shape'] = np.array([m.nrows, m.ncols, m.nnz], dtype=np.int64)
    d[prefix + 'rowptrs'] = np.asarray(m.rowptrs).copy()
    d[prefix + 'colinds'] = np.asarray(m.colinds).copy()
    if m.values is not None:
        d[prefix + 'values'] = np.asarray(m.values).copy()


def gen_kat():
    "fixed known-answer cases from the reference tests"
    d = {}
    rows = np.array([0, 0, 1, 3], dtype=np.int32)
    cols = np.array([1, 2, 0, 1], dtype=np.int32)
    vals = np.arange(4, dtype=np.float64)
    m = CSR.from_coo(rows, cols, vals)          # tests/test_transpose.py:11-27
    put(d, 'a_', m)
    put(d, 'at_', m.transpose())
    put(d, 'ats_', m.transpose(False))
    d['a_extents'] = np.array([m.row_extent(i) for i in range(m.nrows)], dtype=np.int64)  # test_attributes.py:36-45
    d['a_row_nnzs'] = m.row_nnzs()
    d['a_mv_ones'] = m.mult_vec(np.ones(m.ncols))
    np.savez_compressed(os.path.join(OUT, 'kat.npz'), **d)


def gen_spmv(n=60):
    rng = np.random.default_rng(20261003)
    d = {'n': np.array(n)}
    for c in range(n):
        m = draw_csr(rng)
        x = rng.uniform(-1.0e3, 1.0e3, size=m.ncols)
        if c % 7 == 0:
            x = x.astype(np.float32)
        put(d, f'c{c}_', m)
        d[f'c{c}_x'] = x
        with np.errstate(all='ignore'):
            d[f'c{c}_y'] = m.mult_vec(x)
        # sharded path (csr/csr.py:584-590) with a tiny max_nnz, when every row fits
        lim = 40
        if m.nnz > lim and int(np.max(m.row_nnzs())) <= lim:
            shards = m._shard_rows(lim)
            d[f'c{c}_shard_rows'] = np.array([s.nrows for s in shards], dtype=np.int64)
            d[f'c{c}_y_sharded'] = np.concatenate([K.mult_vec(K.to_handle(s), x) for s in shards])
    np.savez_compressed(os.path.join(OUT, 'spmv.npz'), **d)


def gen_cfg1():
    "BASELINE.json configs[0]: 10k x 10k, nnz = 1e5, fp64 (SURVEY.md section 8d row 1)"
    rng = np.random.default_rng(20261003)
    n, nnz = 10000, 100000
    coords = rng.choice(n * n, size=nnz, replace=False)
    coords.sort()
    rows = (coords // n).astype(np.int32)
    cols = (coords % n).astype(np.int32)
    vals = rng.standard_normal(nnz)
    x = rng.standard_normal(n)
    m = CSR.from_coo(rows, cols, vals, (n, n))
    d = {}
    put(d, 'a_', m)
    d['x'] = x
    d['y'] = m.mult_vec(x)
    np.savez_compressed(os.path.join(OUT, 'cfg1_spmv.npz'), **d)


def gen_transpose(n=40):
    rng = np.random.default_rng(77001)
    d = {'n': np.array(n)}
    for c in range(n):
        m = draw_csr(rng)
        if c >= n - 6:
            # duplicate (i, j) entries and unsorted rows: build the struct directly so the
            # stable-scatter order (structure.py:191-197) is observable
            nr, nc = int(rng.integers(2, 20)), int(rng.integers(2, 12))
            lens = rng.integers(0, 9, size=nr)
            rp = np.zeros(nr + 1, dtype=np.int32)
            rp[1:] = np.cumsum(lens)
            ci = rng.integers(0, nc, size=int(rp[-1])).astype(np.int32)   # dups, unsorted
            vs = rng.uniform(-5, 5, size=int(rp[-1]))
            m = CSR(nr, nc, int(rp[-1]), rp, ci, vs)
        put(d, f'c{c}_', m)
        t = m.transpose()
        put(d, f'c{c}_t_', t)
        ts = m.transpose(False)
        put(d, f'c{c}_ts_', ts)
        assert ts.values is None
        d[f'c{c}_row_nnzs'] = m.row_nnzs()
    np.savez_compressed(os.path.join(OUT, 'transpose.npz'), **d)


def gen_rows(n=40):
    "unit_rows / center_rows (csr/transform.py)"
    rng = np.random.default_rng(424242)
    d = {'n': np.array(n)}
    for c in range(n):
        m = draw_csr(rng, values=True)
        if c == n - 1:      # all-zero row, subnormal-scale row, huge row, empty row (f8)
            rp = np.array([0, 3, 3, 6, 9, 10], dtype=np.int32)
            ci = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 1], dtype=np.int32)
            vs = np.array([0.0, 0.0, 0.0, 1e-200, -3e-200, 2e-200, 1e300, -1e300, 5e299, 5e-324])
            m = CSR(5, 3, 10, rp, ci, vs)
        if c == n - 2:      # same idea in f4
            rp = np.array([0, 2, 2, 5, 7], dtype=np.int32)
            ci = np.array([0, 1, 0, 1, 2, 0, 2], dtype=np.int32)
            vs = np.array([0.0, 0.0, 1e-30, -3e-30, 2e-30, 3e38, -1e38], dtype=np.float32)
            m = CSR(4, 3, 7, rp, ci, vs)
        put(d, f'c{c}_', m)
        u = m.copy()
        with np.errstate(all='ignore'):
            d[f'c{c}_unit_norms'] = u.normalize_rows('unit')
        d[f'c{c}_unit_values'] = np.asarray(u.values).copy()
        z = m.copy()
        with np.errstate(all='ignore'):
            d[f'c{c}_center_means'] = z.normalize_rows('center')
        d[f'c{c}_center_values'] = np.asarray(z.values).copy()
    np.savez_compressed(os.path.join(OUT, 'rows.npz'), **d)


def gen_spgemm(n=24):
    "mult_ab / mult_abt (csr/kernels/numba/multiply.py) and CSR.multiply (csr/csr.py:524-567)"
    rng = np.random.default_rng(9001)
    d = {'n': np.array(n)}
    for c in range(n):
        r, mid, k = (int(rng.integers(1, 101)) for _ in range(3))
        dt = rng.choice(['f4', 'f8'])
        A = draw_csr(rng, r, mid, values=True, dtype=dt)
        B = draw_csr(rng, mid, k, values=True, dtype=dt)
        put(d, f'c{c}_a_', A)
        put(d, f'c{c}_b_', B)
        raw = K.mult_ab(K.to_handle(A), K.to_handle(B))      # explicit zeros kept, reference order
        put(d, f'c{c}_raw_', raw)
        put(d, f'c{c}_ab_', A.multiply(B))                   # after _filter_zeros
        Bt = B.transpose()                                    # k x mid
        put(d, f'c{c}_bt_', Bt)
        put(d, f'c{c}_abt_', A.multiply(Bt, transpose=True))
        # order_columns / sort_rows on the raw product (unsorted rows)
        s = CSR(raw.nrows, raw.ncols, raw.nnz, raw.rowptrs.copy(), raw.colinds.copy(), raw.values.copy())
        s.sort_rows()
        put(d, f'c{c}_rawsorted_', s)
    np.savez_compressed(os.path.join(OUT, 'spgemm.npz'), **d)


def gen_shard(n=20):
    "_shard_rows / _assemble_shards (csr/csr.py:599-650; tests/test_transform.py:172-197)"
    rng = np.random.default_rng(5150)
    d = {'n': np.array(n)}
    for c in range(n):
        m = draw_csr(rng, int(rng.integers(10, 101)), int(rng.integers(10, 101)), values=True, max_dim=100)
        put(d, f'c{c}_', m)
        shards = m._shard_rows(500)
        d[f'c{c}_shard_rows'] = np.array([s.nrows for s in shards], dtype=np.int64)
        d[f'c{c}_shard_nnz'] = np.array([s.nnz for s in shards], dtype=np.int64)
        back = CSR._assemble_shards(shards)
        d[f'c{c}_assembled_rowptrs'] = np.asarray(back.rowptrs).copy()
    # the error case: a row larger than the target
    rp = np.array([0, 600, 700], dtype=np.int32)
    m = CSR(2, 1000, 700, rp, np.arange(700, dtype=np.int32) % 1000, np.ones(700))
    try:
        m._shard_rows(500)
        d['big_row_error'] = np.array(0)
    except ValueError:
        d['big_row_error'] = np.array(1)
    np.savez_compressed(os.path.join(OUT, 'shard.npz'), **d)


def gen_pick(n=40):
    "pick_rows (csr/csr.py:347-364, csr/structure.py:84-149); draws as tests/test_transform.py:38-62"
    rng = np.random.default_rng(20261003)
    d = {'n': np.array(n)}
    for c in range(n):
        m = draw_csr(rng)
        include = bool(rng.integers(0, 2))
        k = int(rng.integers(0, m.nrows * 10 + 1))
        rows = rng.integers(0, m.nrows, size=k).astype(np.int32)
        if c == 0:
            rows = np.zeros(0, dtype=np.int32)          # nothing picked
        put(d, f'c{c}_', m)
        d[f'c{c}_rows'] = rows
        d[f'c{c}_include'] = np.array(include)
        sub = m.pick_rows(rows, include_values=include)
        assert sub.nrows == len(rows)
        put(d, f'c{c}_out_', sub)
    np.savez_compressed(os.path.join(OUT, 'pick.npz'), **d)


def gen_coo(n=36):
    """
    CSR.from_coo (csr/csr.py:138-169 -> csr/structure.py:11-67): the COO INPUTS and the reference's CSR.  Unlike
    draw_csr's unique coordinates these draws repeat (i, j) pairs and come in arbitrary order, so the stable
    counting sort's order (entries of a row keep their input order, structure.py:24-31 / :49-56) is observable.
    """
    rng = np.random.default_rng(60061)
    d = {'n': np.array(n)}
    for c in range(n):
        nrows, ncols = int(rng.integers(1, 81)), int(rng.integers(1, 81))
        nnz = int(rng.integers(0, 4 * max(nrows, ncols) + 1))
        if c == 0:
            nnz = 0                                           # nothing at all
        if c == 1:
            nrows, nnz = 1, 17                                # every entry in one row
        rows = rng.integers(0, nrows, size=nnz).astype(np.int32)          # duplicates, unsorted
        cols = rng.integers(0, ncols, size=nnz).astype(np.int32)
        if c % 5 == 2 and nnz:                                # sorted by row already, columns descending
            o = np.lexsort((-cols, rows))
            rows, cols = rows[o], cols[o]
        kind = c % 3                                          # f8 / f4 / structure only
        vals = None if kind == 2 else rng.uniform(-1.0e3, 1.0e3, size=nnz).astype('f8' if kind == 0 else 'f4')
        shape = None if (c % 7 == 3 and nnz) else (nrows, ncols)         # inferred shape (csr.py:160-161)
        m = CSR.from_coo(rows, cols, vals, shape)
        d[f'c{c}_rows'], d[f'c{c}_cols'] = rows, cols
        if vals is not None:
            d[f'c{c}_vals'] = vals
        d[f'c{c}_shape_given'] = np.array(shape is not None)
        put(d, f'c{c}_out_', m)
    np.savez_compressed(os.path.join(OUT, 'coo.npz'), **d)


def gen_spmm_dense(n=12):
    """
    The dense-panel product of BASELINE.json configs[2] through the reference's own entry point: B [ncols x k] handed to
    K.mult_ab as a fully populated CSR (csr/kernels/numba/multiply.py:13-38; numeric recurrence :110-122), the raw
    product (explicit zeros kept) densified AND as the reference returns it (raw rowptrs / colinds / values: k entries per
    row of C whose row of A holds an entry, columns in reverse order of first discovery, multiply.py:79-82, 94-97).
    k in {1, 7, 64}.  Cases n and n + 1 (appended: the first n keep their inputs): the rows of B in a shuffled column
    order -- a dense B that is not the row-major panel -- and an A with whole blocks of empty rows.
    """
    rng = np.random.default_rng(64064)
    d = {'n': np.array(n + 2)}
    for c in range(n + 2):
        k = (1, 7, 64)[c % 3] if c < n else (7, 64)[c - n]
        A = draw_csr(rng, values=True, dtype='f4' if c % 4 == 3 else 'f8')
        if c == n + 1:                                        # rows 3 .. 3 + a third of them emptied
            keep = np.ones(A.nrows, dtype=bool)
            keep[3:3 + A.nrows // 3] = False
            rows = np.repeat(np.arange(A.nrows), np.diff(A.rowptrs))
            m = keep[rows]
            A = CSR.from_coo(rows[m].astype(np.int32), A.colinds[m].copy(), A.values[m].copy(), (A.nrows, A.ncols))
        B = rng.uniform(-1.0, 1.0, size=(A.ncols, k))
        if c == 5:
            B[rng.integers(0, A.ncols), :] = 0.0              # a zero row of B: explicit zeros in the product
        cols = np.tile(np.arange(k, dtype=np.int32), A.ncols)
        vals = B.reshape(-1).copy()
        if c == n:                                            # every row of B in its own column order
            for j in range(A.ncols):
                o = rng.permutation(k)
                cols[j * k:(j + 1) * k] = o
                vals[j * k:(j + 1) * k] = B[j, o]
        Bc = CSR(A.ncols, k, A.ncols * k, np.arange(A.ncols + 1, dtype=np.int32) * k, cols, vals)
        raw = K.mult_ab(K.to_handle(A), K.to_handle(Bc))
        Cd = np.zeros((A.nrows, k))
        rp, ci, vs = np.asarray(raw.rowptrs), np.asarray(raw.colinds), np.asarray(raw.values)
        for i in range(A.nrows):
            Cd[i, ci[rp[i]:rp[i + 1]]] = vs[rp[i]:rp[i + 1]]
        put(d, f'c{c}_a_', A)
        d[f'c{c}_B'] = B
        d[f'c{c}_b_colinds'] = cols
        d[f'c{c}_b_values'] = vals
        d[f'c{c}_C'] = Cd
        d[f'c{c}_raw_nnz'] = np.array(raw.nnz)
        d[f'c{c}_raw_rowptrs'], d[f'c{c}_raw_colinds'], d[f'c{c}_raw_values'] = rp.copy(), ci.copy(), vs.copy()
    np.savez_compressed(os.path.join(OUT, 'spmm_dense.npz'), **d)


def save_stable(path, d):
    """
    np.savez_compressed with fixed zip member timestamps: the same arrays give the same bytes on every run (numpy stamps
    members with the current time).
    """
    import io
    import zipfile
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as z:
        for k, a in d.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def _special_x(rng, ncols):
    """
    x for the special-value cases: finite values in +-4 and, at disjoint columns, NaN, +Inf, -Inf, +0.0, -0.0, exact ones,
    +-1e25 (float32 products with 1e20 overflow, float64 ones do not) and +-1e-20 / 1e-160 (subnormal products).
    Returns x and a dict kind -> columns.
    """
    x = rng.uniform(-4.0, 4.0, size=ncols)
    kinds = ('nan', 'pinf', 'ninf', 'pz', 'nz', 'one', 'huge', 'tiny32', 'tiny64')
    cols = rng.permutation(ncols)[:4 * len(kinds)].reshape(len(kinds), 4)
    at = dict(zip(kinds, (np.sort(c) for c in cols)))
    x[at['nan']] = np.nan
    x[at['pinf']] = np.inf
    x[at['ninf']] = -np.inf
    x[at['pz']] = 0.0
    x[at['nz']] = -0.0
    x[at['one']] = 1.0
    x[at['huge']] = [1e25, -1e25, 1e25, 3e25]
    x[at['tiny32']] = [1e-20, -1e-20, 3e-21, 1e-19]
    x[at['tiny64']] = [1e-160, -1e-160, 3e-161, 1e-159]
    return x, at


def _special_rows(rng, nrows, ncols, at, dt):
    """
    One CSR (row by row, struct built directly: nothing filtered) whose rows cycle through the patterns the kernels get
    wrong: random rows with NaN / +-Inf / +-0.0 values, one-entry rows whose product is -0.0, long rows whose products are
    all -0.0, exact cancellation, +Inf and -Inf in one row, explicit +-0.0 values against non-finite x, float32-overflowing
    and subnormal products, empty rows.
    """
    f4 = dt == 'f4'
    rows_c, rows_v = [], []
    for i in range(nrows):
        kind = i % 11
        if kind == 0 or kind == 10:                 # random row, a few special values
            n = int(rng.integers(1, max(2, ncols // 6)))
            c = rng.choice(ncols, size=n, replace=False)
            v = rng.uniform(-4.0, 4.0, size=n)
            r = rng.random(n)
            v[r < 0.08] = np.nan
            v[(r >= 0.08) & (r < 0.14)] = np.inf
            v[(r >= 0.14) & (r < 0.20)] = -np.inf
            v[(r >= 0.20) & (r < 0.26)] = 0.0
            v[(r >= 0.26) & (r < 0.32)] = -0.0
        elif kind == 1:                             # one entry, product -0.0
            if rng.random() < 0.5:
                c, v = [rng.choice(at['pz'])], [-float(rng.uniform(0.5, 3))]
            else:
                c, v = [rng.choice(at['nz'])], [float(rng.uniform(0.5, 3))]
        elif kind == 2:                             # long row, every product -0.0
            n = int(rng.integers(8, 40))
            c = rng.choice(np.concatenate([at['pz'], at['nz']]), size=n)
            v = rng.uniform(0.5, 3.0, size=n)
            v = np.where(np.isin(c, at['pz']), -v, v)
            v[::5] = np.where(np.isin(c[::5], at['pz']), -0.0, 0.0)   # explicit zeros of the right sign too
        elif kind == 3:                             # exact cancellation on x == 1
            c = rng.choice(at['one'], size=4)
            v = np.array([3.0, -5.0, 2.0, 0.0]) * float(rng.choice([1, 0.25, 8]))
        elif kind == 4:                             # +Inf and -Inf products in one row
            c = [rng.choice(at['pinf']), rng.choice(at['ninf']), rng.choice(at['one'])]
            v = [float(rng.uniform(0.5, 2)), float(rng.uniform(0.5, 2)), 1.5]
        elif kind == 5:                             # explicit +-0.0 against NaN / +-Inf x
            c = [rng.choice(at['nan' if i % 3 == 0 else 'pinf' if i % 3 == 1 else 'ninf'])]
            v = [0.0 if rng.random() < 0.5 else -0.0]
        elif kind == 6:                             # non-finite values against finite x
            c = rng.choice(at['one'], size=2, replace=False)
            v = [(np.nan, np.inf, -np.inf)[i % 3], 1.0]
        elif kind == 7:                             # empty
            c, v = [], []
        elif kind == 8:                             # float32 overflow: 1e20 * 1e25 (float64: 1e45)
            c = [rng.choice(at['huge'])]
            v = [1e20 if f4 else 1e120]
        else:                                       # subnormal products
            if f4:
                c, v = [rng.choice(at['tiny32'])], [float(rng.choice([1e-20, -3e-19, 7e-21]))]
            else:
                c, v = [rng.choice(at['tiny64'])], [float(rng.choice([1e-160, -3e-159, 7e-161]))]
        rows_c.append(np.asarray(c, dtype=np.int32))
        rows_v.append(np.asarray(v, dtype=np.float64))
    rp = np.zeros(nrows + 1, dtype=np.int32)
    rp[1:] = np.cumsum([len(c) for c in rows_c])
    ci = np.concatenate(rows_c).astype(np.int32) if nrows else np.zeros(0, np.int32)
    vs = np.concatenate(rows_v) if nrows else np.zeros(0)
    if dt is not None:
        with np.errstate(all='ignore'):
            vs = vs.astype(dt)
    return CSR(nrows, ncols, int(rp[-1]), rp, ci, None if dt is None else vs)


def _special_mm(rng, r, mid, k, dta, dtb):
    """
    A [r x mid] and B [mid x k] for the sparse products: random sparse rows with NaN / +-Inf / +-0.0 values in both,
    and planted rows -- in A, rows that pick up a B row of -0.0 values (all products -0.0), two B rows that cancel
    exactly, +Inf and -Inf rows of B, one-entry rows against a subnormal or float32-overflowing row of B.
    """
    def rnd(nr, nc, dens):
        rows_c, rows_v = [], []
        for _ in range(nr):
            n = int(rng.binomial(nc, dens))
            c = np.sort(rng.choice(nc, size=n, replace=False))
            v = rng.uniform(-4.0, 4.0, size=n)
            q = rng.random(n)
            v[q < 0.03] = np.nan
            v[(q >= 0.03) & (q < 0.06)] = np.inf
            v[(q >= 0.06) & (q < 0.09)] = -np.inf
            v[(q >= 0.09) & (q < 0.13)] = 0.0
            v[(q >= 0.13) & (q < 0.17)] = -0.0
            rows_c.append(c.astype(np.int32))
            rows_v.append(v)
        return rows_c, rows_v

    ac, av = rnd(r, mid, 0.12)
    bc, bv = rnd(mid, k, 0.2)
    # B rows 0..5 are planted: 0 all -0.0 / +0.0 mixed so that (+a) * row = -0.0 products, 1 and 2 equal (cancellation),
    # 3 all +Inf, 4 all -Inf, 5 tiny (subnormal products with tiny A values) / huge (float32 overflow)
    f4 = dta == 'f4' and dtb == 'f4'
    full = np.sort(rng.choice(k, size=max(1, k // 3), replace=False)).astype(np.int32)
    bc[0], bv[0] = full, -np.zeros(len(full))
    bc[1], bv[1] = full, rng.integers(-3, 4, size=len(full)).astype(np.float64)
    bc[2], bv[2] = full.copy(), bv[1].copy()
    bc[3], bv[3] = full, np.full(len(full), np.inf)
    bc[4], bv[4] = full, np.full(len(full), -np.inf)
    bc[5], bv[5] = full, np.full(len(full), 1e-20 if f4 else 1e-160) * rng.choice([1.0, -3.0], size=len(full))
    for i in range(r):
        kind = i % 7
        if kind == 1:
            ac[i], av[i] = np.array([0], np.int32), np.array([2.5])             # every product -0.0
        elif kind == 2:
            ac[i], av[i] = np.array([1, 2], np.int32), np.array([1.5, -1.5])    # exact cancellation
        elif kind == 3:
            ac[i], av[i] = np.array([3, 4], np.int32), np.array([1.0, 2.0])     # +Inf + -Inf
        elif kind == 4:
            ac[i], av[i] = np.array([5], np.int32), np.array([1e-20 if f4 else 1e-160])   # subnormal products
        elif kind == 5 and f4:
            ac[i], av[i] = np.array([6], np.int32), np.array([1e20])            # float32 overflow against B row 6
    if f4:
        bc[6], bv[6] = full, np.full(len(full), 1e25)

    def build(nr, nc, cs, vs, dt):
        rp = np.zeros(nr + 1, dtype=np.int32)
        rp[1:] = np.cumsum([len(c) for c in cs])
        with np.errstate(all='ignore'):
            v = np.concatenate(vs).astype(dt)
        return CSR(nr, nc, int(rp[-1]), rp, np.concatenate(cs).astype(np.int32), v)
    return build(r, mid, ac, av, dta), build(mid, k, bc, bv, dtb)


def _nan_payloads(rng, n):
    "quiet NaNs of both signs with distinct payloads, as float64"
    bits = (np.uint64(0x7ff8000000000000) | rng.integers(1, 1 << 40, size=n).astype(np.uint64))
    bits[rng.random(n) < 0.5] |= np.uint64(1 << 63)
    return bits.view(np.float64)


def gen_special():
    """
    NaN, +-Inf, signed zeros and the float32 range through the reference (tests/test_oracle_golden.py pins the oracle on
    it; tests/test_gpu_special_values.py feeds the library the same inputs).  Cases:
      mv{c}   mult_vec with float64 and float32 x; values f8 / f4 / structure only
      mm{c}   mult_ab and mult_abt as raw kernel arrays (explicit zeros kept), CSR.multiply (zeros filtered)
      dn{c}   mult_ab with a fully populated B (the dense route's input), raw arrays
      dm{c}   data movement on float64 values holding NaNs with distinct payloads and -0.0: transpose, sort_rows,
              pick_rows, _filter_zeros, from_coo
    """
    rng = np.random.default_rng(20261016)
    d = {}
    n_mv = 9
    d['n_mv'] = np.array(n_mv)
    for c in range(n_mv):
        dt = ('f8', 'f4', None)[c % 3]
        nrows, ncols = int(rng.integers(40, 101)), int(rng.integers(40, 101))
        x, at = _special_x(rng, ncols)
        m = _special_rows(rng, nrows, ncols, at, dt)
        put(d, f'mv{c}_', m)
        d[f'mv{c}_x64'] = x
        with np.errstate(all='ignore'):
            x32 = x.astype(np.float32)
            d[f'mv{c}_x32'] = x32
            d[f'mv{c}_y64'] = K.mult_vec(K.to_handle(m), x)
            d[f'mv{c}_y32'] = K.mult_vec(K.to_handle(m), x32)
    n_mm = 6
    d['n_mm'] = np.array(n_mm)
    for c in range(n_mm):
        dta, dtb = (('f8', 'f8'), ('f4', 'f4'), ('f4', 'f8'))[c % 3]
        r, mid, k = int(rng.integers(20, 61)), int(rng.integers(10, 61)), int(rng.integers(8, 61))
        A, B = _special_mm(rng, r, mid, k, dta, dtb)
        put(d, f'mm{c}_a_', A)
        put(d, f'mm{c}_b_', B)
        with np.errstate(all='ignore'):
            put(d, f'mm{c}_raw_', K.mult_ab(K.to_handle(A), K.to_handle(B)))
            Bt = B.transpose()
            if dtb == 'f4':                           # keep B^T float32 (transpose() widens)
                Bt = CSR(Bt.nrows, Bt.ncols, Bt.nnz, Bt.rowptrs, Bt.colinds, Bt.values.astype(np.float32))
            put(d, f'mm{c}_bt_', Bt)
            put(d, f'mm{c}_rawt_', K.mult_abt(K.to_handle(A), K.to_handle(Bt)))
            put(d, f'mm{c}_ab_', A.multiply(B))
    n_dn = 3
    d['n_dn'] = np.array(n_dn)
    for c in range(n_dn):
        k = (1, 7, 64)[c]
        dt = ('f8', 'f4', 'f8')[c]
        nrows, ncols = int(rng.integers(40, 61)), int(rng.integers(40, 61))
        x, at = _special_x(rng, ncols)
        A = _special_rows(rng, nrows, ncols, at, dt)
        # the panel: row j of B is x[j] times a random positive factor in each column (so the rows' classes follow x)
        B = x[:, None] * rng.uniform(0.5, 2.0, size=(ncols, k))
        B[at['tiny32'] if dt == 'f4' else at['tiny64'], :] = x[at['tiny32'] if dt == 'f4' else at['tiny64'], None]
        Bc = CSR(ncols, k, ncols * k, np.arange(ncols + 1, dtype=np.int32) * k,
                 np.tile(np.arange(k, dtype=np.int32), ncols), B.reshape(-1).copy())
        put(d, f'dn{c}_a_', A)
        d[f'dn{c}_B'] = B
        with np.errstate(all='ignore'):
            put(d, f'dn{c}_raw_', K.mult_ab(K.to_handle(A), K.to_handle(Bc)))
    n_dm = 4
    d['n_dm'] = np.array(n_dm)
    for c in range(n_dm):
        nrows, ncols = int(rng.integers(10, 101)), int(rng.integers(10, 101))
        nnz = int(rng.integers(nrows, 4 * nrows + 1))
        rows = rng.integers(0, nrows, size=nnz).astype(np.int32)
        cols = rng.integers(0, ncols, size=nnz).astype(np.int32)      # duplicates, unsorted
        vals = rng.uniform(-4.0, 4.0, size=nnz)
        q = rng.random(nnz)
        vals[q < 0.2] = _nan_payloads(rng, int(np.sum(q < 0.2)))
        vals[(q >= 0.2) & (q < 0.3)] = -0.0
        vals[(q >= 0.3) & (q < 0.35)] = 0.0
        vals[(q >= 0.35) & (q < 0.4)] = np.inf
        vals[(q >= 0.4) & (q < 0.45)] = -np.inf
        d[f'dm{c}_coo_rows'], d[f'dm{c}_coo_cols'], d[f'dm{c}_coo_vals'] = rows, cols, vals
        m = CSR.from_coo(rows, cols, vals.copy(), (nrows, ncols))
        put(d, f'dm{c}_', m)
        put(d, f'dm{c}_t_', m.transpose())
        s = CSR(m.nrows, m.ncols, m.nnz, m.rowptrs.copy(), m.colinds.copy(), m.values.copy())
        s.sort_rows()
        put(d, f'dm{c}_sorted_', s)
        pick = rng.integers(0, nrows, size=int(rng.integers(1, 2 * nrows))).astype(np.int32)
        d[f'dm{c}_pick_rows'] = pick
        put(d, f'dm{c}_pick_', m.pick_rows(pick))
        f = CSR(m.nrows, m.ncols, m.nnz, m.rowptrs.copy(), m.colinds.copy(), m.values.copy())
        f._filter_zeros()
        put(d, f'dm{c}_fz_', f)
    save_stable(os.path.join(OUT, 'special.npz'), d)


GENERATORS = {'kat': gen_kat, 'spmv': gen_spmv, 'cfg1_spmv': gen_cfg1, 'transpose': gen_transpose, 'rows': gen_rows,
              'spgemm': gen_spgemm, 'shard': gen_shard, 'pick': gen_pick, 'coo': gen_coo, 'spmm_dense': gen_spmm_dense,
              'special': gen_special}


if __name__ == '__main__':
    names = sys.argv[1:] or list(GENERATORS)
    unknown = [n for n in names if n not in GENERATORS]
    if unknown:
        sys.exit(f'unknown fixture(s) {unknown}; known: {sorted(GENERATORS)}')
    for name in names:
        GENERATORS[name]()
        f = name + '.npz'
        print(f, os.path.getsize(os.path.join(OUT, f)))
