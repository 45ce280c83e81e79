"""
Host-side CSR container: the struct the reference keeps in csr/csr.py:46-100
(nrows, ncols, nnz, rowptrs, colinds, values) with the methods that sit on the
`csr.kernels` hot path.  The arrays live in NumPy on the host exactly as in the
reference; every arithmetic method hands them to the active kernel (csr_amd.kernels.hip by
default), which runs hand-written HIP kernels on the MI355X.  Only index bookkeeping that
the reference itself does in NumPy on the host (subset_rows views, shard split points,
shard reassembly) is done here.

Layout rules kept verbatim (csr/csr.py:79-100): rowptrs int32 when nnz <= INT32_MAX else
int64; colinds int32; values any float dtype or None; all C-contiguous.
"""
import logging
import sys
import weakref

import numpy as np

from .kernels import get_kernel, releasing

INTC = np.iinfo(np.intc)
_log = logging.getLogger(__name__)


def _topk_check(K, k, min_value, order):
    "argument errors of topk_rows / multiply_topk, raised before any device work (the kernel's own checker when it has one)"
    chk = getattr(K, 'topk_args', None)
    if chk is not None:
        chk(k, min_value, order)


def _coalesce_check(K, duplicates):
    "the argument error of coalesce / from_coo(duplicates=), raised before any device work"
    chk = getattr(K, 'coalesce_args', None)
    if chk is not None:
        chk(duplicates)
    elif duplicates not in ('sum', 'first', 'last', 'max', 'min'):
        raise ValueError(f"duplicates must be 'sum', 'first', 'last', 'max' or 'min', not {duplicates!r}")


class CSR:
    """
    Compressed sparse row matrix (host arrays), drop-in for the reference's `csr.CSR` on the
    kernel hot path.

    Attributes: nrows, ncols, nnz, rowptrs, colinds, values (None = structure only).
    """

    def __init__(self, nrows, ncols, nnz, rps, cis, vs, _cast=True):
        # csr/csr.py:79-100
        assert nrows >= 0 and nrows <= INTC.max
        assert ncols >= 0 and ncols <= INTC.max
        assert nnz >= 0
        self.nrows = int(nrows)
        self.ncols = int(ncols)
        self.nnz = int(nnz)
        if _cast:
            cis = np.require(cis, np.intc, 'C')
            if nnz <= INTC.max:
                rps = np.require(rps, np.intc, 'C')
            else:
                rps = np.require(rps, np.int64, 'C')
            if vs is not None:
                vs = np.require(vs, requirements='C')
        self.rowptrs = rps
        self.colinds = cis
        self._values = vs

    # While a device copy of this matrix is cached (csr_amd/kernels/hip.py, handle cache) its three arrays are
    # write-protected; every method here that changes them calls _edited() first.
    __csrk_cacheable__ = True

    _parent = None      # subset_rows: the matrix whose colinds / values this one views
    _views = None       # subset_rows: the live sub-matrices that view this one's arrays (weak): while there are any, no
                        # device copy of this matrix is cached -- a write through a view would not be seen

    def _edited(self):
        """
        The arrays are about to change: drop cached device copies (restores the arrays' writeable flags) -- of this
        matrix and of every matrix it is a row range of (subset_rows hands out views: the edit reaches the parent).
        """
        if self._parent is not None:
            self._parent._edited()
        from . import kernels as _k
        mods = list(_k.kernels.values())
        hip = sys.modules.get(_k.__name__ + '.hip')       # (loaded but not yet looked up through the registry)
        if hip is not None and hip not in mods:
            mods.append(hip)
        for kern in mods:
            inv = getattr(kern, 'invalidate', None)
            if inv is not None:
                inv(self)

    # ---- construction ---------------------------------------------------------------------
    @classmethod
    def empty(cls, nrows, ncols, row_nnzs=None, values=True):
        """
        A matrix of the given shape with zeroed arrays: no entries, or (row_nnzs) room for that many per row;
        `values`: True = float64, a dtype, or False = structure only.  (csr/csr.py:102-136 is the counterpart.)
        """
        if nrows < 0 or ncols < 0:
            raise ValueError('negative shape')
        counts = np.zeros(nrows, dtype=np.int64) if row_nnzs is None else np.asarray(row_nnzs, dtype=np.int64)
        if counts.shape != (nrows,):
            raise ValueError('row_nnzs must have one count per row')
        rps = np.concatenate(([0], np.cumsum(counts)))
        nnz = int(rps[-1])
        if not values:
            vs = None
        else:
            vs = np.zeros(nnz, dtype=np.float64 if values is True else values)
        return cls(nrows, ncols, nnz, rps, np.zeros(nnz, dtype=np.intc), vs)

    @classmethod
    def from_coo(cls, rows, cols, vals, shape=None, *, duplicates=None):
        """
        csr/csr.py:138-169 -> csr/structure.py:11-67: stable counting sort of the COO entries
        by row (entries of a row keep their input order).  Host-side ingest, not on the hot
        path (out of scope); done with a stable NumPy argsort.
        duplicates=None keeps every repeated (row, col) pair, as the reference does; 'sum', 'first', 'last', 'max' or
        'min' hands the ingested matrix to coalesce() (on the device), whose result is canonical.
        """
        if duplicates is not None:
            _coalesce_check(get_kernel(), duplicates)
        rows = np.asarray(rows)
        cols = np.asarray(cols)
        assert np.min(rows, initial=0) >= 0 and np.min(cols, initial=0) >= 0
        if shape is not None:
            nrows, ncols = shape
            assert np.max(rows, initial=0) < max(nrows, 1)
            assert np.max(cols, initial=0) < max(ncols, 1)
        else:
            nrows = int(np.max(rows)) + 1
            ncols = int(np.max(cols)) + 1
        nnz = len(rows)
        assert len(cols) == nnz and (vals is None or len(vals) == nnz)
        order = np.argsort(rows, kind='stable')
        rps = np.zeros(nrows + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows, minlength=nrows), out=rps[1:])
        m = cls(nrows, ncols, nnz, rps, cols[order], None if vals is None else np.asarray(vals)[order])
        return m if duplicates is None else m.coalesce(duplicates)

    @classmethod
    def from_scipy(cls, mat, copy=True):
        """
        csr/csr.py:171-192: any SciPy sparse matrix -> CSR (through .tocsr() when it is not CSR already).
        copy=False shares SciPy's arrays where their dtypes allow.  Host only.
        """
        import scipy.sparse as sps
        if not sps.isspmatrix_csr(mat):
            mat, copy = mat.tocsr(), False           # the conversion already made fresh arrays
        parts = []
        for a, dt in ((mat.indptr, np.intc), (mat.indices, np.intc), (mat.data, None)):
            b = np.require(a, dt, 'C')
            parts.append(b.copy() if copy and np.shares_memory(a, b) else b)
        return cls(mat.shape[0], mat.shape[1], mat.nnz, *parts)

    def to_scipy(self):
        "csr/csr.py:194-209: scipy.sparse.csr_matrix over the same arrays (a structure-only matrix gets 1.0 values)"
        import scipy.sparse as sps
        vs = np.ones(self.nnz) if self._values is None else self._values
        return sps.csr_matrix((vs, self.colinds, self.rowptrs), shape=(self.nrows, self.ncols))

    # ---- fields ---------------------------------------------------------------------------
    @property
    def values(self):
        return self._values

    @values.setter
    def values(self, vs):
        "replace the value array (None = structure only); a longer array is cut to nnz (csr/csr.py:224-242)"
        if vs is not None:
            vs = np.ascontiguousarray(vs)
            if vs.shape[0] < self.nnz:
                raise ValueError('value array too small')
            vs = vs[:self.nnz]
        self._edited()
        self._values = vs

    def copy(self, include_values=True, *, copy_structure=True):
        """
        A matrix of its own with the same entries: fresh arrays (copy_structure=False shares rowptrs / colinds
        instead), without values if include_values is false.  (Counterpart: csr/csr.py:298-321.)
        """
        rps, cis = (self.rowptrs.copy(), self.colinds.copy()) if copy_structure else (self.rowptrs, self.colinds)
        vs = self._values.copy() if include_values and self._values is not None else None
        return type(self)(self.nrows, self.ncols, self.nnz, rps, cis, vs, _cast=False)

    # ---- rows -----------------------------------------------------------------------------
    def row_extent(self, row):
        "csr/csr.py:406-417 -> csr/_rows.py:9-13 (host field read, as in the reference)"
        return self.rowptrs[row], self.rowptrs[row + 1]

    def row_nnzs(self):
        "csr/csr.py:432-441.  Host diff like the reference; the device version is kernel.row_nnzs."
        return np.diff(self.rowptrs)

    def rowinds(self):
        "csr/csr.py:366-371 -> csr/_rows.py:116-122: the row index of every stored entry (COO row array), intc"
        return np.repeat(np.arange(self.nrows, dtype=np.intc), np.diff(self.rowptrs))

    def row_cs(self, row):
        "csr/csr.py:419-423: the column indices stored for `row` (a view)"
        lo, hi = self.row_extent(row)
        return self.colinds[lo:hi]

    def row_vs(self, row):
        "csr/csr.py:425-430: the values stored for `row` (a view); 1.0 per entry for a structure-only matrix"
        lo, hi = self.row_extent(row)
        return np.ones(hi - lo) if self._values is None else self._values[lo:hi]

    def _dense_rows(self, row, dtype, ones):
        row = np.asarray(row, dtype=np.int32)
        out = np.zeros(row.shape + (self.ncols,), dtype=dtype)
        for dst, r in zip(out.reshape(-1, self.ncols), row.reshape(-1)):
            lo, hi = self.row_extent(r)
            dst[self.colinds[lo:hi]] = 1 if ones else self._values[lo:hi]
        return out

    def row(self, row):
        """
        csr/csr.py:373-388 -> csr/_rows.py:70-82: one row (or, for an index array, one row per index) densified:
        stored values, 0 elsewhere; a structure-only matrix gives float32 ones.  Host only.
        """
        if self._values is None:
            return self._dense_rows(row, np.float32, True)
        return self._dense_rows(row, self._values.dtype, False)

    def row_mask(self, row):
        "csr/csr.py:390-404: like row(), but True where the row stores an entry"
        return self._dense_rows(row, np.bool_, True)

    def subset_rows(self, begin, end):
        """
        csr/csr.py:331-346 -> csr/structure.py:70-81: views of colinds/values, rebased pointers.  The views write
        through to this matrix, as in the reference: a cached device copy of this matrix is dropped first (views taken
        under the write guard would stay read-only for good), and the sub-matrix's own mutators drop it again.
        """
        self._edited()
        lo, hi = int(self.rowptrs[begin]), int(self.rowptrs[end])
        sub = CSR(end - begin, self.ncols, hi - lo, self.rowptrs[begin:end + 1] - lo, self.colinds[lo:hi],
                  None if self._values is None else self._values[lo:hi])
        sub._parent = self
        if self._views is None:
            self._views = weakref.WeakSet()
        self._views.add(sub)
        return sub

    def pick_rows(self, rows, *, include_values=True):
        """
        csr/csr.py:347-364 -> csr/structure.py:84-149: the given rows, in order (a row may appear more than
        once), as a new matrix; values are dropped with include_values=False.  Runs on the device when the
        active kernel provides `pick_rows`.
        """
        rows = np.asarray(rows)
        assert rows.ndim == 1
        K, pick = self._ext('pick_rows')
        with releasing(K.to_handle(self), K) as h:
            with releasing(pick(h, rows, include_values), K) as ph:
                return K.from_handle(ph)

    # ---- device operations beyond the kernel protocol -----------------------------------------
    def _ext(self, name):
        K = get_kernel()
        fn = getattr(K, name, None)
        if fn is None:
            raise NotImplementedError(f'kernel {K.__name__} does not provide {name}')
        return K, fn

    def transpose(self, include_values=True):
        """
        csr/csr.py:471-486 -> csr/structure.py:240-247.  Runs on the device; bit-exact with the
        reference (stable counting sort, float64 output values, input pointer width).
        """
        K, tr = self._ext('transpose')
        with releasing(K.to_handle(self), K) as h:
            with releasing(tr(h, include_values), K) as th:
                return K.from_handle(th)

    def transpose_structure(self):
        return self.transpose(False)

    def normalize_rows(self, normalization):
        "csr/csr.py:443-469 -> csr/transform.py: in place; returns the per-row norms / means"
        if normalization not in ('center', 'unit'):
            raise ValueError('unknown normalization: ' + normalization)
        K, fn = self._ext('center_rows' if normalization == 'center' else 'unit_rows')
        with releasing(K.to_handle(self), K) as h:
            stat = fn(h)
            vs = K.values_of(h)
        self._edited()
        self._values[...] = vs
        return stat

    def sort_rows(self):
        "csr/csr.py:323-329 -> csr/structure.py:156-169, in place, via the kernel's order_columns"
        K = get_kernel()
        with releasing(K.to_handle(self), K) as h:
            K.order_columns(h)
            out = K.from_handle(h)
        self._edited()
        self.colinds[...] = out.colinds
        if self._values is not None:
            self._values[...] = out.values

    # ---- the kernel protocol's callers --------------------------------------------------------
    def multiply(self, other, transpose=False):
        """
        csr/csr.py:524-567: A @ B (or A @ B^T).  Handle lifetime, row sharding above
        K.max_nnz and the exact-zero filter on the product follow the reference.
        """
        if transpose:
            assert self.ncols == other.ncols
        else:
            assert self.ncols == other.nrows
        K = get_kernel()
        dev_filter = getattr(K, 'filter_zeros', None)

        def mul(A, b_h):
            with releasing(K.to_handle(A), K) as a_h:
                c_h = K.mult_abt(a_h, b_h) if transpose else K.mult_ab(a_h, b_h)
                with releasing(c_h, K):
                    if dev_filter is not None:
                        with releasing(dev_filter(c_h), K) as f_h:
                            return K.from_handle(f_h)
                    crepr = K.from_handle(c_h)
            crepr._filter_zeros()
            return crepr

        with releasing(K.to_handle(other), K) as b_h:
            # one handle of B serves every row block of A; a single block is returned as it is
            blocks = [mul(blk, b_h) for blk in self._row_blocks(K.max_nnz)]
        return blocks[0] if len(blocks) == 1 else CSR._assemble_shards(blocks)

    def mult_vec(self, v):
        "csr/csr.py:569-590: y = A v; above K.max_nnz the row blocks' products are concatenated in row order"
        v = np.asarray(v)
        assert v.shape == (self.ncols,)
        K = get_kernel()
        ys = []
        for blk in self._row_blocks(K.max_nnz):
            with releasing(K.to_handle(blk), K) as h:
                ys.append(K.mult_vec(h, v))
        return ys[0] if len(ys) == 1 else np.concatenate(ys)

    def sddmm(self, U, V, *, scale=False):
        """
        Sampled dense-dense product on this pattern: a new CSR with the same shape, row pointers and column order whose
        value at each stored entry (i, j) is dot(U[i, :], V[j, :]), times the entry's value with scale=True (1.0 for a
        structure-only matrix).  U [nrows x k] and V [ncols x k] are both float32 or both float64; the values are float64.
        The structure is copied from the host arrays; only the values come back from the device.  Above K.max_nnz the
        row blocks' values are concatenated in row order.  Not a reference entry point.
        """
        U, V = np.asarray(U), np.asarray(V)
        if U.ndim != 2 or V.ndim != 2:
            raise ValueError(f'panels must be 2-D, not of shapes {U.shape} and {V.shape}')
        if U.dtype != V.dtype or U.dtype not in (np.float32, np.float64):
            raise ValueError(f'U and V must both be float32 or both float64, not {U.dtype} and {V.dtype}')
        if U.shape[0] != self.nrows or V.shape[0] != self.ncols or U.shape[1] != V.shape[1] or U.shape[1] == 0:
            raise ValueError(f'panels of shapes {U.shape} and {V.shape} do not fit a {self.nrows} x {self.ncols} '
                             'matrix (expected (nrows, k) and (ncols, k), k >= 1)')
        K, fn = self._ext('sddmm')
        vs = []
        r0 = 0
        for blk in self._row_blocks(K.max_nnz):
            with releasing(K.to_handle(blk), K) as h:
                vs.append(fn(h, U[r0:r0 + blk.nrows], V, scale))
            r0 += blk.nrows
        vals = vs[0] if len(vs) == 1 else np.concatenate(vs)
        return CSR(self.nrows, self.ncols, self.nnz, self.rowptrs.copy(), self.colinds.copy(), vals, _cast=False)

    def gram_rows(self, V, *, weighted=False, rows=None, base=None, max_bytes=4 << 30):
        """
        One k x k Gram matrix per row, float64 [n, k, k]: for each row i of rows = (begin, end) (None: all rows), base plus
        the sum over the row's stored columns j of w V[j, :]^T V[j, :], with w = 1 or (weighted=True) the entry's value --
        the left-hand side of the normal equations of alternating least squares (mult_dense gives the right-hand side).  V
        [ncols x k] is float32 or float64; base is None or float64 [k, k] (its lower triangle is read; lambda I for a
        ridge).  Every block is exactly symmetric and every element a fixed chain of one rounded multiply and one fused
        multiply-add per entry, in storage order (include/csrk.h).  A request whose result would exceed max_bytes is
        refused with ValueError: ask for row ranges.  Not a reference entry point.
        """
        K, fn = self._ext('gram_rows')
        V, _, k, _, rb, re_, base = K.gram_args(self, V, rows, base)
        per_row = k * k * 8
        if (re_ - rb) * per_row > max_bytes:
            raise ValueError(f'{re_ - rb} rows of {k} x {k} float64 are {(re_ - rb) * per_row} bytes, above max_bytes = '
                             f'{max_bytes}: at most {max(int(max_bytes) // per_row, 0)} rows fit, ask for rows=(begin, end) ranges')
        if self.nnz > K.max_nnz:
            raise ValueError('CSR size {} exceeds max nnz {}'.format(self.nnz, K.max_nnz))
        with releasing(K.to_handle(self), K) as h:
            return fn(h, V, weighted, (rb, re_), base)

    def als_rows(self, V, *, weighted=False, rhs='values', base=None, reg_per_entry=0.0, rows=None, return_info=False):
        """
        One half-step of alternating least squares, float64 [n, k]: for each row i of rows = (begin, end) (None: all rows)
        the solution u_i of
            (base + sum_j w_ij V[j, :]^T V[j, :] + reg_per_entry * n_i * I) u_i = sum_j c_ij V[j, :]
        over the row's n_i stored columns j, with w = 1 or (weighted=True) the entry's value and c = the value
        (rhs='values'), 1 ('ones') or 1 + the value ('one_plus_values': implicit feedback with values stored as
        confidence - 1).  Explicit ALS: weighted=False, rhs='values', a ridge in base or reg_per_entry.  Implicit ALS:
        weighted=True, rhs='one_plus_values', base = V^T V + lambda I (kernels.hip.panel_gram(V, lambda) computes it on the
        device in a fixed order; als_fit runs whole sweeps).  The k x k block is gram_rows' block bit for bit,
        but it is built and factorised (LDL^T, no pivoting, a fixed order of fused multiply-adds) on the chip and never
        stored, so the result is small whatever k and no max_bytes is needed (include/csrk.h, csrk_als_rows).  A row
        whose system has a pivot that is not positive (an empty row without base, an indefinite base) raises ValueError
        naming the first such row; with return_info=True nothing is raised and (U, info) comes back, info[i] = 0 or
        1 + the first bad pivot of row i.  Not a reference entry point.
        """
        K, fn = self._ext('als_rows')
        _, _, _, _, rb, re_, base, _, lam_n = K.als_args(self, V, rhs, base, reg_per_entry, rows)
        if self.nnz > K.max_nnz:
            raise ValueError('CSR size {} exceeds max nnz {}'.format(self.nnz, K.max_nnz))
        with releasing(K.to_handle(self), K) as h:
            U, info = fn(h, V, weighted, rhs, base, lam_n, (rb, re_))
        if return_info:
            return U, info
        bad = np.flatnonzero(info)
        if len(bad):
            raise ValueError(f'{len(bad)} of {re_ - rb} rows have a system that is not positive definite; the first is row '
                             f'{rb + int(bad[0])}, at pivot {int(info[bad[0]]) - 1} (return_info=True returns the codes)')
        return U

    def als_rows_cg(self, V, *, x0=None, steps=3, weighted=False, rhs='values', base=None, reg=0.0, reg_per_entry=0.0, rows=None,
                    tol=0.0, return_info=False):
        """
        One half-step of alternating least squares by conjugate gradient, float64 [n, k]: for each row i of rows =
        (begin, end) (None: all rows) at most `steps` CG steps, started from x0's row (float64 [n, k], usually the previous
        sweep's factors; None: from zero), on
            (base + sum_j w_ij V[j, :]^T V[j, :] + (reg + reg_per_entry * n_i) * I) u_i = sum_j c_ij V[j, :]
        with w, c, rhs and base as in als_rows.  The k x k block is never formed: a step is one pass over the row's V rows
        and, with a base, one k x k matrix-vector product, so the cost grows with k n_i (+ k^2), not k^2 n_i + k^3.  A few
        warm-started steps per sweep are the usual solver of implicit-feedback ALS; steps = 2 k from zero approaches
        als_rows' solution.  tol is a residual 2-norm: a row stops once its residual is no longer above it.  Of base the
        lower triangle is read and mirrored, as als_rows reads it, so both solvers see the same matrix.  Every output is
        a fixed chain of fused multiply-adds (include/csrk.h, csrk_als_rows_cg): the same bits whatever the launch.
        With return_info=True (U, resid, taken) comes back: the squared residual of the recurrence at each row's stop and
        the steps it made.  A row of at least L entries takes a whole workgroup instead of 16 lanes
        (kernels.hip.als_cg_set_long(L), or the environment variable CSRK_ALS_CG_LONG; 0 turns that off;
        kernels.hip.als_cg_last_stats() counts such rows): it changes the time, never a bit.  Not a reference entry point.
        """
        K, fn = self._ext('als_rows_cg')
        _, _, _, _, rb, re_, base, _, lam, lam_n, steps, _, x0 = K.als_cg_args(self, V, rhs, base, reg, reg_per_entry, rows, steps, x0,
                                                                               tol)
        if self.nnz > K.max_nnz:
            raise ValueError('CSR size {} exceeds max nnz {}'.format(self.nnz, K.max_nnz))
        if base is not None:
            base = np.tril(base) + np.tril(base, -1).T
        with releasing(K.to_handle(self), K) as h:
            U, resid, taken = fn(h, V, weighted, rhs, base, lam, lam_n, (rb, re_), steps, x0, tol)
        return (U, resid, taken) if return_info else U

    def als_objective(self, U, V, *, weighted=False, rhs='values', implicit=False, reg=0.0, reg_per_entry=0.0):
        """
        What the ALS half-steps minimise, one float, for row factors U [nrows x k] and column factors V [ncols x k]
        (float64):
            sum_ij (w_ij s_ij - 2 c_ij) s_ij  +  sum_i (reg + reg_per_entry n_i) |u_i|^2  +  sum_j (reg + reg_per_entry m_j) |v_j|^2
        over the stored entries, s_ij = u_i . v_j, w and c as in als_rows, n_i and m_j the entries of row i and column j;
        with implicit=True plus sum over ALL pairs of s_ij^2, computed as <U^T U, V^T V>.  This is the usual loss minus a
        constant that does not depend on the factors: sum a_ij^2 for explicit ALS (weighted=False, rhs='values'),
        sum (1 + a_ij) for Hu-Koren implicit ALS (weighted=True, rhs='one_plus_values', implicit=True), so a sweep that
        helps lowers it.  Every sum runs on the device in a fixed order (include/csrk.h, rule J).  Not a reference entry
        point.
        """
        K, fn = self._ext('als_objective')
        K.als_objective_args(self, None, U, V, rhs, reg, reg_per_entry)
        if self.nnz > K.max_nnz:
            raise ValueError('CSR size {} exceeds max nnz {}'.format(self.nnz, K.max_nnz))
        with releasing(K.to_handle(self), K) as h:
            with releasing(K.transpose(h, True), K) as th:
                return fn(h, th, U, V, weighted, rhs, implicit, reg, reg_per_entry)

    def als_fit(self, U0, V0, *, sweeps=10, solver='cg', steps=3, weighted=False, rhs='values', implicit=False, reg=0.0,
                reg_per_entry=0.0, tol=0.0, return_objective=False, return_info=False):
        """
        Alternating least squares from the caller's start factors U0 [nrows x k] and V0 [ncols x k] (float64; no random
        numbers are drawn here): `sweeps` times a half-step for the rows' factors, then one for the columns' on the
        transpose, with both panels on the device throughout.  solver='cg': als_rows_cg, `steps` warm-started steps (tol
        as there); solver='exact': als_rows.  The shared base is not a parameter: implicit=True makes it V^T V (resp. U^T U)
        on the device in a fixed order, and reg is the constant ridge, reg_per_entry the one that grows with a row's
        entries; weighted and rhs are als_rows'.  Explicit ALS: the defaults with a reg or reg_per_entry.  Hu-Koren
        implicit ALS: weighted=True, rhs='one_plus_values', implicit=True, values stored as confidence - 1.  The result is
        the caller's own loop over panel_gram, als_rows[_cg] and als_objective bit for bit (include/csrk.h, rule F).
        Returns (U, V); with return_objective=True the float64 [sweeps + 1] objective (als_objective before the first
        sweep and after each) follows, with return_info=True the int64 [2 sweeps] count of rows per half-step whose system
        was not positive definite (solver='exact').  Without return_info such a row raises ValueError naming the first
        half-step that has one.  Not a reference entry point.
        """
        K, fn = self._ext('als_fit')
        K.als_fit_args(self, None, U0, V0, sweeps, solver, steps, rhs, reg, reg_per_entry, tol)
        if self.nnz > K.max_nnz:
            raise ValueError('CSR size {} exceeds max nnz {}'.format(self.nnz, K.max_nnz))
        with releasing(K.to_handle(self), K) as h:
            with releasing(K.transpose(h, True), K) as th:
                U, V, obj, bad = fn(h, th, U0, V0, sweeps, solver, steps, weighted, rhs, implicit, reg, reg_per_entry, tol,
                                    return_objective)
        if not return_info and bad.any():
            first = int(np.flatnonzero(bad)[0])
            raise ValueError(f'half-step {first} (sweep {first // 2}, the {"rows" if first % 2 == 0 else "columns"}) has '
                             f'{int(bad[first])} systems that are not positive definite (return_info=True returns the counts)')
        out = (U, V)
        if return_objective:
            out += (obj,)
        if return_info:
            out += (bad,)
        return out

    def topk_rows(self, k, *, min_value=None, order='descending'):
        """
        Each row's k largest entries that are not below min_value (None: no threshold) as a new CSR of the same shape:
        best first (order='descending') or in the order they had in the row (order='storage').  NaN ranks above +Inf,
        -0.0 ties with +0.0, ties go to the entry stored earlier; indices and values are copied bit for bit and the values
        keep their dtype (include/csrk.h).  Runs on the device, per row block above K.max_nnz.  Not a reference entry point.
        """
        K, fn = self._ext('topk_rows')
        _topk_check(K, k, min_value, order)
        if self._values is None:
            raise ValueError('matrix has no values')

        def top(A):
            with releasing(K.to_handle(A), K) as h:
                with releasing(fn(h, k, min_value, order), K) as t_h:
                    return K.from_handle(t_h)

        blocks = [top(blk) for blk in self._row_blocks(K.max_nnz)]
        return blocks[0] if len(blocks) == 1 else CSR._assemble_shards(blocks)

    def topk_scores(self, U, V, n, *, min_score=None, rows=None, exclude=True):
        """
        Recommendations from a factor model, with this matrix as the pairs already seen: for each row i of rows =
        (begin, end) (None: all rows) the n items j with the largest score dot(U[i, :], V[j, :]) among the columns row i does
        not store (exclude=False: among all columns) whose score is not below min_score (None: no threshold).  Returns
        (items int32 [m, n], scores float64 [m, n], counts int32 [m]): best first, padded with item -1 and score -inf
        beyond counts[i].  U [nrows x k] and V [ncols x k] are both float32 or both float64; every score is one chain of k
        fused multiply-adds in float64, NaN ranks above +Inf, -0.0 ties with +0.0 and ties go to the smaller item, so the
        result is a function of the inputs, bit for bit (include/csrk.h, csrk_topk_scores).  The dense block of scores is
        never formed.  This matrix must be canonical (sort_rows / coalesce); its values are not read.  Runs on the device
        only.  Not a reference entry point.
        """
        K, fn = self._ext('topk_scores')
        K.topk_scores_args(self, U, V, n, min_score, rows)
        if not exclude:      # (the panels have this matrix's shape: checked above)
            return fn(None, U, V, n, min_score, rows)
        if self.nnz > K.max_nnz:
            raise ValueError('CSR size {} exceeds max nnz {}'.format(self.nnz, K.max_nnz))
        with releasing(K.to_handle(self), K) as h:
            return fn(h, U, V, n, min_score, rows)

    def topk_scores_for(self, users, U, V, n, *, min_score=None, exclude=True, splits=None):
        """
        topk_scores for a list of rows -- serving: (items int32 [m, n], scores float64 [m, n], counts int32 [m]) with
        m = len(users), row r of the result for row users[r].  users is a 1-D array of integer row indices in any order,
        repeats allowed; an index outside [0, nrows) is a ValueError naming its position.  Scores, candidates, order and
        padding are topk_scores', bit for bit: for users = arange(b, e) the result equals topk_scores(rows=(b, e)).  The
        items are cut into `splits` ranges that run side by side so that a few rows still fill the card (None: chosen from
        the number of rows; K.topk_scores_for_workspace tells); no bit depends on it (include/csrk.h,
        csrk_topk_scores_for).  Only the listed rows of U are sent.  This matrix must be canonical; its values are not read.
        Runs on the device only.  Not a reference entry point.
        """
        K, fn = self._ext('topk_scores_for')
        K.topk_scores_for_args(self, users, U, V, n, min_score, splits)
        if not exclude:      # (the panels have this matrix's shape: checked above)
            return fn(None, users, U, V, n, min_score, splits)
        if self.nnz > K.max_nnz:
            raise ValueError('CSR size {} exceeds max nnz {}'.format(self.nnz, K.max_nnz))
        with releasing(K.to_handle(self), K) as h:
            return fn(h, users, U, V, n, min_score, splits)

    def rank_entries(self, U, V, test, *, rows=None, exclude=True, return_scores=False):
        """
        Offline evaluation of a factor model, with this matrix as the pairs already seen and `test`, a CSR of the same
        shape, as the held-out pairs: for every entry (i, j) of `test` in rows = (begin, end) (None: all rows), in storage
        order, the position j takes in row i's full ranking of the columns row i does not store here (exclude=False: of all
        columns) -- the number of such columns c != j whose score dot(U[i, :], V[c, :]) comes before j's.  Returns ranks
        (int32, one per entry), or (ranks, scores float64) with return_scores=True.  Scores and order are topk_scores': one
        chain of k fused multiply-adds in float64, NaN above +Inf, -0.0 tied with +0.0, ties to the smaller column, so an
        entry of rank r < n is topk_scores' items[i][r] and every bit is a function of the inputs (include/csrk.h,
        csrk_rank_entries).  Hit rate, MRR and nDCG follow from the ranks; for percentile rank and AUC the number of
        candidates of row i is ncols - row_nnzs()[i] (ncols with exclude=False).  This matrix must be canonical (sort_rows /
        coalesce); `test` may hold its columns in any order and more than once; the values of neither are read.  The dense
        block of scores is never formed.  Runs on the device only.  Not a reference entry point.
        """
        K, fn = self._ext('rank_entries')
        if not isinstance(test, CSR):
            raise ValueError(f'test must be a CSR, not {type(test).__name__}')
        K.rank_entries_args(self, test, U, V, rows)
        for m in ((self, test) if exclude else (test,)):
            if m.nnz > K.max_nnz:
                raise ValueError('CSR size {} exceeds max nnz {}'.format(m.nnz, K.max_nnz))
        with releasing(K.to_handle(test), K) as t_h:
            if not exclude:
                ranks, scores = fn(None, t_h, U, V, rows)
            elif test is self:                   # one device copy serves both sides
                ranks, scores = fn(t_h, t_h, U, V, rows)
            else:
                with releasing(K.to_handle(self), K) as s_h:
                    ranks, scores = fn(s_h, t_h, U, V, rows)
        return (ranks, scores) if return_scores else ranks

    def rank_entries_for(self, users, U, V, test, *, exclude=True, return_scores=False, return_offsets=False, splits=None):
        """
        rank_entries for a list of rows -- evaluating a sample of users: ranks (int32) of the entries `test` stores in rows
        users[0], users[1], ..., row by row in list order and each row's entries in storage order.  users is a 1-D array of
        integer row indices in any order, repeats allowed (each occurrence gets its own outputs); an index outside
        [0, nrows) is a ValueError naming its position.  The entries of users[r] start at offsets[r], the int64 prefix sum of
        test.row_nnzs()[users] (len(users) + 1 of them).  Returns ranks, followed by scores (float64) with
        return_scores=True and by offsets with return_offsets=True.  Scores, candidates and order are rank_entries', bit for
        bit: for users = arange(b, e) the result equals rank_entries(rows=(b, e)).  The items are cut into `splits` ranges
        that run side by side so that a sample still fills the card (None: chosen from the number of rows;
        K.rank_entries_for_splits tells) and the partial ranks, integers, add: no bit depends on it (include/csrk.h,
        csrk_rank_entries_for).  Only the listed rows of U are sent.  This matrix must be canonical (exclude=False: it is not
        looked at); the values of neither are read.  Runs on the device only.  Not a reference entry point.
        """
        K, fn = self._ext('rank_entries_for')
        if not isinstance(test, CSR):
            raise ValueError(f'test must be a CSR, not {type(test).__name__}')
        users = K.rank_entries_for_args(self, test, users, U, V, splits)[0]
        for m in ((self, test) if exclude else (test,)):
            if m.nnz > K.max_nnz:
                raise ValueError('CSR size {} exceeds max nnz {}'.format(m.nnz, K.max_nnz))
        with releasing(K.to_handle(test), K) as t_h:
            if not exclude:
                ranks, scores = fn(None, t_h, users, U, V, splits)
            elif test is self:                   # one device copy serves both sides
                ranks, scores = fn(t_h, t_h, users, U, V, splits)
            else:
                with releasing(K.to_handle(self), K) as s_h:
                    ranks, scores = fn(s_h, t_h, users, U, V, splits)
        out = (ranks,) + ((scores,) if return_scores else ())
        if return_offsets:
            offsets = np.zeros(len(users) + 1, np.int64)
            np.cumsum(test.row_nnzs()[users], out=offsets[1:])
            out += (offsets,)
        return out[0] if len(out) == 1 else out

    # ---- two matrices entry by entry -----------------------------------------------------------
    def _knn_check(self, K, model, users, max_nbrs, min_nbrs, aggregate, offsets, route='walk'):
        "knn_scores' arguments as the kernel takes them, checked before any device work; users=None: all rows"
        K.knn_route_arg(route)
        if not all(hasattr(model, a) for a in ('nrows', 'ncols', 'nnz')) or isinstance(model, np.ndarray):
            raise ValueError(f'model must be a CSR, not {type(model).__name__}')
        users = np.arange(self.nrows, dtype=np.int32) if users is None else users
        args = K.knn_scores_args(model, self, users, 0 if max_nbrs is None else max_nbrs, min_nbrs, aggregate, offsets)
        for m in (self, model):
            if m.nnz > K.max_nnz:
                raise ValueError('CSR size {} exceeds max nnz {}'.format(m.nnz, K.max_nnz))
        return args[0]

    def knn_scores(self, model, users=None, *, max_nbrs=None, min_nbrs=1, aggregate='weighted-average', offsets=None, route='walk'):
        """
        Scores from an item-kNN model, with this matrix as the ratings [users x items]: a CSR [len(users) x model.nrows],
        float64, canonical, row r for user users[r] (users=None: all rows; any order, repeats allowed).  `model` is a CSR
        [targets x items] whose rows hold each target's neighbours, best first -- what multiply_topk(..., transpose=True,
        order='descending') returns.  For each target the neighbour list is walked in storage order; the neighbours the user
        has rated are hits, the walk ends after max_nbrs hits (None: no limit), and a target with at least min_nbrs hits is
        stored: sum(rating * similarity) / sum(|similarity|) over the hits (aggregate='weighted-average') or
        sum(similarity) ('sum'), plus offsets[r] when offsets is given (a user's mean after center_rows).  Every operation is
        rounded on its own in storage order, so the result is a function of the arguments, bit for bit (include/csrk.h,
        csrk_knn_scores).  This matrix must be canonical (sort_rows / coalesce); the model need not be.  route='walk'
        visits every target for every user; route='reach' only the targets that hold one of the user's rated items -- the
        same bits, from an index of the model's pattern that its device copy keeps (the model's columns must lie in
        [0, ncols)).  Runs on the device only.  Not a reference entry point.
        """
        K, fn = self._ext('knn_scores')
        users = self._knn_check(K, model, users, max_nbrs, min_nbrs, aggregate, offsets, route)
        mx = 0 if max_nbrs is None else max_nbrs
        with releasing(K.to_handle(model), K) as m_h:
            with releasing(K.to_handle(self), K) as r_h:
                with releasing(fn(m_h, r_h, users, mx, min_nbrs, aggregate, offsets, route=route), K) as s_h:
                    return K.from_handle(s_h)

    def knn_topk(self, model, users, n, *, exclude=True, min_value=None, **scoring):
        """
        Recommendations from an item-kNN model: knn_scores(model, users, **scoring) -> without the items the user has rated
        (exclude=True) -> each row's n best scores that are not below min_value, best first (topk_rows' order), as a CSR
        [len(users) x model.nrows].  The handle chain knn_scores -> combine 'drop' against pick_rows(ratings, users) ->
        topk_rows stays on the device: only n entries per user cross PCIe.  exclude=True needs a model over the same items
        as its neighbours (model.nrows == ncols).
        """
        K, fn = self._ext('knn_scores')
        _, top = self._ext('topk_rows')
        _, comb = self._ext('combine')
        _, pick = self._ext('pick_rows')
        bad = set(scoring) - {'max_nbrs', 'min_nbrs', 'aggregate', 'offsets', 'route'}
        if bad:
            raise TypeError(f'knn_topk got unexpected scoring arguments {sorted(bad)}')
        max_nbrs, min_nbrs = scoring.get('max_nbrs'), scoring.get('min_nbrs', 1)
        aggregate, offsets = scoring.get('aggregate', 'weighted-average'), scoring.get('offsets')
        route = scoring.get('route', 'walk')
        users = self._knn_check(K, model, users, max_nbrs, min_nbrs, aggregate, offsets, route)
        _topk_check(K, n, min_value, 'descending')
        if exclude and model.nrows != self.ncols:
            raise ValueError(f'exclude=True needs a model over the rated items: model has {model.nrows} rows, ratings {self.ncols} columns')
        mx = 0 if max_nbrs is None else max_nbrs
        with releasing(K.to_handle(model), K) as m_h:
            with releasing(K.to_handle(self), K) as r_h:
                with releasing(fn(m_h, r_h, users, mx, min_nbrs, aggregate, offsets, route=route), K) as s_h:
                    if not exclude:
                        with releasing(top(s_h, n, min_value, 'descending'), K) as t_h:
                            return K.from_handle(t_h)
                    with releasing(pick(r_h, users, False), K) as x_h:
                        with releasing(comb(s_h, x_h, 'drop'), K) as d_h:
                            with releasing(top(d_h, n, min_value, 'descending'), K) as t_h:
                                return K.from_handle(t_h)

    def _combine(self, other, op, alpha=1.0, beta=1.0):
        """
        to_handle x 2 -> combine -> from_handle.  Above K.max_nnz both operands are cut at the same row boundaries (the
        union of their own _shard_cuts, so that every block fits for both) and the blocks' results are stacked.
        """
        K, fn = self._ext('combine')
        chk = getattr(K, 'combine_args', None)
        if chk is not None:
            chk(self, other, op, alpha, beta)
        if (self.nrows, self.ncols) != (other.nrows, other.ncols):
            raise ValueError(f'operands of different shapes: {self.nrows} x {self.ncols} and {other.nrows} x {other.ncols}')

        def comb(A, B):
            with releasing(K.to_handle(A), K) as a_h:
                if B is A:                           # one device copy serves both sides
                    with releasing(fn(a_h, a_h, op, alpha, beta), K) as c_h:
                        return K.from_handle(c_h)
                with releasing(K.to_handle(B), K) as b_h:
                    with releasing(fn(a_h, b_h, op, alpha, beta), K) as c_h:
                        return K.from_handle(c_h)

        if max(self.nnz, other.nnz) <= K.max_nnz:
            return comb(self, other)
        cuts = sorted(set(self._shard_cuts(K.max_nnz)) | set(other._shard_cuts(K.max_nnz)))
        blocks = [comb(self.subset_rows(a, b), other.subset_rows(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
        return CSR._assemble_shards(blocks)

    def add(self, other, alpha=1.0, beta=1.0):
        """
        alpha * self + beta * other over the union of the two patterns, as a new CSR with float64 values and rows ascending
        in column.  Both matrices must be canonical (every row strictly ascending in column: sort_rows sorts, coalesce
        sorts and merges repeated columns; the library refuses anything else with CsrkError).  Every product and the sum are rounded on their own, float32 values are
        widened exactly, a structure-only operand counts as 1.0, and an exact-zero sum stays stored (include/csrk.h,
        csrk_combine).  Runs on the device.  Not a reference entry point.
        """
        return self._combine(other, 'add', alpha, beta)

    def subtract(self, other):
        "self - other: add(other, 1.0, -1.0)"
        return self._combine(other, 'add', 1.0, -1.0)

    def multiply_entries(self, other):
        "the entry-wise product over the intersection of the two patterns (float64; both matrices canonical, as for add)"
        return self._combine(other, 'multiply')

    def keep_entries(self, other):
        """
        The entries of self whose (row, column) `other` stores, in self's storage order, indices and values bit for bit
        (a structure-only self stays structure-only).  Only `other` must be canonical: self may be unsorted and repeat
        columns (a product in the reference's column order is).  other's values are not read.
        """
        return self._combine(other, 'keep')

    def drop_entries(self, other):
        "the entries of self whose (row, column) `other` does NOT store; otherwise as keep_entries"
        return self._combine(other, 'drop')

    # ---- the canonical form ---------------------------------------------------------------------
    def coalesce(self, duplicates='sum'):
        """
        The canonical form as a new CSR: every row strictly ascending in column, one entry per distinct (row, column).  The
        entries of a row that share a column are merged in their storage order: 'sum' adds them left to right (each add
        rounded in the values' dtype; an exact zero stays stored), 'first' / 'last' keep the one stored first / last,
        'max' / 'min' the earliest stored of the largest / the latest stored of the smallest in topk_rows' order (NaN above
        +Inf, -0.0 ties with +0.0); all but 'sum' copy the value bit for bit.  Values keep their dtype, a structure-only
        matrix stays structure-only (include/csrk.h, csrk_coalesce).  What add, multiply_entries and the masks ask of
        their operands.  Runs on the device, per row block above K.max_nnz (a group never leaves its row).  Not a reference
        entry point.
        """
        K, fn = self._ext('coalesce')
        _coalesce_check(K, duplicates)

        def co(A):
            with releasing(K.to_handle(A), K) as h:
                with releasing(fn(h, duplicates), K) as c_h:
                    return K.from_handle(c_h)

        blocks = [co(blk) for blk in self._row_blocks(K.max_nnz)]
        return blocks[0] if len(blocks) == 1 else CSR._assemble_shards(blocks)

    def sum_duplicates(self):
        "coalesce('sum'), under SciPy's name for it (a new matrix: self is not changed)"
        return self.coalesce('sum')

    def is_canonical(self, *, with_row=False):
        """
        Is every row strictly ascending in column (sorted, no column twice)?  Asked on the device.  with_row=True returns
        (answer, the first row that is not -- None when canonical).
        """
        K, fn = self._ext('is_canonical')
        r0 = 0
        ok, row = True, None
        for blk in self._row_blocks(K.max_nnz):
            with releasing(K.to_handle(blk), K) as h:
                ok, row = fn(h)
            if not ok:
                row += r0
                break
            r0 += blk.nrows
        return (ok, row) if with_row else ok

    def multiply_topk(self, other, k, *, transpose=False, min_value=None, order='descending', exclude=None):
        """
        self.multiply(other, transpose).topk_rows(k, min_value=min_value, order=order), array for array, with the product
        left on the device: per row block to_handle -> mult_ab / mult_abt -> filter_zeros -> topk_rows -> from_handle, so
        only the kept entries cross PCIe (item-kNN: each row's k most similar neighbours above a minimum similarity).
        exclude: a canonical CSR of the product's shape whose stored positions are removed from the product before the
        top-k (a recommender's seen items) -- drop_entries on the device between filter_zeros and topk_rows; its device copy
        is made once and pick_rows takes the rows of each block.
        """
        if transpose:
            assert self.ncols == other.ncols
        else:
            assert self.ncols == other.nrows
        K, fn = self._ext('topk_rows')
        _topk_check(K, k, min_value, order)
        _, dev_filter = self._ext('filter_zeros')
        if exclude is not None:
            return self._multiply_topk_excluding(other, k, transpose, min_value, order, exclude)

        def mul(A, b_h):
            with releasing(K.to_handle(A), K) as a_h:
                with releasing(K.mult_abt(a_h, b_h) if transpose else K.mult_ab(a_h, b_h), K) as c_h:
                    with releasing(dev_filter(c_h), K) as f_h:
                        with releasing(fn(f_h, k, min_value, order), K) as t_h:
                            return K.from_handle(t_h)

        with releasing(K.to_handle(other), K) as b_h:
            blocks = [mul(blk, b_h) for blk in self._row_blocks(K.max_nnz)]
        return blocks[0] if len(blocks) == 1 else CSR._assemble_shards(blocks)

    def _multiply_topk_excluding(self, other, k, transpose, min_value, order, exclude):
        "multiply_topk with `exclude`: product -> filter_zeros -> combine(.., 'drop') -> topk_rows, all on the device"
        K, fn = self._ext('topk_rows')
        _, dev_filter = self._ext('filter_zeros')
        _, comb = self._ext('combine')
        _, pick = self._ext('pick_rows')
        shape = (self.nrows, other.nrows if transpose else other.ncols)
        if (exclude.nrows, exclude.ncols) != shape:
            raise ValueError(f'exclude is {exclude.nrows} x {exclude.ncols}, the product {shape[0]} x {shape[1]}')

        def mul(A, b_h, x_h):
            with releasing(K.to_handle(A), K) as a_h:
                with releasing(K.mult_abt(a_h, b_h) if transpose else K.mult_ab(a_h, b_h), K) as c_h:
                    with releasing(dev_filter(c_h), K) as f_h:
                        with releasing(comb(f_h, x_h, 'drop'), K) as d_h:
                            with releasing(fn(d_h, k, min_value, order), K) as t_h:
                                return K.from_handle(t_h)

        blocks = self._row_blocks(K.max_nnz)
        with releasing(K.to_handle(other), K) as b_h:
            with releasing(K.to_handle(exclude), K) as x_h:
                if len(blocks) == 1:
                    return mul(self, b_h, x_h)
                out, r0 = [], 0
                for blk in blocks:
                    with releasing(pick(x_h, np.arange(r0, r0 + blk.nrows, dtype=np.int32), False), K) as xb_h:
                        out.append(mul(blk, b_h, xb_h))
                    r0 += blk.nrows
        return CSR._assemble_shards(out)

    def _row_blocks(self, limit):
        "the matrix itself when it fits the kernel's max_nnz, else its _shard_rows blocks"
        return [self] if self.nnz <= limit else self._shard_rows(limit)

    def _filter_zeros(self):
        """
        csr/csr.py:592-597 -> csr/_struct.py:61-76, host flavour for kernels without a device
        filter: drop entries whose value is exactly 0 (NaN stays), in place.
        """
        if self.values is None:
            return
        keep = self.values != 0
        self._edited()
        cum = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
        self.rowptrs = cum[self.rowptrs].astype(self.rowptrs.dtype)
        self.colinds = np.ascontiguousarray(self.colinds[keep])
        self._values = np.ascontiguousarray(self.values[keep])
        self.nnz = int(cum[-1])

    def _shard_rows(self, tgt_nnz):
        """
        csr/csr.py:599-621: consecutive row blocks of at most tgt_nnz entries each, cut greedily: a block ends at the
        last row boundary that keeps it within the target; a single row larger than the target cannot be placed.
        Pinned by tests/golden/shard.npz (the reference's own cuts).
        """
        cuts = self._shard_cuts(tgt_nnz)
        return [self.subset_rows(a, b) for a, b in zip(cuts[:-1], cuts[1:])]

    def _shard_cuts(self, tgt_nnz):
        "the row boundaries of _shard_rows: [0, ..., nrows]"
        assert tgt_nnz > 0
        ptr = self.rowptrs.astype(np.int64)
        cuts = [0]
        while int(ptr[-1]) - int(ptr[cuts[-1]]) > tgt_nnz:
            first = cuts[-1]
            room = int(ptr[first]) + tgt_nnz
            # first row boundary at or past the target; when it overshoots, the boundary before it ends the block --
            # unless that is the block's own start: then its first row alone exceeds the target
            nxt = first + int(np.searchsorted(ptr[first:], room))
            if ptr[nxt] > room:
                if nxt - first <= 1:
                    raise ValueError("row too large to fit in target matrix size")
                nxt -= 1
            _log.debug('%s: row block [%d, %d) holds %d entries', self, first, nxt, int(ptr[nxt]) - int(ptr[first]))
            cuts.append(nxt)
        cuts.append(self.nrows)
        return cuts

    @classmethod
    def _assemble_shards(cls, shards):
        "csr/csr.py:623-650: stack row blocks (same ncols up to trailing width) back into one matrix, rows in order"
        counts = np.concatenate([np.diff(s.rowptrs) for s in shards]) if shards else np.zeros(0, np.int64)
        rps = np.zeros(len(counts) + 1, np.int64)
        np.cumsum(counts, out=rps[1:])
        nnz = sum(s.nnz for s in shards)
        assert rps[-1] == nnz, f'{rps[-1]} != {nnz}'
        cis = np.concatenate([s.colinds for s in shards])
        vs = None if shards[0].values is None else np.concatenate([s.values for s in shards])
        return cls(len(counts), max(s.ncols for s in shards), nnz, rps, cis, vs)

    def __str__(self):
        return '<CSR {}x{} ({} nnz)>'.format(self.nrows, self.ncols, self.nnz)

    __repr__ = __str__

    def __reduce__(self):
        "csr/csr.py:690-692"
        return (CSR, (self.nrows, self.ncols, self.nnz, self.rowptrs, self.colinds, self.values, False))
