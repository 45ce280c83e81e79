"""
Row-partitioned SpMV across the GPUs of one node: one process per GPU, torch.distributed
for the exchange (backend "nccl" = RCCL over xGMI on ROCm; "gloo" in the CPU tests).

This is the parallel form of what the reference does sequentially when a matrix exceeds a
kernel's max_nnz (csr/csr.py:584-590): split A into contiguous row ranges balanced by nnz
(split points = searchsorted(rowptrs, g*nnz/G), the primitive of _shard_rows, csr/csr.py:609),
multiply every range against the SAME x, and concatenate the pieces (np.concatenate, :590).
Here every rank owns one range, x is replicated, and the concatenation is the one exchange
step of the path:

  allgather  (default) every rank contributes its y slice; slices are padded to the longest
             one so a single all_gather_into_tensor moves them (xGMI is point-to-point: the
             7 peers' slices arrive over 7 links concurrently), then unpadded into y by one
             concatenation kernel.
  allgatherv the slices of y themselves as the output list of one all_gather (RCCL: a group of broadcasts for
             slices of different lengths): no padding, no concatenation.
  allreduce  the form BASELINE.json's north_star names: each rank writes its slice into a
             zeroed full-length y and the ranks sum.  Same result (the slices are disjoint, so
             every sum has one non-zero term and is exact), about twice the bytes per link.

SplitPhaseRowPartitionedSpMV: point-to-point sends of the slices straight into y, hidden behind the tiers' part of one
product (csrk_spmv_device_part).

torch is plumbing here (device buffers + the collective); the product kernels run behind
`local_spmv`, a callable that writes y[r0:r1] = A[r0:r1, :] x into the buffer it is given.

RowPartitionedSpMM: the same partition for C = A B with a dense row-major panel B [ncols x k] (BASELINE configs[2],
csrk_spmm_dense_device): B is replicated, every rank computes its row slab of C, and the same three exchanges complete
C on every rank -- the slabs are k times larger than y's slices, and rows of C are k * 8 bytes apart.  `col_block`
splits the panel into column blocks: block j + 1's product runs on the caller's stream while block j's collective runs
on a second stream, and each exchanged block is copied into its columns of C (a strided copy).  Every column of C is
computed the same way whatever the blocking, so the result is bit-identical for every col_block.

What is measured and what is not: tools/bench_spmm_dist.py times the local product and the whole step per mode and
block width.  Only one RCCL rank (and two gloo ranks sharing one GPU, in the tests) has run any of this; the 8-GPU
exchange -- the 1 GB C of configs[2], 7/8 of it arriving at every rank -- is a cost model, not a
measurement.
"""
import ctypes as C

import torch
import torch.distributed as dist

from ._lib import lib, check

_MODES = ('allgather', 'allgatherv', 'allreduce')


class _RowPartition:
    """
    What the three operators share: rank `rank` of `world` owns rows r0:r1 = bounds[rank]:bounds[rank + 1] of
    nrows = bounds[-1], and the device timing of its local products.  timing = True brackets every launch of a local
    product with an event pair (CUDA outputs only); compute_ms() is their mean device time per step.
    """

    def __init__(self, bounds, rank, world, group, launches_per_step):
        assert len(bounds) == world + 1
        self.bounds = [int(b) for b in bounds]
        self.rank, self.world, self.group = rank, world, group
        self.nrows = self.bounds[-1]
        self.r0, self.r1 = self.bounds[rank], self.bounds[rank + 1]
        self.lens = [self.bounds[g + 1] - self.bounds[g] for g in range(world)]
        self.timing = False
        self._per_step, self._ev = launches_per_step, []

    def _launch(self, local, x, out, *args):
        "local(x, out, *args), timed when `timing` is set"
        if not (self.timing and out.is_cuda):
            return local(x, out, *args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        local(x, out, *args)
        e1.record()
        self._ev.append((e0, e1))

    def compute_ms(self):
        "mean device time per step of the local products over the steps timed so far (call after a synchronize)"
        ev, self._ev = self._ev, []
        if not ev:
            return 0.0
        return sum(a.elapsed_time(b) for a, b in ev) * self._per_step / len(ev)


class _Exchange:
    """
    One exchange that completes `dst` -- a full-height [nrows] or [nrows x w] float64 tensor, possibly a strided column
    block -- on every rank of `part` (a _RowPartition).  The local product writes this rank's rows into `out`
    (contiguous); prepare() goes before that product, finish() after it: the one collective, then the rows into dst.
    """

    def __init__(self, part, mode, dst):
        self.part, self.mode, self.dst = part, mode, dst
        bounds, lens = part.bounds, part.lens
        whole = dst.is_contiguous()
        if mode == 'allgather':
            # this rank's rows padded to the longest rank's: ONE all_gather_into_tensor, then the unpadded pieces go
            # into dst by one concatenation (or, into a column block, one strided copy each)
            m = max(lens)
            self.loc = dst.new_zeros((m,) + dst.shape[1:])
            self.gath = dst.new_zeros((part.world * m,) + dst.shape[1:])
            self.out = self.loc[:part.r1 - part.r0]
            pieces = [(dst[bounds[g]:bounds[g + 1]], self.gath[g * m:g * m + lens[g]])
                      for g in range(part.world) if lens[g]]
            self.cat = [p for _, p in pieces] if whole else []
            self.copies = [] if whole else pieces
        else:
            # every rank's rows of a full-height buffer (dst itself when it is contiguous), as the output list of ONE
            # all_gather (RCCL: a group of broadcasts when the lengths differ; gloo only takes equal ones), or summed
            # by ONE all_reduce after the other ranks' rows were zeroed
            self.full = dst if whole else dst.new_zeros(dst.shape)
            self.views = [self.full[bounds[g]:bounds[g + 1]] for g in range(part.world)]
            self.out = self.views[part.rank]

    def prepare(self):
        "allreduce: zero what the previous step left in the other ranks' rows"
        if self.mode == 'allreduce':
            p = self.part
            if p.r0 > 0:
                self.full[:p.r0].zero_()
            if p.r1 < p.nrows:
                self.full[p.r1:].zero_()

    def finish(self):
        group = self.part.group
        if self.mode == 'allgather':
            dist.all_gather_into_tensor(self.gath, self.loc, group=group)
            if self.cat:
                torch.cat(self.cat, out=self.dst)
            for d, p in self.copies:
                d.copy_(p)
            return
        if self.mode == 'allgatherv':
            dist.all_gather(self.views, self.out, group=group)
        else:
            dist.all_reduce(self.full, op=dist.ReduceOp.SUM, group=group)
        if self.full is not self.dst:
            self.dst.copy_(self.full)


class RowPartitionedSpMV(_RowPartition):
    def __init__(self, bounds, rank, world, local_spmv, device, mode='allgather', group=None):
        """
        bounds: world+1 row indices (rank g owns rows bounds[g]:bounds[g+1]).
        local_spmv(x, out): computes this rank's rows into `out` (a float64 tensor of
        bounds[rank+1]-bounds[rank] entries on `device`); asynchronous on the current stream.
        """
        assert mode in _MODES
        super().__init__(bounds, rank, world, group, 1)
        self.mode = mode
        self.local_spmv = local_spmv
        self.y = torch.zeros(self.nrows, dtype=torch.float64, device=device)
        self._ex = _Exchange(self, mode, self.y) if world > 1 else None

    def step(self, x):
        "y = A x, complete on every rank; returns the (reused) y tensor"
        if self.world == 1:
            self._launch(self.local_spmv, x, self.y)
            return self.y
        self._ex.prepare()
        self._launch(self.local_spmv, x, self._ex.out)
        self._ex.finish()
        return self.y


def _sync_if_host_backend(t, group):
    """
    gloo (the CPU tests, and bench.py's two-ranks-on-one-GPU test hook) sends device tensors from the host without
    waiting for the stream that produces them: wait here.  RCCL orders a send after the producing kernels by itself.
    """
    if t.is_cuda and dist.get_backend(group) == 'gloo':
        torch.cuda.synchronize(t.device)


class SplitPhaseRowPartitionedSpMV(_RowPartition):
    """
    The exchange hidden behind the part of the product that touches few rows.  A rank's SpMV has two parts
    (csrk_spmv_device_part): part 1 computes every row of the row-major path and writes 0.0 into the rows the plan
    cut out for its tiers -- a few thousand long rows holding most of the entries --, part 2 computes those rows.
    So: part 1, then the slice is sent to every peer (point to point, straight into y: one
    grouped batch_isend_irecv) WHILE part 2 runs, and afterwards the cut rows' values -- a few KB per rank -- follow
    in one small all-gather and are written over the stale entries on every rank.  (The big send may read a cut
    row's entry before or after part 2 stores it; either way the small exchange overwrites it with the final value.)
    No extra handles, x is read once per kernel as in the plain product.

    local_part(x, out, part): this rank's rows, part 1 / 2 (asynchronous on the current stream);
    cut_rows: ascending int64 LOCAL row indices part 2 writes (may be empty), on `device`.
    """

    def __init__(self, bounds, rank, world, local_part, cut_rows, device, group=None):
        super().__init__(bounds, rank, world, group, 2)
        self.local_part = local_part
        self.y = torch.zeros(self.nrows, dtype=torch.float64, device=device)
        self.ops = []
        mine = self.y[self.r0:self.r1]
        for d in range(1, world):
            to, frm = (rank + d) % world, (rank - d) % world
            if self.r1 > self.r0:
                self.ops.append(dist.P2POp(dist.isend, mine, to, group))
            if self.lens[frm]:
                self.ops.append(dist.P2POp(dist.irecv, self.y[self.bounds[frm]:self.bounds[frm + 1]], frm, group))
        # the cut rows of every rank, as global row indices: exchanged once
        cut = cut_rows.to(device=device, dtype=torch.int64) + self.r0
        n_mine = int(cut.numel())
        counts = torch.zeros(world, dtype=torch.int64, device=device)
        counts[rank] = n_mine
        if world > 1:
            dist.all_reduce(counts, group=group)
        counts = [int(c) for c in counts.tolist()]
        self.n_mine, self.maxn = n_mine, max(max(counts), 1)
        self.total_cut = sum(counts)
        self.my_rows = cut
        self.hv_loc = torch.zeros(self.maxn, dtype=torch.float64, device=device)
        self.hv_all = torch.zeros(world * self.maxn, dtype=torch.float64, device=device)
        if world > 1 and self.total_cut:
            pad = torch.zeros(self.maxn, dtype=torch.int64, device=device)
            pad[:n_mine] = cut
            rows_all = torch.zeros(world * self.maxn, dtype=torch.int64, device=device)
            dist.all_gather_into_tensor(rows_all, pad, group=group)
            src = [torch.arange(g * self.maxn, g * self.maxn + counts[g], device=device) for g in range(world) if g != rank]
            self.src_pos = torch.cat(src) if src else torch.zeros(0, dtype=torch.int64, device=device)
            self.dst_rows = rows_all.index_select(0, self.src_pos)
            self.tmp = torch.zeros(int(self.src_pos.numel()), dtype=torch.float64, device=device)

    def step(self, x):
        "y = A x, complete on every rank; returns the (reused) y tensor"
        mine = self.y[self.r0:self.r1]
        self._launch(self.local_part, x, mine, 1)
        works = []
        if self.ops:                    # (none with one rank)
            _sync_if_host_backend(self.y, self.group)
            works = dist.batch_isend_irecv(self.ops)
        self._launch(self.local_part, x, mine, 2)
        if self.world > 1 and self.total_cut:
            if self.n_mine:
                torch.index_select(self.y, 0, self.my_rows, out=self.hv_loc[:self.n_mine])
        for w in works:
            w.wait()
        if self.world > 1 and self.total_cut:
            dist.all_gather_into_tensor(self.hv_all, self.hv_loc, group=self.group)
            if self.tmp.numel():
                torch.index_select(self.hv_all, 0, self.src_pos, out=self.tmp)
                self.y.index_copy_(0, self.dst_rows, self.tmp)
        return self.y


class RowPartitionedSpMM(_RowPartition):
    """
    C = A B, B dense row-major [ncols x k] float64, row-partitioned like RowPartitionedSpMV; C [nrows x k] is complete
    and identical on every rank after step().

    local_spmm(B, out, c0, c1): writes A[r0:r1, :] @ B[:, c0:c1] into `out`, a float64 [r1 - r0 x (c1 - c0)] view on
    `device` whose row stride may exceed its width; asynchronous on the current stream.

    The modes are RowPartitionedSpMV's, on row slabs of C (allgatherv: gloo only takes equal slabs; RCCL also takes
    unequal ones).  col_block=kb: ceil(k / kb) column blocks, each exchanged on a second stream while the next block's
    product runs on the caller's; None: one block.  Every block has buffers of its own, so block j + 1's product never
    writes what block j's collective still reads.  The exchange runs whenever a process group is initialised (also with
    one rank, so that a one-rank job rehearses it); without one, the product writes straight into C.
    """

    def __init__(self, bounds, rank, world, local_spmm, device, k, mode='allgather', col_block=None, group=None):
        assert mode in _MODES and int(k) >= 0 and (col_block is None or int(col_block) >= 1)
        self.k = k = int(k)
        kb = k if col_block is None else min(int(col_block), max(k, 1))
        self.col_block = col_block
        self.blocks = [(c0, min(c0 + kb, k)) for c0 in range(0, k, max(kb, 1))]
        super().__init__(bounds, rank, world, group, len(self.blocks))
        self.mode = mode
        self.local_spmm = local_spmm
        self.device = torch.device(device)
        self.exchange = world > 1 or (dist.is_available() and dist.is_initialized())
        self.C = torch.zeros(self.nrows, k, dtype=torch.float64, device=self.device)
        self.comm = torch.cuda.Stream(self.device) if self.device.type == 'cuda' else None
        self._ex = [_Exchange(self, mode, self.C if len(self.blocks) == 1 else self.C[:, c0:c1])
                    for c0, c1 in self.blocks] if self.exchange else []

    def recv_bytes(self):
        """
        bytes this rank receives per step, by the exchange's own arithmetic (allreduce: a ring, 2 (world - 1) / world of
        the panel; RCCL may pick another algorithm)
        """
        if not self.exchange or self.world == 1:
            return 0
        if self.mode == 'allgather':
            return (self.world - 1) * max(self.lens) * self.k * 8
        if self.mode == 'allgatherv':
            return (self.nrows - (self.r1 - self.r0)) * self.k * 8
        return int(2 * (self.world - 1) * self.nrows * self.k * 8 // self.world)

    def step(self, B):
        "C = A B, complete on every rank; returns the (reused) C tensor"
        if not self.exchange:
            for c0, c1 in self.blocks:
                self._launch(self.local_spmm, B, self.C[self.r0:self.r1, c0:c1], c0, c1)
            return self.C
        cur = torch.cuda.current_stream(self.device) if self.comm is not None else None
        for (c0, c1), ex in zip(self.blocks, self._ex):
            ex.prepare()
            self._launch(self.local_spmm, B, ex.out, c0, c1)
            _sync_if_host_backend(ex.out, self.group)
            if cur is None:
                ex.finish()
                continue
            self.comm.wait_stream(cur)
            with torch.cuda.stream(self.comm):
                ex.finish()
        if cur is not None:
            cur.wait_stream(self.comm)
        return self.C


def _stream(t):
    "torch's current stream on t's device, as the hipStream_t libcsrk takes"
    return torch.cuda.current_stream(t.device).cuda_stream


def hip_local_spmv(handle):
    """
    local_spmv callable over a libcsrk handle (csrk_spmv_device on torch's current stream).
    `handle` is the raw csrk_handle_t (int) of this rank's row range.
    """
    def run(x, out):
        assert x.dtype == torch.float64 and out.dtype == torch.float64 and out.is_contiguous()
        check(lib.csrk_spmv_device(handle, x.data_ptr(), out.data_ptr(), _stream(out)))
    return run


def hip_local_spmv_parts(handle, device):
    """
    (local_part, cut_rows) over a libcsrk handle for SplitPhaseRowPartitionedSpMV: csrk_spmv_device_part on torch's
    current stream, and the plan's cut rows (csrk_spmv_cut_rows: builds the plan) as an int64 tensor on `device`.
    """
    def run(x, out, part):
        assert x.dtype == torch.float64 and out.dtype == torch.float64 and out.is_contiguous()
        check(lib.csrk_spmv_device_part(handle, x.data_ptr(), out.data_ptr(), _stream(out), int(part)))

    n = C.c_int64(0)
    check(lib.csrk_spmv_cut_rows(handle, None, 0, C.byref(n)))
    rows = torch.zeros(max(n.value, 1), dtype=torch.int32, device=device)
    if n.value:
        check(lib.csrk_spmv_cut_rows(handle, rows.data_ptr(), n.value, C.byref(n)))
    return run, rows[:n.value].to(torch.int64)


def hip_local_spmm(handle):
    """
    local_spmm callable over a libcsrk handle for RowPartitionedSpMM: csrk_spmm_dense_device on torch's current stream,
    B[:, c0:c1] addressed in place (d_B = column c0 of B, ldb = B's row stride) into `out` (ldc = its row stride).
    Any column offset, ldb and ldc: a block that is not 16-B aligned (odd c0, odd ldb or ldc) takes the kernels' 8-B
    loads and stores (csrk.h), with the same bits.
    `handle` is the raw csrk_handle_t (int) of this rank's row range.
    """
    nr, nc, nnz = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    p64, vt = C.c_int(0), C.c_int(0)
    check(lib.csrk_info(handle, C.byref(nr), C.byref(nc), C.byref(nnz), C.byref(p64), C.byref(vt)))
    nrows, ncols = nr.value, nc.value

    def run(B, out, c0, c1):
        assert B.dtype == torch.float64 and out.dtype == torch.float64 and B.is_cuda and out.is_cuda
        assert B.dim() == 2 and out.dim() == 2 and 0 <= c0 <= c1 <= B.shape[1]
        assert B.shape[0] == ncols and tuple(out.shape) == (nrows, c1 - c0), (tuple(B.shape), tuple(out.shape), nrows, ncols)
        w = c1 - c0
        if nrows == 0 or w == 0:
            return
        assert B.stride(1) == 1 or B.shape[1] == 1, 'B rows must be contiguous'
        assert out.stride(1) == 1 or w == 1, 'rows of out must be contiguous'
        ldb = B.stride(0) if ncols > 1 else max(B.stride(0), B.shape[1])
        ldc = out.stride(0) if nrows > 1 else max(out.stride(0), w)
        assert ldb >= B.shape[1] and ldc >= w
        check(lib.csrk_spmm_dense_device(handle, B.data_ptr() + c0 * 8, w, ldb, out.data_ptr(), ldc, _stream(out)))
    return run
