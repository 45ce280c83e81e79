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
product (csrk_spmv_device_part).  (Rounds 2-3 also carried chunk-pipelined, plain point-to-point and IPC-push forms; none
has ever run with two RCCL ranks, so they were removed: `git log -- csr_amd/dist.py`.)

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
import contextlib

import torch
import torch.distributed as dist


class RowPartitionedSpMV:
    def __init__(self, bounds, rank, world, local_spmv, device, mode='allgather', group=None):
        """
        bounds: world+1 row indices (rank g owns rows bounds[g]:bounds[g+1]).
        local_spmv(x, out): computes this rank's rows into `out` (a float64 tensor of
        bounds[rank+1]-bounds[rank] entries on `device`); asynchronous on the current stream.
        """
        assert len(bounds) == world + 1 and mode in ('allgather', 'allgatherv', 'allreduce')
        self.bounds = [int(b) for b in bounds]
        self.rank, self.world, self.mode, self.group = rank, world, mode, group
        self.local_spmv = local_spmv
        self.nrows = self.bounds[-1]
        self.r0, self.r1 = self.bounds[rank], self.bounds[rank + 1]
        self.lens = [self.bounds[g + 1] - self.bounds[g] for g in range(world)]
        self.y = torch.zeros(self.nrows, dtype=torch.float64, device=device)
        self.timing = False            # set True to record device events around the local product
        self._ev = []
        if world > 1 and mode == 'allgather':
            self.maxlen = max(self.lens)
            self.loc = torch.zeros(self.maxlen, dtype=torch.float64, device=device)
            self.gath = torch.zeros(world * self.maxlen, dtype=torch.float64, device=device)
            # the slices of `gath` that make up y, in rank order: unpadded by ONE concatenation kernel
            self.pieces = [self.gath[g * self.maxlen:g * self.maxlen + self.lens[g]] for g in range(world)
                           if self.lens[g]]

        if world > 1 and mode == 'allgatherv':
            # every rank's slice of y itself, as the output list of ONE all_gather: with slices of different lengths
            # RCCL runs it as a group of broadcasts straight into place (nothing padded, nothing concatenated);
            # gloo only takes equal lengths
            self.views = [self.y[self.bounds[g]:self.bounds[g + 1]] for g in range(world)]

    def _local(self, x, out):
        if self.timing and out.is_cuda:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.local_spmv(x, out)
            e1.record()
            self._ev.append((e0, e1))
        else:
            self.local_spmv(x, out)

    def compute_ms(self):
        "mean device time of the local product over the steps timed so far (call after a synchronize)"
        if not self._ev:
            return 0.0
        ms = sum(a.elapsed_time(b) for a, b in self._ev) / len(self._ev)
        self._ev = []
        return ms

    def step(self, x):
        "y = A x, complete on every rank; returns the (reused) y tensor"
        if self.world == 1:
            self._local(x, self.y)
            return self.y
        if self.mode == 'allgather':
            self._local(x, self.loc[:self.r1 - self.r0])
            dist.all_gather_into_tensor(self.gath, self.loc, group=self.group)
            if self.pieces:
                torch.cat(self.pieces, out=self.y)
            return self.y
        if self.mode == 'allgatherv':
            self._local(x, self.views[self.rank])
            dist.all_gather(self.views, self.views[self.rank], group=self.group)
            return self.y
        # allreduce: zero what the previous step left in the other ranks' slices
        if self.r0 > 0:
            self.y[:self.r0].zero_()
        if self.r1 < self.nrows:
            self.y[self.r1:].zero_()
        self._local(x, self.y[self.r0:self.r1])
        dist.all_reduce(self.y, op=dist.ReduceOp.SUM, group=self.group)
        return self.y


def _sync_if_host_backend(t, group):
    """
    gloo (the CPU tests, and bench.py's two-ranks-on-one-GPU test hook) sends device tensors from the host without
    waiting for the stream that produces them: wait here.  RCCL orders a send after the producing kernels by itself.
    """
    if t.is_cuda and dist.get_backend(group) == 'gloo':
        torch.cuda.synchronize(t.device)


class SplitPhaseRowPartitionedSpMV:
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
        assert len(bounds) == world + 1
        self.bounds = [int(b) for b in bounds]
        self.rank, self.world, self.group = rank, world, group
        self.local_part = local_part
        self.nrows = self.bounds[-1]
        self.r0, self.r1 = self.bounds[rank], self.bounds[rank + 1]
        self.y = torch.zeros(self.nrows, dtype=torch.float64, device=device)
        self.timing = False
        self._ev = []
        self.ops = []
        mine = self.y[self.r0:self.r1]
        for d in range(1, world):
            to, frm = (rank + d) % world, (rank - d) % world
            if self.r1 > self.r0:
                self.ops.append(dist.P2POp(dist.isend, mine, to, group))
            if self.bounds[frm + 1] > self.bounds[frm]:
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

    def compute_ms(self):
        "mean device time per step of the two local parts over the steps timed so far"
        if not self._ev:
            return 0.0
        ms = sum(a.elapsed_time(b) for a, b in self._ev) * 2 / len(self._ev)
        self._ev = []
        return ms

    def _part(self, x, out, part):
        if self.timing and out.is_cuda:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.local_part(x, out, part)
            e1.record()
            self._ev.append((e0, e1))
        else:
            self.local_part(x, out, part)

    def step(self, x):
        "y = A x, complete on every rank; returns the (reused) y tensor"
        mine = self.y[self.r0:self.r1]
        self._part(x, mine, 1)
        if self.world > 1 and self.ops:
            _sync_if_host_backend(self.y, self.group)
        works = dist.batch_isend_irecv(self.ops) if (self.world > 1 and self.ops) else []
        self._part(x, mine, 2)
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


def hip_local_spmv_parts(handle, device):
    """
    (local_part, cut_rows) over a libcsrk handle for SplitPhaseRowPartitionedSpMV: csrk_spmv_device_part on torch's
    current stream, and the plan's cut rows (csrk_spmv_cut_rows: builds the plan) as an int64 tensor on `device`.
    """
    import ctypes as C
    from ._lib import lib, check

    def run(x, out, part):
        assert x.dtype == torch.float64 and out.dtype == torch.float64 and out.is_contiguous()
        stream = torch.cuda.current_stream(out.device).cuda_stream
        check(lib.csrk_spmv_device_part(handle, x.data_ptr(), out.data_ptr(), stream, int(part)))

    n = C.c_int64(0)
    check(lib.csrk_spmv_cut_rows(handle, None, 0, C.byref(n)))
    rows = torch.zeros(max(n.value, 1), dtype=torch.int32, device=device)
    if n.value:
        check(lib.csrk_spmv_cut_rows(handle, rows.data_ptr(), n.value, C.byref(n)))
    return run, rows[:n.value].to(torch.int64)


def hip_local_spmv(handle):
    """
    local_spmv callable over a libcsrk handle (csrk_spmv_device on torch's current stream).
    `handle` is the raw csrk_handle_t (int) of this rank's row range.
    """
    from ._lib import lib, check

    def run(x, out):
        assert x.dtype == torch.float64 and out.dtype == torch.float64 and out.is_contiguous()
        stream = torch.cuda.current_stream(out.device).cuda_stream
        check(lib.csrk_spmv_device(handle, x.data_ptr(), out.data_ptr(), stream))
    return run


class RowPartitionedSpMM:
    """
    C = A B, B dense row-major [ncols x k] float64, row-partitioned like RowPartitionedSpMV; C [nrows x k] is complete
    and identical on every rank after step().

    local_spmm(B, out, c0, c1): writes A[r0:r1, :] @ B[:, c0:c1] into `out`, a float64 [r1 - r0 x (c1 - c0)] view on
    `device` whose row stride may exceed its width; asynchronous on the current stream.

    Modes, as in RowPartitionedSpMV:
      allgather  (default) the local slab is padded to the longest rank's rows, one all_gather_into_tensor moves the
                 padded slabs, and they are unpadded into C.
      allgatherv every rank's row slab (of C, or of the block's buffer) is an entry of the output list of one
                 all_gather: nothing padded.  gloo only takes equal slabs; RCCL also takes unequal ones.
      allreduce  the other ranks' rows are zeroed and the ranks sum: exact, the slabs being disjoint.
    col_block=kb: ceil(k / kb) column blocks, each exchanged on a second stream while the next block's product runs on
    the caller's; None: one block.  The exchange runs whenever a process group is initialised (also with one rank, so
    that a one-rank job rehearses it); without one, the product writes straight into C.
    """

    def __init__(self, bounds, rank, world, local_spmm, device, k, mode='allgather', col_block=None, group=None):
        assert len(bounds) == world + 1 and mode in ('allgather', 'allgatherv', 'allreduce')
        assert int(k) >= 0 and (col_block is None or int(col_block) >= 1)
        self.bounds = [int(b) for b in bounds]
        self.rank, self.world, self.mode, self.group = rank, world, mode, group
        self.local_spmm = local_spmm
        self.k = k = int(k)
        self.nrows = self.bounds[-1]
        self.r0, self.r1 = self.bounds[rank], self.bounds[rank + 1]
        self.lens = [self.bounds[g + 1] - self.bounds[g] for g in range(world)]
        self.device = torch.device(device)
        kb = k if col_block is None else min(int(col_block), max(k, 1))
        self.col_block = col_block
        self.blocks = [(c0, min(c0 + kb, k)) for c0 in range(0, k, max(kb, 1))]
        self.exchange = world > 1 or (dist.is_available() and dist.is_initialized())
        self.C = torch.zeros(self.nrows, k, dtype=torch.float64, device=self.device)
        self.timing = False            # set True to record device events around the local products
        self._ev = []
        self._steps = 0
        self.comm = torch.cuda.Stream(self.device) if self.device.type == 'cuda' else None
        one = len(self.blocks) == 1
        # per block: (the product's output, what the collective needs); every block has buffers of its own, so block
        # j + 1's product never writes what block j's collective still reads
        self.bufs = []
        if not self.exchange:
            return
        if mode == 'allgather':
            self.maxlen = m = max(self.lens)
            loc = torch.zeros(m * k, dtype=torch.float64, device=self.device)
            gath = torch.zeros(world * m * k, dtype=torch.float64, device=self.device)
            for c0, c1 in self.blocks:
                w = c1 - c0
                lj = loc[m * c0:m * c1].view(m, w)
                gj = gath[world * m * c0:world * m * c1].view(world * m, w)
                pieces = [(self.bounds[g], self.bounds[g + 1], gj[g * m:g * m + self.lens[g]])
                          for g in range(world) if self.lens[g]]
                self.bufs.append((lj[:self.r1 - self.r0], (lj, gj, pieces)))
        else:
            # allgatherv / allreduce: a full-height buffer per block (C itself when there is one block)
            flat = None if one else torch.zeros(self.nrows * k, dtype=torch.float64, device=self.device)
            for c0, c1 in self.blocks:
                yj = self.C if one else flat[self.nrows * c0:self.nrows * c1].view(self.nrows, c1 - c0)
                views = [yj[self.bounds[g]:self.bounds[g + 1]] for g in range(world)]
                self.bufs.append((views[rank], (yj, views)))

    def recv_bytes(self):
        """
        bytes this rank receives per step, by the exchange's own arithmetic (allreduce: a ring, 2 (world - 1) / world of
        the panel; RCCL may pick another algorithm)
        """
        if not self.exchange or self.world == 1:
            return 0
        if self.mode == 'allgather':
            return (self.world - 1) * self.maxlen * self.k * 8
        if self.mode == 'allgatherv':
            return (self.nrows - (self.r1 - self.r0)) * self.k * 8
        return int(2 * (self.world - 1) * self.nrows * self.k * 8 // self.world)

    def _local(self, B, out, c0, c1):
        if self.timing and out.is_cuda:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.local_spmm(B, out, c0, c1)
            e1.record()
            self._ev.append((e0, e1))
        else:
            self.local_spmm(B, out, c0, c1)

    def compute_ms(self):
        "mean device time per step of the local products (all blocks) over the steps timed so far (after a synchronize)"
        if not self._ev or not self._steps:
            self._ev, self._steps = [], 0
            return 0.0
        ms = sum(a.elapsed_time(b) for a, b in self._ev) / self._steps
        self._ev, self._steps = [], 0
        return ms

    def _exchange(self, j, out, aux):
        c0, c1 = self.blocks[j]
        whole = len(self.blocks) == 1
        if self.mode == 'allgather':
            lj, gj, pieces = aux
            dist.all_gather_into_tensor(gj, lj, group=self.group)
            if whole and pieces:
                torch.cat([p for _, _, p in pieces], out=self.C)
            else:
                for a, b, p in pieces:
                    self.C[a:b, c0:c1].copy_(p)
            return
        yj, views = aux
        if self.mode == 'allgatherv':
            dist.all_gather(views, views[self.rank], group=self.group)
        else:
            dist.all_reduce(yj, op=dist.ReduceOp.SUM, group=self.group)
        if not whole:
            self.C[:, c0:c1].copy_(yj)

    def step(self, B):
        "C = A B, complete on every rank; returns the (reused) C tensor"
        if self.timing:
            self._steps += 1
        if not self.exchange:
            for c0, c1 in self.blocks:
                self._local(B, self.C[self.r0:self.r1, c0:c1], c0, c1)
            return self.C
        cur = torch.cuda.current_stream(self.device) if self.comm is not None else None
        for j, (out, aux) in enumerate(self.bufs):
            c0, c1 = self.blocks[j]
            if self.mode == 'allreduce':
                # zero what the previous step left in the other ranks' rows
                yj = aux[0]
                if self.r0 > 0:
                    yj[:self.r0].zero_()
                if self.r1 < self.nrows:
                    yj[self.r1:].zero_()
            self._local(B, out, c0, c1)
            _sync_if_host_backend(out, self.group)
            if cur is None:
                self._exchange(j, out, aux)
                continue
            ready = torch.cuda.Event()
            ready.record(cur)
            self.comm.wait_event(ready)
            with torch.cuda.stream(self.comm):
                self._exchange(j, out, aux)
        if cur is not None:
            cur.wait_stream(self.comm)
        return self.C


def hip_local_spmm(handle):
    """
    local_spmm callable over a libcsrk handle for RowPartitionedSpMM: csrk_spmm_dense_device on torch's current stream,
    B[:, c0:c1] addressed in place (d_B = column c0 of B, ldb = B's row stride) into `out` (ldc = its row stride).
    Any column offset, ldb and ldc: a block that is not 16-B aligned (odd c0, odd ldb or ldc) takes the kernels' 8-B
    loads and stores (csrk.h), with the same bits.
    `handle` is the raw csrk_handle_t (int) of this rank's row range.
    """
    import ctypes as C
    from ._lib import lib, check
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
        stream = torch.cuda.current_stream(out.device).cuda_stream
        check(lib.csrk_spmm_dense_device(handle, B.data_ptr() + c0 * 8, w, ldb, out.data_ptr(), ldc, stream))
    return run
