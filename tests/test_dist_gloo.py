"""
The N>1 path on CPU: world_size-2 (and 3) gloo process groups exercise the row partition and
both exchange modes of csr_amd.dist.RowPartitionedSpMV.  The per-rank product is computed by
the oracle here (the HIP kernels need a GPU; they are covered by the -m gpu tests), so this
checks exactly what a multi-GPU run adds: the split points, the padded all-gather / the
all-reduce, and the reassembly.
"""
import os

import numpy as np
import pytest
import torch

from gloo_harness import spawn


def _worker(rank, world, mode, out_dir):
    from csr_amd import synth
    from csr_amd.dist import RowPartitionedSpMV
    from oracle import oracle as O
    nrows, ncols, nnz = 6000, 5000, 90000
    shard = synth.powerlaw_csr(nrows, ncols, nnz, device='cpu', rank=rank, world=world)
    x = synth.dense_vector(ncols, device='cpu')
    rp, ci, vs = (shard[k].numpy() for k in ('rowptrs', 'colinds', 'values'))
    n_loc = shard['row_end'] - shard['row_begin']

    def local_spmv(xt, out):
        out.copy_(torch.from_numpy(O.mult_vec(n_loc, ncols, rp, ci, vs, xt.numpy())))

    op = RowPartitionedSpMV(shard['bounds'], rank, world, local_spmv, 'cpu', mode=mode)
    y1 = op.step(x).clone()
    y2 = op.step(x).clone()          # buffers are reused: a second step must agree
    assert torch.equal(y1, y2)
    np.save(os.path.join(out_dir, f'y_{mode}_{rank}.npy'), y1.numpy())
    np.save(os.path.join(out_dir, f'bounds_{rank}.npy'), np.array(shard['bounds']))


@pytest.mark.parametrize('world', [2, 3])
@pytest.mark.parametrize('mode', ['allgather', 'allreduce'])
def test_row_partitioned_spmv_gloo(tmp_path, world, mode):
    from csr_amd import synth
    from oracle import oracle as O
    spawn(_worker, world, mode, str(tmp_path))
    full = synth.powerlaw_csr(6000, 5000, 90000, device='cpu')
    x = synth.dense_vector(5000, device='cpu').numpy()
    ref = O.mult_vec(6000, 5000, full['rowptrs'].numpy(), full['colinds'].numpy(), full['values'].numpy(), x)
    for r in range(world):
        y = np.load(tmp_path / f'y_{mode}_{r}.npy')
        # disjoint slices: every rank ends with the single-process result, bit for bit
        assert np.array_equal(y, ref)
        b = np.load(tmp_path / f'bounds_{r}.npy')
        assert b[0] == 0 and b[-1] == 6000 and np.all(np.diff(b) >= 0)
    # nnz balance of the split (searchsorted on rowptrs, csr/csr.py:609)
    rp = full['rowptrs'].numpy()
    per = [int(rp[b[g + 1]] - rp[b[g]]) for g in range(world)]
    assert max(per) - min(per) <= int(np.max(np.diff(rp))) + 1


def _worker_split(rank, world, out_dir):
    from csr_amd import synth
    from csr_amd.dist import SplitPhaseRowPartitionedSpMV
    from oracle import oracle as O
    nrows, ncols, nnz = 6000, 5000, 90000
    shard = synth.powerlaw_csr(nrows, ncols, nnz, device='cpu', rank=rank, world=world)
    x = synth.dense_vector(ncols, device='cpu')
    rp, ci, vs = (shard[k].numpy() for k in ('rowptrs', 'colinds', 'values'))
    n_loc = shard['row_end'] - shard['row_begin']
    lens = np.diff(rp)
    # the stand-in for the plan's tiers: rows of 40 entries and more (rank 1 of 3 keeps none: an empty list must work)
    cut = np.flatnonzero(lens >= 40) if not (world == 3 and rank == 1) else np.zeros(0, dtype=np.int64)
    is_cut = np.zeros(n_loc, dtype=bool)
    is_cut[cut] = True

    def local_part(xt, out, part):
        full = O.mult_vec(n_loc, ncols, rp, ci, vs, xt.numpy())
        o = out.numpy()
        if part == 1:
            o[:] = np.where(is_cut, 0.0, full)          # the cut rows get 0.0
        else:
            o[is_cut] = full[is_cut]                    # ... and are overwritten by part 2

    op = SplitPhaseRowPartitionedSpMV(shard['bounds'], rank, world, local_part, torch.from_numpy(cut.astype(np.int64)), 'cpu')
    y1 = op.step(x).clone()
    y2 = op.step(x).clone()
    assert torch.equal(y1, y2)
    np.save(os.path.join(out_dir, f'ys_{rank}.npy'), y1.numpy())


@pytest.mark.parametrize('world', [2, 3])
def test_split_phase_row_partitioned_spmv_gloo(tmp_path, world):
    "the slice travels while the cut rows are computed, their values follow in a small all-gather: the single-process y"
    from csr_amd import synth
    from oracle import oracle as O
    spawn(_worker_split, world, str(tmp_path))
    full = synth.powerlaw_csr(6000, 5000, 90000, device='cpu')
    x = synth.dense_vector(5000, device='cpu').numpy()
    ref = O.mult_vec(6000, 5000, full['rowptrs'].numpy(), full['colinds'].numpy(), full['values'].numpy(), x)
    for r in range(world):
        assert np.array_equal(np.load(tmp_path / f'ys_{r}.npy'), ref)


def _worker_equal(rank, world, out_dir):
    from csr_amd import synth
    from csr_amd.dist import RowPartitionedSpMV
    from oracle import oracle as O
    full = synth.powerlaw_csr(6000, 5000, 90000, device='cpu')
    x = synth.dense_vector(5000, device='cpu')
    rp, ci, vs = (full[k].numpy() for k in ('rowptrs', 'colinds', 'values'))
    bounds = [6000 * g // world for g in range(world + 1)]      # equal slices: the only kind gloo's all_gather takes
    a, b = bounds[rank], bounds[rank + 1]

    def local_spmv(xt, out):
        out.copy_(torch.from_numpy(O.mult_vec(b - a, 5000, rp[a:b + 1] - rp[a], ci[rp[a]:rp[b]], vs[rp[a]:rp[b]], xt.numpy())))

    op = RowPartitionedSpMV(bounds, rank, world, local_spmv, 'cpu', mode='allgatherv')
    y1 = op.step(x).clone()
    assert torch.equal(y1, op.step(x))
    np.save(os.path.join(out_dir, f'yv_{rank}.npy'), y1.numpy())


def test_allgatherv_mode_gloo(tmp_path):
    "the slices of y as the output list of one all_gather (equal slices here: gloo; RCCL also takes unequal ones)"
    from csr_amd import synth
    from oracle import oracle as O
    spawn(_worker_equal, 2, str(tmp_path))
    full = synth.powerlaw_csr(6000, 5000, 90000, device='cpu')
    x = synth.dense_vector(5000, device='cpu').numpy()
    ref = O.mult_vec(6000, 5000, full['rowptrs'].numpy(), full['colinds'].numpy(), full['values'].numpy(), x)
    for r in range(2):
        assert np.array_equal(np.load(tmp_path / f'yv_{r}.npy'), ref)


def test_one_rank_without_process_group():
    """
    world 1, no process group: RowPartitionedSpMV's step is exactly one local product, written straight into op.y (the
    single-GPU headline of bench.py times this path); compute_ms() of every operator is 0.0 when no launch was timed
    (CPU outputs record no events), and stays 0.0 after it reset
    """
    from csr_amd.dist import RowPartitionedSpMM, RowPartitionedSpMV, SplitPhaseRowPartitionedSpMV
    x = torch.ones(3, dtype=torch.float64)
    calls = []

    def local_spmv(xt, out):
        calls.append(out)
        out.fill_(len(calls))

    op = RowPartitionedSpMV([0, 4], 0, 1, local_spmv, 'cpu')
    assert op.compute_ms() == 0.0
    op.timing = True
    for s in range(1, 4):
        assert op.step(x) is op.y and len(calls) == s and calls[-1] is op.y
        assert torch.equal(op.y, torch.full((4,), float(s), dtype=torch.float64))
    assert op.compute_ms() == 0.0 and op.compute_ms() == 0.0

    split = SplitPhaseRowPartitionedSpMV([0, 4], 0, 1, lambda xt, out, part: out.fill_(part),
                                         torch.zeros(0, dtype=torch.int64), 'cpu')
    spmm = RowPartitionedSpMM([0, 4], 0, 1, lambda B, out, c0, c1: out.fill_(c0), 'cpu', 5, col_block=2)
    for o, arg in ((split, x), (spmm, torch.ones(3, 5, dtype=torch.float64))):
        o.timing = True
        o.step(arg)
        assert o.compute_ms() == 0.0 and o.compute_ms() == 0.0
    assert torch.equal(split.y, torch.full((4,), 2.0, dtype=torch.float64))
    assert torch.equal(spmm.C, torch.tensor([0.0, 0.0, 2.0, 2.0, 4.0], dtype=torch.float64).expand(4, 5))
