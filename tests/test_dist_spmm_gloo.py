"""
csr_amd.dist.RowPartitionedSpMM on CPU: world-2 and world-3 gloo process groups run the row partition, the three
exchanges and the column blocks of the dense-panel product C = A B.  The per-rank product is the oracle's
(oracle.spmm_dense on the rank's rows; the HIP kernels are covered by tests/test_gpu_dist_spmm.py), so this checks
what the distributed form adds: the padded all-gather / the all-gather of slabs / the all-reduce, the blocks of
columns (k = 37: blocks of 16 and of 5 leave a short last block) and their strided copies into C.
"""
import os

import numpy as np
import pytest
import torch

from gloo_harness import spawn

NROWS, NCOLS, NNZ, K = 3000, 2500, 40000, 37
BLOCKS = [None, 16, 5]


def _matrix(kind):
    "(nrows, ncols, rowptrs, colinds, values) as numpy arrays"
    if kind == 'powerlaw':
        from csr_amd import synth
        m = synth.powerlaw_csr(NROWS, NCOLS, NNZ, device='cpu')
        return NROWS, NCOLS, m['rowptrs'].numpy(), m['colinds'].numpy(), m['values'].numpy()
    # one row holds almost every entry: nnz-balanced bounds give a middle rank no rows at all
    lens = np.array([600, 1, 1, 1, 1, 0, 1, 1], dtype=np.int64)
    rp = np.zeros(len(lens) + 1, dtype=np.int32)
    rp[1:] = np.cumsum(lens)
    rng = np.random.default_rng(5)
    ci = np.concatenate([np.sort(rng.choice(NCOLS, size=int(n), replace=False)) for n in lens]).astype(np.int32)
    vs = rng.uniform(-1.0, 1.0, size=int(rp[-1]))
    return len(lens), NCOLS, rp, ci, vs


def _panel(ncols):
    from csr_amd import synth
    return synth.dense_vector(ncols * K, device='cpu', stream=7).view(ncols, K)


def _bounds(kind, rp, nrows, world, equal):
    if equal:
        return [nrows * g // world for g in range(world + 1)]
    from csr_amd import synth
    return synth.balanced_row_ranges(torch.from_numpy(rp.astype(np.int64)), world)


def _worker(rank, world, kind, mode, equal, out_dir):
    from csr_amd.dist import RowPartitionedSpMM
    from oracle import oracle as O
    nrows, ncols, rp, ci, vs = _matrix(kind)
    B = _panel(ncols)
    bounds = _bounds(kind, rp, nrows, world, equal)
    a, b = bounds[rank], bounds[rank + 1]
    lrp = rp[a:b + 1] - rp[a]
    lci, lvs = ci[rp[a]:rp[b]], vs[rp[a]:rp[b]]

    def local_spmm(Bt, out, c0, c1):
        assert tuple(out.shape) == (b - a, c1 - c0)
        out.copy_(torch.from_numpy(O.spmm_dense(b - a, lrp, lci, lvs, Bt[:, c0:c1].numpy())))

    for cb in BLOCKS:
        op = RowPartitionedSpMM(bounds, rank, world, local_spmm, 'cpu', K, mode=mode, col_block=cb)
        c1 = op.step(B).clone()
        assert torch.equal(c1, op.step(B))          # buffers are reused: a second step gives the same bytes
        np.save(os.path.join(out_dir, f'c_{cb}_{rank}.npy'), c1.numpy())
    np.save(os.path.join(out_dir, f'bounds_{rank}.npy'), np.array(bounds))


def _check(tmp_path, world, kind):
    from oracle import oracle as O
    nrows, ncols, rp, ci, vs = _matrix(kind)
    ref = O.spmm_dense(nrows, rp, ci, vs, _panel(ncols).numpy())
    for r in range(world):
        for cb in BLOCKS:
            c = np.load(tmp_path / f'c_{cb}_{r}.npy')
            # the same per-row recurrence on disjoint slabs: every rank holds the single-process C, bit for bit, for
            # every column blocking
            assert c.shape == (nrows, K)
            assert np.array_equal(c.view(np.int64), ref.view(np.int64)), (r, cb)
    return [np.load(tmp_path / f'bounds_{r}.npy') for r in range(world)]


@pytest.mark.parametrize('world', [2, 3])
@pytest.mark.parametrize('mode', ['allgather', 'allreduce'])
def test_row_partitioned_spmm_gloo(tmp_path, world, mode):
    spawn(_worker, world, 'powerlaw', mode, False, str(tmp_path))
    b = _check(tmp_path, world, 'powerlaw')[0]
    assert b[0] == 0 and b[-1] == NROWS and np.all(np.diff(b) > 0)


def test_row_partitioned_spmm_allgatherv_gloo(tmp_path):
    "the slabs themselves as the output list of one all_gather (equal slabs: gloo; RCCL also takes unequal ones)"
    spawn(_worker, 2, 'powerlaw', 'allgatherv', True, str(tmp_path))
    _check(tmp_path, 2, 'powerlaw')


@pytest.mark.parametrize('mode', ['allgather', 'allreduce'])
def test_row_partitioned_spmm_rank_without_rows(tmp_path, mode):
    "a world larger than the rows that hold the entries: the middle rank owns no rows and still takes part"
    spawn(_worker, 3, 'one_heavy_row', mode, False, str(tmp_path))
    b = _check(tmp_path, 3, 'one_heavy_row')[0]
    assert b[2] - b[1] == 0 and b[1] - b[0] > 0 and b[3] - b[2] > 0


def test_spmm_blocks_and_recv_bytes_without_process_group():
    "no process group: the product writes its column blocks straight into C (strided views); nothing is exchanged"
    from csr_amd.dist import RowPartitionedSpMM
    from oracle import oracle as O
    nrows, ncols, rp, ci, vs = _matrix('powerlaw')
    B = _panel(ncols)
    seen = []

    def local_spmm(Bt, out, c0, c1):
        seen.append((c0, c1, out.stride(0)))
        out.copy_(torch.from_numpy(O.spmm_dense(nrows, rp, ci, vs, Bt[:, c0:c1].numpy())))

    op = RowPartitionedSpMM([0, nrows], 0, 1, local_spmm, 'cpu', K, col_block=16)
    assert op.blocks == [(0, 16), (16, 32), (32, 37)] and op.recv_bytes() == 0
    c = op.step(B)
    assert seen == [(0, 16, K), (16, 32, K), (32, 37, K)]
    ref = O.spmm_dense(nrows, rp, ci, vs, B.numpy())
    assert np.array_equal(c.numpy().view(np.int64), ref.view(np.int64))
