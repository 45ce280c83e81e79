"""
The row-partitioned dense-panel SpMM on the GPU (csr_amd.dist.RowPartitionedSpMM, hip_local_spmm).

1. One GPU, no collective: column blocks of the panel through csrk_spmm_dense_device (d_B at column c0, ldb = the
   panel's row stride, C written into a strided view) equal one full-width call on the same handle bit for bit -- for
   the register-accumulator (heavy-row) plan and the plan without it, block widths 16, 8, 24 and 5 (odd column offsets:
   the 8-B load path), an output wider than k, and an odd ldb.
2. One rank on RCCL: tools/bench_spmm_dist.py --force-dist, every mode with and without column blocks; the exchanged C
   equals the plain product bit for bit.
3. Two ranks sharing one GPU over gloo on device tensors: every rank's C is the concatenation of the two HIP slabs, and
   within 1e-12 of sum |a||b| of one full-matrix product.
Every GPU process is a child under a time limit; at most two hold the GPU at once.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'bench_spmm_dist.py')


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    env.update(extra)
    return env


def _column_blocks_case(heavy):
    "child process body of test 1 (CSRK_SPMM_HEAVY decides the plan of the handle)"
    import ctypes as C

    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from csr_amd import synth
    from csr_amd._lib import lib, check, handle_t
    from csr_amd.dist import hip_local_spmm
    from oracle import oracle as O

    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    check(lib.csrk_set_device(0))
    n, nc, nnz, k = 60_000, 50_000, 1_500_000, 64
    m = synth.powerlaw_csr(n, nc, nnz, device=dev, max_degree=20_000)
    h = handle_t(0)
    check(lib.csrk_create_device(n, nc, int(m['colinds'].numel()), m['rowptrs'].data_ptr(), 0, m['colinds'].data_ptr(),
                                 m['values'].data_ptr(), 2, C.byref(h)))
    try:
        run = hip_local_spmm(h.value)
        B = synth.dense_vector(nc * k, device=dev, stream=7).view(nc, k)

        def blocked(width, Cout):
            for c0 in range(0, k, width):
                c1 = min(c0 + width, k)
                run(B, Cout[:, c0:c1], c0, c1)
            return Cout

        def same(a, b):
            torch.cuda.synchronize()
            return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))

        c16 = blocked(16, torch.full((n, k), float('nan'), dtype=torch.float64, device=dev))      # k = 16 first ...
        full = torch.full((n, k), float('nan'), dtype=torch.float64, device=dev)
        run(B, full, 0, k)                                                                     # ... then k = 64
        st = (C.c_int64 * 9)()
        check(lib.csrk_spmm_plan_stats(h, C.cast(st, C.c_void_p), 9))
        assert st[0] == (1 if heavy else 0), list(st)
        assert same(c16, full), 'blocks of 16'
        for width in (8, 24, 5):       # (5: blocks start at odd columns -- B not 16-B aligned -- and C rows likewise)
            assert same(blocked(width, torch.full((n, k), float('nan'), dtype=torch.float64, device=dev)), full), width
        assert same(blocked(16, torch.full((n, k), float('nan'), dtype=torch.float64, device=dev)), full), 'k alternates'
        wide = torch.full((n, k + 8), float('nan'), dtype=torch.float64, device=dev)
        run(B, wide[:, :k], 0, k)                        # ldc = 72
        assert same(wide[:, :k], full) and bool(torch.isnan(wide[:, k:]).all()), 'ldc > k'
        wide.fill_(float('nan'))
        run(B, wide[:, 1:k + 1], 0, k)                   # ldc = 72, C rows at odd columns
        assert same(wide[:, 1:k + 1], full) and bool(torch.isnan(wide[:, 0]).all()) and bool(torch.isnan(wide[:, k + 1:]).all())
        b65 = torch.zeros(nc, k + 1, dtype=torch.float64, device=dev)
        b65[:, :k] = B
        out = torch.full((n, k), float('nan'), dtype=torch.float64, device=dev)
        run(b65[:, :k], out, 0, k)                       # ldb = 65 (odd)
        assert same(out, full), 'odd ldb'
        # and the product itself: the rows holding the first 200 000 entries against the oracle
        rp = m['rowptrs'].cpu().numpy()
        r = int(np.searchsorted(rp, 200_000))
        e = int(rp[r])
        ci, vs, Bh = m['colinds'][:e].cpu().numpy(), m['values'][:e].cpu().numpy(), B.cpu().numpy()
        ref = O.spmm_dense(r, rp[:r + 1], ci, vs, Bh)
        bound = O.spmm_dense(r, rp[:r + 1], ci, np.abs(vs), np.abs(Bh))
        assert np.all(np.abs(full[:r].cpu().numpy() - ref) <= 1e-12 * bound + 1e-300)
    finally:
        check(lib.csrk_free(h))
    print('column blocks ok', flush=True)


@pytest.mark.gpu
@pytest.mark.parametrize('heavy', [1, 0])
def test_spmm_column_blocks_equal_full_width(heavy):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), 'column_blocks', str(heavy)], cwd=ROOT,
                         env=_env(CSRK_SPMM_HEAVY=str(heavy)), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    assert 'column blocks ok' in out.stdout


def _tool(args, timeout):
    out = subprocess.run([sys.executable, TOOL] + args, cwd=ROOT, env=_env(), capture_output=True, text=True,
                         timeout=timeout)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{')][-1])


@pytest.mark.gpu
def test_spmm_one_rank_on_rccl():
    d = _tool(['--force-dist', '--scale', '0.05', '--steps', '3', '--warmup', '1', '--blocks', 'none,16',
               '--child-timeout', '400'], timeout=480)
    assert d['world'] == 1 and d['exchange'] is True and d['backend'] == 'nccl'
    got = {(r['mode'], r['col_block']) for r in d['results']}
    assert got == {(m, b) for m in ('allgather', 'allgatherv', 'allreduce') for b in (None, 16)}
    for r in d['results']:
        # the exchanged C is the plain product of the same handle, bit for bit, and the oracle's to 1e-12
        assert r['complete'] and r['slab_exact'] and r['parity'], r
        assert r['local_ms'][0] > 0 and r['step_ms'][0] > 0


@pytest.mark.gpu
def test_spmm_two_ranks_share_one_gpu_over_gloo():
    d = _tool(['--gpus', '2', '--share-gpu', '--backend', 'gloo', '--scale', '0.02', '--steps', '2', '--warmup', '1',
               '--blocks', 'none,16', '--modes', 'allgather,allreduce', '--full-check', '--child-timeout', '400'],
              timeout=480)
    assert d['world'] == 2 and d['backend'] == 'gloo'
    for r in d['results']:
        # complete: both ranks hold the same bytes; slab_exact: each rank's rows are its own HIP product, bit for bit --
        # so C is the concatenation of the two slabs
        assert r['complete'] and r['slab_exact'] and r['parity'], r
        assert len(r['recv_bytes']) == 2 and min(r['recv_bytes']) > 0
    assert d['full_matrix_parity'] is True


if __name__ == '__main__':
    if sys.argv[1] == 'column_blocks':
        _column_blocks_case(int(sys.argv[2]))
