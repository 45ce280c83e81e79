"""
Row-partitioned dense-panel SpMM across GPUs (csr_amd.dist.RowPartitionedSpMM over csrk_spmm_dense_device): every
exchange mode, with and without column blocks, on BASELINE configs[2] -- A 2M x 2M with 5e7 entries (power law,
max_degree 250 000), B dense [2M x 64] float64.

    python tools/bench_spmm_dist.py --gpus N            one rank per GPU over RCCL (child processes)
    python tools/bench_spmm_dist.py --force-dist        one rank on RCCL: the exchange path rehearsed on one GPU

The parent starts one child process per rank -- each under its own `timeout` -- and never touches the GPU itself.  A
child that fails ends the run: its status is reported, the others are stopped, nothing is retried.  Each rank builds
its own row range of the matrix (synth.powerlaw_csr(..., rank, world)), times every (mode, col_block) after a warm-up,
and checks:
  complete     every rank's C equals rank 0's bit for bit (checksums of the raw bytes, gathered);
  slab_exact   this rank's rows of C equal its plain full-width csrk_spmm_dense_device product bit for bit;
  parity       sampled rows of C against oracle.spmm_dense to 1e-12 of sum |a||b| (test_spmm_config3_full_size's bound).
Rank 0 prints one JSON line.  --share-gpu --backend gloo (test hook): all ranks on GPU 0 over gloo (RCCL refuses two
ranks on one device).  --scale shrinks the matrix (tests only: not a configs[2] result).
"""
import argparse
import json
import os
import signal
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODES = ('allgather', 'allgatherv', 'allreduce')


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--force-dist', action='store_true', help='one rank: run the exchange through RCCL anyway')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--k', type=int, default=64)
    ap.add_argument('--blocks', default='none,16,32', help='col_block settings, comma separated ("none": one block)')
    ap.add_argument('--modes', default=','.join(MODES))
    ap.add_argument('--scale', type=float, default=1.0, help='shrink the matrix (testing only; not a configs[2] result)')
    ap.add_argument('--backend', default='nccl', choices=['nccl', 'gloo'])
    ap.add_argument('--share-gpu', action='store_true', help='test hook: every rank on GPU 0 (needs --backend gloo)')
    ap.add_argument('--full-check', action='store_true',
                    help='rank 0 also compares C with one full-matrix product (1e-12 of sum |a||b|)')
    ap.add_argument('--child-timeout', type=int, default=900, help='seconds each rank may run')
    return ap.parse_args()


def launch(args):
    "the parent: one child per rank, each under its own time limit; the first failure ends the run"
    world = args.gpus
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r),
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        cmd = ['timeout', '-k', '10', str(args.child_timeout), sys.executable, os.path.abspath(__file__)] + sys.argv[1:]
        procs.append(subprocess.Popen(cmd, env=env, cwd=ROOT))
    status = [None] * world
    failed = None
    while any(s is None for s in status):
        for r, p in enumerate(procs):
            if status[r] is None:
                status[r] = p.poll()
                if status[r] not in (None, 0) and failed is None:
                    failed = r
        if failed is not None:
            break
        time.sleep(0.2)
    if failed is not None:
        for p in procs:
            if p.poll() is None:
                p.send_signal(signal.SIGTERM)
        for r, p in enumerate(procs):
            try:
                status[r] = p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                p.kill()
                status[r] = p.wait()
        why = {124: 'time limit', 137: 'killed after the time limit', 134: 'abort', 139: 'segmentation fault'}
        s = status[failed]
        print(f'[bench_spmm_dist] rank {failed} failed with status {s} ({why.get(s, "error")}); '
              f'statuses of all ranks: {status}; not retried', file=sys.stderr, flush=True)
        sys.exit(1)
    sys.exit(0)


def checksum(t):
    "order-sensitive checksum of a float64 tensor's raw bytes: two int64 sums (wrapping) over its bit patterns"
    import torch
    bits = t.contiguous().view(torch.int64).view(-1)
    w = torch.arange(bits.numel(), device=bits.device, dtype=torch.int64) % 65521 + 1
    return torch.stack([bits.sum(), (bits * w).sum()])


def rank_main(args):
    import ctypes as C
    import datetime

    import numpy as np
    import torch
    import torch.distributed as dist

    from csr_amd import synth
    from csr_amd._lib import lib, check, handle_t
    from csr_amd.dist import RowPartitionedSpMM, hip_local_spmm
    from oracle import oracle as O

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    if not torch.cuda.is_available():
        sys.exit('bench_spmm_dist.py needs an MI355X: no GPU is visible (the product has no CPU fallback)')
    dev_index = 0 if args.share_gpu else int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(dev_index)
    dev = torch.device('cuda', dev_index)
    check(lib.csrk_set_device(dev_index))
    distd = world > 1 or args.force_dist
    if distd:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if 'MASTER_PORT' not in os.environ:
            with socket.socket() as sk:
                sk.bind(('127.0.0.1', 0))
                os.environ['MASTER_PORT'] = str(sk.getsockname()[1])
        if args.backend == 'gloo':
            dist.init_process_group('gloo', rank=rank, world_size=world)
        else:
            # a collective that does not complete aborts the job after 5 minutes instead of holding the node
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev,
                                    timeout=datetime.timedelta(minutes=5))

    n = int(round(2_000_000 * args.scale))
    nnz = int(round(50_000_000 * args.scale))
    k = args.k
    shard = synth.powerlaw_csr(n, n, nnz, max_degree=250_000, device=dev, rank=rank, world=world)
    rp, ci, vs = shard['rowptrs'], shard['colinds'], shard['values']
    r0, r1 = shard['row_begin'], shard['row_end']
    n_loc = r1 - r0

    def handle(values):
        h = handle_t(0)
        check(lib.csrk_create_device(n_loc, n, int(ci.numel()), rp.data_ptr(), int(rp.dtype == torch.int64),
                                     ci.data_ptr(), values.data_ptr(), 2, C.byref(h)))
        return h

    h = handle(vs)
    B = synth.dense_vector(n * k, device=dev, stream=7).view(n, k)
    local = hip_local_spmm(h.value)

    # the plain full-width product of this rank's rows (the plan is built by this first call), and its time
    plain = torch.zeros(n_loc, k, dtype=torch.float64, device=dev)
    local(B, plain, 0, k)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.warmup):
        local(B, plain, 0, k)
    e0.record()
    for _ in range(args.steps):
        local(B, plain, 0, k)
    e1.record()
    torch.cuda.synchronize()
    plain_ms = e0.elapsed_time(e1) / max(args.steps, 1)
    plan = (C.c_int64 * 9)()
    check(lib.csrk_spmm_plan_stats(h, C.cast(plan, C.c_void_p), 9))

    # parity sample: the rows holding the slab's first ~200 000 entries, its 3 longest rows and 64 rows spread over it
    rp_h = rp.cpu().numpy().astype(np.int64)
    lens = np.diff(rp_h)
    head = int(np.searchsorted(rp_h, min(200_000, int(rp_h[-1]))))
    rows = np.unique(np.concatenate([np.arange(head), np.argsort(lens, kind='stable')[-3:],
                                     np.linspace(0, max(n_loc - 1, 0), 64).astype(np.int64)])) if n_loc else np.zeros(0, np.int64)
    ci_h, vs_h = ci.cpu().numpy(), vs.cpu().numpy()
    srp = np.zeros(len(rows) + 1, dtype=np.int64)
    srp[1:] = np.cumsum(lens[rows]) if len(rows) else []
    sel = np.concatenate([np.arange(rp_h[r], rp_h[r + 1]) for r in rows]) if len(rows) else np.zeros(0, np.int64)
    B_h = B.cpu().numpy()
    ref = O.spmm_dense(len(rows), srp, ci_h[sel], vs_h[sel], B_h)
    bound = O.spmm_dense(len(rows), srp, ci_h[sel], np.abs(vs_h[sel]), np.abs(B_h))
    del B_h
    rows_t = torch.from_numpy(rows + r0).to(dev)

    def gather_floats(vals):
        t = torch.tensor(vals, dtype=torch.float64, device=dev)
        if not distd:
            return [t.tolist()]
        out = torch.zeros(world * t.numel(), dtype=torch.float64, device=dev)
        dist.all_gather_into_tensor(out, t)
        return out.view(world, -1).tolist()

    def barrier():
        if distd:
            dist.barrier()
        torch.cuda.synchronize()

    modes = [m for m in args.modes.split(',') if m] if distd else ['none']
    blocks = [None if b == 'none' else int(b) for b in args.blocks.split(',') if b]
    results = []
    last = None                           # rank 0's C of the first setting, for --full-check
    for mode in modes:
        for cb in blocks:
            bounds = shard['bounds'] if distd else [0, n]
            op = RowPartitionedSpMM(bounds, rank, world, local, dev, k,
                                    mode='allgather' if mode == 'none' else mode, col_block=cb)
            Cm = op.step(B)
            torch.cuda.synchronize()
            for _ in range(args.warmup):
                op.step(B)
            barrier()
            op.compute_ms()
            op.timing = True
            t0 = time.perf_counter()
            for _ in range(args.steps):
                op.step(B)
            torch.cuda.synchronize()
            step_ms = (time.perf_counter() - t0) * 1e3 / max(args.steps, 1)
            op.timing = False
            local_ms = op.compute_ms()
            slab_exact = bool(torch.equal(Cm[r0:r1].view(torch.int64), plain.view(torch.int64)))
            got = Cm.index_select(0, rows_t).cpu().numpy()
            parity = bool(np.all(np.abs(got - ref) <= 1e-12 * bound + 1e-300))
            cs = checksum(Cm)
            if distd:
                alls = torch.zeros(world * 2, dtype=torch.int64, device=dev)
                dist.all_gather_into_tensor(alls, cs)
                alls = alls.view(world, 2)
                complete = bool((alls == alls[0]).all())
            else:
                complete = True
            per = gather_floats([local_ms, step_ms, float(op.recv_bytes()), float(slab_exact), float(parity)])
            results.append(dict(mode=mode, col_block=cb, blocks=len(op.blocks),
                                local_ms=[round(p[0], 4) for p in per], step_ms=[round(p[1], 4) for p in per],
                                recv_bytes=[int(p[2]) for p in per], complete=complete,
                                slab_exact=all(p[3] == 1.0 for p in per), parity=all(p[4] == 1.0 for p in per)))
            if args.full_check and rank == 0 and last is None:
                last = Cm.clone()
            del op, Cm
            torch.cuda.empty_cache()

    full = None
    if args.full_check:
        # rank 0: C against ONE full-matrix product (another handle classes its rows differently: a tolerance, not bits)
        # (a step is a collective: every rank takes part or none -- so C comes from the timed settings above)
        full = False
        if rank == 0:
            m = synth.powerlaw_csr(n, n, nnz, max_degree=250_000, device=dev)
            hf, ha = handle_t(0), handle_t(0)
            for hh, v in ((hf, m['values']), (ha, m['values'].abs())):
                check(lib.csrk_create_device(n, n, int(m['colinds'].numel()), m['rowptrs'].data_ptr(),
                                             int(m['rowptrs'].dtype == torch.int64), m['colinds'].data_ptr(),
                                             v.data_ptr(), 2, C.byref(hh)))
            try:
                cf = torch.empty(n, k, dtype=torch.float64, device=dev)
                cb_ = torch.empty(n, k, dtype=torch.float64, device=dev)
                Ba = B.abs()
                check(lib.csrk_spmm_dense_device(hf, B.data_ptr(), k, k, cf.data_ptr(), k, None))
                check(lib.csrk_spmm_dense_device(ha, Ba.data_ptr(), k, k, cb_.data_ptr(), k, None))
                torch.cuda.synchronize()
                full = bool(((last - cf).abs() <= 1e-12 * cb_ + 1e-300).all())
            finally:
                check(lib.csrk_free(hf))
                check(lib.csrk_free(ha))
        barrier()

    check(lib.csrk_free(h))
    if rank == 0:
        line = dict(tool='bench_spmm_dist', world=world, exchange=distd,
                    backend=args.backend if distd else None,
                    workload=f'spmm_powerlaw_{n}x{n}_nnz{nnz}_k{k}_fp64', scale=args.scale,
                    steps=args.steps, warmup=args.warmup,
                    plain_local_ms=round(plain_ms, 4), plan_heavy_rows=int(plan[0]),
                    c_bytes=n * k * 8, results=results,
                    all_complete=all(r['complete'] for r in results),
                    all_parity=all(r['parity'] for r in results),
                    all_slab_exact=all(r['slab_exact'] for r in results))
        if full is not None:
            line['full_matrix_parity'] = full
        print(json.dumps(line), flush=True)
    if distd:
        dist.destroy_process_group()


def main():
    args = parse()
    if args.share_gpu and args.backend != 'gloo':
        sys.exit('--share-gpu needs --backend gloo (RCCL refuses two ranks on one device)')
    if 'RANK' not in os.environ and (args.gpus > 1 or args.force_dist):
        launch(args)                      # does not return
    rank_main(args)


if __name__ == '__main__':
    main()
