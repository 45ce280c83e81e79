#!/usr/bin/env python3
"""
One ALS half-step on the BASELINE configs[2] pattern (A 2M x 2M, nnz 5e7 power-law: synth.powerlaw_csr, the matrix
tools/bench_gram.py sweeps), V ~ U(-1, 1) [ncols x k], base = lambda I, explicit ALS (scale 0, rhs = values).  Per case
k16|k64|k128 x f64|f32 (panel), e.g. k64f64, three routes are timed, each as the median of --steps (20) hipEvent-timed
repetitions after --warmup, with their spread (min, max, quartiles):
  (a) csrk_als_rows_device over all rows in one launch: k float64 per row leave the chip;
  (b) the route without it: csrk_spmm_dense_device for the right-hand sides, then per block of --block (65 536) rows
      csrk_gram_rows_device into one reused buffer + torch.linalg.cholesky + cholesky_solve in batches of --solve-batch,
      everything in ONE explicit torch stream (the stream matters).  If the torch build has no batched
      solver that is recorded and Gram + SpMM alone are timed: a lower bound on (b);
  (c) csrk_solve_blocks_device on one block of Gram matrices from the middle of the matrix: what of (a) is the solve.
Also: the work per row (fused multiply-adds to accumulate, n_i k (k + 1) / 2 + n_i k, and to solve, about k^3 / 6 + k^2; bytes
written by (a) and by (b)), info of all rows, (a) against (b) and against a NumPy solve on sampled rows, (a) twice: equal bits.
Each case runs in a child process of its own under `timeout -k 10`; the parent prints one JSON line with every case.
    python tools/bench_als.py [--cases k64f64,...] [--steps 20] [--warmup 2] [--scale 1.0] [--rows 50]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL_CASES = [f'k{k}{p}' for k in (16, 64, 128) for p in ('f64', 'f32')]


def _timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    q = np.percentile(ts, [0, 25, 50, 75, 100])
    return {'median_ms': round(float(q[2]), 3), 'min_ms': round(float(q[0]), 3), 'q25_ms': round(float(q[1]), 3),
            'q75_ms': round(float(q[3]), 3), 'max_ms': round(float(q[4]), 3), 'steps': steps, 'warmup': warmup}


def child(case, steps, warmup, scale_n, n_rows, block, solve_batch, steps_b, lam=0.1):
    import torch
    from csr_amd import synth
    from csr_amd._lib import lib, check, handle_t, VAL_F32, VAL_F64, ALS_RHS_VALUES
    k, panel = int(case[1:-3]), case[-3:]
    n, nnz = int(2_000_000 * scale_n), int(50_000_000 * scale_n)
    m = synth.powerlaw_csr(n, n, nnz, device='cuda', max_degree=250_000)
    rp, ci, vs = m['rowptrs'], m['colinds'], m['values']
    h = handle_t(0)
    check(lib.csrk_create_device(n, n, nnz, rp.data_ptr(), int(rp.dtype == torch.int64), ci.data_ptr(), vs.data_ptr(), 2, C.byref(h)))
    V64 = synth.dense_vector(n * k, device='cuda', stream=12).view(n, k)
    V = V64 if panel == 'f64' else V64.float()
    code, es = (VAL_F64, 8) if panel == 'f64' else (VAL_F32, 4)
    if panel == 'f32':
        V64 = V.double()                                        # route (b)'s right-hand side from the same numbers
    block = min(block, n)
    base = (lam * torch.eye(k, dtype=torch.float64, device='cuda')).contiguous()
    side = torch.cuda.Stream()
    sp = C.c_void_p(side.cuda_stream)

    def in_side(fn):
        def run():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fn()
            torch.cuda.current_stream().wait_stream(side)
        return run

    # (a) the fused half-step
    Ua = torch.empty(n, k, dtype=torch.float64, device='cuda')
    info = torch.empty(n, dtype=torch.int32, device='cuda')

    def fused():
        check(lib.csrk_als_rows_device(h, 0, n, V.data_ptr(), k, k, code, 0, ALS_RHS_VALUES, base.data_ptr(), 0.0, Ua.data_ptr(), k,
                                       info.data_ptr(), sp))

    a = _timed(in_side(fused), steps, warmup)
    first = Ua.clone()
    in_side(fused)()
    torch.cuda.synchronize()
    a_repeat_bitwise = bool(torch.equal(first.view(torch.int64), Ua.view(torch.int64)))
    bad_info = int((info != 0).sum())
    del first

    # (b) Gram into a reused buffer + SpMM + torch's batched Cholesky, per block
    G = torch.empty(block, k, k, dtype=torch.float64, device='cuda')
    rhs = torch.empty(n, k, dtype=torch.float64, device='cuda')
    Ub = torch.empty(n, k, dtype=torch.float64, device='cuda')
    solver = {'available': True, 'error': None}
    try:
        L = torch.linalg.cholesky(base.unsqueeze(0))
        torch.cholesky_solve(torch.ones(1, k, 1, dtype=torch.float64, device='cuda'), L)
        torch.cuda.synchronize()
    except RuntimeError as e:                                   # no batched solver in this torch build: Gram + SpMM alone
        solver = {'available': False, 'error': str(e)[:300]}

    def chunked():
        check(lib.csrk_spmm_dense_device(h, V64.data_ptr(), k, k, rhs.data_ptr(), k, sp))
        for rb in range(0, n, block):
            re_ = min(rb + block, n)
            check(lib.csrk_gram_rows_device(h, rb, re_, V.data_ptr(), k, k, code, 0, base.data_ptr(), G.data_ptr(), sp))
            if not solver['available']:
                continue
            for s in range(0, re_ - rb, solve_batch):
                t = min(s + solve_batch, re_ - rb)
                Lb = torch.linalg.cholesky(G[s:t])
                Ub[rb + s:rb + t] = torch.cholesky_solve(rhs[rb + s:rb + t].unsqueeze(-1), Lb).squeeze(-1)

    b = _timed(in_side(chunked), steps_b, min(warmup, 1))

    # (c) the solve alone on one block of Gram matrices from the middle of the matrix
    r0 = min(n // 2, n - block)
    check(lib.csrk_gram_rows_device(h, r0, r0 + block, V.data_ptr(), k, k, code, 0, base.data_ptr(), G.data_ptr(), None))
    torch.cuda.synchronize()
    xc = torch.empty(block, k, dtype=torch.float64, device='cuda')
    ic = torch.empty(block, dtype=torch.int32, device='cuda')

    def solve():
        check(lib.csrk_solve_blocks_device(block, k, G.data_ptr(), rhs[r0:].data_ptr(), k, xc.data_ptr(), k, ic.data_ptr(), sp))

    c = _timed(in_side(solve), steps, warmup)
    torch.cuda.synchronize()
    # the right-hand side of (b) is csrk_spmm_dense's sum, not rule A3's chain: close, not equal
    c_vs_a = float(((xc - Ua[r0:r0 + block]).abs().max() / Ua[r0:r0 + block].abs().max()))

    # agreement on sampled rows: (a) against (b), and against a NumPy solve of the NumPy system
    g = np.random.default_rng(7)
    rows = np.sort(g.choice(n, size=min(n_rows, n), replace=False))
    rph = rp.cpu().numpy().astype(np.int64)
    sel = torch.from_numpy(rows).cuda()
    ua, ub = Ua[sel].cpu().numpy(), Ub[sel].cpu().numpy()
    worst_np = worst_ab = 0.0
    for x, r in enumerate(rows):
        e0, e1 = int(rph[r]), int(rph[r + 1])
        Vr = V[ci[e0:e1].long()].double().cpu().numpy()
        w = vs[e0:e1].cpu().numpy()
        u = np.linalg.solve(Vr.T @ Vr + lam * np.eye(k), w @ Vr)
        nu = max(np.linalg.norm(u), 1e-300)
        worst_np = max(worst_np, float(np.linalg.norm(ua[x] - u) / nu))
        if solver['available']:
            worst_ab = max(worst_ab, float(np.linalg.norm(ua[x] - ub[x]) / nu))
    lens = np.diff(rph)
    check(lib.csrk_free(h))
    mean_len = float(lens.mean())
    return {'case': case, 'k': k, 'panel': panel, 'lambda': lam, 'nrows': n, 'nnz': nnz, 'longest_row': int(lens.max()),
            'block_rows': block, 'solve_batch': solve_batch,
            'a_als_rows_all_rows': a, 'b_gram_spmm_torch_cholesky_per_block': b, 'c_solve_blocks_one_block': c,
            'torch_batched_solver': solver,
            'a_over_b': round(a['median_ms'] / b['median_ms'], 4),
            'c_scaled_to_all_rows_ms': round(c['median_ms'] * n / block, 2),
            'per_row': {'mean_entries': round(mean_len, 2),
                        'fma_accumulate': round(mean_len * (k * (k + 1) / 2 + k), 1), 'fma_solve': round(k ** 3 / 6 + k * k, 1),
                        'bytes_written_a': k * 8 + 4, 'bytes_written_b': k * k * 8 + 2 * k * 8,
                        'bytes_gathered': round(mean_len * k * es, 1)},
            'info_nonzero_rows': bad_info, 'a_repeat_bitwise': a_repeat_bitwise,
            'max_rel_diff_a_vs_numpy_solve': worst_np, 'max_rel_diff_a_vs_b': worst_ab if solver['available'] else None,
            'max_rel_diff_c_vs_a_on_its_block': c_vs_a, 'sampled_rows': int(len(rows)),
            # parity is about the library's route; whether route (b) lands on the same solutions is reported beside it
            'b_agrees_with_a': bool(worst_ab < 1e-8) if solver['available'] else None,
            'parity': {'ok': bad_info == 0 and a_repeat_bitwise and worst_np < 1e-8 and c_vs_a < 1e-8}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default=','.join(ALL_CASES))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--steps-b', type=int, default=None, help='repetitions of route (b) (default: --steps)')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--scale', type=float, default=1.0, help='matrix size relative to configs[2]')
    ap.add_argument('--rows', type=int, default=50, help='rows checked against NumPy')
    ap.add_argument('--block', type=int, default=65536, help='rows per Gram call of route (b), systems of route (c)')
    ap.add_argument('--solve-batch', type=int, default=16384, help='matrices per batched cholesky / cholesky_solve call')
    ap.add_argument('--child-timeout', type=int, default=400)
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    steps_b = a.steps if a.steps_b is None else a.steps_b
    if a.child:
        print(json.dumps(child(a.child, a.steps, a.warmup, a.scale, a.rows, a.block, a.solve_batch, steps_b)), flush=True)
        return
    results, failed = [], None
    for case in a.cases.split(','):
        if case not in ALL_CASES:
            raise SystemExit(f'unknown case {case}')
        cmd = ['timeout', '-k', '10', str(a.child_timeout), sys.executable, os.path.abspath(__file__), '--child', case,
               '--steps', str(a.steps), '--steps-b', str(steps_b), '--warmup', str(a.warmup), '--scale', str(a.scale),
               '--rows', str(a.rows), '--block', str(a.block), '--solve-batch', str(a.solve_batch)]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
        if p.returncode != 0 or not lines:
            failed = {'case': case, 'returncode': p.returncode, 'stderr': p.stderr[-2000:]}
            break                      # a child that failed ends the run: nothing more is started on the GPU
        results.append(json.loads(lines[-1]))
        print(f'[bench_als] {case}: a {results[-1]["a_als_rows_all_rows"]["median_ms"]} ms, b '
              f'{results[-1]["b_gram_spmm_torch_cholesky_per_block"]["median_ms"]} ms, c '
              f'{results[-1]["c_solve_blocks_one_block"]["median_ms"]} ms', file=sys.stderr, flush=True)
    print(json.dumps({'bench': 'als_rows', 'workload': 'configs[2] pattern (2M x 2M, nnz 5e7 power-law), explicit ALS, base = 0.1 I',
                      'results': results, 'failed': failed,
                      'parity_ok': failed is None and all(r['parity']['ok'] for r in results)}), flush=True)
    sys.exit(0 if failed is None else 1)


if __name__ == '__main__':
    main()
