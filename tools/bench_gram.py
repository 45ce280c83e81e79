#!/usr/bin/env python3
"""
Per-row Gram matrices (csrk_gram_rows_device) on the BASELINE configs[2] pattern: A 2M x 2M, nnz 5e7 power-law
(synth.powerlaw_csr, the matrix bench_secondary.spmm multiplies), V ~ U(-1, 1) [ncols x k].  The output of all rows does
not fit (2M rows at k = 64 are 65 GB), so a step SWEEPS the rows in blocks of --block rows (65 536) into one reused buffer.
Cases: k16|k32|k64 x f64|f32 (panel) x s0|s1 (scale), e.g. k64f64s1; `als` is one ALS half-step end to end (k = 64, float64):
the right-hand side A V by csrk_spmm_dense_device, then per block the Gram with base = lambda I, torch.linalg.cholesky and
cholesky_solve; `torch` is the route without the kernel -- nnz_b x k x k outer products materialised and summed by
index_add_ -- on the largest run of rows from the middle of the matrix whose products fit --torch-bytes, with the kernel
timed on the same rows.
Each case runs in a child process of its own under `timeout -k 10`; the parent prints one JSON line with every case.
Per case: the median of --steps hipEvent-timed sweeps after --warmup warm-ups; the bytes of the floor model (V gathers
nnz k elt + output nrows k^2 8 + column indices + values if scaled + row pointers); GB/s against the 8 TB/s spec; GFLOP/s at
k (k + 1) flop per entry; csrk_sddmm_device (scale 1) on the same handle, k and panel type; parity on sampled rows against
NumPy float64 within (len + 2) 2^-52 sum |w v_p v_q|.
    python tools/bench_gram.py [--cases k64f64s0,...,als,torch] [--steps 5] [--warmup 1] [--scale 1.0] [--rows 200]
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

HBM_PEAK_GBS = 8000.0
GRAM_CASES = [f'k{k}{p}s{s}' for k in (16, 32, 64) for p in ('f64', 'f32') for s in (0, 1)]
ALL_CASES = GRAM_CASES + ['als', 'torch']


def floor_bytes(n, nnz, k, es, scale):
    parts = {'V_gathers': nnz * k * es, 'out': n * k * k * 8, 'colinds': 4 * nnz, 'values': 8 * nnz if scale else 0,
             'rowptrs': 4 * (n + 1)}
    return parts, sum(parts.values())


def _median_ms(fn, steps, warmup):
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
    return float(np.median(ts)), [round(t, 3) for t in ts]


def _setup(scale_n):
    import torch
    from csr_amd import synth
    from csr_amd._lib import lib, check, handle_t
    n, nnz = int(2_000_000 * scale_n), int(50_000_000 * scale_n)
    m = synth.powerlaw_csr(n, n, nnz, device='cuda', max_degree=250_000)
    rp, ci, vs = m['rowptrs'], m['colinds'], m['values']
    h = handle_t(0)
    check(lib.csrk_create_device(n, n, nnz, rp.data_ptr(), int(rp.dtype == torch.int64), ci.data_ptr(), vs.data_ptr(), 2,
                                 C.byref(h)))
    return n, nnz, rp, ci, vs, h


def _numpy_rows(rows, rph, ci, vs, V, scale, base):
    "(G, M) of tests/gram_ref.gram_numpy for the sampled rows, V rows fetched from the device"
    import torch
    k = V.shape[1]
    G, M = np.zeros((len(rows), k, k)), np.zeros((len(rows), k, k))
    for x, r in enumerate(rows):
        e0, e1 = int(rph[r]), int(rph[r + 1])
        cols = ci[e0:e1].long()
        Vr = V[cols].double().cpu().numpy()
        w = vs[e0:e1].cpu().numpy() if scale else np.ones(e1 - e0)
        WV = w[:, None] * Vr
        G[x] = WV.T @ Vr + base
        M[x] = np.abs(WV).T @ np.abs(Vr) + np.abs(base)
    return G, M


def child_gram(case, steps, warmup, scale_n, n_rows, block):
    import torch
    from csr_amd import synth
    from csr_amd._lib import lib, check, VAL_F32, VAL_F64
    k, panel, scale = int(case[1:3]), case[3:6], int(case[7])
    n, nnz, rp, ci, vs, h = _setup(scale_n)
    V64 = synth.dense_vector(n * k, device='cuda', stream=12).view(n, k)
    V = V64 if panel == 'f64' else V64.float()
    code, es = (VAL_F64, 8) if panel == 'f64' else (VAL_F32, 4)
    block = min(block, n)
    out = torch.empty(block * k * k, dtype=torch.float64, device='cuda')

    def sweep():
        for rb in range(0, n, block):
            check(lib.csrk_gram_rows_device(h, rb, min(rb + block, n), V.data_ptr(), k, k, code, scale, None, out.data_ptr(), None))

    ms, runs = _median_ms(sweep, steps, warmup)
    # SDDMM (scale 1) on the same handle, k and panel type
    U = synth.dense_vector(n * k, device='cuda', stream=11).view(n, k)
    U = U if panel == 'f64' else U.float()
    sd_out = torch.empty(nnz, dtype=torch.float64, device='cuda')
    sd_ms, sd_runs = _median_ms(
        lambda: check(lib.csrk_sddmm_device(h, U.data_ptr(), k, V.data_ptr(), k, k, code, 1, sd_out.data_ptr(), None)), steps, warmup)
    del U, sd_out
    # parity on sampled rows, and the same bits from a second call
    g = np.random.default_rng(7)
    rows = np.sort(g.choice(n, size=min(n_rows, n), replace=False))
    rph = rp.cpu().numpy().astype(np.int64)
    got = np.zeros((len(rows), k, k))
    one = torch.empty(k * k, dtype=torch.float64, device='cuda')
    for x, r in enumerate(rows):
        check(lib.csrk_gram_rows_device(h, int(r), int(r) + 1, V.data_ptr(), k, k, code, scale, None, one.data_ptr(), None))
        got[x] = one.cpu().numpy().reshape(k, k)
    ref, mag = _numpy_rows(rows, rph, ci, vs, V, scale, np.zeros((k, k)))
    lens = (rph[rows + 1] - rph[rows])[:, None, None]
    bound = (lens + 2) * 2.0 ** -52 * mag
    err = np.abs(got - ref)
    # the first sampled row inside a block of its own against the row alone: the range does not change a bit
    r0 = int(rows[0])
    rb = r0 - r0 % block
    check(lib.csrk_gram_rows_device(h, rb, min(rb + block, n), V.data_ptr(), k, k, code, scale, None, out.data_ptr(), None))
    in_block = out[(r0 - rb) * k * k:(r0 - rb + 1) * k * k].cpu().numpy().reshape(k, k)
    parts, total = floor_bytes(n, nnz, k, es, scale)
    gbs = total / ms / 1e6
    check(lib.csrk_free(h))
    return {'case': case, 'k': k, 'panel': panel, 'scale': scale, 'nrows': n, 'nnz': nnz, 'block_rows': block,
            'longest_row': int(np.diff(rph).max()), 'ms': round(ms, 3), 'runs_ms': runs, 'floor_bytes': parts,
            'floor_total': total, 'gbs': round(gbs, 1), 'frac_of_8TBs': round(gbs / HBM_PEAK_GBS, 4),
            'gflops': round(nnz * k * (k + 1) / ms / 1e6, 1), 'ns_per_entry': round(ms * 1e6 / nnz, 3),
            'sddmm_ms': round(sd_ms, 3), 'sddmm_runs_ms': sd_runs, 'gram_over_sddmm': round(ms / sd_ms, 2),
            'range_bitwise': bool(np.array_equal(in_block.view(np.int64), got[0].view(np.int64))),
            'parity': {'ok': bool(np.all(err <= bound)), 'rows': int(len(rows)),
                       'max_err_over_bound': float(np.max(err / np.maximum(bound, 1e-300)))}}


def child_als(steps, warmup, scale_n, n_rows, block, solve_batch, mode='stream', lam=0.1):
    import torch
    from csr_amd import synth
    from csr_amd._lib import lib, check, VAL_F64
    k = 64
    n, nnz, rp, ci, vs, h = _setup(scale_n)
    V = synth.dense_vector(n * k, device='cuda', stream=12).view(n, k)
    block = min(block, n)
    G = torch.empty(block, k, k, dtype=torch.float64, device='cuda')
    rhs = torch.empty(n, k, dtype=torch.float64, device='cuda')
    Unew = torch.empty(n, k, dtype=torch.float64, device='cuda')
    base = (lam * torch.eye(k, dtype=torch.float64, device='cuda')).contiguous()
    part = {'spmm': 0.0, 'gram': 0.0, 'solve': 0.0}

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    side = torch.cuda.Stream() if mode == 'stream' else None
    sp = C.c_void_p(side.cuda_stream) if side is not None else None

    def half_step(capture=None):
        if side is None:
            return _half_step(capture)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):      # the library's launches and torch's solves in ONE explicit stream
            _half_step(capture)
        torch.cuda.current_stream().wait_stream(side)

    def _half_step(capture=None):
        "capture = (sorted sampled rows as a device tensor, dict): the sampled rows of G and L as the sweep hands them on"
        marks = [ev()]
        check(lib.csrk_spmm_dense_device(h, V.data_ptr(), k, k, rhs.data_ptr(), k, sp))
        marks.append(ev())
        spans = []
        for rb in range(0, n, block):
            re_ = min(rb + block, n)
            a = ev()
            check(lib.csrk_gram_rows_device(h, rb, re_, V.data_ptr(), k, k, VAL_F64, 0, base.data_ptr(), G.data_ptr(), sp))
            b = ev()
            for s in range(0, re_ - rb, solve_batch):           # (batched solves in pieces: see --solve-batch)
                t = min(s + solve_batch, re_ - rb)
                L = torch.linalg.cholesky(G[s:t])
                Unew[rb + s:rb + t] = torch.cholesky_solve(rhs[rb + s:rb + t].unsqueeze(-1), L).squeeze(-1)
                if capture is not None:
                    sel = capture[0][(capture[0] >= rb + s) & (capture[0] < rb + t)]
                    for r in sel.tolist():
                        capture[1][r] = (G[r - rb].clone(), L[r - rb - s].clone())
            spans.append((a, b, ev()))
        torch.cuda.synchronize()
        part['spmm'] = marks[0].elapsed_time(marks[1])
        part['gram'] = sum(a.elapsed_time(b) for a, b, _ in spans)
        part['solve'] = sum(b.elapsed_time(c) for _, b, c in spans)

    ms, runs = _median_ms(half_step, steps, warmup)
    # agreement with a NumPy solve on sampled rows: first the solutions the TIMED half-steps left (no host
    # synchronisation inside the sweep), then a half-step that keeps G and L of the sampled rows
    g = np.random.default_rng(7)
    rows = np.sort(g.choice(n, size=min(n_rows, n), replace=False))
    rph = rp.cpu().numpy().astype(np.int64)
    timed_U = Unew[torch.from_numpy(rows).cuda()].cpu().numpy()
    Gn, _ = _numpy_rows(rows, rph, ci, vs, V, 0, lam * np.eye(k))
    worst = worst_rhs = worst_gram = worst_timed = 0.0
    one = torch.empty(k * k, dtype=torch.float64, device='cuda')
    # one more half-step that keeps the sampled rows of G and L as the sweep handed them to the solve, so that a
    # disagreement names its stage: the kernel's block output, the batched factorisation, the batched solve, or the layout
    kept = {}
    half_step((torch.from_numpy(rows).cuda(), kept))
    st = {'g_block_differs_from_single_row_call': 0, 'L_batched_vs_unbatched_card': 0.0, 'L_batched_vs_numpy': 0.0,
          'u_batched_vs_unbatched_card': 0.0, 'u_batched_vs_numpy_cho_solve_of_batched_L': 0.0, 'residual_of_batched_u': 0.0,
          'cond_of_worst_row': None, 'entries_of_worst_row': None}
    for x, r in enumerate(rows):
        e0, e1 = int(rph[r]), int(rph[r + 1])
        b = (vs[e0:e1].cpu().numpy()[:, None] * V[ci[e0:e1].long()].cpu().numpy()).sum(axis=0)
        u = np.linalg.solve(Gn[x], b)
        got = Unew[int(r)].cpu().numpy()
        worst = max(worst, float(np.linalg.norm(got - u) / max(np.linalg.norm(u), 1e-300)))
        worst_timed = max(worst_timed, float(np.linalg.norm(timed_U[x] - u) / max(np.linalg.norm(u), 1e-300)))
        # the two inputs of the solve, each against NumPy, so that a disagreement above names its stage
        worst_rhs = max(worst_rhs, float(np.linalg.norm(rhs[int(r)].cpu().numpy() - b) / max(np.linalg.norm(b), 1e-300)))
        check(lib.csrk_gram_rows_device(h, int(r), int(r) + 1, V.data_ptr(), k, k, VAL_F64, 0, base.data_ptr(), one.data_ptr(), None))
        worst_gram = max(worst_gram, float(np.abs(one.cpu().numpy().reshape(k, k) - Gn[x]).max() / np.abs(Gn[x]).max()))
        gb, Lb = kept[int(r)]
        st['g_block_differs_from_single_row_call'] += int(not torch.equal(gb.view(torch.int64), one.view(k, k).view(torch.int64)))
        L1 = torch.linalg.cholesky(gb)
        u1 = torch.cholesky_solve(rhs[int(r)].unsqueeze(-1), L1).squeeze(-1)
        gbh, Lbh = gb.cpu().numpy(), Lb.cpu().numpy()
        Ln = np.linalg.cholesky(gbh)
        ub = np.linalg.solve(Lbh.T, np.linalg.solve(Lbh, b))       # the batched L, solved on the host
        rel = lambda a_, b_: float(np.linalg.norm(a_ - b_) / max(np.linalg.norm(b_), 1e-300))
        st['L_batched_vs_unbatched_card'] = max(st['L_batched_vs_unbatched_card'], rel(Lbh, L1.cpu().numpy()))
        st['L_batched_vs_numpy'] = max(st['L_batched_vs_numpy'], rel(Lbh, Ln))
        st['u_batched_vs_unbatched_card'] = max(st['u_batched_vs_unbatched_card'], rel(got, u1.cpu().numpy()))
        st['u_batched_vs_numpy_cho_solve_of_batched_L'] = max(st['u_batched_vs_numpy_cho_solve_of_batched_L'], rel(got, ub))
        st['residual_of_batched_u'] = max(st['residual_of_batched_u'], rel(gbh @ got, b))
        if worst == float(np.linalg.norm(got - u) / max(np.linalg.norm(u), 1e-300)):
            st['cond_of_worst_row'], st['entries_of_worst_row'] = float(np.linalg.cond(Gn[x])), e1 - e0
    check(lib.csrk_free(h))
    return {'case': 'als', 'k': k, 'lambda': lam, 'nrows': n, 'nnz': nnz, 'block_rows': block, 'solve_batch': solve_batch,
            'ms': round(ms, 2), 'runs_ms': runs,
            'last_step_parts_ms': {a: round(b, 2) for a, b in part.items()}, 'sampled_rows': int(len(rows)),
            'mode': mode, 'max_rel_diff_vs_numpy_solve_timed_steps': worst_timed, 'max_rel_diff_vs_numpy_solve': worst, 'max_rel_diff_rhs': worst_rhs, 'max_rel_diff_gram': worst_gram,
            'stages': st, 'parity': {'ok': worst < 1e-8 and worst_timed < 1e-8}}


def child_torch(steps, warmup, scale_n, block, torch_bytes):
    import torch
    from csr_amd import synth
    from csr_amd._lib import lib, check, VAL_F64
    k = 64
    n, nnz, rp, ci, vs, h = _setup(scale_n)
    V = synth.dense_vector(n * k, device='cuda', stream=12).view(n, k)
    rph = rp.cpu().numpy().astype(np.int64)
    r0 = n // 2
    budget = torch_bytes // (k * k * 8)                         # entries whose outer products fit
    r1 = int(np.searchsorted(rph, rph[r0] + budget, side='right')) - 1
    r1 = max(min(r1, r0 + block, n), r0 + 1)
    e0, e1 = int(rph[r0]), int(rph[r1])
    cols = ci[e0:e1].long()
    rowid = torch.repeat_interleave(torch.arange(r1 - r0, device='cuda'), (rp[r0 + 1:r1 + 1] - rp[r0:r1]).long())
    out_t = torch.empty(r1 - r0, k, k, dtype=torch.float64, device='cuda')

    def route():
        Vg = V[cols]
        outer = Vg.unsqueeze(2) * Vg.unsqueeze(1)               # [entries, k, k]: 32 KiB per entry
        out_t.zero_()
        out_t.index_add_(0, rowid, outer)

    t_ms, t_runs = _median_ms(route, steps, warmup)
    out_k = torch.empty(r1 - r0, k, k, dtype=torch.float64, device='cuda')
    k_ms, k_runs = _median_ms(
        lambda: check(lib.csrk_gram_rows_device(h, r0, r1, V.data_ptr(), k, k, VAL_F64, 0, None, out_k.data_ptr(), None)), steps, warmup)
    scale_ref = float(out_t.abs().max())
    diff = float((out_t - out_k).abs().max())
    check(lib.csrk_free(h))
    return {'case': 'torch', 'k': k, 'rows': [r0, r1], 'entries': e1 - e0, 'outer_product_bytes': (e1 - e0) * k * k * 8,
            'torch_ms': round(t_ms, 3), 'torch_runs_ms': t_runs, 'kernel_ms': round(k_ms, 4), 'kernel_runs_ms': k_runs,
            'torch_ns_per_entry': round(t_ms * 1e6 / (e1 - e0), 2), 'kernel_ns_per_entry': round(k_ms * 1e6 / (e1 - e0), 2),
            'torch_over_kernel': round(t_ms / k_ms, 1), 'max_abs_diff': diff, 'parity': {'ok': diff <= 1e-10 * max(scale_ref, 1.0)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default=','.join(ALL_CASES))
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--scale', type=float, default=1.0, help='matrix size relative to configs[2]')
    ap.add_argument('--rows', type=int, default=200, help='rows checked against NumPy')
    ap.add_argument('--block', type=int, default=65536, help='rows per call')
    ap.add_argument('--torch-bytes', type=int, default=8 << 30, help='outer products the torch route may materialise')
    ap.add_argument('--solve-batch', type=int, default=16384, help='als: matrices per batched cholesky / cholesky_solve call')
    ap.add_argument('--als-mode', default='stream', choices=['stream', 'default'],
                    help='als: everything in one explicit torch stream, or the library on the NULL stream beside torch\'s default stream')
    ap.add_argument('--child-timeout', type=int, default=300)
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    if a.child:
        if a.child == 'als':
            r = child_als(a.steps, a.warmup, a.scale, min(a.rows, 50), a.block, a.solve_batch, a.als_mode)
        elif a.child == 'torch':
            r = child_torch(a.steps, a.warmup, a.scale, a.block, a.torch_bytes)
        else:
            r = child_gram(a.child, a.steps, a.warmup, a.scale, a.rows, a.block)
        print(json.dumps(r), flush=True)
        return
    results, failed = [], None
    for case in a.cases.split(','):
        if case not in ALL_CASES:
            raise SystemExit(f'unknown case {case}')
        cmd = ['timeout', '-k', '10', str(a.child_timeout), sys.executable, os.path.abspath(__file__), '--child', case,
               '--steps', str(a.steps), '--warmup', str(a.warmup), '--scale', str(a.scale), '--rows', str(a.rows),
               '--block', str(a.block), '--torch-bytes', str(a.torch_bytes), '--solve-batch', str(a.solve_batch), '--als-mode', a.als_mode]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
        if p.returncode != 0 or not lines:
            failed = {'case': case, 'returncode': p.returncode, 'stderr': p.stderr[-2000:]}
            break                      # a child that failed ends the run: nothing more is started on the GPU
        results.append(json.loads(lines[-1]))
    print(json.dumps({'bench': 'gram_rows', 'workload': 'configs[2] pattern (2M x 2M, nnz 5e7 power-law), rows swept in blocks',
                      'results': results, 'failed': failed,
                      'parity_ok': failed is None and all(r['parity']['ok'] for r in results)}), flush=True)
    sys.exit(0 if failed is None else 1)


if __name__ == '__main__':
    main()
