#!/usr/bin/env python3
"""
SDDMM (csrk_sddmm_device) on the BASELINE configs[2] matrix: A 2M x 2M, nnz 5e7 power-law (synth.powerlaw_csr, the
matrix bench_secondary.spmm multiplies), k = 64, U and V ~ U(-1, 1).  Cases:
    f64      float64 panels, scale 0
    f64s     float64 panels, scale 1 (A's float64 values multiplied in)
    f32      float32 panels, scale 0
Each case runs in a child process of its own under `timeout -k 10`; the parent prints one JSON line with every case.
Per case: the median of --steps hipEvent-timed calls after --warmup warm-ups, GB/s over the compulsory bytes (written
out), the fraction of 8 TB/s, csrk_spmm_dense_device on the same handle and k timed the same way in the same process
(both gather one 512-B panel row per stored entry) and the SDDMM / SpMM ratio, and parity on sampled rows against a
NumPy float64 restatement (|got - ref| <= 1e-12 sum_t |u_t v_t| max(1, |a|)).
    python tools/bench_sddmm.py [--cases f64,f64s,f32] [--steps 10] [--warmup 2] [--scale 1.0] [--rows 2000]
A counter run of one kernel alone runs a child directly with --ops sddmm (or --ops spmm), e.g.
    rocprofv3 --pmc FETCH_SIZE --kernel-trace -d DIR -- python tools/bench_sddmm.py --child f64 --ops sddmm
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
CASES = {'f64': ('f64', 0), 'f64s': ('f64', 1), 'f32': ('f32', 0)}


def compulsory_bytes(n, ncols, nnz, k, es, scale):
    "what any SDDMM must move: the pattern, the values if scaled, each panel once, the output"
    parts = {'colinds': 4 * nnz, 'values': 8 * nnz if scale else 0, 'rowptrs': 4 * (n + 1),
             'U': n * k * es, 'V': ncols * k * es, 'out': 8 * nnz}
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
    return float(np.median(ts)), [round(t, 4) for t in ts]


def child(case, steps, warmup, scale_n, n_rows, ops=('sddmm', 'spmm')):
    import torch
    from csr_amd import synth
    from csr_amd._lib import lib, check, handle_t, VAL_F32, VAL_F64
    panel, scale = CASES[case]
    dev = 'cuda'
    n, nnz, k = int(2_000_000 * scale_n), int(50_000_000 * scale_n), 64
    m = synth.powerlaw_csr(n, n, nnz, device=dev, max_degree=250_000)
    rp, ci, vs = m['rowptrs'], m['colinds'], m['values']
    h = handle_t(0)
    check(lib.csrk_create_device(n, n, nnz, rp.data_ptr(), int(rp.dtype == torch.int64), ci.data_ptr(), vs.data_ptr(), 2,
                                 C.byref(h)))
    U64 = synth.dense_vector(n * k, device=dev, stream=11).view(n, k)
    V64 = synth.dense_vector(n * k, device=dev, stream=12).view(n, k)
    U, V = (U64, V64) if panel == 'f64' else (U64.float(), V64.float())
    code, es = (VAL_F64, 8) if panel == 'f64' else (VAL_F32, 4)
    out = torch.empty(nnz, dtype=torch.float64, device=dev)

    def sddmm():
        check(lib.csrk_sddmm_device(h, U.data_ptr(), k, V.data_ptr(), k, k, code, scale, out.data_ptr(), None))

    if 'sddmm' in ops:
        ms, runs = _median_ms(sddmm, steps, warmup)
        first = out.clone()
        sddmm()
        torch.cuda.synchronize()
        repeat_bitwise = bool(torch.equal(first.view(torch.int64), out.view(torch.int64)))
    spmm_ms = spmm_runs = None
    if 'spmm' in ops:
        Cm = torch.empty(n, k, dtype=torch.float64, device=dev)
        spmm_ms, spmm_runs = _median_ms(
            lambda: check(lib.csrk_spmm_dense_device(h, V64.data_ptr(), k, k, Cm.data_ptr(), k, None)), steps, warmup)
        del Cm
        spmm_ms = round(spmm_ms, 4)
    if 'sddmm' not in ops:
        check(lib.csrk_free(h))
        return {'case': case, 'ops': list(ops), 'spmm_dense_ms': spmm_ms, 'spmm_runs_ms': spmm_runs}

    parts, total = compulsory_bytes(n, n, nnz, k, es, scale)
    gbs = total / ms / 1e6

    # parity: sampled rows against a NumPy float64 restatement
    g = np.random.default_rng(7)
    rows = np.sort(g.choice(n, size=min(n_rows, n), replace=False))
    rph = rp.cpu().numpy().astype(np.int64)
    starts, ends = rph[rows], rph[rows + 1]
    ent = np.concatenate([np.arange(s, e) for s, e in zip(starts, ends)]) if len(rows) else np.zeros(0, np.int64)
    er = np.repeat(rows, ends - starts)
    ent_t = torch.from_numpy(ent).to(dev)
    cols = ci[ent_t].long()
    Ur = U[torch.from_numpy(er).to(dev)].double().cpu().numpy()
    Vr = V[cols].double().cpu().numpy()
    prod = Ur * Vr
    ref = prod.sum(axis=1)
    bnd = np.abs(prod).sum(axis=1)
    got = out[ent_t].cpu().numpy()
    if scale:
        a = vs[ent_t].cpu().numpy()
        ref = ref * a
        bnd = bnd * np.maximum(1.0, np.abs(a))
    err = np.abs(got - ref)
    ok = bool(np.all(err <= 1e-12 * bnd + 1e-300))
    check(lib.csrk_free(h))
    return {'case': case, 'panel': panel, 'scale': scale, 'nrows': n, 'nnz': nnz, 'k': k,
            'ms': round(ms, 4), 'runs_ms': runs, 'compulsory_bytes': parts, 'compulsory_total': total,
            'gbs': round(gbs, 1), 'frac_of_8TBs': round(gbs / HBM_PEAK_GBS, 4),
            'spmm_dense_ms': spmm_ms, 'spmm_runs_ms': spmm_runs,
            'sddmm_over_spmm': round(ms / spmm_ms, 3) if spmm_ms else None,
            'repeat_bitwise': repeat_bitwise,
            'parity': {'ok': ok, 'rows': int(len(rows)), 'entries': int(len(ent)),
                       'max_err_over_bound': float(np.max(err / (1e-12 * bnd + 1e-300))) if len(ent) else 0.0}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='f64,f64s,f32')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--scale', type=float, default=1.0, help='matrix size relative to configs[2]')
    ap.add_argument('--rows', type=int, default=2000, help='rows checked against NumPy')
    ap.add_argument('--child-timeout', type=int, default=300)
    ap.add_argument('--child', default=None)
    ap.add_argument('--ops', default='sddmm,spmm', help='child only: which products to run (a counter run of one kernel)')
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.steps, a.warmup, a.scale, a.rows, tuple(a.ops.split(',')))), flush=True)
        return
    results, failed = [], None
    for case in a.cases.split(','):
        if case not in CASES:
            raise SystemExit(f'unknown case {case}')
        cmd = ['timeout', '-k', '10', str(a.child_timeout), sys.executable, os.path.abspath(__file__), '--child', case,
               '--steps', str(a.steps), '--warmup', str(a.warmup), '--scale', str(a.scale), '--rows', str(a.rows)]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
        if p.returncode != 0 or not lines:
            failed = {'case': case, 'returncode': p.returncode, 'stderr': p.stderr[-2000:]}
            break                      # a child that failed ends the run: nothing more is started on the GPU
        results.append(json.loads(lines[-1]))
    print(json.dumps({'bench': 'sddmm', 'workload': 'configs[2] pattern (2M x 2M, nnz 5e7 power-law), k = 64',
                      'results': results, 'failed': failed,
                      'parity_ok': failed is None and all(r['parity']['ok'] for r in results)}), flush=True)
    sys.exit(0 if failed is None else 1)


if __name__ == '__main__':
    main()
