#!/usr/bin/env python3
"""
ALS sweeps on the device (csrk_als_fit_device) with their parts, on the matrix tools/bench_als_cg.py uses: the BASELINE
configs[2] pattern (A 2M x 2M, nnz 5e7 power-law: synth.powerlaw_csr), float64 factors, per case k16 | k64 | k128:
  (a) gram     csrk_panel_gram_device on the 2M x k panel, float64 and float32, beside torch's V.T @ V in the same process; its
               panel bytes over time as a fraction of the HBM peak; its share of one CG half-step at the same k;
  (b) sweep    one sweep of csrk_als_fit_device (cg, 3 steps; implicit and explicit; no objective) beside the sum of its parts
               timed on their own through the device forms, and beside what a caller did before: the host loop of
               CSR.als_rows_cg with NumPy's V.T @ V (host panels in and out of every half-step);
  (c) objective  csrk_als_fit_device with the objective, 5 sweeps: the objective before the first sweep and after each.
Times are medians of --steps hipEvent-timed repetitions after --warmup with their spread.  Two conditions are checked from the
measured values and make the run fail: a fit sweep takes no longer than its separately timed parts by more than those parts'
spread (the sum of their max - min; more would mean a hidden synchronisation or allocation), and a fit sweep is faster than
the host loop.  Each case runs in a child process of its own under `timeout -k 10`; the parent prints one JSON document and
writes it to --out.
    python tools/bench_als_fit.py [--cases k16,k64,k128] [--steps 5] [--warmup 1] [--scale 1.0] [--out profiles/rNN_als_fit.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL_CASES = ['k16', 'k64', 'k128']
CG_STEPS = 3
HBM_PEAK = 8.0e12      # bytes per second, the MI355X's specified HBM3E peak


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


def child(case, steps, warmup, scale_n, lam=0.1, n_sweeps=5):
    import torch
    from csr_amd import CSR, synth
    from csr_amd._lib import lib, check, handle_t, VAL_F32, VAL_F64, ALS_RHS_VALUES, ALS_RHS_ONE_PLUS
    k = int(case[1:])
    n, nnz = int(2_000_000 * scale_n), int(50_000_000 * scale_n)
    m = synth.powerlaw_csr(n, n, nnz, device='cuda')
    rp, ci, vs = m['rowptrs'], m['colinds'], m['values']
    h, th = handle_t(0), handle_t(0)
    check(lib.csrk_create_device(n, n, nnz, rp.data_ptr(), int(rp.dtype == torch.int64), ci.data_ptr(), vs.data_ptr(), 2, C.byref(h)))
    check(lib.csrk_transpose(h, 1, C.byref(th)))
    U0 = (synth.dense_vector(n * k, device='cuda', stream=21).view(n, k) * 0.1).contiguous()
    V0 = (synth.dense_vector(n * k, device='cuda', stream=22).view(n, k) * 0.1).contiguous()
    side = torch.cuda.Stream()
    sp = C.c_void_p(side.cuda_stream)

    def in_side(fn):
        def run():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fn()
            torch.cuda.current_stream().wait_stream(side)
        return run

    def workspace(fn, *args):
        b = C.c_int64(0)
        check(fn(*args, C.byref(b)))
        return torch.empty(max(b.value, 16), dtype=torch.uint8, device='cuda'), b.value

    # ---- (a) the Gram matrix ----
    G = torch.empty(k, k, dtype=torch.float64, device='cuda')
    pgw, pgb = workspace(lib.csrk_panel_gram_workspace, n, k)
    gram = {}
    for name, V, code in (('f64', V0, VAL_F64), ('f32', V0.float(), VAL_F32)):
        t = _timed(in_side(lambda: check(lib.csrk_panel_gram_device(n, k, V.data_ptr(), k, code, 0.0, G.data_ptr(), pgw.data_ptr(), pgb, sp))),
                   steps, warmup)
        first = G.clone()
        in_side(lambda: check(lib.csrk_panel_gram_device(n, k, V.data_ptr(), k, code, 0.0, G.data_ptr(), pgw.data_ptr(), pgb, sp)))()
        torch.cuda.synchronize()
        tt = _timed(lambda: V.T @ V, steps, warmup)
        ref = (V.double().T @ V.double())
        gram[name] = {'panel_gram': t, 'torch_matmul': tt, 'repeat_bitwise': bool(torch.equal(first.view(torch.int64), G.view(torch.int64))),
                      'symmetric': bool(torch.equal(G, G.T)), 'max_rel_diff_to_torch_f64': float(((G - ref).abs() / ref.abs().clamp_min(1e-300)).max()),
                      'panel_bytes': n * k * V.element_size(), 'workspace_bytes': pgb,
                      'fraction_of_hbm_peak': round(n * k * V.element_size() / (t['median_ms'] * 1e-3) / HBM_PEAK, 4)}
        del ref

    # ---- (b) one sweep: the fit, its parts, the host loop ----
    U, V = U0.clone(), V0.clone()
    base = torch.empty(k, k, dtype=torch.float64, device='cuda')
    sweep = {}
    configs = (('implicit', 1, ALS_RHS_ONE_PLUS, 1), ('explicit', 0, ALS_RHS_VALUES, 0))
    for name, scale, rcode, implicit in configs:
        fw, fb = workspace(lib.csrk_als_fit_workspace, n, n, k, 1, implicit, 0)

        def fit(sweeps=1, obj=None):
            check(lib.csrk_als_fit_device(h, th, k, sweeps, 1, CG_STEPS, 0.0, scale, rcode, implicit, lam, 0.0, U.data_ptr(), k, V.data_ptr(), k,
                                          None if obj is None else obj.data_ptr(), None, fw.data_ptr(), fb, sp))

        def part_gram(P):
            check(lib.csrk_panel_gram_device(n, k, P.data_ptr(), k, VAL_F64, 0.0, base.data_ptr(), pgw.data_ptr(), pgb, sp))

        def part_half(hh, P, X):
            check(lib.csrk_als_rows_cg_device(hh, 0, n, P.data_ptr(), k, k, VAL_F64, scale, rcode, base.data_ptr() if implicit else None, lam,
                                              0.0, CG_STEPS, 0.0, X.data_ptr(), k, X.data_ptr(), k, None, None, sp))

        U.copy_(U0), V.copy_(V0)
        f = _timed(in_side(fit), steps, warmup)
        U.copy_(U0), V.copy_(V0)
        parts = {}
        if implicit:
            parts['gram_V'] = _timed(in_side(lambda: part_gram(V)), steps, warmup)
        parts['half_rows'] = _timed(in_side(lambda: part_half(h, V, U)), steps, warmup)
        if implicit:
            parts['gram_U'] = _timed(in_side(lambda: part_gram(U)), steps, warmup)
        parts['half_cols'] = _timed(in_side(lambda: part_half(th, U, V)), steps, warmup)
        total = sum(p['median_ms'] for p in parts.values())
        spread = sum(p['max_ms'] - p['min_ms'] for p in parts.values())
        sweep[name] = {'fit_one_sweep': f, 'parts': parts, 'parts_sum_ms': round(total, 3), 'parts_spread_ms': round(spread, 3),
                       'fit_within_parts': bool(f['median_ms'] <= total + spread)}
        if implicit:
            sweep[name]['gram_share_of_half_step'] = round(parts['gram_V']['median_ms'] / (parts['gram_V']['median_ms'] + parts['half_rows']['median_ms']), 4)
        del fw

    # ---- (c) the objective over n_sweeps sweeps, and the fit against the loop over its parts ----
    objective = {}
    for name, scale, rcode, implicit in configs:
        fw, fb = workspace(lib.csrk_als_fit_workspace, n, n, k, 1, implicit, 1)
        obj = torch.zeros(n_sweeps + 1, dtype=torch.float64, device='cuda')
        U.copy_(U0), V.copy_(V0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        in_side(lambda: check(lib.csrk_als_fit_device(h, th, k, n_sweeps, 1, CG_STEPS, 0.0, scale, rcode, implicit, lam, 0.0, U.data_ptr(), k,
                                                      V.data_ptr(), k, obj.data_ptr(), None, fw.data_ptr(), fb, sp)))()
        e1.record()
        torch.cuda.synchronize()
        objective[name] = {'objective': [float(x) for x in obj.cpu()], 'ms_with_objective': round(e0.elapsed_time(e1), 3), 'sweeps': n_sweeps}
        o = objective[name]['objective']
        objective[name]['decreasing'] = all(o[i + 1] <= o[i] for i in range(n_sweeps))
        del fw
    check(lib.csrk_free(th))
    check(lib.csrk_free(h))

    # ---- what a caller did before: host panels, NumPy's V.T @ V, CSR.als_rows_cg (one sweep, timed once) ----
    A = CSR(n, n, nnz, rp.cpu().numpy(), ci.cpu().numpy(), vs.cpu().numpy())
    At = A.transpose()
    Uh, Vh = U0.cpu().numpy(), V0.cpu().numpy()
    del U, V, U0, V0, m, rp, ci, vs
    torch.cuda.empty_cache()
    host = {}
    for name, scale, rcode, implicit in configs:
        kw = dict(weighted=bool(scale), rhs='one_plus_values' if implicit else 'values', reg=lam, steps=CG_STEPS)
        for rep in range(2):                                         # (the first builds and caches the handles)
            t0 = time.perf_counter()
            Un = A.als_rows_cg(Vh, x0=Uh, base=(Vh.T @ Vh) if implicit else None, **kw)
            Vn = At.als_rows_cg(Un, x0=Vh, base=(Un.T @ Un) if implicit else None, **kw)
            ms = (time.perf_counter() - t0) * 1e3
        host[name] = {'host_loop_one_sweep_ms': round(ms, 1)}
        sweep[name]['host_loop_one_sweep_ms'] = round(ms, 1)
        sweep[name]['fit_faster_than_host_loop'] = bool(sweep[name]['fit_one_sweep']['median_ms'] < ms)
        sweep[name]['host_loop_over_fit'] = round(ms / sweep[name]['fit_one_sweep']['median_ms'], 2)
        del Un, Vn
    ok = all(s['fit_within_parts'] and s['fit_faster_than_host_loop'] for s in sweep.values()) and \
        all(g['repeat_bitwise'] and g['symmetric'] for g in gram.values())
    return {'case': case, 'k': k, 'nrows': n, 'nnz': nnz, 'lambda': lam, 'cg_steps': CG_STEPS, 'gram': gram, 'sweep': sweep,
            'objective': objective, 'ok': ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default=','.join(ALL_CASES))
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--scale', type=float, default=1.0, help='matrix size relative to configs[2]')
    ap.add_argument('--out', default=None, help='where the JSON document goes as well')
    ap.add_argument('--child-timeout', type=int, default=400)
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.steps, a.warmup, a.scale)), flush=True)
        return
    results, failed = [], None
    for case in a.cases.split(','):
        if case not in ALL_CASES:
            raise SystemExit(f'unknown case {case}')
        cmd = ['timeout', '-k', '10', str(a.child_timeout), sys.executable, os.path.abspath(__file__), '--child', case, '--steps', str(a.steps),
               '--warmup', str(a.warmup), '--scale', str(a.scale)]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
        if p.returncode != 0 or not lines:
            failed = {'case': case, 'returncode': p.returncode, 'stderr': p.stderr[-2000:]}
            break                  # a child that failed ends the run: nothing more is started on the GPU
        results.append(json.loads(lines[-1]))
        r = results[-1]
        print(f'[bench_als_fit] {case}: gram f64 {r["gram"]["f64"]["panel_gram"]["median_ms"]} ms (torch {r["gram"]["f64"]["torch_matmul"]["median_ms"]}), '
              + ', '.join(f'{nm} fit {s["fit_one_sweep"]["median_ms"]} ms / parts {s["parts_sum_ms"]} (+-{s["parts_spread_ms"]}) / host loop '
                          f'{s["host_loop_one_sweep_ms"]}' for nm, s in r['sweep'].items()) + f' ok={r["ok"]}', file=sys.stderr, flush=True)
    doc = {'bench': 'als_fit', 'workload': 'configs[2] pattern (2M x 2M, nnz 5e7 power-law), float64 factors, cg with 3 steps', 'scale': a.scale,
           'hbm_peak_bytes_per_s': HBM_PEAK, 'results': results, 'failed': failed,
           'conditions_ok': failed is None and all(r['ok'] for r in results)}
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(doc, f, indent=1)
    print(json.dumps(doc), flush=True)
    sys.exit(0 if doc['conditions_ok'] else 1)


if __name__ == '__main__':
    main()
