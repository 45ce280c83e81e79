#!/usr/bin/env python3
"""
Row top-k (csrk_topk_rows) at size, float64 values:
    block      the bench_secondary.abt product: rows of the MovieLens-25M-shaped matrix, A[2000] x B[20000]^T, exact zeros
               filtered -- 2000 rows of ~20 000 entries (the long-row class), min_value = 0
    powerlaw   BASELINE configs[2]'s matrix: 2M x 2M, nnz 5e7 power-law (short rows dominate), no threshold
x k in {20, 200} x order in {descending, storage}.  Each case runs in a child process of its own under `timeout -k 10`;
the parent prints one JSON line with every case.  Per case: the median of --steps hipEvent-timed calls after --warmup
warm-ups (a call = csrk_topk_rows + csrk_free of its result), the compulsory bytes (rowptrs + colinds + values read once,
the result written once) and their share of the 8 TB/s roofline, csrk_filter_zeros on the same handle in the same process
timed the same way (the project's yardstick for "read the matrix once, compact it") and the ratio, two calls compared
byte for byte, and parity of the WHOLE result against the NumPy restatement (tests/topk_ref.py).
    python tools/bench_topk.py [--cases block:20:descending,...] [--steps 10] [--warmup 2]
The case `e2e` times what the entry is for: CSR.multiply_topk(B, 20, transpose=True, min_value=0) against the route
without it -- A.multiply(B, transpose=True), then the restatement on the host -- alternating in one process.
A kernel-trace run of one case runs a child directly, e.g.
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_topk.py --child block:20:descending --no-parity
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HBM_PEAK_GBS = 8000.0
ALL_CASES = [f'{m}:{k}:{o}' for m in ('block', 'powerlaw') for k in (20, 200) for o in ('descending', 'storage')] + ['e2e']


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


def _block_operands():
    "A[2000], B[20000]: the leading rows of the MovieLens-25M-shaped matrix, as host CSRs"
    import torch
    from csr_amd import CSR, synth
    m = synth.movielens_like(device='cuda')
    nc = int(m['ncols'])
    rp = m['rowptrs'][:20001].cpu().numpy()
    eb, ea = int(rp[-1]), int(rp[2000])
    ci, vs = m['colinds'][:eb].cpu().numpy(), m['values'][:eb].cpu().numpy()
    del m
    torch.cuda.empty_cache()
    return CSR(2000, nc, ea, rp[:2001].copy(), ci[:ea].copy(), vs[:ea].copy()), CSR(20000, nc, eb, rp, ci, vs)


def _matrix(name):
    "(handle, min_value, free): a device-resident float64 matrix"
    from csr_amd._lib import lib, check, handle_t
    from csr_amd.kernels import hip as K
    if name == 'block':
        A, B = _block_operands()
        a, b = K.to_handle(A), K.to_handle(B)
        c = K.mult_abt(a, b)
        f = K.filter_zeros(c)
        for x in (c, a, b):
            K.release_handle(x)
        return f.H, 0.0, lambda: K.release_handle(f)
    import torch
    from csr_amd import synth
    n, nnz = 2_000_000, 50_000_000
    m = synth.powerlaw_csr(n, n, nnz, device='cuda', max_degree=250_000)
    rp, ci, vs = m['rowptrs'], m['colinds'], m['values']
    h = handle_t(0)
    check(lib.csrk_create_device(n, n, nnz, rp.data_ptr(), int(rp.dtype == torch.int64), ci.data_ptr(), vs.data_ptr(), 2, C.byref(h)))
    keep = (rp, ci, vs)                                  # the handle wraps these tensors
    return h.value, -np.inf, lambda: (check(lib.csrk_free(h.value)), keep)


def child(case, steps, warmup, parity):
    from csr_amd._lib import lib, check, handle_t
    from csr_amd.kernels import hip as K
    if case == 'e2e':
        return child_e2e(max(steps // 2, 5))
    name, k, order = case.split(':')
    k = int(k)
    H, mv, free = _matrix(name)
    code = {'descending': 0, 'storage': 1}[order]

    def topk(keep=False):
        out = handle_t(0)
        check(lib.csrk_topk_rows(H, k, mv, code, C.byref(out)))
        if keep:
            return out.value
        check(lib.csrk_free(out.value))

    def filt():
        out = handle_t(0)
        check(lib.csrk_filter_zeros(H, C.byref(out)))
        check(lib.csrk_free(out.value))

    ms, runs = _median_ms(topk, steps, warmup)
    fms, fruns = _median_ms(filt, steps, warmup)
    nr, nc, nnz, _, _ = K._info(H)
    t1, t2 = K._wrap(topk(True)), K._wrap(topk(True))
    r1, r2 = K.from_handle(t1), K.from_handle(t2)
    K.release_handle(t1)
    K.release_handle(t2)
    repeat = all(x.tobytes() == y.tobytes() for x, y in ((r1.rowptrs, r2.rowptrs), (r1.colinds, r2.colinds), (r1.values, r2.values)))
    parts = {'rowptrs': 4 * (nr + 1), 'colinds': 4 * nnz, 'values': 8 * nnz, 'result': 4 * (nr + 1) + 12 * r1.nnz}
    total = sum(parts.values())
    gbs = total / ms / 1e6
    res = {'case': case, 'nrows': nr, 'nnz': nnz, 'k': k, 'order': order, 'min_value': None if mv == -np.inf else mv, 'kept': r1.nnz,
           'ms': round(ms, 4), 'runs_ms': runs, 'compulsory_bytes': parts, 'compulsory_total': total, 'gbs': round(gbs, 1),
           'frac_of_8TBs_roofline': round(gbs / HBM_PEAK_GBS, 4), 'filter_zeros_ms': round(fms, 4), 'filter_zeros_runs_ms': fruns,
           'topk_over_filter_zeros': round(ms / fms, 3), 'repeat_bitwise': bool(repeat)}
    if parity:
        from topk_ref import topk_rows_vec, same
        P = K.from_handle(K.hip_h(H, nr, nc, nnz))
        t0 = time.perf_counter()
        exp = topk_rows_vec(P.rowptrs, P.colinds, P.values, k, mv, order)
        res['parity'] = {'ok': bool(same((r1.rowptrs, r1.colinds, r1.values), exp)), 'rows': nr, 'entries': nnz,
                         'host_restatement_s': round(time.perf_counter() - t0, 2)}
    free()
    return res


def child_e2e(reps):
    "CSR.multiply_topk against multiply + the restatement on the host, alternating"
    from topk_ref import topk_rows_vec, same
    A, B = _block_operands()
    dev, host = [], []
    one = two = None
    A.multiply_topk(B, 20, transpose=True, min_value=0.0)            # warm-up: handles cached, pools filled
    for _ in range(reps):
        t0 = time.perf_counter()
        one = A.multiply_topk(B, 20, transpose=True, min_value=0.0)
        dev.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        P = A.multiply(B, transpose=True)
        two = topk_rows_vec(P.rowptrs, P.colinds, P.values, 20, 0.0, 'descending')
        host.append(time.perf_counter() - t0)
        nnz = P.nnz
        del P
    d, h = float(np.median(dev)), float(np.median(host))
    return {'case': 'e2e', 'what': 'A[2000] x B[20000]^T of the MovieLens-25M-shaped matrix, k = 20, min_value = 0, by value',
            'product_nnz': nnz, 'kept': one.nnz, 'multiply_topk_s': round(d, 4), 'multiply_topk_runs_s': [round(t, 4) for t in dev],
            'multiply_then_host_topk_s': round(h, 4), 'multiply_then_host_topk_runs_s': [round(t, 4) for t in host],
            'host_over_device': round(h / d, 2), 'parity': {'ok': bool(same((one.rowptrs, one.colinds, one.values), two))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default=','.join(ALL_CASES))
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--child-timeout', type=int, default=300)
    ap.add_argument('--child', default=None)
    ap.add_argument('--no-parity', action='store_true', help='child only: skip the host restatement (a profiler run)')
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.steps, a.warmup, not a.no_parity)), flush=True)
        return
    results, failed = [], None
    for case in a.cases.split(','):
        if case not in ALL_CASES:
            raise SystemExit(f'unknown case {case}')
        cmd = ['timeout', '-k', '10', str(a.child_timeout), sys.executable, os.path.abspath(__file__), '--child', case,
               '--steps', str(a.steps), '--warmup', str(a.warmup)]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
        if p.returncode != 0 or not lines:
            failed = {'case': case, 'returncode': p.returncode, 'stderr': p.stderr[-2000:]}
            break                      # a child that failed ends the run: nothing more is started on the GPU
        results.append(json.loads(lines[-1]))
        print(lines[-1], file=sys.stderr, flush=True)
    print(json.dumps({'bench': 'topk_rows', 'results': results, 'failed': failed,
                      'parity_ok': failed is None and all(r['parity']['ok'] for r in results)}), flush=True)
    sys.exit(0 if failed is None else 1)


if __name__ == '__main__':
    main()
