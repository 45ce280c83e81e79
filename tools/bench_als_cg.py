#!/usr/bin/env python3
"""
The ALS half-step by conjugate gradient (csrk_als_rows_cg_device, steps = 3) beside the exact route (csrk_als_rows_device) on
the matrix tools/bench_als.py uses: the BASELINE configs[2] pattern (A 2M x 2M, nnz 5e7 power-law: synth.powerlaw_csr),
V ~ U(-1, 1) [ncols x k].  Per case k16|k64|k128 x f64|f32 (panel), e.g. k64f64, three requests:
  explicit  scale 0, rhs = values, ridge 0.1: CG with base NULL and lam = 0.1, the exact route with base = 0.1 I; x0 = the exact
            solution perturbed by 1 % (element-wise, relative), standing in for the previous sweep's factors;
  implicit  scale 1, rhs = 1 + values, base = V^T V + 0.1 I (dense, symmetric) for both routes; the same kind of x0;
  cold      the explicit request with x0 NULL.
Each is the median of --steps (20) hipEvent-timed repetitions after --warmup, with the spread (min, quartiles, max); the exact
route is timed in the same process on the same request (--steps-exact repetitions: it is slow at k = 128).  Also per request: the
relative 2-norm distance of each row's CG result to the exact solve (median and largest over the rows the exact route solved
with info = 0), the steps taken, CG twice: equal bits; and the time of the longest row alone (a row range of one row: the tail
one team walks serially).  Each case runs in a child process of its own under `timeout -k 10`; the parent prints one JSON line.
    python tools/bench_als_cg.py [--cases k64f64,...] [--steps 20] [--steps-exact 5] [--warmup 2] [--scale 1.0] [--max-degree N]
    python tools/bench_als_cg.py --long 1024,2048,4096,8192,16384 [--max-degree N] [--out profiles/r30_als_cg_long.json]
                                              the same table with the long-row class (include/csrk.h, rule C11) off and on at each
                                              L, in one process per case: the CG launch, the longest row alone, equal bits with
                                              the class off, the census.  Without --max-degree both patterns run: configs[2] and
                                              the one with the longest row capped at 2 000.  One JSON document goes to --out.
    python tools/bench_als_cg.py --sweeps     5 alternating sweeps on a 20 000 x 20 000 pattern at k = 64: the ALS objective per
                                              sweep for exact sweeps and for CG sweeps (warm, steps 1, 2, 3, 5)
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
CG_STEPS = 3


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


def child(case, steps, steps_exact, warmup, scale_n, max_degree, lam=0.1, longs=None):
    import torch
    from csr_amd.kernels import hip as K
    from csr_amd import synth
    from csr_amd._lib import lib, check, handle_t, VAL_F32, VAL_F64, ALS_RHS_VALUES, ALS_RHS_ONE_PLUS
    k, panel = int(case[1:-3]), case[-3:]
    n, nnz = int(2_000_000 * scale_n), int(50_000_000 * scale_n)
    m = synth.powerlaw_csr(n, n, nnz, device='cuda', max_degree=max_degree)
    rp, ci, vs = m['rowptrs'], m['colinds'], m['values']
    h = handle_t(0)
    check(lib.csrk_create_device(n, n, nnz, rp.data_ptr(), int(rp.dtype == torch.int64), ci.data_ptr(), vs.data_ptr(), 2, C.byref(h)))
    V64 = synth.dense_vector(n * k, device='cuda', stream=12).view(n, k)
    V = V64 if panel == 'f64' else V64.float()
    code = VAL_F64 if panel == 'f64' else VAL_F32
    eye = torch.eye(k, dtype=torch.float64, device='cuda')
    ridge = (lam * eye).contiguous()
    Vd = V.double()
    gram = Vd.T @ Vd
    implicit_base = ((gram + gram.T) / 2 + lam * eye).contiguous()
    del Vd, gram
    side = torch.cuda.Stream()
    sp = C.c_void_p(side.cuda_stream)
    lens = (rp[1:] - rp[:-1]).long()
    longest = int(lens.argmax())

    def in_side(fn):
        def run():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fn()
            torch.cuda.current_stream().wait_stream(side)
        return run

    Ue = torch.empty(n, k, dtype=torch.float64, device='cuda')
    info = torch.empty(n, dtype=torch.int32, device='cuda')
    Uc = torch.empty(n, k, dtype=torch.float64, device='cuda')
    resid = torch.empty(n, dtype=torch.float64, device='cuda')
    taken = torch.empty(n, dtype=torch.int32, device='cuda')
    noise = 1.0 + 0.01 * (synth.dense_vector(n * k, device='cuda', stream=13).view(n, k))
    out = {}
    for name, scale, rcode, exact_base, cg_base, cg_lam, warm in (
            ('explicit', 0, ALS_RHS_VALUES, ridge, None, lam, True),
            ('implicit', 1, ALS_RHS_ONE_PLUS, implicit_base, implicit_base, 0.0, True),
            ('cold', 0, ALS_RHS_VALUES, ridge, None, lam, False)):

        def exact(rb=0, re_=n):
            check(lib.csrk_als_rows_device(h, rb, re_, V.data_ptr(), k, k, code, scale, rcode, exact_base.data_ptr(), 0.0,
                                           Ue[rb:].data_ptr(), k, info[rb:].data_ptr(), sp))

        e = _timed(in_side(exact), steps_exact, min(warmup, 1))
        torch.cuda.synchronize()
        good = info == 0
        x0 = (Ue * noise).contiguous() if warm else None
        if x0 is not None:
            x0[~good] = 0.0                                      # (a row the exact route could not solve: start it from zero)

        def cg(rb=0, re_=n):
            check(lib.csrk_als_rows_cg_device(h, rb, re_, V.data_ptr(), k, k, code, scale, rcode,
                                              None if cg_base is None else cg_base.data_ptr(), cg_lam, 0.0, CG_STEPS, 0.0,
                                              None if x0 is None else x0[rb:].data_ptr(), k, Uc[rb:].data_ptr(), k, resid[rb:].data_ptr(),
                                              taken[rb:].data_ptr(), sp))

        if longs is not None:
            K.als_cg_set_long(0)                                 # the class off: the launch without the class, the base of every column
        c = _timed(in_side(cg), steps, warmup)
        first = Uc.clone()
        in_side(cg)()
        torch.cuda.synchronize()
        repeat = bool(torch.equal(first.view(torch.int64), Uc.view(torch.int64)))
        del first
        num = (Uc - Ue).norm(dim=1)[good]
        den = Ue.norm(dim=1)[good]
        rel = (num / den.clamp_min(1e-300))[den > 0]
        d0 = None
        if x0 is not None:
            d0 = ((x0 - Ue).norm(dim=1)[good] / den.clamp_min(1e-300))[den > 0]
        # the longest row alone: what one team walks serially (steps + 1 passes, or steps + 2 warm), against the exact route's
        tail_cg = _timed(in_side(lambda: cg(longest, longest + 1)), max(3, steps // 4), 1)
        tail_exact = _timed(in_side(lambda: exact(longest, longest + 1)), max(3, steps_exact // 2), 1)
        by_long = None
        if longs is not None:
            # the class on at each L: the whole launch, the longest row alone, the bits against the class off, the census
            by_long = {}
            keep = (Uc.clone(), resid.clone(), taken.clone())
            for L in longs:
                K.als_cg_set_long(L)
                cl = _timed(in_side(cg), steps, warmup)
                torch.cuda.synchronize()
                same = all(bool(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b))
                           for a, b in zip(keep, (Uc, resid, taken)))
                tl = _timed(in_side(lambda: cg(longest, longest + 1)), max(3, steps // 4), 1)
                in_side(cg)()
                st = K.als_cg_last_stats()
                by_long[str(L)] = {'cg_steps3': cl, 'longest_row_cg_ms': tl, 'same_bits_as_off': same, 'workgroups': st[3],
                                   'long_rows': int((lens >= L).sum()), 'long_entries': int(lens[lens >= L].sum())}
            K.als_cg_set_long(0)
            del keep
        out[name] = {'cg_steps3': c, 'exact_als_rows': e, 'exact_over_cg': round(e['median_ms'] / c['median_ms'], 2),
                     'cg_repeat_bitwise': repeat, 'exact_info_nonzero_rows': int((~good).sum()),
                     'taken_min': int(taken.min()), 'taken_max': int(taken.max()),
                     'rel_distance_to_exact': {'median': float(rel.median()), 'max': float(rel.max()),
                                               'rows_not_finite': int((~torch.isfinite(rel)).sum())},
                     'rel_distance_of_x0_to_exact_median': None if d0 is None else float(d0.median()),
                     'longest_row': {'entries': int(lens[longest]), 'cg_ms': tail_cg, 'exact_ms': tail_exact}}
        if by_long is not None:
            out[name]['long'] = by_long
        del x0
    if longs is not None:
        K.als_cg_set_long(None)
    check(lib.csrk_free(h))
    mean_len = float(lens.double().mean())
    return {'case': case, 'k': k, 'panel': panel, 'lambda': lam, 'nrows': n, 'nnz': nnz, 'max_degree': max_degree, 'cg_steps': CG_STEPS,
            'requests': out,
            'per_row': {'mean_entries': round(mean_len, 2), 'fma_cg_no_base': round((CG_STEPS + 1) * mean_len * 2 * k, 1),
                        'fma_cg_with_base': round((CG_STEPS + 1) * (mean_len * 2 * k + k * k), 1),
                        'fma_exact': round(mean_len * (k * (k + 1) / 2 + k) + k ** 3 / 6 + k * k, 1)},
            'parity': {'ok': all(r['cg_repeat_bitwise'] and all(v['same_bits_as_off'] for v in r.get('long', {}).values())
                                 for r in out.values())}}


def sweeps(n=20000, nnz=500000, k=64, lam=0.1, n_sweeps=5):
    """
    Explicit ALS on a small pattern: objective sum_e (a_e - u_i . v_j)^2 + lam (|U|^2 + |V|^2) after each of n_sweeps alternating
    sweeps (rows, then columns), for exact sweeps (als_rows) and for CG sweeps warm-started from the factors they replace.
    """
    from csr_amd import CSR, synth
    m = synth.powerlaw_csr(n, n, nnz, device='cpu', max_degree=2000)
    A = CSR(n, n, nnz, m['rowptrs'].numpy(), m['colinds'].numpy(), m['values'].numpy())
    At = A.transpose()
    rng = np.random.default_rng(5)
    U0, V0 = rng.standard_normal((n, k)) * 0.1, rng.standard_normal((n, k)) * 0.1
    base = lam * np.eye(k)

    def objective(U, V):
        r = A.values - A.sddmm(U, V).values
        return float(r @ r + lam * ((U * U).sum() + (V * V).sum()))

    table = {'start': objective(U0, V0)}
    U, V = U0.copy(), V0.copy()
    table['exact'] = []
    for _ in range(n_sweeps):
        U = A.als_rows(V, base=base)
        V = At.als_rows(U, base=base)
        table['exact'].append(objective(U, V))
    for steps in (1, 2, 3, 5):
        U, V = U0.copy(), V0.copy()
        table[f'cg_steps{steps}'] = []
        for _ in range(n_sweeps):
            U = A.als_rows_cg(V, x0=U, steps=steps, reg=lam)
            V = At.als_rows_cg(U, x0=V, steps=steps, reg=lam)
            table[f'cg_steps{steps}'].append(objective(U, V))
    return {'bench': 'als_cg_sweeps', 'nrows': n, 'ncols': n, 'nnz': nnz, 'k': k, 'lambda': lam, 'sweeps': n_sweeps, 'objective': table}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default=','.join(ALL_CASES))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--steps-exact', type=int, default=5, help='repetitions of the exact route')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--scale', type=float, default=1.0, help='matrix size relative to configs[2]')
    ap.add_argument('--max-degree', type=int, default=None, help='longest row of the pattern (configs[2]: 250 000); a smaller cap\n'
                    'takes the long-row tail out of both routes and shows the rate of the bulk')
    ap.add_argument('--long', default=None, help='L[,L...]: time the long-row class off and on at each L')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r30_als_cg_long.json'), help='where --long writes its document')
    ap.add_argument('--child-timeout', type=int, default=400)
    ap.add_argument('--child', default=None)
    ap.add_argument('--sweeps', action='store_true')
    ap.add_argument('--sweeps-child', action='store_true')
    a = ap.parse_args()
    longs = None if a.long is None else [int(x) for x in a.long.split(',')]
    if longs is not None and (not longs or min(longs) < 1):
        raise SystemExit('--long takes counts of at least 1')
    if a.child:
        print(json.dumps(child(a.child, a.steps, a.steps_exact, a.warmup, a.scale, a.max_degree, longs=longs)), flush=True)
        return
    if a.sweeps_child:
        print(json.dumps(sweeps()), flush=True)
        return
    if a.sweeps:
        cmd = ['timeout', '-k', '10', str(a.child_timeout), sys.executable, os.path.abspath(__file__), '--sweeps-child']
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
        if p.returncode != 0 or not lines:
            print(json.dumps({'bench': 'als_cg_sweeps', 'failed': {'returncode': p.returncode, 'stderr': p.stderr[-2000:]}}), flush=True)
            sys.exit(1)
        print(lines[-1], flush=True)
        return
    results, failed = [], None
    # --long without --max-degree: both patterns, configs[2] and the one whose longest row is capped at 2 000
    degrees = [a.max_degree] if a.max_degree is not None else ([250_000, 2000] if longs is not None else [250_000])
    for degree in degrees:
        for case in a.cases.split(','):
            if case not in ALL_CASES:
                raise SystemExit(f'unknown case {case}')
            cmd = ['timeout', '-k', '10', str(a.child_timeout), sys.executable, os.path.abspath(__file__), '--child', case,
                   '--steps', str(a.steps), '--steps-exact', str(a.steps_exact), '--warmup', str(a.warmup), '--scale', str(a.scale),
                   '--max-degree', str(degree)] + ([] if longs is None else ['--long', a.long])
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
            if p.returncode != 0 or not lines:
                failed = {'case': case, 'max_degree': degree, 'returncode': p.returncode, 'stderr': p.stderr[-2000:]}
                break                  # a child that failed ends the run: nothing more is started on the GPU
            results.append(json.loads(lines[-1]))
            r = results[-1]['requests']
            print(f'[bench_als_cg] {case} (longest row {degree}): ' + ', '.join(
                f'{nm} cg {r[nm]["cg_steps3"]["median_ms"]} ms' + ''.join(f' | L={L} {v["cg_steps3"]["median_ms"]}' for L, v in r[nm].get('long', {}).items())
                + f' / exact {r[nm]["exact_als_rows"]["median_ms"]} ms' for nm in r), file=sys.stderr, flush=True)
        if failed is not None:
            break
    doc = {'bench': 'als_rows_cg', 'workload': 'configs[2] pattern (2M x 2M, nnz 5e7 power-law, longest row capped at '
                                               + ' and '.join(str(d) for d in degrees) + '), CG steps = 3 beside the exact route',
           'long': longs, 'results': results, 'failed': failed,
           'parity_ok': failed is None and all(r['parity']['ok'] for r in results)}
    if longs is not None:
        with open(a.out, 'w') as f:
            json.dump(doc, f, indent=1)
    print(json.dumps(doc), flush=True)
    sys.exit(0 if failed is None else 1)


if __name__ == '__main__':
    main()
