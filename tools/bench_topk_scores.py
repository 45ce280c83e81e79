#!/usr/bin/env python3
"""
csrk_topk_scores on the BASELINE configs[2] pattern as `seen` (2M x 2M, nnz 5e7 power-law: synth.powerlaw_csr, coalesced so
that it is canonical), U, V ~ U(-1, 1) [2M x k], n_top = 20.  Per case k16|k64|k128 x f64|f32 (panel), e.g. k64f64, and per
row range of --ranges (1024, 8192, 65536 rows from the middle of the matrix):
  (a) csrk_topk_scores_device on an explicit stream: 20 hipEvent-timed repetitions after 2 warm-ups (median, min, max,
      quartiles);
  (b) the only route without it: torch U_blk @ V.T in the panels' dtype, the seen pairs set to -inf, torch.topk, in chunks
      of --chunk rows that fit memory (its tie order and its NaN order are torch's, not the contract's); --steps-b
      repetitions (one for ranges above --few-above rows: a repetition takes seconds);
  (c) (a) as a share of the 78.6 TFLOP/s float64 spec figure (2 k flop per pair);
  (d) (a) with CSRK_TOPK_SCORES_SELECT=0 in the environment: the product alone (nothing is selected or written; 5
      repetitions), so that (a) - (d) is what selection costs;
  (e) agreement of (a) with float64 torch on --rows sampled rows: every score within k 2^-53 sum |u v| of torch's for its
      item, and the same item set wherever the n_top-th and (n_top + 1)-th reference scores are further apart than twice
      that bound;  (a) twice: equal bits.
Each case runs in a child process of its own under `timeout -k 10`; the parent prints one JSON line with every case and
writes it to --out.
    python tools/bench_topk_scores.py [--cases k64f64,...] [--ranges 1024,8192,65536] [--steps 20] [--warmup 2] [--out FILE]
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
SPEC_TFLOPS = 78.6
N_TOP = 20


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


def child(case, ranges, steps, warmup, steps_b, few_above, chunk, scale_n, n_rows):
    import torch
    from csr_amd import synth
    from csr_amd._lib import lib, check, handle_t, VAL_F32, VAL_F64, DUP_FIRST
    k, panel = int(case[1:-3]), case[-3:]
    n, nnz = int(2_000_000 * scale_n), int(50_000_000 * scale_n)
    m = synth.powerlaw_csr(n, n, nnz, device='cuda', max_degree=250_000)
    rp, ci, vs = m['rowptrs'], m['colinds'], m['values']
    raw, h = handle_t(0), handle_t(0)
    check(lib.csrk_create_device(n, n, nnz, rp.data_ptr(), int(rp.dtype == torch.int64), ci.data_ptr(), vs.data_ptr(), 2, C.byref(raw)))
    check(lib.csrk_coalesce(raw, DUP_FIRST, C.byref(h)))                # canonical: sorted rows, no column twice
    check(lib.csrk_free(raw))
    del m, rp, ci, vs
    nn, nc, nz, p64, vt = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int(), C.c_int()
    check(lib.csrk_info(h, C.byref(nn), C.byref(nc), C.byref(nz), C.byref(p64), C.byref(vt)))
    rp = torch.empty(n + 1, dtype=torch.int64 if p64.value else torch.int32)
    ci = torch.empty(nz.value, dtype=torch.int32)
    check(lib.csrk_export(h, rp.data_ptr(), ci.data_ptr(), None))
    rp, ci = rp.to(torch.int64).cuda(), ci.cuda()
    ok, bad = C.c_int(0), C.c_int32(0)
    check(lib.csrk_is_canonical(h, C.byref(ok), C.byref(bad)))          # the one look at the rows, outside the timings
    assert ok.value == 1
    dt = torch.float64 if panel == 'f64' else torch.float32
    U = synth.dense_vector(n * k, device='cuda', stream=11).view(n, k).to(dt).contiguous()
    V = synth.dense_vector(n * k, device='cuda', stream=12).view(n, k).to(dt).contiguous()
    code = VAL_F64 if panel == 'f64' else VAL_F32
    side = torch.cuda.Stream()
    sp = C.c_void_p(side.cuda_stream)

    def in_side(fn):
        def run():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fn()
            torch.cuda.current_stream().wait_stream(side)
        return run

    out = []
    for nr in ranges:
        nr = min(nr, n)
        rb = (n - nr) // 2
        re_ = rb + nr
        items = torch.empty(nr, N_TOP, dtype=torch.int32, device='cuda')
        scores = torch.empty(nr, N_TOP, dtype=torch.float64, device='cuda')
        counts = torch.empty(nr, dtype=torch.int32, device='cuda')

        def ours():
            check(lib.csrk_topk_scores_device(h, rb, re_, U.data_ptr(), k, V.data_ptr(), k, n, k, code, N_TOP, -np.inf, items.data_ptr(),
                                              N_TOP, scores.data_ptr(), N_TOP, counts.data_ptr(), sp))
        a = _timed(in_side(ours), steps, warmup)
        first = (items.clone(), scores.clone(), counts.clone())
        os.environ['CSRK_TOPK_SCORES_SELECT'] = '0'
        d = _timed(in_side(ours), min(steps, 5), 1)
        del os.environ['CSRK_TOPK_SCORES_SELECT']
        in_side(ours)()
        torch.cuda.synchronize()
        repeat_bitwise = bool(torch.equal(first[0], items) and torch.equal(first[1].view(torch.int64), scores.view(torch.int64)) and
                              torch.equal(first[2], counts))

        # (b) torch: dense scores, mask, topk, per chunk of rows
        b_items = torch.empty(nr, N_TOP, dtype=torch.int64, device='cuda')
        b_scores = torch.empty(nr, N_TOP, dtype=dt, device='cuda')

        def dense():
            for c0 in range(rb, re_, chunk):
                c1 = min(c0 + chunk, re_)
                S = U[c0:c1] @ V.T
                e0, e1 = int(rp[c0]), int(rp[c1])
                lens = rp[c0 + 1:c1 + 1] - rp[c0:c1]
                rows = torch.repeat_interleave(torch.arange(c1 - c0, device='cuda'), lens)
                S[rows, ci[e0:e1].long()] = -np.inf
                t = torch.topk(S, N_TOP, dim=1)
                b_scores[c0 - rb:c1 - rb], b_items[c0 - rb:c1 - rb] = t.values, t.indices
                del S, t
        nb = steps_b if nr <= few_above else 1
        b = _timed(in_side(dense), nb, 1 if nr <= few_above else 0)

        # (e) sampled rows against float64 torch
        g = np.random.default_rng(7)
        sample = np.sort(g.choice(nr, size=min(n_rows, nr), replace=False))
        worst, sets_checked, sets_equal, b_sets_equal = 0.0, 0, 0, 0
        V64 = V.double()
        for x in sample:
            r = rb + int(x)
            u = U[r].double()
            ref = V64 @ u
            bound = (k * 2.0 ** -53) * (V64.abs() @ u.abs())
            it = items[x, :int(counts[x])].long()
            worst = max(worst, float(((scores[x, :len(it)] - ref[it]).abs() / bound[it].clamp_min(1e-300)).max()))
            ref[ci[int(rp[r]):int(rp[r + 1])].long()] = -np.inf
            top = torch.topk(ref, N_TOP + 1)
            if float(top.values[N_TOP - 1] - top.values[N_TOP]) > 2.0 * float(bound.max()):
                sets_checked += 1
                want = set(top.indices[:N_TOP].tolist())
                sets_equal += set(it.tolist()) == want
                b_sets_equal += set(b_items[x].tolist()) == want
        flop = 2.0 * k * nr * n
        out.append({'rows': nr, 'row_begin': rb,
                    'a_topk_scores_device': a, 'b_torch_dense_mask_topk': b, 'b_chunk_rows': chunk,
                    'a_tflops': round(flop / (a['median_ms'] * 1e-3) / 1e12, 3),
                    'c_share_of_spec_fp64': round(flop / (a['median_ms'] * 1e-3) / 1e12 / SPEC_TFLOPS, 4),
                    'd_product_alone': d, 'selection_ms': round(a['median_ms'] - d['median_ms'], 3),
                    'a_over_b': round(a['median_ms'] / b['median_ms'], 4),
                    'e_sampled_rows': int(len(sample)), 'e_worst_score_error_over_bound': worst,
                    'e_untied_rows': sets_checked, 'e_item_sets_equal': int(sets_equal), 'e_torch_route_item_sets_equal': int(b_sets_equal),
                    'a_repeat_bitwise': repeat_bitwise, 'counts_all_n_top': bool((first[2] == N_TOP).all()),
                    'parity': {'ok': bool(worst <= 1.0 and sets_equal == sets_checked and repeat_bitwise)}})
        del items, scores, counts, b_items, b_scores, first
    check(lib.csrk_free(h))
    return {'case': case, 'k': k, 'panel': panel, 'n_top': N_TOP, 'nrows': n, 'n_items': n, 'seen_nnz': int(nz.value), 'ranges': out,
            'parity': {'ok': all(r['parity']['ok'] for r in out)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default=','.join(ALL_CASES))
    ap.add_argument('--ranges', default='1024,8192,65536')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--steps-b', type=int, default=3, help='repetitions of route (b)')
    ap.add_argument('--few-above', type=int, default=8192, help='row ranges above this take route (b) once, without a warm-up')
    ap.add_argument('--chunk', type=int, default=2048, help='rows per dense block of route (b) (2048 x 2M float64 are 32 GB)')
    ap.add_argument('--scale', type=float, default=1.0, help='matrix size relative to configs[2]')
    ap.add_argument('--rows', type=int, default=16, help='rows checked against float64 torch per range')
    ap.add_argument('--child-timeout', type=int, default=500)
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    ranges = [int(r) for r in a.ranges.split(',')]
    if a.child:
        print(json.dumps(child(a.child, ranges, a.steps, a.warmup, a.steps_b, a.few_above, a.chunk, a.scale, a.rows)), flush=True)
        return
    results, failed = [], None
    for case in a.cases.split(','):
        if case not in ALL_CASES:
            raise SystemExit(f'unknown case {case}')
        cmd = ['timeout', '-k', '10', str(a.child_timeout), sys.executable, os.path.abspath(__file__), '--child', case, '--ranges', a.ranges,
               '--steps', str(a.steps), '--warmup', str(a.warmup), '--steps-b', str(a.steps_b), '--few-above', str(a.few_above),
               '--chunk', str(a.chunk), '--scale', str(a.scale), '--rows', str(a.rows)]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
        if p.returncode != 0 or not lines:
            failed = {'case': case, 'returncode': p.returncode, 'stderr': p.stderr[-2000:]}
            break                      # a child that failed ends the run: nothing more is started on the GPU
        results.append(json.loads(lines[-1]))
        for r in results[-1]['ranges']:
            print(f'[bench_topk_scores] {case} {r["rows"]} rows: a {r["a_topk_scores_device"]["median_ms"]} ms '
                  f'({r["a_tflops"]} TFLOP/s), b {r["b_torch_dense_mask_topk"]["median_ms"]} ms, d {r["d_product_alone"]["median_ms"]} ms',
                  file=sys.stderr, flush=True)
    line = json.dumps({'bench': 'topk_scores', 'workload': 'configs[2] pattern as seen (2M x 2M, nnz 5e7 power-law, coalesced), '
                       'U, V ~ U(-1, 1), n_top 20', 'spec_fp64_tflops': SPEC_TFLOPS, 'results': results, 'failed': failed,
                       'parity_ok': failed is None and all(r['parity']['ok'] for r in results)})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(line + '\n')
    sys.exit(0 if failed is None else 1)


if __name__ == '__main__':
    main()
