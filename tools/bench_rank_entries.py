#!/usr/bin/env python3
"""
csrk_rank_entries on the BASELINE configs[2] pattern (2M x 2M, nnz 5e7 power-law: synth.powerlaw_csr, coalesced), split into
`test` -- up to 1 or up to 10 entries held out of every row (--held; entry p of a row of L is held out when
(7919 p + row) mod L < c) -- and `seen`, the rest; U, V ~ U(-1, 1) [2M x k].  Per case k16|k64|k128 x f64|f32 (panel), e.g.
k64f64, per number held out and per row range of --ranges (65536 and 1024 rows from the middle of the matrix), beside
each other in one run:
  (r) csrk_rank_entries_device on an explicit stream: --steps hipEvent-timed repetitions after --warmup (median, min, max);
  (a) csrk_topk_scores_device with n_top = 20 on the same rows, panels and `seen`: the same product, selecting instead of
      counting;
  (b) the only route without the library: torch U_blk @ V.T in the panels' dtype in chunks of --chunk rows, the seen pairs
      set to -inf, and per held-out entry ((S > s_e) | (S == s_e) & (item < j)).sum(1); one repetition above --few-above rows;
  (c) (r) with CSRK_RANK_ENTRIES_COUNT=0 in the environment: the product alone (nothing is counted or written), so that
      (r) - (c) is what counting costs;
  (e) checks: (r) twice gives equal bits; every held-out entry of rank < 20 sits at that place of (a)'s list with the same
      score bits (csrk_rank_entries' rule 5, all rows of the range); the share of entries whose rank equals route (b)'s
      (float64 panels: torch's product rounds differently, so near-ties may move by a place).
The usage example: HR@10, MRR and nDCG@10 from the ranks on the host, in a few lines of numpy (metrics()).
Each case runs in a child process of its own under `timeout -k 10`; the parent prints one JSON line with every case and
writes it to --out.
    python tools/bench_rank_entries.py [--cases k64f64,...] [--ranges 65536,1024] [--held 1,10] [--steps 5] [--out FILE]
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
N_TOP = 20


def metrics(ranks, rowptrs, cut=10):
    "HR@cut, MRR and nDCG@cut over the rows that hold test entries; ranks in storage order, rowptrs of the same rows"
    lens = np.diff(rowptrs)
    row = np.repeat(np.arange(len(lens)), lens)
    gain = np.where(ranks < cut, 1.0 / np.log2(ranks + 2.0), 0.0)
    dcg = np.bincount(row, gain, len(lens))
    ideal = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(cut) + 2.0))])[np.minimum(lens, cut)]
    has = lens > 0
    best = np.full(len(lens), np.iinfo(np.int64).max)
    np.minimum.at(best, row, ranks.astype(np.int64))
    return {'hr': float(np.mean(np.bincount(row, ranks < cut, len(lens))[has] > 0)), 'mrr': float(np.mean(1.0 / (best[has] + 1.0))),
            'ndcg': float(np.mean(dcg[has] / ideal[has])), 'rows_with_entries': int(has.sum()), 'entries': int(len(ranks))}


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
    q = np.percentile(ts, [0, 50, 100])
    return {'median_ms': round(float(q[1]), 3), 'min_ms': round(float(q[0]), 3), 'max_ms': round(float(q[2]), 3), 'steps': steps,
            'warmup': warmup}


def child(case, ranges, held, steps, warmup, few_above, chunk, scale_n):
    import torch
    from csr_amd import synth
    from csr_amd._lib import lib, check, handle_t, VAL_F32, VAL_F64, VAL_NONE, DUP_FIRST
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
    check(lib.csrk_free(h))
    rp, ci = rp.to(torch.int64).cuda(), ci.cuda()
    lens = rp[1:] - rp[:-1]
    row = torch.repeat_interleave(torch.arange(n, device='cuda'), lens)
    pos = torch.arange(len(ci), device='cuda') - rp[row]
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

    def pattern(keep):
        "a structure-only handle over the kept entries, and the arrays it wraps"
        prp = torch.zeros(n + 1, dtype=torch.int64, device='cuda')
        prp[1:] = torch.cumsum(torch.bincount(row[keep], minlength=n), 0)
        pci = ci[keep].contiguous()
        ph = handle_t(0)
        check(lib.csrk_create_device(n, n, len(pci), prp.data_ptr(), 1, pci.data_ptr(), None, VAL_NONE, C.byref(ph)))
        return ph, prp, pci

    out = []
    for c in held:
        is_test = ((pos * 7919 + row) % lens[row]) < c
        ht, trp, tci = pattern(is_test)
        hs, srp, sci = pattern(~is_test)
        ok, bad = C.c_int(0), C.c_int32(0)
        check(lib.csrk_is_canonical(hs, C.byref(ok), C.byref(bad)))      # the one look at the rows, outside the timings
        assert ok.value == 1
        for nr in ranges:
            nr = min(nr, n)
            rb = (n - nr) // 2
            re_ = rb + nr
            t0, t1 = int(trp[rb]), int(trp[re_])
            ranks = torch.empty(t1 - t0, dtype=torch.int32, device='cuda')
            scores = torch.empty(t1 - t0, dtype=torch.float64, device='cuda')
            items = torch.empty(nr, N_TOP, dtype=torch.int32, device='cuda')
            tsc = torch.empty(nr, N_TOP, dtype=torch.float64, device='cuda')
            counts = torch.empty(nr, dtype=torch.int32, device='cuda')

            def ours():
                check(lib.csrk_rank_entries_device(hs, ht, rb, re_, U.data_ptr(), k, V.data_ptr(), k, k, code, ranks.data_ptr(),
                                                   scores.data_ptr(), sp))

            def topk():
                check(lib.csrk_topk_scores_device(hs, rb, re_, U.data_ptr(), k, V.data_ptr(), k, n, k, code, N_TOP, -np.inf,
                                                  items.data_ptr(), N_TOP, tsc.data_ptr(), N_TOP, counts.data_ptr(), sp))
            few = nr <= few_above
            r = _timed(in_side(ours), steps if few else min(steps, 3), warmup)
            first = (ranks.clone(), scores.clone())
            a = _timed(in_side(topk), steps if few else min(steps, 3), warmup)
            os.environ['CSRK_RANK_ENTRIES_COUNT'] = '0'
            cc = _timed(in_side(ours), min(steps, 2), 1)
            del os.environ['CSRK_RANK_ENTRIES_COUNT']
            ranks.fill_(-1)
            in_side(ours)()
            torch.cuda.synchronize()
            repeat_bitwise = bool(torch.equal(first[0], ranks) and torch.equal(first[1].view(torch.int64), scores.view(torch.int64)))

            # (e) rule 5 against (a), every row of the range
            erow = torch.repeat_interleave(torch.arange(nr, device='cuda'), trp[rb + 1:re_ + 1] - trp[rb:re_])
            ecol = tci[t0:t1]
            low = ranks < N_TOP
            at = ranks[low].long()
            rule5 = bool(torch.equal(items[erow[low], at], ecol[low]) and
                         torch.equal(tsc[erow[low], at].view(torch.int64), scores[low].view(torch.int64)))

            # (b) torch: dense scores, mask, one count per held-out entry, per chunk of rows
            b_ranks = torch.empty(t1 - t0, dtype=torch.int64, device='cuda')
            col = torch.arange(n, device='cuda', dtype=torch.int32)
            epos = torch.arange(t1 - t0, device='cuda') - (trp[rb + erow] - t0)          # an entry's place in its row

            def dense():
                for c0 in range(rb, re_, chunk):
                    c1 = min(c0 + chunk, re_)
                    S = U[c0:c1] @ V.T
                    e0, e1 = int(srp[c0]), int(srp[c1])
                    S[torch.repeat_interleave(torch.arange(c1 - c0, device='cuda'), srp[c0 + 1:c1 + 1] - srp[c0:c1]), sci[e0:e1].long()] = -np.inf
                    f0, f1 = int(trp[c0]) - t0, int(trp[c1]) - t0
                    er, ej = erow[f0:f1] - (c0 - rb), ecol[f0:f1]
                    se = S[er, ej.long()]
                    for q in range(c):                            # the q-th held-out entry of every row that has one
                        sel = torch.nonzero(epos[f0:f1] == q).squeeze(1)
                        if len(sel) == 0:
                            break
                        Sq, s, j = S[er[sel]], se[sel][:, None], ej[sel][:, None]
                        b_ranks[f0 + sel] = ((Sq > s) | ((Sq == s) & (col[None, :] < j))).sum(1)
                        del Sq
                    del S
            b = _timed(in_side(dense), 1, 1 if few else 0)
            hr = ranks.cpu().numpy()
            met = metrics(hr, (trp[rb:re_ + 1] - t0).cpu().numpy())
            equal_b = float((b_ranks == ranks.long()).double().mean()) if t1 > t0 else 1.0
            worst_b = int((b_ranks - ranks.long()).abs().max()) if t1 > t0 else 0
            out.append({'held_out_per_row': c, 'rows': nr, 'row_begin': rb, 'test_entries': t1 - t0,
                        'r_rank_entries_device': r, 'a_topk_scores_device_n20': a, 'b_torch_dense_mask_count': b, 'b_chunk_rows': chunk,
                        'c_product_alone': cc, 'counting_ms': round(r['median_ms'] - cc['median_ms'], 3),
                        'r_over_a': round(r['median_ms'] / a['median_ms'], 4), 'r_over_b': round(r['median_ms'] / b['median_ms'], 4),
                        'r_tflops': round(2.0 * k * nr * n / (r['median_ms'] * 1e-3) / 1e12, 3),
                        'hr_at_10': round(met['hr'], 6), 'mrr': round(met['mrr'], 8), 'ndcg_at_10': round(met['ndcg'], 6),
                        'rows_with_entries': met['rows_with_entries'], 'mean_rank': round(float(hr.mean()), 1) if len(hr) else None,
                        'r_repeat_bitwise': repeat_bitwise, 'e_rule5_against_topk_scores': rule5, 'e_entries_below_n_top': int(low.sum()),
                        'e_share_equal_to_torch_route': round(equal_b, 6), 'e_largest_difference_to_torch_route': worst_b,
                        'parity': {'ok': bool(repeat_bitwise and rule5)}})
            del ranks, scores, items, tsc, counts, b_ranks, first
        check(lib.csrk_free(ht))
        check(lib.csrk_free(hs))
        del trp, tci, srp, sci
    return {'case': case, 'k': k, 'panel': panel, 'nrows': n, 'n_items': n, 'nnz': int(nz.value), 'results': out,
            'parity': {'ok': all(r['parity']['ok'] for r in out)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default=','.join(ALL_CASES))
    ap.add_argument('--ranges', default='65536,1024')
    ap.add_argument('--held', default='1,10', help='entries held out per row')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--few-above', type=int, default=8192, help='row ranges above this take at most 3 repetitions and route (b) without a warm-up')
    ap.add_argument('--chunk', type=int, default=1024, help='rows per dense block of route (b) (1024 x 2M float64 are 16 GB, and the rows of one count are gathered beside them)')
    ap.add_argument('--scale', type=float, default=1.0, help='matrix size relative to configs[2]')
    ap.add_argument('--child-timeout', type=int, default=500)
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    ranges = [int(r) for r in a.ranges.split(',')]
    held = [int(r) for r in a.held.split(',')]
    if a.child:
        print(json.dumps(child(a.child, ranges, held, a.steps, a.warmup, a.few_above, a.chunk, a.scale)), flush=True)
        return
    results, failed = [], None
    for case in a.cases.split(','):
        if case not in ALL_CASES:
            raise SystemExit(f'unknown case {case}')
        cmd = ['timeout', '-k', '10', str(a.child_timeout), sys.executable, os.path.abspath(__file__), '--child', case, '--ranges', a.ranges,
               '--held', a.held, '--steps', str(a.steps), '--warmup', str(a.warmup), '--few-above', str(a.few_above), '--chunk', str(a.chunk),
               '--scale', str(a.scale)]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
        if p.returncode != 0 or not lines:
            failed = {'case': case, 'returncode': p.returncode, 'stderr': p.stderr[-2000:]}
            break                      # a child that failed ends the run: nothing more is started on the GPU
        results.append(json.loads(lines[-1]))
        for r in results[-1]['results']:
            print(f'[bench_rank_entries] {case} held {r["held_out_per_row"]} {r["rows"]} rows: r {r["r_rank_entries_device"]["median_ms"]} ms, '
                  f'a {r["a_topk_scores_device_n20"]["median_ms"]} ms, b {r["b_torch_dense_mask_count"]["median_ms"]} ms, '
                  f'c {r["c_product_alone"]["median_ms"]} ms; HR@10 {r["hr_at_10"]} MRR {r["mrr"]} nDCG@10 {r["ndcg_at_10"]}',
                  file=sys.stderr, flush=True)
    line = json.dumps({'bench': 'rank_entries', 'workload': 'configs[2] pattern (2M x 2M, nnz 5e7 power-law, coalesced) split into test (up to 1 '
                       'or 10 entries of every row) and seen (the rest), U, V ~ U(-1, 1)', 'n_top_of_a': N_TOP, 'results': results,
                       'failed': failed, 'parity_ok': failed is None and all(r['parity']['ok'] for r in results)})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(line + '\n')
    sys.exit(0 if failed is None else 1)


if __name__ == '__main__':
    main()
