#!/usr/bin/env python3
"""
csrk_rank_entries_for on the BASELINE configs[2] pattern (2M x 2M, nnz 5e7 power-law: synth.powerlaw_csr, coalesced), split
into `test` and `seen` as tools/bench_rank_entries.py splits it (up to 1 or up to 10 entries held out of every row: --held);
U, V ~ U(-1, 1) [2M x k].  Per case k16|k64|k128 x f64|f32 (panel), per number held out and per number of listed users of
--users (1, 64, 1 024 and 65 536 random rows among those with held-out entries, sorted), beside each other in one process:
  for      csrk_rank_entries_for_device, splits = 0, on an explicit stream, the offsets made on the device beforehand
           (hipEvent-timed: median, min, max);
  range    csrk_rank_entries_device on a contiguous range of as many rows from the middle of the matrix: what the range
           entry costs for that many rows; from --contiguous-from users on also the list entry on those same rows
           (for_contiguous: the same work named row by row, and it must give the range entry's bits) and the range entry
           once more after it (range_again);
  whole    at 1 024 users only: what a caller pays without the list entry -- csrk_rank_entries_device over ALL rows with a
           `test` that holds only the listed users' entries; its ranks and scores must equal for's, bit for bit;
  torch    up to --torch-above users: route (b) of tools/bench_rank_entries.py (U[users] @ V.T in the panels' dtype in chunks,
           the seen pairs set to -inf, one masked count per held-out entry);
  checks   for twice into the same buffers gives equal bits; splits = 1 gives for's bits (up to --one-above users); the
           number of splits in use.
Routes that take a tenth of a second or more per call are repeated --steps-slow times, the others --steps times.  Each case
runs in a child process of its own under `timeout -k 10`; the parent prints one JSON line with every case and writes it to
--out.
    python tools/bench_rank_entries_for.py [--cases k64f64,...] [--users 1,64,1024,65536] [--held 1,10] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_rank_entries import ALL_CASES, _timed      # noqa: E402


def child(case, batches, held, steps, steps_slow, torch_above, one_above, contiguous_from, chunk, scale_n):
    import torch
    from csr_amd import synth
    from csr_amd._lib import lib, check, handle_t, VAL_F32, VAL_F64, VAL_NONE, DUP_FIRST
    from csr_amd.kernels import hip as K
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

    def timed(fn):
        "a first call decides how often the route is repeated"
        one = _timed(in_side(fn), 1, 1)
        return _timed(in_side(fn), steps_slow if one['median_ms'] >= 100.0 else steps, 0)

    def pattern(keep):
        "a structure-only handle over the kept entries, and the arrays it wraps"
        prp = torch.zeros(n + 1, dtype=torch.int64, device='cuda')
        prp[1:] = torch.cumsum(torch.bincount(row[keep], minlength=n), 0)
        pci = ci[keep].contiguous()
        ph = handle_t(0)
        check(lib.csrk_create_device(n, n, len(pci), prp.data_ptr(), 1, pci.data_ptr(), None, VAL_NONE, C.byref(ph)))
        return ph, prp, pci

    def bits(ranks, scores):
        torch.cuda.synchronize()
        return ranks.clone(), scores.clone().view(torch.int64)

    def same(a, b):
        return bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))

    out = []
    g = np.random.default_rng(29)
    for c in held:
        is_test = ((pos * 7919 + row) % lens[row]) < c
        ht, trp, tci = pattern(is_test)
        hs, srp, sci = pattern(~is_test)
        ok, bad = C.c_int(0), C.c_int32(0)
        check(lib.csrk_is_canonical(hs, C.byref(ok), C.byref(bad)))      # the one look at the rows, outside the timings
        assert ok.value == 1
        has = torch.nonzero(trp[1:] > trp[:-1]).squeeze(1).cpu().numpy()          # the users that have held-out entries
        for nr in batches:
            nr = min(nr, len(has))
            users = np.sort(g.choice(has, size=nr, replace=False))
            d_users = torch.from_numpy(users.astype(np.int32)).cuda()
            d_long = d_users.long()
            ulen = trp[d_long + 1] - trp[d_long]
            d_off = torch.zeros(nr + 1, dtype=torch.int64, device='cuda')
            d_off[1:] = torch.cumsum(ulen, 0)
            n_out = int(d_off[-1])
            ranks = torch.full((max(n_out, 1),), -7, dtype=torch.int32, device='cuda')
            scores = torch.full((max(n_out, 1),), -7.0, dtype=torch.float64, device='cuda')

            def ours(splits):
                def run():
                    check(lib.csrk_rank_entries_for_device(hs, ht, d_users.data_ptr(), nr, n, U.data_ptr(), k, V.data_ptr(), k, k, code,
                                                           d_off.data_ptr(), n_out, ranks.data_ptr(), scores.data_ptr(), splits, sp))
                return run
            rec = {'held_out_per_row': c, 'users': nr, 'test_entries': n_out, 'splits_auto': K.rank_entries_for_splits(nr, n)}
            rec['for'] = timed(ours(0))
            first = bits(ranks, scores)
            in_side(ours(0))()
            rec['for_repeat_bitwise'] = same(first, bits(ranks, scores))
            if nr <= one_above:
                ranks.fill_(-7)
                in_side(ours(1))()
                rec['one_equals_for_bitwise'] = same(first, bits(ranks, scores))

            # the range entry on as many contiguous rows
            rb = (n - nr) // 2
            t0, t1 = int(trp[rb]), int(trp[rb + nr])
            r_ranks = torch.empty(max(t1 - t0, 1), dtype=torch.int32, device='cuda')
            r_scores = torch.empty(max(t1 - t0, 1), dtype=torch.float64, device='cuda')

            def rng_entry():
                check(lib.csrk_rank_entries_device(hs, ht, rb, rb + nr, U.data_ptr(), k, V.data_ptr(), k, k, code, r_ranks.data_ptr(),
                                                   r_scores.data_ptr(), sp))
            rec['range'] = timed(rng_entry)
            rec['range_test_entries'] = t1 - t0
            if nr >= contiguous_from:      # the list entry on those same rows, named one by one: the same work, and the same bits
                c_users = torch.arange(rb, rb + nr, dtype=torch.int32, device='cuda')
                c_off = (trp[rb:rb + nr + 1] - t0).contiguous()
                c_ranks = torch.full((max(t1 - t0, 1),), -7, dtype=torch.int32, device='cuda')
                c_scores = torch.full((max(t1 - t0, 1),), -7.0, dtype=torch.float64, device='cuda')

                def for_c():
                    check(lib.csrk_rank_entries_for_device(hs, ht, c_users.data_ptr(), nr, n, U.data_ptr(), k, V.data_ptr(), k, k, code,
                                                           c_off.data_ptr(), t1 - t0, c_ranks.data_ptr(), c_scores.data_ptr(), 0, sp))
                rec['for_contiguous'] = timed(for_c)
                rec['for_contiguous_equals_range_bitwise'] = same(bits(c_ranks, c_scores), bits(r_ranks, r_scores))
                rec['range_again'] = timed(rng_entry)          # (before and after: the range entry's own spread in this process)
                rec['for_contiguous_over_range'] = round(rec['for_contiguous']['median_ms'] / rec['range']['median_ms'], 4)
                del c_users, c_off, c_ranks, c_scores
            del r_ranks, r_scores

            if nr == 1024:      # what a caller pays today: the whole matrix, a test that holds the sample's entries only
                listed = torch.zeros(n, dtype=torch.bool, device='cuda')
                listed[d_long] = True
                hw, wrp, wci = pattern(is_test & listed[row])
                w_ranks = torch.full((max(n_out, 1),), -7, dtype=torch.int32, device='cuda')
                w_scores = torch.full((max(n_out, 1),), -7.0, dtype=torch.float64, device='cuda')

                def whole():
                    check(lib.csrk_rank_entries_device(hs, hw, 0, n, U.data_ptr(), k, V.data_ptr(), k, k, code, w_ranks.data_ptr(),
                                                       w_scores.data_ptr(), sp))
                rec['whole'] = timed(whole)
                rec['whole_equals_for_bitwise'] = same(first, bits(w_ranks, w_scores))          # (sorted users: the same order)
                check(lib.csrk_free(hw))
                del listed, wrp, wci, w_ranks, w_scores

            if nr <= torch_above:
                erow = torch.repeat_interleave(torch.arange(nr, device='cuda'), ulen)
                epos = torch.arange(n_out, device='cuda') - d_off[erow]
                ecol = tci[trp[d_long][erow] + epos]
                b_ranks = torch.empty(n_out, dtype=torch.int64, device='cuda')
                col = torch.arange(n, device='cuda', dtype=torch.int32)

                def dense():
                    for c0 in range(0, nr, chunk):
                        us = d_long[c0:c0 + chunk]
                        S = U[us] @ V.T
                        sl = srp[us + 1] - srp[us]
                        rr = torch.repeat_interleave(torch.arange(len(us), device='cuda'), sl)
                        so = torch.arange(int(sl.sum()), device='cuda') - torch.repeat_interleave(torch.cumsum(sl, 0) - sl, sl)
                        S[rr, sci[torch.repeat_interleave(srp[us], sl) + so].long()] = -np.inf
                        f0, f1 = int(d_off[c0]), int(d_off[min(c0 + chunk, nr)])
                        er, ej = erow[f0:f1] - c0, ecol[f0:f1]
                        se = S[er, ej.long()]
                        for q in range(c):                        # the q-th held-out entry of every row that has one
                            sel = torch.nonzero(epos[f0:f1] == q).squeeze(1)
                            if len(sel) == 0:
                                break
                            Sq, s, j = S[er[sel]], se[sel][:, None], ej[sel][:, None]
                            b_ranks[f0 + sel] = ((Sq > s) | ((Sq == s) & (col[None, :] < j))).sum(1)
                            del Sq
                        del S
                rec['torch'] = timed(dense)
                rec['share_equal_to_torch_route'] = round(float((b_ranks == first[0][:n_out].long()).double().mean()), 6) if n_out else 1.0
                rec['for_over_torch'] = round(rec['for']['median_ms'] / rec['torch']['median_ms'], 4)
                del erow, epos, ecol, b_ranks, col
            rec['for_over_range'] = round(rec['for']['median_ms'] / rec['range']['median_ms'], 4)
            if 'whole' in rec:
                rec['for_over_whole'] = round(rec['for']['median_ms'] / rec['whole']['median_ms'], 4)
            rec['parity'] = {'ok': bool(rec['for_repeat_bitwise'] and rec.get('one_equals_for_bitwise', True) and
                                         rec.get('whole_equals_for_bitwise', True) and
                                         rec.get('for_contiguous_equals_range_bitwise', True))}
            out.append(rec)
            del ranks, scores, first
        check(lib.csrk_free(ht))
        check(lib.csrk_free(hs))
        del trp, tci, srp, sci
    return {'case': case, 'k': k, 'panel': panel, 'nrows': n, 'n_items': n, 'nnz': int(nz.value), 'results': out,
            'parity': {'ok': all(r['parity']['ok'] for r in out)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default=','.join(ALL_CASES))
    ap.add_argument('--users', default='1,64,1024,65536')
    ap.add_argument('--held', default='1,10', help='entries held out per row')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--steps-slow', type=int, default=3, help='repetitions of a route that takes 0.1 s or more per call')
    ap.add_argument('--torch-above', type=int, default=1024, help='no torch route for more listed users than this')
    ap.add_argument('--one-above', type=int, default=1024, help='no splits = 1 comparison for more listed users than this (it is the automatic choice there)')
    ap.add_argument('--contiguous-from', type=int, default=65536,
                    help='from this many users on, the list entry is also timed on the contiguous rows the range entry takes')
    ap.add_argument('--chunk', type=int, default=1024, help='rows per dense block of the torch route (1024 x 2M float64 are 16 GB)')
    ap.add_argument('--scale', type=float, default=1.0, help='matrix size relative to configs[2]')
    ap.add_argument('--child-timeout', type=int, default=400)
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    batches = [int(r) for r in a.users.split(',')]
    held = [int(r) for r in a.held.split(',')]
    if a.child:
        print(json.dumps(child(a.child, batches, held, a.steps, a.steps_slow, a.torch_above, a.one_above, a.contiguous_from, a.chunk,
                               a.scale)), flush=True)
        return
    results, failed = [], None
    for case in a.cases.split(','):
        if case not in ALL_CASES:
            raise SystemExit(f'unknown case {case}')
        cmd = ['timeout', '-k', '10', str(a.child_timeout), sys.executable, os.path.abspath(__file__), '--child', case, '--users', a.users,
               '--held', a.held, '--steps', str(a.steps), '--steps-slow', str(a.steps_slow), '--torch-above', str(a.torch_above),
               '--one-above', str(a.one_above), '--contiguous-from', str(a.contiguous_from), '--chunk', str(a.chunk), '--scale', str(a.scale)]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
        if p.returncode != 0 or not lines:
            failed = {'case': case, 'returncode': p.returncode, 'stderr': p.stderr[-2000:]}
            break                      # a child that failed ends the run: nothing more is started on the GPU
        results.append(json.loads(lines[-1]))
        for r in results[-1]['results']:
            print(f'[bench_rank_entries_for] {case} held {r["held_out_per_row"]} {r["users"]} users: for (S = {r["splits_auto"]}) '
                  f'{r["for"]["median_ms"]} ms [{r["for"]["min_ms"]}, {r["for"]["max_ms"]}], range {r["range"]["median_ms"]} ms '
                  f'[{r["range"]["min_ms"]}, {r["range"]["max_ms"]}], whole {r.get("whole", {}).get("median_ms")} ms, '
                  f'torch {r.get("torch", {}).get("median_ms")} ms, for_contiguous {r.get("for_contiguous", {}).get("median_ms")} ms '
                  f'[{r.get("for_contiguous", {}).get("min_ms")}, {r.get("for_contiguous", {}).get("max_ms")}], range again '
                  f'{r.get("range_again", {}).get("median_ms")} ms, parity {r["parity"]["ok"]}', file=sys.stderr, flush=True)
    line = json.dumps({'bench': 'rank_entries_for', 'workload': 'configs[2] pattern (2M x 2M, nnz 5e7 power-law, coalesced) split into test (up '
                       'to 1 or 10 entries of every row) and seen (the rest), U, V ~ U(-1, 1); random users, sorted', 'results': results,
                       'failed': failed, 'parity_ok': failed is None and all(r['parity']['ok'] for r in results)})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(line + '\n')
    sys.exit(0 if failed is None else 1)


if __name__ == '__main__':
    main()
