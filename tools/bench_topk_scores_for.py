#!/usr/bin/env python3
"""
csrk_topk_scores_for on the BASELINE configs[2] pattern as `seen` (2M x 2M, nnz 5e7 power-law: synth.powerlaw_csr, coalesced so
that it is canonical), U, V ~ U(-1, 1) [2M x k] float64, n_top = 20, k = 16, 64, 128.  Per k and per batch -- 1, 64 and
1 024 random users (r1, r64, r1024) and the contiguous 1 024 and 65 536 rows from the middle of the matrix that
tools/bench_topk_scores.py takes (c1024, c65536):
  auto     csrk_topk_scores_for_device, splits = 0, on an explicit stream, the workspace sized by
           csrk_topk_scores_for_workspace (hipEvent-timed: median, min, max, quartiles);
  one      the same with splits = 1: one launch, no workspace;
  range    csrk_topk_scores_device on the same rows where they are contiguous, and that its bits equal auto's;
  torch    the only route without either: U[users] @ V.T, the seen pairs set to -inf, torch.topk, in chunks of --chunk rows
           (its tie order and its NaN order are torch's, not the contract's);
  forced   at r64 and r1024: splits = auto / 2, auto, 2 auto forced, to check rule 4's W.
auto and one must give the same bits (checked).  Routes that take a tenth of a second or more per call are repeated
--steps-slow times, the others --steps times.  Each k runs in a child process of its own under `timeout -k 10`; the parent
prints one JSON line with every case and writes it to --out.
    python tools/bench_topk_scores_for.py [--ks 16,64,128] [--batches r1,r64,r1024,c1024,c65536] [--out FILE]
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

from bench_topk_scores import _timed      # noqa: E402

ALL_BATCHES = ['r1', 'r64', 'r1024', 'c1024', 'c65536']
N_TOP = 20


def child(k, batches, steps, steps_slow, chunk, scale_n, with_range):
    import torch
    from csr_amd import synth
    from csr_amd._lib import lib, check, handle_t, VAL_F64, DUP_FIRST
    from csr_amd.kernels import hip as K
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
    U = synth.dense_vector(n * k, device='cuda', stream=11).view(n, k).double().contiguous()
    V = synth.dense_vector(n * k, device='cuda', stream=12).view(n, k).double().contiguous()
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

    out = []
    g = np.random.default_rng(23)
    for b in batches:
        nr = min(int(b[1:]), n)
        rb = (n - nr) // 2
        users = np.arange(rb, rb + nr) if b[0] == 'c' else g.choice(n, size=nr, replace=False)
        d_users = torch.from_numpy(users.astype(np.int32)).cuda()
        d_long = d_users.long()
        items = torch.empty(nr, N_TOP, dtype=torch.int32, device='cuda')
        scores = torch.empty(nr, N_TOP, dtype=torch.float64, device='cuda')
        counts = torch.empty(nr, dtype=torch.int32, device='cuda')
        s_auto, need = K.topk_scores_for_workspace(nr, n, N_TOP)
        most = K.topk_scores_for_workspace(nr, n, N_TOP, 2 * s_auto)[1]
        work = torch.empty(max(most, 16), dtype=torch.uint8, device='cuda')

        def ours(splits):
            def run():
                check(lib.csrk_topk_scores_for_device(h, d_users.data_ptr(), nr, n, U.data_ptr(), k, V.data_ptr(), k, n, k, VAL_F64, N_TOP,
                                                      -np.inf, items.data_ptr(), N_TOP, scores.data_ptr(), N_TOP, counts.data_ptr(), splits,
                                                      work.data_ptr(), work.numel(), sp))
            return run

        def snap():
            torch.cuda.synchronize()
            return items.clone(), scores.clone().view(torch.int64), counts.clone()

        def same(a, b):
            return bool(all(torch.equal(x, y) for x, y in zip(a, b)))
        rec = {'batch': b, 'rows': nr, 'contiguous': b[0] == 'c', 'splits_auto': s_auto, 'workspace_bytes': need}
        rec['auto'] = timed(ours(0))
        first = snap()
        rec['one'] = timed(ours(1))
        rec['one_equals_auto_bitwise'] = same(first, snap())
        if b in ('r64', 'r1024'):
            rec['forced'] = {}
            for s in sorted({max(1, s_auto // 2), s_auto, min(2 * s_auto, K.topk_scores_for_limits()[0])}):
                rec['forced'][str(s)] = timed(ours(s))
                rec['forced'][str(s)]['equals_auto_bitwise'] = same(first, snap())
        if b[0] == 'c' and with_range:
            def rng_entry():
                check(lib.csrk_topk_scores_device(h, rb, rb + nr, U.data_ptr(), k, V.data_ptr(), k, n, k, VAL_F64, N_TOP, -np.inf,
                                                  items.data_ptr(), N_TOP, scores.data_ptr(), N_TOP, counts.data_ptr(), sp))
            rec['range'] = timed(rng_entry)
            rec['range_equals_auto_bitwise'] = same(first, snap())

        def dense():
            for c0 in range(0, nr, chunk):
                us = d_long[c0:c0 + chunk]
                S = U[us] @ V.T
                lens = rp[us + 1] - rp[us]
                rows = torch.repeat_interleave(torch.arange(len(us), device='cuda'), lens)
                offs = torch.arange(int(lens.sum()), device='cuda') - torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens)
                S[rows, ci[torch.repeat_interleave(rp[us], lens) + offs].long()] = -np.inf
                t = torch.topk(S, N_TOP, dim=1)
                del S, t
        rec['torch'] = timed(dense) if nr <= 8192 else _timed(in_side(dense), 1, 0)
        rec['auto_over_one'] = round(rec['auto']['median_ms'] / rec['one']['median_ms'], 4)
        rec['auto_over_torch'] = round(rec['auto']['median_ms'] / rec['torch']['median_ms'], 4)
        rec['parity'] = {'ok': bool(rec['one_equals_auto_bitwise'] and rec.get('range_equals_auto_bitwise', True) and
                                     all(f['equals_auto_bitwise'] for f in rec.get('forced', {}).values()) and
                                     bool((first[2] == N_TOP).all()))}
        out.append(rec)
        del items, scores, counts, work
    check(lib.csrk_free(h))
    return {'k': k, 'panel': 'f64', 'n_top': N_TOP, 'nrows': n, 'n_items': n, 'seen_nnz': int(nz.value), 'batches': out,
            'parity': {'ok': all(r['parity']['ok'] for r in out)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ks', default='16,64,128')
    ap.add_argument('--batches', default=','.join(ALL_BATCHES))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--steps-slow', type=int, default=3, help='repetitions of a route that takes 0.1 s or more per call')
    ap.add_argument('--chunk', type=int, default=2048, help='rows per dense block of the torch route (2048 x 2M float64 are 32 GB)')
    ap.add_argument('--scale', type=float, default=1.0, help='matrix size relative to configs[2]')
    ap.add_argument('--no-range', action='store_true', help='leave out csrk_topk_scores_device on the contiguous batches')
    ap.add_argument('--child-timeout', type=int, default=400)
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', type=int, default=None)
    a = ap.parse_args()
    batches = a.batches.split(',')
    for b in batches:
        if b not in ALL_BATCHES:
            raise SystemExit(f'unknown batch {b}')
    if a.child is not None:
        print(json.dumps(child(a.child, batches, a.steps, a.steps_slow, a.chunk, a.scale, not a.no_range)), flush=True)
        return
    results, failed = [], None
    for k in a.ks.split(','):
        cmd = ['timeout', '-k', '10', str(a.child_timeout), sys.executable, os.path.abspath(__file__), '--child', k, '--batches', a.batches,
               '--steps', str(a.steps), '--steps-slow', str(a.steps_slow), '--chunk', str(a.chunk), '--scale', str(a.scale)] + \
              (['--no-range'] if a.no_range else [])
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
        if p.returncode != 0 or not lines:
            failed = {'k': k, 'returncode': p.returncode, 'stderr': p.stderr[-2000:]}
            break                      # a child that failed ends the run: nothing more is started on the GPU
        results.append(json.loads(lines[-1]))
        for r in results[-1]['batches']:
            print(f'[bench_topk_scores_for] k{k} {r["batch"]}: auto (S = {r["splits_auto"]}) {r["auto"]["median_ms"]} ms, one {r["one"]["median_ms"]} ms, '
                  f'range {r.get("range", {}).get("median_ms")} ms, torch {r["torch"]["median_ms"]} ms, forced '
                  f'{ {s: f["median_ms"] for s, f in r.get("forced", {}).items()} }', file=sys.stderr, flush=True)
    line = json.dumps({'bench': 'topk_scores_for', 'workload': 'configs[2] pattern as seen (2M x 2M, nnz 5e7 power-law, coalesced), '
                       'U, V ~ U(-1, 1) float64, n_top 20', 'results': results, 'failed': failed,
                       'parity_ok': failed is None and all(r['parity']['ok'] for r in results)})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(line + '\n')
    sys.exit(0 if failed is None else 1)


if __name__ == '__main__':
    main()
