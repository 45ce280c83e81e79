#!/usr/bin/env python3
"""
csrk_coalesce at size, float64 values, on BASELINE configs[2]'s matrix (2M x 2M, nnz 5e7 power-law; short rows dominate):
    canonical   the matrix as it is                                                     -> route 0 (a device copy)
    repeats     about 10 % of its entries given their predecessor's column (rows stay sorted)  -> route 1 (merged, no sort)
    shuffled    the same with the entries of every row in a random order                -> route 2 (sorted, then merged)
Each case runs in a child process of its own under `timeout -k 10`; the parent prints one JSON line with every case.  Per
case: the median of --steps hipEvent-timed calls after --warmup warm-ups (a call = csrk_coalesce + csrk_free of its result;
the look at the rows is cached by the warm-ups), csrk_filter_zeros on the same handle and csrk_order_columns on a copy of it
timed the same way in the same process with the ratios, two calls compared byte for byte, and parity of the WHOLE result
against a vectorised NumPy restatement, itself checked against tests/coalesce_ref.py on the leading rows.
    python tools/bench_coalesce.py [--cases canonical,repeats,shuffled] [--dup sum] [--steps 10] [--warmup 2]
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_topk import _median_ms, HBM_PEAK_GBS      # noqa: E402

ALL_CASES = ['canonical', 'repeats', 'shuffled']
ROUTE = {'canonical': 0, 'repeats': 1, 'shuffled': 2}
N, NNZ = 2_000_000, 50_000_000


def _tensors(case, n, nnz):
    "(rowptrs, colinds, values) on the device"
    import torch
    from csr_amd import synth
    m = synth.powerlaw_csr(n, n, nnz, device='cuda', max_degree=250_000)
    rp, ci, vs = m['rowptrs'], m['colinds'], m['values']
    if case == 'canonical':
        return rp, ci, vs
    g = torch.Generator(device='cuda')
    g.manual_seed(7)
    rep = torch.rand(nnz, generator=g, device='cuda') < 0.1
    rep[rp[:-1][rp[:-1] < nnz].long()] = False          # an entry that starts a row keeps its column
    prev = torch.roll(ci, 1)
    ci = torch.where(rep, prev, ci)                      # (two flagged neighbours: the second takes the first's OLD column: still sorted)
    del prev, rep
    if case == 'shuffled':
        rows = torch.repeat_interleave(torch.arange(n, device='cuda', dtype=torch.float64), (rp[1:] - rp[:-1]).long())
        rows += torch.rand(nnz, generator=g, device='cuda', dtype=torch.float64)
        perm = torch.argsort(rows)
        del rows
        ci, vs = ci[perm].contiguous(), vs[perm].contiguous()
        del perm
    torch.cuda.synchronize()
    return rp, ci.contiguous(), vs


def _handle(rp, ci, vs, n, nnz):
    import torch
    from csr_amd._lib import lib, check, handle_t
    h = handle_t(0)
    check(lib.csrk_create_device(n, n, nnz, rp.data_ptr(), int(rp.dtype == torch.int64), ci.data_ptr(), vs.data_ptr(), 2, C.byref(h)))
    return h.value


def _restate(A, dup):
    "coalesce_ref, vectorised over the whole matrix through (row, column) keys"
    rp, ci, vs = A
    nr = len(rp) - 1
    width = int(ci.max(initial=0)) + 1
    keys = np.repeat(np.arange(nr, dtype=np.int64), np.diff(rp)) * width + ci
    if len(keys) and not np.all(keys[1:] >= keys[:-1]):
        o = np.argsort(keys, kind='stable')              # ascending (row, column), storage order among equals
        keys, vs = keys[o], vs[o]
    head = np.concatenate(([True], keys[1:] != keys[:-1])) if len(keys) else np.zeros(0, bool)
    start = np.flatnonzero(head)
    length = np.diff(np.concatenate((start, [len(keys)])))
    out = vs[start].copy()
    above = lambda a, b: np.where(np.isnan(a), ~np.isnan(b), a > b)      # noqa: E731
    if dup == 'last':
        out = vs[start + length - 1].copy()
    elif dup != 'first':
        with np.errstate(all='ignore'):
            for k in range(1, int(length.max(initial=1))):   # the k-th member of every group that has one, left to right
                sel = length > k
                v, w = vs[start[sel] + k], out[sel]
                if dup == 'sum':
                    out[sel] = w + v
                elif dup == 'max':
                    out[sel] = np.where(above(v, w), v, w)
                else:
                    out[sel] = np.where(above(v, w), w, v)
    hk = keys[start]
    orp = np.concatenate(([0], np.cumsum(np.bincount(hk // width, minlength=nr)))).astype(np.int32 if len(hk) <= 2 ** 31 - 1 else np.int64)
    return orp, (hk % width).astype(np.int32), out


def child(case, dup, steps, warmup, parity, n, nnz):
    import torch
    from csr_amd._lib import lib, check, handle_t
    from csr_amd.kernels import hip as K
    rp, ci, vs = _tensors(case, n, nnz)
    H = _handle(rp, ci, vs, n, nnz)
    ci2, vs2 = ci.clone(), vs.clone()                     # order_columns works in place: it gets a copy of its own
    H2 = _handle(rp, ci2, vs2, n, nnz)
    code = K.coalesce_args(dup)

    def co(keep=False):
        out = handle_t(0)
        check(lib.csrk_coalesce(H, code, C.byref(out)))
        if keep:
            return out.value
        check(lib.csrk_free(out.value))

    def filt():
        out = handle_t(0)
        check(lib.csrk_filter_zeros(H, C.byref(out)))
        check(lib.csrk_free(out.value))

    def order():
        check(lib.csrk_order_columns(H2))

    ms, runs = _median_ms(co, steps, warmup)
    route = K.coalesce_last_route()
    fms, fruns = _median_ms(filt, steps, warmup)
    oms, oruns = _median_ms(order, steps, warmup)
    t1, t2 = K._wrap(co(True)), K._wrap(co(True))
    r1, r2 = K.from_handle(t1), K.from_handle(t2)
    K.release_handle(t1)
    K.release_handle(t2)
    repeat = all(x.tobytes() == y.tobytes() for x, y in ((r1.rowptrs, r2.rowptrs), (r1.colinds, r2.colinds), (r1.values, r2.values)))
    parts = {'h': 4 * (n + 1) + 12 * nnz, 'result': 4 * (n + 1) + 12 * r1.nnz}
    total = sum(parts.values())
    gbs = total / ms / 1e6
    res = {'case': case, 'dup': dup, 'nrows': n, 'nnz': nnz, 'nnz_result': r1.nnz, 'route': route, 'route_expected': ROUTE[case],
           'ms': round(ms, 4), 'runs_ms': runs, 'compulsory_bytes': parts, 'compulsory_total': total, 'gbs': round(gbs, 1),
           'frac_of_8TBs_roofline': round(gbs / HBM_PEAK_GBS, 4), 'filter_zeros_ms': round(fms, 4), 'filter_zeros_runs_ms': fruns,
           'order_columns_ms': round(oms, 4), 'order_columns_runs_ms': oruns, 'coalesce_over_filter_zeros': round(ms / fms, 3),
           'coalesce_over_order_columns': round(ms / oms, 3), 'repeat_bitwise': bool(repeat)}
    if parity:
        from coalesce_ref import coalesce_ref, same
        A = (rp.cpu().numpy(), ci.cpu().numpy(), vs.cpu().numpy())
        t0 = time.perf_counter()
        exp = _restate(A, dup)
        head = min(200, n)                                # the vectorised form against the group-by-group one, on the leading rows
        cut = lambda t, k: (t[0][:k + 1], t[1][:t[0][k]], t[2][:t[0][k]])      # noqa: E731
        head_ok = same(cut(exp, head), coalesce_ref(cut(A, head), dup), dup)
        res['parity'] = {'ok': bool(head_ok and route == ROUTE[case] and same((r1.rowptrs, r1.colinds, r1.values), exp, dup)),
                         'restatement_head_ok': bool(head_ok), 'rows': n, 'entries': r1.nnz,
                         'host_restatement_s': round(time.perf_counter() - t0, 2)}
    check(lib.csrk_free(H))
    check(lib.csrk_free(H2))
    del ci2, vs2
    torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default=','.join(ALL_CASES))
    ap.add_argument('--dup', default='sum')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--nrows', type=int, default=N)
    ap.add_argument('--nnz', type=int, default=NNZ)
    ap.add_argument('--child-timeout', type=int, default=300)
    ap.add_argument('--child', default=None)
    ap.add_argument('--no-parity', action='store_true', help='child only: skip the host restatement (a profiler run)')
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.dup, a.steps, a.warmup, not a.no_parity, a.nrows, a.nnz)), flush=True)
        return
    results, failed = [], None
    for case in a.cases.split(','):
        if case not in ALL_CASES:
            raise SystemExit(f'unknown case {case}')
        cmd = ['timeout', '-k', '10', str(a.child_timeout), sys.executable, os.path.abspath(__file__), '--child', case, '--dup', a.dup,
               '--steps', str(a.steps), '--warmup', str(a.warmup), '--nrows', str(a.nrows), '--nnz', str(a.nnz)]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
        if p.returncode != 0 or not lines:
            failed = {'case': case, 'returncode': p.returncode, 'stderr': p.stderr[-2000:]}
            break                      # a child that failed ends the run: nothing more is started on the GPU
        results.append(json.loads(lines[-1]))
        print(lines[-1], file=sys.stderr, flush=True)
    print(json.dumps({'bench': 'coalesce', 'results': results, 'failed': failed,
                      'parity_ok': failed is None and all(r['parity']['ok'] for r in results)}), flush=True)
    sys.exit(0 if failed is None else 1)


if __name__ == '__main__':
    main()
