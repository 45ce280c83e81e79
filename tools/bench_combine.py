#!/usr/bin/env python3
"""
Entry-wise combination (csrk_combine) at size, float64 values:
    block      A = the bench_secondary.abt product: rows of the MovieLens-25M-shaped matrix, A[2000] x B[20000]^T, exact zeros
               filtered (2000 rows of ~20 000 entries, columns in the reference's order; sorted once, untimed, for add and
               multiply); B = the ratings block the product came from, rows [0, 2000), cut to the product's 20 000 columns
    powerlaw   A = BASELINE configs[2]'s matrix, 2M x 2M, nnz 5e7 power-law (short rows dominate); B = a row-permuted copy of it
x op in {drop, add, multiply}.  Each case runs in a child process of its own under `timeout -k 10`; the parent prints one
JSON line with every case.  Per case: the median of --steps hipEvent-timed calls after --warmup warm-ups (a call =
csrk_combine + csrk_free of its result; the operands' canonical flags are cached by the warm-ups), the compulsory bytes
(both operands' arrays the op has to read, once, and the result written once) and their share of the 8 TB/s roofline,
csrk_filter_zeros on the same A in the same process timed the same way (a one-operand compaction: the project's yardstick)
and the ratio, two calls compared byte for byte, and parity of the WHOLE result against a vectorised NumPy restatement
checked here against tests/combine_ref.py on the leading rows.
    python tools/bench_combine.py [--cases block:drop,...] [--steps 10] [--warmup 2]
The case `e2e` times what the mask is for: CSR.multiply_topk(B, 20, transpose=True, min_value=0, exclude=seen) against the
same call without `exclude` and against the host route (A.multiply(B, transpose=True) exported, SciPy removes the seen
pairs, the top-k restatement on the host), alternating in one process.
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

from bench_topk import _median_ms, _block_operands, HBM_PEAK_GBS      # noqa: E402

OPS = ('drop', 'add', 'multiply')
ALL_CASES = [f'{m}:{o}' for m in ('block', 'powerlaw') for o in OPS] + ['e2e']
ALPHA, BETA = 0.75, -1.5


def _seen_block(A, ncols):
    "the ratings rows of A cut to the columns below ncols, structure only: the pairs a recommender has seen"
    from csr_amd import CSR
    keep = A.colinds < ncols
    cum = np.concatenate(([0], np.cumsum(keep, dtype=np.int64)))
    return CSR(A.nrows, ncols, int(cum[-1]), cum[A.rowptrs], A.colinds[keep], None)


def _operands(name, op):
    "(handle of A, handle of B, free)"
    from csr_amd._lib import lib, check, handle_t
    from csr_amd.kernels import hip as K
    if name == 'block':
        A, B = _block_operands()
        a, b = K.to_handle(A), K.to_handle(B)
        c = K.mult_abt(a, b)
        f = K.filter_zeros(c)
        for x in (c, a, b):
            K.release_handle(x)
        if op != 'drop':
            K.order_columns(f)                          # add and multiply need a canonical A; the masks take it as it comes
        s = K.to_handle(_seen_block(A, B.nrows))
        return f.H, s.H, lambda: (K.release_handle(f), K.release_handle(s))
    import torch
    from csr_amd import synth
    n, nnz = 2_000_000, 50_000_000
    m = synth.powerlaw_csr(n, n, nnz, device='cuda', max_degree=250_000)
    rp, ci, vs = m['rowptrs'], m['colinds'], m['values']
    h = handle_t(0)
    check(lib.csrk_create_device(n, n, nnz, rp.data_ptr(), int(rp.dtype == torch.int64), ci.data_ptr(), vs.data_ptr(), 2, C.byref(h)))
    g = torch.Generator(device='cpu')
    g.manual_seed(5)
    perm = torch.randperm(n, generator=g).to(torch.int32).numpy()
    p = K.pick_rows(K.hip_h(h.value, n, n, nnz), perm)
    keep = (rp, ci, vs)                                  # the handle wraps these tensors
    return h.value, p.H, lambda: (K.release_handle(p), check(lib.csrk_free(h.value)), keep)


def _restate(A, B, op):
    "combine_ref, vectorised over the whole matrix through (row, column) keys; A canonical for add / multiply, B canonical"
    arp, aci, avs = A
    brp, bci, bvs = B
    nr = len(arp) - 1
    width = int(max(aci.max(initial=0), bci.max(initial=0))) + 1
    ka = np.repeat(np.arange(nr, dtype=np.int64), np.diff(arp)) * width + aci
    kb = np.repeat(np.arange(nr, dtype=np.int64), np.diff(brp)) * width + bci      # ascending: B is canonical
    pos = np.searchsorted(kb, ka)
    hit = (pos < len(kb)) & (kb[np.minimum(pos, len(kb) - 1)] == ka) if len(kb) else np.zeros(len(ka), bool)
    wb = np.ones(len(kb)) if bvs is None else bvs.astype(np.float64)
    if op == 'drop':
        sel = ~hit
        keys, vals = ka[sel], avs[sel]
        cols = aci[sel]
    elif op == 'multiply':
        keys, vals, cols = ka[hit], avs[hit] * wb[pos[hit]], aci[hit]
    else:
        pa = ALPHA * avs
        both = pa.copy()
        both[hit] = pa[hit] + BETA * wb[pos[hit]]
        only_b = np.ones(len(kb), bool)
        only_b[pos[hit]] = False
        keys = np.concatenate([ka, kb[only_b]])
        vals = np.concatenate([both, BETA * wb[only_b]])
        o = np.argsort(keys, kind='stable')
        keys, vals = keys[o], vals[o]
        cols = (keys % width).astype(np.int32)
    rp = np.concatenate(([0], np.cumsum(np.bincount(keys // width, minlength=nr)))).astype(np.int32 if len(keys) <= 2 ** 31 - 1 else np.int64)
    return rp, cols.astype(np.int32), vals


def child(case, steps, warmup, parity):
    from csr_amd._lib import lib, check, handle_t
    from csr_amd.kernels import hip as K
    if case == 'e2e':
        return child_e2e(max(steps // 2, 5))
    name, op = case.split(':')
    HA, HB, free = _operands(name, op)
    code = K._COMBINE_OPS[op]

    def comb(keep=False):
        out = handle_t(0)
        check(lib.csrk_combine(HA, HB, code, ALPHA, BETA, C.byref(out)))
        if keep:
            return out.value
        check(lib.csrk_free(out.value))

    def filt():
        out = handle_t(0)
        check(lib.csrk_filter_zeros(HA, C.byref(out)))
        check(lib.csrk_free(out.value))

    ms, runs = _median_ms(comb, steps, warmup)
    fms, fruns = _median_ms(filt, steps, warmup)
    nr, nc, nnz, _, _ = K._info(HA)
    _, _, nnzb, _, vtb = K._info(HB)
    t1, t2 = K._wrap(comb(True)), K._wrap(comb(True))
    r1, r2 = K.from_handle(t1), K.from_handle(t2)
    K.release_handle(t1)
    K.release_handle(t2)
    repeat = all(x.tobytes() == y.tobytes() for x, y in ((r1.rowptrs, r2.rowptrs), (r1.colinds, r2.colinds), (r1.values, r2.values)))
    b_vals = 0 if op == 'drop' or vtb == 0 else 8 * nnzb
    parts = {'a': 4 * (nr + 1) + 12 * nnz, 'b': 4 * (nr + 1) + 4 * nnzb + b_vals, 'result': 4 * (nr + 1) + 12 * r1.nnz}
    total = sum(parts.values())
    gbs = total / ms / 1e6
    res = {'case': case, 'nrows': nr, 'nnz_a': nnz, 'nnz_b': nnzb, 'op': op, 'nnz_result': r1.nnz, 'ms': round(ms, 4), 'runs_ms': runs,
           'compulsory_bytes': parts, 'compulsory_total': total, 'gbs': round(gbs, 1),
           'frac_of_8TBs_roofline': round(gbs / HBM_PEAK_GBS, 4), 'filter_zeros_ms': round(fms, 4), 'filter_zeros_runs_ms': fruns,
           'combine_over_filter_zeros': round(ms / fms, 3), 'repeat_bitwise': bool(repeat)}
    if parity:
        from combine_ref import combine_ref, same
        A, B = K.from_handle(K.hip_h(HA, nr, nc, nnz)), K.from_handle(K.hip_h(HB, nr, nc, nnzb))
        ta, tb = (A.rowptrs, A.colinds, A.values), (B.rowptrs, B.colinds, B.values)
        t0 = time.perf_counter()
        exp = _restate(ta, tb, op)
        head = 200                                        # the vectorised form against the row-by-row one, on the leading rows
        cut = lambda t, n: (t[0][:n + 1], t[1][:t[0][n]], None if t[2] is None else t[2][:t[0][n]])      # noqa: E731
        head_ok = same(cut(exp, head), combine_ref(cut(ta, head), cut(tb, head), op, ALPHA, BETA), op)
        res['parity'] = {'ok': bool(head_ok and same((r1.rowptrs, r1.colinds, r1.values), exp, op)), 'restatement_head_ok': bool(head_ok),
                         'rows': nr, 'entries': r1.nnz, 'host_restatement_s': round(time.perf_counter() - t0, 2)}
    free()
    return res


def child_e2e(reps):
    "multiply_topk(exclude=) against the same call without exclude and against the host route, alternating"
    import scipy.sparse as sps
    from topk_ref import topk_rows_vec, same
    A, B = _block_operands()
    seen = _seen_block(A, B.nrows)
    mask = sps.csr_matrix((np.ones(seen.nnz), seen.colinds, seen.rowptrs), shape=(seen.nrows, seen.ncols))
    excl, plain, host = [], [], []
    one = two = None
    A.multiply_topk(B, 20, transpose=True, min_value=0.0, exclude=seen)      # warm-up: handles cached, pools filled
    for _ in range(reps):
        t0 = time.perf_counter()
        one = A.multiply_topk(B, 20, transpose=True, min_value=0.0, exclude=seen)
        excl.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        A.multiply_topk(B, 20, transpose=True, min_value=0.0)
        plain.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        P = A.multiply(B, transpose=True)
        S = sps.csr_matrix((P.values, P.colinds, P.rowptrs), shape=(P.nrows, P.ncols))
        U = (S - S.multiply(mask)).tocsr()                 # the unseen pairs (SciPy sorts the rows)
        topk_rows_vec(U.indptr, U.indices, U.data, 20, 0.0, 'descending')
        host.append(time.perf_counter() - t0)
        nnz = P.nnz
        if two is None:      # parity, untimed: the same removal in the product's own column order (ties go by position)
            d = _restate((P.rowptrs, P.colinds, P.values), (seen.rowptrs, seen.colinds, None), 'drop')
            two = topk_rows_vec(d[0], d[1], d[2], 20, 0.0, 'descending')
        del P, S, U
    e, p, h = float(np.median(excl)), float(np.median(plain)), float(np.median(host))
    return {'case': 'e2e', 'what': 'A[2000] x B[20000]^T of the MovieLens-25M-shaped matrix, k = 20, min_value = 0, by value; '
                                   'exclude = the ratings block cut to 20 000 columns',
            'product_nnz': nnz, 'excluded_pairs': seen.nnz, 'kept': one.nnz,
            'multiply_topk_exclude_s': round(e, 4), 'multiply_topk_exclude_runs_s': [round(t, 4) for t in excl],
            'multiply_topk_s': round(p, 4), 'multiply_topk_runs_s': [round(t, 4) for t in plain],
            'host_route_s': round(h, 4), 'host_route_runs_s': [round(t, 4) for t in host],
            'exclude_over_plain': round(e / p, 3), 'host_over_device': round(h / e, 2),
            'parity': {'ok': bool(same((one.rowptrs, one.colinds, one.values), two))}}


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
    print(json.dumps({'bench': 'combine', 'results': results, 'failed': failed,
                      'parity_ok': failed is None and all(r['parity']['ok'] for r in results)}), flush=True)
    sys.exit(0 if failed is None else 1)


if __name__ == '__main__':
    main()
