#!/usr/bin/env python3
"""
csrk_knn_scores on synth.movielens_like() (162 541 users x 59 047 items, nnz 25 000 095), ratings mean-centred per user
(center_rows; the means go back in as offsets).  The item-kNN model is built ONCE, in a process of its own, with the
library's own operations and kept in a scratch directory: the centred ratings transposed, item rows unit-normalised, and per
block of --block item rows mult_abt -> filter_zeros -> combine 'drop' against the diagonal (an item is not its own
neighbour) -> topk_rows(20, min_value = --min-sim, 'descending').  Then, per batch of 1, 64, 1 024 and 16 384 random users,
each in a fresh process under `timeout -k 10`, with max_nbrs = 20 and after --warmup calls, wall-clock per call (every
entry here waits for the device before it returns; median, min, max, quartiles):
  scores   knn_scores (weighted average, offsets = the users' means), handle in, handle out;
  topk     the chain of CSR.knn_topk on handles: knn_scores -> pick_rows(ratings, users, no values) -> combine 'drop' ->
           topk_rows(20) -> from_handle: only 20 entries per user cross PCIe;
  product  (a) the existing device route that computes the UNLIMITED sum: pick_rows(users) -> mult_abt(model).  It cannot
           express max_nbrs, min_nbrs or the division; it is the only on-device competitor;
  numpy    (b) the host route: a NumPy restatement of the rule over the padded model, one user at a time, on the first
           --numpy-users users of the batch; its values must equal `scores` bit for bit (checked).
A second `scores` call must give the same bits (checked).  The parent prints one JSON line and writes it to --out.
Both routes of knn_scores are measured, each in fresh processes that alternate -- per batch and per min_nbrs in (1, 2): 'walk'
(every target of every user), then 'reach' (only the targets the user's ratings reach; csrk_knn_scores_reach).  The walk
child with min_nbrs = 1 is the run described above; the others time `scores` alone.  A reach child first builds the model's
reach index and reports that one-off time (`index`), and after its timings scores the batch by the walk route too: the two
results must be the same bits (`routes_same_bits`).  `routes` in the result line puts the pairs side by side: the reach
route's median against the walk route's minimum of the same session, and the calls after which the index build is paid for.
    python tools/bench_knn_scores.py [--batches 1,64,1024,16384] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K_NBRS = 20
N_TOP = 20


def _stats(ts, warmup):
    q = np.percentile(ts, [0, 25, 50, 75, 100])
    return {'median_ms': round(float(q[2]), 3), 'min_ms': round(float(q[0]), 3), 'q25_ms': round(float(q[1]), 3),
            'q75_ms': round(float(q[3]), 3), 'max_ms': round(float(q[4]), 3), 'steps': len(ts), 'warmup': warmup}


def _timed(fn, steps, warmup):
    "fn does its own waiting (the library's handle-returning entries drain the device); the result of the last call comes back too"
    import torch
    out = None
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return _stats(ts, warmup), out


def _ratings():
    "the centred ratings as a handle, and the users' means"
    import torch
    from csr_amd import synth
    from csr_amd._lib import lib, check, handle_t, VAL_F64
    from csr_amd.kernels import hip as K
    m = synth.movielens_like(device='cuda')
    rp, ci, vs = m['rowptrs'], m['colinds'], m['values']
    nr, nc, nnz = m['nrows'], m['ncols'], int(ci.numel())
    H = handle_t(0)
    check(lib.csrk_create_device(nr, nc, nnz, rp.data_ptr(), int(rp.dtype == torch.int64), ci.data_ptr(), vs.data_ptr(), VAL_F64, C.byref(H)))
    torch.cuda.synchronize()
    del m, rp, ci, vs
    h = K.hip_h(H.value, nr, nc, nnz)
    assert K.is_canonical(h) == (True, None)                    # the one look at the rows, outside the timings
    means = K.center_rows(h)
    return h, means


def build_model(path, block, min_sim):
    import torch
    from csr_amd import CSR
    from csr_amd.kernels import hip as K
    t0 = time.perf_counter()
    h, _ = _ratings()
    items = K.transpose(h)
    K.unit_rows(items)
    n_items = items.nrows
    blocks, products_ms = [], 0.0
    for b0 in range(0, n_items, block):
        b1 = min(b0 + block, n_items)
        rows = np.arange(b0, b1, dtype=np.int32)
        eye = CSR(b1 - b0, n_items, b1 - b0, np.arange(b1 - b0 + 1, dtype=np.int32), rows.copy(), None)
        t1 = time.perf_counter()
        blk = K.pick_rows(items, rows)
        prod = K.mult_abt(blk, items)
        torch.cuda.synchronize()
        products_ms += (time.perf_counter() - t1) * 1e3
        kept = K.filter_zeros(prod)
        K.release_handle(prod)
        eye_h = K.to_handle(eye)
        off_diag = K.combine(kept, eye_h, 'drop')
        top = K.topk_rows(off_diag, K_NBRS, min_sim, 'descending')
        blocks.append(K.from_handle(top))
        for x in (blk, kept, eye_h, off_diag, top):
            K.release_handle(x)
    model = blocks[0] if len(blocks) == 1 else CSR._assemble_shards(blocks)
    np.save(os.path.join(path, 'rp.npy'), model.rowptrs)
    np.save(os.path.join(path, 'ci.npy'), model.colinds)
    np.save(os.path.join(path, 'vs.npy'), model.values)
    lens = np.diff(model.rowptrs)
    return {'n_targets': int(model.nrows), 'n_items': int(model.ncols), 'nnz': int(model.nnz), 'k': K_NBRS, 'min_sim': min_sim,
            'row_len_mean': round(float(lens.mean()), 2), 'rows_full': int((lens == K_NBRS).sum()), 'rows_empty': int((lens == 0).sum()),
            'block_rows': block, 'products_ms': round(products_ms, 1), 'build_s': round(time.perf_counter() - t0, 2)}


def numpy_scores(mrp, mci, mvs, cols, vals, max_nbrs, offset):
    """
    The rule for ONE user over the model padded to its longest row: position by position in storage order, so that every
    add happens in the contract's order (adding an exact 0.0 for a miss changes no bit of a sum that is not -0.0).
    Returns (targets stored, their values).
    """
    lens = np.diff(mrp)
    width = int(lens.max()) if len(lens) else 0
    at = mrp[:-1, None] + np.arange(width)[None, :]
    inside = np.arange(width)[None, :] < lens[:, None]
    at = np.where(inside, at, 0)
    c, s = mci[at], mvs[at]
    pos = np.searchsorted(cols, c)
    pos = np.minimum(pos, max(len(cols) - 1, 0))
    hit = inside & (cols[pos] == c) if len(cols) else np.zeros_like(inside)
    nn = np.cumsum(hit, axis=1)
    use = hit & (nn <= max_nbrs) if max_nbrs > 0 else hit
    v = vals[pos] if len(cols) else np.zeros_like(s)
    num, den = np.zeros(len(lens)), np.zeros(len(lens))
    for j in range(width):
        u = use[:, j]
        num = num + np.where(u, v[:, j] * s[:, j], 0.0)
        den = den + np.where(u, np.abs(s[:, j]), 0.0)
    stored = use.any(axis=1)
    with np.errstate(all='ignore'):
        val = num[stored] / den[stored] + offset
    return np.flatnonzero(stored).astype(np.int32), val


def _same_bits(a, b):
    return bool(np.array_equal(a.rowptrs, b.rowptrs) and np.array_equal(a.colinds, b.colinds) and a.values.tobytes() == b.values.tobytes())


def child(path, n_users, steps, warmup, numpy_users, route='walk', min_nbrs=1):
    import torch
    from csr_amd import CSR
    from csr_amd.kernels import hip as K, releasing
    K_releasing = lambda x: releasing(x, K)      # noqa: E731
    h, means = _ratings()
    mrp, mci, mvs = (np.load(os.path.join(path, f)) for f in ('rp.npy', 'ci.npy', 'vs.npy'))
    model = CSR(len(mrp) - 1, h.ncols, len(mci), mrp, mci, mvs, _cast=False)
    m_h = K.to_handle(model)
    g = np.random.default_rng(31)
    users = g.choice(h.nrows, size=n_users, replace=False).astype(np.int32)
    off = np.ascontiguousarray(means[users], dtype=np.float64)
    rec = {'users': n_users, 'max_nbrs': K_NBRS, 'n_top': N_TOP, 'route': route, 'min_nbrs': min_nbrs}
    if n_users >= 4096:
        steps = max(3, steps // 4)
    keep = []
    if route == 'reach':                 # the one-off cost of the route: the index the model handle keeps
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        entries, nbytes = K.knn_reach_index(m_h)
        torch.cuda.synchronize()
        rec['index'] = {'build_ms': round((time.perf_counter() - t0) * 1e3, 3), 'entries': entries, 'bytes': nbytes}

    def scores():
        for x in keep:
            K.release_handle(x)
        keep[:] = [K.knn_scores(m_h, h, users, K_NBRS, min_nbrs, 'weighted-average', off, route=route)]
        return keep[0]
    rec['scores'], s_h = _timed(scores, steps, warmup)
    rec['scores_nnz'] = int(s_h.nnz)
    if route == 'reach':
        rec['last_stats'] = dict(zip(K.KNN_STATS, K.knn_scores_last_stats()))
    small = s_h.nnz <= 50_000_000
    first = K.from_handle(s_h) if small else None
    if route != 'walk' or min_nbrs != 1:       # `scores` alone, and for the reach route the same batch by the walk route
        if small:
            rec['second_call_same_bits'] = _same_bits(first, K.from_handle(scores()))
            if route == 'reach':
                with K_releasing(K.knn_scores(m_h, h, users, K_NBRS, min_nbrs, 'weighted-average', off)) as wh:
                    rec['routes_same_bits'] = _same_bits(first, K.from_handle(wh))
        rec['parity'] = {'ok': bool(rec.get('second_call_same_bits', True) and rec.get('routes_same_bits', True))}
        for x in keep + [m_h, h]:
            K.release_handle(x)
        torch.cuda.synchronize()
        return rec

    def topk():
        with K_releasing(K.knn_scores(m_h, h, users, K_NBRS, 1, 'weighted-average', off)) as sh:
            with K_releasing(K.pick_rows(h, users, False)) as xh:
                with K_releasing(K.combine(sh, xh, 'drop')) as dh:
                    with K_releasing(K.topk_rows(dh, N_TOP, None, 'descending')) as th:
                        return K.from_handle(th)
    rec['topk'], top = _timed(topk, steps, warmup)
    rec['topk_nnz'] = int(top.nnz)

    def product():
        with K_releasing(K.pick_rows(h, users)) as ph:
            with K_releasing(K.mult_abt(ph, m_h)) as ch:
                return ch.nnz
    rec['product'], pn = _timed(product, max(3, steps // 2), 1)
    rec['product_nnz'] = int(pn)
    if small:
        rec['second_call_same_bits'] = _same_bits(first, K.from_handle(scores()))
        # the host route on a sample: the first numpy_users users of the batch
        rp = np.empty(h.nrows + 1, np.int32)
        ci = np.empty(h.nnz, np.int32)
        vs = np.empty(h.nnz, np.float64)
        from csr_amd._lib import lib, check
        check(lib.csrk_export(h.H, rp.ctypes.data, ci.ctypes.data, vs.ctypes.data))
        ts, ok = [], True
        for r, u in enumerate(users[:numpy_users]):
            b, e = rp[u], rp[u + 1]
            t0 = time.perf_counter()
            tg, val = numpy_scores(mrp, mci, mvs, ci[b:e], vs[b:e], K_NBRS, off[r])
            ts.append((time.perf_counter() - t0) * 1e3)
            fb, fe = first.rowptrs[r], first.rowptrs[r + 1]
            nan = np.isnan(val)
            ok = ok and np.array_equal(tg, first.colinds[fb:fe]) and np.array_equal(nan, np.isnan(first.values[fb:fe])) and \
                val[~nan].tobytes() == first.values[fb:fe][~nan].tobytes()
        rec['numpy_per_user'] = _stats(ts, 0)
        rec['numpy_users'] = int(min(numpy_users, n_users))
        rec['numpy_equals_scores_bitwise'] = bool(ok)
        rec['scores_ms_per_user'] = round(rec['scores']['median_ms'] / n_users, 5)
    rec['scores_over_product'] = round(rec['scores']['median_ms'] / rec['product']['median_ms'], 4)
    rec['parity'] = {'ok': bool(rec.get('second_call_same_bits', True) and rec.get('numpy_equals_scores_bitwise', True))}
    for x in keep + [m_h, h]:
        K.release_handle(x)
    torch.cuda.synchronize()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,64,1024,16384')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--numpy-users', type=int, default=8, help='users of each batch the NumPy restatement scores')
    ap.add_argument('--block', type=int, default=4096, help='item rows per product block while the model is built')
    ap.add_argument('--min-sim', type=float, default=1e-9, help='smallest similarity kept in the model (> 0)')
    ap.add_argument('--child-timeout', type=int, default=300)
    ap.add_argument('--model-dir', default=None, help='keep the model here (and reuse one that is there)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', default=None, help='(internal) "model" or a number of users')
    ap.add_argument('--route', default='walk', help='(internal) the route a child measures')
    ap.add_argument('--min-nbrs', type=int, default=1, help='(internal) min_nbrs of a child')
    ap.add_argument('--routes', default='walk,reach', help='routes to measure, alternating per batch')
    a = ap.parse_args()
    if a.child == 'model':
        print(json.dumps(build_model(a.model_dir, a.block, a.min_sim)), flush=True)
        return
    if a.child is not None:
        print(json.dumps(child(a.model_dir, int(a.child), a.steps, a.warmup, a.numpy_users, a.route, a.min_nbrs)), flush=True)
        return
    tmp = None
    if a.model_dir is None:
        tmp = tempfile.TemporaryDirectory()
        a.model_dir = tmp.name
    os.makedirs(a.model_dir, exist_ok=True)
    base = ['timeout', '-k', '10', str(a.child_timeout), sys.executable, os.path.abspath(__file__), '--model-dir', a.model_dir, '--steps',
            str(a.steps), '--warmup', str(a.warmup), '--numpy-users', str(a.numpy_users), '--block', str(a.block), '--min-sim', str(a.min_sim)]
    model, results, others, failed = None, [], [], None
    routes = a.routes.split(',')
    jobs = [] if os.path.exists(os.path.join(a.model_dir, 'vs.npy')) else [('model', 'walk', 1)]
    jobs += [(b, route, mn) for b in a.batches.split(',') for mn in (1, 2) for route in routes]
    for job, route, mn in jobs:
        p = subprocess.run(base + ['--child', job, '--route', route, '--min-nbrs', str(mn)], cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
        if p.returncode != 0 or not lines:
            failed = {'job': job, 'route': route, 'min_nbrs': mn, 'returncode': p.returncode, 'stderr': p.stderr[-2000:]}
            break                      # a child that failed ends the run: nothing more is started on the GPU
        r = json.loads(lines[-1])
        if job == 'model':
            model = r
            print(f'[bench_knn_scores] model: {r}', file=sys.stderr, flush=True)
            continue
        if route == 'walk' and mn == 1:
            results.append(r)
            print(f'[bench_knn_scores] {r["users"]} users: scores {r["scores"]["median_ms"]} ms ({r["scores_nnz"]} entries), topk '
                  f'{r["topk"]["median_ms"]} ms, product {r["product"]["median_ms"]} ms ({r["product_nnz"]} entries), numpy per user '
                  f'{r.get("numpy_per_user", {}).get("median_ms")} ms, parity {r["parity"]["ok"]}', file=sys.stderr, flush=True)
        else:
            others.append(r)
            print(f'[bench_knn_scores] {r["users"]} users, {route}, min_nbrs {mn}: scores {r["scores"]["median_ms"]} ms '
                  f'({r["scores_nnz"]} entries), index {r.get("index")}, parity {r["parity"]["ok"]}', file=sys.stderr, flush=True)
    # the routes side by side, per batch and min_nbrs
    table = []
    by = {(r['users'], r['min_nbrs'], r['route']): r for r in results + others}
    for (users, mn, route), r in sorted(by.items()):
        w = by.get((users, mn, 'walk'))
        if route != 'reach' or w is None:
            continue
        row = {'users': users, 'min_nbrs': mn, 'walk': w['scores'], 'reach': r['scores'], 'scores_nnz': r['scores_nnz'],
               'same_entries': r['scores_nnz'] == w['scores_nnz'], 'routes_same_bits': r.get('routes_same_bits'),
               'index_build_ms': r['index']['build_ms'], 'reach_median_below_walk_min': r['scores']['median_ms'] < w['scores']['min_ms'],
               'walk_median_over_reach_median': round(w['scores']['median_ms'] / r['scores']['median_ms'], 3)}
        gain = w['scores']['median_ms'] - r['scores']['median_ms']
        row['calls_to_pay_for_the_index'] = None if gain <= 0 else int(np.ceil(r['index']['build_ms'] / gain))
        product = by.get((users, 1, 'walk'), {}).get('product')
        if product:
            row['product_median_ms'] = product['median_ms']
        table.append(row)
    every = results + others
    line = json.dumps({'bench': 'knn_scores', 'workload': 'synth.movielens_like() centred per user; item-kNN model of 20 neighbours from '
                       'unit item rows (mult_abt -> filter_zeros -> drop diagonal -> topk_rows); max_nbrs 20, min_nbrs 1, weighted '
                       'average, offsets = user means; wall-clock per call', 'model': model, 'results': results, 'other_runs': others,
                       'routes': table, 'failed': failed,
                       'parity_ok': failed is None and all(r['parity']['ok'] for r in every) and all(t['same_entries'] for t in table)})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(line + '\n')
    if tmp is not None:
        tmp.cleanup()
    sys.exit(0 if failed is None else 1)


if __name__ == '__main__':
    main()
