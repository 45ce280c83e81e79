"""
The expected result of row top-k (include/csrk.h, csrk_topk_rows), restated in NumPy for the tests: `topk_rows_ref` row by
row, as the contract reads; `topk_rows_vec` the same with one lexsort over the whole matrix, cheap enough to check every
row of every case.  tests/test_topk_host.py checks both against hand-written rows and against each other.
"""
import numpy as np


def widen(v):
    "float32 -> float64, exactly (a signalling NaN raises the invalid flag on the way: it is still a NaN, which is all that is read)"
    with np.errstate(invalid='ignore'):
        return v.astype(np.float64)


def topk_rows_ref(rp, ci, vs, k, min_value=-np.inf, order='descending'):
    orp, oci, ovs = [0], [ci[:0]], [vs[:0]]
    for i in range(len(rp) - 1):
        s, e = int(rp[i]), int(rp[i + 1])
        v = vs[s:e]
        w = widen(v)
        nan = np.isnan(w)
        key = np.where(nan, np.inf, w)                        # -0.0 == +0.0 under comparison
        o = np.lexsort((np.arange(e - s), -key, -nan.astype(np.int8)))   # NaN first, value descending, position ascending
        o = o[~(w < min_value)[o]][:k]                        # NaN passes the threshold
        if order == 'storage':
            o = np.sort(o)
        oci.append(ci[s:e][o])
        ovs.append(v[o])
        orp.append(orp[-1] + len(o))
    return np.array(orp, dtype=np.int64), np.concatenate(oci), np.concatenate(ovs)


def topk_keep(rp, vs, k, min_value=-np.inf):
    "indices into the matrix's arrays of the kept entries, row by row, best first; and the result's row pointers"
    rp = np.asarray(rp).astype(np.int64)
    nr = len(rp) - 1
    w = widen(vs)
    idx = np.flatnonzero(~(w < min_value))
    row = np.repeat(np.arange(nr, dtype=np.int64), np.diff(rp))[idx]
    nan = np.isnan(w[idx])
    key = np.where(nan, np.inf, w[idx])
    o = np.lexsort((idx, -key, -nan.astype(np.int8), row))    # (a row's entries ascend in idx as they do in position)
    cnt = np.bincount(row, minlength=nr)
    start = np.concatenate(([0], np.cumsum(cnt)))[:-1]
    sel = o[np.arange(len(o), dtype=np.int64) - np.repeat(start, cnt) < k]
    orp = np.concatenate(([0], np.cumsum(np.bincount(row[sel], minlength=nr)))).astype(np.int64)
    return idx[sel], orp


def topk_rows_vec(rp, ci, vs, k, min_value=-np.inf, order='descending', keep=None):
    "keep: a topk_keep(rp, vs, k, min_value) result to reuse (both orders of one selection)"
    keep, orp = topk_keep(rp, vs, k, min_value) if keep is None else keep
    if order == 'storage':
        keep = np.sort(keep)                                  # rows ascend in the index, and so do positions inside a row
    return orp, ci[keep], vs[keep]


def bits(a):
    "a float array as integers of its width: equality of these is equality bit for bit (NaN payloads, -0.0)"
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def same(got, exp):
    "rowptrs, colinds and values equal, the values bit for bit and of the same dtype"
    grp, gci, gvs = got
    erp, eci, evs = exp
    return (np.array_equal(np.asarray(grp).astype(np.int64), np.asarray(erp).astype(np.int64)) and np.array_equal(gci, eci)
            and gvs.dtype == evs.dtype and np.array_equal(bits(gvs), bits(evs)))
