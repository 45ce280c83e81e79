"""
csrk_knn_scores restated as a plain float64 Python loop of rules 2-4 of its contract (include/csrk.h).  No step of the
contract is fused, so Python's *, +, / and abs on floats ARE its roundings and the GPU tests compare bit for bit.
Matrices are (rowptrs, colinds, values) tuples; values may be float64, float32 (widened exactly) or None (1.0 everywhere).
"""
import numpy as np

AGGREGATES = ('weighted-average', 'sum')


def _value(vs, e):
    return 1.0 if vs is None else float(vs[e])


def _div(num, den):
    "one IEEE division: Python raises where IEEE gives NaN or Inf"
    with np.errstate(all='ignore'):
        return float(np.float64(num) / np.float64(den))


def knn_scores_ref(model, ratings, users, max_nbrs=0, min_nbrs=1, aggregate='weighted-average', offsets=None):
    "(rowptrs int32, colinds int32, values float64) of the result [len(users) x n_targets]"
    assert aggregate in AGGREGATES and max_nbrs >= 0 and min_nbrs >= 1
    mrp, mci, mvs = model
    rrp, rci, rvs = ratings
    n_targets = len(mrp) - 1
    rp, ci, vs = [0], [], []
    for r, u in enumerate(users):
        b, e = int(rrp[u]), int(rrp[u + 1])
        cols = [int(c) for c in rci[b:e]]
        assert all(x < y for x, y in zip(cols, cols[1:])), f'ratings row {u} is not strictly ascending'
        rated = {c: b + k for k, c in enumerate(cols)}
        for i in range(n_targets):
            num, den, nn = 0.0, 0.0, 0
            for x in range(int(mrp[i]), int(mrp[i + 1])):
                at = rated.get(int(mci[x]))
                if at is None:
                    continue
                s = _value(mvs, x)
                if aggregate == 'sum':
                    num = num + s
                else:
                    t = _value(rvs, at) * s
                    num = num + t
                    den = den + abs(s)
                nn += 1
                if max_nbrs > 0 and nn == max_nbrs:
                    break
            if nn < min_nbrs:
                continue
            v = num if aggregate == 'sum' else _div(num, den)
            if offsets is not None:
                v = v + float(offsets[r])
            ci.append(i)
            vs.append(v)
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(vs, np.float64)


def knn_scores_dense(M, has_m, R, has_r, users, max_nbrs=0, min_nbrs=1, aggregate='weighted-average', offsets=None):
    """
    The same rule over dense arrays for a model WITHOUT repeated columns whose rows are stored in ascending column order:
    M, R hold the values, has_m, has_r say which positions are stored.  Returns (stored [m x T] bool, value [m x T]).
    """
    T = M.shape[0]
    stored, value = np.zeros((len(users), T), bool), np.zeros((len(users), T))
    for r, u in enumerate(users):
        for i in range(T):
            hits = np.flatnonzero(has_m[i] & has_r[u])
            if max_nbrs > 0:
                hits = hits[:max_nbrs]
            if len(hits) < min_nbrs:
                continue
            num = den = 0.0
            for j in hits:
                if aggregate == 'sum':
                    num = num + float(M[i, j])
                else:
                    num = num + float(R[u, j]) * float(M[i, j])
                    den = den + abs(float(M[i, j]))
            v = num if aggregate == 'sum' else _div(num, den)
            if offsets is not None:
                v = v + float(offsets[r])
            stored[r, i], value[r, i] = True, v
    return stored, value


def same(got, exp):
    "row pointers (int32: rule 4), columns and value BITS agree; a NaN stands for any NaN (rule 6)"
    if np.asarray(got[0]).dtype != np.int32 or not np.array_equal(np.asarray(got[0], np.int64), np.asarray(exp[0], np.int64)):
        return False
    if got[1].dtype != np.int32 or not np.array_equal(got[1], exp[1]):
        return False
    g, e = np.asarray(got[2]), np.asarray(exp[2])
    if g.dtype != np.float64 or g.shape != e.shape:
        return False
    nan = np.isnan(e)
    if not np.array_equal(np.isnan(g), nan):
        return False
    return np.array_equal(g[~nan].view(np.uint64), e[~nan].view(np.uint64))


def first_difference(got, exp):
    if not np.array_equal(np.asarray(got[0], np.int64), np.asarray(exp[0], np.int64)):
        d = np.flatnonzero(np.asarray(got[0], np.int64)[:len(exp[0])] != np.asarray(exp[0], np.int64)[:len(got[0])])
        return f'rowptrs differ first at {d[0] if len(d) else "the end"}: lengths {len(got[0])} / {len(exp[0])}'
    if not np.array_equal(got[1], exp[1]):
        d = np.flatnonzero(got[1] != exp[1])
        return f'colinds differ first at {d[0]}: {got[1][d[0]]} / {exp[1][d[0]]}'
    g, e = np.asarray(got[2], np.float64), np.asarray(exp[2], np.float64)
    d = np.flatnonzero((g.view(np.uint64) != e.view(np.uint64)) & ~(np.isnan(g) & np.isnan(e)))
    return f'values differ first at {d[0]}: {g[d[0]]!r} / {e[d[0]]!r}' if len(d) else 'dtype or shape'
