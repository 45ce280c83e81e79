"""
References for csrk_als_rows_cg (include/csrk.h, rule C), none of which touches the library:

  cg_exact         rules C2 - C7 restated step by step.  Every fma is the exact value rounded once (als_ref.fnma:
                   fma(a, b, c) = fnma(-a, b, c)); the tree additions, the multiply by w_e, the subtraction of C5 and the two
                   divisions are plain float64 operations.  Returns (x [n, k], resid [n], taken [n]).  About 1 s for one row
                   at k = 128 with a dense base, 5 entries and 3 steps, 0.25 s at k = 64: callers size their cases by that.
  cg_two_rounding  the same with multiply-then-add: what a kernel without a fused multiply-add would give.  Only to show
                   that cg_exact can tell the two apart.
  cg_numpy         float64 NumPy with each row's entries taken ascending (order=+1) or descending (order=-1): for rows too
                   long for cg_exact.  The sums over entries are strictly sequential (cumsum), so the two orders are two
                   honest orders of addition.
  owner            C2's partial of element t;  dot  C2 itself.
"""
import numpy as np

from als_ref import fnma, _c

RHS = ('ones', 'values', 'one_plus_values')


def _fma(a, b, c, fused=True):
    return fnma(-float(a), b, c, fused)


def owner(t, f32):
    "rule C2: the partial that element t belongs to"
    return (t % 64) // 4 if f32 else (t % 32) // 2


def _add(a, b):
    with np.errstate(all='ignore'):
        return float(np.float64(a) + np.float64(b))


def _mul(a, b):
    with np.errstate(all='ignore'):
        return float(np.float64(a) * np.float64(b))


def _div(a, b):
    with np.errstate(all='ignore'):
        return float(np.float64(a) / np.float64(b))


def dot(a, b, f32, fused=True):
    "rule C2"
    s = [0.0] * 16
    for t in range(len(a)):
        l = owner(t, f32)
        s[l] = _fma(a[t], b[t], s[l], fused)
    while len(s) > 1:
        s = [_add(s[i], s[i + 1]) for i in range(0, len(s), 2)]
    return s[0]


def _row(k, vs, w, c, base, rho, steps, tol2, x0, f32, fused):
    "one row: vs its V rows as lists of floats in storage order, w its weights (None: no scaling), c its rhs coefficients"

    def matvec(y):
        q = [0.0] * k
        if base is not None:
            for u in range(k):
                bu, yu = base[u], y[u]
                for t in range(k):
                    q[t] = _fma(bu[t], yu, q[t], fused)
        for t in range(k):
            q[t] = _fma(rho, y[t], q[t], fused)
        for e, v in enumerate(vs):
            d = dot(v, y, f32, fused)
            g = d if w is None else _mul(w[e], d)
            for t in range(k):
                q[t] = _fma(g, v[t], q[t], fused)
        return q

    b = [0.0] * k
    for e, v in enumerate(vs):
        for t in range(k):
            b[t] = _fma(c[e], v[t], b[t], fused)
    if x0 is None:
        x, r = [0.0] * k, list(b)
    else:
        x = [float(a) for a in x0]
        q = matvec(x)
        r = [_add(b[t], -q[t]) for t in range(k)]
    p = list(r)
    rs = dot(r, r, f32, fused)
    taken = 0
    while taken < steps and rs > tol2:
        q = matvec(p)
        pq = dot(p, q, f32, fused)
        alpha = _div(rs, pq)
        for t in range(k):
            x[t] = _fma(alpha, p[t], x[t], fused)
            r[t] = _fma(-alpha, q[t], r[t], fused)
        rn = dot(r, r, f32, fused)
        beta = _div(rn, rs)
        for t in range(k):
            p[t] = _fma(beta, p[t], r[t], fused)
        rs = rn
        taken += 1
    return x, rs, taken


def cg_exact(rowptrs, colinds, values, V, scale=False, rhs='values', base=None, lam=0.0, lam_n=0.0, steps=3, tol2=0.0, x0=None,
             rows=None, fused=True):
    "(x [n, k], resid [n], taken [n]): rules C1 - C7 restated"
    assert rhs in RHS
    V = np.asarray(V)
    f32 = V.dtype == np.float32
    k = V.shape[1]
    n = len(rowptrs) - 1
    rb, re_ = (0, n) if rows is None else rows
    Vf = {}
    B = None if base is None else [[float(a) for a in row] for row in np.asarray(base)]      # B[u][t] = base[u * k + t]
    xs, rss, tk = np.zeros((re_ - rb, k)), np.zeros(re_ - rb), np.zeros(re_ - rb, np.int32)
    for i in range(rb, re_):
        e0, e1 = int(rowptrs[i]), int(rowptrs[i + 1])
        for e in range(e0, e1):
            j = int(colinds[e])
            if j not in Vf:
                Vf[j] = [float(a) for a in V[j]]
        vs = [Vf[int(colinds[e])] for e in range(e0, e1)]
        w = [float(values[e]) for e in range(e0, e1)] if (scale and values is not None) else None
        c = [_c(values, rhs, e) for e in range(e0, e1)]
        rho = _fma(float(lam_n), float(e1 - e0), float(lam))
        x, rs, t = _row(k, vs, w, c, B, rho, steps, tol2, None if x0 is None else x0[i - rb], f32, fused)
        xs[i - rb], rss[i - rb], tk[i - rb] = x, rs, t
    return xs, rss, tk


def cg_two_rounding(*a, **kw):
    return cg_exact(*a, fused=False, **kw)


def cg_numpy(rowptrs, colinds, values, V, scale=False, rhs='values', base=None, lam=0.0, lam_n=0.0, steps=3, tol2=0.0, x0=None,
             rows=None, order=1):
    "(x, resid, taken) in float64 NumPy, each row's entries summed ascending (order=+1) or descending (order=-1)"
    assert rhs in RHS and order in (1, -1)
    V = np.asarray(V, dtype=np.float64)
    k = V.shape[1]
    n = len(rowptrs) - 1
    rb, re_ = (0, n) if rows is None else rows
    xs, rss, tk = np.zeros((re_ - rb, k)), np.zeros(re_ - rb), np.zeros(re_ - rb, np.int32)
    B = None if base is None else np.asarray(base, dtype=np.float64)
    for i in range(rb, re_):
        e0, e1 = int(rowptrs[i]), int(rowptrs[i + 1])
        Vr = V[np.asarray(colinds[e0:e1], dtype=np.int64)][::order]
        vals = np.ones(e1 - e0) if values is None else np.asarray(values[e0:e1], dtype=np.float64)[::order]
        w = vals if scale else np.ones(e1 - e0)
        c = np.ones(e1 - e0) if rhs == 'ones' else (vals if rhs == 'values' else 1.0 + vals)
        rho = lam + lam_n * (e1 - e0)

        def seq(G):          # the sum over entries of G[e] * Vr[e], one entry after the other
            return np.cumsum(G[:, None] * Vr, axis=0)[-1] if len(G) else np.zeros(k)

        def matvec(y):
            q = (B.T @ y if B is not None else np.zeros(k)) + rho * y
            return q + seq(w * (Vr @ y))

        b = seq(c)
        if x0 is None:
            x, r = np.zeros(k), b.copy()
        else:
            x = np.array(x0[i - rb], dtype=np.float64)
            r = b - matvec(x)
        p, rs, t = r.copy(), float(r @ r), 0
        with np.errstate(all='ignore'):
            while t < steps and rs > tol2:
                q = matvec(p)
                alpha = rs / float(p @ q)
                x = x + alpha * p
                r = r - alpha * q
                rn = float(r @ r)
                p = r + (rn / rs) * p
                rs = rn
                t += 1
        xs[i - rb], rss[i - rb], tk[i - rb] = x, rs, t
    return xs, rss, tk
