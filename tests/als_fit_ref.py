"""
References for csrk_panel_gram, csrk_als_objective[_rows] and csrk_als_fit (include/csrk.h, rules P, J, T and F).  None
of the *_exact functions touches the library:

  tree_sum              rule P3 / the tree of rule T: adjacent pairs level by level, an unpaired last one carried unchanged.
                        Works on floats and on NumPy arrays (element-wise float64 additions are IEEE additions).
  panel_gram_exact      rule P restated step by step; every fma is the exact value rounded once (als_ref.fnma).  About 10^5
                        fused steps per second: k (k + 1) / 2 of them per row of V.  Callers size their cases by that.
  panel_gram_two_rounding   the same with multiply-then-add: only to show that panel_gram_exact can tell the two apart.
  chunk_sum             rule T: serial chunks of a constant length from +0.0, then the tree.
  objective_rows_exact  rule J1, with als_cg_ref.dot for DOT.
  objective_exact       rule J2.
  loss_numpy            the plain losses in float64 NumPy with their documented constants and the magnitudes a summation
                        bound needs.
  fit_by_parts          rule F's loop written with the public host entries of a kernel module K (panel_gram, als_rows,
                        als_rows_cg, als_objective): this one does call the library, that is its point.
"""
import numpy as np

from als_cg_ref import _add, _fma, _mul, dot
from als_ref import _c


def tree_sum(parts):
    "rule P3 over a list of floats or of equal-shaped float64 arrays; an empty list sums to +0.0"
    parts = list(parts)
    if not parts:
        return 0.0
    with np.errstate(all='ignore'):
        while len(parts) > 1:
            nxt = [parts[i] + parts[i + 1] for i in range(0, len(parts) - 1, 2)]
            if len(parts) % 2:
                nxt.append(parts[-1])
            parts = nxt
    return parts[0]


def panel_gram_exact(V, ridge, R, fused=True):
    "rule P: G [k, k] float64"
    V = np.asarray(V)
    n, k = V.shape
    Vf = [[float(x) for x in r] for r in V]          # float32 widens exactly
    parts = []
    for c0 in range(0, n, R):
        S = np.zeros((k, k))
        rows = Vf[c0:min(c0 + R, n)]
        for t in range(k):
            for u in range(t + 1):
                s = 0.0
                for v in rows:
                    s = _fma(v[t], v[u], s, fused)
                S[t, u] = s
        parts.append(S)
    total = tree_sum(parts) if parts else np.zeros((k, k))
    G = np.zeros((k, k))
    for t in range(k):
        for u in range(t):
            G[t, u] = G[u, t] = total[t, u]
        G[t, t] = _add(total[t, t], ridge)
    return G


def panel_gram_two_rounding(V, ridge, R):
    return panel_gram_exact(V, ridge, R, fused=False)


def chunk_sum(x, L):
    "rule T over a float64 array: chunks of L elements added serially from +0.0, ascending, then tree_sum of the partials"
    x = [float(a) for a in np.asarray(x, dtype=np.float64).ravel()]
    parts = []
    for c0 in range(0, len(x), L):
        s = 0.0
        for a in x[c0:c0 + L]:
            s = _add(s, a)
        parts.append(s)
    return float(tree_sum(parts))


def objective_rows_exact(rowptrs, colinds, values, U, V, scale=False, rhs='values', lam=0.0, lam_n=0.0, data=True, rows=None,
                         fused=True):
    "rule J1: J [row_end - row_begin] float64.  data=False: only the regulariser (V, colinds and values are not looked at)"
    U = np.asarray(U, dtype=np.float64)
    n = len(rowptrs) - 1
    rb, re_ = (0, n) if rows is None else rows
    out = np.zeros(re_ - rb)
    Vf = {}
    for i in range(rb, re_):
        e0, e1 = int(rowptrs[i]), int(rowptrs[i + 1])
        u = [float(a) for a in U[i]]
        J = 0.0
        if data:
            for e in range(e0, e1):
                j = int(colinds[e])
                if j not in Vf:
                    Vf[j] = [float(a) for a in V[j]]
                s = dot(u, Vf[j], False, fused)
                g = _mul(float(values[e]), s) if (scale and values is not None) else s
                h = _add(g, -2.0 * _c(values, rhs, e))
                J = _fma(h, s, J, fused)
        rho = _fma(float(lam_n), float(e1 - e0), float(lam), fused)
        out[i - rb] = _fma(rho, dot(u, u, False, fused), J, fused)
    return out


def objective_exact(a, at_rowptrs, U, V, scale, rhs, implicit, lam, lam_n, R, L):
    "rule J2.  a = (rowptrs, colinds, values) of A; at_rowptrs: the row pointers of A^T; R, L: rule P's and rule T's chunk lengths"
    rp, ci, vs = a
    ja = chunk_sum(objective_rows_exact(rp, ci, vs, U, V, scale, rhs, lam, lam_n), L)
    jt = chunk_sum(objective_rows_exact(at_rowptrs, None, None, V, None, scale, rhs, lam, lam_n, data=False), L)
    F = 0.0
    if implicit:
        gu, gv = panel_gram_exact(U, 0.0, R), panel_gram_exact(V, 0.0, R)
        with np.errstate(all='ignore'):
            F = chunk_sum(gu * gv, L)
    return _add(_add(ja, jt), F)


def loss_numpy(rowptrs, colinds, values, U, V, config, lam, lam_n):
    """
    (loss, constant, magnitude, additions) of one standard configuration in float64 NumPy:
      'explicit'  sum_e (a_e - u.v)^2 + reg                     constant sum a_e^2         (scale 0, rhs values)
      'implicit'  sum_e (1 + a_e)(1 - u.v)^2 + sum_(i,j not stored) (u.v)^2 + reg
                                                                 constant sum (1 + a_e)     (scale 1, rhs one_plus_values,
                                                                 values hold confidence - 1: the weight of a stored pair is
                                                                 1 + a_e, of which 1 is the all-pairs term's)
    reg = sum_i (lam + lam_n n_i) |u_i|^2 + sum_j (lam + lam_n m_j) |v_j|^2.  magnitude = the sum of the absolute values of
    every term of J's sums, additions = how many terms there are: a summation bound is additions 2^-52 magnitude.
    """
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    rp = np.asarray(rowptrs, dtype=np.int64)
    lens = np.diff(rp)
    rows = np.repeat(np.arange(len(lens)), lens)
    cols = np.asarray(colinds, dtype=np.int64)
    a = np.asarray(values, dtype=np.float64)
    s = np.einsum('ek,ek->e', U[rows], V[cols])
    mlens = np.bincount(cols, minlength=V.shape[0])
    ru, rv = (lam + lam_n * lens) * (U * U).sum(axis=1), (lam + lam_n * mlens) * (V * V).sum(axis=1)
    k = U.shape[1]
    if config == 'explicit':
        loss = ((a - s) ** 2).sum() + ru.sum() + rv.sum()
        const = (a * a).sum()
        mag = (np.abs(s * s) + 2 * np.abs(a * s)).sum() + np.abs(ru).sum() + np.abs(rv).sum()
        adds = (k + 2) * len(s) + (k + 1) * (len(ru) + len(rv))
    else:
        allp = ((U @ V.T) ** 2).sum()
        loss = ((1 + a) * (1 - s) ** 2).sum() + allp - (s * s).sum() + ru.sum() + rv.sum()
        const = (1 + a).sum()
        GU, GV = np.abs(U).T @ np.abs(U), np.abs(V).T @ np.abs(V)
        mag = (np.abs(a * s * s) + 2 * np.abs((1 + a) * s)).sum() + (GU * GV).sum() + np.abs(ru).sum() + np.abs(rv).sum()
        adds = (k + 3) * len(s) + (k + 1) * (len(ru) + len(rv)) + k * k + U.shape[0] + V.shape[0]
    return float(loss), float(const), float(mag), int(adds)


def fit_by_parts(K, a_h, at_h, U0, V0, sweeps, solver, steps, scale, rhs, implicit, lam, lam_n, tol, objective):
    "rule F's loop through the public host entries of the kernel module K: (U, V, objective list or None, bad list)"
    U, V = np.array(U0, dtype=np.float64), np.array(V0, dtype=np.float64)
    k = U.shape[1]

    def base_for(P):
        if solver == 'cg':
            return K.panel_gram(P, 0.0) if implicit else None
        if implicit:
            return K.panel_gram(P, lam)
        return None if lam == 0 else K.panel_gram(np.zeros((0, k)), lam)

    def half(h, P, X):
        if solver == 'cg':
            out, _, _ = K.als_rows_cg(h, P, scale=scale, rhs=rhs, base=base_for(P), lam=lam, lam_n=lam_n, steps=steps, x0=X, tol=tol)
            return out, 0
        out, info = K.als_rows(h, P, scale=scale, rhs=rhs, base=base_for(P), lam_n=lam_n)
        return out, int(np.count_nonzero(info))

    def obj():
        return K.als_objective(a_h, at_h, U, V, scale=scale, rhs=rhs, implicit=implicit, lam=lam, lam_n=lam_n)

    objs, bad = ([obj()] if objective else None), []
    for _ in range(sweeps):
        U, b0 = half(a_h, V, U)
        V, b1 = half(at_h, U, V)
        bad += [b0, b1]
        if objective:
            objs.append(obj())
    return U, V, objs, bad
