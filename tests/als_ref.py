"""
References for csrk_solve_blocks and csrk_als_rows (include/csrk.h, rules S and A), none of which touches the library:

  ldl_exact        rule S restated step by step.  fma(-a, b, c) is float(Fraction(c) - Fraction(a) * Fraction(b)): the exact
                   value rounded once (float(Fraction) rounds to nearest even); the multiply and the division are IEEE
                   float64 operations (correctly rounded).  Operands that Fractions cannot hold (NaN, Inf) go through plain
                   float arithmetic: where a NaN or an infinity lands does not depend on the fusing.  Returns (x, info).
                   About 0.6 s at k = 64, 1.5 s at k = 88, 5 s at k = 128: callers size their cases by that.
  ldl_two_rounding the same with multiply-then-subtract: what a kernel without a fused multiply-add would give.  Only to
                   show that ldl_exact can tell the two apart.
  ridge_exact      rule A2 on a batch of blocks;  rhs_exact  rule A3;  als_exact  gram_ref.gram_exact, then those, then
                   ldl_exact: (x, info, G, b).
  als_numpy        float64 NumPy for long rows: G, b and the magnitudes M = |base| + sum |w v_p v_q| (+ |lam_n| n on the
                   diagonal), Mb = sum |c v_p| that the error bounds need.
  residual_bound   the textbook backward-error bound of an unpivoted LDL^T solve, with the accumulation chains' own bounds
                   on top (see there).
"""
from fractions import Fraction

import numpy as np

import gram_ref

RHS = ('ones', 'values', 'one_plus_values')


def _finite(*xs):
    return all(x == x and x not in (float('inf'), float('-inf')) for x in xs)


def fnma(a, b, c, fused=True):
    "round(c - a b): one rounding (fused) or two"
    a, b, c = float(a), float(b), float(c)
    if not fused or not _finite(a, b, c):
        with np.errstate(all='ignore'):
            return float(np.float64(c) - np.float64(a) * np.float64(b))
    v = Fraction(c) - Fraction(a) * Fraction(b)
    if v == 0:
        # IEEE: an exact zero sum is +0.0 unless both addends, c and -(a b), are -0.0
        both = c == 0.0 and (a == 0.0 or b == 0.0) and np.signbit(c) and np.signbit(a) == np.signbit(b)
        return -0.0 if both else 0.0
    return float(v)


def _mul(a, b):
    with np.errstate(all='ignore'):
        return float(np.float64(a) * np.float64(b))


def _recip(d):
    with np.errstate(all='ignore'):
        return float(np.float64(1.0) / np.float64(d))


def ldl_exact(G, b, fused=True, factors=False):
    "(x[k], info) for one system: rule S.  Only G's lower triangle is read.  factors=True: (x, info, L, d) as lists."
    k = len(b)
    C = [[0.0] * k for _ in range(k)]
    L = [[0.0] * k for _ in range(k)]
    r = [0.0] * k
    info = 0
    for j in range(k):
        for i in range(j, k):
            a = float(G[i][j])
            Li, Cj = L[i], C[j]
            for t in range(j):
                a = fnma(Li[t], Cj[t], a, fused)
            C[i][j] = a
        d = C[j][j]
        if info == 0 and not d > 0.0:
            info = j + 1
        r[j] = _recip(d)
        for i in range(j + 1, k):
            L[i][j] = _mul(C[i][j], r[j])
    z = [0.0] * k
    for i in range(k):
        a = float(b[i])
        for t in range(i):
            a = fnma(L[i][t], z[t], a, fused)
        z[i] = a
    x = [_mul(z[i], r[i]) for i in range(k)]
    for i in range(k - 1, -1, -1):
        a = x[i]
        for t in range(k - 1, i, -1):
            a = fnma(L[t][i], x[t], a, fused)
        x[i] = a
    if factors:
        return np.array(x, dtype=np.float64), info, L, [C[j][j] for j in range(k)]
    return np.array(x, dtype=np.float64), info


def ldl_two_rounding(G, b, factors=False):
    return ldl_exact(G, b, False, factors)


def ldl_exact_batch(G, b):
    "(x[n, k], info[n]) for G [n, k, k], b [n, k]"
    G, b = np.asarray(G), np.asarray(b)
    x = np.zeros(b.shape)
    info = np.zeros(len(b), np.int32)
    for s in range(len(b)):
        x[s], info[s] = ldl_exact(G[s], b[s])
    return x, info


def _rows(rowptrs, rows):
    n = len(rowptrs) - 1
    return (0, n) if rows is None else rows


def ridge_exact(G, rowptrs, lam_n, rows=None):
    "rule A2 on a copy of G [n, k, k]: G[p][p] = fma(lam_n, n_i, G[p][p])"
    rb, re_ = _rows(rowptrs, rows)
    G = np.array(G, dtype=np.float64)
    for i in range(rb, re_):
        n_i = float(int(rowptrs[i + 1]) - int(rowptrs[i]))
        for p in range(G.shape[1]):
            G[i - rb, p, p] = fnma(-float(lam_n), n_i, G[i - rb, p, p])
    return G


def _c(values, rhs, e):
    assert rhs in RHS
    if rhs == 'ones':
        return 1.0
    v = 1.0 if values is None else float(values[e])            # float32 widens exactly
    with np.errstate(all='ignore'):
        return v if rhs == 'values' else float(np.float64(1.0) + np.float64(v))


def rhs_exact(rowptrs, colinds, values, V, rhs='values', rows=None):
    "rule A3: b [n, k]"
    V = np.asarray(V)
    k = V.shape[1]
    rb, re_ = _rows(rowptrs, rows)
    out = np.zeros((re_ - rb, k))
    Vf = [[float(x) for x in r] for r in V]
    for i in range(rb, re_):
        for p in range(k):
            a = 0.0
            for e in range(int(rowptrs[i]), int(rowptrs[i + 1])):
                a = fnma(-_c(values, rhs, e), Vf[int(colinds[e])][p], a)
            out[i - rb, p] = a
    return out


def als_exact(rowptrs, colinds, values, V, scale=False, rhs='values', base=None, lam_n=0.0, rows=None):
    "(x [n, k], info [n], G [n, k, k], b [n, k]): rules A1 - A4 restated"
    G = gram_ref.gram_exact(rowptrs, colinds, values, V, scale, base, rows)
    G = ridge_exact(G, rowptrs, lam_n, rows)
    b = rhs_exact(rowptrs, colinds, values, V, rhs, rows)
    x, info = ldl_exact_batch(G, b)
    return x, info, G, b


def als_numpy(rowptrs, colinds, values, V, scale=False, rhs='values', base=None, lam_n=0.0, rows=None):
    "(G, M, b, Mb) in float64 NumPy: the systems and the magnitudes of their sums"
    G, M = gram_ref.gram_numpy(rowptrs, colinds, values, V, scale, base, rows)
    V = np.asarray(V, dtype=np.float64)
    k = V.shape[1]
    rb, re_ = _rows(rowptrs, rows)
    b, Mb = np.zeros((re_ - rb, k)), np.zeros((re_ - rb, k))
    d = np.arange(k)
    for i in range(rb, re_):
        e0, e1 = int(rowptrs[i]), int(rowptrs[i + 1])
        Vr = V[np.asarray(colinds[e0:e1], dtype=np.int64)]
        if rhs == 'ones':
            c = np.ones(e1 - e0)
        else:
            c = np.ones(e1 - e0) if values is None else np.asarray(values[e0:e1], dtype=np.float64)
            if rhs == 'one_plus_values':
                c = 1.0 + c
        b[i - rb] = c @ Vr
        Mb[i - rb] = np.abs(c) @ np.abs(Vr)
        G[i - rb][d, d] += lam_n * (e1 - e0)
        M[i - rb][d, d] += abs(lam_n) * (e1 - e0)
    return G, M, b, Mb


def residual_bound(G, M, b, Mb, lens, x):
    """
    (residual [n], bound [n]) of a computed x against the NumPy systems (G, b) of als_numpy.

    The computed x solves the library's own system (G', b') with the backward error of an unpivoted LDL^T solve,
        |G' x - b'|_inf <= k (3 k + 2) 2^-53 (|G'|_inf |x|_inf + |b'|_inf)
    (three triangular passes of at most k fused steps each, plus the reciprocal and the scaling).  (G', b') are the
    accumulation chains of rules A1 - A3, each within (len + 2) 2^-52 of the magnitude of its sum from the NumPy value
    (tests/test_gpu_gram.py's bound; one more rounding for the ridge and for 1 + value): E = (len + 3) 2^-52 M,
    e = (len + 3) 2^-52 Mb.  So
        |G x - b|_inf <= k (3 k + 2) 2^-53 ((|G|_inf + |E|_inf) |x|_inf + |b|_inf + |e|_inf) + |E|_inf |x|_inf + |e|_inf.
    """
    G, M, b, Mb, x = (np.asarray(a, dtype=np.float64) for a in (G, M, b, Mb, x))
    k = G.shape[1]
    lens = np.asarray(lens, dtype=np.float64)
    nG = np.abs(G).sum(axis=2).max(axis=1)
    nE = (lens + 3) * 2.0 ** -52 * np.abs(M).sum(axis=2).max(axis=1)
    ne = (lens + 3) * 2.0 ** -52 * np.abs(Mb).max(axis=1)
    nb = np.abs(b).max(axis=1)
    nx = np.abs(x).max(axis=1)
    res = np.abs(np.einsum('npq,nq->np', G, x) - b).max(axis=1)
    bound = k * (3 * k + 2) * 2.0 ** -53 * ((nG + nE) * nx + nb + ne) + nE * nx + ne
    return res, bound


def solve_numpy(G, b):
    "(x, |G|_inf, |b|_inf, |x|_inf) per system, by np.linalg.solve on the mirrored lower triangle"
    G, b = np.asarray(G, dtype=np.float64), np.asarray(b, dtype=np.float64)
    S = np.tril(G) + np.tril(G, -1).transpose(0, 2, 1)
    x = np.linalg.solve(S, b[..., None])[..., 0]
    return x, np.abs(S).sum(axis=2).max(axis=1), np.abs(b).max(axis=1), np.abs(x).max(axis=1)
