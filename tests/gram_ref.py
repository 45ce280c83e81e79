"""
References for csrk_gram_rows (include/csrk.h, rule 2), none of which touches the library:

  gram_exact      the contract restated step by step.  t = round(w * V[j][p]) is Python's float multiply (correctly
                  rounded); the fused multiply-add is float(Fraction(t) * Fraction(v) + Fraction(g)): the exact sum,
                  rounded once (float(Fraction) rounds to nearest even).  Finite operands only.  About 10^5
                  element-steps per second: callers keep a case under that.
  gram_two_rounding   the same chain with the multiply-add rounded twice (t * v, then + g): what a kernel without a
                  fused multiply-add would give.  Only to show that gram_exact can tell the two apart.
  gram_numpy      float64 NumPy for larger cases, with the magnitudes sum |w v_p v_q| that the error bound needs.
  gram_positions  where NaN, +Inf and -Inf land (Fractions cannot hold them): the chain in plain floats, classified.

All take the CSR arrays, V, scale, base and a row range and return [n, k, k] arrays.
"""
from fractions import Fraction

import numpy as np


def _weights(values, scale, e0, e1):
    if not scale or values is None:
        return [1.0] * (e1 - e0)
    return [float(v) for v in values[e0:e1]]          # float32 widens exactly


def _rows(rowptrs, rows):
    n = len(rowptrs) - 1
    return (0, n) if rows is None else rows


def gram_exact(rowptrs, colinds, values, V, scale=False, base=None, rows=None, fused=True):
    V = np.asarray(V)
    k = V.shape[1]
    rb, re_ = _rows(rowptrs, rows)
    out = np.zeros((re_ - rb, k, k))
    Vf = [[float(x) for x in r] for r in V]          # float32 widens exactly
    for i in range(rb, re_):
        e0, e1 = int(rowptrs[i]), int(rowptrs[i + 1])
        ws = _weights(values, scale, e0, e1)
        cols = [int(c) for c in colinds[e0:e1]]
        G = out[i - rb]
        for p in range(k):
            if scale and values is not None:
                ts = [w * Vf[j][p] for w, j in zip(ws, cols)]          # one rounded multiply
            else:
                ts = [Vf[j][p] for j in cols]
            for q in range(p + 1):
                g = 0.0 if base is None else float(base[p][q])
                if fused:
                    for t, j in zip(ts, cols):
                        g = float(Fraction(t) * Fraction(Vf[j][q]) + Fraction(g))
                else:
                    for t, j in zip(ts, cols):
                        g = t * Vf[j][q] + g
                G[p, q] = g
                G[q, p] = g
    return out


def gram_two_rounding(rowptrs, colinds, values, V, scale=False, base=None, rows=None):
    return gram_exact(rowptrs, colinds, values, V, scale, base, rows, fused=False)


def gram_numpy(rowptrs, colinds, values, V, scale=False, base=None, rows=None):
    "(G, M): float64 Gram blocks and M[i][p][q] = |base[p][q]| + sum |w v_p v_q| (lower triangle mirrored, as the contract's)"
    V = np.asarray(V, dtype=np.float64)
    k = V.shape[1]
    rb, re_ = _rows(rowptrs, rows)
    G = np.zeros((re_ - rb, k, k))
    M = np.zeros((re_ - rb, k, k))
    if base is None:
        bs = np.zeros((k, k))
    else:
        bs = np.tril(np.asarray(base, dtype=np.float64))
        bs = bs + np.tril(bs, -1).T
    for i in range(rb, re_):
        e0, e1 = int(rowptrs[i]), int(rowptrs[i + 1])
        Vr = V[np.asarray(colinds[e0:e1], dtype=np.int64)]
        w = np.ones(e1 - e0) if (not scale or values is None) else np.asarray(values[e0:e1], dtype=np.float64)
        WV = w[:, None] * Vr
        G[i - rb] = WV.T @ Vr + bs
        M[i - rb] = np.abs(WV).T @ np.abs(Vr) + np.abs(bs)
    return G, M


NAN, PINF, NINF, FINITE = 3, 1, 2, 0


def classify(G):
    "NAN / PINF / NINF / FINITE per element"
    G = np.asarray(G)
    c = np.zeros(G.shape, dtype=np.int8)
    c[np.isnan(G)] = NAN
    c[np.isposinf(G)] = PINF
    c[np.isneginf(G)] = NINF
    return c


def gram_positions(rowptrs, colinds, values, V, scale=False, base=None, rows=None):
    """
    classify() of the contract's chain run in plain floats (two roundings per step).  Where a NaN or an infinity appears
    does not depend on the fusing as long as the finite partial sums stay far from the overflow threshold, which is the
    callers' business: they use small finite values beside the special ones.
    """
    with np.errstate(all='ignore'):
        V = np.asarray(V)
        k = V.shape[1]
        rb, re_ = _rows(rowptrs, rows)
        out = np.zeros((re_ - rb, k, k))
        V64 = V.astype(np.float64)
        for i in range(rb, re_):
            e0, e1 = int(rowptrs[i]), int(rowptrs[i + 1])
            G = np.zeros((k, k)) if base is None else np.array(base, dtype=np.float64)
            for e in range(e0, e1):
                v = V64[int(colinds[e])]
                w = 1.0 if (not scale or values is None) else np.float64(values[e])
                t = v if (not scale or values is None) else w * v
                G = t[:, None] * v[None, :] + G
            lo = np.tril_indices(k)
            out[i - rb][lo] = G[lo]
            out[i - rb].T[lo] = G[lo]
    return classify(out)
