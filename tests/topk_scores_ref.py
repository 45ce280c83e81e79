"""
Restatements of csrk_topk_scores (include/csrk.h) for the tests: nothing here is shared with the library.

    scores_exact         rule 2 with exact rational arithmetic: every step of the chain s = fma(u, v, s) is the exact u v + s
                         rounded once to float64 (Fraction -> float is correctly rounded).  Finite operands only; about 10^5
                         steps (rows x items x k) a second.
    scores_plain         S = S + U[:, t] * V[:, t] in float64, vectorised: multiply, round, add, round.  Equal to the fused
                         chain bit for bit WHENEVER EVERY PRODUCT IS EXACT: float32 panels widened (24 x 24 bits fit 53), or
                         float64 panels on a coarse grid such as integers in [-512, 512) / 64.
    scores_two_rounding  the same loop element by element: what a kernel that multiplies and then adds would give.
    scores_positions     where the scores are NaN / +Inf / -Inf for panels with special values (by the plain loop: valid while
                         no product of two finite elements overflows).
    key                  the total order of csrk_topk_rows' rule 2 as an unsigned integer.
    select               rules 3-5 by a plain sort on (key descending, item ascending).
"""
from fractions import Fraction

import numpy as np


def _fma_exact(u, v, s):
    "round(u v + s) for finite floats, with the IEEE sign of an exact zero"
    r = Fraction(u) * Fraction(v) + Fraction(s)
    if r == 0:
        prod_neg = (np.signbit(u) != np.signbit(v))
        if u != 0.0 and v != 0.0:
            return 0.0                                  # an exact cancellation: +0.0 in round-to-nearest
        return -0.0 if (prod_neg and np.signbit(s)) else 0.0
    return r.numerator / r.denominator                  # int / int: correctly rounded


def scores_exact(U, V):
    U, V = np.asarray(U), np.asarray(V)
    assert np.isfinite(U).all() and np.isfinite(V).all()
    U64, V64 = U.astype(np.float64), V.astype(np.float64)      # (float32 widens exactly)
    S = np.zeros((U.shape[0], V.shape[0]))
    for i in range(U.shape[0]):
        ui = [float(x) for x in U64[i]]
        for j in range(V.shape[0]):
            s = 0.0
            vj = V64[j]
            for t in range(len(ui)):
                s = _fma_exact(ui[t], float(vj[t]), s)
            S[i, j] = s
    return S


def scores_plain(U, V):
    U64, V64 = np.asarray(U).astype(np.float64), np.asarray(V).astype(np.float64)
    S = np.zeros((U64.shape[0], V64.shape[0]))
    with np.errstate(all='ignore'):
        for t in range(U64.shape[1]):
            S = S + U64[:, t][:, None] * V64[:, t][None, :]
    return S


def scores_two_rounding(U, V):
    U64, V64 = np.asarray(U).astype(np.float64), np.asarray(V).astype(np.float64)
    S = np.zeros((U64.shape[0], V64.shape[0]))
    for i in range(U64.shape[0]):
        for j in range(V64.shape[0]):
            s = np.float64(0.0)
            for t in range(U64.shape[1]):
                p = np.float64(U64[i, t] * V64[j, t])
                s = np.float64(s + p)
            S[i, j] = s
    return S


def scores_positions(U, V):
    "(is NaN, is +Inf, is -Inf) of every score"
    S = scores_plain(U, V)
    return np.isnan(S), np.isposinf(S), np.isneginf(S)


def key(x):
    "uint64 keys that sort like the order of rule 4: NaN -> all ones, -0.0 -> +0.0, then the sign flip"
    x = np.ascontiguousarray(np.asarray(x, np.float64))
    b = x.view(np.uint64).copy()
    b[x == 0.0] = 0
    neg = (b >> np.uint64(63)) == 1
    out = np.where(neg, ~b, b | np.uint64(1 << 63))
    out[np.isnan(x)] = np.uint64(0xffffffffffffffff)
    return out


def select(S, seen_rowptrs, seen_colinds, n_top, min_score=None):
    """
    (items int32 [m, n_top], scores float64 [m, n_top], counts int32 [m]) from the dense scores S [m, n_items]; row r of S is
    row r of the seen pattern (seen_rowptrs None: nothing seen).
    """
    S = np.asarray(S, np.float64)
    m, n_items = S.shape
    ms = -np.inf if min_score is None else float(min_score)
    items = np.full((m, n_top), -1, np.int32)
    scores = np.full((m, n_top), -np.inf)
    counts = np.zeros(m, np.int32)
    for r in range(m):
        with np.errstate(invalid='ignore'):
            cand = ~(S[r] < ms)
        if seen_rowptrs is not None:
            cand[np.asarray(seen_colinds[int(seen_rowptrs[r]):int(seen_rowptrs[r + 1])], np.int64)] = False
        idx = np.flatnonzero(cand)
        k = key(S[r, idx])
        order = np.lexsort((idx, np.uint64(0xffffffffffffffff) - k))[:n_top]
        c = len(order)
        counts[r] = c
        items[r, :c] = idx[order]
        scores[r, :c] = S[r, idx[order]]
    return items, scores, counts
