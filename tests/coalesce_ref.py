"""
The expected result of csrk_coalesce (include/csrk.h), restated in plain NumPy / Python for the tests, group by group as the
contract reads.  A matrix is a tuple (rowptrs, colinds, values) with values float64 / float32 / None (structure only).
A NumPy scalar add of two float32 (float64) values is one float32 (float64) rounding -- the contract's arithmetic.
tests/test_coalesce_host.py checks this file against scipy.sparse and against hand-written rows.
"""
import numpy as np

DUPS = ('sum', 'first', 'last', 'max', 'min')
INT32_MAX = 2 ** 31 - 1


def above(a, b):
    "a ranks strictly above b in csrk_topk_rows' order: larger first, NaN above +Inf, all NaNs tied, -0.0 and +0.0 tied"
    if a != a:
        return not (b != b)
    return bool(a > b)


def fold(vs, dup):
    "what the members vs (a 1-D array in storage order, at least one) become: a scalar of their dtype, or their own bits"
    if dup == 'first':
        return vs[0]
    if dup == 'last':
        return vs[-1]
    if dup == 'sum':
        acc = vs[0]                         # not 0.0 + vs[0]: a group of one keeps its bits, -0.0 + -0.0 stays -0.0
        with np.errstate(all='ignore'):
            for v in vs[1:]:
                acc = acc + v               # two scalars of one dtype: one rounding in that dtype
        return acc
    w = vs[0]
    for v in vs[1:]:
        if dup == 'max':
            if above(v, w):                 # the first of the order: a tie stays with the earlier member
                w = v
        elif not above(v, w):               # min, the last of the order: a tie goes to the later member
            w = v
    return w


def is_canonical(rp, ci):
    "(True, None), or (False, the first row that is not strictly ascending in column)"
    for i in range(len(rp) - 1):
        if not np.all(np.diff(ci[int(rp[i]):int(rp[i + 1])].astype(np.int64)) > 0):
            return False, i
    return True, None


def route(rp, ci):
    "the route csrk_coalesce takes: 0 canonical, 1 rows non-descending, 2 anything else"
    if is_canonical(rp, ci)[0]:
        return 0
    if all(np.all(np.diff(ci[int(rp[i]):int(rp[i + 1])].astype(np.int64)) >= 0) for i in range(len(rp) - 1)):
        return 1
    return 2


def coalesce_ref(A, dup):
    rp, ci, vs = A
    assert dup in DUPS
    orp, oci, ovs = [0], [], []
    for i in range(len(rp) - 1):
        s, e = int(rp[i]), int(rp[i + 1])
        cols = ci[s:e]
        order = np.argsort(cols, kind='stable')        # ascending column, storage order among equal columns
        sc = cols[order]
        starts = np.flatnonzero(np.concatenate(([True], sc[1:] != sc[:-1]))) if e > s else np.zeros(0, np.int64)
        ends = np.concatenate((starts[1:], [e - s])) if e > s else starts
        for a, b in zip(starts, ends):
            oci.append(sc[a])
            if vs is not None:
                ovs.append(fold(vs[s:e][order[a:b]], dup))
        orp.append(orp[-1] + len(starts))
    total = orp[-1]
    vals = None if vs is None else np.array(ovs, dtype=vs.dtype) if ovs else vs[:0].copy()
    return (np.array(orp, dtype=np.int64 if total > INT32_MAX else np.int32), np.array(oci, dtype=np.int32), vals)


def bits(a):
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _value_eq(gvs, evs, dup):
    eq = bits(gvs) == bits(evs)
    if dup == 'sum':
        eq = eq | (np.isnan(gvs) & np.isnan(evs))
    return eq


def same(got, exp, dup):
    """
    Pointer dtype and values, column indices, value dtype: exactly.  Values bit for bit; under 'sum' a NaN matches any NaN
    (what payload an add passes on is not part of the contract), under every other rule all bits count.
    """
    grp, gci, gvs = got
    erp, eci, evs = exp
    if grp.dtype != erp.dtype or not np.array_equal(grp, erp):
        return False
    if gci.dtype != eci.dtype or not np.array_equal(gci, eci):
        return False
    if (gvs is None) != (evs is None):
        return False
    if gvs is None:
        return True
    if gvs.dtype != evs.dtype or gvs.shape != evs.shape:
        return False
    return bool(_value_eq(gvs, evs, dup).all())


def first_difference(got, exp, dup):
    "a short description of where two results part, for an assertion message"
    grp, gci, gvs = got
    erp, eci, evs = exp
    if grp.dtype != erp.dtype:
        return f'pointer dtype {grp.dtype} != {erp.dtype}'
    if not np.array_equal(grp, erp):
        r = int(np.flatnonzero(np.asarray(grp) != np.asarray(erp))[0]) if len(grp) == len(erp) else -1
        return f'row pointers differ first at {r}: got {grp[max(r - 1, 0):r + 2]} expected {erp[max(r - 1, 0):r + 2]}'
    if gci.dtype != eci.dtype:
        return f'column dtype {gci.dtype} != {eci.dtype}'
    if not np.array_equal(gci, eci):
        e = int(np.flatnonzero(gci != eci)[0])
        return f'column {e} (row {int(np.searchsorted(erp, e, side="right")) - 1}): got {gci[e]} expected {eci[e]}'
    if (gvs is None) != (evs is None) or (gvs is not None and gvs.dtype != evs.dtype):
        return f'value dtype {None if gvs is None else gvs.dtype} != {None if evs is None else evs.dtype}'
    if gvs is not None:
        eq = _value_eq(gvs, evs, dup)
        if not eq.all():
            e = int(np.flatnonzero(~eq)[0])
            return (f'value {e} (row {int(np.searchsorted(erp, e, side="right")) - 1}, column {eci[e]}): got {gvs[e]!r} '
                    f'({int(bits(gvs)[e]):#x}) expected {evs[e]!r} ({int(bits(evs)[e]):#x})')
    return 'no difference'
