"""
The expected result of csrk_combine (include/csrk.h), restated in NumPy for the tests, row by row as the contract reads.
A matrix is a tuple (rowptrs, colinds, values) with values float64 / float32 / None (structure only).  NumPy multiplies
and adds float64 arrays one rounding at a time -- no fused multiply-add -- which is the contract's arithmetic.
tests/test_combine_host.py checks this file against scipy.sparse and against hand-written rows.
"""
import numpy as np

OPS = ('add', 'multiply', 'keep', 'drop')
INT32_MAX = 2 ** 31 - 1


def widen(v, n):
    "the values as the arithmetic sees them: float32 widened exactly, 1.0 everywhere for a structure-only operand"
    if v is None:
        return np.ones(n, np.float64)
    with np.errstate(invalid='ignore'):
        return v.astype(np.float64)


def is_canonical(rp, ci):
    "every row strictly ascending in column"
    return all(np.all(np.diff(ci[int(rp[i]):int(rp[i + 1])].astype(np.int64)) > 0) for i in range(len(rp) - 1))


def combine_ref(A, B, op, alpha=1.0, beta=1.0):
    arp, aci, avs = A
    brp, bci, bvs = B
    assert op in OPS and len(arp) == len(brp)
    if not is_canonical(brp, bci):
        raise ValueError('B is not canonical')
    if op in ('add', 'multiply') and not is_canonical(arp, aci):
        raise ValueError('A is not canonical')
    mask = op in ('keep', 'drop')
    al, be = np.float64(alpha), np.float64(beta)
    orp, oci, ovs = [0], [aci[:0]], []
    with np.errstate(all='ignore'):
        for i in range(len(arp) - 1):
            sa, ea, sb, eb = int(arp[i]), int(arp[i + 1]), int(brp[i]), int(brp[i + 1])
            ca, cb = aci[sa:ea], bci[sb:eb]
            if mask:
                hit = np.isin(ca, cb)
                sel = hit if op == 'keep' else ~hit
                oci.append(ca[sel])                               # A's storage order
                if avs is not None:
                    ovs.append(avs[sa:ea][sel])                   # A's dtype, A's bits
                orp.append(orp[-1] + int(sel.sum()))
                continue
            wa = widen(None if avs is None else avs[sa:ea], ea - sa)
            wb = widen(None if bvs is None else bvs[sb:eb], eb - sb)
            if op == 'multiply':
                cols = np.intersect1d(ca, cb)                     # ascending
                v = wa[np.isin(ca, cols)] * wb[np.isin(cb, cols)]
            else:
                cols = np.union1d(ca, cb)                         # ascending
                ina, inb = np.isin(cols, ca), np.isin(cols, cb)
                pa, pb = np.zeros(len(cols)), np.zeros(len(cols))
                pa[ina] = al * wa                                 # round(alpha a)
                pb[inb] = be * wb                                 # round(beta b)
                v = np.where(ina & inb, pa + pb, np.where(ina, pa, pb))
            oci.append(cols.astype(np.int32))
            ovs.append(v)
            orp.append(orp[-1] + len(cols))
    total = orp[-1]
    vals = None
    if not mask:
        vals = np.concatenate([np.zeros(0)] + ovs)
    elif avs is not None:
        vals = np.concatenate([avs[:0]] + ovs)
    return (np.array(orp, dtype=np.int64 if total > INT32_MAX else np.int32), np.concatenate(oci).astype(np.int32), vals)


def bits(a):
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def same(got, exp, op):
    """
    Pointer dtype and values, column indices, value dtype: exactly.  Values bit for bit; under 'add' and 'multiply' a NaN
    matches any NaN (what payload arithmetic passes on is not part of the contract), under 'keep' and 'drop' all bits count.
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
    eq = bits(gvs) == bits(evs)
    if op in ('add', 'multiply'):
        eq |= np.isnan(gvs) & np.isnan(evs)
    return bool(eq.all())


def first_difference(got, exp, op):
    "a short description of where two results part, for an assertion message"
    grp, gci, gvs = got
    erp, eci, evs = exp
    if grp.dtype != erp.dtype:
        return f'pointer dtype {grp.dtype} != {erp.dtype}'
    if not np.array_equal(grp, erp):
        r = int(np.flatnonzero(np.asarray(grp) != np.asarray(erp))[0]) if len(grp) == len(erp) else -1
        return f'row pointers differ first at {r}: got {grp[max(r - 1, 0):r + 2]} expected {erp[max(r - 1, 0):r + 2]}'
    if not np.array_equal(gci, eci):
        e = int(np.flatnonzero(gci != eci)[0])
        return f'column {e} (row {int(np.searchsorted(erp, e, side="right")) - 1}): got {gci[e]} expected {eci[e]}'
    if (gvs is None) != (evs is None) or (gvs is not None and gvs.dtype != evs.dtype):
        return f'value dtype {None if gvs is None else gvs.dtype} != {None if evs is None else evs.dtype}'
    if gvs is not None:
        eq = bits(gvs) == bits(evs)
        if op in ('add', 'multiply'):
            eq |= np.isnan(gvs) & np.isnan(evs)
        if not eq.all():
            e = int(np.flatnonzero(~eq)[0])
            return f'value {e} (row {int(np.searchsorted(erp, e, side="right")) - 1}, column {eci[e]}): got {gvs[e]!r} expected {evs[e]!r}'
    return 'no difference'
