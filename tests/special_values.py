"""
Comparison rules for outputs that may hold NaN, +-Inf and signed zeros (tests/test_oracle_golden.py's special-value pin
and tests/test_gpu_special_values.py):

  NaN       by position only: its sign and payload are not specified (x86 gives the negative default NaN, the GPU the
            positive one);
  +-Inf     exactly;
  zeros     by their sign bit;
  finite    bit for bit where a route promises it (`same_bits`), else within `rel` of sum |products| (`close`).
"""
import numpy as np


def kind(a):
    "0 NaN, 1 +Inf, 2 -Inf, 3 +0.0, 4 -0.0, 5 other finite"
    a = np.asarray(a, dtype=np.float64)
    k = np.full(a.shape, 5, dtype=np.int8)
    k[a == 0] = 3
    k[(a == 0) & np.signbit(a)] = 4
    k[np.isposinf(a)] = 1
    k[np.isneginf(a)] = 2
    k[np.isnan(a)] = 0
    return k


def _where(mask, what):
    idx = np.flatnonzero(mask)
    return f'{what}: {len(idx)} differ, first at {idx[:8].tolist()}'


def same_bits(got, want, what=''):
    "NaN at the same positions, every other value (zeros and infinities included) bit for bit"
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~gn & ~wn & (got.view(np.int64) != want.view(np.int64)))
    assert not bad.any(), _where(bad, what) + f' got {got[bad][:4]} want {want[bad][:4]}'


def close(got, want, bound, what='', rel=1e-12):
    """
    NaN by position, +-Inf exactly, zeros by sign bit (a zero the reference returns must come back with its sign), other
    finite values within rel * bound (bound = the same product over |values| and |x|).
    """
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    kg, kw = kind(got), kind(want)
    near = (kw == 5) & (kg >= 3)                     # a finite reference value: a finite (or zero) result near it
    bad = (kg != kw) & ~near
    with np.errstate(all='ignore'):
        err = np.abs(got - want)
    b = np.broadcast_to(np.asarray(bound, dtype=np.float64), want.shape)
    bad |= near & ~(err <= rel * b + 1e-300)
    assert not bad.any(), _where(bad, what) + f' got {got[bad][:4]} want {want[bad][:4]}'


def same_class(got, want, what=''):
    "NaN, +Inf, -Inf and finite agree (the class of an output whose products are far from overflow)"
    kg, kw = kind(got), kind(want)
    kg[kg >= 3] = 3
    kw[kw >= 3] = 3
    bad = kg != kw
    assert not bad.any(), _where(bad, what) + f' got {np.asarray(got)[bad][:4]} want {np.asarray(want)[bad][:4]}'


def raw_bits_equal(got, want):
    "every value bit for bit, NaN payloads included (data movement)"
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(got.view(np.uint8), want.view(np.uint8))
