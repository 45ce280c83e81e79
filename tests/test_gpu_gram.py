"""
csrk_gram_rows on the card (include/csrk.h): bit for bit against the exact restatement of its rule 2 (tests/gram_ref.py) at
every k class and staging boundary that csrk_gram_limits names; within the sequential-sum bound of NumPy float64 on a long
row and on a matrix of mixed rows; the same bits from every variant of one request (pointer width, host and device
entry, row ranges, a row permutation, panel stride and alignment, a repeated call); NaN / Inf by position; every refusal
with the output untouched; the cases without entries.

Matrices have at most 300 rows, 200 columns and 5000 entries; the exact reference runs about 10^5 element-steps per
second, so every exact case is sized in element-steps (lower-triangle elements x entries).
"""
import ctypes as C

import numpy as np
import pytest

import gram_ref as R

pytestmark = pytest.mark.gpu

NCOLS = 200


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _csr(nr, nc, rp, ci, vs, ptr64=False):
    from csr_amd import CSR
    return CSR(nr, nc, int(rp[-1]), np.asarray(rp).astype(np.int64 if ptr64 else np.int32), np.asarray(ci, np.int32).copy(),
               None if vs is None else vs.copy(), _cast=False)


def _pattern(lens, seed, vdt=np.float64):
    "rows of the given lengths over NCOLS columns: unsorted, columns repeated within rows"
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    rp = np.zeros(len(lens) + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    nnz = int(rp[-1])
    ci = rng.integers(0, NCOLS, nnz).astype(np.int32)
    for r in range(len(lens)):                                  # a repeated column in every row of three or more entries
        if lens[r] >= 3:
            ci[rp[r] + 2] = ci[rp[r]]
    vs = None if vdt is None else rng.standard_normal(nnz).astype(vdt)
    return len(lens), NCOLS, rp, ci, vs


def _panel(k, pdt, seed):
    "asymmetric in every sense: no two columns alike, so a p <-> q swap shows"
    rng = np.random.default_rng(1000 + seed)
    return (rng.standard_normal((NCOLS, k)) * (1.0 + np.arange(k) / 7.0)).astype(pdt)


def _base(k, seed):
    "asymmetric: the upper triangle holds other numbers than the lower, so reading it shows"
    rng = np.random.default_rng(2000 + seed)
    b = rng.standard_normal((k, k))
    b[np.triu_indices(k, 1)] += 1000.0
    return b


@pytest.fixture(scope='module')
def limits():
    from csr_amd.kernels import hip as K
    return K.gram_limits()


# scale, value dtype (None: structure-only), panel dtype, with base
COMBOS = [(False, np.float64, np.float64, False), (True, np.float64, np.float64, True), (True, np.float32, np.float32, False),
          (True, None, np.float64, True), (False, np.float32, np.float32, True), (True, np.float64, np.float32, False)]


def _exact_case(K, lens, k, combo, seed):
    scale, vdt, pdt, with_base = combo
    nr, nc, rp, ci, vs = _pattern(lens, seed, vdt)
    V = _panel(k, pdt, seed)
    base = _base(k, seed) if with_base else None
    h = K.to_handle(_csr(nr, nc, rp, ci, vs))
    try:
        got = K.gram_rows(h, V, scale, None, base)
    finally:
        K.release_handle(h)
    want = R.gram_exact(rp, ci, vs, V, scale, base)
    assert got.shape == (nr, k, k) and got.dtype == np.float64
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, (k, combo, len(bad), bad[:4].tolist())
    assert np.array_equal(_bits(got), _bits(got.transpose(0, 2, 1)))


@pytest.mark.parametrize('k', [1, 2, 3, 15, 16, 17])
def test_exact_small_k_at_every_staging_boundary(k, limits):
    "rows of 0, 1 and S - 1, S, S + 1, 2S - 1, 2S, 2S + 1 entries (S staged per step), runs of empty rows at both ends"
    from csr_amd.kernels import hip as K
    S = int(limits[1])
    lens = [0, 0, 1, S - 1, S, S + 1, 0, 2 * S - 1, 2 * S, 2 * S + 1, 0, 0]
    assert sum(lens) * k * (k + 1) // 2 <= 100000 and sum(lens) <= 5000
    first = [1, 2, 3, 15, 16, 17].index(k)
    for c in range(4):                                          # four of the six combinations per k, all six over the ks
        _exact_case(K, lens, k, COMBOS[(first + c) % 6], seed=10 * k + c)


def test_exact_large_k_at_every_class_boundary(limits):
    "k = 31, 33, 64, 65, 128, the largest k and every k class threshold - 1, 0, + 1; rows of 0, 2, 0, 1 entries"
    from csr_amd.kernels import hip as K
    ks = {31, 33, 64, 65, 128, int(limits[0])}
    for t in limits[2:]:
        ks |= {int(t) - 1, int(t), int(t) + 1}
    ks = sorted(x for x in ks if 17 < x <= limits[0])
    assert {31, 33, 64, 65, 128, limits[0]} <= set(ks)
    lens = [0, 2, 0, 1]
    for n, k in enumerate(ks):
        assert sum(lens) * k * (k + 1) // 2 <= 100000
        _exact_case(K, lens, k, COMBOS[(n + 1) % 6], seed=k)


def test_k_above_the_limit_is_unsupported(limits):
    import torch
    from csr_amd.kernels import hip as K
    from csr_amd._lib import lib, ERR_UNSUPPORTED, VAL_F64
    k = int(limits[0]) + 1
    nr, nc, rp, ci, vs = _pattern([2, 1], 3)
    h = K.to_handle(_csr(nr, nc, rp, ci, vs))
    try:
        V = torch.ones(nc, k, dtype=torch.float64, device='cuda')
        out = torch.full((nr * k * k,), -7.0, dtype=torch.float64, device='cuda')
        assert lib.csrk_gram_rows_device(h.H, 0, nr, V.data_ptr(), k, k, VAL_F64, 0, None, out.data_ptr(), None) == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())
        hout = np.full(nr * k * k, -7.0)
        Vh = np.ones((nc, k))
        assert lib.csrk_gram_rows(h.H, 0, nr, Vh.ctypes.data, k, k, VAL_F64, 0, None, hout.ctypes.data) == ERR_UNSUPPORTED
        assert np.all(hout == -7.0)
    finally:
        K.release_handle(h)


# ---- tolerance against NumPy float64 --------------------------------------------------------------------------

def _check_numpy(K, lens, k, seed, scale=True, pdt=np.float64):
    nr, nc, rp, ci, vs = _pattern(lens, seed)
    V = _panel(k, pdt, seed)
    base = _base(k, seed)
    h = K.to_handle(_csr(nr, nc, rp, ci, vs))
    try:
        got = K.gram_rows(h, V, scale, None, base)
    finally:
        K.release_handle(h)
    ref, mag = R.gram_numpy(rp, ci, vs, V, scale, base)
    # both sides are sums of len + 1 terms, each term rounded once more by the weight: (len + 2) 2^-52 sum |w v_p v_q|
    bound = (np.diff(rp)[:, None, None] + 2) * 2.0 ** -52 * mag
    err = np.abs(got - ref)
    assert np.all(err <= bound), (float((err / np.maximum(bound, 1e-300)).max()), np.argwhere(err > bound)[:4].tolist())
    assert np.array_equal(_bits(got), _bits(got.transpose(0, 2, 1)))


def test_one_row_of_5000_entries_at_k_64():
    from csr_amd.kernels import hip as K
    _check_numpy(K, [5000], 64, seed=64)


def test_300_mixed_rows_at_k_33(limits):
    from csr_amd.kernels import hip as K
    _check_numpy(K, _mixed_lens(limits), 33, seed=33)
    _check_numpy(K, _mixed_lens(limits), 33, seed=34, scale=False, pdt=np.float32)


def _mixed_lens(limits):
    "300 rows, at most 5000 entries: empty runs at both ends, every staging boundary, a long row, short rows"
    S = int(limits[1])
    rng = np.random.default_rng(7)
    lens = np.concatenate([np.zeros(5, np.int64), [1, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 700], rng.integers(0, 28, 280),
                           np.zeros(7, np.int64)]).astype(np.int64)
    assert len(lens) == 300 and lens.sum() <= 5000
    return lens


# ---- equal bits among the variants of one request -----------------------------------------------------------

def _device_call(h, dV, ldv, k, code, scale, rb, re_, dbase, stream=None):
    import torch
    from csr_amd._lib import lib, check
    out = torch.full(((re_ - rb), k, k), np.nan, dtype=torch.float64, device='cuda')
    pb = None if dbase is None else dbase.data_ptr()
    if stream is None:
        check(lib.csrk_gram_rows_device(h.H, rb, re_, dV, ldv, k, code, int(scale), pb, out.data_ptr(), None))
        torch.cuda.synchronize()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            check(lib.csrk_gram_rows_device(h.H, rb, re_, dV, ldv, k, code, int(scale), pb, out.data_ptr(),
                                            C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('k', [3, 16, 17, 33, 64, 90])
@pytest.mark.parametrize('pdt', [np.float64, np.float32])
def test_variants_give_the_same_bits(k, pdt, limits):
    import torch
    from csr_amd.kernels import hip as K
    from csr_amd._lib import VAL_F32, VAL_F64
    nr, nc, rp, ci, vs = _pattern(_mixed_lens(limits), seed=k)
    V = _panel(k, pdt, k)
    base = _base(k, k)
    code = VAL_F64 if pdt == np.float64 else VAL_F32
    A32, A64 = _csr(nr, nc, rp, ci, vs), _csr(nr, nc, rp, ci, vs, ptr64=True)
    h32, h64 = K.to_handle(A32), K.to_handle(A64)
    try:
        assert K._info(h32.H)[3] == 0 and K._info(h64.H)[3] == 1
        for scale in (False, True):
            for b in (None, base):
                full = K.gram_rows(h32, V, scale, None, b)
                # the int64 twin, and a second call
                assert np.array_equal(_bits(full), _bits(K.gram_rows(h64, V, scale, None, b)))
                assert np.array_equal(_bits(full), _bits(K.gram_rows(h32, V, scale, None, b)))
                # the same rows asked for in ranges: an empty range, single rows, the rest
                for rb, re_ in ((0, 0), (0, 1), (1, 1), (1, 140), (140, 141), (141, 299), (299, 300), (300, 300)):
                    part = K.gram_rows(h32, V, scale, (rb, re_), b)
                    assert part.shape == (re_ - rb, k, k)
                    assert np.array_equal(_bits(part), _bits(full[rb:re_])), (rb, re_)
            # the host entry with a strided view (it packs the panel on the way)
            Vw = np.zeros((nc, k + 3), pdt)
            Vw[:, 1:1 + k] = V
            assert np.array_equal(_bits(full), _bits(K.gram_rows(h64, Vw[:, 1:1 + k], scale, None, base)))
            # the device entry, default stream and a side stream; V packed, at column 0 of a panel whose row stride is a
            # multiple of 16 B, and at column offset 1 of a wider panel (element loads)
            dbase = torch.from_numpy(base).cuda()
            wide = (k // 4 + 1) * 4
            for n, (off, ld) in enumerate(((0, k), (0, wide), (1, k + 3))):
                dV = torch.zeros(nc, ld, dtype=torch.from_numpy(V).dtype, device='cuda')
                dV[:, off:off + k] = torch.from_numpy(V).cuda()
                pv = dV[:, off:].data_ptr()
                assert (pv % 16 != 0) == (off == 1)
                st = torch.cuda.Stream() if n != 1 else None
                got = _device_call(h32 if n else h64, pv, ld, k, code, scale, 0, nr, dbase, st)
                assert np.array_equal(_bits(full), _bits(got)), (off, ld)
                got = _device_call(h32, pv, ld, k, code, scale, 137, 150, dbase, st)
                assert np.array_equal(_bits(full[137:150]), _bits(got)), (off, ld)
    finally:
        K.release_handle(h32)
        K.release_handle(h64)
    # a permutation of the rows: the Grams are permuted
    perm = np.random.default_rng(k).permutation(nr)
    got = A32.pick_rows(perm).gram_rows(V, weighted=True, base=base)
    assert np.array_equal(_bits(got), _bits(A32.gram_rows(V, weighted=True, base=base)[perm]))


# ---- special values by position -----------------------------------------------------------------------------

def _gram(K, nr, nc, rp, ci, vs, V, scale, base=None):
    h = K.to_handle(_csr(nr, nc, rp, ci, vs))
    try:
        return K.gram_rows(h, V, scale, None, base)
    finally:
        K.release_handle(h)


@pytest.mark.parametrize('k', [5, 20, 64])
def test_nan_and_inf_in_one_v_row_touch_only_the_rows_that_hold_it(k, limits):
    from csr_amd.kernels import hip as K
    nr, nc, rp, ci, vs = _pattern(_mixed_lens(limits), seed=50 + k)
    V = _panel(k, np.float64, k)
    clean = _gram(K, nr, nc, rp, ci, vs, V, True)
    Vs = V.copy()
    col = int(ci[rp[20]])                                       # a column some rows hold
    Vs[col, 0], Vs[col, 1], Vs[col, k - 1] = np.nan, np.inf, -np.inf
    got = _gram(K, nr, nc, rp, ci, vs, Vs, True)
    holds = np.array([col in ci[rp[r]:rp[r + 1]] for r in range(nr)])
    assert holds.any() and not holds.all()
    assert np.array_equal(_bits(got[~holds]), _bits(clean[~holds]))
    assert np.array_equal(R.classify(got), R.gram_positions(rp, ci, vs, Vs, True))
    assert (R.classify(got[holds]) != R.FINITE).any(axis=(1, 2)).all()
    fin = R.classify(got) == R.FINITE                           # what stayed finite in the touched rows kept its bits
    assert np.array_equal(_bits(got)[fin], _bits(clean)[fin])


def test_zero_weights_overflow_cancellation_and_subnormals():
    from csr_amd.kernels import hip as K
    k = 3
    V = np.zeros((NCOLS, k))
    V[0] = [np.inf, 2.0, -3.0]
    V[1] = [1e200, -1e200, 1.0]
    V[2] = [1.5, -2.5, 4.0]
    V[3] = [-1.5, 2.5, 4.0]
    rp = np.array([0, 1, 2, 3, 5, 7], np.int64)
    ci = np.array([0, 0, 1, 2, 3, 2, 2], np.int32)
    vs = np.array([0.0, -0.0, 1e200, 1.0, -1.0, 1.0, -1.0])
    got = _gram(K, 5, NCOLS, rp, ci, vs, V, True)
    want = R.gram_positions(rp, ci, vs, V, True)
    assert np.array_equal(R.classify(got), want)
    # rows 0 and 1: a 0.0 and a -0.0 weight times the Inf element is NaN (no zero is skipped); the finite part is +-0.0
    for r in (0, 1):
        assert np.isnan(got[r][:, 0]).all() and np.isnan(got[r][0, :]).all()
        assert np.all(got[r][1:, 1:] == 0.0)
    # row 2: t = round(1e200 * 1e200) overflows to +Inf, t = round(1e200 * -1e200) to -Inf
    assert got[2][0, 0] == np.inf and got[2][1, 0] == -np.inf and got[2][1, 1] == np.inf and got[2][2, 0] == 1e200 * 1e200
    # row 3: (1) v2 v2^T + (-1) v3 v3^T: the terms of (0,0), (1,0), (1,1), (2,2) cancel exactly, to +0.0
    for p, q in ((0, 0), (1, 0), (1, 1), (2, 2)):
        assert got[3][p, q] == 0.0 and not np.signbit(got[3][p, q]), (p, q)
    assert got[3][2, 0] == 12.0 and got[3][0, 2] == 12.0
    # row 4: the same entry with weights 1 and -1: every element cancels to +0.0
    assert np.all(got[4] == 0.0) and not np.signbit(got[4]).any()
    # float32 subnormal panel elements and values are widened, not flushed
    tiny = np.float32(2.0 ** -140)
    assert tiny > 0 and tiny < np.finfo(np.float32).tiny
    V32 = np.zeros((NCOLS, 2), np.float32)
    V32[0] = [tiny, 1.0]
    rp, ci = np.array([0, 1], np.int64), np.array([0], np.int32)
    g = _gram(K, 1, NCOLS, rp, ci, np.array([tiny], np.float32), V32, True)
    assert g[0][1, 0] == 2.0 ** -280 and g[0][0, 0] == 2.0 ** -420 and g[0][1, 1] == 2.0 ** -140
    g = _gram(K, 1, NCOLS, rp, ci, None, V32, False)
    assert g[0][1, 0] == 2.0 ** -140 and g[0][0, 0] == 2.0 ** -280 and g[0][1, 1] == 1.0


# ---- refusals and the cases without entries -----------------------------------------------------------------

def test_every_refusal_leaves_the_output_untouched():
    import torch
    from csr_amd.kernels import hip as K
    from csr_amd._lib import lib, ERR_INVALID, VAL_F64, VAL_F32
    nr, nc, rp, ci, vs = _pattern([2, 0, 3], 9)
    k = 4
    h = K.to_handle(_csr(nr, nc, rp, ci, vs))
    try:
        V = torch.ones(nc, k, dtype=torch.float64, device='cuda')
        out = torch.full((nr, k, k), -7.0, dtype=torch.float64, device='cuda')
        v, o = V.data_ptr(), out.data_ptr()
        bad = {
            'k = 0': (0, nr, v, k, 0, VAL_F64, 0, None, o, None),
            'k < 0': (0, nr, v, k, -1, VAL_F64, 0, None, o, None),
            'ldv < k': (0, nr, v, k - 1, k, VAL_F64, 0, None, o, None),
            'panel_type none': (0, nr, v, k, k, 0, 0, None, o, None),
            'panel_type 7': (0, nr, v, k, k, 7, 0, None, o, None),
            'scale 2': (0, nr, v, k, k, VAL_F64, 2, None, o, None),
            'scale -1': (0, nr, v, k, k, VAL_F32, -1, None, o, None),
            'row_begin < 0': (-1, nr, v, k, k, VAL_F64, 0, None, o, None),
            'row_end > nrows': (0, nr + 1, v, k, k, VAL_F64, 0, None, o, None),
            'row_begin > row_end': (2, 1, v, k, k, VAL_F64, 0, None, o, None),
            'NULL V': (0, nr, None, k, k, VAL_F64, 0, None, o, None),
        }
        for name, args in bad.items():
            assert lib.csrk_gram_rows_device(h.H, *args) == ERR_INVALID, name
            assert lib.csrk_last_error(), name
        assert lib.csrk_gram_rows_device(h.H, 0, nr, v, k, k, VAL_F64, 0, None, None, None) == ERR_INVALID      # NULL out
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())
        # the host entry refuses the same way
        Vh, oh = np.ones((nc, k)), np.full((nr, k, k), -7.0)
        for name, args in bad.items():
            a = list(args[:-1])
            a[2] = None if args[2] is None else Vh.ctypes.data
            a[8] = oh.ctypes.data
            assert lib.csrk_gram_rows(h.H, *a) == ERR_INVALID, name
        assert lib.csrk_gram_rows(h.H, 0, nr, Vh.ctypes.data, k, k, VAL_F64, 0, None, None) == ERR_INVALID      # NULL out
        assert np.all(oh == -7.0)
        # an empty range is fine and writes nothing, NULL pointers and all
        assert lib.csrk_gram_rows_device(h.H, 1, 1, None, k, k, VAL_F64, 0, None, None, None) == 0
        assert lib.csrk_gram_rows(h.H, 3, 3, None, k, k, VAL_F64, 0, None, None) == 0
        # the handle still computes
        assert np.array_equal(K.gram_rows(h, np.ones((nc, k)))[1], np.zeros((k, k)))
    finally:
        K.release_handle(h)


def test_no_rows_and_no_entries():
    from csr_amd.kernels import hip as K
    k = 5
    V = _panel(k, np.float64, 1)
    base = _base(k, 1)
    sym = np.tril(base) + np.tril(base, -1).T
    # nrows = 0: nothing to write
    got = _gram(K, 0, NCOLS, np.zeros(1, np.int64), np.zeros(0, np.int32), None, V, False, base)
    assert got.shape == (0, k, k)
    # nnz = 0: every row is empty -- all +0.0, or base mirrored
    rp = np.zeros(4, np.int64)
    for vs in (None, np.zeros(0)):
        got = _gram(K, 3, NCOLS, rp, np.zeros(0, np.int32), vs, V, True)
        assert np.array_equal(_bits(got), _bits(np.zeros((3, k, k))))
        got = _gram(K, 3, NCOLS, rp, np.zeros(0, np.int32), vs, V, True, base)
        assert np.array_equal(_bits(got), _bits(np.broadcast_to(sym, (3, k, k))))
