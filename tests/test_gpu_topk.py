"""
Row top-k on the card (csrk_topk_rows, csrc/topk.hip) against the NumPy restatement of its contract (tests/topk_ref.py).
Selection and copying only, so every comparison is exact: np.array_equal on rowptrs, on colinds and on the values viewed
as integers.  Every row of every case is checked.
"""
import ctypes as C

import numpy as np
import pytest

from topk_ref import topk_rows_vec, topk_rows_ref, topk_keep, same, bits

pytestmark = pytest.mark.gpu

INF, NAN = float('inf'), float('nan')
KS = (1, 2, 5, 64, 65, 100, 1000, 5000, 10 ** 6)
ORDERS = ('descending', 'storage')
PATTERNS = ('distinct', 'ties', 'equal', 'all_nan', 'special')


def _K():
    from csr_amd.kernels import hip as K
    return K


def _lens(big=True, seed=1):
    "every boundary the issue names and those of the implementation (read from the library), runs of empty rows, one row of 300 000"
    short, cap, _, mid = _K().topk_limits()
    rng = np.random.default_rng(seed)
    edge = [0, 1, 2, 15, 16, 17, 63, 64, 65, short - 1, short, short + 1, 1023, 1024, 1025, mid - 1, mid, mid + 1, cap - 1, cap, cap + 1]
    lens = [0] * 5 + edge[:12] + [0] * 70 + edge[12:] + ([300_000] if big else [20_000]) + [0] * 3
    lens += list(rng.integers(0, 40, 200)) + [0] * 4
    return np.asarray(lens, np.int64)


def _nan_bits(dtype, rng, n):
    "NaNs of both signs with payloads (float32: signalling ones too)"
    if dtype == np.float32:
        pay = rng.integers(1, 1 << 23, n).astype(np.uint32)
        return (np.uint32(0x7f800000) | pay | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))).view(np.int32)
    pay = rng.integers(1, 1 << 52, n).astype(np.uint64)
    return (np.uint64(0x7ff0000000000000) | pay | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63))).view(np.int64)


def _values(pattern, n, dtype, seed):
    rng = np.random.default_rng(seed)
    if pattern == 'distinct':
        return rng.uniform(-1, 1, n).astype(dtype)
    if pattern == 'ties':
        return rng.integers(-3, 4, n).astype(dtype)
    if pattern == 'equal':
        return np.full(n, 0.75, dtype)
    vs = rng.uniform(-1, 1, n).astype(dtype)
    if pattern == 'all_nan':
        bits(vs)[:] = _nan_bits(dtype, rng, n)
        return vs
    assert pattern == 'special'
    tiny = np.array([1e-40, -1e-40, 1.4e-45, -1.4e-45], np.float32).astype(dtype) if dtype == np.float32 else \
        np.array([5e-324, -5e-324, 1e-310, np.float64(np.float32(1e-40))])
    sp = np.concatenate([np.array([INF, -INF, 0.0, -0.0, 0.0, -0.0], dtype), tiny])
    at = rng.choice(n, n // 4, replace=False)
    vs[at] = sp[rng.integers(0, len(sp), len(at))]
    at = rng.choice(n, n // 10, replace=False)
    bits(vs)[at] = _nan_bits(dtype, rng, len(at))
    return vs


def _arrays(lens, pattern='distinct', dtype=np.float64, seed=3, ncols=1000):
    "unsorted columns in [0, ncols): the long rows hold columns more than once"
    rng = np.random.default_rng(seed)
    rp = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    n = int(rp[-1])
    return rp, rng.integers(0, ncols, n).astype(np.int32), _values(pattern, n, dtype, seed + 1), ncols


def _csr(arrs, ptr64=False):
    from csr_amd import CSR
    rp, ci, vs, nc = arrs
    return CSR(len(rp) - 1, nc, int(rp[-1]), rp.astype(np.int64 if ptr64 else np.int32), ci.copy(), None if vs is None else vs.copy(),
               _cast=False)


def _top(h, k, mv=None, order='descending'):
    K = _K()
    t = K.topk_rows(h, k, mv, order)
    try:
        c = K.from_handle(t)
    finally:
        K.release_handle(t)
    return c.rowptrs, c.colinds, c.values


def _expect(arrs, k, mv, order):
    rp, ci, vs, _ = arrs
    return topk_rows_vec(rp, ci, vs, k, -INF if mv is None else mv, order)


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('pattern', PATTERNS)
def test_every_length_k_order_and_threshold(pattern, dtype):
    K = _K()
    arrs = _arrays(_lens(), pattern, dtype)
    vs = arrs[2]
    finite = vs[np.isfinite(vs)]
    quant = float(np.quantile(finite.astype(np.float64), 0.7)) if len(finite) else 0.5
    h = K.to_handle(_csr(arrs))
    try:
        for k in KS:
            for order in ORDERS:
                got = _top(h, k, None, order)
                assert got[0].dtype == np.int32 and got[2].dtype == dtype
                assert same(got, _expect(arrs, k, None, order)), (k, order)
        for mv in (-INF, 0.0, quant, INF):
            for k in (5, 100, 5000):
                for order in ORDERS:
                    assert same(_top(h, k, mv, order), _expect(arrs, k, mv, order)), (mv, k, order)
    finally:
        K.release_handle(h)
    if pattern == 'special':      # what the case is for did travel: NaN payloads and -0.0 among the kept entries
        _, _, kv = _expect(arrs, 1000, None, 'descending')
        with np.errstate(invalid='ignore'):      # (widening a signalling NaN raises the flag; the value is what is wanted)
            w = kv.astype(np.float64)
        assert np.any(np.isnan(w) & np.signbit(w)) and np.any((w == 0) & np.signbit(w)) and len(np.unique(bits(kv[np.isnan(w)]))) > 10
        if dtype == np.float32:
            assert np.any((np.abs(w) > 0) & (np.abs(w) < 1e-38))


def test_vectorised_restatement_equals_the_row_loop_on_the_test_matrix():
    arrs = _arrays(_lens(big=False), 'special', np.float32)
    rp, ci, vs, _ = arrs
    for k in (1, 64, 5000):
        for mv in (-INF, 0.0):
            for order in ORDERS:
                assert same(topk_rows_vec(rp, ci, vs, k, mv, order), topk_rows_ref(rp, ci, vs, k, mv, order))


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_int32_and_int64_row_pointers_give_the_same_arrays(dtype):
    K = _K()
    arrs = _arrays(_lens(big=False), 'ties', dtype, seed=11)
    out = {}
    for p64 in (False, True):
        h = K.to_handle(_csr(arrs, p64))
        try:
            assert K._info(h.H)[3] == int(p64)
            out[p64] = [_top(h, k, mv, order) for k in (1, 5, 65, 5000) for mv in (None, 0.0) for order in ORDERS]
        finally:
            K.release_handle(h)
    i = 0
    for k in (1, 5, 65, 5000):
        for mv in (None, 0.0):
            for order in ORDERS:
                a, b = out[False][i], out[True][i]
                assert a[0].dtype == np.int32 and b[0].dtype == np.int32       # the layout rule: int32 unless the RESULT needs more
                assert same(a, b) and same(a, _expect(arrs, k, mv, order)), (k, mv, order)
                i += 1


def test_invariants():
    K = _K()
    arrs = _arrays(_lens(big=False), 'ties', np.float64, seed=21)
    rp, ci, vs, nc = arrs
    A = _csr(arrs)
    h = K.to_handle(A)
    try:
        for k in (3, 100, 5000):
            for mv in (None, 1.0):
                byv = _top(h, k, mv, 'descending')
                sto = _top(h, k, mv, 'storage')
                # two calls give identical bytes
                again = _top(h, k, mv, 'descending')
                assert all(x.tobytes() == y.tobytes() for x, y in zip(byv, again))
                # idempotent, in either order
                for order, first in (('descending', byv), ('storage', sto)):
                    from csr_amd import CSR
                    T = CSR(A.nrows, nc, len(first[1]), first[0], first[1], first[2], _cast=False)
                    th = K.to_handle(T)
                    try:
                        assert same(_top(th, k, mv, order), first), (k, mv, order)
                    finally:
                        K.release_handle(th)
                # storage order == the by-value result re-sorted by input position: both keep the same entries of each row, and
                # the storage-order result is a subsequence of the input row
                assert np.array_equal(byv[0], sto[0])
                for i in range(A.nrows):
                    s, e = int(sto[0][i]), int(sto[0][i + 1])
                    if s == e:
                        continue
                    a = sorted(zip(byv[1][s:e].tolist(), bits(byv[2][s:e]).tolist()))
                    b = sorted(zip(sto[1][s:e].tolist(), bits(sto[2][s:e]).tolist()))
                    assert a == b, i
                exp_pos = topk_rows_vec(rp, np.arange(len(ci), dtype=np.int32), vs, k, -INF if mv is None else mv, 'storage')[1]
                assert np.array_equal(sto[1], ci[exp_pos]) and np.all(np.diff(exp_pos) > 0)
        # k >= the longest row, no threshold, storage order: A's arrays unchanged
        kmax = int(np.diff(rp).max())
        for k in (kmax, kmax + 1, 10 ** 9, 2 ** 40):
            assert same(_top(h, k, None, 'storage'), (rp, ci, vs)), k
        # rows are independent: top-k commutes with picking rows (a permutation with repeats)
        rng = np.random.default_rng(4)
        p = np.concatenate([rng.permutation(A.nrows), rng.integers(0, A.nrows, 50)]).astype(np.int32)
        for order in ORDERS:
            ph = K.pick_rows(h, p)
            t = K.topk_rows(h, 70, 0.0, order)
            pt = K.pick_rows(t, p)
            try:
                left = _top(ph, 70, 0.0, order)
                c = K.from_handle(pt)
                assert same(left, (c.rowptrs, c.colinds, c.values)), order
            finally:
                for x in (ph, t, pt):
                    K.release_handle(x)
    finally:
        K.release_handle(h)


def test_input_handle_is_untouched_and_keeps_its_plan():
    from csr_amd import CSR, synth
    from csr_amd._lib import lib, check
    K = _K()
    m = synth.powerlaw_csr(40000, 600000, 1500000, device='cpu')
    W = CSR(40000, 600000, 1500000, m['rowptrs'].numpy(), m['colinds'].numpy(), m['values'].numpy())
    x = synth.dense_vector(600000).numpy()
    h = K.to_handle(W)
    try:
        ys = [K.mult_vec(h, x) for _ in range(3)]                   # the plan is built on the second product
        st0, st1 = (C.c_int64 * 34)(), (C.c_int64 * 34)()
        check(lib.csrk_spmv_plan_stats(h.H, st0, 34))
        b0, b1 = C.c_int64(0), C.c_int64(0)
        check(lib.csrk_device_bytes(h.H, C.byref(b0)))
        assert st0[25] > 0, 'the handle has no SpMV plan to keep'
        for order in ORDERS:
            got = _top(h, 10, 0.0, order)
            assert same(got, topk_rows_vec(W.rowptrs, W.colinds, W.values, 10, 0.0, order))
        check(lib.csrk_spmv_plan_stats(h.H, st1, 34))
        check(lib.csrk_device_bytes(h.H, C.byref(b1)))
        assert list(st0) == list(st1) and b0.value == b1.value
        y = K.mult_vec(h, x)
        assert y.tobytes() == ys[2].tobytes()
        back = K.from_handle(h)
        assert same((back.rowptrs, back.colinds, back.values), (W.rowptrs, W.colinds, W.values))
    finally:
        K.release_handle(h)


def _small_pair(seed=8):
    rng = np.random.default_rng(seed)
    from csr_amd import CSR

    def rnd(nr, nc, nnz):
        r, c = rng.integers(0, nr, nnz), rng.integers(0, nc, nnz)
        key = np.unique(r * nc + c)
        return CSR.from_coo(key // nc, key % nc, rng.integers(-2, 3, len(key)).astype(np.float64), (nr, nc))
    return rnd(300, 120, 14000), rnd(120, 90, 2500), rnd(260, 120, 3500)


def test_on_a_device_resident_product():
    K = _K()
    A, _, Bt = _small_pair()
    a, b = K.to_handle(A), K.to_handle(Bt)
    try:
        c = K.mult_abt(a, b)
        try:
            P = K.from_handle(c)
            for k, mv, order in ((5, None, 'descending'), (5, 0.0, 'storage'), (1000, 1.0, 'descending')):
                assert same(_top(c, k, mv, order), topk_rows_vec(P.rowptrs, P.colinds, P.values, k, -INF if mv is None else mv, order))
        finally:
            K.release_handle(c)
    finally:
        K.release_handle(a)
        K.release_handle(b)


@pytest.mark.parametrize('spgemm_order', ['reference', 'ascending'])
@pytest.mark.parametrize('transpose', [False, True])
def test_multiply_topk_equals_multiply_then_topk(transpose, spgemm_order, monkeypatch):
    K = _K()
    A, B, Bt = _small_pair()
    other = Bt if transpose else B
    K.set_spgemm_order(spgemm_order)
    try:
        for limit in (None, 3500):      # one row block, then several (A: ~11 000 entries, B and B^T within the limit; a product row holds at most 260)
            if limit is not None:
                monkeypatch.setattr(K, 'max_nnz', limit)
                assert len(A._row_blocks(K.max_nnz)) > 2
            P = A.multiply(other, transpose=transpose)
            assert P.nnz > 0
            for k, mv, order in ((7, None, 'descending'), (7, 0.0, 'storage'), (40, 2.0, 'descending'), (10 ** 6, None, 'storage')):
                two = P.topk_rows(k, min_value=mv, order=order)
                one = A.multiply_topk(other, k, transpose=transpose, min_value=mv, order=order)
                assert (one.nrows, one.ncols, one.nnz) == (two.nrows, two.ncols, two.nnz)
                assert one.rowptrs.dtype == two.rowptrs.dtype
                assert same((one.rowptrs, one.colinds, one.values), (two.rowptrs, two.colinds, two.values)), (limit, k, mv, order)
                assert same((one.rowptrs, one.colinds, one.values),
                            topk_rows_vec(P.rowptrs, P.colinds, P.values, k, -INF if mv is None else mv, order))
    finally:
        K.set_spgemm_order(None)


def test_after_sddmm():
    A, _, _ = _small_pair()
    rng = np.random.default_rng(2)
    U, V = rng.uniform(-1, 1, (A.nrows, 8)), rng.uniform(-1, 1, (A.ncols, 8))
    S = A.sddmm(U, V)
    for k, order in ((3, 'descending'), (10, 'storage')):
        T = S.topk_rows(k, order=order)
        assert (T.nrows, T.ncols) == (S.nrows, S.ncols)
        assert same((T.rowptrs, T.colinds, T.values), topk_rows_vec(S.rowptrs, S.colinds, S.values, k, -INF, order))


def test_refusals_on_the_card_leave_the_library_usable():
    from csr_amd._lib import lib, ERR_INVALID, handle_t
    K = _K()
    arrs = _arrays(np.array([3, 0, 70, 5]), 'distinct')
    h = K.to_handle(_csr(arrs))
    s = K.to_handle(_csr((arrs[0], arrs[1], None, arrs[3])))
    try:
        out = handle_t(5)
        for H, k, mv, order, word in ((s.H, 2, -INF, 0, b'no values'), (h.H, 0, -INF, 0, b'k must'), (h.H, -1, 0.0, 1, b'k must'),
                                      (h.H, 2, -INF, 7, b'order'), (h.H, 2, NAN, 0, b'NaN')):
            assert lib.csrk_topk_rows(H, k, mv, order, C.byref(out)) == ERR_INVALID
            assert word in lib.csrk_last_error() and out.value == 0
            with pytest.raises(ValueError):
                K._call(lib.csrk_topk_rows, H, k, mv, order, C.byref(out))
        with pytest.raises(ValueError):
            K.topk_rows(s, 2)
        assert same(_top(h, 2, None, 'descending'), _expect(arrs, 2, None, 'descending'))
    finally:
        K.release_handle(h)
        K.release_handle(s)


def test_empty_matrices():
    from csr_amd import CSR
    K = _K()
    for nr, nc in ((0, 5), (7, 5), (1, 1), (0, 0)):
        for dtype in (np.float64, np.float32):
            for p64 in (False, True):
                E = CSR(nr, nc, 0, np.zeros(nr + 1, np.int64 if p64 else np.int32), np.zeros(0, np.int32), np.zeros(0, dtype), _cast=False)
                h = K.to_handle(E)
                try:
                    for order in ORDERS:
                        t = K.topk_rows(h, 3, 0.0, order)
                        assert (t.nrows, t.ncols, t.nnz) == (nr, nc, 0)
                        c = K.from_handle(t)
                        K.release_handle(t)
                        assert c.rowptrs.dtype == np.int32 and np.array_equal(c.rowptrs, np.zeros(nr + 1)) and len(c.colinds) == 0
                        assert c.values is not None and c.values.dtype == dtype and len(c.values) == 0
                finally:
                    K.release_handle(h)
        got = CSR(nr, nc, 0, np.zeros(nr + 1, np.int32), np.zeros(0, np.int32), np.zeros(0)).topk_rows(2)
        assert (got.nrows, got.ncols, got.nnz) == (nr, nc, 0)


def test_at_size_knn_block():
    "the bench_secondary.abt block: rows of the MovieLens-25M-shaped matrix, 2000 x 20000^T, k = 20, min_value = 0, the whole result"
    import torch
    from csr_amd import CSR, synth
    K = _K()
    m = synth.movielens_like(device='cuda')
    nc = int(m['ncols'])
    rp = m['rowptrs'][:20001].cpu().numpy()
    eb = int(rp[-1])
    ci, vs = m['colinds'][:eb].cpu().numpy(), m['values'][:eb].cpu().numpy()
    del m
    torch.cuda.empty_cache()
    ea = int(rp[2000])
    A = CSR(2000, nc, ea, rp[:2001].copy(), ci[:ea].copy(), vs[:ea].copy())
    B = CSR(20000, nc, eb, rp, ci, vs)
    a, b = K.to_handle(A), K.to_handle(B)
    try:
        c = K.mult_abt(a, b)
        f = K.filter_zeros(c)
        K.release_handle(c)
        try:
            P = K.from_handle(f)
            assert P.nnz > 30_000_000                      # rows almost full: the long-row class at its real length
            got = {order: _top(f, 20, 0.0, order) for order in ORDERS}
        finally:
            K.release_handle(f)
    finally:
        K.release_handle(a)
        K.release_handle(b)
    keep = topk_keep(P.rowptrs, P.values, 20, 0.0)           # one sort of the whole product serves both orders
    for order in ORDERS:
        exp = topk_rows_vec(P.rowptrs, P.colinds, P.values, 20, 0.0, order, keep=keep)
        assert same(got[order], exp), order
    fused = A.multiply_topk(B, 20, transpose=True, min_value=0.0)
    assert same((fused.rowptrs, fused.colinds, fused.values), got['descending'])
