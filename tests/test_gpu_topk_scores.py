"""
csrk_topk_scores on the card (include/csrk.h), bit for bit against the restatements of tests/topk_scores_ref.py: the chain
against exact rational arithmetic on random float64 panels (where a multiply-then-add kernel is shown to fail), against the
vectorised loop on panels whose products are exact at every k, row-block, tile and n_top boundary that
csrk_topk_scores_limits names; running lists under ascending and descending scores; ties; the threshold and the padding;
NaN / Inf by position; the same bits from every variant of one request; the composition drop_entries + topk_rows; every
refusal with the outputs untouched.

Matrices have at most 2 * block + 8 rows and 3 * tile + 5 items (block and tile from the limits).  The exact chain costs
about 10^5 steps (rows x items x k) a second: the exact cases are sized by that.
"""
import ctypes as C

import numpy as np
import pytest

import topk_scores_ref as R

pytestmark = pytest.mark.gpu

INF = np.inf


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same(a, b):
    "equal bits, a NaN matching any NaN (a created NaN has its position specified, not its sign or payload)"
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _eq(got, want):
    return np.array_equal(got[0], want[0]) and _same(got[1], want[1]) and np.array_equal(got[2], want[2])


@pytest.fixture(scope='module')
def lim():
    from csr_amd.kernels import hip as K
    return tuple(int(v) for v in K.topk_scores_limits())


def _grid(shape, rng):
    "float64 on a grid coarse enough that every product is exact"
    return rng.integers(-512, 512, shape) / 64.0


def _f32(shape, rng):
    return rng.standard_normal(shape).astype(np.float32)


def _csr(nrows, ncols, cols, ptr64=False, values=False):
    "the seen matrix from one sorted array of columns per row"
    from csr_amd import CSR
    rp = np.zeros(nrows + 1, np.int64)
    rp[1:] = np.cumsum([len(c) for c in cols])
    ci = np.concatenate([np.asarray(c, np.int32) for c in cols] + [np.zeros(0, np.int32)]).astype(np.int32)
    vs = np.full(len(ci), np.nan) if values else None          # never read: NaN would show
    return CSR(nrows, ncols, int(rp[-1]), rp.astype(np.int64 if ptr64 else np.int32), ci, vs, _cast=False)


def _seen(S, n, seed, ptr64=False, values=False):
    "row r: r % 4 = 0 empty, 1 full, 2 exactly the row's n best items, 3 a random third"
    rng = np.random.default_rng(seed)
    m, ni = S.shape
    best = R.select(S, None, None, n)[0]
    cols = []
    for r in range(m):
        kind = r % 4
        if kind == 0:
            c = np.zeros(0, np.int32)
        elif kind == 1:
            c = np.arange(ni, dtype=np.int32)
        elif kind == 2:
            c = np.sort(best[r][best[r] >= 0])
        else:
            c = np.flatnonzero(rng.random(ni) < 0.33)
        cols.append(c.astype(np.int32))
    return _csr(m, ni, cols, ptr64, values)


def _host(csr, U, V, n, ms=None, rows=None):
    from csr_amd.kernels import hip as K, releasing
    if csr is None:
        return K.topk_scores(None, U, V, n, ms, rows)
    with releasing(K.to_handle(csr), K) as h:
        return K.topk_scores(h, U, V, n, ms, rows)


def _want(csr, U, V, n, ms=None, rows=None, S=None):
    S = R.scores_plain(U, V) if S is None else S
    rb, re_ = (0, S.shape[0]) if rows is None else rows
    if csr is None:
        return R.select(S[rb:re_], None, None, n, ms)
    return R.select(S[rb:re_], csr.rowptrs[rb:re_ + 1], csr.colinds, n, ms)


def _device(csr, U, V, n, ms=None, rows=None, *, pad=0, shift=0, extra=0, counts=True, stream=False, repeat=1):
    """
    The device entry on torch tensors: panels with `pad` extra elements per row (NaN: reading them would show) starting
    `shift` elements into their allocation, outputs `extra` columns wider than n (sentinels, returned as they are).
    """
    import torch
    from csr_amd._lib import lib, check
    from csr_amd.kernels import hip as K
    code = K._PANEL_CODES[U.dtype]
    rb, re_ = (0, U.shape[0]) if rows is None else rows
    m, k = re_ - rb, U.shape[1]
    keep = []

    def put(P):
        r, ld = P.shape[0], k + pad
        buf = torch.full((r * ld + shift + 1,), float('nan'), dtype=torch.from_numpy(P[:0]).dtype, device='cuda')
        if r:
            buf[shift:shift + r * ld].view(r, ld)[:, :k] = torch.from_numpy(np.ascontiguousarray(P)).cuda()
        keep.append(buf)
        return buf.data_ptr() + shift * P.dtype.itemsize, ld
    up, ldu = put(U)
    vp, ldv = put(V)
    items = torch.full((m, n + extra), -77, dtype=torch.int32, device='cuda')
    scores = torch.full((m, n + extra), 77.0, dtype=torch.float64, device='cuda')
    cnt = torch.full((max(m, 1),), -5, dtype=torch.int32, device='cuda')
    h = None if csr is None else K.to_handle(csr)
    try:
        s = torch.cuda.Stream() if stream else None
        torch.cuda.synchronize()
        for _ in range(repeat):
            check(lib.csrk_topk_scores_device(0 if h is None else h.H, rb, re_, up, ldu, vp, ldv, V.shape[0], k, code, n,
                                              -INF if ms is None else ms, items.data_ptr(), n + extra, scores.data_ptr(), n + extra,
                                              cnt.data_ptr() if counts else None, C.c_void_p(s.cuda_stream) if s else None))
        torch.cuda.synchronize()
    finally:
        if h is not None:
            K.release_handle(h)
    return items.cpu().numpy(), scores.cpu().numpy(), cnt.cpu().numpy()[:m]


# ---- 1. the chain against exact arithmetic ------------------------------------------------------------------------

@pytest.fixture(scope='module')
def exact_case():
    "seed 7, 6 x 130 x 8: the exact scores, once"
    rng = np.random.default_rng(7)
    U, V = rng.standard_normal((6, 8)), rng.standard_normal((130, 8))
    return U, V, R.scores_exact(U, V)


def test_exact_random_float64_where_two_roundings_fail(exact_case):
    U, V, S = exact_case
    S2 = R.scores_two_rounding(U, V)
    win = R.select(S, None, None, 10)
    differs = sum(1 for r in range(6) for q in range(10) if S2[r, win[0][r, q]] != win[1][r, q])
    print('scores that differ', np.count_nonzero(S2 != S), 'of', S.size, '; winners that differ', differs, 'of 60')
    assert differs >= 1          # a kernel that multiplies and then adds cannot pass what follows
    seen = _seen(S, 10, 1)
    for csr in (None, seen):
        assert _eq(_host(csr, U, V, 10), _want(csr, U, V, 10, S=S))
        assert _eq(_device(csr, U, V, 10)[:3], _want(csr, U, V, 10, S=S))


@pytest.mark.parametrize('k', [1, 2, 3, 5])
def test_exact_random_float64_small_k(k):
    rng = np.random.default_rng(70 + k)
    U, V = rng.standard_normal((8, k)), rng.standard_normal((130, k))
    S = R.scores_exact(U, V)
    seen = _seen(S, 4, k)
    assert _eq(_host(seen, U, V, 4), _want(seen, U, V, 4, S=S))
    assert _eq(_host(None, U, V, 128, rows=(1, 7)), _want(None, U, V, 128, rows=(1, 7), S=S))


# ---- 2. every boundary, on panels whose products are exact ---------------------------------------------------------

def _ks(lim):
    c = lim[4]
    return sorted({1, 4, 15, 16, 17, 33, 64, c - 1, c, c + 1, 2 * c + 1} - {0})


def _shapes(lim):
    B, T = lim[2], lim[3]
    rows = sorted({1, B - 1, B, B + 1, 2 * B + 3} - {0})
    items = sorted({1, T - 1, T, T + 1, 3 * T + 1} - {0})
    ntop = sorted({1, 2, 10, T, lim[1]})
    return rows, items, ntop


def test_every_k(lim):
    rows, items, ntop = _shapes(lim)
    for x, k in enumerate(_ks(lim)):
        for y, gen in enumerate((_f32, _grid)):
            rng = np.random.default_rng(100 * x + y)
            m, ni, n = rows[(x + y) % len(rows)], items[(2 * x + y + 1) % len(items)], ntop[(3 * x + y) % len(ntop)]
            U, V = gen((m + 5, k), rng), gen((ni, k), rng)
            S = R.scores_plain(U, V)
            csr = _seen(S, n, x, ptr64=bool(x % 2), values=bool(y)) if (x + y) % 3 else None
            rr = (3, 3 + m)
            assert _eq(_host(csr, U, V, n, rows=rr), _want(csr, U, V, n, rows=rr, S=S)), (k, gen.__name__, m, ni, n)


def test_every_row_count_and_item_count(lim):
    rows, items, ntop = _shapes(lim)
    rng = np.random.default_rng(5)
    x = 0
    for m in rows:
        for ni in items:
            x += 1
            n = ntop[x % len(ntop)]
            U, V = _f32((m + 4, 5), rng), _f32((ni, 5), rng)
            S = R.scores_plain(U, V)
            csr = _seen(S, n, x, ptr64=bool(x % 3 == 0)) if x % 2 else None
            rr = (3, 3 + m)
            assert _eq(_device(csr, U, V, n, rows=rr), _want(csr, U, V, n, rows=rr, S=S)), (m, ni, n)


def test_every_n_top_with_and_without_seen_in_both_pointer_widths(lim):
    rows, items, ntop = _shapes(lim)
    rng = np.random.default_rng(6)
    m, ni = lim[2] + 1, 3 * lim[3] + 1
    U, V = _grid((m, 17), rng), _grid((ni, 17), rng)
    S = R.scores_plain(U, V)
    for n in ntop:
        assert _eq(_host(None, U, V, n), _want(None, U, V, n, S=S)), n
        for ptr64 in (False, True):
            csr = _seen(S, n, n, ptr64=ptr64, values=ptr64)
            assert _eq(_host(csr, U, V, n), _want(csr, U, V, n, S=S)), (n, ptr64)


# ---- 3. the running list ---------------------------------------------------------------------------------------------

def test_ascending_descending_and_late_winners(lim):
    B, T, CAP = lim[2], lim[3], lim[5]
    m, ni = B + 1, 3 * T + 5
    U = (np.arange(m, dtype=np.float64) + 1.0)[:, None]
    up = np.arange(ni, dtype=np.float64)[:, None]                 # strictly ascending in item: every tile replaces the list
    late = np.zeros((ni, 1))
    late[3 * T:, 0] = [5.0, 9.0, 7.0, 8.0, 6.0]                    # all winners in the last, partial tile
    burst = np.ones((ni, 1))
    burst[T:2 * T, 0] = 100.0 + np.arange(T)                      # one tile brings more survivors than a list takes at once
    for name, V in (('ascending', up), ('descending', -up), ('late', late), ('burst', burst)):
        for n in (1, 5, CAP - 1, T, lim[1]):
            assert _eq(_host(None, U, V, n), _want(None, U, V, n)), (name, n)
    cols = [np.arange(ni - 1 - (r % 7), ni, dtype=np.int32) if r % 2 else np.zeros(0, np.int32) for r in range(m)]
    csr = _csr(m, ni, cols)                                       # the best items of every other row are seen
    assert _eq(_host(csr, U, up, 10), _want(csr, U, up, 10))


# ---- 4. ties -----------------------------------------------------------------------------------------------------------

def test_ties(lim):
    B, T = lim[2], lim[3]
    rng = np.random.default_rng(8)
    m, ni = 9, 2 * T + 3
    V = _grid((ni, 4), rng)
    # U = 0: every score is +0.0, the winners are the smallest unseen items
    cols = [np.arange(r, dtype=np.int32) for r in range(m)]
    csr = _csr(m, ni, cols)
    got = _host(csr, np.zeros((m, 4)), V, 5)
    assert _eq(got, _want(csr, np.zeros((m, 4)), V, 5))
    assert got[0].tolist() == [list(range(r, r + 5)) for r in range(m)] and not np.signbit(got[1]).any() and np.all(got[1] == 0.0)
    # the best row of V three times, across a tile border
    U = np.abs(_grid((m, 4), rng)) + 1.0
    Vd = np.abs(V)
    Vd[T - 1] = Vd[T] = Vd[T + 1] = 9.0
    got = _host(None, U, Vd, 2)
    assert _eq(got, _want(None, U, Vd, 2)) and np.all(got[0] == [T - 1, T])
    # a tie at the n-th place: only seven distinct rows of V
    Vt = V[np.arange(ni) % 7]
    for n in (1, 10, T):
        assert _eq(_host(None, U, Vt, n), _want(None, U, Vt, n)), n
    # -0.0 (an underflow of the chain) ties with +0.0 and keeps its sign
    Uz, Vz = np.array([[1e-200], [-1e-200]]), np.array([[-1e-200], [0.0], [1e-200], [-3.0], [-1e-200]])
    Sz = R.scores_exact(Uz, Vz)
    assert np.signbit(Sz).tolist() == [[True, False, False, True, True], [False, False, True, False, False]] and np.all(Sz[:, [0, 1, 2, 4]] == 0.0)
    got = _host(None, Uz, Vz, 4)
    assert _eq(got, R.select(Sz, None, None, 4)) and got[0].tolist() == [[0, 1, 2, 4], [3, 0, 1, 2]]
    assert np.signbit(got[1][0]).tolist() == [True, False, False, True]


# ---- 5. threshold and padding ----------------------------------------------------------------------------------------

def test_threshold_padding_and_strides(lim):
    T = lim[3]
    rng = np.random.default_rng(9)
    m, ni = 7, T + 9
    U, V = _grid((m, 6), rng), _grid((ni, 6), rng)
    S = R.scores_plain(U, V)
    csr = _seen(S, 3, 2)
    ms = float(np.sort(S[0])[-4])                                  # equal to a score: it passes
    want = _want(csr, U, V, 8, ms, S=S)
    assert want[2][0] >= 4 and (want[2] < 8).any() and ms in want[1][0]
    assert _eq(_host(csr, U, V, 8, ms), want)
    got = _device(csr, U, V, 8, ms, extra=3)
    assert _eq((got[0][:, :8], got[1][:, :8], got[2]), want)
    assert np.all(got[0][:, 8:] == -77) and np.all(got[1][:, 8:] == 77.0)          # columns beyond n_top are not touched
    got = _device(csr, U, V, 8, ms, counts=False)                  # counts may be NULL
    assert _eq((got[0], got[1], want[2]), want) and np.all(got[2] == -5)
    # n_top > n_items, and a threshold nothing passes (count 0: padding only)
    for n in (ni + 1, lim[1]):
        assert _eq(_host(csr, U, V, n), _want(csr, U, V, n, S=S)), n
    got = _host(csr, U, V, 3, INF)
    assert np.all(got[0] == -1) and np.all(got[1] == -INF) and np.all(got[2] == 0)
    assert _eq(_host(None, U, V, 3, -INF), _want(None, U, V, 3, S=S))
    # no items at all
    got = _host(None, U, np.zeros((0, 6)), 2)
    assert np.all(got[0] == -1) and np.all(got[1] == -INF) and np.all(got[2] == 0)


# ---- 6. special values -------------------------------------------------------------------------------------------------

def test_special_values_by_position(lim):
    T = lim[3]
    rng = np.random.default_rng(10)
    m, ni, j = 8, T + 7, T + 2
    U, V = _grid((m, 5), rng), _grid((ni, 5), rng)
    cols = [np.array([j] if r % 2 else [], np.int32) for r in range(m)]
    csr = _csr(m, ni, cols)
    base = _host(csr, U, V, 6)
    Vn = V.copy()
    Vn[j, 3] = np.nan
    got = _host(csr, U, Vn, 6)
    assert _eq(got, _want(csr, U, Vn, 6))
    for r in range(m):
        if r % 2:                                                  # seen: not one bit changes
            assert all(np.array_equal(_bits(a[r]), _bits(b[r])) for a, b in zip(got[:2], base[:2]))
        else:                                                      # not seen: the NaN ranks first
            assert got[0][r, 0] == j and np.isnan(got[1][r, 0])
    for bad in (np.nan, INF, -INF):
        Ub = U.copy()
        Ub[2, 1] = bad
        got = _host(csr, Ub, V, 6)
        assert _eq(got, _want(csr, Ub, V, 6))
        keep = np.arange(m) != 2
        assert all(np.array_equal(_bits(a[keep]), _bits(b[keep])) for a, b in zip(got[:2], base[:2]))
    # Inf - Inf inside a chain; 0 * Inf; no zero is skipped
    Ui = np.array([[INF, INF, 1.0], [0.0, 1.0, 1.0], [1.0, 1.0, 1.0]])
    Vi = np.array([[1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [INF, 0.0, 0.0], [0.0, 0.0, 2.0], [-INF, 1.0, 1.0]])
    got = _host(None, Ui, Vi, 5)
    assert _eq(got, _want(None, Ui, Vi, 5))
    nan = R.scores_positions(Ui, Vi)[0]
    assert nan.tolist() == [[True, False, True, True, True], [False, False, True, False, True], [False] * 5]
    assert [int(np.isnan(got[1][r]).sum()) for r in range(3)] == [4, 2, 0]


# ---- 7. invariance -----------------------------------------------------------------------------------------------------

def test_same_bits_from_every_variant(lim):
    B, T = lim[2], lim[3]
    rng = np.random.default_rng(12)
    m, ni, n = 2 * B + 3, 2 * T + 5, 10
    for gen, k in ((_f32, 20), (_grid, 18), (_f32, 7)):
        U, V = gen((m, k), rng), gen((ni, k), rng)
        S = R.scores_plain(U, V)
        csr = _seen(S, n, 3)
        whole = _want(csr, U, V, n, S=S)
        assert _eq(_host(csr, U, V, n), whole)
        cuts = [0, 1, B - 2, B + 7, B + 7, 2 * B, m]                # pieces, one of them empty
        parts = [_host(csr, U, V, n, rows=(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
        assert _eq(tuple(np.concatenate([p[x] for p in parts]) for x in range(3)), whole)
        for kw in (dict(), dict(pad=3), dict(shift=1), dict(pad=1, shift=1), dict(pad=4), dict(stream=True), dict(repeat=2),
                   dict(pad=2, shift=3, stream=True, extra=5)):
            got = _device(csr, U, V, n, **kw)
            assert _eq((got[0][:, :n], got[1][:, :n], got[2]), whole), (gen.__name__, k, kw)
        got = _device(csr, U, V, n, rows=(B - 1, B + 9), shift=1)
        assert _eq(got, tuple(w[B - 1:B + 9] for w in whole))


# ---- 8. composition ----------------------------------------------------------------------------------------------------

def test_equals_drop_entries_then_topk_rows(lim):
    from csr_amd import CSR
    T = lim[3]
    rng = np.random.default_rng(13)
    m, ni, n = 11, T + 6, 7
    U, V = _f32((m, 12), rng), _f32((ni, 12), rng)
    S = R.scores_plain(U, V)
    S[:, 5] = S[:, 3]                                              # ties, so that the tie rules have to agree too
    V[5] = V[3]
    seen = _seen(S, n, 4, values=True)
    seen.values[:] = 1.0
    dense = CSR(m, ni, m * ni, np.arange(0, m * ni + 1, ni, dtype=np.int32), np.tile(np.arange(ni, dtype=np.int32), m), S.ravel().copy(),
                _cast=False)
    top = dense.drop_entries(seen).topk_rows(n)
    got = seen.topk_scores(U, V, n)
    assert _eq(got, _want(seen, U, V, n, S=S))
    for r in range(m):
        a, b = int(top.rowptrs[r]), int(top.rowptrs[r + 1])
        assert b - a == got[2][r]
        assert np.array_equal(top.colinds[a:b], got[0][r, :b - a]) and np.array_equal(_bits(top.values[a:b]), _bits(got[1][r, :b - a]))
    free = seen.topk_scores(U, V, n, exclude=False)
    assert _eq(free, _want(None, U, V, n, S=S))


# ---- 9. refusals -------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing_and_limits_hold(lim):
    import torch
    from csr_amd._lib import lib, ERR_INVALID, ERR_UNSUPPORTED, VAL_F64
    from csr_amd.kernels import hip as K
    m, ni, k, n = 5, 9, 3, 4
    rng = np.random.default_rng(14)
    U, V = _grid((m, k), rng), _grid((ni, k), rng)
    tU, tV = torch.from_numpy(U).cuda(), torch.from_numpy(V).cuda()
    good_csr = _csr(m, ni, [np.array([1, 4], np.int32)] * m)
    bad_csr = _csr(m, ni, [np.array([1, 4], np.int32), np.array([2, 7], np.int32), np.array([4, 4], np.int32), np.array([5, 2], np.int32),
                           np.zeros(0, np.int32)])
    other = _csr(m, ni + 1, [np.zeros(0, np.int32)] * m)
    hg, hb, ho = K.to_handle(good_csr), K.to_handle(bad_csr), K.to_handle(other)
    nan = float('nan')
    try:
        for form in ('host', 'device'):
            if form == 'host':
                items, scores, counts = np.full((m, n), 7, np.int32), np.full((m, n), 7.0), np.full(m, 7, np.int32)
                p = dict(u=U.ctypes.data, v=V.ctypes.data, it=items.ctypes.data, sc=scores.ctypes.data, cn=counts.ctypes.data)
            else:
                items = torch.full((m, n), 7, dtype=torch.int32, device='cuda')
                scores = torch.full((m, n), 7.0, dtype=torch.float64, device='cuda')
                counts = torch.full((m,), 7, dtype=torch.int32, device='cuda')
                p = dict(u=tU.data_ptr(), v=tV.data_ptr(), it=items.data_ptr(), sc=scores.data_ptr(), cn=counts.data_ptr())

            def call(**ch):
                a = dict(dict(h=hg.H, rb=0, re=m, ldu=k, ldv=k, ni=ni, k=k, pt=VAL_F64, nt=n, ms=-INF, ldi=n, lds=n, **p), **ch)
                args = (a['h'], a['rb'], a['re'], a['u'], a['ldu'], a['v'], a['ldv'], a['ni'], a['k'], a['pt'], a['nt'], a['ms'], a['it'],
                        a['ldi'], a['sc'], a['lds'], a['cn'])
                return lib.csrk_topk_scores(*args) if form == 'host' else lib.csrk_topk_scores_device(*args, None)
            invalid = {'k < 1': dict(k=0), 'n_top < 1': dict(nt=0), 'n_items < 0': dict(h=0, ni=-1), 'ldu < k': dict(ldu=k - 1),
                       'ldv < k': dict(ldv=k - 1), 'ldi < n_top': dict(ldi=n - 1), 'lds < n_top': dict(lds=n - 1), 'panel type': dict(pt=9),
                       'NaN min_score': dict(ms=nan), 'row_begin < 0': dict(rb=-1), 'row_begin > row_end': dict(rb=3, re=2),
                       'row_end > nrows': dict(re=m + 1), 'n_items != ncols': dict(h=ho.H), 'not canonical': dict(h=hb.H),
                       'not a handle': dict(h=12345), 'NULL items': dict(it=None), 'NULL scores': dict(sc=None), 'NULL U': dict(u=None),
                       'NULL V': dict(v=None)}
            for name, ch in invalid.items():
                assert call(**ch) == ERR_INVALID, (form, name)
                if name == 'not canonical':
                    assert b'row 2' in lib.csrk_last_error()          # the first bad row, as csrk_combine names it
            assert call(k=lim[0] + 1, ldu=lim[0] + 1, ldv=lim[0] + 1) == ERR_UNSUPPORTED
            assert call(nt=lim[1] + 1, ldi=lim[1] + 1, lds=lim[1] + 1) == ERR_UNSUPPORTED
            assert call(rb=2, re=2, u=None, v=None, it=None, sc=None, cn=None) == 0          # no rows: nothing launched
            if form == 'device':
                torch.cuda.synchronize()
                items, scores, counts = items.cpu().numpy(), scores.cpu().numpy(), counts.cpu().numpy()
            assert np.all(items == 7) and np.all(scores == 7.0) and np.all(counts == 7), form
            assert K.is_canonical(hg) == (True, None) and K.is_canonical(hb) == (False, 2)
    finally:
        for h in (hg, hb, ho):
            K.release_handle(h)
    # success at both limits
    kmax, nmax = lim[0], lim[1]
    Uk, Vk = _grid((2, kmax), rng), _grid((5, kmax), rng)
    assert _eq(_host(None, Uk, Vk, 3), _want(None, Uk, Vk, 3))
    Vn = _grid((nmax + 40, k), rng)
    assert _eq(_host(None, U, Vn, nmax), _want(None, U, Vn, nmax))
