"""
csrk_topk_scores_for on the card (include/csrk.h), bit for bit against the restatements of tests/topk_scores_ref.py applied to
the gathered rows, and against csrk_topk_scores where the list is a range: shuffled lists with repeats at every length around
a row block, the four kinds of seen row in both pointer widths and both panel types; every number of splits, forced and
automatic, with the winners in the last range, in the first, tied across range boundaries, with empty partial lists and with
partial lists shorter than n; the device form's strides, alignment, stream, workspace bounds and bad indices; every refusal
with the outputs and the workspace untouched.

Panels are on the exact-product grids of tests/test_gpu_topk_scores.py (restated here), so the plain loop is the chain.
Matrices have at most 2 * block + 8 rows and 4 * tile + 5 items (five tiles), except one case of S_max + 1 tiles and 3 rows.
"""
import ctypes as C

import numpy as np
import pytest

import topk_scores_ref as R

pytestmark = pytest.mark.gpu

INF = np.inf
NTOPS = (1, 32, 33, 128)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same(a, b):
    "equal bits, a NaN matching any NaN (a created NaN has its position specified, not its sign or payload)"
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _eq(got, want):
    return np.array_equal(got[0], want[0]) and _same(got[1], want[1]) and np.array_equal(got[2], want[2])


def _ident(got, want):
    "the same bytes in every array (two runs of the library against each other)"
    return all(np.asarray(g).shape == np.asarray(w).shape and np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


@pytest.fixture(scope='module')
def lim():
    "(rows of a block, items of a tile, S_max) and the two full tuples"
    from csr_amd.kernels import hip as K
    t, f = tuple(int(v) for v in K.topk_scores_limits()), tuple(int(v) for v in K.topk_scores_for_limits())
    assert t[2] == 64 and t[3] == 64          # the shapes below are written for these
    return t, f


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


def _want(csr, users, S, n, ms=None):
    "R.select on the gathered rows of the scores and of the seen pattern"
    users = np.asarray(users, np.int64)
    if csr is None:
        return R.select(S[users], None, None, n, ms)
    rp = np.concatenate([[0], np.cumsum(np.diff(csr.rowptrs)[users])]).astype(np.int64)
    ci = np.concatenate([csr.colinds[int(csr.rowptrs[u]):int(csr.rowptrs[u + 1])] for u in users] + [np.zeros(0, np.int32)])
    return R.select(S[users], rp, ci, n, ms)


def _host(csr, users, U, V, n, ms=None, splits=None):
    from csr_amd.kernels import hip as K, releasing
    if csr is None:
        return K.topk_scores_for(None, users, U, V, n, ms, splits)
    with releasing(K.to_handle(csr), K) as h:
        return K.topk_scores_for(h, users, U, V, n, ms, splits)


GUARD = 256


def _device(csr, users, U, V, n, ms=None, splits=0, *, pad=0, shift=0, extra=0, counts=True, stream=False, repeat=1, at=64, slack=0,
            u_rows=None):
    """
    The device entry on torch tensors: panels with `pad` extra elements per row (NaN: reading them would show) starting
    `shift` elements into their allocation, outputs `extra` columns wider than n (sentinels, returned as they are), the
    workspace of exactly the reported size `at` bytes into a tensor of 0x5a bytes whose other bytes must stay as they are.
    """
    import torch
    from csr_amd._lib import lib, check
    from csr_amd.kernels import hip as K
    code = K._PANEL_CODES[U.dtype]
    users = np.asarray(users, np.int32)
    m, k = len(users), U.shape[1]
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
    d_users = torch.from_numpy(users).cuda() if m else torch.zeros(1, dtype=torch.int32, device='cuda')
    items = torch.full((m, n + extra), -77, dtype=torch.int32, device='cuda')
    scores = torch.full((m, n + extra), 77.0, dtype=torch.float64, device='cuda')
    cnt = torch.full((max(m, 1),), -5, dtype=torch.int32, device='cuda')
    used, need = K.topk_scores_for_workspace(m, V.shape[0], n, splits or None)
    assert at % 16 == 0 and at + need <= 2 * GUARD + need
    work = torch.full((need + 2 * GUARD,), 0x5a, dtype=torch.uint8, device='cuda')
    assert work.data_ptr() % 16 == 0
    h = None if csr is None else K.to_handle(csr)
    try:
        s = torch.cuda.Stream() if stream else None
        torch.cuda.synchronize()
        for _ in range(repeat):
            check(lib.csrk_topk_scores_for_device(0 if h is None else h.H, d_users.data_ptr(), m, U.shape[0] if u_rows is None else u_rows,
                                                  up, ldu, vp, ldv, V.shape[0], k, code, n, -INF if ms is None else ms, items.data_ptr(),
                                                  n + extra, scores.data_ptr(), n + extra, cnt.data_ptr() if counts else None, splits,
                                                  work.data_ptr() + at if need else None, need + slack,
                                                  C.c_void_p(s.cuda_stream) if s else None))
        torch.cuda.synchronize()
    finally:
        if h is not None:
            K.release_handle(h)
    w = work.cpu().numpy()
    assert np.all(w[:at] == 0x5a) and np.all(w[at + need:] == 0x5a), 'the workspace was written outside its reported size'
    return items.cpu().numpy(), scores.cpu().numpy(), cnt.cpu().numpy()[:m]


def _list(rng, nrows, length):
    "a shuffled list with repeats: about a fifth of the positions repeat another"
    base = rng.permutation(nrows)[:max(1, min(length, nrows) - length // 5)]
    users = np.concatenate([base, rng.choice(base, length - len(base))]) if length > len(base) else base[:length]
    return rng.permutation(users).astype(np.int64)


# ---- 1. lists --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def cases():
    "136 x 261 on both grids with k = 5 and 16: panels, scores and one seen matrix per n, once"
    out = {}
    for x, (gen, k) in enumerate(((_grid, 5), (_f32, 16), (_grid, 16), (_f32, 5))):
        rng = np.random.default_rng(40 + x)
        U, V = gen((136, k), rng), gen((261, k), rng)
        S = R.scores_plain(U, V)
        seen = {n: _seen(S, n, 10 * x + y, ptr64=bool((x + y) % 2), values=bool(y % 2)) for y, n in enumerate(NTOPS)}
        out[gen.__name__, k] = (U, V, S, seen)
    return out


@pytest.mark.parametrize('length', [1, 63, 64, 65, 130])
def test_shuffled_lists_with_repeats(cases, lim, length):
    rng = np.random.default_rng(length)
    for x, ((name, k), (U, V, S, seen)) in enumerate(sorted(cases.items())):
        for y, n in enumerate(NTOPS):
            users = _list(rng, 136, length)
            if length >= 63:
                assert len(np.unique(users)) < len(users) and np.any(np.diff(users) < 0)
            csr = seen[n] if (x + y) % 4 else None
            want = _want(csr, users, S, n)
            assert _eq(_host(csr, users, U, V, n), want), (name, k, n, 'host, automatic')
            sp = (1, 2, 5, 0)[(x + y) % 4]
            assert _eq(_device(csr, users, U, V, n, splits=sp), want), (name, k, n, 'device', sp)
    # each occurrence of a row gets the same bits
    U, V, S, seen = cases['_f32', 16]
    got = _host(seen[32], [7, 135, 7, 7, 2, 135], U, V, 32)
    assert all(_ident((a[0], a[0], a[1]), (a[2], a[3], a[5])) for a in got)


# ---- 2. agreement with the range entry ----------------------------------------------------------------------------------------

SPLITS = (1, 2, 3, 4, 5, 9)          # 261 items are five tiles: 9 is clamped to 5


def test_a_range_as_a_list_equals_the_range_entry(cases, lim):
    from csr_amd.kernels import hip as K, releasing
    for x, ((name, k), (U, V, S, seen)) in enumerate(sorted(cases.items())):
        n = NTOPS[x % 4]
        ms = (None, 0.0)[x % 2]
        with releasing(K.to_handle(seen[n]), K) as h:
            for b, e in ((0, 136), (3, 70), (64, 128), (5, 6)):
                rng_entry = K.topk_scores(h, U, V, n, ms, (b, e))
                assert _eq(rng_entry, _want(seen[n], np.arange(b, e), S, n, ms))
                for sp in SPLITS + (None,):
                    got = K.topk_scores_for(h, np.arange(b, e), U, V, n, ms, sp)
                    assert _ident(got, rng_entry), (name, k, n, b, e, sp)


# ---- 3. splits change nothing ---------------------------------------------------------------------------------------------------

def test_every_number_of_splits_gives_the_same_bits(cases, lim):
    from csr_amd.kernels import hip as K
    rng = np.random.default_rng(3)
    for x, ((name, k), (U, V, S, seen)) in enumerate(sorted(cases.items())):
        n = NTOPS[(x + 1) % 4]
        users = _list(rng, 136, 70)
        want = _want(seen[n], users, S, n)
        one = _device(seen[n], users, U, V, n, splits=1)
        assert _eq(one, want)
        for sp in SPLITS:
            assert K.topk_scores_for_workspace(70, 261, n, sp)[0] == min(sp, 5)
            got = _device(seen[n], users, U, V, n, splits=sp)
            assert _ident(got, one), (name, k, n, sp)
    # one tile: splits = 5 is clamped to 1
    U, V, S, seen = cases['_grid', 5]
    assert K.topk_scores_for_workspace(9, 64, 33, 5) == (1, 0)
    users = _list(rng, 136, 9)
    assert _eq(_device(None, users, U, V[:64], 33, splits=5), _want(None, users, S[:, :64], 33))


def test_more_tiles_than_s_max(lim):
    from csr_amd.kernels import hip as K
    s_max, tile = lim[1][0], lim[0][3]
    rng = np.random.default_rng(4)
    ni = tile * (s_max + 1)
    U, V = _grid((3, 5), rng), _grid((ni, 5), rng)
    S = R.scores_plain(U, V)
    csr = _seen(S, 33, 4)
    want = _want(csr, [2, 0, 1], S, 33)
    assert K.topk_scores_for_workspace(3, ni, 33, s_max + 1)[0] == s_max and K.topk_scores_for_workspace(3, ni, 33)[0] == s_max
    for sp in (s_max, 0):          # S_max ranges: the first holds two tiles, the others one each
        assert _eq(_device(csr, [2, 0, 1], U, V, 33, splits=sp), want), sp
    assert _eq(_host(csr, [2, 0, 1], U, V, 128), _want(csr, [2, 0, 1], S, 128))


# ---- 4. split edge cases ----------------------------------------------------------------------------------------------------------

def test_winners_in_one_range_ties_and_short_partial_lists(lim):
    tile = lim[0][3]
    m, ni = 66, 4 * tile + 5
    U = (np.arange(m, dtype=np.float64) + 1.0)[:, None]
    up = np.arange(ni, dtype=np.float64)[:, None]
    users = np.array([65, 0, 64, 3, 3, 1])
    for name, V in (('ascending', up), ('descending', -up), ('equal', np.ones((ni, 1)))):          # every winner in the last range / the first / tied
        S = R.scores_plain(U, V)
        for n in NTOPS:
            want = _want(None, users, S, n)
            for sp in (1, 2, 5):
                got = _device(None, users, U, V, n, splits=sp)
                assert _eq(got, want), (name, n, sp)
            if name == 'equal':          # ties go to the smaller item across the range boundaries
                assert np.all(got[0] == np.arange(n)) and np.all(got[2] == n)
            if name == 'ascending':
                assert np.all(got[0][:, 0] == ni - 1) and (n > 5 or np.all(got[0] >= 4 * tile))
    # a range whose items are all seen (partial count 0), and one whose items are all below min_score
    rng = np.random.default_rng(6)
    U, V = _grid((m, 5), rng), _grid((ni, 5), rng)
    S = R.scores_plain(U, V)
    cols = [np.arange(tile, 3 * tile, dtype=np.int32) if r % 2 else np.arange(4 * tile, ni, dtype=np.int32) for r in range(m)]
    csr = _csr(m, ni, cols, ptr64=True)
    Vlow = V.copy()
    Vlow[2 * tile:3 * tile] = 0.0          # scores +-0.0 there: below min_score = 0.5
    Slow = R.scores_plain(U, Vlow)
    for n in (1, 33):
        for sp in (2, 5):
            assert _eq(_device(csr, users, U, V, n, splits=sp), _want(csr, users, S, n)), (n, sp)
            assert _eq(_device(csr, users, U, Vlow, n, 0.5, splits=sp), _want(csr, users, Slow, n, 0.5)), (n, sp)
    # ranges that hold fewer than n candidates each while the row holds more than n in all: 10 unseen items per tile, n = 33
    few = np.concatenate([np.arange(t * tile, min((t + 1) * tile, ni))[10:] for t in range(5)]).astype(np.int32)
    csr = _csr(m, ni, [few] * m)
    want = _want(csr, users, S, 33)
    assert np.all(want[2] == 33)          # (45 candidates in all)
    for sp in (1, 3, 5):
        assert _eq(_device(csr, users, U, V, 33, splits=sp), want), sp
    # n above n_items, and no items at all
    assert _eq(_device(None, users, U, V[:70], 128, splits=2), _want(None, users, S[:, :70], 128))
    for sp in (0, 3):
        got = _device(None, users, U, np.zeros((0, 5)), 2, splits=sp)
        assert np.all(got[0] == -1) and np.all(got[1] == -INF) and np.all(got[2] == 0)
    got = _host(None, users, U, np.zeros((0, 5)), 2, splits=4)
    assert np.all(got[0] == -1) and np.all(got[1] == -INF) and np.all(got[2] == 0)


def test_special_values_by_position_across_ranges(lim):
    tile = lim[0][3]
    rng = np.random.default_rng(10)
    m, ni, ja, jb = 8, 4 * tile + 5, tile + 2, 3 * tile + 7          # two NaN rows of V, in the ranges 1 and 3 of 5
    U, V = _grid((m, 5), rng), _grid((ni, 5), rng)
    cols = [np.array([ja] if r % 2 else [], np.int32) for r in range(m)]
    csr = _csr(m, ni, cols)
    users = np.array([5, 0, 2, 7, 5])
    base = _device(csr, users, U, V, 6, splits=5)
    Vn = V.copy()
    Vn[ja, 3] = Vn[jb, 0] = np.nan
    Sn = R.scores_plain(U, Vn)
    for sp in (1, 2, 5):
        got = _device(csr, users, U, Vn, 6, splits=sp)
        assert _eq(got, _want(csr, users, Sn, 6)), sp
        for x, r in enumerate(users):
            rest = [j for j in base[0][x] if j not in (ja, jb)]
            if r % 2:                                                  # ja is seen: jb's NaN ranks first, then the rest as before
                assert got[0][x, 0] == jb and np.isnan(got[1][x, 0]) and got[0][x, 1:].tolist() == rest[:5]
            else:                                                      # both NaNs tie: the smaller item first
                assert got[0][x, :2].tolist() == [ja, jb] and np.isnan(got[1][x, :2]).all() and got[0][x, 2:].tolist() == rest[:4]
    for bad in (np.nan, INF, -INF):
        Ub = U.copy()
        Ub[2, 1] = bad
        got = _device(csr, users, Ub, V, 6, splits=5)
        assert _eq(got, _want(csr, users, R.scores_plain(Ub, V), 6))
        keep = users != 2
        assert _ident(tuple(a[keep] for a in got), tuple(b[keep] for b in base))
    Vi = V.copy()
    Vi[5, :] = INF                                                     # +-Inf and Inf - Inf in the first range, -Inf in the last
    Vi[ni - 1, :] = -INF
    assert _eq(_device(csr, users, np.abs(U) + 1.0, Vi, 6, splits=5), _want(csr, users, R.scores_plain(np.abs(U) + 1.0, Vi), 6))
    assert _eq(_device(csr, users, U, Vi, 6, splits=5), _want(csr, users, R.scores_plain(U, Vi), 6))
    # -0.0 (an underflow of the chain) ties with +0.0 across a range boundary and keeps its sign
    Uz = np.array([[1e-200], [-1e-200]])
    Vz = np.zeros((2 * tile + 1, 1))
    Vz[[0, tile, 2 * tile], 0] = [-1e-200, 1e-200, -1e-200]
    Vz[1:tile, 0] = Vz[tile + 1:2 * tile, 0] = -3.0
    Sz = R.scores_exact(Uz, Vz)
    assert np.signbit(Sz[:, [0, tile, 2 * tile]]).tolist() == [[True, False, True], [False, True, False]]
    for sp in (1, 3):
        got = _device(None, [1, 0, 1], Uz, Vz, 3, splits=sp)
        assert _eq(got, R.select(Sz[[1, 0, 1]], None, None, 3)), sp
        assert got[0][1].tolist() == [0, tile, 2 * tile] and np.signbit(got[1][1]).tolist() == [True, False, True]
        assert got[0][0, 0] == 1 and got[1][0, 0] == -3.0 * -1e-200          # row 1: -3.0 * -1e-200 wins there


# ---- 5. the device form -------------------------------------------------------------------------------------------------------------

def test_device_form_variants_give_the_same_bits(cases, lim):
    rng = np.random.default_rng(12)
    for name, k, n in (('_f32', 16, 32), ('_grid', 16, 33), ('_f32', 5, 1)):
        U, V, S, seen = cases[name, k]
        csr = seen[n]
        users = _list(rng, 136, 75)
        want = _want(csr, users, S, n)
        for sp in (1, 4):
            for kw in (dict(), dict(pad=3), dict(shift=1), dict(pad=1, shift=1), dict(pad=4), dict(stream=True), dict(repeat=2),
                       dict(at=16), dict(at=GUARD), dict(slack=256), dict(pad=2, shift=3, stream=True, extra=5, at=48)):
                got = _device(csr, users, U, V, n, splits=sp, **kw)
                assert _eq((got[0][:, :n], got[1][:, :n], got[2]), want), (name, k, sp, kw)
                assert np.all(got[0][:, n:] == -77) and np.all(got[1][:, n:] == 77.0)          # columns beyond n_top are not touched
            got = _device(csr, users, U, V, n, splits=sp, counts=False)                     # counts may be NULL
            assert _eq((got[0], got[1], want[2]), want) and np.all(got[2] == -5)


def test_an_index_outside_the_rows_gets_count_minus_one_and_touches_no_neighbour(cases, lim):
    U, V, S, seen = cases['_grid', 5]
    n = 33
    users = np.array([4, 135, 1, 136, 9, -1, 2 ** 31 - 1, 9, -2 ** 31, 0])
    bad = (users < 0) | (users >= 136)
    want = _want(seen[n], np.where(bad, 0, users), S, n)
    long_ = np.concatenate([np.arange(60), users, np.arange(70, 130)])          # the bad positions straddle a row block
    want_long = _want(seen[n], np.where((long_ < 0) | (long_ >= 136), 0, long_), S, n)
    for sp in (1, 3, 0):
        for us, wt in ((users, want), (long_, want_long)):
            b = (us < 0) | (us >= 136)
            got = _device(seen[n], us, U, V, n, splits=sp)
            assert np.all(got[2][b] == -1) and np.all(got[0][b] == -1) and np.all(got[1][b] == -INF), sp
            assert _eq(tuple(g[~b] for g in got), tuple(w[~b] for w in wt)), sp
    # without a handle u_rows alone bounds the list: rows at or beyond it are not read
    got = _device(None, [3, 100, 99], U, V, n, splits=2, u_rows=100)
    assert got[2].tolist() == [n, -1, n] and _eq(tuple(g[[0, 2]] for g in got), _want(None, [3, 99], S, n))


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing(lim):
    import torch
    from csr_amd._lib import lib, ERR_INVALID, ERR_UNSUPPORTED, VAL_F64
    from csr_amd.kernels import hip as K
    tlim = lim[0]
    m, ni, k, n, nl = 5, 130, 3, 4, 6
    rng = np.random.default_rng(14)
    U, V = _grid((m, k), rng), _grid((ni, k), rng)
    users = np.array([4, 0, 0, 2, 1, 3], np.int32)
    tU, tV, tR = torch.from_numpy(U).cuda(), torch.from_numpy(V).cuda(), torch.from_numpy(users).cuda()
    good_csr = _csr(m, ni, [np.array([1, 4], np.int32)] * m)
    bad_csr = _csr(m, ni, [np.array([1, 4], np.int32), np.array([2, 7], np.int32), np.array([4, 4], np.int32), np.array([5, 2], np.int32),
                           np.zeros(0, np.int32)])
    other = _csr(m, ni + 1, [np.zeros(0, np.int32)] * m)
    taller = _csr(m + 1, ni, [np.zeros(0, np.int32)] * (m + 1))
    hg, hb, ho, ht = (K.to_handle(c) for c in (good_csr, bad_csr, other, taller))
    used, need = K.topk_scores_for_workspace(nl, ni, n, 2)
    assert used == 2 and need == nl * 2 * (16 + 3 * 12)
    work = torch.full((need + 64,), 0x5a, dtype=torch.uint8, device='cuda')
    nan = float('nan')
    P = 'topk_scores_for: '
    try:
        for form in ('host', 'device'):
            if form == 'host':
                items, scores, counts = np.full((nl, n), 7, np.int32), np.full((nl, n), 7.0), np.full(nl, 7, np.int32)
                p = dict(rows=users.ctypes.data, u=U.ctypes.data, v=V.ctypes.data, it=items.ctypes.data, sc=scores.ctypes.data,
                         cn=counts.ctypes.data)
            else:
                items = torch.full((nl, n), 7, dtype=torch.int32, device='cuda')
                scores = torch.full((nl, n), 7.0, dtype=torch.float64, device='cuda')
                counts = torch.full((nl,), 7, dtype=torch.int32, device='cuda')
                p = dict(rows=tR.data_ptr(), u=tU.data_ptr(), v=tV.data_ptr(), it=items.data_ptr(), sc=scores.data_ptr(), cn=counts.data_ptr())

            def call(**ch):
                a = dict(dict(h=hg.H, nr=nl, ur=m, ldu=k, ldv=k, ni=ni, k=k, pt=VAL_F64, nt=n, ms=-INF, ldi=n, lds=n, sp=2,
                              wk=work.data_ptr(), wb=need, **p), **ch)
                args = (a['h'], a['rows'], a['nr'], a['ur'], a['u'], a['ldu'], a['v'], a['ldv'], a['ni'], a['k'], a['pt'], a['nt'], a['ms'],
                        a['it'], a['ldi'], a['sc'], a['lds'], a['cn'], a['sp'])
                return lib.csrk_topk_scores_for(*args) if form == 'host' else lib.csrk_topk_scores_for_device(*args, a['wk'], a['wb'], None)
            refused = [
                (dict(k=0), ERR_INVALID, 'k must be at least 1 (k=0)'),
                (dict(nt=0), ERR_INVALID, 'n_top must be at least 1 (n_top=0)'),
                (dict(h=0, ni=-1), ERR_INVALID, 'n_items must not be negative (n_items=-1)'),
                (dict(ldu=k - 1), ERR_INVALID, f'bad panel geometry k={k} ldu={k - 1} ldv={k}'),
                (dict(ldv=k - 1), ERR_INVALID, f'bad panel geometry k={k} ldu={k} ldv={k - 1}'),
                (dict(ldi=n - 1), ERR_INVALID, f'bad output geometry n_top={n} ldi={n - 1} lds={n}'),
                (dict(lds=n - 1), ERR_INVALID, f'bad output geometry n_top={n} ldi={n} lds={n - 1}'),
                (dict(pt=9), ERR_INVALID, 'panel_type must be CSRK_VAL_F32 or CSRK_VAL_F64, not 9'),
                (dict(ms=nan), ERR_INVALID, 'min_score is NaN'),
                (dict(nr=-1), ERR_INVALID, 'n_rows must not be negative (n_rows=-1)'),
                (dict(ur=-1), ERR_INVALID, 'u_rows must not be negative (u_rows=-1)'),
                (dict(sp=-1), ERR_INVALID, 'splits must not be negative (splits=-1)'),
                (dict(h=ht.H), ERR_INVALID, f'u_rows={m} but seen has {m + 1} rows'),
                (dict(ur=m + 1), ERR_INVALID, f'u_rows={m + 1} but seen has {m} rows'),
                (dict(h=ho.H), ERR_INVALID, f'n_items={ni} but seen has {ni + 1} columns'),
                (dict(h=hb.H), ERR_INVALID, 'seen is not canonical: row 2 is not strictly ascending in column (csrk_order_columns sorts, '
                                            'csrk_coalesce merges repeats)'),
                (dict(k=tlim[0] + 1, ldu=tlim[0] + 1, ldv=tlim[0] + 1), ERR_UNSUPPORTED,
                 f'k={tlim[0] + 1} is above the largest supported k={tlim[0]} (csrk_topk_scores_limits)'),
                (dict(nt=tlim[1] + 1, ldi=tlim[1] + 1, lds=tlim[1] + 1), ERR_UNSUPPORTED,
                 f'n_top={tlim[1] + 1} is above the largest supported n_top={tlim[1]} (csrk_topk_scores_limits)'),
                (dict(nr=64 * 2 ** 31), ERR_UNSUPPORTED, f'n_rows={64 * 2 ** 31} makes more row blocks than a grid holds ({2 ** 31 - 1})'),
                (dict(it=None), ERR_INVALID, 'items or scores is NULL'),
                (dict(sc=None), ERR_INVALID, 'items or scores is NULL'),
                (dict(rows=None), ERR_INVALID, 'rows is NULL'),
                (dict(u=None), ERR_INVALID, 'U is NULL'),
                (dict(v=None), ERR_INVALID, 'V is NULL'),
            ]
            if form == 'device':
                refused += [
                    (dict(wk=None), ERR_INVALID, f'the workspace is NULL but {need} bytes are needed (splits_used=2)'),
                    (dict(wk=work.data_ptr() + 8), ERR_INVALID, 'the workspace is not aligned to 16 bytes'),
                    (dict(wb=need - 1), ERR_INVALID, f'work_bytes={need - 1} but {need} bytes are needed (splits_used=2)'),
                    (dict(wb=0), ERR_INVALID, f'work_bytes=0 but {need} bytes are needed (splits_used=2)'),
                ]
            for ch, code, text in refused:
                assert call(**ch) == code, (form, ch)
                assert lib.csrk_last_error().decode() == P + text, (form, ch)
            assert call(h=12345) == ERR_INVALID and b'invalid csrk handle' in lib.csrk_last_error()
            assert call(nr=0, rows=None, u=None, v=None, it=None, sc=None, cn=None, wk=None, wb=0) == 0          # no rows: nothing launched
            if form == 'host':          # the list is looked at first: position and value
                worse = np.array([4, 0, m, 2, -1, 3], np.int32)
                assert call(rows=worse.ctypes.data) == ERR_INVALID
                assert lib.csrk_last_error().decode() == P + f'rows[2]={m} is outside [0, {m})'
            if form == 'device':
                torch.cuda.synchronize()
                items, scores, counts = items.cpu().numpy(), scores.cpu().numpy(), counts.cpu().numpy()
            assert np.all(items == 7) and np.all(scores == 7.0) and np.all(counts == 7), form
            assert np.all(work.cpu().numpy() == 0x5a), form
        assert K.is_canonical(hg) == (True, None) and K.is_canonical(hb) == (False, 2)
    finally:
        for h in (hg, hb, ho, ht):
            K.release_handle(h)
    # the Python layer: a non-canonical matrix is refused by name, and the limits hold
    with pytest.raises(ValueError, match='row 2'):
        bad_csr.topk_scores_for([0, 1], U, V, n)
    S = R.scores_plain(U, V)
    assert _eq(good_csr.topk_scores_for(users, U, V, n, splits=3), _want(good_csr, users, S, n))
    assert _eq(good_csr.topk_scores_for(users, U, V, n, exclude=False), _want(None, users, S, n))
