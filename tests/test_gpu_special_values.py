"""
NaN, +-Inf, signed zeros and the float32 range through every product kernel, against the oracle (pinned to the reference
on the same kind of inputs by tests/test_oracle_golden.py::test_special_values_golden).

Comparison rules (tests/special_values.py): NaN by position only; +-Inf exactly; zeros by their sign bit; finite values bit
for bit where the library promises it (SpGEMM with B's rows holding no column twice, the dense route for rows of A of at
most 64 entries, one-entry rows, data movement), else within 1e-12 of sum |a x|.  Magnitudes stay far from float64
overflow (products of at most ~1e150), so an output's class depends only on the set of its products.

Locality: a poisoned input may change only the outputs the reference's loop reads it into, and nothing else by a single
bit.  Each form runs one handle (one plan) on a clean input and on poisoned copies; every output that reads no poisoned
element must be the clean run's bits, every one that reads one must have the oracle's class.  Columns 0, the last one and
every multiple of 64 are left unreferenced, so that a padding slot that points at the first column of a window or block
(or the segment kernel's re-read of B row 0) is caught.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import Mat, as_library_orders
from special_values import close, kind, raw_bits_equal, same_bits, same_class

pytestmark = pytest.mark.gpu

ALGOS = ['merge', 'vector', 'scalar']
PLAN_SETTINGS = ['auto', 'forced_split', 'hot', 'forced_split_hot', 'forced_split_nostream']


@pytest.fixture(params=PLAN_SETTINGS)
def plan_setting(request, monkeypatch):
    """
    tests/test_gpu_spmv.py's five plan settings: the library's own choice; split forced; hot-column pack forced; both
    (the light stream with cold staging: a plan stages whenever it has the stream and the pack, CSRK_LS_STAGE=0 turns that
    off); split without the light stream.  Every to_handle copies (no cached handle carries a plan from one setting into
    the next).
    """
    for k in ('CSRK_SPMV_HEAVY_SPLIT', 'CSRK_SPMV_STREAM', 'CSRK_SPMV_HOT', 'CSRK_LS_STAGE'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('CSRK_HANDLE_CACHE', '0')
    p = request.param
    if 'forced_split' in p:
        monkeypatch.setenv('CSRK_SPMV_HEAVY_SPLIT', '1')
    if 'nostream' in p:
        monkeypatch.setenv('CSRK_SPMV_STREAM', '0')
    if 'hot' in p:
        monkeypatch.setenv('CSRK_SPMV_HOT', '1')
    return p


@pytest.fixture(params=['reference', 'ascending'])
def spgemm_order(request):
    from csr_amd.kernels import hip as K
    K.set_spgemm_order(request.param)
    yield request.param
    K.set_spgemm_order(None)


def _csr(nr, nc, rp, ci, vs):
    from csr_amd import CSR
    return CSR(nr, nc, int(rp[-1]), rp, ci, vs, _cast=False)


def _ov(m):
    "oracle tuple of a csr_amd.CSR or a golden Mat"
    return m.nrows, m.ncols, m.rowptrs, m.colinds, m.values


def _mv_ref(m, x):
    from oracle import oracle as O
    with np.errstate(all='ignore'):
        return O.mult_vec(m.nrows, m.ncols, m.rowptrs, m.colinds, m.values, x)


def _mv_bound(m, x):
    from oracle import oracle as O
    vs = None if m.values is None else np.abs(m.values.astype(np.float64))
    with np.errstate(all='ignore'):
        return O.mult_vec(m.nrows, m.ncols, m.rowptrs, m.colinds, vs, np.abs(np.asarray(x, dtype=np.float64)))


def _one_entry_rows(rp):
    return np.flatnonzero(np.diff(rp) == 1)


# ---- SpMV entries -------------------------------------------------------------------------------------------------

def _spmv(h, x, entry):
    """
    y = A x through one entry: 'host' (csrk_spmv / csrk_spmv_f32x by x's dtype), 'device', 'part' (part 1 then part 2),
    'f32x_device'; device outputs land in a NaN-filled buffer (so a row an entry forgets to write shows).
    """
    import torch
    from csr_amd._lib import lib, check
    from csr_amd.kernels import hip as K
    if entry == 'host':
        return K.mult_vec(h, x)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.full((h.nrows,), float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    H = K._live(h)
    if entry == 'device':
        check(lib.csrk_spmv_device(H, xd.data_ptr(), yd.data_ptr(), None))
    elif entry == 'part':
        check(lib.csrk_spmv_device_part(H, xd.data_ptr(), yd.data_ptr(), None, 1))
        check(lib.csrk_spmv_device_part(H, xd.data_ptr(), yd.data_ptr(), None, 2))
    else:
        assert entry == 'f32x_device' and x.dtype == np.float32
        check(lib.csrk_spmv_f32x_device(H, xd.data_ptr(), yd.data_ptr(), None))
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def _entries(algo, x32):
    if x32:
        return ['host', 'f32x_device'] if algo == 'merge' else ['host']
    return ['host', 'device', 'part']


# ---- a. the special-value fixture -----------------------------------------------------------------------------------

@pytest.mark.parametrize('algo', ALGOS)
def test_fixture_spmv(golden, algo, plan_setting):
    "special.npz's mult_vec cases (float64 and float32 x) through every entry: the reference's classes, zeros and one-entry rows bit for bit"
    from csr_amd.kernels import hip as K
    g = golden('special')
    for c in range(int(g['n_mv'])):
        m = Mat(g, f'mv{c}_')
        A = _csr(m.nrows, m.ncols, m.rowptrs, m.colinds, m.values)
        ones = _one_entry_rows(m.rowptrs)
        for xk in ('x64', 'x32'):
            x = g[f'mv{c}_{xk}']
            want = g[f'mv{c}_y' + xk[1:]]
            if m.values is not None and m.values.dtype == np.float32 and xk == 'x32' and algo != 'merge':
                entries = ['host']
            else:
                entries = _entries(algo, xk == 'x32')
            h = K.to_handle(A)
            try:
                K.set_spmv_algo(h, algo)
                for rep in range(2):                    # the first, plan-less product and a planned one
                    for e in entries:
                        y = _spmv(h, x, e)
                        what = f'case {c} {xk} {e} call {rep}'
                        close(y, want, _mv_bound(m, x), what)
                        same_bits(y[ones], want[ones], what + ' (one-entry rows)')
            finally:
                K.release_handle(h)


def _check_raw(ch, want, rp, what, exact=True, bound=None):
    "a product handle against the reference's raw arrays (rowptrs, colinds in the order in force, values)"
    from csr_amd.kernels import hip as K
    got = K.from_handle(ch)
    ci, vs = as_library_orders(rp, want.colinds, want.values)
    assert np.array_equal(got.rowptrs, want.rowptrs), what
    assert np.array_equal(got.colinds, ci), what
    if exact:
        same_bits(got.values, vs, what)
    else:
        close(got.values, vs, bound, what)
    return got


def test_fixture_products(golden, spgemm_order):
    """
    special.npz's mult_ab / mult_abt (general route: B's rows hold no column twice, so bit for bit), CSR.multiply (zeros
    filtered: NaN kept) and mult_ab with a fully populated B (the dense route; rows of A of at most 64 entries: bit for bit)
    """
    from csr_amd.kernels import hip as K
    from oracle import oracle as O
    g = golden('special')
    for c in range(int(g['n_mm'])):
        A, B, Bt = (Mat(g, f'mm{c}_{p}_') for p in ('a', 'b', 'bt'))
        Ac, Bc, Btc = (_csr(*_ov(m)) for m in (A, B, Bt))
        raw, rawt = Mat(g, f'mm{c}_raw_'), Mat(g, f'mm{c}_rawt_')
        ah, bh, bth = K.to_handle(Ac), K.to_handle(Bc), K.to_handle(Btc)
        try:
            ch = K.mult_ab(ah, bh)
            assert K.spgemm_last_route() == 'general'
            _check_raw(ch, raw, raw.rowptrs, f'mult_ab case {c}')
            K.release_handle(ch)
            ch = K.mult_abt(ah, bth)
            _check_raw(ch, rawt, rawt.rowptrs, f'mult_abt case {c}')
            K.release_handle(ch)
        finally:
            for h in (ah, bh, bth):
                K.release_handle(h)
        P = Ac.multiply(Bc)
        ab = Mat(g, f'mm{c}_ab_')
        ci, vs = as_library_orders(ab.rowptrs, ab.colinds, ab.values)
        assert np.array_equal(P.rowptrs, ab.rowptrs) and np.array_equal(P.colinds, ci), c
        same_bits(P.values, vs, f'multiply case {c}')
    for c in range(int(g['n_dn'])):
        a, B, raw = Mat(g, f'dn{c}_a_'), g[f'dn{c}_B'], Mat(g, f'dn{c}_raw_')
        k = B.shape[1]
        assert np.diff(a.rowptrs).max() <= 64
        Bc = _csr(a.ncols, k, np.arange(a.ncols + 1, dtype=np.int32) * k, np.tile(np.arange(k, dtype=np.int32), a.ncols),
                  B.reshape(-1).copy())
        ah, bh = K.to_handle(_csr(*_ov(a))), K.to_handle(Bc)
        try:
            ch = K.mult_ab(ah, bh)
            assert K.spgemm_last_route() == 'dense-panel', c
            _check_raw(ch, raw, raw.rowptrs, f'dense-route case {c}')
            K.release_handle(ch)
        finally:
            K.release_handle(ah)
            K.release_handle(bh)
        ah = K.to_handle(_csr(*_ov(a)))
        try:
            Cm = K.mult_dense(ah, B)
        finally:
            K.release_handle(ah)
        v64 = np.ones(a.nnz) if a.values is None else a.values.astype(np.float64)
        with np.errstate(all='ignore'):
            want = O.spmm_dense(a.nrows, a.rowptrs, a.colinds, v64, B)
        same_bits(Cm, want, f'mult_dense case {c}')


def test_fixture_data_movement(golden):
    "transpose, order_columns, pick_rows, filter_zeros and from_coo keep every bit: NaN payloads and -0.0 included"
    from csr_amd.kernels import hip as K
    g = golden('special')
    for c in range(int(g['n_dm'])):
        m = Mat(g, f'dm{c}_')
        h = K.from_coo(g[f'dm{c}_coo_rows'], g[f'dm{c}_coo_cols'], g[f'dm{c}_coo_vals'], (m.nrows, m.ncols))
        try:
            got = K.from_handle(h)
            assert np.array_equal(got.rowptrs, m.rowptrs) and np.array_equal(got.colinds, m.colinds)
            assert raw_bits_equal(got.values, m.values), c
            for name, fn in (('t', lambda: K.transpose(h)), ('pick', lambda: K.pick_rows(h, g[f'dm{c}_pick_rows'])),
                             ('fz', lambda: K.filter_zeros(h))):
                want = Mat(g, f'dm{c}_{name}_')
                oh = fn()
                o = K.from_handle(oh)
                K.release_handle(oh)
                assert np.array_equal(o.rowptrs, want.rowptrs) and np.array_equal(o.colinds, want.colinds), (c, name)
                assert raw_bits_equal(o.values, want.values), (c, name)
            K.order_columns(h)
            o, want = K.from_handle(h), Mat(g, f'dm{c}_sorted_')
            assert np.array_equal(o.colinds, want.colinds) and raw_bits_equal(o.values, want.values), c
        finally:
            K.release_handle(h)


def test_transpose_three_pass_keeps_nan_payloads():
    "the 3-pass transpose (ncols > 65536) moves NaNs with distinct payloads and -0.0 bit for bit"
    from csr_amd.kernels import hip as K
    from oracle import oracle as O
    rng = np.random.default_rng(65537)
    nrows, ncols = 3000, 200000
    lens = rng.integers(0, 60, nrows)
    rp = np.zeros(nrows + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    ci = rng.integers(0, ncols, int(rp[-1])).astype(np.int32)
    vs = rng.uniform(-1, 1, int(rp[-1]))
    q = rng.random(len(vs))
    bits = np.uint64(0x7ff8000000000000) | rng.integers(1, 1 << 40, size=len(vs)).astype(np.uint64)
    bits[q < 0.1] |= np.uint64(1 << 63)
    vs[q < 0.3] = bits[q < 0.3].view(np.float64)
    vs[(q >= 0.3) & (q < 0.4)] = -0.0
    A = _csr(nrows, ncols, rp, ci, vs)
    h = K.to_handle(A)
    try:
        th = K.transpose(h)
        t = K.from_handle(th)
        K.release_handle(th)
    finally:
        K.release_handle(h)
    _, _, brp, bci, bvs = O.transpose(nrows, ncols, rp, ci, vs)
    assert np.array_equal(t.rowptrs, brp) and np.array_equal(t.colinds, bci) and raw_bits_equal(t.values, bvs)


# ---- b. locality: SpMV on small matrices ----------------------------------------------------------------------------

def _is_edge(c, ncols):
    return (c == 0) | (c == ncols - 1) | (c % 64 == 0)


def _spmv_matrix(seed, dtype=np.float64):
    """
    6000 rows x 20000 columns with rows for every class: short rows (merge tiles and their carries / the light stream),
    tier-0 (5000, 2100 entries) and tier-1 (300, 400) rows, a 3-entry first and last row; ascending columns (so the split
    can cut the long rows).  Columns 0, ncols - 1, every multiple of 64 and a spare band are never referenced; `single`
    columns are each referenced by exactly one entry of one of the `probe` rows.
    """
    rng = np.random.default_rng(seed)
    nrows, ncols = 6000, 20000
    lens = rng.integers(0, 12, nrows)
    lens[[0, -1]] = 3
    lens[100], lens[3000] = 5000, 2100
    lens[200], lens[201] = 300, 400
    cols = np.arange(ncols)
    spare = cols[(cols >= 7000) & (cols < 7300)]                 # unreferenced, away from the edges
    single_pool = cols[(cols >= 9000) & (cols < 9600) & ~_is_edge(cols, ncols)]
    drawn = cols[~_is_edge(cols, ncols) & ~np.isin(cols, spare) & ~np.isin(cols, single_pool)]
    probe = np.array([0, 100, 200, 201, 3000, nrows - 1] + list(range(37, nrows - 1, 131)))
    probe = probe[lens[probe] >= 2]
    rp = np.zeros(nrows + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    ci = np.empty(int(rp[-1]), np.int32)
    pool = iter(rng.permutation(single_pool))
    singles = {}
    for i in range(nrows):
        c = rng.choice(drawn, size=int(lens[i]), replace=False)
        if i in set(probe.tolist()):
            s = [next(pool), next(pool)]
            c[:2] = s
            singles[i] = s
        ci[rp[i]:rp[i + 1]] = np.sort(c)
    vs = rng.uniform(-1, 1, int(rp[-1])).astype(dtype)
    unref = np.setdiff1d(cols, ci)
    assert np.all(np.isin([0, ncols - 1, 64, 128, 19968], unref))
    return _csr(nrows, ncols, rp, ci, vs), unref, singles


def _rows_reading(A, cols_mask=None, entry_mask=None):
    "rows with at least one entry at a masked column or at a masked entry"
    hit = np.zeros(A.nnz, bool)
    if cols_mask is not None:
        hit |= cols_mask[A.colinds]
    if entry_mask is not None:
        hit |= entry_mask
    rows = np.repeat(np.arange(A.nrows), np.diff(A.rowptrs))
    out = np.zeros(A.nrows, bool)
    out[rows[hit]] = True
    return out


def _local(y, clean, want, touched, what):
    "untouched outputs: the clean run's bits; touched ones: the oracle's class"
    same_bits(y[~touched], clean[~touched], what + ' (outputs that read no poisoned input)')
    same_class(y[touched], want[touched], what + ' (outputs that read one)')


@pytest.mark.parametrize('algo', ALGOS)
def test_spmv_locality(algo, plan_setting):
    """
    Poison sets on one plan per entry: (1) x at every unreferenced column -> y unchanged bit for bit; (2) x at columns read
    by exactly one entry (NaN, +Inf, -Inf; a +Inf and a -Inf in the same row) and single values of A in every row class ->
    only their rows change, to the oracle's class; (3) explicit +0.0 / -0.0 values at entries whose x is +-Inf or NaN ->
    NaN (no path skips an explicit zero).
    """
    import ctypes as C
    from csr_amd._lib import lib, check
    from csr_amd.kernels import hip as K
    A, unref, singles = _spmv_matrix(4242)
    rng = np.random.default_rng(7)
    x = rng.uniform(-1, 1, A.ncols)
    x1 = x.copy()
    x1[unref] = np.where(np.arange(len(unref)) % 3 == 0, np.nan, np.where(np.arange(len(unref)) % 3 == 1, np.inf, -np.inf))
    x2 = x.copy()
    poison_cols = np.zeros(A.ncols, bool)
    zero_entries = np.zeros(A.nnz, bool)
    val_entries = np.zeros(A.nnz, bool)
    v3 = A.values.copy()
    for n, (i, (s0, s1)) in enumerate(sorted(singles.items())):
        if n % 4 == 0:                               # +Inf and -Inf into one row
            x2[s0], x2[s1] = np.inf, -np.inf
        elif n % 4 == 1:
            x2[s0] = np.nan
        elif n % 4 == 2:                             # an explicit zero at the poisoned column: NaN
            x2[s0] = (np.inf, -np.inf, np.nan)[n % 3]
            e = A.rowptrs[i] + int(np.flatnonzero(A.colinds[A.rowptrs[i]:A.rowptrs[i + 1]] == s0)[0])
            v3[e] = -0.0 if n % 8 == 2 else 0.0
            zero_entries[e] = True
        else:                                        # one value of A (not at a single column)
            e = A.rowptrs[i + 1] - 1
            if A.colinds[e] in (s0, s1):
                e = A.rowptrs[i] + 2 if A.rowptrs[i + 1] - A.rowptrs[i] > 2 else None
            if e is not None and A.colinds[e] not in (s0, s1):
                v3[e] = (np.nan, np.inf, -np.inf)[n % 3]
                val_entries[e] = True
        poison_cols[[s0, s1]] = x2[[s0, s1]] != x[[s0, s1]]
    A3 = _csr(A.nrows, A.ncols, A.rowptrs, A.colinds, v3)
    t2 = _rows_reading(A, cols_mask=poison_cols)
    t3 = _rows_reading(A, cols_mask=poison_cols, entry_mask=zero_entries | val_entries)
    tv = _rows_reading(A, entry_mask=zero_entries | val_entries)
    assert t2.sum() >= 20 and tv.sum() >= 5 and zero_entries.sum() >= 5
    for x32 in (False, True):
        xs = [v.astype(np.float32) if x32 else v for v in (x, x1, x2)]
        want = [_mv_ref(A, v) for v in xs] + [_mv_ref(A3, xs[0]), _mv_ref(A3, xs[2])]
        for e in _entries(algo, x32):
            h, h3 = K.to_handle(A), K.to_handle(A3)
            try:
                K.set_spmv_algo(h, algo)
                K.set_spmv_algo(h3, algo)
                first = _spmv(h, xs[0], e)                                  # plan-less
                _spmv(h3, xs[0], e)
                clean = _spmv(h, xs[0], e)                                  # planned
                what = f'{algo} {plan_setting} {e} x32={x32}'
                close(first, want[0], _mv_bound(A, xs[0]), what + ' first call')
                close(clean, want[0], _mv_bound(A, xs[0]), what)
                same_bits(_spmv(h, xs[1], e), clean, what + ' set 1')
                _local(_spmv(h, xs[2], e), clean, want[2], t2, what + ' set 2 (x)')
                _local(_spmv(h3, xs[0], e), clean, want[3], tv, what + ' set 2 (values)')
                y = _spmv(h3, xs[2], e)
                _local(y, clean, want[4], t3, what + ' sets 2 + 3')
                assert np.all(np.isnan(y[_rows_reading(A, entry_mask=zero_entries)])), what
                if plan_setting == 'forced_split_hot' and algo == 'merge':      # tiers, pack, light stream, staging
                    st = (C.c_int64 * 34)()
                    check(lib.csrk_spmv_plan_stats(K._live(h), st, 34))
                    assert st[2] > 0 and st[16] > 0 and st[20] == 1 and st[24] > 0, list(st)
            finally:
                K.release_handle(h)
                K.release_handle(h3)


def test_spmv_locality_at_size(monkeypatch):
    """
    The 3M x 3M, 6e7-entry powerlaw matrix (tiers, hot-column pack, light stream, cold staging with the 3-byte index all
    present, as in tests/test_gpu_fullsize.py): x poisoned at every unreferenced column leaves y's bits alone; x poisoned
    at columns read once, chosen in rows of every length class, changes exactly those rows (to NaN / +-Inf as the oracle's
    loop gives); both through csrk_spmv_device and the two-part form.
    """
    import torch
    from csr_amd import synth
    from csr_amd._lib import lib, check, handle_t
    monkeypatch.setenv('CSRK_LS_STAGE', '1')
    dev = 'cuda'
    n, nnz = 3_000_000, 60_000_000
    m = synth.powerlaw_csr(n, n, nnz, device=dev)
    x = synth.dense_vector(n, device=dev, stream=3)
    rp, ci, vs = m['rowptrs'], m['colinds'], m['values']
    counts = torch.bincount(ci.long(), minlength=n)
    unref = torch.nonzero(counts == 0).flatten()
    once = torch.nonzero(counts == 1).flatten()
    assert unref.numel() > 100 and once.numel() > 1000
    # the one row that reads each once-column, and that row's length
    ent = torch.nonzero(counts[ci.long()] == 1).flatten()
    rows = torch.searchsorted(rp.long(), ent, right=True) - 1
    lens = (rp[1:] - rp[:-1]).long()[rows]
    g = torch.Generator(device='cpu').manual_seed(5)
    pick = []
    for lo, hi in ((1, 16), (16, 256), (256, 2048), (2048, 1 << 40)):
        cand = torch.nonzero((lens >= lo) & (lens < hi)).flatten().cpu()
        if cand.numel():
            pick.append(cand[torch.randperm(cand.numel(), generator=g)[:60]])
    pick = torch.cat(pick).to(dev)
    pcols, prows = ci.long()[ent[pick]], rows[pick]
    assert len(pick) >= 120
    h = handle_t(0)
    check(lib.csrk_create_device(n, n, nnz, rp.data_ptr(), 0, ci.data_ptr(), vs.data_ptr(), 2, C.byref(h)))
    try:
        def run(xv, part):
            y = torch.full((n,), float('nan'), dtype=torch.float64, device=dev)
            if part:
                check(lib.csrk_spmv_device_part(h, xv.data_ptr(), y.data_ptr(), None, 1))
                check(lib.csrk_spmv_device_part(h, xv.data_ptr(), y.data_ptr(), None, 2))
            else:
                check(lib.csrk_spmv_device(h, xv.data_ptr(), y.data_ptr(), None))
            torch.cuda.synchronize()
            return y
        run(x, False)
        clean = run(x, False)
        st = (C.c_int64 * 34)()
        check(lib.csrk_spmv_plan_stats(h, st, 34))
        assert st[2] > 0 and st[16] > 0 and st[20] == 1 and st[24] > 0, list(st)     # tiers, pack, light stream, staging
        assert not torch.isnan(clean).any()
        x1 = x.clone()
        x1[unref] = float('nan')
        x2 = x.clone()
        sel = torch.arange(len(pcols), device=dev) % 3
        x2[pcols] = torch.where(sel == 0, float('nan'), torch.where(sel == 1, float('inf'), float('-inf'))).double()
        touched = torch.zeros(n, dtype=torch.bool, device=dev)
        touched[prows] = True
        # the oracle's class of a touched row: NaN if it reads a NaN or both infinities, else the sign of value * inf
        sgn = torch.sign(vs[ent[pick]]) * torch.where(sel == 1, 1.0, -1.0).double()
        for part in (False, True):
            assert torch.equal(run(x1, part).view(torch.int64), clean.view(torch.int64)), f'set 1 part={part}'
            y = run(x2, part)
            assert torch.equal(y[~touched].view(torch.int64), clean[~touched].view(torch.int64)), f'set 2 part={part}'
            nanrow = torch.zeros(n, dtype=torch.bool, device=dev)
            nanrow[prows[sel == 0]] = True
            pos = torch.zeros(n, dtype=torch.int8, device=dev)
            neg = torch.zeros(n, dtype=torch.int8, device=dev)
            pos.index_put_((prows[(sel > 0) & (sgn > 0)],), torch.ones(1, dtype=torch.int8, device=dev), accumulate=True)
            neg.index_put_((prows[(sel > 0) & (sgn < 0)],), torch.ones(1, dtype=torch.int8, device=dev), accumulate=True)
            exp_nan = nanrow | ((pos > 0) & (neg > 0))
            assert torch.equal(torch.isnan(y)[touched], exp_nan[touched]), f'set 2 NaN rows part={part}'
            inf_rows = touched & ~exp_nan
            assert torch.equal(torch.isposinf(y)[inf_rows], (pos > 0)[inf_rows]), f'set 2 +Inf rows part={part}'
            assert torch.equal(torch.isneginf(y)[inf_rows], (neg > 0)[inf_rows]), f'set 2 -Inf rows part={part}'
    finally:
        check(lib.csrk_free(h))


# ---- b. locality: dense-panel SpMM -----------------------------------------------------------------------------------

def _spmm_matrix(seed, dtype=np.float64):
    "1500 x 5000, light rows and 300 heavy ones (>= 256 entries), unsorted columns in odd rows; edge columns unreferenced"
    rng = np.random.default_rng(seed)
    nrows, ncols = 1500, 5000
    lens = rng.integers(0, 9, nrows)
    heavy = rng.choice(np.arange(1, nrows - 1), 300, replace=False)
    lens[heavy] = rng.integers(256, 900, 300)
    lens[[0, -1]] = 3
    cols = np.arange(ncols)
    single_pool = cols[(cols >= 2000) & (cols < 2600) & ~_is_edge(cols, ncols)]
    drawn = cols[~_is_edge(cols, ncols) & ~np.isin(cols, single_pool) & ((cols < 3000) | (cols >= 3100))]
    probe = [0, nrows - 1] + list(heavy[:40]) + list(range(11, nrows - 1, 60))
    probe = set(int(i) for i in probe if lens[i] >= 2)
    pool = iter(rng.permutation(single_pool))
    rp = np.zeros(nrows + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    ci = np.empty(int(rp[-1]), np.int32)
    singles = {}
    for i in range(nrows):
        c = rng.choice(drawn, size=int(lens[i]), replace=False)
        if i in probe:
            c[0] = next(pool)
            singles[i] = int(c[0])
        ci[rp[i]:rp[i + 1]] = np.sort(c) if i % 2 == 0 else c
    vs = rng.uniform(-1, 1, int(rp[-1])).astype(dtype)
    return _csr(nrows, ncols, rp, ci, vs), np.setdiff1d(cols, ci), singles


def _spmm_dev(h, B, k, ldb, off, ldc):
    "csrk_spmm_dense_device with B at column `off` of a panel of width ldb and C of width ldc (NaN beyond k)"
    import torch
    from csr_amd._lib import lib, check
    from csr_amd.kernels import hip as K
    dB = torch.from_numpy(np.ascontiguousarray(B)).cuda()
    dC = torch.full((h.nrows, ldc), float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    check(lib.csrk_spmm_dense_device(K._live(h), dB[:, off:].data_ptr(), k, ldb, dC.data_ptr(), ldc, None))
    torch.cuda.synchronize()
    C_ = dC.cpu().numpy()
    assert np.all(np.isnan(C_[:, k:])), 'nothing is written past the panel width'
    return C_[:, :k]


@pytest.mark.parametrize('k', [1, 7, 64, 130])
@pytest.mark.parametrize('form', ['segment', 'registers1', 'registers4'])
def test_spmm_locality(k, form, monkeypatch):
    """
    Segment form (CSRK_SPMM_HEAVY=0) and register-accumulator form (=1, one and four row groups): B's rows at unreferenced
    columns and the panel columns outside [off, off + k) poisoned -> C unchanged; B[j, t] at a column read once -> only
    C[i, t]; single values of A in light and heavy rows -> only their rows; +0.0 / -0.0 values against a non-finite B row
    -> NaN across that row of C.  Through csrk_spmm_dense (host) and csrk_spmm_dense_device with ldb, ldc > k and B at
    column offset 1.
    """
    from csr_amd.kernels import hip as K
    from oracle import oracle as O
    monkeypatch.setenv('CSRK_HANDLE_CACHE', '0')
    monkeypatch.setenv('CSRK_SPMM_HEAVY', '0' if form == 'segment' else '1')
    if form != 'segment':
        monkeypatch.setenv('CSRK_SPMM_HEAVY_GROUPS', form[-1])
    A, unref, singles = _spmm_matrix(100 + k)
    rng = np.random.default_rng(k)
    ldb, off, ldc = k + 3, 1, k + 2
    Bw = rng.uniform(-1, 1, (A.ncols, ldb))
    Bw[:, :off] = np.nan                                 # panel columns outside the window: never read
    Bw[:, off + k:] = np.inf
    B = np.ascontiguousarray(Bw[:, off:off + k])
    ref = O.spmm_dense(A.nrows, A.rowptrs, A.colinds, A.values, B)
    bound = O.spmm_dense(A.nrows, A.rowptrs, A.colinds, np.abs(A.values), np.abs(B))
    # set 1: B rows nobody reads
    B1w = Bw.copy()
    B1w[unref, off:off + k] = np.nan
    # set 2: B[j, t] at single columns, one t each
    B2w = Bw.copy()
    touched2 = np.zeros((A.nrows, k), bool)
    items = sorted(singles.items())
    for n, (i, j) in enumerate(items):
        t = (n * 7) % k
        B2w[j, off + t] = (np.nan, np.inf, -np.inf)[n % 3]
        touched2[i, t] = True
    # sets 2 and 3 on the values: one value of A per probed row (NaN / +-Inf), explicit +-0.0 at entries whose B row is
    # +Inf / NaN in every column
    v3 = A.values.copy()
    B3w = Bw.copy()
    touched3 = np.zeros(A.nrows, bool)
    zrows = []
    for n, (i, j) in enumerate(items):
        s, e = A.rowptrs[i], A.rowptrs[i + 1]
        if n % 2:
            p = s + int(np.flatnonzero(A.colinds[s:e] == j)[0])
            v3[p] = 0.0 if n % 4 == 1 else -0.0
            B3w[j, off:off + k] = np.inf if n % 3 else np.nan
            zrows.append(i)
        else:
            p = s + int(np.flatnonzero(A.colinds[s:e] != j)[0])
            v3[p] = (np.nan, np.inf, -np.inf)[n % 3]
        touched3[i] = True
    A3 = _csr(A.nrows, A.ncols, A.rowptrs, A.colinds, v3)
    with np.errstate(all='ignore'):
        want2 = O.spmm_dense(A.nrows, A.rowptrs, A.colinds, A.values, B2w[:, off:off + k])
        want3 = O.spmm_dense(A.nrows, A.rowptrs, A.colinds, v3, B3w[:, off:off + k])
    h, h3 = K.to_handle(A), K.to_handle(A3)
    try:
        clean = K.mult_dense(h, B)
        if form != 'segment' and k > 1:
            from csr_amd._lib import lib, check
            st = (C.c_int64 * 9)()
            check(lib.csrk_spmm_plan_stats(K._live(h), st, 9))
            assert st[0] == 1 and st[2] >= 100, list(st)
        close(clean, ref, bound, f'{form} k={k}')
        for entry in ('host', 'device'):
            def run(hh, Bx):
                if entry == 'host':
                    return K.mult_dense(hh, np.ascontiguousarray(Bx[:, off:off + k]))
                return _spmm_dev(hh, Bx, k, ldb, off, ldc)
            what = f'{form} k={k} {entry}'
            same_bits(run(h, Bw), clean, what + ' clean')
            same_bits(run(h, B1w), clean, what + ' set 1')
            y = run(h, B2w)
            same_bits(y[~touched2], clean[~touched2], what + ' set 2 (untouched)')
            same_class(y[touched2], want2[touched2], what + ' set 2 (touched)')
            y = run(h3, B3w)
            same_bits(y[~touched3], clean[~touched3], what + ' sets 2 + 3 (untouched)')
            same_class(y[touched3], want3[touched3], what + ' sets 2 + 3 (touched)')
            assert np.all(np.isnan(y[zrows])), what
    finally:
        K.release_handle(h)
        K.release_handle(h3)


# ---- b. locality: SpGEMM (general route) and the dense route ----------------------------------------------------------

def _uniq_csr(rng, nrows, ncols, lens, dtype, avoid=()):
    rp = np.zeros(nrows + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    allowed = np.setdiff1d(np.arange(ncols), np.asarray(avoid, dtype=np.int64))
    ci = np.concatenate([np.sort(rng.choice(allowed, size=int(n), replace=False)) for n in lens] +
                        [np.zeros(0, np.int64)]).astype(np.int32)
    return _csr(nrows, ncols, rp, ci, rng.uniform(-1, 1, int(rp[-1])).astype(dtype))


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('paths', ['default', 'two-pass strips', 'fallbacks'])
def test_spgemm_locality(paths, dtype, monkeypatch, spgemm_order):
    """
    mult_ab and mult_abt under test_spgemm_deterministic's path settings: poisoned B entries no product uses, B rows no
    entry of A selects, single values of A and of B (NaN / +-Inf), explicit +-0.0 values of A against non-finite B rows,
    B rows of -0.0 and rows that cancel exactly.  B's rows hold no column twice, so every output is the oracle's bit for
    bit (NaN by position) -- which also pins the untouched outputs to the clean run's bits.
    """
    from csr_amd.kernels import hip as K
    from oracle import oracle as O
    if paths == 'two-pass strips':
        monkeypatch.setenv('CSRK_SPGEMM_FUSED', '0')
    if paths == 'fallbacks':
        monkeypatch.setenv('CSRK_SPGEMM_FUSED', '0')
        monkeypatch.setenv('CSRK_SPGEMM_STRIPS', '0')
        monkeypatch.setenv('CSRK_SPGEMM_ESC', '0')
    rng = np.random.default_rng(31)
    la = rng.integers(0, 10, 1200)
    la[::40] = 300
    lb = rng.integers(1, 12, 900)
    lb[::30] = 200
    unread = np.arange(850, 900)                              # rows of B no entry of A selects
    A = _uniq_csr(rng, 1200, 900, la, dtype, avoid=unread)
    B = _uniq_csr(rng, 900, 6000, lb, dtype)
    # planted: B rows 0 and 800 .. 849 hold -0.0, rows 1 and 2 are equal (A rows pick them with +v and -v: exact
    # cancellation)
    bv = B.values.copy()
    for j in [0] + list(range(800, 850)):
        bv[B.rowptrs[j]:B.rowptrs[j + 1]] = -0.0
    B = _csr(B.nrows, B.ncols, B.rowptrs, B.colinds, bv)
    rows_b = [B.colinds[B.rowptrs[j]:B.rowptrs[j + 1]] for j in range(B.nrows)]
    vals_b = [B.values[B.rowptrs[j]:B.rowptrs[j + 1]] for j in range(B.nrows)]
    rows_b[2], vals_b[2] = rows_b[1].copy(), vals_b[1].copy()
    rp = np.zeros(B.nrows + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows_b])
    B = _csr(B.nrows, B.ncols, rp, np.concatenate(rows_b).astype(np.int32), np.concatenate(vals_b).astype(dtype))
    rows_a = [A.colinds[A.rowptrs[i]:A.rowptrs[i + 1]].copy() for i in range(A.nrows)]
    vals_a = [A.values[A.rowptrs[i]:A.rowptrs[i + 1]].copy() for i in range(A.nrows)]
    for i in range(3, A.nrows, 97):                            # one entry: every product -0.0
        rows_a[i], vals_a[i] = np.array([0], np.int32), np.array([1.5], dtype)
    for i in range(5, A.nrows, 89):                            # exact cancellation
        rows_a[i], vals_a[i] = np.array([1, 2], np.int32), np.array([0.75, -0.75], dtype)
    for i in range(7, A.nrows, 101):                           # a long row whose products are all -0.0
        rows_a[i] = np.arange(800, 830, dtype=np.int32)
        vals_a[i] = rng.uniform(0.5, 2, 30).astype(dtype)
    rp = np.zeros(A.nrows + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows_a])
    A = _csr(A.nrows, A.ncols, rp, np.concatenate(rows_a).astype(np.int32), np.concatenate(vals_a).astype(dtype))
    # poisoned copies
    Bp = B.values.copy()
    for j in unread:                                           # set 1: B rows nobody reads
        Bp[B.rowptrs[j]:B.rowptrs[j + 1]] = np.nan
    sel = rng.choice(np.arange(10, 800), 30, replace=False)   # set 2: single B values
    for n, j in enumerate(sel):
        Bp[B.rowptrs[j] + (n % max(1, B.rowptrs[j + 1] - B.rowptrs[j]))] = (np.nan, np.inf, -np.inf)[n % 3]
    Bp[B.rowptrs[3]:B.rowptrs[4]] = np.inf                    # set 3: B rows 3 (+Inf) and 4 (NaN)
    Bp[B.rowptrs[4]:B.rowptrs[5]] = np.nan
    Ap = A.values.copy()
    ent = rng.choice(A.nnz, 40, replace=False)                # set 2: single values of A
    Ap[ent] = np.array([np.nan, np.inf, -np.inf] * 14)[:40]
    for i in range(11, A.nrows, 113):                          # set 3: explicit zeros against rows 3 (+Inf) / 4 (NaN)
        rows_a_i = np.array([3, 4, 10], np.int32)
        s, e = A.rowptrs[i], A.rowptrs[i + 1]
        if e - s >= 3:
            A.colinds[s:s + 3] = rows_a_i
            Ap[s], Ap[s + 1] = (0.0, -0.0) if i % 2 else (-0.0, 0.0)
    Ap = Ap.astype(dtype)
    Bp = Bp.astype(dtype)
    cases = [(A, B), (A, _csr(B.nrows, B.ncols, B.rowptrs, B.colinds, Bp)),
             (_csr(A.nrows, A.ncols, A.rowptrs, A.colinds, Ap), _csr(B.nrows, B.ncols, B.rowptrs, B.colinds, Bp))]
    for n, (Ax, Bx) in enumerate(cases):
        for abt in (False, True):
            if abt:                                            # A B^T with the B^T the caller holds (values float64)
                _, _, trp, tci, tvs = O.transpose(*_ov(Bx))
                Bh = _csr(Bx.ncols, Bx.nrows, trp, tci, tvs)
                with np.errstate(all='ignore'):
                    _, _, rrp, rci, rvs = O.mult_ab(_ov(Ax), _ov(Bx if Bx.values.dtype == np.float64 else
                                                                _csr(*_ov(Bx)[:4], Bx.values.astype(np.float64))))
            else:
                Bh = Bx
                with np.errstate(all='ignore'):
                    _, _, rrp, rci, rvs = O.mult_ab(_ov(Ax), _ov(Bx))
            ah, bh = K.to_handle(Ax), K.to_handle(Bh)
            try:
                ch = K.mult_abt(ah, bh) if abt else K.mult_ab(ah, bh)
                assert K.spgemm_last_route() == 'general'
                got = K.from_handle(ch)
                K.release_handle(ch)
            finally:
                K.release_handle(ah)
                K.release_handle(bh)
            ci, vs = as_library_orders(rrp, rci, rvs)
            what = f'{paths} {np.dtype(dtype).name} case {n} abt={abt}'
            assert np.array_equal(got.rowptrs, rrp) and np.array_equal(got.colinds, ci), what
            same_bits(got.values, vs, what)
            zero = np.isin(kind(vs), [3, 4])
            assert np.all(kind(vs)[zero] == 3), what + ': the reference sums to +0.0 only'
            assert np.all(kind(got.values)[zero] == 3), what
            if n == 0:
                assert zero.sum() > 100, what


@pytest.mark.parametrize('k', [1, 7, 64])
def test_dense_route_locality(k, spgemm_order):
    """
    mult_ab(A, CSR(B)) with a fully populated B (the dense route, csrk_spgemm_last_route = 1): B rows nobody reads
    poisoned -> unchanged; single B values and single A values -> the oracle's bits (rows of A of at most 64 entries);
    explicit +-0.0 against non-finite B rows -> NaN; products that are all -0.0 -> +0.0.
    """
    from csr_amd.kernels import hip as K
    from oracle import oracle as O
    A, unref, singles = _spmm_matrix(900 + k)
    lens = np.diff(A.rowptrs)
    keep = np.flatnonzero(lens <= 64)                        # rows of at most 64 entries: bit for bit
    rp = np.zeros(len(keep) + 1, np.int32)
    rp[1:] = np.cumsum(lens[keep])
    ci = np.concatenate([A.colinds[A.rowptrs[i]:A.rowptrs[i + 1]] for i in keep]).astype(np.int32)
    vs = np.concatenate([A.values[A.rowptrs[i]:A.rowptrs[i + 1]] for i in keep])
    vs[:: 17] = -np.abs(vs[:: 17])
    A = _csr(len(keep), A.ncols, rp, ci, vs)
    rng = np.random.default_rng(k)
    B = rng.uniform(-1, 1, (A.ncols, k))
    Bs = []
    b1 = B.copy()
    b1[unref] = np.nan
    Bs.append(b1)
    b2 = B.copy()
    cnt = np.bincount(A.colinds, minlength=A.ncols)
    once = np.flatnonzero(cnt == 1)
    for n, j in enumerate(once[:40]):
        b2[j, n % k] = (np.nan, np.inf, -np.inf)[n % 3]
    b2[once[40:60]] = 0.0                                     # whole rows of +0.0: products +-0.0
    Bs.append(b2)
    b3 = B.copy()
    b3[once[60:80]] = np.inf
    Bs.append(b3)
    v3 = A.values.copy()
    for j in once[60:80]:
        v3[np.flatnonzero(A.colinds == j)] = 0.0 if j % 2 else -0.0
    A3 = _csr(A.nrows, A.ncols, A.rowptrs, A.colinds, v3)
    for Ax, Bx in [(A, B), (A, Bs[0]), (A, Bs[1]), (A3, Bs[2])]:
        Bc = _csr(A.ncols, k, np.arange(A.ncols + 1, dtype=np.int32) * k, np.tile(np.arange(k, dtype=np.int32), A.ncols),
                  Bx.reshape(-1).copy())
        with np.errstate(all='ignore'):
            _, _, rrp, rci, rvs = O.mult_ab(_ov(Ax), _ov(Bc))
        ah, bh = K.to_handle(Ax), K.to_handle(Bc)
        try:
            ch = K.mult_ab(ah, bh)
            assert K.spgemm_last_route() == 'dense-panel'
            got = K.from_handle(ch)
            K.release_handle(ch)
        finally:
            K.release_handle(ah)
            K.release_handle(bh)
        ci, vs = as_library_orders(rrp, rci, rvs)
        assert np.array_equal(got.rowptrs, rrp) and np.array_equal(got.colinds, ci)
        same_bits(got.values, vs, f'dense route k={k}')
    assert np.isnan(vs).sum() >= 10


# ---- b. locality: SDDMM ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('pdt', [np.float64, np.float32])
@pytest.mark.parametrize('k', [1, 5, 17, 64, 65, 200])
def test_sddmm_locality(k, pdt):
    """
    U rows of empty rows, V rows of unreferenced columns and the panel columns k .. ld - 1 poisoned -> out unchanged bit
    for bit; U[i, t] -> exactly row i's entries; V[j, t] at a column read once -> exactly that entry; explicit +0.0 / -0.0
    values (scale 1) at entries whose U row or V row holds +-Inf or NaN -> NaN, on a second handle of the same pattern;
    a negative value times a +0.0 dot -> -0.0 (csrk.h); products all -0.0 -> +0.0.  Host entry and the device entry with
    ld > k.
    """
    import torch
    from csr_amd._lib import lib, check, VAL_F32, VAL_F64
    from csr_amd.kernels import hip as K
    A, unref, singles = _spmm_matrix(300 + k)
    lens = np.diff(A.rowptrs)
    # empty some rows (U rows nobody reads)
    empties = np.flatnonzero(lens == 0)
    assert len(empties) > 50
    rng = np.random.default_rng(k)
    U = rng.uniform(-1, 1, (A.nrows, k)).astype(pdt)
    V = rng.uniform(-1, 1, (A.ncols, k)).astype(pdt)
    vals = A.values.copy()
    z_rows = list(singles)[:10]
    U[z_rows] = 0.0                                          # dots of exact +0.0 (and of -0.0 products)
    V[[singles[i] for i in z_rows[:5]]] = -1.0
    vals[A.rowptrs[z_rows[0]]] = -0.5                        # negative value times a +0.0 dot: -0.0 (scale 1)
    A = _csr(A.nrows, A.ncols, A.rowptrs, A.colinds, vals)
    ent_rows = np.repeat(np.arange(A.nrows), lens)

    def ref(U_, V_, scale, vals_=None):
        with np.errstate(all='ignore'):
            d = np.einsum('ij,ij->i', U_[ent_rows].astype(np.float64), V_[A.colinds].astype(np.float64))
            # einsum's zeros come from its own order; a dot whose products are all zero is +0.0 (csrk.h)
            prods_zero = np.all(U_[ent_rows].astype(np.float64) * V_[A.colinds].astype(np.float64) == 0, axis=1)
            d[prods_zero] = 0.0
            return d * (A.values if vals_ is None else vals_) if scale else d

    # set 3: explicit +0.0 / -0.0 values at one entry of rows whose U row holds a non-finite value, and at the one entry
    # that reads a poisoned V row (a single column)
    items = sorted(singles.items())
    vals0 = A.values.copy()
    U3, V3 = U.copy(), V.copy()
    zero_ent = []
    for n, (i, j) in enumerate(items[10:40]):
        bad = (np.inf, -np.inf, np.nan)[n % 3]
        if n % 2:
            U3[i, (3 * n) % k] = bad
            e = int(A.rowptrs[i]) + n % int(lens[i])
        else:
            V3[j, (3 * n) % k] = bad
            e = int(np.flatnonzero(A.colinds == j)[0])
        vals0[e] = 0.0 if n % 4 < 2 else -0.0
        zero_ent.append(e)
    A0 = _csr(A.nrows, A.ncols, A.rowptrs, A.colinds, vals0)
    touched3 = np.isin(ent_rows, [i for n, (i, _) in enumerate(items[10:40]) if n % 2]) | \
        np.isin(A.colinds, [j for n, (_, j) in enumerate(items[10:40]) if n % 2 == 0])

    ld = k + 3
    h, h0 = K.to_handle(A), K.to_handle(A0)
    try:
        def run(U_, V_, scale, entry, hh=None):
            hh = h if hh is None else hh
            if entry == 'host':
                return K.sddmm(hh, U_, V_, scale)
            dU = torch.full((A.nrows, ld), float('nan'), dtype=torch.from_numpy(U_).dtype, device='cuda')
            dV = torch.full((A.ncols, ld), float('inf'), dtype=dU.dtype, device='cuda')
            dU[:, :k] = torch.from_numpy(U_).cuda()
            dV[:, :k] = torch.from_numpy(V_).cuda()
            out = torch.full((A.nnz,), float('nan'), dtype=torch.float64, device='cuda')
            torch.cuda.synchronize()
            check(lib.csrk_sddmm_device(hh.H, dU.data_ptr(), ld, dV.data_ptr(), ld, k, VAL_F64 if pdt == np.float64 else VAL_F32,
                                        int(scale), out.data_ptr(), None))
            torch.cuda.synchronize()
            return out.cpu().numpy()

        for scale in (False, True):
            bound = np.einsum('ij,ij->i', np.abs(U[ent_rows]).astype(np.float64), np.abs(V[A.colinds]).astype(np.float64))
            if scale:
                bound = bound * np.abs(A.values)
            for entry in ('host', 'device'):
                what = f'k={k} {np.dtype(pdt).name} scale={scale} {entry}'
                clean = run(U, V, scale, entry)
                close(clean, ref(U, V, scale), bound, what)
                zero_dots = np.isin(ent_rows, z_rows)
                assert np.all(kind(clean[zero_dots & ((A.values > 0) | (not scale))]) == 3), what + ' +0.0 dots'
                if scale:
                    assert kind(clean[A.rowptrs[z_rows[0]]]) == 4, what + ' negative value x +0.0 dot = -0.0'
                U1, V1 = U.copy(), V.copy()
                U1[empties] = np.nan
                V1[unref] = np.inf
                same_bits(run(U1, V1, scale, entry), clean, what + ' set 1')
                U2, V2 = U.copy(), V.copy()
                touched = np.zeros(A.nnz, bool)
                for n, (i, j) in enumerate(items[10:]):
                    if n % 2:
                        U2[i, n % k] = (np.nan, np.inf, -np.inf)[n % 3]
                        touched |= ent_rows == i
                    else:
                        V2[j, n % k] = (np.nan, np.inf, -np.inf)[n % 3]
                        touched |= A.colinds == j
                y = run(U2, V2, scale, entry)
                same_bits(y[~touched], clean[~touched], what + ' set 2 (untouched)')
                same_class(y[touched], ref(U2, V2, scale)[touched], what + ' set 2 (touched)')
                y = run(U3, V3, scale, entry, h0)
                same_bits(y[~touched3], clean[~touched3], what + ' set 3 (untouched)')
                same_class(y[touched3], ref(U3, V3, scale, vals0)[touched3], what + ' set 3 (touched)')
                if scale:
                    assert np.all(np.isnan(y[zero_ent])), what + ' explicit zero values against non-finite dots'
    finally:
        K.release_handle(h)
        K.release_handle(h0)


# ---- c/d. signed zeros and the float32 range through every SpMV form ---------------------------------------------------

def _zero_and_range_matrix(dtype):
    """
    Rows down to tier-0 length whose products are all -0.0 (negative values against x = +0.0, positive ones against
    -0.0), rows that cancel exactly (+-v against x = 1), one-entry rows whose product is -0.0, overflows float32
    (1e20 * 1e25), is float32-subnormal (1e-20 * 1e-20), is float64-subnormal (1e-160 * 1e-160), or reads a float32
    subnormal value; and ordinary rows in between.
    """
    rng = np.random.default_rng(17)
    ncols = 20000
    zcols_p, zcols_n = np.arange(100, 6100), np.arange(6100, 12100)
    one_cols = np.arange(12100, 12400)
    hugec, tiny32c, tiny64c, unitc = 12500, 12501, 12502, 12503
    rows_c, rows_v, kinds = [], [], []
    for i in range(3000):
        r = i % 12
        if i in (50, 1500):                                  # tier-0 length, all -0.0
            n = 5000
            c = np.sort(rng.choice(np.concatenate([zcols_p, zcols_n]), n, replace=False))
            v = np.where(c < 6100, -1.0, 1.0) * rng.uniform(0.5, 2, n)
            kd = 'zero'
        elif i in (300, 301):                                # tier-1 length, all -0.0
            c = np.sort(rng.choice(zcols_p, 300, replace=False))
            v = -rng.uniform(0.5, 2, 300)
            kd = 'zero'
        elif i in (700, 2200):                               # long cancelling rows
            c = np.sort(rng.choice(one_cols, 200, replace=False))
            v = np.tile([1.25, -1.25], 100)
            kd = 'zero'
        elif r == 1:
            c, v, kd = np.array([zcols_p[i % 6000]]), np.array([-2.0]), 'zero1'
        elif r == 2:
            c = np.sort(rng.choice(zcols_n, 20, replace=False))
            v, kd = rng.uniform(0.5, 2, 20), 'zero'
        elif r == 3:
            c, v, kd = np.sort(rng.choice(one_cols, 4, replace=False)), np.array([3.0, -5.0, 2.0, 0.0]), 'zero'
        elif r == 4:
            c, v, kd = np.array([hugec]), np.array([1e20]), 'one'
        elif r == 5:
            c, v, kd = np.array([tiny32c]), np.array([1e-20 * (1 + i % 7)]), 'one'
        elif r == 6 and dtype == np.float64:
            c, v, kd = np.array([tiny64c]), np.array([1e-160 * (1 + i % 5)]), 'one'
        elif r == 7 and dtype == np.float32:
            c, v, kd = np.array([unitc]), np.array([np.float32(1e-40) * (1 + i % 3)]), 'one'
        else:
            n = int(rng.integers(0, 15))
            c = np.sort(rng.choice(np.arange(12600, ncols), n, replace=False))
            v, kd = rng.uniform(-1, 1, n), 'plain'
        rows_c.append(np.asarray(c, np.int32))
        rows_v.append(np.asarray(v))
        kinds.append(kd)
    rp = np.zeros(len(rows_c) + 1, np.int32)
    rp[1:] = np.cumsum([len(c) for c in rows_c])
    with np.errstate(all='ignore'):
        vs = np.concatenate(rows_v).astype(dtype)
    x = rng.uniform(-1, 1, ncols)
    x[zcols_p], x[zcols_n], x[one_cols] = 0.0, -0.0, 1.0
    x[[hugec, tiny32c, tiny64c, unitc]] = [1e25, 1e-20, 1e-160, 1.0]
    return _csr(len(rows_c), ncols, rp, np.concatenate(rows_c), vs), x, np.array(kinds)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('algo', ALGOS)
def test_spmv_signed_zeros_and_float32_range(algo, dtype, plan_setting):
    """
    Every sum whose products are all -0.0, or cancel exactly, is +0.0 (the reference's accumulator starts at +0.0), in
    one-entry rows and in rows down to tier-0 length; float32 values x float32 x round once (1e20 * 1e25 -> +Inf, 1e-20 *
    1e-20 stays subnormal), float32 values x float64 x do not (1e45, finite); float32 subnormal values widen exactly;
    float64 subnormal products survive.  One-entry rows bit for bit.
    """
    from csr_amd.kernels import hip as K
    A, x, kinds = _zero_and_range_matrix(dtype)
    zero = np.isin(kinds, ['zero', 'zero1'])
    ones = _one_entry_rows(A.rowptrs)
    for x32 in (False, True):
        xv = x.astype(np.float32) if x32 else x
        want = _mv_ref(A, xv)
        assert np.all(kind(want[zero]) == 3)
        if dtype == np.float32 and x32:
            assert np.isposinf(want).sum() > 100 and np.sum((want != 0) & (np.abs(want) < 1.2e-38)) > 100
        entries = _entries(algo, x32) if not (dtype == np.float32 and x32) or algo == 'merge' else ['host']
        h = K.to_handle(A)
        try:
            K.set_spmv_algo(h, algo)
            for rep in range(2):
                for e in entries:
                    y = _spmv(h, xv, e)
                    what = f'{algo} {plan_setting} {np.dtype(dtype).name} x32={x32} {e} call {rep}'
                    same_bits(y[zero], want[zero], what + ' (+0.0 sums)')
                    same_bits(y[ones], want[ones], what + ' (one-entry rows)')
                    close(y, want, _mv_bound(A, xv), what)
        finally:
            K.release_handle(h)


@pytest.mark.parametrize('form', ['segment', 'registers'])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_spmm_signed_zeros_and_float32_range(form, dtype, monkeypatch):
    """
    The dense-panel SpMM on the same rows: -0.0 products and exact cancellations sum to +0.0, float32 values are widened
    exactly (1e20f * 1e25 finite, float32 subnormal values kept), float64 subnormal products survive; one-entry rows bit
    for bit; both forms.
    """
    from csr_amd.kernels import hip as K
    from oracle import oracle as O
    monkeypatch.setenv('CSRK_HANDLE_CACHE', '0')
    monkeypatch.setenv('CSRK_SPMM_HEAVY', '0' if form == 'segment' else '1')
    A, x, kinds = _zero_and_range_matrix(dtype)
    k = 7
    B = x[:, None] * np.array([1.0, 2.0, 0.5, 1.0, 4.0, 1.0, 0.25])[None, :k]
    v64 = A.values.astype(np.float64)
    with np.errstate(all='ignore'):
        want = O.spmm_dense(A.nrows, A.rowptrs, A.colinds, v64, B)
        bound = O.spmm_dense(A.nrows, A.rowptrs, A.colinds, np.abs(v64), np.abs(B))
    zero = np.isin(kinds, ['zero', 'zero1'])
    ones = _one_entry_rows(A.rowptrs)
    assert np.all(kind(want[zero]) == 3) and np.all(np.isfinite(want))
    h = K.to_handle(A)
    try:
        for rep in range(2):
            C_ = K.mult_dense(h, B)
            same_bits(C_[zero], want[zero], f'{form} +0.0 sums')
            same_bits(C_[ones], want[ones], f'{form} one-entry rows')
            close(C_, want, bound, form)
    finally:
        K.release_handle(h)


def test_sddmm_float32_panels_widen_exactly():
    "float32 panel entries in the subnormal range and large ones are widened exactly: products taken in float64"
    from csr_amd.kernels import hip as K
    rp = np.array([0, 1, 2, 3], np.int32)
    ci = np.array([0, 1, 2], np.int32)
    A = _csr(3, 3, rp, ci, np.array([1.0, 1.0, -1.0]))
    U = np.array([[1e-40], [1e20], [0.0]], np.float32)
    V = np.array([[1.0], [1e25], [5.0]], np.float32)
    h = K.to_handle(A)
    try:
        out = K.sddmm(h, U, V, scale=True)
    finally:
        K.release_handle(h)
    want = np.array([float(np.float32(1e-40)), float(np.float32(1e20)) * float(np.float32(1e25)), -0.0])
    same_bits(out, want, 'sddmm f32 panels')


@pytest.mark.parametrize('tail', [1, 7, 300, 2047])
def test_spmv_long_last_row_with_infinite_x(tail):
    """
    A last row spanning several merge tiles (2048 path items each): whole tiles inside the row hand their sums on as
    carries to the tile that holds the row's end.  Its last 8 entries read x = +Inf with positive values: the carries and
    the tail must bring +Inf to that row and nothing but finite sums to its neighbours, in every algorithm and entry.
    """
    from csr_amd.kernels import hip as K
    nrows, ncols = 50, 3 * 4096 + 100
    lens = np.full(nrows, 5)
    lens[-1] = 2 * 4096 + tail
    rp = np.zeros(nrows + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    rng = np.random.default_rng(tail)
    ci = np.concatenate([np.sort(rng.choice(np.arange(1, 100), 5, replace=False)) for _ in range(nrows - 1)] +
                        [np.arange(100, 100 + lens[-1])]).astype(np.int32)
    vs = rng.uniform(0.5, 1.0, int(rp[-1]))
    A = _csr(nrows, ncols, rp, ci, vs)
    x = rng.uniform(-1, 1, ncols)
    x[100 + lens[-1] - 8:100 + lens[-1]] = np.inf
    want = _mv_ref(A, x)
    assert np.isposinf(want[-1]) and np.all(np.isfinite(want[:-1]))
    for algo in ALGOS:
        h = K.to_handle(A)
        try:
            K.set_spmv_algo(h, algo)
            for _ in range(2):
                for e in _entries(algo, False):
                    close(_spmv(h, x, e), want, _mv_bound(A, x), f'{algo} {e}')
        finally:
            K.release_handle(h)
