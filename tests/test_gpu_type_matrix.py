"""
Every entry point through every type it accepts, against the pinned oracle (oracle/oracle.py, held to the reference by
tests/test_oracle_golden.py), at the row lengths where the kernels change class.

Each case is drawn once from a seeded generator and built twice: with int32 and with int64 row pointers.  The int64
handle is checked to really be 64-bit (csrk_info), and its results must equal the int32 twin's bit for bit: the pointer
width changes no order of addition, so any difference is a wrong instantiation.  Row lengths cross the class bounds of
the row kernels (rowops.hip: RS_A = 8, RS_B8 = 64, RS_B = 512, RS_CHUNK = 4096) and the dense-panel SpMM's 64-entry
segment, with a block of empty rows at each end.

The products run every route (general fast / generic form, dense panel, A B^T both ways) under both column orders
('reference', 'ascending', and the environment switch), against the oracle's product in the order in force.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import as_library_orders
from test_gpu_ops import _panel_csr

pytestmark = pytest.mark.gpu

EDGE_LENS = [0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 8193, 3 * 4096 + 17]
PTRS = [False, True]


def _lens(rng, n_short=300, edge=EDGE_LENS):
    "empty rows at both ends, every class boundary, and a spread of short rows (class A) between them"
    return np.concatenate([np.zeros(6, np.int64), edge, rng.integers(0, 12, n_short), np.zeros(6, np.int64)]).astype(np.int64)


def _arrays(seed, lens, ncols=3000, dtype=np.float64, sort_unique=False):
    """
    One draw of a CSR's arrays (rowptrs int64).  Random columns in [0, ncols): the long rows hold columns more than once
    (order_columns' stability).  sort_unique: ascending columns, none twice in a row (products with a bit-exact claim).
    """
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    if sort_unique:
        lens = np.minimum(lens, ncols)
        ci = np.concatenate([np.sort(rng.choice(ncols, int(n), replace=False)) for n in lens] or [np.zeros(0)])
    else:
        ci = rng.integers(0, ncols, size=int(lens.sum()))
    rp = np.zeros(len(lens) + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    vs = None if dtype is None else rng.uniform(-1, 1, size=int(rp[-1])).astype(dtype)
    return len(lens), ncols, rp, ci.astype(np.int32), vs


def _mat(arrs, ptr64, values=True):
    "the CSR of one draw with int32 or int64 row pointers (arrays copied: each twin owns its own)"
    from csr_amd import CSR
    nr, nc, rp, ci, vs = arrs
    vs = None if (vs is None or not values) else vs.copy()
    return CSR(nr, nc, int(rp[-1]), rp.astype(np.int64 if ptr64 else np.int32), ci.copy(), vs, _cast=False)


def _handle(m):
    "K.to_handle(m), with the handle's pointer width checked against m's"
    from csr_amd.kernels import hip as K
    h = K.to_handle(m)
    p64 = K._info(h.H)[3]
    assert p64 == int(m.rowptrs.dtype == np.int64), (p64, m.rowptrs.dtype)
    return h


def _run(m, fn):
    from csr_amd.kernels import hip as K
    h = _handle(m)
    try:
        return fn(h)
    finally:
        K.release_handle(h)


def _export(h):
    from csr_amd.kernels import hip as K
    c = K.from_handle(h)
    K.release_handle(h)
    return c


def _bits(a):
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same_csr(c32, c64):
    "a result of the int32 twin and of the int64 twin: the same entries bit for bit (pointer values compared as numbers)"
    assert (c32.nrows, c32.ncols, c32.nnz) == (c64.nrows, c64.ncols, c64.nnz)
    assert np.array_equal(c32.rowptrs.astype(np.int64), c64.rowptrs.astype(np.int64))
    assert np.array_equal(c32.colinds, c64.colinds)
    assert _same_bits(c32.values, c64.values)


# ---- unit_rows / center_rows ------------------------------------------------------------------------------------

def _row_stat_case(op, dtype):
    arrs = _arrays(11 if op == 'unit' else 12, _lens(np.random.default_rng(10)), dtype=dtype)
    nr, nc, rp, ci, vs = arrs
    z = EDGE_LENS.index(63) + 6
    vs[rp[z]:rp[z + 1]] = 0                                  # an all-zero row: unit -> norm 0, NaN values
    if op == 'unit' and dtype == np.float64:                 # values spread over 350 decades (test_unit_rows_properties_large)
        vs *= np.random.default_rng(13).choice([1e-200, 1.0, 1e150], size=vs.size)
    return arrs


def _check_row_stat(op, dtype, arrs, stats, vals):
    from oracle import oracle as O
    nr, nc, rp, ci, vs = arrs
    ref_v = vs.copy()
    with np.errstate(all='ignore'):
        ref = (O.unit_rows if op == 'unit' else O.center_rows)(nr, rp, ref_v)
    assert stats.dtype == dtype and vals.dtype == dtype
    f32 = dtype == np.float32
    rel = 1e-5 if f32 else 1e-9
    if op == 'unit':
        assert stats == pytest.approx(ref, rel=rel, abs=0, nan_ok=True)
        assert np.array_equal(np.isnan(vals), np.isnan(ref_v))
        assert np.isnan(ref_v).any()
        assert vals == pytest.approx(ref_v, rel=rel, abs=1e-300, nan_ok=True)
    else:
        tol = float(np.max(np.abs(vs))) * (1e-6 if f32 else 1e-12)
        assert stats == pytest.approx(ref, rel=rel, abs=tol)
        assert vals == pytest.approx(ref_v, rel=rel, abs=tol)


def _host_row_stat(op, m):
    from csr_amd.kernels import hip as K

    def go(h):
        with np.errstate(all='ignore'):
            s = (K.unit_rows if op == 'unit' else K.center_rows)(h)
        return s.copy(), K.values_of(h).copy()
    return _run(m, go)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('op', ['unit', 'center'])
def test_row_stats_host_entries(op, dtype):
    "csrk_unit_rows / csrk_center_rows (row_stat<UNIT>, classes A / B8 / B / C1-C3) for int32 and int64 row pointers"
    arrs = _row_stat_case(op, dtype)
    out = {p: _host_row_stat(op, _mat(arrs, p)) for p in PTRS}
    _check_row_stat(op, dtype, arrs, *out[False])
    assert _same_bits(out[False][0], out[True][0]) and _same_bits(out[False][1], out[True][1])


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('op', ['unit', 'center'])
def test_row_stats_device_entries(op, dtype):
    """
    csrk_unit_rows_device / csrk_center_rows_device on a handle that wraps torch tensors (csrk_create_device), the norms /
    means written into a torch buffer at an odd element offset: the same bits as the host entry on a copy, for both
    pointer widths, and nothing written outside the view.
    """
    import torch
    from csr_amd import _lib
    from csr_amd._lib import lib, check
    from csr_amd.kernels import hip as K
    arrs = _row_stat_case(op, dtype)
    nr, nc, rp, ci, vs = arrs
    want_s, want_v = _host_row_stat(op, _mat(arrs, False))
    dev = torch.device('cuda', 0)
    fn = lib.csrk_unit_rows_device if op == 'unit' else lib.csrk_center_rows_device
    vt = _lib.VAL_F32 if dtype == np.float32 else _lib.VAL_F64
    for p64 in PTRS:
        d_rp = torch.from_numpy(rp.astype(np.int64 if p64 else np.int32)).to(dev)
        d_ci = torch.from_numpy(ci.copy()).to(dev)
        d_vs = torch.from_numpy(vs.copy()).to(dev)
        buf = torch.full((nr + 2,), float('nan'), dtype=d_vs.dtype, device=dev)
        out = buf[1:nr + 1]
        torch.cuda.synchronize()
        H = _lib.handle_t(0)
        check(lib.csrk_create_device(nr, nc, int(rp[-1]), d_rp.data_ptr(), int(p64), d_ci.data_ptr(), d_vs.data_ptr(), vt,
                                     C.byref(H)))
        try:
            assert K._info(H.value)[3] == int(p64)
            check(fn(H.value, out.data_ptr()))
            torch.cuda.synchronize()
        finally:
            check(lib.csrk_free(H.value))
        b = buf.cpu().numpy()
        assert np.isnan(b[0]) and np.isnan(b[-1])
        assert _same_bits(b[1:nr + 1].copy(), want_s), p64
        assert _same_bits(d_vs.cpu().numpy(), want_v), p64


@pytest.mark.parametrize('ptr64', PTRS)
def test_row_stats_on_a_structure_only_handle(ptr64):
    "no values: every row-stat entry is an error and the handle's arrays are unchanged"
    import torch
    from csr_amd import _lib
    from csr_amd._lib import lib, ptr
    from csr_amd.kernels import hip as K
    arrs = _arrays(14, _lens(np.random.default_rng(14)), dtype=None)
    m = _mat(arrs, ptr64)
    h = _handle(m)
    try:
        assert K._info(h.H)[4] == _lib.VAL_NONE
        host = np.zeros(m.nrows)
        d_out = torch.zeros(m.nrows + 1, dtype=torch.float64, device='cuda')
        for fn, dst in ((lib.csrk_unit_rows, ptr(host)), (lib.csrk_center_rows, ptr(host)),
                        (lib.csrk_unit_rows_device, d_out.data_ptr()), (lib.csrk_center_rows_device, d_out.data_ptr())):
            assert fn(h.H, dst) == _lib.ERR_INVALID
        for fn in (K.unit_rows, K.center_rows):
            with pytest.raises(ValueError):
                fn(h)
        c = K.from_handle(h)
    finally:
        K.release_handle(h)
    assert np.all(host == 0) and not d_out.any().item()
    assert c.rowptrs.dtype == m.rowptrs.dtype and np.array_equal(c.rowptrs, m.rowptrs)
    assert np.array_equal(c.colinds, m.colinds) and c.values is None


# ---- order_columns ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.float64, np.float32, None])
def test_order_columns(dtype):
    "two stable transposes and a copy back (an f32 cast back): bit-exact with sort_rows, duplicates in their order"
    from oracle import oracle as O
    from csr_amd.kernels import hip as K
    for lens in (_lens(np.random.default_rng(20)), np.zeros(9, np.int64)):       # (and nnz = 0)
        arrs = _arrays(21, lens, ncols=3000, dtype=dtype)
        nr, nc, rp, ci, vs = arrs
        ref_ci, ref_vs = O.sort_rows(nr, rp, ci, vs)
        if rp[-1]:
            assert not np.array_equal(ref_ci, ci)

        def go(h):
            K.order_columns(h)
            return K.from_handle(h)
        out = {p: _run(_mat(arrs, p), go) for p in PTRS}
        c = out[False]
        assert np.array_equal(c.rowptrs, rp) and np.array_equal(c.colinds, ref_ci)
        if dtype is None:
            assert c.values is None
        else:
            assert _same_bits(c.values, ref_vs.astype(dtype))
        assert out[True].rowptrs.dtype == np.int64
        _same_csr(out[False], out[True])


# ---- filter_zeros -----------------------------------------------------------------------------------------------

def test_filter_zeros():
    "-0.0 dropped, NaN kept, rows that become empty; an all-zero matrix (result nnz 0); nnz = 0"
    from oracle import oracle as O
    from csr_amd.kernels import hip as K
    arrs = _arrays(30, _lens(np.random.default_rng(30)))
    nr, nc, rp, ci, vs = arrs
    rng = np.random.default_rng(31)
    vs[rng.uniform(size=vs.size) < 0.3] = 0.0
    vs[rng.choice(vs.size, 40, replace=False)] = -0.0
    vs[rng.choice(vs.size, 40, replace=False)] = np.nan
    for L in (65, 4096):                                     # rows that become empty
        z = EDGE_LENS.index(L) + 6
        vs[rp[z]:rp[z + 1]] = 0.0
    zero = (nr, nc, rp, ci, np.zeros_like(vs))
    empty = _arrays(32, np.zeros(7, np.int64))
    for i, case in enumerate((arrs, zero, empty)):
        n, _, crp, cci, cvs = case
        frp, fci, fvs = O.filter_zeros(n, crp, cci, cvs)
        if i == 0:
            assert np.isnan(fvs).any() and np.all(fvs != 0) and (np.diff(frp)[6:6 + len(EDGE_LENS)] == 0).sum() >= 3
        else:
            assert fci.size == 0
        out = {p: _run(_mat(case, p), lambda h: _export(K.filter_zeros(h))) for p in PTRS}
        for p, f in out.items():
            assert f.rowptrs.dtype == (np.int64 if p else np.int32)
            assert np.array_equal(f.rowptrs, frp) and np.array_equal(f.colinds, fci) and _same_bits(f.values, fvs)
        _same_csr(out[False], out[True])


# ---- pick_rows --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.float64, np.float32, None])
def test_pick_rows(dtype):
    "repeated and unsorted row indices (the longest rows among them), with and without values; an empty selection"
    from oracle import oracle as O
    from csr_amd.kernels import hip as K
    arrs = _arrays(40, _lens(np.random.default_rng(40)), dtype=dtype)
    nr, nc, rp, ci, vs = arrs
    rng = np.random.default_rng(41)
    longest = np.arange(6, 6 + len(EDGE_LENS))
    rows = np.concatenate([rng.permutation(longest), longest[::-1], rng.integers(0, nr, 400), [0, nr - 1, 0]]).astype(np.int32)
    for sel in (rows, np.zeros(0, np.int32)):
        for inc in (True, False):
            prp, pci, pvs = O.pick_rows(rp, ci, vs, sel, inc)
            out = {p: _run(_mat(arrs, p), lambda h: _export(K.pick_rows(h, sel, inc))) for p in PTRS}
            for f in out.values():
                assert f.nrows == len(sel) and f.rowptrs.dtype == np.int32
                assert np.array_equal(f.rowptrs, prp) and np.array_equal(f.colinds, pci)
                if inc and dtype is not None:
                    assert _same_bits(f.values, pvs)
                else:
                    assert f.values is None
            _same_csr(out[False], out[True])


# ---- row_nnzs / row_extent --------------------------------------------------------------------------------------

def test_row_nnzs_and_extent():
    "row_nnzs in the handle's pointer width; row_extent of every row"
    from oracle import oracle as O
    from csr_amd.kernels import hip as K
    arrs = _arrays(50, _lens(np.random.default_rng(50)))
    nr, nc, rp, ci, vs = arrs
    got = {}
    for p in PTRS:
        def go(h):
            return K.row_nnzs(h).copy(), [K.row_extent(h, i) for i in range(nr)]
        got[p] = _run(_mat(arrs, p), go)
        nnzs, ext = got[p]
        assert nnzs.dtype == (np.int64 if p else np.int32) and np.array_equal(nnzs, O.row_nnzs(rp))
        assert ext == [tuple(int(v) for v in O.row_extent(rp, i)) for i in range(nr)]
    assert np.array_equal(got[False][0], got[True][0]) and got[False][1] == got[True][1]


# ---- transpose --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.float64, np.float32, None])
def test_transpose(dtype):
    "rowptrs keep the input width, values become float64 (or none), bit-exact with the reference's counting sort"
    from oracle import oracle as O
    from csr_amd.kernels import hip as K
    arrs = _arrays(60, _lens(np.random.default_rng(60)), ncols=5000, dtype=dtype)
    nr, nc, rp, ci, vs = arrs
    for wv in (True, False):
        _, _, trp, tci, tvs = O.transpose(nr, nc, rp, ci, vs, wv)
        out = {p: _run(_mat(arrs, p), lambda h: _export(K.transpose(h, wv))) for p in PTRS}
        for p, t in out.items():
            assert (t.nrows, t.ncols) == (nc, nr) and t.rowptrs.dtype == (np.int64 if p else np.int32)
            assert np.array_equal(t.rowptrs, trp) and np.array_equal(t.colinds, tci)
            assert _same_bits(t.values, tvs)
        _same_csr(out[False], out[True])


# ---- products: every route x both column orders -----------------------------------------------------------------

@pytest.fixture(params=['reference', 'ascending', 'env-ascending'])
def order(request, monkeypatch):
    "the column order of products for one test: set through the API, or through CSRK_SPGEMM_ORDER (read on every call)"
    from csr_amd.kernels import hip as K
    monkeypatch.delenv('CSRK_SPGEMM_ORDER', raising=False)
    if request.param == 'env-ascending':
        K.set_spgemm_order(None)
        monkeypatch.setenv('CSRK_SPGEMM_ORDER', 'ascending')
    else:
        K.set_spgemm_order(request.param)
    yield 'reference' if request.param == 'reference' else 'ascending'
    K.set_spgemm_order(None)


PRODUCT_LENS = [0, 1, 7, 8, 9, 63, 64, 65, 130, 300, 700]

# name: (route, A B^T, A's values, 64-bit pointers on both, B's panel values (None: a sparse B, A's dtype), panel width k)
ROUTES = {
    'general_fast': ('general', False, np.float64, False, None, 0),
    'general_ptr64': ('general', False, np.float64, True, None, 0),
    'general_f32': ('general', False, np.float32, False, None, 0),
    'dense_f64': ('dense-panel', False, np.float64, False, np.float64, 24),
    'dense_f64_ptr64': ('dense-panel', False, np.float64, True, np.float64, 7),
    'dense_f32': ('dense-panel', False, np.float32, False, np.float64, 7),
    'dense_f32_ptr64': ('dense-panel', False, np.float32, True, np.float64, 24),
    'dense_b_f32': ('dense-panel', False, np.float64, False, np.float32, 24),
    'dense_heavy_rows': ('dense-panel', False, np.float64, False, np.float64, 24),
    'abt_general': ('general', True, np.float64, False, None, 0),
    'abt_dense': ('dense-panel', True, np.float64, False, np.float64, 20),
}


def _product_operands(name):
    _, abt, adt, p64, bdt, k = ROUTES[name]
    rng = np.random.default_rng(70 + list(ROUTES).index(name))
    A = _mat(_arrays(rng.integers(1 << 30), _lens(rng, 250, PRODUCT_LENS), ncols=800, dtype=adt), p64)
    if bdt is None:           # sparse B, no column twice in a row: the sums are the reference's, bit for bit
        b = _arrays(rng.integers(1 << 30), rng.integers(0, 15, 500 if abt else A.ncols), ncols=A.ncols if abt else 900,
                    dtype=np.float32 if adt == np.float32 else np.float64, sort_unique=True)
        B = _mat(b, p64)
    else:
        panel = rng.uniform(-1, 1, (k, A.ncols) if abt else (A.ncols, k)).astype(bdt)
        panel[3, :] = 0.0                                  # explicit zeros in the product, kept
        B = _panel_csr(panel, ptr64=p64)
    return A, B


def _multiply(A, B, abt, spmm_stats=False):
    "C = A B or A B^T, the route it took and (spmm_stats) A's dense-panel plan statistics after it"
    from csr_amd._lib import lib, check
    from csr_amd.kernels import hip as K
    ah, bh = _handle(A), _handle(B)
    st = (C.c_int64 * 9)()
    try:
        ch = K.mult_abt(ah, bh) if abt else K.mult_ab(ah, bh)
        route = K.spgemm_last_route()
        if spmm_stats:
            check(lib.csrk_spmm_plan_stats(ah.H, st, 9))
        C_ = K.from_handle(ch)
        K.release_handle(ch)
    finally:
        K.release_handle(ah)
        K.release_handle(bh)
    return C_, route, list(st)


def _triples(C_):
    rows = np.repeat(np.arange(C_.nrows, dtype=np.int64), np.diff(C_.rowptrs))
    bits = C_.values.view(np.int64)
    o = np.lexsort((bits, C_.colinds, rows))
    return rows[o], C_.colinds[o], bits[o]


@pytest.mark.parametrize('name', list(ROUTES))
def test_products_every_route_and_order(name, order, monkeypatch):
    """
    mult_ab / mult_abt on every route (general fast and generic forms, the dense-panel route with int32 / int64 pointers,
    float32 A and widened float32 B, its heavy-row form, A B^T whose B^T is sparse or a panel) under the column order in
    force: the route taken is the intended one, rowptrs and colinds are the oracle's in that order, values bit-exact where
    the suite claims the reference's sums (dense route: rows of A of at most 64 entries; general: B's rows hold no column
    twice) and within 1e-12 of the |A| |B| product elsewhere, and the (row, col, value) triples are the same bits under
    the other order.
    """
    from oracle import oracle as O
    from csr_amd.kernels import hip as K
    route, abt, adt, p64, bdt, k = ROUTES[name]
    heavy = name == 'dense_heavy_rows'
    if heavy:
        monkeypatch.setenv('CSRK_SPMM_HEAVY', '1')
    A, B = _product_operands(name)
    assert K.spgemm_order() == order
    C_, got_route, st = _multiply(A, B, abt, spmm_stats=heavy)
    assert got_route == route
    if heavy:
        assert st[0] == 1 and st[2] > 0                        # rows in the register-accumulator form
    a = (A.nrows, A.ncols, A.rowptrs, A.colinds, A.values)
    tb = (lambda v: O.transpose(B.nrows, B.ncols, B.rowptrs, B.colinds, v)) if abt else \
        (lambda v: (B.nrows, B.ncols, B.rowptrs, B.colinds, v))
    _, _, crp, cci, cvs = O.mult_ab(a, tb(B.values))
    _, _, _, _, cabs = O.mult_ab((A.nrows, A.ncols, A.rowptrs, A.colinds, np.abs(A.values)), tb(np.abs(B.values)))
    rci, rvs = as_library_orders(crp, cci, cvs)
    _, rabs = as_library_orders(crp, cci, cabs)
    assert C_.rowptrs.dtype == np.int32 and np.array_equal(C_.rowptrs, crp)
    assert np.array_equal(C_.colinds, rci)
    assert C_.values.dtype == np.float64 and np.all(np.abs(C_.values - rvs) <= 1e-12 * rabs + 1e-300)
    if route == 'dense-panel':
        exact = np.repeat(np.diff(A.rowptrs) <= 64, np.diff(crp))
        assert exact.any() and (~exact).any()
    else:
        _, bnc, brp, bci, _ = tb(B.values)
        key = np.repeat(np.arange(len(brp) - 1, dtype=np.int64), np.diff(brp)) * bnc + bci
        assert np.unique(key).size == key.size                 # (the operand as multiplied holds no column twice in a row)
        exact = np.ones(C_.nnz, dtype=bool)
    assert np.array_equal(C_.values[exact].view(np.int64), rvs[exact].view(np.int64))
    # the other order: the same entries, bit for bit
    K.set_spgemm_order('ascending' if order == 'reference' else 'reference')
    C2, route2, _ = _multiply(A, B, abt)
    assert route2 == route
    for x, y in zip(_triples(C_), _triples(C2)):
        assert np.array_equal(x, y)


def test_last_route_is_reset_by_a_failed_product(monkeypatch):
    """
    csrk_spgemm_last_route after a call that fails before any product runs reports 'general', not the previous call's
    route: csrk_spgemm_ab with handle 0, and csrk_spgemm_abt with a structure-only B (refused before the transpose).
    """
    from csr_amd import _lib
    from csr_amd._lib import lib
    from csr_amd.kernels import hip as K
    monkeypatch.delenv('CSRK_SPGEMM_DENSE', raising=False)
    rng = np.random.default_rng(80)
    A = _mat(_arrays(81, rng.integers(0, 20, 200), ncols=300), False)
    B = _panel_csr(rng.uniform(-1, 1, (300, 8)))
    Bs = _mat(_arrays(82, rng.integers(0, 20, 50), ncols=300, dtype=None), False)
    ah, bh, sh = _handle(A), _handle(B), _handle(Bs)
    try:
        def dense_product():
            K.release_handle(K.mult_ab(ah, bh))
            assert K.spgemm_last_route() == 'dense-panel'
        out = _lib.handle_t(0)
        dense_product()
        assert lib.csrk_spgemm_ab(0, bh.H, C.byref(out)) == _lib.ERR_INVALID and out.value == 0
        assert K.spgemm_last_route() == 'general'
        dense_product()
        assert lib.csrk_spgemm_abt(ah.H, sh.H, C.byref(out)) == _lib.ERR_INVALID and out.value == 0
        assert 'values' in _lib.last_error()
        assert K.spgemm_last_route() == 'general'
    finally:
        for h in (ah, bh, sh):
            K.release_handle(h)
