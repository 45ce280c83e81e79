"""
The seven HOST entries that take dense panels (csrk_spmm_dense, csrk_sddmm, csrk_gram_rows, csrk_als_rows,
csrk_solve_blocks, csrk_topk_scores, csrk_rank_entries) against their _device entries, bit for bit: what a host entry adds
is packing the caller's strided panels, the offset to row row_begin of U, and unpacking the results into the caller's
strides (csrc/panel.h).  The _device entries are proven against the references by the suites of their own.

5 rows x 6 columns with rows of 0, 1, 2, 3 and 6 entries (solve_blocks: 5 systems); k = 3 (no multiple of a 16-B piece in
either dtype) and 4 (a multiple in both), float32 and float64 where the entry takes both; every input panel packed and as
columns 1 .. 1 + k of a k + 3 wide array whose other columns hold NaN; every strided output packed and 3 wider, filled
with 7, of which only its own columns may change; the row ranges (0, 5), (2, 5), (3, 3); and no columns at all (V NULL).
A few hundred tiny calls.
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NR, NC = 5, 6
LENS = [0, 1, 2, 3, 6]
RANGES = [(0, 5), (2, 5), (3, 3)]
F32, F64 = 1, 2          # CSRK_VAL_F32, CSRK_VAL_F64
DTYPES = {F32: np.float32, F64: np.float64}


def _pattern(seed, ncols=NC):
    "rows of LENS entries, strictly ascending in column (a seen matrix must be canonical)"
    rng = np.random.default_rng(seed)
    lens = LENS if ncols else [0] * NR
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate([np.sort(rng.choice(ncols, n, replace=False)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    return rp, ci, rng.standard_normal(len(ci))


@pytest.fixture(scope='module')
def mats():
    from csr_amd import CSR
    from csr_amd.kernels import hip as K
    hs = {}
    for name, seed, ncols in (('seen', 1, NC), ('test', 2, NC), ('empty', 3, 0)):          # 'empty': no columns, so no entries
        rp, ci, vs = _pattern(seed, ncols)
        hs[name] = K.to_handle(CSR(NR, ncols, len(ci), rp, ci, vs, _cast=False))
    yield hs
    for h in hs.values():
        K.release_handle(h)


def _panel(rows, k, pt, seed):
    return np.random.default_rng(seed).standard_normal((rows, k)).astype(DTYPES[pt])


def _give(a, wide):
    "an input panel as the host entry gets it: (what keeps it alive, address, ld); None stays NULL"
    if a is None:
        return None, None, 1
    if not wide:
        a = np.ascontiguousarray(a)
        return a, a.ctypes.data, max(a.shape[1], 1)
    w = np.full((a.shape[0], a.shape[1] + 3), np.nan, a.dtype)
    w[:, 1:1 + a.shape[1]] = a
    return w, w.ctypes.data + a.dtype.itemsize, w.shape[1]


class _Take:
    "a strided output of the host entry, filled with 7: .address, .ld, .got (its own columns), .padding_untouched()"

    def __init__(self, rows, cols, dt, wide):
        self.w = np.full((rows, cols + (3 if wide else 0)), 7, dt)
        self.got = self.w[:, 1:1 + cols] if wide else self.w
        self.address, self.ld, self.cols, self.wide = self.got.ctypes.data, self.w.shape[1], cols, wide

    def padding_untouched(self):
        return not self.wide or (np.all(self.w[:, :1] == 7) and np.all(self.w[:, 1 + self.cols:] == 7))


def _card(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sevens(shape, dt):
    return _card(np.full(shape, 7, dt))


def _back(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same(a, b):
    "the same bits, and not the sevens both started as"
    written = a.size == 0 or not np.all(a == 7)
    return written and a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _ptr(t):
    return None if t is None else t.data_ptr()


def test_spmm_dense(mats):
    from csr_amd._lib import lib
    h = mats['seen']
    for k, win, wout in itertools.product((3, 4), (False, True), (False, True)):
        B = _panel(NC, k, F64, 10 + k)
        dB, dC = _card(B), _sevens((NR, k), np.float64)
        assert lib.csrk_spmm_dense_device(h.H, dB.data_ptr(), k, k, dC.data_ptr(), k, None) == 0
        keep, b, ldb = _give(B, win)
        C = _Take(NR, k, np.float64, wout)
        assert lib.csrk_spmm_dense(h.H, b, k, ldb, C.address, C.ld) == 0, lib.csrk_last_error()
        assert _same(C.got, _back(dC)) and C.padding_untouched(), (k, win, wout)


def test_sddmm(mats):
    from csr_amd._lib import lib
    h = mats['seen']
    for k, pt, win, scale in itertools.product((3, 4), (F32, F64), (False, True), (0, 1)):
        U, V = _panel(NR, k, pt, 20 + k), _panel(NC, k, pt, 30 + k)
        dU, dV, dO = _card(U), _card(V), _sevens(h.nnz, np.float64)
        assert lib.csrk_sddmm_device(h.H, dU.data_ptr(), k, dV.data_ptr(), k, k, pt, scale, dO.data_ptr(), None) == 0
        ku, u, ldu = _give(U, win)
        kv, v, ldv = _give(V, win)
        out = np.full(h.nnz, 7.0)
        assert lib.csrk_sddmm(h.H, u, ldu, v, ldv, k, pt, scale, out.ctypes.data) == 0, lib.csrk_last_error()
        assert _same(out, _back(dO)), (k, pt, win, scale)


def test_gram_rows(mats):
    from csr_amd._lib import lib
    for name, k, pt, win, (rb, re_), based in itertools.product(('seen', 'empty'), (3, 4), (F32, F64), (False, True), RANGES, (False, True)):
        h = mats[name]
        V = _panel(h.ncols, k, pt, 40 + k) if h.ncols else None
        base = _panel(k, k, F64, 50 + k) if based else None
        dV, dB, dO = (None if V is None else _card(V)), (None if base is None else _card(base)), _sevens((re_ - rb, k, k), np.float64)
        assert lib.csrk_gram_rows_device(h.H, rb, re_, _ptr(dV), k, k, pt, 1, _ptr(dB), dO.data_ptr(), None) == 0
        keep, v, ldv = _give(V, win)
        out = np.full((re_ - rb, k, k), 7.0)
        assert lib.csrk_gram_rows(h.H, rb, re_, v, max(ldv, k), k, pt, 1, None if base is None else base.ctypes.data, out.ctypes.data) == 0, \
            lib.csrk_last_error()
        assert _same(out, _back(dO)), (name, k, pt, win, rb, re_, based)


def test_als_rows(mats):
    from csr_amd._lib import lib
    for name, k, pt, win, wout, (rb, re_) in itertools.product(('seen', 'empty'), (3, 4), (F32, F64), (False, True), (False, True), RANGES):
        h = mats[name]
        n = re_ - rb
        V = _panel(h.ncols, k, pt, 60 + k) if h.ncols else None
        base = np.eye(k) * 2.0
        dV, dB, dO, dI = (None if V is None else _card(V)), _card(base), _sevens((n, k), np.float64), _sevens(n, np.int32)
        assert lib.csrk_als_rows_device(h.H, rb, re_, _ptr(dV), k, k, pt, 1, 2, dB.data_ptr(), 0.25, dO.data_ptr(), k, dI.data_ptr(), None) == 0
        keep, v, ldv = _give(V, win)
        out, info = _Take(n, k, np.float64, wout), np.full(n, 7, np.int32)
        assert lib.csrk_als_rows(h.H, rb, re_, v, max(ldv, k), k, pt, 1, 2, base.ctypes.data, 0.25, out.address, out.ld, info.ctypes.data) == 0, \
            lib.csrk_last_error()
        assert _same(out.got, _back(dO)) and _same(info, _back(dI)) and out.padding_untouched(), (name, k, pt, win, wout, rb, re_)


def test_solve_blocks():
    from csr_amd._lib import lib
    n = 5
    for k, win, wout in itertools.product((3, 4), (False, True), (False, True)):
        A = np.random.default_rng(70 + k).standard_normal((n, k, k))
        G = A @ A.transpose(0, 2, 1) + np.eye(k)
        G[2] = -G[2]                                                       # a system that is refused by its info, like any other
        b = _panel(n, k, F64, 80 + k)
        dG, db, dx, di = _card(G), _card(b), _sevens((n, k), np.float64), _sevens(n, np.int32)
        assert lib.csrk_solve_blocks_device(n, k, dG.data_ptr(), db.data_ptr(), k, dx.data_ptr(), k, di.data_ptr(), None) == 0
        keep, bb, ldb = _give(b, win)
        x, info = _Take(n, k, np.float64, wout), np.full(n, 7, np.int32)
        assert lib.csrk_solve_blocks(n, k, G.ctypes.data, bb, ldb, x.address, x.ld, info.ctypes.data) == 0, lib.csrk_last_error()
        assert _same(x.got, _back(dx)) and _same(info, _back(di)) and x.padding_untouched(), (k, win, wout)
        assert info[2] != 0 and info[0] == 0


def test_topk_scores(mats):
    from csr_amd._lib import lib
    n_top = 3
    for name, k, pt, win, wout, (rb, re_) in itertools.product(('seen', None, 'no items'), (3, 4), (F32, F64), (False, True), (False, True),
                                                             RANGES):
        H = mats[name].H if name == 'seen' else 0
        n_items = 0 if name == 'no items' else NC
        n = re_ - rb
        U = _panel(NR, k, pt, 90 + k)
        V = _panel(n_items, k, pt, 100 + k) if n_items else None
        dU, dV = _card(U), (None if V is None else _card(V))
        dI, dS, dC = _sevens((n, n_top), np.int32), _sevens((n, n_top), np.float64), _sevens(n, np.int32)
        assert lib.csrk_topk_scores_device(H, rb, re_, dU.data_ptr(), k, _ptr(dV), k, n_items, k, pt, n_top, -np.inf, dI.data_ptr(), n_top,
                                           dS.data_ptr(), n_top, dC.data_ptr(), None) == 0
        ku, u, ldu = _give(U, win)
        kv, v, ldv = _give(V, win)
        items, scores, counts = _Take(n, n_top, np.int32, wout), _Take(n, n_top, np.float64, wout), np.full(n, 7, np.int32)
        assert lib.csrk_topk_scores(H, rb, re_, u, ldu, v, max(ldv, k), n_items, k, pt, n_top, -np.inf, items.address, items.ld,
                                    scores.address, scores.ld, counts.ctypes.data) == 0, lib.csrk_last_error()
        case = (name, k, pt, win, wout, rb, re_)
        assert _same(items.got, _back(dI)) and _same(scores.got, _back(dS)) and _same(counts, _back(dC)), case
        assert items.padding_untouched() and scores.padding_untouched(), case


def test_rank_entries(mats):
    from csr_amd._lib import lib
    from csr_amd.kernels import hip as K
    test = mats['test']
    for name, k, pt, win, (rb, re_) in itertools.product(('seen', None), (3, 4), (F32, F64), (False, True), RANGES):
        S = mats[name].H if name else 0
        ne = K.row_extent(test, re_ - 1)[1] - K.row_extent(test, rb)[0] if re_ > rb else 0
        U, V = _panel(NR, k, pt, 110 + k), _panel(NC, k, pt, 120 + k)
        dU, dV, dR, dS = _card(U), _card(V), _sevens(ne, np.int32), _sevens(ne, np.float64)
        assert lib.csrk_rank_entries_device(S, test.H, rb, re_, dU.data_ptr(), k, dV.data_ptr(), k, k, pt, dR.data_ptr(), dS.data_ptr(),
                                            None) == 0
        ku, u, ldu = _give(U, win)
        kv, v, ldv = _give(V, win)
        ranks, scores = np.full(ne, 7, np.int32), np.full(ne, 7.0)
        assert lib.csrk_rank_entries(S, test.H, rb, re_, u, ldu, v, ldv, k, pt, ranks.ctypes.data, scores.ctypes.data) == 0, \
            lib.csrk_last_error()
        assert _same(ranks, _back(dR)) and _same(scores, _back(dS)), (name, k, pt, win, rb, re_)
