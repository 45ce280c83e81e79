"""
The sampled dense-dense product (csrk_sddmm / csrk_sddmm_device, hip.sddmm, CSR.sddmm) on the GPU.

Against a NumPy float64 restatement -- einsum('ij,ij->i', U[rows], V[cols]), times the values with scale -- within
1e-12 sum_t |u_t v_t| max(1, |value|), on the golden matrices, row lengths across every bound the kernel has (its
64-entry group runs, its 16-row window, rows far longer than a run) with empty rows at both ends, one row of 200 000
entries, unsorted and repeated columns, 1 x 1 and nnz = 0; for k across the 64-column chunks and their tails, scale
0 / 1, float32 / float64 panels, float64 / float32 / no values.  Bit for bit, without a tolerance: the int32 and int64
twins; the host entry against the device entry on a side stream, with the device panels packed, at column 0 of wider
panels (ld > k, 16-B loads) and at column offset 1 of wider panels (ld > k, 8-B / 4-B aligned bases: element loads), so
that for odd and even k the two load forms are compared; pick_rows of a permutation; and two calls in a row.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import Mat, load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [1, 3, 4, 5, 16, 17, 63, 64, 65, 128, 200]
EDGE_LENS = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4097]


def _csr(nr, nc, rp, ci, vs, ptr64=False):
    from csr_amd import CSR
    return CSR(nr, nc, int(rp[-1]), np.asarray(rp).astype(np.int64 if ptr64 else np.int32), np.asarray(ci, np.int32).copy(),
               None if vs is None else vs.copy(), _cast=False)


def _lens_pattern(seed, ncols=3000):
    "empty rows at both ends, every length bound, a spread of short rows, runs of empty rows longer than the window"
    rng = np.random.default_rng(seed)
    lens = np.concatenate([np.zeros(6, np.int64), EDGE_LENS, rng.integers(0, 12, 300), np.zeros(40, np.int64),
                           rng.integers(0, 3, 200), np.zeros(6, np.int64)]).astype(np.int64)
    rp = np.zeros(len(lens) + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    ci = rng.integers(0, ncols, size=int(rp[-1])).astype(np.int32)      # unsorted, repeated columns
    vs = rng.uniform(-1, 1, size=int(rp[-1]))
    return len(lens), ncols, rp, ci, vs


def _patterns():
    out = {}
    for name, pre in (('spmv', 'c3_'), ('spmv', 'c9_'), ('rows', 'c2_'), ('kat', 'a_')):
        d = load_golden(name)
        m = Mat(d, pre)
        vs = m.values if m.values is not None else np.random.default_rng(1).uniform(-1, 1, m.nnz)
        out[f'golden-{name}-{pre[:-1]}'] = (m.nrows, m.ncols, np.asarray(m.rowptrs, np.int64), np.asarray(m.colinds, np.int32),
                                            np.asarray(vs, np.float64))
    out['lens'] = _lens_pattern(3)
    rng = np.random.default_rng(5)
    n = 200_000
    out['long-row'] = (3, 50_000, np.array([0, 0, n, n], np.int64), rng.integers(0, 50_000, n).astype(np.int32),
                       rng.uniform(-1, 1, n))
    out['unsorted-repeated'] = (4, 7, np.array([0, 5, 5, 12, 14], np.int64),
                                np.array([6, 2, 2, 0, 6, 3, 3, 3, 1, 5, 0, 1, 4, 4], np.int32), rng.uniform(-1, 1, 14))
    out['1x1'] = (1, 1, np.array([0, 1], np.int64), np.array([0], np.int32), np.array([-0.75]))
    out['nnz0'] = (5, 4, np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0))
    return out


PATTERNS = _patterns()


def _panels(nr, nc, k, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (nr, k)).astype(dtype), rng.uniform(-1, 1, (nc, k)).astype(dtype)


def _reference(rp, ci, vs, U, V, scale):
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    Ur, Vr = U[rows].astype(np.float64), V[ci].astype(np.float64)
    ref = np.einsum('ij,ij->i', Ur, Vr)
    bnd = np.einsum('ij,ij->i', np.abs(Ur), np.abs(Vr))
    if scale and vs is not None:
        a = vs.astype(np.float64)
        ref = ref * a
        bnd = bnd * np.maximum(1.0, np.abs(a))
    return ref, bnd


def _check(got, ref, bnd):
    assert got.dtype == np.float64 and got.shape == ref.shape
    bad = ~(np.abs(got - ref) <= 1e-12 * bnd)
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:5], got[bad][:5], ref[bad][:5])


@pytest.mark.parametrize('pattern', sorted(PATTERNS))
def test_sddmm_against_numpy(pattern):
    nr, nc, rp, ci, vs = PATTERNS[pattern]
    for i, k in enumerate(KS):
        for pdt in (np.float64, np.float32):
            U, V = _panels(nr, nc, k, pdt, seed=i)
            ref0, bnd0 = _reference(rp, ci, None, U, V, False)
            for vdt in (np.float64, np.float32, None):
                v = None if vdt is None else vs.astype(vdt)
                A = _csr(nr, nc, rp, ci, v)
                for scale in (False, True):
                    R = A.sddmm(U, V, scale=scale)
                    assert R.nrows == nr and R.ncols == nc and R.rowptrs.dtype == A.rowptrs.dtype
                    assert np.array_equal(R.rowptrs, A.rowptrs) and np.array_equal(R.colinds, A.colinds)
                    if scale and v is not None:
                        a = v.astype(np.float64)
                        _check(R.values, ref0 * a, bnd0 * np.maximum(1.0, np.abs(a)))
                    else:
                        _check(R.values, ref0, bnd0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize('k', [1, 5, 17, 64, 65, 200])
@pytest.mark.parametrize('pdt', [np.float64, np.float32])
def test_sddmm_bitwise_invariants(k, pdt):
    import torch
    from csr_amd.kernels import hip as K
    from csr_amd._lib import lib, check, VAL_F32, VAL_F64
    nr, nc, rp, ci, vs = PATTERNS['lens']
    U, V = _panels(nr, nc, k, pdt, seed=k)
    A32, A64 = _csr(nr, nc, rp, ci, vs), _csr(nr, nc, rp, ci, vs, ptr64=True)
    h32, h64 = K.to_handle(A32), K.to_handle(A64)
    try:
        assert K._info(h32.H)[3] == 0 and K._info(h64.H)[3] == 1
        for scale in (False, True):
            base = K.sddmm(h32, U, V, scale)
            # the int64 twin
            assert np.array_equal(_bits(base), _bits(K.sddmm(h64, U, V, scale)))
            # the host entry with strided views (it packs them on the way: the kernel sees ld = k)
            Uw = np.zeros((nr, k + 3), pdt)
            Vw = np.zeros((nc, k + 2), pdt)
            Uw[:, 1:1 + k], Vw[:, 1:1 + k] = U, V
            Uo, Vo = Uw[:, 1:1 + k], Vw[:, 1:1 + k]
            assert not Uo.flags.c_contiguous and Uo.strides[1] == U.itemsize
            assert np.array_equal(_bits(base), _bits(K.sddmm(h32, Uo, Vo, scale)))
            assert np.array_equal(_bits(base), _bits(K.sddmm(h64, Uo, Vo, scale)))
            # two calls in a row
            assert np.array_equal(_bits(base), _bits(K.sddmm(h32, U, V, scale)))
            # the device entry on a non-default stream, with the panels as the kernel gets them from a torch caller:
            #   packed (ld = k: 16-B loads where k allows them, as in the host entry),
            #   at column 0 of wider panels whose row stride is a multiple of 16 B (ld > k, 16-B loads for every whole piece),
            #   at column offset 1 of wider panels (ld = k + 3 / k + 2, bases only 8-B / 4-B aligned: element loads only)
            # -- for every k the element-load form is compared with the 16-B form, bit for bit
            wide = (k // 4 + 1) * 4
            for (ou, wu), (ov, wv) in (((0, k), (0, k)), ((0, wide), (0, wide)), ((1, k + 3), (1, k + 2))):
                dU = torch.zeros(nr, wu, dtype=torch.from_numpy(U).dtype, device='cuda')
                dV = torch.zeros(nc, wv, dtype=dU.dtype, device='cuda')
                dU[:, ou:ou + k] = torch.from_numpy(U).cuda()
                dV[:, ov:ov + k] = torch.from_numpy(V).cuda()
                pu, pv = dU[:, ou:].data_ptr(), dV[:, ov:].data_ptr()
                assert (pu % 16 != 0) == (ou == 1) and (pv % 16 != 0) == (ov == 1)
                dout = torch.full((A32.nnz,), np.nan, dtype=torch.float64, device='cuda')
                st = torch.cuda.Stream()
                st.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(st):
                    check(lib.csrk_sddmm_device(h64.H, pu, wu, pv, wv, k, VAL_F64 if pdt == np.float64 else VAL_F32,
                                                int(scale), dout.data_ptr(), C.c_void_p(st.cuda_stream)))
                st.synchronize()
                assert np.array_equal(_bits(base), _bits(dout.cpu().numpy())), (ou, wu, ov, wv)
    finally:
        K.release_handle(h32)
        K.release_handle(h64)
    # pick_rows of a permutation: every entry keeps its value
    perm = np.random.default_rng(k).permutation(nr)
    P = A32.pick_rows(perm)
    got = P.sddmm(U[perm], V).values
    full = A32.sddmm(U, V).values
    idx = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in perm])
    assert np.array_equal(_bits(got), _bits(full[idx]))


@pytest.mark.parametrize('pdt', [np.float64, np.float32])
def test_sddmm_fully_populated_is_masked_product(pdt):
    nr, nc, k = 37, 29, 65
    rp = np.arange(nr + 1, dtype=np.int64) * nc
    ci = np.tile(np.arange(nc, dtype=np.int32), nr)
    vs = np.random.default_rng(2).uniform(-2, 2, nr * nc)
    U, V = _panels(nr, nc, k, pdt, seed=9)
    Ud, Vd = U.astype(np.float64), V.astype(np.float64)
    full = Ud @ Vd.T
    bnd = np.abs(Ud) @ np.abs(Vd).T
    A = _csr(nr, nc, rp, ci, vs)
    _check(A.sddmm(U, V).values, full.ravel(), bnd.ravel())
    Ad = vs.reshape(nr, nc)
    _check(A.sddmm(U, V, scale=True).values, (Ad * full).ravel(), (bnd * np.maximum(1.0, np.abs(Ad))).ravel())


def test_sddmm_nan_and_inf_stay_where_they_belong():
    nr, nc, rp, ci, vs = PATTERNS['lens']
    k = 17
    U, V = _panels(nr, nc, k, np.float64, seed=4)
    rows = np.repeat(np.arange(nr), np.diff(rp))
    j = int(ci[len(ci) // 2])
    Vn = V.copy()
    Vn[j, 5] = np.nan
    A = _csr(nr, nc, rp, ci, vs)
    out = A.sddmm(U, Vn).values
    assert np.array_equal(np.isnan(out), ci == j)
    i = int(rows[len(rows) // 3])
    Ui = U.copy()
    Ui[i, 3] = np.inf
    out = A.sddmm(Ui, V).values
    assert np.array_equal(~np.isfinite(out), rows == i)
    ref, bnd = _reference(rp, ci, None, U, V, False)
    _check(out[rows != i], ref[rows != i], bnd[rows != i])


def test_sddmm_device_entry_errors():
    import torch
    from csr_amd.kernels import hip as K
    from csr_amd._lib import lib, ERR_INVALID, OK, VAL_F64
    nr, nc, rp, ci, vs = PATTERNS['unsorted-repeated']
    A = _csr(nr, nc, rp, ci, vs)
    U, V = (torch.zeros(nr, 4, dtype=torch.float64, device='cuda'), torch.zeros(nc, 4, dtype=torch.float64, device='cuda'))
    out = torch.zeros(A.nnz, dtype=torch.float64, device='cuda')
    h = K.to_handle(A)
    try:
        H = h.H
        args = (U.data_ptr(), 4, V.data_ptr(), 4, 4, VAL_F64, 0, out.data_ptr(), None)
        assert lib.csrk_sddmm_device(H, *args) == OK
        for bad in [(U.data_ptr(), 3, V.data_ptr(), 4, 4, VAL_F64, 0, out.data_ptr(), None),
                    (U.data_ptr(), 4, V.data_ptr(), 3, 4, VAL_F64, 0, out.data_ptr(), None),
                    (U.data_ptr(), 4, V.data_ptr(), 4, 0, VAL_F64, 0, out.data_ptr(), None),
                    (U.data_ptr(), 4, V.data_ptr(), 4, 4, 0, 0, out.data_ptr(), None),
                    (U.data_ptr(), 4, V.data_ptr(), 4, 4, 7, 0, out.data_ptr(), None),
                    (None, 4, V.data_ptr(), 4, 4, VAL_F64, 0, out.data_ptr(), None),
                    (U.data_ptr(), 4, None, 4, 4, VAL_F64, 0, out.data_ptr(), None),
                    (U.data_ptr(), 4, V.data_ptr(), 4, 4, VAL_F64, 0, None, None)]:
            assert lib.csrk_sddmm_device(H, *bad) == ERR_INVALID, bad
    finally:
        K.release_handle(h)
    torch.cuda.synchronize()


def test_sddmm_at_size():
    "configs[2] (2M x 2M, nnz 5e7), k = 64 float64, in a child process under a time limit: parity on 2000 sampled rows"
    import json
    out = subprocess.run(['timeout', '-k', '10', '400', sys.executable, os.path.join(ROOT, 'tools', 'bench_sddmm.py'),
                          '--cases', 'f64', '--steps', '2', '--warmup', '1', '--rows', '2000', '--child-timeout', '380'],
                         cwd=ROOT, capture_output=True, text=True, timeout=420)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{')][-1])
    r = d['results'][0]
    assert d['parity_ok'] and r['parity']['rows'] == 2000 and r['repeat_bitwise'], r


def test_sddmm_row_blocks_above_max_nnz(monkeypatch):
    "above the kernel's max_nnz CSR.sddmm works per row block: the same bits as one call"
    from csr_amd.kernels import hip as K
    nr, nc, rp, ci, vs = PATTERNS['lens']
    U, V = _panels(nr, nc, 17, np.float64, seed=8)
    A = _csr(nr, nc, rp, ci, vs)
    whole = A.sddmm(U, V, scale=True)
    monkeypatch.setattr(K, 'max_nnz', 5000)
    assert len(A._row_blocks(K.max_nnz)) > 2
    blocks = A.sddmm(U, V, scale=True)
    assert np.array_equal(blocks.rowptrs, whole.rowptrs) and np.array_equal(blocks.colinds, whole.colinds)
    assert np.array_equal(_bits(blocks.values), _bits(whole.values))
