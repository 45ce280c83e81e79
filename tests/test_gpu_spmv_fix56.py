"""
Tier 0's 7-byte value stream (csr_amd/csrc/fix56.h): float64 values that lie on one binary grid are
stored in 56 bits and decoded by one exact add, so a product must be BIT FOR BIT what the float64 stream gives.

Every case builds two handles over the same arrays in one process -- one with CSRK_SPMV_FIX56=0 (raw float64 stream), one
without -- runs two products on each with a float64 x and two with a float32 x (csrk_spmv_f32x_device), and compares the
results as int64.  csrk_spmv_plan_stats slot 29 (tier 0's bytes) must be smaller under the packed plan exactly when the
tier's values are packable, and equal otherwise (a float32 matrix keeps its float32 stream either way).

Shapes are the smallest at which the packed path can go wrong: ~300 x 9000 (two full 4096-column blocks and a short one)
with rows of 1 .. 3000 entries -- runs that cross lanes and 512-entry tiles, a group of heavy rows that is absent from the
later blocks, so that a row step over 7 puts padding entries into packed tiles -- and ~40 x 600 with less than one tile.
CSRK_SPMV_HEAVY_SPLIT=1 and CSRK_HEAVY_MIN=64 give these small matrices a tier 0 (rows of >= 64 entries).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOP = float(2 ** 52 - 1)
DEN = 5e-324


def _shape(name):
    "rowptrs, colinds (ascending inside rows), the heavy rows' entry positions"
    rng = np.random.default_rng(7 if name == 'blocks' else 8)
    if name == 'blocks':
        nrows, ncols = 300, 9000
        lens = rng.integers(1, 40, size=nrows)
        heavy = np.arange(5, 300, 6)                                   # 50 heavy rows
        lens[heavy] = rng.integers(64, 900, size=len(heavy))
        lens[[11, 155, 293]] = [3000, 1700, 513]
        low_only = heavy[10:22]                                        # 12 neighbouring heavy rows that stay in block 0
    else:
        nrows, ncols = 40, 600
        lens = rng.integers(1, 20, size=nrows)
        lens[[3, 17, 30]] = [100, 64, 130]
        low_only = np.zeros(0, dtype=np.int64)
    rp = np.zeros(nrows + 1, dtype=np.int32)
    rp[1:] = np.cumsum(lens)
    ci = np.zeros(int(rp[-1]), dtype=np.int32)
    for r in range(nrows):
        hi = 4096 if r in low_only else ncols
        ci[rp[r]:rp[r + 1]] = np.sort(rng.integers(0, hi, size=lens[r]))
    heavy_rows = [r for r in range(nrows) if lens[r] >= 64]
    heavy_pos = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in heavy_rows])
    # what the stream must hold (spmv_plan.h, "long rows, accumulator form"): per 4096-column block the heavy rows' entries,
    # one padding entry per 7 rows of a step over 7 between two rows present in the block, the whole padded to 512-entry tiles
    tiles = pads = 0
    for b in range(-(-ncols // 4096)):
        cnt = [int(np.sum(ci[rp[r]:rp[r + 1]] // 4096 == b)) for r in heavy_rows]
        present = [k for k, c in enumerate(cnt) if c]
        pb = sum((k1 - k0 - 1) // 7 for k0, k1 in zip(present, present[1:]) if k1 - k0 > 7)
        pads += pb
        tiles += -(-(sum(cnt) + pb) // 512)
    return nrows, ncols, rp, ci, heavy_pos, tiles, pads


def _values(kind, nnz, heavy_pos, rng):
    "values of one set and whether tier 0 (the heavy rows' entries) is packable; the special values sit in heavy rows"
    j = rng.integers(-2 ** 52 + 1, 2 ** 52, size=nnz)
    grid = j.astype(np.float64) * 2.0 ** -52                           # the synthetic generator's form: exact
    ints = rng.integers(-1000, 1000, size=nnz).astype(np.float64)
    p = heavy_pos[[1, len(heavy_pos) // 2, -2]]                        # three entries of tier 0
    if kind == 'grid':
        return grid, True
    if kind == 'top':
        ints[p] = [1.0, TOP, -TOP]
        return ints, True
    if kind == 'over':
        ints[p] = [1.0, TOP, 2.0 ** 52]
        return ints, False
    if kind == 'zeros':
        return np.zeros(nnz), True
    if kind in ('neg0', 'nan', 'inf'):
        ints[p[1]] = {'neg0': -0.0, 'nan': np.nan, 'inf': np.inf}[kind]
        return ints, False
    if kind == 'third':
        grid[p[1]] = 1.0 / 3.0
        return grid, False
    if kind == 'subnormal':
        v = ints * 977.0 * DEN
        v[p] = [DEN, 2.0 ** -1023 + DEN, -(2.0 ** -1023)]
        return v, True
    if kind == 'huge':
        v = (2.0 * ints + 1.0) * 2.0 ** 971
        v[p[1]] = TOP * 2.0 ** 971
        return v, True
    if kind == 'g972':
        return (2.0 * ints + 1.0) * 2.0 ** 972, False
    if kind == 'float32':
        return rng.uniform(-1, 1, size=nnz).astype(np.float32), False
    raise AssertionError(kind)


KINDS = ['grid', 'top', 'over', 'zeros', 'neg0', 'nan', 'inf', 'third', 'subnormal', 'huge', 'g972', 'float32']


@pytest.fixture
def tier0_env(monkeypatch):
    for k in ('CSRK_SPMV_STREAM', 'CSRK_SPMV_HOT', 'CSRK_SPMV_FIX56'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('CSRK_SPMV_HEAVY_SPLIT', '1')
    monkeypatch.setenv('CSRK_HEAVY_MIN', '64')
    monkeypatch.setenv('CSRK_TIERB_MIN', '0')
    return monkeypatch


def _run(monkeypatch, shape, vals, fix56, x64, repeats=2):
    "products of a fresh handle: `repeats` with the float64 x, then as many with it as float32; and the plan's statistics"
    import torch
    from csr_amd._lib import lib, check, VAL_F32, VAL_F64
    nrows, ncols, rp, ci = shape[:4]
    if fix56:
        monkeypatch.delenv('CSRK_SPMV_FIX56', raising=False)
    else:
        monkeypatch.setenv('CSRK_SPMV_FIX56', '0')
    dev = torch.device('cuda', 0)
    dx64 = torch.from_numpy(x64).to(dev)
    dx32 = torch.from_numpy(x64.astype(np.float32)).to(dev)
    h = C.c_ssize_t(0)
    check(lib.csrk_create(nrows, ncols, len(ci), rp.ctypes.data_as(C.c_void_p), 0, ci.ctypes.data_as(C.c_void_p),
                          vals.ctypes.data_as(C.c_void_p), VAL_F32 if vals.dtype == np.float32 else VAL_F64, C.byref(h)))
    out = []
    try:
        for entry, dx in ((lib.csrk_spmv_device, dx64), (lib.csrk_spmv_f32x_device, dx32)):
            for _ in range(repeats):
                dy = torch.full((nrows,), float('nan'), dtype=torch.float64, device=dev)
                check(entry(h, dx.data_ptr(), dy.data_ptr(), None))
                torch.cuda.synchronize()
                out.append(dy.cpu().numpy().view(np.int64))
        st = (C.c_int64 * 34)()
        check(lib.csrk_spmv_plan_stats(h, st, 34))
    finally:
        check(lib.csrk_free(h))
    return out, list(st)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape_name', ['blocks', 'one_tile'])
def test_packed_tier0_is_bit_for_bit_the_raw_stream(tier0_env, shape_name, kind):
    shape = _shape(shape_name)
    nrows, ncols, rp, ci, heavy_pos, tiles, pads = shape
    rng = np.random.default_rng(KINDS.index(kind))
    vals, packable = _values(kind, len(ci), heavy_pos, rng)
    x = rng.uniform(-1, 1, size=ncols)
    raw, st_raw = _run(tier0_env, shape, vals, False, x)
    got, st_fix = _run(tier0_env, shape, vals, True, x)
    assert st_raw[10] == st_fix[10] == len(heavy_pos) and st_raw[4] == st_fix[4] == tiles      # the tier 0 the shape was made for
    assert (st_raw[5], tiles > 1, pads > 0) == ((3, True, True) if shape_name == 'blocks' else (1, False, False))
    assert tiles <= 256                      # fewer tiles than workgroups: every tile is stored once (no holes in the stream)
    for i, (a, b) in enumerate(zip(raw, got)):
        assert np.array_equal(a, b), (i, int(np.sum(a != b)))
    if packable:
        assert st_fix[29] == st_raw[29] - st_raw[4] * 512, (st_fix[29], st_raw[29])      # one byte per stored entry
        assert st_fix[25] == st_raw[25] - st_raw[4] * 512
    else:
        assert st_fix[29] == st_raw[29] and st_fix[25] == st_raw[25]


def test_packed_products_repeat_bit_for_bit(tier0_env):
    shape = _shape('blocks')
    nrows, ncols, rp, ci, heavy_pos = shape[:5]
    rng = np.random.default_rng(99)
    vals, _ = _values('grid', len(ci), heavy_pos, rng)
    ys, st = _run(tier0_env, shape, vals, True, rng.uniform(-1, 1, size=ncols), repeats=20)
    for k in (0, 20):                                                   # the float64-x products, then the float32-x ones
        for i in range(1, 20):
            assert np.array_equal(ys[k], ys[k + i]), (k, i)
