"""
Tier 0's 8.5-byte entries (csr_amd/csrc/fix56.h, namespace nib): grid-aligned float64 values in 6.5
bytes -- the mantissa's top nibble in a 4-bit plane -- beside a 16-bit index word {sign, row step, 12-bit column}; "sign set,
mantissa 0" is a padding entry, which the kernel sends to the window's zero slot.  The decode is exact and the addends and
their order are the raw stream's, so a product must be BIT FOR BIT what CSRK_SPMV_FIX56=0 gives.

CSRK_SPMV_NIB=1 takes the form whenever a group is packable (without the knob these small matrices keep the 9-byte entries:
accgroups::choose_nib, checked at the end).  Every case builds handles over the same arrays in one process, runs products
with a float64 x and with a float32 x (csrk_spmv_f32x_device) and compares the results as int64;
csrk_spmv_plan_stats slot 29 (tier 0's bytes) must be smaller by 768 per stored tile exactly when the tier is packable.

Shapes are those of test_gpu_spmv_fix56.py: ~300 x 9000 (two full 4096-column blocks and a short one) with rows of
1 .. 3000 entries -- runs that cross lanes and tiles, twelve neighbouring heavy rows absent from the later blocks, so that
row steps over 7 put padding entries into the tiles -- and ~40 x 600 with less than one tile.  The longest row holds columns
0, 4095 (the 12-bit field's top value), 4096, 8192 and the last one.  CSRK_SPMV_HEAVY_SPLIT=1, CSRK_HEAVY_MIN=64 and
CSRK_TIERB_MIN=0 give them a tier 0 of the rows of >= 64 entries.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOP = float(2 ** 52 - 1)
DEN = 5e-324
LONGEST = {'blocks': 11, 'one_tile': 30}


@functools.lru_cache(maxsize=None)
def _shape(name):
    "rowptrs, colinds (ascending inside rows), the heavy rows' entry positions, tier 0's tiles and padding entries"
    rng = np.random.default_rng(7 if name == 'blocks' else 8)
    if name == 'blocks':
        nrows, ncols = 300, 9000
        lens = rng.integers(1, 40, size=nrows)
        heavy = np.arange(5, 300, 6)                                   # 50 heavy rows
        lens[heavy] = rng.integers(64, 900, size=len(heavy))
        lens[[11, 155, 293]] = [3000, 1700, 513]
        low_only = heavy[10:22]                                        # 12 neighbouring heavy rows that stay in block 0
        edge = [0, 4095, 4096, 8192, ncols - 1]
    else:
        nrows, ncols = 40, 600
        lens = rng.integers(1, 20, size=nrows)
        lens[[3, 17, 30]] = [100, 64, 130]
        low_only = np.zeros(0, dtype=np.int64)
        edge = [0, ncols - 1]
    rp = np.zeros(nrows + 1, dtype=np.int32)
    rp[1:] = np.cumsum(lens)
    ci = np.zeros(int(rp[-1]), dtype=np.int32)
    for r in range(nrows):
        hi = 4096 if r in low_only else ncols
        c = rng.integers(0, hi, size=lens[r])
        if r == LONGEST[name]:
            c[:len(edge)] = edge
        ci[rp[r]:rp[r + 1]] = np.sort(c)
    heavy_rows = [r for r in range(nrows) if lens[r] >= 64]
    heavy_pos = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in heavy_rows])
    tiles, pads = _tiles(ncols, rp, ci, [heavy_rows])
    for a in (rp, ci, heavy_pos):
        a.setflags(write=False)
    return nrows, ncols, rp, ci, heavy_pos, tiles, pads


def _tiles(ncols, rp, ci, groups):
    """
    what the groups' streams must hold (spmv_plan.h, "long rows, accumulator form"): per 4096-column block a group's entries,
    one padding entry per 7 rows of a step over 7 between two rows present in the block, the whole padded to 512-entry tiles
    """
    tiles = pads = 0
    for rows in groups:
        for b in range(-(-ncols // 4096)):
            cnt = [int(np.sum(ci[rp[r]:rp[r + 1]] // 4096 == b)) for r in rows]
            present = [k for k, c in enumerate(cnt) if c]
            pb = sum((k1 - k0 - 1) // 7 for k0, k1 in zip(present, present[1:]) if k1 - k0 > 7)
            pads += pb
            tiles += -(-(sum(cnt) + pb) // 512)
    return tiles, pads


def _values(kind, nnz, heavy_pos, rng):
    "values of one set and whether tier 0 (the heavy rows' entries) is packable; the special values sit in heavy rows"
    j = rng.integers(-2 ** 52 + 1, 2 ** 52, size=nnz)
    grid = j.astype(np.float64) * 2.0 ** -52
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
PACKABLE = ['grid', 'top', 'zeros', 'subnormal', 'huge']


@pytest.fixture
def tier0_env(monkeypatch):
    for k in ('CSRK_SPMV_STREAM', 'CSRK_SPMV_HOT', 'CSRK_SPMV_FIX56', 'CSRK_ACC_GROUPS', 'CSRK_ACC_GROUP_ROWS'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('CSRK_SPMV_NIB', '1')
    monkeypatch.setenv('CSRK_SPMV_HEAVY_SPLIT', '1')
    monkeypatch.setenv('CSRK_HEAVY_MIN', '64')
    monkeypatch.setenv('CSRK_TIERB_MIN', '0')
    return monkeypatch


def _set(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, str(value))


def _run(monkeypatch, shape, vals, x64, fix56=True, nib=1, ptr64=False, groups=None, group_rows=None, repeats=2):
    """
    products of a fresh handle built under the knobs: `repeats` with the float64 x, then as many with it as float32 -> the
    results as int64, and the plan's statistics.  fix56=False: CSRK_SPMV_FIX56=0, the raw stream (whatever CSRK_SPMV_NIB says).
    """
    import torch
    from csr_amd._lib import lib, check, VAL_F32, VAL_F64
    nrows, ncols, rp, ci = shape[:4]
    _set(monkeypatch, 'CSRK_SPMV_FIX56', None if fix56 else 0)
    _set(monkeypatch, 'CSRK_SPMV_NIB', nib)
    _set(monkeypatch, 'CSRK_ACC_GROUPS', groups)
    _set(monkeypatch, 'CSRK_ACC_GROUP_ROWS', group_rows)
    dev = torch.device('cuda', 0)
    dx64 = torch.from_numpy(x64).to(dev)
    dx32 = torch.from_numpy(x64.astype(np.float32)).to(dev)
    rpp = rp.astype(np.int64) if ptr64 else rp
    h = C.c_ssize_t(0)
    check(lib.csrk_create(nrows, ncols, len(ci), rpp.ctypes.data_as(C.c_void_p), 1 if ptr64 else 0, ci.ctypes.data_as(C.c_void_p),
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


def _same(raw, got, tag):
    assert len(raw) == len(got)
    for i, (a, b) in enumerate(zip(raw, got)):
        assert np.array_equal(a, b), (tag, i, int(np.sum(a != b)))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape_name', ['blocks', 'one_tile'])
def test_nib_tier0_is_bit_for_bit_the_raw_stream(tier0_env, shape_name, kind):
    shape = _shape(shape_name)
    nrows, ncols, rp, ci, heavy_pos, tiles, pads = shape
    rng = np.random.default_rng(KINDS.index(kind))
    vals, packable = _values(kind, len(ci), heavy_pos, rng)
    assert packable == (kind in PACKABLE)
    x = rng.uniform(-1, 1, size=ncols)
    raw, st_raw = _run(tier0_env, shape, vals, x, fix56=False)
    assert st_raw[10] == len(heavy_pos) and st_raw[4] == tiles                                 # the tier 0 the shape was made for
    assert (st_raw[5], tiles > 1, pads > 0) == ((3, True, True) if shape_name == 'blocks' else (1, False, False))
    assert tiles <= 256                      # fewer tiles than workgroups: every tile is stored once (no holes in the stream)
    for ptr64 in (False, True):
        got, st = _run(tier0_env, shape, vals, x, ptr64=ptr64)
        assert st[10] == st_raw[10] and st[4] == tiles
        _same(raw, got, (kind, ptr64))
        if packable:
            assert st[29] == st_raw[29] - tiles * 768, (st[29], st_raw[29])      # a byte and a half per stored entry
        else:
            assert st[29] == st_raw[29]
        # (the whole plan's bytes: 64-bit row pointers widen the light view's table, the rest is the same)
        assert st[25] - st[29] == st_raw[25] - st_raw[29] + (4 * (nrows + 1) if ptr64 else 0)


def _deal(lens_heavy, rows_heavy, G, cap):
    "the tier's groups (lists of rows, ascending) and the number of launches: the rule of acc_groups.h"
    if G == 1:
        groups = [rows_heavy[i:i + cap] for i in range(0, len(rows_heavy), cap)]
        return groups, len(groups)
    ranked = [r for _, _, r in sorted((-n, r, r) for n, r in zip(lens_heavy, rows_heavy))]
    groups, launches = [], 0
    for r0 in range(0, len(ranked), G * cap):
        part = ranked[r0:r0 + G * cap]
        gb = min(G, -(-len(part) // cap))
        groups += [sorted(part[g::gb]) for g in range(gb)]
        launches += 1
    return groups, launches


@pytest.mark.parametrize('groups', [1, 2, 3])
def test_nib_with_groups_side_by_side(tier0_env, groups):
    """
    53 heavy rows in groups of 20: three launches (G = 1), a launch of two groups and one of one (G = 2), one launch of three
    (G = 3).  On-grid values: every group takes the form.  One value off the grid: its group is raw, and with it every group
    of its launch -- for G = 3 the whole tier.
    """
    shape = _shape('blocks')
    nrows, ncols, rp, ci, heavy_pos = shape[:5]
    lens = np.diff(rp)
    rows_heavy = [r for r in range(nrows) if lens[r] >= 64]
    dealt, launches = _deal([int(lens[r]) for r in rows_heavy], rows_heavy, groups, 20)
    assert (len(dealt), launches) == {1: (3, 3), 2: (3, 2), 3: (3, 1)}[groups]
    tiles, pads = _tiles(ncols, rp, ci, dealt)
    rng = np.random.default_rng(40 + groups)
    x = rng.uniform(-1, 1, size=ncols)
    for kind in ('grid', 'third'):
        vals, _ = _values(kind, len(ci), heavy_pos, rng)
        raw, st_raw = _run(tier0_env, shape, vals, x, fix56=False, groups=groups, group_rows=20)
        got, st = _run(tier0_env, shape, vals, x, groups=groups, group_rows=20)
        assert st_raw[4] == st[4] == tiles and st[10] == len(heavy_pos)
        _same(raw, got, (kind, groups))
        if kind == 'grid':
            assert st[29] == st_raw[29] - tiles * 768 and st[25] == st_raw[25] - tiles * 768, (st[29], st_raw[29])
        elif groups == 3:       # a packable and an unpackable group in one launch: the launch is raw
            assert st[29] == st_raw[29] and st[25] == st_raw[25], (st[29], st_raw[29])
        else:                   # the launches without the value pack
            assert st_raw[29] - tiles * 768 < st[29] < st_raw[29], (st[29], st_raw[29])


@pytest.mark.parametrize('groups,group_rows', [(None, None), (3, 20)])
def test_nan_and_inf_in_x_reach_only_the_rows_that_hold_them(tier0_env, groups, group_rows):
    """
    NaN and Inf at a block's column 0 (columns 0, 4096, 8192), at column 4095 and at the last column: a padding entry that
    read its column field instead of the zero slot would spread them to rows that do not hold those columns.
    """
    shape = _shape('blocks')
    nrows, ncols, rp, ci, heavy_pos = shape[:5]
    rng = np.random.default_rng(51)
    vals, _ = _values('grid', len(ci), heavy_pos, rng)
    assert np.all(vals != 0.0)
    x = rng.uniform(-1, 1, size=ncols)
    special = {0: np.nan, 4095: np.inf, 4096: -np.inf, 8192: np.nan, ncols - 1: np.inf}
    for c, v in special.items():
        x[c] = v
    holds = np.array([bool(np.isin(ci[rp[r]:rp[r + 1]], list(special)).any()) for r in range(nrows)])
    assert holds[LONGEST['blocks']] and 0 < holds.sum() < nrows
    raw, st_raw = _run(tier0_env, shape, vals, x, fix56=False, groups=groups, group_rows=group_rows)
    got, st = _run(tier0_env, shape, vals, x, groups=groups, group_rows=group_rows)
    assert st[29] == st_raw[29] - st_raw[4] * 768
    _same(raw, got, 'special x')
    for y in got:
        assert np.array_equal(np.isfinite(y.view(np.float64)), ~holds)


def test_column_4095_of_a_heavy_row(tier0_env):
    "x = 1 at column 4095 alone: every row's product is the sum of its values on that column, exactly"
    shape = _shape('blocks')
    nrows, ncols, rp, ci, heavy_pos = shape[:5]
    rng = np.random.default_rng(52)
    vals = rng.integers(-1000, 1000, size=len(ci)).astype(np.float64)
    r = LONGEST['blocks']
    assert 4095 in ci[rp[r]:rp[r + 1]]
    x = np.zeros(ncols)
    x[4095] = 1.0
    want = np.array([np.sum(vals[rp[q]:rp[q + 1]][ci[rp[q]:rp[q + 1]] == 4095]) for q in range(nrows)])
    assert np.any(want != 0.0)
    got, st = _run(tier0_env, shape, vals, x)
    raw, st_raw = _run(tier0_env, shape, vals, x, fix56=False)
    assert st[29] == st_raw[29] - st_raw[4] * 768
    _same(raw, got, 'column 4095')
    for y in got:
        assert np.array_equal(y.view(np.float64), want)


def test_nib_products_repeat_bit_for_bit(tier0_env):
    shape = _shape('blocks')
    nrows, ncols, rp, ci, heavy_pos = shape[:5]
    rng = np.random.default_rng(99)
    vals, _ = _values('grid', len(ci), heavy_pos, rng)
    ys, st = _run(tier0_env, shape, vals, rng.uniform(-1, 1, size=ncols), repeats=20)
    for k in (0, 20):                                                   # the float64-x products, then the float32-x ones
        for i in range(1, 20):
            assert np.array_equal(ys[k], ys[k + i]), (k, i)


@pytest.mark.parametrize('shape_name', ['blocks', 'one_tile'])
def test_without_the_knob_small_tiers_keep_9_byte_entries(tier0_env, shape_name):
    "the selection rule: less than 16 tiles per workgroup -> the 9-byte form, as CSRK_SPMV_NIB=0 gives it"
    shape = _shape(shape_name)
    nrows, ncols, rp, ci, heavy_pos, tiles, pads = shape
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, size=ncols)
    for kind in PACKABLE:
        vals, _ = _values(kind, len(ci), heavy_pos, rng)
        raw, st_raw = _run(tier0_env, shape, vals, x, fix56=False, nib=None)
        for nib in (None, 0):
            got, st = _run(tier0_env, shape, vals, x, nib=nib)
            _same(raw, got, (kind, nib))
            assert st[4] == tiles and st[29] == st_raw[29] - tiles * 512 and st[25] == st_raw[25] - tiles * 512, (kind, nib)
