"""
SpMV tier 0 with several row groups side by side in one launch of the accumulator kernel (DESIGN.md section 4,
csr_amd/csrc/acc_groups.h): CSRK_ACC_GROUPS groups share a launch, CSRK_ACC_GROUP_ROWS (a test hook) sets how many rows a
group holds, so that a small matrix fills several groups and several launches.

Shapes are the smallest at which the grouped tier can go wrong: 300 x 9000 (two full 4096-column blocks and a short one)
with 123 heavy rows -- 120 of 64 .. 900 entries and three of 513, 1700 and 3000 --, twelve neighbouring heavy rows that
stay in block 0 and are dealt to ONE group (their lengths are chosen for it), so that a row step over 7 puts padding
entries into that group's tiles, light rows of 1 .. 39 entries; and 40 x 600 with three heavy rows and less than one tile
per group.  CSRK_SPMV_HEAVY_SPLIT=1, CSRK_HEAVY_MIN=64 and CSRK_TIERB_MIN=0 make the rows of >= 64 entries tier 0 and leave
tier 1 empty (the epilogue reduces every group); CSRK_TIERB_MIN=20 puts the rows of 20 .. 63 entries into tier 1, whose
launch then carries the groups' reduce when tier 0 is a single launch.

Reference: the product summed row by row, sequentially, in NumPy; bound 1e-12 * sum |a x| + 1e-300 (float64 sums of at most
3000 terms in any order differ from it by less than 3000 * 2^-53 = 3.4e-13 of that sum).
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HEAVY = 64


@functools.lru_cache(maxsize=None)
def _shape(name):
    "rowptrs (int32), colinds (ascending inside rows), row lengths"
    rng = np.random.default_rng(27 if name == 'blocks' else 28)
    if name == 'blocks':
        nrows, ncols = 300, 9000
        lens = rng.integers(1, 40, size=nrows)
        heavy = np.sort(rng.choice(nrows, size=123, replace=False))
        # distinct lengths, so that the ranks by length are known: rank 0 the longest
        pool = np.setdiff1d(np.arange(64, 901), [513])
        ranked = np.sort(np.concatenate([[3000, 1700, 513], rng.choice(pool, size=120, replace=False)]))[::-1]
        low_only = heavy[40:52]                                        # 12 neighbouring heavy rows that stay in block 0 ...
        low_ranks = 6 * np.arange(1, 13)                               # ... with ranks = 0 mod 2 and mod 3: one group for G = 2 and 3
        rest = np.setdiff1d(np.arange(123), low_ranks)
        rng.shuffle(rest)
        lens[low_only] = ranked[low_ranks]
        lens[np.setdiff1d(heavy, low_only)] = ranked[rest]
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
        ci[rp[r]:rp[r + 1]] = np.sort(rng.choice(hi, size=lens[r], replace=False) if lens[r] <= hi else rng.integers(0, hi, size=lens[r]))
    return nrows, ncols, rp, ci, lens


def _deal(lens, G, cap):
    "the tier's groups (lists of rows, ascending) and the first group of each launch: the rule of acc_groups.h"
    rows = [r for r in range(len(lens)) if lens[r] >= HEAVY]
    if G == 1:
        groups = [rows[i:i + cap] for i in range(0, len(rows), cap)]
        return groups, list(range(len(groups) + 1))
    ranked = sorted(rows, key=lambda r: (-lens[r], r))
    groups, first = [], [0]
    for r0 in range(0, len(ranked), G * cap):
        part = ranked[r0:r0 + G * cap]
        gb = min(G, -(-len(part) // cap))
        groups += [sorted(part[g::gb]) for g in range(gb)]
        first.append(len(groups))
    return groups, first


def _tiles(shape, groups):
    "512-entry tiles and padding entries of the groups' streams (spmv_plan.h, 'long rows, accumulator form')"
    nrows, ncols, rp, ci, lens = shape
    tiles = pads = 0
    for rows in groups:
        for b in range(-(-ncols // 4096)):
            cnt = [int(np.sum(ci[rp[r]:rp[r + 1]] // 4096 == b)) for r in rows]
            present = [k for k, c in enumerate(cnt) if c]
            pb = sum((k1 - k0 - 1) // 7 for k0, k1 in zip(present, present[1:]) if k1 - k0 > 7)
            pads += pb
            tiles += -(-(sum(cnt) + pb) // 512)
    return tiles, pads


@functools.lru_cache(maxsize=None)
def _values(shape_name, kind):
    nrows, ncols, rp, ci, lens = _shape(shape_name)
    rng = np.random.default_rng(['grid', 'third', 'float32'].index(kind))
    nnz = len(ci)
    if kind == 'float32':
        return rng.uniform(-1, 1, size=nnz).astype(np.float32)
    v = rng.integers(-2 ** 52 + 1, 2 ** 52, size=nnz).astype(np.float64) * 2.0 ** -52      # on one grid: packable
    if kind == 'third':
        r = int(np.argmax(lens))
        v[rp[r] + 5] = 1.0 / 3.0                                                            # one heavy row's group is not
    return v


@functools.lru_cache(maxsize=None)
def _x(shape_name):
    x = np.random.default_rng(5).uniform(-1, 1, size=_shape(shape_name)[1])
    return x, x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(shape_name, kind, x32):
    "sequential row sums and the bound; a float32 matrix times a float32 x rounds each product to float32 (the library's rule)"
    nrows, ncols, rp, ci, lens = _shape(shape_name)
    v = _values(shape_name, kind)
    x = _x(shape_name)[1 if x32 else 0]
    prod = (v * x[ci]).astype(np.float64) if (v.dtype == np.float32 and x32) else v.astype(np.float64) * x[ci].astype(np.float64)
    ref = np.array([np.cumsum(prod[rp[r]:rp[r + 1]])[-1] for r in range(nrows)])
    bound = np.array([np.sum(np.abs(prod[rp[r]:rp[r + 1]])) for r in range(nrows)])
    ref.setflags(write=False)
    bound.setflags(write=False)
    return ref, bound


def _set(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, str(value))


@pytest.fixture
def tier0_env(monkeypatch):
    for k in ('CSRK_SPMV_STREAM', 'CSRK_SPMV_HOT', 'CSRK_SPMV_FIX56', 'CSRK_ACC_GROUPS', 'CSRK_ACC_GROUP_ROWS'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('CSRK_SPMV_HEAVY_SPLIT', '1')
    monkeypatch.setenv('CSRK_HEAVY_MIN', str(HEAVY))
    monkeypatch.setenv('CSRK_TIERB_MIN', '0')
    return monkeypatch


def _run(monkeypatch, shape_name, kind, groups, group_rows, fix56=True, ptr64=False, tier1_min=0, repeats=2):
    """
    a fresh handle under the knobs: `repeats` products by csrk_spmv_device, two by csrk_spmv_f32x_device, one by
    csrk_spmv_device_part (part 1, then part 2) -> the results as int64, the row sums of part 1 alone, the plan's statistics
    """
    import torch
    from csr_amd._lib import lib, check, VAL_F32, VAL_F64
    nrows, ncols, rp, ci, lens = _shape(shape_name)
    vals = _values(shape_name, kind)
    x64, x32 = _x(shape_name)
    _set(monkeypatch, 'CSRK_ACC_GROUPS', groups)
    _set(monkeypatch, 'CSRK_ACC_GROUP_ROWS', group_rows)
    _set(monkeypatch, 'CSRK_SPMV_FIX56', None if fix56 else 0)
    _set(monkeypatch, 'CSRK_TIERB_MIN', tier1_min)
    dev = torch.device('cuda', 0)
    dx64 = torch.from_numpy(x64).to(dev)
    dx32 = torch.from_numpy(x32).to(dev)
    rpp = rp.astype(np.int64) if ptr64 else rp
    h = C.c_ssize_t(0)
    check(lib.csrk_create(nrows, ncols, len(ci), rpp.ctypes.data_as(C.c_void_p), 1 if ptr64 else 0, ci.ctypes.data_as(C.c_void_p),
                          vals.ctypes.data_as(C.c_void_p), VAL_F32 if vals.dtype == np.float32 else VAL_F64, C.byref(h)))
    res = {'f64': [], 'f32x': [], 'parts': None, 'part1': None}
    try:
        def product(call):
            dy = torch.full((nrows,), float('nan'), dtype=torch.float64, device=dev)
            call(dy)
            torch.cuda.synchronize()
            return dy
        for _ in range(repeats):
            res['f64'].append(product(lambda dy: check(lib.csrk_spmv_device(h, dx64.data_ptr(), dy.data_ptr(), None))).cpu().numpy())
        for _ in range(2):
            res['f32x'].append(product(lambda dy: check(lib.csrk_spmv_f32x_device(h, dx32.data_ptr(), dy.data_ptr(), None))).cpu().numpy())
        dy = product(lambda dy: check(lib.csrk_spmv_device_part(h, dx64.data_ptr(), dy.data_ptr(), None, 1)))
        res['part1'] = dy.cpu().numpy()
        check(lib.csrk_spmv_device_part(h, dx64.data_ptr(), dy.data_ptr(), None, 2))
        torch.cuda.synchronize()
        res['parts'] = dy.cpu().numpy()
        st = (C.c_int64 * 34)()
        check(lib.csrk_spmv_plan_stats(h, st, 34))
    finally:
        check(lib.csrk_free(h))
    return res, list(st)


_BASE = {}


def _base(monkeypatch, shape_name, kind, tier1_min):
    "the CSRK_ACC_GROUPS=1 product (one group holds every heavy row): computed once per matrix, shared, never written"
    key = (shape_name, kind, tier1_min)
    if key not in _BASE:
        res, st = _run(monkeypatch, shape_name, kind, 1, None, tier1_min=tier1_min)
        for a in res['f64'] + res['f32x'] + [res['parts'], res['part1']]:
            a.setflags(write=False)
        _BASE[key] = (res, st)
    return _BASE[key]


def _bits(a):
    return a.view(np.int64)


def _check_case(monkeypatch, shape_name, groups, group_rows, tier1_min):
    shape = _shape(shape_name)
    nrows, ncols, rp, ci, lens = shape
    dealt, first = _deal(lens, groups, group_rows)
    tiles, pads = _tiles(shape, dealt)
    heavy_rows = np.flatnonzero(lens >= HEAVY)
    tier_rows = np.flatnonzero(lens >= (tier1_min if tier1_min else HEAVY))
    outside = np.setdiff1d(np.arange(nrows), tier_rows)
    t0_entries = int(np.sum(lens[heavy_rows]))
    for kind in ('grid', 'third', 'float32'):
        base, st_base = _base(monkeypatch, shape_name, kind, tier1_min)
        runs = {}
        for fix56 in ((True, False) if kind != 'float32' else (True,)):
            for ptr64 in ((False, True) if kind == 'grid' else (False,)):
                reps = 20 if (kind == 'grid' and fix56 and not ptr64) else 2
                runs[fix56, ptr64] = _run(monkeypatch, shape_name, kind, groups, group_rows, fix56, ptr64, tier1_min, reps)
        for (fix56, ptr64), (res, st) in runs.items():
            tag = (kind, groups, group_rows, tier1_min, fix56, ptr64)
            # the tier the knobs ask for
            assert st[10] == t0_entries and st[9] == len(heavy_rows), (tag, st[9], st[10])
            assert (st[9] > group_rows) == (len(dealt) > 1), (tag, st[9], len(dealt))
            assert st[4] == tiles and st[5] == -(-ncols // 4096), (tag, st[4], tiles, st[5])
            assert (st[11] > 0) == (tier1_min > 0), (tag, st[11])
            # values: within the bound of the sequential sum, by every entry point
            for name, x32 in (('f64', False), ('f32x', True), ('parts', False)):
                ref, bound = _reference(shape_name, kind, x32)
                for y in (res[name] if isinstance(res[name], list) else [res[name]]):
                    err = np.abs(y - ref)
                    worst = float(np.max(err / (1e-12 * bound + 1e-300)))
                    print(f'{tag} {name}: max |y - ref| / bound = {worst:.3e}')
                    assert np.all(err <= 1e-12 * bound + 1e-300), (tag, name, worst)
            # repeats, and the two-part product, bit for bit
            for y in res['f64'][1:] + [res['parts']]:
                assert np.array_equal(_bits(y), _bits(res['f64'][0])), tag
            assert np.array_equal(_bits(res['f32x'][0]), _bits(res['f32x'][1])), tag
            # part 1 writes 0.0 to the tiers' rows; the rows outside the tiers are what one group leaves, bit for bit
            assert np.all(res['part1'][tier_rows] == 0.0), tag
            for name in ('f64', 'f32x'):
                assert np.array_equal(_bits(res[name][0][outside]), _bits(base[name][0][outside])), (tag, name)
            assert np.array_equal(_bits(res['part1'][outside]), _bits(base['part1'][outside])), tag
            # 64-bit row pointers: the same plan, the same bits
            assert np.array_equal(_bits(res['f64'][0]), _bits(runs[fix56, False][0]['f64'][0])), tag
            assert st[4] == runs[fix56, False][1][4], tag
        if kind != 'float32':
            # the 7-byte stream is exact with groups on: every product bit for bit the raw stream's
            (fx, st_fix), (raw, st_raw) = runs[True, False], runs[False, False]
            for name in ('f64', 'f32x'):
                for a, b in zip(fx[name], raw[name]):
                    assert np.array_equal(_bits(a), _bits(b)), (kind, groups, group_rows, name)
            assert np.array_equal(_bits(fx['parts']), _bits(raw['parts']))
            if kind == 'grid':      # one byte per stored entry, tiles summed over the groups
                assert st_fix[29] == st_raw[29] - st_raw[4] * 512 and st_fix[25] == st_raw[25] - st_raw[4] * 512, (st_fix[29], st_raw[29])
            else:                   # a launch with an unpackable group stays raw as a whole; other launches may pack
                assert st_raw[29] - st_raw[4] * 512 < st_fix[29] <= st_raw[29], (st_fix[29], st_raw[29])
    return dealt, first, pads


@pytest.mark.parametrize('tier1_min', [0, 20])
@pytest.mark.parametrize('groups', [1, 2, 3])
@pytest.mark.parametrize('group_rows', [16, 40, 41, 123])
def test_groups_side_by_side(tier0_env, group_rows, groups, tier1_min):
    """
    123 heavy rows in groups of 16 (more rows than the groups of one launch hold: several launches), 40 (a launch of full
    groups and three rows left over), 41 (exactly full groups for G = 3) and 123 (one group, whatever G is).
    """
    dealt, first, pads = _check_case(tier0_env, 'blocks', groups, group_rows, tier1_min)
    want = {(16, 1): (8, 8), (16, 2): (8, 4), (16, 3): (8, 3), (40, 1): (4, 4), (40, 2): (4, 2), (40, 3): (4, 2),
            (41, 1): (3, 3), (41, 2): (3, 2), (41, 3): (3, 1), (123, 1): (1, 1), (123, 2): (1, 1), (123, 3): (1, 1)}
    assert (len(dealt), len(first) - 1) == want[group_rows, groups]
    if group_rows == 123 or (groups > 1 and group_rows >= 40):
        assert pads > 0        # the twelve block-0 rows sit in one group: its later blocks hold padding entries


@pytest.mark.parametrize('groups,group_rows', [(2, 2), (3, 1), (3, 2)])
def test_groups_of_less_than_one_tile(tier0_env, groups, group_rows):
    "40 x 600, three heavy rows: groups of two rows and one, or of one row each -- fewer tiles than workgroups everywhere"
    dealt, first, pads = _check_case(tier0_env, 'one_tile', groups, group_rows, 0)
    assert [len(g) for g in dealt] == ([2, 1] if group_rows == 2 else [1, 1, 1]) and len(first) == 2


def test_one_group_is_the_plan_without_the_knob(tier0_env):
    "CSRK_ACC_GROUPS=1 against the knob unset: the same plan (statistics) and the same bits"
    for shape_name in ('blocks', 'one_tile'):
        for kind in ('grid', 'float32'):
            one, st_one = _run(tier0_env, shape_name, kind, 1, None)
            unset, st_unset = _run(tier0_env, shape_name, kind, None, None)
            assert st_one == st_unset
            for name in ('f64', 'f32x'):
                for a, b in zip(one[name], unset[name]):
                    assert np.array_equal(_bits(a), _bits(b)), (shape_name, kind, name)
            assert np.array_equal(_bits(one['parts']), _bits(unset['parts']))
