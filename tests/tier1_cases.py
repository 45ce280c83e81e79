"""
Inputs that put the SpMV pair-form tier (tier 1: build_panel and its plan kernels in csrc/spmv_plan.hip, spmv_panel_kernel and
the tier's reduce in spmv_epilogue_kernel in csrc/spmv.hip) on the edges of its column blocks, tiles, carries and workgroup
list, and the NumPy restatement of how the plan lays the tier out (`Layout`).  No GPU imports and nothing from the library:
tests/test_tier1_cases_host.py checks that every case reaches the edges it claims; tests/test_gpu_spmv_tier1.py runs the
library on the same cases and compares csrk_spmv_plan_stats with the model field by field before any value is compared.

The layout, restated.  Inputs: row pointers, columns, heavy_min (CSRK_HEAVY_MIN, at least 64), tier1_min (CSRK_TIERB_MIN) and
the constants BLOCK = 262144 columns, ITEMS = 2048 path items per tile, LONG = 64, CHUNK = 128, CARRY_ROWS = 4, STREAM_MIN =
16 blocks, STREAMS = 8 (the tiny hand-worked layouts of the host test pass smaller ones).
  cut rows     rows of at least tier1_min entries (0 < tier1_min < heavy_min) -- if every one of them has ascending columns,
               else none is (the fallback) --; tier 0 = those of at least heavy_min, tier 1 = the others, ascending
  pairs        nb = ceil(ncols / BLOCK) blocks, n tier-1 rows: pair b * n + h = the entries of tier-1 row h in block b,
               in storage order; M' = the pairs in that order
  tiles        block b is a merge path of n row ends and e_b entries: ceil((n + e_b) / ITEMS) tiles (a block without an
               entry still has its n row ends); row q of the block is finished before diagonal d when its end, the item
               ends[q] + q, lies before d.  A tile = (i0, i1, nn): pairs finished before its start / end, entries in it
  carries      a tile that ends before the last pair (i1 < pairs) leaves the sum of what it holds of pair i1 -- possibly
               nothing: the last tile of block b < nb - 1 ends ON pair (b + 1) * n -- as a carry of tier-1 row i1 % n.  The
               first ncs = min(most carries of a row, CARRY_ROWS) carries of a row go to carry rows behind the block partials,
               the others are listed (crp / cidx)
  groups       one workgroup per tile; below STREAM_MIN blocks in tile order, from there on STREAMS streams (block b in stream
               b % STREAMS) interleaved, the shorter streams filled up with padding groups
  reduce       y[row h] = (sum of the block partials: two wavefronts take half of the blocks each, in order, from 0.0, and
               are joined in order) + the carry rows in order + the listed carries in tile order

The order of one pair's sum, and the bit-exact set.  A pair that no tile boundary cuts is summed by ONE tile: if it has fewer
than LONG entries, left to right from 0.0 (ordered_sum); from LONG entries on by a wavefront -- lane l adds entries l, l + 64,
.. from 0.0, then v[l] += v[l + off] for off = 32, 16, .. 1 (wave_sum) -- which is NOT the sequential loop's order but is a
fixed one: `pair_sum` restates both.  A tier-1 row whose entries all lie in one such pair gets that sum plus zeros only
(0.0 of its empty pairs, 0.0 of carries that are empty sums, -0.0 of untouched carry slots), so its y equals pair_sum of
its products bit for bit.  `Layout.exact_rows` names these rows and says which of the two orders each one has.

How many LONG segments one tile can hold: a tile of nr row ends has nr + 1 segments; all of them LONG needs 64 (nr + 1) + nr <=
2048, so nr <= 30: 31 segments (the tail of a row, 29 whole pairs of 64 and the head of the next row, 81 entries each -- case
'long-31'), three below the kernel's table of MERGE_MAXLONG = 34.  (31 WHOLE pairs of 64 between two such ends do not fit a tile.)

Every case is built from a generator seeded with zlib.crc32 of its name and carries `claims`: census entry -> predicate.
"""
import functools
import zlib

import numpy as np

BLOCK, ITEMS, LONG, CHUNK, CARRY_ROWS, STREAM_MIN, STREAMS, WAVE = 262144, 2048, 64, 128, 4, 16, 8, 64
HEAVY_FLOOR = 64      # CSRK_HEAVY_MIN below this is read as this

STAT_KEYS = ('cut_rows', 't0_rows', 't1_rows', 't1_pairs', 't1_entries', 't1_min', 't1_block_width',
             't1_blocks', 't1_tiles', 't1_carry_rows', 't1_listed_carries', 't1_groups', 't1_pad_groups')


def cdiv(a, b):
    return -(-int(a) // int(b))


def slot_of_rank(rank, nn, chunk=CHUNK):
    "panel_slot_of_rank: where the entry of column rank `rank` of a tile of nn entries is stored"
    c, i = rank // chunk, rank % chunk
    if (c + 1) * chunk > nn:
        return rank
    return c * chunk + (2 * i if i < chunk // 2 else 2 * (i - chunk // 2) + 1)


def pair_sum(p):
    "the sum one tile gives a whole pair of products p (float64, storage order): see the module docstring"
    p = np.asarray(p, dtype=np.float64)
    if len(p) < LONG:
        acc = 0.0
        for v in p:
            acc = acc + v
        return np.float64(acc)
    q = np.zeros(cdiv(len(p), WAVE) * WAVE)
    q[:len(p)] = p                                           # (x + 0.0 = x: the lanes start from 0.0, so no -0.0 is lost)
    v = np.zeros(WAVE)
    for row in q.reshape(-1, WAVE):
        v = v + row
    off = WAVE // 2
    while off:
        v[:off] = v[:off] + v[off:2 * off]
        off //= 2
    return np.float64(v[0])


class Layout:
    "tier 1 of a matrix as build_heavy_split and build_panel lay it out"

    def __init__(self, rowptrs, colinds, ncols, heavy_min, tier1_min, block=BLOCK, items=ITEMS, carry_rows=CARRY_ROWS,
                 stream_min=STREAM_MIN, streams=STREAMS, long=LONG, chunk=CHUNK):
        rp = np.asarray(rowptrs, dtype=np.int64)
        ci = np.asarray(colinds, dtype=np.int64)
        lens = np.diff(rp)
        nrows = len(lens)
        self.block, self.items, self.long, self.chunk = block, items, long, chunk
        heavy_min = max(int(heavy_min), HEAVY_FLOOR)
        tier1 = 0 < tier1_min < heavy_min
        cut_min = tier1_min if tier1 else heavy_min
        erow = np.repeat(np.arange(nrows, dtype=np.int64), lens)
        cand = np.flatnonzero(lens >= cut_min) if (nrows and len(ci) >= cut_min) else np.zeros(0, dtype=np.int64)
        down = np.flatnonzero((np.diff(ci) < 0) & (erow[1:] == erow[:-1]))
        self.fallback = bool(len(cand) and np.any(lens[erow[down]] >= cut_min))
        if self.fallback:
            cand = cand[:0]
        self.cut = cand
        self.t0 = cand[lens[cand] >= heavy_min]
        self.t1 = cand[lens[cand] < heavy_min] if tier1 else cand[:0]
        self.t1_min = int(tier1_min) if len(cand) else 0
        self.nnz_light = int(lens.sum() - lens[cand].sum())
        n = self.n = len(self.t1)
        nb = self.nb = cdiv(max(ncols, 1), block) if n else 0
        pairs = self.pairs = n * nb
        # the pairs
        hof = np.full(nrows, -1, dtype=np.int64)
        hof[self.t1] = np.arange(n)
        keep = hof[erow] >= 0
        self.ecol, self.eh = ci[keep], hof[erow[keep]]
        self.cnt = np.bincount((self.ecol // block) * n + self.eh, minlength=pairs).astype(np.int64) if n else np.zeros(0, dtype=np.int64)
        self.prp = np.concatenate([[0], np.cumsum(self.cnt)]).astype(np.int64)
        self.mcol = self.ecol[np.argsort((self.ecol // block) * n + self.eh, kind='stable')]      # the columns of M', in its order
        self.entries = int(self.prp[-1])
        # the tiles, block by block
        blk, i0, i1, nn, j0, first = [], [], [], [], [], [0]
        for b in range(nb):
            ends = self.prp[b * n + 1:(b + 1) * n + 1] - self.prp[b * n]
            total = n + int(ends[-1])
            nt = cdiv(total, items)
            d = np.minimum(np.arange(nt + 1, dtype=np.int64) * items, total)
            c = np.searchsorted(ends + np.arange(n) + 1, d, side='right')
            blk.append(np.full(nt, b, dtype=np.int64))
            i0.append(b * n + c[:-1])
            i1.append(b * n + c[1:])
            j0.append(self.prp[b * n] + d[:-1] - c[:-1])
            nn.append((d[1:] - c[1:]) - (d[:-1] - c[:-1]))
            first.append(first[-1] + nt)
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
        self.t_blk, self.t_i0, self.t_i1, self.t_nn, self.t_j0 = cat(blk), cat(i0), cat(i1), cat(nn), cat(j0)
        self.blk_tile0 = np.array(first, dtype=np.int64)
        self.n_tiles = len(self.t_blk)
        # the carries: per tier-1 row, the tiles that leave one, in tile order
        self.carry_tiles = [[] for _ in range(n)]
        for t in np.flatnonzero(self.t_i1 < pairs):
            self.carry_tiles[int(self.t_i1[t]) % n].append(int(t))
        self.row_carries = np.array([len(c) for c in self.carry_tiles], dtype=np.int64)
        self.ncs = min(int(self.row_carries.max()), carry_rows) if n else 0
        self.row_listed = np.maximum(self.row_carries - self.ncs, 0)
        self.listed = int(self.row_listed.sum())
        # the workgroup list: (first tile, tiles, block); a padding group is (0, 0, 0)
        per_block = [[(int(t), 1, b) for t in range(first[b], first[b + 1])] for b in range(nb)]
        if nb < stream_min:
            self.groups = [g for gs in per_block for g in gs]
        else:
            st = [[g for b in range(q, nb, streams) for g in per_block[b]] for q in range(streams)]
            longest = max(len(s) for s in st)
            self.groups = [st[q][i] if i < len(st[q]) else (0, 0, 0) for i in range(longest) for q in range(streams)]
        self.pad_groups = sum(1 for g in self.groups if g[1] == 0)

    def stats(self):
        "what csrk_spmv_plan_stats must report under these names (csr_amd.kernels.hip.SPMV_PLAN_STATS)"
        on = self.n > 0
        return dict(cut_rows=len(self.cut), t0_rows=len(self.t0), t1_rows=self.n, t1_pairs=self.pairs, t1_entries=self.entries,
                    t1_min=self.t1_min, t1_block_width=self.block if on else 0, t1_blocks=self.nb, t1_tiles=self.n_tiles,
                    t1_carry_rows=self.ncs, t1_listed_carries=self.listed, t1_groups=len(self.groups), t1_pad_groups=self.pad_groups)

    def tile_segments(self, t):
        "entries of each of the tile's nr + 1 segments: the pairs that end in it, then what it holds of pair i1"
        a, b = int(self.t_i0[t]), int(self.t_i1[t])
        rend = np.concatenate([self.prp[a + 1:b + 1] - self.t_j0[t], [self.t_nn[t]]])
        return np.diff(np.concatenate([[0], rend]))

    def exact_rows(self):
        "(matrix rows, pair longer than LONG - 1) of the tier-1 rows held by one pair that one tile sums whole"
        rows, is_long = [], []
        if not self.n:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
        by_row = self.cnt.reshape(self.nb, self.n)
        for h in np.flatnonzero(np.sum(by_row > 0, axis=0) == 1):
            b = int(np.argmax(by_row[:, h] > 0))
            i = b * self.n + h
            t = self.blk_tile0[b] + int(np.searchsorted(self.t_i1[self.blk_tile0[b]:self.blk_tile0[b + 1]], i, side='right'))
            assert self.t_i0[t] <= i < self.t_i1[t]
            if self.prp[i] >= self.t_j0[t]:
                rows.append(int(self.t1[h]))
                is_long.append(bool(self.cnt[i] >= self.long))
        return np.array(rows, dtype=np.int64), np.array(is_long, dtype=bool)

    def census(self):
        "the edges this layout reaches"
        nr = self.t_i1 - self.t_i0
        nn = self.t_nn
        off = self.ecol % self.block
        e_b = np.array([self.prp[(b + 1) * self.n] - self.prp[b * self.n] for b in range(self.nb)], dtype=np.int64)
        longs = [int(np.sum(self.tile_segments(t) >= self.long)) for t in range(self.n_tiles)]
        ex_rows, ex_long = self.exact_rows()
        c = dict(self.stats())
        c.update(nnz_light=self.nnz_light, fallback=int(self.fallback),
                 tiles_nr0=int(np.sum(nr == 0)), tiles_nn0=int(np.sum(nn == 0)), tiles_nn1=int(np.sum(nn == 1)),
                 tiles_nn_odd=int(np.sum(nn % 2 == 1)), tiles_nn_lt_chunk=int(np.sum((nn > 0) & (nn < self.chunk))),
                 tiles_nn_chunk=int(np.sum(nn == self.chunk)), tiles_nn_chunk1=int(np.sum(nn == self.chunk + 1)),
                 tiles_nn_full=int(np.sum(nn == self.items)),
                 tiles_partial_last_chunk=int(np.sum((nn > self.chunk) & (nn % self.chunk != 0))),
                 tiles_most_row_ends=int(nr.max()) if self.n_tiles else 0,
                 last_nn=int(nn[-1]) if self.n_tiles else 0,
                 pairs_63=int(np.sum(self.cnt == self.long - 1)), pairs_64=int(np.sum(self.cnt == self.long)),
                 pairs_65=int(np.sum(self.cnt == self.long + 1)), longest_pair=int(self.cnt.max()) if self.pairs else 0,
                 max_long_in_tile=max(longs) if longs else 0,
                 rows_carries_4=int(np.sum(self.row_carries == 4)), rows_carries_5=int(np.sum(self.row_carries == 5)),
                 rows_carries_68=int(np.sum(self.row_carries == 68)), rows_carries_69=int(np.sum(self.row_carries == 69)),
                 rows_no_carry=int(np.sum(self.row_carries == 0)),
                 max_row_listed=int(self.row_listed.max()) if self.n else 0,
                 carries_from_blocks=max((len({int(self.t_blk[t]) for t in ts}) for ts in self.carry_tiles), default=0),
                 empty_blocks=int(np.sum(e_b == 0)), last_block_width=0,
                 col_off_0=int(np.sum(off == 0)), col_off_last=int(np.sum(off == self.block - 1)),
                 exact_rows=len(ex_rows), exact_rows_short=int(np.sum(~ex_long)), exact_rows_long=int(np.sum(ex_long)))
        return c


# ---- the cases ---------------------------------------------------------------------------------------------------------

class Case:
    def __init__(self, name, family, claims, spec):
        self.name, self.family, self.claims = name, family, claims
        self.ncols, self.heavy_min, self.tier1_min = spec['ncols'], spec['heavy_min'], spec['tier1_min']
        self.extra_env = spec.get('env', {})
        rows = spec['rows']
        lens = np.array([len(r) for r in rows], dtype=np.int64)
        self.nrows = len(rows)
        self.rowptrs = np.zeros(self.nrows + 1, dtype=np.int32)
        np.cumsum(lens, out=self.rowptrs[1:])
        self.colinds = (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)
        self.nnz = len(self.colinds)
        assert self.nnz == 0 or (self.colinds.min() >= 0 and self.colinds.max() < self.ncols)
        rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
        self.values = rng.uniform(-1, 1, size=self.nnz)
        self.x = rng.uniform(-1, 1, size=self.ncols)
        for a in (self.rowptrs, self.colinds, self.values, self.x):
            a.setflags(write=False)
        self.layout = Layout(self.rowptrs, self.colinds, self.ncols, self.heavy_min, self.tier1_min)
        self._census = None

    def census(self):
        if self._census is None:
            c = self.layout.census()
            c['last_block_width'] = self.ncols - (cdiv(self.ncols, BLOCK) - 1) * BLOCK
            self._census = c
        return self._census

    def env(self, stream=True, hot=False):
        "the environment the case runs under"
        e = dict(CSRK_SPMV_HEAVY_SPLIT='1', CSRK_HEAVY_MIN=str(self.heavy_min), CSRK_TIERB_MIN=str(self.tier1_min),
                 CSRK_SPMV_STREAM='1' if stream else '0', CSRK_SPMV_HOT='1' if hot else '0')
        if hot:
            e['CSRK_LS_STAGE'] = '1'      # the pack AND cold staging, whatever share of the light entries is cold
        e.update(self.extra_env)
        return e

    def failed_claims(self):
        c = self.census()
        return [k for k, ok in self.claims.items() if not ok(c[k])]


ENV_KEYS = ('CSRK_SPMV_HEAVY_SPLIT', 'CSRK_HEAVY_MIN', 'CSRK_TIERB_MIN', 'CSRK_SPMV_STREAM', 'CSRK_SPMV_HOT', 'CSRK_ACC_GROUPS',
            'CSRK_ACC_GROUP_ROWS', 'CSRK_LS_STAGE', 'CSRK_SPMV_FIX56', 'CSRK_SPMV_NIB')
_CASES = {}


def eq(v):
    return lambda got: got == v


def ge(v):
    return lambda got: got >= v


def case(name, family, **claims):
    def deco(fn):
        _CASES[name] = (family, claims, fn)
        return fn
    return deco


def names(*families):
    return [k for k, v in _CASES.items() if not families or v[0] in families]


@functools.lru_cache(maxsize=None)
def build(name):
    family, claims, fn = _CASES[name]
    return Case(name, family, claims, fn(np.random.default_rng(zlib.crc32(name.encode()))))


def cols(rng, lo, hi, k):
    "k ascending columns of [lo, hi): distinct where they fit, else with repeats"
    if k <= hi - lo:
        return np.sort(rng.choice(hi - lo, size=k, replace=False)) + lo
    return np.sort(rng.integers(lo, hi, size=k))


def in_blocks(rng, ncols, counts):
    "one row: counts[b] entries in block b"
    return np.concatenate([cols(rng, b * BLOCK, min((b + 1) * BLOCK, ncols), k) for b, k in sorted(counts.items()) if k])


def with_lights(rng, ncols, cut, around=True):
    "the cut rows in order, a few rows of 0..8 entries before, between and behind them"
    if not around:
        return list(cut)
    out = []
    for r in cut:
        out += [cols(rng, 0, ncols, int(rng.integers(0, 9))) for _ in range(int(rng.integers(0, 3)))]
        out.append(r)
    return [cols(rng, 0, ncols, 3)] + out + [cols(rng, 0, ncols, int(k)) for k in (0, 8, 2)]


def fit(rng, n, total, lo, hi):
    "n row lengths of lo..hi that add up to `total`"
    assert n * lo <= total <= n * hi, (n, total, lo, hi)
    lens = rng.integers(lo, hi + 1, size=n)
    while lens.sum() != total:
        k = int(rng.integers(0, n))
        step = int(np.sign(total - lens.sum()))
        if lo <= lens[k] + step <= hi:
            lens[k] += step
    return lens


def spec(ncols, rows, heavy_min, tier1_min, **env):
    return dict(ncols=ncols, rows=rows, heavy_min=heavy_min, tier1_min=tier1_min, env={k: str(v) for k, v in env.items()})


# -- row counts against the epilogue's sets of 64: one block, tier 0 empty (no rider)
def _rows_case(k):
    @case(f'rows-{k}', 'rows', t1_rows=eq(k), t0_rows=eq(0), t1_blocks=eq(1), exact_rows=ge(min(k, 10)), exact_rows_long=ge(min(k, 10)))
    def _(rng):
        return spec(5000, with_lights(rng, 5000, [cols(rng, 0, 5000, int(L)) for L in rng.integers(128, 141, size=k)]), 5000, 128)


for _k in (1, 63, 64, 65):
    _rows_case(_k)

# -- block edges: three blocks, the last one column wide
W3 = 2 * BLOCK + 1


@case('blocks-edge', 'blocks', t1_blocks=eq(3), last_block_width=eq(1), col_off_0=ge(3), col_off_last=ge(2), exact_rows=ge(10),
      exact_rows_short=ge(5), exact_rows_long=ge(5), empty_blocks=eq(0), pairs_63=ge(1), pairs_64=ge(1), pairs_65=ge(1))
def _(rng):
    edge = np.array([0, BLOCK - 1, BLOCK, 2 * BLOCK - 1, 2 * BLOCK])
    rows = [np.sort(np.concatenate([edge, cols(rng, 1, BLOCK - 1, 30), cols(rng, BLOCK + 1, 2 * BLOCK - 1, 30)])),
            in_blocks(rng, W3, {1: 90}),                                  # entirely inside block 1
            in_blocks(rng, W3, {0: 40, 2: 1}),                            # skips block 1
            in_blocks(rng, W3, {0: 63, 1: 64, 2: 1}), in_blocks(rng, W3, {0: 64, 1: 65}), in_blocks(rng, W3, {0: 65, 1: 63}),
            in_blocks(rng, W3, {2: 25})]                                  # 25 times the last block's one column
    rows += [in_blocks(rng, W3, {int(rng.integers(0, 2)): int(rng.integers(20, 64))}) for _ in range(8)]
    rows += [in_blocks(rng, W3, {int(rng.integers(0, 2)): int(rng.integers(64, 200))}) for _ in range(8)]
    rows += [in_blocks(rng, W3, {0: int(rng.integers(1, 90)), 1: int(rng.integers(20, 90)), 2: int(rng.integers(0, 2))}) for _ in range(17)]
    order = rng.permutation(len(rows))
    return spec(W3, with_lights(rng, W3, [rows[i] for i in order]), 5000, 20)


@case('blocks-empty1-40', 'blocks', t1_rows=eq(40), t1_blocks=eq(3), empty_blocks=eq(1), tiles_nn0=eq(1), exact_rows=ge(10))
def _(rng):
    rows = [in_blocks(rng, W3, {0: int(rng.integers(20, 90)), 2: int(rng.integers(0, 3))}) for _ in range(40)]
    return spec(W3, with_lights(rng, W3, rows), 5000, 20)


def _last_block(name, k):
    @case(name, 'blocks', t1_blocks=eq(3), last_block_width=eq(1), last_nn=eq(k), exact_rows=ge(10))
    def _(rng):
        """
        The one-column last block holds k = 0 or 1 tier-1 entries, the panel's last: its tile has no pair of its own and its lanes
        re-read the pair before it -- block 1's, with offsets up to 262143 that would pass the end of x against block 2's base.
        """
        rows = [in_blocks(rng, W3, {int(rng.integers(0, 2)): int(rng.integers(20, 120))}) for _ in range(20)]
        rows += [in_blocks(rng, W3, {0: int(rng.integers(1, 60)), 1: int(rng.integers(20, 60))}) for _ in range(19)]
        rows.append(np.concatenate([in_blocks(rng, W3, {0: 30}), np.arange(2 * BLOCK - 40, 2 * BLOCK), [2 * BLOCK] * k]).astype(np.int64))
        return spec(W3, with_lights(rng, W3, rows), 5000, 20)


_last_block('blocks-last-nn0', 0)
_last_block('blocks-last-nn1', 1)


@case('blocks-empty1-2100', 'many', t1_rows=eq(2100), empty_blocks=eq(1), tiles_nn0=eq(2), tiles_most_row_ends=eq(ITEMS),
      t1_entries=eq(2100 * 128))
def _(rng):
    "2100 rows of 128 entries, none in block 1: its two tiles hold row ends only, the first 2048 of them (eight per lane)"
    rows = [in_blocks(rng, W3, {0: 128 - k, 2: k}) for k in rng.integers(0, 2, size=2100)]
    return spec(W3, with_lights(rng, W3, rows), 5000, 128)


# -- tile edges: one block
def _tile_total(total, n):
    @case(f'tile-{total}', 'tiles', t1_blocks=eq(1), t1_tiles=eq(cdiv(total, ITEMS)), exact_rows=ge(10),
          **({'tiles_nn0': eq(1)} if total == 2049 else {}))
    def _(rng):
        return spec(5000, with_lights(rng, 5000, [cols(rng, 0, 5000, int(L)) for L in fit(rng, n, total - n, 20, 190)]), 5000, 20)


for _t, _n in ((2047, 24), (2048, 24), (2049, 24), (4096, 40)):
    _tile_total(_t, _n)


def _tile_cut(name, items_before, **claims):
    @case(name, 'tiles', t1_tiles=eq(2), exact_rows=ge(10), **claims)
    def _(rng):
        "the first 20 rows and their ends take `items_before` path items; the tile boundary is item 2048"
        lens = list(fit(rng, 20, items_before - 20, 20, 190)) + list(rng.integers(20, 100, size=12))
        return spec(5000, with_lights(rng, 5000, [cols(rng, 0, 5000, int(L)) for L in lens]), 5000, 20)


_tile_cut('tile-cut-row-end', 2048)            # tile 0 ends with a row's end: the carry is an empty sum
_tile_cut('tile-cut-one-in', 2047)             # ... one entry into the next row
_tile_cut('tile-cut-one-before', 2050)         # ... one entry before a row's end


def _tile_last(nn):
    @case(f'tile-last-{nn}', 'tiles', t1_tiles=eq(2), last_nn=eq(nn), exact_rows=ge(10),
          **({'tiles_nn1': eq(1)} if nn == 1 else {'tiles_nn_chunk': eq(1)} if nn == 128 else {'tiles_nn_chunk1': eq(1)} if nn == 129 else {}))
    def _(rng):
        "14 rows take 1500 path items; the last row begins in tile 0 and leaves nn entries and its end to tile 1"
        lens = list(fit(rng, 14, 1500 - 14, 20, 190)) + [2049 + nn - 1500 - 1]
        return spec(5000, with_lights(rng, 5000, [cols(rng, 0, 5000, int(L)) for L in lens]), 5000, 20)


for _nn in (1, 127, 128, 129, 1025):
    _tile_last(_nn)


# -- long pairs
@case('long-63-64-65', 'long', pairs_63=ge(1), pairs_64=ge(1), pairs_65=ge(1), t1_blocks=eq(2))
def _(rng):
    W = 2 * BLOCK
    rows = [in_blocks(rng, W, {0: 63, 1: 64}), in_blocks(rng, W, {0: 64, 1: 65}), in_blocks(rng, W, {0: 65, 1: 63})]
    rows += [in_blocks(rng, W, {0: int(rng.integers(0, 80)), 1: int(rng.integers(20, 80))}) for _ in range(10)]
    return spec(W, with_lights(rng, W, rows), 5000, 20)


@case('long-31', 'long', max_long_in_tile=eq(31), tiles_nr0=eq(1), pairs_64=eq(29), t1_tiles=eq(3))
def _(rng):
    "tile 0 = 2048 entries of row A; tile 1 = A's last 81 entries and end, 29 pairs of 64 with their ends, the first 81 entries of Z"
    lens = [ITEMS + 81] + [64] * 29 + [81 + 500]
    return spec(5000, with_lights(rng, 5000, [cols(rng, 0, 5000, L) for L in lens], around=False) + [cols(rng, 0, 5000, 5)], 5000, 20)


@case('long-4000', 'long', longest_pair=eq(4000), tiles_nr0=ge(3), t1_rows=eq(3))
def _(rng):
    return spec(5000, with_lights(rng, 5000, [cols(rng, 0, 5000, 4000) for _ in range(3)]), 5000, 128)


# -- tiles inside one pair, and the carry-row limit
def _carry(name, lens, ncols=20000, **claims):
    @case(name, 'carry', **claims)
    def _(rng):
        return spec(ncols, with_lights(rng, ncols, [cols(rng, 0, ncols, L) for L in lens], around=False) + [cols(rng, 0, ncols, 4)], 10 ** 6, 128)


_carry('carry-4', [9000], rows_carries_4=eq(1), t1_carry_rows=eq(4), t1_listed_carries=eq(0), tiles_nr0=eq(4))
_carry('carry-5', [11000], rows_carries_5=eq(1), t1_carry_rows=eq(4), t1_listed_carries=eq(1), tiles_nr0=eq(5))
_carry('carry-5-5', [11000, 11000], rows_carries_5=eq(2), t1_carry_rows=eq(4), t1_listed_carries=eq(2))


@case('carry-two-blocks', 'carry', rows_carries_5=eq(1), t1_carry_rows=eq(4), t1_listed_carries=eq(1), carries_from_blocks=eq(2))
def _(rng):
    "one row, 5500 entries in each of two blocks: two carries of block 0, the empty one of its last tile, two of block 1"
    W = 2 * BLOCK
    return spec(W, with_lights(rng, W, [in_blocks(rng, W, {0: 5500, 1: 5500})]), 10 ** 6, 128)


# -- listed carries across the epilogue's batch of 64: a 300-entry row, the long one, (a row with five)
def _listed(name, big, five, **claims):
    @case(name, 'listed', t1_carry_rows=eq(4), rows_no_carry=eq(1), t1_blocks=eq(1), **claims)
    def _(rng):
        lens = [300, big] + ([10500] if five else [])
        return spec(200000, with_lights(rng, 200000, [cols(rng, 0, 200000, L) for L in lens]), 10 ** 6, 128)


_listed('listed-64', 139500, False, rows_carries_68=eq(1), max_row_listed=eq(64), t1_listed_carries=eq(64))
_listed('listed-65', 141548, False, rows_carries_69=eq(1), max_row_listed=eq(65), t1_listed_carries=eq(65))
_listed('listed-64-and-5', 139500, True, rows_carries_68=eq(1), rows_carries_5=eq(1), max_row_listed=eq(64), t1_listed_carries=eq(65))
_listed('listed-65-and-5', 141548, True, rows_carries_69=eq(1), rows_carries_5=eq(1), max_row_listed=eq(65), t1_listed_carries=eq(66))


# -- group order: the plain order against the eight streams
def _groups(name, ncols, **claims):
    @case(name, 'groups', empty_blocks=eq(1), **claims)
    def _(rng):
        "40 rows over every block but block 5, two rows of 2300 entries in block 3 (three tiles); the other blocks one tile each"
        def spread(k):
            c = cols(rng, 0, ncols - BLOCK, k)
            return np.where(c >= 5 * BLOCK, c + BLOCK, c)
        rows = [spread(int(rng.integers(150, 250))) for _ in range(40)]
        rows[7:7] = [in_blocks(rng, ncols, {3: 2300}), in_blocks(rng, ncols, {3: 2300, cdiv(ncols, BLOCK) - 1: 3})]
        return spec(ncols, with_lights(rng, ncols, rows), 5000, 128)


_groups('groups-15', 15 * BLOCK, t1_blocks=eq(15), t1_tiles=eq(17), t1_groups=eq(17), t1_pad_groups=eq(0))
_groups('groups-16', 16 * BLOCK - 7, t1_blocks=eq(16), t1_tiles=eq(18), t1_groups=eq(32), t1_pad_groups=eq(14), last_block_width=eq(BLOCK - 7))
_groups('groups-17', 17 * BLOCK, t1_blocks=eq(17), t1_tiles=eq(19), t1_groups=eq(32), t1_pad_groups=eq(13))


# -- many rows
@case('many-257', 'many', t1_rows=eq(257), t1_blocks=eq(3), exact_rows=ge(10))
def _(rng):
    W = 2 * BLOCK + 1000
    rows = [in_blocks(rng, W, {0: int(rng.integers(0, 30)), 1: int(rng.integers(20, 40)), 2: int(rng.integers(0, 5))}) for _ in range(247)]
    rows += [in_blocks(rng, W, {int(rng.integers(0, 3)): int(rng.integers(20, 100))}) for _ in range(10)]
    return spec(W, with_lights(rng, W, rows), 5000, 20)


# -- the rider: tier 0's reduce inside the pair kernel's launch (the tile-edge shape beside k tier-0 rows)
def _rider(name, k, **env):
    @case(name, 'rider', t0_rows=eq(k), t1_rows=eq(30), t1_tiles=eq(2), exact_rows=ge(10))
    def _(rng):
        "30 tier-1 rows of 20..190 entries that fill two tiles, k tier-0 rows of 300..400, some of them next to tier-1 rows"
        rows = [cols(rng, 0, 5000, int(L)) for L in fit(rng, 30, 3000, 20, 190)]
        mixed = with_lights(rng, 5000, rows)
        for _ in range(k):
            mixed.insert(int(rng.integers(0, len(mixed) + 1)), cols(rng, 0, 5000, int(rng.integers(300, 401))))
        return spec(5000, mixed, 300, 20, **env)


_rider('rider-0', 0)
_rider('rider-1', 1)
_rider('rider-64', 64)
_rider('rider-65', 65)
_rider('rider-2x65', 130, CSRK_ACC_GROUPS=2, CSRK_ACC_GROUP_ROWS=65)


# -- neighbours
@case('first-last', 'neighbours', t1_rows=eq(12))
def _(rng):
    "a tier-1 row as the matrix's first row and as its last"
    mid = with_lights(rng, 5000, [cols(rng, 0, 5000, int(L)) for L in rng.integers(20, 200, size=10)])
    return spec(5000, [cols(rng, 0, 5000, 77)] + mid + [cols(rng, 0, 5000, 130)], 5000, 20)


@case('all-tier1', 'neighbours', t1_rows=eq(30), nnz_light=eq(0))
def _(rng):
    return spec(5000, [cols(rng, 0, 5000, int(L)) for L in rng.integers(20, 200, size=30)], 5000, 20)


@case('next-to-tier0', 'neighbours', t1_rows=eq(8), t0_rows=eq(4))
def _(rng):
    "tier-1 and tier-0 rows alternate without a light row between them"
    lens = [50, 400, 120, 130, 350, 299, 300, 20, 64, 500, 63, 65]
    return spec(5000, [cols(rng, 0, 5000, 2)] + [cols(rng, 0, 5000, L) for L in lens] + [cols(rng, 0, 5000, 7)], 300, 20)


# -- fallback
@case('fallback', 'fallback', fallback=eq(1), cut_rows=eq(0), t1_rows=eq(0), t1_tiles=eq(0))
def _(rng):
    "one long row with a descending pair of columns: the split is dropped"
    rows = [cols(rng, 0, 5000, int(L)) for L in rng.integers(20, 200, size=8)]
    bad = cols(rng, 0, 5000, 200)
    bad[[100, 101]] = bad[[101, 100]]
    rows.insert(5, bad)
    return spec(5000, with_lights(rng, 5000, rows), 5000, 20)


# the three families the stream-off / pack-on variants and the non-finite x run on
EDGE_FAMILIES = ('blocks', 'tiles', 'rider')
