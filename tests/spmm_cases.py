"""
Inputs that put the dense-panel SpMM (csrc/spmm_dense.hip: spmm_seg_kernel and spmm_fixup_kernel for the light rows,
build_hrows, spmm_hrows_kernel and spmm_hrows_reduce_kernel for the heavy ones) on the edges of its segments, buckets, tiles
and column ranges, and the NumPy restatement of its plan (`Plan`) and of the order of its sums (`product`).  No GPU imports
and nothing from the library: tests/test_spmm_cases_host.py checks that every case reaches the edges it claims and that the
bit comparison is not vacuous; tests/test_spmm_plan_host.py compares `Plan` on every case with the library's own plan
arithmetic (csrc/spmm_plan.h, which build_hrows and spmm_device call) in a host program; tests/test_gpu_spmm_edges.py runs
the library on the same cases and compares csrk_spmm_plan_stats and the range table with the model before any value is
compared.

The plan, restated.  Inputs: row pointers, columns, ncols, the panel width k of the handle's first product, the switch
CSRK_SPMM_HEAVY ('0', '1' or None), CSRK_SPMM_HEAVY_GROUPS, the device's CU count and the constants SEG = 64 entries per
segment, HR_ROWS = 512 rows per workgroup (WAVES = 16 wavefronts of RPW = 32 rows), TILE = 128 rows of B, MAXG = 8 row groups,
the floor of 256 (forced) or 512 entries (the tiny hand-worked layouts of the host test pass smaller ones).
  engage       the heavy form is tried when the switch is '1', or when it is not '0' and ncols * k * 8 > 64 MiB
  candidates   rows of at least `floor` entries, longest first, then by row id
  groups       512 candidates at a time while 4 * (the group's entries) >= 5 * ncols (forced: the first group always;
               CSRK_SPMM_HEAVY_GROUPS = g: g groups, or as many as there are candidates for)
  threshold    hr_min = the length of the last candidate taken; the rows as long come along when all fit G * 512, else
               hr_min moves up by one and the rows shorter than it are dropped -- down to none, which switches the form off;
               then G shrinks while G - 1 groups hold all rows
  places       heavy row of rank i: group i % G, wavefront (i // G) % 16, slot (i // G) // 16
  buckets      (tile, group, wavefront) -> the entries of that wavefront's rows with col // 128 = tile, stably by rank
  R            min(max(cus, G) // G, tiles), rounded down to a multiple of 8 from 8 on; spmm_hrows_kernel maps a workgroup
               to (range, group) by XCD when R is a multiple of 8, else by blockIdx / G, blockIdx % G (`wg_place`)
  ranges       range[q], 0 < q < R: the first tile t whose cumulative cost, entries before tile t + 1 plus 200 G per tile,
               exceeds q / R of the total; clamped to range[q - 1] + 1 from below and tiles - (R - q) from above (float arithmetic)
  light rows   a row that is not heavy has one segment up to 64 entries (an empty row too), else ceil(len / 64); n_segs,
               n_multi (segments of rows with more than one) and n_split (those rows)

The order of the sums (`product`).  A row of one segment: left to right from 0.0.  A split row: each segment from 0.0, then
the partials in segment order from 0.0.  A heavy row: its entries stably sorted by col // 128, one partial per column range
from 0.0, then the R partials in range order from 0.0.  The heavy kernel multiplies and adds fused, the light kernel may or
may not: the bit-exact inputs (`exact_values`) are 24-bit integers times 2^e, e uniform in -30 .. -11, so every product is
exact and both give the same bits, while the sums still round -- over mixed exponents, so their order shows.

Every case is built from a generator seeded with zlib.crc32 of its name and carries `claims`: what it says it reaches ->
whether the model agrees.
"""
import functools
import zlib

import numpy as np

SEG, UNIT, CHUNK, HR_ROWS, RPW, WAVES, TILE, KC, BATCH, MAXG, WAVE = 64, 16, 64, 512, 32, 16, 128, 64, 8, 8, 64
FLOOR_FORCED, FLOOR = 256, 512
TILE_COST = 200               # a tile's fixed cost in entries, per row group
ENGAGE_BYTES = 64 << 20
CUS = 256                     # the CU count the claims are worked out for (MI355X); the GPU test passes the device's own
ENV_KEYS = ('CSRK_SPMM_HEAVY', 'CSRK_SPMM_HEAVY_GROUPS')
STAT_KEYS = ('on', 'hr_min', 'hr_n', 'G', 'R', 'hr_nnz', 'tiles', 'n_segs', 'n_multi')


def cdiv(a, b):
    return -(-int(a) // int(b))


def engage(ncols, k, mode):
    "spmmplan::heavy_engaged: is the heavy form tried at all (mode: CSRK_SPMM_HEAVY)"
    return mode != '0' and (mode == '1' or int(ncols) * int(k) * 8 > ENGAGE_BYTES)


def wg_place(b, G, R, by_xcd=None):
    "spmm_hrows_kernel: workgroup b of a grid of G R -> (range, group)"
    if by_xcd is None:
        by_xcd = (R & 7) == 0                            # the kernel's (gridDim.x / G) & 7, gridDim.x = G R
    return ((b & 7) + 8 * ((b >> 3) // G), (b >> 3) % G) if by_xcd else (b // G, b % G)


class Plan:
    "the dense-panel plan of a matrix as build_hrows (spmmplan::choose_heavy, balance_ranges) and build_mm_plan make it"

    def __init__(self, rowptrs, colinds, ncols, k, mode, groups=0, cus=CUS, hr_rows=HR_ROWS, waves=WAVES, tile=TILE, seg=SEG,
                 maxg=MAXG, floor=None, tile_cost=TILE_COST):
        self.rp = rp = np.asarray(rowptrs, dtype=np.int64)
        self.ci = np.asarray(colinds, dtype=np.int64)
        self.lens = lens = np.diff(rp)
        self.nrows, self.ncols, self.tile, self.waves, self.seg = len(lens), int(ncols), tile, waves, seg
        self.on, self.hr_min, self.G, self.R, self.hr_nnz, self.tiles = False, 0, 0, 0, 0, 0
        self.rows = np.zeros(0, dtype=np.int64)
        self.range = np.zeros(0, dtype=np.int64)
        self.clamp, self.tie, self.G_before_shrink = {}, None, 0
        if engage(ncols, k, mode) and self.nrows and ncols >= 1 and len(self.ci):
            self._heavy(mode == '1', int(groups), cus, hr_rows, maxg, (FLOOR_FORCED if mode == '1' else FLOOR) if floor is None else floor,
                        tile_cost)
        heavy = lens >= self.hr_min if self.on else np.zeros(self.nrows, dtype=bool)
        self.segs = np.where(heavy, 0, np.where(lens <= seg, 1, -(-lens // seg)))
        self.n_segs = int(self.segs.sum())
        self.n_multi = int(self.segs[self.segs > 1].sum())
        self.n_split = int(np.sum(self.segs > 1))

    def _heavy(self, force, groups, cus, hr_rows, maxg, floor, tile_cost):
        lens, ncols, tile, waves = self.lens, self.ncols, self.tile, self.waves
        cand = np.flatnonzero(lens >= floor)
        if not len(cand):
            return
        cand = cand[np.lexsort((cand, -lens[cand]))]
        G = taken = 0
        while G < maxg and taken < len(cand):
            end = min(len(cand), taken + hr_rows)
            gn = int(lens[cand[taken:end]].sum())
            pays = gn * 4 >= 5 * ncols
            if (G >= groups) if groups > 0 else (not pays and not (force and G == 0)):
                break
            taken = end
            G += 1
        if G == 0:
            return
        hmin = int(lens[cand[taken - 1]])
        n = taken
        while n < len(cand) and lens[cand[n]] >= hmin:
            n += 1
        self.tie = 'fit'
        if n > G * hr_rows:
            self.tie = 'move'
            hmin += 1
            n = taken
            while n > 0 and lens[cand[n - 1]] < hmin:
                n -= 1
        if n == 0:
            self.tie = 'off'
            return
        cand = cand[:n]
        nnz_h = int(lens[cand].sum())
        self.G_before_shrink = G
        while G > 1 and (G - 1) * hr_rows >= n:
            G -= 1
        n_tiles = cdiv(ncols, tile)
        R = min(max(cus, G) // G, n_tiles)
        if R >= 8:
            R = R // 8 * 8
        n_buckets = n_tiles * G * waves
        if n_buckets >= 1 << 30 or (not force and n_buckets * 8 > nnz_h * 12):
            return
        # places, entries in (rank, storage) order, buckets
        i = np.arange(n, dtype=np.int64)
        self.group, self.wave, self.slot = i % G, (i // G) % waves, (i // G) // waves
        hl = lens[cand]
        self.h_rank = np.repeat(i, hl)
        self.h_entry = np.repeat(self.rp[cand] - np.concatenate([[0], np.cumsum(hl)[:-1]]), hl) + np.arange(nnz_h, dtype=np.int64)
        self.h_tile = self.ci[self.h_entry] // tile
        key = (self.h_tile * G + self.group[self.h_rank]) * waves + self.wave[self.h_rank]
        self.bucket_len = np.bincount(key, minlength=n_buckets).reshape(n_tiles, G, waves)
        tot = np.concatenate([[0], np.cumsum(np.bincount(self.h_tile, minlength=n_tiles))])
        # column ranges: the loop of spmmplan::balance_ranges, literally (float arithmetic)
        tile_cost = tile_cost * G
        total_cost = float(nnz_h) + float(tile_cost) * float(n_tiles)
        rng_ = [0] * (R + 1)
        t = 0
        for q in range(1, R):
            goal = total_cost * q / R
            while t < n_tiles and float(tot[t + 1]) + float(tile_cost) * float(t + 1) <= goal:
                t += 1
            if t < rng_[q - 1] + 1:
                self.clamp[q] = 'low'
            t = max(t, rng_[q - 1] + 1)
            if t > n_tiles - (R - q):
                self.clamp[q] = 'high'
            t = min(t, n_tiles - (R - q))
            rng_[q] = t
        rng_[R] = n_tiles
        self.range = np.array(rng_, dtype=np.int64)
        self.on, self.hr_min, self.rows, self.G, self.R, self.hr_nnz, self.tiles = True, hmin, cand, G, R, nnz_h, n_tiles

    @property
    def hr_n(self):
        return len(self.rows)

    def stats(self):
        "the nine fields of csrk_spmm_plan_stats, in its order"
        return [int(self.on), self.hr_min, self.hr_n, self.G, self.R, self.hr_nnz, self.tiles, self.n_segs, self.n_multi]

    def by_xcd(self):
        return self.on and (self.R & 7) == 0


def seq_sums(prod, start, length):
    "out[s] = prod[start[s]] + prod[start[s] + 1] + .. (length[s] addends), left to right from 0.0; prod is [N, k]"
    start, length = np.asarray(start, dtype=np.int64), np.asarray(length, dtype=np.int64)
    acc = np.zeros((len(start), prod.shape[1]))
    if not len(start) or not length.max():
        return acc
    order = np.argsort(-length, kind='stable')
    s, l = start[order], length[order]
    live = len(s) - np.cumsum(np.bincount(l))            # live[j] = sequences longer than j: a prefix of the sorted ones
    for j in range(int(l[0])):
        na = live[j]
        acc[:na] = acc[:na] + prod[s[:na] + j]
    out = np.empty_like(acc)
    out[order] = acc
    return out


def product(plan, values, B, ranges=None):
    "C = A B in the order of the kernels' sums (module docstring); `ranges`: another range table than the plan's"
    rp, ci = plan.rp, plan.ci
    v = np.ones(len(ci)) if values is None else np.asarray(values).astype(np.float64)
    prod = v[:, None] * np.asarray(B, dtype=np.float64)[ci]
    Cm = np.zeros((plan.nrows, B.shape[1]))
    rows = np.flatnonzero(plan.segs >= 1)
    ns = plan.segs[rows]
    first = np.concatenate([[0], np.cumsum(ns)])
    seg_row = np.repeat(rows, ns)
    start = rp[seg_row] + (np.arange(first[-1]) - np.repeat(first[:-1], ns)) * plan.seg
    s1 = seq_sums(prod, start, np.minimum(plan.seg, rp[seg_row + 1] - start))
    one = ns == 1
    Cm[rows[one]] = s1[first[:-1][one]]
    Cm[rows[~one]] = seq_sums(s1, first[:-1][~one], ns[~one])
    if plan.on:
        Cm[plan.rows] = heavy_sums(plan, prod, plan.range if ranges is None else ranges)[1]
    return Cm


def heavy_sums(plan, prod, ranges):
    "(the partials [hr_n, R, k], the sums [hr_n, k]) of the heavy rows under a range table"
    ranges = np.asarray(ranges, dtype=np.int64)
    R, n = len(ranges) - 1, plan.hr_n
    order = np.lexsort((plan.h_tile, plan.h_rank))       # (stable: storage order inside a tile)
    q = np.searchsorted(ranges[1:], plan.h_tile[order], side='right')
    length = np.bincount(plan.h_rank[order] * R + q, minlength=n * R)
    part = seq_sums(prod[plan.h_entry[order]], np.concatenate([[0], np.cumsum(length)[:-1]]), length)
    return part.reshape(n, R, -1), seq_sums(part, np.arange(n) * R, np.full(n, R))


def plain_sum(plan, values, B, rows):
    "the rows' sums left to right from 0.0 in storage order: what the kernels' order is compared with"
    v = np.ones(len(plan.ci)) if values is None else np.asarray(values).astype(np.float64)
    return seq_sums(v[:, None] * np.asarray(B, dtype=np.float64)[plan.ci], plan.rp[rows], plan.lens[rows])


def exact_values(rng, n):
    "24-bit integers of either sign times 2^e, e uniform in -30 .. -11: the product of two is exact in float64"
    m = rng.integers(1, 1 << 24, size=n) * (2 * rng.integers(0, 2, size=n) - 1)
    return np.ldexp(m.astype(np.float64), rng.integers(-30, -10, size=n))


def exact_parts(x):
    "(m, e) with x = m 2^e, m a Python integer: for the host test's exactness check"
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return [int(v) for v in np.ldexp(m, 53).astype(np.int64)], [int(v) - 53 for v in e]


class Case:
    def __init__(self, name, rows, ncols, ks, mode, groups=0, sparse_panel=False):
        self.name, self.ncols, self.ks, self.mode, self.groups, self.sparse_panel = name, int(ncols), tuple(ks), mode, groups, sparse_panel
        self.family = name.split(':')[0]
        lens = np.array([len(r) for r in rows], dtype=np.int64)
        self.nrows, self.nnz = len(rows), int(lens.sum())
        self.rowptrs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        self.colinds = (np.concatenate(rows) if self.nnz else np.zeros(0)).astype(np.int32)
        assert self.nnz == 0 or (0 <= self.colinds.min() and self.colinds.max() < ncols), name
        self.lens = lens
        self.values = exact_values(self._rng('values'), self.nnz)
        self.claims, self._plans = {}, {}

    def _rng(self, what):
        return np.random.default_rng([zlib.crc32(self.name.encode()), zlib.crc32(what.encode())])

    def env(self):
        e = {} if self.mode is None else {'CSRK_SPMM_HEAVY': self.mode}
        if self.groups:
            e['CSRK_SPMM_HEAVY_GROUPS'] = str(self.groups)
        return e

    def plan(self, cus=CUS, k=None):
        "the plan a handle builds at its first product (of width k; the case's first width unless given)"
        key = (cus, self.ks[0] if k is None else k)
        if key not in self._plans:
            self._plans[key] = Plan(self.rowptrs, self.colinds, self.ncols, key[1], self.mode, self.groups, cus)
        return self._plans[key]

    def uniform_values(self):
        return self._rng('uniform').uniform(-1, 1, self.nnz)

    def panel(self, k, exact=True):
        """
        B [ncols x k]: exact_values, or full-mantissa uniform(-1, 1).  sparse_panel: only the rows of B some entry reads are
        drawn, the others are zero (the one family whose panel has 8 million values)
        """
        rng = self._rng(f'panel {k} {exact}')
        draw = (lambda n: exact_values(rng, n)) if exact else (lambda n: rng.uniform(-1, 1, n))
        if not self.sparse_panel:
            return draw(self.ncols * k).reshape(self.ncols, k)
        B = np.zeros((self.ncols, k))
        used = np.unique(self.colinds)
        B[used] = draw(len(used) * k).reshape(len(used), k)
        return B

    def failed_claims(self):
        return [c for c, ok in self.claims.items() if not ok]


# ---- the cases ------------------------------------------------------------------------------------------------------------

def _cols(rng, ncols, n, style):
    "n columns of a row: 'dup' (drawn with repeats, unsorted), 'sorted' (distinct, ascending), 'perm' (distinct, unsorted)"
    if style == 'dup' or n > ncols:
        return rng.integers(0, ncols, size=n)
    c = rng.choice(ncols, size=n, replace=False)
    return np.sort(c) if style == 'sorted' else c


def _style(i):
    return ('sorted', 'perm', 'dup')[i % 3]


BESIDE = (0, 1, 5, 64, 65, 100, 128, 129, 200, 255, 0, 17, 192, 193)


def _beside(rng, ncols, lens=BESIDE):
    "light, split (65 .. 255 entries) and empty rows that stand beside the heavy ones"
    return [_cols(rng, ncols, n, _style(i)) for i, n in enumerate(lens)]


def _interleave(heavy, beside):
    "heavy rows in their order with the other rows between them"
    out = []
    for i, h in enumerate(heavy):
        out.append(h)
        if i < len(beside):
            out.append(beside[i])
    return out + list(beside[len(heavy):])


SEG_LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64)


def _seg_lengths(name, nrows):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    lens = [SEG_LENGTHS[(5 * i) % 13] for i in range(nrows)]      # four consecutive rows: four different lengths
    lens[8:12] = [0, 0, 0, 0]                                      # a wavefront of four empty rows
    lens[12:16] = [64, 0, 1, 17]
    c = Case(name, [_cols(rng, 300, n, _style(i)) for i, n in enumerate(lens)], 300, (5, 64), '0')
    p = c.plan()
    quads = [lens[i:i + 4] for i in range(0, nrows - 3, 4)]
    c.claims = {'every length of the list occurs': set(lens) == set(SEG_LENGTHS),
                'every row is one segment': p.n_segs == nrows and p.n_multi == 0,
                'n_segs % 16 is the residue the name says': p.n_segs % 16 == int(name.split(':')[1]) and p.n_segs % 16 != 0,
                'a wavefront of four empty rows': [0, 0, 0, 0] in quads,
                'wavefronts of four unequal units': sum(len(set(q)) == 4 for q in quads) >= len(quads) - 2,
                'a wavefront whose longest unit is 64 beside an empty one': any(64 in q and 0 in q for q in quads)}
    return c


SPLIT_LENGTHS = (3, 65, 127, 40, 128, 129, 0, 192, 193, 64, 4097, 130, 66, 1, 65)


def _split(name):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    c = Case(name, [_cols(rng, 5000, n, _style(i)) for i, n in enumerate(SPLIT_LENGTHS)], 5000, (4, 67), '0')
    p = c.plan()
    L = np.array(SPLIT_LENGTHS)
    c.claims = {'rows of 65, 127, 128, 129, 192, 193 and 4097 entries': {65, 127, 128, 129, 192, 193, 4097} <= set(SPLIT_LENGTHS),
                'two split rows side by side': bool(np.any((p.segs[:-1] > 1) & (p.segs[1:] > 1))),
                'a split row is the last row': p.segs[-1] > 1,
                'last segments of one entry': int(np.sum((L > 64) & (L % 64 == 1))) >= 4,
                'unsorted and duplicate columns in split rows': any(L[i] > 64 and _style(i) == 'dup' for i in range(len(L))),
                'the census': (p.n_segs, p.n_multi, p.n_split) == (int(np.sum(np.where(L <= 64, 1, -(-L // 64)))),
                                                                  int(np.sum(np.where(L <= 64, 0, -(-L // 64)))), int(np.sum(L > 64)))}
    return c


WIDTHS = (1, 2, 3, 4, 5, 60, 63, 64, 65, 67, 68, 128, 129, 132)
WIDTHS_HEAVY = (1, 2, 63, 64, 65, 66, 127, 128, 129)


def _widths(name):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    lens = (0, 1, 5, 64, 65, 130, 17, 200, 0, 33, 129, 2)
    c = Case(name, [_cols(rng, 150, n, _style(i)) for i, n in enumerate(lens)], 150, WIDTHS, '0')
    c.claims = {'split rows, so that the partial buffer exists and grows with k': c.plan().n_multi > 0,
                'widths on both sides of 4 and of a 64-column chunk, and a second chunk of one column': {3, 4, 5, 63, 64, 65} <= set(WIDTHS)}
    return c


def _heavy_lens(rng, n, lo=256, hi=300):
    return rng.integers(lo, hi, size=n)


FEW_TILES = {100: 1, 128: 1, 129: 2, 256: 2, 257: 3, 896: 7, 897: 8, 1024: 8, 1025: 8}


def _few_tiles(name, ncols):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    heavy = [_cols(rng, ncols, n, _style(i)) for i, n in enumerate(_heavy_lens(rng, 520))]
    c = Case(name, _interleave(heavy, _beside(rng, ncols)), ncols, (3,), '1', groups=2)
    p = c.plan()
    grid = [wg_place(b, p.G, p.R) for b in range(p.G * p.R)] if p.on else []
    c.claims = {'the form is on with two row groups': p.on and p.G == 2 and p.hr_n == 520,
                'R is what the issue says': p.R == FEW_TILES[ncols],
                'the mapping by XCD exactly when R is a multiple of 8': p.by_xcd() == (FEW_TILES[ncols] == 8),
                'the mapping is one to one': sorted(grid) == [(r, g) for r in range(p.R) for g in range(p.G)],
                'below 8 ranges the mapping by XCD would be another one': p.R >= 8 or
                [wg_place(b, p.G, p.R, True) for b in range(p.G * p.R)] != grid,
                'a one-tile range everywhere up to 1024 columns (no prefetch)': ncols > 1024 or bool(np.all(np.diff(p.range) == 1)),
                'the last tile is cut or whole as the width says': (ncols % TILE != 0) == (ncols in (100, 129, 257, 897, 1025)),
                'light, split and empty rows beside': p.n_multi > 0 and p.n_segs > p.n_multi and 0 in c.lens}
    return c


PROBES = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 0)
PROBE_TILES, FILL_TILES = 6, 7


def probe_len(w, j):
    "entries of wavefront w's bucket in probe tile j (tile 1 + j): six consecutive probes, starting two further per wavefront"
    return PROBES[(2 * w + j) % len(PROBES)]


def _buckets(name, n_heavy):
    """
    One row group, heavy rows of ONE length (so the rank is the row order), 15 tiles in 8 ranges at 256 CUs.  Tile 0 is
    empty; in tiles 1 .. 6 the bucket of wavefront w holds PROBES[(2 w + j) % 15] entries, j = 0 .. 5 -- every probe length
    in some wavefront, an empty bucket straight after the one of 200 in wavefronts 5 and 6 --; tiles 7 .. 13 fill every row up
    to its length, evenly, and each outweighs tiles 0 .. 6 together; tile 14 is empty and cut by the matrix' width.  The cost
    balance then makes tiles 0 .. 6 ONE range -- every probe bucket is reached through the prefetch and handed over in the
    loop, the empty first tile is followed by six tiles --, gives tiles 7 .. 12 a range each and tiles 13 and 14 the last:
    a bucket of several hundred entries, then the empty last tile.
    """
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    n_tiles = 1 + PROBE_TILES + FILL_TILES + 1
    ncols = n_tiles * TILE - 37
    length = 1000 + 48000 // n_heavy
    heavy = []
    for r in range(n_heavy):
        w = r % WAVES
        owners = [q for q in range(n_heavy) if q % WAVES == w]
        cols = []
        for j in range(PROBE_TILES):
            L = probe_len(w, j)
            n = L // len(owners) + (1 if owners.index(r) < L % len(owners) else 0)
            cols.append((1 + j) * TILE + rng.integers(0, TILE, size=n))      # (repeats allowed: 200 entries in 128 rows of B)
        rest = length - sum(len(x) for x in cols)
        for f in range(FILL_TILES):
            n = rest // FILL_TILES + (1 if f < rest % FILL_TILES else 0)
            cols.append((1 + PROBE_TILES + f) * TILE + rng.integers(0, TILE, size=n))
        cols = np.concatenate(cols)
        heavy.append(rng.permutation(cols) if r % 2 else cols)
    c = Case(name, _interleave(heavy, _beside(rng, ncols)), ncols, (64,), '1', groups=1)
    p = c.plan()
    ok = p.on and p.G == 1 and p.hr_n == n_heavy and p.tiles == n_tiles and p.R == 8
    b = p.bucket_len[:, 0, :] if ok else np.zeros((n_tiles, WAVES), dtype=np.int64)
    rng_ = p.range.tolist() if ok else [0] * 9
    waves = min(n_heavy, WAVES)
    inside = [t for t in range(n_tiles) if t not in rng_[:-1]]               # tiles whose buckets arrive through the prefetch
    handed = {int(b[t, w]) for t in inside for w in range(waves)}
    c.claims = {'one group of the rows asked for, in row order, eight ranges': ok and bool(np.all(np.diff(p.rows) > 0)),
                'the buckets hold the probe lengths': all(b[1 + j, w] == probe_len(w, j) for j in range(PROBE_TILES) for w in range(waves)),
                'tiles 0 .. 6 are one range, tiles 13 and 14 the last': rng_[:2] == [0, 1 + PROBE_TILES] and rng_[-2:] == [n_tiles - 2, n_tiles],
                'every probe length is a bucket that is prefetched and handed over inside a range': set(PROBES) <= handed,
                'an empty bucket directly after one of 200, both inside one range':
                    any(b[t, w] == 200 and b[t + 1, w] == 0 and t in inside and t + 1 in inside for t in range(n_tiles - 1) for w in range(waves)),
                'buckets of 65, 127, 128, 129 and 200 entries are followed by a non-empty one inside the range (the later chunks read at the handed-over start)':
                    all(any(b[t, w] == L and b[t + 1, w] > 0 and t in inside and t + 1 in inside for t in range(n_tiles - 1) for w in range(waves))
                        for L in (65, 127, 128, 129)),
                'the empty first tile is followed by a tile of its range': b[0].sum() == 0 and 1 in inside,
                'the empty last tile follows a bucket of several chunks in its range': b[-1].sum() == 0 and ncols % TILE != 0 and n_tiles - 1 in inside
                    and b[-2, :waves].min() > 64,
                'wavefronts that own no row, when fewer than 16 rows': n_heavy >= WAVES or bool(np.all(b[:, n_heavy:] == 0))}
    return c


def _places(name, n_heavy, groups, ncols=2901):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    heavy = [_cols(rng, ncols, n, _style(i)) for i, n in enumerate(_heavy_lens(rng, n_heavy))]
    c = Case(name, _interleave(heavy, _beside(rng, ncols)), ncols, (2,), '1', groups=groups)
    p = c.plan()
    G = min(groups, cdiv(n_heavy, HR_ROWS))
    c.claims = {'the rows asked for, in the groups there are candidates for': p.on and p.hr_n == n_heavy and p.G == G,
                'the last slot in use is the one the count gives': p.on and int(p.slot.max()) == (cdiv(n_heavy, G) - 1) // WAVES,
                'ranks are not the row order': p.on and (n_heavy == 1 or bool(np.any(np.diff(p.rows) < 0))),
                '23 tiles in 16 ranges: the LDS tile flips': p.on and (p.tiles, p.R) == (23, 16)
                    and int(np.diff(p.range).max()) > 1}
    return c


def _ties(name, lens, groups, want):
    "heavy candidates of the lengths given (rank order), rows shuffled; `want`: (tie rule, hr_min, hr_n, G) or None = off"
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    ncols = 2901
    lens = np.asarray(lens)[rng.permutation(len(lens))]
    heavy = [_cols(rng, ncols, n, _style(i)) for i, n in enumerate(lens)]
    c = Case(name, _interleave(heavy, _beside(rng, ncols)), ncols, (2,), '1', groups=groups)
    p = c.plan()
    if want is None:
        c.claims = {'more than 512 candidates of one length under one group: the form switches itself off':
                    not p.on and p.tie == 'off' and p.stats()[:7] == [0] * 7 and p.n_split >= len(lens)}
    else:
        c.claims = {'tie rule, threshold, rows and groups': p.on and (p.tie, p.hr_min, p.hr_n, p.G) == want,
                    'candidates that stay light are split rows': p.n_split >= len(lens) - want[2],
                    'more tiles than ranges: the LDS tile flips': p.on and p.tiles > p.R and int(np.diff(p.range).max()) > 1}
        if name.endswith('shrink'):
            c.claims['G comes out smaller than forced'] = p.on and p.G < p.G_before_shrink == groups
    return c


def _ranges(name, where):
    """
    16 heavy rows over 300 tiles, two entries of every row in every tile (so every boundary between two tiles shows in the
    bits) and 3400 more per row: skewed towards the first tiles, all in the first ten, or all in the last ten
    """
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    n_tiles, ncols = 300, 38400
    heavy = []
    for r in range(16):
        base = np.repeat(np.arange(n_tiles), 2)
        if where == 'skew':
            more = np.minimum(rng.triangular(0, 0, n_tiles, size=3400).astype(np.int64), n_tiles - 1)
        else:
            more = rng.integers(0, 10, size=3400) + (0 if where == 'first' else n_tiles - 10)
        t = np.concatenate([base, more])
        cols = t * TILE + rng.integers(0, TILE, size=len(t))
        heavy.append(rng.permutation(cols) if r % 2 else cols)
    c = Case(name, _interleave(heavy, _beside(rng, ncols)), ncols, (64,), '1', groups=1)
    p = c.plan()
    w = np.diff(p.range) if p.on else np.zeros(1)
    c.claims = {'more tiles than ranges, R = 256 at 256 CUs': p.on and p.tiles == n_tiles and p.R == 256 and p.G == 1,
                'ranges of unequal numbers of tiles': len(set(w.tolist())) > 1,
                'the panel is under 20 MB': ncols * 64 * 8 < 20e6,
                {'first': 'the clamp from below binds', 'last': 'the clamp from above binds', 'skew': 'ranges of one tile and of several'}[where]:
                    {'first': 'low' in p.clamp.values(), 'last': 'high' in p.clamp.values(), 'skew': w.min() == 1 and w.max() > 1}[where]}
    return c


def _widths_heavy(name):
    """
    40 heavy rows over 23 tiles (the last one cut) in 16 ranges at 256 CUs, their columns thinning out towards the right, so
    that the light last tiles share ranges: the next tile -- the cut one too -- is loaded and stored at every width
    """
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    ncols = 2901
    heavy = []
    for i, n in enumerate(_heavy_lens(rng, 40, 256, 500)):
        cols = np.minimum(rng.triangular(0, 0, ncols, size=n).astype(np.int64), ncols - 1)
        heavy.append(np.sort(cols) if i % 2 else cols)
    c = Case(name, _interleave(heavy, _beside(rng, ncols)), ncols, WIDTHS_HEAVY, '1')
    p = c.plan()
    w = np.diff(p.range) if p.on else np.zeros(1)
    c.claims = {'40 heavy rows beside light ones': p.on and p.hr_n == 40 and p.n_multi > 0,
                '23 tiles in 16 ranges, several of more than one tile': p.on and (p.tiles, p.R) == (23, 16) and int(np.sum(w > 1)) >= 3,
                'the cut last tile is loaded as a NEXT tile': ncols % TILE != 0 and w[-1] > 1,
                'odd widths, a second launch of one column, lanes beyond the width': {1, 63, 65, 127, 129} <= set(WIDTHS_HEAVY)}
    return c


def _all_heavy(name):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    ncols = 1500
    c = Case(name, [_cols(rng, ncols, n, _style(i)) for i, n in enumerate(_heavy_lens(rng, 40, 256, 400))], ncols, (7,), '1')
    p = c.plan()
    c.claims = {'every row is heavy: no segment': p.on and p.hr_n == c.nrows and p.n_segs == 0}
    return c


def _types(name):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    ncols = 1700
    heavy = [_cols(rng, ncols, n, _style(i)) for i, n in enumerate(_heavy_lens(rng, 50, 256, 600))]
    c = Case(name, _interleave(heavy, _beside(rng, ncols)), ncols, (6,), '1')
    p = c.plan()
    c.claims = {'heavy, split and light rows': p.on and p.hr_n == 50 and p.n_multi > 0 and p.n_segs > p.n_multi,
                'the exact values are float32 numbers': bool(np.all(c.values.astype(np.float32).astype(np.float64) == c.values))}
    return c


# name -> (ncols, row lengths, on?): the smallest shapes on either side of each rule of the plan's own decision at k = 64
PAYS = 5 * 131076 // 4                                                       # 163845 entries: 4 gn = 5 ncols exactly
UNFORCED = {
    'unforced:64MiB': (131072, [1000] * 170, False),                        # ncols * 64 * 8 = 64 MiB exactly: not above
    'unforced:64MiB+1': (131073, [1000] * 170, True),
    'unforced:511': (131073, [511] * 330, False),                           # no row reaches the floor of 512
    'unforced:512': (131073, [512] * 321 + [511] * 9, True),
    'unforced:pays': (131076, [1000] * 163 + [845], True),
    'unforced:pays-1': (131076, [1000] * 163 + [844], False),
}


def _unforced(name):
    ncols, lens, on = UNFORCED[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    pool = np.unique(np.concatenate([[0, ncols - 1], rng.choice(ncols, size=6000, replace=False)]))   # (the rows of B that are read)
    heavy = [rng.choice(pool, size=n, replace=False) for n in lens]
    c = Case(name, _interleave(heavy, _beside(rng, ncols)), ncols, (64,), None, sparse_panel=True)
    p = c.plan()
    gn = int(np.sum([n for n in lens if n >= FLOOR]))
    c.claims = {'the plan decides as the rule says': p.on == on,
                'the rule in question is the one that decides': {
                    'unforced:64MiB': ncols * 64 * 8 == ENGAGE_BYTES and gn * 4 >= 5 * ncols,
                    'unforced:64MiB+1': ncols * 64 * 8 == ENGAGE_BYTES + 512,
                    'unforced:511': sum(lens) * 4 >= 5 * ncols and max(lens) == FLOOR - 1,
                    'unforced:512': gn * 4 >= 5 * ncols and p.hr_min == FLOOR and p.hr_n == 321,
                    'unforced:pays': gn * 4 == 5 * ncols,
                    'unforced:pays-1': gn * 4 == 5 * ncols - 4}[name],
                'the first and the last row of B are read': c.colinds.min() == 0 and c.colinds.max() == ncols - 1}
    return c


T512 = list(range(900, 395, -1))                                              # 505 distinct lengths 900 .. 396
CASES = {}
for _r in range(1, 16):
    CASES[f'seg-lengths:{_r}'] = functools.partial(_seg_lengths, nrows=48 + _r)
CASES['split'] = _split
CASES['widths'] = _widths
for _n in FEW_TILES:
    CASES[f'few-tiles:{_n}'] = functools.partial(_few_tiles, ncols=_n)
for _n in (32, 24, 9):
    CASES[f'buckets:{_n}'] = functools.partial(_buckets, n_heavy=_n)
for _n in (1, 15, 16, 17, 511, 512):
    CASES[f'places:{_n}'] = functools.partial(_places, n_heavy=_n, groups=1)
CASES['places:513-g2'] = functools.partial(_places, n_heavy=513, groups=2)
CASES['places:1025-g4'] = functools.partial(_places, n_heavy=1025, groups=4)
CASES['places:ties-fit'] = functools.partial(_ties, lens=T512 + [300] * 7 + list(range(299, 255, -1)) * 2, groups=1, want=('fit', 300, 512, 1))
CASES['places:ties-move'] = functools.partial(_ties, lens=T512 + [300] * 16 + list(range(299, 255, -1)), groups=1, want=('move', 301, 505, 1))
CASES['places:ties-off'] = functools.partial(_ties, lens=[300] * 600, groups=1, want=None)
CASES['places:shrink'] = functools.partial(_ties, lens=list(range(700, 300, -1)) + [300] * 700, groups=2, want=('move', 301, 400, 1))
for _w in ('skew', 'first', 'last'):
    CASES[f'ranges:{_w}'] = functools.partial(_ranges, where=_w)
CASES['widths-heavy'] = _widths_heavy
CASES['all-heavy'] = _all_heavy
CASES['types'] = _types
for _n in UNFORCED:
    CASES[_n] = _unforced

LIGHT_FAMILIES = ('seg-lengths', 'split', 'widths')
HEAVY_FAMILIES = ('few-tiles', 'buckets', 'places', 'ranges', 'widths-heavy', 'all-heavy', 'types')


def names(*families):
    return [n for n in CASES if not families or n.split(':')[0] in families]


@functools.lru_cache(maxsize=None)
def build(name):
    return CASES[name](name)
