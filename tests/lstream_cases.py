"""
Inputs that put the SpMV light stream (spmv_lstream_kernel in csrc/spmv.hip; build_light_stream, build_stream, build_hot_cache
and build_cold_stage in csrc/spmv_plan.hip; copy pass ls_stage_kernel) on the edges of its tiles, runs, pack and rounds, the
NumPy restatement of how the plan lays the stream out (`Layout`) and of the product itself (`seq_product`).  No GPU imports:
tests/test_lstream_cases_host.py checks every case's preconditions, the constants against csrk_spmv_stream_limits and the
restated product against the oracle; tests/test_gpu_lstream_forms.py runs the library on the same cases in three forms and
compares csrk_spmv_plan_stats with the model field by field.

The layout, restated.  Inputs: the row pointers, the columns, whether the long-row split is forced, the form, the CU count.
  light view   with the split forced (CSRK_SPMV_HEAVY_SPLIT=1) the rows of at least TIERB_MIN entries are cut out -- if every
               one of them has ascending columns, else none is --; with it off (=0) the view is the whole matrix
  dense rule   n_pad = rows without an entry in the view (empty or cut); n_pad * 8 <= n_view: the dense layout, where every
               such row takes one padding slot and run k is row k; else row ids, and the runs are the view's non-empty rows
  slots        row r's first slot = the slots of the rows before it; tile = slot // ACC_TILE; a tile's run slots = the row
               starts in it (slot 0 of its output buffer is the part of a row begun in an earlier tile)
  pack         CSRK_SPMV_HOT=1: the columns referenced at least twice by the first 128 entries of the view's rows, while
               that is at most HOT_SLOTS columns; slots by count descending, column ascending.  The stream kernel keeps the
               first LS_HOT_LDS of them in LDS (LS_RND_HOT with staging) and gathers the rest from the pack
  staging      CSRK_LS_STAGE=1 with a pack and at least one unpacked ("cold") entry: workgroup w of min(CUs, ceil(tiles / 8))
               takes tiles [tiles w / G, tiles (w + 1) / G), cut into equal rounds of whole tiles per wavefront; the round is
               the largest of 128, 120, .. 16 tiles at which every round's cold entries fit LS_RND_CAP (8 otherwise).  The copy
               pass works in blocks of W columns, W = ceil(ceil(ncols / goal) / 16) * 16 with goal = 2 CUs * ceil(ncols / (2 CUs
               * LS_STAGE_WMAX)); a block's pairs = its cold entries + its packed columns
The three forms every case runs in, and the kernel each gets: 'nopack' (CSRK_SPMV_HOT=0: LS_PLAIN, no pack), 'pack'
(CSRK_SPMV_HOT=1, CSRK_LS_STAGE=0: LS_PLAIN with the pack) and 'staged' (CSRK_SPMV_HOT=1, CSRK_LS_STAGE=1: LS_RND24 -- the pack
holds at most 524288 < 2^22 - 1 columns, so the default build never runs LS_RND with 4-byte words).

Row lengths stay at or below 100 or at or above 128, so that the cut set does not depend on anything but the lengths, and
at or below 4096, so that 4096 * 2^-53 stays under the 1e-12 bar of the product check.

Every case is built from a generator seeded with zlib.crc32 of its name, names the edge it sits on (`edge`) and carries
`pre`: a function of the three forms' layouts that returns the properties that put it there, each evaluated to a bool.
`failed_preconditions(case, cus)` lists the ones that do not hold.

Not reachable, and so not covered: a copy pass over a matrix of ONE column (its only column is packed as soon as two
entries exist, and one entry alone goes to the one-lane-per-row kernel: case 'ncols-1' runs the stream with an all-packed
tile instead), LS_RND with 4-byte words (above), and the memory-budget fallbacks of build_light_stream and build_cold_stage.
"""
import zlib

import numpy as np

# csrk_spmv_stream_limits, in its order (tests/test_lstream_cases_host.py holds these against the library)
LIMITS = dict(ACC_TILE=512, ACC_K=8, LS_WAVES=8, LS_SEQ=3, LS_RID=4, LS_HOT_LDS=15360, LS_RND_HOT=8176, LS_RND_CAP=8192,
              LS_RND_MAXTILES=128, LS_STAGE_WMAX=9984, LS_STAGE_BATCH=8192, TIERB_MIN=128, HOT_SLOTS=524288)
TILE, K8, NW, WAVE = LIMITS['ACC_TILE'], LIMITS['ACC_K'], LIMITS['LS_WAVES'], 64
EXACT_LEN = (LIMITS['LS_SEQ'] + 1) * K8 - (K8 - 1)      # 25: the longest row that spans at most LS_SEQ + 1 lanes wherever it lies
#   (24 and shorter are summed in the reference's order wherever they lie inside a tile, 25 at every offset but the last: Layout.exact_rows)
RID_SLOTS = LIMITS['LS_RID'] * WAVE                     # 256: run slots whose row ids a tile fetches ahead
HOT_SAMPLE = 128                                        # entries of a row the pack's column census counts (hot_count_kernel)
IDX24_MAX = (1 << 22) - 1

FORMS = ('nopack', 'pack', 'staged')
FORM_ENV = {'nopack': {'CSRK_SPMV_HOT': '0', 'CSRK_LS_STAGE': '0'},
            'pack': {'CSRK_SPMV_HOT': '1', 'CSRK_LS_STAGE': '0'},
            'staged': {'CSRK_SPMV_HOT': '1', 'CSRK_LS_STAGE': '1'}}
ENV_KEYS = ('CSRK_SPMV_STREAM', 'CSRK_SPMV_HEAVY_SPLIT', 'CSRK_SPMV_HOT', 'CSRK_LS_STAGE')


def env_of(case, form):
    "the environment a (case, form) runs under: every key of ENV_KEYS"
    return dict(FORM_ENV[form], CSRK_SPMV_STREAM='1', CSRK_SPMV_HEAVY_SPLIT='1' if case.split else '0')


def cdiv(a, b):
    return -(-int(a) // int(b))


# ---- matrices ----------------------------------------------------------------------------------------------------------

class Mat:
    def __init__(self, nrows, ncols, rowptrs, colinds, values):
        self.nrows, self.ncols, self.rowptrs, self.colinds, self.values = int(nrows), int(ncols), rowptrs, colinds, values
        self.nnz = len(colinds)

    def tup(self):
        return self.nrows, self.ncols, self.rowptrs, self.colinds, self.values

    def retyped(self, ptr64=False, vals='f8'):
        "the same matrix with int64 row pointers and / or float32 ('f4') or no ('none') values"
        rp = self.rowptrs.astype(np.int64 if ptr64 else np.int32)
        vs = {'f8': self.values, 'f4': self.values.astype(np.float32), 'none': None}[vals]
        return Mat(self.nrows, self.ncols, rp, self.colinds, vs)


def assemble(lens, ncols, rng, cols=None, sort=True, values=None):
    "CSR with rows of `lens` entries: columns uniform over ncols unless given, ascending inside rows if `sort`; values in (-1, 1)"
    lens = np.asarray(lens, dtype=np.int64)
    rp = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=rp[1:])
    nnz = int(rp[-1])
    ci = rng.integers(0, ncols, size=nnz) if cols is None else np.asarray(cols)
    assert len(ci) == nnz and (nnz == 0 or (ci.min() >= 0 and ci.max() < ncols))
    if sort:
        ci = ci[np.lexsort((ci, np.repeat(np.arange(len(lens)), lens)))]
    vs = rng.uniform(-1, 1, size=nnz) if values is None else np.asarray(values, dtype=np.float64)
    return Mat(len(lens), ncols, rp, ci.astype(np.int32), vs)


# ---- the product, written out ------------------------------------------------------------------------------------------

def seq_product(m, x):
    """
    y_i = ((0.0 + a_i0 x_c0) + a_i1 x_c1) + ...: every product rounded on its own, added left to right in storage order
    (csr/kernels/numba/__init__.py:55-67).  float32 values times a float32 x multiply in float32; anything else in float64;
    absent values are 1.0.
    """
    x = np.asarray(x)
    ci = m.colinds
    if m.values is not None and m.values.dtype == np.float32 and x.dtype == np.float32:
        p = (m.values * x[ci]).astype(np.float64)
    else:
        xs = x.astype(np.float64)[ci]
        p = xs.copy() if m.values is None else m.values.astype(np.float64) * xs
    rp = np.asarray(m.rowptrs, dtype=np.int64)
    lens = np.diff(rp)
    order = np.argsort(-lens, kind='stable')
    live = np.searchsorted(-lens[order], -np.arange(int(lens.max()) if m.nrows else 0), side='left')      # rows longer than j
    y = np.zeros(m.nrows, dtype=np.float64)
    for j, n in enumerate(live):
        rows = order[:n]
        y[rows] = y[rows] + p[rp[rows] + j]
    return y


def abs_bound(m, x):
    "sum_j |a_ij x_j| of every row: the same loop, with the same rounding of the products, over the absolute values"
    vs = None if m.values is None else np.abs(m.values)
    return seq_product(Mat(m.nrows, m.ncols, m.rowptrs, m.colinds, vs), np.abs(np.asarray(x)))


# ---- the layout, restated ----------------------------------------------------------------------------------------------

def cut_rows(m, split):
    "the rows the forced split cuts out (build_heavy_split): all rows of >= TIERB_MIN entries, or none if one of them is unsorted"
    none = np.zeros(0, dtype=np.int64)
    lens = np.diff(np.asarray(m.rowptrs, dtype=np.int64))
    if not split or m.nrows == 0 or m.nnz < LIMITS['TIERB_MIN']:
        return none
    cand = np.flatnonzero(lens >= LIMITS['TIERB_MIN'])
    for r in cand:
        if np.any(np.diff(m.colinds[int(m.rowptrs[r]):int(m.rowptrs[r + 1])].astype(np.int64)) < 0):
            return none
    return cand


def make_rounds(n_tiles, grid, nt):
    "build_cold_stage's rounds (spmvlayout::stage_rounds in csrc/spmv_layout.h): (first tile of every round + [n_tiles], first round of every workgroup + [rounds])"
    rt0, wr0 = [], []
    for w in range(grid):
        tb, te = n_tiles * w // grid, n_tiles * (w + 1) // grid
        wr0.append(len(rt0))
        if te > tb:
            k = cdiv(te - tb, nt)
            per = cdiv(cdiv(te - tb, k), NW) * NW
            rt0.extend(range(tb, te, per))
    wr0.append(len(rt0))
    rt0.append(n_tiles)
    return np.array(rt0, dtype=np.int64), np.array(wr0, dtype=np.int64)


def stage_blocks(ncols, cus):
    "(W, nblk) of the copy pass"
    wave = 2 * (cus if cus > 0 else 256)
    goal = wave * cdiv(ncols, wave * LIMITS['LS_STAGE_WMAX'])
    W = cdiv(cdiv(ncols, goal), 16) * 16
    return W, cdiv(ncols, W)


class Layout:
    "the light stream of matrix m as the plan builds it for `form` on `cus` compute units"

    def __init__(self, m, split, form, cus):
        rp = np.asarray(m.rowptrs, dtype=np.int64)
        self.form, self.cus, self.nrows = form, cus, m.nrows
        self.cut = cut_rows(m, split)
        vl = np.diff(rp)
        vl[self.cut] = 0
        self.view_lens = vl
        self.n_view = int(vl.sum())
        self.stream = m.nrows > 0 and self.n_view >= 1
        assert self.stream and m.ncols < (1 << 30) - 1, 'every case keeps a stream'
        self.n_pad = int(np.sum(vl == 0))
        self.dense = self.n_pad * 8 <= self.n_view
        sl = np.maximum(vl, 1) if self.dense else vl
        self.slot_lens = sl
        self.first = np.concatenate([[0], np.cumsum(sl)[:-1]]).astype(np.int64)
        self.n_ent = int(sl.sum())
        self.n_tiles = cdiv(self.n_ent, TILE)
        self.n_runs = int(np.sum(sl > 0))
        self.run_rows = np.flatnonzero(sl > 0)
        self.starts_per_tile = np.bincount(self.first[self.run_rows] // TILE, minlength=self.n_tiles)
        self.grid = min(cus, cdiv(self.n_tiles, NW))
        # the view's entries in stream order: row, offset inside the row, slot, column
        self.erow = np.repeat(np.arange(m.nrows, dtype=np.int64), vl)
        vstart = np.concatenate([[0], np.cumsum(vl)[:-1]])
        self.eoff = np.arange(self.n_view, dtype=np.int64) - vstart[self.erow]
        self.eslot = self.first[self.erow] + self.eoff
        self.ecol = m.colinds[rp[self.erow] + self.eoff].astype(np.int64)
        # the pack
        self.n_hot, self.hot_cols, self.slot_of = 0, np.zeros(0, dtype=np.int64), np.full(m.ncols, -1, dtype=np.int64)
        if form != 'nopack' and m.nnz >= 2:
            cnt = np.bincount(self.ecol[self.eoff < HOT_SAMPLE], minlength=m.ncols)
            thr = 2
            while int(np.sum(cnt >= thr)) > LIMITS['HOT_SLOTS']:
                thr += 1
            cols = np.flatnonzero(cnt >= thr)
            self.hot_cols = cols[np.lexsort((cols, -cnt[cols]))]
            self.n_hot = len(cols)
            self.slot_of[self.hot_cols] = np.arange(self.n_hot)
        self.eslot_hot = self.slot_of[self.ecol]
        self.ecold = self.eslot_hot < 0
        self.tile_cold = np.bincount(self.eslot[self.ecold] // TILE, minlength=self.n_tiles)
        # staging
        self.staged, self.n_cold, self.stage_tiles, self.W, self.nblk = False, 0, 0, 0, 0
        self.rt0, self.wr0, self.round_staged, self.blk_pairs = None, None, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        W, nblk = stage_blocks(m.ncols, cus)
        nb_max = (cdiv(self.n_tiles, NW) + self.grid + 2) * nblk
        if form == 'staged' and self.n_hot > 0 and 1 <= nb_max <= 1 << 26 and int(self.tile_cold.sum()) >= 1:
            pre = np.concatenate([[0], np.cumsum(self.tile_cold)])
            nt = LIMITS['LS_RND_MAXTILES'] // NW * NW
            while nt > NW:
                rt0, wr0 = make_rounds(self.n_tiles, self.grid, nt)
                if int(np.max(pre[rt0[1:]] - pre[rt0[:-1]])) <= LIMITS['LS_RND_CAP']:
                    break
                nt -= NW
            self.rt0, self.wr0 = make_rounds(self.n_tiles, self.grid, nt)
            self.round_staged = pre[self.rt0[1:]] - pre[self.rt0[:-1]]
            assert int(self.round_staged.max()) <= LIMITS['LS_RND_CAP']
            self.staged, self.n_cold, self.stage_tiles, self.W, self.nblk = True, int(pre[-1]), nt, W, nblk
            self.blk_pairs = np.bincount(self.ecol[self.ecold] // W, minlength=nblk) + np.bincount(self.hot_cols // W, minlength=nblk)
        lds = LIMITS['LS_RND_HOT'] if self.staged else LIMITS['LS_HOT_LDS']
        self.n_hot_lds = min(self.n_hot, lds)
        self.idx24 = self.staged and self.n_hot < IDX24_MAX
        if self.staged:
            self.n_rounds, self.wg_rounds = len(self.rt0) - 1, np.diff(self.wr0)
        else:      # the plain kernel: a round is one tile per wavefront, workgroup b takes rounds b, b + grid, ...
            self.n_rounds = cdiv(self.n_tiles, NW)
            self.wg_rounds = np.array([cdiv(self.n_rounds - b, self.grid) for b in range(self.grid)], dtype=np.int64)

    def census(self, f32=False):
        "what csrk_spmv_plan_stats must report (the names of csr_amd.kernels.hip.SPMV_PLAN_STATS)"
        return dict(stream=1, cut_rows=len(self.cut), ls_tiles=self.n_tiles, ls_runs=self.n_runs, ls_grid=self.grid,
                    ls_dense=int(self.dense), n_hot=self.n_hot, ls_hot_lds=self.n_hot_lds, ls_staged=self.n_cold,
                    ls_round_tiles=self.stage_tiles, ls_rounds=self.n_rounds, ls_wg_rounds=int(self.wg_rounds.max()),
                    ls_stage_blocks=self.nblk, ls_stage_width=self.W, ls_idx24=int(self.idx24), ls_f32=int(bool(f32)))

    def mode(self):
        return 'LS_RND24' if self.idx24 else 'LS_RND' if self.staged else 'LS_PLAIN+pack' if self.n_hot else 'LS_PLAIN'

    # rows and tiles
    def last_slot(self):
        return self.first + self.slot_lens - 1

    def split_rows(self):
        "rows of the view that a tile boundary cuts (their sum is completed by a carry: not in the reference's order)"
        return np.flatnonzero((self.view_lens > 0) & (self.first // TILE != self.last_slot() // TILE))

    def storing_lane(self):
        """
        Per run (run_rows): the lane that stores its sum -- the lane of the next row start, or lane 63 for a tile's last run,
        which ends with the tile or, in a last tile that is not full, is continued by its padding slots.
        """
        r = self.run_rows
        nxt = np.append(self.first[r[1:]], -TILE)
        return np.where(nxt // TILE == self.first[r] // TILE, (nxt % TILE) // K8, WAVE - 1)

    def exact_rows(self):
        """
        The rows summed in the reference's own order, bit for bit (spmv_lstream_kernel's in-order hand-over): rows of the view
        inside one tile whose sum is stored at most LS_SEQ lanes after the lane they start in.  That is every row of at most 24
        entries but the matrix's last one (unless that starts in lanes 60 .. 63 or fills its tile), and a row of 25 unless it
        starts in a lane's last slot and ends before its tile does; longer rows qualify up to 31 entries when they start early
        enough in a lane.
        """
        r = self.run_rows
        ok = (self.view_lens[r] > 0) & (self.first[r] // TILE == self.last_slot()[r] // TILE)
        return r[ok & (self.storing_lane() - (self.first[r] % TILE) // K8 <= LIMITS['LS_SEQ'])]

    def lanes(self, rows):
        "lanes a row spans (rows inside one tile)"
        return (self.last_slot()[rows] % TILE) // K8 - (self.first[rows] % TILE) // K8 + 1

    def gaps(self):
        "rows without a run: before the first run, between consecutive runs, after the last"
        r = self.run_rows
        return int(r[0]), np.diff(r) - 1, self.nrows - 1 - int(r[-1])

    def gathered_tiles(self):
        "tiles that hold an entry on a packed column beyond the LDS slots (gathered from the pack)"
        return np.unique(self.eslot[self.eslot_hot >= self.n_hot_lds] // TILE)


# ---- cases -------------------------------------------------------------------------------------------------------------

class Case:
    def __init__(self, name, edge, m, x, split, pre):
        self.name, self.edge, self.m, self.x, self.split, self.pre = name, edge, m, x, split, pre
        self._layouts = {}

    def layout(self, form, cus):
        if (form, cus) not in self._layouts:
            self._layouts[(form, cus)] = Layout(self.m, self.split, form, cus)
        return self._layouts[(form, cus)]

    def layouts(self, cus):
        return {f: self.layout(f, cus) for f in FORMS}


CASES = {}          # name -> (edge, builder(rng, cus) -> (m, x, split, pre), depends on the CU count)


def case(name, edge, per_cus=False):
    def reg(fn):
        assert name not in CASES
        CASES[name] = (edge, fn, per_cus)
        return fn
    return reg


def names():
    return list(CASES)


_BUILT = {}


def build(name, cus=256):
    "the case (cached: the arrays are shared, treat them as read-only); only a few cases depend on the CU count"
    edge, fn, per_cus = CASES[name]
    key = (name, cus if per_cus else 0)
    if key not in _BUILT:
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        m, x, split, pre = fn(rng, cus)
        for a in (m.rowptrs, m.colinds, m.values, x):
            a.flags.writeable = False
        _BUILT[key] = Case(name, edge, m, x, split, pre)
    return _BUILT[key]


def failed_preconditions(c, cus):
    "the properties of the case's edge that do not hold on `cus` compute units, by the model (empty: the case sits on its edge)"
    L = c.layouts(cus)
    lens = np.diff(np.asarray(c.m.rowptrs, dtype=np.int64))
    props = dict(c.pre(L))
    props['rows at most 100 or at least 128 entries, none above 4096'] = bool(np.all((lens <= 100) | ((lens >= 128) & (lens <= 4096))))
    props['the three forms lay the rows out alike'] = all(L[f].n_tiles == L['nopack'].n_tiles and L[f].dense == L['nopack'].dense for f in FORMS)
    return [k for k, v in props.items() if not v]


def _x(rng, ncols):
    return rng.uniform(-1, 1, size=ncols)


def _short(rng, total, lo=1, hi=EXACT_LEN):
    "row lengths in [lo, hi] that add up to `total`"
    out, s = [], 0
    while s < total:
        n = int(min(rng.integers(lo, hi + 1), total - s))
        out.append(n)
        s += n
    return out


def _spread(lens, every, n_empty_tail=0):
    "an empty row after every `every`-th row, and `n_empty_tail` at the end"
    out = []
    for i, n in enumerate(lens):
        out.append(n)
        if (i + 1) % every == 0:
            out.append(0)
    return out + [0] * n_empty_tail


def _three_modes(L):
    return {'the forms reach LS_PLAIN, LS_PLAIN with a pack and LS_RND24':
            [L[f].mode() for f in FORMS] == ['LS_PLAIN', 'LS_PLAIN+pack', 'LS_RND24']}


# run slots: a tile with exactly S row starts, in both layouts
def _run_slots(S, dense):
    def b(rng, cus):
        lens = [1] * (S - 1) + [TILE - (S - 1)] + _short(rng, 700)
        if not dense:
            lens = _spread(lens, 1, 40)
        m = assemble(lens, 700, rng)

        def pre(L):
            p = {f'tile 0 has exactly {S} row starts': all(L[f].starts_per_tile[0] == S for f in FORMS),
                 'the layout is ' + ('dense' if dense else 'row ids'): L['nopack'].dense == dense,
                 'the second output loop runs exactly from 256 starts on': (S >= RID_SLOTS) == (L['nopack'].starts_per_tile.max() >= RID_SLOTS)}
            if not dense and S >= RID_SLOTS:
                p['a one-row gap is cleared from the second loop'] = bool(np.all(L['nopack'].gaps()[1][RID_SLOTS - 2:S - 1] == 1))
            p.update(_three_modes(L))
            return p
        return m, _x(rng, m.ncols), False, pre
    return b


for _S in (255, 256, 257, 511, 512):
    for _d in (False, True):
        case(f"starts-{_S}-{'dense' if _d else 'rowid'}",
             f"a tile with exactly {_S} row starts ({'dense' if _d else 'row-id'} layout): "
             + ('the second output loop, which loads its row ids itself, runs' if _S >= 256 else 'one start short of the second output loop'))(_run_slots(_S, _d))

GAPS = (0, 1, 4, 5, 63, 64, 65, 1000)


@case('gaps', 'row-id layout: 0, 1, 4, 5, 63, 64, 65 and 1000 empty rows between runs, empty rows before the first and after the last '
              'run, a gap across a tile boundary, the last run in its tile\'s last slot')
def _gaps(rng, cus):
    lens, pos, i = [0] * 7, 0, 0

    def fill_to(target, last_gap):
        nonlocal pos, i
        while pos < target:
            n = int(min(rng.integers(1, EXACT_LEN + 1), target - pos))
            pos += n
            lens.append(n)
            lens.extend([0] * (last_gap if pos == target else GAPS[i % len(GAPS)]))
            i += 1
    fill_to(TILE, 5)
    fill_to(2 * TILE - 1, 64)
    lens += [1] + [0] * 70
    m = assemble(lens, 600, rng)

    def pre(L):
        a = L['nopack']
        before, between, after = a.gaps()
        r = a.run_rows
        cross = (a.first[r[1:]] // TILE != a.last_slot()[r[:-1]] // TILE) & (between > 4)
        p = {'row ids': not a.dense, 'every gap length occurs': set(GAPS) <= set(between.tolist()),
             'empty rows before the first run and more than 64 after the last': before == 7 and after == 70,
             'a long gap whose runs lie in different tiles': bool(cross.any()),
             'the last run is one entry in the last slot of a whole tile': a.n_view == 2 * TILE and a.view_lens[r[-1]] == 1}
        p.update(_three_modes(L))
        return p
    return m, _x(rng, m.ncols), False, pre


@case('dense-edge-pads', 'dense layout: empty rows whose padding entry is a tile\'s last slot, the next tile\'s first and that tile\'s last')
def _dense_edges(rng, cus):
    lens = _short(rng, TILE - 1) + [0, 0] + _short(rng, TILE - 2) + [0] + _short(rng, 300)
    m = assemble(lens, 700, rng)

    def pre(L):
        a = L['nopack']
        pads = set(a.first[a.view_lens == 0].tolist())
        p = {'dense': a.dense, 'padding entries at slots 511, 512 and 1023': pads == {TILE - 1, TILE, 2 * TILE - 1}}
        p.update(_three_modes(L))
        return p
    return m, _x(rng, m.ncols), False, pre


@case('dense-pad-tile', 'dense layout: a tile made of 512 padding entries')
def _dense_pad_tile(rng, cus):
    lens = _short(rng, TILE) + [0] * TILE + _short(rng, 8 * TILE - TILE + 37)
    m = assemble(lens, 2500, rng)

    def pre(L):
        a = L['nopack']
        in1 = (a.first >= TILE) & (a.first < 2 * TILE)
        p = {'dense': a.dense, 'tile 1 holds 512 rows, all empty': int(in1.sum()) == TILE and bool(np.all(a.view_lens[in1] == 0)),
             'no cold entry in the padding tile': all(L[f].tile_cold[1] == 0 for f in FORMS)}
        p.update(_three_modes(L))
        return p
    return m, _x(rng, m.ncols), False, pre


def _dense_limit(over):
    def b(rng, cus):
        n_pad, out = TILE // 8, []
        for i, n in enumerate(_short(rng, TILE - over, lo=4, hi=8)):          # (at least 64 rows)
            out += [n, 0] if i < n_pad else [n]
        m = assemble(out, 300, rng)

        def pre(L):
            a = L['nopack']
            p = {f'n_pad * 8 = n_view + {over}': a.n_pad * 8 == a.n_view + over, 'dense exactly at the limit': a.dense == (over == 0)}
            p.update(_three_modes(L))
            return p
        return m, _x(rng, m.ncols), False, pre
    return b


case('dense-limit', 'n_pad * 8 equal to n_view: the last matrix that gets the dense layout')(_dense_limit(0))
case('dense-limit-over', 'n_pad * 8 one above n_view: the first matrix that gets row ids')(_dense_limit(1))


def _nview(n):
    def b(rng, cus):
        if n == 1:          # one light entry beside a cut row (a matrix of one entry never reaches the stream)
            cols = np.concatenate([np.sort(rng.choice(400, 200, replace=False)), [7]])
            m = assemble([200, 0, 1], 400, rng, cols=cols, sort=False)
        elif n == 2:
            m = assemble([1, 0, 1], 9, rng, cols=[3, 3], sort=False)
        else:
            m = assemble(_short(rng, n), max(16, n // 2), rng)

        def pre(L):
            a = L['nopack']
            p = {f'n_view is {n}': a.n_view == n, 'tiles': a.n_tiles == cdiv(a.n_ent, TILE)}
            if n in (TILE + 1, 8 * TILE + 1):
                p['the last tile holds one entry'] = a.n_ent == n and a.n_ent % TILE == 1
            if n == 8 * TILE + 1:
                p['the last round has one busy wavefront'] = a.n_tiles % NW == 1
            if n == 1:
                p['the 200-entry row is cut'] = a.cut.tolist() == [0]
            if n > 2:
                p.update(_three_modes(L))
            return p
        return m, _x(rng, m.ncols), n == 1, pre
    return b


for _n in (1, 2, TILE - 1, TILE, TILE + 1, 8 * TILE, 8 * TILE + 1):
    case(f'nview-{_n}', f'a light view of {_n} entries')(_nview(_n))


@case('tile-boundary', 'a row that ends exactly on a tile boundary, the next that starts on it, and a row cut in two by the next boundary')
def _tile_boundary(rng, cus):
    lens = _short(rng, TILE) + _short(rng, TILE - 10) + [20] + _short(rng, 300)
    m = assemble(lens, 700, rng)

    def pre(L):
        a = L['nopack']
        p = {'a row ends in slot 511 and a row starts in slot 512': TILE - 1 in a.last_slot() and TILE in a.first,
             'a row of 20 entries holds slots 1014 .. 1033': bool(np.any((a.first == 2 * TILE - 10) & (a.view_lens == 20)))}
        p.update(_three_modes(L))
        return p
    return m, _x(rng, m.ncols), False, pre


def order_coverage(a):
    "the (length, offset of the first entry inside its lane) pairs of the rows checked bit for bit"
    rows = a.exact_rows()
    return set(zip(a.view_lens[rows].tolist(), (a.first[rows] % K8).tolist()))


@case('order-short', 'rows of 1 .. 25 entries, every length at every offset 0 .. 7 inside a lane: spans of 1, 2, 3 and 4 lanes')
def _order_short(rng, cus):
    lens, pos = [], 0
    for n in range(1, EXACT_LEN + 1):
        for off in rng.permutation(K8):
            pad = (int(off) - pos) % K8
            if (pos + pad) // TILE != (pos + pad + n - 1) // TILE:          # the row would be cut: move on to the next tile
                pad = (-pos) % TILE + int(off)
            if n == EXACT_LEN and off == K8 - 1:          # four lanes and the next start a fifth: in order only where it ends its tile
                lens.append(n)                            # (one that does not, left out of the exact check)
                pos += n
                pad = (TILE - n - pos) % TILE
            while pad:
                f = min(pad, EXACT_LEN)
                lens.append(f)
                pos, pad = pos + f, pad - f
            lens.append(n)
            pos += n
    lens.append(3)          # (the matrix's last row is continued by the last tile's padding: not one of the rows above)
    m = assemble(lens, 2000, rng)

    def pre(L):
        a = L['nopack']
        p = {'every length 1 .. 25 is checked exactly at every lane offset': order_coverage(a) >= {(n, o) for n in range(1, EXACT_LEN + 1) for o in range(K8)},
             'checked rows span 1, 2, 3 and 4 lanes': set(a.lanes(a.exact_rows()).tolist()) == {1, 2, 3, 4},
             'a row of 25 entries from a lane\'s last slot ends its tile': bool(np.any((a.view_lens == EXACT_LEN) & (a.last_slot() % TILE == TILE - 1))),
             'the rows left out are those a tile boundary cuts, rows of 25 from a lane\'s last slot and the last row': set(range(a.nrows)) - set(a.exact_rows().tolist()) - set(a.split_rows().tolist()) <= set(np.flatnonzero((a.view_lens == EXACT_LEN) & (a.first % K8 == K8 - 1)).tolist()) | {a.nrows - 1}}
        p.update(_three_modes(L))
        return p
    return m, _x(rng, m.ncols), False, pre


@case('order-mid', 'rows of 26 .. 100 entries among short ones: runs over 5 and more lanes, joined by the tree scan')
def _order_mid(rng, cus):
    lens = []
    for n in rng.permutation(np.arange(26, 101)):
        lens += [int(n)] + _short(rng, 12)
    m = assemble(lens, 3000, rng)

    def pre(L):
        a = L['nopack']
        inside = np.flatnonzero((a.view_lens > EXACT_LEN) & (a.first // TILE == a.last_slot() // TILE))
        p = {'rows inside a tile span 5 lanes and 13 or more': 5 in a.lanes(inside) and a.lanes(inside).max() >= 13 and a.lanes(inside).min() >= 4,
             'every length 26 .. 100 occurs': set(range(26, 101)) <= set(a.view_lens.tolist())}
        p.update(_three_modes(L))
        return p
    return m, _x(rng, m.ncols), False, pre


@case('order-zeros', 'signed zeros among the products: rows whose products are all zeros, some of them -0.0, must come out +0.0')
def _order_zeros(rng, cus):
    lens = _short(rng, 3000)
    nnz, ncols = sum(lens), 1500
    vs = rng.uniform(-1, 1, size=nnz)
    vs[rng.random(nnz) < 0.25] = 0.0
    vs[rng.random(nnz) < 0.25] = -0.0
    x = rng.uniform(-1, 1, size=ncols)
    x[rng.random(ncols) < 0.2] = 0.0
    x[rng.random(ncols) < 0.2] = -0.0
    m = assemble(lens, ncols, rng, values=vs)

    def pre(L):
        a = L['nopack']
        p = m.values * x[m.colinds]
        neg = (p == 0) & np.signbit(p)
        rp = np.asarray(m.rowptrs, dtype=np.int64)
        nz = np.concatenate([[0], np.cumsum(p != 0)])
        ng = np.concatenate([[0], np.cumsum(neg)])
        rows = a.exact_rows()
        allz = (nz[rp[rows + 1]] == nz[rp[rows]]) & (ng[rp[rows + 1]] > ng[rp[rows]])
        lead = neg[rp[rows]] & (a.view_lens[rows] > 1)
        q = {'+0.0 and -0.0 among the products': bool(neg.any()) and bool(np.any((p == 0) & ~np.signbit(p))),
             'checked rows whose products are all zeros with a -0.0 among them': int(allz.sum()) >= 5,
             'checked rows that open with a -0.0': int(lead.sum()) >= 20}
        q.update(_three_modes(L))
        return q
    return m, x, False, pre


def _long_lens(rng):
    return ([4096] + _short(rng, 300) + [513] + _short(rng, 700) + [2048, 4096] + _short(rng, 200) + [2048] + _short(rng, 100) + [513])


@case('long-rows', 'rows of 513, 2048 and 4096 entries on the stream (split off): carries that chain over 2 .. 9 tiles through '
                   'spmv_merge_fixup_kernel; two such rows adjacent, one first, one last')
def _long_rows(rng, cus):
    lens = _long_lens(rng)
    m = assemble(lens, 6000, rng)

    def pre(L):
        a = L['nopack']
        span = a.last_slot() // TILE - a.first // TILE + 1
        lg = np.flatnonzero(a.view_lens >= 513)
        p = {'nothing is cut': all(len(L[f].cut) == 0 for f in FORMS), 'long rows span 2 and 9 tiles': {2, 9} <= set(span[lg].tolist()),
             'two long rows adjacent': bool(np.any(np.diff(lg) == 1)), 'the first and the last row are long': lg[0] == 0 and lg[-1] == m.nrows - 1}
        p.update(_three_modes(L))
        return p
    return m, _x(rng, m.ncols), False, pre


@case('long-cut200', 'short rows and one sorted 200-entry row under the forced split: the row is cut, so the stream\'s carries are '
                     'added by the epilogue (add_fix) instead of spmv_merge_fixup_kernel')
def _long_cut200(rng, cus):
    lens = _short(rng, 900) + [200] + _short(rng, 1500)
    m = assemble(lens, 1500, rng)
    r200 = lens.index(200)

    def pre(L):
        a = L['nopack']
        p = {'exactly the 200-entry row is cut': all(L[f].cut.tolist() == [r200] for f in FORMS),
             'a tile boundary cuts a row of the view': len(a.split_rows()) >= 1}
        p.update(_three_modes(L))
        return p
    return m, _x(rng, m.ncols), True, pre


def _pack(N):
    def b(rng, cus):
        M = 3000
        ncols = N + M + 7
        ids = rng.permutation(ncols)
        hot, cold = ids[:N], ids[N:N + M]
        cols = np.concatenate([hot, hot, hot[:50], hot[:50], cold])
        rng.shuffle(cols)
        m = assemble(_short(rng, len(cols), lo=5), ncols, rng, cols=cols)

        def pre(L):
            p = {f'the pack holds exactly {N} columns': L['pack'].n_hot == N and L['staged'].n_hot == N,
                 'pack slots in LDS': L['pack'].n_hot_lds == min(N, LIMITS['LS_HOT_LDS']) and L['staged'].n_hot_lds == min(N, LIMITS['LS_RND_HOT']),
                 'the most popular columns take the first slots': N < 50 or set(L['pack'].hot_cols[:50].tolist()) == set(hot[:50].tolist())}
            for f, lim in (('pack', 'LS_HOT_LDS'), ('staged', 'LS_RND_HOT')):
                t = L[f].gathered_tiles()
                p[f'{f}: entries gathered from the pack exactly above {lim}, in several tiles'] = (len(t) >= 2) if N > LIMITS[lim] else len(t) == 0
            p.update(_three_modes(L))
            return p
        return m, _x(rng, ncols), False, pre
    return b


for _N in (1, 8175, 8176, 8177, 15359, 15360, 15361):
    case(f'pack-{_N}', f'a pack of exactly {_N} columns (LS_RND_HOT = 8176 and LS_HOT_LDS = 15360 slots live in LDS; the rest is gathered)')(_pack(_N))


@case('rounds', 'the one large case: 25 CUs + 3 tiles of mostly cold entries, so that every workgroup walks two rounds and its last is '
                'not a multiple of 8 tiles; one round holds exactly LS_RND_CAP staged values (its 16 tiles are all cold), others an odd '
                'count; CSRK_LS_STAGE=0 walks several plain rounds per workgroup', per_cus=True)
def _rounds(rng, cus):
    n_tiles = 25 * cus + 3
    n = n_tiles * TILE - 100
    n_hot, cap = 2000, LIMITS['LS_RND_CAP']
    lens = _short(rng, cap) + _short(rng, n - cap)          # (a row ends where the first 16 tiles do)
    ncols = n + n_hot
    ids = rng.permutation(ncols)
    hot = ids[:n_hot]
    is_hot = rng.random(n) < 0.05
    is_hot[:cap] = False
    is_hot[cap:cap + 2 * n_hot] = True                      # (every packed column is referenced at least twice)
    cols = np.empty(n, dtype=np.int64)
    k = int(is_hot.sum())
    cols[is_hot] = np.concatenate([hot, hot, rng.choice(hot, size=k - 2 * n_hot)])
    cols[~is_hot] = ids[n_hot:n_hot + n - k]
    m = assemble(lens, ncols, rng, cols=cols, sort=False)

    def pre(L):
        s, pk = L['staged'], L['pack']
        last = np.diff(s.rt0)[s.wr0[1:] - 1] if s.staged else np.zeros(1, dtype=np.int64)
        return {'25 CUs + 3 tiles': s.n_tiles == n_tiles and s.grid == cus, 'staged': s.staged and s.n_hot == n_hot,
                'every workgroup walks at least two rounds': s.staged and int(s.wg_rounds.min()) >= 2,
                'no workgroup\'s last round is a multiple of 8 tiles': bool(np.all(last % NW != 0)),
                'a round with an odd staged count': bool(np.any(s.round_staged % 2 == 1)),
                'round 0 holds exactly LS_RND_CAP staged values': s.staged and int(s.round_staged[0]) == cap and int(s.round_staged.max()) == cap,
                'the plain kernel walks several rounds per workgroup': int(pk.wg_rounds.min()) >= 2 and not pk.staged,
                **_three_modes(L)}
    return m, _x(rng, ncols), False, pre


def _ncols(nc, n_once):
    def b(rng, cus):
        lens = _short(rng, 600)
        if nc == 1:
            cols = np.zeros(600, dtype=np.int64)
        else:      # the last n_once columns are referenced exactly once, the others many times
            cols = rng.integers(0, nc - n_once, size=600)
            cols[rng.choice(600, n_once, replace=False)] = np.arange(nc - n_once, nc)
        m = assemble(lens, nc, rng, cols=cols)

        def pre(L):
            s = L['staged']
            W, nblk = stage_blocks(nc, cus)
            if nc == 1:
                return {'one column, packed: nothing is cold, nothing is staged': L['pack'].n_hot == 1 and not s.staged and int(L['pack'].tile_cold.sum()) == 0}
            p = {'staged, cold entries as built': s.staged and s.n_cold == n_once, 'blocks of 16 columns': (s.W, s.nblk) == (W, nblk) and W == 16}
            if nc % 16:
                p['the last block is narrower than W'] = s.nblk * s.W > nc
            if nc > 32:
                p['the blocks are no multiple of 8'] = s.nblk % 8 != 0 and bool(s.blk_pairs[-1] > 0)
            p.update(_three_modes(L))
            return p
        return m, _x(rng, nc), False, pre
    return b


for _nc, _once in ((1, 0), (15, 1), (16, 1), (17, 1), (83, 40)):
    case(f'ncols-{_nc}', f'the copy pass on {_nc} columns' + (': 6 blocks, no multiple of 8, the last one 3 columns wide' if _nc == 83 else ''))(_ncols(_nc, _once))


def _stage_batch(Kp):
    def b(rng, cus):
        # three 4096-entry rows (split off): the pack's census counts a row's first 128 entries only, so the columns 0 .. 15
        # that only their tails reference stay cold however often they occur -- Kp times: one column block of Kp pairs
        ncols, tail = 2000, 4096 - HOT_SAMPLE
        lens = [4096] + _short(rng, 400) + [4096] + _short(rng, 400) + [4096]
        rows = np.repeat(np.arange(len(lens)), lens)
        off = np.arange(len(rows)) - np.concatenate([[0], np.cumsum(lens)[:-1]])[rows]
        cols = rng.integers(16, ncols, size=len(rows))
        t = np.flatnonzero((np.asarray(lens)[rows] == 4096) & (off >= HOT_SAMPLE))
        assert len(t) == 3 * tail >= Kp
        cols[rng.choice(t, Kp, replace=False)] = rng.integers(0, 16, size=Kp)
        m = assemble(lens, ncols, rng, cols=cols, sort=False)

        def pre(L):
            s = L['staged']
            return {'staged, blocks of 16 columns': s.staged and s.W == 16, f'block 0 holds {Kp} pairs': s.staged and int(s.blk_pairs[0]) == Kp,
                    'no other block needs a second batch': s.staged and int(s.blk_pairs[1:].max()) < LIMITS['LS_STAGE_BATCH'],
                    **_three_modes(L)}
        return m, _x(rng, ncols), False, pre
    return b


for _k in (8191, 8192, 8193):
    case(f'stage-batch-{_k}', f'a column block of the copy pass with {_k} staged pairs (its loop takes a second batch above 8192)')(_stage_batch(_k))


def _unsorted(dense):
    def b(rng, cus):
        lens = _short(rng, 1500, lo=3, hi=30)
        if not dense:
            lens = _spread(lens, 3, 200)
        m = assemble(lens, 900, rng, sort=False)
        ci = m.colinds.copy()
        rp = m.rowptrs
        ci[rp[1:][np.diff(rp) >= 3] - 1] = ci[rp[:-1][np.diff(rp) >= 3]]      # every row's last column repeats its first
        m = Mat(m.nrows, m.ncols, rp, ci, m.values)

        def pre(L):
            a = L['nopack']
            d = np.diff(ci.astype(np.int64))
            p = {'the layout is ' + ('dense' if dense else 'row ids'): a.dense == dense, 'descending steps inside rows': int(np.sum(d < 0)) > m.nrows,
                 'rows that hold a column twice': bool(np.any(ci[rp[1:][np.diff(rp) >= 3] - 1] == ci[rp[:-1][np.diff(rp) >= 3]]))}
            p.update(_three_modes(L))
            return p
        return m, _x(rng, m.ncols), False, pre
    return b


case('unsorted-rowid', 'unsorted and repeated columns inside light rows, row-id layout')(_unsorted(False))
case('unsorted-dense', 'unsorted and repeated columns inside light rows, dense layout')(_unsorted(True))

ORDER_CASES = ('order-short', 'order-mid', 'order-zeros')
# the cases that also run with float32 / no values, int64 row pointers, a float32 x and the two-part entry: one per layout,
# and one with a cut row
REPRESENTATIVE = ('gaps', 'dense-edge-pads', 'long-cut200')
