"""
Inputs that put the general sparse product (csrc/spgemm.hip, csrc/spgemm_order.hip) on every one of its accumulators and on
both sides of every threshold between them, the NumPy restatement of the routing (`census`) and of the product itself
(`ref_product`).  No GPU imports: tests/test_spgemm_cases_host.py checks every case's preconditions, the constants against
csrk_spgemm_limits and the restated product against the oracle; tests/test_gpu_spgemm_routes.py runs the library on the
same cases and compares csrk_spgemm_last_stats with the census field by field.  `order_plan` restates what the ordering pass
does with a product's rows (csrc/spgemm_order_plan.h); tests/test_spgemm_order_plan_host.py holds the header against it.

The routing, restated.  A row of the product is sent by its product count u = sum over the entries (i, j) of A of |B_j| and
its entry count J (sg_list_rows; the driver's sg_plan decides what is in force):
  u = 0                                                     nothing
  u > SG_CAP, strip-dense, strips in force                   column strips
  u > SGE_MIN, not (strip-dense and u > SG_CAP), ESC on     expand-sort-compress
  u > SG_CAP otherwise                                       a "large" row: LDS tiles / 8192-slot hash / HBM work row
  the rest (route 0)                                         16 lanes (u <= 32), 32 lanes (<= SG_WAVE_CAP), workgroup hash
strip-dense: S = ceil(ncols_B / SGS_W) <= SGS_MAX_S, u >= SGS_MIN_PER_CELL * J * S and u >= SGS_MIN_PER_UNIT * S.  The strips
are in force for FAST operands (int32 row pointers and float64 values on both) whose right operand's rows ascend --
strictly, checked on the device, for A B; taken for granted for the transpose A B^T multiplies by -- unless
CSRK_SPGEMM_STRIPS=0.  A large row's distinct output columns cnt are counted in LDS when ncols_B <= SGL_MAXBITS; then
8 cnt >= ncols_B and ncols_B <= SGL_W * SGL_MAXTILES: LDS tiles; else cnt <= SGB_CAP: the big hash table; else, and
whenever they were not counted, an HBM work row (sg_split_large).

Every case is built from a generator seeded with zlib.crc32 of its name and carries `pre`: the properties that put it on
its edge, each already evaluated to a bool.  Both test files assert them.

Not reachable with a small input, and so not covered: the memory-budget fallbacks SGE_BUDGET_PRODUCTS (2 * 10^8 products
in expand-sort-compress), its hipMemGetInfo check, SGS_TABLE_BUDGET, SGS_TEMP_BUDGET and nrows * strips > 2^30.  Their
arithmetic (csrc/spgemm_plan.h) is checked on the host at every edge: tests/test_spgemm_plan_host.py.
"""
import zlib

import numpy as np

# csrk_spgemm_limits, in its order (tests/test_spgemm_cases_host.py holds these against the library)
LIMITS = dict(SG_WAVE_CAP=128, SG_CAP=1024, SGE_MIN=32, SGE_TILE=1024, SGS_W=832, SGS_MAX_S=256, SGS_MIN_PER_CELL=4,
              SGS_MIN_PER_UNIT=512, SGS_HEAVY_J=1024, SGL_W=20096, SGL_MAXTILES=8, SGL_MAXBITS=1 << 20, SGB_CAP=4096,
              SG_COUNT_LONG=64, SG_COUNT_VLONG=4096, SO_LEAST=64, SO_TINY=256, SO_WAVE=1024, SO_MID=4096, SO_WIN=1 << 19)
SG_QUAD_CAP = 32            # products of a 16-lane row at most (sg_quad_kernel<16, 32>; not a tunable: the driver writes 32)
SGQ_SLOTS = (64, 256)       # table slots of the 16- and the 32-lane rows
SG_SLOTS = 2048             # of the workgroup hash kernel
HASH_MUL = 2654435761
EXPAND_BATCH = 256          # entries of A sg_esc_expand takes at a time
LIST_THREADS = 1024         # rows per workgroup of sg_list_rows: below this the ESC rows are listed in row order

STATS = ('general', 'fast', 'strips', 'strip_rows', 'strip_entries', 'strip_fused', 'esc_rows', 'esc_products', 'large_rows',
         'lds_symbolic', 'lds_rows', 'hash_big_rows', 'hbm_rows', 'small_fused', 'mid_rows', 'hash_rows')


def quad_slot(k, slots):
    "home slot of column k in a sub-wavefront row's table (sg_quad_kernel)"
    return (int(k) * HASH_MUL) & 0xffffffff & (slots - 1)


def wg_slot(k):
    "home slot of column k in the workgroup hash kernel's 2048-slot table (sg_hash: the top 11 bits)"
    return ((int(k) * HASH_MUL) & 0xffffffff) >> 21


# ---- matrices ----------------------------------------------------------------------------------------------------------

class Mat:
    def __init__(self, nrows, ncols, rowptrs, colinds, values):
        self.nrows, self.ncols, self.rowptrs, self.colinds, self.values = int(nrows), int(ncols), rowptrs, colinds, values
        self.nnz = len(colinds)

    def tup(self):
        return self.nrows, self.ncols, self.rowptrs, self.colinds, self.values

    def retyped(self, ptr64=None, f32=None):
        rp = self.rowptrs if ptr64 is None else self.rowptrs.astype(np.int64 if ptr64 else np.int32)
        vs = self.values if f32 is None else self.values.astype(np.float32 if f32 else np.float64)
        return Mat(self.nrows, self.ncols, rp, self.colinds, vs)


def mat(rows, ncols, rng, values=None):
    "CSR of `rows` (one array of columns per row, stored in that order); values uniform in (-1, 1) unless given"
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    rp = np.zeros(len(rows) + 1, dtype=np.int32)
    np.cumsum(lens, out=rp[1:])
    ci = (np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if len(rows) and rp[-1] else np.zeros(0)).astype(np.int32)
    vs = rng.uniform(-1, 1, size=len(ci)) if values is None else np.asarray(values, dtype=np.float64)
    assert len(vs) == len(ci) and (len(ci) == 0 or (ci.min() >= 0 and ci.max() < ncols))
    return Mat(len(rows), ncols, rp, ci, vs)


def transposed(m):
    "the transpose with the entries of a row in their source order (stable), float64 values: what mult_abt multiplies by"
    rows = np.repeat(np.arange(m.nrows, dtype=np.int32), np.diff(m.rowptrs))
    o = np.argsort(m.colinds, kind='stable')
    rp = np.zeros(m.ncols + 1, dtype=np.int64)
    np.cumsum(np.bincount(m.colinds, minlength=m.ncols), out=rp[1:])
    return Mat(m.ncols, m.nrows, rp.astype(m.rowptrs.dtype), rows[o], m.values[o].astype(np.float64))


def rows_ascend(m, strictly=True):
    "every row's columns ascend in storage order (sg_sorted_check asks for strictly)"
    if m.nnz < 2:
        return True
    d = np.diff(m.colinds.astype(np.int64))
    inner = np.ones(m.nnz - 1, dtype=bool)
    starts = np.asarray(m.rowptrs[1:-1], dtype=np.int64)
    starts = starts[(starts > 0) & (starts < m.nnz)]
    inner[starts - 1] = False                       # (the step from a row's last entry to the next row's first)
    return bool(np.all(d[inner] > 0) if strictly else np.all(d[inner] >= 0))


def no_column_twice(m):
    rows = np.repeat(np.arange(m.nrows, dtype=np.int64), np.diff(m.rowptrs))
    key = rows * m.ncols + m.colinds
    return np.unique(key).size == key.size


# ---- the products, written out -----------------------------------------------------------------------------------------

class Products:
    "every product a_ij b_jk of A R in the reference's order: row i, column k, A entry e, B entry kk (int64 arrays)"

    def __init__(self, a, r):
        lens = np.diff(r.rowptrs).astype(np.int64)
        per = lens[a.colinds]                                              # products of every entry of A
        c = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
        arp = np.asarray(a.rowptrs, dtype=np.int64)
        self.u = c[arp[1:]] - c[arp[:-1]]                                  # products of every row
        self.J = np.diff(arp)
        self.e = np.repeat(np.arange(a.nnz, dtype=np.int64), per)
        self.kk = np.asarray(r.rowptrs, dtype=np.int64)[a.colinds][self.e] + (np.arange(c[-1], dtype=np.int64) - c[:-1][self.e])
        self.row = np.repeat(np.arange(a.nrows, dtype=np.int64), self.u)
        self.col = r.colinds[self.kk].astype(np.int64)
        self.ncols = r.ncols
        key = np.unique(self.row * r.ncols + self.col)
        self.cnt = np.bincount(key // r.ncols, minlength=a.nrows).astype(np.int64)      # distinct output columns of every row


def ref_product(a, r, p=None):
    """
    A R with ascending columns, plainly: (rowptrs int32, colinds int32, values float64, bound) -- every product rounded once
    (to float32 when both operands are float32, multiply.py:120), the products of one output entry added in the reference's
    order; bound = the same sums over |a| |b|.
    """
    p = p or Products(a, r)
    if a.values.dtype == np.float32 and r.values.dtype == np.float32:
        prod = (a.values[p.e] * r.values[p.kk]).astype(np.float64)
    else:
        prod = a.values[p.e].astype(np.float64) * r.values[p.kk].astype(np.float64)
    key = p.row * p.ncols + p.col
    o = np.argsort(key, kind='stable')
    ks, ps = key[o], prod[o]
    first = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]])) if len(ks) else np.zeros(0, dtype=np.int64)
    vs, bound = np.zeros(len(first)), np.zeros(len(first))
    if len(first):
        ends = np.concatenate([first[1:], [len(ks)]])
        pos = first.copy()                    # one more product of every run still open per step: strictly front to back
        live = np.arange(len(first))
        while len(live):
            vs[live] += ps[pos[live]]
            bound[live] += np.abs(ps[pos[live]])
            pos[live] += 1
            live = live[pos[live] < ends[live]]
    rp = np.zeros(a.nrows + 1, dtype=np.int32)
    np.cumsum(p.cnt, out=rp[1:])
    return rp, (ks[first] % p.ncols).astype(np.int32), vs, bound


# ---- the routing, restated ---------------------------------------------------------------------------------------------

def ceil_div(a, b):
    return -(-int(a) // int(b))


def census(a, r, *, fast, b_sorted, esc=True, strips=True, fused=True, p=None, lim=LIMITS):
    """
    What spgemm_run does with the rows of A R (R the right operand as multiplied).  fast: both operands int32 / float64;
    b_sorted: the strips may rely on R's rows (strictly ascending for A B, always for A B^T); esc / strips / fused: the
    environment (CSRK_SPGEMM_ESC / _STRIPS / _FUSED not 0).  Returns a dict: the fields of csrk_spgemm_last_stats under their
    names, and per row `u`, `J`, `route` (0, 1 strips, 2 ESC, 3 large), `dense`, `cnt`, `large` ('lds' / 'hash' / 'hbm' for the
    large rows) and `small` (16 / 32 / 256: the lanes a route-0 row gets).
    """
    p = p or Products(a, r)
    u, J = p.u, p.J
    out = {k: 0 for k in STATS}
    out.update(general=1, fast=int(fast), u=u, J=J, cnt=p.cnt)
    if a.nnz == 0 or r.nnz == 0:
        out.update(route=np.zeros(a.nrows, dtype=np.int64), dense=np.zeros(a.nrows, dtype=bool), large={}, small={})
        return out
    s_dense = ceil_div(r.ncols, lim['SGS_W'])
    if s_dense > lim['SGS_MAX_S']:
        s_dense = 0
    n_strips = s_dense if (fast and strips and a.nrows * s_dense <= 1 << 30) else 0
    if n_strips and r.nnz > 1 and not b_sorted:
        n_strips = 0
    dense = (s_dense > 0) & (u >= lim['SGS_MIN_PER_CELL'] * J * s_dense) & (u >= lim['SGS_MIN_PER_UNIT'] * s_dense)
    route = np.zeros(a.nrows, dtype=np.int64)
    big = u > lim['SG_CAP']
    to_strip = big & dense & (n_strips > 0)
    to_esc = ~to_strip & (u > 0) & bool(esc) & (u > lim['SGE_MIN']) & ~(dense & big)
    to_large = ~to_strip & ~to_esc & big
    route[to_strip], route[to_esc], route[to_large] = 1, 2, 3
    small = {}
    for i in np.flatnonzero((route == 0) & (u > 0)):
        small[int(i)] = 16 if u[i] <= SG_QUAD_CAP else 32 if u[i] <= lim['SG_WAVE_CAP'] else 256
    large = {}
    counted = r.ncols <= lim['SGL_MAXBITS']
    for i in np.flatnonzero(to_large):
        c = int(p.cnt[i])
        if not counted:
            large[int(i)] = 'hbm'
        elif 8 * c >= r.ncols and r.ncols <= lim['SGL_W'] * lim['SGL_MAXTILES']:
            large[int(i)] = 'lds'
        else:
            large[int(i)] = 'hash' if c <= lim['SGB_CAP'] else 'hbm'
    kinds = list(large.values())
    n_strip = int(to_strip.sum())
    out.update(strips=n_strips, strip_rows=n_strip, strip_entries=int(J[to_strip].sum()), strip_fused=int(bool(fused) and n_strip > 0),
               esc_rows=int(to_esc.sum()), esc_products=int(u[to_esc].sum()), large_rows=len(large),
               lds_symbolic=int(len(large) > 0 and counted), lds_rows=kinds.count('lds'), hash_big_rows=kinds.count('hash'),
               hbm_rows=kinds.count('hbm'),
               small_fused=int(bool(fused) and any(v < 256 for v in small.values())),
               mid_rows=int(not esc or lim['SGE_MIN'] > SG_QUAD_CAP), hash_rows=int(not esc or lim['SGE_MIN'] > lim['SG_WAVE_CAP']),
               route=route, dense=dense, large=large, small=small)
    return out


def small_classes(u, route, lim):
    "rows of route 0 by the kernel that serves them, from the limits given: (16-lane, 32-lane, workgroup hash)"
    z = (route == 0) & (u > 0)
    return (int(np.sum(z & (u <= SG_QUAD_CAP))), int(np.sum(z & (u > SG_QUAD_CAP) & (u <= lim['SG_WAVE_CAP']))),
            int(np.sum(z & (u > lim['SG_WAVE_CAP']) & (u <= lim['SG_CAP']))))


# ---- a case ------------------------------------------------------------------------------------------------------------

ENV_KEYS = {'esc': 'CSRK_SPGEMM_ESC', 'strips': 'CSRK_SPGEMM_STRIPS', 'fused': 'CSRK_SPGEMM_FUSED'}


class Case:
    """
    a, b: the operands handed to the library; abt: the call is mult_abt (A B^T) and not mult_ab; env: the switches the case
    sets to 0 (a subset of 'esc', 'strips', 'fused'); pre: the preconditions, each a bool.
    """

    def __init__(self, a, b, abt=False, off=(), pre=None):
        self.name = None
        self.a, self.b, self.abt, self.off = a, b, bool(abt), tuple(off)
        self.pre = dict(pre or {})
        self.r = transposed(b) if abt else b                       # the right operand as multiplied
        self.p = Products(a, self.r)
        self.fast = all(m.rowptrs.dtype == np.int32 and m.values.dtype == np.float64 for m in (a, self.r))
        self.b_sorted = True if abt else rows_ascend(self.r)
        self.census = census(a, self.r, fast=self.fast, b_sorted=self.b_sorted, p=self.p, **{k: k not in self.off for k in ENV_KEYS})
        self.exact = no_column_twice(self.r)                       # the sums are then the sequential loop's bits
        self.pre['the operands fit: A.ncols = rows of the right operand'] = a.ncols == self.r.nrows
        self.pre['B is no fully populated panel (the dense-panel route stays out)'] = self.r.nnz != self.r.nrows * self.r.ncols
        self.pre['at most 6 * 10^5 products'] = int(self.p.u.sum()) <= 600000

    def env(self):
        return {ENV_KEYS[k]: '0' for k in self.off}

    def rows(self, **want):
        "rows whose census entries equal `want` (u=..., route=..., dense=...)"
        m = np.ones(self.a.nrows, dtype=bool)
        for k, v in want.items():
            m &= self.census[k] == v
        return np.flatnonzero(m)

    def has(self, u, route, **more):
        return len(self.rows(u=u, route=route, **more)) > 0


def failed_preconditions(c):
    return [k for k, v in c.pre.items() if not v]


# ---- building blocks ---------------------------------------------------------------------------------------------------

class Builder:
    """
    A and B grown row by row.  A row of A is given as the rows of B it points at; every row of B is made for one row of A
    (`row(...)` returns its number), so a row's product count is the sum of the lengths it was built from.
    """

    def __init__(self, name, ncols):
        self.rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.ncols = ncols
        self.b_rows, self.a_rows = [], []
        self.a_vals, self.b_vals = {}, {}

    def brow(self, cols, sort=True, values=None):
        cols = np.asarray(cols, dtype=np.int64)
        if sort and values is None:                # (given values go with the columns as given)
            cols = np.sort(cols)
        self.b_rows.append(cols)
        if values is not None:
            self.b_vals[len(self.b_rows) - 1] = np.asarray(values, dtype=np.float64)
        return len(self.b_rows) - 1

    def pieces(self, u, piece, pool=None, disjoint=True, sort=True):
        "rows of B of `piece` columns (the last one shorter) holding u entries in all; disjoint: no column twice among them"
        pool = np.arange(self.ncols) if pool is None else np.asarray(pool)
        lens = [piece] * (u // piece) + ([u % piece] if u % piece else [])
        if disjoint:
            perm = self.rng.permutation(pool)[:u]
            assert len(perm) == u
            cuts = np.cumsum([0] + lens)
            return [self.brow(perm[cuts[t]:cuts[t + 1]], sort) for t in range(len(lens))]
        return [self.brow(self.rng.choice(pool, size=n, replace=False), sort) for n in lens]

    def arow(self, js, values=None):
        self.a_rows.append(np.asarray(js, dtype=np.int64))
        if values is not None:
            self.a_vals[len(self.a_rows) - 1] = np.asarray(values, dtype=np.float64)
        return len(self.a_rows) - 1

    def target(self, u, piece, **kw):
        "a row of A with exactly u products"
        return self.arow(self.pieces(u, piece, **kw))

    def finish(self, extra_b_rows=0):
        for _ in range(extra_b_rows):
            self.b_rows.append(np.zeros(0, dtype=np.int64))
        b = mat(self.b_rows, self.ncols, self.rng)
        for j, v in self.b_vals.items():
            b.values[b.rowptrs[j]:b.rowptrs[j + 1]] = v
        a = mat(self.a_rows, len(self.b_rows), self.rng)
        for i, v in self.a_vals.items():
            a.values[a.rowptrs[i]:a.rowptrs[i + 1]] = v
        return a, b


CASES = {}


def case(name):
    def reg(fn):
        CASES[name] = fn
        return fn
    return reg


TYPINGS = {'a64': dict(a=dict(ptr64=True)), 'b64': dict(b=dict(ptr64=True)), 'ab64': dict(a=dict(ptr64=True), b=dict(ptr64=True)),
           'af32': dict(a=dict(f32=True)), 'bf32': dict(b=dict(f32=True)), 'abf32': dict(a=dict(f32=True), b=dict(f32=True))}
TYPED_BASES = ('ladder', 'esc-tiles', 'fb-20096')


def build(name):
    "the case of that name; 'base@typing' is `base` with int64 row pointers or float32 values on A, B or both (the general form)"
    base, _, typing = name.partition('@')
    c = CASES[base](base)
    if typing:
        t = TYPINGS[typing]
        c = Case(c.a.retyped(**t.get('a', {})), c.b.retyped(**t.get('b', {})), c.abt, c.off, c.pre)
        c.pre['the general form: not FAST, no strip rows'] = c.census['fast'] == 0 and c.census['strips'] == 0 and c.census['strip_rows'] == 0
    c.name = name
    return c


def names(prefix=''):
    out = list(CASES) + [f'{b}@{t}' for b in TYPED_BASES for t in TYPINGS]
    return [n for n in out if n.startswith(prefix)]


# ---- route 0: the ladder and the tables' probe chains --------------------------------------------------------------------

LADDER = (1, 31, 32, 33, 127, 128, 129, 1023, 1024, 1025)


def _ladder(name, off):
    """
    Rows of 1 .. 1025 products, once with all output columns distinct and once drawn from 24 columns, an empty row of A and a
    row that points at empty rows of B only.  3000 columns: 4 strips, 2048 products for a strip row, so 1025 products are a
    large row (LDS tiles with 1025 distinct outputs of 3000, the big hash table with 24).
    """
    bld = Builder(name, 3000)
    pool = bld.rng.choice(3000, size=24, replace=False)
    for u in LADDER:
        bld.target(u, 40)
    for u in LADDER:
        bld.target(u, 24, pool=pool, disjoint=False, sort=False)
    bld.arow([])
    bld.arow([bld.brow([]), bld.brow([])])
    a, b = bld.finish()
    c = Case(a, b, off=off)
    n = len(LADDER)
    c.pre['rows 0..9 and 10..19 have the ladder\'s product counts'] = list(c.p.u[:n]) == list(LADDER) == list(c.p.u[n:2 * n])
    c.pre['distinct half: as many outputs as products'] = bool(np.all(c.p.cnt[:n] == c.p.u[:n]))
    c.pre['repeating half: at most 24 outputs'] = bool(np.all(c.p.cnt[n:2 * n] <= 24))
    c.pre['rows of no product: an empty row of A, a row of empty rows of B'] = c.p.J[2 * n] == 0 and c.p.J[2 * n + 1] == 2 and c.p.u[2 * n + 1] == 0
    c.pre['32 / 33, 128 / 129 and 1024 / 1025 products part the kernels'] = (
        [c.census['small'].get(i) for i in range(n)] == [16, 16, 16, 32, 32, 32, 256, 256, 256, None] and c.census['route'][n - 1] == 3)
    c.pre['1025 products: LDS tiles when distinct, the big hash table when not'] = c.census['large'] == {n - 1: 'lds', 2 * n - 1: 'hash'}
    c.pre['no strip or ESC row'] = c.census['strip_rows'] == 0 and c.census['esc_rows'] == 0
    return c


@case('ladder')
def _(name):
    return _ladder(name, ('esc',))


@case('ladder-two-pass')
def _(name):
    c = _ladder(name, ('esc', 'fused'))
    c.pre['the small rows in two passes'] = c.census['small_fused'] == 0
    return c


@case('hash-wrap')
def _(name):
    """
    Rows whose columns all have their home in the last slots of their table, so that every probe chain runs over the table's
    end: 32 products on slot 62 of 64, 128 on slot 254 of 256, 600 on the last 8 of 2048 slots (200 000 columns hold 783 such).
    """
    nc = 200000
    bld = Builder(name, nc)
    k = np.arange(nc, dtype=np.uint64)
    h = (k * np.uint64(HASH_MUL)) & np.uint64(0xffffffff)
    p64 = np.flatnonzero((h & np.uint64(63)) == 62)
    p256 = np.flatnonzero((h & np.uint64(255)) == 254)
    p2048 = np.flatnonzero((h >> np.uint64(21)) >= SG_SLOTS - 8)
    bld.target(32, 8, pool=p64)
    bld.target(128, 32, pool=p256)
    bld.target(600, 100, pool=p2048, sort=False)
    bld.target(31, 8, pool=p64, disjoint=False)
    a, b = bld.finish()
    c = Case(a, b, off=('esc',))
    cols = [c.p.col[c.p.row == i] for i in range(3)]
    c.pre['row 0: 32 distinct columns, all at home in slot 62 of 64'] = len(set(cols[0])) == 32 and {quad_slot(x, SGQ_SLOTS[0]) for x in cols[0]} == {62}
    c.pre['row 1: 128 distinct columns, all at home in slot 254 of 256'] = len(set(cols[1])) == 128 and {quad_slot(x, SGQ_SLOTS[1]) for x in cols[1]} == {254}
    c.pre['row 2: 600 distinct columns at home in the last 8 of 2048 slots'] = len(set(cols[2])) == 600 and min(wg_slot(x) for x in cols[2]) >= SG_SLOTS - 8
    c.pre['16 lanes, 32 lanes, workgroup hash, 16 lanes'] = c.census['small'] == {0: 16, 1: 32, 2: 256, 3: 16}
    return c


# ---- expand, sort, compress -------------------------------------------------------------------------------------------

def esc_positions(c):
    "(row, column) of every position of the sorted product matrix, for cases whose ESC rows are listed in row order"
    m = c.census['route'][c.p.row] == 2
    key = c.p.row[m] * c.p.ncols + c.p.col[m]
    key = np.sort(key, kind='stable')
    return key // c.p.ncols, key % c.p.ncols


@case('esc-tiles')
def _(name):
    """
    5000 columns (7 strips: no row here is strip-dense), B's rows unsorted.  ESC rows in order: 33 products; 991 (the row
    ends on position 1023, tile 0's last, on column 2999); a row that starts tile 1 on column 2999 again; a row of 1500 + 300
    entries of A -- 1500 rows of B that hold column 3000 alone, a run over three tiles, the rest empty rows of B and short
    ones --; a row whose first two products cancel to 0.0 exactly; a row with a -0.0 product alone on its column.
    """
    T = LIMITS['SGE_TILE']
    bld = Builder(name, 5000)
    rng = bld.rng
    low, high = np.arange(0, 2999), np.arange(3001, 5000)
    bld.target(32, 8, sort=False)                                              # (route 0: the other side of 32 / 33)
    bld.target(33, 8, pool=low, disjoint=False, sort=False)
    js = bld.pieces(T - 33 - 1, 37, pool=low, disjoint=False, sort=False)
    bld.arow(js + [bld.brow([2999])])                                          # ESC positions 33 .. 1023
    bld.arow([bld.brow([2999, 4000, 3500])] + bld.pieces(60, 7, pool=high, disjoint=False, sort=False))      # 1024 .. 1086
    ones = [bld.brow([3000]) for _ in range(1500)]
    fill = []
    for t in range(300):
        fill.append(bld.brow(rng.choice(low, size=int(t % 5), replace=False), sort=False))       # (every fifth one empty)
    mix = list(ones[:700]) + fill[:150] + list(ones[700:]) + fill[150:]
    bld.arow(mix)
    b1, b2 = bld.brow([17, 4100], sort=False, values=[0.75, 0.5]), bld.brow([17], values=[0.75])
    bld.arow([b1, b2] + bld.pieces(40, 8, pool=high, disjoint=False, sort=False), values=[0.3, -0.3] + [0.5] * 5)
    bz = bld.brow([4242], values=[0.0])
    bld.arow([bz] + bld.pieces(36, 9, pool=low, disjoint=False, sort=False), values=[-1.5] + [0.25] * 4)
    a, b = bld.finish()
    c = Case(a, b)
    prow, pcol = esc_positions(c)
    cs = c.census
    c.pre['fewer than 1024 rows: ESC rows are listed in row order'] = a.nrows < LIST_THREADS
    c.pre['32 products: 16 lanes; 33: ESC'] = cs['small'] == {0: 16} and cs['route'][1] == 2 and c.p.u[1] == 33
    c.pre['rows 1..6 are ESC rows, nothing else'] = list(cs['route']) == [0, 2, 2, 2, 2, 2, 2]
    c.pre['row 2 ends on tile 0\'s last position'] = int(np.flatnonzero(prow == 2)[-1]) == T - 1
    c.pre['column 2999 is last in row 2 and first in row 3, across the tile boundary'] = (
        prow[T - 1] == 2 and prow[T] == 3 and pcol[T - 1] == 2999 == pcol[T])
    run = np.flatnonzero((prow == 4) & (pcol == 3000))
    c.pre['the run of column 3000 in row 4 is 1500 long and touches three tiles'] = (
        len(run) == 1500 and run[-1] - run[0] == 1499 and run[-1] // T - run[0] // T == 2)
    c.pre['row 4 has more than 256 entries of A (several expand batches), 60 of them on empty rows of B'] = (
        c.p.J[4] == 1800 > EXPAND_BATCH and int(np.sum(np.diff(b.rowptrs)[a.colinds[a.rowptrs[4]:a.rowptrs[5]]] == 0)) == 60)
    rp, ci, vs, _ = ref_product(a, b, c.p)
    v5 = dict(zip(ci[rp[5]:rp[6]], vs[rp[5]:rp[6]]))
    v6 = dict(zip(ci[rp[6]:rp[7]], vs[rp[6]:rp[7]]))
    c.pre['row 5 keeps an entry that cancels to +0.0'] = 17 in v5 and v5[17] == 0.0 and not np.signbit(v5[17])
    c.pre['row 6 holds the sum of one -0.0 product: +0.0'] = 4242 in v6 and v6[4242] == 0.0 and not np.signbit(v6[4242])
    c.pre['B\'s rows are unsorted: no strips'] = not c.b_sorted and cs['strips'] == 0
    return c


def _esc_total(name, total):
    "three ESC rows of 700 + 700 + (total - 1400) products over 300 columns (the columns repeat, runs of every length)"
    bld = Builder(name, 300)
    for u in (700, 700, total - 1400):
        bld.target(u, 50, disjoint=False, sort=False)
    bld.target(20, 5)
    a, b = bld.finish()
    c = Case(a, b)
    c.pre[f'{total} positions in the sorted product matrix'] = c.census['esc_products'] == total and c.census['esc_rows'] == 3
    c.pre['their number mod 4 and mod 1024'] = (total % 4, total % LIMITS['SGE_TILE']) == {2048: (0, 0), 2049: (1, 1), 2050: (2, 2), 2051: (3, 3)}[total]
    return c


for _t in (2048, 2049, 2050, 2051):
    CASES[f'esc-total-{_t}'] = (lambda t: lambda name: _esc_total(name, t))(_t)


# ---- column strips -----------------------------------------------------------------------------------------------------

def _strip_pre(c, pairs, builder=None):
    cs = c.census
    for lo, hi in pairs:
        c.pre[f'{lo} products: ESC, {hi}: strips'] = c.has(lo, 2) and c.has(hi, 1)
    if builder is not None:
        c.pre[f'strip table by {builder}'] = (c.r.nrows <= 2 * cs['strip_entries']) == (builder == 'row starts')
    c.pre['FAST, B\'s rows ascend'] = c.fast and c.b_sorted and cs['strips'] > 0


@case('strips-s1')
def _(name):
    """
    832 columns: one strip.  8 entries of A on rows of B of 128 (1024 products: ESC) against 129 (1025: strips); 300 entries
    and 1199 products (under 4 per entry: ESC) against 1200; rows of 1023, 1024 and 1025 entries of A on rows of B of 4 (the
    heavy-first pass takes 1024 and more).
    """
    bld = Builder(name, 832)
    bld.target(1024, 128, disjoint=False)
    bld.arow([bld.pieces(129, 129)[0] for _ in range(7)] + bld.pieces(122, 122))
    bld.target(8 * 129, 129, disjoint=False)
    bld.target(1199, 4, disjoint=False)
    bld.target(1200, 4, disjoint=False)
    for J in (1023, 1024, 1025):
        bld.target(4 * J, 4, disjoint=False)
    a, b = bld.finish()
    c = Case(a, b)
    _strip_pre(c, [(1024, 1025), (1199, 1200)], 'row starts')
    c.pre['one strip'] = c.census['strips'] == 1
    c.pre['1024 products on 8 entries of A'] = c.p.J[0] == 8 and c.p.J[1] == 8 and c.p.u[1] == 1025
    c.pre['1199 / 1200 products on 300 entries: 4 J S - 1 and 4 J S'] = c.p.J[3] == 300 == c.p.J[4]
    c.pre['strip rows of 1023, 1024 and 1025 entries of A'] = all(len(c.rows(J=J, route=1)) == 1 for J in (1023, LIMITS['SGS_HEAVY_J'], 1025))
    return c


def _strips_s3(name, off=()):
    """
    2400 columns: three strips.  1535 products (512 S - 1: ESC) against 1536; a strip row whose columns are 832 and 1663
    (strip 1's first and last) and strip 0's 0 and 831, nothing in strip 2; the clash path: a row whose first 64 entries of A
    point at rows of B that hold column 900 alone (a chunk of 64 positions, every lane on one address), and one with 32
    other entries in front of 64 such on column 1663 (the 64 lie across two batches); unused and empty rows of B behind, so
    that B has more than twice the strip rows' entries of A: the table is built by bisection.
    """
    bld = Builder(name, 2400)
    bld.arow(bld.pieces(11 * 128, 128) + bld.pieces(127, 127))
    bld.target(1536, 128)
    edge = [0, 831, 832, 1663]
    s01 = np.arange(0, 1664)
    bld.arow([bld.brow(np.union1d(edge, bld.rng.choice(s01, size=130, replace=False))) for _ in range(12)])
    bld.arow([bld.brow([900]) for _ in range(64)] + bld.pieces(1600, 160, disjoint=False))
    bld.arow(bld.pieces(32 * 30, 30, disjoint=False) + [bld.brow([1663]) for _ in range(64)] + bld.pieces(800, 200, disjoint=False))
    a, b = bld.finish(extra_b_rows=600)
    c = Case(a, b, off=off)
    _strip_pre(c, [(1535, 1536)], 'bisection')
    c.pre['three strips'] = c.census['strips'] == 3
    col2 = c.p.col[c.p.row == 2]
    c.pre['row 2 is a strip row on columns 0, 831, 832 and 1663, with strip 2 empty'] = (
        c.census['route'][2] == 1 and set(edge) <= set(col2) and col2.max() == 1663)
    lens = np.diff(b.rowptrs)
    for i, first, col in ((3, 0, 900), (4, 32, 1663)):
        js = a.colinds[a.rowptrs[i]:a.rowptrs[i + 1]][first:first + 64]
        c.pre[f'row {i} is a strip row; its entries {first}..{first + 63} point at rows of B holding column {col} alone'] = (
            c.census['route'][i] == 1 and bool(np.all(lens[js] == 1)) and bool(np.all(b.colinds[b.rowptrs[js]] == col)))
    return c


@case('strips-s3')
def _(name):
    return _strips_s3(name)


@case('strips-s3-two-pass')
def _(name):
    c = _strips_s3(name, ('fused',))
    c.pre['the strips in two passes'] = c.census['strip_fused'] == 0 and c.census['strip_rows'] > 0
    return c


def _strips_wide(name, ncols):
    "128 entries of A on rows of B of 1024: 131072 products = 512 * 256 = 4 * 128 * 256, strip-dense with 256 strips exactly"
    bld = Builder(name, ncols)
    bld.target(131072, 1024)
    bld.target(40, 8)
    a, b = bld.finish()
    c = Case(a, b)
    s = ceil_div(ncols, LIMITS['SGS_W'])
    c.pre['131072 products on 128 entries of A'] = c.p.u[0] == 131072 and c.p.J[0] == 128
    if s <= LIMITS['SGS_MAX_S']:
        c.pre['256 strips: the row takes them'] = s == 256 == c.census['strips'] and c.census['route'][0] == 1
    else:
        c.pre['257 strips are one too many: ESC'] = s == 257 and c.census['strips'] == 0 and c.census['route'][0] == 2
    return c


CASES['strips-256'] = lambda name: _strips_wide(name, 832 * 256)
CASES['strips-257'] = lambda name: _strips_wide(name, 832 * 256 + 1)


@case('strips-abt-repeat')
def _(name):
    """
    A B^T where B stores one entry twice: the transpose's rows ascend, but not strictly (one holds a column twice).  1600
    columns of the product: two strips; a strip row over the repeated entry, an ESC row beside it.
    """
    bld = Builder(name, 1600)
    js = bld.pieces(1400, 140, disjoint=False)
    bld.arow(js)
    bld.target(500, 50, disjoint=False)
    bld.b_rows[js[0]] = np.sort(np.concatenate([bld.b_rows[js[0]], bld.b_rows[js[0]][:1]]))       # one column twice
    a, r = bld.finish()
    b = transposed(r)
    c = Case(a, b, abt=True)
    c.pre['the right operand as multiplied holds a column twice in a row; its rows still ascend'] = (
        not c.exact and rows_ascend(c.r, strictly=False) and not rows_ascend(c.r))
    c.pre['two strips, one strip row and one ESC row'] = c.census['strips'] == 2 and list(c.census['route']) == [1, 2]
    c.pre['1401 products in the strip row'] = c.p.u[0] == 1401
    return c


# ---- fallbacks -----------------------------------------------------------------------------------------------------------

def _fallback(name, ncols, counts, off=('esc', 'strips'), edge_cols=()):
    "large rows of `counts` products, all on distinct columns (rows of B of 157 entries), `edge_cols` among those of every row"
    bld = Builder(name, ncols)
    for u in counts:
        pool = np.setdiff1d(np.arange(ncols), edge_cols)
        js = bld.pieces(u - len(edge_cols), 157, pool=pool)
        if len(edge_cols):
            js.insert(len(js) // 2, bld.brow(edge_cols))
        bld.arow(js)
    bld.target(1024, 128)
    a, b = bld.finish()
    c = Case(a, b, off=off)
    c.pre['every large row has as many distinct outputs as products'] = all(c.p.cnt[i] == c.p.u[i] == u for i, u in enumerate(counts))
    c.pre['1024 products: the workgroup hash kernel, not a large row'] = c.census['small'] == {len(counts): 256}
    return c


@case('fb-20096')
def _(name):
    "20096 columns, one LDS tile: 8 * 2512 = 20096 distinct outputs make a tile row, 2511 a big-hash row"
    c = _fallback(name, 20096, (2512, 2511, 1025), edge_cols=(0, 20095))
    c.pre['2512 outputs: LDS tiles; 2511 and 1025: the big hash table'] = c.census['large'] == {0: 'lds', 1: 'hash', 2: 'hash'}
    c.pre['one tile of columns'] = ceil_div(c.r.ncols, LIMITS['SGL_W']) == 1
    return c


@case('fb-20097')
def _(name):
    "20097 columns, two LDS tiles (the second holds column 20096 alone): 8 * 2513 >= 20097 > 8 * 2512"
    c = _fallback(name, 20097, (2513, 2512), edge_cols=(20095, 20096))
    c.pre['2513 outputs: LDS tiles; 2512: the big hash table'] = c.census['large'] == {0: 'lds', 1: 'hash'}
    c.pre['two tiles of columns'] = ceil_div(c.r.ncols, LIMITS['SGL_W']) == 2
    return c


@case('fb-160768')
def _(name):
    "160768 columns = 8 LDS tiles: 20096 outputs make a tile row, 20095 and 4097 HBM work rows, 4096 a big-hash row"
    c = _fallback(name, 160768, (20096, 20095, 4097, 4096), edge_cols=(20095, 20096, 160767))
    c.pre['20096: LDS tiles; 20095, 4097: HBM work rows; 4096: the big hash table'] = c.census['large'] == {0: 'lds', 1: 'hbm', 2: 'hbm', 3: 'hash'}
    c.pre['eight tiles of columns, the most'] = c.r.ncols == LIMITS['SGL_W'] * LIMITS['SGL_MAXTILES']
    return c


@case('fb-160769')
def _(name):
    "160769 columns: a ninth tile is one too many -- 20097 outputs (8 * 20097 >= 160769) still make an HBM work row"
    c = _fallback(name, 160769, (20097, 4097, 4096), edge_cols=(160768,))
    c.pre['20097, 4097: HBM work rows; 4096: the big hash table'] = c.census['large'] == {0: 'hbm', 1: 'hbm', 2: 'hash'}
    c.pre['8 cnt >= ncols holds for row 0: only the tile limit keeps it off the tiles'] = 8 * c.p.cnt[0] >= c.r.ncols
    return c


@case('fb-no-lds-count')
def _(name):
    "2^20 + 1 columns: the distinct outputs are not counted in LDS, both large rows are HBM work rows"
    c = _fallback(name, (1 << 20) + 1, (1025, 3000), edge_cols=(0, 1 << 20))
    c.pre['no LDS count, two HBM work rows'] = c.census['lds_symbolic'] == 0 and c.census['large'] == {0: 'hbm', 1: 'hbm'}
    return c


@case('fb-unsorted')
def _(name):
    """
    The default environment, B's rows unsorted: no strips, and the rows that are strip-dense above 1024 products are large
    rows (the others ESC rows).  20096 columns (25 strips: 12800 products on at most 128 entries of A are strip-dense):
    12800 distinct outputs (LDS tiles), 12800 products on 2000 columns (the big hash table), 12799 products (ESC).
    """
    bld = Builder(name, 20096)
    bld.arow(bld.pieces(12800, 128, sort=False))
    pool = bld.rng.choice(20096, size=2000, replace=False)
    bld.arow(bld.pieces(12800, 128, pool=pool, disjoint=False, sort=False))
    bld.arow(bld.pieces(12799, 128, pool=pool, disjoint=False, sort=False))
    a, b = bld.finish()
    c = Case(a, b)
    c.pre['B\'s rows are unsorted: no strips'] = not c.b_sorted and c.census['strips'] == 0
    c.pre['12800 products: strip-dense, large (tiles, big hash); 12799: ESC'] = (
        list(c.census['dense']) == [True, True, False] and c.census['large'] == {0: 'lds', 1: 'hash'} and c.census['route'][2] == 2)
    return c


@case('fb-unsorted-wide')
def _(name):
    "the same at 166400 columns (200 strips, more than 8 tiles): 102400 distinct outputs on 128 entries of A, an HBM work row"
    bld = Builder(name, 166400)
    bld.arow(bld.pieces(102400, 800, sort=False))
    bld.target(50, 10, sort=False)
    a, b = bld.finish()
    c = Case(a, b)
    c.pre['strip-dense, B unsorted: an HBM work row by default'] = (
        not c.b_sorted and bool(c.census['dense'][0]) and c.census['large'] == {0: 'hbm'} and c.census['esc_rows'] == 1)
    return c


# ---- the counting kernels' row classes and the walker's passes ---------------------------------------------------------

@case('count-classes')
def _(name):
    "rows of A of 64 / 65 and 4096 / 4097 entries (a sub-group, a wavefront, all wavefronts count them), three of them very long"
    bld = Builder(name, 5000)
    lens = (64, 65, 4096, 4097, 4100, 5000, 3)
    for J in lens:
        bld.arow([bld.brow(bld.rng.choice(5000, size=int(t % 3), replace=False)) for t in range(J)])
    a, b = bld.finish()
    c = Case(a, b)
    c.pre['rows of 64, 65, 4096, 4097, 4100 and 5000 entries'] = list(c.p.J) == list(lens)
    c.pre['on both sides of SG_COUNT_LONG and SG_COUNT_VLONG'] = (
        LIMITS['SG_COUNT_LONG'] in lens and LIMITS['SG_COUNT_LONG'] + 1 in lens and LIMITS['SG_COUNT_VLONG'] in lens
        and sum(J > LIMITS['SG_COUNT_VLONG'] for J in lens) == 3)
    return c


@case('count-all-long')
def _(name):
    """
    4096 rows of 65 .. 68 entries of A, every one long: 128 counting workgroups of 32 rows append to the 64 lists, two
    workgroups -- 64 rows, long_cap -- per list.  Rows of B of one entry.
    """
    bld = Builder(name, 700)
    one = [bld.brow([t]) for t in range(700)]
    for i in range(4096):
        bld.arow(bld.rng.choice(one, size=65 + i % 4, replace=False))
    a, b = bld.finish()
    c = Case(a, b)
    blocks = ceil_div(a.nrows * 8, 256)
    c.pre['every row is long'] = int(c.p.J.min()) > LIMITS['SG_COUNT_LONG']
    c.pre['128 workgroups, 64 rows per list = long_cap'] = blocks == 128 and ceil_div(blocks, 64) * 32 == 64 == a.nrows // 64
    return c


WALK = (16, 17, 32, 33, 64, 65, 144, 145, 256, 257, 288, 289, 2304, 2305)


@case('walker-lengths')
def _(name):
    """
    Rows of B of 16 / 17 ... 2304 / 2305 entries, each the second of three entries of a row of A (3 and 2 entries around it),
    fallback environment: the sub-wavefront kernels take 16 and 32 entries of a row of B per pass, the workgroup walker 256
    first and eight times 256 per further trip (2304 = 256 + 2048), the 1024-thread walkers 1024 and 8192.
    """
    bld = Builder(name, 12000)
    for L in WALK:
        perm = bld.rng.permutation(12000)[:L + 5]
        bld.arow([bld.brow(perm[:3]), bld.brow(perm[3:3 + L]), bld.brow(perm[3 + L:])])
    a, b = bld.finish()
    c = Case(a, b, off=('esc', 'strips'))
    lens = np.diff(b.rowptrs)
    c.pre['the middle entry of row t points at a row of B of WALK[t] entries'] = [int(lens[a.colinds[a.rowptrs[t] + 1]]) for t in range(len(WALK))] == list(WALK)
    c.pre['16-lane, 32-lane, workgroup-hash and LDS-tile rows'] = (
        sorted(set(c.census['small'].values())) == [16, 32, 256] and c.census['large'] == {12: 'lds', 13: 'lds'})
    return c


# ---- the ordering pass -------------------------------------------------------------------------------------------------

# csrc/spgemm_order_plan.h, restated (tests/test_spgemm_order_plan_host.py holds the two against each other on every case)
ORDER_LDS_MAX = 163840      # LDS a workgroup may have on the MI355X (hipDeviceAttributeMaxSharedMemoryPerBlock)
SO_LDS_BYTES = 150 * 1024   # dynamic LDS of the 1024-thread walk at most,
SO_TABLES_BYTES = 18 * 1024  # beside its static batch tables
SO_WIN_ENTRY = 2048         # bitmap words of its placing window by entry,
SO_WIN_COLS = (16384, 8192, 4096, 2048, 1024)      # and by column: the first that fits


def order_plan(c, lds_max=ORDER_LDS_MAX, lim=LIMITS):
    """
    What spgemm_apply_reference_order does with the rows of case c's product on a device of lds_max bytes of LDS per
    workgroup.  The 1024-thread walk works by column when 4 B per column of C, two bits and a window fit and B has fewer
    than 2^32 - 1 entries, else by entry with 8 B per entry of the row; a row is `listed` from SO_LEAST products on and then
    long (1024 threads), mid (256), wave or small by SO_MID, SO_WAVE, SO_TINY; its keys go through memory when it has 2^32 - 1
    products or, by entry, more entries than LDS holds.  `long_forms`: the forms the long rows take, of 'by column',
    'by entry in LDS', 'in memory'; `place`: so_place_kernel runs.
    """
    u, cnt = c.p.u, c.p.cnt
    budget = min(SO_LDS_BYTES, lds_max - SO_TABLES_BYTES)
    by_col = 4 * (c.r.ncols + 2 * ceil_div(c.r.ncols, 32))
    win_cols = next((w for w in SO_WIN_COLS if by_col + 8 * w <= budget), 0)
    cols = win_cols > 0 and c.r.nnz < 2 ** 32 - 1
    win_long = win_cols if cols else SO_WIN_ENTRY
    cap_long = 2 ** 31 - 1 if cols else max(0, budget - 8 * win_long) // 8
    listed = u >= lim['SO_LEAST']
    long = u >= lim['SO_MID']
    memory = listed & ((u >= 2 ** 32 - 1) | (cnt > cap_long))
    forms = {'in memory' if memory[i] else 'by column' if cols else 'by entry in LDS' for i in np.flatnonzero(long)}
    octave = np.array([63 - (int(v).bit_length() - 1) for v in u[listed]], dtype=np.int64)      # leading zeros of an int64
    counts = np.bincount(octave, minlength=64)
    return dict(budget=budget, by_col=by_col, win_cols=win_cols, cols_mode=int(cols), win_long=win_long, cap_long=cap_long,
                lds_long=by_col + 8 * win_long if cols else 8 * cap_long + 8 * win_long, win_mid=lim['SO_MID'] // 32, cap_mid=lim['SO_MID'],
                lds_mid=8 * lim['SO_MID'] + 8 * (lim['SO_MID'] // 32), lds_place=lim['SO_WIN'] // 32 * 8,
                ok=int(lim['SO_WIN'] // 32 * 8 + 2048 <= lds_max and cap_long >= lim['SO_MID']),
                listed=int(listed.sum()), n_long=int(long.sum()), n_mid=int(np.sum((u >= lim['SO_WAVE']) & ~long)),
                n_wave=int(np.sum((u >= lim['SO_TINY']) & (u < lim['SO_WAVE']))), n_small=int(np.sum(listed & (u < lim['SO_TINY']))),
                n_least=int(np.sum((u > 0) & ~listed)), keys_in_memory=int(memory.any()),
                cursors=[int(v) for v in np.concatenate([[0], np.cumsum(counts)[:-1]])], long_forms=forms,
                place=bool(long.any() and memory.any()))


ORDER_TIERS = (63, 64, 255, 256, 1023, 1024, 4095, 4096)


@case('order-tiers')
def _(name):
    "rows of 63 / 64, 255 / 256, 1023 / 1024, 4095 / 4096 products: both sides of every tier of the ordering pass"
    bld = Builder(name, 5000)
    for u in ORDER_TIERS:
        bld.target(u, 61, disjoint=False, sort=False)
    a, b = bld.finish()
    c = Case(a, b)
    c.pre['the rows\' product counts'] = list(c.p.u) == list(ORDER_TIERS)
    c.pre['one less than and exactly SO_LEAST, SO_TINY, SO_WAVE, SO_MID'] = all(
        LIMITS[k] in ORDER_TIERS and LIMITS[k] - 1 in ORDER_TIERS for k in ('SO_LEAST', 'SO_TINY', 'SO_WAVE', 'SO_MID'))
    return c


@case('order-window')
def _(name):
    "one row of 1024 entries of A on rows of B of 520: 532480 products, more than the placing window's 2^19 product indices"
    bld = Builder(name, 100000)
    bld.target(1024 * 520, 520, disjoint=False)
    bld.target(70, 10, disjoint=False)
    a, b = bld.finish()
    c = Case(a, b)
    c.pre['more than SO_WIN products in row 0'] = c.p.u[0] == 532480 > LIMITS['SO_WIN']
    c.pre['a strip row of 121 strips'] = c.census['strips'] == 121 and c.census['route'][0] == 1
    return c
