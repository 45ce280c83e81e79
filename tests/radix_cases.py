"""
Inputs that put the stable radix sort of csrc/transpose.hip (sort_records: transpose, from_coo, order_columns) on every one
of its routes and on the edges of each, and the plain NumPy statement of what it must return.  No GPU imports:
tests/test_radix_cases_host.py checks every case's preconditions and the reference against the oracle,
tests/test_gpu_radix_edges.py runs the library on the same cases.

The route is a function of two numbers (sort_records): bits = ceil(log2(key range)); one pass up to 8 bits, otherwise
ceil(bits / 8) passes; two passes with a payload range of at most 2^24 take the packed route (12-byte records, second-pass
chunks aligned to the first pass's runs), two passes with a larger payload range the plain one.  `transpose` sorts by column
with the source row as payload, `from_coo` by row with the column as payload.

Every case is built from a generator seeded with zlib.crc32 of its name, and carries `pre`: the properties that put it
on its edge ("holds key 65535 with payload 2^24 - 1", "the run of low digit 7 is exactly 4096 long"), each already
evaluated to a bool.  Both test files assert them, so an edit to a builder cannot silently move a case off its edge.
"""
import zlib

import numpy as np

CHUNK = 4096            # records per workgroup of one radix pass (RX_CHUNK)
HIST_GROUP = 4          # chunks per workgroup of the histogram (RX_HC)
SCAN_TRIP = 8192        # chunks per trip of the table scan (RXS_THREADS * RXS_IPT)
P24 = 1 << 24


# ---- the reference -----------------------------------------------------------------------------------------------------

def ref_sort(keys, payload, values, key_range):
    "stable sort of (key, payload, value) records by key: (run starts int64[key_range + 1], payload, values as float64 or None)"
    keys = np.asarray(keys)
    o = np.argsort(keys, kind='stable')
    ptr = np.zeros(key_range + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys, minlength=key_range), out=ptr[1:])
    return ptr, np.asarray(payload)[o], None if values is None else np.asarray(values)[o].astype(np.float64)


def ref_transpose(nrows, ncols, rowptrs, colinds, values):
    "(rowptrs of the input's width, colinds int32, values float64 or None) of the transposed matrix"
    rows = np.repeat(np.arange(nrows, dtype=np.int32), np.diff(rowptrs))
    ptr, pay, vs = ref_sort(colinds, rows, values, ncols)
    return ptr.astype(rowptrs.dtype), pay, vs


def ref_from_coo(nrows, rows, cols, values):
    "(rowptrs int32 -- int64 beyond 2^31 - 1 entries --, colinds int32, values of the input's dtype or None)"
    ptr, pay, vs = ref_sort(rows, cols, values, nrows)
    wide = len(rows) > np.iinfo(np.int32).max
    return ptr.astype(np.int64 if wide else np.int32), pay, None if values is None else vs.astype(values.dtype)


def ref_order_columns(nrows, rowptrs, colinds, values):
    "(colinds, values of the input's dtype or None) with every row sorted by column, equal columns in their stored order"
    rows = np.repeat(np.arange(nrows, dtype=np.int64), np.diff(rowptrs))
    o = np.lexsort((colinds, rows))
    return colinds[o], None if values is None else values[o]


def route(key_range, payload_range):
    "sort_records' choice, restated: '1', 'packed', 'plain2', '3' or '4'"
    bits = 0
    while bits < 31 and (1 << bits) < key_range:
        bits += 1
    passes = 1 if bits <= 8 else (bits + 7) // 8
    if passes == 2:
        return 'packed' if payload_range <= P24 else 'plain2'
    return str(passes)


def plain_chunks(n):
    return -(-n // CHUNK)


def aligned_chunks(keys):
    "chunks the packed route's second pass uses: every run of equal low digits is cut into chunks of its own"
    runs = np.bincount(np.asarray(keys) & 255, minlength=256)
    return int(np.sum(-(-runs // CHUNK)))


# ---- a case ------------------------------------------------------------------------------------------------------------

class Case:
    """
    op 'transpose' / 'order': a CSR (nrows, ncols, rowptrs, colinds, values); op 'from_coo': (nrows, ncols, rows, cols, values).
    `expect` is the route the case is meant for (for 'order': the routes of its two transposes); `pre` the preconditions.
    """

    def __init__(self, op, expect, nrows, ncols, a, b, values, pre=None):
        self.name = None
        self.op, self.expect, self.nrows, self.ncols, self.values = op, expect, int(nrows), int(ncols), values
        self.pre = dict(pre or {})
        if op == 'from_coo':
            self.rows, self.cols = a, b
            self.n = len(a)
            took = route(self.nrows, self.ncols)
        else:
            self.rowptrs, self.colinds = a, b
            self.n = len(b)
            self.pre['row pointers close on the entry count'] = int(a[0]) == 0 and int(a[-1]) == self.n and len(a) == self.nrows + 1
            took = route(self.ncols, self.nrows)
            if op == 'order':
                took = (took, route(self.nrows, self.ncols))
        self.pre[f'takes the route {expect}'] = took == expect
        if self.n:
            k = self.keys()
            self.pre['keys lie inside the key range'] = int(k.min()) >= 0 and int(k.max()) < (self.nrows if op == 'from_coo' else self.ncols)

    def keys(self):
        return self.rows if self.op == 'from_coo' else self.colinds

    def ref(self):
        if self.op == 'from_coo':
            return ref_from_coo(self.nrows, self.rows, self.cols, self.values)
        if self.op == 'transpose':
            return ref_transpose(self.nrows, self.ncols, self.rowptrs, self.colinds, self.values)
        return ref_order_columns(self.nrows, self.rowptrs, self.colinds, self.values)


def _vals(rng, n, kind):
    if kind is None:
        return None
    return rng.uniform(-1, 1, size=n).astype(np.float64 if kind == 'f64' else np.float32)


def _rowptrs(lens, ptr64=False):
    rp = np.zeros(len(lens) + 1, dtype=np.int64 if ptr64 else np.int32)
    np.cumsum(lens, out=rp[1:])
    return rp


def _has(keys, payload, k, p):
    return bool(np.any((keys == k) & (payload == p)))


# ---- A: key-range ladder -----------------------------------------------------------------------------------------------

LADDER = ((1, '1'), (2, '1'), (255, '1'), (256, '1'), (257, 'packed'), (65535, 'packed'), (65536, 'packed'), (65537, '3'),
          (P24, '3'), (P24 + 1, '4'))
EDGE_KEYS = (255, 256, 65535, 65536, P24 - 1, P24)


def _ladder_keys(rng, R, n):
    keys = rng.integers(0, R, size=n).astype(np.int32)
    forced = sorted({0, R - 1} | {k for k in EDGE_KEYS if k < R})
    keys[rng.choice(n, len(forced), replace=False)] = forced
    pre = {f'holds key {k}': bool(np.any(keys == k)) for k in forced}
    pre['about 20 000 records'] = 15000 <= n <= 25000
    return keys, pre


def ladder_transpose(rng, R, expect):
    "ncols = R: the key range; 700 rows of 0 .. 57 entries, float64 values, int32 pointers"
    lens = rng.integers(0, 58, size=700)
    n = int(lens.sum())
    ci, pre = _ladder_keys(rng, R, n)
    return Case('transpose', expect, 700, R, _rowptrs(lens), ci, _vals(rng, n, 'f64'), pre)


def ladder_from_coo(rng, R, expect, kind):
    "nrows = R: the key range; 20 000 entries in input order, columns below 5000"
    n = 20000
    rows, pre = _ladder_keys(rng, R, n)
    return Case('from_coo', expect, R, 5000, rows, rng.integers(0, 5000, size=n).astype(np.int32), _vals(rng, n, kind), pre)


# ---- B: payload edges of the two-pass routes ----------------------------------------------------------------------------

EDGE_COLS = (0, 255, 256, 32767, 32768, 65535)


def _hot(P):
    return [0, (1 << 23) - 1, 1 << 23, P24 - 2, P24 - 1] + ([P24] if P > P24 else [])


def _payload_pre(keys, payload, P):
    pre = {'holds key 65535 with payload 2^24 - 1 (every bit of the packed word set)': _has(keys, payload, 65535, P24 - 1),
           'holds key 32768 (sign bit of the word) with payload 2^23 (bit 23)': _has(keys, payload, 32768, 1 << 23),
           'holds key 0 with payload 0': _has(keys, payload, 0, 0),
           'holds the largest payload': bool(np.any(payload == P - 1)),
           'about 40 000 records': 35000 <= len(keys) <= 45000}
    if P > P24:
        pre['holds key 65535 with payload 2^24'] = _has(keys, payload, 65535, P24)
    return pre


def _edge_cols(rng, n):
    return np.where(rng.random(n) < 0.5, rng.choice(EDGE_COLS, size=n), rng.integers(0, 65536, size=n)).astype(np.int32)


def payload_transpose(rng, nrows, ptr64, expect):
    "nrows x 65536 with all entries in six rows at most: the payload (source row) has its top bits set"
    hot = _hot(nrows)
    lens = np.zeros(nrows, dtype=np.int64)
    lens[hot] = 40000 // len(hot) + rng.integers(-50, 50, size=len(hot))
    rp = _rowptrs(lens, ptr64)
    n = int(rp[-1])
    ci = _edge_cols(rng, n)
    for r in hot:                                   # every (hot row, edge column) pair exists
        ci[int(rp[r]):int(rp[r]) + len(EDGE_COLS)] = EDGE_COLS
    rows = np.repeat(np.arange(nrows, dtype=np.int32), lens)
    pre = _payload_pre(ci, rows, nrows)
    pre['only the hot rows hold entries'] = int(np.count_nonzero(lens)) == len(hot)
    return Case('transpose', expect, nrows, 65536, rp, ci, _vals(rng, n, 'f64'), pre)


def payload_from_coo(rng, ncols, expect):
    "the mirror: 65536 x ncols from unsorted COO entries whose columns (the payload) are the hot values"
    n = 40000
    hot = _hot(ncols)
    rows = _edge_cols(rng, n)
    cols = rng.choice(hot, size=n).astype(np.int32)
    pairs = [(k, p) for p in hot for k in EDGE_COLS]
    at = rng.choice(n, len(pairs), replace=False)
    rows[at] = [k for k, _ in pairs]
    cols[at] = [p for _, p in pairs]
    return Case('from_coo', expect, 65536, ncols, rows, cols, _vals(rng, n, 'f64'), _payload_pre(rows, cols, ncols))


# ---- C: record-count ladder --------------------------------------------------------------------------------------------

COUNTS = (1, 2, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 4 * 4096 - 1, 4 * 4096, 4 * 4096 + 1, 8 * 4096, 8 * 4096 + 1,
          9 * 4096 + 5)
COUNT_ROUTES = ((100, '1'), (1000, 'packed'), (70000, '3'))
KINDS = ('f64', 'f32', None)


def count_case(rng, ncols, n, expect):
    "exactly n entries in rows of 0 .. 40; values cycle through f64 / f32 / none as n goes up"
    lens = []
    left = n
    while left:
        k = min(int(rng.integers(0, 41)), left)
        lens.append(k)
        left -= k
    lens = np.array(lens + [0], dtype=np.int64)
    ci = rng.integers(0, ncols, size=n).astype(np.int32)
    pre = {f'{n} records': int(lens.sum()) == n, 'rows of 0 .. 40 entries': int(lens.max()) <= 40}
    return Case('transpose', expect, len(lens), ncols, _rowptrs(lens), ci, _vals(rng, n, KINDS[COUNTS.index(n) % 3]), pre)


# ---- D: run shapes for the aligned second pass ---------------------------------------------------------------------------

def _index_case(rng, keys, pre):
    "from_coo with 65536 rows (packed) whose payload is the source index: stability is directly visible"
    keys = np.asarray(keys, dtype=np.int32)
    n = len(keys)
    pre = dict(pre)
    pre['the payload is the source index'] = True
    c = Case('from_coo', 'packed', 65536, n, keys, np.arange(n, dtype=np.int32), _vals(rng, n, 'f64'), pre)
    return c


def run_one_key(rng, k):
    n = 3 * CHUNK + 7
    keys = np.full(n, k)
    return _index_case(rng, keys, {f'all {n} records have key {k}': bool(np.all(keys == k)) and n == 12295,
                                   'one run spans 4 aligned chunks': aligned_chunks(keys) == 4})


def run_256_singles(rng):
    keys = rng.integers(0, 256, size=256) * 256 + rng.permutation(256)
    return _index_case(rng, keys, {'every low digit exactly once': bool(np.all(np.bincount(keys & 255, minlength=256) == 1)),
                                   '256 aligned chunks against 1 plain chunk': (aligned_chunks(keys), plain_chunks(len(keys))) == (256, 1),
                                   'several high digits': len(np.unique(keys >> 8)) > 100})


def run_most_descriptors(rng):
    "every low digit holds 4096 q + 1 records, q in {0, 1}: ceil(n / 4096) + 255 aligned chunks, the most the descriptors hold"
    q = rng.integers(0, 2, size=256)
    q[:2] = (0, 1)
    low = np.repeat(np.arange(256), CHUNK * q + 1)
    keys = (rng.integers(0, 256, size=len(low)) * 256 + low)[rng.permutation(len(low))]
    runs = np.bincount(keys & 255, minlength=256)
    return _index_case(rng, keys, {'every run is 1 or 4097 long, both occur': set(runs.tolist()) == {1, CHUNK + 1},
                                   'aligned chunks used == plain chunks + 255': aligned_chunks(keys) == plain_chunks(len(keys)) + 255})


def run_exact_chunks(rng):
    "runs of exactly one and exactly two chunks between empty low digits"
    other = np.setdiff1d(np.arange(256), [6, 7, 8, 199, 200, 201])
    low = np.concatenate([np.full(CHUNK, 7), np.full(2 * CHUNK, 200), rng.choice(other, size=60)])
    keys = (rng.integers(0, 256, size=len(low)) * 256 + low)[rng.permutation(len(low))]
    runs = np.bincount(keys & 255, minlength=256)
    return _index_case(rng, keys, {'the run of low digit 7 is exactly 4096 long': runs[7] == CHUNK,
                                   'the run of low digit 200 is exactly 8192 long': runs[200] == 2 * CHUNK,
                                   'their neighbours are empty': not runs[[6, 8, 199, 201]].any(),
                                   'a few records elsewhere': 0 < runs.sum() - 3 * CHUNK <= 60})


def run_one_low_digit(rng, low):
    "only one low digit populated (255 leading or trailing empty runs), all 256 high digits present"
    high = np.concatenate([np.arange(256), rng.integers(0, 256, size=10000)])
    keys = high[rng.permutation(len(high))] * 256 + low
    return _index_case(rng, keys, {f'only low digit {low}': bool(np.all((keys & 255) == low)),
                                   'all 256 high digits': len(np.unique(keys >> 8)) == 256})


def run_multiples_of_256(rng):
    keys = rng.integers(0, 256, size=2 * CHUNK + 1) * 256
    return _index_case(rng, keys, {'keys are multiples of 256': not np.any(keys & 255), 'several keys': len(np.unique(keys)) > 200})


def run_below_256(rng):
    keys = rng.integers(0, 256, size=10000)
    return _index_case(rng, keys, {'keys below 256 in a range of 65536': int(keys.max()) < 256, 'all of them occur': len(np.unique(keys)) == 256})


def run_sorted(rng, descending):
    keys = np.repeat(np.sort(rng.choice(65536, size=400, replace=False)), rng.integers(40, 61, size=400))
    if descending:
        keys = keys[::-1].copy()
    d = np.diff(keys)
    return _index_case(rng, keys, {'descending input' if descending else 'ascending input': bool(np.all(d <= 0) if descending else np.all(d >= 0)),
                                   'each key about 50 times': 40 <= np.bincount(keys).max() <= 60 and len(np.unique(keys)) == 400})


# ---- E: source-row recovery in the first transpose pass -------------------------------------------------------------------

def _rows_case(rng, lens, ptr64, pre):
    lens = np.asarray(lens, dtype=np.int64)
    n = int(lens.sum())
    ci = rng.integers(0, 1000, size=n).astype(np.int32)
    return Case('transpose', 'packed', len(lens), 1000, _rowptrs(lens, ptr64), ci, _vals(rng, n, 'f64'), pre)


def _compose(rng, total, parts):
    "`parts` row lengths >= 1 that sum to `total`"
    cuts = np.sort(rng.choice(np.arange(1, total), size=parts - 1, replace=False))
    return np.diff(np.concatenate([[0], cuts, [total]]))


def rows_one_long(rng, ptr64):
    n = 3 * CHUNK + 5
    lens = np.concatenate([np.zeros(10000, np.int64), [n], np.zeros(10000, np.int64)])
    return _rows_case(rng, lens, ptr64, {'one row holds all 3 * 4096 + 5 entries': int(lens[10000]) == n == int(lens.sum()),
                                         '10 000 empty rows before it and after it': len(lens) == 20001})


def rows_singletons(rng, ptr64):
    n = 2 * CHUNK + 100
    return _rows_case(rng, np.ones(n, np.int64), ptr64, {f'{n} rows of one entry each': True})


def rows_start_on_edges(rng, ptr64):
    starts = [0, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 9000]
    lens = np.diff(starts)
    rp = np.concatenate([[0], np.cumsum(lens)])
    return _rows_case(rng, lens, ptr64, {'rows start at entries 4095, 4096, 4097 and 8192': rp.tolist() == [0, 4095, 4096, 4097, 8192, 9000]})


def rows_empty_at(rng, ptr64, pos):
    "5000 empty rows whose shared start is entry `pos`, between rows that hold entries"
    lens = np.concatenate([_compose(rng, pos, 100), np.zeros(5000, np.int64), _compose(rng, 3000, 50)])
    rp = np.concatenate([[0], np.cumsum(lens)])
    return _rows_case(rng, lens, ptr64, {f'5001 rows start at entry {pos}': int(np.sum(rp[:-1] == pos)) == 5001,
                                         'the last of them holds entries': int(lens[5100]) > 0 and int(rp[5100]) == pos})


def rows_single_row(rng, ptr64):
    return _rows_case(rng, [5000], ptr64, {'nrows == 1': True})


def rows_empty_margin(rng, ptr64, leading):
    body = rng.integers(1, 20, size=800)
    z = np.zeros(3000, np.int64)
    lens = np.concatenate([z, body] if leading else [body, z])
    return _rows_case(rng, lens, ptr64, {('leading' if leading else 'trailing') + ' empty rows only':
                                         bool(np.all(lens[:3000] == 0) if leading else np.all(lens[-3000:] == 0)) and int(body.min()) > 0,
                                         'more than one chunk': int(lens.sum()) > CHUNK})


def rows_sparse(rng, ptr64):
    lens = (rng.random(20000) < 0.2).astype(np.int64)
    lens[-1] = 1
    return _rows_case(rng, lens, ptr64, {'more than 4096 rows meet one chunk': len(lens) > 4 * CHUNK and int(lens.sum()) <= CHUNK,
                                         'about one row in five holds one entry': 3500 <= int(lens.sum()) and int(lens.max()) == 1})


# ---- F: more than 8192 chunks (the table scan's second trip) ------------------------------------------------------------

def many_chunks(rng):
    "structure-only from_coo, 200 rows (one pass); rows are a multiplicative hash of the index, the column is the index"
    n = SCAN_TRIP * CHUNK + CHUNK + 1
    i = np.arange(n, dtype=np.uint32)
    rows = (((i * np.uint32(2654435761)) >> np.uint32(16)) % np.uint32(200)).astype(np.int32)
    return Case('from_coo', '1', 200, n, rows, i.astype(np.int32), None,
                {'more than 8192 chunks': plain_chunks(n) > SCAN_TRIP, 'the last chunk holds one record': n % CHUNK == 1,
                 'the payload is the source index': True})


# ---- G: order_columns = two transposes on different routes ------------------------------------------------------------

def order_case(rng, nrows, ncols, maxlen, kind, expect):
    lens = rng.integers(0, maxlen + 1, size=nrows)
    corner = (nrows, ncols) == (65536, 65536)
    if corner:                                      # one row in twenty holds entries
        lens[rng.random(nrows) >= 0.05] = 0
        lens[-1] = 1
    n = int(lens.sum())
    ci = rng.integers(0, ncols, size=n).astype(np.int32)
    pre = {}
    if corner:
        ci[-1] = 65535
        pre['holds entry (65535, 65535)'] = int(lens[-1]) == 1 and int(ci[-1]) == 65535
        pre['about 30 000 entries'] = 25000 <= n <= 40000
    rp = _rowptrs(lens)
    key = np.repeat(np.arange(nrows, dtype=np.int64), lens) * ncols + ci
    pre['rows are not sorted'] = bool(np.any((np.diff(ci) < 0) & (np.diff(key // ncols) == 0)))
    if nrows == 100:
        pre['rows hold columns twice (stability shows)'] = len(np.unique(key)) < n
    return Case('order', expect, nrows, ncols, rp, ci, _vals(rng, n, kind), pre)


# ---- the registry --------------------------------------------------------------------------------------------------------

CASES = {}
for _i, (_R, _e) in enumerate(LADDER):
    CASES[f'A-transpose-{_R}'] = (ladder_transpose, (_R, _e))
    CASES[f'A-from_coo-{_R}'] = (ladder_from_coo, (_R, _e, 'f32' if _i % 2 else None))
for _P, _e in ((P24, 'packed'), (P24 + 1, 'plain2')):
    for _w in (32, 64):
        CASES[f'B-transpose-{_P}-ptr{_w}'] = (payload_transpose, (_P, _w == 64, _e))
    CASES[f'B-from_coo-{_P}'] = (payload_from_coo, (_P, _e))
for _nc, _e in COUNT_ROUTES:
    for _n in COUNTS:
        CASES[f'C-{_nc}-{_n}'] = (count_case, (_nc, _n, _e))
for _k in (0, 255, 256, 65535):
    CASES[f'D-a-one-key-{_k}'] = (run_one_key, (_k,))
CASES['D-b-256-singles'] = (run_256_singles, ())
CASES['D-c-most-descriptors'] = (run_most_descriptors, ())
CASES['D-d-exact-chunks'] = (run_exact_chunks, ())
CASES['D-e-low-digit-0'] = (run_one_low_digit, (0,))
CASES['D-e-low-digit-255'] = (run_one_low_digit, (255,))
CASES['D-f-multiples-of-256'] = (run_multiples_of_256, ())
CASES['D-f-below-256'] = (run_below_256, ())
CASES['D-g-ascending'] = (run_sorted, (False,))
CASES['D-g-descending'] = (run_sorted, (True,))
for _w in (32, 64):
    _p = (_w == 64,)
    CASES[f'E-a-one-long-row-ptr{_w}'] = (rows_one_long, _p)
    CASES[f'E-b-singletons-ptr{_w}'] = (rows_singletons, _p)
    CASES[f'E-c-starts-on-edges-ptr{_w}'] = (rows_start_on_edges, _p)
    CASES[f'E-d-empty-at-4096-ptr{_w}'] = (rows_empty_at, _p + (CHUNK,))
    CASES[f'E-d-empty-at-4095-ptr{_w}'] = (rows_empty_at, _p + (CHUNK - 1,))
    CASES[f'E-e-single-row-ptr{_w}'] = (rows_single_row, _p)
    CASES[f'E-e-leading-empty-ptr{_w}'] = (rows_empty_margin, _p + (True,))
    CASES[f'E-e-trailing-empty-ptr{_w}'] = (rows_empty_margin, _p + (False,))
    CASES[f'E-f-sparse-rows-ptr{_w}'] = (rows_sparse, _p)
CASES['F-many-chunks'] = (many_chunks, ())
ORDER_SHAPES = ((300, 70000, 60, ('3', 'packed')), (70000, 200, 2, ('1', '3')), (100, 100, 60, ('1', '1')),
                (65536, 65536, 19, ('packed', 'packed')))
for _nr, _nc, _ml, _e in ORDER_SHAPES:
    for _kind in KINDS:
        CASES[f'G-{_nr}x{_nc}-{_kind or "none"}'] = (order_case, (_nr, _nc, _ml, _kind, _e))


def names(prefix=''):
    return [k for k in CASES if k.startswith(prefix)]


def build(name):
    fn, args = CASES[name]
    c = fn(np.random.default_rng(zlib.crc32(name.encode())), *args)
    c.name = name
    return c


def failed_preconditions(c):
    return [k for k, ok in c.pre.items() if not ok]
