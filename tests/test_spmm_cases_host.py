"""
Host checks of tests/spmm_cases.py (no GPU, nothing from the library): every case reaches the edges it claims according to
the model; the model's places, buckets, ranges and light-row census equal numbers worked out by hand on tiny layouts; the
products of the bit-exact inputs are exact; and the two conditions without which the GPU test's bit comparison would be
vacuous hold for the model alone: the kernels' order of addition shows in the bits, and so does every boundary of the range
table.
"""
import numpy as np
import pytest

import spmm_cases as T

ALL = T.names()


def _bits(a):
    return (np.asarray(a) + 0.0).view(np.int64)


@pytest.mark.parametrize('name', ALL)
def test_case_reaches_what_it_claims(name):
    c = T.build(name)
    assert c.claims and not c.failed_claims(), c.failed_claims()
    assert c.family in T.LIGHT_FAMILIES + T.HEAVY_FAMILIES + ('unforced',)
    assert c.mode == ('0' if c.family in T.LIGHT_FAMILIES else None if c.family == 'unforced' else '1')
    if c.family in T.HEAVY_FAMILIES and c.family != 'all-heavy':
        lens = c.lens
        assert np.any(lens == 0) and np.any((lens >= 65) & (lens <= 255)) and np.any((lens > 0) & (lens <= 64)), name


def test_families_cover_the_issue():
    assert sorted(int(n.split(':')[1]) for n in T.names('seg-lengths')) == list(range(1, 16))
    assert {T.build(n).plan().n_segs % 4 for n in T.names('seg-lengths')} >= {1, 2, 3}
    assert [T.build(n).plan().R for n in T.names('few-tiles')] == [1, 1, 2, 2, 3, 7, 8, 8, 8]
    assert [T.build(n).ncols for n in T.names('few-tiles')] == [100, 128, 129, 256, 257, 896, 897, 1024, 1025]
    assert {T.build(n).plan().by_xcd() for n in T.names('few-tiles')} == {False, True}
    assert T.PROBES == (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 0)
    assert [T.build(f'places:{n}').plan().hr_n for n in (1, 15, 16, 17, 511, 512)] == [1, 15, 16, 17, 511, 512]
    assert T.build('places:513-g2').plan().stats()[2:4] == [513, 2] and T.build('places:1025-g4').plan().stats()[2:4] == [1025, 3]
    assert T.build('widths').ks == (1, 2, 3, 4, 5, 60, 63, 64, 65, 67, 68, 128, 129, 132)
    assert T.build('widths-heavy').ks == (1, 2, 63, 64, 65, 66, 127, 128, 129)
    assert [T.build(n).plan().on for n in T.names('unforced')] == [False, True, False, True, True, False]
    assert (T.SEG, T.UNIT, T.CHUNK, T.HR_ROWS, T.RPW, T.WAVES, T.TILE, T.KC, T.BATCH, T.MAXG, T.FLOOR_FORCED, T.FLOOR) == \
        (64, 16, 64, 512, 32, 16, 128, 64, 8, 8, 256, 512)


def _csr(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return rp, np.concatenate([np.asarray(r, dtype=np.int64) for r in rows])


def test_hand_worked_places_buckets_and_ranges():
    """
    Four rows per workgroup in two wavefronts, tiles of four columns, floor 3, a tile cost of 2, 12 columns (3 tiles), 2 CUs.
    Candidates, longest first then by row: 3 (7 entries), 0 (5), 2 (3), 4 (3) -- one group, threshold 3, all fit.
    Places: rank 0 -> wavefront 0 slot 0, rank 1 -> wavefront 1 slot 0, rank 2 -> wavefront 0 slot 1, rank 3 -> wavefront 1 slot 1.
    Wavefront 0 (rows 3 and 2) has 4 + 1, 1 + 1, 2 + 1 entries in tiles 0, 1, 2; wavefront 1 (rows 0 and 4) has 0, 4, 1 + 3.
    Entries before each tile: 0, 5, 11, 18.  Total cost 18 + 2 * 3 = 24; R = min(2, 3) = 2; the goal of range 1 is 12: after
    tile 0 the cost is 5 + 2 = 7 <= 12, after tile 1 it is 11 + 4 = 15 > 12: range 1 starts at tile 1.
    Light rows: row 1 (2 entries, segments of 1: two segments, both partial) and row 5 (empty: one segment).
    """
    rows = [[4, 5, 6, 7, 11], [1, 2], [0, 4, 8], [0, 1, 2, 3, 4, 8, 9], [9, 10, 11], []]
    rp, ci = _csr(rows)
    p = T.Plan(rp, ci, 12, 1, '1', cus=2, hr_rows=4, waves=2, tile=4, seg=1, floor=3, tile_cost=2)
    assert p.stats() == [1, 3, 4, 1, 2, 18, 3, 3, 2] and p.n_split == 1 and p.tie == 'fit'
    assert p.rows.tolist() == [3, 0, 2, 4]
    assert (p.group.tolist(), p.wave.tolist(), p.slot.tolist()) == ([0, 0, 0, 0], [0, 1, 0, 1], [0, 0, 1, 1])
    assert p.bucket_len[:, 0, :].tolist() == [[5, 0], [2, 4], [3, 4]]
    assert p.range.tolist() == [0, 1, 3] and not p.clamp
    # three CUs: three ranges of three tiles, whatever the costs -- the goal 8 is reached after tile 1 (7 <= 8 < 15), 16 after tile 2
    p3 = T.Plan(rp, ci, 12, 1, '1', cus=3, hr_rows=4, waves=2, tile=4, seg=1, floor=3, tile_cost=2)
    assert p3.R == 3 and p3.range.tolist() == [0, 1, 2, 3]
    # the same product whatever the table: 1 * B summed in the model's order equals the exact integer sums
    B = np.arange(1.0, 13.0).reshape(12, 1)
    want = [[sum(c + 1 for c in r)] for r in rows]
    assert T.product(p, None, B).tolist() == want and T.product(p3, None, B).tolist() == want
    # the order itself: row 3 under ranges [0, 1, 3] is (b0 + b1 + b2 + b3) + (b4 + b8 + b9), storage order inside a range
    v = np.array([1.0, 2.0 ** -60, 2.0 ** -60, -1.0, 2.0 ** -60, 1.0, -1.0])
    vals = np.ones(len(ci))
    vals[rp[3]:rp[4]] = v
    got = T.product(p, vals, np.ones((12, 1)))[3, 0]
    assert got == ((((0.0 + 1.0) + 2.0 ** -60) + 2.0 ** -60) - 1.0) + (((0.0 + 2.0 ** -60) + 1.0) - 1.0) == 0.0
    assert T.plain_sum(p, vals, np.ones((12, 1)), np.array([3]))[0, 0] == 0.0      # (left to right, everything small is lost too)
    got1 = T.product(p, vals, np.ones((12, 1)), ranges=[0, 2, 3])[3, 0]             # tile 1 moved into range 0: b4 survives
    assert got1 == (((((0.0 + 1.0) + 2.0 ** -60) + 2.0 ** -60) - 1.0) + 2.0 ** -60) + ((0.0 + 1.0) - 1.0) == 2.0 ** -60


def test_hand_worked_tie_rule_shrink_and_light_census():
    "two rows per workgroup, floor 3, segments of 2, columns 0 .. len - 1 of 8"
    def plan(lens, groups=1, cus=6):
        rp, ci = _csr([list(range(n)) for n in lens])
        return T.Plan(rp, ci, 8, 1, '1', groups=groups, cus=cus, hr_rows=2, waves=2, tile=4, seg=2, floor=3, tile_cost=2)
    # rows 0 (6) and 3 (5) are taken; the next candidate is shorter than 5: nothing comes along; rows 1, 2 split in two
    p = plan([6, 4, 4, 5, 1, 0])
    assert (p.tie, p.hr_min, p.rows.tolist(), p.G) == ('fit', 5, [0, 3], 1)
    assert (p.n_segs, p.n_multi, p.n_split) == (6, 4, 2) and p.segs.tolist() == [0, 2, 2, 0, 1, 1]
    # rows 0 (6) and 1 (5) are taken, rows 2 and 3 are as long as row 1 and do not fit: the threshold moves to 6, row 0 alone
    p = plan([6, 5, 5, 5])
    assert (p.tie, p.hr_min, p.rows.tolist(), p.G) == ('move', 6, [0], 1) and p.segs.tolist() == [0, 3, 3, 3]
    # three rows of one length under one group of two: none is left, the form is off and every row is split
    p = plan([5, 5, 5])
    assert (p.on, p.tie) == (False, 'off') and p.stats() == [0, 0, 0, 0, 0, 0, 0, 9, 9]
    # two groups forced, three candidates: ranks 0, 1, 2 -> groups 0, 1, 0; wavefronts 0, 0, 1; R = min(6 // 2, 2 tiles) = 2
    p = plan([6, 5, 4], groups=2)
    assert (p.G, p.R, p.rows.tolist(), p.group.tolist(), p.wave.tolist(), p.slot.tolist()) == (2, 2, [0, 1, 2], [0, 1, 0], [0, 0, 1], [0, 0, 0])
    # two groups forced, five candidates of which rows 1 .. 4 tie: taken 4, the fifth does not fit, threshold 6, one row, G shrinks to 1
    p = plan([6, 5, 5, 5, 5], groups=2)
    assert (p.tie, p.hr_min, p.rows.tolist(), p.G_before_shrink, p.G) == ('move', 6, [0], 2, 1)
    # the unforced rule: 4 gn >= 5 ncols (ncols = 8: 10 entries pay, 9 do not)
    rp, ci = _csr([list(range(6)), list(range(4))])
    kw = dict(hr_rows=2, waves=2, tile=4, seg=2, floor=3, tile_cost=2)
    assert T.Plan(rp, ci, 8, T.ENGAGE_BYTES // 64 + 1, None, **kw).on and not T.Plan(rp, ci, 8, T.ENGAGE_BYTES // 64, None, **kw).on
    rp, ci = _csr([list(range(6)), list(range(3))])
    assert not T.Plan(rp, ci, 8, T.ENGAGE_BYTES // 64 + 1, None, **kw).on


def test_workgroup_mapping():
    """
    Both mappings of spmm_hrows_kernel are one to one where they are used.  The mapping by XCD below 8 ranges is not only
    another one: with more than one group it yields a range index r >= R, so the kernel would read range_tile[r + 1] past the
    table's R + 1 entries and store its partial panel past hr_part.  That is why `by_xcd` forced true is a mutation this
    suite checks here, on the host, and never runs on a device.
    """
    for G in range(1, 9):
        for R in list(range(1, 8)) + [8, 16, 32, 64, 128, 256]:
            got = sorted(T.wg_place(b, G, R) for b in range(G * R))
            assert got == [(r, g) for r in range(R) for g in range(G)], (G, R)
            if R < 8 and G > 1:
                forced = [T.wg_place(b, G, R, True) for b in range(G * R)]
                assert sorted(forced) != got and max(r for r, _ in forced) >= R, (G, R)
    for n in T.names('few-tiles'):                      # the cases that run the plain mapping: two groups, R = 1 .. 7
        p = T.build(n).plan()
        if p.R < 8:
            assert p.G == 2 and max(T.wg_place(b, p.G, p.R, True)[0] for b in range(p.G * p.R)) >= p.R, n
    assert T.wg_place(9, 2, 8) == (1, 1) and T.wg_place(9, 2, 7) == (4, 1)      # block 9: XCD 1, second group / range 9 // 2


@pytest.mark.parametrize('name', ALL)
def test_products_are_exact(name):
    """
    every value of A and of the panel is a 24-bit integer times a power of two (checked on all of them), and the float64
    product of a sample of (entry, panel column) pairs equals the product of the two integers, worked out in Python integers
    """
    c = T.build(name)
    k = c.ks[-1]
    B = c.panel(k)
    for x in (c.values, B[np.unique(c.colinds)] if c.sparse_panel else B):
        m = np.ldexp(np.frexp(x)[0], 24)
        assert np.all(m == np.rint(m)) and np.all(np.abs(x) >= 2.0 ** -31) and np.all(np.abs(x) < 2.0 ** 14), name
    assert np.all(c.values.astype(np.float32).astype(np.float64) == c.values)
    rng = np.random.default_rng(5)
    e = rng.integers(0, c.nnz, size=300)
    j = rng.integers(0, k, size=300)
    a, b = c.values[e], B[c.colinds[e], j]
    (ma, ea), (mb, eb), (mp, ep) = T.exact_parts(a), T.exact_parts(b), T.exact_parts(a * b)
    for i in range(300):
        lo = min(ea[i] + eb[i], ep[i])
        assert ma[i] * mb[i] << (ea[i] + eb[i] - lo) == mp[i] << (ep[i] - lo) and ma[i] * mb[i] != 0, (name, i)


ORDER_CASES = [n for n in ALL if T.build(n).plan().on or np.any(T.build(n).plan().segs >= 3)]


@pytest.mark.parametrize('name', ORDER_CASES)
def test_order_shows_in_the_bits(name):
    """
    among the (row, column) sums of the rows that are heavy or split into three or more segments, the model's result differs
    in its bits from the plain left-to-right sum for at least half: an implementation that added in another order than the
    model's would be seen.  (A matrix of ONE tile has one range, and a heavy row's sum is then the left-to-right sum by
    construction -- few-tiles:100 and :128; that is asserted instead, and the split rows of those cases still count.)
    """
    c = T.build(name)
    p = c.plan()
    k = c.ks[-1] if c.family.startswith('widths') else c.ks[0]
    B = c.panel(k)
    rows = np.flatnonzero((p.segs >= 3) | ((p.segs == 0) & (p.tiles > 1)))
    assert len(rows)
    if p.on and p.tiles == 1:
        assert np.array_equal(_bits(T.product(p, c.values, B)[p.rows]), _bits(T.plain_sum(p, c.values, B, p.rows)))
    got = T.product(p, c.values, B)[rows]
    plain = T.plain_sum(p, c.values, B, rows)
    frac = float(np.mean(_bits(got) != _bits(plain)))
    print(f'{name}: {len(rows)} rows x {k} columns, {frac:.3f} of the sums differ from the left-to-right sum')
    assert frac >= 0.5, (name, frac)


@pytest.mark.parametrize('name', T.names('ranges'))
def test_every_range_boundary_shows_in_the_bits(name):
    """
    moving any one interior boundary of the range table by one tile, up or down (as far as the table stays monotone),
    changes at least one sum of the model: a wrong table cannot give the right bits
    """
    c = T.build(name)
    p = c.plan()
    B = c.panel(c.ks[0])
    prod = c.values[:, None] * B[c.colinds]
    part, fin = T.heavy_sums(p, prod, p.range)
    R, n = p.R, p.hr_n
    prefix = np.zeros((R + 1, n, B.shape[1]))
    for q in range(R):
        prefix[q + 1] = prefix[q] + part[:, q]
    assert np.array_equal(_bits(prefix[R]), _bits(fin))
    # the entries of the heavy rows by (rank, tile), storage order inside
    order = np.lexsort((p.h_tile, p.h_rank))
    sp, st, sr = prod[p.h_entry[order]], p.h_tile[order], p.h_rank[order]
    row0 = np.searchsorted(sr, np.arange(n))

    def partial(t0, t1):
        "the rows' sums over tiles [t0, t1)"
        lo = row0 + np.array([np.searchsorted(st[row0[i]:row0[i] + p.lens[p.rows[i]]], t0) for i in range(n)])
        hi = row0 + np.array([np.searchsorted(st[row0[i]:row0[i] + p.lens[p.rows[i]]], t1) for i in range(n)])
        return T.seq_sums(sp, lo, hi - lo)

    moved = 0
    for q in range(1, R):
        for d in (-1, 1):
            t = int(p.range[q]) + d
            if not p.range[q - 1] <= t <= p.range[q + 1]:
                continue
            acc = prefix[q - 1] + partial(int(p.range[q - 1]), t)
            acc = acc + partial(t, int(p.range[q + 1]))
            for r in range(q + 1, R):
                acc = acc + part[:, r]
            moved += 1
            assert np.any(_bits(acc) != _bits(fin)), (name, 'boundary', q, 'moved by', d)
    assert moved >= 2 * (R - 1) - 2, moved
