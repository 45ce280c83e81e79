"""
tests/tier1_cases.py without a GPU: every case reaches the edges it claims (so the GPU suite is known to run them before a GPU
is involved), the model gives the tiles, carries and groups worked out by hand on three layouts of a dozen entries,
panel_slot_of_rank restated is a permutation for every tile size, pair_sum's two orders are what the module says, and the
names the model reports under are the library's.  tests/test_gpu_spmv_tier1.py runs the library on the same cases.
"""
import numpy as np
import pytest

import tier1_cases as T

ALL = T.names()


def test_names_families_and_sizes():
    assert len(set(ALL)) == len(ALL) and len(ALL) >= 40
    fam = {T.build(n).family for n in ALL}
    assert fam == {'rows', 'blocks', 'tiles', 'long', 'carry', 'listed', 'groups', 'many', 'rider', 'neighbours', 'fallback'}
    a = T.build('blocks-edge')
    assert T.build('blocks-edge') is a and not a.colinds.flags.writeable and not a.x.flags.writeable
    assert max(T.build(n).nnz for n in ALL) <= 300000 and max(T.build(n).ncols for n in ALL) == 17 * T.BLOCK


def test_stat_names_are_the_librarys():
    from csr_amd.kernels import hip as K
    assert len(K.SPMV_PLAN_STATS) == 48 and set(T.STAT_KEYS) <= set(K.SPMV_PLAN_STATS)
    assert K.SPMV_PLAN_STATS[42:] == ('t1_blocks', 't1_tiles', 't1_carry_rows', 't1_listed_carries', 't1_groups', 't1_pad_groups')
    assert set(T.build('rows-1').layout.stats()) == set(T.STAT_KEYS)


@pytest.mark.parametrize('name', ALL)
def test_case_reaches_what_it_claims(name):
    c = T.build(name)
    assert c.claims and not c.failed_claims(), (c.failed_claims(), {k: c.census()[k] for k in c.failed_claims()})
    a = c.layout
    lens = np.diff(c.rowptrs.astype(np.int64))
    # the cut rows ascend inside (duplicates allowed), but for the fallback's one descending pair
    assert set(c.env()) <= set(T.ENV_KEYS) and c.env()['CSRK_SPMV_HEAVY_SPLIT'] == '1'
    if name != 'fallback':
        assert np.array_equal(np.sort(np.concatenate([a.t0, a.t1])), np.flatnonzero(lens >= c.tier1_min))
        assert np.all(lens[a.t1] < c.heavy_min) and np.all(lens[a.t0] >= c.heavy_min)
    # the layout's own invariants: every entry in one tile, tiles inside their blocks, the kernel's tables large enough
    assert int(a.t_nn.sum()) == a.entries == int(lens[a.t1].sum())
    nr = a.t_i1 - a.t_i0
    assert np.all(a.t_nn + nr <= T.ITEMS) and np.all(a.t_nn >= 0) and np.all(nr >= 0)
    assert np.all(a.t_i0 >= a.t_blk * a.n) and np.all(a.t_i1 <= (a.t_blk + 1) * a.n)
    assert c.census()['max_long_in_tile'] <= 31
    real = [g for g in a.groups if g[1]]
    assert sorted(g[0] for g in real) == list(range(a.n_tiles)) and all(a.t_blk[g[0]] == g[2] for g in real)
    if a.nb >= T.STREAM_MIN:
        assert all(g[2] % T.STREAMS == k % T.STREAMS for k, g in enumerate(a.groups) if g[1])


def test_edges_are_covered_by_some_case():
    "the union of the censuses holds every edge of the issue's list"
    cs = {n: T.build(n).census() for n in ALL}
    some = lambda key, ok=lambda v: v > 0: [n for n in ALL if ok(cs[n][key])]
    for key in ('tiles_nr0', 'tiles_nn0', 'tiles_nn1', 'tiles_nn_odd', 'tiles_nn_lt_chunk', 'tiles_nn_chunk', 'tiles_nn_chunk1',
                'tiles_nn_full', 'tiles_partial_last_chunk', 'pairs_63', 'pairs_64', 'pairs_65', 'rows_carries_4', 'rows_carries_5',
                'rows_carries_68', 'rows_carries_69', 't1_pad_groups', 'empty_blocks', 'col_off_0', 'col_off_last',
                'exact_rows_short', 'exact_rows_long', 't0_rows'):
        assert some(key), key
    assert some('max_long_in_tile', lambda v: v == 31) and some('tiles_most_row_ends', lambda v: v == T.ITEMS)
    assert some('t1_blocks', lambda v: v >= 2) and some('last_block_width', lambda v: v == 1)
    assert some('last_nn', lambda v: v > 1024 and v % 2 == 1)            # the pair load's clamp at the panel's last entry
    assert some('t1_rows', lambda v: v > 256) and some('t1_rows', lambda v: v > 2048)
    assert sorted(cs[n]['t1_listed_carries'] for n in T.names('carry', 'listed')) == [0, 1, 1, 2, 64, 65, 65, 66]
    for fam in ('rows', 'blocks', 'tiles'):
        for n in T.names(fam):
            assert cs[n]['exact_rows'] >= min(10, cs[n]['t1_rows']), n


def _layout(rows, ncols, **kw):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return T.Layout(rp, np.concatenate(rows), ncols, 64, 2, **kw)


def test_model_by_hand():
    # 1. one block of 8 columns, tiles of 4 items, rows of 3 and 2 entries and a light row of 1 between them.
    #    path: e e e END0 | e e END1 -> tile 0 = (i0 0, i1 1, 3 entries), tile 1 = (1, 2, 2); tile 0 ends ON pair 1: an empty carry of row 1
    a = _layout([[0, 1, 2], [5], [3, 4]], 8, block=8, items=4)
    assert a.t1.tolist() == [0, 2] and (a.nb, a.pairs, a.entries) == (1, 2, 5) and a.cnt.tolist() == [3, 2]
    assert (a.t_i0.tolist(), a.t_i1.tolist(), a.t_nn.tolist(), a.t_j0.tolist()) == ([0, 1], [1, 2], [3, 2], [0, 3])
    assert a.carry_tiles == [[], [0]] and (a.ncs, a.listed) == (1, 0) and a.groups == [(0, 1, 0), (1, 1, 0)] and a.pad_groups == 0
    assert a.tile_segments(0).tolist() == [3, 0] and a.tile_segments(1).tolist() == [2, 0]
    assert a.exact_rows()[0].tolist() == [0, 2]              # row 2's pair begins where tile 1 begins
    # 2. two blocks (8 and 4 columns): row 0 = 5 entries in block 0, 1 in block 1; row 1 = 2 entries in block 1.
    #    block 0: e e e e | e END END -> tiles (0, 0, 4) [no row end: nr == 0] and (0, 2, 1); block 1: e END e e | END -> (2, 3, 3), (3, 4, 0)
    b = _layout([[0, 1, 2, 3, 4, 9], [8, 10]], 12, block=8, items=4)
    assert b.cnt.tolist() == [5, 0, 1, 2] and b.prp.tolist() == [0, 5, 5, 6, 8] and b.blk_tile0.tolist() == [0, 2, 4]
    assert (b.t_i0.tolist(), b.t_i1.tolist(), b.t_nn.tolist()) == ([0, 0, 2, 3], [0, 2, 3, 4], [4, 1, 3, 0])
    assert b.t_j0.tolist() == [0, 4, 5, 8] and b.t_blk.tolist() == [0, 0, 1, 1]
    # tile 0 -> row 0 (four entries of pair 0), tile 1 ends on pair 2 = (block 1, row 0): empty, tile 2 -> pair 3 = row 1
    assert b.carry_tiles == [[0, 1], [2]] and (b.ncs, b.listed) == (2, 0) and b.exact_rows()[0].tolist() == []
    assert b.tile_segments(2).tolist() == [1, 2] and b.tile_segments(3).tolist() == [0, 0]
    b1 = _layout([[0, 1, 2, 3, 4, 9], [8, 10]], 12, block=8, items=4, carry_rows=1)
    assert (b1.ncs, b1.listed, b1.row_listed.tolist()) == (1, 1, [1, 0])
    # 3. sixteen blocks of 4 columns, one row: 8 entries in block 0 (9 items: three tiles), 1 in block 9, every other block its row end only
    g = _layout([[0, 0, 1, 1, 2, 2, 3, 3, 36]], 64, block=4, items=4)
    assert (g.nb, g.n_tiles) == (16, 18) and g.t_nn.tolist() == [4, 4, 0] + [0] * 8 + [1] + [0] * 6
    pad = (0, 0, 0)
    assert g.groups == [(0, 1, 0)] + [(t, 1, t - 2) for t in range(3, 10)] + [(1, 1, 0)] + [(t, 1, t - 2) for t in range(11, 18)] \
        + [(2, 1, 0)] + [pad] * 7 + [(10, 1, 8)] + [pad] * 7
    assert g.pad_groups == 14 and g.stats()['t1_groups'] == 32
    # the row's carries: tiles 0 and 1 inside pair 0, then the last tile of every block but the last ends ON the next block's pair
    assert g.carry_tiles == [[0, 1, 2] + list(range(3, 17))] and (g.ncs, g.listed) == (4, 13)
    assert _layout([[0, 0, 1, 1, 2, 2, 3, 3, 36]], 60, block=4, items=4).pad_groups == 0          # 15 blocks: the plain order
    # an unsorted cut row drops the split; a sorted one next to light rows does not
    assert _layout([[0, 2, 1], [4, 5]], 8, block=8, items=4).stats()['cut_rows'] == 0
    assert _layout([[0, 2, 1], [4, 5]], 8, block=8, items=4).fallback and not a.fallback


def test_slot_of_rank_is_a_permutation():
    for nn in range(1, T.ITEMS + 1):
        slots = [T.slot_of_rank(r, nn) for r in range(nn)]
        assert sorted(slots) == list(range(nn)), nn
    # whole chunks: the even slots hold ranks 0..63, the odd ones 64..127; the partial last chunk is in plain order
    s = [T.slot_of_rank(r, 300) for r in range(300)]
    assert s[:3] == [0, 2, 4] and s[64:67] == [1, 3, 5] and s[128 + 63] == 128 + 126 and s[256:] == list(range(256, 300))


def test_pair_sum_orders():
    rng = np.random.default_rng(3)
    p = rng.uniform(-1, 1, size=63)
    assert T.pair_sum(p) == np.cumsum(p)[-1] and T.pair_sum([]) == 0.0 and T.pair_sum([-0.0]).view(np.int64) == 0
    q = rng.uniform(-1, 1, size=140)
    lanes = [sum(q[l::64].tolist(), 0.0) for l in range(64)]           # lane l: entries l, l + 64, ..
    for off in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[l] + lanes[l + off] for l in range(off)]
    assert T.pair_sum(q) == lanes[0] and abs(T.pair_sum(q) - np.cumsum(q)[-1]) < 1e-13
