"""
tests/lstream_cases.py without a GPU: the constants the module lays the stream out by are the library's
(csrk_spmv_stream_limits: the library loads without a device), every case sits on the edge it is named for on 256 compute
units and on 64, the model gives the layout worked out by hand on matrices of a dozen entries, the module's sequential
product agrees with the oracle's mult_vec bit for bit on every case, the order-of-addition cases check every row length at
every lane offset and leave out only the rows the kernel's in-order hand-over does not reach, and the union of the modelled censuses covers every form the default build can reach.
tests/test_gpu_lstream_forms.py runs the library on the same cases.
"""
import numpy as np
import pytest

import lstream_cases as S

ALL = S.names()
CUS = (256, 64)


def test_names_are_unique_and_seeded_by_name():
    assert len(set(ALL)) == len(ALL) and len(ALL) >= 40
    a = S.build('gaps')
    assert S.build('gaps') is a and all(S.CASES[n][0] for n in ALL)
    assert not np.array_equal(S.build('unsorted-dense').m.values[:8], S.build('tile-boundary').m.values[:8])
    assert not a.m.colinds.flags.writeable and not a.x.flags.writeable            # shared between the tests: read-only


def test_constants_are_the_librarys():
    from csr_amd.kernels import hip as K
    assert K.SPMV_STREAM_LIMITS == tuple(S.LIMITS)
    assert K.spmv_stream_limits() == S.LIMITS
    assert len(K.SPMV_PLAN_STATS) == 48 and set(S.build('gaps').layout('staged', 256).census()) <= set(K.SPMV_PLAN_STATS)
    # what the module derives from them
    assert S.EXACT_LEN == 25 and S.RID_SLOTS == 256 and S.TILE == S.WAVE * S.K8
    assert S.NW * S.TILE <= S.LIMITS['LS_RND_CAP'] and S.LIMITS['HOT_SLOTS'] < S.IDX24_MAX


@pytest.mark.parametrize('cus', CUS)
@pytest.mark.parametrize('name', ALL)
def test_preconditions(name, cus):
    c = S.build(name, cus)
    assert not S.failed_preconditions(c, cus), S.failed_preconditions(c, cus)
    assert c.name == name and c.m.nnz == int(c.m.rowptrs[-1]) and c.x.shape == (c.m.ncols,)
    assert all(set(S.env_of(c, f)) == set(S.ENV_KEYS) for f in S.FORMS)
    assert c.m.nnz <= 40000 or name == 'rounds'


def test_model_by_hand():
    "the layout restated once more on matrices small enough to do by hand"
    rng = np.random.default_rng(0)
    # rows 0, 2, 5 are light, row 3 (130 ascending entries) is cut under the forced split, rows 1 and 4 are empty
    cols = np.concatenate([[1, 2, 3], [2, 5], np.arange(130), [2]])
    m = S.assemble([3, 0, 2, 130, 0, 1], 200, rng, cols=cols, sort=False)
    a = S.Layout(m, True, 'staged', 4)
    assert a.cut.tolist() == [3] and a.n_view == 6 and a.n_pad == 3 and not a.dense            # 3 * 8 > 6: row ids
    assert a.first.tolist() == [0, 3, 3, 5, 5, 5] and (a.n_tiles, a.n_runs) == (1, 3) and a.starts_per_tile.tolist() == [3]
    assert a.run_rows.tolist() == [0, 2, 5] and a.gaps()[0] == 0 and a.gaps()[1].tolist() == [1, 2] and a.gaps()[2] == 0
    assert a.hot_cols.tolist() == [2] and a.n_hot_lds == 1                                    # column 2: three references
    assert a.staged and a.n_cold == 3 and a.tile_cold.tolist() == [3] and a.idx24             # columns 1, 3, 5 once each
    assert (a.W, a.nblk) == (32, 7) and a.blk_pairs.tolist() == [4, 0, 0, 0, 0, 0, 0]         # 200 columns over 8 workgroups: 25 -> 32
    assert a.grid == 1 and a.rt0.tolist() == [0, 1] and a.wr0.tolist() == [0, 1] and a.stage_tiles == 128
    assert a.census() == dict(stream=1, cut_rows=1, ls_tiles=1, ls_runs=3, ls_grid=1, ls_dense=0, n_hot=1, ls_hot_lds=1, ls_staged=3,
                              ls_round_tiles=128, ls_rounds=1, ls_wg_rounds=1, ls_stage_blocks=7, ls_stage_width=32, ls_idx24=1, ls_f32=0)
    # rows 0 and 2 are stored by lane 0 (the next row starts there); the last run is continued by the tile's padding up to lane 63
    assert a.storing_lane().tolist() == [0, 0, 63] and a.exact_rows().tolist() == [0, 2] and a.split_rows().tolist() == []
    assert a.lanes(a.exact_rows()).tolist() == [1, 1]
    # the same rows without the split: the 130-entry row stays, and its entries past the first 128 are not counted for the pack
    b = S.Layout(m, False, 'pack', 4)
    assert len(b.cut) == 0 and b.n_view == 136 and b.n_pad == 2 and b.dense and b.n_ent == 138 and b.n_runs == 6
    assert b.first.tolist() == [0, 3, 4, 6, 136, 137] and b.hot_cols.tolist() == [2, 1, 3, 5]   # (2: four references; 1, 3, 5: two)
    assert b.tile_cold.tolist() == [126] and not b.staged and b.census()['ls_rounds'] == 1 and b.mode() == 'LS_PLAIN+pack'
    assert S.Layout(m, False, 'nopack', 4).n_hot == 0
    # unsorted long row: the split cuts nothing
    u = S.assemble([3, 130], 200, rng, cols=np.concatenate([[1, 2, 3], np.arange(130)[::-1]]), sort=False)
    assert len(S.cut_rows(u, True)) == 0
    # dense rule at 8 empty : 64 entries, rounds of two workgroups by hand, the copy pass's blocks
    d = S.Layout(S.assemble([3, 0, 2, 4], 50, rng), False, 'nopack', 4)
    assert d.dense and d.slot_lens.tolist() == [3, 1, 2, 4] and d.first.tolist() == [0, 3, 4, 6] and d.n_ent == 10 and d.n_runs == 4
    rt0, wr0 = S.make_rounds(53, 2, 16)
    assert rt0.tolist() == [0, 16, 26, 42, 53] and wr0.tolist() == [0, 2, 4]
    assert S.make_rounds(53, 2, 32)[0].tolist() == [0, 26, 53] and S.make_rounds(3, 8, 128)[1].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 3]
    assert S.stage_blocks(17, 256) == (16, 2) and S.stage_blocks(6000000, 256) == (5872, 1022) and S.stage_blocks(9984 * 512, 256) == (9984, 512)


def _variants(name):
    c = S.build(name)
    yield c.m, c.x
    if name in S.REPRESENTATIVE:
        yield c.m.retyped(vals='f4'), c.x
        yield c.m.retyped(vals='f4'), c.x.astype(np.float32)
        yield c.m.retyped(vals='none', ptr64=True), c.x
        yield c.m, c.x.astype(np.float32)


@pytest.mark.parametrize('name', ALL)
def test_sequential_product_is_the_oracles(name):
    "bit for bit, float32 products included: the GPU file's exact checks compare with this loop"
    from oracle import oracle as O
    for m, x in _variants(name):
        ref = O.mult_vec(m.nrows, m.ncols, m.rowptrs, m.colinds, m.values, x)
        y = S.seq_product(m, x)
        assert np.array_equal(y.view(np.int64), ref.view(np.int64))
        bound = S.abs_bound(m, x)
        assert np.all(np.abs(ref) <= bound) and not np.isnan(ref).any()


@pytest.mark.parametrize('name', S.ORDER_CASES)
def test_order_cases_leave_out_only_what_the_hand_over_does_not_reach(name):
    """
    The rows of at most 25 entries left out of the bit-for-bit check are those a tile boundary cuts (at most one per boundary),
    rows of 25 entries that start in a lane's last slot (their sum is stored by a fifth lane) and the matrix's last row, which
    the padding of the last tile continues up to lane 63.
    """
    c = S.build(name)
    a = c.layout('nopack', 256)
    short = np.flatnonzero((a.view_lens > 0) & (a.view_lens <= S.EXACT_LEN))
    left_out = np.setdiff1d(short, a.exact_rows())
    cut = np.intersect1d(left_out, a.split_rows())
    assert len(cut) <= a.n_tiles - 1
    rest = np.setdiff1d(left_out, cut)
    fifth = (a.view_lens[rest] == S.EXACT_LEN) & (a.first[rest] % S.K8 == S.K8 - 1) & (a.last_slot()[rest] % S.TILE != S.TILE - 1)
    assert np.all(fifth | (rest == a.run_rows[-1])), rest[~(fifth | (rest == a.run_rows[-1]))]
    assert len(rest) <= 6 and len(a.exact_rows()) >= 0.9 * len(short)
    assert all(np.array_equal(c.layout(f, 256).exact_rows(), a.exact_rows()) for f in S.FORMS)


def test_every_length_is_checked_at_every_lane_offset():
    a = S.build('order-short').layout('nopack', 256)
    cov = S.order_coverage(a)
    assert all((n, o) in cov for n in range(1, S.EXACT_LEN + 1) for o in range(S.K8))
    rows = a.exact_rows()
    assert set(a.lanes(rows).tolist()) == {1, 2, 3, 4} and int(a.lanes(rows)[a.view_lens[rows] == 25].max()) == 4
    # the one alignment of these lengths whose sum a fifth lane stores is checked where the row ends its tile (lane 63 stores it)
    r25 = rows[(a.view_lens[rows] == 25) & (a.first[rows] % S.K8 == 7)]
    assert len(r25) >= 1 and np.all(a.last_slot()[r25] % S.TILE == S.TILE - 1)


def test_union_of_censuses_covers_every_reachable_form():
    seen = set()
    for name in ALL:
        c = S.build(name)
        for f in S.FORMS:
            a = c.layout(f, 256)
            cs = a.census()
            seen.add((a.mode(), 'dense' if a.dense else 'row ids'))
            if 0 < cs['n_hot'] == cs['ls_hot_lds']:
                seen.add('pack within LDS, ' + f)
            if cs['n_hot'] > cs['ls_hot_lds']:
                seen.add('pack beyond LDS, ' + f)
            if cs['ls_wg_rounds'] >= 2:
                seen.add('several rounds per workgroup, ' + f)
            if len(a.cut):
                seen.add('carries through the epilogue')
            if len(a.cut) == 0 and len(a.split_rows()):
                seen.add('carries through the fix-up kernel')
            if a.starts_per_tile.max() >= S.RID_SLOTS:
                seen.add('second output loop')
            if a.staged and a.blk_pairs.max() > S.LIMITS['LS_STAGE_BATCH']:
                seen.add('second batch of the copy pass')
    want = {(mode, lay) for mode in ('LS_PLAIN', 'LS_PLAIN+pack', 'LS_RND24') for lay in ('dense', 'row ids')}
    want |= {'pack within LDS, pack', 'pack within LDS, staged', 'pack beyond LDS, pack', 'pack beyond LDS, staged',
             'several rounds per workgroup, nopack', 'several rounds per workgroup, pack', 'several rounds per workgroup, staged',
             'carries through the epilogue', 'carries through the fix-up kernel', 'second output loop', 'second batch of the copy pass'}
    assert want <= seen, sorted(map(str, want - seen))
    assert not any(mode == 'LS_RND' for mode, _ in (s for s in seen if isinstance(s, tuple)))      # 4-byte words with staging: unreachable
