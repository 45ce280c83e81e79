// Host check of csr_amd/csrc/spmv_layout.h, built by tests/test_spmv_layout_host.py with the system compiler and
// -fsanitize=address,undefined: every decision of the SpMV plan builder (spmv_plan.hip, "host side") at its edge, and the
// parsing of its knobs.  Several of these branches need rows of 2^16 entries, 256 compute units' worth of tiles or 2^31
// entries to trigger on the device; here the constants are parameters (a segment cap of 3, a histogram of 64 or 8 bins, 8
// compute units), so this is where they are checked.  Every expected value is worked out by hand from the rule's statement.
#include "spmv_layout.h"

#include <cstdio>

using namespace csrk;
using namespace csrk::spmvlayout;

static int failures = 0;
static int case_failures = 0;

#define EXPECT_EQ(expr, want)                                                                                          \
    do {                                                                                                               \
        const long long got_ = (long long)(expr), want_ = (long long)(want);                                          \
        if (got_ != want_) {                                                                                           \
            printf("FAIL %s:%d: %s = %lld, want %lld\n", __FILE__, __LINE__, #expr, got_, want_);                      \
            case_failures++;                                                                                           \
        }                                                                                                              \
    } while (0)

template <class T> static void expect_vec(const char *what, int line, const std::vector<T> &got, const std::vector<long long> &want)
{
    bool same = got.size() == want.size();
    for (size_t i = 0; same && i < got.size(); i++) same = (long long)got[i] == want[i];
    if (same) return;
    printf("FAIL line %d: %s = {", line, what);
    for (const T &v : got) printf(" %lld", (long long)v);
    printf(" }, want {");
    for (long long v : want) printf(" %lld", v);
    printf(" }\n");
    case_failures++;
}
#define EXPECT_VEC(vec, ...) expect_vec(#vec, __LINE__, vec, std::vector<long long> __VA_ARGS__)

static void done(const char *name)
{
    printf("%s %s\n", case_failures ? "FAIL" : "ok  ", name);
    failures += case_failures;
    case_failures = 0;
}

#define EXPECT_GROUP(g, t0_, nt_, blk_)                                                                                \
    do {                                                                                                               \
        EXPECT_EQ((g).t0, t0_);                                                                                        \
        EXPECT_EQ((g).nt, nt_);                                                                                        \
        EXPECT_EQ((g).blk, blk_);                                                                                      \
    } while (0)
#define EXPECT_SEG(sg, tile0_, ptile0_, ntiles_, blk_)                                                                 \
    do {                                                                                                               \
        EXPECT_EQ((sg).tile0, tile0_);                                                                                 \
        EXPECT_EQ((sg).ptile0, ptile0_);                                                                               \
        EXPECT_EQ((sg).ntiles, ntiles_);                                                                               \
        EXPECT_EQ((sg).blk, blk_);                                                                                     \
    } while (0)

static std::vector<PanelTile> tiles_with_i1(const std::vector<int32_t> &i1)
{
    std::vector<PanelTile> t(i1.size());
    for (size_t k = 0; k < i1.size(); k++) {
        t[k].j0 = 0;
        t[k].cslot = 12345;      // (must be overwritten)
        t[k].i0 = 0;
        t[k].i1 = i1[k];
        t[k].nn = 0;
        t[k].blk = 0;
    }
    return t;
}

static void knob_cases()
{
    const SpmvKnobDefaults d = {2048, 128, 2, 3, 15936};
    {
        const SpmvKnobs k = parse_spmv_knobs(SpmvKnobStrings(), d);
        EXPECT_EQ(k.heavy_split, -1);
        EXPECT_EQ(k.hot, -1);
        EXPECT_EQ(k.ls_stage, -1);
        EXPECT_EQ(k.stream, -1);
        EXPECT_EQ(k.fix56_off, 0);
        EXPECT_EQ(k.nib, -1);
        EXPECT_EQ(k.heavy_min, 2048);
        EXPECT_EQ(k.heavy_min_set, 0);
        EXPECT_EQ(k.tierb_min, 128);
        EXPECT_EQ(k.acc_groups, 2);
        EXPECT_EQ(k.acc_groups_set, 0);
        EXPECT_EQ(k.acc_group_rows, 15936);
        EXPECT_EQ(k.trace, 0);
        const SpmvKnobDefaults wide = {2048, 128, 5, 3, 15936};      // a default beyond the maximum is clamped like a value
        EXPECT_EQ(parse_spmv_knobs(SpmvKnobStrings(), wide).acc_groups, 3);
    }
    done("knobs: nothing set");

    auto with = [&](const char *SpmvKnobStrings::*field, const char *v) {
        SpmvKnobStrings e;
        e.*field = v;
        return parse_spmv_knobs(e, d);
    };
    // CSRK_HEAVY_MIN: below 64 reads as 64; being set at all -- even empty -- is remembered
    EXPECT_EQ(with(&SpmvKnobStrings::heavy_min, "10").heavy_min, 64);
    EXPECT_EQ(with(&SpmvKnobStrings::heavy_min, "64").heavy_min, 64);
    EXPECT_EQ(with(&SpmvKnobStrings::heavy_min, "65").heavy_min, 65);
    EXPECT_EQ(with(&SpmvKnobStrings::heavy_min, "4000").heavy_min, 4000);
    EXPECT_EQ(with(&SpmvKnobStrings::heavy_min, "4000").heavy_min_set, 1);
    EXPECT_EQ(with(&SpmvKnobStrings::heavy_min, "").heavy_min, 64);
    EXPECT_EQ(with(&SpmvKnobStrings::heavy_min, "").heavy_min_set, 1);
    EXPECT_EQ(with(&SpmvKnobStrings::heavy_min, "-7").heavy_min, 64);
    done("knobs: CSRK_HEAVY_MIN");

    // CSRK_TIERB_MIN: negative reads as 0 (and 0 is "no tier 1")
    EXPECT_EQ(with(&SpmvKnobStrings::tierb_min, "-5").tierb_min, 0);
    EXPECT_EQ(with(&SpmvKnobStrings::tierb_min, "0").tierb_min, 0);
    EXPECT_EQ(with(&SpmvKnobStrings::tierb_min, "").tierb_min, 0);
    EXPECT_EQ(with(&SpmvKnobStrings::tierb_min, "1").tierb_min, 1);
    EXPECT_EQ(with(&SpmvKnobStrings::tierb_min, "300").tierb_min, 300);
    done("knobs: CSRK_TIERB_MIN");

    // CSRK_ACC_GROUPS: 1 .. max_groups = 3; being set at all is remembered
    EXPECT_EQ(with(&SpmvKnobStrings::acc_groups, "0").acc_groups, 1);
    EXPECT_EQ(with(&SpmvKnobStrings::acc_groups, "-2").acc_groups, 1);
    EXPECT_EQ(with(&SpmvKnobStrings::acc_groups, "").acc_groups, 1);
    EXPECT_EQ(with(&SpmvKnobStrings::acc_groups, "").acc_groups_set, 1);
    EXPECT_EQ(with(&SpmvKnobStrings::acc_groups, "1").acc_groups, 1);
    EXPECT_EQ(with(&SpmvKnobStrings::acc_groups, "3").acc_groups, 3);
    EXPECT_EQ(with(&SpmvKnobStrings::acc_groups, "4").acc_groups, 3);
    EXPECT_EQ(with(&SpmvKnobStrings::acc_groups, "2").acc_groups_set, 1);
    done("knobs: CSRK_ACC_GROUPS");

    // CSRK_ACC_GROUP_ROWS: outside 1 .. acc_maxrows = 15936 reads as acc_maxrows
    EXPECT_EQ(with(&SpmvKnobStrings::acc_group_rows, "0").acc_group_rows, 15936);
    EXPECT_EQ(with(&SpmvKnobStrings::acc_group_rows, "-3").acc_group_rows, 15936);
    EXPECT_EQ(with(&SpmvKnobStrings::acc_group_rows, "1").acc_group_rows, 1);
    EXPECT_EQ(with(&SpmvKnobStrings::acc_group_rows, "40").acc_group_rows, 40);
    EXPECT_EQ(with(&SpmvKnobStrings::acc_group_rows, "15936").acc_group_rows, 15936);
    EXPECT_EQ(with(&SpmvKnobStrings::acc_group_rows, "15937").acc_group_rows, 15936);
    done("knobs: CSRK_ACC_GROUP_ROWS");

    // CSRK_SPMV_NIB: empty is unset; '0' first is 0; anything else is 1
    EXPECT_EQ(with(&SpmvKnobStrings::nib, "").nib, -1);
    EXPECT_EQ(with(&SpmvKnobStrings::nib, "0").nib, 0);
    EXPECT_EQ(with(&SpmvKnobStrings::nib, "01").nib, 0);
    EXPECT_EQ(with(&SpmvKnobStrings::nib, "1").nib, 1);
    EXPECT_EQ(with(&SpmvKnobStrings::nib, "yes").nib, 1);
    done("knobs: CSRK_SPMV_NIB");

    // the tri-state switches look at their first character only
    EXPECT_EQ(with(&SpmvKnobStrings::heavy_split, "0").heavy_split, 0);
    EXPECT_EQ(with(&SpmvKnobStrings::heavy_split, "1").heavy_split, 1);
    EXPECT_EQ(with(&SpmvKnobStrings::heavy_split, "2").heavy_split, -1);
    EXPECT_EQ(with(&SpmvKnobStrings::heavy_split, "").heavy_split, -1);
    EXPECT_EQ(with(&SpmvKnobStrings::heavy_split, "01").heavy_split, 0);
    EXPECT_EQ(with(&SpmvKnobStrings::heavy_split, "10").heavy_split, 1);
    EXPECT_EQ(with(&SpmvKnobStrings::hot, "0").hot, 0);
    EXPECT_EQ(with(&SpmvKnobStrings::hot, "1").hot, 1);
    EXPECT_EQ(with(&SpmvKnobStrings::hot, "on").hot, -1);
    EXPECT_EQ(with(&SpmvKnobStrings::ls_stage, "0").ls_stage, 0);
    EXPECT_EQ(with(&SpmvKnobStrings::ls_stage, "1").ls_stage, 1);
    EXPECT_EQ(with(&SpmvKnobStrings::stream, "0").stream, 0);
    EXPECT_EQ(with(&SpmvKnobStrings::stream, "1").stream, 1);
    EXPECT_EQ(with(&SpmvKnobStrings::stream, "1").hot, -1);      // (each switch from its own variable)
    EXPECT_EQ(with(&SpmvKnobStrings::fix56, "0").fix56_off, 1);
    EXPECT_EQ(with(&SpmvKnobStrings::fix56, "1").fix56_off, 0);
    EXPECT_EQ(with(&SpmvKnobStrings::fix56, "").fix56_off, 0);
    EXPECT_EQ(with(&SpmvKnobStrings::trace, "").trace, 1);
    EXPECT_EQ(with(&SpmvKnobStrings::trace, "0").trace, 1);
    done("knobs: switches");
}

int main()
{
    EXPECT_EQ(sizeof(PanelTile), 32);
    EXPECT_EQ(sizeof(PanelGroup), 16);
    EXPECT_EQ(sizeof(AccSeg), 24);
    done("structures");

    knob_cases();

    // ---- size rules ---------------------------------------------------------------------------------------------------
    EXPECT_EQ(x_fits_l2(524288), 1);      // 4 MiB of float64
    EXPECT_EQ(x_fits_l2(524289), 0);
    EXPECT_EQ(pack_worth_counting(1048575, 1000000), 0);      // 2^20 - 1 entries
    EXPECT_EQ(pack_worth_counting(1048576, 1000000), 1);
    EXPECT_EQ(pack_worth_counting(1048576, 524288), 0);
    EXPECT_EQ(pack_worth_counting(1048576, 524289), 1);
    EXPECT_EQ(pack_cover_pays(0.2), 1);
    EXPECT_EQ(pack_cover_pays(0.1999), 0);
    EXPECT_EQ(cold_stage_pays(10, 160), 1);      // one word in sixteen
    EXPECT_EQ(cold_stage_pays(9, 160), 0);
    EXPECT_EQ(clamp_i32(5), 5);
    EXPECT_EQ(clamp_i32(2147483647ll), 2147483647);
    EXPECT_EQ(clamp_i32(2147483648ll), 2147483647);
    EXPECT_EQ(clamp_i32(1ll << 40), 2147483647);
    done("size rules");

    // 4-column blocks, 10 pairs at most: 8 columns = 2 blocks, 9 columns = 3, no columns = 1
    EXPECT_EQ(tier1_pairs_fit(5, 8, 4, 10), 1);
    EXPECT_EQ(tier1_pairs_fit(6, 8, 4, 10), 0);
    EXPECT_EQ(tier1_pairs_fit(3, 9, 4, 10), 1);
    EXPECT_EQ(tier1_pairs_fit(4, 9, 4, 10), 0);
    EXPECT_EQ(tier1_pairs_fit(10, 0, 4, 10), 1);
    EXPECT_EQ(tier1_pairs_fit(11, 0, 4, 10), 0);
    EXPECT_EQ(tier1_pairs_fit(268435456ll, 262144, 262144), 1);      // the default cap: 256 Mi pairs, inclusive
    EXPECT_EQ(tier1_pairs_fit(268435457ll, 262144, 262144), 0);
    EXPECT_EQ(tier1_pairs_fit(134217728ll, 262145, 262144), 1);      // two blocks
    EXPECT_EQ(tier1_pairs_fit(134217729ll, 262145, 262144), 0);
    done("tier1_pairs_fit");

    // 2 tiles of 512 slots at 12 B, (10 rows + 2 tiles) * 8 B, 64 MiB to spare: 12288 + 96 + 67108864
    EXPECT_EQ(stream_copy_fits(2, 512, 10, 67121248u), 1);
    EXPECT_EQ(stream_copy_fits(2, 512, 10, 67121247u), 0);
    // 1024 words at 20 B, 10 buckets at 16 B, 64 MiB to spare: 20480 + 160 + 67108864
    EXPECT_EQ(stage_temps_fit(1024, 10, 67129504u), 1);
    EXPECT_EQ(stage_temps_fit(1024, 10, 67129503u), 0);
    done("free-memory predicates");

    EXPECT_EQ(dense_rows_pay(80, 10, false), 1);      // an eighth exactly
    EXPECT_EQ(dense_rows_pay(80, 11, false), 0);
    EXPECT_EQ(dense_rows_pay(80, 0, false), 1);
    EXPECT_EQ(dense_rows_pay(2147483640ll, 7, false), 1);      // 2^31 - 1 slots
    EXPECT_EQ(dense_rows_pay(2147483640ll, 8, false), 0);      // 2^31
    EXPECT_EQ(dense_rows_pay(2147483640ll, 8, true), 1);
    done("dense_rows_pay");

    // ---- tile_starts ---------------------------------------------------------------------------------------------------
    {
        const int64_t be[4] = {0, 0, 8, 17};      // blocks of 0, 8 and 9 entries, 8 items per tile
        EXPECT_VEC(tile_starts(be, 3, 8, 0), {0, 0, 1, 3});
        EXPECT_VEC(tile_starts(be, 3, 8, 3), {0, 1, 3, 5});      // tier 1: + 3 row ends per block: 3, 11, 12 items
        const int64_t be1[3] = {0, 5, 11};                        // 5 + 3 = 8 items: one tile; 6 + 3 = 9: two
        EXPECT_VEC(tile_starts(be1, 2, 8, 3), {0, 1, 3});
        EXPECT_VEC(tile_starts(be, 0, 8, 0), {0});
    }
    done("tile_starts");

    // ---- panel_groups --------------------------------------------------------------------------------------------------
    {
        int64_t pads = -1;
        std::vector<int64_t> t0(16);
        for (int b = 0; b <= 15; b++) t0[(size_t)b] = b;      // 15 blocks of one tile: fewer than 2 * 8, plain order
        std::vector<PanelGroup> g = panel_groups(t0.data(), 15, 1, true, 8, &pads);
        EXPECT_EQ(g.size(), 15);
        EXPECT_EQ(pads, 0);
        for (int b = 0; b < 15; b++) EXPECT_GROUP(g[(size_t)b], b, 1, b);
        done("panel_groups: 15 blocks, plain");

        // 16 blocks: block 0 has 3 tiles, the others 1; 2 tiles per workgroup.  Stream 0 = block 0's two groups (2 + 1
        // tiles) and block 8's; streams 1 .. 7 = blocks q and q + 8: the longest has 3 groups, the others get a pad each.
        t0.assign(17, 0);
        t0[1] = 3;
        for (int b = 2; b <= 16; b++) t0[(size_t)b] = b + 2;
        g = panel_groups(t0.data(), 16, 2, true, 8, &pads);
        EXPECT_EQ(g.size(), 24);
        EXPECT_EQ(pads, 7);
        EXPECT_GROUP(g[0], 0, 2, 0);
        for (int q = 1; q < 8; q++) EXPECT_GROUP(g[(size_t)q], q + 2, 1, q);
        EXPECT_GROUP(g[8], 2, 1, 0);      // the third tile of block 0: 2 does not divide 3
        for (int q = 1; q < 8; q++) EXPECT_GROUP(g[(size_t)(8 + q)], q + 10, 1, q + 8);
        EXPECT_GROUP(g[16], 10, 1, 8);
        for (int q = 1; q < 8; q++) EXPECT_GROUP(g[(size_t)(16 + q)], 0, 0, 0);
        done("panel_groups: 16 blocks, streams and pads");

        g = panel_groups(t0.data(), 16, 2, false, 8, &pads);
        EXPECT_EQ(g.size(), 17);
        EXPECT_EQ(pads, 0);
        EXPECT_GROUP(g[0], 0, 2, 0);
        EXPECT_GROUP(g[1], 2, 1, 0);
        for (int b = 1; b < 16; b++) EXPECT_GROUP(g[(size_t)(b + 1)], b + 2, 1, b);
        done("panel_groups: xcd_streams off");
    }

    // ---- panel_carries -------------------------------------------------------------------------------------------------
    {
        // 3 long rows, 4 blocks: 12 pairs; a tile's carry belongs to row i1 % 3.  Row 0 has no carry, row 1 four (tiles 0, 3,
        // 5, 7), row 2 five (tiles 1, 2, 4, 6, 8); tile 9 ends past the last pair.
        std::vector<PanelTile> t = tiles_with_i1({1, 2, 2, 4, 5, 7, 8, 10, 11, 12});
        PanelCarries pc = panel_carries(t, 3, 12, 4);
        EXPECT_EQ(pc.ncs, 4);
        EXPECT_EQ(pc.listed, 1);
        EXPECT_VEC(pc.crp, {0, 0, 0, 1});
        EXPECT_EQ(pc.cidx.size(), 2);
        EXPECT_EQ(pc.cidx[0], 8);      // row 2's fifth
        const long long want[10] = {13, 14, 17, 16, 20, 19, 23, 22, -1, -1};      // 12 + j * 3 + h
        for (int k = 0; k < 10; k++) EXPECT_EQ(t[(size_t)k].cslot, want[k]);
        done("panel_carries: 0, 4 and 5 carries");

        // one carry row: the others are listed, each row's in tile order
        t = tiles_with_i1({1, 2, 2, 4, 5, 7, 8, 10, 11, 12});
        pc = panel_carries(t, 3, 12, 1);
        EXPECT_EQ(pc.ncs, 1);
        EXPECT_EQ(pc.listed, 7);
        EXPECT_VEC(pc.crp, {0, 0, 3, 7});
        EXPECT_EQ(pc.cidx.size(), 8);
        pc.cidx.resize(7);
        EXPECT_VEC(pc.cidx, {3, 5, 7, 2, 4, 6, 8});
        const long long want1[10] = {13, 14, -1, -1, -1, -1, -1, -1, -1, -1};
        for (int k = 0; k < 10; k++) EXPECT_EQ(t[(size_t)k].cslot, want1[k]);
        done("panel_carries: listed in tile order");

        t = tiles_with_i1({1, 12});
        pc = panel_carries(t, 3, 12, 4);
        EXPECT_EQ(pc.ncs, 1);
        EXPECT_EQ(pc.listed, 0);
        EXPECT_VEC(pc.crp, {0, 0, 0, 0});
        EXPECT_EQ(pc.cidx.size(), 1);
        EXPECT_EQ(t[0].cslot, 13);
        EXPECT_EQ(t[1].cslot, -1);
        t = tiles_with_i1({12, 13});      // no tile ends inside a pair
        pc = panel_carries(t, 3, 12, 4);
        EXPECT_EQ(pc.ncs, 0);
        EXPECT_EQ(pc.listed, 0);
        EXPECT_EQ(t[0].cslot, -1);
        EXPECT_EQ(t[1].cslot, -1);
        done("panel_carries: nothing listed");
    }

    // ---- tier 0: one group ---------------------------------------------------------------------------------------------
    {
        const int64_t lens[3] = {0, 4, 5};      // pieces of 4: none, exactly one, one + 1
        std::vector<int32_t> trow, tpiece;
        acc_tasks(lens, 3, 4, trow, tpiece);
        EXPECT_VEC(trow, {1, 2, 2});
        EXPECT_VEC(tpiece, {0, 0, 1});
        done("acc_tasks");
    }
    {
        WgShares sh = wg_shares(0, 0, 8);
        EXPECT_EQ(sh.n_wg, 1);
        EXPECT_VEC(sh.wg_t0, {0, 0});
        EXPECT_EQ(sh.share_max, 0);
        EXPECT_EQ(sh.n_phys, 0);
        sh = wg_shares(3, 0, 8);      // fewer tiles than CUs
        EXPECT_EQ(sh.n_wg, 3);
        EXPECT_VEC(sh.wg_t0, {0, 1, 2, 3});
        EXPECT_EQ(sh.share_max, 1);
        EXPECT_EQ(sh.n_phys, 3);
        sh = wg_shares(10, 0, 4);      // 10 * w / 4: shares of 2, 3, 2, 3
        EXPECT_EQ(sh.n_wg, 4);
        EXPECT_VEC(sh.wg_t0, {0, 2, 5, 7, 10});
        EXPECT_EQ(sh.share_max, 3);
        EXPECT_EQ(sh.n_phys, 12);
        sh = wg_shares(10, 3, 8);      // the launch's split says 3 workgroups
        EXPECT_EQ(sh.n_wg, 3);
        EXPECT_VEC(sh.wg_t0, {0, 3, 6, 10});
        EXPECT_EQ(sh.share_max, 4);
        EXPECT_EQ(sh.n_phys, 12);
        done("wg_shares");
    }
    {
        // blocks of 4, 0 and 6 tiles; two workgroups of 5 tiles; 3 tiles per segment at most
        const int64_t t0[4] = {0, 4, 4, 10};
        std::vector<AccSeg> segs;
        std::vector<int32_t> wg_seg;
        acc_segments({0, 5, 10}, t0, 3, segs, wg_seg);
        EXPECT_EQ(segs.size(), 5);
        EXPECT_VEC(wg_seg, {0, 3, 5});
        if (segs.size() == 5) {
            EXPECT_SEG(segs[0], 0, 0, 3, 0);      // block 0's four tiles: cut at the cap
            EXPECT_SEG(segs[1], 3, 6, 1, 0);      // ptile0 = (3 - 0) * 2 + 0
            EXPECT_SEG(segs[2], 4, 8, 1, 2);      // over the empty block 1 into block 2
            EXPECT_SEG(segs[3], 5, 1, 3, 2);      // workgroup 1: (5 - 5) * 2 + 1
            EXPECT_SEG(segs[4], 8, 7, 2, 2);      // (8 - 5) * 2 + 1
        }
        acc_segments({0, 0}, t0, 3, segs, wg_seg);      // a group without tiles: one workgroup, no segment
        EXPECT_EQ(segs.size(), 0);
        EXPECT_VEC(wg_seg, {0, 0});
        done("acc_segments");
    }
    EXPECT_EQ(acc_lds_bytes(4096, 5, 256), 32784 + 48 + 3072);      // window + zero slot + 1, six accumulators, 256 head slots
    EXPECT_EQ(acc_lds_bytes(4096, 6, 256), 32784 + 48 + 3072);
    EXPECT_EQ(acc_lds_bytes(4096, 7, 256), 32784 + 64 + 3072);
    EXPECT_EQ(acc_lds_bytes(4096, 15936, 256), 32784 + 127488 + 3072);      // 163344 <= 160 KiB = 163840
    done("acc_lds_bytes");

    // ---- tier0_threshold (histogram of 64 bins unless said) ------------------------------------------------------------
    {
        const int64_t a[3] = {100, 90, 80};
        EXPECT_EQ(tier0_threshold(a, 3, 3, 50, 10, 64), 50);       // the tier is full at the default
        EXPECT_EQ(tier0_threshold(a, 3, 2, 50, 10, 64), 50);
        EXPECT_EQ(tier0_threshold(a, 3, 10, 50, 10, 64), 50);      // every cut row reaches the default: nothing to add
        done("tier0_threshold: no extension");
        const int64_t b[5] = {100, 60, 40, 30, 20};      // capacity 3: the third longest
        EXPECT_EQ(tier0_threshold(b, 5, 3, 50, 10, 64), 40);
        EXPECT_EQ(tier0_threshold(b, 5, 4, 50, 10, 64), 30);
        done("tier0_threshold: kth in the histogram");
        const int64_t c[5] = {200, 150, 100, 90, 20};    // four rows in the shared top bin: the histogram cannot say
        EXPECT_EQ(tier0_threshold(c, 5, 3, 180, 10, 64), 100);
        const int64_t c16[4] = {200000, 100000, 70000, 10};      // ... and with the real bound of 2^16
        EXPECT_EQ(tier0_threshold(c16, 4, 3, 150000, 128), 70000);
        EXPECT_EQ(tier0_threshold(c16, 4, 4, 150000, 128), 128);      // (the fourth is in the histogram; the floor)
        done("tier0_threshold: kth beyond the histogram");
        const int64_t e[5] = {100, 40, 40, 40, 20};      // three rows tied at the third place, capacity 3: 4 rows >= 40
        EXPECT_EQ(tier0_threshold(e, 5, 3, 50, 10, 64), 41);
        EXPECT_EQ(tier0_threshold(e, 5, 4, 50, 10, 64), 40);      // capacity 4 holds the ties
        done("tier0_threshold: ties");
        const int64_t f[4] = {100, 5, 4, 3};
        EXPECT_EQ(tier0_threshold(f, 4, 3, 50, 10, 64), 10);
        done("tier0_threshold: floor");
        const int64_t g[3] = {100, 30, 20};      // fewer cut rows than the capacity: down to the shortest
        EXPECT_EQ(tier0_threshold(g, 3, 10, 50, 10, 64), 20);
        done("tier0_threshold: n_cut below the capacity");
        const int64_t h[2] = {100, 5};           // a floor above the default
        EXPECT_EQ(tier0_threshold(h, 2, 10, 50, 60, 64), 50);
        const int64_t i[3] = {100, 49, 49};      // the tie rule lands on the default
        EXPECT_EQ(tier0_threshold(i, 3, 2, 50, 10, 64), 50);
        done("tier0_threshold: never raised");
    }
    {
        const int32_t rows[4] = {3, 7, 9, 12};
        const int64_t lens[4] = {100, 40, 41, 10};
        std::vector<int32_t> r0, r1;
        std::vector<int64_t> len0;
        int64_t nnz1 = -1;
        split_rows(rows, lens, 4, 41, r0, len0, r1, &nnz1);
        EXPECT_VEC(r0, {3, 9});
        EXPECT_VEC(len0, {100, 41});
        EXPECT_VEC(r1, {7, 12});
        EXPECT_EQ(nnz1, 50);
        done("split_rows");
    }

    // ---- hot_threshold_from_hist: 8 bins + the shared top bin, 5 slots ---------------------------------------------------
    {
        unsigned long long hn[9] = {100, 50, 1, 1, 0, 1, 0, 0, 6}, hs[9] = {0, 50, 2, 3, 0, 5, 0, 0, 60};
        HotThreshold h = hot_threshold_from_hist(hn, hs, 8, 5);
        EXPECT_EQ(h.decided, 0);
        done("hot threshold: top bin above the cap");
        hn[8] = 1;
        hs[8] = 20;
        h = hot_threshold_from_hist(hn, hs, 8, 5);      // columns of count 0 and 1 are never packed
        EXPECT_EQ(h.decided, 1);
        EXPECT_EQ(h.thr, 2);
        EXPECT_EQ(h.cols, 4);
        EXPECT_EQ(h.refs, 30);
        done("hot threshold: everything fits");
        const unsigned long long hn2[9] = {9, 9, 9, 9, 1, 2, 1, 1, 2}, hs2[9] = {0, 9, 18, 27, 4, 10, 6, 7, 30};
        h = hot_threshold_from_hist(hn2, hs2, 8, 5);      // 2 + 1 + 1 = 4 columns; bin 5 would make 6 (bin 4's one is not reached)
        EXPECT_EQ(h.decided, 1);
        EXPECT_EQ(h.thr, 6);
        EXPECT_EQ(h.cols, 4);
        EXPECT_EQ(h.refs, 43);
        const unsigned long long hn3[9] = {0, 0, 0, 0, 0, 0, 0, 1, 5}, hs3[9] = {0, 0, 0, 0, 0, 0, 0, 7, 99};
        h = hot_threshold_from_hist(hn3, hs3, 8, 5);      // the top bin fills the slots exactly
        EXPECT_EQ(h.decided, 1);
        EXPECT_EQ(h.thr, 8);
        EXPECT_EQ(h.cols, 5);
        EXPECT_EQ(h.refs, 99);
        const unsigned long long hn4[9] = {0, 0, 2, 1, 0, 0, 0, 1, 1}, hs4[9] = {0, 0, 4, 3, 0, 0, 0, 7, 9};
        h = hot_threshold_from_hist(hn4, hs4, 8, 5);      // bin 2 reaches the slots exactly: taken
        EXPECT_EQ(h.thr, 2);
        EXPECT_EQ(h.cols, 5);
        EXPECT_EQ(h.refs, 23);
        done("hot threshold: stops at the bin that would overflow");
    }

    // ---- cold staging ------------------------------------------------------------------------------------------------------
    {
        // 8 CUs: 16 workgroups fill the chip once; windows of 32 columns at most.  20 tiles in rounds of 8 at least, a grid
        // of 4: (3 + 4 + 2) buckets per block at most.
        StageBlocks sb = stage_blocks(512, 8, 32, 20, 8, 4);      // one chip-fill of full windows
        EXPECT_EQ(sb.W, 32);
        EXPECT_EQ(sb.nblk, 16);
        EXPECT_EQ(sb.nb_max, 9 * 16);
        sb = stage_blocks(513, 8, 32, 20, 8, 4);      // one column more: two chip-fills' worth of blocks, ceil(513 / 32) = 17 wide
        EXPECT_EQ(sb.W, 32);
        EXPECT_EQ(sb.nblk, 17);
        EXPECT_EQ(sb.nb_max, 9 * 17);
        sb = stage_blocks(100, 8, 32, 20, 8, 4);      // ceil(100 / 16) = 7 columns, widened to 16
        EXPECT_EQ(sb.W, 16);
        EXPECT_EQ(sb.nblk, 7);
        sb = stage_blocks(1, 8, 32, 20, 8, 4);
        EXPECT_EQ(sb.W, 16);
        EXPECT_EQ(sb.nblk, 1);
        sb = stage_blocks(5111808, 256, 9984, 16, 8, 1);      // the real constants: 512 windows of 9984
        EXPECT_EQ(sb.W, 9984);
        EXPECT_EQ(sb.nblk, 512);
        EXPECT_EQ(sb.nb_max, (2 + 1 + 2) * 512);
        sb = stage_blocks(5111809, 256, 9984, 16, 8, 1);      // 1024 blocks wanted: ceil(5111809 / 1024) = 4993 -> 5008 wide
        EXPECT_EQ(sb.W, 5008);
        EXPECT_EQ(sb.nblk, 1021);
        for (int64_t nc : {1, 15, 16, 17, 511, 512, 513, 1023, 1024, 1025, 4000}) {
            sb = stage_blocks(nc, 8, 32, 20, 8, 4);
            EXPECT_EQ(sb.W % 16, 0);
            EXPECT_EQ(sb.W <= 32, 1);
            EXPECT_EQ(sb.W * sb.nblk >= nc, 1);
            EXPECT_EQ(sb.W * (sb.nblk - 1) < nc, 1);
        }
        done("stage_blocks");
    }
    {
        std::vector<int32_t> rt0, wr0;
        EXPECT_EQ(stage_rounds(16, 1, 16, 8, rt0, wr0), 1);      // a share of exactly nt
        EXPECT_VEC(rt0, {0, 16});
        EXPECT_VEC(wr0, {0, 1});
        EXPECT_EQ(stage_rounds(17, 1, 16, 8, rt0, wr0), 2);      // nt + 1: two rounds of ceil(9 / 8) * 8 = 16 at most
        EXPECT_VEC(rt0, {0, 16, 17});
        EXPECT_VEC(wr0, {0, 2});
        EXPECT_EQ(stage_rounds(5, 1, 16, 8, rt0, wr0), 1);       // fewer tiles than wavefronts
        EXPECT_VEC(rt0, {0, 5});
        EXPECT_VEC(wr0, {0, 1});
        EXPECT_EQ(stage_rounds(1, 2, 16, 8, rt0, wr0), 1);       // workgroup 0's share is empty
        EXPECT_VEC(rt0, {0, 1});
        EXPECT_VEC(wr0, {0, 0, 1});
        EXPECT_EQ(stage_rounds(40, 2, 16, 8, rt0, wr0), 4);      // shares of 20: two rounds each, 16 + 4
        EXPECT_VEC(rt0, {0, 16, 20, 36, 40});
        EXPECT_VEC(wr0, {0, 2, 4});
        EXPECT_EQ(stage_rounds(50, 1, 16, 8, rt0, wr0), 4);      // ceil(50 / 16) = 4 rounds of ceil(13 / 8) * 8 = 16, the last of 2
        EXPECT_VEC(rt0, {0, 16, 32, 48, 50});
        EXPECT_EQ(stage_rounds(33, 1, 16, 8, rt0, wr0), 3);      // 3 rounds of ceil(11 / 8) * 8 = 16, the last of 1
        EXPECT_VEC(rt0, {0, 16, 32, 33});
        EXPECT_EQ(stage_rounds(0, 2, 16, 8, rt0, wr0), 0);
        EXPECT_VEC(rt0, {0});
        EXPECT_VEC(wr0, {0, 0, 0});
        done("stage_rounds");
    }
    EXPECT_EQ(next_round_size(128, 8192, 16384, 8), 64);      // twice too full: half the size
    EXPECT_EQ(next_round_size(128, 8192, 32768, 8), 32);
    EXPECT_EQ(next_round_size(128, 8192, 10000, 8), 104);     // 104.86 -> 104
    EXPECT_EQ(next_round_size(128, 8192, 8200, 8), 120);      // 127.9 -> 120 = one step down
    EXPECT_EQ(next_round_size(128, 8192, 8193, 8), 120);
    EXPECT_EQ(next_round_size(24, 8192, 8700, 8), 16);        // 22.6 -> 16
    EXPECT_EQ(next_round_size(128, 8192, 8750, 8), 112);      // 119.8 -> 112: below one step down
    done("next_round_size");

    if (failures) {
        printf("%d check(s) failed\n", failures);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
