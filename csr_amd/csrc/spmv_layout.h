// The arithmetic that decides an SpMV plan's layout (spmv_plan.hip, "host side"; DESIGN.md section 4, "The plan builder"):
// tile starts, the tier-1 workgroup list and carry slots, tier 0's tasks, shares, segments and threshold, the pack's
// threshold, the staging blocks and rounds, the size rules -- and the knobs of one plan build (SpmvKnobs).  One pure
// function per decision, its constants passed in.  Plain host C++, no device code: spmv_plan.hip calls these when it builds
// a plan, and tests/spmv_layout_host runs them as a stand-alone program.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace csrk {

// ---- the small structures the plan kernels and the host both read (their layout is the kernels' ABI) ------------------
struct PanelTile {
    int64_t j0;      // first entry of the tile in M'
    int64_t cslot;   // where the tile's carry goes: an index into the partials' carry rows (Panel::ncs), or -1: carry_val[t]
    int32_t i0, i1;  // rows of M' completed before the tile start / end
    int32_t nn;      // entries in the tile
    int32_t blk;     // column block
};
static_assert(sizeof(PanelTile) == 32, "PanelTile is read by the tier-1 kernels");

struct PanelGroup {
    int64_t t0;      // first tile
    int32_t nt;      // tiles handled by this workgroup (all in one column block)
    int32_t blk;
};
static_assert(sizeof(PanelGroup) == 16, "PanelGroup is read by the tier-1 kernels");

// one segment of an accumulator-form workgroup's tile range (see "long rows, accumulator form")
struct AccSeg {
    int64_t tile0;    // first tile of the segment (logical: block-major order)
    int64_t ptile0;   // ... and where it is stored; the segment's tile t is stored at ptile0 + t * n_wg
    int32_t ntiles;   // <= ACC_SEG_TILES, all in one column block
    int32_t blk;
};
static_assert(sizeof(AccSeg) == 24, "AccSeg is read by the accumulator kernel");

// ---- knobs: every environment variable a plan build looks at, read ONCE per build -------------------------------------
// (The tests change them between two builds of one process, so they are not cached across builds.)
struct SpmvKnobStrings {      // getenv's answers, nullptr = unset
    const char *heavy_split = nullptr, *heavy_min = nullptr, *tierb_min = nullptr, *acc_groups = nullptr,
               *acc_group_rows = nullptr, *nib = nullptr, *fix56 = nullptr, *hot = nullptr, *ls_stage = nullptr,
               *stream = nullptr, *trace = nullptr;
};
struct SpmvKnobDefaults {
    int heavy_min, tierb_min, acc_groups, max_groups, acc_maxrows;
};
struct SpmvKnobs {
    // tri-state switches: 0 = off, 1 = forced, -1 = the builder decides.  Only the FIRST character is looked at: '0' is
    // off, '1' is forced, anything else (unset, empty, "2", "on") is -1.
    int heavy_split = -1, hot = -1, ls_stage = -1, stream = -1;
    bool fix56_off = false;        // CSRK_SPMV_FIX56 starts with '0': no packed value form
    int nib = -1;                  // CSRK_SPMV_NIB: unset or EMPTY = -1, first character '0' = 0, anything else = 1
    int heavy_min = 0;             // CSRK_HEAVY_MIN: atoi, below 64 reads as 64; unset = the default
    bool heavy_min_set = false;    // ... and merely being set (even empty) turns tier 0's extension off
    int tierb_min = 0;             // CSRK_TIERB_MIN: atoi, negative reads as 0 (0 = no tier 1); unset = the default
    int acc_groups = 1;            // CSRK_ACC_GROUPS: atoi clamped to 1 .. max_groups; unset = the default, clamped alike
    bool acc_groups_set = false;   // ... and merely being set turns accgroups::choose_groups off
    int32_t acc_group_rows = 0;    // CSRK_ACC_GROUP_ROWS: atoi; outside 1 .. acc_maxrows (or unset) reads as acc_maxrows
    bool trace = false;            // CSRK_PLAN_TRACE is set (any value)
};

inline int knob_tristate(const char *e) { return !e ? -1 : e[0] == '0' ? 0 : e[0] == '1' ? 1 : -1; }

inline SpmvKnobs parse_spmv_knobs(const SpmvKnobStrings &e, const SpmvKnobDefaults &d)
{
    SpmvKnobs k;
    k.heavy_split = knob_tristate(e.heavy_split);
    k.hot = knob_tristate(e.hot);
    k.ls_stage = knob_tristate(e.ls_stage);
    k.stream = knob_tristate(e.stream);
    k.fix56_off = e.fix56 && e.fix56[0] == '0';
    k.nib = !e.nib || !e.nib[0] ? -1 : e.nib[0] == '0' ? 0 : 1;
    k.heavy_min_set = e.heavy_min != nullptr;
    k.heavy_min = e.heavy_min ? (atoi(e.heavy_min) > 64 ? atoi(e.heavy_min) : 64) : d.heavy_min;
    k.tierb_min = e.tierb_min ? (atoi(e.tierb_min) >= 0 ? atoi(e.tierb_min) : 0) : d.tierb_min;
    k.acc_groups_set = e.acc_groups != nullptr;
    const int g = e.acc_groups ? atoi(e.acc_groups) : d.acc_groups;
    k.acc_groups = g < 1 ? 1 : g > d.max_groups ? d.max_groups : g;
    const int r = e.acc_group_rows ? atoi(e.acc_group_rows) : d.acc_maxrows;
    k.acc_group_rows = r < 1 || r > d.acc_maxrows ? d.acc_maxrows : r;
    k.trace = e.trace != nullptr;
    return k;
}

namespace spmvlayout {

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int32_t clamp_i32(int64_t v) { return (int32_t)(v > INT32_MAX ? INT32_MAX : v); }

// ---- size rules: whether a split or a pack is attempted at all ---------------------------------------------------------
// x that fits an XCD's 4 MiB L2 whole: every gather is an L2 hit already, neither the split nor the pack pays
inline bool x_fits_l2(int64_t ncols) { return ncols * 8 <= (4ll << 20); }
// the pack's census is taken only for 2^20 entries or more and an x beyond L2
inline bool pack_worth_counting(int64_t nnz, int64_t ncols) { return !(nnz < (1 << 20) || x_fits_l2(ncols)); }
// ... and the pack is kept only if the packed columns carry a fifth of the sampled entries
inline bool pack_cover_pays(double cover) { return !(cover < 0.2); }
// tier 1 is given up (the cut rows all go to tier 0's threshold alone) beyond `cap` (block, row) pairs
inline bool tier1_pairs_fit(int64_t n_rows1, int64_t ncols, int64_t cb, int64_t cap = 256ll << 20)
{
    return n_rows1 * cdiv(ncols > 0 ? ncols : 1, cb) <= cap;
}
// the light stream's copy (12 B per slot, 8 B per row and tile) must leave 64 MiB of device memory free
inline bool stream_copy_fits(int64_t n_tiles, int64_t tile, int64_t nrows, size_t mfree)
{
    return !((size_t)n_tiles * (size_t)tile * 12 + ((size_t)nrows + (size_t)n_tiles) * 8 + (64u << 20) > mfree);
}
// ... and so must the staging's temporaries (20 B per index word, 16 B per bucket)
inline bool stage_temps_fit(int64_t n_words, int64_t nb_max, size_t mfree)
{
    return !((size_t)n_words * 20 + (size_t)nb_max * 16 + (64u << 20) > mfree);
}
// dense rows (every empty row of the view gets one padding entry): not when the padding adds more than an eighth to the
// stream, nor past the range of 32-bit row pointers
inline bool dense_rows_pay(int64_t n_view, int64_t n_pad, bool p64)
{
    const bool fits = p64 || n_view + n_pad <= (int64_t)INT32_MAX;
    return fits && n_pad * 8 <= n_view;
}

// ---- both panels: tiles per column block ---------------------------------------------------------------------------------
// be[0..nb]: entries before each block's end -> t0[0..nb]: tiles before each block.  A block's items are its entries plus
// `extra` (tier 1: the n row ends of its merge path; tier 0: 0).
inline std::vector<int64_t> tile_starts(const int64_t *be, int32_t nb, int64_t items, int64_t extra)
{
    std::vector<int64_t> t0((size_t)nb + 1);
    t0[0] = 0;
    for (int32_t b = 0; b < nb; b++) t0[(size_t)b + 1] = t0[(size_t)b] + cdiv(extra + be[b + 1] - be[b], items);
    return t0;
}

// ---- tier 1: workgroup list ------------------------------------------------------------------------------------------------
// `tpw` consecutive tiles of one block per workgroup.  With xcd_streams and at least 2 * streams blocks, block b's groups
// go to stream b % streams and the streams are interleaved (group i of stream q is workgroup i * streams + q: blockIdx %
// streams labels the XCD), the shorter streams padded with groups of no tiles; *pad_groups counts those.
inline std::vector<PanelGroup> panel_groups(const int64_t *t0, int32_t nb, int tpw, bool xcd_streams, int streams,
                                            int64_t *pad_groups)
{
    std::vector<PanelGroup> groups;
    auto block_groups = [&](int32_t b, std::vector<PanelGroup> &out) {
        for (int64_t t = t0[b]; t < t0[b + 1]; t += tpw) {
            PanelGroup gq;
            gq.t0 = t;
            gq.nt = (int32_t)(t0[b + 1] - t < tpw ? t0[b + 1] - t : tpw);
            gq.blk = b;
            out.push_back(gq);
        }
    };
    *pad_groups = 0;
    if (!xcd_streams || nb < 2 * streams) {      // too few blocks to keep all XCDs busy per stream
        for (int32_t b = 0; b < nb; b++) block_groups(b, groups);
        return groups;
    }
    std::vector<std::vector<PanelGroup>> st((size_t)streams);
    size_t longest = 0;
    for (int32_t b = 0; b < nb; b++) block_groups(b, st[(size_t)(b % streams)]);
    for (const auto &q : st) longest = q.size() > longest ? q.size() : longest;
    PanelGroup pad;
    pad.t0 = 0;
    pad.nt = 0;
    pad.blk = 0;
    groups.reserve(longest * (size_t)streams);
    for (size_t i = 0; i < longest; i++)
        for (const auto &q : st) {
            groups.push_back(i < q.size() ? q[i] : pad);
            *pad_groups += i >= q.size();
        }
    return groups;
}

// ---- tier 1: carry slots ---------------------------------------------------------------------------------------------------
// A tile's carry belongs to the pair its last, unfinished row end falls in (i1; i1 >= pairs: none), so to long row i1 % n.
// The first `ncs` carries of a row (ncs = the most any row has, at most carry_rows) get a slot in the carry rows behind the
// block partials, cslot = pairs + j * n + h; the others are listed: cidx[crp[h] .. crp[h + 1]) = their tiles, ascending.
struct PanelCarries {
    int32_t ncs = 0;
    std::vector<int32_t> crp, cidx;      // int32[n + 1] (all zero when nothing is listed), int32[listed + 1]
    int64_t listed = 0;
};
inline PanelCarries panel_carries(std::vector<PanelTile> &tiles, int32_t n, int64_t pairs, int32_t carry_rows)
{
    PanelCarries pc;
    std::vector<int32_t> cnt((size_t)n, 0);
    for (const PanelTile &T : tiles)
        if ((int64_t)T.i1 < pairs) {
            const int32_t c = ++cnt[(size_t)(T.i1 % n)];
            pc.ncs = c > pc.ncs ? c : pc.ncs;
        }
    pc.ncs = pc.ncs < carry_rows ? pc.ncs : carry_rows;
    pc.crp.assign((size_t)n + 1, 0);
    for (int32_t h = 0; h < n; h++)
        pc.crp[(size_t)h + 1] = pc.crp[(size_t)h] + (cnt[(size_t)h] > pc.ncs ? cnt[(size_t)h] - pc.ncs : 0);
    pc.listed = pc.crp[(size_t)n];
    pc.cidx.resize((size_t)pc.listed + 1);
    std::vector<int32_t> seen((size_t)n, 0);
    for (size_t t = 0; t < tiles.size(); t++) {      // ascending tiles: each row's carries come out in tile order
        PanelTile &T = tiles[t];
        T.cslot = -1;
        if ((int64_t)T.i1 >= pairs) continue;
        const int32_t h = (int32_t)(T.i1 % n), j = seen[(size_t)h]++;
        if (j < pc.ncs) T.cslot = pairs + (int64_t)j * n + h;
        else pc.cidx[(size_t)(pc.crp[(size_t)h] + j - pc.ncs)] = (int32_t)t;
    }
    return pc;
}

// ---- tier 0: one group --------------------------------------------------------------------------------------------------------
// tasks of the pair-start pass: row c in pieces of `piece` entries (a row without entries has no task)
inline void acc_tasks(const int64_t *lens, int32_t n, int64_t piece, std::vector<int32_t> &trow, std::vector<int32_t> &tpiece)
{
    trow.clear();
    tpiece.clear();
    for (int32_t c = 0; c < n; c++)
        for (int64_t pc = 0; pc * piece < lens[c]; pc++) {
            trow.push_back(c);
            tpiece.push_back((int32_t)pc);
        }
}

// persistent workgroups: wg_want of them (0: one per CU), at most one per tile and one at least, equal shares of the tiles;
// stored interleaved, so n_phys = the longest share times n_wg tiles are stored (the last sweep has holes)
struct WgShares {
    int64_t n_wg = 1, share_max = 0, n_phys = 0;
    std::vector<int64_t> wg_t0;      // int64[n_wg + 1]
};
inline WgShares wg_shares(int64_t n_tiles, int32_t wg_want, int32_t cus)
{
    WgShares sh;
    sh.n_wg = wg_want > 0 ? wg_want : cus;
    if (sh.n_wg > n_tiles) sh.n_wg = n_tiles;
    if (sh.n_wg < 1) sh.n_wg = 1;
    sh.wg_t0.resize((size_t)sh.n_wg + 1);
    for (int64_t w = 0; w <= sh.n_wg; w++) sh.wg_t0[(size_t)w] = n_tiles * w / sh.n_wg;
    for (int64_t w = 0; w < sh.n_wg; w++) sh.share_max = std::max(sh.share_max, sh.wg_t0[(size_t)w + 1] - sh.wg_t0[(size_t)w]);
    sh.n_phys = sh.share_max * sh.n_wg;
    return sh;
}

// a workgroup's share cut into segments: tiles of ONE column block (t0: tiles before each block), seg_cap at most;
// wg_seg[w] .. wg_seg[w + 1] are workgroup w's
inline void acc_segments(const std::vector<int64_t> &wg_t0, const int64_t *t0, int64_t seg_cap, std::vector<AccSeg> &segs,
                         std::vector<int32_t> &wg_seg)
{
    const int64_t n_wg = (int64_t)wg_t0.size() - 1;
    segs.clear();
    wg_seg.assign((size_t)n_wg + 1, 0);
    int32_t b = 0;
    for (int64_t w = 0; w < n_wg; w++) {
        wg_seg[(size_t)w] = (int32_t)segs.size();
        int64_t t = wg_t0[(size_t)w];
        const int64_t t_end = wg_t0[(size_t)w + 1];
        while (t < t_end) {
            while (t0[b + 1] <= t) b++;
            int64_t e = t_end < t0[b + 1] ? t_end : t0[b + 1];
            if (e - t > seg_cap) e = t + seg_cap;
            AccSeg sg;
            sg.tile0 = t;
            sg.ptile0 = (t - wg_t0[(size_t)w]) * n_wg + w;
            sg.ntiles = (int32_t)(e - t);
            sg.blk = b;
            segs.push_back(sg);
            t = e;
        }
    }
    wg_seg[(size_t)n_wg] = (int32_t)segs.size();
}

// LDS of the accumulator kernel: the x window and its zero slot (+ 1 to keep 16 B), the group's accumulators (an even
// number), 12 B per head slot
inline size_t acc_lds_bytes(int cb, int32_t n, int seg_tiles)
{
    return (size_t)(cb + 2) * 8 + (size_t)((n + 1) & ~1) * 8 + (size_t)seg_tiles * 12;
}

// ---- the split: tier 0's threshold -------------------------------------------------------------------------------------------
// Tier 0 holds the cut rows of at least heavy_min entries.  When those are fewer than its capacity t0_cap and shorter cut
// rows exist, the tier is extended downwards to its t0_cap longest rows: the threshold becomes the kth longest row's
// length, k = min(n_cut, t0_cap) -- plus one when the rows tied with the kth would overflow the capacity, never below
// `floor`, and never above heavy_min (the threshold is only ever lowered).  A histogram of the lengths below hist_bound
// finds the kth (nth_element over 10^5 rows was 0.4 ms of the plan) unless the kth row is longer than that.
inline int tier0_threshold(const int64_t *lens, int32_t n_cut, int64_t t0_cap, int heavy_min, int floor,
                           int64_t hist_bound = 1 << 16)
{
    int64_t n_min = 0;
    for (int32_t c = 0; c < n_cut; c++) n_min += lens[c] >= heavy_min;
    if (!(n_min < t0_cap && n_cut > n_min)) return heavy_min;
    const size_t kth = (size_t)(n_cut < t0_cap ? n_cut : t0_cap) - 1;
    int64_t thr = -1;
    {
        const int64_t HB = hist_bound;
        std::vector<int32_t> hist((size_t)HB + 1, 0);
        for (int32_t c = 0; c < n_cut; c++) hist[(size_t)(lens[c] < HB ? lens[c] : HB)]++;
        int64_t seen = hist[(size_t)HB];
        if (seen <= (int64_t)kth)
            for (int64_t v = HB - 1; v >= 0; v--) {
                seen += hist[(size_t)v];
                if (seen > (int64_t)kth) {
                    thr = v;
                    break;
                }
            }
    }
    if (thr < 0) {
        std::vector<int64_t> sl(lens, lens + n_cut);
        std::nth_element(sl.begin(), sl.begin() + (int64_t)kth, sl.end(), [](int64_t a, int64_t b) { return a > b; });
        thr = sl[kth];
    }
    // rows tied with the kth must not push the tier over its capacity
    int64_t n_ge = 0;
    for (int32_t c = 0; c < n_cut; c++) n_ge += lens[c] >= thr;
    if (n_ge > t0_cap) thr++;
    thr = thr < floor ? floor : thr;
    return thr < heavy_min ? (int)thr : heavy_min;
}

// tier 0: the cut rows of at least `thr` entries (with their lengths); tier 1: the others (with their entries in all)
inline void split_rows(const int32_t *rows, const int64_t *lens, int32_t n_cut, int64_t thr, std::vector<int32_t> &r0,
                       std::vector<int64_t> &len0, std::vector<int32_t> &r1, int64_t *nnz1)
{
    r0.clear();
    len0.clear();
    r1.clear();
    *nnz1 = 0;
    r0.reserve((size_t)n_cut);
    r1.reserve((size_t)n_cut);
    len0.reserve((size_t)n_cut);
    for (int32_t c = 0; c < n_cut; c++) {
        if (lens[c] >= thr) {
            r0.push_back(rows[c]);
            len0.push_back(lens[c]);
        } else {
            r1.push_back(rows[c]);
            *nnz1 += lens[c];
        }
    }
}

// ---- the pack: threshold from the census histogram --------------------------------------------------------------------------
// hn[v] / hs[v] = columns with count v / the sum of their counts, v < hist; bin `hist` holds every count at or above it.
// The smallest threshold >= 2 that leaves at most `slots` columns, with those columns and their references -- undecided
// when the shared top bin alone holds more than `slots` (the builder then searches by census launches).
struct HotThreshold {
    bool decided = false;
    int64_t thr = 0;
    unsigned long long cols = 0, refs = 0;
};
inline HotThreshold hot_threshold_from_hist(const unsigned long long *hn, const unsigned long long *hs, int64_t hist,
                                            int64_t slots)
{
    HotThreshold h;
    if (hn[hist] > (unsigned long long)slots) return h;
    h.decided = true;
    h.thr = hist;
    h.cols = hn[hist];
    h.refs = hs[hist];
    for (int64_t v = hist - 1; v >= 2; v--) {
        if (h.cols + hn[v] > (unsigned long long)slots) break;
        h.cols += hn[v];
        h.refs += hs[v];
        h.thr = v;
    }
    return h;
}

// ---- cold staging: column blocks and rounds ---------------------------------------------------------------------------------
// A number of column blocks that fills the chip a whole number of times (two workgroups per CU), each window at most wmax
// columns and a multiple of 16 wide; nb_max bounds the (round, block) buckets: the smallest rounds (round_min tiles) make
// the most, and a balanced layout adds at most one round per workgroup of the stream's `grid`.  ncols >= 1.
struct StageBlocks {
    int64_t W = 0, nblk = 0, nb_max = 0;
};
inline StageBlocks stage_blocks(int64_t ncols, int32_t cus, int64_t wmax, int64_t n_tiles, int64_t round_min, int64_t grid)
{
    StageBlocks sb;
    const int64_t wave_of_wgs = 2 * (int64_t)cus;
    const int64_t nblk_goal = wave_of_wgs * cdiv(ncols, wave_of_wgs * wmax);
    sb.W = cdiv(cdiv(ncols, nblk_goal), 16) * 16;
    sb.nblk = cdiv(ncols, sb.W);
    sb.nb_max = (cdiv(n_tiles, round_min) + grid + 2) * sb.nblk;
    return sb;
}

// Rounds of at most `nt` tiles: every workgroup of the stream's persistent grid gets an equal share of the tiles, cut into
// equal rounds of whole tiles per wavefront (a multiple of NW).  round_tile0[r] = first tile of round r, its last element
// n_tiles; workgroup w walks rounds wg_round0[w] .. wg_round0[w + 1].  Returns the number of rounds.
inline int64_t stage_rounds(int64_t n_tiles, int64_t grid, int nt, int NW, std::vector<int32_t> &round_tile0,
                            std::vector<int32_t> &wg_round0)
{
    round_tile0.clear();
    wg_round0.clear();
    for (int64_t w = 0; w < grid; w++) {
        const int64_t tb = n_tiles * w / grid, te = n_tiles * (w + 1) / grid;
        wg_round0.push_back((int32_t)round_tile0.size());
        if (te > tb) {
            const int64_t k = cdiv(te - tb, nt);
            const int64_t per = cdiv(cdiv(te - tb, k), NW) * NW;
            for (int64_t t = tb; t < te; t += per) round_tile0.push_back((int32_t)t);
        }
    }
    wg_round0.push_back((int32_t)round_tile0.size());
    const int64_t n_rounds = (int64_t)round_tile0.size();
    round_tile0.push_back((int32_t)n_tiles);
    return n_rounds;
}

// after a count pass whose fullest round held max_round > cap values: the fullest round scales with the round's size, so
// jump to the size that would just fit (a multiple of NW), but step down by NW at least
inline int next_round_size(int nt, int64_t cap, int64_t max_round, int NW)
{
    const int next = (int)((double)nt * (double)cap / (double)max_round) / NW * NW;
    return next < nt - NW ? next : nt - NW;
}
// a pass of its own pays only when one index word in sixteen is cold
inline bool cold_stage_pays(int64_t n_cold, int64_t n_words) { return !(n_cold * 16 < n_words); }

}  // namespace spmvlayout
}  // namespace csrk
