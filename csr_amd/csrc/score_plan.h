// What the four factor-score drivers decide (topk_scores.hip, topk_scores_for.hip, rank_entries.hip, rank_entries_for.hip;
// DESIGN.md sections 8d-8i, "The drivers"): their constants, the one split rule behind rules 4 and 11 of include/csrk.h, the
// item interval of a split, the grids and the limits.  Plain C++17: no HIP, no common.h, no pointer into a panel and no
// device, so a host program includes it alone (tests/score_plan_host/main.cpp, under the sanitizers).  score_tile.h,
// score_list.h and rank_list.h take their constants from here.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define CSRK_SCORE_HD __host__ __device__
#else
#define CSRK_SCORE_HD
#endif

namespace csrk {

// ---- the score tile (score_tile.h)
constexpr int TS_THREADS = 256;
constexpr int TS_ROWS = 64;                     // rows of U per workgroup
constexpr int TS_TILE = 64;                     // items per tile
constexpr int SCORE_WAVE = 64;                  // (common.h's WAVE; score_host.h asserts that they agree)
constexpr int SCORE_GRID_CAP = 1 << 20;         // most workgroups of a grid-stride launch (the merge, the lens pass)

// ---- the running lists of topk_scores and topk_scores_for (score_list.h)
constexpr int TS_K_MAX = 1024;
constexpr int TS_NTOP_SMALL = 32;
constexpr int TS_NTOP_MAX = 128;
// The fill targets W are tuned to the 256 CUs of an MI355X and kept as found: they are not read from the device, so that
// splits_used is a function of the request alone (rule 4 [2], rule 11).
constexpr int TSF_S_MAX = 64;                   // most splits: the merge looks at no more than 64 x 128 candidates per row
constexpr int TSF_W_SMALL = 512;                // workgroups that fill the card: two per CU for n_top <= 32 (256 CUs) ...
constexpr int TSF_W_LARGE = 256;                // ... one per CU above that (topk_scores.hip, the two list classes)
constexpr int TSF_MERGE_THREADS = 256;
constexpr int64_t TSF_GRID_MAX = 0x7fffffffll;
// a workspace slot: score bits (8 B) and items (4 B) per list place, a count (4 B), see ts_work of score_list.h
constexpr int64_t TSF_SLOT_BYTES = 16, TSF_NTOP_BYTES = 12;

// ---- the lists of rank_entries and rank_entries_for (rank_list.h)
constexpr int RE_K_MAX = 1024;
constexpr int RE_T = 32;                        // test entries of a row per sweep
constexpr int REF_S_MAX = 64;                   // most splits
constexpr int REF_W = 512;                      // workgroups that fill the card: two per CU (256 CUs)
constexpr int REF_LEN_THREADS = 256;
constexpr int64_t REF_GRID_MAX = 0x7fffffffll;

constexpr bool score_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }
static_assert(score_pow2(TS_ROWS) && score_pow2(TS_TILE), "rows and items are cut into blocks by shifts and masks");
static_assert(score_pow2(TS_THREADS) && score_pow2(TSF_MERGE_THREADS) && score_pow2(REF_LEN_THREADS) && score_pow2(SCORE_WAVE),
              "whole wavefronts, and thread indices split by shifts and masks");
static_assert(TS_THREADS % SCORE_WAVE == 0 && TSF_MERGE_THREADS % SCORE_WAVE == 0, "whole wavefronts");
static_assert(TSF_S_MAX * TS_NTOP_MAX == 64 * 128, "the merge's stated bound: 64 x 128 candidates per row");
static_assert(TSF_W_SMALL == 2 * TSF_W_LARGE, "two workgroups per CU in the small list class, one in the large");
static_assert(TS_NTOP_SMALL < TS_NTOP_MAX && RE_T <= SCORE_WAVE, "two list classes; one lane per listed test entry");
static_assert(TSF_SLOT_BYTES == 8 + 4 + 4 && TSF_NTOP_BYTES == 8 + 4, "score bits, item and count of a slot");

constexpr int64_t score_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- limits and classes
inline bool ts_k_supported(int32_t k) { return k <= TS_K_MAX; }
inline bool ts_ntop_supported(int32_t n_top) { return n_top <= TS_NTOP_MAX; }
inline bool re_k_supported(int32_t k) { return k <= RE_K_MAX; }
inline bool ts_small_class(int32_t n_top) { return n_top <= TS_NTOP_SMALL; }      // TsClass<0>, else TsClass<1>

// 16-B loads: both panels say panel_16b (panel.h) and a row is a whole number of 16-B pieces
inline bool score_wide(bool u_16b, bool v_16b, int32_t k, int64_t per16) { return u_16b && v_16b && k % per16 == 0; }

// a diagnostic knob (CSRK_TOPK_SCORES_SELECT, CSRK_RANK_ENTRIES_COUNT) is off for exactly the string "0"; read per call
inline int score_knob_on(const char *env) { return !(env && env[0] == '0' && !env[1]); }

// ---- grids
inline int64_t score_row_blocks(int64_t n_rows) { return score_ceil_div(n_rows, TS_ROWS); }
inline int64_t score_capped_grid(int64_t items, int64_t per_block)
{
    const int64_t blocks = score_ceil_div(items, per_block);
    return blocks < SCORE_GRID_CAP ? blocks : SCORE_GRID_CAP;
}
inline int64_t tsf_merge_grid(int64_t n_rows) { return score_capped_grid(n_rows, TSF_MERGE_THREADS / SCORE_WAVE); }      // a wavefront per row
inline int64_t ref_lens_grid(int64_t n_rows) { return score_capped_grid(n_rows, REF_LEN_THREADS); }                     // a thread per row
// more workgroups than a grid holds: topk_scores_for's row blocks (grid.x; grid.y = S <= 64 always fits) ...
inline bool tsf_grid_too_large(int64_t n_rows) { return score_row_blocks(n_rows) > TSF_GRID_MAX; }
// ... and rank_entries_for's row blocks times splits
inline bool ref_grid_too_large(int64_t n_rows, int64_t S) { return score_row_blocks(n_rows) > REF_GRID_MAX / S; }

// ---- the split rule (rules 4 and 11 of include/csrk.h): with T tiles of items and B blocks of rows, one split when either
// is zero; else the caller's `forced` (>= 1) or ceil(fill / B), and at most min(T, s_max).
inline int32_t score_splits(int64_t n_rows, int32_t n_items, int32_t forced, int32_t fill, int32_t s_max)
{
    const int64_t tiles = score_ceil_div((int64_t)n_items, TS_TILE), blocks = score_row_blocks(n_rows);
    const int64_t most = tiles < s_max ? tiles : s_max;
    int64_t s = 1;
    if (tiles > 0 && blocks > 0) {
        s = forced >= 1 ? forced : score_ceil_div(fill, blocks);
        s = s > most ? most : s;
    }
    return (int32_t)s;
}
inline int32_t tsf_fill(int32_t n_top) { return ts_small_class(n_top) ? TSF_W_SMALL : TSF_W_LARGE; }
inline int32_t tsf_splits(int64_t n_rows, int32_t n_items, int32_t n_top, int32_t forced)      // rule 4
{
    return score_splits(n_rows, n_items, forced, tsf_fill(n_top), TSF_S_MAX);
}
inline int32_t ref_splits(int64_t n_rows, int32_t n_items, int32_t forced)                      // rule 11
{
    return score_splits(n_rows, n_items, forced, REF_W, REF_S_MAX);
}
// the workspace of topk_scores_for: none for one split, else n_rows * S slots rounded up to 16 bytes
inline int64_t tsf_work_bytes(int64_t n_rows, int32_t S, int32_t n_top)
{
    return S == 1 ? 0 : score_ceil_div(n_rows * S * (TSF_SLOT_BYTES + (n_top - 1) * TSF_NTOP_BYTES), 16) * 16;
}

// ---- the items of split `split` of S: the tiles [split T / S, (split + 1) T / S), cut at n_items.  For S <= T the ranges
// tile [0, n_items), start on tile boundaries and none is empty.  topk_scores_for_kernel and rank_entries_for_kernel call it.
struct ScoreItemRange {
    int64_t j_begin, j_end;
};
CSRK_SCORE_HD inline ScoreItemRange score_item_range(int split, int S, int32_t n_items)
{
    const int64_t tiles = ((int64_t)n_items + TS_TILE - 1) / TS_TILE;
    const int64_t j_begin = split * tiles / S * TS_TILE, j_to = (split + 1) * tiles / S * TS_TILE;
    return {j_begin, j_to < n_items ? j_to : (int64_t)n_items};
}

}  // namespace csrk
