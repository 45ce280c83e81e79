// The general sparse product's host decisions (spgemm.hip, "the driver"): the constants behind them and one pure function
// per decision -- which routes a product may use, when a budget sends its rows to the fallback paths, how large the
// driver's scratch is.  Plain host arithmetic, no device code: spgemm.hip calls it, and tests/spgemm_plan_host runs it as a
// stand-alone program at every budget's edge (no small input reaches those fallbacks on the device).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace csrk {

constexpr int SG_WAVE_CAP = 128;  // rows with at most this many products take the sub-wavefront kernels (sg_quad_kernel)
// (sg_count_products: the long rows' lists and the list of very long rows, spgemm.hip)
constexpr int SG_LONG_LISTS = 64, SG_LONG_STRIDE = 32;      // (counters SG_LONG_STRIDE int32 apart)
constexpr int SG_COUNT_VLONG = 4096;

// (column strips, spgemm.hip: the measurements behind the width are there)
#ifndef CSRK_SGS_W
#define CSRK_SGS_W 832
#endif
constexpr int SGS_W = CSRK_SGS_W;
constexpr int SGS_MAX_S = 256;              // strips per row (wider products fall back to the workgroup paths)
constexpr int64_t SGS_TABLE_BUDGET = 2ll << 30;
constexpr int64_t SGS_TEMP_BUDGET = 24ll << 30;      // bytes of compacted strips held between the one pass and the copy

// (expand, sort, compress, spgemm.hip)
constexpr int64_t SGE_BUDGET_PRODUCTS = 200ll << 20;     // above this the round-1 heavy-row paths are used instead
#ifndef CSRK_SGE_MIN
#define CSRK_SGE_MIN 32
#endif
constexpr int64_t SGE_MIN = CSRK_SGE_MIN;                // rows with more products than this (and not dense enough for strips)

namespace sgplan {

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// padded length of a dense work row's column list for the bitonic network: the power of two at or above ncols_b
inline int64_t scratch_len(int32_t ncols_b)
{
    int64_t n = 1;
    while (n < (int64_t)ncols_b) n <<= 1;
    return n;
}

// sg_count_products: workgroups of 32 rows (eight lanes a row), and the rows one of the SG_LONG_LISTS lists holds at most
inline int64_t count_blocks(int32_t nrows_a) { return ceil_div((int64_t)nrows_a * 8, 256); }
inline int32_t long_cap(int32_t nrows_a) { return (int32_t)(ceil_div(count_blocks(nrows_a), (int64_t)SG_LONG_LISTS) * 32); }

// int32 slots of the strip list's allocation: the strip rows later (at most every row), before that the lists of long
// rows and, behind them, the list of very long rows (at most nnz / SG_COUNT_VLONG of them)
inline int64_t list_s_slots(int32_t nrows_a, int64_t nnz_a)
{
    return std::max<int64_t>((int64_t)nrows_a + 1, (int64_t)SG_LONG_LISTS * long_cap(nrows_a) + nnz_a / SG_COUNT_VLONG + 1);
}

// column strips per row in force: FAST operands only, unless the knob (CSRK_SPGEMM_STRIPS=0: workgroup paths only) turns
// them off, the product is too wide or has too many (row, strip) units.  0: off
inline int32_t strips_in_force(int32_t ncols_b, int32_t nrows_a, bool fast, bool knob_on)
{
    int32_t strips = 0;
    if (fast && knob_on) {
        strips = (int32_t)ceil_div(ncols_b, SGS_W);
        if (strips > SGS_MAX_S || (int64_t)nrows_a * strips > (1ll << 30)) strips = 0;
    }
    return strips;
}

// the strips' density test (sg_list_rows), whether they can be used or not
inline int32_t s_dense(int32_t ncols_b)
{
    int32_t s = (int32_t)ceil_div(ncols_b, SGS_W);
    if (s > SGS_MAX_S) s = 0;
    return s;
}

// does the sub-range table of n_strip_e entries of A pay for itself?  (no: the rows are listed again without strips)
inline bool table_pays(int32_t n_strip_e, int32_t strips) { return (int64_t)n_strip_e * (strips + 1) * 4 <= SGS_TABLE_BUDGET; }

// rows above this many products go to expand-sort-compress (-1: none; CSRK_SPGEMM_ESC=0, or a budget below said so)
inline int64_t esc_min(bool knob_on) { return knob_on ? SGE_MIN : -1; }

// do the products of the expand-sort-compress rows fit the sort's budget ...
inline bool esc_fits_sort(int64_t products) { return products <= SGE_BUDGET_PRODUCTS; }

// ... and free device memory?  The product matrix, its two transposes and the sort's scratch are ~52 B per product at the
// peak, beside 64 MiB for everything else.
inline bool esc_fits_memory(int64_t products, size_t mfree) { return (size_t)products * 52 + (64u << 20) <= mfree; }

// with expand-sort-compress taking every row above 32 products, the workgroup-hash and 32-lane kernels have no rows
inline bool hash_rows(int64_t esc_min) { return esc_min < 0 || esc_min > SG_WAVE_CAP; }
inline bool mid_rows(int64_t esc_min) { return esc_min < 0 || esc_min > 32; }

// the rows of at most SG_WAVE_CAP products in one pass: when there are any and their temporary (12 B an entry) fits its budget
inline bool small_fused(int64_t total) { return total > 0 && total * 12 <= SGS_TEMP_BUDGET / 4; }

// the strips in one pass: when their temporary (12 B an entry of the units' capacities) fits its budget
inline bool strip_fused(int64_t total_cap) { return total_cap * 12 <= SGS_TEMP_BUDGET; }

// workgroups of the dense path, each with an HBM work, marker and scratch row: at most 256, a row each, and 4 GiB together
inline int grid_dense(int32_t n_large, int32_t ncols_b, int64_t scratch_len)
{
    const int64_t per = (int64_t)ncols_b * 12 + scratch_len * 4;
    int64_t g_max = (4ll << 30) / (per > 0 ? per : 1);
    if (g_max < 1) g_max = 1;
    int grid = (int)(n_large < 256 ? n_large : 256);
    if (grid > g_max) grid = (int)g_max;
    return grid;
}

}  // namespace sgplan
}  // namespace csrk
