// Host check of csr_amd/csrc/score_plan.h, built by tests/test_score_plan_host.py with the system compiler and
// -fsanitize=address,undefined.  Two modes.
//   (no argument)  every function of the header at its edges, the expected values worked out by hand from rules 4 and 11 of
//                  include/csrk.h; the constants are pinned first, so that a changed constant shows here and not as a
//                  shifted edge.
//   case           requests on stdin, one per line -- "4 n_rows n_items n_top splits" or "11 n_rows n_items splits"
//                  (splits = 0: automatic) -- answered with "S bytes" or "S", which the Python test compares with
//                  tests/score_rules.py's restatement of the two rules.
#include "score_plan.h"

#include <climits>
#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace csrk;

static int failures = 0;
static int case_failures = 0;

static void expect_eq(const char *what, int line, long long got, long long want)
{
    if (got == want) return;
    printf("FAIL %s:%d: %s = %lld, want %lld\n", __FILE__, line, what, got, want);
    case_failures++;
}
#define EXPECT_EQ(expr, want) expect_eq(#expr, __LINE__, (long long)(expr), (long long)(want))

static void done(const char *name)
{
    printf("%s %s\n", case_failures ? "FAIL" : "ok  ", name);
    failures += case_failures;
    case_failures = 0;
}

static const int32_t MANY = 2000000;      // 31 250 tiles: the tile count never binds

static void constants()
{
    EXPECT_EQ(TS_THREADS, 256), EXPECT_EQ(TS_ROWS, 64), EXPECT_EQ(TS_TILE, 64), EXPECT_EQ(SCORE_WAVE, 64);
    EXPECT_EQ(TS_K_MAX, 1024), EXPECT_EQ(TS_NTOP_SMALL, 32), EXPECT_EQ(TS_NTOP_MAX, 128);
    EXPECT_EQ(TSF_S_MAX, 64), EXPECT_EQ(TSF_W_SMALL, 512), EXPECT_EQ(TSF_W_LARGE, 256), EXPECT_EQ(TSF_MERGE_THREADS, 256);
    EXPECT_EQ(TSF_GRID_MAX, 2147483647ll), EXPECT_EQ(TSF_SLOT_BYTES, 16), EXPECT_EQ(TSF_NTOP_BYTES, 12);
    EXPECT_EQ(RE_K_MAX, 1024), EXPECT_EQ(RE_T, 32), EXPECT_EQ(REF_S_MAX, 64), EXPECT_EQ(REF_W, 512), EXPECT_EQ(REF_LEN_THREADS, 256);
    EXPECT_EQ(REF_GRID_MAX, 2147483647ll), EXPECT_EQ(SCORE_GRID_CAP, 1048576);
    // the predicate behind the header's static asserts
    EXPECT_EQ(score_pow2(1), 1), EXPECT_EQ(score_pow2(2), 1), EXPECT_EQ(score_pow2(64), 1), EXPECT_EQ(score_pow2(1ll << 62), 1);
    EXPECT_EQ(score_pow2(0), 0), EXPECT_EQ(score_pow2(-4), 0), EXPECT_EQ(score_pow2(3), 0), EXPECT_EQ(score_pow2(6), 0), EXPECT_EQ(score_pow2(96), 0);
    done("constants");
}

static void knob()
{
    EXPECT_EQ(score_knob_on(nullptr), 1), EXPECT_EQ(score_knob_on(""), 1), EXPECT_EQ(score_knob_on("0"), 0);
    EXPECT_EQ(score_knob_on("00"), 1), EXPECT_EQ(score_knob_on("1"), 1), EXPECT_EQ(score_knob_on("0 "), 1);
    done("the knob parser");
}

static void limits_and_classes()
{
    EXPECT_EQ(ts_k_supported(1), 1), EXPECT_EQ(ts_k_supported(1024), 1), EXPECT_EQ(ts_k_supported(1025), 0);
    EXPECT_EQ(ts_ntop_supported(1), 1), EXPECT_EQ(ts_ntop_supported(128), 1), EXPECT_EQ(ts_ntop_supported(129), 0);
    EXPECT_EQ(re_k_supported(1024), 1), EXPECT_EQ(re_k_supported(1025), 0), EXPECT_EQ(re_k_supported(INT32_MAX), 0);
    EXPECT_EQ(ts_small_class(1), 1), EXPECT_EQ(ts_small_class(32), 1), EXPECT_EQ(ts_small_class(33), 0), EXPECT_EQ(ts_small_class(128), 0);
    EXPECT_EQ(tsf_fill(1), 512), EXPECT_EQ(tsf_fill(32), 512), EXPECT_EQ(tsf_fill(33), 256), EXPECT_EQ(tsf_fill(128), 256);
    done("limits and list classes");
}

static void wide()
{
    EXPECT_EQ(score_wide(true, true, 4, 2), 1), EXPECT_EQ(score_wide(true, true, 5, 2), 0), EXPECT_EQ(score_wide(true, true, 2, 2), 1);
    EXPECT_EQ(score_wide(true, true, 1, 2), 0), EXPECT_EQ(score_wide(true, true, 4, 4), 1), EXPECT_EQ(score_wide(true, true, 6, 4), 0);
    EXPECT_EQ(score_wide(true, true, 8, 4), 1), EXPECT_EQ(score_wide(false, true, 4, 2), 0), EXPECT_EQ(score_wide(true, false, 4, 2), 0);
    EXPECT_EQ(score_wide(false, false, 4, 4), 0);
    done("the wide rule");
}

static void row_blocks()
{
    EXPECT_EQ(score_row_blocks(0), 0), EXPECT_EQ(score_row_blocks(1), 1), EXPECT_EQ(score_row_blocks(64), 1);
    EXPECT_EQ(score_row_blocks(65), 2), EXPECT_EQ(score_row_blocks(128), 2), EXPECT_EQ(score_row_blocks(129), 3);
    EXPECT_EQ(score_row_blocks(64 * 512), 512), EXPECT_EQ(score_row_blocks(64 * 512 + 1), 513);
    EXPECT_EQ(score_row_blocks(64 * 512 - 64), 511), EXPECT_EQ(score_row_blocks(64 * 512 + 64), 513);
    EXPECT_EQ(score_row_blocks(64ll * 2147483647), 2147483647ll), EXPECT_EQ(score_row_blocks(64ll * 2147483647 + 1), 2147483648ll);
    done("row blocks");
}

// W workgroups fill the card; B = ceil(n_rows / 64) row blocks take ceil(W / B) splits, at most 64
static void rows_against_fill(const char *name, int32_t W, int32_t n_top)
{
    const bool r11 = n_top == 0;
    auto S = [&](int64_t n_rows) { return r11 ? ref_splits(n_rows, MANY, 0) : tsf_splits(n_rows, MANY, n_top, 0); };
    EXPECT_EQ(S(0), 1);                       // no row block: one split
    EXPECT_EQ(S(1), 64), EXPECT_EQ(S(64), 64), EXPECT_EQ(S(65), 64);      // W / 1 and W / 2 are above S_max
    EXPECT_EQ(S(64 * (W / 64)), 64);          // B = W / 64: exactly 64
    EXPECT_EQ(S(64 * (W / 64) + 1), W == 512 ? 57 : 52);                  // B = 9: ceil(512 / 9) = 57; B = 5: ceil(256 / 5) = 52
    EXPECT_EQ(S(1024), W / 16);               // B = 16
    EXPECT_EQ(S(64ll * W - 64), 2);           // B = W - 1: ceil(W / (W - 1)) = 2
    EXPECT_EQ(S(64ll * W), 1);                // B = W
    EXPECT_EQ(S(64ll * W + 1), 1);            // B = W + 1
    EXPECT_EQ(S(64ll * W + 64), 1);
    EXPECT_EQ(S(64ll * (W / 2)), 2), EXPECT_EQ(S(64ll * (W / 2) + 1), 2), EXPECT_EQ(S(64ll * (W / 2) - 64), 3);      // 512/255 = 2.008, 256/127 = 2.02
    done(name);
}

static void tile_counts()
{
    // T tiles with n_items on the boundary (64 T) and one past the boundary before (64 (T - 1) + 1); one row block, automatic
    for (int r = 0; r < 2; r++) {
        auto S = [&](int32_t n_items, int32_t forced) { return r ? ref_splits(1, n_items, forced) : tsf_splits(1, n_items, 20, forced); };
        EXPECT_EQ(S(0, 0), 1), EXPECT_EQ(S(0, 5), 1);                    // T = 0: one split whatever is asked
        EXPECT_EQ(S(64, 0), 1), EXPECT_EQ(S(1, 0), 1), EXPECT_EQ(S(64, 7), 1);      // T = 1
        EXPECT_EQ(S(65, 0), 2), EXPECT_EQ(S(128, 0), 2), EXPECT_EQ(S(129, 0), 3);   // T = 2, 2, 3
        EXPECT_EQ(S(64 * 63, 0), 63), EXPECT_EQ(S(64 * 63 + 1, 0), 64);  // T = 63, 64
        EXPECT_EQ(S(64 * 64, 0), 64), EXPECT_EQ(S(64 * 63 + 1, 0), 64);  // T = S_max
        EXPECT_EQ(S(64 * 65, 0), 64), EXPECT_EQ(S(64 * 64 + 1, 0), 64);  // T = S_max + 1
        EXPECT_EQ(S(INT32_MAX, 0), 64);                                  // T = 2^25: no overflow on the way
    }
    done("tile counts");
}

static void forced_splits()
{
    for (int r = 0; r < 2; r++) {
        auto S = [&](int64_t n_rows, int32_t n_items, int32_t forced) {
            return r ? ref_splits(n_rows, n_items, forced) : tsf_splits(n_rows, n_items, 33, forced);
        };
        EXPECT_EQ(S(1, MANY, 1), 1), EXPECT_EQ(S(1, MANY, 2), 2), EXPECT_EQ(S(1, MANY, 64), 64), EXPECT_EQ(S(1, MANY, 65), 64);
        EXPECT_EQ(S(1, MANY, INT32_MAX), 64);
        EXPECT_EQ(S(1, 130, 2), 2), EXPECT_EQ(S(1, 130, 3), 3), EXPECT_EQ(S(1, 130, 4), 3), EXPECT_EQ(S(1, 130, INT32_MAX), 3);      // 3 tiles
        EXPECT_EQ(S(64 * 512 + 1, MANY, 5), 5);                         // forced beats the fill rule ...
        EXPECT_EQ(S(0, MANY, 5), 1), EXPECT_EQ(S(1, 0, 5), 1);           // ... but not "nothing to split"
    }
    done("forced splits");
}

static void workspace_bytes()
{
    for (int32_t n_top : {1, 32, 33, 128}) EXPECT_EQ(tsf_work_bytes(1000, 1, n_top), 0);      // S = 1: no workspace
    EXPECT_EQ(tsf_work_bytes(0, 1, 20), 0);
    EXPECT_EQ(tsf_work_bytes(1, 2, 1), 32);             // a slot of n_top = 1 is 16 B
    EXPECT_EQ(tsf_work_bytes(3, 3, 2), 256);            // 9 slots of 28 B = 252, rounded up
    EXPECT_EQ(tsf_work_bytes(1, 2, 32), 784);           // 16 + 31 * 12 = 388; 776 -> 784
    EXPECT_EQ(tsf_work_bytes(1, 2, 33), 800);           // 16 + 32 * 12 = 400; 800 is a multiple
    EXPECT_EQ(tsf_work_bytes(1, 2, 128), 3088);         // 16 + 127 * 12 = 1540; 3080 -> 3088
    EXPECT_EQ(tsf_work_bytes(1, 3, 128), 4624);         // 4620 -> 4624
    EXPECT_EQ(tsf_work_bytes(1024, 32, 20), 7995392);   // 32 768 slots of 244 B, a multiple
    EXPECT_EQ(tsf_work_bytes(64, 64, 20), 999424);
    EXPECT_EQ(tsf_work_bytes(64ll * 2147483647, 64, 128), 64ll * 2147483647 * 64 * 1540);      // 1.35e16: int64 all the way
    done("workspace bytes");
}

static void grid_limits()
{
    const int64_t most = 2147483647;          // 0x7fffffff
    EXPECT_EQ(tsf_grid_too_large(0), 0), EXPECT_EQ(tsf_grid_too_large(64 * most), 0), EXPECT_EQ(tsf_grid_too_large(64 * most - 63), 0);
    EXPECT_EQ(tsf_grid_too_large(64 * most + 1), 1);
    EXPECT_EQ(ref_grid_too_large(64 * most, 1), 0), EXPECT_EQ(ref_grid_too_large(64 * most + 1, 1), 1);
    EXPECT_EQ(ref_grid_too_large(64ll * 1073741823, 2), 0), EXPECT_EQ(ref_grid_too_large(64ll * 1073741823 + 1, 2), 1);      // floor(most / 2)
    EXPECT_EQ(ref_grid_too_large(64ll * 33554431, 64), 0), EXPECT_EQ(ref_grid_too_large(64ll * 33554431 + 1, 64), 1);        // floor(most / 64)
    EXPECT_EQ(ref_grid_too_large(0, 64), 0);
    done("the two grid limits");
}

static void capped_grids()
{
    const int64_t cap = 1 << 20;
    EXPECT_EQ(tsf_merge_grid(1), 1), EXPECT_EQ(tsf_merge_grid(4), 1), EXPECT_EQ(tsf_merge_grid(5), 2);      // four rows per workgroup
    EXPECT_EQ(tsf_merge_grid(4 * cap - 4), cap - 1), EXPECT_EQ(tsf_merge_grid(4 * cap), cap), EXPECT_EQ(tsf_merge_grid(4 * cap + 1), cap);
    EXPECT_EQ(tsf_merge_grid(64ll * 2147483647), cap);
    EXPECT_EQ(ref_lens_grid(1), 1), EXPECT_EQ(ref_lens_grid(256), 1), EXPECT_EQ(ref_lens_grid(257), 2);     // 256 rows per workgroup
    EXPECT_EQ(ref_lens_grid(256 * cap - 256), cap - 1), EXPECT_EQ(ref_lens_grid(256 * cap), cap), EXPECT_EQ(ref_lens_grid(256 * cap + 1), cap);
    EXPECT_EQ(ref_lens_grid(64ll * 2147483647), cap);
    done("the capped grids");
}

static void item_ranges()
{
    // 129 items are two tiles and one item
    ScoreItemRange a = score_item_range(0, 1, 129);
    EXPECT_EQ(a.j_begin, 0), EXPECT_EQ(a.j_end, 129);
    a = score_item_range(0, 2, 129);
    EXPECT_EQ(a.j_begin, 0), EXPECT_EQ(a.j_end, 64);                  // tiles [0, 1)
    a = score_item_range(1, 2, 129);
    EXPECT_EQ(a.j_begin, 64), EXPECT_EQ(a.j_end, 129);                // tiles [1, 3), cut at n_items
    a = score_item_range(2, 3, 129);
    EXPECT_EQ(a.j_begin, 128), EXPECT_EQ(a.j_end, 129);               // one item
    a = score_item_range(63, 64, INT32_MAX);                          // 2^25 tiles: the last of 64 ranges
    EXPECT_EQ(a.j_begin, 63ll * 524288 * 64), EXPECT_EQ(a.j_end, INT32_MAX);
    a = score_item_range(1, 3, 2000000);                              // 31 250 tiles exactly: tiles [10 416, 20 833)
    EXPECT_EQ(a.j_begin, 666624), EXPECT_EQ(a.j_end, 1333312);
    a = score_item_range(0, 1, 0);
    EXPECT_EQ(a.j_begin, 0), EXPECT_EQ(a.j_end, 0);
    for (int32_t n_items : {1, 63, 64, 65, 129, 64 * 64, 64 * 64 + 1, 2000000}) {
        const int64_t tiles = (n_items + 63) / 64;
        for (int S = 1; S <= (tiles < 64 ? tiles : 64); S++) {
            int64_t at = 0;
            for (int s = 0; s < S; s++) {
                const ScoreItemRange r = score_item_range(s, S, n_items);
                EXPECT_EQ(r.j_begin, at);                             // the ranges tile [0, n_items) ...
                EXPECT_EQ(r.j_begin % 64, 0);                         // ... every one starts on a tile boundary ...
                EXPECT_EQ(r.j_end > r.j_begin, 1);                    // ... and none is empty
                at = r.j_end;
            }
            EXPECT_EQ(at, n_items);
        }
    }
    done("item ranges");
}

static int answer_requests()
{
    int rule;
    while (scanf("%d", &rule) == 1) {
        long long n_rows;
        int n_items, n_top, splits;
        if (rule == 4 && scanf("%lld %d %d %d", &n_rows, &n_items, &n_top, &splits) == 4) {
            const int32_t S = tsf_splits(n_rows, n_items, n_top, splits);
            printf("%d %lld\n", S, (long long)tsf_work_bytes(n_rows, S, n_top));
        } else if (rule == 11 && scanf("%lld %d %d", &n_rows, &n_items, &splits) == 3) {
            printf("%d\n", ref_splits(n_rows, n_items, splits));
        } else {
            printf("bad request\n");
            return 2;
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "case")) return answer_requests();
    constants();
    knob();
    limits_and_classes();
    wide();
    row_blocks();
    rows_against_fill("rule 11 over the rows", 512, 0);
    rows_against_fill("rule 4 over the rows, n_top <= 32", 512, 32);
    rows_against_fill("rule 4 over the rows, n_top > 32", 256, 33);
    tile_counts();
    forced_splits();
    workspace_bytes();
    grid_limits();
    capped_grids();
    item_ranges();
    if (failures) {
        printf("%d check(s) failed\n", failures);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
