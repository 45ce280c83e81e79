// Host check of csr_amd/csrc/spgemm_order_plan.h, built by tests/test_spgemm_order_plan_host.py with the system compiler
// and -fsanitize=address,undefined.  Two modes.
//   (no argument)                every function of the header at its edges, the expected values worked out by hand from the
//                                rule's statement; the constants are pinned first, so that a changed constant shows here and
//                                not as a shifted edge.
//   case LDS_MAX NCOLS B_NNZ     one product of tests/spgemm_cases.py: a line "PRODUCTS ENTRIES" per row of C on standard
//                                input.  The rows are counted by octave as so_list_rows_kernel counts them (a row of at least
//                                SO_LEAST products under the leading zeros of its count; the memory flag for 2^32 - 1
//                                products or more entries than the plan's cap_long), then the header's LDS plan and tiers
//                                are printed: "constants ...", "lds ...", "tiers ...", "cursors ...".
#include "spgemm_order_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace csrk;
using namespace csrk::soplan;

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

constexpr int MI355X = 163840;      // LDS a workgroup may have there
constexpr int64_t P32 = 0xffffffffll;

static void constant_cases()
{
    EXPECT_EQ(SO_LEAST, 64), EXPECT_EQ(SO_TINY, 256), EXPECT_EQ(SO_WAVE, 1024), EXPECT_EQ(SO_MID, 4096), EXPECT_EQ(SO_SUB, 16);
    EXPECT_EQ(SO_OCTAVES, 64), EXPECT_EQ(SO_LDS_BYTES, 153600), EXPECT_EQ(SO_WIN_WORDS, 16384), EXPECT_EQ(SO_WIN, 524288);
    EXPECT_EQ(SO_PLACE_THREADS, 1024), EXPECT_EQ(SO_TABLES_BYTES, 18432), EXPECT_EQ(SO_WIN_ENTRY, 2048);
    EXPECT_EQ(SO_WIN_COLS_MOST, 16384), EXPECT_EQ(SO_WIN_COLS_LEAST, 1024);
    EXPECT_EQ(LANES, 64), EXPECT_EQ(LONG_THREADS, 1024), EXPECT_EQ(MID_THREADS, 256);
    done("constants");

    // leading zeros of an int64: 2^k has 63 - k
    EXPECT_EQ(octave_of(1), 63), EXPECT_EQ(octave_of(2), 62), EXPECT_EQ(octave_of(3), 62), EXPECT_EQ(octave_of(4), 61);
    EXPECT_EQ(octave_of(63), 58), EXPECT_EQ(octave_of(64), 57), EXPECT_EQ(octave_of(255), 56), EXPECT_EQ(octave_of(256), 55);
    EXPECT_EQ(octave_of(1023), 54), EXPECT_EQ(octave_of(1024), 53), EXPECT_EQ(octave_of(4095), 52), EXPECT_EQ(octave_of(4096), 51);
    EXPECT_EQ(octave_of(P32), 32), EXPECT_EQ(octave_of(P32 + 1), 31), EXPECT_EQ(octave_of(INT64_MAX), 1);
    EXPECT_EQ(octave_of(SO_LEAST), 57), EXPECT_EQ(octave_of(SO_TINY), 55), EXPECT_EQ(octave_of(SO_WAVE), 53), EXPECT_EQ(octave_of(SO_MID), 51);
    EXPECT_EQ(is_pow2(1), 1), EXPECT_EQ(is_pow2(4096), 1), EXPECT_EQ(is_pow2(4097), 0), EXPECT_EQ(is_pow2(4095), 0), EXPECT_EQ(is_pow2(0), 0);
    EXPECT_EQ(is_pow2(96), 0), EXPECT_EQ(is_pow2(-4), 0);
    done("the tier exponents");

    // s_bs 8 T, s_off 8 (T + 1), s_wave64 8 T / 64, s_take and s_found 4 each, s_wave 4 T / 64
    EXPECT_EQ(walk_static_lds(1024, 64), 8192 + 8200 + 128 + 8 + 64), EXPECT_EQ(walk_static_lds(1024, 64), 16592);
    EXPECT_EQ(walk_static_lds(256, 64), 2048 + 2056 + 32 + 8 + 16), EXPECT_EQ(walk_static_lds(64, 64), 512 + 520 + 8 + 8 + 4);
    EXPECT_EQ(walk_static_lds(LONG_THREADS, LANES) <= (size_t)SO_TABLES_BYTES, 1);
    done("the static tables");
}

static void lds_cases()
{
    // min(150 KiB, the device's limit - 18 KiB): they meet at 153600 + 18432 = 172032
    EXPECT_EQ(so_lds_plan(MI355X, 5000, 10).budget, 145408);
    EXPECT_EQ(so_lds_plan(172031, 5000, 10).budget, 153599), EXPECT_EQ(so_lds_plan(172032, 5000, 10).budget, 153600);
    EXPECT_EQ(so_lds_plan(172033, 5000, 10).budget, 153600), EXPECT_EQ(so_lds_plan(1 << 20, 5000, 10).budget, 153600);
    EXPECT_EQ(so_lds_plan(65536, 5000, 10).budget, 47104), EXPECT_EQ(so_lds_plan(18432, 5000, 10).budget, 0);
    EXPECT_EQ(so_lds_plan(0, 5000, 10).budget, -18432), EXPECT_EQ(so_lds_plan(INT32_MAX, 5000, 10).budget, 153600);
    done("the budget");

    // by column: 4 (ncols + 2 ceil(ncols / 32)) bytes and 8 per word of the window, 145408 in all on the MI355X.  A window
    // of w words asks ncols + 2 ceil(ncols / 32) <= (145408 - 8 w) / 4: 3584, 19968, 28160, 32256, 34304 for 16384 ... 1024
    const struct {
        int32_t ncols;
        long long by_col;
        int32_t win;
    } ladder[] = {{0, 0, 16384},           {1, 12, 16384},         {32, 136, 16384},        {33, 148, 16384},
                  {3372, 14336, 16384},    {3373, 14340, 8192},    {18792, 79872, 8192},    {18793, 79876, 4096},
                  {26502, 112640, 4096},   {26503, 112644, 2048},  {30358, 129024, 2048},   {30359, 129028, 1024},
                  {32286, 137216, 1024},   {32287, 137220, 0},     {100000, 425000, 0},     {INT32_MAX, 9126805500ll, 0}};
    for (const auto &l : ladder) {
        const LdsPlan p = so_lds_plan(MI355X, l.ncols, 10);
        EXPECT_EQ(p.by_col, l.by_col), EXPECT_EQ(p.win_cols, l.win), EXPECT_EQ(p.cols_mode, l.win > 0), EXPECT_EQ(p.ok, 1);
        if (l.win) {
            EXPECT_EQ(p.win_long, l.win), EXPECT_EQ(p.cap_long, INT32_MAX), EXPECT_EQ(p.lds_long, l.by_col + 8ll * l.win);
            EXPECT_EQ((long long)p.lds_long <= p.budget, 1);
        } else {
            EXPECT_EQ(p.win_long, 2048), EXPECT_EQ(p.cap_long, 16128), EXPECT_EQ(p.lds_long, 145408);
        }
    }
    // with the cap in force (153600): 16384 words ask ncols + 2 ceil(ncols / 32) <= 5632: 5300 + 2 * 166 = 5632
    EXPECT_EQ(so_lds_plan(172032, 5300, 10).win_cols, 16384), EXPECT_EQ(so_lds_plan(172032, 5301, 10).win_cols, 8192);
    EXPECT_EQ(so_lds_plan(172031, 5300, 10).win_cols, 8192);
    done("the window ladder");

    // a row of B of 2^32 - 1 entries could fill a batch's 32-bit indices: by entry then, whatever fits
    const LdsPlan below = so_lds_plan(MI355X, 5000, P32 - 1), at = so_lds_plan(MI355X, 5000, P32), above = so_lds_plan(MI355X, 5000, P32 + 1);
    EXPECT_EQ(below.cols_mode, 1), EXPECT_EQ(below.win_cols, 8192), EXPECT_EQ(below.win_long, 8192), EXPECT_EQ(below.lds_long, 21256 + 65536);      // 4 (5000 + 2 * 157)
    EXPECT_EQ(at.cols_mode, 0), EXPECT_EQ(at.win_cols, 8192), EXPECT_EQ(at.win_long, 2048), EXPECT_EQ(at.cap_long, 16128), EXPECT_EQ(at.lds_long, 145408);
    EXPECT_EQ(above.cols_mode, 0), EXPECT_EQ(above.cap_long, 16128), EXPECT_EQ(so_lds_plan(MI355X, 5000, 0).cols_mode, 1);
    done("cols_mode at 2^32 - 1 entries of B");

    // by entry: a window of 2048 words (16384 B) and 8 B per entry of the row in what is left; the 256-thread walk and the
    // placing pass do not depend on the device
    const struct {
        int lds_max;
        int32_t cap;
    } entry[] = {{MI355X, 16128}, {172032, 17152}, {1 << 20, 17152}, {65536, 3840}, {67583, 4095}, {67584, 4096}, {34816, 0}, {34824, 1}, {18432, 0}, {0, 0}};
    for (const auto &e : entry) {
        const LdsPlan p = so_lds_plan(e.lds_max, 100000, 10);
        EXPECT_EQ(p.cols_mode, 0), EXPECT_EQ(p.win_cols, 0), EXPECT_EQ(p.win_long, 2048), EXPECT_EQ(p.cap_long, e.cap);
        EXPECT_EQ(p.lds_long, 8ll * e.cap + 16384);
        EXPECT_EQ(p.win_mid, 128), EXPECT_EQ(p.cap_mid, 4096), EXPECT_EQ(p.lds_mid, 33792), EXPECT_EQ(p.lds_place, 131072);
    }
    done("by entry, and the 256-thread walk");

    // ok = the placing pass's 131072 B and 2048 more fit the device, and the 1024-thread walk holds a row of SO_MID entries.
    // 64 KiB: neither.  The first asks 133120 B, the second (by entry) 18432 + 16384 + 32768 = 67584: the first binds.
    const LdsPlan small = so_lds_plan(65536, 100000, 10);
    EXPECT_EQ(small.ok, 0), EXPECT_EQ(small.cap_long, 3840), EXPECT_EQ(small.cap_long < SO_MID, 1), EXPECT_EQ(small.lds_place, 131072);
    EXPECT_EQ((long long)small.lds_place + 2048 > 65536, 1);
    const LdsPlan small_cols = so_lds_plan(65536, 1000, 10);      // by column there: 4256 B of tables and a window of 4096 words
    EXPECT_EQ(small_cols.cols_mode, 1), EXPECT_EQ(small_cols.win_long, 4096), EXPECT_EQ(small_cols.lds_long, 37024), EXPECT_EQ(small_cols.ok, 0);
    EXPECT_EQ(so_lds_plan(133119, 100000, 10).ok, 0), EXPECT_EQ(so_lds_plan(133120, 100000, 10).ok, 1), EXPECT_EQ(so_lds_plan(133120, 100000, 10).cap_long, 12288);
    EXPECT_EQ(so_lds_plan(133119, 1000, 10).ok, 0), EXPECT_EQ(so_lds_plan(133120, 1000, 10).ok, 1);
    EXPECT_EQ(so_lds_plan(67584, 100000, 10).ok, 0), EXPECT_EQ(so_lds_plan(MI355X, 100000, P32).ok, 1), EXPECT_EQ(so_lds_plan(0, 0, 0).ok, 0);
    done("ok, and a 64 KiB device");
}

struct Want {
    int32_t listed, n_long, n_mid, n_wave, n_small;
};

static void expect_tiers(int line, const int32_t counts[SO_OCTAVES + 1], Want w)
{
    const Tiers t = so_tiers(counts);
    expect_eq("listed", line, t.listed, w.listed), expect_eq("n_long", line, t.n_long, w.n_long), expect_eq("n_mid", line, t.n_mid, w.n_mid);
    expect_eq("n_wave", line, t.n_wave, w.n_wave), expect_eq("n_small", line, t.n_small, w.n_small);
    expect_eq("keys_in_memory", line, t.keys_in_memory, counts[SO_OCTAVES] != 0), expect_eq("the flag, as counted", line, t.cursor[SO_OCTAVES], counts[SO_OCTAVES]);
    long long before = 0;      // the cursors: the rows of the octaves before
    for (int o = 0; o < SO_OCTAVES; o++) {
        expect_eq("cursor", line, t.cursor[o], before);
        before += counts[o];
    }
}

// counts with n rows of [2^k, 2^(k + 1)) products: octave 63 - k
static void put(int32_t counts[SO_OCTAVES + 1], int k, int32_t n) { counts[63 - k] = n; }

static void tier_cases()
{
    int32_t none[SO_OCTAVES + 1] = {};
    expect_tiers(__LINE__, none, {0, 0, 0, 0, 0});
    none[SO_OCTAVES] = 1;      // (the flag alone lists nothing)
    expect_tiers(__LINE__, none, {0, 0, 0, 0, 0});
    done("tiers: no row");

    // a row in each of the octaves 2^5, 2^6 ... 2^13 and 2^63: 12, 13 and 63 are long, 10 and 11 mid, 8 and 9 a wavefront
    // each, the others sixteen lanes (the kernel lists no row below 2^6 products; the split leaves it with the last tier)
    int32_t each[SO_OCTAVES + 1] = {};
    for (int k = 5; k <= 13; k++) put(each, k, 1);
    put(each, 63, 1);
    expect_tiers(__LINE__, each, {10, 3, 2, 2, 3});
    const Tiers t = so_tiers(each);
    EXPECT_EQ(t.cursor[0], 0), EXPECT_EQ(t.cursor[1], 1), EXPECT_EQ(t.cursor[49], 1), EXPECT_EQ(t.cursor[50], 1), EXPECT_EQ(t.cursor[51], 2);
    EXPECT_EQ(t.cursor[52], 3), EXPECT_EQ(t.cursor[53], 4), EXPECT_EQ(t.cursor[54], 5), EXPECT_EQ(t.cursor[55], 6), EXPECT_EQ(t.cursor[56], 7);
    EXPECT_EQ(t.cursor[57], 8), EXPECT_EQ(t.cursor[58], 9), EXPECT_EQ(t.cursor[59], 10), EXPECT_EQ(t.cursor[63], 10), EXPECT_EQ(t.cursor[64], 0);
    // one octave at a time: the tier of its rows
    const struct {
        int k;
        Want w;
    } alone[] = {{63, {1, 1, 0, 0, 0}}, {32, {1, 1, 0, 0, 0}}, {13, {1, 1, 0, 0, 0}}, {12, {1, 1, 0, 0, 0}}, {11, {1, 0, 1, 0, 0}}, {10, {1, 0, 1, 0, 0}},
                 {9, {1, 0, 0, 1, 0}},  {8, {1, 0, 0, 1, 0}},  {7, {1, 0, 0, 0, 1}},  {6, {1, 0, 0, 0, 1}},  {5, {1, 0, 0, 0, 1}},  {0, {1, 0, 0, 0, 1}}};
    for (const auto &a : alone) {
        int32_t c[SO_OCTAVES + 1] = {};
        put(c, a.k, 1);
        expect_tiers(__LINE__, c, a.w);
    }
    done("tiers: a row in every octave");

    // prefix sums that land on every boundary: 7 rows of 2^12, 5 of 2^11, none of 2^10, 3 of 2^9, none of 2^8 and 2^7, 2 of 2^6
    int32_t edge[SO_OCTAVES + 1] = {};
    put(edge, 12, 7), put(edge, 11, 5), put(edge, 9, 3), put(edge, 6, 2);
    expect_tiers(__LINE__, edge, {17, 7, 5, 3, 2});
    edge[SO_OCTAVES] = 1;
    expect_tiers(__LINE__, edge, {17, 7, 5, 3, 2});
    EXPECT_EQ(so_tiers(edge).keys_in_memory, 1), EXPECT_EQ(so_tiers(edge).cursor[SO_OCTAVES], 1);
    edge[SO_OCTAVES] = 0;
    EXPECT_EQ(so_tiers(edge).keys_in_memory, 0), EXPECT_EQ(so_tiers(edge).cursor[SO_OCTAVES], 0);
    put(edge, 12, 0), put(edge, 10, 4), put(edge, 8, 6), put(edge, 7, 9);      // no long row: 5 + 4 mid, 3 + 6 a wavefront, 9 + 2 small
    expect_tiers(__LINE__, edge, {29, 0, 9, 9, 11});
    // 2^31 - 1 rows, the most a matrix has: 2^30 long and 2^30 - 1 of 2^10 products
    int32_t most[SO_OCTAVES + 1] = {};
    put(most, 20, 1 << 30), put(most, 10, (1 << 30) - 1);
    expect_tiers(__LINE__, most, {INT32_MAX, 1 << 30, (1 << 30) - 1, 0, 0});
    EXPECT_EQ(so_tiers(most).cursor[63], INT32_MAX), EXPECT_EQ(so_tiers(most).cursor[53], 1 << 30);
    put(most, 20, 0), put(most, 10, 0), put(most, 6, INT32_MAX);
    expect_tiers(__LINE__, most, {INT32_MAX, 0, 0, 0, INT32_MAX});
    done("tiers: the boundaries, the flag, 2^31 - 1 rows");
}

static void call_cases()
{
    // a wavefront per row of A from 32 entries a row on, the quotient rounded down
    EXPECT_EQ(wave_per_row(31, 1), 0), EXPECT_EQ(wave_per_row(32, 1), 1), EXPECT_EQ(wave_per_row(33, 1), 1);
    EXPECT_EQ(wave_per_row(319, 10), 0), EXPECT_EQ(wave_per_row(320, 10), 1), EXPECT_EQ(wave_per_row(330, 10), 1), EXPECT_EQ(wave_per_row(0, 7), 0);
    EXPECT_EQ(wave_per_row(32ll * INT32_MAX - 1, INT32_MAX), 0), EXPECT_EQ(wave_per_row(32ll * INT32_MAX, INT32_MAX), 1);
    // the product kernels' count: a_nrows + 1 int64
    const char some = 0;
    EXPECT_EQ(products_counted(&some, 88, 10), 1), EXPECT_EQ(products_counted(&some, 87, 10), 0), EXPECT_EQ(products_counted(&some, 1 << 20, 10), 1);
    EXPECT_EQ(products_counted(nullptr, 88, 10), 0), EXPECT_EQ(products_counted(nullptr, 0, 0), 0), EXPECT_EQ(products_counted(&some, 8, 0), 1);
    EXPECT_EQ(products_counted(&some, 7, 0), 0);
    // in order already: at most one entry, no row, or an A without entries
    EXPECT_EQ(nothing_to_order(0, 5, 5), 1), EXPECT_EQ(nothing_to_order(1, 5, 5), 1), EXPECT_EQ(nothing_to_order(2, 5, 5), 0);
    EXPECT_EQ(nothing_to_order(2, 0, 5), 1), EXPECT_EQ(nothing_to_order(2, 1, 5), 0), EXPECT_EQ(nothing_to_order(2, 5, 0), 1), EXPECT_EQ(nothing_to_order(2, 5, 1), 0);
    EXPECT_EQ(nothing_to_order(1ll << 40, INT32_MAX, 1ll << 40), 0);
    done("what the call starts from");

    // 256 threads a workgroup: a thread per row; sixteen lanes per row; a wavefront per row
    const struct {
        int32_t n;
        unsigned rows, sixteen, wave;
    } g[] = {{1, 1, 1, 1},       {4, 1, 1, 1},       {5, 1, 1, 2},   {16, 1, 1, 4},  {17, 1, 2, 5},
             {256, 1, 16, 64},   {257, 2, 17, 65},   {INT32_MAX, 8388608u, 134217728u, 536870912u}};
    for (const auto &c : g) {
        EXPECT_EQ(grid_rows(c.n), c.rows), EXPECT_EQ(list_grid(c.n), c.rows);
        EXPECT_EQ(grid_lanes(c.n, 16), c.sixteen), EXPECT_EQ(least_grid(c.n), c.sixteen), EXPECT_EQ(small_grid(c.n), c.sixteen), EXPECT_EQ(products_grid(c.n, false), c.sixteen);
        EXPECT_EQ(grid_lanes(c.n, 64), c.wave), EXPECT_EQ(wave_grid(c.n), c.wave), EXPECT_EQ(products_grid(c.n, true), c.wave);
    }
    done("the grids");

    EXPECT_EQ(tp_bytes(0), 8), EXPECT_EQ(tp_bytes(10), 88), EXPECT_EQ(tp_bytes(INT32_MAX - 1), 17179869176ll);
    EXPECT_EQ(flag_bytes(), 4), EXPECT_EQ(cursor_bytes(), 260);
    EXPECT_EQ(rows_bytes(0), 4), EXPECT_EQ(rows_bytes(10), 44), EXPECT_EQ(rows_bytes(INT32_MAX), 8589934592ll);      // 4 * 2^31
    EXPECT_EQ(oci_bytes(3), 12), EXPECT_EQ(ovs_bytes(3), 24), EXPECT_EQ(key_bytes(3), 24);
    EXPECT_EQ(oci_bytes(1ll << 33), 1ll << 35), EXPECT_EQ(ovs_bytes(1ll << 33), 1ll << 36), EXPECT_EQ(key_bytes(1ll << 33), 1ll << 36);      // (beyond 2^31 entries: 64-bit sizes)
    done("the byte sizes");

    EXPECT_EQ(order_from_knob(nullptr), 1), EXPECT_EQ(order_from_knob(""), 1), EXPECT_EQ(order_from_knob("a"), 0), EXPECT_EQ(order_from_knob("A"), 0);
    EXPECT_EQ(order_from_knob("0"), 0), EXPECT_EQ(order_from_knob("ascending"), 0), EXPECT_EQ(order_from_knob("reference"), 1), EXPECT_EQ(order_from_knob("1"), 1);
    EXPECT_EQ(order_from_knob("Ascending"), 0), EXPECT_EQ(order_from_knob(" ascending"), 1), EXPECT_EQ(order_from_knob("00"), 0);
    done("the knob");
}

static int edge_mode()
{
    constant_cases();
    lds_cases();
    tier_cases();
    call_cases();
    printf(failures ? "%d checks failed\n" : "all cases passed\n", failures);
    return failures ? 1 : 0;
}

static int case_mode(int argc, char **argv)
{
    if (argc != 5) return 2;
    const long long lds_max = atoll(argv[2]), ncols = atoll(argv[3]), b_nnz = atoll(argv[4]);
    if (lds_max < 0 || lds_max > INT32_MAX || ncols < 0 || ncols > INT32_MAX || b_nnz < 0) return 2;
    const LdsPlan p = so_lds_plan((int)lds_max, (int32_t)ncols, b_nnz);
    int32_t counts[SO_OCTAVES + 1] = {};
    long long u, entries;
    while (scanf("%lld %lld", &u, &entries) == 2) {
        if (u < SO_LEAST) continue;
        counts[__builtin_clzll((unsigned long long)u)]++;
        if (u >= P32 || entries > p.cap_long) counts[SO_OCTAVES] = 1;
    }
    const Tiers t = so_tiers(counts);
    printf("constants %d %d %d %d %d %d %d %d\n", SO_LEAST, SO_TINY, SO_WAVE, SO_MID, SO_WIN, SO_LDS_BYTES, SO_TABLES_BYTES, SO_WIN_ENTRY);
    printf("lds %lld %lld %d %d %d %d %zu %d %d %zu %zu %d\n", (long long)p.budget, (long long)p.by_col, p.win_cols, (int)p.cols_mode, p.win_long,
           p.cap_long, p.lds_long, p.win_mid, p.cap_mid, p.lds_mid, p.lds_place, (int)p.ok);
    printf("tiers %d %d %d %d %d %d\n", t.listed, t.n_long, t.n_mid, t.n_wave, t.n_small, (int)t.keys_in_memory);
    printf("cursors");
    for (int o = 0; o <= SO_OCTAVES; o++) printf(" %d", t.cursor[o]);
    printf("\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && strcmp(argv[1], "case") == 0) return case_mode(argc, argv);
    return edge_mode();
}
