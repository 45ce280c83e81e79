// Host check of csr_amd/csrc/spmm_plan.h, built by tests/test_spmm_plan_host.py with the system compiler and
// -fsanitize=address,undefined.  Two modes.
//   (no argument)  every function of the header at its edges, the expected values worked out by hand from the rule's
//                  statement; the constants are pinned first, so that a changed constant shows here and not as a shifted edge.
//   case           one matrix on stdin -- "ncols k n_cus cus.." / the four knob strings ("-" = unset, else "=" + value) /
//                  "nrows nnz" / row pointers / column indices -- taken through the header's functions in the builder's
//                  order (spmm_dense.hip: build_hrows, build_mm_plan), the tile totals formed the plain way on the host;
//                  per CU count it prints the nine statistics, R, the range table, the heavy rows and their places, which
//                  the Python test compares with tests/spmm_cases.py's NumPy statement of the same plan.
#include "spmm_plan.h"

#include <cstdio>
#include <cstring>
#include <string>

using namespace csrk;
using namespace csrk::spmmplan;

static int failures = 0;
static int case_failures = 0;

static void expect_eq(const char *what, int line, long long got, long long want)
{
    if (got == want) return;
    printf("FAIL %s:%d: %s = %lld, want %lld\n", __FILE__, line, what, got, want);
    case_failures++;
}
#define EXPECT_EQ(expr, want) expect_eq(#expr, __LINE__, (long long)(expr), (long long)(want))

template <class T> static void expect_list(const char *what, int line, const std::vector<T> &got, std::vector<long long> want)
{
    bool same = got.size() == want.size();
    for (size_t i = 0; same && i < got.size(); i++) same = (long long)got[i] == want[i];
    if (same) return;
    printf("FAIL %s:%d: %s =", __FILE__, line, what);
    for (const T &v : got) printf(" %lld", (long long)v);
    printf(", want");
    for (long long v : want) printf(" %lld", v);
    printf("\n");
    case_failures++;
}
#define EXPECT_LIST(expr, ...) expect_list(#expr, __LINE__, (expr), {__VA_ARGS__})

static void done(const char *name)
{
    printf("%s %s\n", case_failures ? "FAIL" : "ok  ", name);
    failures += case_failures;
    case_failures = 0;
}

static SpmmKnobs knobs_of(const char *heavy, const char *groups, const char *trace = nullptr, const char *dense = nullptr)
{
    return parse_spmm_knobs(SpmmKnobStrings{heavy, groups, trace, dense});
}

// `n` rows of length `len`, appended
static void rows_of(std::vector<int64_t> &v, size_t n, int64_t len) { v.insert(v.end(), n, len); }
// lengths hi, hi - 1, .., lo, appended
static void descending(std::vector<int64_t> &v, int64_t hi, int64_t lo)
{
    for (int64_t x = hi; x >= lo; x--) v.push_back(x);
}

static void knob_cases()
{
    SpmmKnobs k = knobs_of(nullptr, nullptr);      // unset: the defaults
    EXPECT_EQ(k.never, 0), EXPECT_EQ(k.force, 0), EXPECT_EQ(k.groups, 0), EXPECT_EQ(k.trace, 0), EXPECT_EQ(k.dense_b, 1);
    k = knobs_of("", "", "", "");                  // empty: as unset, but CSRK_PLAN_TRACE is set
    EXPECT_EQ(k.never, 0), EXPECT_EQ(k.force, 0), EXPECT_EQ(k.groups, 0), EXPECT_EQ(k.trace, 1), EXPECT_EQ(k.dense_b, 1);
    k = knobs_of("0", "0", "0", "0");
    EXPECT_EQ(k.never, 1), EXPECT_EQ(k.force, 0), EXPECT_EQ(k.groups, 0), EXPECT_EQ(k.trace, 1), EXPECT_EQ(k.dense_b, 0);
    k = knobs_of("1", "1", "1", "1");
    EXPECT_EQ(k.never, 0), EXPECT_EQ(k.force, 1), EXPECT_EQ(k.groups, 1), EXPECT_EQ(k.trace, 1), EXPECT_EQ(k.dense_b, 1);
    k = knobs_of("2", "2", nullptr, "2");          // neither '0' nor '1'
    EXPECT_EQ(k.never, 0), EXPECT_EQ(k.force, 0), EXPECT_EQ(k.groups, 2), EXPECT_EQ(k.dense_b, 1);
    k = knobs_of("01", "8", nullptr, "01");        // the first character decides
    EXPECT_EQ(k.never, 1), EXPECT_EQ(k.force, 0), EXPECT_EQ(k.groups, 8), EXPECT_EQ(k.dense_b, 0);
    k = knobs_of("10", "2x", nullptr, "10");
    EXPECT_EQ(k.never, 0), EXPECT_EQ(k.force, 1), EXPECT_EQ(k.groups, 2), EXPECT_EQ(k.dense_b, 1);
    EXPECT_EQ(knobs_of(nullptr, "-1").groups, 0);  // negative counts: unset
    EXPECT_EQ(knobs_of(nullptr, "-3").groups, 0);
    EXPECT_EQ(knobs_of(nullptr, "x").groups, 0);
    done("the knob parser");
}

static void choice_cases()
{
    const SpmmKnobs unset = knobs_of(nullptr, nullptr), forced = knobs_of("1", nullptr), never = knobs_of("0", nullptr);
    // B is ncols * k * 8 bytes: 2^17 * 64 * 8 = 2^23 * 1 * 8 = 64 MiB exactly is not above; the next size is (8 bytes a value)
    EXPECT_EQ(heavy_engaged(131072, 64, unset), 0);
    EXPECT_EQ(heavy_engaged(131073, 64, unset), 1);
    EXPECT_EQ(heavy_engaged(8388608, 1, unset), 0);       // 67108864 bytes
    EXPECT_EQ(heavy_engaged(8388609, 1, unset), 1);       // 67108872
    EXPECT_EQ(heavy_engaged(1, 1, forced), 1);
    EXPECT_EQ(heavy_engaged(8388609, 1, never), 0);
    EXPECT_EQ(heavy_engaged(2000000, 64, unset), 1);      // BASELINE configs[2]
    EXPECT_EQ(has_entries(1, 1, 1), 1), EXPECT_EQ(has_entries(0, 1, 1), 0), EXPECT_EQ(has_entries(1, 0, 1), 0), EXPECT_EQ(has_entries(1, 1, 0), 0);
    done("engage at 64 MiB");

    // the floor: 512 entries, 256 when forced; longest first, then by row id
    EXPECT_LIST(candidates({600, 700, 600, 100, 512, 511}, false), 1, 0, 2, 4);
    EXPECT_LIST(candidates({256, 255, 300, 256}, true), 2, 0, 3);
    EXPECT_LIST(candidates({511, 0}, false));
    done("candidates");

    // 4 gn >= 5 ncols: ncols = 131076 -> 655380 = 4 * 163845 (tests/spmm_cases.py: PAYS)
    EXPECT_EQ(group_pays(163845, 131076), 1);
    EXPECT_EQ(group_pays(163844, 131076), 0);
    EXPECT_EQ(group_pays(0, 0), 1);
    {   // through the loop: 163 rows of 1000 and one of 845 / 844 entries
        std::vector<int64_t> len;
        rows_of(len, 163, 1000);
        len.push_back(845);
        Groups g = choose_groups(len, candidates(len, false), 131076, unset);
        EXPECT_EQ(g.G, 1), EXPECT_EQ(g.taken, 164), EXPECT_EQ(g.tried.size(), 1), EXPECT_EQ(g.tried[0].entries, 163845), EXPECT_EQ(g.tried[0].pays, 1);
        EXPECT_EQ(g.tried[0].longest, 1000), EXPECT_EQ(g.tried[0].shortest, 845), EXPECT_EQ(g.tried[0].first, 0), EXPECT_EQ(g.tried[0].end, 164);
        len.back() = 844;
        g = choose_groups(len, candidates(len, false), 131076, unset);
        EXPECT_EQ(g.G, 0), EXPECT_EQ(g.taken, 0), EXPECT_EQ(g.tried.size(), 1), EXPECT_EQ(g.tried[0].entries, 163844), EXPECT_EQ(g.tried[0].pays, 0);
    }
    done("the pays rule");

    {   // 600 rows of 300 entries under a million columns: no group pays; forced, the first one is taken all the same
        std::vector<int64_t> len;
        rows_of(len, 600, 300);
        const std::vector<int32_t> cand = candidates(len, true);
        Groups g = choose_groups(len, cand, 1000000, forced);
        EXPECT_EQ(g.G, 1), EXPECT_EQ(g.taken, 512), EXPECT_EQ(g.tried.size(), 2);
        EXPECT_EQ(g.tried[0].pays, 0), EXPECT_EQ(g.tried[0].entries, 153600);
        EXPECT_EQ(g.tried[1].first, 512), EXPECT_EQ(g.tried[1].end, 600), EXPECT_EQ(g.tried[1].entries, 26400), EXPECT_EQ(g.tried[1].pays, 0);
        g = choose_groups(len, cand, 1000000, unset);      // (the same candidates, not forced)
        EXPECT_EQ(g.G, 0), EXPECT_EQ(g.taken, 0), EXPECT_EQ(g.tried.size(), 1);
        g = choose_groups(len, cand, 100, unset);          // both groups pay: the loop ends with the candidates
        EXPECT_EQ(g.G, 2), EXPECT_EQ(g.taken, 600), EXPECT_EQ(g.tried.size(), 2);
    }
    done("the forced first group");

    {   // CSRK_SPMM_HEAVY_GROUPS: that many groups whether they pay or not, or as many as there are candidates for
        std::vector<int64_t> len;
        rows_of(len, 520, 300);
        const std::vector<int32_t> cand = candidates(len, true);
        Groups g = choose_groups(len, cand, 1000000, knobs_of("1", "4"));
        EXPECT_EQ(g.G, 2), EXPECT_EQ(g.taken, 520), EXPECT_EQ(g.tried.size(), 2);
        g = choose_groups(len, cand, 1000000, knobs_of("1", "2"));
        EXPECT_EQ(g.G, 2), EXPECT_EQ(g.taken, 520), EXPECT_EQ(g.tried.size(), 2);
        g = choose_groups(len, cand, 1000000, knobs_of("1", "1"));      // the second group is looked at, and is where the loop stops
        EXPECT_EQ(g.G, 1), EXPECT_EQ(g.taken, 512), EXPECT_EQ(g.tried.size(), 2), EXPECT_EQ(g.tried[1].first, 512), EXPECT_EQ(g.tried[1].end, 520);
        g = choose_groups(len, cand, 100, knobs_of(nullptr, "1"));      // (both would pay)
        EXPECT_EQ(g.G, 1), EXPECT_EQ(g.taken, 512);
        rows_of(len, 8 * 512 + 5 - 520, 300);                            // candidates for more than HR_MAXG groups
        g = choose_groups(len, candidates(len, true), 1000000, knobs_of("1", "9"));
        EXPECT_EQ(g.G, 8), EXPECT_EQ(g.taken, 4096), EXPECT_EQ(g.tried.size(), 8);
    }
    done("HEAVY_GROUPS larger than the candidates allow");
}

static void threshold_cases()
{
    // lengths in rank order, so that candidate i is row i: 505 distinct ones 900 .. 396, then ties at 300 across the edge of
    // the one group (512 rows)
    std::vector<int64_t> len;
    descending(len, 900, 396);
    rows_of(len, 7, 300);
    descending(len, 299, 256);
    std::vector<int32_t> cand = candidates(len, true);
    Threshold t = threshold(len, cand, 512, 1);      // the 7 rows of 300 end the group exactly: they fit
    EXPECT_EQ(t.on, 1), EXPECT_EQ(t.moved, 0), EXPECT_EQ(t.hmin, 300), EXPECT_EQ(t.n, 512);
    t = threshold(len, cand, 511, 1);                // one of them not taken yet: it comes along
    EXPECT_EQ(t.on, 1), EXPECT_EQ(t.moved, 0), EXPECT_EQ(t.hmin, 300), EXPECT_EQ(t.n, 512);
    done("ties that fit");

    len.clear();
    descending(len, 900, 396);
    rows_of(len, 16, 300);                           // 521 rows of at least 300 entries: one group cannot hold them
    cand = candidates(len, true);
    t = threshold(len, cand, 512, 1);
    EXPECT_EQ(t.on, 1), EXPECT_EQ(t.moved, 1), EXPECT_EQ(t.hmin, 301), EXPECT_EQ(t.n, 505);
    t = threshold(len, cand, 521, 2);                // two groups hold them
    EXPECT_EQ(t.on, 1), EXPECT_EQ(t.moved, 0), EXPECT_EQ(t.hmin, 300), EXPECT_EQ(t.n, 521);
    done("ties that move the threshold");

    len.clear();
    rows_of(len, 600, 300);                          // every candidate as long as the last one taken: none is left
    cand = candidates(len, true);
    t = threshold(len, cand, 512, 1);
    EXPECT_EQ(t.on, 0), EXPECT_EQ(t.moved, 1), EXPECT_EQ(t.hmin, 301), EXPECT_EQ(t.n, 0);
    len.assign(1, 2147483647ll);                     // the threshold is an int32 on the device
    t = threshold(len, candidates(len, true), 1, 1);
    EXPECT_EQ(t.on, 1), EXPECT_EQ(t.hmin, 2147483647ll), EXPECT_EQ(t.n, 1);
    len.assign(1, 2147483648ll);
    t = threshold(len, candidates(len, true), 1, 1);
    EXPECT_EQ(t.on, 0), EXPECT_EQ(t.moved, 0), EXPECT_EQ(t.n, 1);
    done("ties that switch the form off");

    EXPECT_EQ(shrink_groups(3, 400), 1);             // places:shrink of tests/spmm_cases.py in small
    EXPECT_EQ(shrink_groups(3, 512), 1);
    EXPECT_EQ(shrink_groups(3, 513), 2);
    EXPECT_EQ(shrink_groups(3, 1024), 2);
    EXPECT_EQ(shrink_groups(3, 1025), 3);
    EXPECT_EQ(shrink_groups(1, 1), 1);
    EXPECT_EQ(shrink_groups(8, 1), 1);
    done("shrink from 3 groups to 1");
}

static void size_cases()
{
    EXPECT_EQ(tiles_of(1), 1), EXPECT_EQ(tiles_of(128), 1), EXPECT_EQ(tiles_of(129), 2), EXPECT_EQ(tiles_of(2147483647), 16777216);
    done("n_tiles");

    EXPECT_EQ(ranges_for(2, 3, 100), 1);             // cus < G: one range, G workgroups
    EXPECT_EQ(ranges_for(0, 1, 100), 1);
    EXPECT_EQ(ranges_for(7, 8, 100), 1);
    EXPECT_EQ(ranges_for(8, 8, 100), 1);
    EXPECT_EQ(ranges_for(16, 8, 100), 2);
    done("R at cus < G");
    EXPECT_EQ(ranges_for(256, 1, 7), 7);             // a range needs a tile; from 8 on a multiple of 8
    EXPECT_EQ(ranges_for(256, 1, 8), 8);
    EXPECT_EQ(ranges_for(256, 1, 9), 8);
    EXPECT_EQ(ranges_for(256, 1, 15), 8);
    EXPECT_EQ(ranges_for(256, 1, 16), 16);
    EXPECT_EQ(ranges_for(256, 1, 1000), 256);
    EXPECT_EQ(ranges_for(256, 3, 1000), 80);         // 85 -> 80
    EXPECT_EQ(ranges_for(7, 1, 1000), 7);
    EXPECT_EQ(ranges_for(20, 1, 1000), 16);
    EXPECT_EQ(ranges_for(304, 2, 1000), 152);
    done("R at 7, 8, 9, 15, 16 tiles");

    EXPECT_EQ(buckets_of(23, 2), 736);               // 23 tiles x 2 groups x 16 wavefronts
    EXPECT_EQ(buckets_of(67108864, 1), 1073741824);  // 2^26 tiles: 2^30 buckets
    EXPECT_EQ(bucket_keys_fit(1073741823), 1);       // 2^30 - 1
    EXPECT_EQ(bucket_keys_fit(1073741824), 0);       // 2^30
    EXPECT_EQ(bucket_keys_fit(buckets_of(67108863, 1)), 1);
    EXPECT_EQ(bucket_keys_fit(buckets_of(67108864, 1)), 0);
    EXPECT_EQ(bucket_keys_fit(buckets_of(16777216, 8)), 0);      // every int32 column count at 8 groups: 2^31
    done("the bucket limit at 2^30");

    EXPECT_EQ(table_pays(3, 2, false), 1);           // 24 bytes of table against 24 of stream: not heavier
    EXPECT_EQ(table_pays(3, 1, false), 0);           // 24 > 12
    EXPECT_EQ(table_pays(16, 11, false), 1);         // 128 <= 132
    EXPECT_EQ(table_pays(16, 10, false), 0);         // 128 > 120
    EXPECT_EQ(table_pays(16, 10, true), 1);          // forced: not asked
    done("8 n_buckets against 12 nnz_h");

    // 1000 entries x 40 B + 16 buckets x 8 B + 64 MiB = 40000 + 128 + 67108864 = 67148992
    EXPECT_EQ(build_fits_memory(1000, 16, 67148992), 1);
    EXPECT_EQ(build_fits_memory(1000, 16, 67148991), 0);
    EXPECT_EQ(build_fits_memory(0, 0, 67108864), 1);
    EXPECT_EQ(build_fits_memory(0, 0, 67108863), 0);
    EXPECT_EQ(build_fits_memory(50000000, 500000, (size_t)3 << 30), 1);      // 2.07e9 bytes
    EXPECT_EQ(build_fits_memory(50000000, 500000, (size_t)1 << 30), 0);
    done("the free-memory refusal");
}

static void place_cases()
{
    const int G = 3;      // rank i: group i % 3, wavefront (i / 3) % 16, slot (i / 3) / 16; code = group << 9 | wavefront << 5 | slot
    EXPECT_EQ(place_code(0, G), 0);
    EXPECT_EQ(place_code(G - 1, G), 2 << 9);
    EXPECT_EQ(place_code(G, G), 1 << 5);
    EXPECT_EQ(place_code(16 * G - 1, G), (2 << 9) | (15 << 5));
    EXPECT_EQ(place_code(16 * G, G), 1);
    EXPECT_EQ(place_code(512 * G - 1, G), (2 << 9) | (15 << 5) | 31);
    EXPECT_EQ(place_code(512 * G - 1, G), 1535);
    EXPECT_EQ(place_code(511, 1), 511), EXPECT_EQ(place_code(17, 1), (1 << 5) | 1);
    EXPECT_EQ(place_code(4095, 8), 4095);            // the last of 8 groups of 512
    EXPECT_LIST(place_codes(5, 2), 0, 512, 32, 544, 64);
    EXPECT_LIST(place_codes(0, 1));
    for (size_t i : {(size_t)0, (size_t)2, (size_t)3, (size_t)47, (size_t)48, (size_t)1535}) {
        const Place p = place_of(place_code(i, G));
        EXPECT_EQ(p.group, i % 3), EXPECT_EQ(p.wave, (i / 3) % 16), EXPECT_EQ(p.slot, (i / 3) / 16);
        EXPECT_EQ((p.group * 512 + p.wave * 32 + p.slot), (int)(i % 3) * 512 + (int)((i / 3) % 16) * 32 + (int)(i / 48));
    }
    done("place codes");

    const std::vector<int64_t> len = {5, 0, 7, 3};
    EXPECT_LIST(entry_offsets(len, {2, 0, 3}), 0, 7, 12, 15);
    EXPECT_LIST(entry_offsets(len, {1}), 0, 0);
    EXPECT_EQ(entries_of(len, {2, 0, 3}), 15);
    EXPECT_EQ(entries_of(len, {}), 0);
    done("entry offsets");
}

static void range_cases()
{
    // tot[t] = heavy entries before tile t; cost of tiles 0 .. t = tot[t + 1] + 200 G (t + 1); goal of range q = q / R of the total
    // G = 2, 4 tiles of 100 entries: total 400 + 400 * 4 = 2000, goal 1000 = the cost of tiles 0 .. 1 exactly (<=): range 1 starts at tile 2
    EXPECT_LIST(balance_ranges({0, 100, 200, 300, 400}, 4, 2, 2, 400), 0, 2, 4);
    // one entry fewer in tile 1 and the total is 1999, the goal 999.5 and tiles 0 .. 1 cost 999: still 2; one more in tile 0: 1001 > 1000.5
    EXPECT_LIST(balance_ranges({0, 100, 199, 299, 399}, 4, 2, 2, 399), 0, 2, 4);
    EXPECT_LIST(balance_ranges({0, 102, 202, 302, 401}, 4, 2, 2, 401), 0, 1, 4);
    EXPECT_LIST(balance_ranges({0, 100, 200, 300, 400}, 4, 2, 1, 400), 0, 4);
    done("balance_ranges at a goal met exactly");
    // everything in the first of 10 tiles, G = 1: total 100000 + 2000, goals 25500, 51000, 76500, tile 0 alone costs 100200:
    // the search stays at tile 0 and every range takes the one tile the clamp from below gives it
    EXPECT_LIST(balance_ranges({0, 100000, 100000, 100000, 100000, 100000, 100000, 100000, 100000, 100000, 100000}, 10, 1, 4, 100000), 0, 1, 2, 3, 10);
    done("balance_ranges: the clamp low");
    // everything in the last tile: tiles 0 .. 8 cost 1800, under the first goal: the search runs to tile 9 and the clamp from
    // above leaves a tile to each range after it: 10 - 3, 10 - 2, 10 - 1
    EXPECT_LIST(balance_ranges({0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 100000}, 10, 1, 4, 100000), 0, 7, 8, 9, 10);
    done("balance_ranges: the clamp high");
    // as many ranges as tiles: a tile each, whatever the weights (both clamps meet)
    EXPECT_LIST(balance_ranges({0, 10, 10, 10}, 3, 1, 3, 10), 0, 1, 2, 3);
    EXPECT_LIST(balance_ranges({0, 0, 0, 10}, 3, 1, 3, 10), 0, 1, 2, 3);
    EXPECT_LIST(balance_ranges({0, 7}, 1, 8, 1, 7), 0, 1);
    done("balance_ranges with R == n_tiles");
}

static void light_cases()
{
    EXPECT_EQ(light_segments(0, 0), 1);              // an empty row has a segment: it stores the row's zeros
    EXPECT_EQ(light_segments(1, 0), 1);
    EXPECT_EQ(light_segments(64, 0), 1);
    EXPECT_EQ(light_segments(65, 0), 2);
    EXPECT_EQ(light_segments(128, 0), 2);
    EXPECT_EQ(light_segments(129, 0), 3);
    EXPECT_EQ(light_segments(299, 300), 5);          // below heavy_min: ceil(299 / 64)
    EXPECT_EQ(light_segments(300, 300), 0);          // at it: the heavy kernels' row
    EXPECT_EQ(light_segments(301, 300), 0);
    EXPECT_EQ(light_segments(300, 0), 5);            // heavy_min = 0: no heavy rows
    EXPECT_EQ(light_segments(0, 1), 1), EXPECT_EQ(light_segments(1, 1), 0);
    static_assert(light_segments(65, 0) == 2, "light_segments is a constant expression");
    done("light_segments");
}

static void launch_cases()
{
    alignas(16) static double buf[4];
    const void *p0 = buf, *p8 = buf + 1;             // 0 and 8 mod 16
    EXPECT_EQ(aligned16(p0, 4), 1), EXPECT_EQ(aligned16(p0, 5), 0), EXPECT_EQ(aligned16(p8, 4), 0), EXPECT_EQ(aligned16(p8, 5), 0);
    EXPECT_EQ(aligned16(p0, 0), 1), EXPECT_EQ(aligned16(buf + 2, 66), 1);
    EXPECT_EQ(aligned16((const char *)p0 + 1, 4), 0), EXPECT_EQ(aligned16((const char *)p0 + 4, 4), 0);      // (every low bit counts)
    for (int k = 1; k <= 9; k++) {
        EXPECT_EQ(full4(k, true, true), k == 4 || k == 8);
        EXPECT_EQ(full4(k, false, true), 0), EXPECT_EQ(full4(k, true, false), 0);
        EXPECT_EQ(hrows_even(k, true), k % 2 == 0), EXPECT_EQ(hrows_even(k, false), 0);
    }
    EXPECT_EQ(full4(64, aligned16(p0, 64), aligned16(p0, 64)), 1);
    EXPECT_EQ(full4(64, aligned16(p0, 65), aligned16(p0, 64)), 0);      // an odd ldb
    EXPECT_EQ(full4(64, aligned16(p0, 64), aligned16(p8, 64)), 0);      // C at 8 mod 16
    EXPECT_EQ(hrows_even(64, aligned16(p8, 64)), 0), EXPECT_EQ(hrows_even(63, aligned16(p0, 64)), 0), EXPECT_EQ(hrows_even(64, aligned16(p0, 64)), 1);
    done("full4 and hrows_even");

    EXPECT_EQ(col_blocks(1), 1), EXPECT_EQ(col_block(1, 0).c0, 0), EXPECT_EQ(col_block(1, 0).kc, 1);
    EXPECT_EQ(col_blocks(64), 1), EXPECT_EQ(col_block(64, 0).kc, 64);
    EXPECT_EQ(col_blocks(65), 2), EXPECT_EQ(col_block(65, 0).kc, 64), EXPECT_EQ(col_block(65, 1).c0, 64), EXPECT_EQ(col_block(65, 1).kc, 1);
    EXPECT_EQ(col_blocks(128), 2), EXPECT_EQ(col_block(128, 1).c0, 64), EXPECT_EQ(col_block(128, 1).kc, 64);
    EXPECT_EQ(col_blocks(129), 3), EXPECT_EQ(col_block(129, 1).kc, 64), EXPECT_EQ(col_block(129, 2).c0, 128), EXPECT_EQ(col_block(129, 2).kc, 1);
    EXPECT_EQ(col_blocks(0), 0);
    done("column blocks");

    EXPECT_EQ(hrows_grid(2, 8), 16), EXPECT_EQ(hrows_grid(1, 256), 256);
    EXPECT_EQ(seg_grid(0), 0), EXPECT_EQ(seg_grid(1), 1), EXPECT_EQ(seg_grid(16), 1), EXPECT_EQ(seg_grid(17), 2);      // 16 segments a workgroup
    EXPECT_EQ(seg_grid(268435456), 16777216);        // 2^28 segments: 2^32 lanes
    EXPECT_EQ(reduce_grid(0), 0), EXPECT_EQ(reduce_grid(4), 1), EXPECT_EQ(reduce_grid(5), 2), EXPECT_EQ(reduce_grid(4096), 1024);      // 4 rows a workgroup
    EXPECT_EQ(fixup_grid(0), 0), EXPECT_EQ(fixup_grid(4), 1), EXPECT_EQ(fixup_grid(5), 2), EXPECT_EQ(fixup_grid(2147483647), 536870912);
    done("the three grids");

    EXPECT_EQ(grow_partials(0, 0, 5), 0);            // no split row: no buffer
    EXPECT_EQ(grow_partials(3, 0, 5), 1);
    EXPECT_EQ(grow_partials(1, 0, 5), 1);
    EXPECT_EQ(grow_partials(3, 5, 5), 0);
    EXPECT_EQ(grow_partials(3, 5, 6), 1);
    EXPECT_EQ(grow_partials(3, 6, 5), 0);            // kept when k shrinks again
    done("grow_partials");

    int64_t out[9];
    const PlanCounts off = {false, 7, 8, 9, 10, 11, 12, 13, 14}, on = {true, 7, 8, 9, 10, 11, 12, 13, 14};
    plan_stats(off, out);
    EXPECT_LIST(std::vector<int64_t>(out, out + 9), 0, 0, 0, 0, 0, 0, 0, 13, 14);
    plan_stats(on, out);
    EXPECT_LIST(std::vector<int64_t>(out, out + 9), 1, 7, 8, 9, 10, 11, 12, 13, 14);
    plan_stats(PlanCounts{}, out);
    EXPECT_LIST(std::vector<int64_t>(out, out + 9), 0, 0, 0, 0, 0, 0, 0, 0, 0);
    done("the nine stats with the heavy form off");
}

static void dense_b_cases()
{
    const SpmmKnobs on = knobs_of(nullptr, nullptr), off = knobs_of(nullptr, nullptr, nullptr, "0");
    const int NONE = 0, F32 = 1, F64 = 2;
    // A [.. x 10] with 7 entries, B [10 x 4] fully populated
    EXPECT_EQ(dense_b_gate(on, 10, 7, F64, 10, 4, 40, F64), 1);
    EXPECT_EQ(dense_b_gate(off, 10, 7, F64, 10, 4, 40, F64), 0);      // CSRK_SPGEMM_DENSE=0
    EXPECT_EQ(dense_b_gate(on, 11, 7, F64, 10, 4, 40, F64), 0);       // the shapes disagree
    EXPECT_EQ(dense_b_gate(on, 0, 7, F64, 0, 4, 0, F64), 0);          // B without rows
    EXPECT_EQ(dense_b_gate(on, 10, 7, F64, 10, 0, 0, F64), 0);        // B without columns
    EXPECT_EQ(dense_b_gate(on, 10, 0, F64, 10, 4, 40, F64), 0);       // A without entries
    EXPECT_EQ(dense_b_gate(on, 10, 7, F64, 10, 4, 39, F64), 0);       // B one entry short, or one over
    EXPECT_EQ(dense_b_gate(on, 10, 7, F64, 10, 4, 41, F64), 0);
    EXPECT_EQ(dense_b_gate(on, 10, 7, NONE, 10, 4, 40, F64), 0);      // an operand without values
    EXPECT_EQ(dense_b_gate(on, 10, 7, F64, 10, 4, 40, NONE), 0);
    EXPECT_EQ(dense_b_gate(on, 10, 7, F32, 10, 4, 40, F32), 0);       // float32 products
    EXPECT_EQ(dense_b_gate(on, 10, 7, F32, 10, 4, 40, F64), 1);
    EXPECT_EQ(dense_b_gate(on, 10, 7, F64, 10, 4, 40, F32), 1);
    EXPECT_EQ(dense_b_gate(on, 10, 7, F64, 10, 1, 10, F64), 1);       // a panel of one column; a B of one row
    EXPECT_EQ(dense_b_gate(on, 1, 7, F64, 1, 4, 4, F64), 1);
    EXPECT_EQ(dense_b_shapes(2000000, 1, 2000000, 2000, 4000000000ll), 1);      // nrows * k beyond int32
    done("the dense-B gate");

    EXPECT_EQ(dense_c_nnz(2147483647, 1), 2147483647ll), EXPECT_EQ(dense_c_overflows(2147483647ll), 0);      // INT32_MAX
    EXPECT_EQ(dense_c_overflows(dense_c_nnz(2147483647, 1)), 0);
    EXPECT_EQ(dense_c_overflows(2147483648ll), 1);
    EXPECT_EQ(dense_c_overflows(dense_c_nnz(33554432, 64)), 1);       // 2^25 rows x 64 = 2^31
    EXPECT_EQ(dense_c_overflows(dense_c_nnz(33554431, 64)), 0);       // 2^31 - 64
    EXPECT_EQ(dense_c_overflows(dense_c_nnz(2000000, 2000)), 1);      // 4e9
    EXPECT_EQ(dense_c_overflows(0), 0);
    done("c_nnz at INT32_MAX");
}

static int edge_mode()
{
    EXPECT_EQ(MM_SEG, 64), EXPECT_EQ(MM_G, 16), EXPECT_EQ(MM_CHUNK, 64);
    EXPECT_EQ(HR_LANES, 64), EXPECT_EQ(HR_THREADS, 1024), EXPECT_EQ(HR_WAVES, 16), EXPECT_EQ(HR_RPW, 32), EXPECT_EQ(HR_ROWS, 512);
    EXPECT_EQ(HR_TILE, 128), EXPECT_EQ(HR_KC, 64), EXPECT_EQ(HR_PAD, 128), EXPECT_EQ(HR_MAXG, 8), EXPECT_EQ(HR_LDS, 131072);
    EXPECT_EQ(HR_ENGAGE_BYTES, 67108864), EXPECT_EQ(HR_FLOOR, 512), EXPECT_EQ(HR_FLOOR_FORCED, 256);
    EXPECT_EQ(HR_PAYS_ENTRIES, 4), EXPECT_EQ(HR_PAYS_COLS, 5), EXPECT_EQ(HR_TILE_COST, 200), EXPECT_EQ(HR_MAX_BUCKETS, 1073741824);
    EXPECT_EQ(HR_TABLE_BYTES, 8), EXPECT_EQ(HR_STREAM_BYTES, 12);
    EXPECT_EQ(HR_BUILD_ENTRY_BYTES, 40), EXPECT_EQ(HR_BUILD_BUCKET_BYTES, 8), EXPECT_EQ(HR_BUILD_SPARE, 67108864);
    EXPECT_EQ(DB_VAL_NONE, 0), EXPECT_EQ(DB_VAL_F32, 1);
    done("constants");
    knob_cases();
    choice_cases();
    threshold_cases();
    size_cases();
    place_cases();
    range_cases();
    light_cases();
    launch_cases();
    dense_b_cases();
    {   // the steps together: two rows of 300 under 300 columns, forced, 256 CUs
        const std::vector<int64_t> len = {300, 5, 300, 0};
        HeavyChoice h = choose_heavy(len, 300, 256, knobs_of("1", nullptr));
        EXPECT_EQ(h.on, 1), EXPECT_LIST(h.rows, 0, 2), EXPECT_EQ(h.hmin, 300), EXPECT_EQ(h.nnz_h, 600), EXPECT_EQ(h.G, 1), EXPECT_EQ(h.G_taken, 1);
        EXPECT_EQ(h.n_tiles, 3), EXPECT_EQ(h.R, 3), EXPECT_EQ(h.n_buckets, 48), EXPECT_EQ(h.moved, 0), EXPECT_EQ(h.tried.size(), 1);
        h = choose_heavy(len, 300, 256, knobs_of(nullptr, nullptr));      // no row reaches 512
        EXPECT_EQ(h.on, 0), EXPECT_EQ(h.tried.size(), 0), EXPECT_EQ(h.rows.size(), 0);
        EXPECT_EQ(h.hmin, 0), EXPECT_EQ(h.nnz_h, 0), EXPECT_EQ(h.n_tiles, 0), EXPECT_EQ(h.n_buckets, 0), EXPECT_EQ(h.G_taken, 0), EXPECT_EQ(h.G, 0), EXPECT_EQ(h.R, 0);
        // not forced: 2 rows of 600 pay under 900 columns (4800 >= 4500), but 8 tiles x 16 buckets x 8 B > 1200 x 12 B is false
        // (1024 <= 14400): on; under 960 columns they no longer pay
        h = choose_heavy({600, 600}, 900, 256, knobs_of(nullptr, nullptr));
        EXPECT_EQ(h.on, 1), EXPECT_EQ(h.n_tiles, 8), EXPECT_EQ(h.R, 8), EXPECT_EQ(h.n_buckets, 128);
        h = choose_heavy({600, 600}, 961, 256, knobs_of(nullptr, nullptr));
        EXPECT_EQ(h.on, 0), EXPECT_EQ(h.tried.size(), 1);
        // one row of 1000 under 800 columns pays (4000 >= 4000); 7 tiles x 16 x 8 = 896 B of table <= 12000: on.  Under
        // CSRK_SPMM_HEAVY_GROUPS=1 a row of 600 under 200000 columns is taken without paying, and 1563 x 16 x 8 = 200064 > 7200
        // refuses the table -- unless forced
        h = choose_heavy({1000}, 800, 256, knobs_of(nullptr, nullptr));
        EXPECT_EQ(h.on, 1);
        h = choose_heavy({600}, 200000, 256, knobs_of(nullptr, "1"));
        EXPECT_EQ(h.on, 0), EXPECT_EQ(h.rows.size(), 1), EXPECT_EQ(h.n_buckets, 25008);
        h = choose_heavy({600}, 200000, 256, knobs_of("1", "1"));
        EXPECT_EQ(h.on, 1);
        done("choose_heavy");
    }
    printf(failures ? "%d FAILURES\n" : "all cases passed\n", failures);
    return failures ? 1 : 0;
}

// ---- case mode --------------------------------------------------------------------------------------------------------------
static bool read_knob(std::string &store, const char **out)
{
    char buf[256];
    if (scanf("%255s", buf) != 1) return false;
    if (buf[0] == '-') {
        *out = nullptr;
        return true;
    }
    if (buf[0] != '=') return false;
    store = buf + 1;
    *out = store.c_str();
    return true;
}

template <class T> static void print_list(const char *name, const std::vector<T> &v)
{
    printf("%s", name);
    for (const T &x : v) printf(" %lld", (long long)x);
    printf("\n");
}

static int case_mode()
{
    int ncols = 0, k = 0, n_cus = 0;
    if (scanf("%d %d %d", &ncols, &k, &n_cus) != 3 || n_cus < 1 || n_cus > 16) return 2;
    std::vector<int> cus((size_t)n_cus);
    for (int &c : cus)
        if (scanf("%d", &c) != 1) return 2;
    std::string store[4];
    SpmmKnobStrings e;
    if (!read_knob(store[0], &e.heavy) || !read_knob(store[1], &e.heavy_groups) || !read_knob(store[2], &e.plan_trace) ||
        !read_knob(store[3], &e.spgemm_dense))
        return 2;
    long long nrows = 0, nnz = 0;
    if (scanf("%lld %lld", &nrows, &nnz) != 2 || nrows < 0 || nnz < 0) return 2;
    std::vector<int64_t> rp((size_t)nrows + 1), ci((size_t)nnz);
    for (int64_t &v : rp) {
        long long x;
        if (scanf("%lld", &x) != 1) return 2;
        v = x;
    }
    for (int64_t &v : ci) {
        long long x;
        if (scanf("%lld", &x) != 1 || x < 0 || x >= ncols) return 2;
        v = x;
    }
    if (rp[0] != 0 || rp[(size_t)nrows] != nnz) return 2;
    std::vector<int64_t> len((size_t)nrows);
    for (size_t r = 0; r < len.size(); r++) {
        len[r] = rp[r + 1] - rp[r];
        if (len[r] < 0) return 2;
    }

    const SpmmKnobs knobs = parse_spmm_knobs(e);
    for (int c : cus) {
        // spmm_device, build_hrows: engage, the choice, (free memory: not asked here), places and offsets, ranges
        HeavyChoice h;
        if (heavy_engaged(ncols, k, knobs) && has_entries((int32_t)nrows, ncols, nnz)) h = choose_heavy(len, ncols, c, knobs);
        std::vector<int32_t> range, group, wave, slot;
        if (h.on) {
            const std::vector<int64_t> off = entry_offsets(len, h.rows);
            if (off.back() != h.nnz_h) return 3;
            std::vector<int64_t> tot((size_t)h.n_tiles + 1, 0);      // entries of the heavy rows with col / 128 < t
            for (int32_t r : h.rows)
                for (int64_t q = rp[(size_t)r]; q < rp[(size_t)r + 1]; q++) tot[(size_t)(ci[(size_t)q] / HR_TILE) + 1]++;
            for (size_t t = 1; t < tot.size(); t++) tot[t] += tot[t - 1];
            range = balance_ranges(tot, h.n_tiles, h.G, h.R, h.nnz_h);
            for (int32_t code : place_codes(h.rows.size(), h.G)) {
                const Place p = place_of(code);
                group.push_back(p.group), wave.push_back(p.wave), slot.push_back(p.slot);
            }
        }
        // build_mm_plan: mm_count_kernel's segments
        PlanCounts pc = {h.on, (int32_t)h.hmin, (int32_t)h.rows.size(), h.G, h.R, h.nnz_h, (int32_t)h.n_tiles, 0, 0};
        for (int64_t l : len) {
            const int64_t n = light_segments(l, h.on ? pc.hr_min : 0);
            pc.n_segs += n;
            pc.n_multi += n > 1 ? n : 0;
        }
        int64_t st[9];
        plan_stats(pc, st);
        printf("cus %d\n", c);
        print_list("stats", std::vector<int64_t>(st, st + 9));
        printf("R %d\n", h.on ? h.R : 0);
        printf("tie %s\n", !h.on ? "-" : h.moved ? "move" : "fit");
        printf("G_taken %d\n", h.on ? h.G_taken : 0);
        print_list("range", range);
        print_list("rows", h.on ? h.rows : std::vector<int32_t>());
        print_list("group", group);
        print_list("wave", wave);
        print_list("slot", slot);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && strcmp(argv[1], "case") == 0) return case_mode();
    return edge_mode();
}
