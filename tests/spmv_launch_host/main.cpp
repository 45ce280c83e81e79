// Host check of csr_amd/csrc/spmv_launch.h, built by tests/test_spmv_launch_host.py with the system compiler and
// -fsanitize=address,undefined: every decision an SpMV product takes on the host before it launches (spmv.hip, "host
// side") at its edge -- the lazy split, the algorithm and its parts, the light stream's form, tier 0's launches, the rider,
// the epilogue's jobs and their batches.  Every expected value is worked out by hand from the rule's statement.
#include "spmv_launch.h"

#include <cstdio>
#include <vector>

using namespace csrk;
using namespace csrk::spmvlaunch;

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

// the kernels' constants as spmv_plan.h has them by default
static const SpmvKnobDefaults KNOB_DEFAULTS = {2048, 128, 2, 3, 15936};
static const LsLimits LS_DEFAULTS = {15360, 8176, 8192, 8, 512};
constexpr int MERGE = 1, VECTOR = 2, SCALAR = 3;

static void split_cases()
{
    auto forced = [](const char *SpmvKnobStrings::*field, const char *v) {
        SpmvKnobStrings e;
        e.*field = v;
        return split_forced(parse_spmv_knobs(e, KNOB_DEFAULTS));
    };
    EXPECT_EQ(split_forced(parse_spmv_knobs(SpmvKnobStrings(), KNOB_DEFAULTS)), 0);
    for (const char *SpmvKnobStrings::*field : {&SpmvKnobStrings::heavy_split, &SpmvKnobStrings::hot, &SpmvKnobStrings::stream}) {
        EXPECT_EQ(forced(field, "1"), 1);
        EXPECT_EQ(forced(field, "11"), 1);      // the first character decides
        EXPECT_EQ(forced(field, "0"), 0);
        EXPECT_EQ(forced(field, ""), 0);
        EXPECT_EQ(forced(field, "2"), 0);
        EXPECT_EQ(forced(field, "on"), 0);
    }
    // the other switches force nothing
    EXPECT_EQ(forced(&SpmvKnobStrings::ls_stage, "1"), 0);
    EXPECT_EQ(forced(&SpmvKnobStrings::nib, "1"), 0);
    EXPECT_EQ(forced(&SpmvKnobStrings::fix56, "1"), 0);
    done("split: forced by each of three variables");

    EXPECT_EQ(split_wanted(false, true, 1), 0);      // a handle's first launch
    EXPECT_EQ(split_wanted(false, true, 2), 1);      // its second
    EXPECT_EQ(split_wanted(false, true, 3), 1);
    EXPECT_EQ(split_wanted(false, false, 0), 1);     // a query before any launch
    EXPECT_EQ(split_wanted(false, false, 1), 1);
    EXPECT_EQ(split_wanted(true, true, 1), 1);       // forced
    done("split: query or launch, first or second");

    // (have_plan, split_considered, algo, profiling)
    EXPECT_EQ(split_open(false, false, MERGE, false), 1);     // no plan yet
    EXPECT_EQ(split_open(false, false, VECTOR, false), 1);
    EXPECT_EQ(split_open(true, false, MERGE, false), 1);      // the first product's plan
    EXPECT_EQ(split_open(true, true, MERGE, false), 0);       // final
    EXPECT_EQ(split_open(true, false, MERGE, true), 0);       // being profiled
    EXPECT_EQ(split_open(true, false, VECTOR, false), 0);
    EXPECT_EQ(split_open(true, false, SCALAR, false), 0);
    // (have_plan, split_considered, wanted, algo, profiling)
    EXPECT_EQ(plan_needs_rebuild(true, false, true, MERGE, false), 1);
    EXPECT_EQ(plan_needs_rebuild(false, false, true, MERGE, false), 0);      // nothing to rebuild
    EXPECT_EQ(plan_needs_rebuild(true, true, true, MERGE, false), 0);
    EXPECT_EQ(plan_needs_rebuild(true, false, false, MERGE, false), 0);      // not wanted yet
    EXPECT_EQ(plan_needs_rebuild(true, false, true, MERGE, true), 0);        // no rebuild while profiling
    EXPECT_EQ(plan_needs_rebuild(true, false, true, VECTOR, false), 0);      // nor under the other algorithms
    EXPECT_EQ(plan_needs_rebuild(true, false, true, SCALAR, false), 0);
    done("split: open, and the rebuild");
}

static void algo_cases()
{
    EXPECT_EQ(effective_algo(MERGE, 0), SCALAR);
    EXPECT_EQ(effective_algo(MERGE, 1), SCALAR);
    EXPECT_EQ(effective_algo(MERGE, 2), MERGE);
    EXPECT_EQ(effective_algo(VECTOR, 0), VECTOR);
    EXPECT_EQ(effective_algo(VECTOR, 1000), VECTOR);
    EXPECT_EQ(effective_algo(SCALAR, 1000), SCALAR);
    done("algorithm: fewer than two entries");

    EXPECT_EQ(parts_of(1).light, 1);
    EXPECT_EQ(parts_of(1).heavy, 0);
    EXPECT_EQ(parts_of(2).light, 0);
    EXPECT_EQ(parts_of(2).heavy, 1);
    EXPECT_EQ(parts_of(3).light, 1);
    EXPECT_EQ(parts_of(3).heavy, 1);
    EXPECT_EQ(launches_nothing(VECTOR, 2), 1);
    EXPECT_EQ(launches_nothing(SCALAR, 2), 1);
    EXPECT_EQ(launches_nothing(VECTOR, 1), 0);
    EXPECT_EQ(launches_nothing(VECTOR, 3), 0);
    EXPECT_EQ(launches_nothing(MERGE, 2), 0);
    EXPECT_EQ(launches_nothing(MERGE, 1), 0);
    done("algorithm: parts");
}

static void stream_form_cases()
{
    // (n_cold, rounds, idx24) -> mode
    EXPECT_EQ(ls_form(0, false, false, false, false, LS_DEFAULTS).mode, LS_PLAIN);
    EXPECT_EQ(ls_form(0, false, true, false, false, LS_DEFAULTS).mode, LS_PLAIN);
    EXPECT_EQ(ls_form(0, true, false, false, false, LS_DEFAULTS).mode, LS_PLAIN);      // rounds without cold entries
    EXPECT_EQ(ls_form(0, true, true, false, false, LS_DEFAULTS).mode, LS_PLAIN);
    EXPECT_EQ(ls_form(7, false, false, false, false, LS_DEFAULTS).mode, LS_PLAIN);
    EXPECT_EQ(ls_form(7, false, true, false, false, LS_DEFAULTS).mode, LS_PLAIN);      // 3-byte words without rounds
    EXPECT_EQ(ls_form(7, true, false, false, false, LS_DEFAULTS).mode, LS_RND);
    EXPECT_EQ(ls_form(7, true, true, false, false, LS_DEFAULTS).mode, LS_RND24);
    EXPECT_EQ(ls_form(1, true, false, false, false, LS_DEFAULTS).mode, LS_RND);        // one cold entry is cold staging
    EXPECT_EQ(LS_PLAIN, 0);      // the kernel's MODE values
    EXPECT_EQ(LS_RND, 2);
    EXPECT_EQ(LS_RND24, 3);
    const LsForm f = ls_form(7, true, true, true, false, LS_DEFAULTS), g = ls_form(0, false, false, false, true, LS_DEFAULTS);
    EXPECT_EQ(f.dense, 1);
    EXPECT_EQ(f.f32, 0);
    EXPECT_EQ(f.staged, 1);
    EXPECT_EQ(g.dense, 0);
    EXPECT_EQ(g.f32, 1);
    EXPECT_EQ(g.staged, 0);
    EXPECT_EQ(ls_form(7, false, false, false, false, LS_DEFAULTS).staged, 1);      // staged without rounds: plain, from xg
    done("stream form: modes");

    EXPECT_EQ(ls_form(0, false, false, false, false, LS_DEFAULTS).lds, (15360 + 8 * 514) * 8);      // 155 776 B
    EXPECT_EQ(ls_form(0, false, false, false, false, LS_DEFAULTS).lds, 155776);
    EXPECT_EQ(ls_form(7, false, true, false, false, LS_DEFAULTS).lds, 155776);
    EXPECT_EQ(ls_form(7, true, false, false, false, LS_DEFAULTS).lds, (8176 + 8192 + 8 * 514) * 8);      // all 160 KiB
    EXPECT_EQ(ls_form(7, true, false, false, false, LS_DEFAULTS).lds, 163840);
    EXPECT_EQ(ls_form(7, true, true, true, true, LS_DEFAULTS).lds, 163840);
    const LsLimits small = {100, 30, 50, 2, 10};      // every term on its own: (100 + 2 * 12) * 8, (30 + 50 + 2 * 12) * 8
    EXPECT_EQ(ls_form(0, false, false, false, false, small).lds, 992);
    EXPECT_EQ(ls_form(7, true, false, false, false, small).lds, 832);
    done("stream form: LDS");

    const double x[4] = {0, 0, 0, 0}, xg[16] = {0}, xh[4] = {0, 0, 0, 0};
    const LsBases a = ls_bases(ls_form(0, true, true, false, false, LS_DEFAULTS), 0, x, xg, xh);
    EXPECT_EQ(a.cold == x, 1);
    EXPECT_EQ(a.pack == xh, 1);
    const LsBases b = ls_bases(ls_form(7, true, false, false, false, LS_DEFAULTS), 7, x, xg, xh);
    EXPECT_EQ(b.cold == xg, 1);
    EXPECT_EQ(b.pack == xg + 7, 1);
    const LsBases c = ls_bases(ls_form(5, false, false, false, false, LS_DEFAULTS), 5, nullptr, xg, xh);      // staged, plain form
    EXPECT_EQ(c.cold == xg, 1);
    EXPECT_EQ(c.pack == xg + 5, 1);
    done("stream form: bases");

    const LsForm plain = ls_form(7, false, false, false, false, LS_DEFAULTS), rnd = ls_form(7, true, false, false, false, LS_DEFAULTS),
                 rnd24 = ls_form(7, true, true, false, false, LS_DEFAULTS);
    EXPECT_EQ(f32x_direct(MERGE, 1000, true, rnd), 1);
    EXPECT_EQ(f32x_direct(MERGE, 1000, true, rnd24), 1);
    EXPECT_EQ(f32x_direct(MERGE, 1000, true, plain), 0);
    EXPECT_EQ(f32x_direct(MERGE, 1000, false, rnd), 0);      // (a form worked out for a stream that is off)
    EXPECT_EQ(f32x_direct(MERGE, 2, true, rnd), 1);
    EXPECT_EQ(f32x_direct(MERGE, 1, true, rnd), 0);          // the scalar kernel reads the CSR arrays
    EXPECT_EQ(f32x_direct(VECTOR, 1000, true, rnd), 0);
    EXPECT_EQ(f32x_direct(SCALAR, 1000, true, rnd), 0);
    done("stream form: float32 x read directly");
}

// walks launch_groups[] the way launch_tier0 does: -> the (first, count) of every launch, or {-1} on a disagreement
static std::vector<int> launches_of(const std::vector<int32_t> &launch_groups)
{
    std::vector<int> out;
    int gb = 0;
    for (size_t a0 = 0; a0 < launch_groups.size(); a0 += (size_t)gb) {
        if (!acc_launch_count(a0, launch_groups[a0], launch_groups.size(), &gb)) return {-1};
        out.push_back((int)a0);
        out.push_back(gb);
    }
    return out;
}

static void tier0_cases()
{
    EXPECT_VEC(launches_of({1}), {0, 1});
    EXPECT_VEC(launches_of({2, 0}), {0, 2});
    EXPECT_VEC(launches_of({3, 0, 0}), {0, 3});
    EXPECT_VEC(launches_of({2, 0, 1}), {0, 2, 2, 1});
    EXPECT_VEC(launches_of({3, 0, 0, 2, 0}), {0, 3, 3, 2});
    EXPECT_VEC(launches_of({1, 1, 1, 1, 1, 1, 1, 1}), {0, 1, 1, 1, 2, 1, 3, 1, 4, 1, 5, 1, 6, 1, 7, 1});
    EXPECT_VEC(launches_of({}), {});
    done("tier 0: groups as launches");

    EXPECT_VEC(launches_of({0}), {-1});
    EXPECT_VEC(launches_of({4, 0, 0, 0}), {-1});      // more than a launch serves
    EXPECT_VEC(launches_of({2}), {-1});               // the count runs past the end
    EXPECT_VEC(launches_of({2, 0, 3, 0}), {-1});
    EXPECT_VEC(launches_of({-1}), {-1});
    EXPECT_VEC(launches_of({1, 0}), {-1});            // a group that belongs to no launch
    done("tier 0: groups and launches disagree");

    const size_t one[1] = {5000}, three[3] = {3000, 9000, 4000}, last[2] = {10, 20};
    const AccLaunch a = acc_launch(1, 999, 256, one);      // one group: its own workgroups, block b = workgroup b
    EXPECT_EQ(a.blocks, 256);
    EXPECT_EQ(a.lds, 5000);
    EXPECT_EQ(a.mapped, 0);
    const AccLaunch b = acc_launch(3, 255, 86, three);     // side by side: the launch's blocks through the map
    EXPECT_EQ(b.blocks, 255);
    EXPECT_EQ(b.lds, 9000);
    EXPECT_EQ(b.mapped, 1);
    const AccLaunch c = acc_launch(2, 256, 128, last);     // the maximum is the last group's
    EXPECT_EQ(c.blocks, 256);
    EXPECT_EQ(c.lds, 20);
    EXPECT_EQ(c.mapped, 1);
    done("tier 0: blocks, LDS and map of a launch");

    EXPECT_EQ(acc_form(false, false, false), ACC_F64);
    EXPECT_EQ(acc_form(false, false, true), ACC_FIX56);
    EXPECT_EQ(acc_form(false, true, true), ACC_NIB);       // a nib launch is a fix56 launch too
    EXPECT_EQ(acc_form(false, true, false), ACC_NIB);
    EXPECT_EQ(acc_form(true, false, false), ACC_F32);
    EXPECT_EQ(acc_form(true, true, true), ACC_F32);
    done("tier 0: value form");
}

static void rider_cases()
{
    EXPECT_EQ(t0_rides(4, 1, 1, true), 1);
    EXPECT_EQ(t0_rides(4, 2, 2, true), 1);
    EXPECT_EQ(t0_rides(4, 3, 3, true), 1);
    EXPECT_EQ(t0_rides(4, 2, 1, true), 0);       // two launches
    EXPECT_EQ(t0_rides(4, 8, 1, true), 0);
    EXPECT_EQ(t0_rides(4, 4, 4, true), 0);       // more groups than the rider has slots
    EXPECT_EQ(t0_rides(4, 2, 2, false), 0);      // nowhere to leave the sums
    EXPECT_EQ(t0_rides(8, 2, 2, true), 0);       // other than four wavefronts per pair workgroup
    EXPECT_EQ(t0_rides(2, 2, 2, true), 0);
    EXPECT_EQ(t0_rides(4, 0, 0, true), 0);       // no tier 0
    done("rider: when it rides");

    const int32_t r64[1] = {64}, r65[1] = {65}, r2x65[2] = {65, 65}, r3[3] = {1, 128, 129};
    const RiderBlocks a = rider_blocks(r64, 1);
    EXPECT_EQ(a.total, 1);
    EXPECT_EQ(a.start[0], 0);
    EXPECT_EQ(a.start[1], INT32_MAX);
    EXPECT_EQ(a.start[2], INT32_MAX);
    EXPECT_EQ(rider_blocks(r65, 1).total, 2);
    const RiderBlocks b = rider_blocks(r2x65, 2);
    EXPECT_EQ(b.start[0], 0);
    EXPECT_EQ(b.start[1], 2);
    EXPECT_EQ(b.start[2], INT32_MAX);
    EXPECT_EQ(b.total, 4);
    const RiderBlocks c = rider_blocks(r3, 3);      // 1, 2 and 3 blocks
    EXPECT_EQ(c.start[0], 0);
    EXPECT_EQ(c.start[1], 1);
    EXPECT_EQ(c.start[2], 3);
    EXPECT_EQ(c.total, 6);
    const RiderBlocks none = rider_blocks(nullptr, 0);      // nothing rides: the pair kernel's own groups alone
    EXPECT_EQ(none.total, 0);
    EXPECT_EQ(none.start[0], INT32_MAX);
    EXPECT_EQ(pair_grid(100, none.total), 100);
    EXPECT_EQ(pair_grid(100, b.total), 104);
    done("rider: blocks");
}

static std::vector<int> kinds(const EpiJobs &jobs)
{
    std::vector<int> k;
    for (int i = 0; i < jobs.n; i++) k.push_back(jobs.j[i].kind);
    return k;
}

static void epilogue_cases()
{
    static const int32_t rows[1] = {0};
    static const double vals[1] = {0.0};
    static double y[1] = {0.0};
    EXPECT_EQ(epi_fix(rows, vals, 1, y).blocks, 1);
    EXPECT_EQ(epi_fix(rows, vals, 1024, y).blocks, 1);
    EXPECT_EQ(epi_fix(rows, vals, 1025, y).blocks, 2);
    EXPECT_EQ(epi_fix(rows, vals, 1025, y).kind, 0);
    EXPECT_EQ(epi_fix(rows, vals, 1025, y).n, 1025);
    EXPECT_EQ(epi_fix(rows, vals, 1025, y).fy == y, 1);
    // reduce: G wavefronts per set of 64 rows, 16 wavefronts per workgroup
    EXPECT_EQ(epi_reduce(vals, rows, 256, 9, 4, nullptr, nullptr, nullptr, 0).blocks, 1);
    EXPECT_EQ(epi_reduce(vals, rows, 257, 9, 4, nullptr, nullptr, nullptr, 0).blocks, 2);
    EXPECT_EQ(epi_reduce(vals, rows, 512, 9, 2, nullptr, nullptr, nullptr, 0).blocks, 1);
    EXPECT_EQ(epi_reduce(vals, rows, 513, 9, 2, nullptr, nullptr, nullptr, 0).blocks, 2);
    EXPECT_EQ(epi_scatter(vals, rows, 1024).blocks, 1);
    EXPECT_EQ(epi_scatter(vals, rows, 1025).blocks, 2);
    EXPECT_EQ(epi_scatter(vals, rows, 1025).kind, 2);
    EXPECT_EQ(epi_scatter(vals, rows, 1025).H, 1025);
    done("epilogue: blocks of a fix, a reduce, a scatter");

    const EpiJob r = epi_tier0(false, vals, vals + 1, rows, 257, 63);
    EXPECT_EQ(r.kind, 1);
    EXPECT_EQ(r.G, 4);
    EXPECT_EQ(r.blocks, 2);
    EXPECT_EQ(r.n_wg, 63);
    EXPECT_EQ(r.extra, 0);
    EXPECT_EQ(r.partial == vals, 1);
    EXPECT_EQ(r.crp == nullptr, 1);
    const EpiJob sc = epi_tier0(true, vals, vals + 1, rows, 1025, 63);
    EXPECT_EQ(sc.kind, 2);
    EXPECT_EQ(sc.blocks, 2);
    EXPECT_EQ(sc.partial == vals + 1, 1);      // the rider's sums, not the workgroups' partials
    const EpiJob t64 = epi_tier1(vals, rows, 513, 64, rows, rows, vals, 3), t65 = epi_tier1(vals, rows, 513, 65, rows, rows, vals, 4);
    EXPECT_EQ(t64.kind, 1);
    EXPECT_EQ(t64.G, 2);
    EXPECT_EQ(t64.blocks, 2);      // 513 rows, 512 per workgroup
    EXPECT_EQ(t64.n_wg, 64);
    EXPECT_EQ(t64.extra, 3);
    EXPECT_EQ(t65.G, 4);
    EXPECT_EQ(t65.blocks, 3);      // 513 rows, 256 per workgroup
    EXPECT_EQ(t65.extra, 4);
    EXPECT_EQ(t65.crp == rows && t65.cidx == rows && t65.cval == vals, 1);
    done("epilogue: tier 0's and tier 1's jobs");

    // what one product hands to the launch, batch by batch: kinds, and each batch's grid
    std::vector<std::vector<int>> batches;
    std::vector<unsigned> grids;
    auto launch = [&](const EpiQueue &q) {
        batches.push_back(kinds(q.jobs));
        grids.push_back(q.grid());
        return 0;
    };
    const EpiJob fix = epi_fix(rows, vals, 1025, y), red1 = epi_tier1(vals, rows, 513, 65, rows, rows, vals, 0);
    auto reduce0 = [&](size_t g) { return epi_tier0(false, vals, vals, rows, 256 + (int32_t)g, 9); };      // group 0: 1 block, the others 2
    auto scatter0 = [&](size_t) { return epi_tier0(true, vals, vals, rows, 100, 9); };
    EXPECT_EQ(epi_run(&fix, 2, scatter0, &red1, launch), 0);
    EXPECT_EQ(batches.size(), 1);
    EXPECT_VEC(batches[0], {0, 2, 2, 1});
    EXPECT_EQ(grids[0], 2 + 1 + 1 + 3);
    batches.clear(), grids.clear();
    EXPECT_EQ(epi_run(&fix, 1, reduce0, &red1, launch), 0);
    EXPECT_VEC(batches[0], {0, 1, 1});
    EXPECT_EQ(grids[0], 2 + 1 + 3);
    batches.clear(), grids.clear();
    EXPECT_EQ(epi_run(nullptr, 1, reduce0, nullptr, launch), 0);      // part 2 of a plan without tier 1
    EXPECT_VEC(batches[0], {1});
    batches.clear(), grids.clear();
    EXPECT_EQ(epi_run(&fix, 0, reduce0, nullptr, launch), 0);         // part 1
    EXPECT_VEC(batches[0], {0});
    done("epilogue: order fix, tier 0, tier 1");

    batches.clear(), grids.clear();
    EXPECT_EQ(epi_run(&fix, 8, reduce0, &red1, launch), 0);      // eight groups that do not ride: ten jobs
    EXPECT_EQ(batches.size(), 2);
    EXPECT_VEC(batches[0], {0, 1, 1, 1, 1, 1});
    EXPECT_VEC(batches[1], {1, 1, 1, 1});
    EXPECT_EQ(grids[0], 2 + 1 + 2 + 2 + 2 + 2);
    EXPECT_EQ(grids[1], 2 + 2 + 2 + 3);
    batches.clear(), grids.clear();
    EXPECT_EQ(epi_run(&fix, 4, reduce0, &red1, launch), 0);      // exactly six: one batch, no empty second one
    EXPECT_EQ(batches.size(), 1);
    EXPECT_EQ(batches[0].size(), 6);
    batches.clear(), grids.clear();
    EXPECT_EQ(epi_run(&fix, 5, reduce0, &red1, launch), 0);      // seven: six and one
    EXPECT_EQ(batches.size(), 2);
    EXPECT_VEC(batches[1], {1});
    batches.clear(), grids.clear();
    EXPECT_EQ(epi_run(&fix, 11, reduce0, nullptr, launch), 0);   // twelve: two full batches
    EXPECT_EQ(batches.size(), 2);
    EXPECT_EQ(batches[1].size(), 6);
    batches.clear(), grids.clear();
    EXPECT_EQ(epi_run(nullptr, 0, reduce0, nullptr, launch), 0);      // nothing to do: no launch
    EXPECT_EQ(batches.size(), 0);
    done("epilogue: batches of six");

    batches.clear(), grids.clear();
    const EpiJob fix0 = epi_fix(rows, vals, 0, y), red_none = epi_tier1(vals, rows, 0, 65, rows, rows, vals, 0);
    auto some_empty = [&](size_t g) { return epi_tier0(false, vals, vals, rows, g == 1 ? 0 : 256, 9); };
    EXPECT_EQ(epi_nothing_to_do(fix0), 1);
    EXPECT_EQ(epi_nothing_to_do(fix), 0);
    EXPECT_EQ(epi_nothing_to_do(red_none), 1);
    EXPECT_EQ(epi_nothing_to_do(epi_scatter(vals, rows, 0)), 0);      // (a scatter is queued as it is)
    EXPECT_EQ(epi_run(&fix0, 3, some_empty, &red_none, launch), 0);
    EXPECT_EQ(batches.size(), 1);
    EXPECT_VEC(batches[0], {1, 1});
    EXPECT_EQ(grids[0], 2);
    batches.clear(), grids.clear();
    EXPECT_EQ(epi_run(&fix0, 0, some_empty, &red_none, launch), 0);      // only empty jobs: no launch
    EXPECT_EQ(batches.size(), 0);
    done("epilogue: empty jobs are skipped");

    // a launch that fails stops the product and hands its code back
    int calls = 0;
    auto failing = [&](const EpiQueue &) { return ++calls == 1 ? 7 : 0; };
    EXPECT_EQ(epi_run(&fix, 8, reduce0, &red1, failing), 7);
    EXPECT_EQ(calls, 1);
    calls = 1;      // (the next call returns 0: the last batch alone fails nothing)
    EXPECT_EQ(epi_run(&fix, 1, reduce0, nullptr, failing), 0);
    calls = 0;
    EXPECT_EQ(epi_run(&fix, 1, reduce0, nullptr, failing), 7);      // ... and the last batch's failure comes back too
    done("epilogue: a failed launch");
}

int main()
{
    static_assert(sizeof(EpiJob) == 96 && sizeof(EpiJobs) == 584, "the epilogue kernel's argument");
    split_cases();
    algo_cases();
    stream_form_cases();
    tier0_cases();
    rider_cases();
    epilogue_cases();
    if (failures) {
        printf("%d check(s) failed\n", failures);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
