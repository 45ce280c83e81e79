// The decisions one SpMV product takes on the host before it launches anything (spmv.hip, "host side"; DESIGN.md section 4,
// "The launch side"): whether the long-row split is wanted now, which algorithm and which parts run, which form of the light
// stream the plan holds, how tier 0's groups fall into launches, whether its reduce rides in tier 1's launch, and what the
// epilogue's jobs are.  One pure function per decision, plain values in; nothing here allocates.  Plain host C++, no device
// code: spmv.hip calls these on every product, and tests/spmv_launch_host runs them as a stand-alone program.  The constants
// it shares with the kernels are checked against theirs in spmv_plan.h.
#pragma once
#include "spmv_layout.h"

#include <cstddef>
#include <cstdint>

namespace csrk {

// ---- the epilogue's jobs (spmv_epilogue_kernel takes EpiJobs by value: their layout is the kernel's ABI) ---------------
struct EpiJob {
    int32_t kind, blocks;      // 0 = fix, 1 = reduce, 2 = scatter
    // fix
    const int32_t *carry_row;
    const double *carry_val;
    int64_t n;
    double *fy;
    // reduce, scatter
    const double *partial;
    const int32_t *row_list;
    int32_t H, n_wg, G;
    int32_t extra;                  // rows of partial[] behind the n_wg: added last, in order (tier 1's carry rows, Panel::ncs)
    const int32_t *crp, *cidx;      // optional (nullptr: no listed carries to add)
    const double *cval;
};
constexpr int EPI_BATCH = 6;        // jobs one launch of the epilogue covers at most
struct EpiJobs {
    EpiJob j[EPI_BATCH];
    int32_t n;
};
static_assert(sizeof(EpiJob) == 96 && sizeof(EpiJobs) == 6 * 96 + 8, "EpiJobs is read by spmv_epilogue_kernel");
constexpr int EPI_THREADS = 1024;

// the forms of spmv_lstream_kernel (its MODE)
constexpr int LS_PLAIN = 0, LS_RND = 2, LS_RND24 = 3;

namespace spmvlaunch {

constexpr int LANES = 64;            // a wavefront
constexpr int MAX_GROUPS = 3;        // groups one accumulator launch serves at most (accgroups::MAX_GROUPS)
constexpr int ALGO_MERGE = 1, ALGO_SCALAR = 3;      // CSRK_SPMV_MERGE, CSRK_SPMV_SCALAR

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- the long-row split: built on a handle's second product, unless something asks for it at once ----------------------
inline bool split_forced(const SpmvKnobs &k) { return k.heavy_split == 1 || k.hot == 1 || k.stream == 1; }
// a query (plan stats, cut rows, profiling) wants the split; a launch wants it from the handle's second one on
inline bool split_wanted(bool forced, bool launching, int64_t launches) { return forced || !launching || launches >= 2; }
// The decision is open -- and the environment worth reading -- while there is no plan, or a merge plan that was built without
// looking at the split and is not being profiled (its event slots would go with it).
inline bool split_open(bool have_plan, bool split_considered, int algo, bool profiling)
{
    return !have_plan || (!split_considered && algo == ALGO_MERGE && !profiling);
}
inline bool plan_needs_rebuild(bool have_plan, bool split_considered, bool wanted, int algo, bool profiling)
{
    return have_plan && wanted && split_open(have_plan, split_considered, algo, profiling);
}

// ---- the algorithm a product runs, and its parts ---------------------------------------------------------------------------
// the tile kernel's pair loads need two entries: a smaller matrix under the merge algorithm runs the scalar kernel
inline int effective_algo(int algo, int64_t nnz) { return algo == ALGO_MERGE && nnz < 2 ? ALGO_SCALAR : algo; }
// part (csrk_spmv_device_part): bit 0 = the rows of the row-major path (every row gets a value: the rows cut out for the
// tiers get 0.0), bit 1 = the tiers' rows (their reduces overwrite those zeros).  1 then 2 = 3.
struct Parts {
    bool light, heavy;
};
inline Parts parts_of(int part) { return {(part & 1) != 0, (part & 2) != 0}; }
// there are no tiers outside the merge algorithm
inline bool launches_nothing(int algo, int part) { return algo != ALGO_MERGE && !parts_of(part).light; }

// ---- the light stream's form ----------------------------------------------------------------------------------------------
struct LsLimits {      // LS_HOT_LDS, LS_RND_HOT, LS_RND_CAP, wavefronts per workgroup, ACC_TILE
    int hot_lds, rnd_hot, rnd_cap, waves, tile;
};
struct LsForm {
    int mode;             // LS_PLAIN, LS_RND, LS_RND24
    bool dense, f32;      // run k is row k; float32 values
    size_t lds;           // dynamic LDS: the pack's slots (and a round's staged values), then ACC_TILE + 2 run sums per wavefront
    bool staged;          // cold staging: the stream gathers from xg, not from the caller's x
};
// rounds: the plan holds round tables; they serve only what the copy pass staged, and 3-byte words only a round's offsets
inline LsForm ls_form(int64_t n_cold, bool rounds, bool idx24, bool dense, bool f32, const LsLimits &L)
{
    LsForm f;
    f.staged = n_cold > 0;
    f.mode = f.staged && rounds ? (idx24 ? LS_RND24 : LS_RND) : LS_PLAIN;
    f.dense = dense;
    f.f32 = f32;
    const size_t slots = f.mode == LS_PLAIN ? (size_t)L.hot_lds : (size_t)L.rnd_hot + (size_t)L.rnd_cap;
    f.lds = (slots + (size_t)L.waves * (size_t)(L.tile + 2)) * 8;
    return f;
}
// where the kernel's gathers start: the unpacked columns', and the pack's beyond its LDS slots
struct LsBases {
    const double *cold, *pack;
};
inline LsBases ls_bases(const LsForm &f, int64_t n_cold, const double *x, const double *xg, const double *xh)
{
    if (f.staged) return {xg, xg + n_cold};      // the staged values, in the stream's order, and the pack behind them
    return {x, xh};
}
// A float32 x is read as it is when no kernel of the product takes the CSR arrays and the light stream reads x through the
// copy pass alone: the merge algorithm on two entries or more, the stream on, in a rounds form.  Otherwise it is widened first.
inline bool f32x_direct(int algo, int64_t nnz, bool stream_on, const LsForm &f)
{
    return effective_algo(algo, nnz) == ALGO_MERGE && stream_on && f.mode != LS_PLAIN;
}

// ---- tier 0: its groups as launches -----------------------------------------------------------------------------------------
// The first group of a launch says how many groups the launch serves (AccPanel::launch_groups; 0 in the others).  The launch
// that starts at group `first` of n_groups: false when the groups and the launches disagree.
inline bool acc_launch_count(size_t first, int32_t launch_groups, size_t n_groups, int *count)
{
    if (launch_groups < 1 || launch_groups > MAX_GROUPS || first + (size_t)launch_groups > n_groups) return false;
    *count = launch_groups;
    return true;
}
enum AccForm { ACC_F32, ACC_NIB, ACC_FIX56, ACC_F64 };      // what a launch's value tiles hold (AccPanel: f32, nib, fix56)
inline AccForm acc_form(bool f32, bool nib, bool fix56) { return f32 ? ACC_F32 : nib ? ACC_NIB : fix56 ? ACC_FIX56 : ACC_F64; }
struct AccLaunch {
    unsigned blocks;
    size_t lds;       // the largest of its groups'
    bool mapped;      // several groups: block -> (group, workgroup) through wg_map
};
// launch_wgs, n_wg: the launch's first group's; lds[count]: every group's
inline AccLaunch acc_launch(int count, int32_t launch_wgs, int32_t n_wg, const size_t *lds)
{
    AccLaunch a;
    a.mapped = count > 1;
    a.blocks = (unsigned)(a.mapped ? launch_wgs : n_wg);
    a.lds = 0;
    for (int g = 0; g < count; g++) a.lds = lds[g] > a.lds ? lds[g] : a.lds;
    return a;
}

// ---- the rider: tier 0's reduce as extra workgroups of the pair kernel's launch (PanelRider) ---------------------------------
// pair_waves: wavefronts of a pair workgroup.  Tier 0 must be ONE launch (its groups, side by side, ride one behind the
// other) and hold somewhere to leave the sums (AccPanel::z).
inline bool t0_rides(int pair_waves, size_t n_groups, int32_t first_launch_groups, bool z_allocated)
{
    return pair_waves == 4 && n_groups > 0 && (size_t)first_launch_groups == n_groups && n_groups <= (size_t)MAX_GROUPS &&
           z_allocated;
}
struct RiderBlocks {
    int32_t start[MAX_GROUPS];      // each group's first rider block; INT32_MAX: no such group
    int64_t total;
};
// a rider block serves 64 rows, one per lane
inline RiderBlocks rider_blocks(const int32_t *rows, int n_groups)
{
    RiderBlocks r;
    r.total = 0;
    for (int q = 0; q < MAX_GROUPS; q++) {
        r.start[q] = INT32_MAX;
        if (q >= n_groups) continue;
        r.start[q] = (int32_t)r.total;
        r.total += cdiv(rows[q], LANES);
    }
    return r;
}
inline unsigned pair_grid(int64_t groups, int64_t rider_total) { return (unsigned)(groups + rider_total); }

// ---- the epilogue: one launch per EPI_BATCH jobs ------------------------------------------------------------------------------
// fix: y[row] += the carries of the tiles that end inside `row` (one thread per tile)
inline EpiJob epi_fix(const int32_t *carry_row, const double *carry_val, int64_t n_tiles, double *y)
{
    EpiJob J = {};
    J.kind = 0;
    J.blocks = (int32_t)cdiv(n_tiles, EPI_THREADS);
    J.carry_row = carry_row;
    J.carry_val = carry_val;
    J.n = n_tiles;
    J.fy = y;
    return J;
}
// reduce: y[row_list[h]] = the n_wg partials of row h in order, then `extra` carry rows, then the listed carries; G wavefronts
// share a set of 64 rows, so a workgroup takes 1024 / (64 G) sets
inline EpiJob epi_reduce(const double *partial, const int32_t *row_list, int32_t H, int32_t n_wg, int G, const int32_t *crp,
                         const int32_t *cidx, const double *cval, int32_t extra)
{
    EpiJob J = {};
    J.kind = 1;
    J.blocks = (int32_t)cdiv(H, LANES * (EPI_THREADS / LANES / G));
    J.partial = partial;
    J.row_list = row_list;
    J.H = H;
    J.n_wg = n_wg;
    J.G = G;
    J.extra = extra;
    J.crp = crp;
    J.cidx = cidx;
    J.cval = cval;
    return J;
}
// scatter: y[row_list[h]] = z[h], the sums a rider left (one thread per row)
inline EpiJob epi_scatter(const double *z, const int32_t *row_list, int32_t H)
{
    EpiJob J = {};
    J.kind = 2;
    J.blocks = (int32_t)cdiv(H, EPI_THREADS);
    J.partial = z;
    J.row_list = row_list;
    J.H = H;
    return J;
}
// one group of tier 0: its sums are scattered when its reduce rode in the pair kernel's launch, else reduced here (G = 4)
inline EpiJob epi_tier0(bool rides, const double *partial, const double *z, const int32_t *row_list, int32_t H, int32_t n_wg)
{
    if (rides) return epi_scatter(z, row_list, H);
    return epi_reduce(partial, row_list, H, n_wg, 4, nullptr, nullptr, nullptr, 0);
}
// tier 1: over the nb column blocks (G = 4 above 64 of them, else 2), then the ncs carry rows and the listed carries
inline EpiJob epi_tier1(const double *partial, const int32_t *row_list, int32_t H, int32_t nb, const int32_t *crp,
                        const int32_t *cidx, const double *cval, int32_t ncs)
{
    return epi_reduce(partial, row_list, H, nb, nb > 64 ? 4 : 2, crp, cidx, cval, ncs);
}
// a fix without tiles and a reduce without rows are not queued
inline bool epi_nothing_to_do(const EpiJob &J) { return J.kind == 0 ? J.n <= 0 : J.kind == 1 ? J.H <= 0 : false; }

struct EpiQueue {
    EpiJobs jobs;
    EpiQueue() { jobs.n = 0; }
    // true: the batch is full -- launch it (grid() blocks) and clear() before the next push
    bool push(const EpiJob &J)
    {
        if (!epi_nothing_to_do(J)) jobs.j[jobs.n++] = J;
        return jobs.n == EPI_BATCH;
    }
    bool empty() const { return jobs.n == 0; }
    unsigned grid() const
    {
        unsigned g = 0;
        for (int i = 0; i < jobs.n; i++) g += (unsigned)jobs.j[i].blocks;
        return g;
    }
    void clear() { jobs.n = 0; }
    // push, and hand a full batch to `launch` (int(const EpiQueue &), 0 = ok)
    template <class Launch> int add(const EpiJob &J, Launch &launch)
    {
        if (!push(J)) return 0;
        const int rc = launch(*this);
        clear();
        return rc;
    }
};

// The jobs of one product in their order -- the light stream's fix (nullptr: no rows were cut, or no light part), tier 0's
// groups (t0_job(g), g < n_groups), tier 1's reduce (nullptr: no tier 1) -- handed to `launch` a batch at a time.
template <class GroupJob, class Launch>
inline int epi_run(const EpiJob *fix, size_t n_groups, GroupJob &&t0_job, const EpiJob *tier1, Launch &&launch)
{
    EpiQueue q;
    int rc = fix ? q.add(*fix, launch) : 0;
    for (size_t g = 0; g < n_groups && rc == 0; g++) rc = q.add(t0_job(g), launch);
    if (tier1 && rc == 0) rc = q.add(*tier1, launch);
    if (rc != 0 || q.empty()) return rc;
    return launch(q);
}

}  // namespace spmvlaunch
}  // namespace csrk
