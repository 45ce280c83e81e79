// Tier 0's row groups (spmv_plan.h, "long rows, accumulator form"): how the tier's rows are dealt to groups, how many
// persistent workgroups each group of one launch gets, and which block of the launch serves which (group, workgroup).
// Plain host arithmetic, no device code: spmv_plan.hip calls it when it builds a plan, and tests/acc_groups_host runs it
// as a stand-alone program.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

namespace csrk {
namespace accgroups {

constexpr int MAX_GROUPS = 3;      // groups one launch of the accumulator kernel serves at most
constexpr int XCDS = 8;            // blocks b and b + 8 of a launch share an XCD, and with it an L2 (observed; speed only)

// The tier's rows as groups, and the groups as launches.  groups[k] lists positions in the caller's (ascending) row list,
// ascending; launch j is groups[first[j]] .. groups[first[j + 1]).
struct Deal {
    std::vector<std::vector<int32_t>> groups;
    std::vector<int32_t> first;
};

// G = 1: consecutive ranges of `cap` rows, a launch each.
// G > 1: the rows ranked by length (longest first, ties by position) are taken G * cap at a time; the n of one launch make
// min(G, ceil(n / cap)) groups and rank i goes to group i mod that.  Every group then has about the same entries in every
// column block, so the groups of a launch walk the column blocks at the same pace.  n <= cap gives the one group of G = 1.
inline Deal deal_rows(const int64_t *lens, int32_t n, int G, int32_t cap)
{
    Deal d;
    d.first.push_back(0);
    if (n <= 0) return d;
    if (cap < 1) cap = 1;
    if (G < 1) G = 1;
    if (G > MAX_GROUPS) G = MAX_GROUPS;
    if (G == 1) {
        for (int32_t g0 = 0; g0 < n; g0 += cap) {
            const int32_t g1 = n - g0 < cap ? n : g0 + cap;
            std::vector<int32_t> g((size_t)(g1 - g0));
            std::iota(g.begin(), g.end(), g0);
            d.groups.push_back(std::move(g));
            d.first.push_back((int32_t)d.groups.size());
        }
        return d;
    }
    std::vector<int32_t> rank((size_t)n);
    std::iota(rank.begin(), rank.end(), 0);
    std::stable_sort(rank.begin(), rank.end(), [&](int32_t a, int32_t b) { return lens[a] > lens[b]; });
    const int64_t per_launch = (int64_t)G * cap;
    for (int64_t r0 = 0; r0 < n; r0 += per_launch) {
        const int64_t nl = n - r0 < per_launch ? n - r0 : per_launch;
        const int gb = (int)std::min<int64_t>(G, (nl + cap - 1) / cap);
        const size_t base = d.groups.size();
        d.groups.resize(base + (size_t)gb);
        for (int64_t i = 0; i < nl; i++) d.groups[base + (size_t)(i % gb)].push_back(rank[(size_t)(r0 + i)]);
        for (int g = 0; g < gb; g++) std::sort(d.groups[base + (size_t)g].begin(), d.groups[base + (size_t)g].end());
        d.first.push_back((int32_t)d.groups.size());
    }
    return d;
}

// How many groups pay (when CSRK_ACC_GROUPS does not say).  A further group halves or thirds the tiles of a segment (a
// segment = one column block of one workgroup's share: a window fill, two barriers and a head fold, and with few tiles per
// wavefront the tile loop's loads are no longer hidden), and what it takes from tier 1 shrinks with the matrix.  Measured on
// the headline matrix and its 2-way row partition: 2 groups at 57 tiles per segment gain 12 us, 3 groups
// at 41 and 2 groups at 32 (the partition) lose.  So g groups are taken only if the tier's tiles, over the g * nb + cus
// segments they are cut into, leave MIN_SEG_TILES per segment: three per wavefront of the sixteen.
// lens: the cut rows' lengths; the tier would hold the g * cap longest of those not shorter than floor_len.
constexpr int64_t TILE_ENTRIES = 512;
constexpr int64_t MIN_SEG_TILES = 48;
inline int choose_groups(const int64_t *lens, int32_t n, int g_max, int32_t cap, int64_t floor_len, int64_t nb, int32_t cus)
{
    if (cap < 1) cap = 1;
    if (g_max > MAX_GROUPS) g_max = MAX_GROUPS;
    if (g_max < 2 || n <= cap) return 1;
    std::vector<int64_t> sl;
    for (int32_t i = 0; i < n; i++)
        if (lens[i] >= floor_len) sl.push_back(lens[i]);
    for (int g = g_max; g > 1; g--) {
        const int64_t k = std::min<int64_t>((int64_t)sl.size(), (int64_t)g * cap);
        if (k <= (int64_t)(g - 1) * cap) continue;      // the rows fit fewer groups
        // the k longest in front, in any order (a full sort of 10^5 lengths would be milliseconds of the plan)
        if (k < (int64_t)sl.size()) std::nth_element(sl.begin(), sl.begin() + k, sl.end(), [](int64_t a, int64_t b) { return a > b; });
        int64_t entries = 0;
        for (int64_t i = 0; i < k; i++) entries += sl[(size_t)i];
        if (entries / TILE_ENTRIES >= MIN_SEG_TILES * ((int64_t)g * nb + cus)) return g;
    }
    return 1;
}

// Whether a launch whose groups are packable takes the 8.5-byte entries (fix56.h, nib) instead of the 9-byte ones.  Both
// decode exactly; the 8.5-byte form reads 256 B less per tile and spends a few more vector instructions per entry on the
// nibble, the sign and the padding test.  The bytes are the kernel's time only where the stream is: a workgroup that walks
// less than a tile per wavefront spends its time on the window fills, barriers and head folds of its segments, and the
// smaller entry buys nothing there.  So without CSRK_SPMV_NIB (knob < 0) the form is taken when the launch's entries make
// NIB_MIN_WG_TILES whole tiles per workgroup, one per wavefront of the sixteen; knob = 1 takes it whenever the groups are
// packable, knob = 0 never.  (The headline matrix has about 1130 tiles per workgroup.)
constexpr int64_t NIB_MIN_WG_TILES = 16;
inline bool choose_nib(int knob, int64_t launch_entries, int32_t launch_wgs)
{
    if (knob >= 0) return knob != 0;
    if (launch_wgs < 1) launch_wgs = 1;
    return launch_entries >= 0 && launch_entries / TILE_ENTRIES >= NIB_MIN_WG_TILES * (int64_t)launch_wgs;
}

// workgroups of group g when `cus` compute units serve the gb groups of one launch: equal shares, the remainder to the
// first groups, one at least
inline int32_t group_wgs(int32_t cus, int gb, int g)
{
    const int32_t n = cus / gb + (g < cus % gb ? 1 : 0);
    return n < 1 ? 1 : n;
}

// Block b of a launch of sum(n_wg) blocks serves workgroup (map[b] & 0xffff) of group (map[b] >> 16).  Workgroup w of every
// group covers about the same column range (each group's tiles are cut into equal shares), so the workgroups w of all
// groups are given blocks that are equal mod XCDS: the window one of them pulls into its XCD's L2 is there for the others.
// Blocks are handed out in the order (w, group), so workgroups of one column range are also dispatched together.  An XCD
// holds ceil or floor of blocks / XCDS; what does not fit where it belongs (group sizes that are no multiple of XCDS)
// takes the blocks left over, lowest first.
inline std::vector<uint32_t> place_wgs(const int32_t *n_wg, int gb)
{
    int64_t total = 0;
    int32_t w_max = 0;
    for (int g = 0; g < gb; g++) {
        total += n_wg[g];
        w_max = std::max(w_max, n_wg[g]);
    }
    std::vector<uint32_t> map((size_t)total, ~0u);
    int64_t fill[XCDS], room[XCDS];
    for (int c = 0; c < XCDS; c++) {
        fill[c] = 0;
        room[c] = total / XCDS + (c < total % XCDS ? 1 : 0);
    }
    std::vector<uint32_t> late;
    for (int32_t w = 0; w < w_max; w++)
        for (int g = 0; g < gb; g++) {
            if (w >= n_wg[g]) continue;
            const uint32_t id = ((uint32_t)g << 16) | (uint32_t)w;
            const int c = w % XCDS;
            if (fill[c] < room[c]) map[(size_t)(c + XCDS * fill[c]++)] = id;
            else late.push_back(id);
        }
    size_t b = 0;
    for (uint32_t id : late) {
        while (map[b] != ~0u) b++;
        map[b] = id;
    }
    return map;
}

}  // namespace accgroups
}  // namespace csrk
