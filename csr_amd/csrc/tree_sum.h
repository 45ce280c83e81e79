// The fixed tree of rounded additions that rule P3 (csrk_panel_gram) and rule T (csrk_als_objective) share, one copy
// (include/csrk.h): `cnt` partials are combined level by level -- within a level the adjacent pairs (2 m, 2 m + 1) are
// added, an unpaired last partial is carried unchanged -- until one is left.  The pairs of level l never cross an aligned
// group of 2^l partials, so a thread that folds an aligned group of TREE_F = 32 in registers makes five levels of that tree
// at once, and a launch per five levels finishes it: 977 partials take two launches.  A partial is `width` doubles
// (k k for a Gram matrix, 1 for a sum); launches ping-pong between two regions.
#pragma once
#include "common.h"

namespace csrk {

constexpr int TREE_F = 32;               // partials a thread folds per launch
constexpr int TREE_THREADS = 256;
static_assert((TREE_F & (TREE_F - 1)) == 0, "an aligned group of a power of two is a subtree of the tree");

// element e of the partials [first, min(first + TREE_F, cnt)) at `in`, `width` doubles apart, folded into one; no partial
// (cnt <= first): +0.0
__device__ __forceinline__ double tree_fold_group(const double *__restrict__ in, int64_t width, int64_t e, int64_t first, int64_t cnt)
{
    int lc = cnt - first < TREE_F ? (int)(cnt - first) : TREE_F;
    double x[TREE_F];
#pragma unroll
    for (int i = 0; i < TREE_F; i++) x[i] = i < lc ? in[(first + i) * width + e] : 0.0;
#pragma unroll
    for (int w = TREE_F; w > 1; w /= 2) {
#pragma unroll
        for (int m = 0; m < w / 2; m++) x[m] = 2 * m + 1 < lc ? __dadd_rn(x[2 * m], x[2 * m + 1]) : x[2 * m];
        lc = (lc + 1) / 2;
    }
    return x[0];
}

// thread (g, e): element e of group g of `in` into partial g of out.  tri_k > 0: a partial is a tri_k x tri_k matrix of
// which only the lower triangle (t >= u) exists.
static __global__ __launch_bounds__(TREE_THREADS) void tree_fold_kernel(const double *__restrict__ in, int64_t cnt, int64_t width,
                                                                       int64_t groups, int tri_k, double *__restrict__ out)
{
    const int64_t idx = (int64_t)blockIdx.x * TREE_THREADS + threadIdx.x, g = idx / width, e = idx % width;
    if (g >= groups) return;
    if (tri_k > 0 && e % tri_k > e / tri_k) return;
    out[g * width + e] = tree_fold_group(in, width, e, g * TREE_F, cnt);
}

// partials behind the cnt partials that the launches need for their ping-pong
inline int64_t tree_extra_partials(int64_t cnt) { return cnt > TREE_F ? ceil_div(cnt, TREE_F) : 0; }

// Launches on s until at most TREE_F partials are left: cur then points at them and cnt counts them.  other: room for
// tree_extra_partials(cnt) partials, not overlapping cur's.
static void tree_fold_down(double *&cur, double *&other, int64_t &cnt, int64_t width, int tri_k, hipStream_t s)
{
    while (cnt > TREE_F) {
        const int64_t groups = ceil_div(cnt, TREE_F);
        tree_fold_kernel<<<(unsigned)ceil_div(groups * width, TREE_THREADS), TREE_THREADS, 0, s>>>(cur, cnt, width, groups, tri_k, other);
        double *t = cur;
        cur = other, other = t, cnt = groups;
    }
}

}  // namespace csrk
