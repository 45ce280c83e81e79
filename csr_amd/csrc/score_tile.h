// The score tile that topk_scores.hip and rank_entries.hip share: the constants of the register-tiled float64 product
// (a 256-thread workgroup, 64 rows x 64 items per tile, 4 x 4 chains per thread, 16 factors per LDS chunk), the loads
// that bring a chunk of a panel into LDS transposed, and the lookup of a column in a sorted row.  Both kernels run the
// same chains, so a score has the same bits in either.  (The order they rank by: topk_order.h.  A unit of a panel row and
// the sorted-row search: device_loads.h.)
#pragma once
#include "common.h"
#include "device_loads.h"
#include "score_plan.h"
#include "topk_order.h"

namespace csrk {

// (TS_THREADS, TS_ROWS, TS_TILE: score_plan.h, with everything else the host side reads)
constexpr int TS_B = 4;                         // register tile edge
constexpr int TS_KC = 16;                       // factors per LDS chunk
constexpr int TS_LD = TS_ROWS + 2;              // doubles per staged line
static_assert(TS_ROWS == TS_TILE && TS_ROWS * TS_TILE == TS_THREADS * TS_B * TS_B, "one 4 x 4 block of chains per thread");

// factors [t0, t0 + TS_KC) of the panel rows first .. first + 63, in two halves: ts_fetch loads this thread's units into
// registers (rows at or beyond nvalid and factors at or beyond k become +0.0: such rows' chains are never looked at, such
// factors never enter a chain), ts_put writes them to s[factor][row].  The loads of the next chunk are in flight while the
// current one is used.
template <class T, int PER> struct TsUnits {
    static constexpr int UPR = TS_KC / PER;                       // units per row and chunk
    static constexpr int NL = TS_ROWS * UPR / TS_THREADS;         // units per thread
    double d[NL][PER];
};

template <class T, int PER>
__device__ __forceinline__ void ts_fetch(TsUnits<T, PER> &u, const T *__restrict__ P, int64_t ld, int64_t first, int64_t nvalid, int t0,
                                         int k, int tid)
{
    typedef TsUnits<T, PER> N;
#pragma unroll
    for (int l = 0; l < N::NL; l++) {
        const int x = tid + l * TS_THREADS, r = x / N::UPR, t = t0 + (x % N::UPR) * PER;
#pragma unroll
        for (int e = 0; e < PER; e++) u.d[l][e] = 0.0;
        if (r < nvalid && t < k) panel_unit<T, PER>(P + (first + r) * ld + t, u.d[l]);      // (PER > 1: k is a whole number of pieces)
    }
}

template <class T, int PER>
__device__ __forceinline__ void ts_put(const TsUnits<T, PER> &u, double (*__restrict__ s)[TS_LD], int tid)
{
    typedef TsUnits<T, PER> N;
#pragma unroll
    for (int l = 0; l < N::NL; l++) {
        const int x = tid + l * TS_THREADS, r = x / N::UPR, o = (x % N::UPR) * PER;
#pragma unroll
        for (int e = 0; e < PER; e++) s[o + e][r] = u.d[l][e];
    }
}

// does the sorted row ci[e0 .. e1) hold column j?  (indices are compared, never used as addresses)
__device__ __forceinline__ bool ts_seen(const int32_t *__restrict__ ci, int64_t e0, int64_t e1, int32_t j)
{
    const int64_t lo = first_not_below(ci, e0, e1, j);
    return lo < e1 && ci[lo] == j;
}

}  // namespace csrk
