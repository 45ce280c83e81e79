// The score tile that topk_scores.hip and rank_entries.hip share: the constants of the register-tiled float64 product
// (a 256-thread workgroup, 64 rows x 64 items per tile, 4 x 4 chains per thread, 16 factors per LDS chunk), the total
// order of csrk_topk_rows as an integer key, the loads that bring a chunk of a panel into LDS transposed, and the lookup
// of a column in a sorted row.  Both kernels run the same chains, so a score has the same bits in either.
#pragma once
#include "common.h"

namespace csrk {

constexpr int TS_THREADS = 256;
constexpr int TS_ROWS = 64;                     // rows of U per workgroup
constexpr int TS_TILE = 64;                     // items per tile
constexpr int TS_B = 4;                         // register tile edge
constexpr int TS_KC = 16;                       // factors per LDS chunk
constexpr int TS_LD = TS_ROWS + 2;              // doubles per staged line
static_assert(TS_ROWS == TS_TILE && TS_ROWS * TS_TILE == TS_THREADS * TS_B * TS_B, "one 4 x 4 block of chains per thread");

typedef double ts_d2 __attribute__((ext_vector_type(2)));
typedef float ts_f4 __attribute__((ext_vector_type(4)));

// csrk_topk_rows' order as an integer (topk.hip): NaN -> all ones, -0.0 -> +0.0, then the usual sign flip
__device__ __forceinline__ uint64_t topk_key(double w)
{
    uint64_t b = (uint64_t)__double_as_longlong(w);
    if (w != w) return ~0ull;                    // every NaN: above +Inf, all tied
    if (w == 0.0) b = 0;                         // -0.0 ties with +0.0
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// one unit of a panel row as float64: PER elements (a 16-B piece when PER > 1, else one element)
template <class T, int PER> __device__ __forceinline__ void ts_load(const T *__restrict__ p, double d[PER]);
template <> __device__ __forceinline__ void ts_load<double, 1>(const double *__restrict__ p, double d[1]) { d[0] = *p; }
template <> __device__ __forceinline__ void ts_load<float, 1>(const float *__restrict__ p, double d[1]) { d[0] = (double)*p; }
template <> __device__ __forceinline__ void ts_load<double, 2>(const double *__restrict__ p, double d[2])
{
    const ts_d2 a = *(const ts_d2 *)p;
    d[0] = a.x, d[1] = a.y;
}
template <> __device__ __forceinline__ void ts_load<float, 4>(const float *__restrict__ p, double d[4])
{
    const ts_f4 a = *(const ts_f4 *)p;
    d[0] = (double)a.x, d[1] = (double)a.y, d[2] = (double)a.z, d[3] = (double)a.w;
}

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
        if (r < nvalid && t < k) ts_load<T, PER>(P + (first + r) * ld + t, u.d[l]);      // (PER > 1: k is a whole number of pieces)
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
    int64_t lo = e0, hi = e1;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ci[mid] < j)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < e1 && ci[lo] == j;
}

}  // namespace csrk
