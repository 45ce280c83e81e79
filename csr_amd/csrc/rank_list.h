// What rank_entries.hip and rank_entries_for.hip share beyond the score tile: the size of a row's list of test entries, the
// chain of one (row, item) pair straight from the panels, and the search of a score's place in a row's ordered list (moved
// here from rank_entries.hip unchanged).  Both kernels keep their own text.
#pragma once
#include "common.h"
#include "score_tile.h"

namespace csrk {

// (RE_T, RE_K_MAX and the REF_* constants: score_plan.h)
constexpr int RE_LDT = RE_T + 1;                // list line (rows fall into different banks)
constexpr int32_t RE_BAD_ITEM = 0x7fffffff;     // listed for a test column outside [0, n_items): never dereferenced
static_assert(RE_T <= WAVE, "one lane per listed entry");

// csrk_topk_scores' rule 2 for one pair, straight from the panels
template <class T> __device__ __forceinline__ double re_chain(const T *__restrict__ u, const T *__restrict__ v, int k)
{
    double s = 0.0;
    for (int t = 0; t < k; t++) s = __builtin_fma((double)u[t], (double)v[t], s);
    return s;
}

// the first of the n listed entries (best first) that (ks, j) comes before; n when there is none
__device__ __forceinline__ int re_slot(const uint64_t *__restrict__ sk, const int32_t *__restrict__ si, int n, uint64_t ks, int32_t j)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key_before(ks, j, sk[mid], si[mid]))
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

}  // namespace csrk
