// The total order of csrk_topk_rows, which topk_scores, topk_scores_for and rank_entries rank by as well: one definition,
// so that they cannot come to rank differently.  A value becomes an integer key whose unsigned order is the order of the
// values with every NaN on top (above +Inf) and all NaNs tied, and -0.0 tied with +0.0; among equal keys the smaller
// index (a column, an item, a position in the row) comes first.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace csrk {

// NaN -> all ones, -0.0 -> +0.0, then the usual sign flip
__device__ __forceinline__ uint64_t topk_key(double w)
{
    uint64_t b = (uint64_t)__double_as_longlong(w);
    if (w != w) return ~0ull;                    // every NaN: above +Inf, all tied
    if (w == 0.0) b = 0;                         // -0.0 ties with +0.0
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// a comes before b: the larger key, then the smaller index
template <class J>
__device__ __forceinline__ bool key_before(uint64_t ka, J ja, uint64_t kb, J jb)
{
    return ka > kb || (ka == kb && ja < jb);
}

}  // namespace csrk
