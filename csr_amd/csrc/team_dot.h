// Rule C2's DOT (include/csrk.h) over a team of PANEL_G = 16 lanes, one copy for the kernels that take it: the CG
// half-step (als_cg.hip) and the ALS objective (als_objective.hip).  A lane holds its four columns of every 64-column chunk
// (panel_off in device_loads.h); a DOT is the lane's fma chain over its columns and four DPP adds that form a butterfly
// (lane ^ 1, ^ 2, then the half-row and row mirrors), so EVERY lane ends with the sum in C2's tree shape -- floating-point
// addition commutes, so the lanes agree bit for bit (NaN payloads apart) -- and no broadcast follows.
#pragma once
#include "device_loads.h"
#include "wave.h"

namespace csrk {

// dpp_ctrl encodings (CDNA ISA): quad_perm [1, 0, 3, 2] and [2, 3, 0, 1], lanes 7 - l of a half row, 15 - l of a row
constexpr int DPP_QUAD_X1 = 0xB1, DPP_QUAD_X2 = 0x4E, DPP_ROW_HALF_MIRROR = 0x141, DPP_ROW_MIRROR = 0x140;

// rule C2's tree, in every lane of the team
__device__ __forceinline__ double cg_team_sum(double s)
{
    s = __dadd_rn(s, dpp_f64<DPP_QUAD_X1>(0.0, s));
    s = __dadd_rn(s, dpp_f64<DPP_QUAD_X2>(0.0, s));
    s = __dadd_rn(s, dpp_f64<DPP_ROW_HALF_MIRROR>(0.0, s));
    s = __dadd_rn(s, dpp_f64<DPP_ROW_MIRROR>(0.0, s));
    return s;
}

// rule C2: DOT(a, b); OFFT is the panel type (it fixes which columns the lane owns)
template <class OFFT, int NCH, class A>
__device__ __forceinline__ double cg_dot(const A (&a)[NCH][4], const double (&b)[NCH][4], int sub, int k)
{
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (64 * c + panel_off<OFFT>(sub, q) < k) s = __builtin_fma((double)a[c][q], b[c][q], s);
    return cg_team_sum(s);
}

}  // namespace csrk
