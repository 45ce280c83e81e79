// The row accumulation that gram.hip and als.hip share: for one row of a CSR matrix, the lower triangle of
//     G = base + sum over the row's stored entries e = (i, j), in storage order, of w_e v_j v_j^T        (k x k, float64)
// in 4 x 4 register tiles, and with RHS the right-hand side b = sum c_e v_j beside it.  One definition of the k classes, the
// tile numbering, the staging pipeline and the multiply-add loop, so that an als_rows row and a gram_rows row are the same
// arithmetic (include/csrk.h, rule A) because they are the same code; and the host-side refusal of a k above the classes.
// (Panel checks, the 16-B predicate and packing: panel.h.  The panel loads and an entry's value: device_loads.h.  The
// team fence: wave.h.)
//
// Work split.  A TEAM of threads owns a row: 16 lanes for k <= 16, a wavefront for k <= 40, a 256-thread workgroup above.
// The lower triangle is cut into 4 x 4 register tiles (tile (bp, bq), bq <= bp, holds p = 4 bp .. 4 bp + 3, q = 4 bq ..
// 4 bq + 3); a thread keeps one tile (k <= 88) or up to three (k <= 128) in registers for the whole row.  The row's V rows
// go through LDS GT_STAGE entries per step, widened to float64, in two buffers: while a step is consumed the next step's V
// rows and weights are in flight to registers and the column indices of the step after that are in flight behind them, so
// a step waits for one round trip at most (SDDMM's discipline).  Per staged entry a tile reads its four p- and four q-
// operands from LDS (four 16-B reads) for four rounded multiplies and sixteen fused multiply-adds; the strictly upper part of
// a diagonal tile is computed and dropped.  V is read in 16-B pieces when its base pointer, ldv and k allow whole
// pieces, else element by element: the same bits.
#pragma once
#include "common.h"
#include "device_loads.h"
#include "panel.h"
#include "wave.h"

namespace csrk {

constexpr int GT_THREADS = 256;
constexpr int GT_STAGE = 8;                      // entries staged per step
constexpr int GT_B = 4;                          // register tile edge
constexpr int GT_K_SUB = 16;                     // k up to this: 16 lanes per row
constexpr int GT_K_WAVE = 40;                    // k up to this: a wavefront per row
constexpr int GT_K_ONE = 88;                     // k up to this: a workgroup per row, one tile per thread
constexpr int GT_K_MAX = 128;                    // k up to this: a workgroup per row, up to three tiles per thread

template <int CLS> struct GramClass;
template <> struct GramClass<0> { static constexpr int TEAM = 16, KMAX = GT_K_SUB, TPT = 1; };
template <> struct GramClass<1> { static constexpr int TEAM = 64, KMAX = GT_K_WAVE, TPT = 1; };
template <> struct GramClass<2> { static constexpr int TEAM = 256, KMAX = GT_K_ONE, TPT = 1; };
template <> struct GramClass<3> { static constexpr int TEAM = 256, KMAX = GT_K_MAX, TPT = 3; };

// tile t of the lower triangle, row-major over 4 x 4 blocks: block row bp, block column bq <= bp
__device__ __forceinline__ void gt_tile(int t, bool has, int &p0, int &q0)
{
    int b = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while (b * (b + 1) / 2 > t) b--;
    while ((b + 1) * (b + 2) / 2 <= t) b++;
    p0 = has ? GT_B * b : 0;
    q0 = has ? GT_B * (t - b * (b + 1) / 2) : 0;
}

// The row's entries [e0, e1) into the team's register tiles acc (tile r at p0[r], q0[r], already holding base or +0.0):
// per entry in storage order t = round(w v_p), G[p][q] = fma(t, v_q, G[p][q]), w the entry's value under SCALE, else 1.0.
// sv[2][GT_STAGE][KP] and sw[2][GT_STAGE] are the team's LDS; every thread of the team calls this (it holds team fences).
// RHS = false: weights are loaded and staged under SCALE only, and rhs_mode and b are not looked at.
// RHS = true: weights are loaded when vals is not NULL (else every one is 1.0) and always staged, and thread tid < k
// carries b = b[tid] along: b = fma(c, v_tid, b) with c = 1, the weight, or 1 + the weight by rhs_mode.
template <class T, bool WIDE, int CLS, bool SCALE, bool RHS>
__device__ __forceinline__ void gt_accumulate(int64_t e0, int64_t e1, const int32_t *__restrict__ ci, const void *__restrict__ vals,
                                              int vt, const T *__restrict__ V, int64_t ldv, int k, int rhs_mode, int tid,
                                              double (*sv)[GT_STAGE][GramClass<CLS>::KMAX], double (*sw)[GT_STAGE],
                                              double (&acc)[GramClass<CLS>::TPT][GT_B][GT_B], const int (&p0)[GramClass<CLS>::TPT],
                                              const int (&q0)[GramClass<CLS>::TPT], double &b)
{
    constexpr int TEAM = GramClass<CLS>::TEAM, KP = GramClass<CLS>::KMAX, TPT = GramClass<CLS>::TPT;
    constexpr int PER = WIDE ? 16 / (int)sizeof(T) : 1;                     // elements per load
    constexpr int NL = (GT_STAGE * (KP / PER) + TEAM - 1) / TEAM;           // loads per thread and step
    const bool wload = (RHS ? vals != nullptr : SCALE) && tid < GT_STAGE;   // this thread fetches a weight per step
    const bool wstage = (RHS || SCALE) && tid < GT_STAGE;                   // ... and stages one

    // this thread's share of a step: unit x = tid + l TEAM is piece x % upr of staged entry x / upr
    const int upr = k / PER;                                                // units per panel row (WIDE: k is a whole number of pieces)
    int ue[NL], uo[NL];
#pragma unroll
    for (int l = 0; l < NL; l++) {
        const int x = tid + l * TEAM;
        ue[l] = x / upr;                                                    // (>= GT_STAGE: no such unit)
        uo[l] = (x % upr) * PER;
    }
    const int64_t last = e1 - 1;
    int32_t coln[NL] = {};                                                  // (only this thread's units are loaded)
    double vreg[NL][PER], wreg = 1.0;                                       // (no values wanted or none stored: 1.0)
    if (e0 < e1) {
#pragma unroll
        for (int l = 0; l < NL; l++) {
            const int64_t e = e0 + ue[l];
            if (ue[l] < GT_STAGE) coln[l] = ci[e < last ? e : last];
        }
#pragma unroll
        for (int l = 0; l < NL; l++)
            if (ue[l] < GT_STAGE) panel_unit<T, PER>(V + (int64_t)coln[l] * ldv + uo[l], vreg[l]);
        if (wload) {
            const int64_t e = e0 + tid < last ? e0 + tid : last;
            wreg = csr_stored_val(vals, vt, e);
        }
#pragma unroll
        for (int l = 0; l < NL; l++) {
            const int64_t e = e0 + GT_STAGE + ue[l];
            if (ue[l] < GT_STAGE) coln[l] = ci[e < last ? e : last];
        }
    }

    int buf = 0;
    for (int64_t es = e0; es < e1; es += GT_STAGE, buf ^= 1) {
        const int cnt = e1 - es < GT_STAGE ? (int)(e1 - es) : GT_STAGE;
        // this step's V rows and weights: registers -> LDS  (entries past the row's end hold its last entry again, unused)
#pragma unroll
        for (int l = 0; l < NL; l++)
            if (ue[l] < GT_STAGE) {
#pragma unroll
                for (int x = 0; x < PER; x++) sv[buf][ue[l]][uo[l] + x] = vreg[l][x];
            }
        if (wstage) sw[buf][tid] = wreg;
        team_sync<TEAM>();
        // the next step's V rows and weights and the column indices of the step after it, in flight while this one is used
        if (es + GT_STAGE < e1) {
#pragma unroll
            for (int l = 0; l < NL; l++)
                if (ue[l] < GT_STAGE) panel_unit<T, PER>(V + (int64_t)coln[l] * ldv + uo[l], vreg[l]);
            if (wload) {
                const int64_t e = es + GT_STAGE + tid < last ? es + GT_STAGE + tid : last;
                wreg = csr_stored_val(vals, vt, e);
            }
#pragma unroll
            for (int l = 0; l < NL; l++) {
                const int64_t e = es + 2 * GT_STAGE + ue[l];
                if (ue[l] < GT_STAGE) coln[l] = ci[e < last ? e : last];
            }
        }
        // the staged entries in storage order.  (Columns k .. 4 nb - 1 of a staged row are never written: an edge tile reads
        // whatever LDS holds there into accumulators with p >= k or q >= k, which no caller stores or publishes.)
        for (int x = 0; x < cnt; x++) {
            const double wv = (RHS || SCALE) ? sw[buf][x] : 1.0;
            const double w = SCALE ? wv : 1.0;
            const double c = rhs_mode == CSRK_ALS_RHS_ONES ? 1.0 : (rhs_mode == CSRK_ALS_RHS_VALUES ? wv : 1.0 + wv);
#pragma unroll
            for (int r = 0; r < TPT; r++) {
                const f64x2_t a0 = *(const f64x2_t *)&sv[buf][x][p0[r]], a1 = *(const f64x2_t *)&sv[buf][x][p0[r] + 2];
                const f64x2_t b0 = *(const f64x2_t *)&sv[buf][x][q0[r]], b1 = *(const f64x2_t *)&sv[buf][x][q0[r] + 2];
                const double vp[GT_B] = {a0.x, a0.y, a1.x, a1.y}, vq[GT_B] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
                for (int i = 0; i < GT_B; i++) {
                    const double t = SCALE ? __dmul_rn(w, vp[i]) : vp[i];
#pragma unroll
                    for (int j = 0; j < GT_B; j++) acc[r][i][j] = __builtin_fma(t, vq[j], acc[r][i][j]);
                }
            }
            if (RHS && tid < k) b = __builtin_fma(c, sv[buf][x][tid], b);
        }
    }
}

// ---- host side: the row range and the k classes' limit; stem, "csrk_gram" or "csrk_als", is what the UNSUPPORTED message names
static int gt_check_rows(const char *stem, const Matrix *m, int32_t row_begin, int32_t row_end, int32_t k)
{
    CSRK_CHECK_ROW_RANGE("", row_begin, row_end, m->nrows);
    if (k > GT_K_MAX) {
        set_error("%s_rows: k=%d is above the largest supported k=%d (%s_limits)", stem, k, GT_K_MAX, stem);
        return CSRK_ERR_UNSUPPORTED;
    }
    return CSRK_OK;
}

}  // namespace csrk
