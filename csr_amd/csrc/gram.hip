// Per-row Gram matrices for libcsrk on gfx950: for every row i of a CSR matrix in [row_begin, row_end),
//     G_i = base + sum over the row's stored entries e = (i, j), in storage order, of w_e v_j v_j^T        (k x k, float64)
// with v_j = V[j, :] a row of a dense row-major panel [ncols x k] (float32 or float64) and w_e = 1 (scale = 0) or the
// entry's value (scale = 1; a structure-only matrix counts as 1.0).  It is the left-hand side of the normal equations of
// alternating least squares; the reference has no such entry.  The gather is SDDMM's (sddmm.hip: a k-wide panel row per
// stored entry, by its column index), the reduction runs the other way: across a row's entries into a dense block.
//
// Arithmetic (include/csrk.h, rule 2): for p >= q, G[p][q] starts at base[p][q] (or +0.0) and takes one step per entry,
// t = round(w * V[j][p]), G[p][q] = fma(t, V[j][q], G[p][q]); then G[q][p] = G[p][q].  Every element is a serial chain over
// its row's entries, so nothing about the launch can change a bit of it: parallelism is over rows and over the elements
// of the lower triangle, never over a row's entries.  No atomics, no split sums.
//
// Work split.  A TEAM of threads owns a row: 16 lanes for k <= 16, a wavefront for k <= 40, a 256-thread workgroup above.
// The lower triangle is cut into 4 x 4 register tiles (tile (bp, bq), bq <= bp, holds p = 4 bp .. 4 bp + 3, q = 4 bq ..
// 4 bq + 3); a thread keeps one tile (k <= 88) or up to three (k <= 128) in registers for the whole row.  The row's V rows
// go through LDS GR_STAGE entries per step, widened to float64, in two buffers: while a step is consumed the next step's V
// rows and weights are in flight to registers and the column indices of the step after that are in flight behind them, so
// a step waits for one round trip at most (SDDMM's discipline).  Per staged entry a tile reads its four p- and four q-
// operands from LDS (four 16-B reads) for four rounded multiplies and sixteen fused multiply-adds; the strictly upper part of
// a diagonal tile is computed and dropped.  V is read in 16-B pieces when its base pointer, ldv and k allow whole
// pieces, else element by element: the same bits.  Output offsets are 64-bit.
#include "common.h"

namespace csrk {

constexpr int GR_THREADS = 256;
constexpr int GR_STAGE = 8;                      // entries staged per step
constexpr int GR_B = 4;                          // register tile edge
constexpr int GR_K_SUB = 16;                     // k up to this: 16 lanes per row
constexpr int GR_K_WAVE = 40;                    // k up to this: a wavefront per row
constexpr int GR_K_ONE = 88;                     // k up to this: a workgroup per row, one tile per thread
constexpr int GR_K_MAX = 128;                    // k up to this: a workgroup per row, up to three tiles per thread

template <int CLS> struct GrClass;
template <> struct GrClass<0> { static constexpr int TEAM = 16, KMAX = GR_K_SUB, TPT = 1; };
template <> struct GrClass<1> { static constexpr int TEAM = 64, KMAX = GR_K_WAVE, TPT = 1; };
template <> struct GrClass<2> { static constexpr int TEAM = 256, KMAX = GR_K_ONE, TPT = 1; };
template <> struct GrClass<3> { static constexpr int TEAM = 256, KMAX = GR_K_MAX, TPT = 3; };

typedef double gr_d2 __attribute__((ext_vector_type(2)));
typedef float gr_f4 __attribute__((ext_vector_type(4)));

// one unit of a panel row as float64: PER elements (a 16-B piece when PER > 1, else one element)
template <class T, int PER> __device__ __forceinline__ void gr_load(const T *__restrict__ p, double d[PER]);
template <> __device__ __forceinline__ void gr_load<double, 1>(const double *__restrict__ p, double d[1]) { d[0] = *p; }
template <> __device__ __forceinline__ void gr_load<float, 1>(const float *__restrict__ p, double d[1]) { d[0] = (double)*p; }
template <> __device__ __forceinline__ void gr_load<double, 2>(const double *__restrict__ p, double d[2])
{
    const gr_d2 a = *(const gr_d2 *)p;
    d[0] = a.x, d[1] = a.y;
}
template <> __device__ __forceinline__ void gr_load<float, 4>(const float *__restrict__ p, double d[4])
{
    const gr_f4 a = *(const gr_f4 *)p;
    d[0] = (double)a.x, d[1] = (double)a.y, d[2] = (double)a.z, d[3] = (double)a.w;
}

// the team's threads have all written their LDS words before any of them reads (a team never spans workgroups)
template <int TEAM> __device__ __forceinline__ void gr_team_sync()
{
    if constexpr (TEAM > WAVE) {
        __syncthreads();
    } else {      // within one wavefront LDS operations complete in issue order: order the compiler and the counters
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

template <class T, bool WIDE, int CLS, bool SCALE>
__global__ __launch_bounds__(GR_THREADS) void gram_kernel(const void *__restrict__ rp, int ptr64, const int32_t *__restrict__ ci,
                                                          const void *__restrict__ vals, int vt, int32_t row_begin, int32_t row_end,
                                                          const T *__restrict__ V, int64_t ldv, int32_t k,
                                                          const double *__restrict__ base, double *__restrict__ out)
{
    typedef GrClass<CLS> C;
    constexpr int TEAM = C::TEAM, KP = C::KMAX, TPT = C::TPT, TEAMS = GR_THREADS / TEAM;
    constexpr int PER = WIDE ? 16 / (int)sizeof(T) : 1;                     // elements per load
    constexpr int NL = (GR_STAGE * (KP / PER) + TEAM - 1) / TEAM;           // loads per thread and step
    __shared__ __attribute__((aligned(16))) double sv[TEAMS][2][GR_STAGE][KP];
    __shared__ double sw[TEAMS][2][GR_STAGE];

    const int team = threadIdx.x / TEAM, tid = threadIdx.x % TEAM;
    const int64_t row = (int64_t)row_begin + (int64_t)blockIdx.x * TEAMS + team;
    if (TEAM < GR_THREADS && row >= row_end) return;                        // (a whole team; teams never meet at a barrier)
    const int64_t e0 = ptr64 ? ((const int64_t *)rp)[row] : (int64_t)((const int32_t *)rp)[row];
    const int64_t e1 = ptr64 ? ((const int64_t *)rp)[row + 1] : (int64_t)((const int32_t *)rp)[row + 1];

    // this thread's tiles of the lower triangle
    const int nb = (k + GR_B - 1) / GR_B, ntiles = nb * (nb + 1) / 2;
    int p0[TPT], q0[TPT];
    bool has[TPT];
    double acc[TPT][GR_B][GR_B];
#pragma unroll
    for (int r = 0; r < TPT; r++) {
        const int t = tid + r * TEAM;
        has[r] = t < ntiles;
        int b = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
        while (b * (b + 1) / 2 > t) b--;
        while ((b + 1) * (b + 2) / 2 <= t) b++;
        p0[r] = has[r] ? GR_B * b : 0;
        q0[r] = has[r] ? GR_B * (t - b * (b + 1) / 2) : 0;
#pragma unroll
        for (int i = 0; i < GR_B; i++)
#pragma unroll
            for (int j = 0; j < GR_B; j++) {
                const int p = p0[r] + i, q = q0[r] + j;
                acc[r][i][j] = (has[r] && base && p < k && q <= p) ? base[(int64_t)p * k + q] : 0.0;
            }
    }

    // this thread's share of a step: unit x = tid + l TEAM is piece x % upr of staged entry x / upr
    const int upr = k / PER;                                                // units per panel row (WIDE: k is a whole number of pieces)
    int ue[NL], uo[NL];
#pragma unroll
    for (int l = 0; l < NL; l++) {
        const int x = tid + l * TEAM;
        ue[l] = x / upr;                                                    // (>= GR_STAGE: no such unit)
        uo[l] = (x % upr) * PER;
    }
    const int64_t last = e1 - 1;
    int32_t coln[NL] = {};                                                  // (only this thread's units are loaded)
    double vreg[NL][PER], wreg = 1.0;
    if (e0 < e1) {
#pragma unroll
        for (int l = 0; l < NL; l++) {
            const int64_t e = e0 + ue[l];
            if (ue[l] < GR_STAGE) coln[l] = ci[e < last ? e : last];
        }
#pragma unroll
        for (int l = 0; l < NL; l++)
            if (ue[l] < GR_STAGE) gr_load<T, PER>(V + (int64_t)coln[l] * ldv + uo[l], vreg[l]);
        if (SCALE && tid < GR_STAGE) {
            const int64_t e = e0 + tid < last ? e0 + tid : last;
            wreg = vt == CSRK_VAL_F64 ? ((const double *)vals)[e] : (double)((const float *)vals)[e];
        }
#pragma unroll
        for (int l = 0; l < NL; l++) {
            const int64_t e = e0 + GR_STAGE + ue[l];
            if (ue[l] < GR_STAGE) coln[l] = ci[e < last ? e : last];
        }
    }

    int buf = 0;
    for (int64_t es = e0; es < e1; es += GR_STAGE, buf ^= 1) {
        const int cnt = e1 - es < GR_STAGE ? (int)(e1 - es) : GR_STAGE;
        // this step's V rows and weights: registers -> LDS  (entries past the row's end hold its last entry again, unused)
#pragma unroll
        for (int l = 0; l < NL; l++)
            if (ue[l] < GR_STAGE) {
#pragma unroll
                for (int x = 0; x < PER; x++) sv[team][buf][ue[l]][uo[l] + x] = vreg[l][x];
            }
        if (SCALE && tid < GR_STAGE) sw[team][buf][tid] = wreg;
        gr_team_sync<TEAM>();
        // the next step's V rows and weights and the column indices of the step after it, in flight while this one is used
        if (es + GR_STAGE < e1) {
#pragma unroll
            for (int l = 0; l < NL; l++)
                if (ue[l] < GR_STAGE) gr_load<T, PER>(V + (int64_t)coln[l] * ldv + uo[l], vreg[l]);
            if (SCALE && tid < GR_STAGE) {
                const int64_t e = es + GR_STAGE + tid < last ? es + GR_STAGE + tid : last;
                wreg = vt == CSRK_VAL_F64 ? ((const double *)vals)[e] : (double)((const float *)vals)[e];
            }
#pragma unroll
            for (int l = 0; l < NL; l++) {
                const int64_t e = es + 2 * GR_STAGE + ue[l];
                if (ue[l] < GR_STAGE) coln[l] = ci[e < last ? e : last];
            }
        }
        // the staged entries in storage order: t = round(w v_p), G[p][q] = fma(t, v_q, G[p][q]).  (Columns k .. 4 nb - 1 of a
        // staged row are never written: an edge tile reads whatever LDS holds there into accumulators with p >= k or
        // q >= k, which the stores below leave out.)
        for (int x = 0; x < cnt; x++) {
            const double w = SCALE ? sw[team][buf][x] : 1.0;
#pragma unroll
            for (int r = 0; r < TPT; r++) {
                const gr_d2 a0 = *(const gr_d2 *)&sv[team][buf][x][p0[r]], a1 = *(const gr_d2 *)&sv[team][buf][x][p0[r] + 2];
                const gr_d2 b0 = *(const gr_d2 *)&sv[team][buf][x][q0[r]], b1 = *(const gr_d2 *)&sv[team][buf][x][q0[r] + 2];
                const double vp[GR_B] = {a0.x, a0.y, a1.x, a1.y}, vq[GR_B] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
                for (int i = 0; i < GR_B; i++) {
                    const double t = SCALE ? __dmul_rn(w, vp[i]) : vp[i];
#pragma unroll
                    for (int j = 0; j < GR_B; j++) acc[r][i][j] = __builtin_fma(t, vq[j], acc[r][i][j]);
                }
            }
        }
    }

    double *__restrict__ g = out + (int64_t)(row - row_begin) * k * k;      // (64-bit: the block of rows may pass 2^31 elements)
#pragma unroll
    for (int r = 0; r < TPT; r++) {
        if (!has[r]) continue;
#pragma unroll
        for (int i = 0; i < GR_B; i++)                                      // the lower triangle: runs along q
#pragma unroll
            for (int j = 0; j < GR_B; j++) {
                const int p = p0[r] + i, q = q0[r] + j;
                if (p < k && q <= p) g[(int64_t)p * k + q] = acc[r][i][j];
            }
#pragma unroll
        for (int j = 0; j < GR_B; j++)                                      // its mirror: runs along p
#pragma unroll
            for (int i = 0; i < GR_B; i++) {
                const int p = p0[r] + i, q = q0[r] + j;
                if (p < k && q < p) g[(int64_t)q * k + p] = acc[r][i][j];
            }
    }
}

static int gram_check(Matrix *m, int32_t row_begin, int32_t row_end, int64_t ldv, int32_t k, int panel_type, int scale)
{
    CSRK_REQUIRE(k >= 1, "k must be at least 1 (k=%d)", k);
    CSRK_REQUIRE(ldv >= k, "bad panel geometry k=%d ldv=%lld", k, (long long)ldv);
    CSRK_REQUIRE(panel_type == CSRK_VAL_F32 || panel_type == CSRK_VAL_F64, "panel_type must be CSRK_VAL_F32 or CSRK_VAL_F64, not %d",
                 panel_type);
    CSRK_REQUIRE(scale == 0 || scale == 1, "scale must be 0 or 1, not %d", scale);
    CSRK_REQUIRE(row_begin >= 0 && row_begin <= row_end && row_end <= m->nrows, "bad row range [%d, %d) of %d rows", row_begin,
                 row_end, m->nrows);
    if (k > GR_K_MAX) {
        set_error("csrk_gram_rows: k=%d is above the largest supported k=%d (csrk_gram_limits)", k, GR_K_MAX);
        return CSRK_ERR_UNSUPPORTED;
    }
    return CSRK_OK;
}

static int gram_device(Matrix *m, int32_t row_begin, int32_t row_end, const void *dV, int64_t ldv, int32_t k, int panel_type,
                       int scale, const double *dbase, double *dout, hipStream_t s)
{
    CSRK_TRY(gram_check(m, row_begin, row_end, ldv, k, panel_type, scale));
    if (row_begin == row_end) return CSRK_OK;
    CSRK_REQUIRE(dout && (dV || m->nnz == 0), "V or out is NULL");
    const size_t es = panel_type == CSRK_VAL_F64 ? 8 : 4;
    CSRK_REQUIRE(((uintptr_t)dV % es) == 0 && ((uintptr_t)dout % 8) == 0 && ((uintptr_t)dbase % 8) == 0,
                 "V, base or out is not aligned to its element size");
    {
        std::lock_guard<std::mutex> lk(m->mu);
        if (s) m->used_user_stream = true;
    }
    // 16-B loads when every piece of every panel row is whole and 16-B aligned; else element loads: the same bits
    const int64_t per16 = (int64_t)(16 / es);
    const bool wide = ((uintptr_t)dV & 15) == 0 && ldv % per16 == 0 && k % per16 == 0;
    const bool scaled = scale && m->val_type != CSRK_VAL_NONE;      // (a structure-only matrix: w = 1.0, as scale = 0)
    const int64_t n = (int64_t)row_end - row_begin;
#define GR_GO(T, W, CLS, SC)                                                                                            \
    gram_kernel<T, W, CLS, SC><<<(unsigned)ceil_div(n, GR_THREADS / GrClass<CLS>::TEAM), GR_THREADS, 0, s>>>(           \
        m->d_rowptrs, m->ptr64, m->d_colinds, m->d_values, m->val_type, row_begin, row_end, (const T *)dV, ldv, k, dbase, dout)
#define GR_SC(T, W, CLS)                                                                                                \
    do {                                                                                                               \
        if (scaled) GR_GO(T, W, CLS, true);                                                                            \
        else GR_GO(T, W, CLS, false);                                                                                  \
    } while (0)
#define GR_CLS(T, W)                                                                                                   \
    do {                                                                                                               \
        if (k <= GR_K_SUB) GR_SC(T, W, 0);                                                                             \
        else if (k <= GR_K_WAVE) GR_SC(T, W, 1);                                                                       \
        else if (k <= GR_K_ONE) GR_SC(T, W, 2);                                                                        \
        else GR_SC(T, W, 3);                                                                                           \
    } while (0)
    if (panel_type == CSRK_VAL_F64) {
        if (wide) GR_CLS(double, true);
        else GR_CLS(double, false);
    } else {
        if (wide) GR_CLS(float, true);
        else GR_CLS(float, false);
    }
#undef GR_CLS
#undef GR_SC
#undef GR_GO
    CSRK_LAUNCH_CHECK();
    return CSRK_OK;
}

}  // namespace csrk

using namespace csrk;

extern "C" {

int csrk_gram_limits(int64_t *out, int n)
{
    CSRK_REQUIRE(out && n >= 0, "csrk_gram_limits: out is NULL or n < 0");
    const int64_t v[5] = {GR_K_MAX, GR_STAGE, GR_K_SUB, GR_K_WAVE, GR_K_ONE};
    for (int i = 0; i < n && i < 5; i++) out[i] = v[i];
    return CSRK_OK;
}

int csrk_gram_rows_device(csrk_handle_t h, int32_t row_begin, int32_t row_end, const void *d_V, int64_t ldv, int32_t k,
                          int panel_type, int scale, const double *d_base, double *d_out, void *stream)
{
    Matrix *m = from_handle(h);
    if (!m) return CSRK_ERR_INVALID;
    return gram_device(m, row_begin, row_end, d_V, ldv, k, panel_type, scale, d_base, d_out, (hipStream_t)stream);
}

int csrk_gram_rows(csrk_handle_t h, int32_t row_begin, int32_t row_end, const void *V, int64_t ldv, int32_t k, int panel_type,
                   int scale, const double *base, double *out)
{
    Matrix *m = from_handle(h);
    if (!m) return CSRK_ERR_INVALID;
    // argument checks first, with the caller's pointers (the device call below sees packed copies)
    CSRK_TRY(gram_check(m, row_begin, row_end, ldv, k, panel_type, scale));
    if (row_begin == row_end) return CSRK_OK;
    CSRK_REQUIRE(out && (V || m->nnz == 0), "V or out is NULL");
    const size_t es = panel_type == CSRK_VAL_F64 ? 8 : 4;
    const size_t nout = (size_t)(row_end - row_begin) * k * k * 8;
    // the panel travels packed (ld = k): the bits do not depend on the stride
    DevBuf dV, dB, dO;
    CSRK_TRY(dV.alloc((size_t)m->ncols * k * es));
    CSRK_TRY(dO.alloc(nout));
    if (m->ncols && V)
        CSRK_HIP(hipMemcpy2D(dV.p, (size_t)k * es, V, (size_t)ldv * es, (size_t)k * es, m->ncols, hipMemcpyHostToDevice));
    if (base) {
        CSRK_TRY(dB.alloc((size_t)k * k * 8));
        CSRK_HIP(hipMemcpy(dB.p, base, (size_t)k * k * 8, hipMemcpyHostToDevice));
    }
    CSRK_TRY(gram_device(m, row_begin, row_end, dV.p, k, k, panel_type, scale, base ? dB.as<double>() : nullptr, dO.as<double>(),
                         nullptr));
    CSRK_HIP(hipMemcpy(out, dO.p, nout, hipMemcpyDeviceToHost));
    return CSRK_OK;
}

}  // extern "C"
