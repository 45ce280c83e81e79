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
// The k classes, the 4 x 4 register tiles of the lower triangle and the walk over a row's entries (gt_accumulate) are
// gram_tile.h's, which als.hip runs too; here are the kernel around them -- the tiles start from base and are stored twice,
// as the lower triangle and as its mirror -- and the entry points.  Output offsets are 64-bit.
#include "gram_tile.h"

namespace csrk {

template <class T, bool WIDE, int CLS, bool SCALE>
__global__ __launch_bounds__(GT_THREADS) void gram_kernel(const void *__restrict__ rp, int ptr64, const int32_t *__restrict__ ci,
                                                          const void *__restrict__ vals, int vt, int32_t row_begin, int32_t row_end,
                                                          const T *__restrict__ V, int64_t ldv, int32_t k,
                                                          const double *__restrict__ base, double *__restrict__ out)
{
    typedef GramClass<CLS> C;
    constexpr int TEAM = C::TEAM, KP = C::KMAX, TPT = C::TPT, TEAMS = GT_THREADS / TEAM;
    __shared__ __attribute__((aligned(16))) double sv[TEAMS][2][GT_STAGE][KP];
    __shared__ double sw[TEAMS][2][GT_STAGE];

    const int team = threadIdx.x / TEAM, tid = threadIdx.x % TEAM;
    const int64_t row = (int64_t)row_begin + (int64_t)blockIdx.x * TEAMS + team;
    if (TEAM < GT_THREADS && row >= row_end) return;                        // (a whole team; teams never meet at a barrier)
    const int64_t e0 = ptr64 ? ((const int64_t *)rp)[row] : (int64_t)((const int32_t *)rp)[row];
    const int64_t e1 = ptr64 ? ((const int64_t *)rp)[row + 1] : (int64_t)((const int32_t *)rp)[row + 1];

    // this thread's tiles of the lower triangle
    const int nb = (k + GT_B - 1) / GT_B, ntiles = nb * (nb + 1) / 2;
    int p0[TPT], q0[TPT];
    bool has[TPT];
    double acc[TPT][GT_B][GT_B];
#pragma unroll
    for (int r = 0; r < TPT; r++) {
        const int t = tid + r * TEAM;
        has[r] = t < ntiles;
        gt_tile(t, has[r], p0[r], q0[r]);
#pragma unroll
        for (int i = 0; i < GT_B; i++)
#pragma unroll
            for (int j = 0; j < GT_B; j++) {
                const int p = p0[r] + i, q = q0[r] + j;
                acc[r][i][j] = (has[r] && base && p < k && q <= p) ? base[(int64_t)p * k + q] : 0.0;
            }
    }

    double none = 0.0;                                                      // (no right-hand side here)
    gt_accumulate<T, WIDE, CLS, SCALE, false>(e0, e1, ci, vals, vt, V, ldv, k, 0, tid, sv[team], sw[team], acc, p0, q0, none);

    double *__restrict__ g = out + (int64_t)(row - row_begin) * k * k;      // (64-bit: the block of rows may pass 2^31 elements)
#pragma unroll
    for (int r = 0; r < TPT; r++) {
        if (!has[r]) continue;
#pragma unroll
        for (int i = 0; i < GT_B; i++)                                      // the lower triangle: runs along q
#pragma unroll
            for (int j = 0; j < GT_B; j++) {
                const int p = p0[r] + i, q = q0[r] + j;
                if (p < k && q <= p) g[(int64_t)p * k + q] = acc[r][i][j];
            }
#pragma unroll
        for (int j = 0; j < GT_B; j++)                                      // its mirror: runs along p
#pragma unroll
            for (int i = 0; i < GT_B; i++) {
                const int p = p0[r] + i, q = q0[r] + j;
                if (p < k && q < p) g[(int64_t)q * k + p] = acc[r][i][j];
            }
    }
}

static int gram_check(Matrix *m, int32_t row_begin, int32_t row_end, int64_t ldv, int32_t k, int panel_type, int scale)
{
    CSRK_CHECK_K("", k);
    CSRK_CHECK_ONE_PANEL(k, ldv);
    CSRK_CHECK_PANEL_TYPE("", panel_type);
    CSRK_CHECK_SCALE(scale);
    return gt_check_rows("csrk_gram", m, row_begin, row_end, k);
}

static int gram_device(Matrix *m, int32_t row_begin, int32_t row_end, const void *dV, int64_t ldv, int32_t k, int panel_type,
                       int scale, const double *dbase, double *dout, hipStream_t s)
{
    CSRK_TRY(gram_check(m, row_begin, row_end, ldv, k, panel_type, scale));
    if (row_begin == row_end) return CSRK_OK;
    CSRK_REQUIRE(dout && (dV || m->nnz == 0), "V or out is NULL");
    const size_t es = panel_es(panel_type);
    CSRK_REQUIRE(((uintptr_t)dV % es) == 0 && ((uintptr_t)dout % 8) == 0 && ((uintptr_t)dbase % 8) == 0,
                 "V, base or out is not aligned to its element size");
    mark_user_stream(m, s);
    const bool wide = panel_16b(dV, ldv, es) && k % panel_per16(es) == 0;
    const bool scaled = scale && m->val_type != CSRK_VAL_NONE;      // (a structure-only matrix: w = 1.0, as scale = 0)
    const int64_t n = (int64_t)row_end - row_begin;
#define GR_GO(T, W, CLS, SC)                                                                                            \
    gram_kernel<T, W, CLS, SC><<<(unsigned)ceil_div(n, GT_THREADS / GramClass<CLS>::TEAM), GT_THREADS, 0, s>>>(         \
        m->d_rowptrs, m->ptr64, m->d_colinds, m->d_values, m->val_type, row_begin, row_end, (const T *)dV, ldv, k, dbase, dout)
#define GR_SC(T, W, CLS)                                                                                                \
    do {                                                                                                               \
        if (scaled) GR_GO(T, W, CLS, true);                                                                            \
        else GR_GO(T, W, CLS, false);                                                                                  \
    } while (0)
#define GR_CLS(T, W)                                                                                                   \
    do {                                                                                                               \
        if (k <= GT_K_SUB) GR_SC(T, W, 0);                                                                             \
        else if (k <= GT_K_WAVE) GR_SC(T, W, 1);                                                                       \
        else if (k <= GT_K_ONE) GR_SC(T, W, 2);                                                                        \
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
    const int64_t v[5] = {GT_K_MAX, GT_STAGE, GT_K_SUB, GT_K_WAVE, GT_K_ONE};
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
    const size_t nout = (size_t)(row_end - row_begin) * k * k * 8;
    DevBuf dV, dB, dO;
    CSRK_TRY(pack_panel(dV, V, ldv, k, panel_es(panel_type), m->ncols));
    CSRK_TRY(dO.alloc(nout));
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
