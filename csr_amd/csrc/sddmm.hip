// Sampled dense-dense product (SDDMM) for libcsrk on gfx950: for every stored entry e = (i, j) of a CSR pattern S,
//     out[e] = dot(U[i, :], V[j, :])                      (scale = 0)
//     out[e] = S.values[e] * dot(U[i, :], V[j, :])        (scale = 1; a structure-only S counts as 1.0)
// with U dense row-major [nrows x k], V dense row-major [ncols x k], both float64 or both float32, out float64.  The
// reference has no such entry (its mult_ab is sparse x sparse only); it is the transpose-dual of the dense-panel SpMM
// (spmm_dense.hip): every stored entry gathers one k-wide row of a dense panel by its column index, but nothing is
// reduced ACROSS entries, so there are no partial panels, no heavy-row plan and no atomics.
//
// Work split.  Over entries, not rows: a group of 16 lanes (one DPP row) owns a fixed run of SD_RUN consecutive
// entries, four groups per wavefront.  A group finds the row of its first entry with a 16-way search in rowptrs
// (16 probes per step, one per lane, a ballot picks the interval: ~6 dependent loads for 2M rows), then keeps a window
// of the next 16 row ends in registers: the row of each further entry is the window's count of row ends <= e (one
// ballot, no load); a window that runs out (16 rows crossed, i.e. empty rows) is replaced by another search from its
// end.  So empty rows and rows shorter than a run cost O(entries + rows) in all, and long runs of empty rows cost a
// logarithmic search, not a walk.  U[i, :] is loaded when the row changes and kept in registers while consecutive
// entries stay in row i (k <= SD_KREG); four entries' V rows (float32: eight) are gathered per group per step (16 or
// 32 V rows in flight per wavefront at k <= 64), in 16-B pieces when the panels' base pointers and strides allow it,
// else element by element.
//
// Order of addition (fixed: it depends on k and the panel dtype only -- not on the entry's position, its row's length,
// the pointer width, the strides, the load form, the stream or the launch).  Lane l (0..15) of a group owns, in each
// 64-column chunk c = 0, 1, ..., four panel columns (those below k): float64 64 c + {2 l, 2 l + 1, 32 + 2 l, 33 + 2 l},
// float32 64 c + {4 l, .., 4 l + 3} (panel_off and panel_load4 in device_loads.h, which ALS-CG uses too).  Its partial
// sum starts at +0.0 and takes its columns in ascending order, one
// fused multiply-add each: s_l = fma(u_t, v_t, s_l).  (With float32 panels u_t and v_t are widened to float64 first;
// their product is exact in float64, so each step is one rounding of s_l + u_t v_t.)  The 16 partials are then added
// by the DPP tree of rows shifted right by 1, 2, 4, 8 (lane 15 of the row ends holding ((s_15 + s_14) + (s_13 + s_12))
// + ... in that fixed shape).  With scale = 1 the value (float32 widened, 1.0 when there are none) multiplies the sum
// once, after it.
#include "common.h"
#include "device_loads.h"
#include "panel.h"
#include "wave.h"

namespace csrk {

constexpr int SD_G = 16;                 // lanes per group (one DPP row)
static_assert(SD_G == PANEL_G, "a group is the lanes that share a panel row (device_loads.h)");
constexpr int SD_GROUPS = WAVE / SD_G;   // 4 groups per wavefront
constexpr int SD_RUN = 64;               // consecutive entries per group
constexpr int SD_THREADS = 256;
constexpr int SD_KREG = 256;             // k up to this: U's row held in registers (4 chunks of 64 columns)

// this group's 16 bits of a wavefront ballot
__device__ __forceinline__ int sd_group_count(bool pred, int grp)
{
    const unsigned long long b = __ballot(pred);
    return __popcll((b >> (grp * SD_G)) & 0xffffull);
}

// probe s (0..15) strictly inside (lo, hi), non-decreasing in s; span = hi - lo >= 2
__device__ __forceinline__ int64_t sd_probe(int64_t lo, int64_t span, int s)
{
    if (span - 1 <= SD_G) return lo + 1 + (s < span - 2 ? s : span - 2);
    return lo + 1 + ((int64_t)s * (span - 2)) / (SD_G - 1);
}

// The row r in [lo, hi) with rp[r] <= e < rp[r + 1], given rp[lo] <= e < rp[hi]: 16 probes per step, one per lane of
// the group (group-uniform control flow; every lane returns the same row).
template <class P>
__device__ int64_t sd_find_row(const P *__restrict__ rp, int64_t lo, int64_t hi, int64_t e, int sub, int grp)
{
    while (hi - lo > 1) {
        const int64_t span = hi - lo;
        const bool le = (int64_t)rp[sd_probe(lo, span, sub)] <= e;
        const int c = sd_group_count(le, grp);             // probes form a prefix of <= e (rp is non-decreasing)
        const int64_t nlo = c > 0 ? sd_probe(lo, span, c - 1) : lo;
        const int64_t nhi = c < SD_G ? sd_probe(lo, span, c) : hi;
        lo = nlo;
        hi = nhi;
    }
    return lo;
}

// the fixed order of addition (header comment): a lane's partial over its columns, then the group's DPP tree
template <class T>
__device__ __forceinline__ double sd_partial(double s, const T u[4], const T v[4], int sub, int kk)
{
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (panel_off<T>(sub, q) < kk) s = __builtin_fma((double)u[q], (double)v[q], s);
    return s;
}

__device__ __forceinline__ double sd_group_sum(double s)      // lane 15 of the group gets the sum
{
    s += dpp_f64<DPP_ROW_SHR1>(0.0, s);
    s += dpp_f64<DPP_ROW_SHR2>(0.0, s);
    s += dpp_f64<DPP_ROW_SHR4>(0.0, s);
    s += dpp_f64<DPP_ROW_SHR8>(0.0, s);
    return s;
}

// NCH > 0: k <= 64 NCH, U's row in registers (NCH chunks of 64 columns).  NCH == 0: any k, U's chunks re-read per entry.
// A step takes UN entries per group: their U rows (only where the row changes) and V rows are all loaded before the first
// is used, the step's values and the next step's column indices are fetched behind them, so a step waits for one round trip.
// UN * NC * 4 elements per lane and step: 8 KiB of V rows in flight per wavefront at k <= 64 for either panel type.
template <class P, class T, bool WIDE, int NCH>
__global__ __launch_bounds__(SD_THREADS) void sddmm_kernel(const P *__restrict__ rp, const int32_t *__restrict__ ci,
                                                           const void *__restrict__ vals, int vt, int64_t nrows, int64_t nnz,
                                                           const T *__restrict__ U, int64_t ldu, const T *__restrict__ V,
                                                           int64_t ldv, int32_t k, double *__restrict__ out)
{
    constexpr int UN = (NCH == 4 ? 1 : (NCH == 2 ? 2 : 4)) * (sizeof(T) == 4 ? 2 : 1);
    constexpr int NC = NCH > 0 ? NCH : 1;                 // chunks per pass
    const int lane = threadIdx.x & (WAVE - 1), grp = lane / SD_G, sub = lane % SD_G;
    const int64_t gid = ((int64_t)blockIdx.x * (SD_THREADS / WAVE) + threadIdx.x / WAVE) * SD_GROUPS + grp;
    const int64_t e0 = gid * SD_RUN;
    if (e0 >= nnz) return;                                // (group-uniform from here on)
    const int64_t e1 = e0 + SD_RUN < nnz ? e0 + SD_RUN : nnz;

    int32_t coln[UN];                                     // the next step's column indices
#pragma unroll
    for (int x = 0; x < UN; x++) coln[x] = ci[e0 + x < e1 ? e0 + x : e1 - 1];
    int32_t wbase = (int32_t)sd_find_row(rp, 0, nrows, e0, sub, grp);      // (rows fit int32: csrk.h)
    int64_t wend = (int64_t)rp[(int64_t)wbase + 1 + sub < nrows ? (int64_t)wbase + 1 + sub : nrows];      // window: rp[wbase + 1 + sub]
    int32_t urow = -1;
    T u[NC][4];                                           // U's row urow
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
        for (int q = 0; q < 4; q++) u[c][q] = (T)0;
    const int nchunks = (k + 63) / 64;

    for (int64_t e = e0; e < e1; e += UN) {
        int32_t col[UN];
        double a[UN];
#pragma unroll
        for (int x = 0; x < UN; x++) col[x] = coln[x];      // (past the run: its last entry again, result dropped)
        // the rows of the step's entries: the window's count of row ends <= e
        int32_t row[UN];
#pragma unroll
        for (int x = 0; x < UN; x++) {
            if (e + x >= e1) {
                row[x] = row[x > 0 ? x - 1 : 0];
                continue;
            }
            int c = sd_group_count(wend <= e + x, grp);
            if (c == SD_G) {                              // 16 rows crossed (empty rows): search from the window's end
                wbase = (int32_t)sd_find_row(rp, (int64_t)wbase + SD_G, nrows, e + x, sub, grp);
                wend = (int64_t)rp[(int64_t)wbase + 1 + sub < nrows ? (int64_t)wbase + 1 + sub : nrows];
                c = 0;
            }
            const int64_t r = (int64_t)wbase + c;
            row[x] = (int32_t)(r < nrows - 1 ? r : nrows - 1);
        }
        double acc[UN];
#pragma unroll
        for (int x = 0; x < UN; x++) acc[x] = 0.0;
        if constexpr (NCH > 0) {
            T uw[UN][NC][4], v[UN][NC][4];
#pragma unroll
            for (int x = 0; x < UN; x++) {
                const int32_t prev = x > 0 ? row[x - 1] : urow;
                if (row[x] != prev) {                     // group-uniform: a new row's U
#pragma unroll
                    for (int c = 0; c < NC; c++)
                        panel_load4<T, WIDE>(U + (int64_t)row[x] * ldu + 64 * c, sub, k - 64 * c, uw[x][c]);
                } else {
#pragma unroll
                    for (int c = 0; c < NC; c++)
#pragma unroll
                        for (int q = 0; q < 4; q++) uw[x][c][q] = x > 0 ? uw[x > 0 ? x - 1 : 0][c][q] : u[c][q];
                }
            }
#pragma unroll
            for (int x = 0; x < UN; x++)
#pragma unroll
                for (int c = 0; c < NC; c++)
                    panel_load4<T, WIDE>(V + (int64_t)col[x] * ldv + 64 * c, sub, k - 64 * c, v[x][c]);
#pragma unroll
            for (int x = 0; x < UN; x++) {
                a[x] = csr_val(vals, vt, e + x < e1 ? e + x : e1 - 1);      // (in flight with the V rows)
                coln[x] = ci[e + UN + x < e1 ? e + UN + x : e1 - 1];
            }
#pragma unroll
            for (int x = 0; x < UN; x++)
#pragma unroll
                for (int c = 0; c < NC; c++) acc[x] = sd_partial<T>(acc[x], uw[x][c], v[x][c], sub, k - 64 * c);
            urow = row[UN - 1];
#pragma unroll
            for (int c = 0; c < NC; c++)
#pragma unroll
                for (int q = 0; q < 4; q++) u[c][q] = uw[UN - 1][c][q];
        } else {
#pragma unroll
            for (int x = 0; x < UN; x++) {
                a[x] = csr_val(vals, vt, e + x < e1 ? e + x : e1 - 1);      // (in flight with the V rows)
                coln[x] = ci[e + UN + x < e1 ? e + UN + x : e1 - 1];
            }
            for (int c = 0; c < nchunks; c++) {
                T v[UN][4], w[UN][4];
#pragma unroll
                for (int x = 0; x < UN; x++) {
                    panel_load4<T, WIDE>(V + (int64_t)col[x] * ldv + 64 * c, sub, k - 64 * c, v[x]);
                    panel_load4<T, WIDE>(U + (int64_t)row[x] * ldu + 64 * c, sub, k - 64 * c, w[x]);
                }
#pragma unroll
                for (int x = 0; x < UN; x++) acc[x] = sd_partial<T>(acc[x], w[x], v[x], sub, k - 64 * c);
            }
        }
#pragma unroll
        for (int x = 0; x < UN; x++) {
            const double s = sd_group_sum(acc[x]);
            if (sub == SD_G - 1 && e + x < e1) __builtin_nontemporal_store(vt == CSRK_VAL_NONE ? s : a[x] * s, out + e + x);
        }
    }
}

static int sddmm_check(int64_t ldu, int64_t ldv, int32_t k, int panel_type, int scale)
{
    CSRK_CHECK_K("", k);
    CSRK_CHECK_TWO_PANELS("", k, ldu, ldv);
    CSRK_CHECK_PANEL_TYPE("", panel_type);
    CSRK_CHECK_SCALE(scale);
    return CSRK_OK;
}

static int sddmm_device(Matrix *m, const void *dU, int64_t ldu, const void *dV, int64_t ldv, int32_t k, int panel_type,
                        int scale, double *dout, hipStream_t s)
{
    CSRK_TRY(sddmm_check(ldu, ldv, k, panel_type, scale));
    if (m->nnz == 0 || m->nrows == 0) return CSRK_OK;
    CSRK_REQUIRE(dU && dV && dout, "U, V or out is NULL");
    const size_t es = panel_es(panel_type);
    CSRK_REQUIRE(((uintptr_t)dU % es) == 0 && ((uintptr_t)dV % es) == 0 && ((uintptr_t)dout % 8) == 0,
                 "U, V or out is not aligned to its element size");
    mark_user_stream(m, s);
    // 16-B loads when every lane's four columns start 16-B aligned: base pointers 16-B aligned, strides a multiple of
    // 16 B.  Otherwise element loads (8 B for float64, 4 B for float32): the same products in the same order.
    const bool wide = panel_16b(dU, ldu, es) && panel_16b(dV, ldv, es);
    const int vt = scale ? m->val_type : CSRK_VAL_NONE;
    const int64_t groups = ceil_div(m->nnz, SD_RUN);
    const unsigned grid = (unsigned)ceil_div(groups, (int64_t)(SD_THREADS / WAVE) * SD_GROUPS);
#define SD_GO(P, T, W, NCH)                                                                                            \
    sddmm_kernel<P, T, W, NCH><<<grid, SD_THREADS, 0, s>>>((const P *)m->d_rowptrs, m->d_colinds, m->d_values, vt,      \
                                                          (int64_t)m->nrows, m->nnz, (const T *)dU, ldu, (const T *)dV, \
                                                          ldv, k, dout)
#define SD_NCH(P, T, W)                                                                                                \
    do {                                                                                                               \
        if (k <= 64) SD_GO(P, T, W, 1);                                                                                \
        else if (k <= 128) SD_GO(P, T, W, 2);                                                                          \
        else if (k <= SD_KREG) SD_GO(P, T, W, 4);                                                                      \
        else SD_GO(P, T, W, 0);                                                                                        \
    } while (0)
#define SD_W(P, T)                                                                                                     \
    do {                                                                                                               \
        if (wide) SD_NCH(P, T, true);                                                                                  \
        else SD_NCH(P, T, false);                                                                                      \
    } while (0)
    if (m->ptr64) {
        if (panel_type == CSRK_VAL_F64) SD_W(int64_t, double);
        else SD_W(int64_t, float);
    } else {
        if (panel_type == CSRK_VAL_F64) SD_W(int32_t, double);
        else SD_W(int32_t, float);
    }
#undef SD_W
#undef SD_NCH
#undef SD_GO
    CSRK_LAUNCH_CHECK();
    return CSRK_OK;
}

}  // namespace csrk

using namespace csrk;

extern "C" {

int csrk_sddmm_device(csrk_handle_t h, const void *d_U, int64_t ldu, const void *d_V, int64_t ldv, int32_t k, int panel_type,
                      int scale, double *d_out, void *stream)
{
    Matrix *m = from_handle(h);
    if (!m) return CSRK_ERR_INVALID;
    return sddmm_device(m, d_U, ldu, d_V, ldv, k, panel_type, scale, d_out, (hipStream_t)stream);
}

int csrk_sddmm(csrk_handle_t h, const void *U, int64_t ldu, const void *V, int64_t ldv, int32_t k, int panel_type, int scale,
               double *out)
{
    Matrix *m = from_handle(h);
    if (!m) return CSRK_ERR_INVALID;
    // argument checks first, with the caller's pointers (the device call below sees packed copies)
    CSRK_TRY(sddmm_check(ldu, ldv, k, panel_type, scale));
    if (m->nnz == 0 || m->nrows == 0) return CSRK_OK;
    CSRK_REQUIRE(U && V && out, "U, V or out is NULL");
    const size_t es = panel_es(panel_type);
    DevBuf dU, dV, dO;
    CSRK_TRY(pack_panel(dU, U, ldu, k, es, m->nrows));
    CSRK_TRY(pack_panel(dV, V, ldv, k, es, m->ncols));
    CSRK_TRY(dO.alloc((size_t)m->nnz * 8));
    CSRK_TRY(sddmm_device(m, dU.p, k, dV.p, k, k, panel_type, scale, dO.as<double>(), nullptr));
    CSRK_HIP(hipMemcpy(out, dO.p, (size_t)m->nnz * 8, hipMemcpyDeviceToHost));
    return CSRK_OK;
}

}  // extern "C"
