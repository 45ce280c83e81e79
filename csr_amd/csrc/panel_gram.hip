// The Gram matrix of a dense panel for libcsrk on gfx950: G = V^T V + ridge I, k x k float64, from V [n x k] float32 or
// float64 (include/csrk.h, rule P).  Implicit-feedback ALS passes it as the `base` of csrk_als_rows[_cg]; until now the
// caller made it with a BLAS whose order of addition nobody states.  Here every element is a fixed chain of fused
// multiply-adds per chunk of PG_R rows and a fixed tree of rounded additions over the chunks.
//
// Work split.  ONE WORKGROUP PER CHUNK of PG_R consecutive rows (rule P2); the chunk length is a constant of the build,
// never a function of the card or the launch, because it decides where the chains are cut.  The lower triangle is cut
// into the 4 x 4 register tiles of gram_tile.h (the k classes, the tile numbering and the four 16-B LDS reads per tile and
// row are csrk_gram_rows'): a wavefront with one tile per thread for k <= 40, 256 threads with one tile for k <= 88, with
// up to three for k <= 128.  The chunk's rows go through LDS PG_S at a time, widened to float64, in two buffers: while a
// slice is consumed the next one is in flight to registers, one barrier per slice.  The rows of a chunk are consecutive in
// memory, so a slice is one contiguous span (ldv = k) or PG_S spans of k elements.  Per staged row a tile makes sixteen
// fused multiply-adds; the strictly upper part of a diagonal tile is computed and dropped.
//
// No matrix cores: v_mfma_f64_* adds four products per instruction in an order that is not documented as a chain, and
// rule P is bit for bit (as section 7 says for the panel product).
//
// The tree (rule P3).  Chunk c's partial is k x k doubles of the workspace (only t >= u is written or read).  The launches
// of tree_sum.h fold every aligned group of 32 partials into one, five levels of P3's tree at once, ping-ponging between
// the workspace's two regions until at most 32 are left; panel_gram_finish_kernel folds those, adds the ridge and writes
// both triangles of the output.  977 chunks (n = 2 000 000) take two tree launches.
#include "common.h"
#include "device_loads.h"
#include "gram_tile.h"
#include "panel.h"
#include "tree_sum.h"
#include "wave.h"

namespace csrk {

constexpr int PG_R = 2048;               // rows per chunk (rule P2; csrk_panel_gram_limits' out[1])
constexpr int PG_S = 16;                 // rows per staged slice
constexpr int PG_K_MAX = GT_K_MAX;
constexpr int64_t PG_N_MAX = (int64_t)1 << 40;      // rows: the workspace's bytes and the grids stay far inside their types
static_assert(PG_R % PG_S == 0, "a chunk is a whole number of slices");

// chunk blockIdx.x of V into part + blockIdx.x k k: S[t][u], t >= u, from +0.0, rows ascending, S = fma(v[t], v[u], S)
template <class T, bool WIDE, int CLS>
__global__ __launch_bounds__(GramClass<CLS>::TEAM) void panel_gram_chunk_kernel(const T *__restrict__ V, int64_t ldv, int64_t n, int k,
                                                                                double *__restrict__ part)
{
    constexpr int TEAM = GramClass<CLS>::TEAM, KP = GramClass<CLS>::KMAX, TPT = GramClass<CLS>::TPT;
    constexpr int PER = WIDE ? 16 / (int)sizeof(T) : 1;                     // elements per load
    constexpr int NL = (PG_S * (KP / PER) + TEAM - 1) / TEAM;               // loads per thread and slice
    __shared__ __attribute__((aligned(16))) double sv[2][PG_S][KP];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * PG_R, r1 = r0 + PG_R < n ? r0 + PG_R : n, last = r1 - 1;

    const int nb = (k + GT_B - 1) / GT_B, ntiles = nb * (nb + 1) / 2;
    int p0[TPT], q0[TPT], nt = 0;                                           // this thread's tiles: tid, tid + TEAM, ...
    double acc[TPT][GT_B][GT_B];
#pragma unroll
    for (int r = 0; r < TPT; r++) {
        const bool has = tid + r * TEAM < ntiles;
        gt_tile(tid + r * TEAM, has, p0[r], q0[r]);
        nt += has;
#pragma unroll
        for (int i = 0; i < GT_B; i++)
#pragma unroll
            for (int j = 0; j < GT_B; j++) acc[r][i][j] = 0.0;
    }

    // this thread's share of a slice: unit x = tid + l TEAM is piece x % upr of staged row x / upr
    const int upr = k / PER;                                                // units per panel row (WIDE: k is a whole number of pieces)
    int ue[NL], uo[NL];
#pragma unroll
    for (int l = 0; l < NL; l++) {
        const int x = tid + l * TEAM;
        ue[l] = x / upr;                                                    // (>= PG_S: no such unit)
        uo[l] = (x % upr) * PER;
    }
    double vreg[NL][PER];
#pragma unroll
    for (int l = 0; l < NL; l++)                                            // (past the chunk: its last row again, unused)
        if (ue[l] < PG_S) panel_unit<T, PER>(V + (r0 + ue[l] < last ? r0 + ue[l] : last) * ldv + uo[l], vreg[l]);

    int buf = 0;
    for (int64_t rs = r0; rs < r1; rs += PG_S, buf ^= 1) {
        const int cnt = r1 - rs < PG_S ? (int)(r1 - rs) : PG_S;
#pragma unroll
        for (int l = 0; l < NL; l++)
            if (ue[l] < PG_S) {
#pragma unroll
                for (int x = 0; x < PER; x++) sv[buf][ue[l]][uo[l] + x] = vreg[l][x];
            }
        team_sync<TEAM>();
        if (rs + PG_S < r1) {                                               // the next slice, in flight while this one is used
#pragma unroll
            for (int l = 0; l < NL; l++)
                if (ue[l] < PG_S) {
                    const int64_t row = rs + PG_S + ue[l];
                    panel_unit<T, PER>(V + (row < last ? row : last) * ldv + uo[l], vreg[l]);
                }
        }
        // the staged rows ascending.  (Columns k .. 4 nb - 1 of a staged row are never written: an edge tile reads whatever
        // LDS holds there into accumulators with t >= k or u >= k, which are not stored.)
        for (int x = 0; x < cnt; x++) {
#pragma unroll
            for (int r = 0; r < TPT; r++)
                if (r < nt) {
                    const f64x2_t a0 = *(const f64x2_t *)&sv[buf][x][p0[r]], a1 = *(const f64x2_t *)&sv[buf][x][p0[r] + 2];
                    const f64x2_t b0 = *(const f64x2_t *)&sv[buf][x][q0[r]], b1 = *(const f64x2_t *)&sv[buf][x][q0[r] + 2];
                    const double vp[GT_B] = {a0.x, a0.y, a1.x, a1.y}, vq[GT_B] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
                    for (int i = 0; i < GT_B; i++)
#pragma unroll
                        for (int j = 0; j < GT_B; j++) acc[r][i][j] = __builtin_fma(vp[i], vq[j], acc[r][i][j]);
                }
        }
    }

    double *o = part + (int64_t)blockIdx.x * k * k;
#pragma unroll
    for (int r = 0; r < TPT; r++)
        if (r < nt) {
#pragma unroll
            for (int i = 0; i < GT_B; i++)
#pragma unroll
                for (int j = 0; j < GT_B; j++) {
                    const int t = p0[r] + i, u = q0[r] + j;
                    if (t < k && u <= t) o[t * k + u] = acc[r][i][j];
                }
        }
}

// The last fold (cnt <= TREE_F partials at `in`, k k doubles apart; cnt = 0: the sum is +0.0) and rule P4: element (t, u),
// t >= u, per thread; the ridge on the diagonal, both triangles of out.
__global__ __launch_bounds__(TREE_THREADS) void panel_gram_finish_kernel(const double *__restrict__ in, int64_t cnt, int k, double ridge,
                                                                         double *__restrict__ out)
{
    const int e = blockIdx.x * TREE_THREADS + threadIdx.x;
    if (e >= k * k) return;
    const int t = e / k, u = e % k;
    if (u > t) return;
    const double sum = tree_fold_group(in, (int64_t)k * k, e, 0, cnt);
    const double v = t == u ? __dadd_rn(sum, ridge) : sum;
    out[t * k + u] = v;
    out[u * k + t] = v;
}

static int64_t pg_chunks(int64_t n) { return ceil_div(n, PG_R); }

// the workspace in doubles: the chunks' partials, and behind them the first fold's when one launch does not finish the tree
static int64_t pg_work_doubles(int64_t n, int32_t k)
{
    const int64_t c = pg_chunks(n);
    return (c + tree_extra_partials(c)) * k * k;
}

// what can be refused without a pointer (no device is touched)
static int pg_check_scalars(int64_t n, int32_t k)
{
    CSRK_REQUIRE(n >= 0, "csrk_panel_gram: n must not be negative (n=%lld)", (long long)n);
    CSRK_CHECK_K("", k);
    if (k > PG_K_MAX) {
        set_error("csrk_panel_gram: k=%d is above the largest supported k=%d (csrk_panel_gram_limits)", k, PG_K_MAX);
        return CSRK_ERR_UNSUPPORTED;
    }
    if (n > PG_N_MAX) {
        set_error("csrk_panel_gram: n=%lld is above the largest supported n=%lld", (long long)n, (long long)PG_N_MAX);
        return CSRK_ERR_OVERFLOW;
    }
    return CSRK_OK;
}

static int pg_check(int64_t n, int32_t k, const void *V, int64_t ldv, int panel_type, double ridge, const double *out)
{
    CSRK_TRY(pg_check_scalars(n, k));
    CSRK_CHECK_ONE_PANEL(k, ldv);
    CSRK_CHECK_PANEL_TYPE("", panel_type);
    CSRK_REQUIRE(ridge == ridge, "ridge is NaN");
    CSRK_REQUIRE(out && (V || n == 0), "V or out is NULL");
    CSRK_REQUIRE(((uintptr_t)V % panel_es(panel_type)) == 0 && ((uintptr_t)out % 8) == 0, "V or out is not aligned to its element size");
    return CSRK_OK;
}

static int pg_device(int64_t n, int32_t k, const void *dV, int64_t ldv, int panel_type, double ridge, double *dout, void *dwork,
                     int64_t work_bytes, hipStream_t s)
{
    CSRK_TRY(pg_check(n, k, dV, ldv, panel_type, ridge, dout));
    const int64_t need = pg_work_doubles(n, k) * 8;
    CSRK_REQUIRE(work_bytes >= need && (dwork || need == 0) && ((uintptr_t)dwork % 8) == 0,
                 "the workspace is NULL, misaligned or too small: %lld bytes, csrk_panel_gram_workspace asks for %lld", (long long)work_bytes,
                 (long long)need);
    const size_t es = panel_es(panel_type);
    const bool wide = panel_16b(dV, ldv, es) && k % panel_per16(es) == 0;   // a thread loads whole pieces of a row
    const int64_t c = pg_chunks(n), kk = (int64_t)k * k;
    double *cur = (double *)dwork, *other = cur + c * kk;
    if (c > 0) {
        const unsigned grid = (unsigned)c;
#define PG_GO(T, W, CLS) panel_gram_chunk_kernel<T, W, CLS><<<grid, GramClass<CLS>::TEAM, 0, s>>>((const T *)dV, ldv, n, k, cur)
#define PG_CLS(T, W)                                                                                                              \
    do {                                                                                                                          \
        if (k <= GT_K_WAVE) PG_GO(T, W, 1);                                                                                       \
        else if (k <= GT_K_ONE) PG_GO(T, W, 2);                                                                                   \
        else PG_GO(T, W, 3);                                                                                                      \
    } while (0)
        if (panel_type == CSRK_VAL_F64) {
            if (wide) PG_CLS(double, true);
            else PG_CLS(double, false);
        } else {
            if (wide) PG_CLS(float, true);
            else PG_CLS(float, false);
        }
#undef PG_CLS
#undef PG_GO
    }
    int64_t cnt = c;
    tree_fold_down(cur, other, cnt, kk, k, s);
    panel_gram_finish_kernel<<<(unsigned)ceil_div(kk, TREE_THREADS), TREE_THREADS, 0, s>>>(cur, cnt, k, ridge, dout);
    CSRK_LAUNCH_CHECK();
    return CSRK_OK;
}

}  // namespace csrk

using namespace csrk;

extern "C" {

int csrk_panel_gram_limits(int64_t *out, int n)
{
    CSRK_REQUIRE(out && n >= 0, "csrk_panel_gram_limits: out is NULL or n < 0");
    const int64_t v[2] = {PG_K_MAX, PG_R};
    for (int i = 0; i < n && i < 2; i++) out[i] = v[i];
    return CSRK_OK;
}

int csrk_panel_gram_workspace(int64_t n, int32_t k, int64_t *bytes)
{
    CSRK_REQUIRE(bytes, "bytes is NULL");
    CSRK_TRY(pg_check_scalars(n, k));
    *bytes = pg_work_doubles(n, k) * 8;
    return CSRK_OK;
}

int csrk_panel_gram_device(int64_t n, int32_t k, const void *d_V, int64_t ldv, int panel_type, double ridge, double *d_out, void *d_work,
                           int64_t work_bytes, void *stream)
{
    return pg_device(n, k, d_V, ldv, panel_type, ridge, d_out, d_work, work_bytes, (hipStream_t)stream);
}

int csrk_panel_gram(int64_t n, int32_t k, const void *V, int64_t ldv, int panel_type, double ridge, double *out)
{
    // argument checks first, with the caller's pointers (the device call below sees packed copies)
    CSRK_TRY(pg_check(n, k, V, ldv, panel_type, ridge, out));
    const int64_t need = pg_work_doubles(n, k) * 8;
    DevBuf dV, dO, dW;
    CSRK_TRY(pack_panel(dV, V, ldv, k, panel_es(panel_type), n));
    CSRK_TRY(dO.alloc((size_t)k * k * 8));
    CSRK_TRY(dW.alloc((size_t)need));
    CSRK_TRY(pg_device(n, k, dV.p, k, panel_type, ridge, dO.as<double>(), dW.p, need, nullptr));
    CSRK_HIP(hipMemcpy(out, dO.p, (size_t)k * k * 8, hipMemcpyDeviceToHost));
    return CSRK_OK;
}

}  // extern "C"
