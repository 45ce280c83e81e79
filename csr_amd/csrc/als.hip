// The ALS half-step for libcsrk on gfx950: per row of a CSR matrix, build the k x k normal equations and solve them, and the
// solve on its own for any batch of packed symmetric systems.
//     csrk_solve_blocks   x = G^-1 b for n packed k x k systems, by the LDL^T factorisation of include/csrk.h, rule S
//     csrk_als_rows       per row i: G_i (csrk_gram_rows' rule 2) + the count-weighted ridge, b_i = sum c_e v_j in storage
//                         order, then rule S; k float64 per row leave the chip, the block never does
// Both run one device routine, al_ldl_solve, so a fused row and the composed path (gram_rows, then solve_blocks) agree bit
// for bit.
//
// Where the block lives.  The accumulation is the routine gram.hip runs, gram_tile.h's gt_accumulate, with the right-hand
// side switched on: a TEAM of threads owns a row (16 lanes for k <= 16, a wavefront for k <= 40, a 256-thread workgroup
// above), the lower triangle is cut into 4 x 4 register tiles, one per thread (up to three for k > 88), and the row's V rows
// go through LDS GT_STAGE entries per step in two buffers.  When the row's entries are done the block sits in registers, and it is
// factorised THERE: a right-looking LDL^T step for column j is a rank-one update of the trailing triangle,
//     a[i][m] = fma(-L[i][j], C[m][j], a[i][m])      (j < m <= i),      L[i][j] = round(C[i][j] * r_j),   r_j = 1.0 / C[j][j]
// which has the shape of one more staged entry of the accumulation: a tile needs four p- and four q-operands of column j.
// So the only thing that crosses LDS is the current column: its owners publish C[j .. k-1][j] (k doubles), everyone reads
// the pivot and its own eight operands, computes the reciprocal and the L's it needs redundantly (the same operations on the
// same operands: the same bits in every thread) and updates its tiles in registers.  The column buffer is double
// buffered, so a column costs ONE team barrier.  No k x k triangle in LDS: 2 KB per team at k = 128 next to the 16 KB of
// staging, instead of 66 KB, and the occupancy of the Gram kernel is kept.  Every trailing element takes its updates in
// ascending j, which is rule S's order.
//
// The right-hand side rides along: thread p < k holds b[p] during the accumulation, then z[p]; at column j thread j
// publishes the finished z_j with the column and threads p > j take z_p = fma(-L[p][j], z_j, z_p): forward substitution,
// ascending, inside the factorisation loop.  y = round(z * r).  Back substitution walks t = k-1 .. 1: the owners of row t
// of L publish it (k doubles, the same two buffers), thread t publishes x_t, threads p < t take x_p = fma(-L[t][p], x_t,
// x_p): descending t, one barrier per step.  2 k - 1 team barriers per system in all; below a wavefront they are free.
//
// info = j + 1 for the first pivot with d_j > 0 false (every thread sees every pivot), 0 otherwise.  No pivoting, no square
// root, no special case: a bad pivot goes through IEEE arithmetic.
#include "gram_tile.h"

namespace csrk {

// acc[..][i][jj] for a jj known only at run time (the tiles live in registers: no indexed access)
__device__ __forceinline__ double al_pick(const double (&a)[GT_B], int jj)
{
    return jj == 0 ? a[0] : jj == 1 ? a[1] : jj == 2 ? a[2] : a[3];
}

// Rule S on a team's register tiles.  acc: the lower triangle (elements with q > p or p >= k hold anything and are never
// published); zx: b[tid] in, x[tid] out, for tid < k; col[2][KP] and piv[2]: the team's LDS.  Returns info, the same in
// every thread of the team.  Every thread of the team calls it (it holds team barriers).
template <int TEAM, int TPT, int KP>
__device__ __forceinline__ int al_ldl_solve(double (&acc)[TPT][GT_B][GT_B], const int (&p0)[TPT], const int (&q0)[TPT],
                                            const bool (&has)[TPT], double &zx, int k, int tid, double (*col)[KP], double *piv)
{
    int info = 0, step = 0;
    double z = zx, rmine = 0.0;
    for (int j = 0; j < k; j++, step++) {
        const int buf = step & 1;
        // column j as it stands is C[j .. k-1][j]: its owners publish it, thread j publishes z_j
#pragma unroll
        for (int r = 0; r < TPT; r++)
            if (has[r] && q0[r] <= j && j < q0[r] + GT_B) {
                const int jj = j - q0[r];
#pragma unroll
                for (int i = 0; i < GT_B; i++) {
                    const int p = p0[r] + i;
                    if (p >= j && p < k) col[buf][p] = al_pick(acc[r][i], jj);
                }
            }
        if (tid == j) piv[buf] = z;
        team_sync<TEAM>();
        const double d = col[buf][j];
        const double rj = 1.0 / d;                                          // one correctly rounded division
        if (info == 0 && !(d > 0.0)) info = j + 1;
#pragma unroll
        for (int r = 0; r < TPT; r++)
            if (has[r] && q0[r] + GT_B > j && p0[r] + GT_B > j) {
                const f64x2_t a0 = *(const f64x2_t *)&col[buf][p0[r]], a1 = *(const f64x2_t *)&col[buf][p0[r] + 2];
                const f64x2_t b0 = *(const f64x2_t *)&col[buf][q0[r]], b1 = *(const f64x2_t *)&col[buf][q0[r] + 2];
                const double cp[GT_B] = {a0.x, a0.y, a1.x, a1.y}, cq[GT_B] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
                for (int i = 0; i < GT_B; i++) {
                    const double l = __dmul_rn(cp[i], rj);                  // L[p][j]
#pragma unroll
                    for (int jj = 0; jj < GT_B; jj++) {
                        const int q = q0[r] + jj;
                        const double u = __builtin_fma(-l, cq[jj], acc[r][i][jj]);
                        acc[r][i][jj] = q > j ? u : (q == j ? l : acc[r][i][jj]);
                    }
                }
            }
        if (tid > j && tid < k) z = __builtin_fma(-__dmul_rn(col[buf][tid], rj), piv[buf], z);
        if (tid == j) rmine = rj;
    }
    double x = __dmul_rn(z, rmine);                                         // y = round(z r)
    for (int t = k - 1; t >= 1; t--, step++) {
        const int buf = step & 1;
        // row t of L, columns 0 .. t-1: its owners publish it, thread t publishes x_t
#pragma unroll
        for (int r = 0; r < TPT; r++)
            if (has[r] && p0[r] <= t && t < p0[r] + GT_B) {
                const int i = t - p0[r];
#pragma unroll
                for (int jj = 0; jj < GT_B; jj++) {
                    const int q = q0[r] + jj;
                    const double a[GT_B] = {acc[r][0][jj], acc[r][1][jj], acc[r][2][jj], acc[r][3][jj]};
                    if (q < t) col[buf][q] = al_pick(a, i);
                }
            }
        if (tid == t) piv[buf] = x;
        team_sync<TEAM>();
        if (tid < t) x = __builtin_fma(-col[buf][tid], piv[buf], x);
    }
    zx = x;
    return info;
}

template <int CLS>
__global__ __launch_bounds__(GT_THREADS) void solve_blocks_kernel(int64_t n, int32_t k, const double *__restrict__ G,
                                                                 const double *__restrict__ b, int64_t ldb, double *__restrict__ x,
                                                                 int64_t ldx, int32_t *__restrict__ info)
{
    typedef GramClass<CLS> C;
    constexpr int TEAM = C::TEAM, KP = C::KMAX, TPT = C::TPT, TEAMS = GT_THREADS / TEAM;
    __shared__ __attribute__((aligned(16))) double col[TEAMS][2][KP];
    __shared__ double piv[TEAMS][2];

    const int team = threadIdx.x / TEAM, tid = threadIdx.x % TEAM;
    const int64_t sys = (int64_t)blockIdx.x * TEAMS + team;
    if (TEAM < GT_THREADS && sys >= n) return;                              // (a whole team; teams never meet at a barrier)
    const double *__restrict__ g = G + sys * k * k;

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
                acc[r][i][j] = (has[r] && p < k && q <= p) ? g[(int64_t)p * k + q] : 0.0;
            }
    }
    double z = tid < k ? b[sys * ldb + tid] : 0.0;
    const int inf = al_ldl_solve<TEAM, TPT, KP>(acc, p0, q0, has, z, k, tid, col[team], piv[team]);
    if (tid < k) x[sys * ldx + tid] = z;
    if (info && tid == 0) info[sys] = inf;
}

template <class T, bool WIDE, int CLS, bool SCALE>
__global__ __launch_bounds__(GT_THREADS) void als_kernel(const void *__restrict__ rp, int ptr64, const int32_t *__restrict__ ci,
                                                         const void *__restrict__ vals, int vt, int32_t row_begin, int32_t row_end,
                                                         const T *__restrict__ V, int64_t ldv, int32_t k, int rhs_mode,
                                                         const double *__restrict__ base, double lam_n, double *__restrict__ out,
                                                         int64_t ldo, int32_t *__restrict__ info)
{
    typedef GramClass<CLS> C;
    constexpr int TEAM = C::TEAM, KP = C::KMAX, TPT = C::TPT, TEAMS = GT_THREADS / TEAM;
    __shared__ __attribute__((aligned(16))) double sv[TEAMS][2][GT_STAGE][KP];
    __shared__ __attribute__((aligned(16))) double col[TEAMS][2][KP];
    __shared__ double sw[TEAMS][2][GT_STAGE];
    __shared__ double piv[TEAMS][2];

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
    double bacc = 0.0;                                                      // b[tid], for tid < k
    gt_accumulate<T, WIDE, CLS, SCALE, true>(e0, e1, ci, vals, vt, V, ldv, k, rhs_mode, tid, sv[team], sw[team], acc, p0, q0, bacc);

    // the ridge, after the chain: G[p][p] = fma(lam_n, n_i, G[p][p])
    const double cnt_d = (double)(e1 - e0);
#pragma unroll
    for (int r = 0; r < TPT; r++)
        if (p0[r] == q0[r]) {
#pragma unroll
            for (int i = 0; i < GT_B; i++) acc[r][i][i] = __builtin_fma(lam_n, cnt_d, acc[r][i][i]);
        }

    const int inf = al_ldl_solve<TEAM, TPT, KP>(acc, p0, q0, has, bacc, k, tid, col[team], piv[team]);
    if (tid < k) out[(int64_t)(row - row_begin) * ldo + tid] = bacc;
    if (info && tid == 0) info[row - row_begin] = inf;
}

static int solve_check(int64_t n, int32_t k, int64_t ldb, int64_t ldx)
{
    CSRK_REQUIRE(n >= 0, "n must not be negative (n=%lld)", (long long)n);
    CSRK_CHECK_K("", k);
    CSRK_REQUIRE(ldb >= k && ldx >= k, "bad geometry k=%d ldb=%lld ldx=%lld", k, (long long)ldb, (long long)ldx);
    if (k > GT_K_MAX) {
        set_error("csrk_solve_blocks: k=%d is above the largest supported k=%d (csrk_als_limits)", k, GT_K_MAX);
        return CSRK_ERR_UNSUPPORTED;
    }
    return CSRK_OK;
}

static int solve_device(int64_t n, int32_t k, const double *dG, const double *db, int64_t ldb, double *dx, int64_t ldx,
                        int32_t *dinfo, hipStream_t s)
{
    CSRK_TRY(solve_check(n, k, ldb, ldx));
    if (n == 0) return CSRK_OK;
    CSRK_REQUIRE(dG && db && dx, "G, b or x is NULL");
    CSRK_REQUIRE(((uintptr_t)dG % 8) == 0 && ((uintptr_t)db % 8) == 0 && ((uintptr_t)dx % 8) == 0 && ((uintptr_t)dinfo % 4) == 0,
                 "G, b, x or info is not aligned to its element size");
    const int team = k <= GT_K_SUB ? GramClass<0>::TEAM : k <= GT_K_WAVE ? GramClass<1>::TEAM : GT_THREADS;
    CSRK_REQUIRE(ceil_div(n, GT_THREADS / team) <= INT32_MAX, "n=%lld systems are more than one launch takes", (long long)n);
#define AL_GO(CLS) \
    solve_blocks_kernel<CLS><<<(unsigned)ceil_div(n, GT_THREADS / GramClass<CLS>::TEAM), GT_THREADS, 0, s>>>(n, k, dG, db, ldb, dx, ldx, dinfo)
    if (k <= GT_K_SUB) AL_GO(0);
    else if (k <= GT_K_WAVE) AL_GO(1);
    else if (k <= GT_K_ONE) AL_GO(2);
    else AL_GO(3);
#undef AL_GO
    CSRK_LAUNCH_CHECK();
    return CSRK_OK;
}

static int als_check(Matrix *m, int32_t row_begin, int32_t row_end, int64_t ldv, int32_t k, int panel_type, int scale, int rhs_mode,
                     int64_t ldo)
{
    CSRK_CHECK_K("", k);
    CSRK_CHECK_ONE_PANEL(k, ldv);
    CSRK_REQUIRE(ldo >= k, "bad output geometry k=%d ldo=%lld", k, (long long)ldo);
    CSRK_CHECK_PANEL_TYPE("", panel_type);
    CSRK_CHECK_SCALE(scale);
    CSRK_REQUIRE(rhs_mode == CSRK_ALS_RHS_ONES || rhs_mode == CSRK_ALS_RHS_VALUES || rhs_mode == CSRK_ALS_RHS_ONE_PLUS,
                 "rhs_mode must be CSRK_ALS_RHS_ONES, _VALUES or _ONE_PLUS, not %d", rhs_mode);
    return gt_check_rows("csrk_als", m, row_begin, row_end, k);
}

static int als_device(Matrix *m, int32_t row_begin, int32_t row_end, const void *dV, int64_t ldv, int32_t k, int panel_type, int scale,
                      int rhs_mode, const double *dbase, double lam_n, double *dout, int64_t ldo, int32_t *dinfo, hipStream_t s)
{
    CSRK_TRY(als_check(m, row_begin, row_end, ldv, k, panel_type, scale, rhs_mode, ldo));
    if (row_begin == row_end) return CSRK_OK;
    CSRK_REQUIRE(dout && (dV || m->nnz == 0), "V or out is NULL");
    const size_t es = panel_es(panel_type);
    CSRK_REQUIRE(((uintptr_t)dV % es) == 0 && ((uintptr_t)dout % 8) == 0 && ((uintptr_t)dbase % 8) == 0 && ((uintptr_t)dinfo % 4) == 0,
                 "V, base, out or info is not aligned to its element size");
    mark_user_stream(m, s);
    const bool wide = panel_16b(dV, ldv, es) && k % panel_per16(es) == 0;
    const bool stored = m->val_type != CSRK_VAL_NONE;               // (a structure-only matrix: every value is 1.0)
    const bool scaled = scale && stored;
    const void *vals = stored && (scaled || rhs_mode != CSRK_ALS_RHS_ONES) ? m->d_values : nullptr;
    const int64_t n = (int64_t)row_end - row_begin;
#define AL_GO(T, W, CLS, SC)                                                                                            \
    als_kernel<T, W, CLS, SC><<<(unsigned)ceil_div(n, GT_THREADS / GramClass<CLS>::TEAM), GT_THREADS, 0, s>>>(            \
        m->d_rowptrs, m->ptr64, m->d_colinds, vals, m->val_type, row_begin, row_end, (const T *)dV, ldv, k, rhs_mode, dbase, lam_n, \
        dout, ldo, dinfo)
#define AL_SC(T, W, CLS)                                                                                                \
    do {                                                                                                               \
        if (scaled) AL_GO(T, W, CLS, true);                                                                            \
        else AL_GO(T, W, CLS, false);                                                                                  \
    } while (0)
#define AL_CLS(T, W)                                                                                                   \
    do {                                                                                                               \
        if (k <= GT_K_SUB) AL_SC(T, W, 0);                                                                             \
        else if (k <= GT_K_WAVE) AL_SC(T, W, 1);                                                                       \
        else if (k <= GT_K_ONE) AL_SC(T, W, 2);                                                                        \
        else AL_SC(T, W, 3);                                                                                           \
    } while (0)
    if (panel_type == CSRK_VAL_F64) {
        if (wide) AL_CLS(double, true);
        else AL_CLS(double, false);
    } else {
        if (wide) AL_CLS(float, true);
        else AL_CLS(float, false);
    }
#undef AL_CLS
#undef AL_SC
#undef AL_GO
    CSRK_LAUNCH_CHECK();
    return CSRK_OK;
}

}  // namespace csrk

using namespace csrk;

extern "C" {

int csrk_als_limits(int64_t *out, int n)
{
    CSRK_REQUIRE(out && n >= 0, "csrk_als_limits: out is NULL or n < 0");
    const int64_t v[5] = {GT_K_MAX, GT_STAGE, GT_K_SUB, GT_K_WAVE, GT_K_ONE};
    for (int i = 0; i < n && i < 5; i++) out[i] = v[i];
    return CSRK_OK;
}

int csrk_solve_blocks_device(int64_t n, int32_t k, const double *d_G, const double *d_b, int64_t ldb, double *d_x, int64_t ldx,
                             int32_t *d_info, void *stream)
{
    return solve_device(n, k, d_G, d_b, ldb, d_x, ldx, d_info, (hipStream_t)stream);
}

int csrk_solve_blocks(int64_t n, int32_t k, const double *G, const double *b, int64_t ldb, double *x, int64_t ldx, int32_t *info)
{
    // argument checks first, with the caller's pointers (the device call below sees packed copies)
    CSRK_TRY(solve_check(n, k, ldb, ldx));
    if (n == 0) return CSRK_OK;
    CSRK_REQUIRE(G && b && x, "G, b or x is NULL");
    const size_t ng = (size_t)n * k * k * 8, nv = (size_t)n * k * 8;
    int dev = 0;
    CSRK_HIP(hipGetDevice(&dev));                                           // (no handle vouches for a device here)
    DevBuf dG, dB, dX, dI;
    CSRK_TRY(dG.alloc(ng));
    CSRK_TRY(dX.alloc(nv));
    CSRK_TRY(dI.alloc((size_t)n * 4));
    CSRK_HIP(hipMemcpy(dG.p, G, ng, hipMemcpyHostToDevice));
    CSRK_TRY(pack_panel(dB, b, ldb, k, 8, n));
    CSRK_TRY(solve_device(n, k, dG.as<double>(), dB.as<double>(), k, dX.as<double>(), k, dI.as<int32_t>(), nullptr));
    CSRK_TRY(unpack_panel(x, ldx, dX, k, 8, n));
    if (info) CSRK_HIP(hipMemcpy(info, dI.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return CSRK_OK;
}

int csrk_als_rows_device(csrk_handle_t h, int32_t row_begin, int32_t row_end, const void *d_V, int64_t ldv, int32_t k, int panel_type,
                         int scale, int rhs_mode, const double *d_base, double lam_n, double *d_out, int64_t ldo, int32_t *d_info,
                         void *stream)
{
    Matrix *m = from_handle(h);
    if (!m) return CSRK_ERR_INVALID;
    return als_device(m, row_begin, row_end, d_V, ldv, k, panel_type, scale, rhs_mode, d_base, lam_n, d_out, ldo, d_info,
                      (hipStream_t)stream);
}

int csrk_als_rows(csrk_handle_t h, int32_t row_begin, int32_t row_end, const void *V, int64_t ldv, int32_t k, int panel_type, int scale,
                  int rhs_mode, const double *base, double lam_n, double *out, int64_t ldo, int32_t *info)
{
    Matrix *m = from_handle(h);
    if (!m) return CSRK_ERR_INVALID;
    // argument checks first, with the caller's pointers (the device call below sees packed copies)
    CSRK_TRY(als_check(m, row_begin, row_end, ldv, k, panel_type, scale, rhs_mode, ldo));
    if (row_begin == row_end) return CSRK_OK;
    CSRK_REQUIRE(out && (V || m->nnz == 0), "V or out is NULL");
    const size_t n = (size_t)(row_end - row_begin);
    DevBuf dV, dB, dO, dI;
    CSRK_TRY(pack_panel(dV, V, ldv, k, panel_es(panel_type), m->ncols));
    CSRK_TRY(dO.alloc(n * k * 8));
    CSRK_TRY(dI.alloc(n * 4));
    if (base) {
        CSRK_TRY(dB.alloc((size_t)k * k * 8));
        CSRK_HIP(hipMemcpy(dB.p, base, (size_t)k * k * 8, hipMemcpyHostToDevice));
    }
    CSRK_TRY(als_device(m, row_begin, row_end, dV.p, k, k, panel_type, scale, rhs_mode, base ? dB.as<double>() : nullptr, lam_n,
                        dO.as<double>(), k, dI.as<int32_t>(), nullptr));
    CSRK_TRY(unpack_panel(out, ldo, dO, k, 8, n));
    if (info) CSRK_HIP(hipMemcpy(info, dI.p, n * 4, hipMemcpyDeviceToHost));
    return CSRK_OK;
}

}  // extern "C"
