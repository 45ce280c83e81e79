// The ALS objective for libcsrk on gfx950: the quadratic form that csrk_als_rows and csrk_als_rows_cg minimise, per row
// (rule J1) and in total (rule J2), with every sum in a stated order (include/csrk.h, rules J and T).
//     csrk_als_objective_rows   J_i = sum_e (g_e - 2 c_e) s_e + rho_i |u_i|^2,  s_e = u_i . v_e,  g_e = w_e s_e or s_e
//     csrk_als_objective        T(J over A's rows) + T(the regulariser over A^T's rows) + <U^T U, V^T V> (implicit)
//
// Work split of the rows.  ONE 16-LANE TEAM PER ROW, at every k, in csrk_als_rows_cg's layout: a lane owns its four
// columns of every 64-column chunk (panel_off in device_loads.h), u_i lives in registers, OBJ_E entries' V rows are loaded
// and their dots taken (team_dot.h: rule C2's DOT, the code the CG step runs) before the first is used; only the one fma
// per entry into J_i is serial.  Every lane of the team ends with the same J_i; lane 0 writes it.
//
// The total.  Rule T cuts an array into chunks of OBJ_L elements, adds each serially from +0.0 (one thread per chunk) and
// combines the partials by the tree of tree_sum.h.  csrk_als_objective[_device] is a sequence of launches on one stream --
// the two row kernels, with `implicit` csrk_panel_gram_device twice and an element-wise product, three rule-T sums and a
// one-thread kernel for the last two additions -- that allocates nothing and never synchronises.
#include "common.h"
#include "device_loads.h"
#include "panel.h"
#include "team_dot.h"
#include "tree_sum.h"
#include "wave.h"

namespace csrk {

constexpr int OBJ_G = PANEL_G;           // lanes per team (one DPP row)
constexpr int OBJ_THREADS = 256;
constexpr int OBJ_TEAMS = OBJ_THREADS / OBJ_G;
constexpr int OBJ_E = 4;                 // entries in flight per team and step of the entry loop
constexpr int OBJ_K_MAX = 128;           // two chunks of 64 columns
constexpr int OBJ_L = 256;               // elements per serial chunk of rule T (csrk_als_objective_limits' out[1])

// NCH chunks of 64 columns: k <= 64 NCH.  vals: NULL when no value is wanted or none is stored (every one 1.0).
template <bool WIDE, int NCH>
__global__ __launch_bounds__(OBJ_THREADS) void als_objective_rows_kernel(const void *__restrict__ rp, int ptr64, const int32_t *__restrict__ ci,
                                                                         const void *__restrict__ vals, int vt, int scaled, int rhs_mode,
                                                                         int data, int32_t row_begin, int32_t row_end,
                                                                         const double *__restrict__ U, int64_t ldu,
                                                                         const double *__restrict__ V, int64_t ldv, int32_t k, double lam,
                                                                         double lam_n, double *__restrict__ out)
{
    const int team = threadIdx.x / OBJ_G, sub = threadIdx.x % OBJ_G;
    const int64_t row = (int64_t)row_begin + (int64_t)blockIdx.x * OBJ_TEAMS + team;
    if (row >= row_end) return;                                             // (a whole team; teams never meet at a barrier)
    const int64_t e0 = load_ptr(rp, ptr64, row), e1 = load_ptr(rp, ptr64, row + 1);
    const double rho = __builtin_fma(lam_n, (double)(e1 - e0), lam);
    const double *ur = U + row * ldu;
    double u[NCH][4];
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int t = 64 * c + panel_off<double>(sub, i);
            u[c][i] = t < k ? ur[t] : 0.0;
        }

    double J = 0.0;
    if (data && e0 < e1) {
        const int64_t last = e1 - 1;
        int32_t coln[OBJ_E];                                                // the next step's column indices
#pragma unroll
        for (int x = 0; x < OBJ_E; x++) coln[x] = ci[e0 + x < last ? e0 + x : last];
        for (int64_t es = e0; es < e1; es += OBJ_E) {
            double v[OBJ_E][NCH][4], wv[OBJ_E], s[OBJ_E];
#pragma unroll
            for (int x = 0; x < OBJ_E; x++)                                 // (past the row: its last entry again, unused)
#pragma unroll
                for (int c = 0; c < NCH; c++) panel_load4<double, WIDE>(V + (int64_t)coln[x] * ldv + 64 * c, sub, k - 64 * c, v[x][c]);
#pragma unroll
            for (int x = 0; x < OBJ_E; x++) {
                const int64_t e = es + x < last ? es + x : last;
                wv[x] = vals ? csr_stored_val(vals, vt, e) : 1.0;
                const int64_t en = es + OBJ_E + x < last ? es + OBJ_E + x : last;
                coln[x] = ci[en];
            }
#pragma unroll
            for (int x = 0; x < OBJ_E; x++) s[x] = cg_dot<double, NCH>(u, v[x], sub, k);
#pragma unroll
            for (int x = 0; x < OBJ_E; x++)
                if (es + x < e1) {
                    const double g = scaled ? __dmul_rn(wv[x], s[x]) : s[x];
                    const double cc = rhs_mode == CSRK_ALS_RHS_ONES ? 1.0 : (rhs_mode == CSRK_ALS_RHS_VALUES ? wv[x] : __dadd_rn(1.0, wv[x]));
                    const double h = __dsub_rn(g, 2.0 * cc);                // (2 c_e is exact)
                    J = __builtin_fma(h, s[x], J);
                }
        }
    }
    J = __builtin_fma(rho, cg_dot<double, NCH>(u, u, sub, k), J);
    if (sub == 0) out[row - row_begin] = J;
}

// rule T's chunks: thread c adds x[c OBJ_L .. min(n, (c + 1) OBJ_L)) serially from +0.0
__global__ __launch_bounds__(TREE_THREADS) void chunk_sum_kernel(const double *__restrict__ x, int64_t n, double *__restrict__ part)
{
    const int64_t c = (int64_t)blockIdx.x * TREE_THREADS + threadIdx.x, b = c * OBJ_L;
    if (b >= n) return;
    const int64_t e = b + OBJ_L < n ? b + OBJ_L : n;
    double s = 0.0;
    for (int64_t i = b; i < e; i++) s = __dadd_rn(s, x[i]);
    part[c] = s;
}

// rule J2's products: p[e] = round(a[e] b[e])
__global__ __launch_bounds__(TREE_THREADS) void product_kernel(const double *__restrict__ a, const double *__restrict__ b, int n,
                                                               double *__restrict__ p)
{
    const int e = blockIdx.x * TREE_THREADS + threadIdx.x;
    if (e < n) p[e] = __dmul_rn(a[e], b[e]);
}

// rule J2's last line: objective = round(round(r[0] + r[1]) + F), F = r[2] or +0.0
__global__ void objective_total_kernel(const double *__restrict__ r, int implicit, double *__restrict__ objective)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *objective = __dadd_rn(__dadd_rn(r[0], r[1]), implicit ? r[2] : 0.0);
}

// doubles of workspace that rule T needs over n elements
static int64_t t_sum_doubles(int64_t n)
{
    const int64_t c = ceil_div(n, OBJ_L);
    return c + tree_extra_partials(c);
}

// rule T of x[0 .. n) into *result, on s; work: t_sum_doubles(n) doubles
static void t_sum(const double *x, int64_t n, double *result, double *work, hipStream_t s)
{
    int64_t cnt = ceil_div(n, OBJ_L);
    double *cur = work, *other = work + cnt;
    if (cnt > 0) chunk_sum_kernel<<<(unsigned)ceil_div(cnt, TREE_THREADS), TREE_THREADS, 0, s>>>(x, n, cur);
    tree_fold_down(cur, other, cnt, 1, 0, s);
    tree_fold_kernel<<<1, TREE_THREADS, 0, s>>>(cur, cnt, 1, 1, 0, result);      // (no partial: +0.0)
}

// what can be refused without looking at a handle
static int obj_check_scalars(int64_t ldu, int64_t ldv, int32_t k, int scale, int rhs_mode, int flag, const char *flag_name)
{
    CSRK_CHECK_K("", k);
    CSRK_CHECK_TWO_PANELS("", k, ldu, ldv);
    CSRK_CHECK_SCALE(scale);
    CSRK_REQUIRE(rhs_mode == CSRK_ALS_RHS_ONES || rhs_mode == CSRK_ALS_RHS_VALUES || rhs_mode == CSRK_ALS_RHS_ONE_PLUS,
                 "rhs_mode must be CSRK_ALS_RHS_ONES, _VALUES or _ONE_PLUS, not %d", rhs_mode);
    CSRK_REQUIRE(flag == 0 || flag == 1, "%s must be 0 or 1, not %d", flag_name, flag);
    if (k > OBJ_K_MAX) {
        set_error("csrk_als_objective: k=%d is above the largest supported k=%d (csrk_als_objective_limits)", k, OBJ_K_MAX);
        return CSRK_ERR_UNSUPPORTED;
    }
    return CSRK_OK;
}

// the launch of rule J1 over [row_begin, row_end); every check but the scalars' is the caller's
static void obj_rows_launch(Matrix *m, int32_t row_begin, int32_t row_end, const double *dU, int64_t ldu, const double *dV, int64_t ldv,
                            int32_t k, int scale, int rhs_mode, int data, double lam, double lam_n, double *dout, hipStream_t s)
{
    if (row_begin == row_end) return;
    mark_user_stream(m, s);
    const bool wide = panel_16b(dV, ldv, 8);       // a lane loads four columns at a time, as csrk_sddmm's do: no k term
    const bool stored = m->val_type != CSRK_VAL_NONE;               // (a structure-only matrix: every value is 1.0)
    const int scaled = scale && stored;
    const void *vals = data && stored && (scaled || rhs_mode != CSRK_ALS_RHS_ONES) ? m->d_values : nullptr;
    const unsigned grid = (unsigned)ceil_div((int64_t)row_end - row_begin, OBJ_TEAMS);
#define OBJ_GO(W, NCH)                                                                                                            \
    als_objective_rows_kernel<W, NCH><<<grid, OBJ_THREADS, 0, s>>>(m->d_rowptrs, m->ptr64, m->d_colinds, vals, m->val_type, scaled,       \
                                                                  rhs_mode, data, row_begin, row_end, dU, ldu, dV, ldv, k, lam, lam_n, \
                                                                  dout)
    if (wide) {
        if (k <= 64) OBJ_GO(true, 1);
        else OBJ_GO(true, 2);
    } else {
        if (k <= 64) OBJ_GO(false, 1);
        else OBJ_GO(false, 2);
    }
#undef OBJ_GO
}

static int obj_rows_check(Matrix *m, int32_t row_begin, int32_t row_end, const double *U, const double *V, int data, const double *out)
{
    CSRK_CHECK_ROW_RANGE("", row_begin, row_end, m->nrows);
    if (row_begin == row_end) return CSRK_OK;
    CSRK_REQUIRE(out && U && (V || !data || m->nnz == 0), "U, V or out is NULL");
    CSRK_REQUIRE(((uintptr_t)U % 8) == 0 && ((uintptr_t)V % 8) == 0 && ((uintptr_t)out % 8) == 0, "U, V or out is not aligned to its element size");
    return CSRK_OK;
}

// the workspace of csrk_als_objective_device in doubles, in the order it is laid out: J over A's rows, J over A^T's rows, the
// three sums, rule T's partials; with implicit the two Grams, their products and csrk_panel_gram's own workspace
struct ObjLayout {
    int64_t ja, jt, res, tsum, gu, gv, prod, pg, total;
    int64_t pg_bytes;
};

static int obj_layout(int32_t nrows, int32_t ncols, int32_t k, int implicit, ObjLayout *L)
{
    const int64_t kk = (int64_t)k * k, big = nrows > ncols ? nrows : ncols;
    int64_t o = 0;
    L->ja = o, o += nrows;
    L->jt = o, o += ncols;
    L->res = o, o += 4;
    L->tsum = o, o += t_sum_doubles(big > kk ? big : kk);
    L->gu = L->gv = L->prod = L->pg = o;
    L->pg_bytes = 0;
    if (implicit) {
        L->gu = o, o += kk;
        L->gv = o, o += kk;
        L->prod = o, o += kk;
        CSRK_TRY(csrk_panel_gram_workspace(big, k, &L->pg_bytes));
        L->pg = o, o += L->pg_bytes / 8;
    }
    L->total = o;
    return CSRK_OK;
}

static int obj_total_device(csrk_handle_t hA, csrk_handle_t hAt, const double *dU, int64_t ldu, const double *dV, int64_t ldv, int32_t k,
                            int scale, int rhs_mode, int implicit, double lam, double lam_n, double *dobj, void *dwork,
                            int64_t work_bytes, hipStream_t s)
{
    CSRK_TRY(obj_check_scalars(ldu, ldv, k, scale, rhs_mode, implicit, "implicit"));
    Matrix *a = from_handle(hA);
    if (!a) return CSRK_ERR_INVALID;
    Matrix *at = from_handle(hAt);
    if (!at) return CSRK_ERR_INVALID;
    CSRK_TRY(check_transpose_shape(a, at));
    CSRK_REQUIRE(dobj && (dU || a->nrows == 0) && (dV || a->ncols == 0), "U, V or objective is NULL");
    CSRK_REQUIRE(((uintptr_t)dU % 8) == 0 && ((uintptr_t)dV % 8) == 0 && ((uintptr_t)dobj % 8) == 0 && ((uintptr_t)dwork % 8) == 0,
                 "U, V, objective or the workspace is not aligned to 8 bytes");
    ObjLayout L;
    CSRK_TRY(obj_layout(a->nrows, a->ncols, k, implicit, &L));
    CSRK_REQUIRE(dwork && work_bytes >= L.total * 8, "the workspace is NULL or too small: %lld bytes, csrk_als_objective_workspace asks for %lld",
                 (long long)work_bytes, (long long)(L.total * 8));
    double *w = (double *)dwork;
    obj_rows_launch(a, 0, a->nrows, dU, ldu, dV, ldv, k, scale, rhs_mode, 1, lam, lam_n, w + L.ja, s);
    obj_rows_launch(at, 0, at->nrows, dV, ldv, dU, ldu, k, scale, rhs_mode, 0, lam, lam_n, w + L.jt, s);
    t_sum(w + L.ja, a->nrows, w + L.res, w + L.tsum, s);
    t_sum(w + L.jt, at->nrows, w + L.res + 1, w + L.tsum, s);
    if (implicit) {
        const int kk = k * k;
        CSRK_TRY(csrk_panel_gram_device(a->nrows, k, dU, ldu, CSRK_VAL_F64, 0.0, w + L.gu, w + L.pg, L.pg_bytes, s));
        CSRK_TRY(csrk_panel_gram_device(a->ncols, k, dV, ldv, CSRK_VAL_F64, 0.0, w + L.gv, w + L.pg, L.pg_bytes, s));
        product_kernel<<<(unsigned)ceil_div(kk, TREE_THREADS), TREE_THREADS, 0, s>>>(w + L.gu, w + L.gv, kk, w + L.prod);
        t_sum(w + L.prod, kk, w + L.res + 2, w + L.tsum, s);
    }
    objective_total_kernel<<<1, 64, 0, s>>>(w + L.res, implicit, dobj);
    CSRK_LAUNCH_CHECK();
    return CSRK_OK;
}

}  // namespace csrk

using namespace csrk;

extern "C" {

int csrk_als_objective_limits(int64_t *out, int n)
{
    CSRK_REQUIRE(out && n >= 0, "csrk_als_objective_limits: out is NULL or n < 0");
    const int64_t v[4] = {OBJ_K_MAX, OBJ_L, OBJ_G, OBJ_E};
    for (int i = 0; i < n && i < 4; i++) out[i] = v[i];
    return CSRK_OK;
}

int csrk_als_objective_rows_device(csrk_handle_t h, int32_t row_begin, int32_t row_end, const double *d_U, int64_t ldu, const double *d_V,
                                   int64_t ldv, int32_t k, int scale, int rhs_mode, int data, double lam, double lam_n, double *d_out,
                                   void *stream)
{
    CSRK_TRY(obj_check_scalars(ldu, ldv, k, scale, rhs_mode, data, "data"));
    CSRK_CHECK_ROW_ORDER("", row_begin, row_end);
    Matrix *m = from_handle(h);
    if (!m) return CSRK_ERR_INVALID;
    CSRK_TRY(obj_rows_check(m, row_begin, row_end, d_U, d_V, data, d_out));
    obj_rows_launch(m, row_begin, row_end, d_U, ldu, d_V, ldv, k, scale, rhs_mode, data, lam, lam_n, d_out, (hipStream_t)stream);
    CSRK_LAUNCH_CHECK();
    return CSRK_OK;
}

int csrk_als_objective_rows(csrk_handle_t h, int32_t row_begin, int32_t row_end, const double *U, int64_t ldu, const double *V, int64_t ldv,
                            int32_t k, int scale, int rhs_mode, int data, double lam, double lam_n, double *out)
{
    CSRK_TRY(obj_check_scalars(ldu, ldv, k, scale, rhs_mode, data, "data"));
    CSRK_CHECK_ROW_ORDER("", row_begin, row_end);
    Matrix *m = from_handle(h);
    if (!m) return CSRK_ERR_INVALID;
    // argument checks first, with the caller's pointers (the launch below sees packed copies)
    CSRK_TRY(obj_rows_check(m, row_begin, row_end, U, V, data, out));
    if (row_begin == row_end) return CSRK_OK;
    const size_t n = (size_t)(row_end - row_begin);
    DevBuf dU, dV, dO;
    CSRK_TRY(pack_panel(dU, U, ldu, k, 8, m->nrows));
    CSRK_TRY(pack_panel(dV, data ? V : nullptr, ldv, k, 8, data ? m->ncols : 0));
    CSRK_TRY(dO.alloc(n * 8));
    obj_rows_launch(m, row_begin, row_end, dU.as<double>(), k, dV.as<double>(), k, k, scale, rhs_mode, data, lam, lam_n, dO.as<double>(),
                    nullptr);
    CSRK_LAUNCH_CHECK();
    CSRK_HIP(hipMemcpy(out, dO.p, n * 8, hipMemcpyDeviceToHost));
    return CSRK_OK;
}

int csrk_als_objective_workspace(int32_t nrows, int32_t ncols, int32_t k, int implicit, int64_t *bytes)
{
    CSRK_REQUIRE(bytes, "bytes is NULL");
    CSRK_REQUIRE(nrows >= 0 && ncols >= 0, "bad shape %d x %d", nrows, ncols);
    CSRK_TRY(obj_check_scalars(k, k, k, 0, CSRK_ALS_RHS_ONES, implicit, "implicit"));
    ObjLayout L;
    CSRK_TRY(obj_layout(nrows, ncols, k, implicit, &L));
    *bytes = L.total * 8;
    return CSRK_OK;
}

int csrk_als_objective_device(csrk_handle_t hA, csrk_handle_t hAt, const double *d_U, int64_t ldu, const double *d_V, int64_t ldv, int32_t k,
                              int scale, int rhs_mode, int implicit, double lam, double lam_n, double *d_objective, void *d_work,
                              int64_t work_bytes, void *stream)
{
    return obj_total_device(hA, hAt, d_U, ldu, d_V, ldv, k, scale, rhs_mode, implicit, lam, lam_n, d_objective, d_work, work_bytes,
                            (hipStream_t)stream);
}

int csrk_als_objective(csrk_handle_t hA, csrk_handle_t hAt, const double *U, int64_t ldu, const double *V, int64_t ldv, int32_t k,
                       int scale, int rhs_mode, int implicit, double lam, double lam_n, double *objective)
{
    CSRK_TRY(obj_check_scalars(ldu, ldv, k, scale, rhs_mode, implicit, "implicit"));
    Matrix *a = from_handle(hA);
    if (!a) return CSRK_ERR_INVALID;
    Matrix *at = from_handle(hAt);
    if (!at) return CSRK_ERR_INVALID;
    // argument checks first, with the caller's pointers (the device call below sees packed copies)
    CSRK_TRY(check_transpose_shape(a, at));
    CSRK_REQUIRE(objective && (U || a->nrows == 0) && (V || a->ncols == 0), "U, V or objective is NULL");
    CSRK_REQUIRE(((uintptr_t)U % 8) == 0 && ((uintptr_t)V % 8) == 0 && ((uintptr_t)objective % 8) == 0,
                 "U, V or objective is not aligned to 8 bytes");
    ObjLayout L;
    CSRK_TRY(obj_layout(a->nrows, a->ncols, k, implicit, &L));
    DevBuf dU, dV, dW, dR;
    CSRK_TRY(pack_panel(dU, U, ldu, k, 8, a->nrows));
    CSRK_TRY(pack_panel(dV, V, ldv, k, 8, a->ncols));
    CSRK_TRY(dW.alloc((size_t)L.total * 8));
    CSRK_TRY(dR.alloc(8));
    CSRK_TRY(obj_total_device(hA, hAt, dU.as<double>(), k, dV.as<double>(), k, k, scale, rhs_mode, implicit, lam, lam_n, dR.as<double>(), dW.p,
                              L.total * 8, nullptr));
    CSRK_HIP(hipMemcpy(objective, dR.p, 8, hipMemcpyDeviceToHost));
    return CSRK_OK;
}

}  // extern "C"
