// ALS sweeps on the device for libcsrk: csrk_als_fit keeps both factor panels in HBM for any number of sweeps and runs
// each half-step, each V^T V and each objective there (include/csrk.h, rule F).  A host driver: rule F DEFINES the result as
// the public device entries csrk_panel_gram_device, csrk_als_rows_device, csrk_als_rows_cg_device and
// csrk_als_objective_device called in a fixed order on one stream, so this file calls exactly those and adds one kernel,
// the count of the exact solver's rows with a bad pivot.  Everything a part could refuse is refused here before the first
// launch, so a refused fit has written nothing.
#include "common.h"
#include "panel.h"

namespace csrk {

constexpr int FIT_K_MAX = 128;           // the smallest of the parts' limits (each is at least 128)
constexpr int FIT_COUNT_THREADS = 256;

// *bad += the rows of info[0 .. n) that are not 0: one integer atomic per bad row
__global__ __launch_bounds__(FIT_COUNT_THREADS) void fit_count_bad_kernel(const int32_t *__restrict__ info, int64_t n,
                                                                          unsigned long long *__restrict__ bad)
{
    const int64_t i = (int64_t)blockIdx.x * FIT_COUNT_THREADS + threadIdx.x;
    if (i < n && info[i] != 0) atomicAdd(bad, 1ull);
}

// the workspace in bytes, in the order it is laid out (every part 16-B aligned)
struct FitLayout {
    int64_t base, pg, info, obj, total;
    int64_t pg_bytes, obj_bytes;
};

static int64_t up16(int64_t b) { return (b + 15) & ~(int64_t)15; }

static int fit_layout(int32_t nrows, int32_t ncols, int32_t k, int solver, int implicit, int with_objective, FitLayout *L)
{
    const int64_t big = nrows > ncols ? nrows : ncols;
    int64_t o = 0;
    L->base = o, o += up16((int64_t)k * k * 8);
    L->pg_bytes = 0;
    if (implicit) CSRK_TRY(csrk_panel_gram_workspace(big, k, &L->pg_bytes));
    L->pg = o, o += up16(L->pg_bytes);
    L->info = o, o += solver == 0 ? up16(big * 4) : 0;
    L->obj_bytes = 0;
    if (with_objective) CSRK_TRY(csrk_als_objective_workspace(nrows, ncols, k, implicit, &L->obj_bytes));
    L->obj = o, o += up16(L->obj_bytes);
    L->total = o;
    return CSRK_OK;
}

static int fit_check_scalars(int32_t k, int32_t sweeps, int solver, int32_t cg_steps, double tol2, int scale, int rhs_mode, int implicit,
                             int64_t ldu, int64_t ldv)
{
    CSRK_CHECK_K("", k);
    CSRK_CHECK_TWO_PANELS("", k, ldu, ldv);
    CSRK_REQUIRE(sweeps >= 0, "sweeps must not be negative (sweeps=%d)", sweeps);
    CSRK_REQUIRE(solver == 0 || solver == 1, "solver must be 0 (exact) or 1 (cg), not %d", solver);
    CSRK_CHECK_SCALE(scale);
    CSRK_REQUIRE(rhs_mode == CSRK_ALS_RHS_ONES || rhs_mode == CSRK_ALS_RHS_VALUES || rhs_mode == CSRK_ALS_RHS_ONE_PLUS,
                 "rhs_mode must be CSRK_ALS_RHS_ONES, _VALUES or _ONE_PLUS, not %d", rhs_mode);
    CSRK_REQUIRE(implicit == 0 || implicit == 1, "implicit must be 0 or 1, not %d", implicit);
    CSRK_REQUIRE(solver == 0 || cg_steps >= 0, "steps must not be negative (steps=%d)", cg_steps);
    CSRK_REQUIRE(solver == 0 || tol2 >= 0.0, "tol2 must be a number that is not negative (tol2=%g)", tol2);      // (false for NaN)
    if (k > FIT_K_MAX) {
        set_error("csrk_als_fit: k=%d is above the largest supported k=%d", k, FIT_K_MAX);
        return CSRK_ERR_UNSUPPORTED;
    }
    return CSRK_OK;
}

// do the byte ranges [p, p + pb) and [q, q + qb) meet?  fit_span: the bytes a panel of `rows` rows reaches over
static bool fit_overlap(const void *p, int64_t pb, const void *q, int64_t qb)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return pb > 0 && qb > 0 && a < b + (uintptr_t)qb && b < a + (uintptr_t)pb;
}
static int64_t fit_span(int64_t rows, int64_t ld, int32_t k) { return rows > 0 ? ((rows - 1) * ld + k) * 8 : 0; }

static int fit_device(csrk_handle_t hA, csrk_handle_t hAt, int32_t k, int32_t sweeps, int solver, int32_t cg_steps, double tol2, int scale,
                      int rhs_mode, int implicit, double lam, double lam_n, double *dU, int64_t ldu, double *dV, int64_t ldv,
                      double *dobj, int64_t *dbad, void *dwork, int64_t work_bytes, hipStream_t s)
{
    CSRK_TRY(fit_check_scalars(k, sweeps, solver, cg_steps, tol2, scale, rhs_mode, implicit, ldu, ldv));
    Matrix *a = from_handle(hA);
    if (!a) return CSRK_ERR_INVALID;
    Matrix *at = from_handle(hAt);
    if (!at) return CSRK_ERR_INVALID;
    CSRK_TRY(check_transpose_shape(a, at));
    const int32_t nrows = a->nrows, ncols = a->ncols;
    CSRK_REQUIRE((dU || nrows == 0) && (dV || ncols == 0), "U or V is NULL");
    CSRK_REQUIRE(((uintptr_t)dU % 8) == 0 && ((uintptr_t)dV % 8) == 0 && ((uintptr_t)dobj % 8) == 0 && ((uintptr_t)dbad % 8) == 0 &&
                     ((uintptr_t)dwork % 16) == 0,
                 "U, V, objective or bad is not aligned to 8 bytes, or the workspace to 16");
    FitLayout L;
    CSRK_TRY(fit_layout(nrows, ncols, k, solver, implicit, dobj != nullptr, &L));
    CSRK_REQUIRE(dwork && work_bytes >= L.total, "the workspace is NULL or too small: %lld bytes, csrk_als_fit_workspace asks for %lld",
                 (long long)work_bytes, (long long)L.total);
    const int64_t ub = fit_span(nrows, ldu, k), vb = fit_span(ncols, ldv, k);
    CSRK_REQUIRE(!fit_overlap(dU, ub, dV, vb) && !fit_overlap(dU, ub, dwork, L.total) && !fit_overlap(dV, vb, dwork, L.total),
                 "U, V and the workspace overlap");

    char *w = (char *)dwork;
    double *base = (double *)(w + L.base);
    int32_t *info = (int32_t *)(w + L.info);
    void *pgw = L.pg_bytes ? (void *)(w + L.pg) : nullptr;
    const bool exact = solver == 0;

    // rule F's base_for(P): NULL, or the workspace's k x k block filled by csrk_panel_gram_device
    auto base_for = [&](const double *P, int64_t rows, int64_t ld, const double **out) -> int {
        *out = nullptr;
        if (implicit) {
            CSRK_TRY(csrk_panel_gram_device(rows, k, P, ld, CSRK_VAL_F64, exact ? lam : 0.0, base, pgw, L.pg_bytes, s));
            *out = base;
        } else if (exact && lam != 0.0) {
            CSRK_TRY(csrk_panel_gram_device(0, k, nullptr, k, CSRK_VAL_F64, lam, base, nullptr, 0, s));
            *out = base;
        }
        return CSRK_OK;
    };
    // one half-step: X (the side of h's rows) from P (the other side); bad: its counter or NULL
    auto half = [&](csrk_handle_t h, int32_t rows, const double *P, int64_t prows, int64_t ldp, double *X, int64_t ldx, int64_t *bad) -> int {
        const double *B;
        CSRK_TRY(base_for(P, prows, ldp, &B));
        if (bad) CSRK_HIP(hipMemsetAsync(bad, 0, 8, s));
        if (exact) {
            CSRK_TRY(csrk_als_rows_device(h, 0, rows, P, ldp, k, CSRK_VAL_F64, scale, rhs_mode, B, lam_n, X, ldx, info, s));
            if (bad && rows > 0)
                fit_count_bad_kernel<<<(unsigned)ceil_div(rows, FIT_COUNT_THREADS), FIT_COUNT_THREADS, 0, s>>>(info, rows,
                                                                                                             (unsigned long long *)bad);
        } else {
            CSRK_TRY(csrk_als_rows_cg_device(h, 0, rows, P, ldp, k, CSRK_VAL_F64, scale, rhs_mode, B, lam, lam_n, cg_steps, tol2, X, ldx, X, ldx,
                                             nullptr, nullptr, s));
        }
        return CSRK_OK;
    };
    auto objective = [&](int32_t at_sweep) -> int {
        if (!dobj) return CSRK_OK;
        return csrk_als_objective_device(hA, hAt, dU, ldu, dV, ldv, k, scale, rhs_mode, implicit, lam, lam_n, dobj + at_sweep, w + L.obj,
                                         L.obj_bytes, s);
    };

    CSRK_TRY(objective(0));
    for (int32_t sw = 0; sw < sweeps; sw++) {
        CSRK_TRY(half(hA, nrows, dV, ncols, ldv, dU, ldu, dbad ? dbad + 2 * sw : nullptr));
        CSRK_TRY(half(hAt, ncols, dU, nrows, ldu, dV, ldv, dbad ? dbad + 2 * sw + 1 : nullptr));
        CSRK_TRY(objective(sw + 1));
    }
    CSRK_LAUNCH_CHECK();
    return CSRK_OK;
}

}  // namespace csrk

using namespace csrk;

extern "C" {

int csrk_als_fit_workspace(int32_t nrows, int32_t ncols, int32_t k, int solver, int implicit, int with_objective, int64_t *bytes)
{
    CSRK_REQUIRE(bytes, "bytes is NULL");
    CSRK_REQUIRE(nrows >= 0 && ncols >= 0, "bad shape %d x %d", nrows, ncols);
    CSRK_REQUIRE(with_objective == 0 || with_objective == 1, "with_objective must be 0 or 1, not %d", with_objective);
    CSRK_TRY(fit_check_scalars(k, 0, solver, 0, 0.0, 0, CSRK_ALS_RHS_ONES, implicit, k, k));
    FitLayout L;
    CSRK_TRY(fit_layout(nrows, ncols, k, solver, implicit, with_objective, &L));
    *bytes = L.total;
    return CSRK_OK;
}

int csrk_als_fit_device(csrk_handle_t hA, csrk_handle_t hAt, int32_t k, int32_t sweeps, int solver, int32_t cg_steps, double tol2, int scale,
                        int rhs_mode, int implicit, double lam, double lam_n, double *d_U, int64_t ldu, double *d_V, int64_t ldv,
                        double *d_objective, int64_t *d_bad, void *d_work, int64_t work_bytes, void *stream)
{
    return fit_device(hA, hAt, k, sweeps, solver, cg_steps, tol2, scale, rhs_mode, implicit, lam, lam_n, d_U, ldu, d_V, ldv, d_objective,
                      d_bad, d_work, work_bytes, (hipStream_t)stream);
}

int csrk_als_fit(csrk_handle_t hA, csrk_handle_t hAt, int32_t k, int32_t sweeps, int solver, int32_t cg_steps, double tol2, int scale,
                 int rhs_mode, int implicit, double lam, double lam_n, double *U, int64_t ldu, double *V, int64_t ldv, double *objective,
                 int64_t *bad)
{
    // argument checks first, with the caller's pointers (the device call below sees packed copies)
    CSRK_TRY(fit_check_scalars(k, sweeps, solver, cg_steps, tol2, scale, rhs_mode, implicit, ldu, ldv));
    Matrix *a = from_handle(hA);
    if (!a) return CSRK_ERR_INVALID;
    Matrix *at = from_handle(hAt);
    if (!at) return CSRK_ERR_INVALID;
    CSRK_TRY(check_transpose_shape(a, at));
    CSRK_REQUIRE((U || a->nrows == 0) && (V || a->ncols == 0), "U or V is NULL");
    CSRK_REQUIRE(((uintptr_t)U % 8) == 0 && ((uintptr_t)V % 8) == 0 && ((uintptr_t)objective % 8) == 0 && ((uintptr_t)bad % 8) == 0,
                 "U, V, objective or bad is not aligned to 8 bytes");
    CSRK_REQUIRE(!fit_overlap(U, fit_span(a->nrows, ldu, k), V, fit_span(a->ncols, ldv, k)), "U and V overlap");
    FitLayout L;
    CSRK_TRY(fit_layout(a->nrows, a->ncols, k, solver, implicit, objective != nullptr, &L));
    DevBuf dU, dV, dW, dJ, dB;
    CSRK_TRY(pack_panel(dU, U, ldu, k, 8, a->nrows));
    CSRK_TRY(pack_panel(dV, V, ldv, k, 8, a->ncols));
    CSRK_TRY(dW.alloc((size_t)L.total));
    CSRK_TRY(dJ.alloc((size_t)(sweeps + 1) * 8));
    CSRK_TRY(dB.alloc((size_t)sweeps * 16));
    CSRK_TRY(fit_device(hA, hAt, k, sweeps, solver, cg_steps, tol2, scale, rhs_mode, implicit, lam, lam_n, dU.as<double>(), k, dV.as<double>(),
                        k, objective ? dJ.as<double>() : nullptr, bad ? dB.as<int64_t>() : nullptr, dW.p, L.total, nullptr));
    CSRK_TRY(unpack_panel(U, ldu, dU, k, 8, a->nrows));
    CSRK_TRY(unpack_panel(V, ldv, dV, k, 8, a->ncols));
    if (objective) CSRK_HIP(hipMemcpy(objective, dJ.p, (size_t)(sweeps + 1) * 8, hipMemcpyDeviceToHost));
    if (bad && sweeps > 0) CSRK_HIP(hipMemcpy(bad, dB.p, (size_t)sweeps * 16, hipMemcpyDeviceToHost));
    return CSRK_OK;
}

}  // extern "C"
