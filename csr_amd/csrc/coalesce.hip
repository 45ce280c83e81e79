// The canonical form of a CSR matrix on gfx950: csrk_coalesce merges the entries of a row that share a column (SUM, FIRST,
// LAST, MAX, MIN) and leaves every row strictly ascending; csrk_is_canonical asks whether there is anything to do.  The
// contract is in include/csrk.h.
//
// Flat, one thread per ENTRY, like filter_zeros (rowops.hip) -- not a wavefront per row, which costs 6.6-9x the flat filter
// on the 2M-row power-law matrix:
//   LOOK    an entry whose column is not above its predecessor's does one binary search of the row pointers: where it
//           starts a row nothing is wrong; elsewhere the row is not canonical (the lowest such row comes back) and, where
//           the column is BELOW the predecessor's, not non-descending either.  One launch answers both questions; the handle
//           remembers them.
//   route 0 canonical: the arrays are copied.
//   route 1 non-descending: the members of a group already lie side by side in storage order.
//   route 2 anything else: two stable transposes (what csrk_order_columns does) put them side by side in storage order.
//   FLAG    entry e heads a group iff its column differs from its predecessor's or it starts a row (only an entry that equals
//           its predecessor searches the row pointers).
//   SCAN    pos = exclusive scan of the flags: pos[e] is the slot of the group that e heads, pos[nnz] the result's size,
//           pos[rowptr[r]] the result's row pointer.
//   PLACE   a head writes its column and walks its group forward while pos[e' + 1] == pos[e'], folding in storage order; the
//           others do nothing.  One lane walks one group on purpose: a left-to-right float sum has no parallel form with the
//           same bits.  (One column 10^6 times in one row is 10^6 dependent adds on one lane.)
// Every slot is counted, nothing is appended in arrival order and no atomic touches a value: the result is a function of
// (h, dup).  Column indices are compared and copied, never used as addresses.
#include "result.h"
#include "sort.h"

namespace csrk {

static thread_local int g_coalesce_route = 0;

// ---- LOOK -------------------------------------------------------------------------------------------------------------------
// res[0]: the lowest row that is not strictly ascending (INT32_MAX: none);  res[1]: 1 if some entry lies below its predecessor
// in the row.  Only flags come back.
template <class P>
__global__ __launch_bounds__(256) void coalesce_look_kernel(const P *__restrict__ rp, const int32_t *__restrict__ ci, int32_t nrows,
                                                           int64_t nnz, int32_t *__restrict__ res)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (e >= nnz) return;
    const int32_t a = ci[e - 1], b = ci[e];
    if (a < b) return;
    const int64_t r = last_at_or_below(rp, 0, (int64_t)nrows - 1, e);      // the row that holds e (nrows >= 1, rp[0] = 0 <= e)
    if ((int64_t)rp[r] == e) return;                  // starts a row
    atomicMin(res, (int32_t)r);
    if (b < a) atomicOr(res + 1, 1);
}

int look_at_rows(Matrix *m)
{
    if (m->canonical >= 0 && m->nondescending >= 0) return CSRK_OK;
    int32_t res[2] = {INT32_MAX, 0};
    if (m->nnz > 1 && m->nrows > 0) {
        DevBuf d;
        CSRK_TRY(d.alloc(8));
        CSRK_HIP(hipMemcpy(d.p, res, 8, hipMemcpyHostToDevice));
        const unsigned grid = (unsigned)ceil_div(m->nnz - 1, 256);
        if (m->ptr64)
            coalesce_look_kernel<int64_t><<<grid, 256>>>((const int64_t *)m->d_rowptrs, m->d_colinds, m->nrows, m->nnz, d.as<int32_t>());
        else
            coalesce_look_kernel<int32_t><<<grid, 256>>>((const int32_t *)m->d_rowptrs, m->d_colinds, m->nrows, m->nnz, d.as<int32_t>());
        CSRK_LAUNCH_CHECK();
        CSRK_HIP(hipMemcpy(res, d.p, 8, hipMemcpyDeviceToHost));      // (waits for the kernel: `d` may go back to the pool)
    }
    m->canonical = res[0] == INT32_MAX ? 1 : 0;
    m->noncanonical_row = res[0] == INT32_MAX ? -1 : res[0];
    m->nondescending = res[1] ? 0 : 1;
    return CSRK_OK;
}

int ensure_canonical(Matrix *m, const char *name)
{
    CSRK_TRY(look_at_rows(m));
    CSRK_REQUIRE(m->canonical == 1,
                 "combine: operand %s is not canonical: row %d is not strictly ascending in column (csrk_order_columns "
                 "sorts; repeated columns have to be merged by the caller)",
                 name, m->noncanonical_row);
    return CSRK_OK;
}

// ---- FLAG -------------------------------------------------------------------------------------------------------------------
template <class P, class C>
__global__ __launch_bounds__(256) void coalesce_flag_kernel(const P *__restrict__ rp, const int32_t *__restrict__ ci, int32_t nrows,
                                                           int64_t nnz, C *__restrict__ flags)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    bool head = true;
    if (e > 0 && ci[e] == ci[e - 1]) head = (int64_t)rp[last_at_or_below(rp, 0, (int64_t)nrows - 1, e)] == e;
    flags[e] = head ? 1 : 0;
}

// ---- PLACE ------------------------------------------------------------------------------------------------------------------
struct CoArgs {
    const int32_t *ci;                  // columns, the members of a group side by side (h's, or the sorted copy's)
    const void *vs;                     // their values (vti: CSRK_VAL_*; the sorted copy holds float32 values widened)
    const void *pos;                    // the scan (int32, or int64: pos64), nnz + 1 slots
    int vti, vto, dup, pos64;
    int64_t nnz;
    int32_t *oc;
    void *ov;                           // vto: h's value type
};

__device__ __forceinline__ int64_t co_pos(const CoArgs &g, int64_t e)
{
    return g.pos64 ? ((const int64_t *)g.pos)[e] : (int64_t)((const int32_t *)g.pos)[e];
}

// a value in the result's dtype T: its own bits, or a widened float32 narrowed back (exact)
template <class T>
__device__ __forceinline__ T co_val(const CoArgs &g, int64_t e)
{
    return g.vti == CSRK_VAL_F64 ? (T)((const double *)g.vs)[e] : (T)((const float *)g.vs)[e];
}

// a ranks strictly above b in csrk_topk_rows' order: larger first, NaN above everything, NaNs tied, -0.0 and +0.0 tied
template <class T>
__device__ __forceinline__ bool co_above(T a, T b)
{
    return a != a ? !(b != b) : a > b;
}

template <class T, class U>
__device__ __forceinline__ void co_fold(const CoArgs &g, int64_t e, int64_t o)
{
    const int dup = g.dup;
    T w = co_val<T>(g, e);              // SUM: the running sum; otherwise the member that stands for the group so far
    for (int64_t f = e + 1; dup != CSRK_DUP_FIRST && f < g.nnz && co_pos(g, f + 1) == co_pos(g, f); f++) {
        const T v = co_val<T>(g, f);
        if (dup == CSRK_DUP_SUM) {
            w = w + v;                  // one rounding in T (there is no multiply here: nothing for the compiler to contract)
        } else if (dup == CSRK_DUP_LAST) {
            w = v;
        } else if (dup == CSRK_DUP_MAX) {
            if (co_above(v, w)) w = v;          // a tie stays with the earlier member
        } else {
            if (!co_above(v, w)) w = v;         // MIN: the last of the order -- a tie goes to the later member
        }
    }
    // one vector store of the value's bits (an integer move unless an add made them: NaN payloads and -0.0 included)
    ((U *)g.ov)[o] = __builtin_bit_cast(U, w);
}

__global__ __launch_bounds__(256) void coalesce_place_kernel(const CoArgs g)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= g.nnz) return;
    const int64_t o = co_pos(g, e);
    if (co_pos(g, e + 1) == o) return;                // not a head
    g.oc[o] = g.ci[e];
    if (g.vto == CSRK_VAL_F64)
        co_fold<double, uint64_t>(g, e, o);
    else if (g.vto == CSRK_VAL_F32)
        co_fold<float, uint32_t>(g, e, o);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static void mark_canonical(Matrix *t)
{
    t->canonical = 1;
    t->noncanonical_row = -1;
    t->nondescending = 1;
}

// route 0: a device copy (the row pointers narrowed where h's are wider than the result needs)
template <class P>
static int copy_impl(Matrix *m, Matrix **out)
{
    Matrix *t = nullptr;
    CSRK_TRY(new_matrix(m->nrows, m->ncols, m->nnz, m->nnz > INT32_MAX, m->val_type, &t));
    write_rowptrs_through<P, int32_t>(m, nullptr, t);
    // (a copy that cannot be issued is the thread's last error, like a launch that cannot: finish_result reports either)
    (void)hipMemcpyAsync(t->d_colinds, m->d_colinds, (size_t)m->nnz * 4, hipMemcpyDeviceToDevice, nullptr);
    if (m->val_type != CSRK_VAL_NONE)
        (void)hipMemcpyAsync(t->d_values, m->d_values, (size_t)m->nnz * m->val_bytes(), hipMemcpyDeviceToDevice, nullptr);
    CSRK_TRY(finish_result(t, "coalesce"));
    *out = t;
    return CSRK_OK;
}

// routes 1 and 2: FLAG, SCAN, PLACE over the columns `ci` and values `vs` (vti), which hold every group side by side
template <class P, class C>
static int merge_impl(Matrix *m, const int32_t *ci, const void *vs, int vti, int dup, Matrix **out)
{
    const int64_t nnz = m->nnz;
    const unsigned grid = (unsigned)ceil_div(nnz, 256);
    DevBuf pos;
    CSRK_TRY(pos.alloc((size_t)(nnz + 1) * sizeof(C)));
    DrainOnExit drain_on_exit;      // (before `pos` goes back to the pool)
    coalesce_flag_kernel<P, C><<<grid, 256>>>((const P *)m->d_rowptrs, ci, m->nrows, nnz, pos.as<C>());
    CSRK_LAUNCH_CHECK();
    C total = 0;
    CSRK_TRY(scan_total(pos.as<C>(), nnz, &total));
    Matrix *t = nullptr;
    CSRK_TRY(new_matrix(m->nrows, m->ncols, (int64_t)total, (int64_t)total > INT32_MAX, m->val_type, &t));
    write_rowptrs_through<P, C>(m, pos.as<C>(), t);
    CoArgs g{};
    g.ci = ci, g.vs = vs, g.pos = pos.p;
    g.vti = vti, g.vto = m->val_type, g.dup = dup, g.pos64 = sizeof(C) == 8;
    g.nnz = nnz;
    g.oc = t->d_colinds, g.ov = t->d_values;
    coalesce_place_kernel<<<grid, 256>>>(g);
    CSRK_TRY(finish_result(t, "coalesce"));
    *out = t;
    return CSRK_OK;
}

template <class P>
static int merge_any(Matrix *m, const int32_t *ci, const void *vs, int vti, int dup, Matrix **out)
{
    return m->nnz >= INT32_MAX ? merge_impl<P, int64_t>(m, ci, vs, vti, dup, out) : merge_impl<P, int32_t>(m, ci, vs, vti, dup, out);
}

static int coalesce_impl(Matrix *m, int dup, int *route, Matrix **out)
{
    CSRK_TRY(look_at_rows(m));
    if (m->canonical == 1) {
        *route = 0;
        return m->ptr64 ? copy_impl<int64_t>(m, out) : copy_impl<int32_t>(m, out);
    }
    if (m->nondescending == 1) {
        *route = 1;
        return m->ptr64 ? merge_any<int64_t>(m, m->d_colinds, m->d_values, m->val_type, dup, out)
                        : merge_any<int32_t>(m, m->d_colinds, m->d_values, m->val_type, dup, out);
    }
    // Every row sorted by column, stably (sorted_rows_copy, as csrk_order_columns): t2 has h's row pointers, the columns
    // ascending and, among equal columns, h's storage order; its values are float64 (float32 widened exactly).
    *route = 2;
    Matrix *t2 = nullptr;
    CSRK_TRY(sorted_rows_copy(m, &t2));
    const int rc = m->ptr64 ? merge_any<int64_t>(m, t2->d_colinds, t2->d_values, t2->val_type, dup, out)
                  : merge_any<int32_t>(m, t2->d_colinds, t2->d_values, t2->val_type, dup, out);
    delete t2;                                        // (merge_impl drained the device)
    return rc;
}

}  // namespace csrk

using namespace csrk;

extern "C" {

int csrk_coalesce(csrk_handle_t h, int dup, csrk_handle_t *out)
{
    g_coalesce_route = 0;
    CSRK_REQUIRE(out, "out is NULL");
    *out = 0;
    Matrix *m = from_handle(h);
    if (!m) return CSRK_ERR_INVALID;
    CSRK_REQUIRE(dup >= CSRK_DUP_SUM && dup <= CSRK_DUP_MIN, "coalesce: unknown dup %d", dup);
    std::lock_guard<std::mutex> lk(m->mu);
    Matrix *t = nullptr;
    int route = 0;
    if (m->nrows == 0 || m->nnz == 0)                 // an empty result; nothing is launched
        CSRK_TRY(empty_matrix(m->nrows, m->ncols, m->val_type, "coalesce", &t));
    else
        CSRK_TRY(coalesce_impl(m, dup, &route, &t));
    mark_canonical(t);
    g_coalesce_route = route;
    *out = to_handle(t);
    return CSRK_OK;
}

int csrk_coalesce_last_route(int *route)
{
    CSRK_REQUIRE(route, "route is NULL");
    *route = g_coalesce_route;
    return CSRK_OK;
}

int csrk_is_canonical(csrk_handle_t h, int *canonical, int32_t *first_bad_row)
{
    CSRK_REQUIRE(canonical, "canonical is NULL");
    *canonical = 0;
    if (first_bad_row) *first_bad_row = -1;
    Matrix *m = from_handle(h);
    if (!m) return CSRK_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    CSRK_TRY(look_at_rows(m));
    *canonical = m->canonical;
    if (first_bad_row) *first_bad_row = m->noncanonical_row;
    return CSRK_OK;
}

}  // extern "C"
