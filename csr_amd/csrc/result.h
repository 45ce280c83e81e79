// Host-side steps shared by the operations that return a NEW matrix (csrk_combine, csrk_coalesce, csrk_topk_rows,
// csrk_filter_zeros, csrk_pick_rows; DESIGN.md section 8, "Building a result matrix"):
//   counts or flags -> scan_total -> new_matrix -> write_rowptrs / write_rowptrs_through -> the placing kernels -> finish_result
// with a DrainOnExit declared after the temporaries, and empty_matrix where nothing is launched.  The *_impl functions call
// these in a straight line; everything runs on the default stream.
#pragma once
#include "common.h"

namespace csrk {

// Declared after the DevBufs of a function: the device drains before they go back to the pool, on every way out (a way out
// that has drained the device itself disarms it).
struct DrainOnExit {
    bool armed = true;
    ~DrainOnExit()
    {
        if (armed) (void)hipDeviceSynchronize();
    }
};

// Exclusive scan of p[0 .. n) in place (p has n + 1 slots), then ONE blocking copy of the total p[n] to the host.
template <class C>
int scan_total(C *p, int64_t n, C *total)
{
    static_assert(sizeof(C) == 4 || sizeof(C) == 8, "int32_t or int64_t counts");
    if constexpr (sizeof(C) == 8)
        CSRK_TRY(exclusive_scan_i64((const int64_t *)p, (int64_t *)p, n, nullptr));
    else
        CSRK_TRY(exclusive_scan_i32((const int32_t *)p, (int32_t *)p, n, nullptr));
    CSRK_HIP(hipMemcpy(total, p + n, sizeof(C), hipMemcpyDeviceToHost));
    return CSRK_OK;
}

// t's row pointers (either width) from the offsets off[0 .. nr].  Like every launch here, checked by finish_result or
// CSRK_LAUNCH_CHECK.  (handle.hip)
void write_rowptrs(const int64_t *off, int64_t nr, Matrix *t);

// t's row pointers through a scan over m's entries: pos[rowptr[r]], or rowptr[r] itself for a copy (pos = NULL)
template <class P, class C, class PO>
__global__ __launch_bounds__(256) void rowptrs_through_kernel(const P *__restrict__ rp, int32_t nrows, const C *__restrict__ pos,
                                                             PO *__restrict__ orp)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > nrows) return;
    const int64_t s = (int64_t)rp[r];
    orp[r] = (PO)(pos ? (int64_t)pos[s] : s);
}

template <class P, class C>
void write_rowptrs_through(const Matrix *m, const C *pos, Matrix *t)
{
    const unsigned grid = (unsigned)ceil_div((int64_t)m->nrows + 1, 256);
    if (t->ptr64)
        rowptrs_through_kernel<P, C, int64_t><<<grid, 256>>>((const P *)m->d_rowptrs, m->nrows, pos, (int64_t *)t->d_rowptrs);
    else
        rowptrs_through_kernel<P, C, int32_t><<<grid, 256>>>((const P *)m->d_rowptrs, m->nrows, pos, (int32_t *)t->d_rowptrs);
}

// A result without entries: nrows + 1 zero row pointers (int32); nothing is launched.  `what` names the operation in the
// error ("<what> failed: ...").  (handle.hip)
int empty_matrix(int32_t nrows, int32_t ncols, int val_type, const char *what, Matrix **out);

// The end of an operation: the last launch error, then the device drains.  On failure the error is "<what> failed: ...",
// t is deleted (NULL: nothing to delete) and CSRK_ERR_HIP comes back.  (handle.hip)
int finish_result(Matrix *t, const char *what);

}  // namespace csrk
