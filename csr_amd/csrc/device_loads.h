// Device-side loads the kernels share, one copy each: the 16-byte vector types, an entry's value as float64, a unit of a
// panel row as float64, the lane ownership of a 64-column chunk of a panel row with its 16-B piece loads (SDDMM's and
// ALS-CG's order of addition hangs on it), and the lower bound in a sorted row.  Device code only: the host test
// programmes compile common.h and panel.h with the system compiler, so neither includes this.
#pragma once
#include "common.h"

namespace csrk {

// ---- vector types (naturally aligned; spmv_plan.h has the 4-byte-aligned variants its streams need) ----
typedef int32_t i32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef double f64x2_t __attribute__((ext_vector_type(2)));

// ---- the value of entry e as float64: float32 widened exactly, 1.0 (nothing read) for a structure-only matrix ----
__device__ __forceinline__ double csr_val(const void *v, int vt, int64_t e)
{
    if (vt == CSRK_VAL_F64) return ((const double *)v)[e];
    if (vt == CSRK_VAL_F32) return (double)((const float *)v)[e];
    return 1.0;
}

// ... with the value type a template argument
template <int VT>
__device__ __forceinline__ double csr_val(const void *v, int64_t e)
{
    if (VT == CSRK_VAL_F64) return ((const double *)v)[e];
    if (VT == CSRK_VAL_F32) return (double)((const float *)v)[e];
    return 1.0;
}

// ... for a caller that has already established that the matrix stores values (vt is F64 or F32).  Not folded into
// csr_val: the third way costs a scalar register there and moves some 17 000 lines of gram.hip's assembly.
__device__ __forceinline__ double csr_stored_val(const void *v, int vt, int64_t e)
{
    return vt == CSRK_VAL_F64 ? ((const double *)v)[e] : (double)((const float *)v)[e];
}

// ---- one unit of a panel row as float64: PER elements (a 16-B piece when PER > 1, else one element) ----
template <class T, int PER> __device__ __forceinline__ void panel_unit(const T *__restrict__ p, double d[PER]);
template <> __device__ __forceinline__ void panel_unit<double, 1>(const double *__restrict__ p, double d[1]) { d[0] = *p; }
template <> __device__ __forceinline__ void panel_unit<float, 1>(const float *__restrict__ p, double d[1]) { d[0] = (double)*p; }
template <> __device__ __forceinline__ void panel_unit<double, 2>(const double *__restrict__ p, double d[2])
{
    const f64x2_t a = *(const f64x2_t *)p;
    d[0] = a.x, d[1] = a.y;
}
template <> __device__ __forceinline__ void panel_unit<float, 4>(const float *__restrict__ p, double d[4])
{
    const f32x4_t a = *(const f32x4_t *)p;
    d[0] = (double)a.x, d[1] = (double)a.y, d[2] = (double)a.z, d[3] = (double)a.w;
}

// ---- a panel row over a group of PANEL_G lanes (one DPP row), four columns per lane and 64-column chunk ----
constexpr int PANEL_G = 16;

// A lane's four columns in a 64-column chunk are 16-B pieces of PIECE = 16 / sizeof(T) elements: float64 columns
// 2 l, 2 l + 1, 32 + 2 l, 33 + 2 l; float32 columns 4 l .. 4 l + 3.  So each load instruction of a group reads one
// contiguous 256-B span of a panel row.  Element q (0..3) of lane l:
template <class T>
__device__ __forceinline__ int panel_off(int sub, int q)
{
    constexpr int PIECE = 16 / (int)sizeof(T);
    return (q / PIECE) * (PANEL_G * PIECE) + sub * PIECE + q % PIECE;
}

// one 16-B piece, p 16-B aligned
__device__ __forceinline__ void panel_piece(const double *p, double *d)
{
    const f64x2_t a = *(const f64x2_t *)p;
    d[0] = a.x, d[1] = a.y;
}
__device__ __forceinline__ void panel_piece(const float *p, float *d)
{
    const f32x4_t a = *(const f32x4_t *)p;
    d[0] = a.x, d[1] = a.y, d[2] = a.z, d[3] = a.w;
}

// the lane's four elements of one 64-column chunk of a panel row (p = the chunk's first column; kk = columns left from
// it); columns at or past k read as 0 and are never added.  WIDE: 16-B loads for whole pieces (aligned by the caller).
template <class T, bool WIDE>
__device__ __forceinline__ void panel_load4(const T *__restrict__ p, int sub, int kk, T d[4])
{
    constexpr int PIECE = 16 / (int)sizeof(T);
#pragma unroll
    for (int q0 = 0; q0 < 4; q0 += PIECE) {
        const int o = panel_off<T>(sub, q0);
        if (WIDE && o + PIECE <= kk) {
            panel_piece(p + o, d + q0);
        } else {
#pragma unroll
            for (int i = 0; i < PIECE; i++) d[q0 + i] = o + i < kk ? p[o + i] : (T)0;
        }
    }
}

// ---- the first position in [lo, hi) of the ascending c whose element is not below key (hi when there is none) ----
template <class C, class I>
__device__ __forceinline__ I first_not_below(const C *c, I lo, I hi, int32_t key)
{
    while (lo < hi) {
        const I mid = lo + ((hi - lo) >> 1);
        if (c[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

}  // namespace csrk
