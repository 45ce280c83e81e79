// Entry-wise combination of two CSR matrices on gfx950: csrk_combine gives A + B (alpha a + beta b over the union of the
// patterns), A o B (a b over their intersection), or the entries of A whose position B stores (keep) or does not (drop).
// The contract is in include/csrk.h.
//
// Two passes over the operands with the row-pointer scan between them -- COUNT, then PLACE -- and no merge loop: every
// entry finds its own place with one binary search in the other operand's row (a canonical row: strictly ascending
// columns), which stays in L1 / L2 while the row's wavefront or workgroup is at work.
//   m(i)     the A entry at position i has its column in B's row: B[lb_B(c)] == c, lb_X(c) = the entries of row X below c
//   M(i)     m over A[0 .. i): a ballot prefix count inside a wavefront, wave totals through LDS inside a workgroup, and an
//            offset carried from one chunk of the row to the next
//   count    add: len_a + len_b - M(len_a);  multiply, keep: M(len_a);  drop: len_a - M(len_a)
//   place    add: A[i] -> i + lb_B(c) - M(i); a B entry at j that A lacks -> j + lb_A(c) - (B's matches before j)
//            multiply, keep: a matching A[i] -> M(i);  drop: the others -> i - M(i)
// keep and drop only ask "is c in B's row", so A may be unsorted and repeat columns; its entries stay in storage order.
// Every slot is counted: nothing is appended in arrival order, no atomic touches a result, and the value arithmetic
// (add, multiply) is one or two roundings per entry -- the result is a function of (A, B, op, alpha, beta).
//
// Row classes by len_a + len_b:
//   0 .. CB_WAVE_MAX     one WAVEFRONT per row, in chunks of 64 entries (no LDS, no barrier)
//   above                one CB_THREADS-thread WORKGROUP per listed row, in chunks of CB_THREADS entries, one barrier each
// Column indices are compared and copied, never used as addresses.
#include "device_loads.h"
#include "result.h"
#include "wave.h"

#include <functional>

namespace csrk {

constexpr int CB_THREADS = 256;         // workgroup of the long class = its chunk of a row
constexpr int CB_WAVE_MAX = 512;        // longest len_a + len_b one wavefront takes (8 chunks)
constexpr int CB_NW = CB_THREADS / WAVE;

struct CbArgs {
    const void *rpa, *rpb;              // row pointers (int32 or int64: pa64 / pb64)
    const int32_t *ca, *cb;
    const void *va, *vb;                // values (vta / vtb: CSRK_VAL_*)
    int pa64, pb64, vta, vtb, op;
    int32_t nrows;
    double alpha, beta;
    const int32_t *list;                // the long rows (workgroup class)
    int64_t *cnt;                       // COUNT: the result's row lengths
    const int64_t *off;                 // PLACE: the result's row offsets
    int32_t *oc;
    void *ov;
};

// the entries of c[0 .. n) below key (c strictly ascending); the probes stay inside [0, n) whatever c holds
__device__ __forceinline__ uint32_t cb_lower(const int32_t *__restrict__ c, uint32_t n, int32_t key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;      // n <= 2^31 - 1: no wrap
        if (c[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// One row by a group of NT threads (NT = 64: a wavefront, no barrier; NT = CB_THREADS: the workgroup, s_tot = 2 * CB_NW words).
template <int NT, bool PLACE>
__device__ __forceinline__ void cb_row(const CbArgs &g, int64_t r, int t, uint32_t *s_tot)
{
    // No FMA contraction here: add's contract rounds alpha a and beta b on their own before the sum is rounded.  hipcc
    // compiles device code with -ffp-contract=fast, and the rounding intrinsics (__dmul_rn, __dadd_rn) are plain * and +
    // that fuse after inlining (csrc/spmv.hip, the light-stream kernel); the pragma governs the operators written in
    // this body.
#pragma clang fp contract(off)
    const int lane = t & (WAVE - 1), w = t / WAVE;
    const unsigned long long below = lane ? (~0ull >> (WAVE - lane)) : 0ull;
    const int64_t spa = load_ptr(g.rpa, g.pa64, r), spb = load_ptr(g.rpb, g.pb64, r);
    const uint32_t la = (uint32_t)(load_ptr(g.rpa, g.pa64, r + 1) - spa), lb = (uint32_t)(load_ptr(g.rpb, g.pb64, r + 1) - spb);
    const int32_t *__restrict__ ca = g.ca + spa;
    const int32_t *__restrict__ cb = g.cb + spb;
    const int op = g.op;
    int it = 0;                                       // barriers so far: the parity of the LDS totals
    // exclusive prefix count of `f` over the group's threads (`pre`) and its total (`tot`); uniform over the group
    auto count = [&](bool f, uint32_t &pre, uint32_t &tot) {
        const unsigned long long bal = __ballot(f);
        pre = (uint32_t)__popcll(bal & below);
        tot = (uint32_t)__popcll(bal);
        if constexpr (NT > WAVE) {
            uint32_t *s = s_tot + (it & 1) * CB_NW;   // (two sets: a wavefront may be a barrier ahead of the slowest reader)
            if (lane == 0) s[w] = tot;
            __syncthreads();
            tot = 0;
#pragma unroll
            for (int q = 0; q < CB_NW; q++) {
                const uint32_t x = s[q];
                if (q < w) pre += x;
                tot += x;
            }
            it++;
        }
    };
    const int64_t ob = PLACE ? g.off[r] : 0;
    uint32_t M = 0;                                   // matches among the entries of A before this chunk
    for (uint32_t base = 0; base < la; base += NT) {
        const uint32_t i = base + t;
        const bool in = i < la;
        const int32_t c = in ? ca[i] : 0;
        const uint32_t p = in ? cb_lower(cb, lb, c) : 0;
        const bool m = in && p < lb && cb[p] == c;
        uint32_t pre, tot;
        count(m, pre, tot);
        if (PLACE && in) {
            const uint32_t mi = M + pre;              // M(i)
            if (op == CSRK_COMBINE_ADD) {
                const int64_t o = ob + ((int64_t)i + p - mi);
                const double pa = g.alpha * csr_val(g.va, g.vta, spa + i);
                double v = pa;
                if (m) {
                    const double pb = g.beta * csr_val(g.vb, g.vtb, spb + p);
                    v = pa + pb;
                }
                g.oc[o] = c;
                ((double *)g.ov)[o] = v;
            } else if (op == CSRK_COMBINE_MUL) {
                if (m) {
                    const int64_t o = ob + mi;
                    g.oc[o] = c;
                    ((double *)g.ov)[o] = csr_val(g.va, g.vta, spa + i) * csr_val(g.vb, g.vtb, spb + p);
                }
            } else if (m == (op == CSRK_COMBINE_KEEP)) {      // keep: the matches; drop: the others
                const int64_t o = ob + (op == CSRK_COMBINE_KEEP ? (int64_t)mi : (int64_t)i - mi);
                g.oc[o] = c;
                // the value's bits, whatever they are (an integer move: NaN payloads and -0.0 included)
                if (g.vta == CSRK_VAL_F64)
                    ((uint64_t *)g.ov)[o] = ((const uint64_t *)g.va)[spa + i];
                else if (g.vta == CSRK_VAL_F32)
                    ((uint32_t *)g.ov)[o] = ((const uint32_t *)g.va)[spa + i];
            }
        }
        M += tot;
    }
    if (!PLACE) {
        if (t == 0) {
            int64_t n;
            if (op == CSRK_COMBINE_ADD)
                n = (int64_t)la + lb - M;
            else if (op == CSRK_COMBINE_DROP)
                n = (int64_t)la - M;
            else
                n = M;
            g.cnt[r] = n;
        }
        return;
    }
    if (op != CSRK_COMBINE_ADD) return;
    // add: the entries of B that A lacks
    uint32_t MB = 0;
    for (uint32_t base = 0; base < lb; base += NT) {
        const uint32_t j = base + t;
        const bool in = j < lb;
        const int32_t c = in ? cb[j] : 0;
        const uint32_t p = in ? cb_lower(ca, la, c) : 0;
        const bool m = in && p < la && ca[p] == c;
        uint32_t pre, tot;
        count(m, pre, tot);
        if (in && !m) {
            const int64_t o = ob + ((int64_t)j + p - (MB + pre));
            g.oc[o] = c;
            ((double *)g.ov)[o] = g.beta * csr_val(g.vb, g.vtb, spb + j);
        }
        MB += tot;
    }
}

// every row is visited: the wavefront class is done here (the empty rows get their count here too), the rest is listed
template <bool PLACE>
__global__ __launch_bounds__(256) void combine_wave_kernel(const CbArgs g)
{
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    if (r >= g.nrows) return;                         // (whole wavefronts leave together)
    const int64_t len = (load_ptr(g.rpa, g.pa64, r + 1) - load_ptr(g.rpa, g.pa64, r)) +
                        (load_ptr(g.rpb, g.pb64, r + 1) - load_ptr(g.rpb, g.pb64, r));
    if (len > CB_WAVE_MAX) return;                    // the workgroup kernel's
    cb_row<WAVE, PLACE>(g, r, threadIdx.x & (WAVE - 1), nullptr);
}

template <bool PLACE>
__global__ __launch_bounds__(CB_THREADS) void combine_block_kernel(const CbArgs g)
{
    __shared__ uint32_t s_tot[2 * CB_NW];
    cb_row<CB_THREADS, PLACE>(g, (int64_t)g.list[blockIdx.x], threadIdx.x, s_tot);
}

// the long rows' flags, and a flag for a row no 32-bit count can hold
__global__ __launch_bounds__(256) void combine_class_kernel(const CbArgs g, int32_t *__restrict__ is_long, int32_t *__restrict__ bad)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= g.nrows) return;
    const int64_t la = load_ptr(g.rpa, g.pa64, r + 1) - load_ptr(g.rpa, g.pa64, r);
    const int64_t lb = load_ptr(g.rpb, g.pb64, r + 1) - load_ptr(g.rpb, g.pb64, r);
    if (la < 0 || la > INT32_MAX || lb < 0 || lb > INT32_MAX) atomicOr(bad, 1);
    is_long[r] = la + lb > CB_WAVE_MAX ? 1 : 0;
}

__global__ __launch_bounds__(256) void combine_list_kernel(const CbArgs g, const int32_t *__restrict__ pos, int32_t *__restrict__ list)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= g.nrows) return;
    const int64_t len = (load_ptr(g.rpa, g.pa64, r + 1) - load_ptr(g.rpa, g.pa64, r)) +
                        (load_ptr(g.rpb, g.pb64, r + 1) - load_ptr(g.rpb, g.pb64, r));
    if (len > CB_WAVE_MAX) list[pos[r]] = (int32_t)r;
}

static int combine_impl(Matrix *a, Matrix *b, int op, double alpha, double beta, int vt, Matrix **out)
{
    const int32_t nrows = a->nrows;
    const unsigned gr = (unsigned)ceil_div((int64_t)nrows, 256);
    const unsigned gw = (unsigned)ceil_div((int64_t)nrows * WAVE, 256);
    DevBuf lpos, cnt, bad, list;
    CSRK_TRY(lpos.alloc((size_t)(nrows + 1) * 4));
    CSRK_TRY(cnt.alloc((size_t)(nrows + 1) * 8));
    CSRK_TRY(bad.alloc(4));
    DrainOnExit drain_on_exit;      // (before the buffers above go back to the pool)
    CbArgs g{};
    g.rpa = a->d_rowptrs, g.rpb = b->d_rowptrs;
    g.ca = a->d_colinds, g.cb = b->d_colinds;
    g.va = a->d_values, g.vb = b->d_values;
    g.pa64 = a->ptr64, g.pb64 = b->ptr64, g.vta = a->val_type, g.vtb = b->val_type, g.op = op;
    g.nrows = nrows;
    g.alpha = alpha, g.beta = beta;
    g.cnt = cnt.as<int64_t>();
    CSRK_HIP(hipMemsetAsync(bad.p, 0, 4, nullptr));
    combine_class_kernel<<<gr, 256>>>(g, lpos.as<int32_t>(), bad.as<int32_t>());
    CSRK_LAUNCH_CHECK();
    int32_t n_long = 0, is_bad = 0;
    CSRK_TRY(scan_total(lpos.as<int32_t>(), nrows, &n_long));
    CSRK_HIP(hipMemcpy(&is_bad, bad.p, 4, hipMemcpyDeviceToHost));
    if (is_bad) {
        set_error("combine: a row holds more than 2^31 - 1 entries");
        return CSRK_ERR_UNSUPPORTED;
    }
    if (n_long > 0) {
        CSRK_TRY(list.alloc((size_t)n_long * 4));
        combine_list_kernel<<<gr, 256>>>(g, lpos.as<int32_t>(), list.as<int32_t>());
        CSRK_LAUNCH_CHECK();
        g.list = list.as<int32_t>();
        combine_block_kernel<false><<<(unsigned)n_long, CB_THREADS>>>(g);      // the long rows first: the call's tail
        CSRK_LAUNCH_CHECK();
    }
    combine_wave_kernel<false><<<gw, 256>>>(g);
    CSRK_LAUNCH_CHECK();
    int64_t total = 0;
    CSRK_TRY(scan_total(cnt.as<int64_t>(), nrows, &total));
    Matrix *t = nullptr;
    CSRK_TRY(new_matrix(nrows, a->ncols, total, total > INT32_MAX, vt, &t));
    write_rowptrs(cnt.as<int64_t>(), nrows, t);
    if (total > 0) {
        g.off = cnt.as<int64_t>();
        g.cnt = nullptr;
        g.oc = t->d_colinds;
        g.ov = t->d_values;
        if (n_long > 0) combine_block_kernel<true><<<(unsigned)n_long, CB_THREADS>>>(g);
        combine_wave_kernel<true><<<gw, 256>>>(g);
    }
    CSRK_TRY(finish_result(t, "combine"));
    *out = t;
    return CSRK_OK;
}

}  // namespace csrk

using namespace csrk;

extern "C" {

int csrk_combine_limits(int64_t *out, int n)
{
    CSRK_REQUIRE(out && n >= 0, "out is NULL");
    const int64_t v[3] = {WAVE, CB_THREADS, CB_WAVE_MAX};
    for (int i = 0; i < n && i < 3; i++) out[i] = v[i];
    return CSRK_OK;
}

int csrk_combine(csrk_handle_t ah, csrk_handle_t bh, int op, double alpha, double beta, csrk_handle_t *out)
{
    CSRK_REQUIRE(out, "out is NULL");
    *out = 0;
    Matrix *a = from_handle(ah);
    if (!a) return CSRK_ERR_INVALID;
    Matrix *b = from_handle(bh);
    if (!b) return CSRK_ERR_INVALID;
    CSRK_REQUIRE(op >= CSRK_COMBINE_ADD && op <= CSRK_COMBINE_DROP, "combine: unknown op %d", op);
    CSRK_REQUIRE(a->nrows == b->nrows && a->ncols == b->ncols, "combine: A is %d x %d and B is %d x %d", a->nrows, a->ncols,
                 b->nrows, b->ncols);
    CSRK_REQUIRE(a->device == b->device, "combine: the operands live on devices %d and %d", a->device, b->device);
    // both handles' locks, in one fixed order (by address) so that combine(a, b) and combine(b, a) cannot wait for each other
    std::unique_lock<std::mutex> l1, l2;
    if (a == b) {
        l1 = std::unique_lock<std::mutex>(a->mu);
    } else {
        Matrix *first = std::less<Matrix *>()(a, b) ? a : b, *second = first == a ? b : a;
        l1 = std::unique_lock<std::mutex>(first->mu);
        l2 = std::unique_lock<std::mutex>(second->mu);
    }
    const bool mask = op == CSRK_COMBINE_KEEP || op == CSRK_COMBINE_DROP;
    const int vt = mask ? a->val_type : CSRK_VAL_F64;
    Matrix *t = nullptr;
    if (a->nrows == 0 || (a->nnz == 0 && b->nnz == 0)) {      // an empty result; nothing is launched
        CSRK_TRY(empty_matrix(a->nrows, a->ncols, vt, "combine", &t));
        *out = to_handle(t);
        return CSRK_OK;
    }
    if (!mask) CSRK_TRY(ensure_canonical(a, "A"));
    CSRK_TRY(ensure_canonical(b, "B"));
    CSRK_TRY(combine_impl(a, b, op, alpha, beta, vt, &t));
    *out = to_handle(t);
    return CSRK_OK;
}

}  // extern "C"
