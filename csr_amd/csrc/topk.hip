// Row top-k of libcsrk on gfx950: csrk_topk_rows keeps, in every row, the k largest entries that pass a threshold
// (the contract is in include/csrk.h).  Selection and copying only: no arithmetic touches a value.
//
// The order is a KEY (topk_order.h): a value becomes a 64-bit unsigned integer that sorts like the contract's total order
// (NaN -> all ones, -0.0 -> +0.0, then the usual sign flip; float32 is widened exactly first), and an entry beats another
// when its key is larger, or equal with an earlier position in the row.  An entry that fails the threshold gets key 0,
// below every real key (the smallest is -Inf's, 0x000fffffffffffff).
//
// Three row classes:
//   short   1 .. 64 entries     one WAVEFRONT per row, one entry per lane: an entry's rank is the number of entries that beat
//                               it, counted all-pairs with v_readlane (no LDS).  The rank is the output slot in by-value
//                               order, a ballot prefix count the slot in storage order.  One read, one write.
//   medium  65 .. 1024          one 256-thread WORKGROUP per listed row, 20 KiB of LDS (8 workgroups per CU), and
//   large   1025 .. any length  one 512-thread workgroup per listed row, 57 KiB (2 per CU): the same kernel.  MSB-first radix
//                               select over 11-bit digits on an LDS histogram (integer LDS atomics: order-free) finds the k-th
//                               key T and how many of its ties are taken; the passes re-read the row (it stays in the XCD's
//                               L2 while one workgroup works on it) until at most CAP candidates are left (1024 / 4096),
//                               which the next pass gathers into LDS for the remaining digits -- a row of at most CAP
//                               entries (every medium row) is gathered by the first pass and read from memory once.
//                               Placement is one more pass in storage order: a ballot / LDS scan gives every winner its
//                               slot (ties by position: the earliest), winners go straight out in storage order, or as
//                               (key, position) into LDS, through a bitonic network, and out in rank order.  More than
//                               TK_CAP winners in by-value order take the same network on a scratch array in memory
//                               (slow, general).
// The winners are written at offsets bounded by min(k, row length), known from the row pointers alone, so that no row is
// selected twice; rows that keep fewer (threshold) are then closed up by one copy of the RESULT (k entries per row, not
// the input).  When every row keeps its bound the bounded arrays ARE the result.
// No float atomic, no unordered append decides a winner or its place: the result is a function of the inputs.
#include "result.h"
#include "topk_order.h"
#include "wave.h"

namespace csrk {

constexpr int TK_SHORT = 64;            // longest row of the wavefront class
constexpr int TK_MID = 1024;            // longest row of the medium class: 256 threads, the whole row in LDS (20 KiB: 8 workgroups per CU)
constexpr int TK_MID_THREADS = 256;
constexpr int TK_THREADS = 512;         // workgroup of the large class
constexpr int TK_CAP = 4096;            // candidates / winners a large-class workgroup holds in LDS (key 8 B + position 4 B: 48 KiB)
constexpr int TK_BITS = 11;             // radix-select digit
constexpr int TK_BINS = 1 << TK_BITS;
constexpr int TK_UNROLL = 4;             // entries a thread of the long class loads before it uses the first
constexpr uint32_t TK_ALL = 0xffffffffu;          // "every tie is taken"

__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int lane)      // `lane` uniform over the wavefront
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

// bound[i] = min(k, row length) (the room row i gets), the row's class, and a flag for a row no 32-bit count can hold
template <class P>
__global__ __launch_bounds__(256) void topk_bound_kernel(const P *__restrict__ rp, int32_t nrows, int64_t k,
                                                        int64_t *__restrict__ bound, int32_t *__restrict__ is_mid,
                                                        int32_t *__restrict__ is_big, int32_t *__restrict__ bad)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const int64_t len = (int64_t)rp[r + 1] - (int64_t)rp[r];
    if (len < 0 || len > INT32_MAX) atomicOr(bad, 1);
    bound[r] = len < k ? (len < 0 ? 0 : len) : k;
    is_mid[r] = len > TK_SHORT && len <= TK_MID ? 1 : 0;
    is_big[r] = len > TK_MID ? 1 : 0;
}

// the medium and the large rows, ascending (pos_* = the exclusive scans of the class flags)
template <class P>
__global__ __launch_bounds__(256) void topk_list_kernel(const P *__restrict__ rp, int32_t nrows, const int32_t *__restrict__ pos_mid,
                                                       const int32_t *__restrict__ pos_big, int32_t *__restrict__ list_mid,
                                                       int32_t *__restrict__ list_big)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const int64_t len = (int64_t)rp[r + 1] - (int64_t)rp[r];
    if (len > TK_MID)
        list_big[pos_big[r]] = (int32_t)r;
    else if (len > TK_SHORT)
        list_mid[pos_mid[r]] = (int32_t)r;
}

// ---- short rows: a wavefront per row (every row is visited: the empty ones get their count here too) ------------------
template <class P, class T>
__global__ __launch_bounds__(256) void topk_short_kernel(const P *__restrict__ rp, const int32_t *__restrict__ ci,
                                                        const T *__restrict__ vs, int32_t nrows, int64_t k, double minv,
                                                        int by_value, const int64_t *__restrict__ boff,
                                                        int32_t *__restrict__ tci, T *__restrict__ tvs,
                                                        int32_t *__restrict__ kept)
{
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const int lane = threadIdx.x & (WAVE - 1);
    if (r >= nrows) return;                                   // (whole wavefronts leave together)
    const int64_t sp = rp[r];
    const int64_t len64 = (int64_t)rp[r + 1] - sp;
    if (len64 > TK_SHORT) return;                             // the long kernel's
    const int len = __builtin_amdgcn_readfirstlane((int)len64);      // (the same in every lane: a scalar loop bound and lane index)
    if (len <= 0) {
        if (lane == 0) kept[r] = 0;
        return;
    }
    const bool in = lane < len;
    const T v = in ? vs[sp + lane] : (T)0;
    const int32_t c = in ? ci[sp + lane] : 0;
    const bool pass = in && !((double)v < minv);
    const uint64_t key = pass ? topk_key((double)v) : 0ull;
    int rank = 0;                                             // entries that beat this one
    for (int j = 0; j < len; j++) {
        const uint64_t kj = readlane_u64(key, j);
        rank += (kj > key || (kj == key && j < lane)) ? 1 : 0;
    }
    const bool sel = pass && (int64_t)rank < k;
    const unsigned long long ms = __ballot(sel), mp = __ballot(pass);
    const unsigned long long below = lane ? (~0ull >> (WAVE - lane)) : 0ull;
    if (sel) {
        const int64_t o = boff[r] + (by_value ? rank : __popcll(ms & below));
        tci[o] = c;
        tvs[o] = v;
    }
    if (lane == 0) {
        const int np = __popcll(mp);
        kept[r] = (int64_t)np < k ? np : (int32_t)k;
    }
}

// ---- long rows ----------------------------------------------------------------------------------------------------------
// Bitonic network in the form whose comparators all point the same way (the first step of a merge pairs i with its mirror
// in the block, i ^ (size - 1); the others i with i ^ j): the better record always goes to the lower index, so n need not
// be a power of two -- the slots from n up to the next power of two stand for records worse than any, which no comparator
// would move, and comparators that reach them are skipped.  Records are distinct (positions are), so there is one order.
template <int NT, class KP, class PP>
__device__ __forceinline__ void topk_bitonic(KP key, PP pos, int n, int tid)
{
    int np2 = 1;
    while (np2 < n) np2 <<= 1;
    const int half = np2 >> 1;
    for (int size = 2; size <= np2; size <<= 1) {
        for (int j = size >> 1; j > 0; j >>= 1) {
            const bool flip = j == (size >> 1);
            for (int q = tid; q < half; q += NT) {
                int i, l;
                if (flip) {
                    const int blk = q / j, off = q - blk * j;
                    i = blk * size + off;
                    l = blk * size + size - 1 - off;
                } else {
                    i = 2 * j * (q / j) + (q % j);
                    l = i + j;
                }
                if (l < n) {
                    const uint64_t ki = key[i], kl = key[l];
                    const uint32_t pi = pos[i], pl = pos[l];
                    if (key_before(kl, pl, ki, pi)) {
                        key[i] = kl;
                        pos[i] = pl;
                        key[l] = ki;
                        pos[l] = pi;
                    }
                }
            }
            __syncthreads();
        }
    }
}

template <class P, class T, int NT, int CAP>
__global__ __launch_bounds__(NT) void topk_long_kernel(const P *__restrict__ rp, const int32_t *__restrict__ ci,
                                                              const T *__restrict__ vs, const int32_t *__restrict__ list,
                                                              int64_t k, double minv, int by_value,
                                                              const int64_t *__restrict__ boff, int32_t *__restrict__ tci,
                                                              T *__restrict__ tvs, int32_t *__restrict__ kept,
                                                              uint64_t *__restrict__ g_key, uint32_t *__restrict__ g_pos)
{
    __shared__ uint32_t s_hist[TK_BINS];
    __shared__ uint64_t s_key[CAP];
    __shared__ uint32_t s_pos[CAP];
    __shared__ uint32_t s_wsum[NT / WAVE];
    __shared__ uint32_t s_sel[3];            // the bucket that holds the k-th key: digit, entries above it, its count
    __shared__ uint32_t s_ncand;
    __shared__ uint32_t s_tot[2][TK_UNROLL][NT / WAVE][2];

    constexpr int BPT = TK_BINS / NT;      // histogram bins per thread in the bucket search
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int32_t r = list[blockIdx.x];
    const int64_t sp = rp[r];
    const uint32_t n = (uint32_t)((int64_t)rp[r + 1] - sp);
    const T *__restrict__ rv = vs + sp;

    // ---- select: T, and how many entries with key == T are taken ----
    uint64_t prefix = 0;                     // the digits of T found so far
    uint32_t need = 0;                       // winners still to be found among the candidates
    uint32_t cand = n;                       // an upper bound of the candidates (entries that match `prefix`)
    uint32_t npass = 0, need_eq = TK_ALL;
    uint64_t thr = 0;                        // T
    bool in_lds = false;                     // the candidates are in s_key[0 .. ncand)
    uint32_t ncand = 0;
    int lo = 64;
    for (int d = 0; lo > 0; d++) {
        const int hi = lo;                   // this pass reads bits [lo, hi)
        lo = hi > TK_BITS ? hi - TK_BITS : 0;
        const uint32_t mask = (1u << (hi - lo)) - 1u;
        for (int b = tid; b < TK_BINS; b += NT) s_hist[b] = 0;
        const bool gather = !in_lds && cand <= (uint32_t)CAP;
        if (tid == 0) s_ncand = 0;
        __syncthreads();
        if (in_lds) {
            for (uint32_t i = tid; i < ncand; i += NT) {
                const uint64_t key = s_key[i];
                if ((key >> hi) == (prefix >> hi)) atomicAdd(&s_hist[(uint32_t)(key >> lo) & mask], 1u);
            }
        } else {
            for (uint32_t i0 = tid; i0 < n; i0 += TK_UNROLL * NT) {
                double wv[TK_UNROLL];      // TK_UNROLL loads in flight: one workgroup walks the row, its time is the loads' latency
#pragma unroll
                for (int u = 0; u < TK_UNROLL; u++) {
                    const uint32_t i = i0 + u * NT;
                    wv[u] = (double)rv[i < n ? i : i0];
                }
#pragma unroll
                for (int u = 0; u < TK_UNROLL; u++) {
                    if (i0 + u * NT >= n || wv[u] < minv) continue;
                    const uint64_t key = topk_key(wv[u]);
                    if (d == 0 || (key >> hi) == (prefix >> hi)) {
                        atomicAdd(&s_hist[(uint32_t)(key >> lo) & mask], 1u);
                        if (gather) s_key[atomicAdd(&s_ncand, 1u)] = key;      // (a multiset for the histograms: its order decides nothing)
                    }
                }
            }
        }
        __syncthreads();
        if (gather) {
            in_lds = true;
            ncand = s_ncand;
        }
        // the bucket: thread t owns the digits TK_BINS - 1 - BPT t - j, j = 0 .. BPT - 1 (descending)
        uint32_t c[BPT], tsum = 0;
#pragma unroll
        for (int j = 0; j < BPT; j++) {
            c[j] = s_hist[TK_BINS - 1 - (BPT * tid + j)];
            tsum += c[j];
        }
        uint32_t run = (uint32_t)wave_exscan_i32((int)tsum, lane);
        if (lane == WAVE - 1) s_wsum[w] = run + tsum;
        __syncthreads();
        uint32_t total = 0;
        for (int q = 0; q < NT / WAVE; q++) {
            if (q < w) run += s_wsum[q];
            total += s_wsum[q];
        }
        if (d == 0) {
            npass = total;
            if ((int64_t)npass <= k) break;      // every passing entry is kept: T = 0, all "ties" (uniform: no barrier is skipped by a part of the workgroup)
            need = (uint32_t)k;
        }
#pragma unroll
        for (int j = 0; j < BPT; j++) {
            if (run < need && need <= run + c[j]) {
                s_sel[0] = (uint32_t)(TK_BINS - 1 - (BPT * tid + j));
                s_sel[1] = run;
                s_sel[2] = c[j];
            }
            run += c[j];
        }
        __syncthreads();
        const uint32_t digit = s_sel[0], above = s_sel[1], cnt = s_sel[2];
        prefix |= (uint64_t)digit << lo;
        need -= above;
        cand = cnt;
        thr = prefix;
        if (cnt == need) {                       // the whole bucket is taken: key >= prefix wins
            need_eq = TK_ALL;
            break;
        }
        need_eq = need;                          // (final when lo == 0: the keys equal to T, the earliest `need`)
    }
    const uint32_t n_keep = (int64_t)npass <= k ? npass : (uint32_t)k;
    __syncthreads();                             // the candidates in LDS are done with

    // ---- place: one pass in storage order ----
    const int64_t ob = boff[r];
    const bool lds_sort = by_value && n_keep <= (uint32_t)CAP;
    const unsigned long long below = lane ? (~0ull >> (WAVE - lane)) : 0ull;
    uint32_t carry_g = 0, carry_e = 0;
    int it = 0;
    for (uint32_t base = 0; base < n; base += TK_UNROLL * NT, it++) {      // TK_UNROLL chunks of NT entries per barrier
        T v[TK_UNROLL];
        unsigned long long bg[TK_UNROLL], be[TK_UNROLL];
#pragma unroll
        for (int u = 0; u < TK_UNROLL; u++) {
            const uint32_t i = base + u * NT + tid;
            v[u] = rv[i < n ? i : 0];
        }
#pragma unroll
        for (int u = 0; u < TK_UNROLL; u++) {
            const uint32_t i = base + u * NT + tid;
            const double wv = (double)v[u];
            bool gt = false, eq = false;
            if (i < n && !(wv < minv)) {
                const uint64_t key = topk_key(wv);
                gt = key > thr;
                eq = key == thr;
            }
            bg[u] = __ballot(gt);
            be[u] = __ballot(eq);
            if (lane == 0) {
                s_tot[it & 1][u][w][0] = (uint32_t)__popcll(bg[u]);
                s_tot[it & 1][u][w][1] = (uint32_t)__popcll(be[u]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < TK_UNROLL; u++) {
            const uint32_t i = base + u * NT + tid;
            uint32_t g_before = carry_g + (uint32_t)__popcll(bg[u] & below), e_before = carry_e + (uint32_t)__popcll(be[u] & below);
            for (int q = 0; q < NT / WAVE; q++) {
                const uint32_t tg = s_tot[it & 1][u][q][0], te = s_tot[it & 1][u][q][1];
                if (q < w) {
                    g_before += tg;
                    e_before += te;
                }
                carry_g += tg;
                carry_e += te;
            }
            const bool gt = (bg[u] >> lane) & 1ull, eq = (be[u] >> lane) & 1ull;
            if (gt || (eq && e_before < need_eq)) {
                const uint32_t slot = g_before + (e_before < need_eq ? e_before : need_eq);      // < n_keep
                if (!by_value) {
                    tci[ob + slot] = ci[sp + i];
                    tvs[ob + slot] = v[u];
                } else if (lds_sort) {
                    s_key[slot] = topk_key((double)v[u]);
                    s_pos[slot] = i;
                } else {
                    g_key[ob + slot] = topk_key((double)v[u]);
                    g_pos[ob + slot] = i;
                }
            }
        }
    }
    if (tid == 0) kept[r] = (int32_t)n_keep;
    if (!by_value) return;
    __syncthreads();
    if (lds_sort) {
        topk_bitonic<NT>(s_key, s_pos, (int)n_keep, tid);
        for (uint32_t j = tid; j < n_keep; j += NT) {
            const uint32_t p = s_pos[j];
            tci[ob + j] = ci[sp + p];
            tvs[ob + j] = rv[p];
        }
    } else {
        topk_bitonic<NT>(g_key + ob, g_pos + ob, (int)n_keep, tid);
        for (uint32_t j = tid; j < n_keep; j += NT) {
            const uint32_t p = g_pos[ob + j];
            tci[ob + j] = ci[sp + p];
            tvs[ob + j] = rv[p];
        }
    }
}

// ---- closing up: rows that kept fewer entries than their bound ---------------------------------------------------------
// one thread per entry of the result: its row is the last one whose offset is <= the entry (empty rows repeat an offset)
template <class T>
__global__ __launch_bounds__(256) void topk_close_kernel(const int64_t *__restrict__ ooff, const int64_t *__restrict__ boff,
                                                        int64_t nr, int64_t total, const int32_t *__restrict__ tci,
                                                        const T *__restrict__ tvs, int32_t *__restrict__ oci,
                                                        T *__restrict__ ovs)
{
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= total) return;
    int64_t lo = 0, hi = nr - 1;      // last_at_or_below (common.h), written out: through the helper the compiler orders
    while (lo < hi) {                 // this loop's instructions differently
        const int64_t mid = (lo + hi + 1) >> 1;
        if (ooff[mid] <= o)
            lo = mid;
        else
            hi = mid - 1;
    }
    const int64_t src = boff[lo] + (o - ooff[lo]);
    oci[o] = tci[src];
    ovs[o] = tvs[src];
}

template <class P, class T>
static int topk_impl(Matrix *m, int64_t k, double minv, int by_value, Matrix **out)
{
    const int32_t nrows = m->nrows;
    const unsigned gr = (unsigned)ceil_div((int64_t)nrows, 256);
    const P *rp = (const P *)m->d_rowptrs;
    DevBuf boff, mpos, lpos, bad, mlist, list, kept, ooff, gkey, gpos;
    CSRK_TRY(boff.alloc((size_t)(nrows + 1) * 8));
    CSRK_TRY(mpos.alloc((size_t)(nrows + 1) * 4));
    CSRK_TRY(lpos.alloc((size_t)(nrows + 1) * 4));
    CSRK_TRY(kept.alloc((size_t)nrows * 4));
    CSRK_TRY(ooff.alloc((size_t)(nrows + 1) * 8));
    CSRK_TRY(bad.alloc(4));
    DrainOnExit drain_on_exit;      // (before the buffers above go back to the pool)
    CSRK_HIP(hipMemsetAsync(bad.p, 0, 4, nullptr));
    topk_bound_kernel<P><<<gr, 256>>>(rp, nrows, k, boff.as<int64_t>(), mpos.as<int32_t>(), lpos.as<int32_t>(), bad.as<int32_t>());
    CSRK_LAUNCH_CHECK();
    CSRK_TRY(exclusive_scan_i64(boff.as<int64_t>(), boff.as<int64_t>(), nrows, nullptr));
    CSRK_TRY(exclusive_scan_i32(mpos.as<int32_t>(), mpos.as<int32_t>(), nrows, nullptr));
    CSRK_TRY(exclusive_scan_i32(lpos.as<int32_t>(), lpos.as<int32_t>(), nrows, nullptr));
    int64_t btotal = 0;
    int32_t n_mid = 0, n_long = 0, is_bad = 0;
    CSRK_HIP(hipMemcpy(&btotal, boff.as<int64_t>() + nrows, 8, hipMemcpyDeviceToHost));
    CSRK_HIP(hipMemcpy(&n_mid, mpos.as<int32_t>() + nrows, 4, hipMemcpyDeviceToHost));
    CSRK_HIP(hipMemcpy(&n_long, lpos.as<int32_t>() + nrows, 4, hipMemcpyDeviceToHost));
    CSRK_HIP(hipMemcpy(&is_bad, bad.p, 4, hipMemcpyDeviceToHost));
    if (is_bad) {
        set_error("topk_rows: a row holds more than 2^31 - 1 entries");
        return CSRK_ERR_UNSUPPORTED;
    }
    Matrix *t = nullptr;
    CSRK_TRY(new_matrix(nrows, m->ncols, btotal, btotal > INT32_MAX, m->val_type, &t));
    struct Owner {      // the bounded arrays, until they are returned as the result
        Matrix *p;
        ~Owner() { delete p; }
    } t_own{t};
    topk_short_kernel<P, T><<<(unsigned)ceil_div((int64_t)nrows * WAVE, 256), 256>>>(
        rp, m->d_colinds, (const T *)m->d_values, nrows, k, minv, by_value, boff.as<int64_t>(), t->d_colinds,
        (T *)t->d_values, kept.as<int32_t>());
    CSRK_LAUNCH_CHECK();
    if (n_mid > 0 || n_long > 0) {
        CSRK_TRY(mlist.alloc((size_t)n_mid * 4));
        CSRK_TRY(list.alloc((size_t)n_long * 4));
        topk_list_kernel<P><<<gr, 256>>>(rp, nrows, mpos.as<int32_t>(), lpos.as<int32_t>(), mlist.as<int32_t>(), list.as<int32_t>());
        CSRK_LAUNCH_CHECK();
    }
    if (n_long > 0) {      // the large rows first: the longest of them is the call's tail
        if (by_value && k > TK_CAP) {      // a row may keep more winners than LDS orders: scratch for the network in memory
            CSRK_TRY(gkey.alloc((size_t)btotal * 8));
            CSRK_TRY(gpos.alloc((size_t)btotal * 4));
        }
        topk_long_kernel<P, T, TK_THREADS, TK_CAP><<<(unsigned)n_long, TK_THREADS>>>(
            rp, m->d_colinds, (const T *)m->d_values, list.as<int32_t>(), k, minv, by_value, boff.as<int64_t>(),
            t->d_colinds, (T *)t->d_values, kept.as<int32_t>(), gkey.as<uint64_t>(), gpos.as<uint32_t>());
        CSRK_LAUNCH_CHECK();
    }
    if (n_mid > 0) {
        topk_long_kernel<P, T, TK_MID_THREADS, TK_MID><<<(unsigned)n_mid, TK_MID_THREADS>>>(
            rp, m->d_colinds, (const T *)m->d_values, mlist.as<int32_t>(), k, minv, by_value, boff.as<int64_t>(),
            t->d_colinds, (T *)t->d_values, kept.as<int32_t>(), nullptr, nullptr);
        CSRK_LAUNCH_CHECK();
    }
    CSRK_TRY(exclusive_scan_i32_to_i64(kept.as<int32_t>(), ooff.as<int64_t>(), nrows, nullptr));
    int64_t total = 0;
    CSRK_HIP(hipMemcpy(&total, ooff.as<int64_t>() + nrows, 8, hipMemcpyDeviceToHost));
    Matrix *res = nullptr;
    if (total == btotal) {      // every row kept its bound: the bounded arrays are the result
        res = t;
        write_rowptrs(boff.as<int64_t>(), nrows, res);
        CSRK_LAUNCH_CHECK();
    } else {
        CSRK_TRY(new_matrix(nrows, m->ncols, total, total > INT32_MAX, m->val_type, &res));
        write_rowptrs(ooff.as<int64_t>(), nrows, res);
        if (total > 0)
            topk_close_kernel<T><<<(unsigned)ceil_div(total, 256), 256>>>(ooff.as<int64_t>(), boff.as<int64_t>(), nrows, total,
                                                                         t->d_colinds, (const T *)t->d_values,
                                                                         res->d_colinds, (T *)res->d_values);
    }
    CSRK_TRY(finish_result(res != t ? res : nullptr, "topk_rows"));      // (t_own deletes the bounded arrays)
    if (res == t) t_own.p = nullptr;
    *out = res;
    return CSRK_OK;
}

}  // namespace csrk

using namespace csrk;

extern "C" {

int csrk_topk_limits(int64_t *out, int n)
{
    CSRK_REQUIRE(out && n >= 0, "out is NULL");
    const int64_t v[4] = {TK_SHORT, TK_CAP, TK_THREADS, TK_MID};
    for (int i = 0; i < n && i < 4; i++) out[i] = v[i];
    return CSRK_OK;
}

int csrk_topk_rows(csrk_handle_t h, int64_t k, double min_value, int order, csrk_handle_t *out)
{
    CSRK_REQUIRE(out, "out is NULL");
    *out = 0;
    Matrix *m = from_handle(h);
    if (!m) return CSRK_ERR_INVALID;
    CSRK_REQUIRE(k >= 1, "topk_rows: k must be at least 1, not %lld", (long long)k);
    CSRK_REQUIRE(min_value == min_value, "topk_rows: min_value is NaN");
    CSRK_REQUIRE(order == CSRK_TOPK_BY_VALUE || order == CSRK_TOPK_STORAGE, "topk_rows: unknown order %d", order);
    CSRK_REQUIRE(m->val_type != CSRK_VAL_NONE, "matrix has no values");
    std::lock_guard<std::mutex> lk(m->mu);
    Matrix *t = nullptr;
    if (m->nrows == 0 || m->nnz == 0) {      // an empty result; nothing is launched
        CSRK_TRY(empty_matrix(m->nrows, m->ncols, m->val_type, "topk_rows", &t));
        *out = to_handle(t);
        return CSRK_OK;
    }
    const int bv = order == CSRK_TOPK_BY_VALUE;
    int rc;
    if (m->ptr64)
        rc = m->val_type == CSRK_VAL_F32 ? topk_impl<int64_t, float>(m, k, min_value, bv, &t)
                                         : topk_impl<int64_t, double>(m, k, min_value, bv, &t);
    else
        rc = m->val_type == CSRK_VAL_F32 ? topk_impl<int32_t, float>(m, k, min_value, bv, &t)
                                         : topk_impl<int32_t, double>(m, k, min_value, bv, &t);
    if (rc != CSRK_OK) return rc;
    *out = to_handle(t);
    return CSRK_OK;
}

}  // extern "C"
