// Offline evaluation of a factor model for libcsrk on gfx950: csrk_rank_entries gives, for every entry (i, j) of a CSR
// matrix `test`, the number of items that row i has not seen and that come before j in the row's full ranking by
// U[i] . V[c] (the contract is in include/csrk.h).  The rows x n_items block of scores never leaves the chip.
//
// Score.  The tile of topk_scores.hip (score_tile.h): a 256-thread workgroup owns 64 rows of U and sweeps V in tiles of 64
// items, 4 x 4 serial chains of fused multiply-adds per thread, the panels staged through LDS 16 factors at a time in two
// buffers.  Nothing is summed in pieces, so a score has the bits csrk_topk_scores gives it.
//
// Counting.  A workgroup takes up to RE_T (32) test entries of each of its rows per SWEEP of V:
//   pre-pass   one wavefront per row: lane x runs the chain of the row's x-th entry straight from the panels (the same k
//              fused multiply-adds in the same order as the tile's chain: the same bits), writes the score out, and the
//              wavefront orders the entries by (key descending, item ascending) all-pairs, as ts_compact does, keeping
//              every entry's place in the row;
//   sweep      every score of a tile that comes before the row's LAST listed entry (one comparison against registers:
//              most scores of a row whose held-out items rank high end here) finds by binary search the first listed
//              entry m it comes before and adds one to hist[row][m], an integer LDS atomic.  (key, item) pairs equal to a
//              listed entry's -- the entry's own item -- come before nothing they tie with, so no item counts itself;
//   seen       the sweep counted every item.  One wavefront per row then runs the chain of every entry `seen` stores in
//              the row and takes the same step with -1.  Integers: the order of the atomics decides nothing;
//   finish     a prefix sum over hist[row][0 .. m] is the rank of the entry listed at m, written to its place.
// A row with more than RE_T entries is swept again per RE_T of them; the number of sweeps of a workgroup is the largest
// its rows need, found in the kernel.  No scratch memory, no host round trip.
//
// LDS: 33 KiB of staging lines + 43.5 KiB of lists and counters = 76.5 KiB per workgroup, two workgroups per CU.
#include <cstdlib>

#include "common.h"
#include "rank_list.h"
#include "score_host.h"
#include "score_tile.h"

namespace csrk {

// (the list constants RE_*, re_chain and re_slot: rank_list.h, shared with rank_entries_for.hip)
template <class T, bool WIDE>
__global__ __launch_bounds__(TS_THREADS) void rank_entries_kernel(const void *__restrict__ seen_rp, int seen_ptr64,
                                                                 const int32_t *__restrict__ seen_ci, const void *__restrict__ test_rp,
                                                                 int test_ptr64, const int32_t *__restrict__ test_ci, int32_t row_begin,
                                                                 int32_t nrows, const T *__restrict__ U, int64_t ldu,
                                                                 const T *__restrict__ V, int64_t ldv, int32_t n_items, int32_t k, int count,
                                                                 int32_t *__restrict__ ranks, double *__restrict__ scores)
{
    constexpr int PER = WIDE ? 16 / (int)sizeof(T) : 1;
    __shared__ __attribute__((aligned(16))) double su2[2][TS_KC][TS_LD];      // two buffers: one barrier per chunk
    __shared__ __attribute__((aligned(16))) double sv2[2][TS_KC][TS_LD];
    __shared__ uint64_t s_key[TS_ROWS][RE_LDT];                   // a row's listed entries, best first
    __shared__ int32_t s_item[TS_ROWS][RE_LDT];
    __shared__ int32_t s_pos[TS_ROWS][RE_LDT];                    // the place of each in this sweep's part of the row
    __shared__ int32_t s_hist[TS_ROWS][RE_LDT];
    __shared__ int64_t s_t0[TS_ROWS], s_t1[TS_ROWS], s_e0[TS_ROWS], s_e1[TS_ROWS];
    __shared__ int32_t s_cnt[TS_ROWS];
    __shared__ unsigned long long s_nsw;

    const int tid = threadIdx.x, ty = tid / (TS_TILE / TS_B), tx = tid % (TS_TILE / TS_B);
    const int lane = tid & (WAVE - 1), w = tid / WAVE;
    const int64_t r0 = (int64_t)blockIdx.x * TS_ROWS;             // the block's first row, relative to row_begin
    const int64_t nvalid = (int64_t)nrows - r0 < TS_ROWS ? (int64_t)nrows - r0 : TS_ROWS;
    const int64_t base = load_ptr(test_rp, test_ptr64, row_begin);

    if (tid == 0) s_nsw = 0;
    __syncthreads();
    if (tid < TS_ROWS) {
        int64_t t0 = 0, t1 = 0, e0 = 0, e1 = 0;
        if (tid < nvalid) {
            const int64_t row = (int64_t)row_begin + r0 + tid;
            t0 = load_ptr(test_rp, test_ptr64, row);
            t1 = load_ptr(test_rp, test_ptr64, row + 1);
            if (seen_rp) {
                e0 = load_ptr(seen_rp, seen_ptr64, row);
                e1 = load_ptr(seen_rp, seen_ptr64, row + 1);
            }
        }
        if (t1 < t0) t1 = t0;
        s_t0[tid] = t0, s_t1[tid] = t1, s_e0[tid] = e0, s_e1[tid] = e1;
        if (t1 > t0) atomicMax(&s_nsw, (unsigned long long)((t1 - t0 + RE_T - 1) / RE_T));
    }
    __syncthreads();
    const int64_t nsw = (int64_t)s_nsw;
    if (nsw == 0) return;                                         // no test entry in these rows
    uint64_t sink = 0;

    for (int64_t c = 0; c < nsw; c++) {
        // ---- pre-pass: this sweep's entries of every row, scored and ordered (one wavefront per row)
        for (int r = w; r < TS_ROWS; r += TS_THREADS / WAVE) {
            const int64_t first = s_t0[r] + c * RE_T, left = s_t1[r] - first;
            const int n = left <= 0 ? 0 : (left < RE_T ? (int)left : RE_T);
            uint64_t key = 0;
            int32_t item = RE_BAD_ITEM;
            if (lane < RE_LDT) s_hist[r][lane] = 0;
            if (lane < n) {
                const int32_t j = test_ci[first + lane];
                double s = __longlong_as_double(0x7ff8000000000000ll);
                if (j >= 0 && j < n_items) {
                    s = re_chain<T>(U + (r0 + r) * ldu, V + (int64_t)j * ldv, k);
                    key = topk_key(s);
                    item = j;
                }
                if (scores) scores[first + lane - base] = s;
                s_key[r][lane] = key;
                s_item[r][lane] = item;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            int rank = 0;
            for (int y = 0; y < n; y++) {
                const uint64_t ky = s_key[r][y];
                const int32_t iy = s_item[r][y];
                rank += (key_before(ky, iy, key, item) || (ky == key && iy == item && y < lane)) ? 1 : 0;
            }
            // the wavefront has read the list before any lane rewrites it (LDS operations of one wavefront complete in issue order)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            if (lane < n) {
                s_key[r][rank] = key;
                s_item[r][rank] = item;
                s_pos[r][rank] = lane;
            }
            if (lane == 0) s_cnt[r] = n;
        }
        __syncthreads();

        // a row's last listed entry: a score that does not come before it comes before none (no entry: nothing does)
        int cnt[TS_B];
        uint64_t lastk[TS_B];
        int32_t lasti[TS_B];
#pragma unroll
        for (int i = 0; i < TS_B; i++) {
            const int r = TS_B * ty + i;
            cnt[i] = s_cnt[r];
            lastk[i] = cnt[i] ? s_key[r][cnt[i] - 1] : ~0ull;
            lasti[i] = cnt[i] ? s_item[r][cnt[i] - 1] : -1;
        }

        // ---- sweep: the product of topk_scores.hip, tile by tile
        TsUnits<T, PER> fu, fv;                                   // the chunk after the one in use
        if (n_items > 0) {
            ts_fetch<T, PER>(fu, U, ldu, r0, nvalid, 0, k, tid);
            ts_fetch<T, PER>(fv, V, ldv, 0, (int64_t)n_items, 0, k, tid);
        }
        int buf = 0;
        for (int64_t j0 = 0; j0 < n_items; j0 += TS_TILE) {
            double acc[TS_B][TS_B];
#pragma unroll
            for (int i = 0; i < TS_B; i++)
#pragma unroll
                for (int jj = 0; jj < TS_B; jj++) acc[i][jj] = 0.0;
            for (int t0 = 0; t0 < k; t0 += TS_KC, buf ^= 1) {
                double (*__restrict__ su)[TS_LD] = su2[buf], (*__restrict__ sv)[TS_LD] = sv2[buf];
                ts_put<T, PER>(fu, su, tid);
                ts_put<T, PER>(fv, sv, tid);
                __syncthreads();      // (one per chunk: whoever writes this buffer again has passed the next chunk's barrier, after everyone's use of it)
                {
                    const bool more = t0 + TS_KC < k;             // the next chunk: of this tile, or the first of the next tile
                    const int64_t jn = more ? j0 : j0 + TS_TILE;
                    if (jn < n_items) {
                        ts_fetch<T, PER>(fu, U, ldu, r0, nvalid, more ? t0 + TS_KC : 0, k, tid);
                        ts_fetch<T, PER>(fv, V, ldv, jn, (int64_t)n_items - jn, more ? t0 + TS_KC : 0, k, tid);
                    }
                }
                const int kc = k - t0 < TS_KC ? k - t0 : TS_KC;
                if (kc == TS_KC) {
#pragma unroll
                    for (int t = 0; t < TS_KC; t++) {
                        const f64x2_t a0 = *(const f64x2_t *)&su[t][TS_B * ty], a1 = *(const f64x2_t *)&su[t][TS_B * ty + 2];
                        const f64x2_t b0 = *(const f64x2_t *)&sv[t][TS_B * tx], b1 = *(const f64x2_t *)&sv[t][TS_B * tx + 2];
                        const double u[TS_B] = {a0.x, a0.y, a1.x, a1.y}, v[TS_B] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
                        for (int i = 0; i < TS_B; i++)
#pragma unroll
                            for (int jj = 0; jj < TS_B; jj++) acc[i][jj] = __builtin_fma(u[i], v[jj], acc[i][jj]);
                    }
                } else {
                    for (int t = 0; t < kc; t++) {
                        const f64x2_t a0 = *(const f64x2_t *)&su[t][TS_B * ty], a1 = *(const f64x2_t *)&su[t][TS_B * ty + 2];
                        const f64x2_t b0 = *(const f64x2_t *)&sv[t][TS_B * tx], b1 = *(const f64x2_t *)&sv[t][TS_B * tx + 2];
                        const double u[TS_B] = {a0.x, a0.y, a1.x, a1.y}, v[TS_B] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
                        for (int i = 0; i < TS_B; i++)
#pragma unroll
                            for (int jj = 0; jj < TS_B; jj++) acc[i][jj] = __builtin_fma(u[i], v[jj], acc[i][jj]);
                    }
                }
            }
            if (!count) {                                         // diagnostic: the product alone
#pragma unroll
                for (int i = 0; i < TS_B; i++)
#pragma unroll
                    for (int jj = 0; jj < TS_B; jj++) sink ^= (uint64_t)__double_as_longlong(acc[i][jj]);
                continue;
            }
#pragma unroll
            for (int i = 0; i < TS_B; i++)
#pragma unroll
                for (int jj = 0; jj < TS_B; jj++) {
                    const int64_t j = j0 + TS_B * tx + jj;
                    const uint64_t ks = topk_key(acc[i][jj]);
                    if (j < n_items && key_before(ks, (int32_t)j, lastk[i], lasti[i])) {
                        const int r = TS_B * ty + i;
                        atomicAdd(&s_hist[r][re_slot(s_key[r], s_item[r], cnt[i], ks, (int32_t)j)], 1);      // (a slot < cnt[i]: it comes before the last)
                    }
                }
        }
        __syncthreads();

        // ---- the items `seen` stores were counted like any other: take them out again (one wavefront per row)
        if (seen_rp && count)
            for (int r = w; r < nvalid; r += TS_THREADS / WAVE) {
                const int n = s_cnt[r];
                if (!n) continue;
                const uint64_t lk = s_key[r][n - 1];
                const int32_t li = s_item[r][n - 1];
                for (int64_t e = s_e0[r] + lane; e < s_e1[r]; e += WAVE) {
                    const int32_t j = seen_ci[e];
                    if (j < 0 || j >= n_items) continue;          // (no item: the sweep did not count it)
                    const uint64_t ks = topk_key(re_chain<T>(U + (r0 + r) * ldu, V + (int64_t)j * ldv, k));
                    if (key_before(ks, j, lk, li)) atomicSub(&s_hist[r][re_slot(s_key[r], s_item[r], n, ks, j)], 1);
                }
            }
        __syncthreads();

        // ---- finish: the entry listed at m is preceded by what fell into slots 0 .. m
        if (count && tid < nvalid) {
            const int n = s_cnt[tid];
            const int64_t first = s_t0[tid] + c * RE_T - base;
            int32_t run = 0;
            for (int m = 0; m < n; m++) {
                run += s_hist[tid][m];
                ranks[first + s_pos[tid][m]] = s_item[tid][m] == RE_BAD_ITEM ? -1 : run;
            }
        }
        __syncthreads();
    }
    if (!count && sink == 0x7ff8c0dec0dec0deull && tid < nvalid && s_t1[tid] > s_t0[tid]) ranks[s_t0[tid] - base] = 0;      // (keeps the product alive)
}

// the kernel's arguments in its order (the grid follows from n)
struct ReLaunch {
    ScoreCsr seen, test;
    int32_t row_begin, n;
    const void *U;
    int64_t ldu;
    const void *V;
    int64_t ldv;
    int32_t n_items, k;
    int count;
    int32_t *ranks;
    double *scores;
    hipStream_t s;
};

template <class T, bool WIDE> static void re_launch(const ReLaunch &a)
{
    rank_entries_kernel<T, WIDE><<<(unsigned)score_row_blocks(a.n), TS_THREADS, 0, a.s>>>(
        a.seen.rp, a.seen.ptr64, a.seen.ci, a.test.rp, a.test.ptr64, a.test.ci, a.row_begin, a.n, (const T *)a.U, a.ldu, (const T *)a.V,
        a.ldv, a.n_items, a.k, a.count, a.ranks, a.scores);
}

// the refusals that need no handle come first: they are answered whatever the handles are
static int re_scalars(int32_t row_begin, int32_t row_end, int64_t ldu, int64_t ldv, int32_t k, int panel_type)
{
    CSRK_CHECK_K("rank_entries: ", k);
    CSRK_CHECK_TWO_PANELS("rank_entries: ", k, ldu, ldv);
    CSRK_CHECK_PANEL_TYPE("rank_entries: ", panel_type);
    CSRK_CHECK_ROW_ORDER("rank_entries: ", row_begin, row_end);
    return check_supported(re_k_supported(k), "csrk_rank_entries", "k", k, RE_K_MAX, "csrk_rank_entries_limits");
}

// the scalars, then the handles (seen may be 0) and what they must agree on; the caller holds no lock
static int re_check(csrk_handle_t seen_h, csrk_handle_t test_h, int32_t row_begin, int32_t row_end, int64_t ldu, int64_t ldv, int32_t k,
                    int panel_type, Matrix **ms, Matrix **mt)
{
    CSRK_TRY(re_scalars(row_begin, row_end, ldu, ldv, k, panel_type));
    CSRK_TRY(optional_handle(seen_h, ms));
    Matrix *const seen = *ms, *const test = from_handle(test_h);
    if (!test) return CSRK_ERR_INVALID;
    *mt = test;
    CSRK_CHECK_ROW_RANGE("rank_entries: ", row_begin, row_end, test->nrows);
    if (seen) {
        CSRK_TRY(check_seen_matches_test("rank_entries", seen, test));
        CSRK_TRY(check_seen_canonical("rank_entries", seen));
    }
    return CSRK_OK;
}

static int re_pointers(const void *ranks, const void *scores, const void *U, const void *V, size_t es)
{
    CSRK_REQUIRE(ranks, "rank_entries: ranks is NULL");
    CSRK_REQUIRE(U && V, "rank_entries: U or V is NULL");
    CSRK_REQUIRE(((uintptr_t)U % es) == 0 && ((uintptr_t)V % es) == 0 && ((uintptr_t)scores % 8) == 0 && ((uintptr_t)ranks % 4) == 0,
                 "rank_entries: U, V, ranks or scores is not aligned to its element size");
    return CSRK_OK;
}

// dU points at row row_begin of U; there are rows and test stores entries
static int re_device(Matrix *seen, Matrix *test, int32_t row_begin, int32_t row_end, const void *dU, int64_t ldu, const void *dV,
                     int64_t ldv, int32_t k, int panel_type, int32_t *dranks, double *dscores, hipStream_t s)
{
    const size_t es = panel_es(panel_type);
    CSRK_TRY(re_pointers(dranks, dscores, dU, dV, es));
    mark_user_stream(seen, s);
    mark_user_stream(test, s);
    const int count = score_knob_on(getenv("CSRK_RANK_ENTRIES_COUNT"));       // diagnostic: "0" times the product alone (the outputs are not written)
    const ReLaunch L{score_csr(seen), score_csr(test), row_begin, row_end - row_begin, dU, ldu, dV, ldv, test->ncols, k, count, dranks,
                     dscores, s};
    score_for_panel(panel_type, panels_wide(dU, ldu, dV, ldv, k, es),
                    [&](auto t, auto w) { re_launch<typename decltype(t)::type, decltype(w)::value>(L); });
    CSRK_LAUNCH_CHECK();
    return CSRK_OK;
}

// the entries of the rows [row_begin, row_end) of `test`: two row pointers fetched (the host form is synchronous anyway)
static int re_fetch_entry_range(const Matrix *test, int32_t row_begin, int32_t row_end, int64_t e[2])
{
    for (int i = 0; i < 2; i++) {
        const int64_t row = i ? row_end : row_begin;
        if (test->ptr64) {
            CSRK_HIP(hipMemcpy(&e[i], (const int64_t *)test->d_rowptrs + row, 8, hipMemcpyDeviceToHost));
        } else {
            int32_t v = 0;
            CSRK_HIP(hipMemcpy(&v, (const int32_t *)test->d_rowptrs + row, 4, hipMemcpyDeviceToHost));
            e[i] = v;
        }
    }
    return CSRK_OK;
}

}  // namespace csrk

using namespace csrk;

extern "C" {

int csrk_rank_entries_limits(int64_t *out, int n)
{
    CSRK_REQUIRE(out && n >= 0, "csrk_rank_entries_limits: out is NULL or n < 0");
    const int64_t v[5] = {RE_K_MAX, TS_ROWS, TS_TILE, TS_KC, RE_T};
    for (int i = 0; i < n && i < 5; i++) out[i] = v[i];
    return CSRK_OK;
}

int csrk_rank_entries_device(csrk_handle_t seen, csrk_handle_t test, int32_t row_begin, int32_t row_end, const void *d_U, int64_t ldu,
                             const void *d_V, int64_t ldv, int32_t k, int panel_type, int32_t *d_ranks, double *d_scores, void *stream)
{
    Matrix *ms, *mt;
    CSRK_TRY(re_check(seen, test, row_begin, row_end, ldu, ldv, k, panel_type, &ms, &mt));
    if (row_begin == row_end || mt->nnz == 0) return CSRK_OK;
    const void *u0 = panel_rows_from(d_U, row_begin, ldu, panel_es(panel_type));
    return re_device(ms, mt, row_begin, row_end, u0, ldu, d_V, ldv, k, panel_type, d_ranks, d_scores, (hipStream_t)stream);
}

int csrk_rank_entries(csrk_handle_t seen, csrk_handle_t test, int32_t row_begin, int32_t row_end, const void *U, int64_t ldu,
                      const void *V, int64_t ldv, int32_t k, int panel_type, int32_t *ranks, double *scores)
{
    Matrix *ms, *mt;
    // argument checks first, with the caller's pointers (the device call below sees packed copies)
    CSRK_TRY(re_check(seen, test, row_begin, row_end, ldu, ldv, k, panel_type, &ms, &mt));
    if (row_begin == row_end || mt->nnz == 0) return CSRK_OK;
    int64_t e[2];
    CSRK_TRY(re_fetch_entry_range(mt, row_begin, row_end, e));
    if (e[1] <= e[0]) return CSRK_OK;
    const size_t es = panel_es(panel_type);
    CSRK_TRY(re_pointers(ranks, scores, U, V, es));
    const size_t n = (size_t)(row_end - row_begin), ne = (size_t)(e[1] - e[0]), n_items = (size_t)mt->ncols;
    DevBuf dU, dV, dR, dS;
    CSRK_TRY(pack_panel(dU, panel_rows_from(U, row_begin, ldu, es), ldu, k, es, n));
    CSRK_TRY(pack_panel(dV, V, ldv, k, es, n_items));
    CSRK_TRY(dR.alloc(ne * 4));
    if (scores) CSRK_TRY(dS.alloc(ne * 8));
    CSRK_TRY(re_device(ms, mt, row_begin, row_end, dU.p, k, dV.p, k, k, panel_type, dR.as<int32_t>(), scores ? dS.as<double>() : nullptr,
                       nullptr));
    CSRK_HIP(hipMemcpy(ranks, dR.p, ne * 4, hipMemcpyDeviceToHost));
    if (scores) CSRK_HIP(hipMemcpy(scores, dS.p, ne * 8, hipMemcpyDeviceToHost));
    return CSRK_OK;
}

}  // extern "C"
