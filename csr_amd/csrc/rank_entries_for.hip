// Offline evaluation of a sample of rows for libcsrk on gfx950: csrk_rank_entries_for is csrk_rank_entries for a LIST of
// rows, with the items cut into S contiguous ranges of whole tiles so that a sample of a thousand users still fills the card
// (the contract is in include/csrk.h).  Every score, list and count is rank_entries.hip's: the kernel below is that kernel's
// text made general in three things and in nothing else:
//   * where a block's rows come from: a list of absolute rows staged in LDS (the row of `test`, of `seen`, and of U unless U
//     travels packed in list order), fetched as topk_scores_for does (ts_row_offsets, ts_fetch_rows of score_list.h);
//   * the item interval [j_begin, j_end) it sweeps (whole tiles from j_begin), and with it the part of each row of `seen` it
//     takes out again: `seen` is canonical, so two lower bounds in the row give the entries whose column lies in the interval;
//   * where a rank goes: to ranks[offsets[r] + x], stored (S = 1) or added (S > 1).
// One launch, grid (row blocks, S).  Every split of a block runs the same pre-pass and so lists the same entries in the same
// order; what it counts over its interval is a partial rank, an integer, and the partial ranks of an entry add to its rank.
// S > 1: ranks[0 .. n_out) is cleared on the stream first and every workgroup adds with one integer atomicAdd per listed
// entry (none for a partial rank of zero).  Integer addition commutes: no bit depends on S or on who arrives first.  Only
// split 0 writes the scores and the -1 of a test column that is no item.  No float atomic, no workspace, and no workgroup
// waits for another.  rank_entries_kernel keeps its own text (DESIGN.md sections 8f, 8i).
//
// LDS: 33 KiB of staging lines + 43.5 KiB of lists and counters + 1 KiB of list rows and offsets = 77.5 KiB per workgroup,
// two workgroups per CU (160 KiB).
#include <vector>

#include "common.h"
#include "rank_list.h"
#include "score_host.h"
#include "score_list.h"
#include "score_tile.h"

namespace csrk {

// (the constants REF_*, the split rule and the item interval of a split: score_plan.h)
template <class T, bool WIDE>
__global__ __launch_bounds__(TS_THREADS) void rank_entries_for_kernel(const void *__restrict__ seen_rp, int seen_ptr64,
                                                                     const int32_t *__restrict__ seen_ci, const void *__restrict__ test_rp,
                                                                     int test_ptr64, const int32_t *__restrict__ test_ci,
                                                                     const int32_t *__restrict__ rows, int64_t n_rows, int32_t u_rows,
                                                                     int u_packed, const T *__restrict__ U, int64_t ldu,
                                                                     const T *__restrict__ V, int64_t ldv, int32_t n_items, int32_t k,
                                                                     const int64_t *__restrict__ offsets, int64_t n_out,
                                                                     int32_t *__restrict__ ranks, double *__restrict__ scores, int n_splits)
{
    constexpr int PER = WIDE ? 16 / (int)sizeof(T) : 1;
    __shared__ __attribute__((aligned(16))) double su2[2][TS_KC][TS_LD];      // two buffers: one barrier per chunk
    __shared__ __attribute__((aligned(16))) double sv2[2][TS_KC][TS_LD];
    __shared__ uint64_t s_key[TS_ROWS][RE_LDT];                   // a row's listed entries, best first
    __shared__ int32_t s_item[TS_ROWS][RE_LDT];
    __shared__ int32_t s_pos[TS_ROWS][RE_LDT];                    // the place of each in this sweep's part of the row
    __shared__ int32_t s_hist[TS_ROWS][RE_LDT];
    __shared__ int64_t s_t0[TS_ROWS], s_t1[TS_ROWS], s_e0[TS_ROWS], s_e1[TS_ROWS];
    __shared__ int64_t s_urow[TS_ROWS];                           // the row of U, -1 for none
    __shared__ int64_t s_off[TS_ROWS];                            // where the row's outputs start
    __shared__ int32_t s_cnt[TS_ROWS];
    __shared__ unsigned long long s_nsw;

    const int tid = threadIdx.x, ty = tid / (TS_TILE / TS_B), tx = tid % (TS_TILE / TS_B);
    const int lane = tid & (WAVE - 1), w = tid / WAVE;
    const int split = blockIdx.y;
    const ScoreItemRange range = score_item_range(split, n_splits, n_items);
    const int64_t j_begin = range.j_begin, j_end = range.j_end;
    const int64_t r0 = (int64_t)blockIdx.x * TS_ROWS;             // the block's first row, as a place in the list
    const int64_t nvalid = n_rows - r0 < TS_ROWS ? n_rows - r0 : TS_ROWS;

    if (tid == 0) s_nsw = 0;
    __syncthreads();
    if (tid < TS_ROWS) {
        int64_t t0 = 0, t1 = 0, e0 = 0, e1 = 0, urow = -1, off = 0;
        const int64_t row = tid < nvalid ? (int64_t)rows[r0 + tid] : -1;
        if (row >= 0 && row < u_rows) {                           // (an index outside is not dereferenced: the place takes nothing)
            urow = u_packed ? r0 + tid : row;
            off = offsets[r0 + tid];
            t0 = load_ptr(test_rp, test_ptr64, row);
            t1 = load_ptr(test_rp, test_ptr64, row + 1);
            if (seen_rp && j_begin < j_end) {                     // the row's entries whose column lies in [j_begin, j_end)
                e0 = load_ptr(seen_rp, seen_ptr64, row);
                e1 = load_ptr(seen_rp, seen_ptr64, row + 1);
                e0 = first_not_below(seen_ci, e0, e1, (int32_t)j_begin);
                e1 = first_not_below(seen_ci, e0, e1, (int32_t)j_end);      // (j_end <= n_items: it fits)
            }
        }
        if (t1 < t0) t1 = t0;
        s_t0[tid] = t0, s_t1[tid] = t1, s_e0[tid] = e0, s_e1[tid] = e1, s_urow[tid] = urow, s_off[tid] = off;
        if (t1 > t0) atomicMax(&s_nsw, (unsigned long long)((t1 - t0 + RE_T - 1) / RE_T));
    }
    __syncthreads();
    const int64_t nsw = (int64_t)s_nsw;
    if (nsw == 0) return;                                         // no test entry in these rows
    int64_t u_off[TsUnits<T, PER>::NL];                           // where this thread's rows of U start
    ts_row_offsets<T, PER>(u_off, s_urow, ldu, tid);

    for (int64_t c = 0; c < nsw; c++) {
        // ---- pre-pass: this sweep's entries of every row, scored and ordered (one wavefront per row); the same in every split
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
                    s = re_chain<T>(U + s_urow[r] * ldu, V + (int64_t)j * ldv, k);
                    key = topk_key(s);
                    item = j;
                }
                const int64_t at = s_off[r] + c * RE_T + lane;
                if (scores && split == 0 && at >= 0 && at < n_out) scores[at] = s;
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

        // ---- sweep: the product of topk_scores.hip, tile by tile over this split's interval
        TsUnits<T, PER> fu, fv;                                   // the chunk after the one in use
        if (j_begin < j_end) {
            ts_fetch_rows<T, PER>(fu, U, u_off, 0, k, tid);
            ts_fetch<T, PER>(fv, V, ldv, j_begin, j_end - j_begin, 0, k, tid);
        }
        int buf = 0;
        for (int64_t j0 = j_begin; j0 < j_end; j0 += TS_TILE) {
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
                    if (jn < j_end) {
                        ts_fetch_rows<T, PER>(fu, U, u_off, more ? t0 + TS_KC : 0, k, tid);
                        ts_fetch<T, PER>(fv, V, ldv, jn, j_end - jn, more ? t0 + TS_KC : 0, k, tid);
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
#pragma unroll
            for (int i = 0; i < TS_B; i++)
#pragma unroll
                for (int jj = 0; jj < TS_B; jj++) {
                    const int64_t j = j0 + TS_B * tx + jj;
                    const uint64_t ks = topk_key(acc[i][jj]);
                    if (j < j_end && key_before(ks, (int32_t)j, lastk[i], lasti[i])) {
                        const int r = TS_B * ty + i;
                        atomicAdd(&s_hist[r][re_slot(s_key[r], s_item[r], cnt[i], ks, (int32_t)j)], 1);      // (a slot < cnt[i]: it comes before the last)
                    }
                }
        }
        __syncthreads();

        // ---- the items `seen` stores in the interval were counted like any other: take them out again (one wavefront per row)
        if (seen_rp)
            for (int r = w; r < nvalid; r += TS_THREADS / WAVE) {
                const int n = s_cnt[r];
                if (!n) continue;
                const uint64_t lk = s_key[r][n - 1];
                const int32_t li = s_item[r][n - 1];
                for (int64_t e = s_e0[r] + lane; e < s_e1[r]; e += WAVE) {
                    const int32_t j = seen_ci[e];
                    if (j < j_begin || j >= j_end) continue;      // (not of this interval: the sweep did not count it)
                    const uint64_t ks = topk_key(re_chain<T>(U + s_urow[r] * ldu, V + (int64_t)j * ldv, k));
                    if (key_before(ks, j, lk, li)) atomicSub(&s_hist[r][re_slot(s_key[r], s_item[r], n, ks, j)], 1);
                }
            }
        __syncthreads();

        // ---- finish: the entry listed at m is preceded, within the interval, by what fell into slots 0 .. m
        if (tid < nvalid) {
            const int n = s_cnt[tid];
            const int64_t first = s_off[tid] + c * RE_T;
            int32_t run = 0;
            for (int m = 0; m < n; m++) {
                run += s_hist[tid][m];
                const int64_t at = first + s_pos[tid][m];
                if (at < 0 || at >= n_out) continue;              // (offsets that are not the prefix sum: nothing outside is written)
                const bool bad = s_item[tid][m] == RE_BAD_ITEM;
                if (n_splits == 1)
                    ranks[at] = bad ? -1 : run;
                else if (bad ? split == 0 : run != 0)
                    atomicAdd(&ranks[at], bad ? -1 : run);
            }
        }
        __syncthreads();
    }
}

// the test entries of every listed row (the host form sums them into the offsets)
__global__ __launch_bounds__(REF_LEN_THREADS) void rank_entries_for_lens_kernel(const void *__restrict__ test_rp, int test_ptr64,
                                                                              const int32_t *__restrict__ rows, int64_t n_rows,
                                                                              int64_t *__restrict__ lens)
{
    for (int64_t r = (int64_t)blockIdx.x * REF_LEN_THREADS + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * REF_LEN_THREADS) {
        const int64_t n = load_ptr(test_rp, test_ptr64, (int64_t)rows[r] + 1) - load_ptr(test_rp, test_ptr64, rows[r]);
        lens[r] = n > 0 ? n : 0;
    }
}

// the kernel's arguments in its order (the grid: row blocks x S)
struct RefLaunch {
    ScoreCsr seen, test;
    const int32_t *rows;
    int64_t n_rows;
    int32_t u_rows;
    int u_packed;
    const void *U;
    int64_t ldu;
    const void *V;
    int64_t ldv;
    int32_t n_items, k;
    const int64_t *offsets;
    int64_t n_out;
    int32_t *ranks;
    double *scores;
    int S;
    hipStream_t s;
};

template <class T, bool WIDE> static void ref_launch(const RefLaunch &a)
{
    const dim3 grid((unsigned)score_row_blocks(a.n_rows), (unsigned)a.S);
    rank_entries_for_kernel<T, WIDE><<<grid, TS_THREADS, 0, a.s>>>(a.seen.rp, a.seen.ptr64, a.seen.ci, a.test.rp, a.test.ptr64, a.test.ci,
                                                                   a.rows, a.n_rows, a.u_rows, a.u_packed, (const T *)a.U, a.ldu,
                                                                   (const T *)a.V, a.ldv, a.n_items, a.k, a.offsets, a.n_out, a.ranks,
                                                                   a.scores, a.S);
}

// the refusals that need no handle come first: they are answered whatever the handles are
static int ref_scalars(int64_t n_rows, int32_t u_rows, int64_t ldu, int64_t ldv, int32_t k, int panel_type, int64_t n_out, int32_t splits)
{
    CSRK_CHECK_K("rank_entries_for: ", k);
    CSRK_CHECK_TWO_PANELS("rank_entries_for: ", k, ldu, ldv);
    CSRK_CHECK_PANEL_TYPE("rank_entries_for: ", panel_type);
    CSRK_REQUIRE(n_rows >= 0, "rank_entries_for: n_rows must not be negative (n_rows=%lld)", (long long)n_rows);
    CSRK_REQUIRE(u_rows >= 0, "rank_entries_for: u_rows must not be negative (u_rows=%d)", u_rows);
    CSRK_REQUIRE(splits >= 0, "rank_entries_for: splits must not be negative (splits=%d)", splits);
    CSRK_REQUIRE(n_out >= 0, "rank_entries_for: n_out must not be negative (n_out=%lld)", (long long)n_out);
    return check_supported(re_k_supported(k), "rank_entries_for", "k", k, RE_K_MAX, "csrk_rank_entries_limits");
}

// then the handles (seen may be 0) and what they must agree on; the caller holds no lock
static int ref_check(csrk_handle_t seen_h, csrk_handle_t test_h, int64_t n_rows, int32_t u_rows, int32_t splits, Matrix **ms, Matrix **mt)
{
    CSRK_TRY(optional_handle(seen_h, ms));
    Matrix *const seen = *ms, *const test = from_handle(test_h);
    if (!test) return CSRK_ERR_INVALID;
    *mt = test;
    CSRK_REQUIRE(u_rows == test->nrows, "rank_entries_for: u_rows=%d but test has %d rows", u_rows, test->nrows);
    if (seen) {
        CSRK_TRY(check_seen_matches_test("rank_entries_for", seen, test));
        CSRK_TRY(check_seen_canonical("rank_entries_for", seen));
    }
    const int64_t S = ref_splits(n_rows, test->ncols, splits);
    if (ref_grid_too_large(n_rows, S)) {
        set_error("rank_entries_for: n_rows=%lld in %lld splits makes more workgroups than a grid holds (%lld)", (long long)n_rows,
                  (long long)S, (long long)REF_GRID_MAX);
        return CSRK_ERR_UNSUPPORTED;
    }
    return CSRK_OK;
}

// u_packed: dU holds the listed rows only, in list order (the host form); drows names rows of `test` and `seen` either way
static int ref_device(Matrix *seen, Matrix *test, const int32_t *drows, int64_t n_rows, int32_t u_rows, int u_packed, const void *dU,
                      int64_t ldu, const void *dV, int64_t ldv, int32_t k, int panel_type, const int64_t *doffsets, int64_t n_out,
                      int32_t *dranks, double *dscores, int32_t splits, hipStream_t s)
{
    CSRK_REQUIRE(dranks, "rank_entries_for: ranks is NULL");
    CSRK_REQUIRE(dU && dV, "rank_entries_for: U or V is NULL");
    CSRK_REQUIRE(drows && doffsets, "rank_entries_for: rows or offsets is NULL");
    const size_t es = panel_es(panel_type);
    CSRK_REQUIRE(((uintptr_t)dU % es) == 0 && ((uintptr_t)dV % es) == 0 && ((uintptr_t)dscores % 8) == 0 && ((uintptr_t)dranks % 4) == 0 &&
                     ((uintptr_t)drows % 4) == 0 && ((uintptr_t)doffsets % 8) == 0,
                 "rank_entries_for: rows, offsets, U, V, ranks or scores is not aligned to its element size");
    mark_user_stream(seen, s);
    mark_user_stream(test, s);
    const int32_t S = ref_splits(n_rows, test->ncols, splits);
    if (S > 1) CSRK_HIP(hipMemsetAsync(dranks, 0, (size_t)n_out * 4, s));      // the partial ranks add onto zero
    const RefLaunch L{score_csr(seen), score_csr(test), drows, n_rows, u_rows, u_packed, dU, ldu, dV, ldv, test->ncols, k, doffsets, n_out,
                      dranks, dscores, S, s};
    score_for_panel(panel_type, panels_wide(dU, ldu, dV, ldv, k, es),
                    [&](auto t, auto w) { ref_launch<typename decltype(t)::type, decltype(w)::value>(L); });
    CSRK_LAUNCH_CHECK();
    return CSRK_OK;
}

// the host form's offsets: the test entries of every listed row, counted on the device and summed here (the host form is
// synchronous anyway); off[n_rows] is their total
static int ref_host_offsets(const Matrix *test, const int32_t *drows, int64_t n_rows, int64_t *dlens, std::vector<int64_t> &off)
{
    rank_entries_for_lens_kernel<<<(unsigned)ref_lens_grid(n_rows), REF_LEN_THREADS>>>(test->d_rowptrs, test->ptr64, drows, n_rows, dlens);
    CSRK_LAUNCH_CHECK();
    const size_t n = (size_t)n_rows;
    off.resize(n + 1);
    CSRK_HIP(hipMemcpy(off.data(), dlens, n * 8, hipMemcpyDeviceToHost));
    int64_t total = 0;
    for (size_t r = 0; r < n; r++) {
        const int64_t len = off[r];
        off[r] = total;
        total += len;
    }
    off[n] = total;
    return CSRK_OK;
}

}  // namespace csrk

using namespace csrk;

extern "C" {

int csrk_rank_entries_for_limits(int64_t *out, int n)
{
    CSRK_REQUIRE(out && n >= 0, "csrk_rank_entries_for_limits: out is NULL or n < 0");
    const int64_t v[2] = {REF_S_MAX, REF_W};
    for (int i = 0; i < n && i < 2; i++) out[i] = v[i];
    return CSRK_OK;
}

int csrk_rank_entries_for_splits(int64_t n_rows, int32_t n_items, int32_t splits, int32_t *splits_used)
{
    CSRK_REQUIRE(splits_used, "rank_entries_for: splits_used is NULL");
    CSRK_REQUIRE(n_rows >= 0, "rank_entries_for: n_rows must not be negative (n_rows=%lld)", (long long)n_rows);
    CSRK_REQUIRE(n_items >= 0, "rank_entries_for: n_items must not be negative (n_items=%d)", n_items);
    CSRK_REQUIRE(splits >= 0, "rank_entries_for: splits must not be negative (splits=%d)", splits);
    *splits_used = ref_splits(n_rows, n_items, splits);
    return CSRK_OK;
}

int csrk_rank_entries_for_device(csrk_handle_t seen, csrk_handle_t test, const int32_t *d_rows, int64_t n_rows, int32_t u_rows,
                                 const void *d_U, int64_t ldu, const void *d_V, int64_t ldv, int32_t k, int panel_type,
                                 const int64_t *d_offsets, int64_t n_out, int32_t *d_ranks, double *d_scores, int32_t splits, void *stream)
{
    Matrix *ms, *mt;
    CSRK_TRY(ref_scalars(n_rows, u_rows, ldu, ldv, k, panel_type, n_out, splits));
    CSRK_TRY(ref_check(seen, test, n_rows, u_rows, splits, &ms, &mt));
    if (n_rows == 0 || n_out == 0) return CSRK_OK;
    return ref_device(ms, mt, d_rows, n_rows, u_rows, 0, d_U, ldu, d_V, ldv, k, panel_type, d_offsets, n_out, d_ranks, d_scores, splits,
                      (hipStream_t)stream);
}

int csrk_rank_entries_for(csrk_handle_t seen, csrk_handle_t test, const int32_t *rows, int64_t n_rows, int32_t u_rows, const void *U,
                          int64_t ldu, const void *V, int64_t ldv, int32_t k, int panel_type, int32_t *ranks, double *scores, int64_t n_out,
                          int32_t splits)
{
    Matrix *ms, *mt;
    // argument checks first, with the caller's pointers (the device call below sees packed copies)
    CSRK_TRY(ref_scalars(n_rows, u_rows, ldu, ldv, k, panel_type, n_out, splits));
    CSRK_TRY(ref_check(seen, test, n_rows, u_rows, splits, &ms, &mt));
    if (n_rows == 0) {
        CSRK_REQUIRE(n_out == 0, "rank_entries_for: n_out=%lld but the listed rows hold 0 test entries", (long long)n_out);
        return CSRK_OK;
    }
    CSRK_REQUIRE(rows, "rank_entries_for: rows is NULL");
    CSRK_REQUIRE(((uintptr_t)rows % 4) == 0, "rank_entries_for: rows is not aligned to its element size");
    CSRK_TRY(check_listed_rows("rank_entries_for", rows, n_rows, u_rows));
    const size_t n = (size_t)n_rows, ne = (size_t)n_out, es = panel_es(panel_type);
    DevBuf dR, dO, dU, dV, dK, dS;
    std::vector<int64_t> off;
    CSRK_TRY(dR.alloc(n * 4));
    CSRK_TRY(dO.alloc((n + 1) * 8));
    CSRK_HIP(hipMemcpy(dR.p, rows, n * 4, hipMemcpyHostToDevice));
    CSRK_TRY(ref_host_offsets(mt, dR.as<int32_t>(), n_rows, dO.as<int64_t>(), off));
    CSRK_REQUIRE(n_out == off[n], "rank_entries_for: n_out=%lld but the listed rows hold %lld test entries", (long long)n_out,
                 (long long)off[n]);
    if (n_out == 0) return CSRK_OK;
    CSRK_REQUIRE(ranks, "rank_entries_for: ranks is NULL");
    CSRK_REQUIRE(U && V, "rank_entries_for: U or V is NULL");
    CSRK_REQUIRE(((uintptr_t)U % es) == 0 && ((uintptr_t)V % es) == 0 && ((uintptr_t)scores % 8) == 0 && ((uintptr_t)ranks % 4) == 0,
                 "rank_entries_for: rows, offsets, U, V, ranks or scores is not aligned to its element size");
    CSRK_HIP(hipMemcpy(dO.p, off.data(), (n + 1) * 8, hipMemcpyHostToDevice));
    CSRK_TRY(pack_listed_rows(dU, U, ldu, k, es, rows, n));
    CSRK_TRY(pack_panel(dV, V, ldv, k, es, (size_t)mt->ncols));
    CSRK_TRY(dK.alloc(ne * 4));
    if (scores) CSRK_TRY(dS.alloc(ne * 8));
    CSRK_TRY(ref_device(ms, mt, dR.as<int32_t>(), n_rows, u_rows, 1, dU.p, k, dV.p, k, k, panel_type, dO.as<int64_t>(), n_out,
                        dK.as<int32_t>(), scores ? dS.as<double>() : nullptr, splits, nullptr));
    CSRK_HIP(hipMemcpy(ranks, dK.p, ne * 4, hipMemcpyDeviceToHost));
    if (scores) CSRK_HIP(hipMemcpy(scores, dS.p, ne * 8, hipMemcpyDeviceToHost));
    return CSRK_OK;
}

}  // extern "C"
