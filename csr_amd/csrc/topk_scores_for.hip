// Serving from a factor model for libcsrk on gfx950: csrk_topk_scores_for is csrk_topk_scores for a LIST of rows, with the
// items cut into S contiguous ranges of whole tiles so that a handful of rows still fills the card (the contract is in
// include/csrk.h).  Every score, every list and every compaction is topk_scores.hip's: ts_sweep of score_list.h is that
// kernel's body, over a list of rows staged in LDS and over one range of items.
//
// Two launches when S > 1, one when S = 1:
//   sweep   grid (row blocks, S): workgroup (b, s) takes rows 64 b .. of the list and the tiles [s T / S, (s + 1) T / S),
//           keeps the rows' running lists in LDS and writes each row's final partial list -- the count, then the score bits
//           and items in use, best first -- to slot (row, s) of the caller's workspace.  S = 1 writes the outputs instead.
//   merge   one wavefront per output row.  The S partial lists are sorted in the order of rule 4 and hold disjoint items, so
//           the place of a candidate in the row's list is its place in its own list plus, for every other list, the number
//           of entries that come before it there: a binary search each.  Places below n_top are written, the rest of the
//           row is padding.  Places are counted, nothing is appended in arrival order; there is no atomic at all.
// No workgroup waits for another, and neither kernel has a loop without a bound.
#include "common.h"
#include "score_host.h"
#include "score_list.h"
#include "score_tile.h"

namespace csrk {

// (the constants TSF_*, the split rule and the item interval of a split: score_plan.h)
template <class T, bool WIDE, int CLS>
__global__ __launch_bounds__(TS_THREADS) void topk_scores_for_kernel(const void *__restrict__ rp, int ptr64, const int32_t *__restrict__ ci,
                                                                    const int32_t *__restrict__ rows, int64_t n_rows, int32_t u_rows,
                                                                    int u_packed, const T *__restrict__ U, int64_t ldu,
                                                                    const T *__restrict__ V, int64_t ldv, int32_t n_items, int32_t k,
                                                                    int32_t n_top, double min_score, int32_t *__restrict__ items,
                                                                    int64_t ldi, double *__restrict__ scores, int64_t lds,
                                                                    int32_t *__restrict__ counts, void *__restrict__ work, int n_splits)
{
    const int split = blockIdx.y;
    const ScoreItemRange j = score_item_range(split, n_splits, n_items);
    ts_sweep<T, WIDE, CLS>(rp, ptr64, ci, n_rows, rows, u_rows, u_packed, U, ldu, V, ldv, j.j_begin, j.j_end, k, n_top, min_score, items,
                           ldi, scores, lds, counts, work, split, n_splits);
}

__global__ __launch_bounds__(TSF_MERGE_THREADS) void topk_scores_for_merge_kernel(const int32_t *__restrict__ rows, int64_t n_rows,
                                                                                 int32_t u_rows, int32_t n_top, int n_splits,
                                                                                 const void *__restrict__ work, int32_t *__restrict__ items,
                                                                                 int64_t ldi, double *__restrict__ scores, int64_t lds,
                                                                                 int32_t *__restrict__ counts)
{
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    constexpr int RPB = TSF_MERGE_THREADS / WAVE;                 // rows per workgroup and step
    const TsWork ws = ts_work(const_cast<void *>(work), n_rows * n_splits, n_top);
    for (int64_t row = (int64_t)blockIdx.x * RPB + w; row < n_rows; row += (int64_t)gridDim.x * RPB) {
        const int32_t at = rows[row];
        const bool bad = at < 0 || at >= u_rows;                  // (the sweep wrote count 0 for it)
        const int32_t *cnt = ws.cnt + row * n_splits;
        int total = 0;
        for (int t = 0; t < n_splits; t++) total += cnt[t];
        const int kept = bad ? 0 : (total < n_top ? total : n_top);
        for (int q = kept + lane; q < n_top; q += WAVE) {
            items[row * ldi + q] = -1;
            scores[row * lds + q] = -INFINITY;
        }
        if (counts && lane == 0) counts[row] = bad ? -1 : kept;
        if (bad) continue;
        for (int c = lane; c < n_splits * n_top; c += WAVE) {
            const int s = c / n_top, p = c - s * n_top;
            if (p >= cnt[s]) continue;
            const int64_t x = (row * n_splits + s) * n_top + p;
            const uint64_t bits = ws.sc[x], key = topk_key(__longlong_as_double((long long)bits));
            const int32_t item = ws.it[x];
            int place = p;
            for (int t = 0; t < n_splits && place < n_top; t++) {
                if (t == s) continue;
                const int64_t base = (row * n_splits + t) * n_top;
                int lo = 0, hi = cnt[t] < n_top - place ? cnt[t] : n_top - place;      // (beyond n_top no place matters)
                while (lo < hi) {
                    const int mid = lo + ((hi - lo) >> 1);
                    if (key_before(topk_key(__longlong_as_double((long long)ws.sc[base + mid])), ws.it[base + mid], key, item))
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                place += lo;
            }
            if (place < n_top) {
                items[row * ldi + place] = item;
                scores[row * lds + place] = __longlong_as_double((long long)bits);
            }
        }
    }
}

// the sweep's arguments in its order (the grid: row blocks x S)
struct TsfLaunch {
    ScoreCsr seen;
    const int32_t *rows;
    int64_t n_rows;
    int32_t u_rows;
    int u_packed;
    const void *U;
    int64_t ldu;
    const void *V;
    int64_t ldv;
    int32_t n_items, k, n_top;
    double min_score;
    int32_t *items;
    int64_t ldi;
    double *scores;
    int64_t lds;
    int32_t *counts;
    void *work;
    int S;
    hipStream_t s;
};

template <class T, bool WIDE, int CLS> static void tsf_launch(const TsfLaunch &a)
{
    const dim3 grid((unsigned)score_row_blocks(a.n_rows), (unsigned)a.S);
    topk_scores_for_kernel<T, WIDE, CLS><<<grid, TS_THREADS, 0, a.s>>>(a.seen.rp, a.seen.ptr64, a.seen.ci, a.rows, a.n_rows, a.u_rows,
                                                                       a.u_packed, (const T *)a.U, a.ldu, (const T *)a.V, a.ldv, a.n_items,
                                                                       a.k, a.n_top, a.min_score, a.items, a.ldi, a.scores, a.lds, a.counts,
                                                                       a.work, a.S);
}

static int tsf_unsupported(int64_t n_rows, int32_t k, int32_t n_top)
{
    CSRK_TRY(check_supported(ts_k_supported(k), "topk_scores_for", "k", k, TS_K_MAX, "csrk_topk_scores_limits"));
    CSRK_TRY(check_supported(ts_ntop_supported(n_top), "topk_scores_for", "n_top", n_top, TS_NTOP_MAX, "csrk_topk_scores_limits"));
    if (tsf_grid_too_large(n_rows)) {
        set_error("topk_scores_for: n_rows=%lld makes more row blocks than a grid holds (%lld)", (long long)n_rows, (long long)TSF_GRID_MAX);
        return CSRK_ERR_UNSUPPORTED;
    }
    return CSRK_OK;
}

// the handle (seen may be 0), then every refusal that needs no look at the pointers, in csrk_topk_scores' order; the caller
// holds no lock
static int tsf_check(csrk_handle_t seen, int64_t n_rows, int32_t u_rows, int64_t ldu, int64_t ldv, int32_t n_items, int32_t k,
                     int panel_type, int32_t n_top, double min_score, int64_t ldi, int64_t lds, int32_t splits, Matrix **mp)
{
    Matrix *m;
    CSRK_TRY(optional_handle(seen, &m));
    CSRK_CHECK_K("topk_scores_for: ", k);
    CSRK_REQUIRE(n_top >= 1, "topk_scores_for: n_top must be at least 1 (n_top=%d)", n_top);
    CSRK_REQUIRE(n_items >= 0, "topk_scores_for: n_items must not be negative (n_items=%d)", n_items);
    CSRK_CHECK_TWO_PANELS("topk_scores_for: ", k, ldu, ldv);
    CSRK_REQUIRE(ldi >= n_top && lds >= n_top, "topk_scores_for: bad output geometry n_top=%d ldi=%lld lds=%lld", n_top, (long long)ldi,
                 (long long)lds);
    CSRK_CHECK_PANEL_TYPE("topk_scores_for: ", panel_type);
    CSRK_REQUIRE(min_score == min_score, "topk_scores_for: min_score is NaN");
    CSRK_REQUIRE(n_rows >= 0, "topk_scores_for: n_rows must not be negative (n_rows=%lld)", (long long)n_rows);
    CSRK_REQUIRE(u_rows >= 0, "topk_scores_for: u_rows must not be negative (u_rows=%d)", u_rows);
    CSRK_REQUIRE(splits >= 0, "topk_scores_for: splits must not be negative (splits=%d)", splits);
    if (m) {
        CSRK_REQUIRE(u_rows == m->nrows, "topk_scores_for: u_rows=%d but seen has %d rows", u_rows, m->nrows);
        CSRK_REQUIRE(n_items == m->ncols, "topk_scores_for: n_items=%d but seen has %d columns", n_items, m->ncols);
        CSRK_TRY(check_seen_canonical("topk_scores_for", m));
    }
    *mp = m;
    return tsf_unsupported(n_rows, k, n_top);
}

static int tsf_nulls(const void *items, const void *scores, const void *rows, const void *U, const void *V, int32_t n_items)
{
    CSRK_REQUIRE(items && scores, "topk_scores_for: items or scores is NULL");
    CSRK_REQUIRE(rows, "topk_scores_for: rows is NULL");
    CSRK_REQUIRE(U, "topk_scores_for: U is NULL");
    CSRK_REQUIRE(V || n_items == 0, "topk_scores_for: V is NULL");
    return CSRK_OK;
}

// S > 1: the caller's workspace holds the partial lists
static int tsf_check_workspace(const void *dwork, int64_t work_bytes, int64_t need, int32_t S)
{
    if (need == 0) return CSRK_OK;
    CSRK_REQUIRE(dwork, "topk_scores_for: the workspace is NULL but %lld bytes are needed (splits_used=%d)", (long long)need, S);
    CSRK_REQUIRE(((uintptr_t)dwork % 16) == 0, "topk_scores_for: the workspace is not aligned to 16 bytes");
    CSRK_REQUIRE(work_bytes >= need, "topk_scores_for: work_bytes=%lld but %lld bytes are needed (splits_used=%d)", (long long)work_bytes,
                 (long long)need, S);
    return CSRK_OK;
}

// u_packed: dU holds the listed rows only, in list order (the host form); drows names rows of `seen` either way
static int tsf_device(Matrix *m, const int32_t *drows, int64_t n_rows, int32_t u_rows, int u_packed, const void *dU, int64_t ldu,
                      const void *dV, int64_t ldv, int32_t n_items, int32_t k, int panel_type, int32_t n_top, double min_score,
                      int32_t *ditems, int64_t ldi, double *dscores, int64_t lds, int32_t *dcounts, int32_t splits, void *dwork,
                      int64_t work_bytes, hipStream_t s)
{
    if (n_rows == 0) return CSRK_OK;
    CSRK_TRY(tsf_nulls(ditems, dscores, drows, dU, dV, n_items));
    const size_t es = panel_es(panel_type);
    CSRK_REQUIRE(((uintptr_t)dU % es) == 0 && ((uintptr_t)dV % es) == 0 && ((uintptr_t)dscores % 8) == 0 &&
                     ((uintptr_t)ditems % 4) == 0 && ((uintptr_t)dcounts % 4) == 0 && ((uintptr_t)drows % 4) == 0,
                 "topk_scores_for: rows, U, V, items, scores or counts is not aligned to its element size");
    const int32_t S = tsf_splits(n_rows, n_items, n_top, splits);
    CSRK_TRY(tsf_check_workspace(dwork, work_bytes, tsf_work_bytes(n_rows, S, n_top), S));
    mark_user_stream(m, s);
    const TsfLaunch L{score_csr(m), drows, n_rows, u_rows, u_packed, dU, ldu, dV, ldv, n_items, k, n_top, min_score, ditems, ldi,
                      dscores, lds, dcounts, S > 1 ? dwork : nullptr, S, s};
    score_for_panel(panel_type, panels_wide(dU, ldu, dV, ldv, k, es), [&](auto t, auto w) {
        using T = typename decltype(t)::type;
        if (ts_small_class(n_top)) tsf_launch<T, decltype(w)::value, 0>(L);
        else tsf_launch<T, decltype(w)::value, 1>(L);
    });
    CSRK_LAUNCH_CHECK();
    if (S > 1) {
        topk_scores_for_merge_kernel<<<(unsigned)tsf_merge_grid(n_rows), TSF_MERGE_THREADS, 0, s>>>(drows, n_rows, u_rows, n_top, S, dwork,
                                                                                                  ditems, ldi, dscores, lds, dcounts);
        CSRK_LAUNCH_CHECK();
    }
    return CSRK_OK;
}

}  // namespace csrk

using namespace csrk;

extern "C" {

int csrk_topk_scores_for_limits(int64_t *out, int n)
{
    CSRK_REQUIRE(out && n >= 0, "csrk_topk_scores_for_limits: out is NULL or n < 0");
    const int64_t v[5] = {TSF_S_MAX, TSF_W_SMALL, TSF_W_LARGE, TSF_SLOT_BYTES, TSF_NTOP_BYTES};
    for (int i = 0; i < n && i < 5; i++) out[i] = v[i];
    return CSRK_OK;
}

int csrk_topk_scores_for_workspace(int64_t n_rows, int32_t n_items, int32_t n_top, int32_t splits, int32_t *splits_used, int64_t *bytes)
{
    CSRK_REQUIRE(splits_used && bytes, "topk_scores_for: splits_used or bytes is NULL");
    CSRK_REQUIRE(n_top >= 1, "topk_scores_for: n_top must be at least 1 (n_top=%d)", n_top);
    CSRK_REQUIRE(n_items >= 0, "topk_scores_for: n_items must not be negative (n_items=%d)", n_items);
    CSRK_REQUIRE(n_rows >= 0, "topk_scores_for: n_rows must not be negative (n_rows=%lld)", (long long)n_rows);
    CSRK_REQUIRE(splits >= 0, "topk_scores_for: splits must not be negative (splits=%d)", splits);
    CSRK_TRY(tsf_unsupported(n_rows, 1, n_top));
    *splits_used = tsf_splits(n_rows, n_items, n_top, splits);
    *bytes = tsf_work_bytes(n_rows, *splits_used, n_top);
    return CSRK_OK;
}

int csrk_topk_scores_for_device(csrk_handle_t seen, const int32_t *d_rows, int64_t n_rows, int32_t u_rows, const void *d_U, int64_t ldu,
                                const void *d_V, int64_t ldv, int32_t n_items, int32_t k, int panel_type, int32_t n_top, double min_score,
                                int32_t *d_items, int64_t ldi, double *d_scores, int64_t lds, int32_t *d_counts, int32_t splits, void *d_work,
                                int64_t work_bytes, void *stream)
{
    Matrix *m;
    CSRK_TRY(tsf_check(seen, n_rows, u_rows, ldu, ldv, n_items, k, panel_type, n_top, min_score, ldi, lds, splits, &m));
    return tsf_device(m, d_rows, n_rows, u_rows, 0, d_U, ldu, d_V, ldv, n_items, k, panel_type, n_top, min_score, d_items, ldi, d_scores, lds,
                      d_counts, splits, d_work, work_bytes, (hipStream_t)stream);
}

int csrk_topk_scores_for(csrk_handle_t seen, const int32_t *rows, int64_t n_rows, int32_t u_rows, const void *U, int64_t ldu, const void *V,
                         int64_t ldv, int32_t n_items, int32_t k, int panel_type, int32_t n_top, double min_score, int32_t *items,
                         int64_t ldi, double *scores, int64_t lds, int32_t *counts, int32_t splits)
{
    Matrix *m;
    // argument checks first, with the caller's pointers (the device call below sees packed copies)
    CSRK_TRY(tsf_check(seen, n_rows, u_rows, ldu, ldv, n_items, k, panel_type, n_top, min_score, ldi, lds, splits, &m));
    if (n_rows == 0) return CSRK_OK;
    CSRK_TRY(tsf_nulls(items, scores, rows, U, V, n_items));
    CSRK_TRY(check_listed_rows("topk_scores_for", rows, n_rows, u_rows));
    const size_t es = panel_es(panel_type), n = (size_t)n_rows;
    const int64_t need = tsf_work_bytes(n_rows, tsf_splits(n_rows, n_items, n_top, splits), n_top);
    int dev = 0;
    CSRK_HIP(hipGetDevice(&dev));                                           // (without a handle nothing vouches for a device)
    DevBuf dR, dU, dV, dI, dS, dC, dW;
    CSRK_TRY(dR.alloc(n * 4));
    CSRK_HIP(hipMemcpy(dR.p, rows, n * 4, hipMemcpyHostToDevice));
    CSRK_TRY(pack_listed_rows(dU, U, ldu, k, es, rows, n));
    CSRK_TRY(pack_panel(dV, V, ldv, k, es, n_items));
    CSRK_TRY(dI.alloc(n * n_top * 4));
    CSRK_TRY(dS.alloc(n * n_top * 8));
    CSRK_TRY(dC.alloc(n * 4));
    CSRK_TRY(dW.alloc((size_t)need));
    CSRK_TRY(tsf_device(m, dR.as<int32_t>(), n_rows, u_rows, 1, dU.p, k, dV.p, k, n_items, k, panel_type, n_top, min_score, dI.as<int32_t>(),
                        n_top, dS.as<double>(), n_top, dC.as<int32_t>(), splits, dW.p, need, nullptr));
    CSRK_TRY(unpack_panel(items, ldi, dI, n_top, 4, n));
    CSRK_TRY(unpack_panel(scores, lds, dS, n_top, 8, n));
    if (counts) CSRK_HIP(hipMemcpy(counts, dC.p, n * 4, hipMemcpyDeviceToHost));
    return CSRK_OK;
}

}  // extern "C"
