// Recommendations from a factor model for libcsrk on gfx950: csrk_topk_scores scores every item against a block of users
// from the dense panels U and V, drops the pairs a CSR matrix `seen` stores and the scores below a threshold, and keeps the
// n_top best per row (the contract is in include/csrk.h).  The rows x n_items block of scores never leaves the chip.
//
// Score.  A register-tiled float64 product without any matrix instruction: a 256-thread workgroup owns TS_ROWS (64) rows of U
// and sweeps V in tiles of TS_TILE (64) items; thread (ty, tx) = (tid / 16, tid % 16) owns the 4 x 4 chains of rows
// 4 ty .. 4 ty + 3 and items 4 tx .. 4 tx + 3 of the tile.  U's block and V's tile go through LDS TS_KC (16) factors at a time
// (two buffers, the next chunk's loads in flight in registers while this one is used),
// transposed ([factor][row], 66 doubles per line: the 16-B reads of four neighbouring rows stay aligned and the transposing
// writes of a wavefront fall into 64 different banks), and every chain takes its factors in ascending order:
//     s = fma(U[i][t], V[j][t], s)
// one fused multiply-add per factor, float32 widened exactly first.  Nothing is summed in pieces.
//
// Selection.  A row's running list lives in LDS: up to CAP (score bits, item) pairs, of which the first cnt are in use, and a
// threshold thr = the key (topk_key of topk_order.h) of the row's n_top-th best at its last compaction, 0 while
// fewer than n_top are known.  After a tile a score SURVIVES when its item exists, it does not fail min_score, its key is
// above thr (items arrive in ascending order, so on equal keys the listed, smaller item wins) and `seen` does not store the
// pair (a binary search of the row's sorted columns, made only for scores that got this far).  Most tiles of a long sweep
// have no survivor at all: one workgroup-wide OR ends them.  Otherwise the survivors are appended in four passes (item
// 4 tx + p of every thread in pass p: at most 16 per row and pass) at slots handed out by an integer LDS atomic, and after
// each pass every row with more than CAP - 16 entries -- or with n_top entries and no threshold yet -- is COMPACTED by one
// wavefront: an entry's rank is the number of entries that beat it (larger key, or equal key and smaller item), counted
// all-pairs; entries of rank < n_top move to slot `rank`, the rest are dropped, thr becomes the key at rank n_top - 1.  The
// slot an atomic hands out decides nothing: ranks do.  After the last tile every row is compacted once more, which sorts
// it, and the list is written out with its padding.
//
// Two list classes keep LDS in bounds: n_top <= 32 holds 48 entries per row (71 KiB per workgroup with the staging lines:
// two workgroups per CU), n_top <= 128 holds 144 (143 KiB: one per CU).
#include <cstdlib>

#include "common.h"
#include "score_host.h"
#include "score_list.h"
#include "score_tile.h"

namespace csrk {

template <class T, bool WIDE, int CLS>
__global__ __launch_bounds__(TS_THREADS) void topk_scores_kernel(const void *__restrict__ rp, int ptr64, const int32_t *__restrict__ ci,
                                                                int32_t row_begin, int32_t nrows, const T *__restrict__ U, int64_t ldu,
                                                                const T *__restrict__ V, int64_t ldv, int32_t n_items, int32_t k,
                                                                int32_t n_top, double min_score, int select,
                                                                int32_t *__restrict__ items, int64_t ldi, double *__restrict__ scores,
                                                                int64_t lds, int32_t *__restrict__ counts)
{
    constexpr int CAP = TsClass<CLS>::CAP;
    constexpr int PER = WIDE ? 16 / (int)sizeof(T) : 1;
    __shared__ __attribute__((aligned(16))) double su2[2][TS_KC][TS_LD];      // two buffers: one barrier per chunk
    __shared__ __attribute__((aligned(16))) double sv2[2][TS_KC][TS_LD];
    __shared__ uint64_t s_sc[TS_ROWS][CAP];
    __shared__ int32_t s_it[TS_ROWS][CAP];
    __shared__ uint64_t s_thr[TS_ROWS];
    __shared__ int64_t s_e0[TS_ROWS], s_e1[TS_ROWS];
    __shared__ int32_t s_cnt[TS_ROWS];

    const int tid = threadIdx.x, ty = tid / (TS_TILE / TS_B), tx = tid % (TS_TILE / TS_B);
    const int lane = tid & (WAVE - 1), w = tid / WAVE;
    const int64_t r0 = (int64_t)blockIdx.x * TS_ROWS;             // the block's first row, relative to row_begin
    const int64_t nvalid = (int64_t)nrows - r0 < TS_ROWS ? (int64_t)nrows - r0 : TS_ROWS;

    if (tid < TS_ROWS) {
        const bool ok = tid < nvalid;
        s_cnt[tid] = 0;
        s_thr[tid] = ok ? 0ull : ~0ull;                           // a row that does not exist takes nothing
        int64_t e0 = 0, e1 = 0;
        if (ok && rp) {
            const int64_t row = (int64_t)row_begin + r0 + tid;
            e0 = ptr64 ? ((const int64_t *)rp)[row] : (int64_t)((const int32_t *)rp)[row];
            e1 = ptr64 ? ((const int64_t *)rp)[row + 1] : (int64_t)((const int32_t *)rp)[row + 1];
        }
        s_e0[tid] = e0;
        s_e1[tid] = e1;
    }
    __syncthreads();
    uint64_t thr[TS_B];
#pragma unroll
    for (int i = 0; i < TS_B; i++) thr[i] = s_thr[TS_B * ty + i];
    uint64_t sink = 0;
    TsUnits<T, PER> fu, fv;                                       // the chunk after the one in use
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
                const bool more = t0 + TS_KC < k;                 // the next chunk: of this tile, or the first of the next tile
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
        if (!select) {                                            // diagnostic: the product alone
#pragma unroll
            for (int i = 0; i < TS_B; i++)
#pragma unroll
                for (int jj = 0; jj < TS_B; jj++) sink ^= (uint64_t)__double_as_longlong(acc[i][jj]);
            continue;
        }

        // ---- survivors: bit 4 i + jj for the chain of row 4 ty + i and item j0 + 4 tx + jj
        uint32_t mask = 0;
#pragma unroll
        for (int i = 0; i < TS_B; i++)
#pragma unroll
            for (int jj = 0; jj < TS_B; jj++) {
                const int64_t j = j0 + TS_B * tx + jj;
                const double s = acc[i][jj];
                if (j < n_items && !(s < min_score) && topk_key(s) > thr[i]) {
                    const int r = TS_B * ty + i;
                    if (!(rp && ts_seen(ci, s_e0[r], s_e1[r], (int32_t)j))) mask |= 1u << (TS_B * i + jj);
                }
            }
        if (!__syncthreads_or(mask != 0)) continue;
#pragma unroll
        for (int jj = 0; jj < TS_B; jj++) {
#pragma unroll
            for (int i = 0; i < TS_B; i++)
                if (mask & (1u << (TS_B * i + jj))) {
                    const int r = TS_B * ty + i;
                    const int slot = atomicAdd(&s_cnt[r], 1);     // (< CAP: at most CAP - TS_PASS before the pass; the slot decides nothing)
                    s_sc[r][slot] = (uint64_t)__double_as_longlong(acc[i][jj]);
                    s_it[r][slot] = (int32_t)(j0 + TS_B * tx + jj);
                }
            __syncthreads();
            bool full = false;
            if (tid < TS_ROWS) full = s_cnt[tid] > CAP - TS_PASS || (s_cnt[tid] >= n_top && s_thr[tid] == 0);
            if (__syncthreads_or(full)) {
                for (int r = w; r < TS_ROWS; r += TS_THREADS / WAVE)
                    if (s_cnt[r] > n_top || (s_cnt[r] == n_top && s_thr[r] == 0))
                        ts_compact<CAP>(s_sc[r], s_it[r], &s_cnt[r], &s_thr[r], n_top, lane);
                __syncthreads();
            }
        }
        // thresholds change only between tiles: within a tile a listed item may be larger than a later pass's
#pragma unroll
        for (int i = 0; i < TS_B; i++) thr[i] = s_thr[TS_B * ty + i];
    }

    if (!select) {
        if (sink == 0x7ff8c0dec0dec0deull && tid < nvalid) scores[(r0 + tid) * lds] = 0.0;      // (keeps the product alive)
        return;
    }
    __syncthreads();
    for (int r = w; r < TS_ROWS; r += TS_THREADS / WAVE)
        if (s_cnt[r] > 1) ts_compact<CAP>(s_sc[r], s_it[r], &s_cnt[r], &s_thr[r], n_top, lane);
    __syncthreads();
    for (int x = tid; x < TS_ROWS * n_top; x += TS_THREADS) {
        const int r = x / n_top, q = x - r * n_top;
        if (r >= nvalid) break;
        const bool in = q < s_cnt[r];
        items[(r0 + r) * ldi + q] = in ? s_it[r][q] : -1;
        scores[(r0 + r) * lds + q] = in ? __longlong_as_double((long long)s_sc[r][q]) : -INFINITY;
    }
    if (counts && tid < nvalid) counts[r0 + tid] = s_cnt[tid];
}

// the kernel's arguments in its order (the grid follows from n)
struct TsLaunch {
    ScoreCsr seen;
    int32_t row_begin, n;
    const void *U;
    int64_t ldu;
    const void *V;
    int64_t ldv;
    int32_t n_items, k, n_top;
    double min_score;
    int select;
    int32_t *items;
    int64_t ldi;
    double *scores;
    int64_t lds;
    int32_t *counts;
    hipStream_t s;
};

template <class T, bool WIDE, int CLS> static void ts_launch(const TsLaunch &a)
{
    topk_scores_kernel<T, WIDE, CLS><<<(unsigned)score_row_blocks(a.n), TS_THREADS, 0, a.s>>>(
        a.seen.rp, a.seen.ptr64, a.seen.ci, a.row_begin, a.n, (const T *)a.U, a.ldu, (const T *)a.V, a.ldv, a.n_items, a.k, a.n_top,
        a.min_score, a.select, a.items, a.ldi, a.scores, a.lds, a.counts);
}

// the handle (seen may be 0), then every refusal that needs no look at the pointers; the caller holds no lock
static int ts_check(csrk_handle_t seen, int32_t row_begin, int32_t row_end, int64_t ldu, int64_t ldv, int32_t n_items, int32_t k,
                    int panel_type, int32_t n_top, double min_score, int64_t ldi, int64_t lds, Matrix **mp)
{
    Matrix *m;
    CSRK_TRY(optional_handle(seen, &m));
    CSRK_CHECK_K("topk_scores: ", k);
    CSRK_REQUIRE(n_top >= 1, "topk_scores: n_top must be at least 1 (n_top=%d)", n_top);
    CSRK_REQUIRE(n_items >= 0, "topk_scores: n_items must not be negative (n_items=%d)", n_items);
    CSRK_CHECK_TWO_PANELS("topk_scores: ", k, ldu, ldv);
    CSRK_REQUIRE(ldi >= n_top && lds >= n_top, "topk_scores: bad output geometry n_top=%d ldi=%lld lds=%lld", n_top, (long long)ldi,
                 (long long)lds);
    CSRK_CHECK_PANEL_TYPE("topk_scores: ", panel_type);
    CSRK_REQUIRE(min_score == min_score, "topk_scores: min_score is NaN");
    CSRK_CHECK_ROW_ORDER("topk_scores: ", row_begin, row_end);
    if (m) {
        CSRK_CHECK_ROW_RANGE("topk_scores: ", row_begin, row_end, m->nrows);
        CSRK_REQUIRE(n_items == m->ncols, "topk_scores: n_items=%d but seen has %d columns", n_items, m->ncols);
        CSRK_TRY(check_seen_canonical("topk_scores", m));
    }
    CSRK_TRY(check_supported(ts_k_supported(k), "csrk_topk_scores", "k", k, TS_K_MAX, "csrk_topk_scores_limits"));
    CSRK_TRY(check_supported(ts_ntop_supported(n_top), "csrk_topk_scores", "n_top", n_top, TS_NTOP_MAX, "csrk_topk_scores_limits"));
    *mp = m;
    return CSRK_OK;
}

static int ts_nulls(const void *items, const void *scores, const void *U, const void *V, int32_t n_items)
{
    CSRK_REQUIRE(items && scores, "topk_scores: items or scores is NULL");
    CSRK_REQUIRE(U, "topk_scores: U is NULL");
    CSRK_REQUIRE(V || n_items == 0, "topk_scores: V is NULL");
    return CSRK_OK;
}

// dU points at row row_begin of U
static int ts_device(Matrix *m, int32_t row_begin, int32_t row_end, const void *dU, int64_t ldu, const void *dV, int64_t ldv,
                     int32_t n_items, int32_t k, int panel_type, int32_t n_top, double min_score, int32_t *ditems, int64_t ldi,
                     double *dscores, int64_t lds, int32_t *dcounts, hipStream_t s)
{
    if (row_begin == row_end) return CSRK_OK;
    CSRK_TRY(ts_nulls(ditems, dscores, dU, dV, n_items));
    const size_t es = panel_es(panel_type);
    CSRK_REQUIRE(((uintptr_t)dU % es) == 0 && ((uintptr_t)dV % es) == 0 && ((uintptr_t)dscores % 8) == 0 &&
                     ((uintptr_t)ditems % 4) == 0 && ((uintptr_t)dcounts % 4) == 0,
                 "topk_scores: U, V, items, scores or counts is not aligned to its element size");
    mark_user_stream(m, s);
    const int select = score_knob_on(getenv("CSRK_TOPK_SCORES_SELECT"));      // diagnostic: "0" times the product alone (the outputs are not written)
    const TsLaunch L{score_csr(m), row_begin, row_end - row_begin, dU, ldu, dV, ldv, n_items, k, n_top, min_score, select, ditems, ldi,
                     dscores, lds, dcounts, s};
    score_for_panel(panel_type, panels_wide(dU, ldu, dV, ldv, k, es), [&](auto t, auto w) {
        using T = typename decltype(t)::type;
        if (ts_small_class(n_top)) ts_launch<T, decltype(w)::value, 0>(L);
        else ts_launch<T, decltype(w)::value, 1>(L);
    });
    CSRK_LAUNCH_CHECK();
    return CSRK_OK;
}

}  // namespace csrk

using namespace csrk;

extern "C" {

int csrk_topk_scores_limits(int64_t *out, int n)
{
    CSRK_REQUIRE(out && n >= 0, "csrk_topk_scores_limits: out is NULL or n < 0");
    const int64_t v[6] = {TS_K_MAX, TS_NTOP_MAX, TS_ROWS, TS_TILE, TS_KC, TsClass<0>::CAP};
    for (int i = 0; i < n && i < 6; i++) out[i] = v[i];
    return CSRK_OK;
}

int csrk_topk_scores_device(csrk_handle_t seen, int32_t row_begin, int32_t row_end, const void *d_U, int64_t ldu, const void *d_V,
                            int64_t ldv, int32_t n_items, int32_t k, int panel_type, int32_t n_top, double min_score, int32_t *d_items,
                            int64_t ldi, double *d_scores, int64_t lds, int32_t *d_counts, void *stream)
{
    Matrix *m;
    CSRK_TRY(ts_check(seen, row_begin, row_end, ldu, ldv, n_items, k, panel_type, n_top, min_score, ldi, lds, &m));
    const void *u0 = panel_rows_from(d_U, row_begin, ldu, panel_es(panel_type));
    return ts_device(m, row_begin, row_end, u0, ldu, d_V, ldv, n_items, k, panel_type, n_top, min_score, d_items, ldi, d_scores, lds,
                     d_counts, (hipStream_t)stream);
}

int csrk_topk_scores(csrk_handle_t seen, int32_t row_begin, int32_t row_end, const void *U, int64_t ldu, const void *V, int64_t ldv,
                     int32_t n_items, int32_t k, int panel_type, int32_t n_top, double min_score, int32_t *items, int64_t ldi,
                     double *scores, int64_t lds, int32_t *counts)
{
    Matrix *m;
    // argument checks first, with the caller's pointers (the device call below sees packed copies)
    CSRK_TRY(ts_check(seen, row_begin, row_end, ldu, ldv, n_items, k, panel_type, n_top, min_score, ldi, lds, &m));
    if (row_begin == row_end) return CSRK_OK;
    CSRK_TRY(ts_nulls(items, scores, U, V, n_items));
    const size_t es = panel_es(panel_type), n = (size_t)(row_end - row_begin);
    int dev = 0;
    CSRK_HIP(hipGetDevice(&dev));                                           // (without a handle nothing vouches for a device)
    DevBuf dU, dV, dI, dS, dC;
    CSRK_TRY(pack_panel(dU, panel_rows_from(U, row_begin, ldu, es), ldu, k, es, n));
    CSRK_TRY(pack_panel(dV, V, ldv, k, es, n_items));
    CSRK_TRY(dI.alloc(n * n_top * 4));
    CSRK_TRY(dS.alloc(n * n_top * 8));
    CSRK_TRY(dC.alloc(n * 4));
    CSRK_TRY(ts_device(m, row_begin, row_end, dU.p, k, dV.p, k, n_items, k, panel_type, n_top, min_score, dI.as<int32_t>(), n_top,
                       dS.as<double>(), n_top, dC.as<int32_t>(), nullptr));
    CSRK_TRY(unpack_panel(items, ldi, dI, n_top, 4, n));
    CSRK_TRY(unpack_panel(scores, lds, dS, n_top, 8, n));
    if (counts) CSRK_HIP(hipMemcpy(counts, dC.p, n * 4, hipMemcpyDeviceToHost));
    return CSRK_OK;
}

}  // extern "C"
