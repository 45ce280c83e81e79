// The running lists that topk_scores.hip and topk_scores_for.hip share: the list classes and the compaction of one row's list by
// one wavefront (moved here from topk_scores.hip unchanged), and ts_sweep, topk_scores_kernel's body made general in three
// things and in nothing else:
//   * where a block's rows come from: a list of absolute rows staged in LDS (the row of `seen`, and the row of U unless U
//     travels packed in list order), not a range;
//   * the item interval [j_begin, j_end) it sweeps (whole tiles from j_begin), not [0, n_items);
//   * where the final lists go: the outputs with their padding, or (work != NULL) the workspace slot of (output row, split):
//     the count, and the first `count` score bits and items, best first.
// The product, the survivors, the passes and the compactions are topk_scores_kernel's line for line, so a score and a list
// have the same bits in either.  topk_scores_kernel itself keeps its own text: instantiated from ts_sweep it compiled to a
// different schedule and measured up to 1.3 % slower at k = 16.
#pragma once
#include "common.h"
#include "score_tile.h"

namespace csrk {

constexpr int TS_PASS = TS_TILE / TS_B;         // most survivors a row takes in one pass
// (TS_K_MAX, TS_NTOP_SMALL, TS_NTOP_MAX and the TSF_* constants: score_plan.h)

template <int CLS> struct TsClass;
template <> struct TsClass<0> { static constexpr int NTOP = TS_NTOP_SMALL, CAP = TS_NTOP_SMALL + TS_PASS; };
template <> struct TsClass<1> { static constexpr int NTOP = TS_NTOP_MAX, CAP = TS_NTOP_MAX + TS_PASS; };

// one wavefront orders the list of one row and cuts it to n_top (every lane of the wavefront calls it)
template <int CAP>
__device__ __forceinline__ void ts_compact(uint64_t *__restrict__ sc, int32_t *__restrict__ it, int32_t *__restrict__ cnt,
                                           uint64_t *__restrict__ thr, int n_top, int lane)
{
    constexpr int EPL = (CAP + WAVE - 1) / WAVE;                  // entries per lane
    const int n = *cnt;
    uint64_t bits[EPL], key[EPL];
    int32_t item[EPL];
    int rank[EPL];
#pragma unroll
    for (int e = 0; e < EPL; e++) {
        const int x = lane + e * WAVE;
        bits[e] = x < n ? sc[x] : 0;
        item[e] = x < n ? it[x] : 0;
        key[e] = topk_key(__longlong_as_double((long long)bits[e]));
        rank[e] = 0;
    }
    for (int j = 0; j < n; j++) {
        const uint64_t kj = topk_key(__longlong_as_double((long long)sc[j]));
        const int32_t ij = it[j];
#pragma unroll
        for (int e = 0; e < EPL; e++) rank[e] += (kj > key[e] || (kj == key[e] && ij < item[e])) ? 1 : 0;
    }
    // the wavefront has read the list before any lane rewrites it (LDS operations of one wavefront complete in issue order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
    for (int e = 0; e < EPL; e++) {
        const int x = lane + e * WAVE;
        if (x < n && rank[e] < n_top) {
            sc[rank[e]] = bits[e];
            it[rank[e]] = item[e];
            if (rank[e] == n_top - 1) *thr = key[e];
        }
    }
    if (lane == 0) *cnt = n < n_top ? n : n_top;
}

// The workspace of csrk_topk_scores_for for n_rows output rows, S splits and n_top: three arrays over the slots
// slot = output row * S + split, one after the other -- score bits [slots][n_top] (8 B), items [slots][n_top] (4 B),
// counts [slots] (4 B): TSF_SLOT_BYTES + (n_top - 1) * TSF_NTOP_BYTES per slot (score_plan.h, tsf_work_bytes), every array
// aligned to its element.
struct TsWork {
    uint64_t *sc;
    int32_t *it, *cnt;
};
__host__ __device__ __forceinline__ TsWork ts_work(void *work, int64_t slots, int32_t n_top)
{
    TsWork w;
    w.sc = (uint64_t *)work;
    w.it = (int32_t *)(w.sc + slots * n_top);
    w.cnt = w.it + slots * n_top;
    return w;
}

// ts_fetch for rows named one by one.  A thread loads the same rows of the block in every chunk, so it keeps their places in
// registers: ts_row_offsets reads urow[r] (LDS: the panel row of the block's row r, -1 for a row that takes nothing) once.
template <class T, int PER>
__device__ __forceinline__ void ts_row_offsets(int64_t *off, const int64_t *urow, int64_t ld, int tid)
{
    typedef TsUnits<T, PER> N;
#pragma unroll
    for (int l = 0; l < N::NL; l++) {
        const int64_t row = urow[(tid + l * TS_THREADS) / N::UPR];
        off[l] = row < 0 ? -1 : row * ld;
    }
}

template <class T, int PER>
__device__ __forceinline__ void ts_fetch_rows(TsUnits<T, PER> &u, const T *__restrict__ P, const int64_t *off, int t0, int k,
                                              int tid)
{
    typedef TsUnits<T, PER> N;
#pragma unroll
    for (int l = 0; l < N::NL; l++) {
        const int t = t0 + ((tid + l * TS_THREADS) % N::UPR) * PER;
#pragma unroll
        for (int e = 0; e < PER; e++) u.d[l][e] = 0.0;
        if (off[l] >= 0 && t < k) panel_unit<T, PER>(P + off[l] + t, u.d[l]);
    }
}

// Output row r0 + r is row rows[r0 + r] of `seen` and of U (u_packed: row r0 + r of U); an index outside [0, u_rows) is not
// dereferenced, its row takes nothing and gets count -1.  r0 = blockIdx.x * TS_ROWS; nrows = the rows of the list.
// work != NULL: the lists go to slot (r0 + r) * n_splits + split instead of the outputs.
template <class T, bool WIDE, int CLS>
__device__ __forceinline__ void ts_sweep(const void *__restrict__ rp, int ptr64, const int32_t *__restrict__ ci, int64_t nrows,
                                         const int32_t *__restrict__ rows, int32_t u_rows, int u_packed, const T *__restrict__ U,
                                         int64_t ldu, const T *__restrict__ V, int64_t ldv, int64_t j_begin, int64_t j_end, int32_t k,
                                         int32_t n_top, double min_score, int32_t *__restrict__ items, int64_t ldi,
                                         double *__restrict__ scores, int64_t lds, int32_t *__restrict__ counts,
                                         void *__restrict__ work, int split, int n_splits)
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
    __shared__ int64_t s_urow[TS_ROWS];                           // the row of U, -1 for none
    __shared__ int32_t s_bad[TS_ROWS];                            // the index is outside [0, u_rows)

    const int tid = threadIdx.x, ty = tid / (TS_TILE / TS_B), tx = tid % (TS_TILE / TS_B);
    const int lane = tid & (WAVE - 1), w = tid / WAVE;
    const int64_t r0 = (int64_t)blockIdx.x * TS_ROWS;             // the block's first row, as a place in the list
    const int64_t nvalid = (int64_t)nrows - r0 < TS_ROWS ? (int64_t)nrows - r0 : TS_ROWS;

    if (tid < TS_ROWS) {
        const int64_t row = tid < nvalid ? (int64_t)rows[r0 + tid] : -1;
        const bool ok = row >= 0 && row < u_rows;
        s_bad[tid] = tid < nvalid && !ok;
        s_urow[tid] = ok ? (u_packed ? r0 + tid : row) : -1;
        s_cnt[tid] = 0;
        s_thr[tid] = ok ? 0ull : ~0ull;                           // a row that does not exist takes nothing
        int64_t e0 = 0, e1 = 0;
        if (ok && rp) {
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
    TsUnits<T, PER> fu, fv;                                       // the chunk after the one in use
    int64_t u_off[TsUnits<T, PER>::NL];                           // where this thread's rows of U start
    ts_row_offsets<T, PER>(u_off, s_urow, ldu, tid);
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
                const bool more = t0 + TS_KC < k;                 // the next chunk: of this tile, or the first of the next tile
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
        // ---- survivors: bit 4 i + jj for the chain of row 4 ty + i and item j0 + 4 tx + jj
        uint32_t mask = 0;
#pragma unroll
        for (int i = 0; i < TS_B; i++)
#pragma unroll
            for (int jj = 0; jj < TS_B; jj++) {
                const int64_t j = j0 + TS_B * tx + jj;
                const double s = acc[i][jj];
                if (j < j_end && !(s < min_score) && topk_key(s) > thr[i]) {
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

    __syncthreads();
    for (int r = w; r < TS_ROWS; r += TS_THREADS / WAVE)
        if (s_cnt[r] > 1) ts_compact<CAP>(s_sc[r], s_it[r], &s_cnt[r], &s_thr[r], n_top, lane);
    __syncthreads();
    if (work) {                                                   // the partial lists of this split: what is in use, no padding
        const TsWork ws = ts_work(work, nrows * n_splits, n_top);
        for (int x = tid; x < TS_ROWS * n_top; x += TS_THREADS) {
            const int r = x / n_top, q = x - r * n_top;
            if (r >= nvalid) break;
            if (q < s_cnt[r]) {
                const int64_t at = ((r0 + r) * n_splits + split) * n_top + q;
                ws.sc[at] = s_sc[r][q];
                ws.it[at] = s_it[r][q];
            }
        }
        if (tid < nvalid) ws.cnt[(r0 + tid) * n_splits + split] = s_cnt[tid];
        return;
    }
    for (int x = tid; x < TS_ROWS * n_top; x += TS_THREADS) {
        const int r = x / n_top, q = x - r * n_top;
        if (r >= nvalid) break;
        const bool in = q < s_cnt[r];
        items[(r0 + r) * ldi + q] = in ? s_it[r][q] : -1;
        scores[(r0 + r) * lds + q] = in ? __longlong_as_double((long long)s_sc[r][q]) : -INFINITY;
    }
    if (counts && tid < nvalid) counts[r0 + tid] = s_bad[tid] ? -1 : s_cnt[tid];
}

}  // namespace csrk
