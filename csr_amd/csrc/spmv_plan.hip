// SpMV plans for libcsrk on gfx950: everything that is computed ONCE per handle (on its second product: see
// get_plan_locked in spmv.hip) -- the long-row split and its two tiers, the hot-column pack, the light stream and
// its cold staging lists.  The kernels of a product and their launches are in spmv.hip; DESIGN.md section 4 describes
// the forms.  Reference: csr/kernels/numba/__init__.py:55-67 has no plan (one sequential loop).
#include "spmv_plan.h"

#include <algorithm>
#include <cstring>
#include <ctime>
#include <type_traits>

namespace csrk {
// CSRK_PLAN_TRACE (SpmvKnobs::trace): laps of the plan builders on stderr (each lap waits for the device)
struct PlanTrace {
    bool on;
    double t0;
    static double now()
    {
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
    }
    explicit PlanTrace(const SpmvKnobs &knobs) : on(knobs.trace), t0(0.0)
    {
        if (on) {
            (void)hipDeviceSynchronize();
            t0 = now();
        }
    }
    void lap(const char *what)
    {
        if (!on) return;
        (void)hipDeviceSynchronize();
        const double t = now();
        fprintf(stderr, "[csrk plan] %-28s %8.3f ms\n", what, t - t0);
        t0 = t;
    }
};

// tile_row[t] = number of row ends consumed before merge-path diagonal d = min(t*ITEMS, nrows+nnz).
// Row end r (= rp[r+1]) is consumed once all its nnz are: it lies before diagonal d iff
// rp[r+1] + r + 1 <= d.
template <class P>
__global__ void merge_plan_kernel(const P *__restrict__ rp, int32_t nrows, int64_t nnz, int items,
                                  int64_t n_tiles, int32_t *__restrict__ tile_row)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_tiles) return;
    int64_t total = (int64_t)nrows + nnz;
    int64_t d = t * items;
    if (d > total) d = total;
    int64_t lo = d - nnz > 0 ? d - nnz : 0;
    int64_t hi = d < nrows ? d : nrows;
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if ((int64_t)rp[mid + 1] <= d - mid - 1)
            lo = mid + 1;
        else
            hi = mid;
    }
    tile_row[t] = (int32_t)lo;
}

// 4-byte-aligned pair types: tile starts fall on arbitrary nnz indices, and gfx950 global loads
// only need dword alignment, so two consecutive colinds / values are fetched with one
// dwordx2 / dwordx4 load per lane (512 B / 1 KiB per wave-instruction).
// ---- hot-column cache: plan-time kernels ------------------------------------------------------------
// Column reference counts over the rows the tile kernel serves, from every `row_stride`-th GROUP of 64 consecutive rows
// and at most 128 entries of a row (a sample is enough to rank popularity); total[0] = entries counted.  One wavefront per
// group: the rows' kept entries are one run of colinds (but for the rows cut out to the tiers), walked 64 at a time by
// consecutive lanes -- an entry finds its row by bisection in the wavefront's table of row starts.  (A thread per row
// walking its entries one after the other waited out a memory round trip per entry with two workgroups on a CU: 2.8 ms of
// the headline matrix's plan, its largest item.)
// Popular columns collect millions of these increments: as global atomics they serialise (14 ms for the 4*10^7
// sampled entries of the headline matrix).  Each persistent workgroup therefore counts into an LDS hash table
// first (a column that finds a slot within HOT_PROBE probes stays there; the others go straight to memory) and
// flushes its <= HOT_TABLE distinct columns once at the end.
constexpr int HOT_TABLE = 8192, HOT_PROBE = 4;
constexpr int HOT_THREADS = 512;
template <class P>
__global__ __launch_bounds__(HOT_THREADS) void hot_count_kernel(const P *__restrict__ rp, const P *__restrict__ rp_light,
                                                               const int32_t *__restrict__ ci, int32_t nrows, int64_t row_stride,
                                                               int32_t *__restrict__ cnt, unsigned long long *__restrict__ total)
{
    __shared__ int32_t s_key[HOT_TABLE];
    __shared__ int32_t s_cnt[HOT_TABLE];
    __shared__ int32_t s_start[HOT_THREADS / WAVE][WAVE];
    for (int k = threadIdx.x; k < HOT_TABLE; k += HOT_THREADS) {
        s_key[k] = -1;
        s_cnt[k] = 0;
    }
    __syncthreads();
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    int32_t *starts = s_start[wv];
    const int64_t n_groups = ((int64_t)nrows + WAVE * row_stride - 1) / (WAVE * row_stride);
    unsigned long long n = 0;
    for (int64_t q = (int64_t)blockIdx.x * (HOT_THREADS / WAVE) + wv; q < n_groups; q += (int64_t)gridDim.x * (HOT_THREADS / WAVE)) {
        const int64_t r = q * WAVE * row_stride + lane;
        int64_t s = 0;
        int32_t len = 0;
        if (r < nrows && !(rp_light && rp_light[r + 1] == rp_light[r])) {      // (not a row cut out to the tiers)
            s = rp[r];
            const int64_t l = (int64_t)rp[r + 1] - s;
            len = (int32_t)(l > 128 ? 128 : l);
        }
        const int32_t start = wave_exscan_i32(len, lane);
        const int32_t all = __builtin_amdgcn_readlane(start + len, WAVE - 1);
        __builtin_amdgcn_wave_barrier();             // (the group before has read its starts)
        starts[lane] = start;
        __builtin_amdgcn_wave_barrier();
        for (int32_t d0 = 0; d0 < all; d0 += WAVE) {
            const int32_t d = d0 + lane;
            const bool in = d < all;
            int p = 0;                               // the last row that starts at or before d (the one with entries there)
#pragma unroll
            for (int step = WAVE / 2; step; step >>= 1)
                if (in && starts[p + step] <= d) p += step;
            const int64_t k = __shfl(s, p, WAVE) + (d - __shfl(start, p, WAVE));
            if (!in) continue;
            const int32_t c = ci[k];
            uint32_t slot = ((uint32_t)c * 2654435761u) >> 19;      // 13 bits
            bool done = false;
#pragma unroll
            for (int pr = 0; pr < HOT_PROBE && !done; pr++) {
                const int32_t old = atomicCAS(&s_key[slot], -1, c);
                if (old == -1 || old == c) {
                    atomicAdd(&s_cnt[slot], 1);
                    done = true;
                }
                slot = (slot + 1) & (HOT_TABLE - 1);
            }
            if (!done) atomicAdd(&cnt[c], 1);
        }
        if (lane == 0) n += (unsigned long long)all;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < HOT_TABLE; k += HOT_THREADS)
        if (s_key[k] >= 0) atomicAdd(&cnt[s_key[k]], s_cnt[k]);
    for (int off = WAVE / 2; off; off >>= 1) n += __shfl_down(n, off, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0 && n) atomicAdd(total, n);
}

// out[0] = #columns with count >= thr, out[1] = sum of their counts
__global__ __launch_bounds__(256) void hot_census_kernel(const int32_t *__restrict__ cnt, int32_t ncols, int32_t thr,
                                                        unsigned long long *__restrict__ out)
{
    unsigned long long n = 0, sum = 0;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < ncols; c += (int64_t)gridDim.x * 256) {
        const int32_t v = cnt[c];
        if (v >= thr) {
            n++;
            sum += (unsigned long long)v;
        }
    }
    for (int off = WAVE / 2; off; off >>= 1) {
        n += __shfl_down(n, off, WAVE);
        sum += __shfl_down(sum, off, WAVE);
    }
    if ((threadIdx.x & (WAVE - 1)) == 0 && n) {
        atomicAdd(&out[0], n);
        atomicAdd(&out[1], sum);
    }
}

// The whole census in one pass: hist[v] = {#columns with count == v, sum of their counts} for v < HOT_HIST (counts at or
// above it share the last bin), so that the host finds the threshold for any slot budget from ONE copy instead of a
// binary search of ~27 launches and round trips (2.5 ms of the headline matrix's plan).  Small counts -- nearly all
// columns -- go through an LDS histogram.
constexpr int HOT_HIST = 65536, HOT_HIST_LDS = 2048;
__global__ __launch_bounds__(256) void hot_hist_kernel(const int32_t *__restrict__ cnt, int32_t ncols,
                                                      unsigned long long *__restrict__ hist_n,
                                                      unsigned long long *__restrict__ hist_sum)
{
    __shared__ unsigned int s_n[HOT_HIST_LDS];
    for (int k = threadIdx.x; k < HOT_HIST_LDS; k += 256) s_n[k] = 0u;
    __syncthreads();
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < ncols; c += (int64_t)gridDim.x * 256) {
        const int32_t v = cnt[c];
        if (v < HOT_HIST_LDS) {
            atomicAdd(&s_n[v], 1u);
        } else {
            const int b = v < HOT_HIST ? v : HOT_HIST;
            atomicAdd(&hist_n[b], 1ull);
            atomicAdd(&hist_sum[b], (unsigned long long)v);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < HOT_HIST_LDS; k += 256)
        if (s_n[k]) {
            atomicAdd(&hist_n[k], (unsigned long long)s_n[k]);
            atomicAdd(&hist_sum[k], (unsigned long long)s_n[k] * (unsigned long long)k);
        }
}

__global__ void hot_flag_kernel(const int32_t *__restrict__ cnt, int32_t ncols, int32_t thr, int32_t *__restrict__ flag)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c <= ncols) flag[c] = (c < ncols && cnt[c] >= thr) ? 1 : 0;
}

// pos[c] = exclusive scan of the flags: the packed columns in column order, with their counts
__global__ void hot_list_kernel(const int32_t *__restrict__ cnt, const int32_t *__restrict__ pos, int32_t ncols,
                                int32_t thr, int32_t *__restrict__ hot_cols, int32_t *__restrict__ hot_cnt)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < ncols && cnt[c] >= thr) {
        hot_cols[pos[c]] = (int32_t)c;
        hot_cnt[pos[c]] = cnt[c];
    }
}

// The packed columns in order of popularity: a stable LSD radix sort of (count, column) by count DESCENDING (digits of the
// complemented count), 8 bits a pass, one wavefront per chunk of 1024 -- digit counts per chunk, one scan over
// (digit, chunk), then the chunk places its elements in order (rank among the lanes of the same digit by ballots).  (On the
// host -- two 16-bit passes plus the copies both ways -- this was 1.5 ms of the headline matrix's plan.)
constexpr int HS_CHUNK = 1024;
__global__ __launch_bounds__(WAVE) void hot_sort_count_kernel(const uint32_t *__restrict__ key, int32_t n, int shift, int32_t nchunk,
                                                             int32_t *__restrict__ cnt)
{
    __shared__ int32_t h[256];
    const int lane = threadIdx.x;
    for (int d = lane; d < 256; d += WAVE) h[d] = 0;
    __syncthreads();
    for (int r = 0; r < HS_CHUNK / WAVE; r++) {
        const int64_t i = (int64_t)blockIdx.x * HS_CHUNK + r * WAVE + lane;
        if (i < n) atomicAdd(&h[(~key[i] >> shift) & 255u], 1);
    }
    __syncthreads();
    for (int d = lane; d < 256; d += WAVE) cnt[(int64_t)d * nchunk + blockIdx.x] = h[d];
}
__global__ __launch_bounds__(WAVE) void hot_sort_place_kernel(const uint32_t *__restrict__ key, const int32_t *__restrict__ val, int32_t n,
                                                             int shift, int32_t nchunk, const int32_t *__restrict__ base,
                                                             uint32_t *__restrict__ key_out, int32_t *__restrict__ val_out)
{
    __shared__ int32_t b[256];
    const int lane = threadIdx.x;
    const unsigned long long below = lane ? (~0ull >> (WAVE - lane)) : 0ull;
    for (int d = lane; d < 256; d += WAVE) b[d] = base[(int64_t)d * nchunk + blockIdx.x];
    __syncthreads();
    for (int r = 0; r < HS_CHUNK / WAVE; r++) {
        const int64_t i = (int64_t)blockIdx.x * HS_CHUNK + r * WAVE + lane;
        const bool ok = i < n;
        const uint32_t k = ok ? key[i] : 0u;
        const uint32_t d = (~k >> shift) & 255u;
        unsigned long long same = __ballot(ok);      // the lanes that hold the same digit
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            const unsigned long long bb = __ballot((d >> bit) & 1u);
            same &= ((d >> bit) & 1u) ? bb : ~bb;
        }
        const int rank = __popcll(same & below), group = __popcll(same);
        if (ok) {
            const int32_t pos = b[d] + rank;
            key_out[pos] = k;
            val_out[pos] = val[i];
        }
        __syncthreads();
        if (ok && rank == group - 1) b[d] += group;
        __syncthreads();
    }
}

// slot[hot_cols[k]] = k (hot_cols in its final, popularity order)
__global__ void hot_slot_kernel(const int32_t *__restrict__ hot_cols, int32_t n_hot, int32_t *__restrict__ slot)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_hot) slot[hot_cols[k]] = k;
}

constexpr int HEAVY_MIN_DEFAULT = 2048;      // tier 0 threshold (CSRK_HEAVY_MIN; the split may lower it per matrix: build_heavy_split)
// (tier 1's threshold: TIERB_MIN_DEFAULT, CSRK_TIERB_MIN; 0 disables tier 1)

template <class P>
__global__ void heavy_flag_kernel(const P *__restrict__ rp, int32_t nrows, int32_t *__restrict__ flag,
                                  int64_t *__restrict__ hlen, int cut_min)
{
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > nrows) return;
    int64_t len = r < nrows ? (int64_t)rp[r + 1] - (int64_t)rp[r] : 0;
    bool h = len >= cut_min;
    flag[r] = h ? 1 : 0;
    hlen[r] = h ? len : 0;
}

template <class P>
__global__ void heavy_view_kernel(const P *__restrict__ rp, int32_t nrows, const int32_t *__restrict__ hidx,
                                  const int64_t *__restrict__ hbefore, P *__restrict__ rp_light,
                                  int32_t *__restrict__ heavy_row, int64_t *__restrict__ cut_pos,
                                  int64_t *__restrict__ cut_cum, int64_t *__restrict__ cut_len, int32_t n_heavy)
{
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > nrows) return;
    const int64_t light = (int64_t)rp[r] - hbefore[r];
    rp_light[r] = (P)light;
    if (r < nrows && hidx[r + 1] != hidx[r]) {     // row r is cut out
        const int32_t c = hidx[r];
        heavy_row[c] = (int32_t)r;
        cut_pos[c] = light;
        cut_cum[c] = hbefore[r];
        cut_len[c] = (int64_t)rp[r + 1] - (int64_t)rp[r];
    }
    if (r == nrows) cut_cum[n_heavy] = hbefore[nrows];
}

template <class P>
__global__ void heavy_sorted_kernel(const P *__restrict__ rp, const int32_t *__restrict__ ci,
                                    const int32_t *__restrict__ heavy_row, int32_t n_heavy, int32_t *__restrict__ bad)
{
    const int c = blockIdx.x;
    if (c >= n_heavy) return;
    const int32_t r = heavy_row[c];
    const int64_t s = rp[r], e = rp[r + 1];
    // (a 10^6-entry row is one workgroup's: 1024 threads with four comparisons in flight each; 256 threads one at a time
    // made this check 1.8 ms of the headline matrix's plan; the rows cut into pieces over a second grid dimension: 2.8 ms
    // -- a million workgroups that mostly have nothing to do)
    bool b = false;
    const int64_t step = (int64_t)blockDim.x * 4;
    for (int64_t k0 = s + threadIdx.x; k0 + 1 < e; k0 += step) {
        int32_t a[4], n[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t k = k0 + (int64_t)u * blockDim.x;
            const bool in = k + 1 < e;
            a[u] = in ? ci[k] : 0;
            n[u] = in ? ci[k + 1] : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) b |= a[u] > n[u];
    }
    if (b) atomicOr(bad, 1);
}

__device__ __forceinline__ int64_t lower_bound_col(const int32_t *__restrict__ ci, int64_t lo, int64_t hi, int64_t col)
{
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if ((int64_t)ci[mid] < col)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// cuts at or before each tile start: tile_cut[t] = #{c : cut_pos[c] <= j0(t)}
__global__ void heavy_tilecut_kernel(const int32_t *__restrict__ tile_row, int64_t n_tiles, int items, int64_t total,
                                     const int64_t *__restrict__ cut_pos, int32_t n_heavy, int32_t *__restrict__ tile_cut)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_tiles) return;
    int64_t d = t * items;
    if (d > total) d = total;
    const int64_t j0 = d - tile_row[t];
    int32_t lo = 0, hi = n_heavy;
    while (lo < hi) {
        int32_t mid = (lo + hi) >> 1;
        if (cut_pos[mid] <= j0)
            lo = mid + 1;
        else
            hi = mid;
    }
    tile_cut[t] = lo;
}

// XCD-aware walk over (column block, row chunk): workgroup g of a grid of xcd_block_chunk_grid() works on block b and
// chunk q, and the workgroups one XCD receives (g % 8) are ITS chunks (q % 8 == g % 8), block after block.  A row's entries
// in consecutive column blocks are neighbours in memory (a few entries each): walked this way the lines that hold them are
// fetched into one L2 once instead of once per block by whichever XCD the flat index fell on (tier 1's count + fill: 1.8 ->
// 1.1 ms of the headline matrix's plan; tier 0's acc_fill_kernel, a wavefront per 64 pairs, did not gain: 2.6 -> 3.0 ms).
__device__ __forceinline__ bool xcd_block_chunk(int64_t g, int32_t chunks, int32_t n_blocks, int32_t &b, int32_t &q)
{
    const int32_t per = (chunks + 7) / 8;
    const int64_t idx = g / 8;
    b = (int32_t)(idx / per);
    q = (int32_t)(g % 8) + 8 * (int32_t)(idx % per);
    return b < n_blocks && q < chunks;
}
static inline int64_t xcd_block_chunk_grid(int64_t chunks, int64_t n_blocks) { return 8 * ceil_div(chunks, 8) * n_blocks; }

template <class P>
__global__ void panel_count_kernel(const P *__restrict__ rp, const int32_t *__restrict__ ci,
                                   const int32_t *__restrict__ heavy_row, int32_t n_heavy, int32_t n_blocks,
                                   int32_t cb, int64_t *__restrict__ cnt)
{
    int32_t b, q;
    if (!xcd_block_chunk(blockIdx.x, (n_heavy + (int)blockDim.x - 1) / (int)blockDim.x, n_blocks, b, q)) return;
    const int32_t c = q * (int)blockDim.x + (int)threadIdx.x;
    if (c >= n_heavy) return;
    const int64_t i = (int64_t)b * n_heavy + c;      // index = b * H + c
    const int32_t r = heavy_row[c];
    const int64_t s = rp[r], e = rp[r + 1];
    const int64_t lo = lower_bound_col(ci, s, e, (int64_t)b * cb);
    const int64_t hi = lower_bound_col(ci, lo, e, (int64_t)(b + 1) * cb);
    cnt[i] = hi - lo;
}

template <class P, int VT, class PP>
__global__ void panel_fill_kernel(const P *__restrict__ rp, const int32_t *__restrict__ ci, const void *__restrict__ vs,
                                  const int32_t *__restrict__ heavy_row, int32_t n_heavy, int32_t n_blocks,
                                  int32_t cb, const int64_t *__restrict__ off, PP *__restrict__ prp,
                                  int32_t *__restrict__ pci, double *__restrict__ pvs)
{
    int32_t b, q;
    if (!xcd_block_chunk(blockIdx.x, (n_heavy + (int)blockDim.x - 1) / (int)blockDim.x, n_blocks, b, q)) return;
    const int32_t c = q * (int)blockDim.x + (int)threadIdx.x;
    if (c >= n_heavy) return;
    const int64_t i = (int64_t)b * n_heavy + c, pairs = (int64_t)n_heavy * n_blocks;
    prp[i] = (PP)off[i];
    if (i == pairs - 1) prp[pairs] = (PP)off[pairs];
    const int32_t r = heavy_row[c];
    const int64_t s = rp[r], e = rp[r + 1];
    const int64_t lo = lower_bound_col(ci, s, e, (int64_t)b * cb);
    const int64_t n = off[i + 1] - off[i];
    int64_t o = off[i];
    for (int64_t k = lo; k < lo + n; k++, o++) {
        pci[o] = ci[k];
        pvs[o] = csr_val<VT>(vs, k);
    }
}

// one thread per tile: merge-path coordinates inside the tile's block
template <class PP>
__global__ void panel_plan_kernel(const PP *__restrict__ prp, int32_t n_heavy, int32_t n_blocks,
                                  const int64_t *__restrict__ blk_tile0, int64_t n_tiles, int items,
                                  PanelTile *__restrict__ tiles)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    int32_t lo = 0, hi = n_blocks;                 // block with blk_tile0[b] <= t < blk_tile0[b+1]
    while (hi - lo > 1) {
        int32_t mid = (lo + hi) >> 1;
        if (blk_tile0[mid] <= t)
            lo = mid;
        else
            hi = mid;
    }
    const int32_t b = lo;
    const int64_t r0 = (int64_t)b * n_heavy;                    // first row of the block in M'
    const int64_t e0 = (int64_t)prp[r0], e1 = (int64_t)prp[r0 + n_heavy];
    const int64_t total = (int64_t)n_heavy + (e1 - e0);
    const int64_t lt = t - blk_tile0[b];
    int64_t coord[2];
    for (int q = 0; q < 2; q++) {
        int64_t d = (lt + q) * items;
        if (d > total) d = total;
        int64_t a = d - (e1 - e0) > 0 ? d - (e1 - e0) : 0, z = d < n_heavy ? d : n_heavy;
        while (a < z) {
            int64_t mid = (a + z) >> 1;
            if ((int64_t)prp[r0 + mid + 1] - e0 <= d - mid - 1)
                a = mid + 1;
            else
                z = mid;
        }
        coord[q] = a;                                           // rows of the block consumed before d
    }
    int64_t d0 = lt * items, d1 = (lt + 1) * items;
    if (d0 > total) d0 = total;
    if (d1 > total) d1 = total;
    PanelTile pt;
    pt.i0 = (int32_t)(r0 + coord[0]);
    pt.i1 = (int32_t)(r0 + coord[1]);
    pt.j0 = e0 + (d0 - coord[0]);
    pt.nn = (int32_t)((d1 - coord[1]) - (d0 - coord[0]));
    pt.blk = b;
    pt.cslot = -1;
    tiles[t] = pt;
}

// Column order inside a tile (tier 1).  A tile of M' holds ~250 (block, row) pairs of ~7 entries each; in row-major order
// the repeats of a popular column are hundreds of gathers apart and L1 has dropped the line by then (0.83 line fills per
// entry).  The tile's entries are therefore STORED sorted by column: the index word becomes {column - block start : 21
// bits | position of the entry in the tile's row-major order : 11 bits}, the kernel gathers x[block start + column] with
// neighbouring lanes on neighbouring (often the same) columns and puts each product back at its row-major position in
// LDS, so the row sums see the very same addends in the very same order.  Inside a whole chunk of 128 ranks the even
// slots hold ranks 0..63 and the odd slots ranks 64..127: a lane loads the pair (2q, 2q + 1), so each of its two gather
// instructions then covers 64 CONSECUTIVE ranks.  One workgroup per tile: bitonic sort of the 2048 words in LDS.
__global__ __launch_bounds__(256) void panel_colsort_kernel(const PanelTile *__restrict__ tiles, int32_t cb,
                                                           int32_t *__restrict__ pci, double *__restrict__ pvs)
{
    __shared__ uint32_t s_key[MERGE_ITEMS];
    __shared__ double s_val[MERGE_ITEMS];
    const PanelTile pt = tiles[blockIdx.x];
    const int nn = pt.nn;
    const int64_t base = (int64_t)pt.blk * cb;
    for (int k = threadIdx.x; k < MERGE_ITEMS; k += 256) {
        uint32_t w = 0xffffffffu;
        if (k < nn) {
            w = ((uint32_t)((int64_t)pci[pt.j0 + k] - base) << PANEL_POS_BITS) | (uint32_t)k;
            s_val[k] = pvs[pt.j0 + k];
        }
        s_key[k] = w;
    }
    __syncthreads();
    for (int size = 2; size <= MERGE_ITEMS; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < MERGE_ITEMS / 2; i += 256) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint32_t a = s_key[lo], b = s_key[hi];
                if ((a > b) == up) {
                    s_key[lo] = b;
                    s_key[hi] = a;
                }
            }
            __syncthreads();
        }
    for (int k = threadIdx.x; k < nn; k += 256) {
        const uint32_t w = s_key[k];
        pci[pt.j0 + panel_slot_of_rank(k, nn)] = (int32_t)w;
        pvs[pt.j0 + panel_slot_of_rank(k, nn)] = s_val[w & ((1u << PANEL_POS_BITS) - 1)];
    }
}

__global__ void panel_blockends_kernel(const int64_t *__restrict__ off, int32_t n_heavy, int32_t n_blocks,
                                       int64_t *__restrict__ out)
{
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b <= n_blocks) out[b] = off[(int64_t)b * n_heavy];
}

// Where each column block starts inside each heavy row, from ONE pass over the rows' (ascending) columns:
// pstart[b * H + c] = entries of heavy row c in blocks < b, for b = 0 .. n_blocks (the last = the row's length).
// One wavefront per 4096-entry piece of a row; an entry whose block differs from its predecessor's opens that
// block and every empty block skipped in between.  (A binary search per (block, row) pair -- 3.7 * 10^7 pairs on
// the headline matrix, twice -- was 14 ms of the plan.)
constexpr int ACC_PIECE = 4096;
template <class P>
__global__ __launch_bounds__(256) void acc_pairstart_kernel(const P *__restrict__ rp, const int32_t *__restrict__ ci,
                                                           const int32_t *__restrict__ heavy_row, int32_t n_heavy,
                                                           int32_t n_blocks, int32_t cb, const int32_t *__restrict__ task_row,
                                                           const int32_t *__restrict__ task_piece, int64_t n_tasks,
                                                           int32_t *__restrict__ pstart)
{
    // (an XCD, blockIdx % 8, takes a contiguous range of the tasks: neighbouring rows share the lines of pstart they write)
    const int64_t wpg = blockDim.x / WAVE, per = ((int64_t)gridDim.x + 7) / 8;
    const int64_t q = (((int64_t)blockIdx.x % 8) * per + (int64_t)blockIdx.x / 8) * wpg + threadIdx.x / WAVE;
    const int lane = threadIdx.x & (WAVE - 1);
    if (q >= n_tasks) return;
    const int32_t c = task_row[q];
    const int64_t s = rp[heavy_row[c]], e = rp[heavy_row[c] + 1];
    const int64_t k0 = s + (int64_t)task_piece[q] * ACC_PIECE;
    const int64_t k1 = k0 + ACC_PIECE < e ? k0 + ACC_PIECE : e;
    for (int64_t k = k0 + lane; k < k1; k += WAVE) {
        const int32_t b = ci[k] / cb;
        const int32_t bp = k > s ? ci[k - 1] / cb : -1;
        for (int32_t bb = bp + 1; bb <= b; bb++) pstart[(int64_t)bb * n_heavy + c] = (int32_t)(k - s);
        if (k == e - 1)
            for (int32_t bb = b + 1; bb <= n_blocks; bb++) pstart[(int64_t)bb * n_heavy + c] = (int32_t)(e - s);
    }
}

__global__ void acc_paircount_kernel(const int32_t *__restrict__ pstart, int64_t pairs, int32_t n_heavy,
                                     int64_t *__restrict__ cnt)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < pairs) cnt[i] = (int64_t)pstart[i + n_heavy] - (int64_t)pstart[i];
}

// One wavefront per column block: gap[b * H + c] = distance from heavy row c to the previous heavy row with entries in
// block b (0 for the block's first one and for absent pairs), and the padding entries a gap over ACC_MAXSTEP needs
// are added to the pair's count.
__global__ __launch_bounds__(256) void acc_gap_kernel(int64_t *__restrict__ cnt, int32_t n_heavy, int32_t n_blocks,
                                                     int32_t *__restrict__ gap)
{
    const int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const int lane = threadIdx.x & (WAVE - 1);
    if (b >= n_blocks) return;
    int32_t last = -1;
    for (int32_t c0 = 0; c0 < n_heavy; c0 += WAVE) {
        const int32_t c = c0 + lane;
        const bool present = c < n_heavy && cnt[b * n_heavy + c] > 0;
        const unsigned long long mask = __ballot(present);
        const unsigned long long below = lane ? (mask & (~0ull >> (WAVE - lane))) : 0ull;
        const int32_t prev = below ? c0 + 63 - __clzll((long long)below) : last;
        if (c < n_heavy) {
            const int32_t g = present && prev >= 0 ? c - prev : 0;
            gap[b * n_heavy + c] = g;
            if (g > ACC_MAXSTEP) cnt[b * n_heavy + c] += (g - 1) / ACC_MAXSTEP;
        }
        if (mask) last = c0 + 63 - __clzll((long long)mask);
    }
}

// Where logical tile t is stored.  Workgroup w owns the logical tiles [wg_t0[w], wg_t0[w + 1]); its k-th tile is stored
// at k * n_wg + w, i.e. the workgroups' streams are interleaved tile by tile: the persistent workgroups advance at
// about the same pace, so at any moment they read one contiguous ~1 MB window of the array, spread over all HBM
// channels.  (Contiguous per-workgroup ranges put 256 concurrent streams at a fixed stride: when that stride
// resonates with the channel interleave the kernel loses up to 38 % -- 0.129 -> 0.177 ms measured on a 2-way partition's
// shard at 580 tiles per workgroup, 0.218 -> 0.224 on the headline matrix; any other workgroup count restored the rate.)
__device__ __forceinline__ int64_t acc_phys_tile(int64_t t, const int64_t *__restrict__ wg_t0, int32_t n_wg)
{
    // the workgroup with wg_t0[w] <= t < wg_t0[w + 1], wg_t0[w] = floor(n_tiles w / n_wg) (build_acc_panel): w is
    // floor(t n_wg / n_tiles) or a neighbour -- an estimate and two looks at the table instead of a bisection per entry
    // (eight dependent loads each, for every entry of tier 0)
    const int64_t n_tiles = wg_t0[n_wg];
    int64_t w = (int64_t)((double)t * (double)n_wg / (double)(n_tiles > 0 ? n_tiles : 1));      // (an estimate: the table decides)
    w = w > n_wg - 1 ? n_wg - 1 : (w < 0 ? 0 : w);
    while (w > 0 && wg_t0[w] > t) w--;
    while (w + 1 < n_wg && wg_t0[w + 1] <= t) w++;
    return (t - wg_t0[w]) * n_wg + w;
}

// The grid test of a group's values (fix56.h): bad flag, lowest and highest set bit over the entries of the listed rows, into
// out[0..2] (preset to 0, INT32_MAX, INT32_MIN).  blockIdx.x = the row, whose entries gridDim.y workgroups share.
template <class P>
__global__ __launch_bounds__(256) void acc_range_kernel(const P *__restrict__ rp, const double *__restrict__ vs,
                                                       const int32_t *__restrict__ rows, int32_t *__restrict__ out)
{
    const int32_t row = rows[blockIdx.x];
    const int64_t k1 = (int64_t)rp[row + 1];
    fix56::Range r;
    for (int64_t k = (int64_t)rp[row] + blockIdx.y * 256 + threadIdx.x; k < k1; k += (int64_t)gridDim.y * 256) fix56::fold(r, vs[k]);
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        fix56::Range o;
        o.bad = __shfl_xor(r.bad, off, WAVE);
        o.lo = __shfl_xor(r.lo, off, WAVE);
        o.hi = __shfl_xor(r.hi, off, WAVE);
        fix56::merge(r, o);
    }
    // a wavefront's atomics only where they would change the result so far (a stale look costs an atomic, never the result):
    // unconditional, the headline matrix's 250 k wavefronts queued 19 ms on these three words
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        const volatile int32_t *seen = out;
        if (r.bad && !seen[0]) atomicOr(out, 1);
        if (r.lo < seen[1]) atomicMin(out + 1, r.lo);
        if (r.hi > seen[2]) atomicMax(out + 2, r.hi);
    }
}

// One entry of tier 0's stream -- value v, column `col` inside the block (ACC_CB: a padding entry, v = 0.0), row step -- stored
// by the fill kernels; or, VERIFY (packed tiles only), read back from the finished tile by the routine the product kernel uses
// (AccVals: the loads of lane el / 8, its decode) and compared with the source bit for bit.
// The 8.5-byte form (fix56.h, nib) keeps the sign in the index word and eight nibbles of neighbouring entries in one dword:
// the nibble is or-ed in atomically (the tiles are zeroed first), and VERIFY also compares the column and the step the
// kernel would see; a padding entry must come back as -0.0 on column ACC_CB.
template <class SV, bool VERIFY>
__device__ __forceinline__ void acc_put(SV *__restrict__ pvals, uint16_t *__restrict__ pidx, int64_t pt, int el, double v,
                                        uint32_t col, uint32_t step, int32_t fx_g, int32_t *__restrict__ mismatch)
{
    if constexpr (std::is_same<SV, fix56::nib::Bytes>::value) {
        namespace nib = fix56::nib;
        unsigned char *tile = (unsigned char *)acc_tile_at(pvals, pt);
        const bool pad = col == (uint32_t)ACC_CB;
        if constexpr (!VERIFY) {
            const uint64_t p = pad ? nib::PAD_CODE : fix56::encode(v, fx_g);
            ((uint32_t *)tile)[fix56::lo_slot(el)] = fix56::lo_of(p);
            ((uint16_t *)(tile + nib::MID_OFF))[el] = fix56::mid_of(p);
            if (nib::hi_of(p)) atomicOr((uint32_t *)(tile + nib::HI_OFF) + nib::hi_word(el), nib::hi_of(p) << nib::hi_shift(el));
            pidx[pt * ACC_TILE + el] = nib::index_word(p, col, step);
        } else {
            AccVals<SV> t;
            t.load((const SV *)tile, el >> 3);
            const u32x4_t ix = *((const u32x4_t *)(pidx + pt * ACC_TILE) + (el >> 3));
            uint32_t e[ACC_K] = {ix.x & 0xffffu, ix.x >> 16, ix.y & 0xffffu, ix.y >> 16,
                                 ix.z & 0xffffu, ix.z >> 16, ix.w & 0xffffu, ix.w >> 16};
            double a[ACC_K];
            t.get(a, fx_g, e);
            double d = a[0];
            uint32_t w = e[0];
#pragma unroll
            for (int j = 1; j < ACC_K; j++) {
                d = (el & 7) == j ? a[j] : d;
                w = (el & 7) == j ? e[j] : w;
            }
            if (fix56::bits_of(d) != (pad ? 1ull << 63 : fix56::bits_of(v)) || w != (col | step << ACC_ROW_SHIFT)) *mismatch = 1;
        }
    } else if constexpr (!std::is_same<SV, fix56::Packed>::value) {
        pvals[pt * ACC_TILE + acc_slot_of<SV>(el)] = (SV)v;
        pidx[pt * ACC_TILE + el] = (uint16_t)(col | step << ACC_ROW_SHIFT);
    } else if constexpr (!VERIFY) {
        fix56::put((unsigned char *)(pvals + pt * ACC_TILE), el, fix56::encode(v, fx_g));
        pidx[pt * ACC_TILE + el] = (uint16_t)(col | step << ACC_ROW_SHIFT);
    } else {
        AccVals<SV> t;
        t.load(pvals + pt * ACC_TILE, el >> 3);
        double a[ACC_K];
        t.get(a, fx_g);
        double d = a[0];
#pragma unroll
        for (int j = 1; j < ACC_K; j++) d = (el & 7) == j ? a[j] : d;
        if (fix56::bits_of(d) != fix56::bits_of(v)) *mismatch = 1;
    }
}

// One wavefront per 64 consecutive (block, heavy row) pairs of ONE block: their slots are one contiguous range of the
// block's logical stream, walked 64 slots at a time -- a slot finds its pair by bisection in the wavefront's own table of
// pair starts, a padding slot (the first ones of a pair whose row lies more than ACC_MAXSTEP rows after the previous one)
// writes (0.0, zero slot, step 7), the others copy the pair's entries -- so the stream is written by consecutive lanes and
// every lane works.  (A thread per pair walking its 3.6 entries one after the other wrote and read 64 scattered lines
// per instruction: 6.9 ms of the headline matrix's plan, its largest item; this form 2.7.)
// VERIFY: the same walk writes nothing and checks the values of a finished fix56 stream instead (acc_put).
template <class P, int VT, class SV, bool VERIFY = false>
__global__ __launch_bounds__(256) void acc_fill_kernel(const P *__restrict__ rp, const int32_t *__restrict__ ci,
                                                      const void *__restrict__ vs, const int32_t *__restrict__ heavy_row,
                                                      int32_t n_heavy, int32_t n_blocks, int32_t cb,
                                                      const int64_t *__restrict__ off, const int64_t *__restrict__ blk_tile0,
                                                      const int32_t *__restrict__ pstart, const int32_t *__restrict__ gap,
                                                      SV *__restrict__ pvals, uint16_t *__restrict__ pidx,
                                                      int32_t *__restrict__ tile_row0, const int64_t *__restrict__ wg_t0,
                                                      int32_t n_wg, int32_t waves_per_block, int32_t fx_g,
                                                      int32_t *__restrict__ mismatch)
{
    __shared__ int32_t s_start[256 / WAVE][WAVE];
    const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    const int32_t b = (int32_t)(w / waves_per_block);
    if (b >= n_blocks) return;
    const int32_t c0 = (int32_t)(w % waves_per_block) * WAVE, c = c0 + lane;
    const bool valid = c < n_heavy;
    const int64_t i = (int64_t)b * n_heavy + (valid ? c : c0);
    const int64_t off_i = off[i];
    int32_t n_all = 0, g = 0;
    int64_t lo = 0;
    if (valid) {
        n_all = (int32_t)(off[i + 1] - off_i);
        g = gap[i];
        lo = (int64_t)rp[heavy_row[c]] + pstart[i];
    }
    const int32_t npad = g > ACC_MAXSTEP ? (g - 1) / ACC_MAXSTEP : 0;
    const int32_t start = wave_exscan_i32(n_all, lane);
    const int32_t total = __builtin_amdgcn_readlane(start + n_all, WAVE - 1);
    if (total == 0) return;
    // logical position of the wavefront's first slot (lane 0's pair: c0 < n_heavy)
    const int64_t L0 = blk_tile0[b] * ACC_TILE + (__shfl(off_i, 0, WAVE) - off[(int64_t)b * n_heavy]);
    int32_t *starts = s_start[wv];
    starts[lane] = start;
    __builtin_amdgcn_wave_barrier();
    for (int32_t d0 = 0; d0 < total; d0 += WAVE) {
        const int32_t d = d0 + lane;
        const bool in = d < total;
        int p = 0;                                   // the last pair that starts at or before slot d (an empty pair shares its
#pragma unroll                                       // start with the next one: the last of them is the one with entries)
        for (int step = WAVE / 2; step; step >>= 1)
            if (in && starts[p + step] <= d) p += step;
        const int32_t at = d - __shfl(start, p, WAVE);      // slot inside the pair
        const int32_t npad_p = __shfl(npad, p, WAVE), g_p = __shfl(g, p, WAVE);
        const int64_t lo_p = __shfl(lo, p, WAVE);
        if (!in) continue;
        const int64_t L = L0 + d;
        const int64_t t = L / ACC_TILE;
        const int el = (int)(L % ACC_TILE);
        const int64_t pt = acc_phys_tile(t, wg_t0, n_wg);
        if (at < npad_p) {                           // padding entry k = at + 1 stands on heavy row c - g + 7k
            acc_put<SV, VERIFY>(pvals, pidx, pt, el, 0.0, (uint32_t)cb, el ? (uint32_t)ACC_MAXSTEP : 0u, fx_g, mismatch);
            if (VERIFY) continue;
            if (el == 0) tile_row0[t] = c0 + p - g_p + ACC_MAXSTEP * (at + 1);
        } else {
            const int64_t k = lo_p + (at - npad_p);
            // the pair's first entry: the step from the previous row (or the last padding entry) to this row
            const uint32_t step_in = at == npad_p ? (uint32_t)(g_p - ACC_MAXSTEP * npad_p) : 0u;
            acc_put<SV, VERIFY>(pvals, pidx, pt, el, csr_val<VT>(vs, k), (uint32_t)(ci[k] - b * cb), el ? step_in : 0u, fx_g,
                                mismatch);
            if (VERIFY) continue;
            if (el == 0) tile_row0[t] = c0 + p;
        }
    }
}

// one workgroup per block: pads the block's last tile with (0.0, column slot ACC_CB (a zero in LDS), step 0 = the
// block's last heavy row) -- a padding entry adds 0.0 * 0.0 to an accumulator
template <class SV, bool VERIFY = false>
__global__ __launch_bounds__(256) void acc_pad_kernel(const int64_t *__restrict__ off, int32_t n_heavy, int32_t n_blocks,
                                                     const int64_t *__restrict__ blk_tile0, SV *__restrict__ pvals,
                                                     uint16_t *__restrict__ pidx, const int64_t *__restrict__ wg_t0, int32_t n_wg,
                                                     int32_t fx_g, int32_t *__restrict__ mismatch)
{
    const int32_t b = blockIdx.x;
    if (b >= n_blocks) return;
    const int64_t cnt = off[(int64_t)(b + 1) * n_heavy] - off[(int64_t)b * n_heavy];
    const int64_t L0 = blk_tile0[b] * ACC_TILE + cnt, L1 = blk_tile0[b + 1] * ACC_TILE;
    for (int64_t L = L0 + threadIdx.x; L < L1; L += blockDim.x) {      // (the tail of the block's last tile: one tile)
        const int64_t pt = acc_phys_tile(L / ACC_TILE, wg_t0, n_wg);
        const int el = (int)(L % ACC_TILE);
        acc_put<SV, VERIFY>(pvals, pidx, pt, el, 0.0, (uint32_t)ACC_CB, 0u, fx_g, mismatch);
    }
}

// (wave_exscan_i32 / wave_segscan: wave.h)

// smallest r in [0, nrows) with rpv[r + 1] > L (the row holding view entry L); L < rpv[nrows]
template <class P>
__device__ __forceinline__ int32_t ls_row_of(const P *__restrict__ rpv, int32_t nrows, int64_t L)
{
    int32_t lo = 0, hi = nrows - 1;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)rpv[mid + 1] > L)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// tile_row[t] = the row that holds a tile's first entry, tile_row[n_tiles] = the last row: the fill kernel then looks for an
// entry's row between its tile's bounds (9 steps over neighbouring pointers instead of 23 over the whole array: 1.07 ms of
// the headline matrix's plan)
template <class P>
__global__ void ls_tilerow_kernel(const P *__restrict__ rpv, int32_t nrows, int64_t n_ent, int64_t n_tiles, int32_t *__restrict__ tile_row)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_tiles) return;
    const int64_t e0 = t * ACC_TILE;
    tile_row[t] = t < n_tiles && e0 < n_ent ? ls_row_of(rpv, nrows, e0) : nrows - 1;
}

template <class P>
__global__ void ls_rowflag_kernel(const P *__restrict__ rpv, int32_t nrows, int32_t *__restrict__ flag)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= nrows) flag[r] = (r < nrows && rpv[r + 1] > rpv[r]) ? 1 : 0;
}

// dense rows: rpd[r] = rpv[r] + (empty rows before r) -- every empty row of the view gets one slot; nz = exclusive scan of
// the non-empty flags (so r - nz[r] = empty rows before r)
template <class P>
__global__ void ls_dense_ptr_kernel(const P *__restrict__ rpv, const int32_t *__restrict__ nz, int32_t nrows, P *__restrict__ rpd)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= nrows) rpd[r] = (P)((int64_t)rpv[r] + (r - (int64_t)nz[r]));
}

template <class P>
__global__ void ls_rowids_kernel(const P *__restrict__ rpv, int32_t nrows, const int32_t *__restrict__ ridx,
                                 int32_t *__restrict__ rowids)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < nrows && rpv[r + 1] > rpv[r]) rowids[ridx[r]] = (int32_t)r;
}

// One thread per slot of the stream (n_ent entries, then padding to a whole tile): view entry L of view row r is the
// source entry src[r] + (L - rpv[r]) (a view row is a whole row of the source or empty).
template <class P, int VT, class SV>
__global__ __launch_bounds__(256) void ls_fill_kernel(const P *__restrict__ src, const P *__restrict__ rpv, int32_t nrows,
                                                     const int32_t *__restrict__ ci, const void *__restrict__ vs,
                                                     int64_t n_ent, int64_t n_slots, const int32_t *__restrict__ slot_map, SV *__restrict__ svals,
                                                     uint32_t *__restrict__ sidx, const P *__restrict__ rp_len,
                                                     const int32_t *__restrict__ tile_row)
{
    // rp_len (dense rows): the view's own row pointers; rpv then gives every row at least one slot, and a row that is
    // empty in rp_len becomes one padding entry that opens (and is) its run
    const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_slots) return;
    const int64_t t = slot / ACC_TILE;
    const int el = (int)(slot % ACC_TILE);
    const int64_t L = slot;
    double v = 0.0;
    uint32_t ix = LS_PAD;
    if (L < n_ent) {
        int32_t lo = tile_row[t], hi = tile_row[t + 1];      // ls_row_of between the tile's bounds
        while (lo < hi) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if ((int64_t)rpv[mid + 1] > L)
                hi = mid;
            else
                lo = mid + 1;
        }
        const int32_t r = lo;
        const int64_t first = (int64_t)rpv[r];
        if (rp_len && rp_len[r + 1] == rp_len[r]) {
            ix = LS_PAD | LS_START_BIT;
        } else {
            const int64_t a = (int64_t)src[r] + (L - first);
            v = csr_val<VT>(vs, a);
            const int32_t c = ci[a];
            const int32_t sl = slot_map ? slot_map[c] : -1;         // slot of a packed column
            ix = sl >= 0 ? (LS_HOT_BIT | (uint32_t)sl) : (uint32_t)c;
            if (L == first) ix |= LS_START_BIT;
        }
    }
    svals[t * ACC_TILE + acc_slot_of<SV>(el)] = (SV)v;
    sidx[t * ACC_TILE + acc_idx_slot(el)] = ix;
}

// per tile: run numbering base
template <class P>
__global__ void ls_tilebase_kernel(const P *__restrict__ rpv, int32_t nrows, const int32_t *__restrict__ ridx, int64_t n_tiles,
                                   const int32_t *__restrict__ tile_row, int32_t *__restrict__ tile_base)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    const int64_t e0 = t * ACC_TILE;      // (< the entry count: the stream has no empty tile)
    const int32_t r = tile_row[t];
    tile_base[t] = ridx[r] + ((int64_t)rpv[r] == e0 ? 0 : 1);
}

template <class P>
__global__ void vec_count_kernel(const P *__restrict__ rp, int32_t nrows, int64_t *__restrict__ cnt)
{
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    int64_t len = (int64_t)rp[r + 1] - (int64_t)rp[r];
    cnt[r] = len <= VEC_SEG ? 1 : (len + VEC_SEG - 1) / VEC_SEG;
}

__global__ void vec_fill_kernel(const int64_t *__restrict__ seg_off, int32_t nrows, int32_t *__restrict__ seg_row)
{
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    for (int64_t q = seg_off[r]; q < seg_off[r + 1]; q++) seg_row[q] = (int32_t)r;
}

// ---- host side ----------------------------------------------------------------------------------
// The builders are the steps of DESIGN.md section 4, "The plan builder", in its order.  What DECIDES a layout is plain
// arithmetic in spmv_layout.h (checked on the host: tests/spmv_layout_host); here are the launches, the round trips and
// the allocations.  The order in which the steps ask the pool for memory, release it and launch is behaviour (it decides
// pool reuse and plan_bytes): a builder declares its temporaries itself, in the order they are released in reverse, and
// hands them to its steps by reference.  Everything runs on the default stream.
constexpr int HEAVY_STREAMS = 8;   // XCDs: blockIdx % 8 labels the XCD group (speed assumption only)

// The knobs of one plan build (spmv_layout.h: SpmvKnobs, with their parsing rules): read here, once, at the top of
// build_plan, and handed down.  No builder reads the environment.  (spmv.hip's get_plan_locked reads them the same way
// while it decides whether a plan is built with the split.)
SpmvKnobs read_spmv_knobs()
{
    SpmvKnobStrings e;
    e.heavy_split = getenv("CSRK_SPMV_HEAVY_SPLIT");
    e.heavy_min = getenv("CSRK_HEAVY_MIN");
    e.tierb_min = getenv("CSRK_TIERB_MIN");
    e.acc_groups = getenv("CSRK_ACC_GROUPS");
    e.acc_group_rows = getenv("CSRK_ACC_GROUP_ROWS");
    e.nib = getenv("CSRK_SPMV_NIB");
    e.fix56 = getenv("CSRK_SPMV_FIX56");
    e.hot = getenv("CSRK_SPMV_HOT");
    e.ls_stage = getenv("CSRK_LS_STAGE");
    e.stream = getenv("CSRK_SPMV_STREAM");
    e.trace = getenv("CSRK_PLAN_TRACE");
    const SpmvKnobDefaults d = {HEAVY_MIN_DEFAULT, TIERB_MIN_DEFAULT, ACC_GROUPS_DEFAULT, accgroups::MAX_GROUPS, ACC_MAXROWS};
    return parse_spmv_knobs(e, d);
}

// the device's compute units (256 where the runtime does not say)
static int device_cus(const Matrix *m, int *cus)
{
    int n = 0;
    CSRK_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, m->device));
    *cus = n > 0 ? n : 256;
    return CSRK_OK;
}

// Both panels: `off` holds the scanned (block, row) pair counts.  Entries before each block's end -> the host -> tiles before
// each block (spmvlayout::tile_starts: `items` per tile, `extra` items per block), in t0 and, for the kernels, in `bends`.
static int block_tile_starts(const DevBuf &off, int32_t n, int32_t nb, int64_t items, int64_t extra, DevBuf &bends,
                             std::vector<int64_t> &t0, hipStream_t s)
{
    CSRK_TRY(bends.alloc((size_t)(nb + 1) * 8));
    panel_blockends_kernel<<<(unsigned)ceil_div(nb + 1, 256), 256, 0, s>>>(off.as<int64_t>(), n, nb, bends.as<int64_t>());
    CSRK_LAUNCH_CHECK();
    std::vector<int64_t> be((size_t)nb + 1);      // (host: nb is at most a few thousand)
    CSRK_TRY(stage_d2h(be.data(), bends.p, (size_t)(nb + 1) * 8, s));
    CSRK_HIP(hipStreamSynchronize(s));
    t0 = spmvlayout::tile_starts(be.data(), nb, items, extra);
    CSRK_TRY(stage_h2d(bends.p, t0.data(), (size_t)(nb + 1) * 8, s));
    return CSRK_OK;
}

// ---- tier 1 (pair form): build_panel and its steps ------------------------------------------------
// M': the pair counts, their scan, and the column-block-major copy of the listed rows (float64 values)
template <class P, int VT>
static int panel_matrix(Matrix *m, Panel *pn, int32_t n, int32_t nb, int32_t cb, int64_t nnz_rows, DevBuf &off, hipStream_t s)
{
    const P *rp = (const P *)m->d_rowptrs;
    const int64_t pairs = (int64_t)n * nb;
    CSRK_TRY(off.alloc((size_t)(pairs + 1) * 8));
    const unsigned g = (unsigned)xcd_block_chunk_grid(ceil_div(n, 256), nb);
    panel_count_kernel<P><<<g, 256, 0, s>>>(rp, m->d_colinds, pn->row_list.as<int32_t>(), n, nb, cb, off.as<int64_t>());
    CSRK_LAUNCH_CHECK();
    CSRK_TRY(exclusive_scan_i64(off.as<int64_t>(), off.as<int64_t>(), pairs, s));
    pn->p64 = nnz_rows > INT32_MAX;
    CSRK_TRY(pn->rp.alloc((size_t)(pairs + 1) * (pn->p64 ? 8 : 4)));
    CSRK_TRY(pn->ci.alloc((size_t)nnz_rows * 4));
    CSRK_TRY(pn->vs.alloc((size_t)nnz_rows * 8));
    if (pn->p64)
        panel_fill_kernel<P, VT, int64_t><<<g, 256, 0, s>>>(rp, m->d_colinds, m->d_values, pn->row_list.as<int32_t>(), n, nb,
                                                          cb, off.as<int64_t>(), pn->rp.as<int64_t>(),
                                                          pn->ci.as<int32_t>(), pn->vs.as<double>());
    else
        panel_fill_kernel<P, VT, int32_t><<<g, 256, 0, s>>>(rp, m->d_colinds, m->d_values, pn->row_list.as<int32_t>(), n, nb,
                                                          cb, off.as<int64_t>(), pn->rp.as<int32_t>(),
                                                          pn->ci.as<int32_t>(), pn->vs.as<double>());
    CSRK_LAUNCH_CHECK();
    return CSRK_OK;
}

// the tiles' coordinates (bends: tiles before each block), then every tile's entries into column order
static int panel_tiles(Panel *pn, int32_t n, int32_t nb, int32_t cb, const DevBuf &bends, int64_t n_tiles, hipStream_t s)
{
    CSRK_TRY(pn->tile.alloc((size_t)n_tiles * sizeof(PanelTile)));
    if (pn->p64)
        panel_plan_kernel<int64_t><<<(unsigned)ceil_div(n_tiles, 256), 256, 0, s>>>(
            pn->rp.as<int64_t>(), n, nb, bends.as<int64_t>(), n_tiles, MERGE_ITEMS, pn->tile.as<PanelTile>());
    else
        panel_plan_kernel<int32_t><<<(unsigned)ceil_div(n_tiles, 256), 256, 0, s>>>(
            pn->rp.as<int32_t>(), n, nb, bends.as<int64_t>(), n_tiles, MERGE_ITEMS, pn->tile.as<PanelTile>());
    CSRK_LAUNCH_CHECK();
    CSRK_REQUIRE(((int64_t)cb << PANEL_POS_BITS) <= (1ll << 32), "column block too wide for the tile's index word");
    if (n_tiles > 0) {
        panel_colsort_kernel<<<(unsigned)n_tiles, 256, 0, s>>>(pn->tile.as<PanelTile>(), cb, pn->ci.as<int32_t>(), pn->vs.as<double>());
        CSRK_LAUNCH_CHECK();
    }
    return CSRK_OK;
}

// The tiles' carries per long row (spmvlayout::panel_carries; Panel::ncs): the tiles come to the host, get their carry
// slots and go back; the carries beyond the slots are listed in crp / cidx, which exist only then.
static int panel_carry_slots(Panel *pn, int32_t n, int64_t pairs, int64_t n_tiles)
{
    std::vector<PanelTile> ht((size_t)n_tiles);
    CSRK_TRY(stage_d2h(ht.data(), pn->tile.p, (size_t)n_tiles * sizeof(PanelTile), nullptr));
    const spmvlayout::PanelCarries pc = spmvlayout::panel_carries(ht, n, pairs, PANEL_CARRY_ROWS);
    pn->listed = pc.listed;
    pn->ncs = pc.ncs;
    CSRK_TRY(stage_h2d(pn->tile.p, ht.data(), (size_t)n_tiles * sizeof(PanelTile), nullptr));
    if (pc.listed) {
        CSRK_TRY(pn->crp.alloc(pc.crp.size() * 4));
        CSRK_TRY(pn->cidx.alloc(pc.cidx.size() * 4));
        CSRK_TRY(stage_h2d(pn->crp.p, pc.crp.data(), pc.crp.size() * 4, nullptr));
        CSRK_TRY(stage_h2d(pn->cidx.p, pc.cidx.data(), pc.cidx.size() * 4, nullptr));
    }
    return CSRK_OK;
}

// what a product writes: the workgroup list, the tiles' carries, the partials with their pn->ncs carry rows
static int panel_outputs(Panel *pn, const std::vector<PanelGroup> &groups, int32_t n, int64_t pairs, int64_t n_tiles, hipStream_t s)
{
    pn->groups = (int64_t)groups.size();
    CSRK_TRY(pn->group.alloc(groups.size() * sizeof(PanelGroup)));
    CSRK_TRY(stage_h2d(pn->group.p, groups.data(), groups.size() * sizeof(PanelGroup), s));
    CSRK_TRY(pn->carry_row.alloc((size_t)n_tiles * 4));
    CSRK_TRY(pn->carry_val.alloc((size_t)n_tiles * 8));
    CSRK_TRY(pn->y.alloc((size_t)(pairs + (int64_t)pn->ncs * n) * 8));
    if (pn->ncs) {      // -0.0 where no tile writes (x + -0.0 = x for every x)
        std::vector<double> neg0((size_t)pn->ncs * n, -0.0);
        CSRK_TRY(stage_h2d(pn->y.as<double>() + pairs, neg0.data(), neg0.size() * 8, s));
    }
    return CSRK_OK;
}

// Build one panel tier: M' (column-block-major copy of the listed rows, float64 values), its tiles and
// the workgroup list.  `xcd_streams`: order the groups so that column block b is served by workgroups
// with blockIdx % 8 == b % 8.
template <class P, int VT>
static int build_panel(Matrix *m, Panel *pn, const std::vector<int32_t> &rows, int64_t nnz_rows, int32_t cb, int tpw,
                       bool xcd_streams, const SpmvKnobs &knobs, hipStream_t s)
{
    PlanTrace tr(knobs);
    const int32_t n = (int32_t)rows.size();
    const int32_t nb = (int32_t)ceil_div(m->ncols > 0 ? m->ncols : 1, cb);
    const int64_t pairs = (int64_t)n * nb;
    CSRK_TRY(pn->row_list.alloc((size_t)n * 4));
    CSRK_TRY(stage_h2d(pn->row_list.p, rows.data(), (size_t)n * 4, s));
    DevBuf off, bends;
    CSRK_TRY((panel_matrix<P, VT>(m, pn, n, nb, cb, nnz_rows, off, s)));
    std::vector<int64_t> t0;      // tiles before each block: a block's merge path is its entries and n row ends
    CSRK_TRY(block_tile_starts(off, n, nb, MERGE_ITEMS, n, bends, t0, s));
    const int64_t n_tiles = t0[(size_t)nb];
    tr.lap("  tier 1: count, scan, fill");
    CSRK_TRY(panel_tiles(pn, n, nb, cb, bends, n_tiles, s));
    tr.lap("  tier 1: tiles, column order");
    const std::vector<PanelGroup> groups = spmvlayout::panel_groups(t0.data(), nb, tpw, xcd_streams, HEAVY_STREAMS, &pn->pad_groups);
    CSRK_TRY(panel_carry_slots(pn, n, pairs, n_tiles));
    CSRK_TRY(panel_outputs(pn, groups, n, pairs, n_tiles, s));
    CSRK_HIP(hipStreamSynchronize(s));     // `groups`, `t0` are host temporaries of async copies
    tr.lap("  tier 1: groups, carries (host)");
    pn->on = true;
    pn->cb = cb;
    pn->nb = nb;
    pn->nrow = n;
    pn->rows = pairs;
    pn->tiles = n_tiles;
    pn->nnz = nnz_rows;
    return CSRK_OK;
}

// ---- tier 0 (accumulator form): build_acc_panel and its steps -------------------------------------
// form: what packable float64 values are stored as -- ACC_FORM_RAW: the raw stream whatever the values (another group of the
// launch could not be packed), ACC_FORM_FIX56: 9-byte entries, ACC_FORM_NIB: 8.5-byte entries (the launch's choice:
// accgroups::choose_nib).
enum { ACC_FORM_RAW = 0, ACC_FORM_FIX56 = 1, ACC_FORM_NIB = 2 };

// One group's plan-time temporaries, in the order they are released in reverse, and what its steps share.
struct AccBuild {
    DevBuf off, bends, pstart, d_trow, d_tpiece, gap, d_wg_t0;
    DevBuf fx;      // int32[4]: the grid test's bad flag, lowest and highest set bit; the verification's mismatch flag
    int32_t n = 0, nb = 0;
    int64_t pairs = 0, n_tiles = 0;
    std::vector<int64_t> t0;      // tiles before each column block
    spmvlayout::WgShares sh;
};

// block starts inside every row (one pass over the rows' entries, a task per ACC_PIECE entries of a row)
template <class P>
static int acc_pair_starts(Matrix *m, AccPanel *ap, const int64_t *lens, AccBuild &B, hipStream_t s)
{
    CSRK_TRY(B.off.alloc((size_t)(B.pairs + 1) * 8));
    std::vector<int32_t> trow, tpiece;
    spmvlayout::acc_tasks(lens, B.n, ACC_PIECE, trow, tpiece);
    const int64_t n_tasks = (int64_t)trow.size();
    CSRK_TRY(B.pstart.alloc((size_t)(B.pairs + B.n) * 4));
    CSRK_TRY(B.d_trow.alloc((size_t)(n_tasks ? n_tasks : 1) * 4));
    CSRK_TRY(B.d_tpiece.alloc((size_t)(n_tasks ? n_tasks : 1) * 4));
    CSRK_TRY(stage_h2d(B.d_trow.p, trow.data(), (size_t)n_tasks * 4, s));
    CSRK_TRY(stage_h2d(B.d_tpiece.p, tpiece.data(), (size_t)n_tasks * 4, s));
    acc_pairstart_kernel<P><<<(unsigned)(ceil_div(ceil_div(n_tasks * WAVE, 256), 8) * 8), 256, 0, s>>>(
        (const P *)m->d_rowptrs, m->d_colinds, ap->row_list.as<int32_t>(), B.n, B.nb, ACC_CB, B.d_trow.as<int32_t>(),
        B.d_tpiece.as<int32_t>(), n_tasks, B.pstart.as<int32_t>());
    CSRK_LAUNCH_CHECK();
    return CSRK_OK;
}

// the pair counts, the padding gaps between the pairs of a block, the counts' scan, and the tiles before each block
static int acc_pair_counts(AccBuild &B, hipStream_t s)
{
    acc_paircount_kernel<<<(unsigned)ceil_div(B.pairs, 256), 256, 0, s>>>(B.pstart.as<int32_t>(), B.pairs, B.n, B.off.as<int64_t>());
    CSRK_LAUNCH_CHECK();
    CSRK_TRY(B.gap.alloc((size_t)B.pairs * 4));
    acc_gap_kernel<<<(unsigned)ceil_div((int64_t)B.nb * WAVE, 256), 256, 0, s>>>(B.off.as<int64_t>(), B.n, B.nb, B.gap.as<int32_t>());
    CSRK_LAUNCH_CHECK();
    CSRK_TRY(exclusive_scan_i64(B.off.as<int64_t>(), B.off.as<int64_t>(), B.pairs, s));
    CSRK_TRY(block_tile_starts(B.off, B.n, B.nb, ACC_TILE, 0, B.bends, B.t0, s));
    B.n_tiles = B.t0[(size_t)B.nb];
    return CSRK_OK;
}

// persistent workgroups: one per CU (or wg_want), equal shares of the tiles (stored interleaved: acc_phys_tile)
static int acc_shares(Matrix *m, int32_t wg_want, AccBuild &B, hipStream_t s)
{
    int cus = 0;
    CSRK_TRY(device_cus(m, &cus));
    B.sh = spmvlayout::wg_shares(B.n_tiles, wg_want, cus);
    CSRK_TRY(B.d_wg_t0.alloc((size_t)(B.sh.n_wg + 1) * 8));
    CSRK_TRY(stage_h2d(B.d_wg_t0.p, B.sh.wg_t0.data(), (size_t)(B.sh.n_wg + 1) * 8, s));
    return CSRK_OK;
}

// float64 values that lie on one binary grid are kept in 7 bytes (fix56.h: 9 B per entry; decoded exactly).  One switch for
// the whole group: the grid test over its values, and CSRK_SPMV_FIX56=0 forbids the form (tests, measurements)
template <class P, int VT>
static int acc_value_form(Matrix *m, AccPanel *ap, int form, const SpmvKnobs &knobs, AccBuild &B, PlanTrace &tr, hipStream_t s)
{
    CSRK_TRY(B.fx.alloc(16));
    if (!(VT == CSRK_VAL_F64 && B.n > 0 && form != ACC_FORM_RAW) || knobs.fix56_off) return CSRK_OK;
    int32_t h[4] = {0, INT32_MAX, INT32_MIN, 0};
    CSRK_TRY(stage_h2d(B.fx.p, h, sizeof h, s));
    acc_range_kernel<P><<<dim3((unsigned)B.n, 16), 256, 0, s>>>((const P *)m->d_rowptrs, (const double *)m->d_values,
                                                               ap->row_list.as<int32_t>(), B.fx.as<int32_t>());
    CSRK_LAUNCH_CHECK();
    CSRK_TRY(stage_d2h(h, B.fx.p, sizeof h, s));
    CSRK_HIP(hipStreamSynchronize(s));
    fix56::Range r;
    r.bad = h[0];
    r.lo = h[1];
    r.hi = h[2];
    ap->fix56 = fix56::packable(r, ap->fx_g);
    ap->nib = ap->fix56 && form == ACC_FORM_NIB;
    tr.lap("  tier 0: value grid test");
    return CSRK_OK;
}

// the group's entries into tiles of SV values and 16-bit index words, then the padding of every block's last tile;
// VERIFY: nothing is written, every stored entry is decoded as the product decodes it and compared with the source (fx[3])
template <class P, int VT, class SV, bool VERIFY>
static int acc_fill(Matrix *m, AccPanel *ap, AccBuild &B, hipStream_t s)
{
    const int32_t n = B.n, nb = B.nb, n_wg = (int32_t)B.sh.n_wg;
    const int32_t fill_waves = (int32_t)ceil_div(n, WAVE);      // wavefronts per block: 64 pairs each
    acc_fill_kernel<P, VT, SV, VERIFY><<<(unsigned)ceil_div((int64_t)nb * fill_waves * WAVE, 256), 256, 0, s>>>(
        (const P *)m->d_rowptrs, m->d_colinds, m->d_values, ap->row_list.as<int32_t>(), n, nb, ACC_CB, B.off.as<int64_t>(),
        B.bends.as<int64_t>(), B.pstart.as<int32_t>(), B.gap.as<int32_t>(), ap->vals.as<SV>(), ap->idx.as<uint16_t>(),
        ap->tile_row0.as<int32_t>(), B.d_wg_t0.as<int64_t>(), n_wg, fill_waves, ap->fx_g, B.fx.as<int32_t>() + 3);
    CSRK_LAUNCH_CHECK();
    acc_pad_kernel<SV, VERIFY><<<(unsigned)nb, 256, 0, s>>>(B.off.as<int64_t>(), n, nb, B.bends.as<int64_t>(), ap->vals.as<SV>(),
                                                            ap->idx.as<uint16_t>(), B.d_wg_t0.as<int64_t>(), n_wg, ap->fx_g,
                                                            B.fx.as<int32_t>() + 3);
    CSRK_LAUNCH_CHECK();
    return CSRK_OK;
}

// The stream in the form acc_value_form chose.  A packed form is the library's own proof of "exact", on every plan: every
// stored entry decoded as the product decodes it, against the source (the 8.5-byte form: its column and row step too); a
// single mismatch and the group is filled raw.
template <class P, int VT>
static int acc_fill_stream(Matrix *m, AccPanel *ap, AccBuild &B, PlanTrace &tr, hipStream_t s)
{
    const int64_t n_phys = B.sh.n_phys;
    CSRK_TRY(ap->idx.alloc((size_t)n_phys * ACC_TILE * 2));
    CSRK_TRY(ap->tile_row0.alloc((size_t)(B.n_tiles ? B.n_tiles : 1) * 4));
    if (ap->fix56) {
        int32_t mismatch = 1;
        if (ap->nib) {
            CSRK_TRY(ap->vals.alloc((size_t)n_phys * fix56::nib::TILE_BYTES));
            CSRK_HIP(hipMemsetAsync(ap->vals.p, 0, (size_t)n_phys * fix56::nib::TILE_BYTES, s));      // (the nibbles are or-ed in)
            CSRK_TRY((acc_fill<P, VT, fix56::nib::Bytes, false>(m, ap, B, s)));
            tr.lap("  tier 0: fill (nib)");
            CSRK_TRY((acc_fill<P, VT, fix56::nib::Bytes, true>(m, ap, B, s)));
        } else {
            CSRK_TRY(ap->vals.alloc((size_t)n_phys * fix56::TILE_BYTES));
            CSRK_TRY((acc_fill<P, VT, fix56::Packed, false>(m, ap, B, s)));
            tr.lap("  tier 0: fill (fix56)");
            CSRK_TRY((acc_fill<P, VT, fix56::Packed, true>(m, ap, B, s)));
        }
        CSRK_TRY(stage_d2h(&mismatch, B.fx.as<int32_t>() + 3, 4, s));
        CSRK_HIP(hipStreamSynchronize(s));
        tr.lap(ap->nib ? "  tier 0: verify (nib)" : "  tier 0: verify (fix56)");
        if (mismatch) {
            ap->fix56 = ap->nib = false;
            ap->fx_g = 0;
        }
    }
    if (!ap->fix56) {
        CSRK_TRY(ap->vals.alloc((size_t)n_phys * ACC_TILE * (ap->f32 ? 4 : 8)));
        if (ap->f32) CSRK_TRY((acc_fill<P, VT, float, false>(m, ap, B, s)));
        else CSRK_TRY((acc_fill<P, VT, double, false>(m, ap, B, s)));
        tr.lap("  tier 0: fill");
    }
    return CSRK_OK;
}

// the workgroups' shares cut into one-block segments (spmvlayout::acc_segments), the partials, the kernel's LDS
static int acc_segment_tables(AccPanel *ap, AccBuild &B, hipStream_t s)
{
    std::vector<AccSeg> segs;
    std::vector<int32_t> wg_seg;
    spmvlayout::acc_segments(B.sh.wg_t0, B.t0.data(), ACC_SEG_TILES, segs, wg_seg);
    CSRK_TRY(ap->segs.alloc(segs.size() * sizeof(AccSeg)));
    CSRK_TRY(ap->wg_seg.alloc(wg_seg.size() * 4));
    CSRK_TRY(stage_h2d(ap->segs.p, segs.data(), segs.size() * sizeof(AccSeg), s));
    CSRK_TRY(stage_h2d(ap->wg_seg.p, wg_seg.data(), wg_seg.size() * 4, s));
    CSRK_TRY(ap->partial.alloc((size_t)B.sh.n_wg * B.n * 8));
    CSRK_TRY(ap->z.alloc((size_t)B.n * 8));
    ap->lds = spmvlayout::acc_lds_bytes(ACC_CB, B.n, ACC_SEG_TILES);
    CSRK_TRY(spmv_kernel_attributes());
    CSRK_HIP(hipStreamSynchronize(s));     // `segs`, `wg_seg`, `t0` are host temporaries of async copies
    ap->n_segs = (int64_t)segs.size();
    return CSRK_OK;
}

// Build one accumulator-form group: the listed heavy rows (<= ACC_MAXROWS, ascending) as a tiled,
// column-block-major (value, packed index) stream plus the persistent workgroups' segment lists.
// wg_want: the group's workgroups when it shares its launch with other groups (0: one per CU); form: above.
template <class P, int VT>
static int build_acc_panel(Matrix *m, AccPanel *ap, const int32_t *rows, const int64_t *lens, int32_t n, int64_t nnz_rows,
                           const SpmvKnobs &knobs, hipStream_t s, int32_t wg_want = 0, int form = ACC_FORM_FIX56)
{
    ap->fix56 = false;
    ap->nib = false;
    ap->fx_g = 0;
    PlanTrace tr(knobs);
    CSRK_TRY(ap->row_list.alloc((size_t)n * 4));
    CSRK_TRY(stage_h2d(ap->row_list.p, rows, (size_t)n * 4, s));
    AccBuild B;
    B.n = n;
    B.nb = (int32_t)ceil_div(m->ncols > 0 ? m->ncols : 1, ACC_CB);
    B.pairs = (int64_t)n * B.nb;
    CSRK_TRY(acc_pair_starts<P>(m, ap, lens, B, s));
    tr.lap("  tier 0: pair starts");
    CSRK_TRY(acc_pair_counts(B, s));
    tr.lap("  tier 0: counts, gaps, scan");
    CSRK_TRY(acc_shares(m, wg_want, B, s));
    // a float32 matrix keeps float32 values in the stream (6 B per entry; widened in the kernel, exactly)
    ap->f32 = VT == CSRK_VAL_F32;
    CSRK_TRY((acc_value_form<P, VT>(m, ap, form, knobs, B, tr, s)));
    CSRK_TRY((acc_fill_stream<P, VT>(m, ap, B, tr, s)));
    CSRK_TRY(acc_segment_tables(ap, B, s));
    ap->nrow = n;
    ap->nb = B.nb;
    ap->n_wg = (int32_t)B.sh.n_wg;
    ap->tiles = B.n_tiles;
    ap->nnz = nnz_rows;
    if (tr.on)
        fprintf(stderr, "[csrk plan]   tier 0 group: rows %d entries %lld workgroups %lld tiles %lld, %.1f per segment%s\n", n,
                (long long)nnz_rows, (long long)B.sh.n_wg, (long long)B.n_tiles,
                ap->n_segs ? (double)B.n_tiles / (double)ap->n_segs : 0.0,
                ap->nib ? " (nib)" : ap->fix56 ? " (fix56)" : ap->f32 ? " (float32)" : " (raw)");
    tr.lap("  tier 0: segments");
    return CSRK_OK;
}

// ---- the long-row split: build_heavy_split and its steps ------------------------------------------
// which rows are cut out (at least cut_min entries): flags, their scans -> the cut rows and their entries in all
template <class P>
static int split_flags(Matrix *m, int cut_min, DevBuf &flag, DevBuf &hlen, int32_t *n_cut, int64_t *nnz_cut, hipStream_t s)
{
    const int32_t nr = m->nrows;
    CSRK_TRY(flag.alloc((size_t)(nr + 2) * 4));
    CSRK_TRY(hlen.alloc((size_t)(nr + 2) * 8));
    heavy_flag_kernel<P><<<(unsigned)ceil_div((int64_t)nr + 1, 256), 256, 0, s>>>((const P *)m->d_rowptrs, nr, flag.as<int32_t>(),
                                                                                 hlen.as<int64_t>(), cut_min);
    CSRK_LAUNCH_CHECK();
    CSRK_TRY(exclusive_scan_i32(flag.as<int32_t>(), flag.as<int32_t>(), nr, s));      // -> cut-row index
    CSRK_TRY(exclusive_scan_i64(hlen.as<int64_t>(), hlen.as<int64_t>(), nr, s));      // -> cut entries before
    CSRK_TRY(stage_d2h(n_cut, flag.as<int32_t>() + nr, 4, s));
    CSRK_TRY(stage_d2h(nnz_cut, hlen.as<int64_t>() + nr, 8, s));
    CSRK_HIP(hipStreamSynchronize(s));
    return CSRK_OK;
}

// the light view (row pointers with the cut rows collapsed), the cut rows' tables, and whether their columns ascend
template <class P>
static int split_view(Matrix *m, SpmvPlan *p, int32_t n_cut, const DevBuf &flag, const DevBuf &hlen, DevBuf &bad, DevBuf &clen,
                      hipStream_t s)
{
    const P *rp = (const P *)m->d_rowptrs;
    const int32_t nr = m->nrows;
    CSRK_TRY(p->rp_light.alloc((size_t)(nr + 1) * sizeof(P)));
    CSRK_TRY(p->heavy_row.alloc((size_t)n_cut * 4));
    CSRK_TRY(p->cut_pos.alloc((size_t)n_cut * 8));
    CSRK_TRY(p->cut_cum.alloc((size_t)(n_cut + 1) * 8));
    CSRK_TRY(clen.alloc((size_t)n_cut * 8));
    heavy_view_kernel<P><<<(unsigned)ceil_div((int64_t)nr + 1, 256), 256, 0, s>>>(
        rp, nr, flag.as<int32_t>(), hlen.as<int64_t>(), p->rp_light.as<P>(), p->heavy_row.as<int32_t>(), p->cut_pos.as<int64_t>(),
        p->cut_cum.as<int64_t>(), clen.as<int64_t>(), n_cut);
    CSRK_LAUNCH_CHECK();
    CSRK_TRY(bad.alloc(4));
    CSRK_HIP(hipMemsetAsync(bad.p, 0, 4, s));
    heavy_sorted_kernel<P><<<(unsigned)n_cut, 1024, 0, s>>>(rp, m->d_colinds, p->heavy_row.as<int32_t>(), n_cut,
                                                         bad.as<int32_t>());
    CSRK_LAUNCH_CHECK();
    return CSRK_OK;
}

// Tier 0's groups side by side in one launch: what CSRK_ACC_GROUPS says, else as many (ACC_GROUPS_DEFAULT at most) as keep
// the segments long enough to pay (accgroups::choose_groups).  `extend`: tier 0 may be extended below heavy_min.
static int split_acc_groups(Matrix *m, const SpmvKnobs &knobs, const std::vector<int64_t> &lens, bool extend, int cut_min,
                            int heavy_min, int *groups)
{
    *groups = knobs.acc_groups;
    if (knobs.acc_groups_set) return CSRK_OK;
    int cus = 0;
    CSRK_TRY(device_cus(m, &cus));
    *groups = accgroups::choose_groups(lens.data(), (int32_t)lens.size(), ACC_GROUPS_DEFAULT, knobs.acc_group_rows,
                                       extend ? (int64_t)std::max(ACC_FLOOR, cut_min) : (int64_t)heavy_min,
                                       ceil_div(m->ncols > 0 ? m->ncols : 1, ACC_CB), cus);
    return CSRK_OK;
}

// Cut the long rows out of the merge path and list them for their tiers (build_tiers builds those).  The two thresholds
// are locals, seeded from the knobs: tier 0's may be lowered for this matrix (spmvlayout::tier0_threshold), and what was
// chosen goes to p->heavy_min / p->tier1_min.
template <class P>
static int build_heavy_split(Matrix *m, SpmvPlan *p, const SpmvKnobs &knobs, hipStream_t s, bool allow_tier1 = true)
{
    p->n_heavy = 0;
    if (knobs.heavy_split == 0) return CSRK_OK;
    // (CSRK_HEAVY_MIN, CSRK_TIERB_MIN: test hooks, not tuning switches: a small matrix gets more "heavy" rows than one
    // accumulator group holds, or no tier 1)
    int heavy_min = knobs.heavy_min;
    const int tierb_min = knobs.tierb_min;
    const bool tier1 = allow_tier1 && tierb_min > 0 && tierb_min < heavy_min;
    const int cut_min = tier1 ? tierb_min : heavy_min;
    if (m->nrows == 0 || m->nnz < cut_min) return CSRK_OK;
    // The split pays for itself only when x does not fit in an XCD's 4 MiB L2: otherwise every gather
    // is an L2 hit already and the panels only add (block, row) overhead (MovieLens-25M shape, x = 472 KB:
    // 0.146 ms on the single merge path against 0.176-0.53 ms split; measured).  CSRK_SPMV_HEAVY_SPLIT=1 forces it.
    if (spmvlayout::x_fits_l2(m->ncols) && knobs.heavy_split != 1) return CSRK_OK;
    PlanTrace tr(knobs);
    DevBuf flag, hlen, bad, clen;
    int32_t n_cut = 0;
    int64_t nnz_cut = 0;
    CSRK_TRY(split_flags<P>(m, cut_min, flag, hlen, &n_cut, &nnz_cut, s));
    tr.lap("  split: flags + scans");
    if (n_cut == 0) return CSRK_OK;
    CSRK_TRY(split_view<P>(m, p, n_cut, flag, hlen, bad, clen, s));
    tr.lap("  split: view + sorted kernels");
    int32_t is_bad = 0;
    std::vector<int32_t> rows((size_t)n_cut);
    std::vector<int64_t> lens((size_t)n_cut);
    CSRK_TRY(stage_d2h(&is_bad, bad.p, 4, s));
    CSRK_TRY(stage_d2h(rows.data(), p->heavy_row.p, (size_t)n_cut * 4, s));
    CSRK_TRY(stage_d2h(lens.data(), clen.p, (size_t)n_cut * 8, s));
    CSRK_HIP(hipStreamSynchronize(s));
    if (tr.on) fprintf(stderr, "[csrk plan]   n_cut %d\n", n_cut);
    tr.lap("  split: copies to the host");
    if (is_bad) return CSRK_OK;      // unsorted columns in a long row: column blocking needs order

    // tier 0: accumulator form (groups of <= ACC_MAXROWS rows).  The accumulator form costs 1.8 ps per entry against 4.8 for
    // tier 1 (measured, headline matrix), and one group holds up to ACC_MAXROWS rows at no extra window traffic: when fewer
    // rows than the tier holds reach heavy_min, tier 0 is extended downwards to its longest rows (not below ACC_FLOOR).
    // With G groups side by side in one launch (build_acc_groups) the tier holds G times as many rows.  Setting
    // CSRK_HEAVY_MIN at all turns the extension off.
    const bool extend = tier1 && !knobs.heavy_min_set;
    CSRK_TRY(split_acc_groups(m, knobs, lens, extend, cut_min, heavy_min, &p->acc_groups));
    const int64_t t0_cap = (int64_t)p->acc_groups * knobs.acc_group_rows;
    if (extend) heavy_min = spmvlayout::tier0_threshold(lens.data(), n_cut, t0_cap, heavy_min, ACC_FLOOR);
    p->heavy_min = heavy_min;
    p->tier1_min = tierb_min;
    std::vector<int32_t> r0, r1;     // tier 0: >= heavy_min entries; tier 1: the rest of the cut rows
    std::vector<int64_t> len0;
    int64_t nnz1 = 0;
    spmvlayout::split_rows(rows.data(), lens.data(), n_cut, heavy_min, r0, len0, r1, &nnz1);
    // Too many (block, row) pairs for tier 1: once more without it.  The second pass re-reads nothing -- the same knobs,
    // its own thresholds seeded from them -- and runs the same launches again with heavy_min as the only cut.
    if (tier1 && !spmvlayout::tier1_pairs_fit((int64_t)r1.size(), m->ncols, PANEL_CB1)) return build_heavy_split<P>(m, p, knobs, s, false);

    p->n_heavy = n_cut;
    p->nnz_light = m->nnz - nnz_cut;
    p->t0_rows = std::move(r0);
    p->t0_lens = std::move(len0);
    p->t1_rows = std::move(r1);
    p->t1_nnz = nnz1;
    tr.lap("  split: host lists");
    return CSRK_OK;
}

// Tier 0: deal its rows to groups (accgroups::deal_rows) and build them.  The groups of one launch split the CUs between
// them, hold values of one form, and their workgroups are placed so that those of one column range share an XCD
// (accgroups::place_wgs).  One group in a launch is built as it always was: a workgroup per CU, no map.
template <class P, int VT>
static int build_acc_groups(Matrix *m, SpmvPlan *p, const SpmvKnobs &knobs, hipStream_t s)
{
    const std::vector<int32_t> &r0 = p->t0_rows;
    const std::vector<int64_t> &len0 = p->t0_lens;
    if (r0.empty()) return CSRK_OK;
    const accgroups::Deal deal = accgroups::deal_rows(len0.data(), (int32_t)r0.size(), p->acc_groups, knobs.acc_group_rows);
    int cus = 0;
    CSRK_TRY(device_cus(m, &cus));
    std::vector<int32_t> rows;
    std::vector<int64_t> lens;
    for (size_t j = 0; j + 1 < deal.first.size(); j++) {
        const int k0 = deal.first[j], gb = deal.first[j + 1] - k0;
        const size_t a0 = p->acc.size();
        // the launch's packed form: 8.5-byte entries where the stream is what the kernel's time is (accgroups::choose_nib)
        int64_t launch_entries = 0;
        for (int g = 0; g < gb; g++)
            for (int32_t pos : deal.groups[(size_t)(k0 + g)]) launch_entries += len0[(size_t)pos];
        const int packed = accgroups::choose_nib(knobs.nib, launch_entries, cus) ? ACC_FORM_NIB : ACC_FORM_FIX56;
        auto build = [&](int g, int form) -> int {
            const std::vector<int32_t> &pos = deal.groups[(size_t)(k0 + g)];
            rows.resize(pos.size());
            lens.resize(pos.size());
            int64_t gn = 0;
            for (size_t i = 0; i < pos.size(); i++) {
                rows[i] = r0[(size_t)pos[i]];
                lens[i] = len0[(size_t)pos[i]];
                gn += lens[i];
            }
            return build_acc_panel<P, VT>(m, p->acc[a0 + (size_t)g], rows.data(), lens.data(), (int32_t)pos.size(), gn, knobs, s,
                                          gb > 1 ? accgroups::group_wgs(cus, gb, g) : 0, form);
        };
        bool any_raw = false;
        for (int g = 0; g < gb; g++) {
            AccPanel *ap = new (std::nothrow) AccPanel();
            CSRK_REQUIRE(ap, "out of host memory");
            p->acc.push_back(ap);
            CSRK_TRY(build(g, packed));
            any_raw = any_raw || !ap->fix56;
        }
        AccPanel *head = p->acc[a0];
        if (gb == 1) continue;
        // one kernel serves the launch: its groups hold one form of values
        for (int g = 0; g < gb; g++)
            if (any_raw && p->acc[a0 + (size_t)g]->fix56) CSRK_TRY(build(g, ACC_FORM_RAW));
        int32_t n_wg[accgroups::MAX_GROUPS];
        for (int g = 0; g < gb; g++) {
            n_wg[g] = p->acc[a0 + (size_t)g]->n_wg;
            p->acc[a0 + (size_t)g]->launch_groups = 0;
        }
        const std::vector<uint32_t> map = accgroups::place_wgs(n_wg, gb);
        head->launch_groups = gb;
        head->launch_wgs = (int32_t)map.size();
        CSRK_TRY(head->wg_map.alloc(map.size() * 4));
        CSRK_TRY(stage_h2d(head->wg_map.p, map.data(), map.size() * 4, s));
        CSRK_HIP(hipStreamSynchronize(s));     // `map` is a host temporary of an async copy
    }
    return CSRK_OK;
}

// Build the tiers of the rows build_heavy_split cut out: tier 0's groups, then tier 1's panel.
template <class P>
static int build_tiers(Matrix *m, SpmvPlan *p, const SpmvKnobs &knobs, hipStream_t s)
{
    if (!p->n_heavy) return CSRK_OK;
    return with_val_type(m->val_type, [&](auto vt) -> int {
        constexpr int VT = decltype(vt)::value;
        CSRK_TRY((build_acc_groups<P, VT>(m, p, knobs, s)));
        if (!p->t1_rows.empty()) CSRK_TRY((build_panel<P, VT>(m, &p->tier1, p->t1_rows, p->t1_nnz, PANEL_CB1, 1, true, knobs, s)));
        return CSRK_OK;
    });
}

// ---- the hot-column pack: build_hot_cache and its steps -------------------------------------------
// sampled reference counts per column (hot_count_kernel); *n_samples = entries counted
template <class P>
static int hot_counts(Matrix *m, SpmvPlan *p, DevBuf &cnt, DevBuf &census, int64_t *n_samples, hipStream_t s)
{
    const int32_t nc = m->ncols;
    CSRK_HIP(hipMemsetAsync(cnt.p, 0, (size_t)(nc + 1) * 4, s));
    CSRK_HIP(hipMemsetAsync(census.p, 0, 16, s));
    const int64_t row_stride = p->nnz_light > (1ll << 25) ? p->nnz_light >> 25 : 1;
    const int64_t hc_need = ceil_div(ceil_div(m->nrows, WAVE * row_stride), HOT_THREADS / WAVE);
    hot_count_kernel<P><<<(unsigned)(hc_need < 1024 ? hc_need : 1024), HOT_THREADS, 0, s>>>(
        (const P *)m->d_rowptrs, p->n_heavy ? p->rp_light.as<P>() : (const P *)nullptr, m->d_colinds, m->nrows,
        row_stride, cnt.as<int32_t>(), census.as<unsigned long long>());
    CSRK_LAUNCH_CHECK();
    unsigned long long n_samples_u = 0;
    CSRK_TRY(stage_d2h(&n_samples_u, census.p, 8, s));
    CSRK_HIP(hipStreamSynchronize(s));
    *n_samples = (int64_t)n_samples_u;
    return CSRK_OK;
}

// out[0] = columns with count >= thr, out[1] = the sum of their counts: one launch and one round trip
static int hot_census_at(const DevBuf &cnt, DevBuf &census, int32_t nc, int32_t thr, unsigned long long out[2], hipStream_t s)
{
    CSRK_HIP(hipMemsetAsync(census.p, 0, 16, s));
    hot_census_kernel<<<1024, 256, 0, s>>>(cnt.as<int32_t>(), nc, thr, census.as<unsigned long long>());
    CSRK_LAUNCH_CHECK();
    CSRK_TRY(stage_d2h(out, census.p, 16, s));
    CSRK_HIP(hipStreamSynchronize(s));
    return CSRK_OK;
}

// The smallest threshold (>= 2 references in the sample) that leaves at most `slots` columns; c[0] = those columns, c[1]
// = their references.  One histogram pass decides it (spmvlayout::hot_threshold_from_hist) unless more than `slots` columns
// sit in the histogram's shared top bin: then a binary search, a census launch per probe.
static int hot_threshold(const DevBuf &cnt, DevBuf &census, int32_t nc, int64_t n_samples, int64_t slots, int32_t *thr,
                         unsigned long long c[2], hipStream_t s)
{
    int64_t lo = 2, hi = n_samples + 1;     // invariant: census(hi).n <= slots
    spmvlayout::HotThreshold ht;
    {
        DevBuf hist;
        CSRK_TRY(hist.alloc((size_t)2 * (HOT_HIST + 1) * 8));
        CSRK_HIP(hipMemsetAsync(hist.p, 0, (size_t)2 * (HOT_HIST + 1) * 8, s));
        hot_hist_kernel<<<1024, 256, 0, s>>>(cnt.as<int32_t>(), nc, hist.as<unsigned long long>(),
                                             hist.as<unsigned long long>() + (HOT_HIST + 1));
        CSRK_LAUNCH_CHECK();
        std::vector<unsigned long long> hh((size_t)2 * (HOT_HIST + 1));
        CSRK_TRY(stage_d2h(hh.data(), hist.p, hh.size() * 8, s));
        CSRK_HIP(hipStreamSynchronize(s));
        ht = spmvlayout::hot_threshold_from_hist(hh.data(), hh.data() + (HOT_HIST + 1), HOT_HIST, slots);
    }
    if (ht.decided) {
        lo = ht.thr;
        c[0] = ht.cols;
        c[1] = ht.refs;
    } else {
        CSRK_TRY(hot_census_at(cnt, census, nc, (int32_t)lo, c, s));
        if (c[0] > (unsigned long long)slots) {
            while (lo + 1 < hi) {
                const int64_t mid = lo + (hi - lo) / 2;
                CSRK_TRY(hot_census_at(cnt, census, nc, spmvlayout::clamp_i32(mid), c, s));
                if (c[0] <= (unsigned long long)slots)
                    hi = mid;
                else
                    lo = mid;
            }
            CSRK_TRY(hot_census_at(cnt, census, nc, spmvlayout::clamp_i32(hi), c, s));
            lo = hi;
        }
    }
    *thr = spmvlayout::clamp_i32(lo);
    return CSRK_OK;
}

// The packed columns, in column order (hot_cols, with their counts in hcnt), then in order of popularity: stable, count
// descending (hot_sort_*_kernel): four 8-bit passes, ping-pong between (hcnt, hot_cols) and (k2, v2)
static int hot_order(SpmvPlan *p, const DevBuf &cnt, DevBuf &slot, DevBuf &hcnt, int32_t nc, int32_t thr, int32_t n_hot, hipStream_t s)
{
    const unsigned gc = (unsigned)ceil_div((int64_t)nc + 1, 256);
    hot_flag_kernel<<<gc, 256, 0, s>>>(cnt.as<int32_t>(), nc, thr, slot.as<int32_t>());
    CSRK_LAUNCH_CHECK();
    CSRK_TRY(exclusive_scan_i32(slot.as<int32_t>(), slot.as<int32_t>(), nc, s));
    CSRK_TRY(p->hot_cols.alloc((size_t)n_hot * 4));
    CSRK_TRY(hcnt.alloc((size_t)n_hot * 4));
    hot_list_kernel<<<gc, 256, 0, s>>>(cnt.as<int32_t>(), slot.as<int32_t>(), nc, thr, p->hot_cols.as<int32_t>(),
                                      hcnt.as<int32_t>());
    CSRK_LAUNCH_CHECK();
    const int32_t nchunk = (int32_t)ceil_div(n_hot, HS_CHUNK);
    DevBuf k2, v2, dc;
    CSRK_TRY(k2.alloc((size_t)n_hot * 4));
    CSRK_TRY(v2.alloc((size_t)n_hot * 4));
    CSRK_TRY(dc.alloc((size_t)(256 * (int64_t)nchunk + 1) * 4));
    uint32_t *ka = hcnt.as<uint32_t>(), *kb = k2.as<uint32_t>();
    int32_t *va = p->hot_cols.as<int32_t>(), *vb = v2.as<int32_t>();
    for (int pass = 0; pass < 4; pass++) {
        hot_sort_count_kernel<<<(unsigned)nchunk, WAVE, 0, s>>>(ka, n_hot, 8 * pass, nchunk, dc.as<int32_t>());
        CSRK_LAUNCH_CHECK();
        CSRK_TRY(exclusive_scan_i32(dc.as<int32_t>(), dc.as<int32_t>(), 256 * (int64_t)nchunk, s));
        hot_sort_place_kernel<<<(unsigned)nchunk, WAVE, 0, s>>>(ka, va, n_hot, 8 * pass, nchunk, dc.as<int32_t>(), kb, vb);
        CSRK_LAUNCH_CHECK();
        std::swap(ka, kb);
        std::swap(va, vb);
    }
    CSRK_HIP(hipStreamSynchronize(s));      // k2, v2, dc are freed here (the sorted columns are back in hot_cols)
    return CSRK_OK;
}

// Pick the (at most HOT_SLOTS_MAX) most referenced columns and renumber them in a copy of colinds.  Built
// with the lazy plan (second launch on a handle).  Skipped when x is small enough to live in L1/L2
// next to the streams anyway, when the matrix is small, or when the cached columns would carry less
// than a fifth of the entries (no popularity skew: nothing to gain, and the persistent grid has fewer
// wavefronts in flight than the plain one).  CSRK_SPMV_HOT=0 disables, =1 forces.
template <class P>
static int build_hot_cache(Matrix *m, SpmvPlan *p, const SpmvKnobs &knobs, hipStream_t s)
{
    p->n_hot = 0;
    if (knobs.hot == 0) return CSRK_OK;
    const bool force = knobs.hot == 1;
    if (m->nnz < 2 || m->ncols < 1) return CSRK_OK;
    PlanTrace tr(knobs);
    // 4 MiB of packed x, most popular first (light stream, LDS for the first 8192: 64k 0.340, 256k 0.308, 512k 0.302, 1M 0.297,
    // 2M 0.297 ms, but the per-call pack costs more than that gains past 512k); earlier sweep, tile kernel, 512 KiB of packed
    // x (measured on the headline matrix: 16k 0.431, 64k 0.422, 256k 0.430, 1M 0.439, 4M 0.460 ms for the tile kernel; none
    // 0.481)
    const int64_t slots = HOT_SLOTS_MAX;
    p->hot_slots = (int32_t)slots;
    // x that fits in L2 whole needs no packing
    if (!force && !spmvlayout::pack_worth_counting(m->nnz, m->ncols)) return CSRK_OK;
    const int32_t nc = m->ncols;
    DevBuf cnt, slot, census;
    CSRK_TRY(cnt.alloc((size_t)(nc + 1) * 4));
    CSRK_TRY(slot.alloc((size_t)(nc + 2) * 4));
    CSRK_TRY(census.alloc(16));
    int64_t n_samples = 0;
    CSRK_TRY(hot_counts<P>(m, p, cnt, census, &n_samples, s));
    tr.lap("  hot: column counts");
    if (n_samples == 0) return CSRK_OK;
    int32_t thr = 0;
    unsigned long long c[2] = {0, 0};
    CSRK_TRY(hot_threshold(cnt, census, nc, n_samples, slots, &thr, c, s));
    const int32_t n_hot = (int32_t)c[0];
    tr.lap("  hot: threshold");
    p->hot_cover = n_samples ? (double)c[1] / (double)n_samples : 0.0;
    if (n_hot == 0 || (!force && !spmvlayout::pack_cover_pays(p->hot_cover))) return CSRK_OK;

    // Slots in order of popularity (count descending, column ascending among equals): the first
    // LS_HOT_LDS slots are the ones the light stream keeps in LDS, and the packed lines that follow
    // are referenced less and less often, so what L2 fails to retain is the pack's tail.
    DevBuf hcnt;
    CSRK_TRY(hot_order(p, cnt, slot, hcnt, nc, thr, n_hot, s));
    tr.lap("  hot: list, order by count");
    // column -> slot map (-1: not packed); the light stream's fill reads it, as does the renumbered colinds copy
    // the tile kernel needs when no stream is built
    CSRK_TRY(p->hot_slot.alloc((size_t)nc * 4));
    CSRK_HIP(hipMemsetAsync(p->hot_slot.p, 0xff, (size_t)nc * 4, s));
    hot_slot_kernel<<<(unsigned)ceil_div(n_hot, 256), 256, 0, s>>>(p->hot_cols.as<int32_t>(), n_hot, p->hot_slot.as<int32_t>());
    CSRK_LAUNCH_CHECK();
    CSRK_TRY(p->xh.alloc((size_t)n_hot * 8));
    p->n_hot = n_hot;
    p->n_hot_lds = n_hot < LS_HOT_LDS ? n_hot : LS_HOT_LDS;
    CSRK_HIP(hipStreamSynchronize(s));     // hcnt is freed on return
    return CSRK_OK;
}

// ---- the light stream: build_stream, build_cold_stage, build_light_stream -------------------------
// Build the arrays of the light stream from a view: view row r (r < nrows_view) is the source entries
// src[r] .. src[r] + (rpv[r+1] - rpv[r]) of (ci, vs); n_ent entries in n_tiles tiles.
template <class P, int VT>
static int build_stream(Matrix *m, LightStream *ls, const P *src, const P *rpv, int32_t nrows_view, const int32_t *ci,
                        const void *vs, int64_t n_ent, int64_t n_tiles, int32_t n_out, const int32_t *slot_map,
                        const SpmvKnobs &knobs, hipStream_t s, const P *rp_len = nullptr)
{
    // rp_len (dense rows): rpv gives every row of the view at least one slot; a row that is empty in rp_len is one padding
    // entry.  Run k is then row k, and no row-id table is built.
    ls->on = false;
    ls->dense = rp_len != nullptr;
    PlanTrace tr(knobs);
    DevBuf ridx;
    CSRK_TRY(ridx.alloc((size_t)(nrows_view + 2) * 4));
    const unsigned gr = (unsigned)ceil_div((int64_t)nrows_view + 1, 256);
    ls_rowflag_kernel<P><<<gr, 256, 0, s>>>(rpv, nrows_view, ridx.as<int32_t>());
    CSRK_LAUNCH_CHECK();
    CSRK_TRY(exclusive_scan_i32(ridx.as<int32_t>(), ridx.as<int32_t>(), nrows_view, s));
    int32_t n_runs = 0;
    CSRK_TRY(stage_d2h(&n_runs, ridx.as<int32_t>() + nrows_view, 4, s));
    CSRK_HIP(hipStreamSynchronize(s));
    if (n_runs < 1) return CSRK_OK;
    if (!ls->dense) {
        CSRK_TRY(ls->rowids.alloc((size_t)n_runs * 4));
        ls_rowids_kernel<P><<<gr, 256, 0, s>>>(rpv, nrows_view, ridx.as<int32_t>(), ls->rowids.as<int32_t>());
        CSRK_LAUNCH_CHECK();
    }
    ls->f32 = VT == CSRK_VAL_F32;      // a float32 matrix keeps float32 values in the stream (widened in the kernel, exactly)
    CSRK_TRY(ls->vals.alloc((size_t)n_tiles * ACC_TILE * (ls->f32 ? 4 : 8)));
    CSRK_TRY(ls->idx.alloc((size_t)n_tiles * ACC_TILE * 4));
    ls->idx24 = false;
    DevBuf tile_row;
    CSRK_TRY(tile_row.alloc((size_t)(n_tiles + 1) * 4));
    ls_tilerow_kernel<P><<<(unsigned)ceil_div(n_tiles + 1, 256), 256, 0, s>>>(rpv, nrows_view, n_ent, n_tiles, tile_row.as<int32_t>());
    CSRK_LAUNCH_CHECK();
    if (ls->f32)
        ls_fill_kernel<P, VT, float><<<(unsigned)ceil_div(n_tiles * ACC_TILE, 256), 256, 0, s>>>(
            src, rpv, nrows_view, ci, vs, n_ent, n_tiles * ACC_TILE, slot_map, ls->vals.as<float>(), ls->idx.as<uint32_t>(), rp_len,
            tile_row.as<int32_t>());
    else
        ls_fill_kernel<P, VT, double><<<(unsigned)ceil_div(n_tiles * ACC_TILE, 256), 256, 0, s>>>(
            src, rpv, nrows_view, ci, vs, n_ent, n_tiles * ACC_TILE, slot_map, ls->vals.as<double>(), ls->idx.as<uint32_t>(), rp_len,
            tile_row.as<int32_t>());
    CSRK_LAUNCH_CHECK();
    CSRK_TRY(ls->tile_base.alloc((size_t)n_tiles * 4));
    ls_tilebase_kernel<P><<<(unsigned)ceil_div(n_tiles, 256), 256, 0, s>>>(
        rpv, nrows_view, ridx.as<int32_t>(), n_tiles, tile_row.as<int32_t>(), ls->tile_base.as<int32_t>());
    CSRK_LAUNCH_CHECK();
    CSRK_TRY(ls->carry_row.alloc((size_t)n_tiles * 4));
    CSRK_TRY(ls->carry_val.alloc((size_t)n_tiles * 8));
    int cus = 0;
    CSRK_TRY(device_cus(m, &cus));
    CSRK_TRY(spmv_kernel_attributes());
    const int64_t need = ceil_div(n_tiles, LS_THREADS / WAVE);      // one persistent workgroup per CU at most
    ls->grid = (unsigned)((int64_t)cus < need ? (int64_t)cus : need);
    ls->n_tiles = n_tiles;
    ls->n_runs = n_runs;
    ls->n_out = n_out;
    CSRK_HIP(hipStreamSynchronize(s));      // ridx, tile_row are freed on return
    tr.lap("  light: runs, fill");
    ls->on = true;
    return CSRK_OK;
}
// per index word: count into the (round, block) bucket; the old count is the entry's place inside the bucket
__global__ __launch_bounds__(256) void ls_cold_count_kernel(const uint32_t *__restrict__ sidx, int64_t n_words, int32_t nblk, int32_t W,
                                                           const int32_t *__restrict__ tile_round, int32_t *__restrict__ cnt,
                                                           int32_t *__restrict__ off)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    const uint32_t ix = sidx[w];
    if (!ls_is_cold(ix)) return;
    const int64_t r = tile_round[w / ACC_TILE];
    const int32_t b = (int32_t)((ix & LS_COL_MASK) / (uint32_t)W);
    off[w] = atomicAdd(&cnt[r * nblk + b], 1);
}

__global__ void ls_cold_transpose_kernel(const int32_t *__restrict__ cnt, int32_t nround, int32_t nblk, int32_t *__restrict__ cntT)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)nround * nblk) return;
    const int64_t r = i / nblk, b = i % nblk;
    cntT[b * nround + r] = cnt[i];
}

// position in xg = bucket base in (round, block) order + place; position in the copy list = bucket base in
// (block, round) order + place
// (rel: the index word keeps the position relative to the round's start -- the round-in-LDS form)
__global__ __launch_bounds__(256) void ls_cold_place_kernel(uint32_t *__restrict__ sidx, int64_t n_words, int32_t nround,
                                                           int32_t nblk, int32_t W, const int32_t *__restrict__ tile_round, int rel,
                                                           const int32_t *__restrict__ base_rb,
                                                           const int32_t *__restrict__ base_br, const int32_t *__restrict__ off,
                                                           uint16_t *__restrict__ a_col, int32_t *__restrict__ a_dst)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    const uint32_t ix = sidx[w];
    if (!ls_is_cold(ix)) return;
    const int64_t r = tile_round[w / ACC_TILE];
    const uint32_t c = ix & LS_COL_MASK;
    const int32_t b = (int32_t)(c / (uint32_t)W);
    const int32_t pos = base_rb[r * nblk + b] + off[w];
    const int32_t pa = base_br[(int64_t)b * nround + r] + off[w];
    a_col[pa] = (uint16_t)(c - (uint32_t)b * (uint32_t)W);      // offset inside the block's window
    a_dst[pa] = pos;
    sidx[w] = (ix & LS_START_BIT) | (uint32_t)(rel ? pos - base_rb[r * nblk] : pos);
}

// round_start[r] = position in xg of round r's first staged value, r = 0 .. nround_ls (the last = n_cold)
__global__ void ls_round_start_kernel(const int32_t *__restrict__ base_rb, int32_t nround_ls, int32_t nblk,
                                      int32_t *__restrict__ round_start)
{
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= nround_ls) round_start[r] = base_rb[(int64_t)r * nblk];
}

__global__ void ls_stage_starts_kernel(const int32_t *__restrict__ base_br, int32_t nround, int32_t nblk, int32_t *__restrict__ blk_start)
{
    const int32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b <= nblk) blk_start[b] = base_br[(int64_t)b * nround];      // base_br has nround * nblk + 1 entries
}

// The packed columns ride along: slot k of the pack is entry (column hot_cols[k], position n_cold + k) of a virtual
// last round, so xh = xg + n_cold is filled by the same pass and hot_pack_kernel (10^5.6 gathers of 128 B) goes.
__global__ void ls_pack_count_kernel(const int32_t *__restrict__ hot_cols, int32_t n_hot, int32_t W, int32_t *__restrict__ cnt_last,
                                     int32_t *__restrict__ offp)
{
    const int32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_hot) offp[k] = atomicAdd(&cnt_last[hot_cols[k] / W], 1);
}

__global__ void ls_pack_place_kernel(const int32_t *__restrict__ hot_cols, int32_t n_hot, int32_t W, int32_t nround_all,
                                     const int32_t *__restrict__ base_br, const int32_t *__restrict__ offp, int32_t n_cold,
                                     uint16_t *__restrict__ a_col, int32_t *__restrict__ a_dst)
{
    const int32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_hot) return;
    const int32_t c = hot_cols[k];
    const int32_t pa = base_br[(int64_t)(c / W) * nround_all + (nround_all - 1)] + offp[k];
    a_col[pa] = (uint16_t)(c % W);
    a_dst[pa] = n_cold + k;
}

// Round-in-LDS form (default; CSRK_LS_RND=0 for the round-major form read by gathers): the round is the largest number
// of tiles (a multiple of the workgroup's wavefronts, at most LS_RND_MAXTILES) whose staged values fit LS_RND_CAP in
// every round.

// tile_round[t] = the round that holds tile t (round r = tiles round_tile0[r] .. round_tile0[r + 1])
__global__ void ls_tile_round_kernel(const int32_t *__restrict__ round_tile0, int32_t n_rounds, int64_t n_tiles,
                                     int32_t *__restrict__ tile_round)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    int32_t lo = 0, hi = n_rounds - 1;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo + 1) >> 1);
        if ((int64_t)round_tile0[mid] <= t)
            lo = mid;
        else
            hi = mid - 1;
    }
    tile_round[t] = lo;
}

__global__ void ls_round_total_kernel(const int64_t *__restrict__ tot, int32_t nround_ls, int32_t nblk, int64_t *__restrict__ out)
{
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= nround_ls) out[r] = tot[(int64_t)r * nblk];
}

// tile_cold[t] = cold entries of tile t (one wavefront per tile): with their prefix sums the host finds the largest round
// size whose rounds all fit the LDS round buffer without counting buckets once per candidate size
__global__ __launch_bounds__(256) void ls_tile_cold_kernel(const uint32_t *__restrict__ sidx, int64_t n_tiles, int32_t *__restrict__ tile_cold)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t t = g / WAVE;
    const int lane = (int)(g % WAVE);
    if (t >= n_tiles) return;
    const u32x4_t *ip = (const u32x4_t *)(sidx + t * ACC_TILE);
    const u32x4_t a = ip[lane], b = ip[WAVE + lane];
    int c = (int)ls_is_cold(a.x) + (int)ls_is_cold(a.y) + (int)ls_is_cold(a.z) + (int)ls_is_cold(a.w) + (int)ls_is_cold(b.x) +
            (int)ls_is_cold(b.y) + (int)ls_is_cold(b.z) + (int)ls_is_cold(b.w);
    c = wave_exscan_i32(c, lane) + c;
    if (lane == WAVE - 1) tile_cold[t] = c;
}

// One thread per (tile, lane): the lane's eight uint32 index words -> their 3-byte form (LS24_*: spmv_plan.h).
__global__ __launch_bounds__(256) void ls_idx24_kernel(const uint32_t *__restrict__ sidx, int64_t n_tiles, unsigned char *__restrict__ out)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t t = g / WAVE;
    const int lane = (int)(g % WAVE);
    if (t >= n_tiles) return;
    const u32x4_t *ip = (const u32x4_t *)(sidx + t * ACC_TILE);
    const u32x4_t a = ip[lane], b = ip[WAVE + lane];
    const uint32_t w[ACC_K] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t n[ACC_K];
#pragma unroll
    for (int j = 0; j < ACC_K; j++) {
        const uint32_t c = w[j] & LS_COL_MASK;
        n[j] = (w[j] & LS_HOT_BIT ? LS24_HOT_BIT : 0u) | (w[j] & LS_START_BIT ? 1u << LS24_START_SHIFT : 0u) |
               (c == LS_PAD ? LS24_COL_MASK : c);
    }
    u32x4_t lo;
    lo.x = (n[0] & 0xffffu) | (n[1] << 16);
    lo.y = (n[2] & 0xffffu) | (n[3] << 16);
    lo.z = (n[4] & 0xffffu) | (n[5] << 16);
    lo.w = (n[6] & 0xffffu) | (n[7] << 16);
    u32x2_t hi;
    hi.x = (n[0] >> 16) | ((n[1] >> 16) << 8) | ((n[2] >> 16) << 16) | ((n[3] >> 16) << 24);
    hi.y = (n[4] >> 16) | ((n[5] >> 16) << 8) | ((n[6] >> 16) << 16) | ((n[7] >> 16) << 24);
    unsigned char *tp = out + t * LS24_TILE_BYTES;
    ((u32x4_t *)tp)[lane] = lo;
    ((u32x2_t *)(tp + ACC_TILE * 2))[lane] = hi;
}

// Cold staging of one light stream (spmv_plan.h, "cold staging"): the temporaries in the order they are released in
// reverse, the column blocks, and the rounds of the last count pass.  build_cold_stage runs the steps.
struct ColdStage {
    static constexpr int NW = LS_THREADS / WAVE;      // a round is a whole number of tiles per wavefront
    static_assert(NW * ACC_TILE <= LS_RND_CAP, "the smallest round must fit the LDS round buffer");
    LightStream *ls;
    hipStream_t s;
    DevBuf cnt, cntT, off, offp, tot, tile_round, d_rt0;
    spmvlayout::StageBlocks sb;      // W columns per block, nblk blocks, nb_max (round, block) buckets at most
    int64_t n_words = 0;
    int stage_tiles = LS_STAGE_TILES;
    int64_t nround_ls = 0, nround = 0, nb = 0, n_cold = 0;      // n_cold = where the virtual round starts
    std::vector<int32_t> h_rt0, h_wr0;                          // round_tile0, wg_round0 (spmvlayout::stage_rounds)

    void make_rounds(int nt) { nround_ls = spmvlayout::stage_rounds(ls->n_tiles, ls->grid, nt, NW, h_rt0, h_wr0); }

    int alloc(int32_t n_hot)
    {
        CSRK_TRY(tile_round.alloc((size_t)ls->n_tiles * 4));
        CSRK_TRY(d_rt0.alloc((size_t)(ls->n_tiles + 2) * 4));
        CSRK_TRY(offp.alloc((size_t)n_hot * 4));
        CSRK_TRY(cnt.alloc((size_t)(sb.nb_max + 1) * 4));
        CSRK_TRY(cntT.alloc((size_t)(sb.nb_max + 1) * 4));
        CSRK_TRY(off.alloc((size_t)n_words * 4));
        CSRK_TRY(tot.alloc((size_t)(sb.nb_max + 1) * 8));
        return CSRK_OK;
    }

    // counts per (round, block) bucket for rounds of `nt` tiles; the old count is an entry's place inside its bucket.
    // *max_round = the staged values of the fullest round.
    int count_pass(int nt, int64_t *max_round)
    {
        const int64_t nblk = sb.nblk;
        stage_tiles = nt;
        make_rounds(nt);
        nround = nround_ls + 1;      // + the virtual round of the packed columns
        nb = nround * nblk;
        if (nb > sb.nb_max) return CSRK_ERR_INVALID;      // (cannot happen: a round holds at least LS_STAGE_TILES or NW tiles)
        CSRK_TRY(stage_h2d(d_rt0.p, h_rt0.data(), h_rt0.size() * 4, s));
        ls_tile_round_kernel<<<(unsigned)ceil_div(ls->n_tiles, 256), 256, 0, s>>>(d_rt0.as<int32_t>(), (int32_t)nround_ls, ls->n_tiles,
                                                                                tile_round.as<int32_t>());
        CSRK_LAUNCH_CHECK();
        CSRK_HIP(hipMemsetAsync(cnt.p, 0, (size_t)(nb + 1) * 4, s));
        ls_cold_count_kernel<<<(unsigned)ceil_div(n_words, 256), 256, 0, s>>>(ls->idx.as<uint32_t>(), n_words, (int32_t)nblk, (int32_t)sb.W,
                                                                            tile_round.as<int32_t>(), cnt.as<int32_t>(), off.as<int32_t>());
        CSRK_LAUNCH_CHECK();
        // the counts are 32-bit: total them in 64 bits before trusting the 32-bit scans
        CSRK_TRY(exclusive_scan_i32_to_i64(cnt.as<int32_t>(), tot.as<int64_t>(), nround_ls * nblk, s));
        std::vector<int64_t> rs((size_t)nround_ls + 1);
        DevBuf drs;
        CSRK_TRY(drs.alloc((size_t)(nround_ls + 1) * 8));
        ls_round_total_kernel<<<(unsigned)ceil_div(nround_ls + 1, 256), 256, 0, s>>>(tot.as<int64_t>(), (int32_t)nround_ls, (int32_t)nblk,
                                                                                   drs.as<int64_t>());
        CSRK_LAUNCH_CHECK();
        CSRK_TRY(stage_d2h(rs.data(), drs.p, (size_t)(nround_ls + 1) * 8, s));
        CSRK_HIP(hipStreamSynchronize(s));
        n_cold = rs[(size_t)nround_ls];
        *max_round = 0;
        for (int64_t r = 0; r < nround_ls; r++) *max_round = std::max(*max_round, rs[(size_t)r + 1] - rs[(size_t)r]);
        return CSRK_OK;
    }

    // where to start: the largest round size that fits by the tiles' own cold counts (then one count pass confirms it)
    int first_round_size(int *nt_first)
    {
        *nt_first = LS_RND_MAXTILES / NW * NW;
        DevBuf tcold, tpre;
        CSRK_TRY(tcold.alloc((size_t)(ls->n_tiles + 1) * 4));
        CSRK_TRY(tpre.alloc((size_t)(ls->n_tiles + 2) * 8));
        ls_tile_cold_kernel<<<(unsigned)ceil_div(ls->n_tiles * WAVE, 256), 256, 0, s>>>(ls->idx.as<uint32_t>(), ls->n_tiles,
                                                                                      tcold.as<int32_t>());
        CSRK_LAUNCH_CHECK();
        CSRK_TRY(exclusive_scan_i32_to_i64(tcold.as<int32_t>(), tpre.as<int64_t>(), ls->n_tiles, s));
        std::vector<int64_t> pre((size_t)ls->n_tiles + 1);
        CSRK_TRY(stage_d2h(pre.data(), tpre.p, pre.size() * 8, s));
        CSRK_HIP(hipStreamSynchronize(s));
        for (; *nt_first > NW; *nt_first -= NW) {
            make_rounds(*nt_first);
            int64_t mx = 0;
            for (int64_t r = 0; r < nround_ls; r++)
                mx = std::max(mx, pre[(size_t)h_rt0[(size_t)r + 1]] - pre[(size_t)h_rt0[(size_t)r]]);
            if (mx <= LS_RND_CAP) break;
        }
        return CSRK_OK;
    }

    // the largest rounds whose staged values fit the LDS round buffer (a round of one tile per wavefront always does)
    int choose_round_size(bool *fits)
    {
        *fits = false;
        int nt_first = 0;
        CSRK_TRY(first_round_size(&nt_first));
        for (int nt = nt_first; nt >= NW;) {
            int64_t max_round = 0;
            CSRK_TRY(count_pass(nt, &max_round));
            if (max_round <= LS_RND_CAP) {
                *fits = true;
                break;
            }
            nt = spmvlayout::next_round_size(nt, LS_RND_CAP, max_round, NW);
        }
        return CSRK_OK;
    }

    // the packed columns ride along as a virtual last round; then the counts in (block, round) order beside (round, block)
    int count_pack(const int32_t *hot_cols, int32_t n_hot)
    {
        const int64_t nblk = sb.nblk;
        CSRK_HIP(hipMemsetAsync(cnt.as<int32_t>() + nround_ls * nblk, 0, (size_t)(nblk + 1) * 4, s));
        ls_pack_count_kernel<<<(unsigned)ceil_div(n_hot, 256), 256, 0, s>>>(hot_cols, n_hot, (int32_t)sb.W,
                                                                           cnt.as<int32_t>() + nround_ls * nblk, offp.as<int32_t>());
        CSRK_LAUNCH_CHECK();
        CSRK_HIP(hipMemsetAsync(cntT.p, 0, (size_t)(nb + 1) * 4, s));
        ls_cold_transpose_kernel<<<(unsigned)ceil_div(nb, 256), 256, 0, s>>>(cnt.as<int32_t>(), (int32_t)nround, (int32_t)nblk,
                                                                           cntT.as<int32_t>());
        CSRK_LAUNCH_CHECK();
        return CSRK_OK;
    }

    // the stream's staging arrays: where every cold entry and packed column is copied from and to, the index words rewritten
    // to round offsets, the rounds' and blocks' starts
    int place(const int32_t *hot_cols, int32_t n_hot)
    {
        const int64_t nblk = sb.nblk, n_all = n_cold + n_hot;
        CSRK_TRY(exclusive_scan_i32(cnt.as<int32_t>(), cnt.as<int32_t>(), nb + 1, s));
        CSRK_TRY(exclusive_scan_i32(cntT.as<int32_t>(), cntT.as<int32_t>(), nb + 1, s));
        CSRK_TRY(ls->xg.alloc((size_t)(n_all + WAVE) * 8));      // (+ padding: the stream kernel's last pair of an odd count)
        CSRK_TRY(ls->a_col.alloc((size_t)n_all * 2));
        CSRK_TRY(ls->a_dst.alloc((size_t)n_all * 4));
        CSRK_TRY(ls->round_start.alloc((size_t)(nround_ls + 1) * 4));
        ls_round_start_kernel<<<(unsigned)ceil_div(nround_ls + 1, 256), 256, 0, s>>>(cnt.as<int32_t>(), (int32_t)nround_ls, (int32_t)nblk,
                                                                                   ls->round_start.as<int32_t>());
        CSRK_LAUNCH_CHECK();
        CSRK_TRY(ls->round_tile0.alloc(h_rt0.size() * 4));
        CSRK_TRY(ls->wg_round0.alloc(h_wr0.size() * 4));
        CSRK_TRY(stage_h2d(ls->round_tile0.p, h_rt0.data(), h_rt0.size() * 4, s));
        CSRK_TRY(stage_h2d(ls->wg_round0.p, h_wr0.data(), h_wr0.size() * 4, s));
        ls_cold_place_kernel<<<(unsigned)ceil_div(n_words, 256), 256, 0, s>>>(ls->idx.as<uint32_t>(), n_words, (int32_t)nround, (int32_t)nblk,
                                                                            (int32_t)sb.W, tile_round.as<int32_t>(), 1, cnt.as<int32_t>(),
                                                                            cntT.as<int32_t>(), off.as<int32_t>(), ls->a_col.as<uint16_t>(),
                                                                            ls->a_dst.as<int32_t>());
        CSRK_LAUNCH_CHECK();
        ls_pack_place_kernel<<<(unsigned)ceil_div(n_hot, 256), 256, 0, s>>>(hot_cols, n_hot, (int32_t)sb.W, (int32_t)nround,
                                                                           cntT.as<int32_t>(), offp.as<int32_t>(), (int32_t)n_cold,
                                                                           ls->a_col.as<uint16_t>(), ls->a_dst.as<int32_t>());
        CSRK_LAUNCH_CHECK();
        CSRK_TRY(ls->blk_start.alloc((size_t)(nblk + 1) * 4));
        ls_stage_starts_kernel<<<(unsigned)ceil_div(nblk + 1, 256), 256, 0, s>>>(cntT.as<int32_t>(), (int32_t)nround, (int32_t)nblk,
                                                                                ls->blk_start.as<int32_t>());
        CSRK_LAUNCH_CHECK();
        ls->n_stage_blk = (int32_t)nblk;
        ls->stage_w = (int32_t)sb.W;
        CSRK_TRY(spmv_kernel_attributes());
        return CSRK_OK;
    }

    // every column field is now a pack slot (< n_hot) or an offset into a round's staged values (< LS_RND_CAP): 3-byte words
    int narrow_words(int32_t n_hot)
    {
        DevBuf idx24;
        const bool narrow = CSRK_LS_IDX24 && (int64_t)n_hot < (int64_t)LS24_COL_MASK && (int64_t)LS_RND_CAP < (int64_t)LS24_COL_MASK;
        if (narrow) {
            CSRK_TRY(idx24.alloc((size_t)ls->n_tiles * LS24_TILE_BYTES));
            ls_idx24_kernel<<<(unsigned)ceil_div(ls->n_tiles * WAVE, 256), 256, 0, s>>>(ls->idx.as<uint32_t>(), ls->n_tiles,
                                                                                       idx24.as<unsigned char>());
            CSRK_LAUNCH_CHECK();
        }
        CSRK_HIP(hipStreamSynchronize(s));      // the temporaries are freed on return
        if (narrow) {
            ls->idx.release();
            ls->idx.p = idx24.take();
            ls->idx.bytes = (size_t)ls->n_tiles * LS24_TILE_BYTES;
            ls->idx24 = true;
        }
        return CSRK_OK;
    }
};

static int build_cold_stage(Matrix *m, LightStream *ls, const int32_t *hot_cols, int32_t n_hot, const SpmvKnobs &knobs, hipStream_t s)
{
    ls->idx24 = false;
    ls->n_cold = 0;
    ls->stage_tiles = 0;
    ls->n_rounds = 0;
    ls->max_wg_rounds = 0;
    if (knobs.ls_stage == 0) return CSRK_OK;
    ColdStage C;
    C.ls = ls;
    C.s = s;
    C.n_words = ls->n_tiles * ACC_TILE;
    int cus = 0;
    CSRK_TRY(device_cus(m, &cus));
    C.sb = spmvlayout::stage_blocks(m->ncols, cus, LS_STAGE_WMAX, ls->n_tiles,
                                    LS_STAGE_TILES < ColdStage::NW ? LS_STAGE_TILES : ColdStage::NW, ls->grid);
    if (C.sb.nb_max < 1 || C.sb.nb_max > (int64_t)1 << 26) return CSRK_OK;
    size_t mfree = 0, mtotal = 0;
    CSRK_HIP(hipMemGetInfo(&mfree, &mtotal));
    if (!spmvlayout::stage_temps_fit(C.n_words, C.sb.nb_max, mfree)) return CSRK_OK;
    if (ls->n_tiles >= INT32_MAX) return CSRK_OK;
    PlanTrace tr(knobs);
    CSRK_TRY(C.alloc(n_hot));
    bool fits = false;
    CSRK_TRY(C.choose_round_size(&fits));
    if (!fits) return CSRK_OK;
    tr.lap("  cold: round size (count passes)");
    if (C.nround > INT32_MAX) return CSRK_OK;
    CSRK_TRY(C.count_pack(hot_cols, n_hot));
    // worth a pass of its own only when the cold columns cannot live in L2 anyway and there are enough of them
    if (C.n_cold < 1 || C.n_cold + n_hot >= (int64_t)LS_PAD || (knobs.ls_stage != 1 && !spmvlayout::cold_stage_pays(C.n_cold, C.n_words)))
        return CSRK_OK;
    CSRK_TRY(C.place(hot_cols, n_hot));
    CSRK_TRY(C.narrow_words(n_hot));
    ls->n_cold = C.n_cold;
    ls->stage_tiles = C.stage_tiles;
    ls->n_rounds = (int32_t)C.nround_ls;
    for (size_t w = 0; w + 1 < C.h_wr0.size(); w++) ls->max_wg_rounds = std::max(ls->max_wg_rounds, C.h_wr0[w + 1] - C.h_wr0[w]);
    tr.lap("  cold: place, 3-byte words");
    return CSRK_OK;
}

// Dense rows: when few rows of the view are empty (rows without entries, rows cut out for the tiers: 7 % on the
// headline matrix) each of them gets ONE padding entry, so every row has a run, run k IS row k, and the stream kernel
// neither loads row ids (4 loads per tile: 12 of its 170 us) nor clears gaps.  rpd = the view's pointers with empty
// rows widened to one slot (left empty where spmvlayout::dense_rows_pay says no); *n_pad = the view's empty rows.
template <class P>
static int dense_row_pointers(Matrix *m, const P *rpv, int64_t n_view, DevBuf &rpd, int64_t *n_pad, hipStream_t s)
{
    DevBuf nz;
    CSRK_TRY(nz.alloc((size_t)(m->nrows + 2) * 4));
    ls_rowflag_kernel<P><<<(unsigned)ceil_div((int64_t)m->nrows + 1, 256), 256, 0, s>>>(rpv, m->nrows, nz.as<int32_t>());
    CSRK_LAUNCH_CHECK();
    CSRK_TRY(exclusive_scan_i32(nz.as<int32_t>(), nz.as<int32_t>(), m->nrows, s));
    int32_t n_nonempty = 0;
    CSRK_TRY(stage_d2h(&n_nonempty, nz.as<int32_t>() + m->nrows, 4, s));
    CSRK_HIP(hipStreamSynchronize(s));
    *n_pad = (int64_t)m->nrows - n_nonempty;
    if (spmvlayout::dense_rows_pay(n_view, *n_pad, sizeof(P) == 8)) {
        CSRK_TRY(rpd.alloc((size_t)(m->nrows + 1) * sizeof(P)));
        ls_dense_ptr_kernel<P><<<(unsigned)ceil_div((int64_t)m->nrows + 1, 256), 256, 0, s>>>(rpv, nz.as<int32_t>(), m->nrows, rpd.as<P>());
        CSRK_LAUNCH_CHECK();
    }
    CSRK_HIP(hipStreamSynchronize(s));      // nz is released here
    return CSRK_OK;
}

// Copy the rows of the row-major path (the light view, or the whole matrix when nothing was cut out) into
// the light stream.  Built with the lazy plan.  Skipped (the tile kernel stays in charge) when ncols needs
// the two flag bits, when the copy does not fit in device memory, or with CSRK_SPMV_STREAM=0.
template <class P, int VT>
static int build_light_stream(Matrix *m, SpmvPlan *p, const SpmvKnobs &knobs, hipStream_t s)
{
    p->ls.on = false;
    if (knobs.stream == 0) return CSRK_OK;
    const bool force = knobs.stream == 1;
    const int64_t n_view = p->n_heavy ? p->nnz_light : m->nnz;
    if (m->nrows == 0 || n_view < 1 || (int64_t)m->ncols > (int64_t)LS_COL_MASK) return CSRK_OK;
    // Without long rows cut out and without a popularity skew worth packing, the gathers are either local
    // (banded: the tile kernel's entry-per-lane order coalesces them better: 0.526 vs 0.638 ms measured) or
    // all equally cold (uniform random columns: both kernels run at the 128-B-per-gather fabric rate), and
    // the stream's copy of the matrix buys nothing.
    if (!p->n_heavy && !p->n_hot && !force) return CSRK_OK;
    const P *rp = (const P *)m->d_rowptrs;
    const P *rpv = p->n_heavy ? p->rp_light.as<P>() : rp;
    const int32_t *slot_map = p->n_hot ? p->hot_slot.as<int32_t>() : (const int32_t *)nullptr;
    size_t mfree = 0, mtotal = 0;
    CSRK_HIP(hipMemGetInfo(&mfree, &mtotal));
    if (!spmvlayout::stream_copy_fits(ceil_div(n_view, ACC_TILE), ACC_TILE, m->nrows, mfree) && !force) return CSRK_OK;
    DevBuf rpd_buf;
    int64_t n_pad = 0;
    CSRK_TRY(dense_row_pointers<P>(m, rpv, n_view, rpd_buf, &n_pad, s));
    const P *rp_dense = rpd_buf.p ? rpd_buf.as<P>() : (const P *)nullptr;
    const int64_t n_ent = rp_dense ? n_view + n_pad : n_view;
    CSRK_TRY((build_stream<P, VT>(m, &p->ls, rp, rp_dense ? rp_dense : rpv, m->nrows, m->d_colinds, m->d_values, n_ent,
                                  ceil_div(n_ent, ACC_TILE), m->nrows, slot_map, knobs, s, rp_dense ? rpv : (const P *)nullptr)));
    if (p->ls.on && p->n_hot) {
        CSRK_TRY(build_cold_stage(m, &p->ls, p->hot_cols.as<int32_t>(), p->n_hot, knobs, s));
        // (round-in-LDS form: the round's staged values take the place of the hot window's tail)
        if (p->ls.n_cold && p->ls.round_start.p && p->n_hot_lds > LS_RND_HOT) p->n_hot_lds = LS_RND_HOT;
    }
    return CSRK_OK;
}

// ---- the plans: merge (with the lazy plan's split, pack and streams) and vector -------------------
template <class P>
static int build_merge_plan(Matrix *m, SpmvPlan *p, const SpmvKnobs &knobs, hipStream_t s, bool allow_split)
{
    const P *rp = (const P *)m->d_rowptrs;
    p->tile_items = MERGE_ITEMS;
    p->nnz_light = m->nnz;
    p->split_considered = allow_split;
    PlanTrace tr(knobs);
    if (allow_split) CSRK_TRY(build_heavy_split<P>(m, p, knobs, s));
    tr.lap("heavy split");
    const P *rp_path = p->n_heavy ? p->rp_light.as<P>() : rp;
    int64_t total = (int64_t)m->nrows + p->nnz_light;
    p->n_tiles = ceil_div(total, MERGE_ITEMS);
    CSRK_TRY(p->tile_row.alloc((size_t)(p->n_tiles + 1) * 4));
    CSRK_TRY(p->carry_row.alloc((size_t)p->n_tiles * 4));
    CSRK_TRY(p->carry_val.alloc((size_t)p->n_tiles * 8));
    int64_t nthr = p->n_tiles + 1;
    merge_plan_kernel<P><<<(unsigned)ceil_div(nthr, 256), 256, 0, s>>>(rp_path, m->nrows, p->nnz_light, MERGE_ITEMS,
                                                                      p->n_tiles, p->tile_row.as<int32_t>());
    CSRK_LAUNCH_CHECK();
    if (p->n_heavy) {
        CSRK_TRY(p->tile_cut.alloc((size_t)(p->n_tiles + 1) * 4));
        heavy_tilecut_kernel<<<(unsigned)ceil_div(nthr, 256), 256, 0, s>>>(
            p->tile_row.as<int32_t>(), p->n_tiles, MERGE_ITEMS, total, p->cut_pos.as<int64_t>(), p->n_heavy,
            p->tile_cut.as<int32_t>());
        CSRK_LAUNCH_CHECK();
    }
    tr.lap("merge-path tables");
    if (!allow_split) return CSRK_OK;
    CSRK_TRY(build_hot_cache<P>(m, p, knobs, s));
    tr.lap("hot-column census + pack");
    CSRK_TRY(build_tiers<P>(m, p, knobs, s));
    tr.lap("tiers");
    CSRK_TRY(with_val_type(m->val_type, [&](auto vt) -> int { return build_light_stream<P, decltype(vt)::value>(m, p, knobs, s); }));
    tr.lap("light stream + cold staging");
    if (p->n_hot && !p->ls.on) {        // no stream (no memory for it, CSRK_SPMV_STREAM=0): the tile kernel reads x itself
        p->n_hot = 0;
        p->hot_cols.release();
        p->xh.release();
    }
    p->hot_slot.release();
    return CSRK_OK;
}

template <class P>
static int build_vector_plan(Matrix *m, SpmvPlan *p, hipStream_t s)
{
    const P *rp = (const P *)m->d_rowptrs;
    CSRK_TRY(p->seg_off.alloc((size_t)(m->nrows + 1) * 8));
    if (m->nrows > 0) {
        vec_count_kernel<P><<<(unsigned)ceil_div(m->nrows, 256), 256, 0, s>>>(rp, m->nrows, p->seg_off.as<int64_t>());
        CSRK_LAUNCH_CHECK();
    }
    CSRK_TRY(exclusive_scan_i64(p->seg_off.as<int64_t>(), p->seg_off.as<int64_t>(), m->nrows, s));
    int64_t n_segs = 0;
    CSRK_TRY(stage_d2h(&n_segs, p->seg_off.as<int64_t>() + m->nrows, 8, s));
    CSRK_HIP(hipStreamSynchronize(s));
    p->n_segs = n_segs;
    CSRK_TRY(p->seg_row.alloc((size_t)n_segs * 4));
    CSRK_TRY(p->seg_part.alloc((size_t)n_segs * 8));
    if (m->nrows > 0) {
        vec_fill_kernel<<<(unsigned)ceil_div(m->nrows, 256), 256, 0, s>>>(p->seg_off.as<int64_t>(), m->nrows,
                                                                         p->seg_row.as<int32_t>());
        CSRK_LAUNCH_CHECK();
    }
    return CSRK_OK;
}

template <class P>
static int build_plan(Matrix *m, SpmvPlan *p, hipStream_t s, bool allow_split)
{
    const SpmvKnobs knobs = read_spmv_knobs();      // once per build: the builders read no environment
    if (p->algo == CSRK_SPMV_MERGE) return build_merge_plan<P>(m, p, knobs, s, allow_split);
    if (p->algo == CSRK_SPMV_VECTOR) return build_vector_plan<P>(m, p, s);
    return CSRK_OK;
}

int build_spmv_plan(Matrix *m, SpmvPlan *p, bool allow_split)
{
    return m->ptr64 ? build_plan<int64_t>(m, p, nullptr, allow_split) : build_plan<int32_t>(m, p, nullptr, allow_split);
}

}  // namespace csrk
