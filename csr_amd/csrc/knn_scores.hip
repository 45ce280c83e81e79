// Scoring from an item-kNN model for libcsrk on gfx950: csrk_knn_scores walks each target's neighbour list in storage order,
// takes the first max_nbrs neighbours the user has rated and gives their similarity-weighted average rating (or the sum of
// the similarities) as a canonical CSR [listed rows x targets].  The contract is in include/csrk.h.
//
// The grid is (listed rows) x (runs of consecutive tiles of KS_TILE targets), one KS_THREADS-thread workgroup each; a run is
// one tile until the call has more than KS_WGS_FILL (row, tile) pairs, then up to KS_TILES_MAX (the row is staged once per run):
//   stage   the user's rating row -- columns and widened values -- goes into LDS when it holds at most KS_LDS_ROW entries;
//           a longer row is searched where it lies, in device memory, with the same comparisons and so the same bits.
//           Beside it a filter of KS_BITS bits: bit (column mod KS_BITS) is set for every rated column.
//   filter  a model entry whose bit is clear is a miss without a search -- nearly all are (a user has rated a few hundred
//           of tens of thousands of items) -- and a step in which no lane of the wavefront has a set bit ends there.
//   walk    a group of KS_LANES lanes takes one target (a kNN model row holds tens of entries).  Per step the group loads
//           KS_LANES consecutive model entries (coalesced), every lane looks its column up in the rating row by binary
//           search, the group ballots the hits, and EVERY lane of the group folds the hit lanes' entries in ascending lane
//           order -- a serial loop over the set bits, the values fetched by shuffle.  Ascending lane order inside a step and
//           ascending steps is storage order: the order of the additions and the place of the cut at max_nbrs are those of
//           the contract by construction.  Nothing inside a walk is summed in parallel.
//           A walk is a chain of dependent loads -- row pointers, the model entry, the filter word, then ~log2(row) probes
//           where the bit is set -- so a group takes KS_ILP targets side by side (KS_GROUPS x KS_ILP targets per round,
//           KS_TILE / that rounds) and their loads are in flight together.  The search has the same number of steps in
//           every lane (it halves a range whose length only depends on the row), so a wavefront never diverges in it.
//           The model's value is loaded by the hit lanes only.  (What each of these bought: DESIGN.md section 8g.)
//   rank    the tile's KS_TILE flags (nn >= min_nbrs) lie in LDS; a ballot and the wavefront totals give every stored target
//           its rank in the tile.
// Two passes that both walk: COUNT writes one count per (listed row, tile), scan_total runs over them, the row pointers are
// the offsets at tile 0, and PLACE repeats the walk for the tiles that store something and writes at offset + rank.  Every
// slot is counted; nothing is appended in arrival order and there is no atomic on a result.
//
// LDS: KS_LDS_ROW x 12 bytes of rating row + KS_BITS / 8 bytes of filter + KS_TILE x 12 bytes of flags and values = 35 KiB
// per workgroup, so four workgroups (16 wavefronts) fit the 160 KiB of a CU -- as many as the PLACE kernel's registers allow
// (between 64 and 128 VGPRs: 4 wavefronts per SIMD): the walk is chains of dependent loads, and what hides them is other wavefronts.  A
// bound of 4096 entries (59 KiB) would leave two workgroups per CU; rating rows above 2048 entries are rare in the data this
// serves and the device-memory search takes them.
// Column indices are compared, never used as addresses; every wavefront stays whole inside the loops that ballot and shuffle.
#include "device_loads.h"
#include "result.h"
#include "sort.h"

#include <functional>

namespace csrk {

constexpr int KS_LANES = 16;                    // lanes that share one target's walk = model entries per step
constexpr int KS_THREADS = 256;
constexpr int KS_GROUPS = KS_THREADS / KS_LANES;
constexpr int KS_TILE = 256;                    // targets of a workgroup tile (= KS_THREADS: one flag per thread in the rank step)
constexpr int KS_LDS_ROW = 2048;                // entries of a rating row held in LDS
constexpr int KS_ILP = 4;                       // targets a group walks side by side
constexpr int KS_BITS = 1 << 16;                // bits of the rated-column filter (a power of two; 8 KiB of LDS)
constexpr int KS_NW = KS_THREADS / WAVE;
constexpr int KS_TILES_MAX = 16;                // most tiles one workgroup takes (its rating row is staged once for all of them) ...
constexpr int64_t KS_WGS_FILL = 4096;           // ... as long as about this many workgroups are left: 4 per CU, 4 times over (256 CUs)
constexpr int64_t KS_GRID_MAX = 0x7fffffffll;
static_assert(KS_TILE == KS_THREADS && KS_TILE % (KS_GROUPS * KS_ILP) == 0 && WAVE % KS_LANES == 0,
              "the rank step takes one target per thread; whole rounds of KS_GROUPS x KS_ILP targets");

struct KsArgs {
    const void *rpm, *rpr;              // row pointers of the model and of the ratings (pm64 / pr64)
    const int32_t *cm, *cr;
    const void *vm, *vr;                // values (vtm / vtr: CSRK_VAL_*)
    int pm64, pr64, vtm, vtr, aggregate;
    int32_t n_targets, max_nbrs, min_nbrs;
    int64_t n_tiles, tiles_per_wg;      // tiles of KS_TILE targets in all; consecutive tiles one workgroup takes
    const int32_t *rows;                // the listed rows (device copy; checked on the host)
    const double *offsets;              // NULL or one per listed row (device copy)
    int64_t *cnt;                       // COUNT: one per (listed row, tile)
    const int64_t *off;                 // PLACE: their exclusive scan
    int32_t *oc;
    double *ov;
};

// The filter in front of the search: one bit per residue of the column modulo KS_BITS, set for every column of the rating
// row.  A clear bit says the column is not rated; a set bit says "search".  (c & mask is a residue for any int32, so a
// column index is still never an address.)
__device__ __forceinline__ uint32_t ks_slot(int32_t c) { return (uint32_t)c & (uint32_t)(KS_BITS - 1); }
__device__ __forceinline__ bool ks_bit(const uint32_t *s_bits, int32_t c) { return (s_bits[ks_slot(c) >> 5] >> (ks_slot(c) & 31)) & 1u; }

struct KsRow {                        // the user's rating row where it lies in device memory
    const int32_t *cols;
    const void *vals;
    int64_t start;
    uint32_t len;                       // >= 1
};

// The walks of one round: every group of KS_LANES lanes takes the KS_ILP targets tgt[] (a negative one is no target: an empty
// walk) side by side and leaves, in every lane of the group, their sums and hit counts.  The targets' walks do not depend on
// each other, so their model loads and their filter tests are in flight together.  The one routine both routes walk with
// (knn_scores_kernel: the targets of a tile; knn_reach_kernel: the candidates its marks name), so their bits agree by
// construction.  Every thread of the workgroup calls it: the wavefront stays whole in the loops that ballot and shuffle.
template <bool STAGED>
__device__ __forceinline__ void ks_fold(const KsArgs &g, const KsRow &row, const uint32_t *s_bits, const int32_t *s_cols,
                                        const double *s_vals, const int64_t (&tgt)[KS_ILP], double (&num)[KS_ILP],
                                        double (&den)[KS_ILP], int32_t (&nn)[KS_ILP])
{
    // every multiply, add and divide below is rounded on its own (rule 2 of the contract): see csrc/combine.hip, cb_row
#pragma clang fp contract(off)
    const int t = threadIdx.x, lane = t & (WAVE - 1);
    const int sub = t & (KS_LANES - 1), gshift = lane & ~(KS_LANES - 1);
    const bool average = g.aggregate == CSRK_KNN_WEIGHTED_AVERAGE;
    const uint32_t lr = row.len;
    auto col_at = [&](uint32_t p) { return STAGED ? s_cols[p] : row.cols[p]; };
    int64_t ms[KS_ILP];
    uint32_t len[KS_ILP];
    bool done[KS_ILP];
#pragma unroll
    for (int j = 0; j < KS_ILP; j++) {
        const int64_t i = tgt[j];
        ms[j] = 0, len[j] = 0;
        if (i >= 0) {
            ms[j] = load_ptr(g.rpm, g.pm64, i);
            len[j] = (uint32_t)(load_ptr(g.rpm, g.pm64, i + 1) - ms[j]);
        }
        num[j] = 0.0, den[j] = 0.0, nn[j] = 0, done[j] = false;
    }
    for (uint32_t base = 0;; base += KS_LANES) {             // (base < len <= 2^31 - 1: base + sub does not wrap)
        bool live = false;
#pragma unroll
        for (int j = 0; j < KS_ILP; j++) live |= base < len[j] && !done[j];
        if (!__any(live)) break;
        const uint32_t e = base + sub;
        int32_t c[KS_ILP];
        bool maybe[KS_ILP];
#pragma unroll
        for (int j = 0; j < KS_ILP; j++) {                   // KS_ILP independent loads, then KS_ILP independent bit tests
            const bool in = !done[j] && e < len[j];
            c[j] = in ? g.cm[ms[j] + e] : 0;
            maybe[j] = in;
        }
#pragma unroll
        for (int j = 0; j < KS_ILP; j++) maybe[j] = maybe[j] && ks_bit(s_bits, c[j]);
#pragma unroll
        for (int j = 0; j < KS_ILP; j++) {
            if (!__any(maybe[j])) continue;                  // (the whole wavefront: most steps end here, without a search)
            // the last entry of the rating row that is not above c, if there is one: the range [lo, lo + n) holds it; n
            // shrinks the same way in every lane and the probes stay in [0, lr) whatever c is
            uint32_t lo = 0;
            for (uint32_t n = lr; n > 1;) {
                const uint32_t half = n >> 1;
                if (col_at(lo + half) <= c[j]) lo += half;
                n -= half;
            }
            const bool hit = maybe[j] && col_at(lo) == c[j];
            double s = 0.0, v = 0.0;
            if (hit) {
                s = csr_val(g.vm, g.vtm, ms[j] + e);
                if (average) v = STAGED ? s_vals[lo] : csr_val(row.vals, g.vtr, row.start + lo);
            }
            uint32_t bits = (uint32_t)(__ballot(hit) >> gshift) & ((1u << KS_LANES) - 1);
            while (__any(bits != 0)) {                       // the whole wavefront shuffles; a group with no bit left idles
                const bool act = bits != 0;
                const int src = gshift + (act ? __ffs(bits) - 1 : 0);
                const double sl = __shfl(s, src), vl = __shfl(v, src);
                if (act) {
                    if (average) {
                        const double p = vl * sl;
                        num[j] = num[j] + p;
                        den[j] = den[j] + fabs(sl);
                    } else {
                        num[j] = num[j] + sl;
                    }
                    nn[j]++;
                    bits &= bits - 1;
                    if (g.max_nbrs > 0 && nn[j] == g.max_nbrs) {
                        done[j] = true;
                        bits = 0;
                    }
                }
            }
        }
    }
}

// a target's value from its sums (rule 3 of the contract): one division, then the listed row's offset
__device__ __forceinline__ double ks_score_of(const KsArgs &g, int64_t r, double num, double den)
{
#pragma clang fp contract(off)
    double x = g.aggregate == CSRK_KNN_WEIGHTED_AVERAGE ? num / den : num;
    if (g.offsets) x = x + g.offsets[r];
    return x;
}

// The walks of one tile: KS_TILE / (KS_GROUPS KS_ILP) rounds, in each of which every group takes KS_ILP targets side by side.
template <bool PLACE, bool STAGED>
__device__ __forceinline__ void ks_walk(const KsArgs &g, const KsRow &row, int64_t r, int64_t tile_base, const uint32_t *s_bits,
                                        const int32_t *s_cols, const double *s_vals, double *s_score, int32_t *s_flag)
{
    const int t = threadIdx.x, grp = t / KS_LANES, sub = t & (KS_LANES - 1);
    for (int k = 0; k < KS_TILE / (KS_GROUPS * KS_ILP); k++) {
        int64_t tgt[KS_ILP];
        double num[KS_ILP], den[KS_ILP];
        int32_t nn[KS_ILP];
#pragma unroll
        for (int j = 0; j < KS_ILP; j++) {
            const int64_t i = tile_base + (k * KS_ILP + j) * KS_GROUPS + grp;
            tgt[j] = i < g.n_targets ? i : -1;
        }
        ks_fold<STAGED>(g, row, s_bits, s_cols, s_vals, tgt, num, den, nn);
        if (sub == 0) {
#pragma unroll
            for (int j = 0; j < KS_ILP; j++) {
                const int q = (k * KS_ILP + j) * KS_GROUPS + grp;
                s_flag[q] = nn[j] >= g.min_nbrs ? 1 : 0;
                if (PLACE) s_score[q] = ks_score_of(g, r, num[j], den[j]);
            }
        }
    }
}

template <bool PLACE>
__global__ __launch_bounds__(KS_THREADS) void knn_scores_kernel(const KsArgs g, int64_t first_block)
{
    __shared__ int32_t s_cols[KS_LDS_ROW];
    __shared__ double s_vals[KS_LDS_ROW];
    __shared__ double s_score[KS_TILE];
    __shared__ int32_t s_flag[KS_TILE];
    __shared__ uint32_t s_tot[KS_NW];
    __shared__ uint32_t s_bits[KS_BITS / 32];
    // workgroup (r, q) takes the tiles [q tpw, (q + 1) tpw) of listed row r
    const int64_t wg = first_block + blockIdx.x, n_runs = (g.n_tiles + g.tiles_per_wg - 1) / g.tiles_per_wg;
    const int64_t r = wg / n_runs, tile0 = (wg - r * n_runs) * g.tiles_per_wg;
    const int64_t tile1 = tile0 + g.tiles_per_wg < g.n_tiles ? tile0 + g.tiles_per_wg : g.n_tiles;
    if (PLACE && g.off[r * g.n_tiles + tile1] == g.off[r * g.n_tiles + tile0]) return;      // (the whole workgroup: nothing is stored)
    const int t = threadIdx.x, lane = t & (WAVE - 1), w = t / WAVE;
    const int32_t u = g.rows[r];
    const int64_t rs = load_ptr(g.rpr, g.pr64, u);
    const uint32_t lr = (uint32_t)(load_ptr(g.rpr, g.pr64, (int64_t)u + 1) - rs);
    const bool staged = lr <= (uint32_t)KS_LDS_ROW;
    const bool average = g.aggregate == CSRK_KNN_WEIGHTED_AVERAGE;
    const int32_t *__restrict__ gcols = g.cr + rs;
    for (int x = t; x < KS_BITS / 32; x += KS_THREADS) s_bits[x] = 0;
    __syncthreads();
    for (uint32_t j = t; j < lr; j += KS_THREADS) {
        const int32_t c = gcols[j];
        atomicOr(&s_bits[ks_slot(c) >> 5], 1u << (ks_slot(c) & 31));      // (an integer OR in LDS: its order changes nothing)
        if (staged) {
            s_cols[j] = c;
            if (average) s_vals[j] = csr_val(g.vr, g.vtr, rs + j);
        }
    }
    __syncthreads();
    for (int64_t tile = tile0; tile < tile1; tile++) {
        const int64_t blk = r * g.n_tiles + tile, tile_base = tile * KS_TILE;
        if (PLACE && g.off[blk + 1] == g.off[blk]) continue;     // (the whole workgroup: nothing of this tile is stored)
        if (lr == 0) {
            s_flag[t] = 0;                                       // no rating, no hit: the tile stores nothing
        } else {
            const KsRow row{gcols, g.vr, rs, lr};
            if (staged)
                ks_walk<PLACE, true>(g, row, r, tile_base, s_bits, s_cols, s_vals, s_score, s_flag);
            else
                ks_walk<PLACE, false>(g, row, r, tile_base, s_bits, s_cols, s_vals, s_score, s_flag);
        }
        __syncthreads();
        // thread t takes target tile_base + t: its rank among the tile's stored targets
        const bool f = s_flag[t] != 0;
        const unsigned long long bal = __ballot(f);
        uint32_t pre = (uint32_t)__popcll(bal & (lane ? (~0ull >> (WAVE - lane)) : 0ull));
        if (lane == 0) s_tot[w] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t tot = 0;
#pragma unroll
        for (int x = 0; x < KS_NW; x++) {
            const uint32_t n = s_tot[x];
            if (x < w) pre += n;
            tot += n;
        }
        if (!PLACE) {
            if (t == 0) g.cnt[blk] = tot;
        } else if (f) {
            const int64_t o = g.off[blk] + pre;
            g.oc[o] = (int32_t)(tile_base + t);
            g.ov[o] = s_score[t];
        }
        __syncthreads();                                         // (the next tile writes s_flag, s_score and s_tot again)
    }
}

// ---- the reach route: walk only the targets a user's ratings reach -------------------------------------------------------------
// A target i has a hit for user u exactly when some item j that u rated is stored in model row i, that is when i lies in row j
// of the transpose of the model's pattern -- the REACH INDEX the model handle keeps (Matrix::knn_reach; row j: the targets
// whose model row stores column j, ascending, once per stored occurrence).  One workgroup takes one (listed row, range of KR_R
// targets) pair:
//   mark       KR_R bits in LDS, zeroed; for every rated item j a lower bound finds the first entry of reach row j that is not
//              below the range's base and bit (target - base) is set for the entries below base + KR_R.  Thread t looks up rated
//              item t of KS_THREADS at a time; the lanes of a group then take the group's KS_LANES reach rows one after the other,
//              KS_LANES entries per step (a kNN model's reach rows hold tens of entries), and a reach row with more than KR_LONG
//              entries at or above the base (a popular item) is left to the whole wavefront, WAVE entries per step.  Integer ORs
//              in LDS: their order changes nothing.
//   enumerate  the candidates are the set bits in ascending target order: thread t counts the bits of its KR_WPT consecutive words, a
//              workgroup scan gives every word the number of candidates before it, and candidate q is found by a search over
//              those prefixes and a select inside its word.  Nothing is appended in arrival order; no counter hands out slots.
//   walk       KR_ROUND = KS_GROUPS x KS_ILP candidates per round, through ks_fold: the same filter, search and fold as the
//              walk-all route.  The round's flags (nn >= min_nbrs) are ranked by one ballot of the first wavefront, which carries
//              the number stored so far: ranks ascend with the target.
// min_nbrs >= 1, so every stored target is a candidate; with min_nbrs == 1 every candidate is stored (the cut at max_nbrs
// cannot take nn below 1) and COUNT is the popcount of the marks, with no rating row staged and no walk (knn_reach_marks_kernel).
// LDS of the walking kernel: the 32 KiB of staged row and filter + KR_R / 8 bytes of marks + KR_R / 8 bytes of prefixes + the
// round's flags, targets and values = 34 KiB: four workgroups per CU, as the walk-all route.  KR_R is small because a workgroup
// walks its range's candidates one round after the other: a user who rated thousands of items reaches nearly every target, and
// the ranges are what spreads that user over the card (DESIGN.md section 8h has the ranges tried).
#ifndef CSRK_KR_R
#define CSRK_KR_R 4096
#endif
constexpr int KR_R = CSRK_KR_R;                   // targets of a range = bits of the mark bitmap (a power of two, a multiple of 32)
constexpr int KR_WORDS = KR_R / 32;
constexpr int KR_WPT = (KR_WORDS + KS_THREADS - 1) / KS_THREADS;      // words of the bitmap a thread counts in the scan
constexpr int KR_ROUND = KS_GROUPS * KS_ILP;      // candidates a workgroup walks per round
constexpr int KR_LONG = 256;                      // a reach row with more entries at or above the base goes to the whole wavefront
static_assert(KR_ROUND == WAVE && (KR_R & (KR_R - 1)) == 0 && KR_R % 32 == 0 && KR_R <= 65536,
              "one wavefront ranks a round; whole words; the candidates of a range fit the prefixes");

struct KrArgs {
    KsArgs g;
    const void *tp;                     // the reach index: row pointers (tp64), one row per item ...
    const int32_t *ti;                  // ... and its entries, the targets
    int tp64;
    int32_t n_items;
    int64_t n_ranges;                   // ranges of KR_R targets per listed row
};

__device__ __forceinline__ void kr_set(uint32_t *s_mark, int64_t i, int64_t base)
{
    const uint64_t b = (uint64_t)(i - base);
    if (b < (uint64_t)KR_R) atomicOr(&s_mark[b >> 5], 1u << (b & 31));      // (an integer OR in LDS: its order changes nothing)
}

// mark: s_mark is zero and the workgroup is whole on entry; the caller synchronises afterwards
__device__ __forceinline__ void kr_mark(const KrArgs &a, const int32_t *__restrict__ gcols, uint32_t lr, int64_t base, uint32_t *s_mark)
{
    const int t = threadIdx.x, lane = t & (WAVE - 1), sub = t & (KS_LANES - 1), gshift = lane & ~(KS_LANES - 1);
    const int64_t top = base + KR_R;
    const int32_t *__restrict__ ti = a.ti;
    for (uint32_t jb = 0; jb < lr; jb += KS_THREADS) {           // (the same trip count in every thread)
        // this thread's rated item: the part [lo, end) of its reach row that is not below the base.  A column outside
        // [0, n_items) reaches nothing -- which is what the walk finds -- and is never an address.
        int64_t lo = 0, end = 0;
        if (jb + t < lr) {
            const int32_t j = gcols[jb + t];
            if (j >= 0 && j < a.n_items) {
                lo = load_ptr(a.tp, a.tp64, j);
                end = load_ptr(a.tp, a.tp64, (int64_t)j + 1);
                for (int64_t n = end - lo; n > 0;) {             // the first entry that is not below base (reach rows ascend)
                    const int64_t half = n >> 1;
                    if (ti[lo + half] < base) {
                        lo += half + 1;
                        n -= half + 1;
                    } else {
                        n = half;
                    }
                }
            }
        }
        const bool is_long = end - lo > KR_LONG;
        for (int k = 0; k < KS_LANES; k++) {                     // the group's reach rows, one after the other
            const int64_t l = __shfl(lo, gshift + k), e = __shfl(end, gshift + k);
            if (e - l <= KR_LONG) {
                for (int64_t p = l + sub; p < e; p += KS_LANES) {
                    const int64_t i = ti[p];
                    if (i >= top) break;
                    kr_set(s_mark, i, base);
                }
            }
        }
        for (unsigned long long longs = __ballot(is_long); longs; longs &= longs - 1) {      // (the same in every lane)
            const int src = __ffsll(longs) - 1;
            const int64_t l = __shfl(lo, src), e = __shfl(end, src);
            for (int64_t p = l + lane; p < e; p += WAVE) {
                const int64_t i = ti[p];
                if (i >= top) break;
                kr_set(s_mark, i, base);
            }
        }
    }
}

// the sum of v over the workgroup, and in *pre the sum over the threads before this one (every thread calls)
__device__ __forceinline__ uint32_t kr_scan(uint32_t v, uint32_t *s_tot, uint32_t *pre)
{
    const int t = threadIdx.x, lane = t & (WAVE - 1), w = t / WAVE;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == WAVE - 1) s_tot[w] = inc;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int x = 0; x < KS_NW; x++) {
        const uint32_t n = s_tot[x];
        if (x < w) before += n;
        tot += n;
    }
    *pre = before + inc - v;
    return tot;
}

// COUNT when min_nbrs == 1: the candidates of every (listed row, range) pair are its stored targets
__global__ __launch_bounds__(KS_THREADS) void knn_reach_marks_kernel(const KrArgs a, int64_t first_block)
{
    __shared__ uint32_t s_mark[KR_WORDS];
    __shared__ uint32_t s_tot[KS_NW];
    const KsArgs &g = a.g;
    const int64_t wg = first_block + blockIdx.x;
    const int64_t r = wg / a.n_ranges, base = (wg - r * a.n_ranges) * KR_R;
    const int t = threadIdx.x;
    const int32_t u = g.rows[r];
    const int64_t rs = load_ptr(g.rpr, g.pr64, u);
    const uint32_t lr = (uint32_t)(load_ptr(g.rpr, g.pr64, (int64_t)u + 1) - rs);
    for (int x = t; x < KR_WORDS; x += KS_THREADS) s_mark[x] = 0;
    __syncthreads();
    kr_mark(a, g.cr + rs, lr, base, s_mark);
    __syncthreads();
    uint32_t mine = 0, pre;
#pragma unroll
    for (int k = 0; k < KR_WPT; k++)
        if (t * KR_WPT + k < KR_WORDS) mine += (uint32_t)__popc(s_mark[t * KR_WPT + k]);
    const uint32_t tot = kr_scan(mine, s_tot, &pre);
    if (t == 0) g.cnt[wg] = tot;
}

// COUNT when min_nbrs > 1, and PLACE
template <bool PLACE>
__global__ __launch_bounds__(KS_THREADS) void knn_reach_kernel(const KrArgs a, int64_t first_block)
{
    __shared__ int32_t s_cols[KS_LDS_ROW];
    __shared__ double s_vals[KS_LDS_ROW];
    __shared__ uint32_t s_bits[KS_BITS / 32];
    __shared__ uint32_t s_mark[KR_WORDS];
    __shared__ uint32_t s_pre[KR_WORDS];
    __shared__ double s_score[KR_ROUND];
    __shared__ int32_t s_tgt[KR_ROUND];
    __shared__ int32_t s_flag[KR_ROUND];
    __shared__ uint32_t s_tot[KS_NW];
    const KsArgs &g = a.g;
    const int64_t wg = first_block + blockIdx.x;
    const int64_t r = wg / a.n_ranges, base = (wg - r * a.n_ranges) * KR_R;
    if (PLACE && g.off[wg + 1] == g.off[wg]) return;             // (the whole workgroup: nothing of this range is stored)
    const int t = threadIdx.x, lane = t & (WAVE - 1), w = t / WAVE, grp = t / KS_LANES, sub = t & (KS_LANES - 1);
    const int32_t u = g.rows[r];
    const int64_t rs = load_ptr(g.rpr, g.pr64, u);
    const uint32_t lr = (uint32_t)(load_ptr(g.rpr, g.pr64, (int64_t)u + 1) - rs);
    const bool staged = lr <= (uint32_t)KS_LDS_ROW;
    const bool average = g.aggregate == CSRK_KNN_WEIGHTED_AVERAGE;
    const int32_t *__restrict__ gcols = g.cr + rs;
    if (lr == 0) {                                               // (the whole workgroup) no rating, no candidate
        if (!PLACE && t == 0) g.cnt[wg] = 0;
        return;
    }
    for (int x = t; x < KS_BITS / 32; x += KS_THREADS) s_bits[x] = 0;
    for (int x = t; x < KR_WORDS; x += KS_THREADS) s_mark[x] = 0;
    __syncthreads();
    kr_mark(a, gcols, lr, base, s_mark);
    for (uint32_t j = t; j < lr; j += KS_THREADS) {              // the rating row and its filter, as knn_scores_kernel stages them
        const int32_t c = gcols[j];
        atomicOr(&s_bits[ks_slot(c) >> 5], 1u << (ks_slot(c) & 31));
        if (staged) {
            s_cols[j] = c;
            if (average) s_vals[j] = csr_val(g.vr, g.vtr, rs + j);
        }
    }
    __syncthreads();
    // enumerate: s_pre[x] = the candidates in the words before x
    uint32_t mine = 0, pre;
#pragma unroll
    for (int k = 0; k < KR_WPT; k++)
        if (t * KR_WPT + k < KR_WORDS) mine += (uint32_t)__popc(s_mark[t * KR_WPT + k]);
    const uint32_t n_cand = kr_scan(mine, s_tot, &pre);
#pragma unroll
    for (int k = 0; k < KR_WPT; k++)
        if (t * KR_WPT + k < KR_WORDS) {
            s_pre[t * KR_WPT + k] = pre;
            pre += (uint32_t)__popc(s_mark[t * KR_WPT + k]);
        }
    __syncthreads();
    const KsRow row{gcols, g.vr, rs, lr};
    uint32_t stored = 0;                                         // (the first wavefront's) targets stored in the rounds so far
    for (uint32_t q0 = 0; q0 < n_cand; q0 += KR_ROUND) {         // (n_cand is the same in every thread)
        int64_t tgt[KS_ILP];
        double num[KS_ILP], den[KS_ILP];
        int32_t nn[KS_ILP];
#pragma unroll
        for (int j = 0; j < KS_ILP; j++) {
            const uint32_t q = q0 + j * KS_GROUPS + grp;
            tgt[j] = -1;
            if (q < n_cand) {
                // the last word x with s_pre[x] <= q holds candidate q (an empty word repeats its successor's prefix) ...
                uint32_t x = 0;
                for (uint32_t n = KR_WORDS; n > 1;) {
                    const uint32_t half = n >> 1;
                    if (s_pre[x + half] <= q) x += half;
                    n -= half;
                }
                // ... as its (q - s_pre[x])-th set bit
                const uint32_t m = s_mark[x];
                uint32_t k = q - s_pre[x], pos = 0;
#pragma unroll
                for (uint32_t h = 16; h; h >>= 1) {
                    const uint32_t c = (uint32_t)__popc((m >> pos) & ((1u << h) - 1));
                    if (k >= c) {
                        k -= c;
                        pos += h;
                    }
                }
                const int64_t i = base + (int64_t)x * 32 + pos;
                if (i < g.n_targets) tgt[j] = i;                 // (a mark is a target of the model: kept for the bound's sake)
            }
        }
        if (staged)
            ks_fold<true>(g, row, s_bits, s_cols, s_vals, tgt, num, den, nn);
        else
            ks_fold<false>(g, row, s_bits, s_cols, s_vals, tgt, num, den, nn);
        if (sub == 0) {
#pragma unroll
            for (int j = 0; j < KS_ILP; j++) {
                const int q = j * KS_GROUPS + grp;
                s_flag[q] = tgt[j] >= 0 && nn[j] >= g.min_nbrs ? 1 : 0;
                if (PLACE) {
                    s_tgt[q] = (int32_t)tgt[j];
                    s_score[q] = ks_score_of(g, r, num[j], den[j]);
                }
            }
        }
        __syncthreads();
        if (w == 0) {                                            // lane t takes candidate q0 + t: its rank among the stored ones
            const bool f = s_flag[lane] != 0;
            const unsigned long long bal = __ballot(f);
            if (PLACE && f) {
                const uint32_t before = (uint32_t)__popcll(bal & (lane ? (~0ull >> (WAVE - lane)) : 0ull));
                const int64_t o = g.off[wg] + stored + before;
                if (o < g.off[wg + 1]) {                         // (COUNT walked the same candidates: kept for the bound's sake)
                    g.oc[o] = s_tgt[lane];
                    g.ov[o] = s_score[lane];
                }
            }
            stored += (uint32_t)__popcll(bal);
        }
        __syncthreads();                                         // (the next round writes s_flag, s_tgt and s_score again)
    }
    if (!PLACE && t == 0) g.cnt[wg] = stored;
}

// the offsets at tile 0 of every listed row, and the total: what write_rowptrs turns into row pointers
__global__ __launch_bounds__(256) void knn_row_offsets_kernel(const int64_t *__restrict__ off, int64_t n_rows, int64_t n_tiles,
                                                             int64_t *__restrict__ rowoff)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= n_rows) rowoff[r] = off[r * n_tiles];
}

// a row no 32-bit count can hold
__global__ __launch_bounds__(256) void knn_long_row_kernel(const void *__restrict__ rp, int ptr64, int32_t nrows, int32_t *__restrict__ bad)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const int64_t len = load_ptr(rp, ptr64, r + 1) - load_ptr(rp, ptr64, r);
    if (len < 0 || len > INT32_MAX) atomicOr(bad, 1);
}

static int knn_long_rows(Matrix *m, const char *what, const char *name)
{
    if (m->nnz <= INT32_MAX) return CSRK_OK;                  // (no row can be longer than the matrix)
    DevBuf bad;
    CSRK_TRY(bad.alloc(4));
    CSRK_HIP(hipMemsetAsync(bad.p, 0, 4, nullptr));
    knn_long_row_kernel<<<(unsigned)ceil_div((int64_t)m->nrows, 256), 256>>>(m->d_rowptrs, m->ptr64, m->nrows, bad.as<int32_t>());
    CSRK_LAUNCH_CHECK();
    int32_t is_bad = 0;
    CSRK_HIP(hipMemcpy(&is_bad, bad.p, 4, hipMemcpyDeviceToHost));      // (waits for the kernel: `bad` may go back to the pool)
    if (is_bad) {
        set_error("%s: a row of %s holds more than 2^31 - 1 entries", what, name);
        return CSRK_ERR_UNSUPPORTED;
    }
    return CSRK_OK;
}

// a grid of n_wgs workgroups, cut into launches of at most KS_GRID_MAX
template <class A>
static void knn_launch(void (*kernel)(const A, int64_t), const A &g, int64_t n_wgs)
{
    for (int64_t b = 0; b < n_wgs; b += KS_GRID_MAX) {
        const int64_t n = n_wgs - b < KS_GRID_MAX ? n_wgs - b : KS_GRID_MAX;
        kernel<<<(unsigned)n, KS_THREADS>>>(g, b);
    }
}

// csrk_knn_scores_last_stats: what the calling thread's last scoring call did (include/csrk.h has the layout); filled from
// what the host holds anyway
constexpr int KS_N_STATS = 6;
static thread_local int64_t t_knn_stats[KS_N_STATS];

// The reach index of a model (Matrix::knn_reach): the structure-only transpose of its pattern, built once and kept with the
// handle like a plan.  Caller holds model->mu.
static int knn_reach_index(Matrix *model, bool *built)
{
    *built = false;
    if (model->knn_reach) return CSRK_OK;
    Matrix *t = nullptr;
    CSRK_TRY(transpose_matrix(model, 0, &t, nullptr));      // (waits for its launches)
    model->knn_reach = t;
    *built = true;
    return CSRK_OK;
}

static int64_t knn_reach_bytes(const Matrix *t)
{
    return (int64_t)((size_t)(t->nrows + 1) * t->ptr_bytes() + (size_t)t->nnz * 4);
}

// both routes: COUNT per block, scan, row pointers, PLACE.  A block is a (listed row, tile) pair of the walk-all route and a
// (listed row, range) pair of the reach route.
static int knn_impl(bool reach, const char *what, Matrix *model, Matrix *ratings, const int32_t *rows, int64_t n_rows, int32_t max_nbrs,
                    int32_t min_nbrs, int aggregate, const double *offsets, Matrix **out)
{
    const int64_t per_row = ceil_div((int64_t)model->nrows, reach ? KR_R : KS_TILE), n_blocks = n_rows * per_row;
    bool built = false;
    if (reach) CSRK_TRY(knn_reach_index(model, &built));
    DevBuf d_rows, d_offsets, cnt, rowoff;
    CSRK_TRY(d_rows.alloc((size_t)n_rows * 4));
    if (offsets) CSRK_TRY(d_offsets.alloc((size_t)n_rows * 8));
    CSRK_TRY(cnt.alloc((size_t)(n_blocks + 1) * 8));
    CSRK_TRY(rowoff.alloc((size_t)(n_rows + 1) * 8));
    DrainOnExit drain_on_exit;      // (before the buffers above go back to the pool)
    CSRK_HIP(hipMemcpy(d_rows.p, rows, (size_t)n_rows * 4, hipMemcpyHostToDevice));
    if (offsets) CSRK_HIP(hipMemcpy(d_offsets.p, offsets, (size_t)n_rows * 8, hipMemcpyHostToDevice));
    KrArgs a{};
    KsArgs &g = a.g;
    g.rpm = model->d_rowptrs, g.rpr = ratings->d_rowptrs;
    g.cm = model->d_colinds, g.cr = ratings->d_colinds;
    g.vm = model->d_values, g.vr = ratings->d_values;
    g.pm64 = model->ptr64, g.pr64 = ratings->ptr64, g.vtm = model->val_type, g.vtr = ratings->val_type, g.aggregate = aggregate;
    g.n_targets = model->nrows, g.max_nbrs = max_nbrs, g.min_nbrs = min_nbrs;
    g.n_tiles = per_row;
    g.tiles_per_wg = n_blocks / KS_WGS_FILL < 1 ? 1 : (n_blocks / KS_WGS_FILL > KS_TILES_MAX ? KS_TILES_MAX : n_blocks / KS_WGS_FILL);
    g.rows = d_rows.as<int32_t>();
    g.offsets = offsets ? d_offsets.as<double>() : nullptr;
    g.cnt = cnt.as<int64_t>();
    int64_t n_wgs = n_rows * ceil_div(per_row, g.tiles_per_wg);
    if (reach) {
        const Matrix *t = model->knn_reach;
        a.tp = t->d_rowptrs, a.ti = t->d_colinds, a.tp64 = t->ptr64, a.n_items = t->nrows, a.n_ranges = per_row;
        n_wgs = n_blocks;
        if (min_nbrs == 1)
            knn_launch(knn_reach_marks_kernel, a, n_wgs);
        else
            knn_launch(knn_reach_kernel<false>, a, n_wgs);
    } else {
        knn_launch(knn_scores_kernel<false>, g, n_wgs);
    }
    CSRK_LAUNCH_CHECK();
    int64_t total = 0;
    CSRK_TRY(scan_total(cnt.as<int64_t>(), n_blocks, &total));
    Matrix *t = nullptr;
    CSRK_TRY(new_matrix((int32_t)n_rows, model->nrows, total, total > INT32_MAX, CSRK_VAL_F64, &t));
    knn_row_offsets_kernel<<<(unsigned)ceil_div(n_rows + 1, 256), 256>>>(cnt.as<int64_t>(), n_rows, per_row, rowoff.as<int64_t>());
    write_rowptrs(rowoff.as<int64_t>(), n_rows, t);
    if (total > 0) {
        g.off = cnt.as<int64_t>();
        g.cnt = nullptr;
        g.oc = t->d_colinds;
        g.ov = (double *)t->d_values;
        if (reach)
            knn_launch(knn_reach_kernel<true>, a, n_wgs);
        else
            knn_launch(knn_scores_kernel<true>, g, n_wgs);
    }
    CSRK_TRY(finish_result(t, what));
    if (reach) {
        const int64_t st[KS_N_STATS] = {1, per_row, n_wgs, min_nbrs == 1, built, total};
        for (int k = 0; k < KS_N_STATS; k++) t_knn_stats[k] = st[k];
    }
    *out = t;
    return CSRK_OK;
}

// known canonical, like csrk_coalesce's result: a following csrk_combine does not look at the rows again
static void knn_mark_canonical(Matrix *t)
{
    t->canonical = 1;
    t->noncanonical_row = -1;
    t->nondescending = 1;
}

// csrk_knn_scores and csrk_knn_scores_reach: one list of refusals, in one order, under the entry's own name
static int knn_entry(bool reach, csrk_handle_t model_h, csrk_handle_t ratings_h, const int32_t *rows, int64_t n_rows, int32_t max_nbrs,
                     int32_t min_nbrs, int aggregate, const double *offsets, csrk_handle_t *out)
{
    const char *what = reach ? "knn_scores_reach" : "knn_scores";
    for (int k = 0; k < KS_N_STATS; k++) t_knn_stats[k] = 0;      // (a failed call, an empty result and the walk-all route report nothing)
    CSRK_REQUIRE(out, "%s: out is NULL", what);
    *out = 0;
    Matrix *model = from_handle(model_h);
    if (!model) return CSRK_ERR_INVALID;
    Matrix *ratings = from_handle(ratings_h);
    if (!ratings) return CSRK_ERR_INVALID;
    CSRK_REQUIRE(model->ncols == ratings->ncols, "%s: model is %d x %d and ratings is %d x %d: the columns differ", what, model->nrows,
                 model->ncols, ratings->nrows, ratings->ncols);
    CSRK_REQUIRE(model->device == ratings->device, "%s: the operands live on devices %d and %d", what, model->device, ratings->device);
    CSRK_REQUIRE(n_rows >= 0 && n_rows <= INT32_MAX - 1, "%s: bad row count n_rows=%lld", what, (long long)n_rows);
    CSRK_REQUIRE(rows || n_rows == 0, "%s: rows is NULL", what);
    CSRK_REQUIRE(max_nbrs >= 0, "%s: max_nbrs must not be negative (max_nbrs=%d)", what, max_nbrs);
    CSRK_REQUIRE(min_nbrs >= 1, "%s: min_nbrs must be at least 1 (min_nbrs=%d)", what, min_nbrs);
    CSRK_REQUIRE(aggregate == CSRK_KNN_WEIGHTED_AVERAGE || aggregate == CSRK_KNN_SUM, "%s: unknown aggregate %d", what, aggregate);
    for (int64_t r = 0; r < n_rows; r++)                          // the list is looked at before anything is sent
        CSRK_REQUIRE(rows[r] >= 0 && rows[r] < ratings->nrows, "%s: rows[%lld]=%d is outside [0, %d)", what, (long long)r, rows[r],
                     ratings->nrows);
    // both handles' locks, in one fixed order (by address), as csrk_combine takes them
    std::unique_lock<std::mutex> l1, l2;
    if (model == ratings) {
        l1 = std::unique_lock<std::mutex>(model->mu);
    } else {
        Matrix *first = std::less<Matrix *>()(model, ratings) ? model : ratings, *second = first == model ? ratings : model;
        l1 = std::unique_lock<std::mutex>(first->mu);
        l2 = std::unique_lock<std::mutex>(second->mu);
    }
    Matrix *t = nullptr;
    if (n_rows == 0 || model->nrows == 0 || model->nnz == 0 || ratings->nnz == 0) {      // an empty result; nothing is launched or built
        CSRK_TRY(empty_matrix((int32_t)n_rows, model->nrows, CSRK_VAL_F64, what, &t));
        knn_mark_canonical(t);
        *out = to_handle(t);
        return CSRK_OK;
    }
    CSRK_TRY(ensure_canonical(ratings, "ratings"));
    CSRK_TRY(knn_long_rows(model, what, "model"));
    CSRK_TRY(knn_long_rows(ratings, what, "ratings"));      // (a canonical row holds at most ncols entries: kept for the contract's sake)
    CSRK_TRY(knn_impl(reach, what, model, ratings, rows, n_rows, max_nbrs, min_nbrs, aggregate, offsets, &t));
    knn_mark_canonical(t);
    *out = to_handle(t);
    return CSRK_OK;
}

}  // namespace csrk

using namespace csrk;

extern "C" {

int csrk_knn_scores_limits(int64_t *out, int n)
{
    CSRK_REQUIRE(out && n >= 0, "csrk_knn_scores_limits: out is NULL or n < 0");
    const int64_t v[6] = {KS_LANES, KS_TILE, KS_LDS_ROW, KS_BITS, KS_TILES_MAX, KS_WGS_FILL};
    for (int i = 0; i < n && i < 6; i++) out[i] = v[i];
    return CSRK_OK;
}

int csrk_knn_scores_reach_limits(int64_t *out, int n)
{
    CSRK_REQUIRE(out && n >= 0, "csrk_knn_scores_reach_limits: out is NULL or n < 0");
    const int64_t v[7] = {KR_R, KS_LANES, KS_LDS_ROW, KS_BITS, KR_ROUND, KR_R, KR_LONG};
    for (int i = 0; i < n && i < 7; i++) out[i] = v[i];
    return CSRK_OK;
}

int csrk_knn_scores_last_stats(int64_t *out, int n)
{
    CSRK_REQUIRE(out && n >= 0, "csrk_knn_scores_last_stats: out is NULL or n < 0");
    for (int i = 0; i < n && i < KS_N_STATS; i++) out[i] = t_knn_stats[i];
    return CSRK_OK;
}

int csrk_knn_scores(csrk_handle_t model_h, csrk_handle_t ratings_h, const int32_t *rows, int64_t n_rows, int32_t max_nbrs, int32_t min_nbrs,
                    int aggregate, const double *offsets, csrk_handle_t *out)
{
    return knn_entry(false, model_h, ratings_h, rows, n_rows, max_nbrs, min_nbrs, aggregate, offsets, out);
}

int csrk_knn_scores_reach(csrk_handle_t model_h, csrk_handle_t ratings_h, const int32_t *rows, int64_t n_rows, int32_t max_nbrs,
                          int32_t min_nbrs, int aggregate, const double *offsets, csrk_handle_t *out)
{
    return knn_entry(true, model_h, ratings_h, rows, n_rows, max_nbrs, min_nbrs, aggregate, offsets, out);
}

int csrk_knn_reach_index(csrk_handle_t model_h, int build, int64_t *entries, int64_t *bytes)
{
    CSRK_REQUIRE(entries && bytes, "knn_reach_index: entries or bytes is NULL");
    *entries = 0, *bytes = 0;
    Matrix *model = from_handle(model_h);
    if (!model) return CSRK_ERR_INVALID;
    std::lock_guard<std::mutex> lk(model->mu);
    if (build && !model->knn_reach) {
        bool built = false;
        CSRK_TRY(knn_reach_index(model, &built));
    }
    if (model->knn_reach) {
        *entries = model->knn_reach->nnz;
        *bytes = knn_reach_bytes(model->knn_reach);
    }
    return CSRK_OK;
}

}  // extern "C"
