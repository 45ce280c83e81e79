// The dense-panel SpMM's host decisions (spmm_dense.hip; DESIGN.md section 7, "The plan builder and launch side"): the
// constants behind them and one pure function per decision -- which rows are heavy and in how many row groups, how the
// column tiles fall into ranges, when the heavy form is refused, how a product's panel is cut into launches, and when
// mult_ab's dense-B route takes a product.  Plain host arithmetic over host vectors, no device code and no call into the
// runtime: spmm_dense.hip calls it, and tests/spmm_plan_host runs it as a stand-alone program -- at every rule's edge, and
// on every case of tests/spmm_cases.py against that module's NumPy statement of the same plan.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace csrk {

// ---- the light rows (spmm_seg_kernel) ---------------------------------------------------------------------------------
constexpr int MM_SEG = 64;       // entries per segment (light rows)
constexpr int MM_G = 16;         // lanes per unit (segment or row slice): 16 lanes x 4 columns = a 64-column chunk of the panel
constexpr int MM_CHUNK = 64;     // panel columns per pass over a unit's entries

// ---- the heavy rows (spmm_hrows_kernel; the layout is described there) ----------------------------------------------
constexpr int HR_LANES = 64;                     // a wavefront (spmm_dense.hip checks it against WAVE)
constexpr int HR_THREADS = 1024;
constexpr int HR_WAVES = HR_THREADS / HR_LANES;  // 16
constexpr int HR_RPW = 32;                       // rows per wavefront
constexpr int HR_ROWS = HR_WAVES * HR_RPW;       // 512 rows per workgroup
constexpr int HR_TILE = 128;                     // rows of B per tile
constexpr int HR_KC = 64;                        // panel columns per launch (wider panels: one launch per 64 columns)
constexpr int HR_PAD = 2 * HR_LANES;             // the entry arrays' padding: a wavefront loads 64 entries from a bucket's start whatever its length
constexpr int HR_MAXG = 8;                       // at most 8 row groups (4096 heavy rows)
constexpr size_t HR_LDS = (size_t)2 * HR_TILE * HR_KC * 8;

// the rules of the heavy-row choice
constexpr int64_t HR_ENGAGE_BYTES = 64ll << 20;  // the form is tried when B as a whole is larger (it does not fit the caches)
constexpr int64_t HR_FLOOR = 512;                // shorter rows never pay for a register slot ...
constexpr int64_t HR_FLOOR_FORCED = 256;         // ... (forced: small test matrices)
constexpr int64_t HR_PAYS_ENTRIES = 4, HR_PAYS_COLS = 5;      // a row group pays when 4 x its entries >= 5 x the rows of B it stages
constexpr int64_t HR_TILE_COST = 200;            // a tile's fixed cost (staging + barrier) in entries, per row group
constexpr int64_t HR_MAX_BUCKETS = 1ll << 30;    // bucket keys are 32-bit (and sorted with a payload)
constexpr int64_t HR_TABLE_BYTES = 8, HR_STREAM_BYTES = 12;   // a bucket bound; an entry of the stream: the table must not outweigh it
constexpr size_t HR_BUILD_ENTRY_BYTES = 40, HR_BUILD_BUCKET_BYTES = 8, HR_BUILD_SPARE = 64u << 20;      // free memory a build needs

// ---- the knobs ---------------------------------------------------------------------------------------------------------
struct SpmmKnobStrings {      // getenv's answers, nullptr = unset
    const char *heavy, *heavy_groups, *plan_trace, *spgemm_dense;      // CSRK_SPMM_HEAVY, CSRK_SPMM_HEAVY_GROUPS, CSRK_PLAN_TRACE, CSRK_SPGEMM_DENSE
};
struct SpmmKnobs {
    bool never, force;      // CSRK_SPMM_HEAVY=0 / =1 (the first character decides)
    int groups;             // CSRK_SPMM_HEAVY_GROUPS: that many row groups, or as many as there are candidates for; 0 = unset
    bool trace;             // CSRK_PLAN_TRACE is set (to anything): a line per row group tried
    bool dense_b;           // mult_ab's dense-B route (CSRK_SPGEMM_DENSE=0: off)
};
inline SpmmKnobs parse_spmm_knobs(const SpmmKnobStrings &e)
{
    SpmmKnobs k;
    k.never = e.heavy && e.heavy[0] == '0';
    k.force = e.heavy && e.heavy[0] == '1';
    const int g = e.heavy_groups ? atoi(e.heavy_groups) : 0;
    k.groups = g > 0 ? g : 0;
    k.trace = e.plan_trace != nullptr;
    k.dense_b = !(e.spgemm_dense && e.spgemm_dense[0] == '0');
    return k;
}

namespace spmmplan {

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- the heavy-row choice, in the builder's order ----------------------------------------------------------------------
// is the heavy form tried at all: B as a whole does not fit the caches, or it is forced
inline bool heavy_engaged(int32_t ncols, int32_t k, const SpmmKnobs &knobs)
{
    return !knobs.never && ((int64_t)ncols * k * 8 > HR_ENGAGE_BYTES || knobs.force);
}
inline bool has_entries(int32_t nrows, int32_t ncols, int64_t nnz) { return !(nrows < 1 || ncols < 1 || nnz < 1); }

// rows of at least the floor, longest first, then by row id
inline std::vector<int32_t> candidates(const std::vector<int64_t> &len, bool force)
{
    std::vector<int32_t> cand;
    const int64_t floor_len = force ? HR_FLOOR_FORCED : HR_FLOOR;
    for (int32_t r = 0; r < (int32_t)len.size(); r++)
        if (len[(size_t)r] >= floor_len) cand.push_back(r);
    std::sort(cand.begin(), cand.end(), [&](int32_t a, int32_t b) { return len[(size_t)a] != len[(size_t)b] ? len[(size_t)a] > len[(size_t)b] : a < b; });
    return cand;
}

// Every row group sweeps all of B once (G n_cols rows of B staged in all), tile by tile, whatever it finds there: a
// group costs its tiles (staging, a barrier, a partial batch per wavefront) plus ~21 ps per entry, and saves the ~63 ps
// per entry of the light-row kernel.  Measured on the BASELINE matrix (2M columns; groups of 23.0 / 3.2 / 1.8 / 1.2 M
// entries): one group 2.22 ms for the product, two 2.12, four 2.13, eight 2.55.  Take row groups, longest rows first,
// while the group's entries are at least 1.25 x the rows of B it stages (forced: the first group always;
// CSRK_SPMM_HEAVY_GROUPS = g: g groups, whether they pay or not).
inline bool group_pays(int64_t entries, int32_t ncols) { return entries * HR_PAYS_ENTRIES >= HR_PAYS_COLS * (int64_t)ncols; }
struct GroupTry {      // a row group the loop looked at: candidates [first, end), the last record is where it stopped (if it did)
    size_t first, end;
    int64_t longest, shortest, entries;
    bool pays;
};
struct Groups {
    int G = 0;
    size_t taken = 0;      // candidates in the G groups
    std::vector<GroupTry> tried;
};
inline Groups choose_groups(const std::vector<int64_t> &len, const std::vector<int32_t> &cand, int32_t ncols, const SpmmKnobs &knobs)
{
    Groups c;
    while (c.G < HR_MAXG && c.taken < cand.size()) {
        GroupTry t;
        t.first = c.taken;
        t.end = std::min(cand.size(), c.taken + (size_t)HR_ROWS);
        t.entries = 0;
        for (size_t i = t.first; i < t.end; i++) t.entries += len[(size_t)cand[i]];
        t.longest = len[(size_t)cand[t.first]];
        t.shortest = len[(size_t)cand[t.end - 1]];
        t.pays = group_pays(t.entries, ncols);
        c.tried.push_back(t);
        if (knobs.groups > 0 ? c.G >= knobs.groups : (!t.pays && !(knobs.force && c.G == 0))) break;
        c.taken = t.end;
        c.G++;
    }
    return c;
}

// The threshold is a row LENGTH (the light path skips rows by length): rows as long as the last one taken come along
// when they fit the G groups, else the threshold moves up to the next length and the rows shorter than it are dropped --
// down to none, which switches the form off (as does a length no int32 holds).
struct Threshold {
    bool on, moved;
    int64_t hmin;
    size_t n;      // heavy rows: the first n candidates
};
inline Threshold threshold(const std::vector<int64_t> &len, const std::vector<int32_t> &cand, size_t taken, int G)
{
    Threshold t;
    t.hmin = len[(size_t)cand[taken - 1]];
    t.n = taken;
    t.moved = false;
    while (t.n < cand.size() && len[(size_t)cand[t.n]] >= t.hmin) t.n++;
    if (t.n > (size_t)G * HR_ROWS) {
        t.moved = true;
        t.hmin++;
        t.n = taken;
        while (t.n > 0 && len[(size_t)cand[t.n - 1]] < t.hmin) t.n--;
    }
    t.on = !(t.n == 0 || t.hmin > INT32_MAX);
    return t;
}

// G shrinks while G - 1 groups hold all n rows
inline int shrink_groups(int G, size_t n)
{
    while (G > 1 && (size_t)(G - 1) * HR_ROWS >= n) G--;
    return G;
}

inline int64_t tiles_of(int32_t ncols) { return cdiv((int64_t)ncols, HR_TILE); }
// G R workgroups, one per CU; a range needs a tile; with R a multiple of 8 the G workgroups of a column range sit side by
// side on one XCD (spmm_hrows_kernel)
inline int ranges_for(int cus, int G, int64_t n_tiles)
{
    int R = (int)std::min<int64_t>(std::max(cus, G) / G, n_tiles);
    if (R >= 8) R = R / 8 * 8;
    return R;
}
inline int64_t buckets_of(int64_t n_tiles, int G) { return n_tiles * G * HR_WAVES; }      // bucket = (tile * G + group) * 16 + wavefront
inline bool bucket_keys_fit(int64_t n_buckets) { return n_buckets < HR_MAX_BUCKETS; }
// unless forced: the bucket table must not outweigh the stream
inline bool table_pays(int64_t n_buckets, int64_t nnz_h, bool force) { return force || !(n_buckets * HR_TABLE_BYTES > nnz_h * HR_STREAM_BYTES); }
// the stream, the records it is sorted from and the sort's scratch, beside 64 MiB for everything else
inline bool build_fits_memory(int64_t nnz_h, int64_t n_buckets, size_t mfree)
{
    return !((size_t)nnz_h * HR_BUILD_ENTRY_BYTES + (size_t)n_buckets * HR_BUILD_BUCKET_BYTES + HR_BUILD_SPARE > mfree);
}

// places: rank i (longest first) -> group i % G, then wavefront and slot round robin, so every wavefront of every group
// holds the same mix of lengths.  The code is group << 9 | wavefront << 5 | slot; the reduce kernel reads group and
// (wavefront << 5 | slot) = the row inside the workgroup back out of it.
inline int32_t place_code(size_t i, int G)
{
    const int32_t g = (int32_t)(i % (size_t)G), j = (int32_t)(i / (size_t)G);
    return (g << 9) | ((j % HR_WAVES) << 5) | (j / HR_WAVES);
}
inline std::vector<int32_t> place_codes(size_t n, int G)
{
    std::vector<int32_t> code(n);
    for (size_t i = 0; i < n; i++) code[i] = place_code(i, G);
    return code;
}
struct Place {
    int32_t group, wave, slot;
};
inline Place place_of(int32_t code) { return {code >> 9, (code >> 5) & (HR_WAVES - 1), code & (HR_RPW - 1)}; }

inline int64_t entries_of(const std::vector<int64_t> &len, const std::vector<int32_t> &rows)
{
    int64_t n = 0;
    for (int32_t r : rows) n += len[(size_t)r];
    return n;
}
// where heavy row i's entries start in the (rank, storage order) stream; off[n] = all of them
inline std::vector<int64_t> entry_offsets(const std::vector<int64_t> &len, const std::vector<int32_t> &rows)
{
    std::vector<int64_t> off(rows.size() + 1);
    off[0] = 0;
    for (size_t i = 0; i < rows.size(); i++) off[i + 1] = off[i] + len[(size_t)rows[i]];
    return off;
}

// everything above in the builder's order, up to the question only the device answers (free memory)
struct HeavyChoice {
    bool on = false;
    std::vector<GroupTry> tried;      // for CSRK_PLAN_TRACE
    std::vector<int32_t> rows;        // the heavy rows by rank
    bool moved = false;               // the threshold moved up past the ties
    int64_t hmin = 0, nnz_h = 0, n_tiles = 0, n_buckets = 0;
    int G_taken = 0, G = 0, R = 0;    // row groups before and after the shrink, column ranges
};
inline HeavyChoice choose_heavy(const std::vector<int64_t> &len, int32_t ncols, int cus, const SpmmKnobs &knobs)
{
    HeavyChoice h;
    std::vector<int32_t> cand = candidates(len, knobs.force);
    if (cand.empty()) return h;
    Groups c = choose_groups(len, cand, ncols, knobs);
    h.tried = std::move(c.tried);
    if (c.G == 0) return h;
    const Threshold t = threshold(len, cand, c.taken, c.G);
    h.moved = t.moved;
    if (!t.on) return h;
    cand.resize(t.n);
    h.rows = std::move(cand);
    h.hmin = t.hmin;
    h.nnz_h = entries_of(len, h.rows);
    h.G_taken = c.G;
    h.G = shrink_groups(c.G, t.n);
    h.n_tiles = tiles_of(ncols);
    h.R = ranges_for(cus, h.G, h.n_tiles);
    h.n_buckets = buckets_of(h.n_tiles, h.G);
    h.on = bucket_keys_fit(h.n_buckets) && table_pays(h.n_buckets, h.nnz_h, knobs.force);
    return h;
}

// Column ranges: whole tiles, balanced by entries plus a fixed cost per tile (staging + barrier ~ 200 entries' worth per
// row group).  tot[t] = heavy entries before tile t.  range[q], 0 < q < R: the first tile whose cumulative cost exceeds
// q / R of the total; every range keeps at least one tile, and leaves one for each range after it.  (float arithmetic:
// tests/spmm_cases.py restates it operation for operation)
inline std::vector<int32_t> balance_ranges(const std::vector<int64_t> &tot, int64_t n_tiles, int G, int R, int64_t nnz_h)
{
    const int64_t tile_cost = HR_TILE_COST * (int64_t)G;
    const double total_cost = (double)nnz_h + (double)tile_cost * (double)n_tiles;
    std::vector<int32_t> range((size_t)R + 1);
    range[0] = 0;
    int64_t t = 0;
    for (int q = 1; q < R; q++) {
        const double goal = total_cost * q / R;
        while (t < n_tiles && (double)tot[(size_t)t + 1] + (double)tile_cost * (double)(t + 1) <= goal) t++;
        t = std::max<int64_t>(t, (int64_t)range[(size_t)q - 1] + 1);
        t = std::min<int64_t>(t, n_tiles - (R - q));
        range[(size_t)q] = (int32_t)t;
    }
    range[(size_t)R] = (int32_t)n_tiles;
    return range;
}

// ---- the light rows ------------------------------------------------------------------------------------------------------
// segments of a row of `len` entries (mm_count_kernel): none when the heavy kernels serve it (heavy_min > 0: rows of at
// least that many entries), one up to MM_SEG entries -- an empty row too --, else one per MM_SEG
constexpr int64_t light_segments(int64_t len, int32_t heavy_min)
{
    return (heavy_min > 0 && len >= heavy_min) ? 0 : (len <= MM_SEG ? 1 : (len + MM_SEG - 1) / MM_SEG);
}

// ---- a product's launches ------------------------------------------------------------------------------------------------
// The 16-B loads and stores (FULL4, EVEN) need 16-B aligned B / C rows: a column block of a wider panel that starts at an
// odd column, or an odd ldb / ldc, takes the 8-B forms instead (same products, same order of the sums: the bits do not
// depend on the form)
inline bool aligned16(const void *p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && (ld & 1) == 0; }
inline bool full4(int32_t k, bool b_al, bool c_al) { return (k % 4) == 0 && b_al && c_al; }
inline bool hrows_even(int32_t kc, bool b_al) { return kc % 2 == 0 && b_al; }
// the heavy kernels take HR_KC panel columns per launch: block b of a width k
struct ColBlock {
    int32_t c0, kc;
};
inline int32_t col_blocks(int32_t k) { return (int32_t)cdiv(k, HR_KC); }
inline ColBlock col_block(int32_t k, int32_t b)
{
    const int32_t c0 = b * HR_KC;
    return {c0, k - c0 < HR_KC ? k - c0 : HR_KC};
}
inline unsigned hrows_grid(int G, int R) { return (unsigned)(G * R); }                                   // one workgroup per (range, group)
inline unsigned seg_grid(int64_t n_segs) { return (unsigned)cdiv(n_segs * MM_G, 256); }                   // 16 lanes per segment
inline unsigned reduce_grid(int32_t hr_n) { return (unsigned)cdiv((int64_t)hr_n * HR_LANES, 256); }       // a wavefront per heavy row
inline unsigned fixup_grid(int32_t n_split) { return (unsigned)cdiv((int64_t)n_split * HR_LANES, 256); }  // a wavefront per split row
// a wider panel than any before needs a larger partial buffer (some row is split: n_multi partial panels)
inline bool grow_partials(int64_t n_multi, int32_t part_k, int32_t k) { return n_multi > 0 && part_k < k; }

// the nine fields of csrk_spmm_plan_stats; fields 1 .. 6 read 0 while the heavy form is off (a handle without a plan: PlanCounts{})
struct PlanCounts {
    bool hr_on;
    int32_t hr_min, hr_n, hr_G, hr_R;
    int64_t hr_nnz;
    int32_t hr_tiles;
    int64_t n_segs, n_multi;
};
inline void plan_stats(const PlanCounts &p, int64_t out[9])
{
    const int64_t v[9] = {p.hr_on ? 1 : 0, p.hr_min, p.hr_n, p.hr_G, p.hr_R, p.hr_nnz, p.hr_tiles, p.n_segs, p.n_multi};
    for (int i = 0; i < 9; i++) out[i] = !p.hr_on && i >= 1 && i <= 6 ? 0 : v[i];
}

// ---- mult_ab's dense-B route (spgemm_dense_b) ----------------------------------------------------------------------------
constexpr int DB_VAL_NONE = 0, DB_VAL_F32 = 1;      // CSRK_VAL_NONE, CSRK_VAL_F32 (checked in spmm_dense.hip)
// B may be a row-major panel: the shapes agree, there is something to multiply, and B holds nrows x k entries
inline bool dense_b_shapes(int32_t a_ncols, int64_t a_nnz, int32_t b_nrows, int32_t b_ncols, int64_t b_nnz)
{
    return !(a_ncols != b_nrows || b_ncols < 1 || b_nrows < 1 || a_nnz == 0 || b_nnz != (int64_t)b_nrows * b_ncols);
}
// declined: an operand without values (the general product reports it), float32 values on BOTH operands (the reference
// rounds those products to float32)
inline bool dense_b_types(int a_val, int b_val)
{
    return !(a_val == DB_VAL_NONE || b_val == DB_VAL_NONE) && !(a_val == DB_VAL_F32 && b_val == DB_VAL_F32);
}
inline bool dense_b_gate(const SpmmKnobs &knobs, int32_t a_ncols, int64_t a_nnz, int a_val, int32_t b_nrows, int32_t b_ncols,
                         int64_t b_nnz, int b_val)
{
    return knobs.dense_b && dense_b_shapes(a_ncols, a_nnz, b_nrows, b_ncols, b_nnz) && dense_b_types(a_val, b_val);
}
// C's row pointers are int32, as the reference's: live rows x k entries
inline int64_t dense_c_nnz(int64_t live_rows, int32_t k) { return live_rows * k; }
inline bool dense_c_overflows(int64_t c_nnz) { return c_nnz > INT32_MAX; }

}  // namespace spmmplan
}  // namespace csrk
