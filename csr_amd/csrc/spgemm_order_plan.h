// The ordering pass's host decisions (spgemm_order.hip: spgemm_apply_reference_order; DESIGN.md section 6, "The ordering
// pass's driver"): the constants the kernels share with them and one pure function per decision -- the LDS plan of the two
// walks and the placing pass, the split of the listed rows into their four tiers, the grid of every launch, the byte size of
// every temporary, the early exit, the parse of CSRK_SPGEMM_ORDER.  Plain host arithmetic in the integer types and
// expressions the driver always used, no device code, no allocation and no call into the runtime: spgemm_order.hip reads the
// plan and decides nothing itself, and tests/spgemm_order_plan_host runs the header as a stand-alone program -- at every
// rule's edge, and on every case of tests/spgemm_cases.py against that module's order_plan().
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace csrk {

// ---- the constants the kernels are written for ------------------------------------------------------------------------
constexpr int SO_LEAST = 64;                 // (2^6) rows of fewer products: SO_SUB lanes each, straight from the row number
constexpr int SO_TINY = 256;                 // (2^8) rows of fewer products: SO_SUB lanes each, from the list
constexpr int SO_WAVE = 1024;                // (2^10) rows of fewer products: a wavefront each, from the list
constexpr int SO_MID = 4096;                 // (2^12) rows of fewer products: a 256-thread workgroup each; the others 1024 threads
constexpr int SO_SUB = 16;
constexpr int SO_OCTAVES = 64;               // the listed rows by the octave of their product count (so_list_rows_kernel)
constexpr int SO_LDS_BYTES = 150 * 1024;     // dynamic LDS of the 1024-thread walk at most
constexpr int SO_WIN_WORDS = 16384;          // so_place_kernel: 64 KB of bits + 64 KB of counts
constexpr int SO_WIN = SO_WIN_WORDS * 32;
constexpr int SO_PLACE_THREADS = 1024;
constexpr int SO_TABLES_BYTES = 18 * 1024;   // kept back for the static batch tables of the 1024-thread walk (walk_static_lds)
constexpr int SO_WIN_ENTRY = 2048;           // bitmap words of the 1024-thread walk's placing window, by entry
constexpr int SO_WIN_COLS_MOST = 16384;      // and by column: the largest of 16384, 8192 ... 1024 that fits
constexpr int SO_WIN_COLS_LEAST = 1024;

namespace soplan {

constexpr int LANES = 64;                             // of a wavefront (common.h: WAVE)
constexpr int LONG_THREADS = 1024, MID_THREADS = 256; // so_walk_kernel's workgroup for the rows of at least SO_MID products, and below

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- the tiers ----------------------------------------------------------------------------------------------------------
// so_list_rows_kernel files a listed row under o = the leading zeros of its product count: octave o holds the rows of
// [2^(63 - o), 2^(64 - o)) products, the longest rows first.  A tier bound is a power of two, so a whole octave lies on one
// side of it: the rows of octave o have at least `bound` products exactly when o <= octave_of(bound).
constexpr bool is_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }
constexpr int octave_of(int64_t products) { return products <= 1 ? 63 : octave_of(products >> 1) - 1; }
static_assert(is_pow2(SO_LEAST) && is_pow2(SO_TINY) && is_pow2(SO_WAVE) && is_pow2(SO_MID), "an octave lies on one side of every tier bound");
static_assert(SO_LEAST < SO_TINY && SO_TINY < SO_WAVE && SO_WAVE < SO_MID, "the tiers nest");
static_assert(octave_of(SO_MID) == 51 && octave_of(1) == 63 && octave_of(INT64_MAX) == 1, "octave = leading zeros of an int64");

struct Tiers {
    int32_t cursor[SO_OCTAVES + 1];      // where each octave's rows start in the list; [SO_OCTAVES] as counted (the memory flag)
    int32_t listed;                      // rows of at least SO_LEAST products
    int32_t n_long, n_mid, n_wave, n_small;      // of them: at least SO_MID (first in the list), SO_WAVE, SO_TINY, SO_LEAST
    bool keys_in_memory;                 // some row needs key[]: more entries than the walk's LDS holds, or 2^32 products
};

// from the counts so_list_rows_kernel left (fill = false): counts[o] rows in octave o, counts[SO_OCTAVES] the memory flag
inline Tiers so_tiers(const int32_t counts[SO_OCTAVES + 1])
{
    Tiers t = {};
    for (int o = 0; o < SO_OCTAVES; o++) {
        t.cursor[o] = t.listed;
        t.listed += counts[o];
        if (o <= octave_of(SO_MID)) t.n_long = t.listed;
        if (o <= octave_of(SO_WAVE)) t.n_mid = t.listed - t.n_long;
        if (o <= octave_of(SO_TINY)) t.n_wave = t.listed - t.n_long - t.n_mid;
    }
    t.n_small = t.listed - t.n_long - t.n_mid - t.n_wave;
    t.cursor[SO_OCTAVES] = counts[SO_OCTAVES];
    t.keys_in_memory = counts[SO_OCTAVES] != 0;
    return t;
}

// ---- LDS ----------------------------------------------------------------------------------------------------------------
// static __shared__ of so_walk_kernel<.., THREADS, ..>: s_bs and s_off (int64 per thread, s_off one more), s_wave64 and s_wave
// (int64 and int32 per wavefront), s_take and s_found
constexpr size_t walk_static_lds(int threads, int lanes)
{
    return (size_t)threads * 8 + ((size_t)threads + 1) * 8 + (size_t)(threads / lanes) * 8 + 4 + 4 + (size_t)(threads / lanes) * 4;
}

// The 1024-thread walk (the device's own limit decides; SO_TABLES_BYTES of it are the kernel's batch tables).  By column --
// 4 B per column of C and a bit, twice: `seen` and the counts before its words -- when that leaves a window of 2^15 product
// indices at least and no row of B can hold 2^32 entries (32-bit indices inside a batch); else by entry, 8 B each, with a
// window of 2^16.  The 256-thread walk: rows of fewer than SO_MID products (and entries), by entry.  so_place_kernel: its
// window's bits and counts.  A window of w words costs 8 w bytes: the bitmap and the counts before its words.
struct LdsPlan {
    int64_t budget;                      // dynamic LDS of the 1024-thread walk
    int64_t by_col;                      // bytes of the by-column tables for this product's column count
    int32_t win_cols;                    // window words by column (0: none fits)
    bool cols_mode;
    int32_t win_long, cap_long;          // the 1024-thread walk: window words, entries of a row LDS holds (by column: any)
    size_t lds_long;
    int32_t win_mid, cap_mid;            // the 256-thread walk
    size_t lds_mid;
    size_t lds_place;                    // so_place_kernel
    bool ok;                             // false: the device has too little LDS for the pass
};

inline LdsPlan so_lds_plan(int lds_max, int32_t c_ncols, int64_t b_nnz)
{
    LdsPlan p = {};
    p.budget = std::min<int64_t>(SO_LDS_BYTES, (int64_t)lds_max - SO_TABLES_BYTES);
    p.by_col = (((int64_t)c_ncols + 31) / 32 * 2 + c_ncols) * 4;
    for (int32_t w = SO_WIN_COLS_MOST; w >= SO_WIN_COLS_LEAST; w >>= 1)
        if (p.by_col + (int64_t)w * 8 <= p.budget) {
            p.win_cols = w;
            break;
        }
    p.cols_mode = p.win_cols > 0 && b_nnz < 0xffffffffll;
    p.win_long = p.cols_mode ? p.win_cols : SO_WIN_ENTRY;
    p.cap_long = p.cols_mode ? INT32_MAX : (int32_t)std::max<int64_t>(0, (p.budget - (int64_t)p.win_long * 8) / 8);
    p.lds_long = p.cols_mode ? (size_t)(p.by_col + (int64_t)p.win_long * 8) : (size_t)p.cap_long * 8 + (size_t)p.win_long * 8;
    p.win_mid = SO_MID / 32;
    p.cap_mid = SO_MID;
    p.lds_mid = (size_t)p.cap_mid * 8 + (size_t)p.win_mid * 8;
    p.lds_place = (size_t)SO_WIN_WORDS * 8;
    p.ok = (int64_t)p.lds_place + 2048 <= lds_max && p.cap_long >= SO_MID;
    return p;
}

// ---- what the call starts from --------------------------------------------------------------------------------------------
// a product of at most one entry, of no row, or of an A without entries is in order
inline bool nothing_to_order(int64_t c_nnz, int32_t c_nrows, int64_t a_nnz) { return c_nnz <= 1 || c_nrows == 0 || a_nnz == 0; }

// did the product kernels leave their own count of every row's products (a_nrows + 1 int64)?
inline bool products_counted(const void *p, size_t bytes, int32_t a_nrows) { return p && bytes >= (size_t)(a_nrows + 1) * 8; }

// so_row_products_kernel: a wavefront per row of A when the rows are long (a ratings matrix's), else sixteen lanes
inline bool wave_per_row(int64_t a_nnz, int32_t a_nrows) { return a_nnz / a_nrows >= 32; }

// the reference's order (1) unless CSRK_SPGEMM_ORDER begins with 'a', 'A' or '0' (0: ascending)
inline int order_from_knob(const char *e) { return !(e && (e[0] == 'a' || e[0] == 'A' || e[0] == '0')); }

// ---- grids: workgroups of 256 threads ---------------------------------------------------------------------------------------
inline unsigned grid_rows(int32_t nrows) { return (unsigned)cdiv(nrows, 256); }                                     // a thread per row
inline unsigned grid_lanes(int32_t nrows, int lanes) { return (unsigned)cdiv((int64_t)nrows * lanes, 256); }        // `lanes` threads per row
inline unsigned list_grid(int32_t a_nrows) { return grid_rows(a_nrows); }                                           // so_list_rows_kernel
inline unsigned products_grid(int32_t a_nrows, bool wave) { return grid_lanes(a_nrows, wave ? LANES : 16); }        // so_row_products_kernel
inline unsigned least_grid(int32_t a_nrows) { return grid_lanes(a_nrows, SO_SUB); }                                 // so_tiny_kernel on every row
inline unsigned wave_grid(int32_t n_wave) { return grid_lanes(n_wave, LANES); }                                     // on the listed rows below SO_WAVE
inline unsigned small_grid(int32_t n_small) { return grid_lanes(n_small, SO_SUB); }                                 // and below SO_TINY

// ---- byte sizes of the temporaries ------------------------------------------------------------------------------------------
inline size_t tp_bytes(int32_t a_nrows) { return (size_t)(a_nrows + 1) * 8; }      // products of every row, int64 (when not counted)
inline size_t flag_bytes() { return 4; }                                           // raised by an entry no product lands on
inline size_t rows_bytes(int32_t a_nrows) { return (size_t)a_nrows * 4 + 4; }      // the list of rows, longest first
inline size_t cursor_bytes() { return (SO_OCTAVES + 1) * 4; }                      // octave counters, then cursors; the memory flag
inline size_t oci_bytes(int64_t c_nnz) { return (size_t)c_nnz * 4; }               // the re-ordered columns
inline size_t ovs_bytes(int64_t c_nnz) { return (size_t)c_nnz * 8; }               // and values
inline size_t key_bytes(int64_t c_nnz) { return (size_t)c_nnz * 8; }               // 64-bit keys of the rows LDS does not hold

}  // namespace soplan
}  // namespace csrk
