// The stable radix sort's host decisions (transpose.hip: sort_records; DESIGN.md section 5, "The driver"): the constants the
// kernels share with them and one pure function per decision -- the route, the chunks, the byte size of every temporary, the
// grid of every launch, the pass schedule of the plain routes -- and radix_plan(), which states them all for one sort.  Plain
// host arithmetic in the integer types and expressions the driver always used, no device code, no allocation and no call
// into the runtime: transpose.hip reads the plan and decides nothing itself, and tests/radix_plan_host runs the header as a
// stand-alone program -- at every rule's edge, and on every case of tests/radix_cases.py against that module's route().
#pragma once
#include <cstddef>
#include <cstdint>

namespace csrk {

// ---- the constants the kernels are written for ------------------------------------------------------------------------
#ifndef CSRK_RX_THREADS
#define CSRK_RX_THREADS 512
#endif
constexpr int RX_THREADS = CSRK_RX_THREADS;
constexpr int RX_ROUNDS = 8;
constexpr int RX_CHUNK = RX_THREADS * RX_ROUNDS;     // 4096 records per workgroup (8192: 0.67 vs 0.65 ms)
constexpr int RX_HC = 4;                             // chunks per workgroup of the histogram (rx_hist_kernel)
constexpr int RXS_THREADS = 1024;                    // the table scan (rx_scan_kernel): one workgroup per digit,
constexpr int RXS_IPT = 8;                           // RXS_THREADS * RXS_IPT chunks per trip
constexpr int RX_PACKED_SHIFT = 24;                  // the packed word: the key's high digit in bits 31..24, the payload below

namespace radixplan {

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- the route: a function of the key range and the payload range alone ---------------------------------------------
// bits = ceil(log2(key range)), at most 31: keys are non-negative int32
inline int key_bits(int32_t key_range)
{
    int bits = 0;
    while (bits < 31 && (1ll << bits) < (int64_t)key_range) bits++;
    return bits;
}
// 8-bit digits
inline int passes(int bits) { return bits <= 8 ? 1 : (bits + 7) / 8; }

enum class Route { Empty, One, Packed, Plain2, Three, Four };
constexpr int64_t PACKED_PAYLOADS = 1ll << 24;       // two passes with payloads below it: the payload fits the packed word
inline Route route(int64_t n, int32_t key_range, int64_t payload_range)
{
    if (n == 0) return Route::Empty;
    const int p = passes(key_bits(key_range));
    if (p == 2) return payload_range <= PACKED_PAYLOADS ? Route::Packed : Route::Plain2;
    return p == 1 ? Route::One : (p == 3 ? Route::Three : Route::Four);
}

// ---- chunks -----------------------------------------------------------------------------------------------------------
inline int64_t chunks(int64_t n) { return cdiv(n, RX_CHUNK); }
// The packed route's second pass cuts every run of equal low digits into chunks of its own (rx_align_kernel): the full
// chunks of all runs are at most n / RX_CHUNK, and each of the 256 runs ends in at most one partial chunk more.
inline int64_t aligned_capacity(int64_t n_chunks) { return n_chunks + 256; }

// ---- byte sizes of the temporaries --------------------------------------------------------------------------------------
inline size_t table_bytes(int64_t n_chunks) { return (size_t)(256 * n_chunks + 1) * 8; }      // (digit, chunk) counts, int64
inline size_t total_bytes() { return 256 * 8; }                                               // a count per digit
inline size_t bound_bytes(int64_t n_chunks) { return (size_t)n_chunks * 4; }                  // first / last source row per chunk
inline size_t cstart_bytes(int64_t cap) { return (size_t)cap * 8; }                           // chunk descriptors: first record,
inline size_t ccnt_bytes(int64_t cap) { return (size_t)cap * 4; }                             // record count
inline size_t run0_bytes() { return 257 * 8; }                                                // first chunk of every run, and the end
inline size_t word_bytes(int64_t n) { return (size_t)n * 4; }                                 // keys or payloads
inline size_t value_bytes(int64_t n) { return (size_t)n * 8; }                                // float64 values

// ---- grids ------------------------------------------------------------------------------------------------------------
constexpr unsigned SCAN_GRID = 256, ALIGN_GRID = 1;                                           // a workgroup per digit; one workgroup
inline unsigned bounds_grid(int64_t n_chunks) { return (unsigned)cdiv(n_chunks, 256); }       // a thread per chunk
inline unsigned hist_grid(int64_t n_chunks) { return (unsigned)cdiv(n_chunks, RX_HC); }
inline unsigned scatter_grid(int64_t n_chunks) { return (unsigned)(8 * cdiv(n_chunks, 8)); }  // padded to the 8 XCDs (rx_chunk_of)
inline unsigned ptr_table_grid(int32_t key_range) { return (unsigned)cdiv((int64_t)key_range + 1, 256); }      // a thread per pointer
inline unsigned ptr_keys_grid(int64_t n) { return (unsigned)cdiv(cdiv(n + 1, 4), 256); }      // four positions per thread, position n too

// ---- the pass schedule of the plain routes --------------------------------------------------------------------------------
// Pass p sorts by bits 8 p .. 8 p + 7.  The first reads the caller's arrays, the last writes the sorted keys (keyL) and the
// caller's outputs; between them the records go A, B, A.
enum Where { Source = 0, A = 1, B = 2, Last = 3 };
struct Pass {
    int shift;
    bool first;      // reads the caller's arrays (a CSR's, or the given keys / payloads / values in their own dtype)
    Where src, dst;
};
inline Pass pass_of(int p, int n_passes)
{
    Pass s;
    s.shift = 8 * p;
    s.first = p == 0;
    s.src = p == 0 ? Source : (((p - 1) & 1) ? B : A);
    s.dst = p == n_passes - 1 ? Last : ((p & 1) ? B : A);
    return s;
}

// ---- one sort ---------------------------------------------------------------------------------------------------------
struct Buf {
    bool used = false;      // the route requests it
    size_t bytes = 0;
};
struct Grids {
    unsigned bounds, hist, scatter, hist2, scatter2, ptr_table, ptr_keys;      // hist2 / scatter2: the aligned second pass
};
struct Plan {
    Route route = Route::Empty;
    bool packed = false;
    int bits = 0, passes = 0;
    size_t ptr_slots = 0;          // Empty only: run starts to clear
    int64_t chunks = 0;            // plain chunks: records [c * RX_CHUNK, (c + 1) * RX_CHUNK)
    int64_t chunks2 = 0;           // chunks behind the table: the descriptor capacity on the packed route, else `chunks`
    Buf table, total;              // every route
    Buf rlo, rhi;                  // a CSR's source rows per chunk
    Buf cstart, ccnt, run0, total2;      // packed
    Buf keyL;                      // plain: the last pass's sorted keys
    Buf keyA, rowA, valA;          // plain with two passes or more; packed: rowA holds the words, no keyA
    Buf keyB, rowB, valB;          // plain with three passes or more
    Grids grid = {};
    Pass pass[4] = {};             // plain: pass[0 .. passes)
};

inline Buf want(bool used, size_t bytes) { return used ? Buf{true, bytes} : Buf{}; }

inline Plan radix_plan(int64_t n, int32_t key_range, int64_t payload_range, bool from_csr, bool has_values)
{
    Plan pl;
    pl.route = route(n, key_range, payload_range);
    if (pl.route == Route::Empty) {
        pl.ptr_slots = (size_t)(key_range + 1);
        return pl;
    }
    pl.bits = key_bits(key_range);
    pl.passes = passes(pl.bits);
    pl.packed = pl.route == Route::Packed;
    pl.chunks = chunks(n);
    pl.chunks2 = pl.packed ? aligned_capacity(pl.chunks) : pl.chunks;
    const bool plain = !pl.packed;

    pl.table = want(true, table_bytes(pl.chunks2));
    pl.total = want(true, total_bytes());
    pl.rlo = pl.rhi = want(from_csr, bound_bytes(pl.chunks));
    pl.cstart = want(pl.packed, cstart_bytes(pl.chunks2));
    pl.ccnt = want(pl.packed, ccnt_bytes(pl.chunks2));
    pl.run0 = want(pl.packed, run0_bytes());
    pl.total2 = want(pl.packed, total_bytes());
    pl.keyL = want(plain, word_bytes(n));
    pl.keyA = want(plain && pl.passes > 1, word_bytes(n));
    pl.rowA = want(pl.packed || pl.passes > 1, word_bytes(n));
    pl.valA = want((pl.packed || pl.passes > 1) && has_values, value_bytes(n));
    pl.keyB = pl.rowB = want(plain && pl.passes > 2, word_bytes(n));
    pl.valB = want(plain && pl.passes > 2 && has_values, value_bytes(n));

    pl.grid.bounds = bounds_grid(pl.chunks);
    pl.grid.hist = hist_grid(pl.chunks);
    pl.grid.scatter = scatter_grid(pl.chunks);
    pl.grid.hist2 = hist_grid(pl.chunks2);
    pl.grid.scatter2 = scatter_grid(pl.chunks2);
    pl.grid.ptr_table = ptr_table_grid(key_range);
    pl.grid.ptr_keys = ptr_keys_grid(n);
    if (plain)
        for (int p = 0; p < pl.passes; p++) pl.pass[p] = pass_of(p, pl.passes);
    return pl;
}

}  // namespace radixplan
}  // namespace csrk
