// fix56: float64 values that lie on ONE binary grid, kept in 7 bytes and decoded by one float64 add.
//
// A set of doubles is PACKABLE when every value is finite, none is -0.0, and with g = the lowest set bit over all
// non-zero values (as an exponent of two) every non-zero value is +-M * 2^g with an integer M < 2^52, and the "magic"
// constant 2^(52 + g) is a normal number (1 <= 1075 + g <= 2046).  Ratings, counts, fixed-point data, anything that was
// float32 once and a uniform variate drawn as j * 2^-52 are of this kind.  A zero packs as M = 0; a set without non-zero
// values takes g = 0.
//
// Stored form, 56 bits: M in bits 0..51, bits 52..54 zero, the sign in bit 55 -- as three planes, a 32-bit word (M[31:0]),
// a 16-bit word (M[47:32]) and a byte (sign << 7 | M[51:48]).
//
// Decode, exact arithmetic only: the double with exponent field 1075 + g and mantissa M IS 2^(52 + g) + M * 2^g, so
//     d = as_double(((1075 + g) << 20) | M[51:32], M[31:0]) - 2^(52 + g)
// is M * 2^g without rounding (Sterbenz-like: the result is representable), and the sign is xor-ed into its top bit.  No
// integer-to-double conversion, one v_add_f64 against a constant.
//
// The header compiles as plain C++ (the plan's host side, the host test) and as HIP device code (the product kernels,
// the fill and verification kernels): both run the same routines.
//
// Namespace nib at the end: the same values in 6.5 bytes, with the sign moved into the stream's index word (8.5 B per entry).
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define FIX56_HD __host__ __device__ __forceinline__
#else
#define FIX56_HD inline
#endif

namespace csrk {
namespace fix56 {

constexpr int TILE = 512;                                // entries per tile (ACC_TILE)
constexpr int LO_BYTES = TILE * 4, MID_BYTES = TILE * 2, HI_BYTES = TILE;
constexpr int MID_OFF = LO_BYTES, HI_OFF = LO_BYTES + MID_BYTES;
constexpr int TILE_BYTES = LO_BYTES + MID_BYTES + HI_BYTES;      // 3584 instead of 4096
constexpr uint64_t MANT_MASK = (1ull << 52) - 1;
constexpr uint32_t W_MANT = 0x000fffffu, W_SIGN = 0x00800000u;  // the word {0, byte plane, 16-bit plane}: M[51:32], sign

// one stored value: sizeof = 7, so that pointer arithmetic in entries lands on tile starts (512 * 7 = TILE_BYTES)
struct Packed {
    unsigned char b[7];
};
static_assert(sizeof(Packed) * TILE == TILE_BYTES, "a tile of Packed entries is the three planes");

FIX56_HD uint64_t bits_of(double v)
{
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
}
FIX56_HD double double_of(uint32_t hi, uint32_t lo)
{
    const uint64_t b = ((uint64_t)hi << 32) | lo;
    double v;
    memcpy(&v, &b, 8);
    return v;
}
FIX56_HD int ctz64(uint64_t x) { return __builtin_ctzll(x); }
FIX56_HD int msb64(uint64_t x) { return 63 - __builtin_clzll(x); }

// What a set's grid test needs to know, folded value by value (fold) and set by set (merge): whether a value rules packing
// out by itself (NaN, Inf, -0.0), the lowest set bit of any non-zero value and the highest, as exponents of two.
struct Range {
    int32_t bad = 0, lo = INT32_MAX, hi = INT32_MIN;
};
// integer significand and the exponent of its unit: |v| = sig * 2^unit (v finite and non-zero)
FIX56_HD void split(uint64_t bits, uint64_t &sig, int &unit)
{
    const int e = (int)((bits >> 52) & 0x7ff);
    sig = (bits & MANT_MASK) | (e ? 1ull << 52 : 0ull);
    unit = (e ? e : 1) - 1075;
}
FIX56_HD void fold(Range &r, double v)
{
    const uint64_t b = bits_of(v);
    if (b == 0) return;                                                  // +0.0: M = 0 on every grid
    if (((b >> 52) & 0x7ff) == 0x7ff || b == 1ull << 63) {
        r.bad = 1;
        return;
    }
    uint64_t sig;
    int unit;
    split(b, sig, unit);
    const int lo = unit + ctz64(sig), hi = unit + msb64(sig);
    r.lo = lo < r.lo ? lo : r.lo;
    r.hi = hi > r.hi ? hi : r.hi;
}
FIX56_HD void merge(Range &r, const Range &o)
{
    r.bad |= o.bad;
    r.lo = o.lo < r.lo ? o.lo : r.lo;
    r.hi = o.hi > r.hi ? o.hi : r.hi;
}
// the grid test: true and the grid's exponent g when the set behind `r` is packable
FIX56_HD bool packable(const Range &r, int32_t &g)
{
    g = 0;
    if (r.bad) return false;
    if (r.lo > r.hi) return true;                                        // no non-zero value
    g = r.lo;
    return r.hi - g < 52 && 1075 + g >= 1 && 1075 + g <= 2046;
}

// v (a member of a packable set with grid exponent g) -> its 56 bits
FIX56_HD uint64_t encode(double v, int32_t g)
{
    const uint64_t b = bits_of(v);
    if ((b << 1) == 0) return 0;
    uint64_t sig;
    int unit;
    split(b, sig, unit);
    const uint64_t M = unit >= g ? sig << (unit - g) : sig >> (g - unit);
    return M | (b >> 63) << 55;
}
// the three planes' shares of the 56 bits
FIX56_HD uint32_t lo_of(uint64_t p) { return (uint32_t)p; }
FIX56_HD uint16_t mid_of(uint64_t p) { return (uint16_t)(p >> 32); }
FIX56_HD unsigned char hi_of(uint64_t p) { return (unsigned char)(p >> 48); }

// The decode every reader uses.  lo = the 32-bit plane's word, w = {0, the byte plane's byte, the 16-bit plane's word},
// ebits = (1075 + g) << 20, magic = 2^(52 + g) = as_double(ebits, 0).
FIX56_HD double decode(uint32_t lo, uint32_t w, uint32_t ebits, double magic)
{
    const double d = double_of((w & W_MANT) | ebits, lo) - magic;
    return double_of((uint32_t)(bits_of(d) >> 32) ^ ((w & W_SIGN) << 8), (uint32_t)bits_of(d));
}
FIX56_HD uint32_t ebits_of(int32_t g) { return (uint32_t)(1075 + g) << 20; }
FIX56_HD double magic_of(int32_t g) { return double_of(ebits_of(g), 0u); }

// where entry e (0..511: lane = e / 8, j = e % 8) of a tile sits in each plane: a lane's eight 32-bit words come by two
// 16-B loads (like the index words of the light stream), its eight 16-bit words by one, its eight bytes by one 8-B load
FIX56_HD int lo_slot(int e) { return ((e & 7) >> 2) * 256 + (e >> 3) * 4 + (e & 3); }

// store / fetch one entry of the tile at `tile` (scalar forms: the plan's fill kernel, the host test)
FIX56_HD void put(unsigned char *tile, int e, uint64_t p)
{
    ((uint32_t *)tile)[lo_slot(e)] = lo_of(p);
    ((uint16_t *)(tile + MID_OFF))[e] = mid_of(p);
    tile[HI_OFF + e] = hi_of(p);
}
FIX56_HD double get(const unsigned char *tile, int e, int32_t g)
{
    const uint32_t lo = ((const uint32_t *)tile)[lo_slot(e)];
    const uint32_t w = (uint32_t)((const uint16_t *)(tile + MID_OFF))[e] | (uint32_t)tile[HI_OFF + e] << 16;
    return decode(lo, w, ebits_of(g), magic_of(g));
}

// nib: the same values in 6.5 bytes beside a 16-bit index word that carries their sign -- 8.5 B per entry of tier 0's stream
// instead of 9.  The 56-bit form holds three bits that are always zero, and the stream's index word spends its 13th column
// bit only on the window's zero slot (padding entries).  So per 512-entry tile:
//     32-bit plane  M[31:0]    2048 B   as above (lo_slot)
//     16-bit plane  M[47:32]   1024 B   as above
//      4-bit plane  M[51:48]    256 B   a lane's eight nibbles in one dword: entry e in dword e / 8, bits 4 (e % 8) ..
//     index word    {sign : 1, row step : 3, column in block : 12}, 1024 B, an array of its own
// A packable set holds no -0.0, so "sign set, M = 0" is free: it marks a PADDING entry, which the reader sends to column
// PAD_COL (the zero slot) whatever its column field says.  It decodes to -0.0, and -0.0 * 0.0 = -0.0 added to a run sum leaves
// that sum's bits alone: a run sum starts at +0.0, +0.0 + -0.0 = +0.0 in round-to-nearest, and a sum of two doubles is -0.0
// only when both are -- so no run sum is ever -0.0, and x + -0.0 = x for every other x.  (The raw stream's padding adds
// +0.0 * 0.0 = +0.0, which likewise changes nothing: x + +0.0 = x unless x is -0.0.)
namespace nib {

constexpr int LO_BYTES = TILE * 4, MID_BYTES = TILE * 2, HI_BYTES = TILE / 2;
constexpr int MID_OFF = LO_BYTES, HI_OFF = LO_BYTES + MID_BYTES;
constexpr int TILE_BYTES = LO_BYTES + MID_BYTES + HI_BYTES;      // 3328: 6.5 B per entry, so tiles are addressed by byte offset
constexpr int COL_BITS = 12, STEP_SHIFT = 12;
constexpr uint32_t COL_MASK = (1u << COL_BITS) - 1, STEP_MASK = 7u, SIGN = 1u << 15;
constexpr uint32_t PAD_COL = 1u << COL_BITS;                     // the column a padding entry reads: the window's zero slot
constexpr uint64_t PAD_CODE = 1ull << 55;                        // encode()'s form of "sign set, M = 0"

// a stream of such tiles: sizeof = 1, pointer arithmetic is in bytes
struct Bytes {
    unsigned char b;
};

// the index word of an entry whose value encodes as p (encode(), or PAD_CODE for a padding entry, whose column field is 0)
FIX56_HD uint16_t index_word(uint64_t p, uint32_t col, uint32_t step)
{
    const bool pad = p == PAD_CODE;
    return (uint16_t)((pad ? 0u : col & COL_MASK) | (step & STEP_MASK) << STEP_SHIFT | (uint32_t)(p >> 55) << 15);
}
// where entry e's nibble sits in the 4-bit plane
FIX56_HD int hi_word(int e) { return e >> 3; }
FIX56_HD int hi_shift(int e) { return (e & 7) * 4; }
FIX56_HD uint32_t hi_of(uint64_t p) { return (uint32_t)(p >> 48) & 0xfu; }

// a double from its two words and back, without a 64-bit integer in between (little-endian, like every target of this code)
FIX56_HD double join(uint32_t hi, uint32_t lo)
{
    const uint32_t t[2] = {lo, hi};
    double v;
    memcpy(&v, t, 8);
    return v;
}
FIX56_HD uint32_t high_of(double v)
{
    uint32_t t[2];
    memcpy(t, &v, 8);
    return t[1];
}

// The decode every reader uses.  lo = the 32-bit plane's word, hi = ebits | M[51:32] (the exponent field of 2^(52 + g) over the
// nibble over the 16-bit plane's word: the high word of the double 2^(52 + g) + M * 2^g), word = the index word.  Returns the
// value; col = the window slot to read (PAD_COL for a padding entry), step = the row step.
FIX56_HD double entry(uint32_t lo, uint32_t hi, uint32_t word, double magic, uint32_t &col, uint32_t &step)
{
    // d = M * 2^g >= +0.0 (x - x is +0.0 in round-to-nearest): its sign bit is clear and the stored sign is or-ed in.  "Sign
    // set, M = 0" then IS the double -0.0, which no packable set holds: one 64-bit compare finds a padding entry.
    const double d = join(hi, lo) - magic;
    const double a = join(high_of(d) | ((word << 16) & 0x80000000u), (uint32_t)bits_of(d));
    col = bits_of(a) == 1ull << 63 ? PAD_COL : word & COL_MASK;
    step = (word >> STEP_SHIFT) & STEP_MASK;
    return a;
}

// store / fetch one entry of the value tile at `tile` and of the tile's 512 index words at `idx` (scalar forms: the host
// test; the plan's fill kernel stores the planes the same way but ors the nibble in atomically, its lanes sharing dwords)
FIX56_HD void put(unsigned char *tile, uint16_t *idx, int e, uint64_t p, uint32_t col, uint32_t step)
{
    ((uint32_t *)tile)[lo_slot(e)] = lo_of(p);
    ((uint16_t *)(tile + MID_OFF))[e] = mid_of(p);
    uint32_t *h = (uint32_t *)(tile + HI_OFF) + hi_word(e);
    *h = (*h & ~(0xfu << hi_shift(e))) | hi_of(p) << hi_shift(e);
    idx[e] = index_word(p, col, step);
}
FIX56_HD double get(const unsigned char *tile, const uint16_t *idx, int e, int32_t g, uint32_t &col, uint32_t &step)
{
    const uint32_t lo = ((const uint32_t *)tile)[lo_slot(e)];
    const uint32_t nibble = (((const uint32_t *)(tile + HI_OFF))[hi_word(e)] >> hi_shift(e)) & 0xfu;
    const uint32_t w = (uint32_t)((const uint16_t *)(tile + MID_OFF))[e] | nibble << 16;
    return entry(lo, w | ebits_of(g), idx[e], magic_of(g), col, step);
}

}  // namespace nib

}  // namespace fix56
}  // namespace csrk
