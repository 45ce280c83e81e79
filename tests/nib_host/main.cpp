// Host check of the 8.5-byte entries of csr_amd/csrc/fix56.h (namespace nib) and of the rule that selects them
// (accgroups::choose_nib), built by tests/test_nib_host.py with the system compiler and -fsanitize=address,undefined:
// encode -> put -> get (the decode the product kernel runs) for every slot of a tile, compared bit for bit -- value, column
// and row step -- with padding entries among the values.
#include "acc_groups.h"
#include "fix56.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

using namespace csrk;
namespace nib = csrk::fix56::nib;

static int failures = 0;

struct Entry {
    double v;
    uint32_t col, step;
    bool pad;
};

// One tile's worth of `in` at a time (the last tile is short; its other slots keep what a zeroed tile holds), written in the
// order `stride` gives -- slot (k * stride) % 512 k-th, stride odd -- so that an entry's nibble is stored after and before its
// dword's other nibbles.  Every entry must come back: value bits, column, step; a padding entry as -0.0 on column PAD_COL.
static void check(const char *name, const std::vector<Entry> &in, int32_t g, int stride)
{
    size_t bad = 0;
    for (size_t i0 = 0; i0 < in.size(); i0 += fix56::TILE) {
        const int n = (int)(in.size() - i0 < (size_t)fix56::TILE ? in.size() - i0 : (size_t)fix56::TILE);
        std::vector<unsigned char> tile(nib::TILE_BYTES, 0xff);      // (stale bytes: put must not depend on a cleared tile)
        std::vector<uint16_t> idx(fix56::TILE, 0xffff);
        for (int k = 0; k < fix56::TILE; k++) {
            const int e = (int)(((int64_t)k * stride) % fix56::TILE);
            if (e >= n) continue;
            const Entry &q = in[i0 + (size_t)e];
            const uint64_t p = q.pad ? nib::PAD_CODE : fix56::encode(q.v, g);
            if ((p >> 52) & 7) bad++;
            nib::put(tile.data(), idx.data(), e, p, q.pad ? nib::PAD_COL : q.col, q.step);
        }
        for (int e = 0; e < n; e++) {
            const Entry &q = in[i0 + (size_t)e];
            uint32_t col = ~0u, step = ~0u;
            const double d = nib::get(tile.data(), idx.data(), e, g, col, step);
            const uint64_t want = q.pad ? 1ull << 63 : fix56::bits_of(q.v);
            if (fix56::bits_of(d) != want || col != (q.pad ? nib::PAD_COL : q.col) || step != q.step) bad++;
        }
    }
    if (bad) {
        printf("FAIL %s: %zu entries did not come back\n", name, bad);
        failures++;
        return;
    }
    printf("ok   %-28s g %d  (%zu entries, stride %d)\n", name, (int)g, in.size(), stride);
}

// values -> entries: columns and steps that sweep their fields (0 and 4095, 0 and 7 among them), a padding entry every
// `pad_every`-th slot (0: none)
static std::vector<Entry> entries(const std::vector<double> &v, int pad_every)
{
    std::vector<Entry> out;
    uint32_t h = 12345u;
    for (size_t i = 0; i < v.size(); i++) {
        h = h * 1664525u + 1013904223u;
        Entry q;
        q.v = v[i];
        q.col = i % 5 == 0 ? 4095u : i % 7 == 0 ? 0u : (h >> 8) & nib::COL_MASK;
        q.step = i % 3 == 0 ? 7u : (h >> 28) & nib::STEP_MASK;
        q.pad = pad_every && i % (size_t)pad_every == (size_t)pad_every - 1;
        out.push_back(q);
    }
    return out;
}

static int32_t grid_of(const std::vector<double> &v)
{
    fix56::Range r;
    for (double x : v) fix56::fold(r, x);
    int32_t g = 0;
    if (!fix56::packable(r, g)) {
        printf("FAIL a test set is not packable\n");
        failures++;
    }
    return g;
}

static void rule(const char *name, bool got, bool want)
{
    if (got != want) {
        printf("FAIL rule: %s\n", name);
        failures++;
    } else {
        printf("ok   rule: %s\n", name);
    }
}

int main()
{
    static_assert(nib::TILE_BYTES == 3328 && nib::HI_OFF == 3072 && nib::PAD_COL == 4096, "the layout the kernels load");
    const double top = (double)((1ull << 52) - 1);
    for (int g : {-52, 0, 3, -1074, 971}) {      // random grids: M uniform in (-2^52, 2^52), at several exponents
        std::vector<double> v;
        uint64_t h = 0x9e3779b97f4a7c15ull + (uint64_t)(g + 2000);
        for (int i = 0; i < 3000; i++) {
            h ^= h << 13;
            h ^= h >> 7;
            h ^= h << 17;
            const int64_t j = (int64_t)(h >> 11) - (1ll << 52);
            if (j == -(1ll << 52)) continue;
            v.push_back(std::ldexp((double)j, g));
        }
        v.push_back(std::ldexp(1.0, g));      // pins the grid's unit
        char name[64];
        snprintf(name, sizeof name, "random grid, g = %d", g);
        const int32_t gg = grid_of(v);
        if (gg != g) {
            printf("FAIL %s: grid %d\n", name, (int)gg);
            failures++;
        }
        check(name, entries(v, 0), gg, 1);
        check(name, entries(v, 9), gg, 509);
    }
    {
        // the extremes: +-(2^52 - 1) (every nibble bit set), +-1 (M = 1: the smallest value that is no padding entry), zeros
        std::vector<double> v;
        for (int i = 0; i < 512; i++) v.push_back(i % 4 == 0 ? top : i % 4 == 1 ? -top : i % 4 == 2 ? -1.0 : 1.0);
        check("extremes", entries(v, 0), grid_of(v), 1);
        check("extremes", entries(v, 3), grid_of(v), 255);
        std::vector<double> z(700, 0.0);
        z[5] = 1.0;
        check("zeros", entries(z, 0), grid_of(z), 1);
        check("zeros and padding", entries(z, 2), grid_of(z), 3);
        // a negative value whose low 48 bits are zero: only the nibble tells it from a padding entry
        std::vector<double> n(512, -std::ldexp(1.0, 48));
        n[0] = 1.0;
        check("sign and nibble only", entries(n, 0), grid_of(n), 1);
        // ... one whose low word alone is set, one with the 16-bit plane alone
        std::vector<double> m(512, -1.0);
        for (int i = 0; i < 512; i += 2) m[(size_t)i] = -std::ldexp(1.0, 32);
        check("sign and one plane only", entries(m, 4), grid_of(m), 7);
    }
    {
        // a whole tile of padding entries, and a tile whose every slot is one
        std::vector<Entry> pads(512, Entry{0.0, 0u, 7u, true});
        pads[0].step = 0;
        check("padding only", pads, 0, 1);
    }
    // the selection rule: 16 whole tiles per workgroup, unless the knob decides
    using accgroups::choose_nib;
    rule("unset, 16 tiles per workgroup", choose_nib(-1, 16ll * 512 * 256, 256), true);
    rule("unset, one entry short", choose_nib(-1, 16ll * 512 * 256 - 1, 256), false);
    rule("unset, the headline tier", choose_nib(-1, 148200000ll, 256), true);
    rule("unset, a test matrix", choose_nib(-1, 60 * 512, 256), false);
    rule("unset, nothing", choose_nib(-1, 0, 256), false);
    rule("unset, no workgroups counts as one", choose_nib(-1, 16 * 512, 0), true);
    rule("unset, beyond 2^31 entries", choose_nib(-1, 1ll << 40, 304), true);
    rule("knob 1, small", choose_nib(1, 1, 256), true);
    rule("knob 0, large", choose_nib(0, 1ll << 40, 256), false);
    if (failures) {
        printf("%d case(s) failed\n", failures);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
