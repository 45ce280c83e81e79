// Host check of csr_amd/csrc/fix56.h, built by tests/test_fix56_host.py with the system compiler and
// -fsanitize=address,undefined: the grid test, and encode -> tile planes -> decode compared bit for bit.
#include "fix56.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

using namespace csrk;

static int failures = 0;

// grid test over `v`; when packable: every value through a tile (put / get, every slot of the tile in turn) and back
static void check(const char *name, const std::vector<double> &v, bool want_packable, int want_g = INT32_MIN)
{
    fix56::Range r;
    for (size_t lo = 0; lo < v.size(); lo += 1000) {      // folded in pieces and merged, as a reduction does
        fix56::Range part;
        for (size_t i = lo; i < v.size() && i < lo + 1000; i++) fix56::fold(part, v[i]);
        fix56::merge(r, part);
    }
    int32_t g = 0;
    const bool ok = fix56::packable(r, g);
    if (ok != want_packable || (ok && want_g != INT32_MIN && g != want_g)) {
        printf("FAIL %s: packable %d (want %d), g %d (want %d)\n", name, (int)ok, (int)want_packable, (int)g, want_g);
        failures++;
        return;
    }
    size_t bad = 0;
    if (ok) {
        std::vector<unsigned char> tile(fix56::TILE_BYTES);
        for (size_t i0 = 0; i0 < v.size(); i0 += fix56::TILE) {
            const size_t n = v.size() - i0 < (size_t)fix56::TILE ? v.size() - i0 : (size_t)fix56::TILE;
            for (size_t e = 0; e < n; e++) {
                const uint64_t p = fix56::encode(v[i0 + e], g);
                if ((p >> 52) & 7) bad++;                  // bits 52..54 stay zero
                fix56::put(tile.data(), (int)e, p);
            }
            for (size_t e = 0; e < n; e++)
                if (fix56::bits_of(fix56::get(tile.data(), (int)e, g)) != fix56::bits_of(v[i0 + e])) bad++;
        }
        if (bad) {
            printf("FAIL %s: %zu values did not come back bit for bit\n", name, bad);
            failures++;
            return;
        }
    }
    printf("ok   %-28s packable %d  g %d  (%zu values)\n", name, (int)ok, (int)g, v.size());
}

int main()
{
    // the synthetic generator's form: j * 2^-52, |j| < 2^52 (53 hashed bits mapped to (-1, 1))
    {
        std::vector<double> v;
        uint64_t h = 0x9e3779b97f4a7c15ull;
        for (int i = 0; i < 100000; i++) {
            h ^= h << 13;
            h ^= h >> 7;
            h ^= h << 17;
            const int64_t j = (int64_t)(h >> 11) - (1ll << 52);      // [-2^52, 2^52)
            if (j == -(1ll << 52)) continue;
            v.push_back(std::ldexp((double)j, -52));
        }
        v.push_back(std::ldexp(1.0, -52));      // the grid's unit itself
        check("j * 2^-52", v, true, -52);
    }
    const double top = (double)((1ull << 52) - 1);
    check("M = 2^52 - 1", {1.0, top, -top, 3.0, 0.0}, true, 0);
    check("M = 2^52", {1.0, top, (double)(1ull << 52)}, false);
    check("all zeros", std::vector<double>(700, 0.0), true, 0);
    check("one -0.0", {1.0, 2.0, -0.0, 3.0}, false);
    check("one NaN", {1.0, 2.0, std::numeric_limits<double>::quiet_NaN(), 3.0}, false);
    check("one Inf", {1.0, 2.0, -std::numeric_limits<double>::infinity(), 3.0}, false);
    check("1/3 among grid values", {0.25, 0.5, 1.0 / 3.0, 7.0}, false);
    {
        const double d = std::numeric_limits<double>::denorm_min();      // 5e-324 = 2^-1074
        std::vector<double> v;
        for (int k = 1; k < 2000; k++) v.push_back((k & 1 ? 1.0 : -1.0) * d * (double)k * 977.0);
        v.push_back(d);
        v.push_back(std::ldexp(1.0, -1023) + d);               // a subnormal with its top bit set
        v.push_back(std::ldexp(1.0, -1022));                   // the smallest normal number: M = 2^52, off the grid's range
        check("subnormal grid, too wide", v, false);
        v.pop_back();
        check("subnormal grid", v, true, -1074);
    }
    {
        std::vector<double> v;
        for (int k = 1; k < 2000; k++) v.push_back(std::ldexp((k & 1 ? 1.0 : -1.0) * (double)(2 * k + 1), 971));
        v.push_back(std::ldexp(top, 971));                       // the largest packable magnitude there is
        check("huge grid, g = 971", v, true, 971);
    }
    check("g = 972: 1075 + g > 2046", {std::ldexp(1.0, 972), std::ldexp(3.0, 972)}, false);
    check("g = 1000", {std::ldexp(1.0, 1000)}, false);
    check("float32 values", {(double)0.1f, (double)-3.7f, (double)1e-3f, (double)123.456f}, true);
    if (failures) {
        printf("%d case(s) failed\n", failures);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
