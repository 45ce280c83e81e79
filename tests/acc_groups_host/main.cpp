// Host check of csr_amd/csrc/acc_groups.h, built by tests/test_acc_groups_host.py with the system compiler and
// -fsanitize=address,undefined: tier 0's rows dealt to groups and launches, the workgroups each group gets, and the
// placement of the (group, workgroup) pairs on the blocks of one launch.
#include "acc_groups.h"

#include <cstdio>
#include <random>
#include <set>

using namespace csrk;

static int failures = 0;

#define EXPECT(cond, ...)                                                                                              \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            printf("FAIL %s:%d: ", __FILE__, __LINE__);                                                                \
            printf(__VA_ARGS__);                                                                                       \
            printf("\n");                                                                                              \
            failures++;                                                                                                \
            return;                                                                                                    \
        }                                                                                                              \
    } while (0)

// every row in exactly one group, groups ascending and within `cap`, launches of at most G groups; G > 1: a launch takes
// the longest rows left, and its groups' sizes and entry sums are level
static void check_deal(const char *name, const std::vector<int64_t> &lens, int G, int32_t cap, size_t want_groups,
                       size_t want_launches)
{
    const int32_t n = (int32_t)lens.size();
    const accgroups::Deal d = accgroups::deal_rows(lens.data(), n, G, cap);
    EXPECT(d.groups.size() == want_groups, "%s: %zu groups, want %zu", name, d.groups.size(), want_groups);
    EXPECT(d.first.size() == want_launches + 1, "%s: %zu launches, want %zu", name, d.first.size() - 1, want_launches);
    EXPECT(d.first.front() == 0 && d.first.back() == (int32_t)d.groups.size(), "%s: launch table ends", name);
    std::vector<int> seen((size_t)n, 0);
    for (const std::vector<int32_t> &g : d.groups) {
        EXPECT(!g.empty() && (int32_t)g.size() <= cap, "%s: a group of %zu rows (cap %d)", name, g.size(), (int)cap);
        for (size_t i = 0; i < g.size(); i++) {
            EXPECT(g[i] >= 0 && g[i] < n, "%s: position %d out of range", name, (int)g[i]);
            EXPECT(i == 0 || g[i - 1] < g[i], "%s: a group is not ascending", name);
            seen[(size_t)g[i]]++;
        }
    }
    for (int32_t i = 0; i < n; i++) EXPECT(seen[(size_t)i] == 1, "%s: row %d is in %d groups", name, (int)i, seen[(size_t)i]);
    int64_t floor_prev = INT64_MAX;
    for (size_t j = 0; j + 1 < d.first.size(); j++) {
        const int gb = d.first[j + 1] - d.first[j];
        EXPECT(gb >= 1 && gb <= (G < 1 ? 1 : G), "%s: a launch of %d groups", name, gb);
        if (G <= 1) continue;
        size_t smin = SIZE_MAX, smax = 0;
        int64_t longest = 0, shortest = INT64_MAX, emin = INT64_MAX, emax = 0;
        for (int k = d.first[j]; k < d.first[j + 1]; k++) {
            int64_t e = 0;
            for (int32_t i : d.groups[(size_t)k]) {
                e += lens[(size_t)i];
                longest = std::max(longest, lens[(size_t)i]);
                shortest = std::min(shortest, lens[(size_t)i]);
            }
            smin = std::min(smin, d.groups[(size_t)k].size());
            smax = std::max(smax, d.groups[(size_t)k].size());
            emin = std::min(emin, e);
            emax = std::max(emax, e);
        }
        EXPECT(smax - smin <= 1, "%s: group sizes %zu .. %zu in one launch", name, smin, smax);
        EXPECT(longest <= floor_prev, "%s: launch %zu holds a longer row than the one before", name, j);
        // dealt by rank: a group's sum exceeds another's by less than the launch's longest row
        EXPECT(emax - emin <= longest, "%s: entries %lld .. %lld in one launch", name, (long long)emin, (long long)emax);
        floor_prev = shortest;
    }
    printf("ok   %-34s %zu groups in %zu launches\n", name, d.groups.size(), d.first.size() - 1);
}

// every (group, workgroup) on exactly one block; workgroup w of every group on blocks equal mod XCDS, but for the few that
// an uneven split leaves over (`late_max`)
static void check_place(const char *name, int32_t cus, int gb, size_t late_max)
{
    int32_t n_wg[accgroups::MAX_GROUPS] = {0, 0, 0};
    int64_t total = 0;
    for (int g = 0; g < gb; g++) {
        n_wg[g] = accgroups::group_wgs(cus, gb, g);
        EXPECT(n_wg[g] >= 1 && (g == 0 || n_wg[g] <= n_wg[g - 1]), "%s: shares", name);
        total += n_wg[g];
    }
    EXPECT(total == (cus >= gb ? cus : gb), "%s: %lld workgroups for %d CUs", name, (long long)total, (int)cus);
    const std::vector<uint32_t> map = accgroups::place_wgs(n_wg, gb);
    EXPECT((int64_t)map.size() == total, "%s: %zu blocks", name, map.size());
    std::set<uint32_t> ids;
    size_t late = 0;
    int64_t per_xcd[accgroups::XCDS] = {};
    for (size_t b = 0; b < map.size(); b++) {
        const uint32_t g = map[b] >> 16, w = map[b] & 0xffffu;
        EXPECT((int)g < gb && (int32_t)w < n_wg[g], "%s: block %zu -> (%u, %u)", name, b, g, w);
        EXPECT(ids.insert(map[b]).second, "%s: (%u, %u) placed twice", name, g, w);
        late += (w % accgroups::XCDS) != (b % accgroups::XCDS);
        per_xcd[b % accgroups::XCDS]++;
    }
    for (int c = 0; c < accgroups::XCDS; c++)
        EXPECT(per_xcd[c] <= (total + accgroups::XCDS - 1) / accgroups::XCDS, "%s: XCD share", name);
    EXPECT(late <= late_max, "%s: %zu workgroups away from their XCD (at most %zu)", name, late, late_max);
    printf("ok   %-34s %lld blocks, %zu off their XCD\n", name, (long long)total, late);
}

int main()
{
    std::mt19937_64 rng(27);
    auto lens_of = [&](size_t n, int64_t lo, int64_t hi) {
        std::vector<int64_t> v(n);
        for (int64_t &x : v) x = lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1));
        return v;
    };
    check_deal("no rows", {}, 2, 16, 0, 0);
    check_deal("one group, as ever", lens_of(123, 64, 3000), 1, 15936, 1, 1);
    check_deal("G = 1, ranges of 40", lens_of(123, 64, 3000), 1, 40, 4, 4);
    check_deal("G = 2, rows fit one group", lens_of(123, 64, 3000), 2, 123, 1, 1);
    check_deal("G = 2, cap 41: 82 + 41", lens_of(123, 64, 3000), 2, 41, 3, 2);
    check_deal("G = 3, cap 41: exactly full", lens_of(123, 64, 3000), 3, 41, 3, 1);
    check_deal("G = 3, cap 40: 120 + 3", lens_of(123, 64, 3000), 3, 40, 4, 2);
    check_deal("G = 3, cap 61: three of 41", lens_of(123, 64, 3000), 3, 61, 3, 1);
    check_deal("G = 2, cap 61: 122 + 1", lens_of(123, 64, 3000), 2, 61, 3, 2);
    check_deal("G = 2, cap 16", lens_of(123, 64, 3000), 2, 16, 8, 4);
    check_deal("G = 3, cap 1", lens_of(7, 64, 70), 3, 1, 7, 3);
    check_deal("equal lengths", std::vector<int64_t>(100, 64), 3, 20, 5, 2);
    check_deal("G beyond the limit", lens_of(50, 64, 900), 9, 10, 5, 2);
    check_deal("headline-sized", lens_of(47808, 238, 2000000), 3, 15936, 3, 1);

    check_place("256 CUs, 2 groups", 256, 2, 0);
    check_place("256 CUs, 3 groups", 256, 3, 16);
    check_place("304 CUs, 3 groups", 304, 3, 16);
    check_place("64 CUs, 3 groups", 64, 3, 16);
    check_place("7 CUs, 2 groups", 7, 2, 7);
    check_place("2 CUs, 3 groups", 2, 3, 3);
    check_place("1 CU, 1 group", 1, 1, 0);
    // how many groups pay: 48 tiles of 512 entries per segment, over g * nb + cus segments.  With nb = 2442 column blocks,
    // 256 CUs and groups of 15936 rows, 2 groups need 48 * 512 * 5140 = 126.3 M entries and 3 need 48 * 512 * 7582 = 186.3 M
    {
        struct Case {
            const char *name;
            size_t n_long;
            int64_t len_long;
            size_t n_short;
            int64_t len_short;
            int g_max, want;
        };
        const Case cases[] = {{"rows fit one group", 15936, 9000, 0, 0, 3, 1},
                              {"2 groups, long segments", 31872, 4000, 0, 0, 2, 2},             // 127.5 M entries
                              {"2 groups, short segments", 31872, 3900, 0, 0, 2, 1},            // 124.3 M
                              {"3 groups pay", 47808, 4000, 0, 0, 3, 3},                        // 191.2 M
                              {"3 groups asked, 2 pay", 31872, 4000, 15936, 1000, 3, 2},        // 143.4 M for 3, 127.5 M for 2
                              {"3 rows' worth in 2 groups", 31872, 4000, 15936, 1000, 2, 2},
                              {"one group asked", 47808, 9000, 0, 0, 1, 1},
                              {"rows below the floor", 15936, 9000, 15936, 100, 2, 1}};         // the tier fits one group
        for (const Case &c : cases) {
            std::vector<int64_t> lens(c.n_long, c.len_long);
            lens.insert(lens.end(), c.n_short, c.len_short);
            std::shuffle(lens.begin(), lens.end(), rng);
            const int g = accgroups::choose_groups(lens.data(), (int32_t)lens.size(), c.g_max, 15936, 128, 2442, 256);
            if (g != c.want) {
                printf("FAIL choose_groups, %s: %d groups, want %d\n", c.name, g, c.want);
                failures++;
            } else {
                printf("ok   %-34s %d group(s)\n", c.name, g);
            }
        }
    }
    // groups with fewer tiles than workgroups: any sizes
    {
        const int32_t n_wg[3] = {128, 5, 1};
        const std::vector<uint32_t> map = accgroups::place_wgs(n_wg, 3);
        std::set<uint32_t> ids(map.begin(), map.end());
        if (map.size() != 134 || ids.size() != 134 || ids.count(~0u)) {
            printf("FAIL uneven groups: %zu blocks, %zu distinct\n", map.size(), ids.size());
            failures++;
        } else {
            printf("ok   %-34s %zu blocks\n", "uneven groups 128 + 5 + 1", map.size());
        }
    }
    if (failures) {
        printf("%d case(s) failed\n", failures);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
