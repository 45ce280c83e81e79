// Host check of csr_amd/csrc/spgemm_plan.h, built by tests/test_spgemm_plan_host.py with the system compiler and
// -fsanitize=address,undefined: every decision of the general sparse product's driver at its edge.  The budgets are far
// beyond what a small input reaches on the device (a 2 GiB table, 200 Mi products, a 6 and a 24 GiB temporary), so this is
// where those fallbacks are checked.  Every expected value is worked out by hand from the rule's statement; the constants
// are pinned first, so that a changed constant shows here and not as a shifted edge.
#include "spgemm_plan.h"

#include <cstdio>

using namespace csrk;

static int failures = 0;
static int case_failures = 0;

#define EXPECT_EQ(expr, want)                                                                                          \
    do {                                                                                                               \
        const long long got_ = (long long)(expr), want_ = (long long)(want);                                          \
        if (got_ != want_) {                                                                                           \
            printf("FAIL %s:%d: %s = %lld, want %lld\n", __FILE__, __LINE__, #expr, got_, want_);                      \
            case_failures++;                                                                                           \
        }                                                                                                              \
    } while (0)

static void done(const char *name)
{
    printf("%s %s\n", case_failures ? "FAIL" : "ok  ", name);
    failures += case_failures;
    case_failures = 0;
}

int main()
{
    EXPECT_EQ(SGS_W, 832);
    EXPECT_EQ(SGS_MAX_S, 256);
    EXPECT_EQ(SGS_TABLE_BUDGET, 2147483648ll);            // 2 GiB
    EXPECT_EQ(SGS_TEMP_BUDGET, 25769803776ll);            // 24 GiB
    EXPECT_EQ(SGE_MIN, 32);
    EXPECT_EQ(SGE_BUDGET_PRODUCTS, 209715200ll);          // 200 Mi
    EXPECT_EQ(SG_WAVE_CAP, 128);
    EXPECT_EQ(SG_LONG_LISTS, 64);
    EXPECT_EQ(SG_LONG_STRIDE, 32);
    EXPECT_EQ(SG_COUNT_VLONG, 4096);
    done("constants");

    // strips = ceil(ncols / 832); off for the general form, by the knob, above 256 strips, above 2^30 (row, strip) units
    EXPECT_EQ(sgplan::strips_in_force(1, 10, true, true), 1);
    EXPECT_EQ(sgplan::strips_in_force(832, 10, true, true), 1);
    EXPECT_EQ(sgplan::strips_in_force(833, 10, true, true), 2);
    EXPECT_EQ(sgplan::strips_in_force(833, 10, false, true), 0);
    EXPECT_EQ(sgplan::strips_in_force(833, 10, true, false), 0);
    EXPECT_EQ(sgplan::strips_in_force(212992, 10, true, true), 256);         // 256 * 832 columns: SGS_MAX_S strips
    EXPECT_EQ(sgplan::strips_in_force(212993, 10, true, true), 0);           // one more column: SGS_MAX_S + 1
    EXPECT_EQ(sgplan::strips_in_force(832, 1073741823, true, true), 1);      // 2^30 - 1 units
    EXPECT_EQ(sgplan::strips_in_force(832, 1073741824, true, true), 1);      // 2^30
    EXPECT_EQ(sgplan::strips_in_force(832, 1073741825, true, true), 0);      // 2^30 + 1
    EXPECT_EQ(sgplan::strips_in_force(1664, 536870912, true, true), 2);      // 2 * 2^29 = 2^30
    EXPECT_EQ(sgplan::strips_in_force(1664, 536870913, true, true), 0);      // 2^30 + 2
    EXPECT_EQ(sgplan::strips_in_force(212992, 2147483647, true, true), 0);   // 256 * (2^31 - 1): not an int32 product
    done("strips in force");

    // the density test keeps its strips whether they are in force or not; only the width turns it off
    EXPECT_EQ(sgplan::s_dense(1), 1);
    EXPECT_EQ(sgplan::s_dense(832), 1);
    EXPECT_EQ(sgplan::s_dense(833), 2);
    EXPECT_EQ(sgplan::s_dense(212992), 256);
    EXPECT_EQ(sgplan::s_dense(212993), 0);
    EXPECT_EQ(sgplan::s_dense(2147483647), 0);
    done("s_dense");

    // the table is 4 (strips + 1) bytes per entry of A and pays up to 2 GiB = 2147483648 bytes, inclusive.  Its size moves
    // in steps of 4 (strips + 1) bytes: the edges are the last size at or below the budget and the first above it.
    EXPECT_EQ(sgplan::table_pays(0, 1), 1);
    EXPECT_EQ(sgplan::table_pays(268435455, 1), 1);       // 8 bytes an entry: 2^31 - 8
    EXPECT_EQ(sgplan::table_pays(268435456, 1), 1);       // 2^28 * 8 = 2^31: the budget itself
    EXPECT_EQ(sgplan::table_pays(268435457, 1), 0);       // 2^31 + 8
    EXPECT_EQ(sgplan::table_pays(2097152, 255), 1);       // 1024 bytes an entry: 2^21 * 2^10 = 2^31
    EXPECT_EQ(sgplan::table_pays(2097153, 255), 0);
    EXPECT_EQ(sgplan::table_pays(2088991, 256), 1);       // 1028 bytes an entry: 2147482748, 900 below the budget
    EXPECT_EQ(sgplan::table_pays(2088992, 256), 0);       // 2147483776, 128 above it
    EXPECT_EQ(sgplan::table_pays(2147483647, 256), 0);    // 2.2e12 bytes: not an int32 product
    done("the sub-range table pays");

    EXPECT_EQ(sgplan::esc_min(true), 32);
    EXPECT_EQ(sgplan::esc_min(false), -1);
    EXPECT_EQ(sgplan::esc_fits_sort(0), 1);
    EXPECT_EQ(sgplan::esc_fits_sort(209715199), 1);
    EXPECT_EQ(sgplan::esc_fits_sort(209715200), 1);       // the budget itself
    EXPECT_EQ(sgplan::esc_fits_sort(209715201), 0);
    done("the ESC products fit the sort's budget");

    // 52 bytes a product and 64 MiB = 67108864 bytes beside them must be free
    EXPECT_EQ(sgplan::esc_fits_memory(0, 67108864), 1);
    EXPECT_EQ(sgplan::esc_fits_memory(0, 67108863), 0);
    EXPECT_EQ(sgplan::esc_fits_memory(1, 67108916), 1);                  // + 52
    EXPECT_EQ(sgplan::esc_fits_memory(1, 67108915), 0);
    EXPECT_EQ(sgplan::esc_fits_memory(1000000, 119108864), 1);           // 52000000 + 67108864, exactly
    EXPECT_EQ(sgplan::esc_fits_memory(1000000, 119108863), 0);           // one byte short
    EXPECT_EQ(sgplan::esc_fits_memory(209715200, 10972299264ull), 1);    // the sort's budget: 10905190400 + 67108864
    EXPECT_EQ(sgplan::esc_fits_memory(209715200, 10972299263ull), 0);
    EXPECT_EQ(sgplan::esc_fits_memory(209715200, 0), 0);
    done("the ESC products fit free memory");

    // the workgroup hash kernel has rows when rows of 129 .. 1024 products do not go to ESC, the 32-lane kernel when rows
    // of 33 .. 128 do not
    EXPECT_EQ(sgplan::hash_rows(-1), 1);
    EXPECT_EQ(sgplan::hash_rows(32), 0);
    EXPECT_EQ(sgplan::hash_rows(127), 0);
    EXPECT_EQ(sgplan::hash_rows(128), 0);
    EXPECT_EQ(sgplan::hash_rows(129), 1);
    EXPECT_EQ(sgplan::mid_rows(-1), 1);
    EXPECT_EQ(sgplan::mid_rows(0), 0);
    EXPECT_EQ(sgplan::mid_rows(31), 0);
    EXPECT_EQ(sgplan::mid_rows(32), 0);
    EXPECT_EQ(sgplan::mid_rows(33), 1);
    done("hash_rows and mid_rows");

    // 12 bytes an entry within a quarter of the temporary budget: 6 GiB = 6442450944 = 12 * 536870912; none when no entry
    EXPECT_EQ(sgplan::small_fused(0), 0);
    EXPECT_EQ(sgplan::small_fused(1), 1);
    EXPECT_EQ(sgplan::small_fused(536870911), 1);
    EXPECT_EQ(sgplan::small_fused(536870912), 1);         // the budget itself
    EXPECT_EQ(sgplan::small_fused(536870913), 0);         // 12 bytes above
    done("small_fused");

    // 12 bytes an entry within the whole budget: 24 GiB = 25769803776 = 12 * 2147483648; an empty temporary fits
    EXPECT_EQ(sgplan::strip_fused(0), 1);
    EXPECT_EQ(sgplan::strip_fused(2147483647), 1);
    EXPECT_EQ(sgplan::strip_fused(2147483648ll), 1);      // the budget itself
    EXPECT_EQ(sgplan::strip_fused(2147483649ll), 0);
    done("strip_fused");

    // a workgroup a row up to 256; each has 12 ncols + 4 scratch_len bytes, 4 GiB = 4294967296 for all, one at least
    EXPECT_EQ(sgplan::grid_dense(0, 1000, 1024), 0);
    EXPECT_EQ(sgplan::grid_dense(5, 1000, 1024), 5);
    EXPECT_EQ(sgplan::grid_dense(255, 1000, 1024), 255);
    EXPECT_EQ(sgplan::grid_dense(256, 1000, 1024), 256);
    EXPECT_EQ(sgplan::grid_dense(257, 1000, 1024), 256);
    EXPECT_EQ(sgplan::grid_dense(300, 1048576, 1048576), 256);           // 16 MiB each: 256 fit exactly
    EXPECT_EQ(sgplan::grid_dense(300, 1048577, 2097152), 204);           // 20971532 bytes each: 204.8
    EXPECT_EQ(sgplan::grid_dense(100, 134217728, 134217728), 2);         // 2^31 bytes each: two
    EXPECT_EQ(sgplan::grid_dense(100, 134217729, 268435456), 1);         // 2684354572 each: 1.6
    EXPECT_EQ(sgplan::grid_dense(100, 268435456, 268435456), 1);         // 2^32 each: exactly one
    EXPECT_EQ(sgplan::grid_dense(100, 268435457, 536870912), 1);         // 5368709132 each: none fits, one all the same
    EXPECT_EQ(sgplan::grid_dense(100, 2147483647, 2147483648ll), 1);
    EXPECT_EQ(sgplan::grid_dense(1, 268435456, 268435456), 1);
    done("grid_dense");

    // the power of two at or above ncols, 1 at least
    EXPECT_EQ(sgplan::scratch_len(0), 1);
    EXPECT_EQ(sgplan::scratch_len(1), 1);
    EXPECT_EQ(sgplan::scratch_len(2), 2);
    EXPECT_EQ(sgplan::scratch_len(3), 4);
    EXPECT_EQ(sgplan::scratch_len(1023), 1024);
    EXPECT_EQ(sgplan::scratch_len(1024), 1024);
    EXPECT_EQ(sgplan::scratch_len(1025), 2048);
    EXPECT_EQ(sgplan::scratch_len(1073741823), 1073741824);
    EXPECT_EQ(sgplan::scratch_len(1073741824), 1073741824);
    EXPECT_EQ(sgplan::scratch_len(1073741825), 2147483648ll);            // beyond int32
    EXPECT_EQ(sgplan::scratch_len(2147483647), 2147483648ll);
    done("scratch_len");

    // 32 rows a workgroup; workgroup w appends to list w % 64, so a list holds the rows of ceil(workgroups / 64) of them
    EXPECT_EQ(sgplan::count_blocks(1), 1);
    EXPECT_EQ(sgplan::count_blocks(32), 1);
    EXPECT_EQ(sgplan::count_blocks(33), 2);
    EXPECT_EQ(sgplan::count_blocks(2147483647), 67108864);
    EXPECT_EQ(sgplan::long_cap(1), 32);
    EXPECT_EQ(sgplan::long_cap(2048), 32);                // 64 workgroups: one each
    EXPECT_EQ(sgplan::long_cap(2049), 64);                // 65
    EXPECT_EQ(sgplan::long_cap(4096), 64);
    EXPECT_EQ(sgplan::long_cap(4097), 96);
    EXPECT_EQ(sgplan::long_cap(2147483647), 33554432);    // 2^26 workgroups / 64 * 32
    // slots: nrows + 1 for the strip list, or 64 lists of long_cap and a very long row per 4096 entries of A, and one
    EXPECT_EQ(sgplan::list_s_slots(1, 1), 2049);
    EXPECT_EQ(sgplan::list_s_slots(2048, 4095), 2049);    // both sides 2049
    EXPECT_EQ(sgplan::list_s_slots(2048, 4096), 2050);
    EXPECT_EQ(sgplan::list_s_slots(2049, 4095), 4097);
    EXPECT_EQ(sgplan::list_s_slots(100, 40960000), 12049);               // 2048 + 10000 + 1
    EXPECT_EQ(sgplan::list_s_slots(2147483647, 1099511627776ll), 2415919105ll);      // 2^31 + 2^28 + 1: beyond int32
    done("long_cap and the size of list_s");

    if (failures) {
        printf("%d check(s) failed\n", failures);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
