// Host check of csr_amd/csrc/radix_plan.h, built by tests/test_radix_plan_host.py with the system compiler and
// -fsanitize=address,undefined.  Two modes.
//   (no argument)             every function of the header at its edges, the expected values worked out by hand from the
//                             rule's statement; the constants are pinned first, so that a changed constant shows here and
//                             not as a shifted edge.
//   case OP NROWS NCOLS N     the sorts one operation of tests/radix_cases.py makes -- transpose: keys = columns, payload =
//                             source row; from_coo: keys = rows, payload = columns; order: a transpose and the transpose of
//                             its result -- one line "sort ROUTE CHUNKS CAPACITY" each, and the constants that module restates.
#include "radix_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

using namespace csrk;
using namespace csrk::radixplan;

static int failures = 0;
static int case_failures = 0;

static void expect_eq(const char *what, int line, long long got, long long want)
{
    if (got == want) return;
    printf("FAIL %s:%d: %s = %lld, want %lld\n", __FILE__, line, what, got, want);
    case_failures++;
}
#define EXPECT_EQ(expr, want) expect_eq(#expr, __LINE__, (long long)(expr), (long long)(want))

static void done(const char *name)
{
    printf("%s %s\n", case_failures ? "FAIL" : "ok  ", name);
    failures += case_failures;
    case_failures = 0;
}

static const char *route_name(Route r)
{
    switch (r) {
    case Route::Empty: return "empty";
    case Route::One: return "1";
    case Route::Packed: return "packed";
    case Route::Plain2: return "plain2";
    case Route::Three: return "3";
    case Route::Four: return "4";
    }
    return "?";
}

constexpr int64_t P24 = 1ll << 24;

static void route_cases()
{
    EXPECT_EQ(RX_THREADS, 512), EXPECT_EQ(RX_ROUNDS, 8), EXPECT_EQ(RX_CHUNK, 4096), EXPECT_EQ(RX_HC, 4);
    EXPECT_EQ(RXS_THREADS, 1024), EXPECT_EQ(RXS_IPT, 8), EXPECT_EQ(RX_PACKED_SHIFT, 24), EXPECT_EQ(PACKED_PAYLOADS, 16777216);
    EXPECT_EQ(SCAN_GRID, 256), EXPECT_EQ(ALIGN_GRID, 1);
    done("constants");

    // key range -> bits = ceil(log2), passes of 8 bits, the route of 5 records with payloads below 1000
    const struct {
        long long range;
        int bits, passes;
        Route route;
    } ladder[] = {{1, 0, 1, Route::One},          {2, 1, 1, Route::One},          {255, 8, 1, Route::One},
                  {256, 8, 1, Route::One},        {257, 9, 2, Route::Packed},     {65535, 16, 2, Route::Packed},
                  {65536, 16, 2, Route::Packed},  {65537, 17, 3, Route::Three},   {P24, 24, 3, Route::Three},
                  {P24 + 1, 25, 4, Route::Four},  {1ll << 30, 30, 4, Route::Four}, {(1ll << 31) - 1, 31, 4, Route::Four}};
    for (const auto &l : ladder) {
        const int32_t range = (int32_t)l.range;
        EXPECT_EQ(key_bits(range), l.bits);
        EXPECT_EQ(passes(key_bits(range)), l.passes);
        EXPECT_EQ(route(5, range, 1000), l.route);
        const Plan pl = radix_plan(5, range, 1000, false, false);
        EXPECT_EQ(pl.route, l.route), EXPECT_EQ(pl.bits, l.bits), EXPECT_EQ(pl.passes, l.passes), EXPECT_EQ(pl.packed, l.route == Route::Packed);
        EXPECT_EQ(pl.ptr_slots, 0);      // (the empty sort's only)
    }
    EXPECT_EQ(passes(0), 1), EXPECT_EQ(passes(8), 1), EXPECT_EQ(passes(9), 2), EXPECT_EQ(passes(16), 2), EXPECT_EQ(passes(17), 3);
    EXPECT_EQ(passes(24), 3), EXPECT_EQ(passes(25), 4), EXPECT_EQ(passes(31), 4);
    done("the key-range ladder");

    // the payload range decides between the two two-pass routes, and nothing else
    EXPECT_EQ(route(5, 65536, P24), Route::Packed), EXPECT_EQ(route(5, 65536, P24 + 1), Route::Plain2);
    EXPECT_EQ(route(5, 257, P24), Route::Packed), EXPECT_EQ(route(5, 257, P24 + 1), Route::Plain2);
    EXPECT_EQ(route(5, 65536, 1), Route::Packed), EXPECT_EQ(route(5, 65536, 1ll << 40), Route::Plain2);
    EXPECT_EQ(route(5, 256, P24), Route::One), EXPECT_EQ(route(5, 256, P24 + 1), Route::One);
    EXPECT_EQ(route(5, 65537, P24), Route::Three), EXPECT_EQ(route(5, 65537, P24 + 1), Route::Three);
    EXPECT_EQ(radix_plan(5, 65536, P24, true, true).packed, 1), EXPECT_EQ(radix_plan(5, 65536, P24 + 1, true, true).packed, 0);
    EXPECT_EQ(radix_plan(5, 65536, P24 + 1, true, true).passes, 2);
    done("the payload range at 2^24");

    // no record: nothing but the run starts to clear, whatever the ranges
    const long long ranges[] = {0, 1, 256, 257, 65536, 65537, P24 + 1, (1ll << 31) - 2};
    for (long long kr : ranges)
        for (long long pr : {0ll, 1ll, (long long)P24, (long long)P24 + 1}) {
            EXPECT_EQ(route(0, (int32_t)kr, pr), Route::Empty);
            const Plan pl = radix_plan(0, (int32_t)kr, pr, true, true);
            EXPECT_EQ(pl.route, Route::Empty), EXPECT_EQ(pl.ptr_slots, kr + 1), EXPECT_EQ(pl.passes, 0), EXPECT_EQ(pl.chunks, 0);
            EXPECT_EQ(pl.bits, 0), EXPECT_EQ(pl.chunks2, 0), EXPECT_EQ(pl.packed, 0);
            EXPECT_EQ(pl.table.used || pl.total.used || pl.rlo.used || pl.rhi.used || pl.keyL.used || pl.rowA.used || pl.cstart.used, 0);
        }
    EXPECT_EQ(route(1, 0, 0), Route::One);      // (one record is a sort)
    done("n = 0");
}

// every count-dependent number of one sort of n records: the packed route from a CSR with values (key range 1000), and
// the table of the plain routes
struct Counts {
    long long n, chunks, capacity, table_packed, table_plain, bound, cstart, ccnt, word, value;
    unsigned bounds, hist, scatter, hist2, scatter2, ptr_keys;
    long long scan_trips;
};

static void count_cases()
{
    // chunks = ceil(n / 4096); capacity = chunks + 256; table = (256 chunks' + 1) 8 bytes; bounds 4 bytes a chunk; descriptors
    // 8 and 4 bytes; grids: bounds ceil(chunks / 256), hist ceil(chunks / 4), scatter 8 ceil(chunks / 8), the same two over the
    // capacity, pointers from keys ceil(ceil((n + 1) / 4) / 256); scan trips ceil(chunks / 8192)
    const Counts t[] = {
        {1, 1, 257, 526344, 2056, 4, 2056, 1028, 4, 8, 1, 1, 8, 65, 264, 1, 1},
        {4095, 1, 257, 526344, 2056, 4, 2056, 1028, 16380, 32760, 1, 1, 8, 65, 264, 4, 1},
        {4096, 1, 257, 526344, 2056, 4, 2056, 1028, 16384, 32768, 1, 1, 8, 65, 264, 5, 1},
        {4097, 2, 258, 528392, 4104, 8, 2064, 1032, 16388, 32776, 1, 1, 8, 65, 264, 5, 1},
        {4 * 4096 - 1, 4, 260, 532488, 8200, 16, 2080, 1040, 65532, 131064, 1, 1, 8, 65, 264, 16, 1},
        {4 * 4096 + 1, 5, 261, 534536, 10248, 20, 2088, 1044, 65540, 131080, 1, 2, 8, 66, 264, 17, 1},
        {8 * 4096, 8, 264, 540680, 16392, 32, 2112, 1056, 131072, 262144, 1, 2, 8, 66, 264, 33, 1},
        {8 * 4096 + 1, 9, 265, 542728, 18440, 36, 2120, 1060, 131076, 262152, 1, 3, 16, 67, 272, 33, 1},
        {8192ll * 4096, 8192, 8448, 17301512, 16777224, 32768, 67584, 33792, 134217728, 268435456, 32, 2048, 8192, 2112, 8448, 32769, 1},
        {8192ll * 4096 + 1, 8193, 8449, 17303560, 16779272, 32772, 67592, 33796, 134217732, 268435464, 33, 2049, 8200, 2113, 8456, 32769, 2}};
    for (const Counts &c : t) {
        EXPECT_EQ(chunks(c.n), c.chunks), EXPECT_EQ(aligned_capacity(chunks(c.n)), c.capacity);
        EXPECT_EQ(cdiv(chunks(c.n), (int64_t)RXS_THREADS * RXS_IPT), c.scan_trips);
        const Plan pk = radix_plan(c.n, 1000, 700, true, true);
        EXPECT_EQ(pk.route, Route::Packed), EXPECT_EQ(pk.chunks, c.chunks), EXPECT_EQ(pk.chunks2, c.capacity);
        EXPECT_EQ(pk.table.bytes, c.table_packed), EXPECT_EQ(pk.total.bytes, 2048), EXPECT_EQ(pk.rlo.bytes, c.bound), EXPECT_EQ(pk.rhi.bytes, c.bound);
        EXPECT_EQ(pk.cstart.bytes, c.cstart), EXPECT_EQ(pk.ccnt.bytes, c.ccnt), EXPECT_EQ(pk.run0.bytes, 2056), EXPECT_EQ(pk.total2.bytes, 2048);
        EXPECT_EQ(pk.rowA.bytes, c.word), EXPECT_EQ(pk.valA.bytes, c.value);
        EXPECT_EQ(pk.grid.bounds, c.bounds), EXPECT_EQ(pk.grid.hist, c.hist), EXPECT_EQ(pk.grid.scatter, c.scatter);
        EXPECT_EQ(pk.grid.hist2, c.hist2), EXPECT_EQ(pk.grid.scatter2, c.scatter2), EXPECT_EQ(pk.grid.ptr_table, 4);      // 1001 pointers
        EXPECT_EQ(pk.grid.ptr_keys, c.ptr_keys);
        const Plan p4 = radix_plan(c.n, (int32_t)P24 + 1, 700, true, true);      // four passes: every plain buffer
        EXPECT_EQ(p4.route, Route::Four), EXPECT_EQ(p4.chunks, c.chunks), EXPECT_EQ(p4.chunks2, c.chunks), EXPECT_EQ(p4.table.bytes, c.table_plain);
        EXPECT_EQ(p4.total.bytes, 2048), EXPECT_EQ(p4.rlo.bytes, c.bound), EXPECT_EQ(p4.rhi.bytes, c.bound);
        EXPECT_EQ(p4.keyL.bytes, c.word), EXPECT_EQ(p4.keyA.bytes, c.word), EXPECT_EQ(p4.rowA.bytes, c.word), EXPECT_EQ(p4.keyB.bytes, c.word);
        EXPECT_EQ(p4.rowB.bytes, c.word), EXPECT_EQ(p4.valA.bytes, c.value), EXPECT_EQ(p4.valB.bytes, c.value);
        EXPECT_EQ(p4.grid.bounds, c.bounds), EXPECT_EQ(p4.grid.hist, c.hist), EXPECT_EQ(p4.grid.scatter, c.scatter);
        EXPECT_EQ(p4.grid.hist2, c.hist), EXPECT_EQ(p4.grid.scatter2, c.scatter), EXPECT_EQ(p4.grid.ptr_keys, c.ptr_keys);
        EXPECT_EQ(p4.grid.ptr_table, 65537);      // 2^24 + 2 pointers, 256 a workgroup
    }
    done("record counts 1 .. 8192 * 4096 + 1");

    EXPECT_EQ(table_bytes(0), 8), EXPECT_EQ(table_bytes(1), 2056), EXPECT_EQ(total_bytes(), 2048), EXPECT_EQ(run0_bytes(), 2056);
    EXPECT_EQ(bound_bytes(3), 12), EXPECT_EQ(cstart_bytes(3), 24), EXPECT_EQ(ccnt_bytes(3), 12), EXPECT_EQ(word_bytes(3), 12), EXPECT_EQ(value_bytes(3), 24);
    EXPECT_EQ(word_bytes(1ll << 33), 1ll << 35), EXPECT_EQ(value_bytes(1ll << 33), 1ll << 36);      // (beyond 2^31 entries: 64-bit sizes)
    done("the size functions");

    // a thread per pointer, key_range + 1 of them
    EXPECT_EQ(ptr_table_grid(1), 1), EXPECT_EQ(ptr_table_grid(255), 1), EXPECT_EQ(ptr_table_grid(256), 2), EXPECT_EQ(ptr_table_grid(511), 2);
    EXPECT_EQ(ptr_table_grid(512), 3), EXPECT_EQ(ptr_table_grid(65536), 257), EXPECT_EQ(ptr_table_grid(INT32_MAX), 8388608);
    // four positions a thread, positions 0 .. n: n = 1023 is 1024 positions = 256 threads, n = 1024 one thread more
    EXPECT_EQ(ptr_keys_grid(1), 1), EXPECT_EQ(ptr_keys_grid(3), 1), EXPECT_EQ(ptr_keys_grid(4), 1), EXPECT_EQ(ptr_keys_grid(1023), 1), EXPECT_EQ(ptr_keys_grid(1024), 2);
    EXPECT_EQ(bounds_grid(256), 1), EXPECT_EQ(bounds_grid(257), 2), EXPECT_EQ(hist_grid(4), 1), EXPECT_EQ(hist_grid(5), 2);
    EXPECT_EQ(scatter_grid(1), 8), EXPECT_EQ(scatter_grid(8), 8), EXPECT_EQ(scatter_grid(9), 16), EXPECT_EQ(scatter_grid(16), 16), EXPECT_EQ(scatter_grid(17), 24);
    done("the grids");
}

static void expect_pass(const Plan &pl, int p, int shift, bool first, Where src, Where dst)
{
    EXPECT_EQ(pl.pass[p].shift, shift), EXPECT_EQ(pl.pass[p].first, first), EXPECT_EQ(pl.pass[p].src, src), EXPECT_EQ(pl.pass[p].dst, dst);
}

static void schedule_cases()
{
    const Plan p1 = radix_plan(5, 256, 700, false, true), p2 = radix_plan(5, 65536, P24 + 1, false, true);
    const Plan p3 = radix_plan(5, 65537, 700, false, true), p4 = radix_plan(5, (int32_t)P24 + 1, 700, false, true);
    EXPECT_EQ(p1.passes, 1), EXPECT_EQ(p2.passes, 2), EXPECT_EQ(p3.passes, 3), EXPECT_EQ(p4.passes, 4);
    expect_pass(p1, 0, 0, true, Source, Last);
    expect_pass(p2, 0, 0, true, Source, A), expect_pass(p2, 1, 8, false, A, Last);
    expect_pass(p3, 0, 0, true, Source, A), expect_pass(p3, 1, 8, false, A, B), expect_pass(p3, 2, 16, false, B, Last);
    expect_pass(p4, 0, 0, true, Source, A), expect_pass(p4, 1, 8, false, A, B), expect_pass(p4, 2, 16, false, B, A), expect_pass(p4, 3, 24, false, A, Last);
    EXPECT_EQ(Source, 0), EXPECT_EQ(A, 1), EXPECT_EQ(B, 2), EXPECT_EQ(Last, 3);      // (the driver indexes its buffer sets by them)
    for (const Plan *pl : {&p1, &p2, &p3, &p4})
        for (int p = 0; p < pl->passes; p++) {
            const Pass &s = pl->pass[p];
            EXPECT_EQ(s.src != s.dst, 1);                                        // no pass reads the buffer it writes
            EXPECT_EQ(s.first, s.src == Source), EXPECT_EQ(s.dst == Last, p == pl->passes - 1);
            if (p > 0) EXPECT_EQ(s.src, pl->pass[p - 1].dst);                    // a pass reads what the pass before wrote
            EXPECT_EQ(s.dst == B && !pl->keyB.used, 0), EXPECT_EQ(s.dst == A && !pl->keyA.used, 0);      // written buffers exist
        }
    done("the pass schedule");
}

// table total rlo rhi cstart ccnt run0 total2 keyL keyA rowA valA keyB rowB valB, '1' = requested
static void expect_buffers(int line, int32_t key_range, int64_t payload_range, bool from_csr, bool has_values, const char *want)
{
    const Plan pl = radix_plan(9, key_range, payload_range, from_csr, has_values);
    const Buf *b[15] = {&pl.table, &pl.total, &pl.rlo,  &pl.rhi,  &pl.cstart, &pl.ccnt, &pl.run0, &pl.total2,
                        &pl.keyL,  &pl.keyA,  &pl.rowA, &pl.valA, &pl.keyB,   &pl.rowB, &pl.valB};
    char got[16] = {0};
    for (int i = 0; i < 15; i++) {
        got[i] = b[i]->used ? '1' : '0';
        if (!b[i]->used) expect_eq("bytes of a buffer that is not requested", line, (long long)b[i]->bytes, 0);
    }
    if (strcmp(got, want) != 0) {
        printf("FAIL %s:%d: buffers %s, want %s\n", __FILE__, line, got, want);
        case_failures++;
    }
}
#define EXPECT_BUFFERS(...) expect_buffers(__LINE__, __VA_ARGS__)

static void buffer_cases()
{
    const int32_t four = (int32_t)P24 + 1;
    //                                                  tt rr cc r2 L  AAA BBB
    EXPECT_BUFFERS(256, 700, true, true,               "111100001000000");      // one pass from a CSR: bounds, sorted keys
    EXPECT_BUFFERS(256, 700, false, true,              "110000001000000");
    EXPECT_BUFFERS(256, 700, false, false,             "110000001000000");
    EXPECT_BUFFERS(65536, P24, true, true,             "111111110011000");      // packed: descriptors, words, values; no key array
    EXPECT_BUFFERS(65536, P24, true, false,            "111111110010000");
    EXPECT_BUFFERS(65536, P24, false, true,            "110011110011000");
    EXPECT_BUFFERS(65536, P24, false, false,           "110011110010000");
    EXPECT_BUFFERS(65536, P24 + 1, true, true,         "111100001111000");      // plain two-pass: the A set
    EXPECT_BUFFERS(65536, P24 + 1, true, false,        "111100001110000");
    EXPECT_BUFFERS(65536, P24 + 1, false, true,        "110000001111000");
    EXPECT_BUFFERS(65536, P24 + 1, false, false,       "110000001110000");
    EXPECT_BUFFERS(65537, 700, true, true,             "111100001111111");      // three passes: the B set too
    EXPECT_BUFFERS(65537, 700, true, false,            "111100001110110");
    EXPECT_BUFFERS(65537, 700, false, true,            "110000001111111");
    EXPECT_BUFFERS(65537, 700, false, false,           "110000001110110");
    EXPECT_BUFFERS(four, 700, true, true,              "111100001111111");      // four passes: as three
    EXPECT_BUFFERS(four, 700, true, false,             "111100001110110");
    EXPECT_BUFFERS(four, 700, false, true,             "110000001111111");
    EXPECT_BUFFERS(four, 700, false, false,            "110000001110110");
    done("which buffers exist");
}

static int edge_mode()
{
    route_cases();
    count_cases();
    schedule_cases();
    buffer_cases();
    printf(failures ? "%d checks failed\n" : "all cases passed\n", failures);
    return failures ? 1 : 0;
}

static void print_sort(int64_t n, int32_t key_range, int64_t payload_range, bool from_csr)
{
    const Plan pl = radix_plan(n, key_range, payload_range, from_csr, false);
    printf("sort %s %lld %lld\n", route_name(pl.route), (long long)pl.chunks, (long long)aligned_capacity(pl.chunks));
}

static int case_mode(int argc, char **argv)
{
    if (argc != 6) return 2;
    const char *op = argv[2];
    const long long nrows = atoll(argv[3]), ncols = atoll(argv[4]), n = atoll(argv[5]);
    if (nrows < 0 || ncols < 0 || n < 0 || nrows > INT32_MAX || ncols > INT32_MAX) return 2;
    printf("constants %d %d %d\n", RX_CHUNK, RX_HC, RXS_THREADS * RXS_IPT);
    if (strcmp(op, "transpose") == 0)
        print_sort(n, (int32_t)ncols, nrows, true);
    else if (strcmp(op, "from_coo") == 0)
        print_sort(n, (int32_t)nrows, ncols, false);
    else if (strcmp(op, "order") == 0)
        print_sort(n, (int32_t)ncols, nrows, true), print_sort(n, (int32_t)nrows, ncols, true);
    else
        return 2;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && strcmp(argv[1], "case") == 0) return case_mode(argc, argv);
    return edge_mode();
}
