// csr_amd/csrc/score_host.h on the host: check_listed_rows and pack_listed_rows -- pointer arithmetic with a caller's stride,
// rows[r] * ldu * es -- with tests/panel_host/main.cpp's stand-ins: hipMemcpy2D is memcpy and the pool is malloc of the exact
// size, and every source and destination here has exactly its size, so that AddressSanitizer sees a stride or an offset that
// is off by one element.  Also the optional handle, the seen / test agreement, the refusal texts that take the entry's name,
// and the panel-type ladder.  Built by tests/test_score_host_host.py for the host only, without the HIP runtime: it cannot
// touch a GPU.
#include "common.h"
static hipError_t copy2d(void *d, size_t dp, const void *s, size_t sp, size_t w, size_t h, hipMemcpyKind)
{
    for (size_t r = 0; r < h; r++) memcpy((char *)d + r * dp, (const char *)s + r * sp, w);
    return hipSuccess;
}
#define hipMemcpy2D copy2d
#include "score_host.h"
#include <cstdlib>
#include <string>
#include <vector>

static std::string last_error;
static int canonical_looks = 0;
namespace csrk {
void set_error(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    last_error = buf;
}
hipError_t pool_alloc(void **p, size_t n) { return (*p = malloc(n)) ? hipSuccess : hipErrorOutOfMemory; }
void pool_free(void *p) { free(p); }
Matrix::~Matrix() {}
Matrix *from_handle(csrk_handle_t h)      // 1 is the only live handle
{
    static Matrix live;
    if (h == (csrk_handle_t)1) return &live;
    set_error("invalid csrk handle");
    return nullptr;
}
int look_at_rows(Matrix *) { return canonical_looks++, CSRK_OK; }
}  // namespace csrk
extern "C" const char *hipGetErrorString(hipError_t) { return "no HIP runtime is linked"; }
using namespace csrk;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s  (last error: %s)\n", __LINE__, #c, last_error.c_str()); return 1; } } while (0)

static int listed_rows()
{
    const int32_t u_rows = 5;
    for (int32_t bad : {-1, u_rows, INT32_MIN, INT32_MAX}) {
        const std::vector<int32_t> rows = {4, 0, bad, -7};       // the first bad position is the one named
        CHECK(check_listed_rows("topk_scores_for", rows.data(), 4, u_rows) == CSRK_ERR_INVALID);
        CHECK(last_error == "topk_scores_for: rows[2]=" + std::to_string(bad) + " is outside [0, 5)");
    }
    for (int32_t good : {0, u_rows - 1}) {
        const std::vector<int32_t> rows = {good};
        CHECK(check_listed_rows("rank_entries_for", rows.data(), 1, u_rows) == CSRK_OK);
    }
    CHECK(check_listed_rows("rank_entries_for", nullptr, 0, u_rows) == CSRK_OK);      // an empty list is not looked at
    const std::vector<int32_t> one = {0};
    CHECK(check_listed_rows("rank_entries_for", one.data(), 1, 0) == CSRK_ERR_INVALID);
    CHECK(last_error == "rank_entries_for: rows[0]=0 is outside [0, 0)");

    const std::vector<std::vector<int32_t>> lists = {{}, {2}, {u_rows - 1, 0, u_rows - 1}};
    for (size_t es : {4, 8}) for (int k : {1, 3, 4}) for (int pad : {0, 3}) for (const std::vector<int32_t> &rows : lists) {
        const int64_t ldu = k + pad;
        // U ends with its last row's k elements: no padding behind it, so a read of ldu elements there is out of bounds
        std::vector<unsigned char> U((((size_t)u_rows - 1) * ldu + k) * es);
        for (size_t i = 0; i < U.size(); i++) U[i] = (unsigned char)(i * 7 + 1);
        DevBuf d;
        CHECK(pack_listed_rows(d, U.data(), ldu, k, es, rows.data(), rows.size()) == CSRK_OK && d.p);
        CHECK(d.bytes == rows.size() * k * es);                  // (the stand-in pool allocated exactly this, or 16 for none)
        for (size_t r = 0; r < rows.size(); r++)
            CHECK(!memcmp((char *)d.p + r * k * es, U.data() + (size_t)rows[r] * ldu * es, (size_t)k * es));
    }
    return 0;
}

static int handles_and_agreement()
{
    Matrix *m = (Matrix *)16;
    CHECK(optional_handle(0, &m) == CSRK_OK && m == nullptr);
    CHECK(optional_handle((csrk_handle_t)1, &m) == CSRK_OK && m == from_handle((csrk_handle_t)1));
    CHECK(optional_handle((csrk_handle_t)2, &m) == CSRK_ERR_INVALID && m == nullptr && last_error == "invalid csrk handle");
    const ScoreCsr none = score_csr(nullptr);
    CHECK(none.rp == nullptr && none.ptr64 == 0 && none.ci == nullptr);

    Matrix seen, test;
    seen.nrows = test.nrows = 3, seen.ncols = test.ncols = 4;
    seen.device = test.device = 0;
    CHECK(check_seen_matches_test("rank_entries", &seen, &test) == CSRK_OK);
    seen.ncols = 5;
    CHECK(check_seen_matches_test("rank_entries", &seen, &test) == CSRK_ERR_INVALID);
    CHECK(last_error == "rank_entries: seen is 3 x 5 but test is 3 x 4");
    seen.ncols = 4, seen.nrows = 2;
    CHECK(check_seen_matches_test("rank_entries_for", &seen, &test) == CSRK_ERR_INVALID);
    CHECK(last_error == "rank_entries_for: seen is 2 x 4 but test is 3 x 4");
    seen.nrows = 3, seen.device = 1;
    CHECK(check_seen_matches_test("rank_entries_for", &seen, &test) == CSRK_ERR_INVALID);
    CHECK(last_error == "rank_entries_for: seen and test are on different devices");

    seen.canonical = 1;
    CHECK(check_seen_canonical("topk_scores", &seen) == CSRK_OK && canonical_looks == 1);
    seen.canonical = 0, seen.noncanonical_row = 7;
    CHECK(check_seen_canonical("topk_scores", &seen) == CSRK_ERR_INVALID && canonical_looks == 2);
    CHECK(last_error == "topk_scores: seen is not canonical: row 7 is not strictly ascending in column (csrk_order_columns sorts, "
                        "csrk_coalesce merges repeats)");
    CHECK(seen.mu.try_lock());                                   // the lock was given back
    seen.mu.unlock();

    CHECK(check_supported(true, "csrk_topk_scores", "k", 1024, 1024, "csrk_topk_scores_limits") == CSRK_OK);
    CHECK(check_supported(false, "csrk_topk_scores", "k", 1025, 1024, "csrk_topk_scores_limits") == CSRK_ERR_UNSUPPORTED);
    CHECK(last_error == "csrk_topk_scores: k=1025 is above the largest supported k=1024 (csrk_topk_scores_limits)");
    return 0;
}

static int ladder()
{
    alignas(16) double a[8];
    CHECK(panels_wide(a, 4, a, 2, 4, 8) && !panels_wide(a + 1, 4, a, 2, 4, 8) && !panels_wide(a, 4, a, 3, 4, 8) && !panels_wide(a, 4, a, 4, 3, 8));
    CHECK(panels_wide(a, 4, a, 8, 4, 4) && !panels_wide(a, 4, a, 8, 6, 4) && !panels_wide(a, 6, a, 8, 4, 4));
    for (int type : {CSRK_VAL_F64, CSRK_VAL_F32}) for (bool wide : {false, true}) {
        int calls = 0;
        size_t size = 0;
        bool w = !wide;
        score_for_panel(type, wide, [&](auto t, auto wd) {
            calls++;
            size = sizeof(typename decltype(t)::type);
            w = decltype(wd)::value;
        });
        CHECK(calls == 1 && size == panel_es(type) && w == wide);
    }
    return 0;
}

int main()
{
    if (listed_rows() || handles_and_agreement() || ladder()) return 1;
    printf("all cases passed\n");
    return 0;
}
