// csr_amd/csrc/panel.h on the host: pack_panel / unpack_panel / panel_rows_from / panel_16b with the two HIP copies replaced
// by memcpy and the pool by malloc of the exact size, so that AddressSanitizer sees an offset or a pitch that is off by one
// element.  Built by tests/test_panel_host.py for the host only, without the HIP runtime: it cannot touch a GPU.
#include "common.h"
static hipError_t copy2d(void *d, size_t dp, const void *s, size_t sp, size_t w, size_t h, hipMemcpyKind)
{
    for (size_t r = 0; r < h; r++) memcpy((char *)d + r * dp, (const char *)s + r * sp, w);
    return hipSuccess;
}
#define hipMemcpy2D copy2d
#include "panel.h"
#include <cstdlib>
#include <vector>

namespace csrk {
void set_error(const char *, ...) {}
hipError_t pool_alloc(void **p, size_t n) { return (*p = malloc(n)) ? hipSuccess : hipErrorOutOfMemory; }
void pool_free(void *p) { free(p); }
Matrix::~Matrix() {}
}  // namespace csrk
extern "C" const char *hipGetErrorString(hipError_t) { return "no HIP runtime is linked"; }
using namespace csrk;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main()
{
    for (size_t es : {4, 8}) for (int k : {1, 3, 4}) for (int pad : {0, 3}) for (int rows : {0, 1, 5}) for (int rb : {0, 2}) {
        const int64_t ld = k + pad, all = rows + rb;
        std::vector<unsigned char> in((size_t)all * ld * es), out((size_t)rows * ld * es, 0xee);      // exact sizes
        for (size_t i = 0; i < in.size(); i++) in[i] = (unsigned char)(i * 7 + 1);
        const void *from = panel_rows_from(in.data(), rb, ld, es);
        CHECK(from == in.data() + (size_t)rb * ld * es && panel_rows_from(nullptr, rb, ld, es) == nullptr);
        DevBuf d, none;
        CHECK(pack_panel(d, rows ? from : in.data(), ld, k, es, rows) == CSRK_OK && d.p);
        CHECK(pack_panel(none, nullptr, ld, k, es, rows) == CSRK_OK && none.p);          // NULL source: allocated, nothing copied
        for (int r = 0; r < rows; r++)
            CHECK(!memcmp((char *)d.p + (size_t)r * k * es, in.data() + ((size_t)(rb + r) * ld) * es, (size_t)k * es));
        CHECK(unpack_panel(rows ? out.data() : nullptr, ld, d, k, es, rows) == CSRK_OK);
        CHECK(unpack_panel(nullptr, ld, d, k, es, rows) == CSRK_OK);                      // NULL destination: nothing copied
        for (size_t i = 0; i < out.size(); i++) {
            const size_t r = i / (ld * es), c = i % (ld * es);
            CHECK(out[i] == (c < (size_t)k * es ? in[((size_t)(rb + r) * ld) * es + c] : 0xee));      // the padding is untouched
        }
    }
    alignas(16) double a[8];
    CHECK(panel_es(CSRK_VAL_F64) == 8 && panel_es(CSRK_VAL_F32) == 4 && panel_per16(8) == 2 && panel_per16(4) == 4);
    CHECK(panel_16b(a, 4, 8) && !panel_16b(a + 1, 4, 8) && !panel_16b(a, 3, 8) && panel_16b(a, 4, 4) && !panel_16b(a, 6, 4));
    Matrix m;
    mark_user_stream(nullptr, (hipStream_t)a);
    mark_user_stream(&m, nullptr);
    CHECK(!m.used_user_stream);
    mark_user_stream(&m, (hipStream_t)a);
    CHECK(m.used_user_stream);
    printf("all cases passed\n");
    return 0;
}
