// Host-side steps shared by the operations that take dense row-major panels (csrk_spmm_dense, csrk_sddmm, csrk_gram_rows,
// csrk_als_rows, csrk_solve_blocks, csrk_topk_scores, csrk_rank_entries and the two list forms csrk_topk_scores_for,
// csrk_rank_entries_for; DESIGN.md section 8, "Taking dense panels"):
//   checks -> early return -> NULL checks -> pack_panel -> the _device function with packed strides -> unpack_panel
// The entry points call these in a straight line, and every entry keeps its own ORDER of refusals.  Here: the element size,
// the 16-B predicate, pack_panel / unpack_panel, panel_rows_from, mark_user_stream, check_transpose_shape and the scalar
// refusals.  What only the four factor-score drivers share -- the optional handle, the canonical check of `seen`, the listed
// rows (check_listed_rows, pack_listed_rows), the seen / test agreement and the panel-type ladder -- is score_host.h's.
#pragma once
#include "common.h"

namespace csrk {

inline size_t panel_es(int panel_type) { return panel_type == CSRK_VAL_F64 ? 8 : 4; }
inline int64_t panel_per16(size_t es) { return (int64_t)(16 / es); }      // elements per 16-B piece

// Every row of the panel starts 16-B aligned.  A launch may use 16-B loads when this holds for each panel it reads -- and,
// where a lane loads whole pieces of a row (gram, als, topk_scores, rank_entries), k % panel_per16(es) == 0 as well; SDDMM's
// lanes load four columns at a time and need no k term.  Otherwise element loads: the same bits.
inline bool panel_16b(const void *d, int64_t ld, size_t es) { return ((uintptr_t)d & 15) == 0 && ld % panel_per16(es) == 0; }

// A host panel travels packed (ld = k): the bits do not depend on the stride.  d is allocated in any case; nothing is
// copied for rows == 0 or a NULL source.
static int pack_panel(DevBuf &d, const void *host, int64_t ld, int64_t k, size_t es, int64_t rows)
{
    CSRK_TRY(d.alloc((size_t)rows * k * es));
    if (rows && host)
        CSRK_HIP(hipMemcpy2D(d.p, (size_t)k * es, host, (size_t)ld * es, (size_t)k * es, (size_t)rows, hipMemcpyHostToDevice));
    return CSRK_OK;
}

// ... and a packed result goes back into the caller's stride
static int unpack_panel(void *host, int64_t ld, const DevBuf &d, int64_t k, size_t es, int64_t rows)
{
    if (rows && host)
        CSRK_HIP(hipMemcpy2D(host, (size_t)ld * es, d.p, (size_t)k * es, (size_t)k * es, (size_t)rows, hipMemcpyDeviceToHost));
    return CSRK_OK;
}

// row row_begin of a panel (NULL stays NULL)
inline const void *panel_rows_from(const void *p, int32_t row_begin, int64_t ld, size_t es)
{
    return p ? (const char *)p + (size_t)row_begin * (size_t)ld * es : nullptr;
}

// a launch on a caller's stream marks its handle (common.h, the caching allocator's contract); m may be NULL
inline void mark_user_stream(Matrix *m, hipStream_t s)
{
    if (!m || !s) return;
    std::lock_guard<std::mutex> lk(m->mu);
    m->used_user_stream = true;
}

// `at` has the shape and the entry count of a's transpose (csrk_als_objective, csrk_als_fit; that it IS the transpose is
// the caller's business)
static int check_transpose_shape(const Matrix *a, const Matrix *at)
{
    CSRK_REQUIRE(at->nrows == a->ncols && at->ncols == a->nrows && at->nnz == a->nnz,
                 "the second matrix is %d x %d with %lld entries: not the shape of the transpose of %d x %d with %lld", at->nrows, at->ncols,
                 (long long)at->nnz, a->nrows, a->ncols, (long long)a->nnz);
    return CSRK_OK;
}

// ---- the scalar refusals the entries share, one each: CSRK_REQUIRE with the shared words behind the entry's prefix (pre, a
// string literal: "" or "topk_scores: " / "rank_entries: ").  A refusal that an entry words differently stays in that entry.
#define CSRK_CHECK_K(pre, k) CSRK_REQUIRE((k) >= 1, pre "k must be at least 1 (k=%d)", k)
#define CSRK_CHECK_ONE_PANEL(k, ldv) CSRK_REQUIRE((ldv) >= (k), "bad panel geometry k=%d ldv=%lld", k, (long long)(ldv))
#define CSRK_CHECK_TWO_PANELS(pre, k, ldu, ldv)                                                                                   \
    CSRK_REQUIRE((ldu) >= (k) && (ldv) >= (k), pre "bad panel geometry k=%d ldu=%lld ldv=%lld", k, (long long)(ldu), (long long)(ldv))
#define CSRK_CHECK_PANEL_TYPE(pre, t)                                                                                             \
    CSRK_REQUIRE((t) == CSRK_VAL_F32 || (t) == CSRK_VAL_F64, pre "panel_type must be CSRK_VAL_F32 or CSRK_VAL_F64, not %d", t)
#define CSRK_CHECK_SCALE(sc) CSRK_REQUIRE((sc) == 0 || (sc) == 1, "scale must be 0 or 1, not %d", sc)
// the row range before a handle is looked at, and against a handle's rows
#define CSRK_CHECK_ROW_ORDER(pre, rb, re) CSRK_REQUIRE((rb) >= 0 && (rb) <= (re), pre "bad row range [%d, %d)", rb, re)
#define CSRK_CHECK_ROW_RANGE(pre, rb, re, nr)                                                                                     \
    CSRK_REQUIRE((rb) >= 0 && (rb) <= (re) && (re) <= (nr), pre "bad row range [%d, %d) of %d rows", rb, re, nr)

}  // namespace csrk
