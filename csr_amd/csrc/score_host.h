// The host steps that the four factor-score drivers share (topk_scores.hip, topk_scores_for.hip, rank_entries.hip,
// rank_entries_for.hip; DESIGN.md sections 8d-8i, "The drivers").  Every entry point reads
//   scalar refusals -> handles -> early return -> NULL and alignment refusals -> plan -> pack -> device step -> unpack
// and keeps its own ORDER of refusals; what they decide is score_plan.h's.  `name` is the entry's prefix without the colon
// ("topk_scores", "rank_entries_for", ...).  For this family only: nothing here is a library-wide helper.
#pragma once
#include <cstring>
#include <type_traits>
#include <vector>

#include "panel.h"
#include "score_plan.h"

namespace csrk {

static_assert(SCORE_WAVE == WAVE, "score_plan.h restates the wavefront size");

// `seen` may be 0: *m is then NULL.  An invalid handle is refused (from_handle words it).
static int optional_handle(csrk_handle_t h, Matrix **m)
{
    *m = h ? from_handle(h) : nullptr;
    return h && !*m ? CSRK_ERR_INVALID : CSRK_OK;
}

// the kernels' three words for `seen` (all zero without one) or `test`
struct ScoreCsr {
    const void *rp;
    int ptr64;
    const int32_t *ci;
};
inline ScoreCsr score_csr(const Matrix *m) { return m ? ScoreCsr{m->d_rowptrs, m->ptr64, m->d_colinds} : ScoreCsr{nullptr, 0, nullptr}; }

// "`what`=v is above the largest supported `what`=most (`limits`)": the one refusal with CSRK_ERR_UNSUPPORTED's wording
static int check_supported(bool ok, const char *name, const char *what, int32_t v, int32_t most, const char *limits)
{
    if (ok) return CSRK_OK;
    set_error("%s: %s=%d is above the largest supported %s=%d (%s)", name, what, v, what, most, limits);
    return CSRK_ERR_UNSUPPORTED;
}

// the lists are searched, not scanned: `seen` must be canonical.  Takes the handle's lock; the caller holds none.
static int check_seen_canonical(const char *name, Matrix *seen)
{
    std::lock_guard<std::mutex> lk(seen->mu);
    CSRK_TRY(look_at_rows(seen));                                 // (remembered: a device pass only the first time a handle is asked)
    CSRK_REQUIRE(seen->canonical == 1,
                 "%s: seen is not canonical: row %d is not strictly ascending in column (csrk_order_columns sorts, "
                 "csrk_coalesce merges repeats)",
                 name, seen->noncanonical_row);
    return CSRK_OK;
}

// what `seen` and `test` must agree on (rank_entries, rank_entries_for): the shape and the device
static int check_seen_matches_test(const char *name, const Matrix *seen, const Matrix *test)
{
    CSRK_REQUIRE(seen->nrows == test->nrows && seen->ncols == test->ncols, "%s: seen is %d x %d but test is %d x %d", name, seen->nrows,
                 seen->ncols, test->nrows, test->ncols);
    CSRK_REQUIRE(seen->device == test->device, "%s: seen and test are on different devices", name);
    return CSRK_OK;
}

// the host forms look at the list before anything is sent: the first position outside [0, u_rows) is named
static int check_listed_rows(const char *name, const int32_t *rows, int64_t n_rows, int32_t u_rows)
{
    for (int64_t r = 0; r < n_rows; r++)
        CSRK_REQUIRE(rows[r] >= 0 && rows[r] < u_rows, "%s: rows[%lld]=%d is outside [0, %d)", name, (long long)r, rows[r], u_rows);
    return CSRK_OK;
}

// the listed rows of U only, in list order, packed (ld = k) on the device; rows[] has passed check_listed_rows
static int pack_listed_rows(DevBuf &d, const void *U, int64_t ldu, int64_t k, size_t es, const int32_t *rows, size_t n)
{
    const size_t line = (size_t)k * es;
    std::vector<char> picked(n * line);
    for (size_t r = 0; r < n; r++) memcpy(picked.data() + r * line, (const char *)U + (size_t)rows[r] * (size_t)ldu * es, line);
    return pack_panel(d, picked.data(), k, k, es, (int64_t)n);
}

inline bool panels_wide(const void *dU, int64_t ldu, const void *dV, int64_t ldv, int32_t k, size_t es)
{
    return score_wide(panel_16b(dU, ldu, es), panel_16b(dV, ldv, es), k, panel_per16(es));
}

// The panel-type ladder of the four launches: f(ScoreElem<T>{}, std::bool_constant<WIDE>{}) with the element type and the
// 16-B flag as compile-time tags, from a generic lambda that names the driver's xx_launch<T, WIDE ...>.
template <class T> struct ScoreElem {
    using type = T;
};
template <class F> static void score_for_panel(int panel_type, bool wide, F &&f)
{
    if (panel_type == CSRK_VAL_F64) {
        if (wide) f(ScoreElem<double>{}, std::true_type{});
        else f(ScoreElem<double>{}, std::false_type{});
    } else {
        if (wide) f(ScoreElem<float>{}, std::true_type{});
        else f(ScoreElem<float>{}, std::false_type{});
    }
}

}  // namespace csrk
