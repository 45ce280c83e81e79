// What spgemm_order.hip offers the other translation units: the column order a product is wanted in, the pass that gives a
// finished product the reference's order, and the pass's row tiers for csrk_spgemm_limits.
#pragma once
#include "common.h"

namespace csrk {

// The reference's order unless the caller (csrk_spgemm_set_order(0)) or the environment (CSRK_SPGEMM_ORDER=ascending) asks
// for ascending columns.  Used by spgemm.hip and by the dense-panel route of mult_ab (spmm_dense.hip), which writes either
// order itself.
bool spgemm_reference_order_wanted();

// c = a b as the product kernels left it (ascending columns, int32 row pointers, float64 values): re-ordered in place.
// `products`: the product kernels' own count of every row's products (a->nrows + 1 int64) when they made one, or nullptr.
int spgemm_apply_reference_order(Matrix *a, Matrix *b, Matrix *c, const DevBuf *products);

// SO_LEAST, SO_TINY, SO_WAVE, SO_MID, SO_WIN: the pass's row tiers and the placing window, for csrk_spgemm_limits
void spgemm_order_limits(int64_t out[5]);

}  // namespace csrk
