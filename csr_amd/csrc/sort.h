// What transpose.hip offers the other translation units: the transpose, the stable sort of float64 records, and "every row
// sorted by column" (all on the stable radix sort of sort_records).
#pragma once
#include "common.h"

namespace csrk {

// Transpose `a` into a new matrix (float64 values, or none: with_values == 0 or `a` holds none), entries of an output row in
// ascending source position.  Used by spgemm_abt, the knn reach index, sorted_rows_copy.
int transpose_matrix(Matrix *a, int with_values, Matrix **out, hipStream_t s);

// Stable sort of (key, int32 payload, float64 value) records by key in [0, key_range): the sorted payloads and values,
// and the run start of every key in out_ptr[0 .. key_range] (the COO-ingest form of the radix passes).  Used by
// spmm_dense.hip (the heavy rows' entries bucketed by (column tile, row group, wavefront)).
int stable_sort_records_f64(const int32_t *keys, const int32_t *payload, const double *vals, int64_t n, int32_t key_range,
                            int64_t payload_range, int64_t *out_ptr, int32_t *out_payload, double *out_vals, hipStream_t s);

// Sorting every row by column, stably, is what two stable transposes do: the first orders entries by (col, source
// position), the second by (row, col, source position).  *out has m's row pointers, the columns ascending and, among equal
// columns, m's storage order; its values are float64 (float32 widened exactly).  The caller deletes it.  Used by
// csrk_order_columns and csrk_coalesce's route 2.
int sorted_rows_copy(Matrix *m, Matrix **out);

}  // namespace csrk
