/*
 * csrk.h -- C ABI of libcsrk, the MI355X (gfx950) kernel backend for the lenskit/csr
 * `csr.kernels` hot path.
 *
 * This is the drop-in boundary: plain C, opaque integer handles, raw pointers and
 * sizes, `int` status returns (0 = CSRK_OK; on failure csrk_last_error() describes the
 * error and nothing aborts the process).  Its shape follows the reference's one native
 * interface, the MKL helper (csr/kernels/mkl/mkl_ops.h:1-31: lk_mkl_spcreate / spfree /
 * spexport / sporder / spmv / spmab / spmabt), extended by the operations the reference
 * runs outside its kernel protocol but which belong to the same hot path
 * (transpose, row extents, row normalisation).
 *
 * Each entry point names the reference interface it replaces (paths relative to the
 * reference checkout).  The Python kernel module csr_amd/kernels/hip.py binds these
 * with ctypes and implements the reference's kernel-module protocol
 * (csr/kernel.py:9-16, docs/kernels.rst:61-104) on top of them; INTEGRATION.md shows the
 * binding a reference maintainer would add.
 *
 * Memory model.  A handle owns a device-resident (HBM) copy of one CSR matrix:
 *   rowptrs[nrows+1]  int32, or int64 when ptr_is_64  (csr/csr.py:88-93)
 *   colinds[nnz]      int32                           (csr/csr.py:89)
 *   values[nnz]       float64 / float32 / absent      (csr/csr.py:94-95)
 * "host" entry points take host pointers and copy across PCIe; "_device" entry points
 * take device pointers (e.g. torch tensors' data_ptr()) and a hipStream_t passed as
 * void* (NULL = the default stream) and never synchronise the host.
 *
 * Threading: handles are immutable after creation except for the in-place operations
 * that say so; all entry points may be called concurrently from several host threads
 * (calls on the SAME handle serialise on a per-handle lock).  ctypes releases the GIL
 * around every call, matching the reference's `nogil=True` kernels.
 */
#ifndef CSRK_H
#define CSRK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSRK_API __attribute__((visibility("default")))

typedef intptr_t csrk_handle_t;      /* 0 is never a valid handle (cf. lk_mh_t, mkl_ops.h:1) */

enum {
    CSRK_OK = 0,
    CSRK_ERR_INVALID = -1,           /* bad argument / shape mismatch */
    CSRK_ERR_HIP = -2,               /* a HIP runtime call failed (no device, OOM, ...) */
    CSRK_ERR_UNSUPPORTED = -3,
    CSRK_ERR_OVERFLOW = -4           /* result does not fit the reference's int32 fields */
};

enum { CSRK_VAL_NONE = 0, CSRK_VAL_F32 = 1, CSRK_VAL_F64 = 2 };

/* SpMV algorithm selector (csrk_set_spmv_algo).  AUTO picks per matrix. */
enum {
    CSRK_SPMV_AUTO = 0,
    CSRK_SPMV_MERGE = 1,             /* merge-path tiles, LDS-staged products            */
    CSRK_SPMV_VECTOR = 2,            /* one wavefront per row segment, shfl reduction    */
    CSRK_SPMV_SCALAR = 3             /* one lane per row                                 */
};

/* ---- library / device ------------------------------------------------------------ */
CSRK_API int csrk_version(void);
/* Thread-local description of the calling thread's most recent failure. */
CSRK_API const char *csrk_last_error(void);
CSRK_API int csrk_device_count(int *count);
/* Select the HIP device used by subsequent calls from this thread (one process per
 * GPU normally passes LOCAL_RANK). */
CSRK_API int csrk_set_device(int device);
CSRK_API int csrk_synchronize(void *stream);
/* Several GPUs from one compiled host (the reference's sequential analogue is _shard_rows,
 * csr/csr.py:599-621): cut the rows into `parts` contiguous ranges balanced by entries -- bounds[g] = the first row whose
 * row pointer is >= g * nnz / parts (searchsorted(rowptrs, g * nnz / parts), the primitive of csr/csr.py:609), bounds[0] = 0,
 * bounds[parts] = nrows, never descending -- from HOST row pointers; no device is touched.  Range g then becomes a handle
 * of its own on device g (csrk_set_device(g); csrk_create with rowptrs + bounds[g] rebased by the caller, or
 * csrk_create_device on a slice already there), x is replicated, every device runs csrk_spmv_device on its range and the
 * caller's collective (RCCL all-gather of the disjoint slices, or the all-reduce north_star names) completes y: what
 * csr_amd/dist.py does with one process per GPU. */
CSRK_API int csrk_partition_rows(int32_t nrows, const void *rowptrs, int ptr_is_64, int32_t parts, int32_t *bounds);
/* Return the library's cached (free) device memory to the driver.  libcsrk keeps freed temporaries
 * and released handles' arrays in a size-bucketed pool (at most 16 GiB) to avoid hipMalloc/hipFree. */
CSRK_API int csrk_trim_cache(void);

/* ---- handles: replaces to_handle / from_handle / release_handle ---------------------
 * csr/kernels/numba/__init__.py:16-44; csr/kernels/mkl/handle.py:61-70, 95-148;
 * lk_mkl_spcreate / lk_mkl_spexport / lk_mkl_spfree (mkl_ops.h:11-14).               */

/* Copy a host CSR to the device.  `values` may be NULL iff val_type == CSRK_VAL_NONE.
 * nnz must equal rowptrs[nrows]; nnz == 0 and nrows == 0 are valid (the reference's
 * kernel fixture creates a 1x1 empty matrix, conftest.py:33-35). */
CSRK_API int csrk_create(int32_t nrows, int32_t ncols, int64_t nnz,
                         const void *rowptrs, int ptr_is_64,
                         const int32_t *colinds,
                         const void *values, int val_type,
                         csrk_handle_t *out);
/* Wrap arrays that already live in HBM.  Nothing is copied or owned: the caller keeps
 * them alive AND UNCHANGED for the handle's lifetime (same contract as to_handle,
 * docs/kernels.rst): the SpMV / SpMM plans built on the second call keep re-ordered copies of
 * colinds and values.  (libcsrk's own in-place operations -- csrk_unit_rows, csrk_center_rows,
 * csrk_order_columns -- drop those plans themselves.) */
CSRK_API int csrk_create_device(int32_t nrows, int32_t ncols, int64_t nnz,
                                const void *d_rowptrs, int ptr_is_64,
                                const int32_t *d_colinds,
                                const void *d_values, int val_type,
                                csrk_handle_t *out);
/* Idempotent on 0. */
CSRK_API int csrk_free(csrk_handle_t h);
CSRK_API int csrk_info(csrk_handle_t h, int32_t *nrows, int32_t *ncols, int64_t *nnz,
                       int *ptr_is_64, int *val_type);
/* Device memory the handle holds right now: its three arrays plus whatever SpMV / SpMM plans it has built (private
 * re-ordered streams, tables, scratch).  Builds nothing.  (The host side's handle cache budgets with it; the
 * reference's handles are host objects and have no counterpart.) */
CSRK_API int csrk_device_bytes(csrk_handle_t h, int64_t *bytes);
/* Copy the matrix back to caller-allocated host arrays sized from csrk_info
 * (any of the three may be NULL to skip it). */
CSRK_API int csrk_export(csrk_handle_t h, void *rowptrs, int32_t *colinds, void *values);
/* Device pointers of the handle's arrays (for zero-copy torch interop). */
CSRK_API int csrk_device_ptrs(csrk_handle_t h, void **d_rowptrs, void **d_colinds,
                              void **d_values);

/* ---- mult_vec: y = A x ---------------------------------------------------------------
 * csr/kernels/numba/__init__.py:55-67; lk_mkl_spmv (mkl_ops.h:29).  x has ncols float64
 * entries, y receives nrows float64 entries (every entry is written; empty rows get 0).
 * Structure-only matrices multiply with implicit 1.0 (csr/csr.py:254-262).            */
CSRK_API int csrk_spmv(csrk_handle_t h, const double *x, double *y);
/* Special values, for every product (mult_vec, mult_ab / _abt, the dense-panel SpMM, SDDMM), as the reference computes them
 * (tests/test_gpu_special_values.py pins each point):
 *   - NaN and +-Inf propagate as IEEE says: which outputs are NaN, +Inf or -Inf is the reference's.  An explicit 0.0 or -0.0
 *     value times an infinite or NaN operand gives NaN: no path skips an explicit zero.
 *   - A sum starts at +0.0, like the reference's accumulators: a row whose products are all -0.0, or cancel exactly, is +0.0.
 *     (SDDMM: its dot starts at +0.0 and is then multiplied by the value, so a negative value times a +0.0 dot is -0.0.)
 *   - float32 values times float32 x (csrk_spmv_f32x*, and mult_ab with float32 values on both operands) is a float32
 *     product: rounded once, +-Inf above FLT_MAX, subnormal (not flushed) below FLT_MIN.  Every other float32 input -- values
 *     against float64 x, float32-valued SpMM, SDDMM's float32 panels -- is widened exactly, subnormals included, and its
 *     products are float64.
 *   - An output depends only on the inputs the reference's loop reads into it: a NaN or Inf in an x entry, a B / U / V row
 *     or a panel column that no product of that output uses changes nothing, not a single bit.
 *   - Data movement (transpose, order_columns, pick_rows, from_coo, filter_zeros, topk_rows) copies values bit for bit, NaN
 *     payloads and -0.0 included; filter_zeros drops +0.0 and -0.0 and keeps every NaN; topk_rows ranks every NaN above +Inf.
 * Deliberate difference from the reference: the sign and payload of a NaN a product creates are not specified (the
 * reference's x86 loop gives the negative default NaN, the GPU the positive one); only its position is. */
/* The same with x given as float32 (host pointers).  Numba types the reference's loop by its operands
 * (csr/kernels/numba/__init__.py:55-67): float32 values times float32 x is a float32 product -- one rounding -- added to the
 * float64 accumulator; with float64 or absent values x is widened and the product is float64 (= csrk_spmv). */
CSRK_API int csrk_spmv_f32x(csrk_handle_t h, const float *x, double *y);
/* ... and with x (float32) and y (float64) already on the device; `stream` as for csrk_spmv_device: stream-ordered, nothing
 * allocated or waited for per call.  From a handle's second product on, the planned kernels widen x as they load it (the
 * copy pass, tier 0's windows, tier 1's gathers); a first product and the plan-less forms widen it once into a buffer
 * the plan keeps.  Merge algorithm only (CSRK_ERR_INVALID under `vector` / `scalar` with float32 values). */
CSRK_API int csrk_spmv_f32x_device(csrk_handle_t h, const float *d_x, double *d_y, void *stream);
CSRK_API int csrk_spmv_device(csrk_handle_t h, const double *d_x, double *d_y, void *stream);
/* The same product in two parts, for callers that ship y elsewhere while it is being completed (csr_amd/dist.py:
 * the row-partitioned multi-GPU form of csr/csr.py:584-590, where a rank's slice travels to its peers):
 *   part 1  every row of the row-major path; rows the plan cut out for its tiers (csrk_spmv_cut_rows) get 0.0
 *   part 2  the cut rows: their sums overwrite those zeros
 *   part 3  both (= csrk_spmv_device).
 * Part 1 then part 2 on one stream give bit for bit what part 3 gives. */
CSRK_API int csrk_spmv_device_part(csrk_handle_t h, const double *d_x, double *d_y, void *stream, int part);
/* The rows (ascending indices into this handle's rows) whose y entries part 2 writes: *n_rows of them, copied to the
 * device buffer d_rows if it is not NULL and holds `capacity` >= *n_rows entries.  Builds the SpMV plan if needed. */
CSRK_API int csrk_spmv_cut_rows(csrk_handle_t h, int32_t *d_rows, int64_t capacity, int64_t *n_rows);
CSRK_API int csrk_set_spmv_algo(csrk_handle_t h, int algo);
/* Name of the kernel the handle's plan resolved to, e.g. "merge" (after first use). */
CSRK_API const char *csrk_spmv_algo_name(csrk_handle_t h);
/* Launch geometry of the dominant SpMV kernel (for roofline accounting in bench.py). */
CSRK_API int csrk_spmv_plan_info(csrk_handle_t h, int64_t *n_tiles, int32_t *tile_items);

/* out[0..n) <- {0 tiles (or segments), 1 items per tile, 2 rows cut out of the tile path, 3 entries on
 * the tile path, 4 tier-0 tiles, 5 tier-0 column blocks, 6 tier-0 row threshold, 7 tier-0 block width,
 * 8 split mode (0 none, 2 panels), 9 tier-0 rows,
 * 10 tier-0 entries, 11 tier-1 rows, 12 tier-1 pairs, 13 tier-1 entries, 14 tier-1 row threshold,
 * 15 tier-1 block width, 16 columns in the hot-column pack (0: none), 17 sampled share of the row-major
 * path's entries on packed columns (ppm), 18 1 (tier 0 in accumulator form: the only one), 19 pack slots,
 * 20 short rows on the light stream (1) or on the merge-path tile kernel (0), 21 light-stream tiles,
 * 22 non-empty rows of the light stream, 23 its workgroups, 24 light-stream entries whose x values are staged
 * per call (cold staging), 25 bytes of device memory the plan holds, 26 tiles per staging round held in LDS (0: none),
 * 27 workgroups of the tier-0 accumulator kernel, 28 0 (reserved), 29..33 the plan's bytes by part: tier 0's accumulator
 * stream, tier 1's pair panel, the light stream, cold staging + pack, tables,
 * the light stream's form, all 0 without a stream: 34 dense layout (every row of the view has a run: no row ids, no gaps)
 * (0/1), 35 3-byte index words (0/1), 36 pack slots the stream kernel reads from LDS, 37 rounds in all and 38 the most one
 * workgroup walks (staged rounds; without staging the kernel's own rounds of one tile per wavefront), 39 column blocks of
 * the copy pass and 40 their width in columns (0 without staging), 41 float32 stored values (0/1),
 * tier 1's layout, all 0 without the tier: 42 column blocks, 43 tiles, 44 carry rows kept behind the block partials (a row's
 * first carries, at most 4), 45 carries listed beyond those, 46 workgroups of the pair kernel's own list (padding groups of
 * the XCD streams included), 47 the padding groups among them};  n <= 48. */
CSRK_API int csrk_spmv_plan_stats(csrk_handle_t h, int64_t *out, int n);
/* The compile-time constants the light stream's form is decided by, callable without a device: out[0..n) <- {0 entries per
 * tile (512), 1 consecutive entries per lane (8), 2 wavefronts per workgroup (8), 3 in-order carry hand-overs (3: a run whose
 * sum is stored at most 3 lanes after the lane it starts in is summed in the reference's order), 4 batches of 64 run slots whose row ids are fetched
 * ahead (4), 5 pack slots in LDS without staging (15360) and 6 with it (8176), 7 staged values per round at most (8192),
 * 8 tiles per round at most (128), 9 columns per block of the copy pass at most (9984), 10 pairs per batch of its loop
 * (8192), 11 the shortest row the forced split cuts out (128), 12 pack slots at most (524288)};  n <= 13. */
CSRK_API int csrk_spmv_stream_limits(int64_t *out, int n);

/* Kernel timing for roofline accounting: between begin and end every csrk_spmv_device call on
 * this handle brackets its streaming kernels -- [0] the tile / segment / row kernel, [1] and [2]
 * the panel kernels of tier 0 and tier 1 (merge algorithm only) -- with hipEvent pairs recorded on
 * the launch stream; nothing synchronises until csrk_spmv_profile_end, which returns the number of
 * recorded launches and mean_ms[3], their mean durations in milliseconds (0 if a kernel did not run).
 * At most `max_records` launches are recorded. */
CSRK_API int csrk_spmv_profile_begin(csrk_handle_t h, int max_records);
/* Time only every n-th csrk_spmv_device call between begin and end (default 1: all of them).  The event
 * pairs sit on the launch stream between the kernels and cost ~3 us apiece -- 20 us per SpMV with three
 * timed kernels, 3 % of the headline step; call before csrk_spmv_profile_begin. */
CSRK_API int csrk_spmv_profile_every(csrk_handle_t h, int every_n);
/* Which of the four kernels get event pairs: bit c of `mask` = channel c of csrk_spmv_profile_end4 (default 0xf: all).
 * A timed region that needs one kernel's duration pays for one event pair per timed call instead of four. */
CSRK_API int csrk_spmv_profile_channels(csrk_handle_t h, int mask);
CSRK_API int csrk_spmv_profile_end(csrk_handle_t h, int *n_records, float *mean_ms);
/* The same with mean_ms[4]: [3] = the cold-staging pass that feeds the light stream (ls_stage_kernel; 0 if the plan
 * has none). */
CSRK_API int csrk_spmv_profile_end4(csrk_handle_t h, int *n_records, float *mean_ms);

/* ---- mult_ab / mult_abt: sparse x sparse -> sparse ------------------------------------
 * csr/kernels/numba/multiply.py:13-57; lk_mkl_spmab / lk_mkl_spmabt (mkl_ops.h:30-31).
 * The product is a NEW handle owned by the caller (rowptrs int32 as in multiply.py:28,
 * values float64).  Structural zeros produced by cancellation are KEPT (the caller
 * filters them, csr/csr.py:555).  Columns inside a product row come in the reference's
 * order (reverse order of first discovery: csrk_spgemm_set_order below).
 * Both operands need values (multiply.py:115,120).  CSRK_ERR_OVERFLOW if the product
 * has more than INT32_MAX entries.                                                     */
CSRK_API int csrk_spgemm_ab(csrk_handle_t a, csrk_handle_t b, csrk_handle_t *c);
CSRK_API int csrk_spgemm_abt(csrk_handle_t a, csrk_handle_t b, csrk_handle_t *c);
/* Column order inside the rows of a product: 1 = the reference's (default) -- _sym_mm pushes a newly discovered column
 * onto the front of the row's list (csr/kernels/numba/multiply.py:79-82) and copies the list out front to back (:94-97):
 * reverse order of first discovery, so colinds and values are the reference's arrays bit for bit --, 0 = ascending (what
 * the product kernels emit; saves the ordering pass: a second walk over the products, csrc/spgemm_order.hip), -1 = follow
 * the environment variable CSRK_SPGEMM_ORDER ("ascending" selects 0; unset or anything else: 1).  Process-wide; every
 * value has the same bits either way.  csrk_spgemm_get_order: the order in force (0 or 1). */
CSRK_API int csrk_spgemm_set_order(int order);
CSRK_API int csrk_spgemm_get_order(int *order);
/* A x dense B through the reference's own entry (BASELINE configs[2]: the reference has no dense-panel call; a caller hands
 * B over as a fully populated CSR, csr/csr.py:524-567 -> multiply.py:13-38).  csrk_spgemm_ab / _abt recognise such a B on the
 * device -- every row holds all k columns 0 .. k - 1 in ascending order, so that its values ARE the row-major panel -- and
 * run the dense-panel kernels (csrk_spmm_dense's), writing C as the reference returns it: int32 row pointers with k entries
 * per row of C whose row of A holds an entry and none otherwise, columns in the order in force (csrk_spgemm_set_order):
 * k - 1 .. 0 in the reference's (reverse order of first discovery, multiply.py:79-82, 94-97), 0 .. k - 1 in ascending
 * order -- the same values either way --, explicit zeros kept, values = the panel's sums (work[c] += a * b over the row's entries in
 * storage order, :110-122: bit for bit for rows of A of at most 64 entries, the dense-panel kernels' fixed order of
 * partial sums beyond -- within 1e-12 of sum |a b|).  A B whose rows are short of a column or in another order, and
 * float32 values on BOTH operands (float32 products, multiply.py:120), take the general product.  CSRK_SPGEMM_DENSE=0
 * switches the route off.  csrk_spgemm_last_route: what the calling thread's last product took -- 0 the general product,
 * 1 the dense-panel route; 0 after a call that failed. */
CSRK_API int csrk_spgemm_last_route(int *route);
/* Diagnostics: what the general product (csrc/spgemm.hip) did with the rows of the calling thread's last csrk_spgemm_ab /
 * _abt.  All zero after a call that failed or took the dense-panel route; filled from what the driver holds on the host,
 * without a kernel, a copy or a synchronisation of its own.  Rows by their product count u = sum over A_i of |B_j|:
 *   out[0]  1: the general product ran
 *   out[1]  1: FAST form (int32 row pointers and float64 values on both operands), 0: the general form
 *   out[2]  column strips per row in force (0: strips off -- general form, B's rows not ascending, too many columns,
 *           CSRK_SPGEMM_STRIPS=0)
 *   out[3]  rows on the strips, [4] their entries of A, [5] 1: the strips' one-pass form, 0: two passes (or no strip row)
 *   out[6]  rows of expand-sort-compress, [7] their products
 *   out[8]  rows of the fallback paths (more than 1024 products, neither strips nor expand-sort-compress),
 *   out[9]  1: their distinct outputs were counted in LDS, which splits them into [10] LDS tiles, [11] the 8192-slot hash
 *           table, [12] HBM work rows (without the LDS count all of them are HBM work rows)
 *   out[13] 1: the rows of at most 128 products in one pass (0: two passes, or there is none)
 *   out[14] 1: the 32-lane kernel (33 .. 128 products) ran, [15] 1: the workgroup hash kernel (129 .. 1024 products) ran
 * csrk_spgemm_limits: the constants behind those decisions -- [0] products of a sub-wavefront row at most (128), [1] of a
 * workgroup-hash row (1024), [2] rows above this many products go to expand-sort-compress (32), [3] its positions per tile
 * (1024), [4] columns per strip (832), [5] strips per row at most (256), [6] products per (A entry, strip) and [7] per
 * (row, strip) a strip row has at least on average (4, 512), [8] entries of A from which a strip row is scheduled first
 * (1024), [9] columns per LDS tile (20096), [10] LDS tiles per row at most (8), [11] columns the LDS count covers (2^20),
 * [12] distinct outputs of a big-hash row at most (4096), [13] / [14] entries of A above which a row is counted by a
 * wavefront / by all wavefronts (64, 4096), [15] .. [18] the ordering pass's row tiers in products (64, 256, 1024, 4096),
 * [19] product indices per window of its placing kernel (2^19). */
CSRK_API int csrk_spgemm_last_stats(int64_t *out, int n);
CSRK_API int csrk_spgemm_limits(int64_t *out, int n);

/* ---- dense-panel SpMM: C = A B, B dense row-major [ncols x k] --------------------------
 * Not a reference entry point (the reference's mult_ab is sparse x sparse only); serves
 * BASELINE.json configs[2].  Equals mult_ab(A, CSR(B)) densified.  ldb/ldc in elements.
 * Column blocks of a wider panel: d_B may point at column c0 of a panel with ldb > k, and d_C into a wider output
 * (ldc > k); every column of C is computed as it is in a full-width call on the same handle, bit for bit.  B and C need
 * only 8-B alignment: when d_B or d_C is not 16-B aligned, or ldb or ldc is odd, the kernels take their 8-B loads and
 * stores for that call.  The plan is built by a handle's first call and serves every k after it (the first call's
 * k * ncols decides whether the longest rows take the register-accumulator form). */
CSRK_API int csrk_spmm_dense(csrk_handle_t a, const double *B, int32_t k, int64_t ldb,
                             double *C, int64_t ldc);
CSRK_API int csrk_spmm_dense_device(csrk_handle_t a, const double *d_B, int32_t k, int64_t ldb,
                                    double *d_C, int64_t ldc, void *stream);
/* Diagnostics: the dense-panel plan of a handle after its first csrk_spmm_dense*: out[0] = 1 when the longest rows run in
 * the register-accumulator form (csrc/spmm_dense.hip), [1] their row-length threshold, [2] their number, [3] row groups,
 * [4] column ranges, [5] their entries, [6] column tiles, [7] segments of the other rows, [8] of which partial (split rows). */
CSRK_API int csrk_spmm_plan_stats(csrk_handle_t a, int64_t *out, int n);
/* Diagnostics, read-only: the plan's column ranges, out[q] = first column tile (128 rows of B) of range q, q = 0 .. R, with
 * out[R] = the number of tiles (R = csrk_spmm_plan_stats' [4]); n, the room in out, must be at least R + 1.  Without the
 * register-accumulator form (stats' [0] = 0) nothing is written. */
CSRK_API int csrk_spmm_plan_ranges(csrk_handle_t a, int32_t *out, int n);

/* ---- sampled dense-dense product (SDDMM): one value per stored entry ---------------------
 * Not a reference entry point (the reference's mult_ab is sparse x sparse only); the transpose-dual of
 * csrk_spmm_dense.  U is dense row-major [nrows x k], V dense row-major [ncols x k], both float32 or both float64
 * (panel_type CSRK_VAL_F32 / CSRK_VAL_F64); ldu / ldv >= k in elements.  For every stored entry e = (i, j), in the
 * handle's storage order (unsorted and repeated columns are just more entries):
 *   out[e] = dot(U[i, :], V[j, :])                        scale = 0
 *   out[e] = values[e] * dot(U[i, :], V[j, :])            scale = 1 (float32 values widened; structure-only: 1.0, as above)
 * out is float64 whatever the panel type.  Order of addition, fixed by k and the panel type alone (not by the entry's
 * position, its row's length, the pointer width, the strides, the alignment, the stream or the launch, so an entry gets
 * the same bits whatever else the matrix holds): 16 partial sums, partial l over its columns below k in ascending order
 * (in each 64-column chunk c: float64 64 c + {2 l, 2 l + 1, 32 + 2 l, 33 + 2 l}, float32 64 c + {4 l .. 4 l + 3}),
 * each step one fused multiply-add from +0.0 (float32 panels: the product of the
 * widened operands is exact, so one rounding per step); then the 16 partials added by the fixed tree of distances
 * 1, 2, 4, 8 (csrc/sddmm.hip); then the value multiplied in once.  Accuracy: within (k / 16 + 4) ulp-scale roundings of
 * sum_t |u_t v_t| (times |value|), far inside 1e-12 of it for any k a panel holds.  NaN and Inf propagate as IEEE says.
 * Alignment: U and V need their element size; when both are 16-B aligned and ldu, ldv are multiples of 16 B the kernel
 * takes 16-B loads, else 8-B (float64) or 4-B (float32) ones -- the same bits either way.
 * nnz = 0 or nrows = 0: CSRK_OK, nothing launched.  CSRK_ERR_INVALID for k < 1, ldu < k, ldv < k, an unknown panel_type,
 * a scale other than 0 / 1, or a NULL U, V or out when nnz > 0.
 * Host form: host panels in, out[nnz] float64 in host memory (the panels cross packed; synchronous). */
CSRK_API int csrk_sddmm(csrk_handle_t s, const void *U, int64_t ldu, const void *V, int64_t ldv,
                        int32_t k, int panel_type, int scale, double *out);
/* Device form: d_U, d_V, d_out in HBM (e.g. torch tensors' data_ptr()), launched on `stream` (NULL = the default
 * stream); nothing is allocated and the host is not synchronised. */
CSRK_API int csrk_sddmm_device(csrk_handle_t s, const void *d_U, int64_t ldu, const void *d_V, int64_t ldv,
                               int32_t k, int panel_type, int scale, double *d_out, void *stream);

/* ---- per-row Gram matrices: one k x k block per row ------------------------------------------
 * Not a reference entry point: the left-hand side of the normal equations of alternating least squares,
 * (sum_j w_ij v_j v_j^T + lambda I) u_i = sum_j c_ij v_j over row i's stored columns j; the right-hand side is
 * csrk_spmm_dense, the solve is the caller's.  The gather of csrk_sddmm (a row of V per stored entry), reduced across a
 * row's entries into a dense block.  out is float64, packed: out[(i - row_begin) * k * k + p * k + q] for rows
 * row_begin <= i < row_end.
 *   1. Operands.  V is dense row-major [ncols x k], float32 or float64 (panel_type CSRK_VAL_F32 / CSRK_VAL_F64), ldv >= k in
 *      elements.  scale = 0: w = 1 for every entry.  scale = 1: w = values[e], float32 values widened exactly, 1.0 for a
 *      structure-only matrix (csrk_sddmm's rule).  base is NULL or a k x k float64 matrix, packed row-major, of which
 *      only the lower triangle (p >= q) is read.
 *   2. Fixed arithmetic, per element.  For each row i and each p >= q the accumulator G[p][q] starts at base[p][q], or at
 *      +0.0 when base is NULL.  Then, for the row's entries in storage order, j the entry's column, one step each:
 *          t = round(w * V[j][p]);   G[p][q] = fma(t, V[j][q], G[p][q])
 *      one rounded multiply and one fused multiply-add (scale = 0: t is V[j][p] itself; float32 panel elements are
 *      widened exactly first).  Then G[q][p] = G[p][q]: the block is exactly symmetric.  Unsorted and repeated columns
 *      are just more entries.  An empty row gives base mirrored, or all +0.0 when base is NULL.
 *   3. An element depends on its row's entries, V's rows at those columns, k, the panel type, scale and base only: not on
 *      the row range asked for, the pointer width, ldv, the alignment, the stream, the launch geometry or repeated calls.
 *      (csrc/gram.hip: parallel over rows and over the k (k + 1) / 2 elements, never over a row's entries; no float
 *      atomics, no split sums.)
 *   4. Special values.  NaN and +-Inf propagate as IEEE says; an explicit 0.0 or -0.0 weight or V element times an
 *      infinite or NaN operand gives NaN: no path skips a zero.  A row is changed only by NaN / Inf in V rows that it
 *      references.  A created NaN has its position specified, not its sign or payload (csrk_combine's rule 7).
 *   5. Alignment.  V needs its element size; base and out 8 B.  When V is 16-B aligned and ldv and k are whole numbers of
 *      16-B pieces the kernel takes 16-B loads, else element loads -- the same bits either way.
 *   6. Offsets into out are 64-bit: (row_end - row_begin) * k * k may exceed 2^31.  The caller chooses the row range so
 *      that the output fits (2 10^6 rows at k = 64 would be 65 GB).
 *   7. CSRK_ERR_INVALID: k < 1, ldv < k, an unknown panel_type, a scale other than 0 / 1, row_begin < 0, row_end > nrows,
 *      row_begin > row_end, or a NULL out (or a NULL V when the matrix stores entries) when there is something to write.
 *      CSRK_ERR_UNSUPPORTED: k above csrk_gram_limits' out[0] (at least 128).  row_begin == row_end: CSRK_OK, nothing
 *      launched.  out is not written by a refused call.  h is not modified and keeps its plans.
 *   8. Limits (csrk_gram_limits, below): out[0] = the largest k; [1] = the entries of a row staged through LDS per step;
 *      then the k classes, ascending: [2] = the largest k at which 16 lanes take a row, [3] = the largest k at which a
 *      wavefront takes a row, [4] = the largest k at which a workgroup takes a row with one 4 x 4 tile per thread (above
 *      it, up to three).  By rule 3 no class changes a bit of the result.
 * Column indices address V: they must lie in [0, ncols), as for csrk_sddmm.
 * Host form: host pointers in and out (the panel crosses packed; synchronous). */
CSRK_API int csrk_gram_rows(csrk_handle_t h, int32_t row_begin, int32_t row_end, const void *V, int64_t ldv,
                            int32_t k, int panel_type, int scale, const double *base, double *out);
/* Device form: d_V, d_base, d_out in HBM, launched on `stream` (NULL = the default stream); nothing is allocated and the
 * host is not synchronised. */
CSRK_API int csrk_gram_rows_device(csrk_handle_t h, int32_t row_begin, int32_t row_end, const void *d_V, int64_t ldv,
                                   int32_t k, int panel_type, int scale, const double *d_base, double *d_out,
                                   void *stream);
/* Diagnostics: the five limits of rule 8 above, in its order;  n <= 5.  No device is touched. */
CSRK_API int csrk_gram_limits(int64_t *out, int n);

/* ---- the ALS half-step: solve each row's normal equations ----------------------------------------
 * Not reference entry points.  csrk_solve_blocks solves n packed symmetric k x k systems; csrk_als_rows builds each row's
 * system (csrk_gram_rows' block, a ridge, the right-hand side) in one pass over the row's entries and solves it on the
 * chip: k float64 per row are written, the k x k block never is.  It accumulates with the routine csrk_gram_rows runs
 * (csrc/gram_tile.h) and both solve with one device routine (csrc/als.hip), so
 * csrk_als_rows equals csrk_gram_rows + the ridge + csrk_solve_blocks bit for bit.  All arithmetic is float64;
 * fma(-a, b, c) is round(c - a b), one rounding.
 *
 * S. The solve.  Per system: G (k x k, packed row-major, ONLY THE LOWER TRIANGLE p >= q IS READ) and b[k] in, x[k] and an
 *    info word out.  An LDL^T factorisation with a fixed order of operations:
 *        for j = 0 .. k-1:
 *            for i = j .. k-1:
 *                a = G[i][j];   for t = 0 .. j-1 (ascending):  a = fma(-L[i][t], C[j][t], a);   C[i][j] = a
 *            d_j = C[j][j];   r_j = 1.0 / d_j                       (one correctly rounded division per column)
 *            for i = j+1 .. k-1:  L[i][j] = round(C[i][j] * r_j)
 *        forward:  for i = 0 .. k-1:   z_i = b[i];  for t = 0 .. i-1 ascending:    z_i = fma(-L[i][t], z_t, z_i)
 *        scale:    y_i = round(z_i * r_i)
 *        back:     for i = k-1 .. 0:   x_i = y_i;   for t = k-1 .. i+1 descending: x_i = fma(-L[t][i], x_t, x_i)
 *   S1. No pivoting, no square root, no special case.  A zero, negative or NaN pivot goes through IEEE arithmetic and the
 *       system's x becomes Inf or NaN; info = j + 1 for the first j where d_j > 0 is false, 0 when every pivot is positive.
 *   S2. Every element of C, L, z and x is one serial chain in the order above.  Parallelism is over systems and over
 *       elements, never inside a chain; no float atomics, no split sums.  The result depends on (G's lower triangle, b, k)
 *       only: not on the launch geometry, the k class, ldb, ldx, the alignment, the stream or repeated calls.
 *   S3. csrk_solve_blocks: G is n * k * k float64, system s at G + s k k; b[s * ldb + p], x[s * ldx + p], ldb, ldx >= k in
 *       elements; info is int32[n] or NULL.  x may not overlap G or b.  CSRK_ERR_INVALID: n < 0, k < 1, ldb < k, ldx < k,
 *       or a NULL G, b or x when n > 0.  CSRK_ERR_UNSUPPORTED: k above csrk_als_limits' out[0] (at least 128).  n = 0:
 *       CSRK_OK, nothing launched.  A refused call writes neither x nor info.
 *
 * A. The fused row.  For row i of [row_begin, row_end), its entries e = (i, j) in storage order, n_i of them:
 *   A1. Block.  G is exactly csrk_gram_rows' rule 2, with the same V, panel_type, scale, base and lower triangle.
 *   A2. Ridge.  After the chain, for each p: G[p][p] = fma(lam_n, (double)n_i, G[p][p]).  lam_n is one double for every row;
 *       0.0 leaves finite values as they are.  lam_n * n_i is the count-weighted ridge of explicit ALS; base carries
 *       lambda I and, for implicit feedback, V^T V.
 *   A3. Right-hand side.  b[p] starts at +0.0 and takes one step per entry, in storage order:
 *           b[p] = fma(c_e, V[j][p], b[p])
 *       with c_e by rhs_mode: CSRK_ALS_RHS_ONES 1.0; CSRK_ALS_RHS_VALUES the entry's value, float32 widened exactly, 1.0 for
 *       a structure-only matrix (csrk_sddmm's rule); CSRK_ALS_RHS_ONE_PLUS round(1.0 + that value) (values stored as
 *       confidence - 1).
 *   A4. Solve and output.  Rule S on (G, b); out[(i - row_begin) * ldo + p] = x[p], ldo >= k in elements, so the caller
 *       may write straight into a wider factor panel (the other columns of out are not touched); info[i - row_begin] is
 *       int32, and info may be NULL.
 *   A5. Empty rows solve base x = 0: x is +0.0 everywhere when base is positive definite (info 0).  With base NULL the
 *       first pivot is +0.0: info is 1 and every x is NaN.
 *   A6. The rest is csrk_gram_rows': unsorted and repeated columns are just more entries; NaN and Inf reach only the rows
 *       that reference them; V is read in 16-B pieces when its pointer, ldv and k allow, else by element -- the same bits;
 *       offsets are 64-bit; h is not modified and keeps its plans; the device form allocates nothing and never
 *       synchronises the host; a refused call writes neither out nor info.
 *   A7. CSRK_ERR_INVALID: every refusal of csrk_gram_rows (its rule 7), ldo < k, an unknown rhs_mode, a NULL out when
 *       there are rows.  CSRK_ERR_UNSUPPORTED: k above csrk_als_limits' out[0] (at least 128).  row_begin == row_end:
 *       CSRK_OK, nothing launched.
 *   Limits (csrk_als_limits): out[0] = the largest k; [1] = the entries of a row staged through LDS per step; then the k
 *   classes, ascending: [2] = the largest k at which 16 lanes take a system, [3] = a wavefront, [4] = a workgroup with one
 *   4 x 4 tile per thread (above it, up to three).  By S2 no class changes a bit.
 * Host forms: host pointers in and out (panels cross packed; synchronous). */
enum { CSRK_ALS_RHS_ONES = 0, CSRK_ALS_RHS_VALUES = 1, CSRK_ALS_RHS_ONE_PLUS = 2 };
CSRK_API int csrk_solve_blocks(int64_t n, int32_t k, const double *G, const double *b, int64_t ldb, double *x,
                               int64_t ldx, int32_t *info);
CSRK_API int csrk_als_rows(csrk_handle_t h, int32_t row_begin, int32_t row_end, const void *V, int64_t ldv, int32_t k,
                           int panel_type, int scale, int rhs_mode, const double *base, double lam_n, double *out,
                           int64_t ldo, int32_t *info);
/* Device forms: every pointer in HBM, launched on `stream` (NULL = the default stream); nothing is allocated and the host
 * is not synchronised. */
CSRK_API int csrk_solve_blocks_device(int64_t n, int32_t k, const double *d_G, const double *d_b, int64_t ldb,
                                      double *d_x, int64_t ldx, int32_t *d_info, void *stream);
CSRK_API int csrk_als_rows_device(csrk_handle_t h, int32_t row_begin, int32_t row_end, const void *d_V, int64_t ldv,
                                  int32_t k, int panel_type, int scale, int rhs_mode, const double *d_base,
                                  double lam_n, double *d_out, int64_t ldo, int32_t *d_info, void *stream);
/* Diagnostics: the five limits above, in that order;  n <= 5.  No device is touched. */
CSRK_API int csrk_als_limits(int64_t *out, int n);

/* ---- the ALS half-step by conjugate gradient: no k x k block ---------------------------------------
 * Not a reference entry point.  csrk_als_rows_cg runs at most `steps` conjugate-gradient steps per row on the system of
 * csrk_als_rows, M_i x = b_i with M_i = base + sum_e w_e v_e v_e^T + rho_i I, warm-started from x0, WITHOUT forming M_i:
 * a step is one pass over the row's V rows (a dot and an axpy per entry) and, with a base, one k x k matrix-vector
 * product, where the exact route pays n_i k^2 / 2 to build the block and k^3 / 6 to factorise it.  The result is a
 * function of the inputs, fixed below.  All arithmetic is float64; fma(a, b, c) is round(a b + c), one rounding.
 *
 * C. For row i of [row_begin, row_end), its entries e = (i, j_e) in storage order, n_i of them, v_e = row j_e of V
 *    widened exactly to float64:
 *   C1. Operands.  V, panel_type, scale, rhs_mode, ldv and ldo are csrk_als_rows'; w_e follows its scale rule (rule 1 of
 *       csrk_gram_rows), c_e rule A3.  base is NULL or k x k float64, packed row-major, and it is read AS STORED, ALL OF
 *       IT: the element used for (t, u) is base[u * k + t]; the caller passes a symmetric matrix.  (csrk_als_rows reads
 *       the lower triangle only: a caller who filled just that must mirror it before calling this entry.)  lam and lam_n
 *       are doubles; the diagonal term is rho_i = fma(lam_n, (double)n_i, lam).  steps >= 0; tol2 >= 0 and not NaN.  x0
 *       is NULL or float64 with ldx0 >= k in elements: row i reads x0[(i - row_begin) * ldx0 + t].  resid (float64[n])
 *       and taken (int32[n]), n = row_end - row_begin, may each be NULL.
 *   C2. DOT(a, b) over k elements is csrk_sddmm's order for the call's panel type: 16 partials s_0 .. s_15 from +0.0;
 *       element t belongs to partial l = (t mod 32) div 2 for float64 panels, l = (t mod 64) div 4 for float32 panels;
 *       each partial takes its elements in ascending t, s_l = fma(a_t, b_t, s_l); then the balanced tree in index order,
 *       (s_0 + s_1), (s_2 + s_3), ..., pairs of those, again, then the last two: every addition rounded on its own.
 *   C3. MATVEC(y) -> q.  q_t starts at +0.0.  With a base, for u = 0 .. k-1 ascending: q_t = fma(base[u * k + t], y_u, q_t).
 *       Then q_t = fma(rho_i, y_t, q_t).  Then for the entries in storage order: d_e = DOT(v_e, y); g_e = round(w_e d_e)
 *       under scale = 1, else d_e; q_t = fma(g_e, v_e[t], q_t).
 *   C4. Right-hand side.  b_t is rule A3's chain: from +0.0, b_t = fma(c_e, v_e[t], b_t) in storage order.
 *   C5. Start.  x0 NULL: x = +0.0 and r = b; no product is formed.  Otherwise x = the x0 row, q = MATVEC(x),
 *       r_t = round(b_t - q_t).  Then p = r, rs = DOT(r, r), taken = 0.
 *   C6. Step.  At most `steps` times, and only while rs > tol2 is true (a NaN rs stops):
 *           q = MATVEC(p);  pq = DOT(p, q);  alpha = round(rs / pq);
 *           x_t = fma(alpha, p_t, x_t);  r_t = fma(-alpha, q_t, r_t);
 *           rn = DOT(r, r);  beta = round(rn / rs);  p_t = fma(beta, p_t, r_t);  rs = rn;  taken += 1
 *       Both divisions are correctly rounded.  No other special case: pq <= 0 or NaN goes through IEEE arithmetic.
 *   C7. Output.  out[(i - row_begin) * ldo + t] = x_t (the other columns of out are not touched); resid[i - row_begin] =
 *       rs, the squared 2-norm of the recurrence's residual at the stop; taken[i - row_begin] = taken.  d_x0 == d_out
 *       with ldx0 == ldo is allowed (a row's x0 is read before its out is written, by the team that writes it); any other
 *       overlap is undefined.
 *   C8. A row's outputs depend only on its entries, the V rows they name, base, lam, lam_n, steps, tol2, its x0 row, k,
 *       the panel type, scale and rhs_mode: not on the row range, the pointer width, ldv, ldx0, ldo, the alignment, the
 *       load form, the stream, the launch geometry or repeated calls.  Parallelism is over rows and over elements t, never
 *       inside a chain; no float atomics.  Unsorted and repeated columns are just more entries.  NaN and Inf reach only
 *       the rows that reference them (a created NaN has its position specified, not its sign or payload).  An empty row
 *       with x0 NULL gives x = +0.0, resid +0.0, taken 0.
 *   C9. CSRK_ERR_INVALID: every refusal of csrk_als_rows (rule A7), steps < 0, tol2 < 0 or NaN, ldx0 < k with an x0, an
 *       x0, resid or taken that is not aligned to its element size.  CSRK_ERR_UNSUPPORTED: k above csrk_als_cg_limits'
 *       out[0].  What the scalars alone decide (everything but row_end > nrows, NULL pointers and alignment) is refused
 *       before the handle is looked at.  row_begin == row_end: CSRK_OK, nothing launched.  A refused call writes nothing.  The device form
 *       allocates nothing and never synchronises the host; h is not modified and keeps its plans.
 *   C10. A hazard, not a special case.  With tol2 = 0 and steps far past convergence the residual walks into the
 *       subnormals, where pq can reach 0 before rs does and IEEE gives Inf.  (k = 1, M = 12.75, b = 8 never reaches
 *       rs = 0: after 5 steps rs = 1.7e-167.)  Callers who ask for many steps pass a tol2.
 *   C11. Long rows.  A row of at least L entries (csrk_als_cg_set_long below; L = 0: no row) is a long row: a whole
 *       workgroup takes it instead of one team -- several teams take the d_e, which are independent of one another, one
 *       wavefront the chains into q_t and b_t in storage order.  C8 already covers it: the launch geometry changes no
 *       bit, so out, resid and taken are the same with the class on, off, or at any L.  The device form issues up to two
 *       launches on `stream`, the long rows' first (workgroup g scans the lengths of rows [g S, (g + 1) S) of the range
 *       and solves the long ones among them); it still allocates nothing and never synchronises.  C7's in-place rule
 *       holds: a long row's x0 is read by the workgroup that later writes its out, and no team touches that row.
 *   Limits (csrk_als_cg_limits): out[0] = the largest k (at least 128); [1] = the lanes of a row's team; [2] = the entries a
 *   team has in flight per step of its entry loop;  n <= 3.  No device is touched.
 * Host form: host pointers in and out (panels cross packed; synchronous). */
CSRK_API int csrk_als_rows_cg(csrk_handle_t h, int32_t row_begin, int32_t row_end, const void *V, int64_t ldv, int32_t k,
                              int panel_type, int scale, int rhs_mode, const double *base, double lam, double lam_n,
                              int32_t steps, double tol2, const double *x0, int64_t ldx0, double *out, int64_t ldo,
                              double *resid, int32_t *taken);
/* Device form: every pointer in HBM, launched on `stream` (NULL = the default stream). */
CSRK_API int csrk_als_rows_cg_device(csrk_handle_t h, int32_t row_begin, int32_t row_end, const void *d_V, int64_t ldv,
                                     int32_t k, int panel_type, int scale, int rhs_mode, const double *d_base, double lam,
                                     double lam_n, int32_t steps, double tol2, const double *d_x0, int64_t ldx0,
                                     double *d_out, int64_t ldo, double *d_resid, int32_t *d_taken, void *stream);
CSRK_API int csrk_als_cg_limits(int64_t *out, int n);
/* The long-row class of rule C11.  Process-wide, like csrk_spgemm_set_order: entries >= 1: a row of at least that many
 * entries is a long row; 0: the class is off (one launch, as without the class); -1: follow the environment variable
 * CSRK_ALS_CG_LONG (a decimal count; unset, or not a count: the default, csrk_als_cg_long_limits' out[0]).  Anything below
 * -1 is CSRK_ERR_INVALID and changes nothing.  csrk_als_cg_get_long: the L in force (0 = off).  No device is touched. */
CSRK_API int csrk_als_cg_set_long(int64_t entries);
CSRK_API int csrk_als_cg_get_long(int64_t *entries);
/* out[0] = the default L; [1] = the threads of a long row's workgroup; [2] = S, the rows of the range whose lengths one
 * workgroup scans; [3..6] = C, the entries of one chunk of the row's LDS image, for (float64 panel, k <= 64), (float64,
 * k <= 128), (float32, k <= 64), (float32, k <= 128); [7] = the image's buffers (2);  n <= 8.  No device is touched. */
CSRK_API int csrk_als_cg_long_limits(int64_t *out, int n);
/* The calling thread's last csrk_als_rows_cg[_device], all 0 after a refused or failed call: out[0] = 1 when it launched
 * (there were rows); [1] = the L in force (0 = off); [2] = 1 when the long rows' launch was issued (L > 0, rows, and the
 * matrix has entries); [3] = its workgroups; [4] = the rows it solved and [5] = their entries, counted on the device
 * (one integer atomic add per row) and read back by the host form -- the device form never synchronises and reports -1
 * in both when it issued the launch;  n <= 6. */
CSRK_API int csrk_als_cg_last_stats(int64_t *out, int n);

/* ---- panel_gram: G = V^T V + ridge I, the matrix every row's system shares ---------------------------
 * Not a reference entry point.  Implicit-feedback ALS passes base = V^T V (+ lambda I) to csrk_als_rows[_cg]; this entry
 * computes it on the device in a stated order, like every other number of the ALS path.  All arithmetic is float64;
 * fma(a, b, c) is round(a b + c), one rounding.
 *
 * P. V is n rows of k elements, float32 or float64 by panel_type, row j at V + j * ldv (ldv >= k in elements); out is
 *    k x k float64, packed row-major.
 *   P1. Operands.  v_j[t] is element t of row j, float32 widened exactly to float64.  ridge is one double, not NaN.
 *   P2. Chunks.  The rows are cut into consecutive chunks of R rows, chunk c = rows [c R, min((c + 1) R, n)); the last may
 *       be shorter.  R is a constant of the build (csrk_panel_gram_limits' out[1]), never a function of the device, its
 *       compute units or the launch.  For chunk c and every t >= u: S_c[t][u] starts at +0.0 and takes one step per row of
 *       the chunk, j ascending: S_c[t][u] = fma(v_j[t], v_j[u], S_c[t][u]).
 *   P3. Tree.  The chunk partials S_0, S_1, ... are combined level by level: within a level the adjacent pairs (2 m, 2 m + 1)
 *       are added, every addition rounded on its own, and an unpaired last partial is carried unchanged to the next level;
 *       this repeats until one partial is left, the sum.  n = 0 (no chunk): the sum is +0.0.
 *   P4. Output.  out[t][t] = round(sum[t][t] + ridge), the addition always made (ridge = 0.0 leaves a -0.0 sum as +0.0);
 *       for t > u, out[t][u] = sum[t][u] and out[u][t] = out[t][u]: the result is exactly symmetric.  n = 0 gives ridge I.
 *   P5. The result depends only on V's values, n, k, the panel type and ridge: not on ldv, the alignment, the load form,
 *       the stream, the launch geometry or repeated calls.  Parallelism is over chunks and over (t, u), never inside a
 *       chain; no float atomics.  NaN and Inf follow IEEE arithmetic (a created NaN has its position specified, not its
 *       sign or payload).
 *   P6. CSRK_ERR_INVALID: n < 0, k < 1, ldv < k, an unknown panel_type, a NaN ridge, a NULL out, a NULL V when n > 0, a V,
 *       out or workspace that is not aligned to its element size (8 bytes for the workspace), a workspace that is NULL or
 *       smaller than csrk_panel_gram_workspace asks for.  CSRK_ERR_UNSUPPORTED: k above csrk_panel_gram_limits' out[0] (at
 *       least 128).  CSRK_ERR_OVERFLOW: n above 2^40.  A refused call writes nothing.  The device form allocates nothing
 *       and never synchronises the host; its launches go on `stream` in order, and the workspace's contents afterwards
 *       are unspecified.
 *   Limits (csrk_panel_gram_limits): out[0] = the largest k; [1] = R;  n <= 2.  No device is touched.
 * Host form: host pointers in and out (the panel crosses packed; synchronous). */
CSRK_API int csrk_panel_gram(int64_t n, int32_t k, const void *V, int64_t ldv, int panel_type, double ridge, double *out);
/* Device form: every pointer in HBM, launched on `stream` (NULL = the default stream).  d_work: work_bytes bytes, at least
 * what csrk_panel_gram_workspace reports for (n, k) (0 for n = 0: d_work may then be NULL). */
CSRK_API int csrk_panel_gram_device(int64_t n, int32_t k, const void *d_V, int64_t ldv, int panel_type, double ridge,
                                    double *d_out, void *d_work, int64_t work_bytes, void *stream);
CSRK_API int csrk_panel_gram_workspace(int64_t n, int32_t k, int64_t *bytes);
CSRK_API int csrk_panel_gram_limits(int64_t *out, int n);

/* ---- the ALS objective: what a half-step minimises, per row and in total ---------------------------------
 * Not reference entry points.  For a side with matrix A, row factors U [nrows x k] and column factors V [ncols x k], both
 * float64, the quadratic form that csrk_als_rows and csrk_als_rows_cg minimise over U with V fixed.  J is the usual loss
 * MINUS A CONSTANT that does not depend on the factors, so differences of J are differences of the loss:
 *     explicit ALS (scale = 0, rhs = values, implicit = 0):
 *         sum_e (a_e - u_i . v_j)^2 + regulariser                                          = J + sum_e a_e^2
 *     Hu-Koren implicit ALS (scale = 1, rhs = one_plus_values, implicit = 1, values = confidence - 1):
 *         sum_e (1 + a_e) (1 - u_i . v_j)^2 + sum over pairs not stored (u_i . v_j)^2 + regulariser = J + sum_e (1 + a_e)
 *     regulariser = sum_i rho_i |u_i|^2 + sum_j rho'_j |v_j|^2 with the rhos of J1 over A's and A^T's rows.
 * All arithmetic is float64; fma(a, b, c) is round(a b + c), one rounding.
 *
 * J. For row i of [row_begin, row_end), its entries e = (i, j_e) in storage order, n_i of them, u_i = row i of U,
 *    v_e = row j_e of V:
 *   J1. Per row.  w_e and c_e are exactly csrk_als_rows' (rule 1 of csrk_gram_rows and rule A3, chosen by scale and
 *       rhs_mode); rho_i = fma(lam_n, (double)n_i, lam).  J_i starts at +0.0 and takes one step per entry, in storage order:
 *           s_e = DOT(u_i, v_e)               rule C2's order for float64 panels
 *           g_e = round(w_e s_e) under scale = 1, else s_e
 *           h_e = round(g_e - 2 c_e)          (2 c_e is exact)
 *           J_i = fma(h_e, s_e, J_i)
 *       and after the entries J_i = fma(rho_i, DOT(u_i, u_i), J_i).  data = 0 skips the entry loop: only n_i and u_i matter
 *       (V, the columns and the values are not read), which gives the other side's regulariser from A^T's row lengths.
 *       csrk_als_objective_rows writes out[i - row_begin] = J_i, float64.
 *   T.  The fixed-order sum of a float64 array x[0 .. n): x is cut into consecutive chunks of L elements (L a constant of
 *       the build, csrk_als_objective_limits' out[1]; the last chunk may be shorter); each chunk is added serially,
 *       ascending, from +0.0, every addition rounded; the chunk partials are combined by rule P3's tree.  n = 0: +0.0.
 *   J2. Total.  objective = round(round(T(J over all rows of A with U, V) + T(J with data = 0 over all rows of A^T with V
 *       in U's place)) + F).  F is +0.0 unless implicit = 1; then F = T of the k k numbers round(G_U[t][u] G_V[t][u]) in
 *       row-major order, G_U and G_V rule P's Gram matrices of U and V with ridge 0.0: sum_i u_i^T (V^T V) u_i =
 *       <U^T U, V^T V>, the all-pairs term of implicit ALS without a visit to all pairs.
 *   J3. A row's J_i depends only on its entries, u_i, the V rows they name, k, scale, rhs_mode, data, lam and lam_n; the
 *       objective only on those of all rows, on the row lengths of A^T and on implicit: not on the row range, the pointer
 *       width, ldu, ldv, the alignment, the load form, the stream, the launch geometry or repeated calls.  Parallelism is
 *       over rows, chunks and elements, never inside a chain; no float atomics.  Unsorted and repeated columns are just
 *       more entries.  NaN and Inf follow IEEE arithmetic (a created NaN has its position specified, not its sign or
 *       payload).
 *   J4. csrk_als_objective takes A and a second handle for A^T and requires it to be ncols x nrows with A's entry count:
 *       anything else is CSRK_ERR_INVALID.  It does NOT verify that the second matrix is the transpose; only its row
 *       lengths are read.
 *   J5. CSRK_ERR_INVALID: k < 1, ldu < k or ldv < k, scale, data or implicit outside {0, 1}, an unknown rhs_mode, a bad row
 *       range, a NULL or misaligned U, V (when read) or output, a workspace that is NULL, misaligned or smaller than
 *       csrk_als_objective_workspace asks for.  CSRK_ERR_UNSUPPORTED: k above csrk_als_objective_limits' out[0] (at least
 *       128).  What the scalars alone decide is refused before a handle is looked at.  row_begin == row_end: CSRK_OK,
 *       nothing launched.  A refused call writes nothing.  The device forms allocate nothing and never synchronise the
 *       host; the handles are not modified and keep their plans.
 *   Limits (csrk_als_objective_limits): out[0] = the largest k; [1] = L; [2] = the lanes of a row's team; [3] = the
 *   entries a team has in flight per step;  n <= 4.  No device is touched.
 * Host forms: host pointers in and out (panels cross packed; synchronous).  U has the matrix's nrows rows whatever the
 * row range: row i reads U + i * ldu. */
CSRK_API int csrk_als_objective_rows(csrk_handle_t h, int32_t row_begin, int32_t row_end, const double *U, int64_t ldu,
                                     const double *V, int64_t ldv, int32_t k, int scale, int rhs_mode, int data, double lam,
                                     double lam_n, double *out);
CSRK_API int csrk_als_objective(csrk_handle_t hA, csrk_handle_t hAt, const double *U, int64_t ldu, const double *V,
                                int64_t ldv, int32_t k, int scale, int rhs_mode, int implicit, double lam, double lam_n,
                                double *objective);
/* Device forms: every pointer in HBM, launched on `stream` (NULL = the default stream).  d_work: work_bytes bytes, at least
 * what csrk_als_objective_workspace reports; its contents afterwards are unspecified. */
CSRK_API int csrk_als_objective_rows_device(csrk_handle_t h, int32_t row_begin, int32_t row_end, const double *d_U,
                                            int64_t ldu, const double *d_V, int64_t ldv, int32_t k, int scale,
                                            int rhs_mode, int data, double lam, double lam_n, double *d_out, void *stream);
CSRK_API int csrk_als_objective_device(csrk_handle_t hA, csrk_handle_t hAt, const double *d_U, int64_t ldu,
                                       const double *d_V, int64_t ldv, int32_t k, int scale, int rhs_mode, int implicit,
                                       double lam, double lam_n, double *d_objective, void *d_work, int64_t work_bytes,
                                       void *stream);
CSRK_API int csrk_als_objective_workspace(int32_t nrows, int32_t ncols, int32_t k, int implicit, int64_t *bytes);
CSRK_API int csrk_als_objective_limits(int64_t *out, int n);

/* ---- als_fit: ALS sweeps with both factor panels on the device ---------------------------------------------
 * Not a reference entry point.  A composition: rule F defines the result as the public entries above called in a fixed
 * order, so the fit equals a caller's own loop over them bit for bit -- without the factors crossing to the host between
 * half-steps.
 *
 * F. hA is A (nrows x ncols), hAt its transpose (with values); U [nrows x k] and V [ncols x k] are float64, in: the start,
 *    out: the result.
 *   F1. The sequence.
 *           objective[0] = csrk_als_objective(hA, hAt, U, V)                               (when objective is not NULL)
 *           for s = 0 .. sweeps-1:
 *               B = base_for(V);  U = half(hA,  V, B, start U)     -> bad[2 s]
 *               B = base_for(U);  V = half(hAt, U, B, start V)     -> bad[2 s + 1]
 *               objective[s + 1] = csrk_als_objective(hA, hAt, U, V)
 *       scale, rhs_mode, implicit, lam and lam_n go to every part as given.
 *   F2. base_for(P).  solver cg: csrk_panel_gram(P, ridge 0.0) with implicit = 1, else NULL.  solver exact:
 *       csrk_panel_gram(P, ridge lam) with implicit = 1; else NULL when lam == 0, and otherwise csrk_panel_gram over 0 rows
 *       with ridge lam, which is lam I (rule P4).
 *   F3. half.  solver cg: csrk_als_rows_cg over all rows, float64 panel, lam and lam_n as given, steps = cg_steps, tol2,
 *       x0 = the side's current factors written in place (rule C7), resid and taken NULL; its bad count is 0.  solver
 *       exact: csrk_als_rows over all rows with lam_n (lam is in the base); bad is the number of rows whose info is not 0.
 *       The fit does not stop on bad rows (the device form cannot know): it returns CSRK_OK with bad filled, and the rows'
 *       Inf or NaN factors go into the next half-step as rule A5 and IEEE arithmetic have them.
 *   F4. Nothing else influences a bit: U, V, objective and bad depend only on the two matrices, the start factors and the
 *       scalar arguments.  sweeps = 0 is valid: the factors are unchanged and only objective[0] is written.
 *   F5. CSRK_ERR_INVALID: every refusal of the parts (rules P6, A7, C9, J5), sweeps < 0, a solver outside {0, 1}, an hAt
 *       that is not ncols x nrows with A's entry count, any overlap of U, V and the workspace, a workspace that is NULL,
 *       not 16-B aligned or smaller than csrk_als_fit_workspace asks for.  CSRK_ERR_UNSUPPORTED: k above 128.  All of it
 *       is refused before the first launch: a refused call writes nothing.  The device form issues every launch on
 *       `stream`, in order, allocates nothing and never synchronises the host.
 * solver: 0 exact, 1 cg.  objective: float64[sweeps + 1] or NULL; bad: int64[2 sweeps] or NULL. */
CSRK_API int csrk_als_fit(csrk_handle_t hA, csrk_handle_t hAt, int32_t k, int32_t sweeps, int solver, int32_t cg_steps,
                          double tol2, int scale, int rhs_mode, int implicit, double lam, double lam_n, double *U,
                          int64_t ldu, double *V, int64_t ldv, double *objective, int64_t *bad);
/* Device form: every pointer in HBM.  with_objective: 1 when d_objective is not NULL. */
CSRK_API int csrk_als_fit_device(csrk_handle_t hA, csrk_handle_t hAt, int32_t k, int32_t sweeps, int solver,
                                 int32_t cg_steps, double tol2, int scale, int rhs_mode, int implicit, double lam,
                                 double lam_n, double *d_U, int64_t ldu, double *d_V, int64_t ldv, double *d_objective,
                                 int64_t *d_bad, void *d_work, int64_t work_bytes, void *stream);
CSRK_API int csrk_als_fit_workspace(int32_t nrows, int32_t ncols, int32_t k, int solver, int implicit, int with_objective,
                                    int64_t *bytes);

/* ---- transpose ------------------------------------------------------------------------
 * csr/structure.py:172-247 (_transpose_values / _transpose_structure / transpose).
 * Bit-exact with the reference's stable counting sort: output rowptrs keep the input
 * pointer width, output colinds are the source row ids in ascending source position,
 * output values are float64 whatever the input dtype (:177).  with_values == 0, or a
 * structure-only input, gives a structure-only result (:241-242).                      */
CSRK_API int csrk_transpose(csrk_handle_t h, int with_values, csrk_handle_t *out);

/* ---- COO ingest -----------------------------------------------------------------------------
 * csr/structure.py:11-67 (_from_coo_structure / _from_coo_values / from_coo), the ingest behind
 * CSR.from_coo (csr/csr.py:138-169).  Host COO arrays -> a NEW device handle.  Entries of a row
 * keep their input order (the reference's stable counting sort); values keep their dtype; row
 * pointers are int32 unless nnz > INT32_MAX.  rows[] must lie in [0, nrows), cols[] in [0, ncols). */
CSRK_API int csrk_from_coo(int32_t nrows, int32_t ncols, int64_t nnz, const int32_t *rows,
                           const int32_t *cols, const void *values, int val_type, csrk_handle_t *out);

/* ---- row extents / counts ---------------------------------------------------------------
 * csr/_rows.py:9-13 (extent), csr/csr.py:432-441 (row_nnzs = diff(rowptrs)).
 * `out` has nrows entries of the handle's pointer width (int32 or int64).              */
CSRK_API int csrk_row_nnzs(csrk_handle_t h, void *out);
CSRK_API int csrk_row_extent(csrk_handle_t h, int32_t row, int64_t *start, int64_t *end);

/* ---- row normalisation (IN PLACE on the handle's values) --------------------------------
 * csr/transform.py:29-66 (unit_rows) and :13-26 (center_rows).  `out` receives nrows
 * norms / means in the VALUES' dtype (float32 or float64), host memory.  Requires values. */
CSRK_API int csrk_unit_rows(csrk_handle_t h, void *norms);
CSRK_API int csrk_center_rows(csrk_handle_t h, void *means);
/* The same with the norms / means left in DEVICE memory (nrows entries of the values' dtype): the caller copies them out
 * when and how it likes (a pinned buffer, another stream) -- 80 MB for 10^7 rows is 3 ms of pageable copy otherwise. */
CSRK_API int csrk_unit_rows_device(csrk_handle_t h, void *d_norms);
CSRK_API int csrk_center_rows_device(csrk_handle_t h, void *d_means);

/* ---- order_columns (IN PLACE) -------------------------------------------------------------
 * csr/kernels/numba/__init__.py:47-52 -> csr/structure.py:156-169; lk_mkl_sporder.
 * Stable sort of every row by column index; values follow.                              */
CSRK_API int csrk_order_columns(csrk_handle_t h);

/* ---- pick_rows ---------------------------------------------------------------------------
 * csr/csr.py:347-364 -> csr/structure.py:84-149 (_pick_rows, _pick_rows_nvs).  NEW handle with the
 * rows rows[0..n_rows) of h, in that order (a row may appear more than once); `rows` is a host
 * array.  with_values = 0 drops the values; otherwise they keep their dtype.  Row pointers are
 * int32 (as the reference's) unless the result has more than 2^31 - 1 entries.  An index outside
 * [0, nrows) is CSRK_ERR_INVALID (the reference raises IndexError).                        */
CSRK_API int csrk_pick_rows(csrk_handle_t h, const int32_t *rows, int64_t n_rows, int with_values,
                            csrk_handle_t *out);

/* ---- _filter_zeros ----------------------------------------------------------------------
 * csr/_struct.py:61-76.  Returns a NEW handle without the entries whose value is
 * exactly 0.0 (NaN is kept).  Requires float64 values.                                  */
CSRK_API int csrk_filter_zeros(csrk_handle_t h, csrk_handle_t *out);

/* ---- row top-k: keep each row's k largest entries ------------------------------------------
 * Not a reference entry point: the step a caller of mult_abt (item-kNN: each row's N most similar neighbours above a
 * minimum similarity) or of SDDMM (each user's N best candidates) takes next, on the device, so that only the kept entries
 * cross PCIe.  Returns a NEW handle of h's shape whose row i holds the kept entries of row i of h:
 *   1. An entry PASSES unless value < min_value: NaN passes, -0.0 passes min_value = 0.0; min_value = -INFINITY is no
 *      threshold.
 *   2. Of a row's passing entries the first k in this total order are kept: larger value first; NaN (any sign, any
 *      payload) ranks above +Inf and all NaNs tie; -0.0 and +0.0 tie; ties go to the entry stored earlier in the row
 *      (the order torch.topk / a reversed np.sort give to values, made a function of the input by the tie rule).  A row
 *      with fewer than k passing entries keeps them all.
 *   3. order = CSRK_TOPK_BY_VALUE: the kept entries are written in that rank order, best first.  order = CSRK_TOPK_STORAGE:
 *      the same entries in the order they had in the input row (a column-sorted matrix stays column-sorted).
 *   4. Column indices and values are copied bit for bit (NaN payloads, -0.0, float32 subnormals); values keep their dtype.
 *      Unsorted and repeated columns are just more entries.
 *   5. Row pointers are int32 unless the result holds more than 2^31 - 1 entries, whatever the input's pointer width (the
 *      layout rule of csr/csr.py:88-93, as csrk_pick_rows).
 *   6. h is not modified and keeps its plans.  CSRK_ERR_INVALID for k < 1, a NaN min_value, an unknown order, or a
 *      structure-only h (no values to rank: the refusal of csrk_unit_rows).  nrows = 0 or nnz = 0: CSRK_OK, an empty result,
 *      nothing launched.  k may exceed every row length (then only rule 1 filters, and `order` still applies).
 *   7. The result depends on (h, k, min_value, order) only: not on launch geometry, repeated calls, the pointer width or what
 *      else the matrix holds (csrc/topk.hip: ranks and slots are counted, never appended in arrival order).
 * A row of more than 2^31 - 1 entries is CSRK_ERR_UNSUPPORTED. */
enum { CSRK_TOPK_BY_VALUE = 0, CSRK_TOPK_STORAGE = 1 };
CSRK_API int csrk_topk_rows(csrk_handle_t h, int64_t k, double min_value, int order, csrk_handle_t *out);
/* Diagnostics: the row classes of csrk_topk_rows: out[0] = the longest row one wavefront ranks, [1] = the candidates /
 * winners a large-class workgroup holds in LDS (more winners than that in by-value order are ordered in device memory),
 * [2] = its threads, [3] = the longest row of the medium class (a smaller workgroup, the whole row in LDS);  n <= 4.
 * No device is touched. */
CSRK_API int csrk_topk_limits(int64_t *out, int n);

/* ---- combine: two matrices entry by entry -> a new one -------------------------------------------
 * Not a reference entry point: what a caller does between the kernels above -- drop the (user, item) pairs already seen
 * from a product before csrk_topk_rows, a residual or a blend of two matrices (alpha A + beta B), a weighting (A o B),
 * A + A^T.  Returns a NEW handle of A's shape.  CANONICAL below means: every row strictly ascending in column (sorted,
 * no column twice); csrk_order_columns sorts.
 *   1. A and B have the same nrows and ncols.  a == b is allowed.  Neither is modified; both keep their plans.  The
 *      operands may differ in pointer width and in value type.
 *   2. op = CSRK_COMBINE_ADD (the union of the patterns; A and B canonical): rows strictly ascending, float64 values --
 *      an entry of both round(round(alpha a) + round(beta b)), of A alone round(alpha a), of B alone round(beta b).  Each
 *      multiply and the add is rounded on its own (no fused multiply-add); float32 values are widened exactly first; a
 *      structure-only operand counts as 1.0 everywhere (csrk_sddmm's rule).  alpha and beta get no special cases: an
 *      exact-zero result stays stored (csrk_filter_zeros removes it), NaN and Inf behave as IEEE says (0 * Inf is NaN).
 *   3. op = CSRK_COMBINE_MUL (the intersection; A and B canonical; alpha, beta ignored): the columns both rows hold,
 *      ascending, float64 round(a b), operands widened as in 2.
 *   4. op = CSRK_COMBINE_KEEP / CSRK_COMBINE_DROP (a mask; only B canonical; alpha, beta ignored): the entries of A whose
 *      column is (KEEP) / is not (DROP) stored in the same row of B, in A's storage order -- A may be unsorted and may
 *      repeat columns (a product in the reference's column order is).  Column indices and values are copied bit for bit
 *      in A's value type (NaN payloads, -0.0, float32 subnormals); a structure-only A gives a structure-only result.
 *      B's values are never read.
 *   5. Row pointers are int32 unless the result holds more than 2^31 - 1 entries, whatever the inputs' widths (the rule
 *      of csrk_pick_rows).
 *   6. CSRK_ERR_INVALID: a NULL out, an unknown op, different shapes, or an operand that has to be canonical and is not
 *      (the message names the operand and the first such row).  The rows are looked at on the device, once per handle:
 *      the answer is remembered and dropped by whatever rewrites the handle's columns (csrk_order_columns).
 *      CSRK_ERR_UNSUPPORTED: a row of more than 2^31 - 1 entries.  nrows = 0, or both operands without entries: CSRK_OK,
 *      an empty result, nothing launched.
 *   7. The result depends on (A, B, op, alpha, beta) only: not on launch geometry, the pointer widths or repeated calls
 *      (csrc/combine.hip: every slot is counted, never appended in arrival order; no float atomics).  A NaN the
 *      arithmetic of ADD / MUL creates or passes on has no specified sign or payload, only its position.
 * Column indices are compared and copied, never used as addresses. */
enum { CSRK_COMBINE_ADD = 0, CSRK_COMBINE_MUL = 1, CSRK_COMBINE_KEEP = 2, CSRK_COMBINE_DROP = 3 };
CSRK_API int csrk_combine(csrk_handle_t a, csrk_handle_t b, int op, double alpha, double beta, csrk_handle_t *out);
/* Diagnostics: the row classes of csrk_combine, ascending: out[0] = the entries of a row one wavefront takes per step,
 * [1] = the entries a workgroup takes per step (its threads), [2] = the largest len_a + len_b of the wavefront class (longer
 * rows get a workgroup each);  n <= 3.  No device is touched. */
CSRK_API int csrk_combine_limits(int64_t *out, int n);

/* ---- coalesce: the canonical form of any matrix --------------------------------------------------
 * Not a reference entry point: what csrk_combine asks of its operands and nothing above supplies.  csrk_from_coo keeps every
 * repeated (row, column) pair (a re-rated item in a ratings log) and csrk_order_columns only sorts; csrk_coalesce merges.
 *   1. The result is a NEW handle of h's shape: every row strictly ascending in column, one entry per distinct
 *      (row, column) that h stores.  h is not modified and keeps its plans.  The result is known to be canonical: a
 *      following csrk_combine or csrk_is_canonical does not look at its rows again.
 *   2. A GROUP is the set of entries of one row with one column; its members v0 .. v(m-1) are taken in h's storage order,
 *      earlier in the row first.  A group never crosses a row boundary: the last entry of row r and the first of the next
 *      non-empty row stay two entries when their columns agree.  `dup` says what a group becomes:
 *        CSRK_DUP_SUM    ((v0 + v1) + v2) + ..., left to right, every add rounded in the values' dtype (float32 values: float32
 *                        adds).  The sum does not start at +0.0: a group of one is copied bit for bit and -0.0 + -0.0 stays
 *                        -0.0.  An exact-zero sum stays stored (csrk_filter_zeros removes it).  A NaN that an add creates or
 *                        passes on has its position specified, not its sign or payload (csrk_combine's rule 7).
 *        CSRK_DUP_FIRST  v0, copied bit for bit.       CSRK_DUP_LAST  v(m-1), copied bit for bit.
 *        CSRK_DUP_MAX / CSRK_DUP_MIN   the first / the last member in the total order of csrk_topk_rows (rule 2): larger
 *                        first, NaN above +Inf and all NaNs tied, -0.0 and +0.0 tied, tied members in storage order.  So MAX
 *                        takes the EARLIEST stored of the largest members and MIN the LATEST stored of the smallest; MIN is
 *                        a NaN only when every member is one.  The value is copied bit for bit.
 *      Bit for bit holds for -0.0, subnormals and quiet-NaN payloads in both dtypes; a signalling float32 NaN may come back
 *      quieted when the entries had to be sorted (as from csrk_order_columns).  Values keep their dtype; a structure-only h
 *      gives a structure-only result (dup must still be valid).
 *   3. Row pointers are int32 unless the result holds more than 2^31 - 1 entries, whatever h's width (csrk_pick_rows' rule).
 *   4. Three routes, the same arrays from each for the same matrix (csrk_coalesce_last_route):
 *        0  h is canonical: the result is a device copy.
 *        1  h's rows are non-descending in column, only repeats are present: the groups are merged without any sort.
 *        2  the entries are sorted by column within rows, stably, then merged.
 *      Which one applies is found by one look at the rows on the device, remembered by the handle like csrk_combine's.
 *   5. The result depends on (h, dup) only: not on launch geometry, the pointer width or repeated calls (csrc/coalesce.hip:
 *      every slot is counted, a group is folded by one thread in storage order; no float atomics, nothing appended in
 *      arrival order).
 *   6. CSRK_ERR_INVALID: a NULL out, an unknown dup, a bad handle; *out is 0 on any failure.  nrows = 0 or nnz = 0: CSRK_OK,
 *      an empty result, nothing launched.
 * Column indices are compared and copied, never used as addresses. */
enum { CSRK_DUP_SUM = 0, CSRK_DUP_FIRST = 1, CSRK_DUP_LAST = 2, CSRK_DUP_MAX = 3, CSRK_DUP_MIN = 4 };
CSRK_API int csrk_coalesce(csrk_handle_t h, int dup, csrk_handle_t *out);
/* The route the calling thread's last csrk_coalesce took: 0 copied, 1 merged without sorting, 2 sorted and merged; 0 after
 * a failed call.  No device is touched. */
CSRK_API int csrk_coalesce_last_route(int *route);
/* Is every row of h strictly ascending in column?  *canonical = 1 or 0; *first_bad_row (may be NULL) = the first row that
 * is not, -1 when canonical.  The rows are looked at on the device once per handle: the answer is remembered (it is the one
 * csrk_combine and csrk_coalesce use) and dropped by whatever rewrites the handle's columns (csrk_order_columns). */
CSRK_API int csrk_is_canonical(csrk_handle_t h, int *canonical, int32_t *first_bad_row);

/* ---- topk_scores: each row's n_top best unseen items from the factors U and V ----------------------
 * Not a reference entry point: from trained factors to recommendations (csrk_als_rows trains, csrk_sddmm gives loss and
 * residuals, csrk_rank_entries below evaluates): for every row of a range, score ALL items as U[i] . V[j], leave out the (row, item) pairs `seen` stores and the scores
 * below a threshold, keep the n_top best.  The rows x n_items block of scores is never stored.
 *   1. Operands.  U is dense row-major, indexed by the ABSOLUTE row i of [row_begin, row_end): U[i][t] at U + i * ldu + t.
 *      V is dense row-major [n_items x k].  Both are float32 or both float64 (panel_type = CSRK_VAL_F32 / CSRK_VAL_F64);
 *      ldu, ldv >= k in elements.  `seen` is 0 (nothing is excluded) or a handle; with a handle n_items must equal its
 *      ncols and row_end <= its nrows, and it must be canonical (every row strictly ascending in column): the check is
 *      csrk_is_canonical's remembered one, and the refusal names the first bad row as csrk_combine's does.  Its values are
 *      never read (a structure-only handle will do), either pointer width is taken, and its column indices are compared,
 *      never used as addresses.  `seen` is not modified and keeps its plans.
 *   2. Score.  For row i and item j:   s = +0.0;  for t = 0 .. k-1 ascending:  s = fma(U[i][t], V[j][t], s)
 *      -- one serial chain of fused multiply-adds in float64, float32 elements widened exactly first.  Parallelism is over
 *      (row, item) pairs, never inside a chain: no split sums, no float atomics, no matrix instructions.
 *   3. Candidates.  Item j is a candidate of row i unless `seen` stores (i, j) or s < min_score is true: NaN passes, and
 *      min_score = -INFINITY is no threshold (csrk_topk_rows' rule 1).
 *   4. Selection.  Of a row's candidates the first n_top in the total order of csrk_topk_rows (its rule 2) are kept, best
 *      first: larger score first; any NaN above +Inf and all NaNs tied; -0.0 ties +0.0; TIES GO TO THE SMALLER ITEM INDEX.
 *      Items are distinct, so the order is strict and the result unique.
 *   5. Output.  counts[i - row_begin] = the number kept; for r < that, items[(i - row_begin) * ldi + r] is the item index
 *      and scores[(i - row_begin) * lds + r] the chain's bits unchanged (-0.0 stays -0.0); for count <= r < n_top the
 *      padding is item -1 and score -INFINITY.  ldi, lds >= n_top in elements; columns at or beyond n_top are not touched.
 *      counts may be NULL.
 *   6. Invariance.  An output depends only on U's row i, V, row i of `seen`, k, the panel type, n_top and min_score: not on
 *      the row range asked for, the strides, the alignment, the pointer width, the stream, the launch geometry or repeated
 *      calls.  U and V are read in 16-B pieces when both pointers, both strides and k allow it, else by element: the same
 *      bits either way.
 *   7. Special values.  IEEE throughout; no path skips a zero.  A NaN or Inf in U's row i reaches row i only.  A NaN in V's
 *      row j reaches every row for which j is not seen, and no other output bit.  A NaN that the chain creates (Inf - Inf,
 *      0 * Inf) has its position specified, not its sign or payload.
 *   8. Device form.  Allocates nothing and does not synchronise the host, with one exception: the first call that asks a
 *      handle whether it is canonical looks at its rows (rule 1; csrk_is_canonical beforehand takes that look).  One
 *      workgroup takes a block of rows across all items and keeps the rows' running lists on the chip: no scratch memory.
 *      The items of a small row range are not split across workgroups (csrk_topk_scores_for splits them).  The host form
 *      sends the panels packed (the rows of the range only) and is synchronous.
 *   9. Refusals; a refused call writes nothing.  CSRK_ERR_INVALID: k < 1, n_top < 1, n_items < 0; ldu < k, ldv < k,
 *      ldi < n_top, lds < n_top; an unknown panel_type; a NaN min_score; row_begin < 0 or row_begin > row_end; with a handle,
 *      row_end > nrows or n_items != ncols; a `seen` that is not canonical or not a handle; NULL items or scores when there
 *      are rows; a NULL U when there are rows; a NULL V when there are rows and items; a pointer not aligned to its
 *      element.  CSRK_ERR_UNSUPPORTED: k above out[0] of csrk_topk_scores_limits (at least 256), n_top above out[1] (at
 *      least 128).  row_begin == row_end: CSRK_OK, nothing launched.  n_items == 0: CSRK_OK, counts 0 and padding only.
 *      n_top may exceed n_items.
 *  10. Limits (csrk_topk_scores_limits): out[0] = the largest k; [1] = the largest n_top; [2] = the rows of a workgroup;
 *      [3] = the items of a tile; [4] = the factors staged through LDS per chunk (a chain crosses chunks in order); [5] = the
 *      entries a row's running list holds between compactions when n_top <= 32 (n_top + 16 above that);  n <= 6.  By rule
 *      6 none of them changes a bit. */
CSRK_API int csrk_topk_scores(csrk_handle_t seen, int32_t row_begin, int32_t row_end, const void *U, int64_t ldu,
                              const void *V, int64_t ldv, int32_t n_items, int32_t k, int panel_type, int32_t n_top,
                              double min_score, int32_t *items, int64_t ldi, double *scores, int64_t lds, int32_t *counts);
/* Device form: every pointer in HBM, launched on `stream` (NULL = the default stream). */
CSRK_API int csrk_topk_scores_device(csrk_handle_t seen, int32_t row_begin, int32_t row_end, const void *d_U, int64_t ldu,
                                     const void *d_V, int64_t ldv, int32_t n_items, int32_t k, int panel_type,
                                     int32_t n_top, double min_score, int32_t *d_items, int64_t ldi, double *d_scores,
                                     int64_t lds, int32_t *d_counts, void *stream);
/* Diagnostics: the six limits of rule 10, in its order;  n <= 6.  No device is touched. */
CSRK_API int csrk_topk_scores_limits(int64_t *out, int n);

/* ---- topk_scores_for: csrk_topk_scores for a list of rows, the items split across workgroups ------
 * Not a reference entry point: serving.  A request is a list of user ids, and a handful of rows does not fill the card when
 * one workgroup takes 64 rows across all items: here the rows are named one by one and the items are cut into S ranges that
 * run side by side, with the partial lists in a workspace the caller supplies.  Everything not said here is
 * csrk_topk_scores' rule of the same number.
 *   1. Rows.  rows[r] (int32, n_rows of them) is an ABSOLUTE row index and output row r belongs to it: U[rows[r]] is the
 *      factor row, row rows[r] of `seen` the exclusion list.  The list may be in any order and may repeat a row; each
 *      occurrence is computed on its own and gets the same bits.  u_rows is the number of rows U holds; with a handle it
 *      must equal the handle's nrows.  In the device form an index outside [0, u_rows) is not dereferenced: that output row
 *      gets count -1 and padding only, and no other row is affected (csrk_rank_entries' rule for a bad column).  The host
 *      form looks at the list first and refuses with CSRK_ERR_INVALID, naming the first bad position and its value; it
 *      sends only the listed rows of U.
 *   2. Score, candidates, selection, output and special values are rules 2-5 and 7 of csrk_topk_scores, word for word
 *      (output row r where it says i - row_begin).  For rows = b, b + 1, ..., e - 1 every output bit equals that of
 *      csrk_topk_scores(row_begin = b, row_end = e).
 *   3. Splits.  With tile = out[3] of csrk_topk_scores_limits and T = ceil(n_items / tile), the items are cut at tile
 *      boundaries into S contiguous ranges: range s holds the tiles [s T / S, (s + 1) T / S) (integer division).  One
 *      workgroup takes one (row block, range) pair, keeps its rows' running lists on the chip exactly as csrk_topk_scores
 *      does, and writes each row's final partial list (the count, then score bits and items, best first) to the workspace.
 *      A second launch merges the S partial lists of each row: a candidate's place is its place in its own list plus the
 *      number of entries of every other list that come before it in rule 4's order.  Places are counted, never handed out
 *      in arrival order; places below n_top are written, the rest is padding.  No float atomics, no device-scope atomics,
 *      and no workgroup waits for another: two launches, not a last-block-finishes scheme; neither launch can spin.  S = 1
 *      writes the outputs directly, needs no workspace and launches once.
 *   4. Choice of S.  splits >= 1 forces S = min(splits, T, S_max), and S = 1 when T = 0 or n_rows = 0.  splits = 0 is automatic:
 *      S = clamp(ceil(W / ceil(n_rows / 64)), 1, min(T, S_max)), with W the workgroups that fill the card: 512 for
 *      n_top <= 32 (two workgroups per CU for that list class, 256 CUs), 256 above that (one per CU).  S_max = 64, which
 *      bounds the merge at 64 * 128 candidates per row.  csrk_topk_scores_for_workspace returns S and the bytes for it from
 *      these constants alone, so a caller can size a buffer once without a device:
 *      bytes = 0 for S = 1, else n_rows * S * (out[3] + (n_top - 1) * out[4]) of csrk_topk_scores_for_limits, rounded up to
 *      a multiple of 16.
 *   5. Workspace.  16-B aligned, work_bytes >= the reported size; nothing at or beyond the reported size is touched; d_work
 *      may be NULL when the size is 0.  Its contents before and after a call mean nothing.
 *   6. Invariance.  No output bit depends on splits, the workspace address, the order or repetition of rows, or anything in
 *      csrk_topk_scores' rule 6.
 *   7. Device form.  Allocates nothing and does not synchronise the host, apart from the remembered canonical look of
 *      csrk_topk_scores' rule 8; both launches go to `stream`.  The host form allocates its own workspace and is
 *      synchronous.
 *   8. Refusals; a refused call writes nothing.  Every refusal of csrk_topk_scores that applies, in the same order, with
 *      texts that begin "topk_scores_for: ".  CSRK_ERR_INVALID further: n_rows < 0; u_rows < 0; splits < 0; with a handle,
 *      u_rows != nrows or n_items != ncols; NULL rows when n_rows > 0; a workspace that is NULL, misaligned or too small when
 *      one is needed.  CSRK_ERR_UNSUPPORTED: k or n_top above csrk_topk_scores_limits, and more row blocks (of 64 rows) than
 *      a grid holds (2^31 - 1).  n_rows = 0: CSRK_OK, nothing launched.
 *   9. Limits (csrk_topk_scores_for_limits): out[0] = S_max; [1] = W for n_top <= 32; [2] = W above that; [3] = the
 *      workspace bytes per (row, split) at n_top = 1; [4] = the further bytes per unit of n_top;  n <= 5. */
CSRK_API int csrk_topk_scores_for(csrk_handle_t seen, const int32_t *rows, int64_t n_rows, int32_t u_rows, const void *U,
                                  int64_t ldu, const void *V, int64_t ldv, int32_t n_items, int32_t k, int panel_type,
                                  int32_t n_top, double min_score, int32_t *items, int64_t ldi, double *scores, int64_t lds,
                                  int32_t *counts, int32_t splits);
/* Device form: every pointer in HBM, launched on `stream` (NULL = the default stream). */
CSRK_API int csrk_topk_scores_for_device(csrk_handle_t seen, const int32_t *d_rows, int64_t n_rows, int32_t u_rows,
                                         const void *d_U, int64_t ldu, const void *d_V, int64_t ldv, int32_t n_items,
                                         int32_t k, int panel_type, int32_t n_top, double min_score, int32_t *d_items,
                                         int64_t ldi, double *d_scores, int64_t lds, int32_t *d_counts, int32_t splits,
                                         void *d_work, int64_t work_bytes, void *stream);
/* Rule 4: *splits_used = S and *bytes = the workspace for it.  CSRK_ERR_INVALID: n_rows < 0, n_items < 0, n_top < 1,
 * splits < 0, a NULL result pointer; CSRK_ERR_UNSUPPORTED as in rule 8.  No device is touched. */
CSRK_API int csrk_topk_scores_for_workspace(int64_t n_rows, int32_t n_items, int32_t n_top, int32_t splits,
                                            int32_t *splits_used, int64_t *bytes);
/* Diagnostics: the five limits of rule 9, in its order;  n <= 5.  No device is touched. */
CSRK_API int csrk_topk_scores_for_limits(int64_t *out, int n);

/* ---- rank_entries: where each held-out entry lands among its row's unseen items --------------------
 * Not a reference entry point: offline evaluation after csrk_topk_scores.  For every entry (i, j) of `test`, the number of
 * items that row i has not seen and that come before j in the row's full ranking by U[i] . V[c].  Hit rate, MRR and nDCG
 * at any cut-off, AUC and mean percentile rank follow from that number on the host; the rows x n_items block of scores is
 * never stored.
 *   1. Operands.  `test` is a handle; n_items is its ncols.  U and V are as in csrk_topk_scores' rule 1: U is indexed by the
 *      ABSOLUTE row i of [row_begin, row_end), V is [n_items x k], both float32 or both float64 (panel_type), ldu, ldv >= k
 *      in elements.  `seen` is 0 (nothing is excluded) or a handle with test's nrows and ncols; it must be canonical: the
 *      check is csrk_is_canonical's remembered one, and the refusal names the first bad row as csrk_topk_scores' does.
 *      `test` need not be canonical: unsorted and repeated columns are just more entries.  The values of neither are ever
 *      read (structure-only handles will do), either pointer width is taken for either, neither is modified and both keep
 *      their plans.  The columns of `test` and `seen` select rows of V, as csrk_sddmm's pattern does, and must lie in
 *      [0, n_items); one that does not is not dereferenced: as an entry of `test` it gets rank -1 and a NaN score, as an
 *      entry of `seen` it excludes nothing.
 *   2. Score.  csrk_topk_scores' rule 2:   s = +0.0;  for t = 0 .. k-1 ascending:  s = fma(U[i][t], V[j][t], s)
 *      -- one serial chain of fused multiply-adds in float64, float32 elements widened exactly first; no split sums, no float
 *      atomics, no matrix instructions.  The score of a pair has the bits csrk_topk_scores gives it.
 *   3. Rank.  For a test entry e = (i, j) with score s_e let C be the items c of [0, n_items), c != j, that `seen` does not
 *      store in row i.  rank_e = the number of c in C whose (s_c, c) comes before (s_e, j) in the total order of
 *      csrk_topk_scores' rule 4: larger score first; any NaN above +Inf and all NaNs tied; -0.0 ties +0.0; on equal keys the
 *      smaller item index first.  j itself is ranked whether or not `seen` stores (i, j); the other test entries of the row
 *      are ordinary competitors; an item repeated in a test row gets the same rank each time.  Row i has
 *      n_items - (the entries `seen` stores in row i) candidates, the held-out item included when `seen` does not store it.
 *   4. Output.  With base = test.rowptrs[row_begin], for every entry e of rows [row_begin, row_end) in test's storage order:
 *      ranks[e - base] = rank_e and, when scores is not NULL, scores[e - base] = the chain's bits unchanged (-0.0 stays
 *      -0.0).  Nothing else is written.
 *   5. Agreement with csrk_topk_scores.  With the same U, V and `seen`, min_score = -INFINITY and any n_top: a test entry
 *      that `seen` does not store and whose rank_e < n_top has items[i][rank_e] == j there, and scores[i][rank_e] has the
 *      bits of scores[e - base] here.
 *   6. Invariance.  An output depends only on U's row i, V, row i of `seen`, the entry's column, k and the panel type: not
 *      on the row range asked for, the strides, the alignment (16-B pieces or element loads: the same bits), the pointer
 *      widths, the other entries of `test` or their number, the stream, the launch geometry or repeated calls.
 *   7. Special values.  IEEE throughout; no path skips a zero.  A NaN that a chain creates has its position specified, not
 *      its sign or payload; every NaN has the same key, so the ranks are specified even then.
 *   8. Device form.  Allocates nothing and does not synchronise the host, with one exception: the first call that asks
 *      `seen` whether it is canonical looks at its rows (csrk_is_canonical beforehand takes that look).  A workgroup takes a
 *      block of rows across all items and holds up to out[4] test entries per row on the chip; rows with more are swept
 *      again, decided on the device: no scratch memory.  The items of a small row range are not split across workgroups
 *      (csrk_rank_entries_for splits them).
 *      The host form sends the panels packed (the rows of the range only) and is synchronous.
 *   9. Refusals; a refused call writes nothing.  The scalar arguments are looked at first and answered whatever the handles
 *      are: CSRK_ERR_INVALID for k < 1, ldu < k, ldv < k, an unknown panel_type, row_begin < 0 or row_begin > row_end;
 *      CSRK_ERR_UNSUPPORTED for k above out[0] of csrk_rank_entries_limits (at least 256).  Then CSRK_ERR_INVALID: a `test`
 *      or a non-zero `seen` that is not a handle; row_end > nrows; a `seen` of another shape than `test` or not canonical;
 *      when there is work, a NULL ranks, U or V or a pointer not aligned to its element.  row_begin == row_end, or a range
 *      without test entries: CSRK_OK, nothing launched (the device form, which does not read row pointers on the host,
 *      launches unless `test` is empty altogether; workgroups without test entries end at once).
 *  10. Limits (csrk_rank_entries_limits): out[0] = the largest k; [1] = the rows of a workgroup; [2] = the items of a tile;
 *      [3] = the factors staged through LDS per chunk; [4] = T, the test entries of a row held on the chip per sweep (a row
 *      with more is swept again per T of them, so any number works);  n <= 5.  By rule 6 none of them changes a bit. */
CSRK_API int csrk_rank_entries(csrk_handle_t seen, csrk_handle_t test, int32_t row_begin, int32_t row_end, const void *U,
                               int64_t ldu, const void *V, int64_t ldv, int32_t k, int panel_type, int32_t *ranks,
                               double *scores);
/* Device form: every pointer in HBM, launched on `stream` (NULL = the default stream). */
CSRK_API int csrk_rank_entries_device(csrk_handle_t seen, csrk_handle_t test, int32_t row_begin, int32_t row_end,
                                      const void *d_U, int64_t ldu, const void *d_V, int64_t ldv, int32_t k, int panel_type,
                                      int32_t *d_ranks, double *d_scores, void *stream);
/* Diagnostics: the five limits of rule 10, in its order;  n <= 5.  No device is touched. */
CSRK_API int csrk_rank_entries_limits(int64_t *out, int n);

/* ---- rank_entries_for: csrk_rank_entries for a list of rows, the items split across workgroups ------
 * Not a reference entry point: offline evaluation of a SAMPLE of users.  The rows with held-out entries are scattered over
 * the matrix, and a thousand of them do not fill the card when one workgroup takes 64 rows across all items: here the rows
 * are named one by one and the items are cut into S ranges that run side by side; the partial ranks are integers and add.
 * Everything not said here is csrk_rank_entries' rule of the same number; rules 11 and 12 are this entry's own.
 *   1. Rows.  rows[r] (int32, n_rows of them) is an ABSOLUTE row index: U[rows[r]] is the factor row, row rows[r] of `test`
 *      holds the entries ranked and row rows[r] of `seen` the exclusion list.  The list may be in any order and may repeat
 *      a row; each occurrence is computed on its own and gets its own output positions (rule 4).  u_rows is the number of
 *      rows U holds and must equal test's nrows.  In the device form an index outside [0, u_rows) is not dereferenced: that
 *      list position reads and writes nothing, and no neighbour is affected.  The host form looks at the list first and
 *      refuses with CSRK_ERR_INVALID, naming the first bad position and its value (as csrk_topk_scores_for does); it sends
 *      only the listed rows of U, packed in list order.  The bad-column part of csrk_rank_entries' rule 1 holds: a test
 *      column outside [0, n_items) gets rank -1 and a NaN score -- exactly -1, for any number of splits.
 *   2. Score, 3. Rank and 7. Special values are rules 2, 3 and 7 of csrk_rank_entries, word for word (i = rows[r]).  For
 *      rows = b, b + 1, ..., e - 1 every output bit equals that of csrk_rank_entries(row_begin = b, row_end = e).
 *   4. Output.  With len(r) = the entries `test` stores in row rows[r] and offsets[r] = len(0) + ... + len(r - 1): the x-th
 *      entry of that row, in test's storage order, goes to ranks[offsets[r] + x], and its score to scores[offsets[r] + x]
 *      when scores is not NULL.  n_out = offsets[n_rows].  The device form takes d_offsets (int64, n_rows + 1 of them, 8-B
 *      aligned) from the caller, since it allocates nothing; it cannot verify them, so a position outside [0, n_out) is
 *      never written: offsets that are not this prefix sum give unspecified ranks, but no write outside [0, n_out).  The
 *      host form computes the offsets itself and refuses with CSRK_ERR_INVALID, naming the total, when n_out is not it.
 *   5. Agreement.  csrk_rank_entries' rule 5 holds with csrk_topk_scores_for on the same list: a test entry that `seen`
 *      does not store and whose rank < n_top is items[r][rank] there, with the same score bits.
 *   6. Invariance.  No output bit depends on splits, the order or repetition of rows, the previous contents of `ranks`,
 *      repeated calls into the same buffers, or anything in csrk_rank_entries' rule 6.
 *   8. Device form.  Allocates nothing and does not synchronise the host, apart from the remembered canonical look at
 *      `seen` of csrk_rank_entries' rule 8; the clear and the launch go to `stream`.  The host form is synchronous.
 *   9. Refusals; a refused call writes nothing.  Every refusal of csrk_rank_entries that applies, the scalars first, in the
 *      same order, with texts that begin "rank_entries_for: ".  CSRK_ERR_INVALID further: n_rows < 0, u_rows < 0,
 *      splits < 0, n_out < 0 (after the panel type, in this order); u_rows != test's nrows; when there is work, NULL rows
 *      or offsets, and rows or offsets not aligned to their element.  CSRK_ERR_UNSUPPORTED: k above out[0] of
 *      csrk_rank_entries_limits, and more row blocks x splits than a grid holds (2^31 - 1).  n_rows == 0 or n_out == 0:
 *      CSRK_OK, nothing launched and nothing cleared.
 *  10. Limits (csrk_rank_entries_for_limits): out[0] = S_max; [1] = W;  n <= 2.
 *  11. Splits.  With tile = out[2] of csrk_rank_entries_limits and T = ceil(n_items / tile), the items are cut at tile
 *      boundaries into S contiguous ranges: range s holds the tiles [s T / S, (s + 1) T / S) (integer division;
 *      csrk_topk_scores_for's rule 3).  One workgroup takes one (block of 64 list rows, range s) pair.  It scores and orders
 *      its rows' test entries exactly as csrk_rank_entries does -- every split of a block lists the same entries in the
 *      same order --, sweeps only its item interval, takes out again only the `seen` entries whose column lies in that
 *      interval (`seen` is canonical: a lower bound in the row finds where they start) and forms the prefix sums as
 *      csrk_rank_entries does: partial ranks.  splits >= 1 forces S = min(splits, T, S_max), and S = 1 when T = 0 or
 *      n_rows = 0.  splits = 0 is automatic: S = clamp(ceil(W / ceil(n_rows / 64)), 1, min(T, S_max)), with S_max = 64 and
 *      W = 512 the workgroups that fill the card (two per CU, 256 CUs).  csrk_rank_entries_for_splits returns S from these
 *      constants alone.
 *  12. Combining.  S = 1 stores the ranks directly in one launch and touches nothing else of `ranks`.  S > 1 clears
 *      ranks[0 .. n_out) on the stream first; every workgroup then adds its partial rank with one integer atomic add per
 *      listed entry (none where the partial rank is 0).  Only split 0 writes `scores`, and only split 0 contributes the -1
 *      of a bad column.  Integer addition commutes, so no bit depends on S, on the order in which workgroups arrive or on
 *      what `ranks` held before the call.  No float atomics, no workspace, and no workgroup waits for another.  A row with
 *      more than out[4] of csrk_rank_entries_limits test entries is swept again per out[4] of them inside its workgroup. */
CSRK_API int csrk_rank_entries_for(csrk_handle_t seen, csrk_handle_t test, const int32_t *rows, int64_t n_rows, int32_t u_rows,
                                   const void *U, int64_t ldu, const void *V, int64_t ldv, int32_t k, int panel_type,
                                   int32_t *ranks, double *scores, int64_t n_out, int32_t splits);
/* Device form: every pointer in HBM, launched on `stream` (NULL = the default stream). */
CSRK_API int csrk_rank_entries_for_device(csrk_handle_t seen, csrk_handle_t test, const int32_t *d_rows, int64_t n_rows,
                                          int32_t u_rows, const void *d_U, int64_t ldu, const void *d_V, int64_t ldv, int32_t k,
                                          int panel_type, const int64_t *d_offsets, int64_t n_out, int32_t *d_ranks,
                                          double *d_scores, int32_t splits, void *stream);
/* Rule 11: *splits_used = S.  CSRK_ERR_INVALID: n_rows < 0, n_items < 0, splits < 0, a NULL result pointer.  No device is
 * touched. */
CSRK_API int csrk_rank_entries_for_splits(int64_t n_rows, int32_t n_items, int32_t splits, int32_t *splits_used);
/* Diagnostics: the two limits of rule 10, in its order;  n <= 2.  No device is touched. */
CSRK_API int csrk_rank_entries_for_limits(int64_t *out, int n);

/* ---- knn_scores: score items from an item-kNN model's nearest rated neighbours -------------------------
 * Not a reference entry point: the scoring side of the neighbourhood model that csrk_spgemm_abt + csrk_topk_rows build (each
 * row of `model` holds an item's most similar items, best first).  The rule is the one of an item-item recommender: for each
 * target item walk its neighbour list, take the first max_nbrs neighbours the user has rated and average the user's ratings
 * weighted by similarity.  The cut at max_nbrs depends on the user, so no pruning of the model and no product reproduces it.
 * Returns a NEW handle [n_rows x n_targets], row r for user rows[r]; `rows` and `offsets` are host arrays (as csrk_pick_rows'
 * `rows`).
 *   1. Operands.  model is [n_targets x n_items], ratings [n_users x n_items]: model.ncols == ratings.ncols.  ratings must
 *      be CANONICAL (csrk_combine's word; the check is csrk_is_canonical's remembered one and the refusal names the first bad
 *      row).  model need not be: its rows are in by-value order after csrk_topk_rows, and unsorted or repeated columns are
 *      just more entries.  Either pointer width and any value type on either operand; float32 values are widened exactly, a
 *      structure-only operand counts as 1.0 everywhere (csrk_sddmm's rule).  Neither handle is modified, both keep their
 *      plans; model == ratings is allowed.  Model column indices are compared, never used as addresses.
 *   2. The walk.  For output row r (user u = rows[r]) and target i the entries of model row i are taken in STORAGE order.
 *      An entry (j, s) is a HIT when ratings stores (u, j), with value v.  Each hit takes one step, in this order:
 *          t = round(v * s);  num = round(num + t);  den = round(den + |s|);  nn += 1
 *      num and den start at +0.0; every operation is rounded on its own (no fused multiply-add).  With aggregate =
 *      CSRK_KNN_SUM the step is num = round(num + s): v is not read and den is not formed.  With max_nbrs > 0 the walk ends
 *      after the hit that makes nn == max_nbrs; max_nbrs = 0 is no limit.
 *   3. What is stored.  Target i is stored in row r iff nn >= min_nbrs (min_nbrs >= 1).  Its value is round(num / den), one
 *      correctly rounded division, for CSRK_KNN_WEIGHTED_AVERAGE (den = 0 gives NaN or Inf as IEEE says, and the value stays
 *      stored) and num for CSRK_KNN_SUM; with offsets != NULL the value is then round(value + offsets[r]) (a user's mean put
 *      back after csrk_center_rows).
 *   4. Result.  [n_rows x n_targets], float64 values, every row strictly ascending in target index.  It is known to be
 *      canonical (as csrk_coalesce's result): a following csrk_combine or csrk_is_canonical does not look at its rows again.
 *      Row pointers are int32 unless the result holds more than 2^31 - 1 entries (csrk_pick_rows' rule).
 *   5. Invariance.  An output entry depends only on model row i, ratings row u, max_nbrs, min_nbrs, aggregate and offsets[r]:
 *      not on the list's order, length or repeats (a repeated row is computed on its own and gets the same bits), the pointer
 *      widths, launch geometry, the limits below or repeated calls (csrc/knn_scores.hip: parallel over (row, target) pairs,
 *      never inside a walk; every slot is counted, nothing appended in arrival order; no float atomics).
 *   6. Special values.  IEEE throughout.  No path skips an explicit zero similarity or rating: a hit with s = 0.0 counts
 *      toward nn and max_nbrs.  A created NaN has its position specified, not its sign or payload (csrk_combine's rule 7).
 *   7. Refusals; *out = 0 on every failure.  CSRK_ERR_INVALID: a NULL out, a bad handle, model.ncols != ratings.ncols,
 *      operands on different devices, n_rows < 0, NULL rows with n_rows > 0, max_nbrs < 0, min_nbrs < 1, an unknown aggregate,
 *      a non-canonical ratings, or an index of rows outside [0, n_users): the list is looked at on the host before anything
 *      is sent and the message names the first bad position and its value.  CSRK_ERR_UNSUPPORTED: a ratings or model row of
 *      more than 2^31 - 1 entries (a canonical row holds at most ncols <= 2^31 - 1 entries, so in effect a model row).
 *      n_rows = 0, n_targets = 0, model.nnz = 0 or ratings.nnz = 0: CSRK_OK, an empty result, nothing launched -- not
 *      even the look at the rows of ratings, so with one of these a ratings that is not canonical is not refused (the
 *      arguments that need no look at the device are still checked first).
 *   8. Limits (csrk_knn_scores_limits): out[0] = the lanes that share one target's walk; [1] = the targets of a workgroup
 *      tile; [2] = the entries of a rating row held in LDS (a longer row is searched in device memory and gives the same
 *      bits); [3] = the bits of the filter in front of the search (a model column is searched for only when the bit of its
 *      residue modulo [3] is set by some rated column; columns that share a residue cost a search, nothing else); [4] = the
 *      most consecutive tiles one workgroup takes for a row, staging the rating row once; [5] = the workgroups a call is
 *      cut into at least before a workgroup takes more than one tile (tiles per workgroup = n_rows x tiles / [5], within
 *      1 .. [4]);  n <= 6.  No device is touched; by rule 5 none of them changes a bit. */
enum { CSRK_KNN_WEIGHTED_AVERAGE = 0, CSRK_KNN_SUM = 1 };
CSRK_API int csrk_knn_scores(csrk_handle_t model, csrk_handle_t ratings, const int32_t *rows, int64_t n_rows, int32_t max_nbrs,
                             int32_t min_nbrs, int aggregate, const double *offsets, csrk_handle_t *out);
CSRK_API int csrk_knn_scores_limits(int64_t *out, int n);

/* ---- knn_scores, the reach route: walk only the targets a user's ratings reach ------------------------------
 * csrk_knn_scores visits every target for every listed row, and nearly all (row, target) pairs have no rated neighbour.  A
 * target i has a hit for user u exactly when some item j that u rated is stored in model row i -- when i lies in row j of
 * the transpose of the model's pattern.  csrk_knn_scores_reach marks those targets per listed row and walks only them.
 * Rules 1-7 of csrk_knn_scores hold word for word (the refusal texts begin "knn_scores_reach: "; same order, same status
 * codes, same empty-result cases, in which nothing is launched, nothing is built and ratings is not looked at), and the row
 * pointers, columns and values of the result equal csrk_knn_scores' bit for bit for every input: min_nbrs >= 1, so every
 * stored target is a marked one, and a marked target is walked by the routine csrk_knn_scores walks with.
 *   One further requirement: model column indices must lie in [0, ncols), as csrk_transpose requires of its operand -- the
 *   index is built from them.  A ratings column outside [0, n_items) is never an address: it reaches nothing.
 *   The reach index of a model is the structure-only transpose of its pattern: row j holds, ascending, the targets whose
 *   model row stores column j, once per stored occurrence (entries = the model's nnz).  The model handle keeps it the way it
 *   keeps its plans: built under the handle's lock by the first csrk_knn_scores_reach or by csrk_knn_reach_index(build = 1),
 *   counted by csrk_device_bytes, dropped by everything that drops the plans -- csrk_order_columns, which rewrites the
 *   columns, and the in-place value operations (csrk_unit_rows, csrk_center_rows ...) too, although they would leave it
 *   right -- and freed with the handle.  csrk_knn_reach_index with build = 0 only reports: *entries = *bytes = 0 when the
 *   handle holds no index.
 *   Limits (csrk_knn_scores_reach_limits): out[0] = R, the targets of one range = the bits of the mark bitmap a workgroup
 *   holds in LDS (a power of two, a multiple of 32; one workgroup takes one (listed row, range) pair); [1] = the lanes that
 *   share a walk, [2] = the staged rating-row entries, [3] = the filter bits (csrk_knn_scores_limits' [0], [2], [3]); [4] =
 *   the candidates a workgroup walks per round; [5] = the targets per enumeration chunk (= [0]: a range is enumerated in one
 *   piece); [6] = a reach row with more entries than this at or above the range's base is marked by a whole wavefront
 *   rather than by [1] lanes;  n <= 7.  No device is touched; none of them changes a bit.
 *   Diagnostics (csrk_knn_scores_last_stats; thread-local, filled from what the host holds, like csrk_spgemm_last_stats):
 *   out[0] = 1 when the calling thread's last scoring call took the reach route (0 after csrk_knn_scores, after a failed
 *   call and after an empty result, and then every slot is 0); [1] = ranges per listed row = ceil(n_targets / R); [2] =
 *   workgroups per pass; [3] = 1 when the first pass counted marks without walking (min_nbrs == 1); [4] = 1 when this call
 *   built the index; [5] = entries stored;  n <= 6. */
CSRK_API int csrk_knn_scores_reach(csrk_handle_t model, csrk_handle_t ratings, const int32_t *rows, int64_t n_rows,
                                   int32_t max_nbrs, int32_t min_nbrs, int aggregate, const double *offsets, csrk_handle_t *out);
CSRK_API int csrk_knn_reach_index(csrk_handle_t model, int build, int64_t *entries, int64_t *bytes);
CSRK_API int csrk_knn_scores_reach_limits(int64_t *out, int n);
CSRK_API int csrk_knn_scores_last_stats(int64_t *out, int n);

#ifdef __cplusplus
}
#endif
#endif /* CSRK_H */
