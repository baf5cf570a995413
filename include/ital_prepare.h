/*
 * Preparing feature rows on the device (csrc/prepare.hip): column statistics, min-max scaling, the centred scatter matrix
 * of a store on v_mfma_f64_16x16x4_f64 and the projection of its rows onto a few axes -- what the reference's
 * Dataset._preprocess (datasets.py:107-112) and a PCA reduction do on the host (ital_amd/prepare.py).  Conventions as in
 * ital_knn.h and ital_ingest.h: borrowed device pointers, asynchronous on `stream`, 0 or a negative errno-style code with its
 * message in ital_last_error, argument checks before any HIP call, no allocation across the ABI.  Plain vector stores, no
 * floating-point atomics, no workgroup waits for another.
 *
 * X is always [n][ldx] of the element type `xtype` (the ITAL_INGEST_* codes), ldx a multiple of 16 ELEMENTS and >= d, the
 * matrix aligned to 16 B; narrow elements are widened in registers, which is exact.  Only the columns j < d are read.
 *
 * THE RANGE RULE.  Sums over the n rows are formed over row ranges and the ranges are added in ascending order.  With a
 * unit of u rows and a cap of c ranges:
 *     units = ceil(n / u);  per = ceil(units / min(c, units));  ranges = ceil(units / per);
 *     range r = rows [r * per * u, min(n, (r + 1) * per * u)).
 * ital_col_stats: u = ITAL_PREPARE_STATS_UNIT, c = ITAL_PREPARE_STATS_CAP (a function of n alone).
 * ital_col_cov:   u = ITAL_PREPARE_COV_UNIT,   c = ital_col_cov_cap(d) = clamp(2^24 / d^2, 1, ITAL_PREPARE_COV_CAP): at
 *                 most 32 partial d x d results, at most 128 MB of them up to d = 4096 (a function of (n, d) alone).
 * The bits of a result therefore depend on the values, n, d and ldx, not on the device, the stream or a launch shape.
 */
#ifndef ITAL_PREPARE_H
#define ITAL_PREPARE_H

#include <stddef.h>

#include "ital_hip.h"
#include "ital_ingest.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ITAL_PREPARE_STATS_UNIT 128
#define ITAL_PREPARE_STATS_CAP 1024
#define ITAL_PREPARE_COV_UNIT 512
#define ITAL_PREPARE_COV_CAP 32
#define ITAL_PREPARE_MAX_K 512

/* Number of row ranges of the rule above (host only, no HIP call); 0 for n <= 0, unit < 1 or cap < 1. */
int64_t ital_prepare_ranges(int64_t n, int unit, int cap);
/* The cap of ital_col_cov's ranges for d columns; 0 for d < 1. */
int ital_col_cov_cap(int d);

/* Per column j < d: cmin[j], cmax[j] = the smallest / largest of the n values, csum[j] = their FP64 sum.
 *
 * DEFINITION.  A column that holds a NaN gives NaN (the canonical quiet NaN) in all three outputs, as np.min does.  Otherwise
 * min and max are exact (of +0 and -0 either may be returned).  The sum of a range: row i of the range, counted from its
 * start, belongs to chain i % 4; a chain adds its rows in ascending order starting from +0; the range's sum is
 * ((chain0 + chain1) + chain2) + chain3; the ranges are added in ascending order starting from the first range's sum.
 *
 * workspace: at least ital_col_stats_workspace(n, d) bytes, aligned to 8 B; nothing but the three outputs and the workspace
 * is written.
 *
 * -22 (before any HIP call): n < 0 or n > 2^31 - 1; d < 1; ldx not a positive multiple of 16 or < d; an unknown xtype; with
 * n > 0 a NULL X, cmin, cmax, csum or workspace, an X not aligned to 16 B, an output or workspace not aligned to 8 B, or
 * workspace_bytes below ital_col_stats_workspace.  n == 0 returns 0 without a launch and writes nothing. */
int ital_col_stats(const void* X, int xtype, int64_t n, int d, int ldx, double* cmin, double* cmax, double* csum,
                   void* workspace, size_t workspace_bytes, hipStream_t stream);
size_t ital_col_stats_workspace(int64_t n, int d);

/* Y[i][j] = (x[i][j] - lo[j]) / span[j] for j < d: one IEEE FP64 subtraction, then one IEEE FP64 division (no reciprocal,
 * no fused operation), so that an FP64 result has the bits of numpy's (X - lo) / span.  Y: [n][ldy] of the element type
 * `ytype`, ldy a multiple of 16 and >= d, aligned to 16 B; a narrower type is reached from the FP64 value by ONE rounding
 * to nearest, ties to even, values beyond the largest finite number plus half a unit go to infinity, subnormals are kept;
 * columns d <= j < ldy get +0.0.  lo, span: [d] FP64 on the device.  X and Y must not overlap.
 *
 * -22 (before any HIP call): n < 0 or n > 2^31 - 1; d < 1; ldx or ldy not a positive multiple of 16 or < d; an unknown xtype
 * or ytype; with n > 0 a NULL X, lo, span or Y, an X or Y not aligned to 16 B, lo or span not aligned to 8 B.  n == 0 returns
 * 0 without a launch. */
int ital_scale_rows(const void* X, int xtype, int64_t n, int d, int ldx, const double* lo, const double* span, void* Y,
                    int ytype, int ldy, hipStream_t stream);

/* C[a][b] = sum over the n rows of (x[i][a] - mean[a]) * (x[i][b] - mean[b]), a, b < d; C: [d][ldc] FP64, ldc >= d.
 *
 * DEFINITION.  Every element is widened and centred first (one FP64 subtraction), then multiplied: never sum x x^T - n m m^T.
 * The products of a range are added on v_mfma_f64_16x16x4_f64 in steps of 16 rows ascending, within a step the four MFMAs
 * of rows 4 g + j, j = 0..3, within an MFMA the hardware's fixed order over its four row groups g; rows at or beyond the end
 * of the range enter as exact zeros (masked after centring), so do columns >= d.  The partial results of the ranges (the
 * rule above) are added in ascending order starting from the first.  C[a][b] and C[b][a] are one number written twice:
 * equal in bits.  n == 1 with mean == the row gives exactly +0.
 *
 * mean: [d] FP64 on the device.  workspace: at least ital_col_cov_workspace(n, d) bytes, aligned to 8 B.
 *
 * -22 (before any HIP call): n < 0 or n > 2^31 - 1; d < 1; ldx not a positive multiple of 16 or < d; ldc < d; an unknown
 * xtype; with n > 0 a NULL X, mean, C or workspace, an X not aligned to 16 B, mean, C or the workspace not aligned to 8 B,
 * workspace_bytes below ital_col_cov_workspace.  n == 0 returns 0 without a launch. */
int ital_col_cov(const void* X, int xtype, int64_t n, int d, int ldx, const double* mean, double* C, int64_t ldc,
                 void* workspace, size_t workspace_bytes, hipStream_t stream);
size_t ital_col_cov_workspace(int64_t n, int d);

/* Y[i][c] = sum over j < d of (x[i][j] - shift[j]) * W[j][c], c < k; W: [d][ldw] FP64 on the device, ldw >= k.
 *
 * DEFINITION.  The sum runs on v_mfma_f64_16x16x4_f64 over j < ldx in steps of 16 ascending (columns d <= j < ldx enter as
 * exact zeros), within a step the four MFMAs of columns 4 g + j', j' = 0..3, within an MFMA the hardware's fixed order over
 * g: a function of ldx alone, not of n, k, the types or where a row stands in its tile.  Y: [n][ldy] of the element type
 * `ytype`, ldy a multiple of 16 and >= k, aligned to 16 B, narrowed as in ital_scale_rows; columns k <= c < ldy get +0.0.
 * A workgroup owns 128 rows and 128 columns of Y (64 columns when k <= 64) and stages its columns of W once; X is therefore
 * read once per 128 columns of Y: once for k <= 128, four times at k = 512.  X and Y must not overlap.
 *
 * -22 (before any HIP call): n < 0 or n > 2^31 - 1; d < 1; k < 1 or k > ITAL_PREPARE_MAX_K; ldx or ldy not a positive
 * multiple of 16, ldx < d or ldy < k; ldw < k; an unknown xtype or ytype; with n > 0 a NULL X, shift, W or Y, an X or Y not
 * aligned to 16 B, shift or W not aligned to 8 B.  n == 0 returns 0 without a launch. */
int ital_project_rows(const void* X, int xtype, int64_t n, int d, int ldx, const double* shift, const double* W, int64_t ldw,
                      int k, void* Y, int ytype, int ldy, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_PREPARE_H */
