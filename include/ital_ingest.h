/*
 * Feature rows as the caller has them -> the padded FP64 rows and squared norms every kernel reads (ital_amd DeviceData,
 * GaussianProcess.predict on a tensor; csrc/ingest.hip).  Conventions as in ital_dense.h: borrowed device pointers,
 * asynchronous on `stream`, 0 or a negative errno-style code with its message in ital_last_error, argument checks before any
 * HIP call, no allocation across the ABI (the call needs no workspace).
 */
#ifndef ITAL_INGEST_H
#define ITAL_INGEST_H

#include "ital_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Element types of `src`. */
#define ITAL_INGEST_F64 0
#define ITAL_INGEST_F32 1
#define ITAL_INGEST_F16 2
#define ITAL_INGEST_BF16 3

/* dtype: 0 = f64, 1 = f32, 2 = f16, 3 = bf16.  src: DEVICE memory, n rows of d elements, row stride ld_src ELEMENTS.
 *
 * DEFINITION: X[i][j] = (double)src[i * ld_src + j] for j < d (exact for all four types); X[i][j] = +0.0 for d <= j < ldx,
 * whatever the buffer held before; xnorm[i] has the bits ital_row_norms(X, n, ldx, xnorm) gives on the rows just written (it
 * IS a launch of ital_row_norms behind the conversion); rows >= n of X and xnorm are not touched.
 *
 * One wave per row, 16-B stores.  The load width is chosen per call from the actual pointer and stride: 16 B per lane when src
 * and ld_src * sizeof(element) are both multiples of 16 B (a row's ragged last vector is still read element by element: nothing
 * past src[i][d - 1] is ever read), single elements otherwise -- both write the same bits.
 *
 * -22 (before any HIP call): a NULL pointer with n > 0, n < 0, d < 1, ldx not a multiple of 16, ldx < d, ld_src < d, an
 * unknown dtype, src not aligned to its element size, X not aligned to 16 B or xnorm not to 8 B.  n == 0 returns 0 without a
 * launch. */
int ital_ingest_rows(const void* src, int dtype, int64_t n, int d, int64_t ld_src, double* X, int ldx, double* xnorm,
                     hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_INGEST_H */
