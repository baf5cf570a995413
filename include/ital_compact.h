/*
 * Deleting data rows from a live model: the surviving rows, and everything that is indexed by row, gathered into fresh
 * buffers (ital_amd DeviceData.remove, GaussianProcess.drop_rows / sync_data; csrc/compact.hip).  Pure data movement: no
 * arithmetic, no bit of a survivor changes.  Conventions as in ital_ingest.h / ital_rows.h: borrowed device pointers,
 * asynchronous on `stream`, 0 or a negative errno-style code with its message in ital_last_error, argument checks before any
 * HIP call, no allocation across the ABI (the calls need no workspace).
 *
 * keep: DEVICE array of n_keep strictly ascending row indices in [0, n).  Both calls are OUT OF PLACE: a destination that
 * overlaps its source is refused.
 *
 * Defensive indexing (both calls): a keep[j] outside [0, n) is never dereferenced; the destination entries of that j are
 * written as +0.0 and, if `status` is not NULL, bit 0 of *status is set (an atomic OR; *status is otherwise left as it is).
 */
#ifndef ITAL_COMPACT_H
#define ITAL_COMPACT_H

#include "ital_hip.h"
#include "ital_ingest.h"

#ifdef __cplusplus
extern "C" {
#endif

/* X: n padded rows of ldx ELEMENTS of type `xtype` (the ITAL_INGEST_* codes), xnorm: their n squared norms.
 *
 * DEFINITION: X_dst[j][c] has the bits of X[keep[j]][c] for every c < ldx (pad columns included) and xnorm_dst[j] the bits of
 * xnorm[keep[j]], j < n_keep; rows >= n_keep of the destinations are not touched.
 *
 * -22 (before any HIP call): a NULL pointer (status apart) with n_keep > 0, n < 0, n_keep < 0, n_keep > n, ldx < 16 or no
 * multiple of 16, an unknown xtype, X or X_dst not aligned to 16 B, a destination byte range (n_keep rows) that overlaps its
 * source range (n rows).  n_keep == 0 returns 0 without a launch. */
int ital_compact_rows(const void* X, const double* xnorm, int64_t n, int ldx, int xtype, const int64_t* keep, int64_t n_keep,
                      void* X_dst, double* xnorm_dst, int* status, hipStream_t stream);

/* V: the whitened block, m rows of n columns with leading dimension ldv; mu, s2: n entries each.
 *
 * DEFINITION: V_dst[r][j] = V[r][keep[j]] for r < m, j < n_keep; V_dst[r][j] = +0.0 for n_keep <= j < ldv_dst, r < m, and for
 * all j < ldv_dst, m <= r < v_rows_dst (V stays zero outside [0:m, 0:n)); mu_dst[j] = mu[keep[j]] and s2_dst[j] = s2[keep[j]]
 * for j < n_keep, entries >= n_keep of both are not touched.  m == 0 is valid: only mu / s2 move and V_dst is zeroed.
 *
 * -22 (before any HIP call): a NULL pointer with n_keep > 0 (status apart; V may be NULL when m == 0 and V_dst when
 * v_rows_dst == 0), n < 0, n_keep < 0, n_keep > n, m < 0, v_rows_dst < m, ldv < n with m > 0, ldv_dst no multiple of 16,
 * ldv_dst < n_keep, a destination byte range that overlaps its source range.  n_keep == 0 still zero-fills V_dst. */
int ital_compact_cols(const double* V, int64_t ldv, int m, const double* mu, const double* s2, int64_t n, const int64_t* keep,
                      int64_t n_keep, double* V_dst, int64_t ldv_dst, int v_rows_dst, double* mu_dst, double* s2_dst,
                      int* status, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_COMPACT_H */
