/*
 * The device kernel of the RBMAL learner (ital_amd/competitors.py, the reference's ital/baseline_methods.py:477-513): the
 * cosine distance of every data row to its nearest labelled row (csrc/cosine.hip).  Conventions as in ital_dense.h and
 * ital_rows.h: borrowed device pointers, asynchronous on `stream`, 0 or a negative errno-style code with its message in
 * ital_last_error, argument checks before any HIP call, no allocation across the ABI.
 */
#ifndef ITAL_COSINE_H
#define ITAL_COSINE_H

#include "ital_hip.h"
#include "ital_ingest.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[i] = min_j ( 1 - clip( x_i . t_j / (sqrt(xnorm[i]) * sqrt(tnorm[j])) ) ),  i < n, j < c.
 * Replaces scipy.spatial.distance.cdist(data[candidates], data[train_ids], 'cosine').min(axis=-1),
 * reference ital/baseline_methods.py:500.
 *
 * X: [n][ldx] of the element type `xtype` (the ITAL_INGEST_* codes), ldx a multiple of 16 ELEMENTS, pad columns +0, the
 * matrix aligned to 16 B (the conventions of ital_rows.h).  xnorm: the FP64 squared norms of its rows (ital_row_norms on the
 * widened rows: what a store or a GP already holds).  T: [c][ldx] FP64, pad columns +0, aligned to 16 B; tnorm: the squared
 * norms of its rows.
 *
 * DEFINITION, per pair (i, j):
 *   dot = the FP64 sum over the ldx columns, formed on v_mfma_f64_16x16x4_f64 in an order that depends on nothing but ldx:
 *         not on n, c, where row i or row j stands, how the rows of T are cut into blocks or calls, `accumulate` or `xtype`
 *         (narrow elements are widened in registers, which is exact);
 *   cos = dot / (sqrt(xnorm[i]) * sqrt(tnorm[j]))       IEEE division, correctly rounded roots;
 *   if (fabs(cos) > 1) cos = copysign(1, cos)           scipy's own clip;
 *   d   = 1 - cos.
 * The minimum over j propagates NaN as np.min does (a zero row gives 0 / 0: NaN, as scipy returns for it); a NaN result is
 * the canonical quiet NaN.  With accumulate != 0 the result is min(out[i], that) by the same rule, otherwise out[i] is
 * overwritten: a minimum is exact, so T cut into several calls gives the bits of one call.
 *
 * Rows >= n of out are not touched, rows >= c of T and tnorm are not read.  X is streamed ceil(c / 64) times.
 *
 * -22 (before any HIP call): n < 0, n > 2^36, c < 1, ldx <= 0 or not a multiple of 16, an unknown xtype, and with n > 0 a
 * NULL pointer, X or T not aligned to 16 B.  n == 0 returns 0 without a launch. */
int ital_cosine_min(const void* X, int xtype, const double* xnorm, int64_t n, int ldx, const double* T, const double* tnorm,
                    int c, int accumulate, double* out, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_COSINE_H */
