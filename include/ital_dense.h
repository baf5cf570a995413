/*
 * Dense FP64 kernels of the cross-validated hyper-parameter search (ital_amd/tune.py, the reference's
 * optimize_parameters.py): fold Grams, a batched blocked Cholesky, the triangular solves and a kernel-times-matrix
 * product (csrc/dense.hip).  Conventions as in ital_hip.h: borrowed device pointers, asynchronous on `stream`, 0 or a
 * negative errno-style code with its message in ital_last_error; no allocation crosses the ABI.
 *
 * Batched calls take arrays in DEVICE memory with one entry per matrix: matrix pointers, sizes n[b] and leading dimensions
 * ld[b] (row-major, ld[b] >= n[b]); max_n (host) is the largest n[b].  Only the lower triangle (j <= i < n) is read or
 * written; the strict upper triangle and the padding past n are left as they are.  The matrices of one call are
 * independent: a matrix gets the same bits alone or in any batch. */
#ifndef ITAL_DENSE_H
#define ITAL_DENSE_H

#include "ital_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* K_b[i][j] = var*exp(-|x_p - x_q|^2 / (2 l^2)) + noise*(i == j), p = idx_b[i], q = idx_b[j], for rows of X (ldx a multiple
 * of 16, squared norms xnorm): the Gram of a fold's training set, distances on FP64 MFMA, nothing of size N^2 formed.
 * Replaces K_all[np.ix_(ind, ind)] + noise * eye of GaussianProcess.fit, reference ital/gp.py:128, :157-158, :419-436, as
 * optimize_parameters.py:28-62 reaches it (a precomputed pdist, :137-138, is not needed). */
int ital_gram_rows(const double* X, const double* xnorm, int ldx, const int64_t* const* idx, const int* n, double* const* K,
                   const int64_t* ld, int count, int max_n, double var, double length_scale, double noise,
                   hipStream_t stream);

/* In-place lower Cholesky A_b = L_b L_b^T of every matrix (blocked: 64 x 64 diagonal blocks, row-wise panel solve, trailing
 * update on FP64 MFMA).  info[b] <- 0, or j + 1 for the first column j whose pivot is not > 0 in floating point (NaN
 * included); such a matrix also sets *status |= 1 and is left partially factored.  Replaces invh's dpotrf, reference
 * ital/gp.py:8-37, as GaussianProcess.fit calls it, :141-161. */
int ital_chol_batched(double* const* A, const int* n, const int64_t* ld, int count, int max_n, int* info, int* status,
                      hipStream_t stream);

/* y_b <- L_b^-T L_b^-1 y_b (alpha = K^-1 y) for every factor with info[b] == 0 (info may be NULL); others are skipped.
 * Replaces the dpotri + np.dot(K_inv, y) of GaussianProcess.fit, reference ital/gp.py:30-37, :159. */
int ital_chol_solve_batched(const double* const* L, const int* n, const int64_t* ld, double* const* y, int count,
                            const int* info, hipStream_t stream);

/* out[i][f] = sum_j var*exp(-|a_i - b_j|^2 / (2 l^2)) W[j][f] for F <= 16 right-hand sides, without forming the kernel
 * matrix (distances and the accumulation on FP64 MFMA).  With W[j][f] = alpha of fold f at sample j (0 outside its
 * training set) one call yields every fold's held-out predictions.  work: ital_kernel_matvec_workspace(na, nb) doubles of
 * device memory (0: may be NULL); the sum over b is split in a fixed order, so the result does not depend on the run.
 * Replaces predict_stored's K_all[np.ix_(ind, test)] and np.dot(w.T, k_test), reference ital/gp.py:203-232 (:219-220). */
int ital_kernel_matvec(const double* Xa, const double* an, int64_t na, const double* Xb, const double* bn, int64_t nb,
                       int ldx, const double* W, int64_t ldw, int F, double var, double length_scale, double* out,
                       int64_t ldo, double* work, int64_t work_doubles, hipStream_t stream);
int64_t ital_kernel_matvec_workspace(int64_t na, int64_t nb);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_DENSE_H */
