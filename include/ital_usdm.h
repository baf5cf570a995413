/*
 * Device side of the USDM learner (ital_amd/usdm.py, the reference's ital/baseline_methods.py:575-658; csrc/usdm.hip): the
 * graph Laplacian of the unlabelled rows, a dense LU without pivoting for its harmonic solve, and the two kernels the
 * augmented-Lagrangian loop needs beside the Cholesky of ital_dense.h -- the shifted copy of the Gram and a symmetric
 * matrix-vector product.  Conventions as in ital_dense.h: borrowed device pointers, asynchronous on `stream`, 0 or a
 * negative errno-style code with its message in ital_last_error, every argument check before any HIP call, no allocation
 * across the ABI.  Matrices are row-major with a leading dimension ld >= n; the padding past n and every byte outside the
 * stated write set are left as they are.  -22 for a negative size, ld < n, or (with work to do) a NULL pointer or a pointer
 * to doubles / int64 that is not aligned to 8 bytes.  A size of 0 is no work: 0 is returned without a launch.
 */
#ifndef ITAL_USDM_H
#define ITAL_USDM_H

#include "ital_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The system (D_uu - W_uu) p = W_ul y of the harmonic label propagation over the directed neighbour graph
 * W_ij = eps + [j is a neighbour of i], deg_i = k + n eps (baseline_methods.py:603-608, :619-620).
 *
 * idx: [n][k] neighbour lists as ital_knn_rows writes them (a -1 slot is no neighbour); u: [n_u] ascending unlabelled rows;
 * pos: [n] position of a row in u, or -1; rel: [n] bytes, nonzero on relevant rows; n_rel: the number of relevant rows.
 * DEFINITION, in bits (fl: one FP64 rounding, no fused multiply-add), i = u[a], j = u[b]:
 *   w1 = fl(1 + eps);  deg = fl(k + fl(n * eps));
 *   M[a * ld + b] = -(j is in the list of i ? w1 : eps)   for a != b,
 *   M[a * ld + a] = fl(deg - eps),
 *   rhs[a] = fl(c_a + fl(n_rel * eps)),   c_a = the number of slots of i's list that hold a relevant row.
 * The whole n_u x n_u block of M and rhs[0 .. n_u) are written, nothing else.
 * -22 also for k < 1 or k > 32 (ITAL_KNN_MAX_K), n_u > n, n_rel < 0 or n_rel > n. */
int ital_usdm_laplacian(const int64_t* idx, int k, int64_t n, const int64_t* u, int64_t n_u, const int64_t* pos,
                        const unsigned char* rel, int64_t n_rel, double eps, double* M, int64_t ld, double* rhs,
                        hipStream_t stream);

/* In-place LU factorisation WITHOUT PIVOTING of one n x n matrix: A = L U, L unit lower (its ones are not stored), U upper.
 * Blocked as ital_chol_batched: 64 x 64 diagonal blocks, L21 = A21 U11^-1 one row per thread, U12 = L11^-1 A12 one column
 * per thread, the trailing update A22 -= L21 U12 over 128 x 128 tiles on v_mfma_f64_16x16x4_f64.
 *
 * CONTRACT.  This is not a general solver.  It is for matrices that need no pivoting: strictly diagonally dominant by rows
 * (as D_uu - W_uu is, with margin (n - n_u) eps or more), which stay so under elimination with a growth factor of at most
 * 2 (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 9.9), or symmetric positive definite ones.
 *
 * info <- 0, or j + 1 for the first column j whose pivot is not > 0 in floating point (NaN included); then *status |= 1, the
 * factorisation stops and the matrix is left partially factored.  -22 also for more than 2^31 - 1 tiles of 128 x 128
 * (n above about 5.9 million). */
int ital_lu_factor(double* A, int64_t n, int64_t ld, int* info, int* status, hipStream_t stream);

/* y <- U^-1 L^-1 y from the factor of ital_lu_factor; skipped when info (may be NULL) points to a nonzero value.  One
 * workgroup, as ital_chol_solve_batched. */
int ital_lu_solve(const double* LU, int64_t n, int64_t ld, double* y, const int* info, hipStream_t stream);

/* The matrix of one iteration of the loop (baseline_methods.py:642-644), lower triangle only:
 * B[i * ldb + j] = fl(K[i * ldk + j] + mu) for j < i and fl(fl(K[i * ldk + i] + mu) + mu) on the diagonal, the reference's two
 * additions in its order.  The strict upper triangle of B is neither read nor written; K == B (ldk == ldb) is allowed. */
int ital_usdm_shift(const double* K, int64_t n, int64_t ldk, double mu, double* B, int64_t ldb, hipStream_t stream);

/* out = K_sym x for the symmetric matrix whose lower triangle (j <= i) K holds; the strict upper triangle is never read.
 * Every stored off-diagonal entry is loaded once and serves two outputs.  The partial sums of the 64 x 64 blocks go to
 * `work` (at least ital_symv_lower_workspace(n) doubles) and are added in ascending block order by a second kernel: no
 * floating-point atomics, two calls give equal bits.  Nothing but out[0 .. n) and work is written. */
int ital_symv_lower(const double* K, int64_t n, int64_t ld, const double* x, double* out, double* work,
                    int64_t work_doubles, hipStream_t stream);
int64_t ital_symv_lower_workspace(int64_t n);   /* 0 for n <= 0 or n > 2^31 - 1 - 128 */

#ifdef __cplusplus
}
#endif
#endif /* ITAL_USDM_H */
