/*
 * Device kernels of the AdaptAL learner (ital_amd/adapt_al.py, the reference's ital/adapt_al.py): the diagonal of the
 * inverse of a Cholesky-factored Gram, the entropy / information-density pair and the expected classification error
 * (csrc/adapt.hip).  Conventions as in ital_dense.h: borrowed device pointers, asynchronous on `stream`, 0 or a negative
 * errno-style code with its message in ital_last_error, argument checks before any HIP call, no allocation across the
 * ABI; every sum runs in a fixed order, so results do not depend on the run.
 */
#ifndef ITAL_ADAPT_H
#define ITAL_ADAPT_H

#include "ital_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[i] = sum_j (L^-1)[j][i]^2 = (K^-1)_ii for the lower Cholesky factor L (row-major, n x n, leading dimension ld >= n;
 * only j <= i is read) that ital_chol_batched left of K.  1 / out[i] is the Schur complement K_ii - k_i^T K_(-i)^-1 k_i,
 * the `sigma_updated` that information_density obtains from one reduced_inv per candidate, reference
 * ital/adapt_al.py:11-36, :143-157.  Blocked triangular inverse by recursive doubling: the 64 x 64 diagonal blocks first,
 * then the off-diagonal block of every pair of neighbouring inverted blocks, M21 = -M22 (L21 M11), both products on FP64
 * MFMA over their triangular k-range only (n^3 / 3 flop); the squared column sums are taken from the accumulators, L^-1 is
 * not read again.  work: ital_chol_inv_diag_workspace(n) doubles.  info (may be NULL): the factorisation's info word; if
 * *info != 0 nothing is computed and out is filled with NaN. */
int ital_chol_inv_diag(const double* L, int n, int64_t ld, double* out, double* work, int64_t work_doubles, const int* info,
                       hipStream_t stream);
int64_t ital_chol_inv_diag_workspace(int n);

/* entropy[i] = H(clip(norm.cdf(0, mu[i], sqrt(max(s2[i], 0))), 1e-8, 1 - 1e-8)) (no noise under the root; NaN where the
 * clamped variance is 0, as scipy's scale check) and density[i] = log(kdiag / max(1e-6, 1 / inv_diag[i])) / 2 with
 * kdiag = var + noise, the diagonal of the candidate Gram: reference ital/adapt_al.py:115-129, :159. */
int ital_adapt_scores(const double* mu, const double* s2, const double* inv_diag, int64_t n, double kdiag, double* entropy,
                      double* density, hipStream_t stream);

/* err[a] = expected classification error of candidate rows[a] (a < r), reference ital/adapt_al.py:162-190: for the
 * simulated targets y = 1 (fb True) and y = 0 (fb False; the reference passes float(fb), not -1) the rank-one update
 * g = 1 / (s2_i + noise), mean'_j = mu_j + C[a][j] g (y - mu_i), var'_j = max(0, s2_j - C[a][j]^2 g) of every other candidate
 * j, p'_j the clipped norm.cdf(0, mean'_j, sqrt(var'_j)), sum_j (mu_j > 0 ? p'_j : 1 - p'_j), weighted with 1 - p_i
 * (True) and p_i (False) and added in that order.  C: the posterior covariance rows of the r candidates with all nc
 * (ital_cov_block), leading dimension ldc >= nc; mu, s2 (unclamped) over the nc candidates; work: 2 r doubles.  One
 * workgroup per (row, fb), a fixed-order reduction. */
int ital_adapt_error(const double* C, int64_t ldc, const int* rows, int r, int64_t nc, const double* mu, const double* s2,
                     double noise, double* work, double* err, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_ADAPT_H */
