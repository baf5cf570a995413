/*
 * What taking each label back would change, without doing it (ital_amd GaussianProcess.influence / preview_remove,
 * ActiveRetrievalBase.audit / preview_revoke; csrc/influence.hip).  From the Cholesky-whitened GP state of ital_revoke.h --
 * L (K_SS + noise I = L L^T), alpha = L^-1 y, V = L^-1 K_S,:, mu = V^T alpha, s2 = var - colsum(V^2) -- with M = L^-1:
 *
 *     c_i = (K^-1)_ii = sum_{p >= i} M[p][i]^2        w = K^-1 y = M^T alpha        B = K^-1 K_S,: = M^T V   (m x n)
 *
 * and removing labelled position i gives, for every row j,
 *
 *     mu'_ij = mu_j - (w_i / c_i) B_ij        s2'_ij = s2_j + B_ij^2 / c_i
 *     loo_mean_i = y_i - w_i / c_i            loo_var_i = 1 / c_i                    (R&W 5.12, as in ital_evidence.h)
 *
 * So the effect of all m removals is one product M^T V on v_mfma_f64_16x16x4_f64; nothing of size m x n is stored and the
 * state is only read.  Conventions as in ital_dense.h: borrowed device pointers, asynchronous on `stream`, 0 or a negative
 * errno-style code with its message in ital_last_error, argument checks before any HIP call, no allocation across the ABI.
 * Every sum runs in a fixed order and there are no floating-point atomics: equal inputs give equal bits.
 */
#ifndef ITAL_INFLUENCE_H
#define ITAL_INFLUENCE_H

#include "ital_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ital_influence_desc {
    const double* L;        /* lower Cholesky factor of K_SS + noise I, row-major, leading dimension ldl >= m; rows >= m are not read */
    int ldl;
    const double* alpha;    /* [>= m] L^-1 y */
    int m;                  /* labelled samples, >= 1 */
    const double* V;        /* [>= m][ldv] whitened block of this rank's n columns (may be NULL when n == 0); rows >= m and
                               columns >= n are not read */
    int64_t ldv;            /* >= n */
    int64_t n;              /* >= 0 */
    const double* mu;       /* [n] V^T alpha */
    const double* s2;       /* [n] var - colsum(V^2); ital_gp_preview_remove only (ital_gp_influence ignores it) */
    const uint8_t* mask;    /* [n] rows that count in `stats` (!= 0), or NULL for all; ital_gp_influence only */
    double* coef;           /* out [m][2]: c_i, w_i */
    double* stats;          /* out [m][4]: dmu_sq, dmu_max, flips, ds2 (below); ital_gp_influence only */
    double* work;           /* ital_gp_influence_workspace(m, n) doubles */
    int64_t work_doubles;
    int* status;            /* |= 1 when some c_i is not finite or not > 0 (a factor that was broken before) */
} ital_influence_desc;

/* coef[i] = (c_i, w_i) and, over the rows j < n with mask[j] != 0,
 *
 *     stats[i][0] = dmu_sq_i  = sum_j (mu'_ij - mu_j)^2
 *     stats[i][1] = dmu_max_i = max_j |mu'_ij - mu_j|
 *     stats[i][2] = flips_i   = #{ j : (mu_j > 0) != (mu'_ij > 0) }     (a count kept as a double: exact up to 2^53)
 *     stats[i][3] = ds2_i     = sum_j B_ij^2 / c_i                      (the total variance that label i removes)
 *
 * Stage 1: ital_chol_inv_diag_batched with count = 1 leaves M in `work` and gives c; w_i = sum_{p >= i} M[p][i] alpha_p, p
 * ascending.  Stage 2: the 128 x 128 tiles of M^T V (k-blocks above the diagonal of M^T are skipped), each reduced to
 * per-row partials (sum B^2, max |B|, flips) in `work`; a last kernel adds the column tiles in ascending order (beyond 256 tiles in
 * 256 ascending chunks, whose sums it then adds in ascending order: a grouping that depends on n alone) and scales by
 * w_i / c_i and 1 / c_i.  n == 0: stage 1 only, `stats` is zero.  A row whose c_i is not finite or not > 0 gets NaN in all six
 * outputs and sets *status |= 1; the other rows are unaffected.  Several ranks: L and alpha are replicated, V is
 * column-sharded; every rank calls with its own columns, sums add and maxima take the max.
 * -22: a NULL descriptor or required pointer, m < 1, n < 0, ldl < m, ldv < n, work smaller than
 * ital_gp_influence_workspace(m, n). */
int ital_gp_influence(const ital_influence_desc* desc, hipStream_t stream);

/* Doubles of `work` for m labelled samples and n columns (0 for m < 1 or n < 0). */
int64_t ital_gp_influence_workspace(int m, int64_t n);

/* mu_out[q * ldo + j] = mu'_{sel[q], j} and s2_out[q * ldo + j] = s2'_{sel[q], j} (not clamped), j < n, q < r, for the labelled
 * positions sel[0 .. r) (HOST array, positions may repeat): stage 1 as above (coef is written), then the same tile with the
 * listed rows of M^T as its first operand and a writing epilogue, 128 listed positions per launch.  The mask and `stats` are
 * not used.  A listed position whose c is not finite or not > 0 gets NaN.
 * -22: as above, and a NULL sel, s2 or output, r < 1, ldo < n, a sel entry outside [0, m). */
int ital_gp_preview_remove(const ital_influence_desc* desc, const int* sel, int r, double* mu_out, double* s2_out, int64_t ldo,
                           hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_INFLUENCE_H */
