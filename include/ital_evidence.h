/*
 * Scoring many kernel hyper-parameter candidates against a session's own labels (ital_amd GaussianProcess.evidence,
 * tune.session_scores / optimize_session_params, ActiveRetrievalBase.tune_params; csrc/evidence.hip): for each candidate
 * theta_g = (length_scale_g, var_g, noise_g), g < G, over the m labelled rows XT with targets y, all in FP64,
 *
 *     D_ij  = |x_i|^2 + |x_j|^2 - 2 x_i . x_j                      (not clamped; the expansion of ital_gram_rows)
 *     K_g   = var_g exp(D / (-2 l_g^2)) + noise_g I = L L^T
 *     alpha = K_g^-1 y,    c_i = (K_g^-1)_ii = sum_{j >= i} (L^-1)[j][i]^2
 *     lml        = -1/2 y.alpha - sum_i log L_ii - (m/2) log(2 pi)                                   (R&W 2.30)
 *     loo_mean_i = y_i - alpha_i / c_i,   loo_var_i = 1 / c_i  (variance of the noisy target)        (R&W 5.12)
 *     loo_logp   = sum_i [ -1/2 log loo_var_i - (y_i - loo_mean_i)^2 / (2 loo_var_i) - 1/2 log(2 pi) ]  (R&W 5.10)
 *     loo_mse    = mean_i (alpha_i / c_i)^2
 *
 * Every sum runs in a fixed order, i (or k, j) ascending; a candidate gets the same bits alone or in any batch, at any
 * position.  Conventions as in ital_dense.h: borrowed device pointers, asynchronous on `stream`, 0 or a negative errno-style
 * code with its message in ital_last_error, argument checks before any HIP call, no allocation across the ABI.  Matrices are
 * row-major; only the lower triangle (j <= i < m) is read or written.
 */
#ifndef ITAL_EVIDENCE_H
#define ITAL_EVIDENCE_H

#include "ital_dense.h"

#ifdef __cplusplus
extern "C" {
#endif

/* K[g][i][j] = var_g exp(D_ij / (-2 l_g^2)) + noise_g (i == j), j <= i < m, for g < G: matrix g starts at K + g * m * ld.
 * params: [G][3] in DEVICE memory, (length_scale, var, noise) per candidate.  The feature dot products of a 128 x 128 tile
 * are formed once on v_mfma_f64_16x16x4_f64 and serve every candidate of the workgroup's group (grid: lower tile pairs x
 * groups of candidates); what G calls of ital_gram_rows recompute G times.
 * -22: a NULL pointer, ldx not a positive multiple of 16, ld < m, m < 1, G < 1. */
int ital_gram_grid(const double* XT, const double* XTn, int m, int ldx, const double* params, int G, double* K, int64_t ld,
                   hipStream_t stream);

/* out[g * ldo + i] = (K_g^-1)_ii = sum_{j >= i} M[j][i]^2, M = L_g^-1, from `count` lower factors of equal n with their own
 * pointers: L[g] and ld[g] are arrays in DEVICE memory (as ital_chol_batched takes them).  One workgroup per matrix,
 * row by row: M_jj = 1 / L_jj, M[j][i] = -(sum_{k=i}^{j-1} L[j][k] M[k][i]) / L_jj, k ascending, then the column sums, j
 * ascending.  A matrix with info[g] != 0 (info may be NULL) is skipped and gets NaN.  Any n >= 1.
 * work: ital_chol_inv_diag_batched_workspace(n, count) doubles (M of every matrix).
 * -22: a NULL pointer, n < 1, count < 1, ldo < n, work too small. */
int ital_chol_inv_diag_batched(const double* const* L, const int64_t* ld, int n, int count, const int* info, double* out,
                               int64_t ldo, double* work, int64_t work_doubles, hipStream_t stream);
int64_t ital_chol_inv_diag_batched_workspace(int n, int count);

typedef struct ital_evidence_desc {
    const double* XT;       /* [m][ldx] feature rows of the labelled samples, zero padded to ldx */
    const double* XTn;      /* [m] their squared norms */
    int ldx;                /* multiple of 16 */
    const double* y;        /* [m] targets */
    int m;                  /* labelled samples, >= 1 */
    const double* params;   /* [G][3] (length_scale, var, noise), device memory */
    int G;                  /* candidates of this call, 1 .. 65535 */
    double* K;              /* [G][m][ld] scratch: the Grams, then their factors */
    int64_t ld;             /* >= m */
    double* scores;         /* out [G][3]: lml, loo_logp, loo_mse */
    int* info;              /* out [G]: 0, or column + 1 of the first pivot that is not > 0 (ital_chol_batched) */
    double* loo_mean;       /* out [G][ldm] */
    double* loo_var;        /* out [G][ldm] */
    int64_t ldm;            /* >= m */
    int* status;            /* |= 1 when a candidate's Gram is not positive definite */
    double* work;           /* ital_gp_evidence_workspace(m, G) doubles */
    int64_t work_doubles;
    void* const* ev;        /* NULL, or 6 hipEvent_t (host array): recorded before the first stage and after each of the five */
} ital_evidence_desc;

/* The whole chain for G candidates: Gram grid, ital_chol_batched, ital_chol_solve_batched, inverse diagonals, one reduction
 * kernel.  The pointer, size and leading-dimension arrays of the batched calls are built on the device in `work`; the number
 * of launches depends on m alone, never on G.  A candidate whose Gram is not positive definite in floating point has
 * info[g] != 0, lml = loo_logp = -inf, loo_mse = +inf, loo_mean = loo_var = NaN and sets *status |= 1; the other candidates
 * are unaffected.
 * -22: a NULL descriptor or pointer, ldx not a positive multiple of 16, ld < m, ldm < m, m < 1, G < 1 or > 65535, work
 * smaller than ital_gp_evidence_workspace(m, G). */
int ital_gp_evidence(const ital_evidence_desc* desc, hipStream_t stream);

/* Doubles of `work` for ital_gp_evidence (0 for m < 1 or G < 1). */
int64_t ital_gp_evidence_workspace(int m, int G);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_EVIDENCE_H */
