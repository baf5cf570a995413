/*
 * The closed-form leave-one-out scores of many kernel hyper-parameter candidates AND their gradients in the logarithms of the
 * three parameters (ital_amd GaussianProcess.loo_grad, tune.fit_session_params(criterion='loo_logp' / 'loo_mse'),
 * ActiveRetrievalBase.fit_params; csrc/loo_grad.hip).  For candidate g with theta_g = (l, var, noise), and D, K, L, alpha,
 * c_i = (K^-1)_ii, Kf and W = K^-1 as defined in ital_evidence.h and ital_evidence_grad.h, let A = dK / d log theta:
 *
 *     A_l = Kf o D / l^2          A_var = Kf          A_noise = noise I
 *     P = W A,    r = P alpha,    s_i = (P W)_ii = sum_j P_ij W_ji
 *
 *     loo_logp, loo_mse           as ital_gp_evidence's scores[g][1] and scores[g][2], bit for bit: the same code forms them
 *     d loo_logp / d log theta = sum_i [ alpha_i r_i - 1/2 (1 + alpha_i^2 / c_i) s_i ] / c_i                    (R&W 5.13)
 *     d loo_mse  / d log theta = (2 / m) sum_i (alpha_i / c_i) (alpha_i s_i / c_i - r_i) / c_i
 *
 * For A_noise the products collapse to row sums, r = noise W alpha and s_i = noise sum_j W_ij^2.  For A_l and A_var P is
 * formed as a product on v_mfma_f64_16x16x4_f64, both through the same kernel and epilogue (the identity W Kf = I - noise W
 * cancels when the noise dominates and is not used); Kf is recomputed from the stored D as var exp(D / (-2 l^2)).
 *
 * The workspace is ital_gp_evidence's, followed by D, the stored lower triangles of W, the product's partial row sums and
 * the rows' r and s; the first five stages are the host function ital_gp_evidence runs (csrc/evidence_chain.h).
 *
 * Every sum runs in a fixed order and no kernel uses atomics or lets one matrix see another: a candidate gets the same bits
 * alone or in any batch, at any position.  Conventions as in ital_evidence.h: borrowed device pointers, asynchronous on
 * `stream`, 0 or a negative errno-style code with its message in ital_last_error, argument checks before any HIP call, no
 * allocation across the ABI.  Matrices are row-major; of K only the lower triangle (j <= i < m) is read or written.
 */
#ifndef ITAL_LOO_GRAD_H
#define ITAL_LOO_GRAD_H

#include "ital_evidence_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ital_loo_grad_desc {
    const double* XT;       /* [m][ldx] feature rows of the labelled samples, zero padded to ldx */
    const double* XTn;      /* [m] their squared norms */
    int ldx;                /* multiple of 16 */
    const double* y;        /* [m] targets */
    int m;                  /* labelled samples, >= 1 */
    const double* params;   /* [G][3] (length_scale, var, noise), device memory */
    int G;                  /* candidates of this call, 1 .. 65535 */
    double* K;              /* [G][m][ld] scratch: the Grams, then their factors */
    int64_t ld;             /* >= m */
    double* values;         /* out [G][2]: loo_logp, loo_mse, the bits of ital_gp_evidence's scores[g][1] and scores[g][2] */
    double* grad;           /* out [G][2][3]: d loo_logp, then d loo_mse / d log l, d log var, d log noise */
    int* info;              /* out [G]: 0, or column + 1 of the first pivot that is not > 0 (ital_chol_batched) */
    int* status;            /* |= 1 when a candidate's Gram is not positive definite */
    double* work;           /* ital_gp_loo_grad_workspace(m, G) doubles */
    int64_t work_doubles;
    void* const* ev;        /* NULL, or 9 hipEvent_t (host array): recorded before the first stage and after each of the eight */
} ital_loo_grad_desc;

/* The whole chain for G candidates: setup, then eight stages -- Gram grid, ital_chol_batched, ital_chol_solve_batched,
 * ital_chol_inv_diag_batched (which leaves M in `work`), the shared squared distances, the stored lower triangles of W
 * (the kernel of ital_chol_gram_inverse_batched), the product P = W A for A = Kf o D and A = Kf (all 128 x 128 tiles of P,
 * the symmetric operands read mirrored from their lower triangles; no tile of P is stored: per tile row the epilogue sums
 * P_ij alpha_j and P_ij W_ij over the tile's columns in a fixed order), and one workgroup per candidate that adds the
 * partials in ascending column-tile order, forms the noise row sums and closes every sum over the samples, i ascending.
 * The number of launches depends on m alone, never on G.  A candidate whose Gram is not positive definite in floating point
 * has info[g] != 0, values[g] = (-inf, +inf), NaN in grad[g] and sets *status |= 1; the other candidates are unaffected.
 * -22: a NULL descriptor or pointer, ldx not a positive multiple of 16, ld < m, m < 1, G < 1 or > 65535, work smaller than
 * ital_gp_loo_grad_workspace(m, G). */
int ital_gp_loo_grad(const ital_loo_grad_desc* desc, hipStream_t stream);

/* Doubles of `work` for ital_gp_loo_grad (0 for m < 1 or G < 1). */
int64_t ital_gp_loo_grad_workspace(int m, int G);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_LOO_GRAD_H */
