/*
 * The log marginal likelihood of many kernel hyper-parameter candidates AND its gradient in the logarithms of the three
 * parameters (ital_amd GaussianProcess.evidence_grad, tune.maximize_lml / fit_session_params,
 * ActiveRetrievalBase.fit_params; csrc/evidence_grad.hip).  For candidate g with theta_g = (l, var, noise), and D, K, L,
 * alpha, c_i = (K^-1)_ii as defined in ital_evidence.h, let Kf = var exp(D / (-2 l^2)) (K without its noise) and W = K^-1:
 *
 *     lml        as ital_gp_evidence, bit for bit: the same code forms it                                (R&W 2.30)
 *     g_logl     = 1/2 sum_ij (alpha_i alpha_j - W_ij) Kf_ij D_ij / l^2           d lml / d log l        (R&W 5.9)
 *     g_logvar   = 1/2 sum_ij (alpha_i alpha_j - W_ij) Kf_ij                      d lml / d log var
 *     g_lognoise = 1/2 noise (alpha.alpha - sum_i c_i)                            d lml / d log noise
 *
 * W = M^T M with M = L^-1, the inverse factor that ital_chol_inv_diag_batched leaves in its workspace: matrix g at
 * work + g n n, row-major [j][i] with row stride n, lower triangle (i <= j) only -- the rest of that workspace is unwritten
 * memory and is never read here.  ital_gp_evidence_grad depends on that layout, and cannot drift from it: its workspace is
 * ital_gp_evidence's, followed by D and the partials, and its first five stages are the host function ital_gp_evidence
 * runs (csrc/evidence_chain.h), so it reads M where that function's last launch wrote it.
 *
 * Every sum runs in a fixed order and no kernel uses atomics or lets one matrix see another: a candidate gets the same bits
 * alone or in any batch, at any position.  Conventions as in ital_evidence.h: borrowed device pointers, asynchronous on
 * `stream`, 0 or a negative errno-style code with its message in ital_last_error, argument checks before any HIP call, no
 * allocation across the ABI.  Matrices are row-major; only the lower triangle (j <= i < m) is read or written.
 */
#ifndef ITAL_EVIDENCE_GRAD_H
#define ITAL_EVIDENCE_GRAD_H

#include "ital_evidence.h"

#ifdef __cplusplus
extern "C" {
#endif

/* D[i][j] = |x_i|^2 + |x_j|^2 - 2 x_i . x_j, j <= i < m (not clamped), row stride ld: the squared distances that every
 * candidate of ital_gram_grid shares, from the same 128 x 128 v_mfma_f64_16x16x4_f64 tile in the same accumulation order,
 * so that var exp(D_ij / (-2 l^2)) recomputed from it has the bits of the Gram's entry.
 * -22: a NULL pointer, ldx not a positive multiple of 16, ld < m, m < 1. */
int ital_sqdist_lower(const double* XT, const double* XTn, int m, int ldx, double* D, int64_t ld, hipStream_t stream);

/* W[g][i][j] = sum_{k >= i} M_g[k][i] M_g[k][j], j <= i < n (k ascending): the lower triangle of K_g^-1 = M_g^T M_g from
 * `count` inverse factors in the layout above (M_g at M + g n n); W_g starts at W + g n ldw.  One 128 x 128 tile pair per
 * workgroup on v_mfma_f64_16x16x4_f64, both operands read k-major behind predicates: nothing above the diagonal of M is
 * read.  A matrix with info[g] != 0 (info may be NULL) is skipped and its lower triangle gets NaN.  count <= 65535.
 * -22: a NULL pointer, n < 1, count < 1 or > 65535, ldw < n. */
int ital_chol_gram_inverse_batched(const double* M, int n, int count, const int* info, double* W, int64_t ldw,
                                   hipStream_t stream);

typedef struct ital_evidence_grad_desc {
    const double* XT;       /* [m][ldx] feature rows of the labelled samples, zero padded to ldx */
    const double* XTn;      /* [m] their squared norms */
    int ldx;                /* multiple of 16 */
    const double* y;        /* [m] targets */
    int m;                  /* labelled samples, >= 1 */
    const double* params;   /* [G][3] (length_scale, var, noise), device memory */
    int G;                  /* candidates of this call, 1 .. 65535 */
    double* K;              /* [G][m][ld] scratch: the Grams, then their factors */
    int64_t ld;             /* >= m */
    double* values;         /* out [G]: lml, the bits of ital_gp_evidence's scores[g][0] */
    double* grad;           /* out [G][3]: d lml / d log l, d log var, d log noise */
    int* info;              /* out [G]: 0, or column + 1 of the first pivot that is not > 0 (ital_chol_batched) */
    int* status;            /* |= 1 when a candidate's Gram is not positive definite */
    double* work;           /* ital_gp_evidence_grad_workspace(m, G) doubles */
    int64_t work_doubles;
    void* const* ev;        /* NULL, or 8 hipEvent_t (host array): recorded before the first stage and after each of the seven */
} ital_evidence_grad_desc;

/* The whole chain for G candidates: setup, then seven stages -- Gram grid, ital_chol_batched, ital_chol_solve_batched,
 * ital_chol_inv_diag_batched (which leaves M in `work`), the shared squared distances, the fused product (each 128 x 128
 * tile of W in the MFMA accumulators; (alpha_i alpha_j - W_ij) Kf_ij and the same times D_ij summed over the tile's lower
 * elements, strictly lower ones twice, in a fixed order inside the workgroup: one pair of partials per tile pair; W itself is
 * never stored), and one workgroup per candidate that adds the partials in ascending tile order and forms lml and the three
 * components.  The number of launches depends on m alone, never on G.  A candidate whose Gram is not positive definite in
 * floating point has info[g] != 0, values[g] = -inf, NaN in grad[g] and sets *status |= 1; the other candidates are
 * unaffected.
 * -22: a NULL descriptor or pointer, ldx not a positive multiple of 16, ld < m, m < 1, G < 1 or > 65535, work smaller than
 * ital_gp_evidence_grad_workspace(m, G). */
int ital_gp_evidence_grad(const ital_evidence_grad_desc* desc, hipStream_t stream);

/* Doubles of `work` for ital_gp_evidence_grad (0 for m < 1 or G < 1). */
int64_t ital_gp_evidence_grad_workspace(int m, int G);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_EVIDENCE_GRAD_H */
