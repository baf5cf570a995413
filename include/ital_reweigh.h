/*
 * Trusting a label less without taking it back (ital_amd GaussianProcess.reweigh, ActiveRetrievalBase.set_label_noise;
 * csrc/reweigh.hip): the diagonal entry K_pp of the labelled Gram changes by delta, which is a rank-one update
 * (delta > 0) or downdate (delta < 0) of the trailing block of the Cholesky factor with the vector sqrt(|delta|) e_p, and
 * one streaming pass over the whitened block for up to eight such labels together.  Conventions as in ital_revoke.h:
 * borrowed device pointers, asynchronous on `stream`, 0 or a negative errno-style code with its message in
 * ital_last_error, argument checks before any HIP call, no allocation across the ABI.
 *
 * The C context layer (ital_ctx_*) does not offer this call yet: a context keeps one scalar noise.
 */
#ifndef ITAL_REWEIGH_H
#define ITAL_REWEIGH_H

#include "ital_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Labels in one sweep over V (the carries a lane holds per column); a call with more runs ceil(r / 8) sweeps. */
#define ITAL_REWEIGH_PASS 8

/* The GP state of ital_remove_desc without the feature rows (none is read), and which diagonal entries change by how much. */
typedef struct ital_reweigh_desc {
    double* L;            /* lower Cholesky factor of K_TT + noise I + diag(e), row-major, leading dimension ldl >= m */
    int ldl;
    double* alpha;        /* [>= m] L^-1 y */
    double* V;            /* [>= m][ldv] whitened block L^-1 K_T,: of this rank's n columns; NULL with n == 0: factor only */
    int64_t ldv;          /* >= n, even (ital_amd: n padded to 16); the pad columns are swept too and stay finite */
    int64_t n;
    double* mu;           /* [n] V^T alpha */
    double* s2;           /* [n] var - colsum(V^2), not clamped */
    int m;                /* labelled samples */
    double* work;         /* ital_gp_reweigh_workspace(m, r) doubles, 16-byte aligned: the "refused" word, the rotation
                             coefficients of every (label, row), the carries, the new trailing block before it is written back */
    int64_t work_doubles;
    int* status;          /* bit 1 is set if a pivot of any chain was not positive and finite: the call was refused */
    int r;                /* labels whose diagonal entry changes, >= 1 */
    const int* pos;       /* [r] their labelled positions, strictly increasing, in [0, m): a HOST array, read before the call
                             returns */
    const double* delta;  /* [r] signed change of K_pp per position (finite; 0 is the identity): a HOST array likewise */
} ital_reweigh_desc;

/* (L, alpha, V, mu, s2) <- the state of the Gram with K_pp + delta_j at every listed position p = pos[j], up to rounding.
 * Per label a chain of rotations k = p .. m-1 with x = sqrt(|delta|) e_p, top-down:
 *   update   (delta > 0):  r = hypot(L_kk, x_k)
 *   downdate (delta < 0):  r = sqrt((L_kk - x_k)(L_kk + x_k))     (the mixed form of Bojanczyk, Brent, Van Dooren, de Hoog)
 *   c = r / L_kk, s = x_k / L_kk, L_kk <- r;  rows i > k:  L_ik <- (L_ik +- s x_i) / c,  x_i <- c x_i - s L_ik
 * and the same recurrence down alpha and down every column of V with a carry u that starts at 0; what is left in the carries
 * corrects the means and variances: mu' = mu -+ u a_u, s2' = s2 +- u^2 (upper sign: update).  Rows < pos[0] of L and V are
 * not touched; no feature row is read.  The chains run one after the other on the factor (chain j sees what chains < j left)
 * and together, at most ITAL_REWEIGH_PASS at a time, in one pass over rows pos[0] .. m-1 of V.
 *
 * Refusal: if any pivot of any chain is not positive and finite (a downdate that would leave the Gram indefinite), bit 1 of
 * *status is set and NOTHING on the device changes -- the factor is built in `work` and written back only after the last
 * chain, and every sweep first reads the "refused" word the factor kernels left in `work`.  No host round trip in between.
 *
 * Launches: ceil(r / 8) factor kernels (one workgroup each), then, if n > 0, ceil(r / 8) sweeps.  Several ranks: L and alpha
 * are replicated and V is column-sharded, every rank makes the same call with its own columns.
 *
 * -22: a NULL descriptor or buffer (V, mu, s2 may be NULL only with n == 0), m <= 0, r < 1, ldl < m, ldv < n or odd, pos not
 * strictly increasing inside [0, m), a non-finite delta, a workspace smaller than ital_gp_reweigh_workspace(m, r) or not
 * 16-byte aligned. */
int ital_gp_reweigh(const ital_reweigh_desc* desc, hipStream_t stream);

/* Doubles of `work` for r labels of a labelled set of m samples (0 for m <= 0 or r <= 0). */
int64_t ital_gp_reweigh_workspace(int m, int r);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_REWEIGH_H */
