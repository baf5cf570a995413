/*
 * Taking a label back (ital_amd GaussianProcess.remove, ActiveRetrievalBase.revoke / relabel; csrc/revoke.hip): one
 * labelled sample leaves the Cholesky-whitened GP state by a row deletion of the factor and one orthogonal sweep over the
 * whitened block.  Conventions as in ital_dense.h: borrowed device pointers, asynchronous on `stream`, 0 or a negative
 * errno-style code with its message in ital_last_error, argument checks before any HIP call, no allocation across the ABI.
 */
#ifndef ITAL_REVOKE_H
#define ITAL_REVOKE_H

#include "ital_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The GP state of ital_append_desc, and which labelled position leaves it. */
typedef struct ital_remove_desc {
    double* XT;           /* [>= m][ldx] feature rows of the labelled samples; rows p+1 .. m-1 move up, row m-1 <- 0 */
    double* XTn;          /* [>= m] their squared norms, moved alike */
    int ldx;
    double* L;            /* lower Cholesky factor of K_TT + noise I, row-major, leading dimension ldl >= m */
    int ldl;
    double* alpha;        /* [>= m] L^-1 y */
    double* V;            /* [>= m][ldv] whitened block L^-1 K_T,: of this rank's n columns (may be NULL when n == 0) */
    int64_t ldv;          /* >= n, even (ital_amd: n padded to 16); the pad columns are swept too and stay finite */
    int64_t n;
    double* mu;           /* [n] V^T alpha */
    double* s2;           /* [n] var - colsum(V^2), not clamped */
    int m;                /* labelled samples before the call */
    int p;                /* position (insertion order) of the one that leaves, 0 <= p < m */
    double* work;         /* ital_gp_remove_workspace(m) doubles, 16-byte aligned: rotation coefficients, the left-over
                             component of alpha, the compacted factor before it is written back */
    int64_t work_doubles;
    int* status;          /* bit 1 is set if a rotation met a non-positive or non-finite pivot (a factor that was broken before) */
} ital_remove_desc;

/* Removes labelled position p from (L, alpha, V, mu, s2, XT, XTn): afterwards they are what m - 1 appends of the surviving
 * samples in their order give, up to rounding -- L without row p is brought back to lower triangular form with a positive
 * diagonal by Givens rotations G_q of the column pairs (q, q + 1), q = p .. m-2 (the rank-one UPDATE
 * L33' L33'^T = L33 L33^T + l32 l32^T of the trailing block), V' = (G^T V)[0 : m-1] with w the row that is left over,
 * alpha' = (G^T alpha)[0 : m-1] with a_last left over, mu' = mu - w a_last, s2' = s2 + w^2.  Row m-1 of L, V and XT and entry
 * m-1 of alpha and XTn are zero afterwards.  Two launches: the factor (one workgroup) and the sweep over V (in place, p = m-1
 * needs no rotation).  Several ranks: L, alpha, XT are replicated and V is column-sharded, every rank makes the same call
 * with its own columns.
 *
 * Stands in for what the reference cannot do: a label, once given, stays (RuntimeError 'Cannot change feedback once given.',
 * reference ital/retrieval_base.py:183-189), so its only way back is a fit from scratch on the survivors
 * (reference ital/gp.py:141-161).  -22: a NULL descriptor or buffer, m <= 0, p outside [0, m), ldl < m, ldv < n or odd,
 * ldx < 1, a workspace smaller than ital_gp_remove_workspace(m). */
int ital_gp_remove(const ital_remove_desc* desc, hipStream_t stream);

/* Doubles of `work` for a labelled set of m samples (0 for m <= 0). */
int64_t ital_gp_remove_workspace(int m);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_REVOKE_H */
