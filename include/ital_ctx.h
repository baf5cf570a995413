/*
 * Context layer of libital_hip.so, beyond the perfect user: user models, caller-given candidate lists with a
 * change-estimation subset, MCMI_min, top_results and predict at external points.  A learner whose device buffers the
 * LIBRARY owns (see the context section of ital_hip.h for create / fit / update / fetch / predict_stored); everything below is
 * host code over the descriptor entry points of this same library (csrc/ctx.hip).  Return values: 0, a count, or a negative
 * errno-style code with its message in ital_last_error; every call here synchronises `stream` (its results are host data).
 *
 * Codes shared by the entry points below:
 *   -22  bad arguments: a labelled, repeated or out-of-range sample in a list; no label given yet; k outside its range
 *   -95  a configuration the device scorers do not cover (the message names it as ITAL._unsupported does in Python)
 *   -61  fetch_list: k larger than the list -- the steps the reference runs are run, then "attempt to get argmax of an
 *        empty sequence" (reference ital/ital.py:130)
 *   -38  MCMI_min on several ranks (its objective needs an all-reduce; the context exchanges records only)
 *   -33  kernel matrix not positive definite / singular conditional covariance in the orthant integrator
 */
#ifndef ITAL_CTX_H
#define ITAL_CTX_H

#include "ital_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The user model of reference ITAL.__init__ (ital/ital.py:15-81).  The defaults are the perfect user. */
typedef struct ital_ctx_model {
    double label_prob;        /* ITAL(label_prob=1.0): probability that the user labels a shown sample at all */
    double mistake_prob;      /* ITAL(mistake_prob=0.0): probability that a given label is wrong */
    int label_estimation;     /* 0 'mean', 1 'optimistic', 2 'pessimistic' (as ital_gscore_desc.label_mode) */
    int monte_carlo_num_rel;  /* 0 = None; anything else is -95 (sampling on numpy's generator is not in the context) */
    int monte_carlo_num_fb;   /* 0 = None; anything else is -95 */
    double clip_cov;          /* 0; a value inside (0, 1) is -95 */
} ital_ctx_model;

/* Sets the user model.  Once set (the perfect user included), ital_ctx_fetch follows ITAL._select: the perfect user on the
 * lattice scorer, its rounds with duplicate samples or large noise redone through the general scorer from the same stream
 * position; every other model on the general scorer.  A context without a model keeps the perfect-user layer of ital_hip.h
 * (-71 for such rounds, k <= ITAL_MAX_T).  -95 for the Monte-Carlo switches, clip_cov inside (0, 1) and an unknown
 * label_estimation (the model is then left as it was). */
int ital_ctx_set_model(ital_ctx* ctx, const ital_ctx_model* model);

/* fetch_unlabelled(k) over a caller-given candidate list, in the reference's order: cand[0 .. n_cand) global sample
 * indices (host memory), or NULL for all unlabelled samples in ascending order (what top_candidates and the reference's
 * argpartition would otherwise choose, reference ital/ital.py:98-117).  n_subset > 0: change-estimation subset mode with
 * ce_subset[0 .. n_subset) as the subset (change_estimation_subset=None: the list itself, at most ITAL_GENERIC_MAX_DIM).
 * Several ranks pass the same global list.  picks[0 .. k) <- the batch; returns the number of picks (k clamped to the
 * unlabelled samples) or a negative code.  Uses the model of ital_ctx_set_model (the perfect user when none was set). */
int ital_ctx_fetch_list(ital_ctx* ctx, int k, const int64_t* cand, int64_t n_cand, const int64_t* ce_subset, int n_subset,
                        int64_t* picks, hipStream_t stream);

/* MCMI_min.fetch_unlabelled(k) on one rank (reference ital/mcmi.py:48-81): cand[0 .. n_cand) the candidate subsample in draw
 * order, NULL for all unlabelled samples ascending.  k clamped to the list; picks[0 .. k) <- the batch.  -95 for
 * k > ITAL_MAX_T, -38 on several ranks.  ital_ctx_update of the picks works afterwards as after ital_ctx_fetch. */
int ital_ctx_mcmi_fetch(ital_ctx* ctx, int k, const int64_t* cand, int64_t n_cand, int64_t* picks, hipStream_t stream);

/* idx[0 .. k) <- the k samples of largest predictive mean, np.argsort(rel_mean)[::-1][:k] (NaN first, ties by descending
 * index; reference ital/retrieval_base.py:64-75).  Several ranks: every rank returns the same list.  -22 before the first
 * label and for k outside 1 .. min(ITAL_TOPK_MAX, n_total). */
int ital_ctx_top_results(ital_ctx* ctx, int k, int64_t* idx, hipStream_t stream);

/* Predictive mean and variance at nt external points Xt [nt][d] (host memory); mean / variance: nt doubles of host memory,
 * either may be NULL; the variance clamped at 0 (reference gp.predict(X, cov_mode='diag'), ital/gp.py:264-292).  -22
 * before the first label. */
int ital_ctx_predict(ital_ctx* ctx, const double* Xt, int64_t nt, double* mean, double* variance, hipStream_t stream);

/* Takes the labels of idx[0 .. c) back (global sample indices, host memory): each leaves the labelled set by a Cholesky row
 * deletion and one sweep over the whitened block (ital_gp_remove, ital_revoke.h), highest labelled position first, and is a
 * candidate again afterwards; ital_ctx_update may then label it anew.  What the reference refuses (RuntimeError 'Cannot
 * change feedback once given.', reference ital/retrieval_base.py:183-189) and could only undo by a fit from scratch on the
 * surviving labels (reference ital/gp.py:141-161).  The context remembers the insertion order of its labelled samples for
 * this.  Several ranks make the same call (no exchange: factor and labels are replicated, every rank sweeps its own
 * columns).  -22 for a NULL context or list, c < 1, a sample that has no label, a sample named twice; nothing is changed
 * then. */
int ital_ctx_revoke(ital_ctx* ctx, const int64_t* idx, int c, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_CTX_H */
