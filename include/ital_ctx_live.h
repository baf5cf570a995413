/*
 * A live session in a library-owned context (ital_ctx.h, ital_hip.h; csrc/ctx_live.hip): the labelled-set capacity grows,
 * data rows arrive and leave, the kernel hyper-parameters change and candidates for them are scored against the session's
 * own labels -- in place, by device-to-device copies and one whitening pass, without a new context, a second upload of the
 * rows or a replay of the labels.  What ital_amd's Python learners do in add_data / remove_data / set_params / tune_params
 * (ital_amd/gp.py: extend, drop_rows, set_params, evidence), as host code over the descriptor entry points of this same
 * library (ital_whiten_rows, ital_compact_rows, ital_compact_cols, ital_gp_remove, ital_chol_append, ital_gp_evidence).  The
 * reference has none of this: its dense K_all (reference ital/gp.py:128) is built once.
 *
 * Every call synchronises `stream` before it returns and returns 0 or a negative errno-style code with its message in
 * ital_last_error.  Arguments are checked before any HIP call.  A call that fails leaves the context exactly as it was: the
 * new state is built in fresh buffers and swapped in once it is known to be good; the old buffers are given back after the
 * stream has drained.
 *
 * Codes shared by the entry points below:
 *   -22  bad arguments: a NULL context, a context without ital_ctx_fit, and what each entry point names
 *   -12  out of device memory (nothing changed)
 *   -38  rows arriving or leaving on several ranks: row sharding cannot grow or shrink
 *   -33  ital_ctx_set_params: the kernel matrix of the labelled samples is not positive definite with these parameters
 *    -5  a HIP copy or the stream failed
 *
 * Limits: FP64 rows only; rows arrive and leave on one rank only; a context holds no external queries.
 */
#ifndef ITAL_CTX_LIVE_H
#define ITAL_CTX_LIVE_H

#include "ital_ctx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Raises the labelled-set capacity (ital_ctx_create: capacity) to `capacity` rounded up to a multiple of 16; a value not
 * above the current capacity is a no-op.  The factor is re-strided to its new leading dimension, the feature rows and
 * labels of the labelled samples, the whitened block, the batch state of the last fetch and the selection records follow.
 * ital_ctx_update, which returns -12 at the capacity, has room again afterwards.  -22 for a capacity above 2^20.  Several
 * ranks make the same call; nothing is exchanged. */
int ital_ctx_reserve(ital_ctx* ctx, int capacity, hipStream_t stream);

/* Appends k samples: rows [k][d] with leading dimension d, host memory, or device memory when on_device != 0 (as
 * ital_ctx_fit).  They get the indices n_total .. n_total + k - 1 and are unlabelled.  The feature rows, their norms, the
 * whitened block (with its new leading dimension), the means and the variances grow by device-to-device copies; the new
 * range alone is whitened against the labelled set, in one ital_whiten_rows call: by that call's DEFINITION the new rows
 * get the bits a context created on all rows gives them after the same ital_ctx_update calls.  The batch of the last fetch
 * is forgotten; the position in mvndst's random stream stays.  k == 0 returns 0.  -22 for k < 0 or rows == NULL, -38 on
 * several ranks. */
int ital_ctx_add_rows(ital_ctx* ctx, const double* rows, int64_t k, int on_device, hipStream_t stream);

/* Deletes the c samples idx[0 .. c) (host memory), like np.delete(X, idx, axis=0): the survivors keep their order and get
 * the indices 0 .. n_total - c - 1.  The labelled ones among them first leave the model as ital_ctx_revoke takes them out,
 * highest labelled position first; what is left is a gather without arithmetic (ital_compact_rows, ital_compact_cols): no
 * bit of a survivor changes.  index_map: NULL, or n_total (before the call) entries of host memory that receive the new
 * index of each old sample, -1 for a deleted one.  The batch of the last fetch is forgotten.  -22 for idx == NULL, c < 1, an
 * index outside the data, an index named twice, c == n_total (no row would be left) and a gather that flagged an index;
 * -38 on several ranks. */
int ital_ctx_remove_rows(ital_ctx* ctx, const int64_t* idx, int64_t c, int64_t* index_map, hipStream_t stream);

/* Other kernel hyper-parameters; a NaN argument keeps the current value.  Before the first label only the prior variance
 * changes.  Otherwise the factor and alpha are built anew in fresh buffers from the stored feature rows and the remembered
 * labels (ital_chol_append in blocks of 16 from position 0); if that Gram is positive definite they are swapped in and every
 * local row is whitened again in one ital_whiten_rows call: the state of a context created with these parameters and given
 * the labels in this context's insertion order in one ital_ctx_update call.  -22 for length_scale <= 0, var <= 0 or
 * noise < 0 (after the substitution), -33 when the Gram is not positive definite.  Several ranks make the same call; nothing
 * is exchanged. */
int ital_ctx_set_params(ital_ctx* ctx, double length_scale, double var, double noise, hipStream_t stream);

/* Scores G hyper-parameter candidates against the context's own labelled samples without touching its state
 * (ital_gp_evidence, ital_evidence.h).  All pointers are host memory.  params [G][3]: length_scale, var, noise;
 * scores [G][3]: lml, loo_logp, loo_mse; ok [G]: 1 where the candidate's Gram was positive definite (otherwise -inf, -inf,
 * +inf).  The candidates go to the device in chunks whose Grams, workspace and outputs stay below 1 GiB; a candidate's values
 * do not depend on the chunking.  -22 before the first label, for G < 1 and for a NULL pointer; -12 when one candidate alone
 * exceeds 1 GiB.  With ital_ctx_set_params this is a grid search: score the grid, apply the best candidate. */
int ital_ctx_evidence(ital_ctx* ctx, const double* params, int G, double* scores, int* ok, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_CTX_LIVE_H */
