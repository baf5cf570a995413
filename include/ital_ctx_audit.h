/*
 * Auditing the labels of a live session in a library-owned context (ital_ctx.h; csrc/ctx_audit.hip): which of them deserve a
 * second look and what taking each of them back would change, without touching the context.  Host code over
 * ital_gp_influence of ital_influence.h, what ital_amd's ActiveRetrievalBase.audit does in Python.  Conventions of
 * ital_ctx_live.h: the call synchronises `stream` before it returns, returns 0 or a negative errno-style code with its message
 * in ital_last_error, checks its arguments before any HIP call and leaves the context exactly as it was, whatever it returns.
 */
#ifndef ITAL_CTX_AUDIT_H
#define ITAL_CTX_AUDIT_H

#include "ital_ctx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* All pointers are host memory.  For the m labelled samples in insertion order (*count = m; give room for the capacity):
 * ids [m] and table [m][8] = label, loo_mean, loo_var (the prediction for the sample from all the other labels, R&W 5.12),
 * disagreement = ndtr(-label loo_mean / sqrt(loo_var)), dmu_rms, dmu_max, flips, ds2: root mean square and maximum of the
 * change of the predictive mean, number of rows whose mean changes sign and total variance the label removes, over the
 * samples without a label (unseen_only != 0) or over all of them.  A label whose diagonal entry of K^-1 is not positive and
 * finite has NaN in columns 1 .. 7.  -22 before the first label and for a NULL pointer; -38 on several ranks (the per-rank
 * tables are not exchanged); -12 out of device memory; -5 a HIP copy or the stream failed. */
int ital_ctx_audit(ital_ctx* ctx, int unseen_only, int64_t* ids, double* table, int* count, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_CTX_AUDIT_H */
