/*
 * Feature rows kept on the device in their SOURCE precision (ital_amd DeviceData(storage="source")): every entry point that
 * reads whole rows of the data matrix X, with the element type of X as an argument.  Conventions as in ital_dense.h:
 * borrowed device pointers, asynchronous on `stream`, 0 or a negative errno-style code with its message in ital_last_error,
 * argument checks before any HIP call, no allocation across the ABI.
 *
 * X is [n][ldx] of the element type `xtype` (the ITAL_INGEST_* codes of ital_ingest.h: f64, f32, f16, bf16), ldx a multiple
 * of 16 ELEMENTS, pad columns +0, the matrix aligned to 16 B.  xnorm stays FP64 and holds what ital_row_norms gives on the
 * rows widened to FP64.  Everything else -- selected rows, labelled rows, V, records, batch state, every output -- is FP64
 * exactly as in the entry point of the same name without the suffix.
 *
 * DEFINITION: each ital_NAME_t(..., xtype, stream) computes, bit for bit, what ital_NAME(..., stream) computes on the matrix
 * (double)X.  The widening conversion is exact for all four types, and the kernels form (double)element in registers and
 * feed the same operands in the same order to the same FP64 MFMA and FP64 arithmetic.  With ITAL_INGEST_F64 ital_NAME_t and
 * ital_NAME are one and the same code.
 *
 * -22 before any HIP call, in addition to what ital_NAME refuses: an unknown xtype, X not aligned to 16 B.
 */
#ifndef ITAL_ROWS_H
#define ITAL_ROWS_H

#include "ital_hip.h"
#include "ital_ingest.h"
#include "ital_rewhiten.h"

#ifdef __cplusplus
extern "C" {
#endif

int ital_rbf_cols_t(const void* X, const double* xnorm, int64_t n, int ldx, const double* Xs, const double* sn, int c,
                    double var, double length_scale, double* out, int64_t ldo, int xtype, hipStream_t stream);

int ital_cross_cov_cols_t(const void* X, const double* xnorm, int64_t n, int ldx, const double* Xs, const double* sn, int c,
                          const double* W, int ldw, const double* V, int64_t ldv, int m, double var, double length_scale,
                          double* out, int64_t ldo, int xtype, hipStream_t stream);

int ital_whiten_append_t(const void* X, const double* xnorm, int64_t n, int ldx, const double* Xnew, const double* snew, int c,
                         const double* L21, int ldw, const double* L22, const double* alpha_new, double* V, int64_t ldv, int m,
                         double var, double length_scale, double* mu, double* s2, int xtype, hipStream_t stream);

/* a->X is of type xtype; a->rows (the batch state the samples are staged from) is FP64 as ever. */
int ital_gp_append_t(const ital_append_desc* a, int xtype, hipStream_t stream);

/* d->sel_X (r->step.sel_X) is of type xtype: the record's feature row is widened while it is gathered, and the round's
 * covariance columns stream the typed rows. */
int ital_score_step_t(const ital_score_desc* d, int xtype, hipStream_t stream);
int ital_fetch_round_t(const ital_round_desc* r, int xtype, hipStream_t stream);

int ital_select_local_t(const double* mi, const int32_t* cand, const uint8_t* alive, int64_t n_cand, int64_t pos_offset,
                        const int64_t* gpos, int64_t row_offset, int rank, int mode, const double* mu, const double* s2,
                        const void* X, const double* xnorm, int ldx, const double* V, int64_t ldv, int m, int ldw,
                        const double* C, int64_t ldc, int nprev, int kmax, const int* status, double* work, double* record,
                        int xtype, hipStream_t stream);

int ital_select_fused_t(const double* mi, const int32_t* cand, uint8_t* alive, int64_t n_cand, int64_t pos_offset,
                        const int64_t* gpos, int64_t row_offset, int rank, int mode, const double* mu, const double* s2,
                        const void* X, const double* xnorm, int ldx, const double* V, int64_t ldv, int m, int ldw,
                        const double* C, int64_t ldc, int nprev, int slot, ital_batch batch, const int* status, double* record,
                        int64_t* ret, int xtype, hipStream_t stream);

/* Xc (FP64) receives the widened rows. */
int ital_gather_block_t(const int64_t* cand, int64_t nc, int64_t row0, int64_t n_rows, const void* X, const double* xnorm,
                        int ldx, const double* V, int64_t ldv, int m, const double* mu, const double* s2, double* Xc, double* Vc,
                        int64_t ldc, double* xnc, double* muc, double* s2c, int xtype, hipStream_t stream);

/* desc->X is of type xtype (cast to the field's pointer type).  With ITAL_INGEST_F64 this is ital_whiten_rows: xnorm is
 * written by ital_row_norms first.  With a narrower type xnorm is an INPUT ONLY -- the store's norms, written when the rows
 * were ingested, are already the bits ital_row_norms gives on the widened rows -- and is not touched.  -22 additionally for
 * a NULL xnorm (any type). */
int ital_whiten_rows_t(const ital_rewhiten_desc* desc, int xtype, hipStream_t stream);

/* Rows in the caller's type and stride -> padded rows of the SAME type and their FP64 squared norms.
 *
 * src: DEVICE memory, n rows of d elements of type dtype, row stride ld_src ELEMENTS (any alignment to the element size).
 * DEFINITION: X[i][j] has the bits of src[i * ld_src + j] for j < d (the sign of -0.0 included) and is +0 for d <= j < ldx,
 * whatever the buffer held; xnorm[i] has the bits ital_ingest_rows gives for the same source -- it IS ital_ingest_rows, run
 * on blocks of at most scratch_rows rows into `scratch` ([scratch_rows][ldx] FP64, the caller's), whose xnorm goes straight
 * to its place; the full FP64 matrix never exists.  Rows >= n of X and xnorm are not touched; nothing behind column d of a
 * source row is read.  With dtype == ITAL_INGEST_F64 X is the FP64 matrix itself and scratch is not used (may be NULL).
 *
 * -22 (before any HIP call): what ital_ingest_rows refuses, a NULL scratch or scratch_rows < 1 (narrow types, n > 0),
 * scratch not aligned to 16 B.  n == 0 returns 0 without a launch. */
int ital_ingest_rows_t(const void* src, int dtype, int64_t n, int d, int64_t ld_src, void* X, int ldx, double* xnorm,
                       double* scratch, int64_t scratch_rows, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_ROWS_H */
