/*
 * The k nearest neighbours of rows of a store among rows of the same store (csrc/knn.hip): a tiled self-join on
 * v_mfma_f64_16x16x4_f64 whose epilogue keeps the k best pairs of every query row and never writes a distance tile to
 * memory.  The neighbour structure of the SUD learner (ital_amd/sud.py, the reference's ital/baseline_methods.py:440-473)
 * and the graph of USDM (baseline_methods.py:604).  Conventions as in ital_dense.h and ital_rows.h: borrowed device
 * pointers, asynchronous on `stream`, 0 or a negative errno-style code with its message in ital_last_error, argument checks
 * before any HIP call, no allocation across the ABI.
 */
#ifndef ITAL_KNN_H
#define ITAL_KNN_H

#include <stddef.h>

#include "ital_hip.h"
#include "ital_ingest.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ITAL_KNN_MAX_K 32          /* the lists of a workgroup's 128 query rows live in LDS next to the staged tile */
#define ITAL_KNN_MAX_SPLITS 64     /* the documented cap of `splits` */
#define ITAL_KNN_AUTO_SPLITS 16    /* the most that splits = 0 picks: what ital_knn_workspace(nq, k, 0) makes room for */

#define ITAL_KNN_COSINE 0
#define ITAL_KNN_SQEUCLIDEAN 1

/* For every query row i in [q0, q1) of X the first k pairs (i, j), j in [c0, c1), in the order below.
 *
 * X: [n][ldx] of the element type `xtype` (the ITAL_INGEST_* codes), ldx a multiple of 16 ELEMENTS, pad columns +0, the
 * matrix aligned to 16 B; xnorm: the FP64 squared norms of its rows (the conventions of ital_rows.h).
 *
 * DEFINITION, per pair (i, j):
 *   dot = the FP64 sum over the ldx columns, formed on v_mfma_f64_16x16x4_f64 in an order that depends on nothing but ldx:
 *         not on n, the ranges, `splits`, `xtype` (narrow elements are widened in registers, which is exact) or where a row
 *         stands in its tile;
 *   metric 0 (cosine distance, as the RBMAL kernel defines it):
 *         cos = dot / (sqrt(xnorm[i]) * sqrt(xnorm[j]))     IEEE division, correctly rounded roots;
 *         if (fabs(cos) > 1) cos = copysign(1, cos);
 *         d   = 1 - cos                                     a zero row gives NaN (the canonical quiet NaN);
 *   metric 1 (squared Euclidean distance, the reference's expansion, not clamped at 0):
 *         d   = xnorm[i] + xnorm[j] - 2 * dot.
 *   The bits of d(i, j) equal the bits of d(j, i).
 *
 * ORDER.  The pairs of one query row are ordered by a total order: numbers ascending; equal numbers by ascending j; NaN
 * after every number, by ascending j (where np.sort puts it).  With skip_self != 0 the pair j == i is left out.
 * dist[r * k + s] / idx[r * k + s], r = i - q0, hold the first k pairs of that order; slots beyond the available pairs get
 * +inf / -1.  With accumulate != 0 the order covers those pairs together with the k entries already in dist / idx (which
 * must be a result of this function: sorted, -1 where empty); an entry already there is never duplicated.  Selection does
 * no arithmetic, so the result is one array of bits: the same for any cutting of [c0, c1) into accumulating calls, any
 * cutting of [q0, q1), any `splits` and any of the four element types holding the same values.
 *
 * rowsum[r], if given, is the sum of row r's k kept distances added in slot order, sequentially in FP64 (+inf slots are
 * included, NaN propagates).
 *
 * splits: how many workgroups share the data range of one tile of 128 query rows (for small n); their partial lists go to
 * the workspace and a second kernel merges them by the same order.  0 picks a value from the number of query tiles and the
 * compute units of the current device, at most ITAL_KNN_AUTO_SPLITS.
 *
 * workspace: at least ital_knn_workspace(q1 - q0, k, splits) bytes, aligned to 8 B.  Nothing but dist, idx, rowsum and the
 * workspace is written.  X is streamed once per tile of 128 query rows.
 *
 * -22 (before any HIP call): n < 0 or n > 2^31 - 1; a range outside [0, n] or reversed; ldx <= 0 or not a multiple of 16; an
 * unknown xtype or metric; k < 1 or k > ITAL_KNN_MAX_K; splits < 0 or > ITAL_KNN_MAX_SPLITS; workspace_bytes below
 * ital_knn_workspace; with a non-empty query range a NULL dist, idx or workspace or a workspace not aligned to 8 B; with both
 * ranges non-empty a NULL X or xnorm or an X not aligned to 16 B.  An empty query range returns 0 without a launch; an empty
 * data range fills +inf / -1 (or, accumulating, keeps the lists) and forms rowsum by the rule above. */
int ital_knn_rows(const void* X, int xtype, const double* xnorm, int64_t n, int ldx, int64_t q0, int64_t q1, int64_t c0,
                  int64_t c1, int metric, int k, int skip_self, int accumulate, int splits, double* dist, int64_t* idx,
                  double* rowsum, void* workspace, size_t workspace_bytes, hipStream_t stream);

/* Bytes of workspace for nq query rows (host only, no HIP call); 0 for arguments ital_knn_rows refuses. */
size_t ital_knn_workspace(int64_t nq, int k, int splits);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_KNN_H */
