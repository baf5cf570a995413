/*
 * The complete ranking of a score vector and its evaluation against relevance labels on the device (csrc/rank.hip): what
 * the reference does on the host at the end of every round (retrieval_base.py:64-75 `top_results`, utils.py:174-200 `ndcg`,
 * run_experiment.py:154-168 average precision).  ital_topk (ital_hip.h) selects up to ITAL_TOPK_MAX results; this header is
 * the ranking beyond that bound and the two metrics of the experiment loop.  Conventions as in ital_dense.h and ital_knn.h:
 * borrowed device pointers, asynchronous on `stream`, 0 or a negative errno-style code with its message in ital_last_error,
 * argument checks before any HIP call, no allocation across the ABI, workspace sized by a query function.
 */
#ifndef ITAL_RANK_H
#define ITAL_RANK_H

#include <stddef.h>

#include "ital_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ITAL_RANK_TILE 2048        /* elements one workgroup sorts, merges or scans in LDS */
#define ITAL_RANK_EVAL_LEN 6       /* doubles ital_rank_eval writes */
#define ITAL_RANK_AP 0
#define ITAL_RANK_NDCG 1
#define ITAL_RANK_N_POS 2
#define ITAL_RANK_N_NEG 3
#define ITAL_RANK_N_UNKNOWN 4
#define ITAL_RANK_N_NAN 5

/* The complete ranking of v[0..n): out_idx[r] = index_offset + (position of the r-th entry), out_vals[r] (optional, NULL:
 * not written) = that entry with its own bits.
 *
 * ORDER: that of ital_topk, np.argsort(v, kind="stable")[::-1]: value descending; every NaN before every number, whatever
 * its sign bit and payload; NaNs among themselves by descending position; equal values by descending position; -0.0 and
 * +0.0 are equal.  The pair (64-bit order-preserving key, position) is sorted as one composite key; all composite keys are
 * distinct, so the result is one array of bits that depends on nothing but v.
 *
 * ROUTES, by n alone (T = ITAL_RANK_TILE):
 *   n <= T        one workgroup: a bitonic sort in LDS that writes the result itself (1 launch);
 *   T < n <= 2T   several workgroups sort one tile of T each in LDS, one merge pass, one launch that writes the result;
 *   n > 2T        the same with ceil(log2(ceil(n / T))) merge passes (9 at n = 10^6: 11 launches).
 * A merge pass is one launch: every workgroup finds the part of the two sorted runs that makes its T outputs by a binary
 * search (merge path) in what the previous launch wrote, and merges it in LDS.  No workgroup waits on another one of its
 * launch; no atomics.
 *
 * 1 <= n < 2^31.  workspace: at least ital_rank_workspace(n) bytes, aligned to 8 B; nothing but out_idx, out_vals and the
 * workspace is written.
 * -22 (before any HIP call): n < 1 or n >= 2^31; a NULL v, out_idx or workspace; a workspace not aligned to 8 B or smaller
 * than ital_rank_workspace(n). */
int ital_rank_desc(const double* v, int64_t n, int64_t index_offset, int64_t* out_idx, double* out_vals, void* workspace,
                   size_t workspace_bytes, hipStream_t stream);

/* Bytes of workspace of ital_rank_desc (host only, no HIP call); 0 for an n it refuses. */
size_t ital_rank_workspace(int64_t n);

/* Average precision and NDCG of a ranking.  order: int64[n], a result of ital_rank_desc(v, n, index_offset, ...); rel:
 * int8[n], > 0 relevant, < 0 irrelevant, 0 unknown.  out: double[ITAL_RANK_EVAL_LEN] (device memory).
 *
 * DEFINITION.  The known samples (rel != 0) are taken in the order of the ranking; the r-th of them (r = 1, 2, ...) has
 * rank r; unknown samples have no rank.  n_pos, n_neg, n_unknown: the three counts; n_nan: known samples whose score is NaN.
 *   ap    scikit-learn's average_precision_score(rel[rel != 0], v[rel != 0]): known samples of equal score (-0.0 == +0.0)
 *         form one group; the sum over the groups of (positives in the group / n_pos) * (positives so far / known samples so
 *         far), the two counts of the second factor taken at the group's last sample;
 *   ndcg  the reference's utils.ndcg: the sum of 1 / log2(r + 1) over the ranks r of the positives, divided by the same sum
 *         over r = 1 .. n_pos.
 * n_pos == 0 or n_nan > 0: ap and ndcg are NaN, the counts are written.  An entry of `order` outside index_offset + [0, n)
 * is read as an unknown sample.
 *
 * Four launches whatever n: per tile of T ranks the counts and group boundaries, one workgroup that scans the tile records
 * in order, per tile the summands, one workgroup that adds the tile sums.  Integer scans are exact; the floating-point sums
 * have a shape fixed by n (per thread in rank order, a tree over the threads of a tile, tile sums per thread in tile order,
 * a tree over the threads): the same input gives the same bits on every call.  No atomics on floating-point data.
 *
 * workspace: at least ital_rank_eval_workspace(n) bytes, aligned to 8 B.
 * -22 (before any HIP call): n < 1 or n >= 2^31; a NULL order, v, rel, out or workspace; a workspace not aligned to 8 B or
 * smaller than ital_rank_eval_workspace(n). */
int ital_rank_eval(const int64_t* order, const double* v, const signed char* rel, int64_t n, int64_t index_offset, double* out,
                   void* workspace, size_t workspace_bytes, hipStream_t stream);

/* Bytes of workspace of ital_rank_eval (host only, no HIP call); 0 for an n it refuses. */
size_t ital_rank_eval_workspace(int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_RANK_H */
