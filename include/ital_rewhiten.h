/*
 * Whitening a range of data rows against the whole current labelled set (ital_amd GaussianProcess.extend / set_params,
 * ActiveRetrievalBase.add_data / set_params; csrc/rewhiten.hip): what ital_whiten_append does for c <= 16 new labelled rows
 * against all data rows, transposed -- new (or all) data rows against all m labelled rows, in ceil(m / chunk) passes over the
 * feature rows instead of ceil(m / 16).  Conventions as in ital_dense.h: borrowed device pointers, asynchronous on `stream`,
 * 0 or a negative errno-style code with its message in ital_last_error, argument checks before any HIP call, no allocation
 * across the ABI (the call needs no workspace).
 */
#ifndef ITAL_REWHITEN_H
#define ITAL_REWHITEN_H

#include "ital_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A row range of the data matrix, the labelled-set state it is whitened against, and where the results go.  Every per-row
 * pointer (X, xnorm, V, mu, s2) points at the FIRST row of the range: the caller offsets them. */
typedef struct ital_rewhiten_desc {
    const double* X;      /* [n_rows][ldx] feature rows of the range, zero padded to ldx */
    int64_t n_rows;
    int ldx;              /* multiple of 16 */
    const double* XT;     /* [m][ldx] feature rows of the labelled samples (may be NULL when m == 0, like XTn, L, alpha) */
    const double* XTn;    /* [m] their squared norms */
    const double* L;      /* lower Cholesky factor of K_TT + noise I, row-major, leading dimension ldl >= m */
    int ldl;
    const double* alpha;  /* [m] L^-1 y */
    int m;                /* labelled samples */
    double var;
    double length_scale;
    double* xnorm;        /* out [n_rows] squared norms of the rows, as ital_row_norms gives them */
    double* V;            /* out [v_rows][ldv]: column i of rows 0 .. m-1 <- L^-1 K(T, row i); rows m .. v_rows-1 <- 0 */
    int64_t ldv;          /* >= n_rows */
    int v_rows;           /* the caller's capacity, >= m */
    double* mu;           /* out [n_rows] V^T alpha */
    double* s2;           /* out [n_rows] var - colsum(V^2), not clamped */
    int chunk;            /* labelled rows per launch: 0 (the default, ital_whiten_rows_chunk()), 32, 64 or 128 */
} ital_rewhiten_desc;

/* xnorm, V[0:m], mu, s2 of the range.  DEFINITION: bit for bit what ital_row_norms followed by one ital_whiten_append per
 * block of 16 labelled rows from row 0 up gives (block b, b0 = 16 b: m = b0, L21 = &L[b0][0], L22 = &L[b0][b0],
 * alpha_new = &alpha[b0], c = min(16, m - b0)), started from mu = 0, s2 = var -- independent of how the labelled set was
 * appended or revoked.  m == 0: mu = 0, s2 = var.  One wave owns 16 data rows: their feature tile is read once per launch
 * and serves `chunk` labelled rows, whose whitened values stay in LDS for the later blocks of the launch; a labelled set
 * beyond the chunk takes ceil(m / chunk) launches, which read the earlier chunks' rows of V from global memory.
 * -22: a NULL descriptor or buffer, ldx not a positive multiple of 16, ldl < m, ldv < n_rows, v_rows < m, a negative size,
 * a chunk other than the four above.  n_rows == 0 is a no-op. */
int ital_whiten_rows(const ital_rewhiten_desc* desc, hipStream_t stream);

/* The chunk a descriptor with chunk == 0 gets. */
int ital_whiten_rows_chunk(void);

#ifdef __cplusplus
}
#endif
#endif /* ITAL_REWHITEN_H */
