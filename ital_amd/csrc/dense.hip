// Dense FP64 building blocks of the cross-validated hyper-parameter search (ital_amd/tune.py), the reference's
// optimize_parameters.py:28-62 driving GaussianProcess.fit / predict_stored (ital/gp.py:141-161, :203-232) once per fold:
//
//   ital_gram_rows           K_f = var exp(-|x_a - x_b|^2 / (2 l^2)) + noise I over a fold's training rows (lower triangle)
//   ital_chol_batched        blocked right-looking Cholesky of many such matrices at once, in place
//   ital_chol_solve_batched  alpha_f = K_f^-1 y_f from the factors
//   ital_kernel_matvec       out[i][f] = sum_j k(a_i, b_j) W[j][f]: every fold's held-out predictions in one pass,
//                            the kernel matrix never materialised
//
// Matrices are row-major with their own leading dimension; the factor overwrites the lower triangle (L[i][j], j <= i) and
// nothing else: the strict upper triangle and the padding past n are never written.  Every product with a k-dimension runs
// on v_mfma_f64_16x16x4_f64 through the 128 x 128 LDS-staged tile of mfma_tile.h; the diagonal blocks (64 x 64, one workgroup
// each) and the row-wise panel solve are VALU work, a few per cent of the flops.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ital_dense.h"
#include "ital_internal.h"
#include "mfma_tile.h"

namespace ital {
namespace dense {

using namespace ital::tile;

constexpr int NB = 64;         // Cholesky block

// ---------------------------------------------------------------------------------------------------------------- Gram
struct GramArgs {
    const double* X; const double* xn; int ldx;
    const int64_t* const* idx; const int* n; double* const* K; const int64_t* ld;
    double var, s, noise;
};

// grid: (lower tile pairs of the largest matrix, matrices)
__global__ __launch_bounds__(256, 2) void gram_kernel(GramArgs a) {
    __shared__ StageLds lds;
    const int b = blockIdx.y;
    const int64_t n = a.n[b];
    int ti, tj;
    tri_pair(blockIdx.x, ti, tj);
    const int64_t i0 = (int64_t)ti * T, j0 = (int64_t)tj * T;
    if (i0 >= n) return;
    const int64_t* idx = a.idx[b];
    int sk, srow;
    stage_role(sk, srow);
    const double* pa[4];
    const double* pb[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {     // rows past n: the last row (computed, never stored)
        pa[u] = a.X + idx[min(i0 + srow + 8 * u, n - 1)] * a.ldx + sk;
        pb[u] = a.X + idx[min(j0 + srow + 8 * u, n - 1)] * a.ldx + sk;
    }
    d4 acc[4][4];
    zero_acc(acc);
    tile_nt(pa, pb, a.ldx, lds, acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, kg = lane >> 4;
    const int64_t iw = i0 + 64 * (wave >> 1), jw = j0 + 64 * (wave & 1);
    double* K = a.K[b];
    const int64_t ld = a.ld[b];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int64_t j = jw + 16 * q + col;
        const double bnj = a.xn[idx[min(j, n - 1)]];
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int64_t i = iw + 16 * p + kg + 4 * reg;
                const double ani = a.xn[idx[min(i, n - 1)]];
                // reference: K_all = v * exp((A + B - 2 C) / s) (gp.py:412 / dist_kernel :436), then + noise * eye (:158)
                double v = a.var * exp(rbf_sqdist(ani, bnj, acc[p][q][reg]) / a.s);
                if (i == j) v += a.noise;
                if (i < n && j <= i) K[i * ld + j] = v;
            }
    }
}

// ------------------------------------------------------------------------------------------------------------ Cholesky
struct CholArgs {
    double* const* A; const int* n; const int64_t* ld; int* info; int* status; int k0;
};

// Unblocked right-looking factor of the diagonal block at (k0, k0), staged in LDS; one workgroup per matrix.  A pivot that
// is not > 0 (NaN included) records info = column + 1, sets status bit 1 and stops this matrix: the later kernels skip it.
__global__ __launch_bounds__(256) void chol_diag_kernel(CholArgs a) {
    __shared__ double s[NB][NB + 1];
    const int b = blockIdx.x;
    const int n = a.n[b], k0 = a.k0;
    if (k0 >= n || a.info[b] != 0) return;
    const int m = min(NB, n - k0);
    const int64_t ld = a.ld[b];
    double* A = a.A[b] + (int64_t)k0 * ld + k0;
    const int tid = threadIdx.x;
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e / NB, c = e % NB;
        if (r < m && c <= r) s[r][c] = A[(int64_t)r * ld + c];
    }
    __syncthreads();
    for (int j = 0; j < m; j++) {
        const double d = s[j][j];
        if (!(d > 0)) {                     // the same value in every thread: the whole workgroup leaves
            if (tid == 0) {
                a.info[b] = k0 + j + 1;
                atomicOr(a.status, 1);
            }
            return;
        }
        __syncthreads();                    // every thread has read the pivot
        const double ljj = sqrt(d);
        if (tid == 0) s[j][j] = ljj;
        for (int r = j + 1 + tid; r < m; r += 256) s[r][j] /= ljj;
        __syncthreads();
        const int w = m - j - 1;
        for (int e = tid; e < w * w; e += 256) {
            const int r = j + 1 + e / w, c = j + 1 + e % w;
            if (c <= r) s[r][c] -= s[r][j] * s[c][j];
        }
        __syncthreads();
    }
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e / NB, c = e % NB;
        if (r < m && c <= r) A[(int64_t)r * ld + c] = s[r][c];
    }
}

// Panel: L21 = A21 L11^-T, one row per thread (forward substitution against L11 in LDS).  Only full blocks have rows below.
__global__ __launch_bounds__(256) void chol_trsm_kernel(CholArgs a) {
    __shared__ double l[NB][NB + 1];
    const int b = blockIdx.y;
    const int n = a.n[b], k0 = a.k0;
    if (k0 + NB >= n || a.info[b] != 0) return;
    const int64_t ld = a.ld[b];
    double* A = a.A[b];
    for (int e = threadIdx.x; e < NB * NB; e += 256) {
        const int r = e / NB, c = e % NB;
        if (c <= r) l[r][c] = A[(int64_t)(k0 + r) * ld + k0 + c];
    }
    __syncthreads();
    const int64_t i = (int64_t)k0 + NB + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double* row = A + i * ld + k0;
    double x[NB];
#pragma unroll
    for (int c = 0; c < NB; c++) x[c] = row[c];
#pragma unroll
    for (int c = 0; c < NB; c++) {
        double v = x[c];
#pragma unroll
        for (int p = 0; p < c; p++) v -= x[p] * l[c][p];
        x[c] = v / l[c][c];
    }
#pragma unroll
    for (int c = 0; c < NB; c++) row[c] = x[c];
}

// Trailing update A22 -= L21 L21^T (lower triangle), 128 x 128 MFMA tiles over the tile pairs ti >= tj.
__global__ __launch_bounds__(256, 2) void chol_syrk_kernel(CholArgs a) {
    __shared__ StageLds lds;
    const int b = blockIdx.y;
    const int n = a.n[b], k0 = a.k0, k1 = k0 + NB;
    if (k1 >= n || a.info[b] != 0) return;
    int ti, tj;
    tri_pair(blockIdx.x, ti, tj);
    const int64_t i0 = (int64_t)k1 + (int64_t)ti * T, j0 = (int64_t)k1 + (int64_t)tj * T;
    if (i0 >= n) return;
    const int64_t ld = a.ld[b];
    double* A = a.A[b];
    int sk, srow;
    stage_role(sk, srow);
    const double* pa[4];
    const double* pb[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        pa[u] = A + min(i0 + srow + 8 * u, (int64_t)n - 1) * ld + k0 + sk;
        pb[u] = A + min(j0 + srow + 8 * u, (int64_t)n - 1) * ld + k0 + sk;
    }
    d4 acc[4][4];
    zero_acc(acc);
    tile_nt(pa, pb, NB, lds, acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, kg = lane >> 4;
    const int64_t iw = i0 + 64 * (wave >> 1), jw = j0 + 64 * (wave & 1);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int64_t j = jw + 16 * q + col;
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int64_t i = iw + 16 * p + kg + 4 * reg;
                if (i < n && j <= i) A[i * ld + j] -= acc[p][q][reg];
            }
    }
}

// -------------------------------------------------------------------------------------------------------------- solves
struct SolveArgs {
    const double* const* L; const int* n; const int64_t* ld; double* const* y; const int* info;
};

// y <- L^-T L^-1 y, one workgroup per matrix: blocks of NB unknowns, the diagonal block by wave 0 (one unknown per lane),
// the rest of the vector updated by all threads.
__global__ __launch_bounds__(256) void chol_solve_kernel(SolveArgs a) {
    __shared__ double xs[NB];
    const int b = blockIdx.x;
    const int n = a.n[b];
    if (n <= 0 || (a.info && a.info[b] != 0)) return;
    const double* L = a.L[b];
    const int64_t ld = a.ld[b];
    double* y = a.y[b];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int kb = 0; kb < n; kb += NB) {                // L z = y
        const int m = min(NB, n - kb);
        if (tid < 64) {
            double v = lane < m ? y[kb + lane] : 0.0;
            for (int c = 0; c < m; c++) {
                const double xc = __shfl(v, c, 64) / L[(int64_t)(kb + c) * ld + kb + c];
                if (lane == c) v = xc;
                if (lane > c && lane < m) v -= L[(int64_t)(kb + lane) * ld + kb + c] * xc;
            }
            if (lane < m) {
                y[kb + lane] = v;
                xs[lane] = v;
            }
        }
        __syncthreads();
        for (int64_t i = (int64_t)kb + m + tid; i < n; i += 256) {
            const double* row = L + i * ld + kb;
            double v = y[i];
            for (int c = 0; c < m; c++) v -= row[c] * xs[c];
            y[i] = v;
        }
        __syncthreads();
    }
    for (int kb = ((n - 1) / NB) * NB; kb >= 0; kb -= NB) {     // L^T x = z
        const int m = min(NB, n - kb);
        if (tid < 64) {
            double v = lane < m ? y[kb + lane] : 0.0;
            for (int r = m - 1; r >= 0; r--) {
                const double xr = __shfl(v, r, 64) / L[(int64_t)(kb + r) * ld + kb + r];
                if (lane == r) v = xr;
                if (lane < r) v -= L[(int64_t)(kb + r) * ld + kb + lane] * xr;
            }
            if (lane < m) {
                y[kb + lane] = v;
                xs[lane] = v;
            }
        }
        __syncthreads();
        for (int64_t i = tid; i < kb; i += 256) {
            double v = y[i];
            for (int c = 0; c < m; c++) v -= L[(int64_t)(kb + c) * ld + i] * xs[c];
            y[i] = v;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------ kernel times W
struct KwArgs {
    const double *Xa, *an; int64_t na;
    const double *Xb, *bn; int64_t nb;
    int ldx;
    const double* W; int64_t ldw; int F;
    double var, s;
    double* out; int64_t ldo; int64_t split_stride;   // out of split y: out + y * split_stride
    int64_t jchunk;
};

// grid: (row tiles of a, splits of b).  Per 128 x 128 tile (first operand b, second a, so that the kernel values land with
// a's row on the lane): distances on MFMA, exp in place, then outT[f][i] += sum_j W[j][f] k(a_i, b_j) on MFMA with the
// kernel tile as the B operand straight from the accumulators (register r of a D tile = k-step r).  The two waves that
// share a's rows are summed through LDS at the end.
__global__ __launch_bounds__(256, 2) void kernel_w_kernel(KwArgs a) {
    __shared__ StageLds lds;
    const int64_t i0 = (int64_t)blockIdx.x * T;
    const int64_t jbeg = (int64_t)blockIdx.y * a.jchunk, jend = min(a.nb, jbeg + a.jchunk);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, kg = lane >> 4, wy = wave >> 1, wx = wave & 1;
    int sk, srow;
    stage_role(sk, srow);
    const double* pa[4];
    const double* pb[4];
#pragma unroll
    for (int u = 0; u < 4; u++) pb[u] = a.Xa + min(i0 + srow + 8 * u, a.na - 1) * a.ldx + sk;
    const int64_t iw = i0 + 64 * wx;
    double ani[4];
#pragma unroll
    for (int q = 0; q < 4; q++) ani[q] = a.an[min(iw + 16 * q + col, a.na - 1)];
    d4 o[4];
#pragma unroll
    for (int q = 0; q < 4; q++) o[q] = (d4){0, 0, 0, 0};
    for (int64_t j0 = jbeg; j0 < jend; j0 += T) {
#pragma unroll
        for (int u = 0; u < 4; u++) pa[u] = a.Xb + min(j0 + srow + 8 * u, a.nb - 1) * a.ldx + sk;
        d4 acc[4][4];
        zero_acc(acc);
        tile_nt(pa, pb, a.ldx, lds, acc);
        const int64_t jw = j0 + 64 * wy;
#pragma unroll
        for (int p = 0; p < 4; p++) {
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const double bnj = a.bn[min(jw + 16 * p + kg + 4 * reg, a.nb - 1)];
#pragma unroll
                for (int q = 0; q < 4; q++) acc[p][q][reg] = a.var * exp(rbf_sqdist(bnj, ani[q], acc[p][q][reg]) / a.s);
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int64_t j = jw + 16 * p + 4 * r + kg;     // k-index kg of step r
                const double w = (j < jend && col < a.F) ? a.W[j * a.ldw + col] : 0.0;
#pragma unroll
                for (int q = 0; q < 4; q++) o[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(w, acc[p][q][r], o[q], 0, 0, 0);
            }
        }
    }
    // o[q]: column = row i = iw + 16 q + col of a, row = f = kg + 4 reg.  tile_nt ended with a barrier: lds is free.
    double* red = &lds[0][0][0][0];                      // [wx][64 rows][16 f]
    if (jbeg >= jend) return;
    if (wy == 1) {
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) red[(wx * 64 + 16 * q + col) * 16 + kg + 4 * reg] = o[q][reg];
    }
    __syncthreads();
    if (wy == 0) {
        double* out = a.out + (int64_t)blockIdx.y * a.split_stride;
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int64_t i = iw + 16 * q + col;
                const int f = kg + 4 * reg;
                const double v = o[q][reg] + red[(wx * 64 + 16 * q + col) * 16 + f];
                if (i < a.na && f < a.F) out[i * a.ldo + f] = v;
            }
    }
}

// out[i][f] = sum_s part[s][i][f], s ascending
__global__ __launch_bounds__(256) void kernel_w_reduce(const double* part, int64_t na, int nsplit, int F, double* out,
                                                       int64_t ldo) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= na * F) return;
    const int64_t i = e / F;
    const int f = (int)(e % F);
    double v = 0.0;
    for (int s_ = 0; s_ < nsplit; s_++) v += part[((int64_t)s_ * na + i) * 16 + f];
    out[i * ldo + f] = v;
}

constexpr int64_t KW_TARGET_BLOCKS = 1024;   // 256 CUs x 2 workgroups x 2 waves of them

__host__ inline void kw_split(int64_t na, int64_t nb, int64_t& nsplit, int64_t& jchunk) {
    const int64_t gx = (na + T - 1) / T, tiles_b = (nb + T - 1) / T;
    int64_t want = (KW_TARGET_BLOCKS + gx - 1) / gx;
    want = want < 1 ? 1 : (want > tiles_b ? tiles_b : want);
    jchunk = ((tiles_b + want - 1) / want) * T;
    nsplit = (nb + jchunk - 1) / jchunk;
}

}  // namespace dense
}  // namespace ital

using namespace ital::dense;

extern "C" int ital_gram_rows(const double* X, const double* xnorm, int ldx, const int64_t* const* idx, const int* n,
                              double* const* K, const int64_t* ld, int count, int max_n, double var, double length_scale,
                              double noise, hipStream_t stream) {
    if (count <= 0 || max_n <= 0) return 0;
    if (ldx <= 0 || ldx % 16 != 0) return ital_fail(-22, "ital_gram_rows: ldx must be a positive multiple of 16");
    if (count > 65535) return ital_fail(-22, "ital_gram_rows: more than 65535 matrices per call");
    const int64_t tn = ((int64_t)max_n + T - 1) / T, pairs = tn * (tn + 1) / 2;
    if (pairs > INT32_MAX) return ital_fail(-22, "ital_gram_rows: matrix too large");
    GramArgs a = {X, xnorm, ldx, idx, n, K, ld, var, -2.0 * length_scale * length_scale, noise};
    ITAL_LAUNCH(gram_kernel, dim3((unsigned)pairs, (unsigned)count), dim3(256), 0, stream, a);
    return ital_check_launch("ital_gram_rows");
}

extern "C" int ital_chol_batched(double* const* A, const int* n, const int64_t* ld, int count, int max_n, int* info,
                                 int* status, hipStream_t stream) {
    if (count <= 0 || max_n <= 0) return 0;
    if (count > 65535) return ital_fail(-22, "ital_chol_batched: more than 65535 matrices per call");
    if (!info || !status) return ital_fail(-22, "ital_chol_batched: info and status are required");
    if (hipMemsetAsync(info, 0, sizeof(int) * (size_t)count, stream) != hipSuccess)
        return ital_fail(-5, "ital_chol_batched: hipMemsetAsync failed");
    CholArgs a = {A, n, ld, info, status, 0};
    for (int k0 = 0; k0 < max_n; k0 += NB) {
        a.k0 = k0;
        ITAL_LAUNCH(chol_diag_kernel, dim3((unsigned)count), dim3(256), 0, stream, a);
        const int64_t below = (int64_t)max_n - k0 - NB;
        if (below > 0) {
            ITAL_LAUNCH(chol_trsm_kernel, dim3((unsigned)((below + 255) / 256), (unsigned)count), dim3(256), 0, stream, a);
            const int64_t tr = (below + T - 1) / T;
            ITAL_LAUNCH(chol_syrk_kernel, dim3((unsigned)(tr * (tr + 1) / 2), (unsigned)count), dim3(256), 0, stream, a);
        }
        const int rc = ital_check_launch("ital_chol_batched");
        if (rc) return rc;
    }
    return 0;
}

extern "C" int ital_chol_solve_batched(const double* const* L, const int* n, const int64_t* ld, double* const* y, int count,
                                       const int* info, hipStream_t stream) {
    if (count <= 0) return 0;
    SolveArgs a = {L, n, ld, y, info};
    ITAL_LAUNCH(chol_solve_kernel, dim3((unsigned)count), dim3(256), 0, stream, a);
    return ital_check_launch("ital_chol_solve_batched");
}

extern "C" int64_t ital_kernel_matvec_workspace(int64_t na, int64_t nb) {
    if (na <= 0 || nb <= 0) return 0;
    int64_t nsplit, jchunk;
    kw_split(na, nb, nsplit, jchunk);
    return nsplit > 1 ? nsplit * na * 16 : 0;
}

extern "C" int ital_kernel_matvec(const double* Xa, const double* an, int64_t na, const double* Xb, const double* bn,
                                  int64_t nb, int ldx, const double* W, int64_t ldw, int F, double var, double length_scale,
                                  double* out, int64_t ldo, double* work, int64_t work_doubles, hipStream_t stream) {
    if (na <= 0 || F == 0) return 0;
    if (F < 0 || F > 16) return ital_fail(-22, "ital_kernel_matvec: F must be between 1 and 16");
    if (ldx <= 0 || ldx % 16 != 0) return ital_fail(-22, "ital_kernel_matvec: ldx must be a positive multiple of 16");
    if (ldw < F || ldo < F) return ital_fail(-22, "ital_kernel_matvec: ldw and ldo must be at least F");
    if (nb <= 0) return ital_fail(-22, "ital_kernel_matvec: nb must be positive");
    const int64_t gx = (na + T - 1) / T;
    if (gx > INT32_MAX) return ital_fail(-22, "ital_kernel_matvec: too many rows");
    int64_t nsplit, jchunk;
    kw_split(na, nb, nsplit, jchunk);
    KwArgs a = {Xa, an, na, Xb, bn, nb, ldx, W, ldw, F, var, -2.0 * length_scale * length_scale, out, ldo, 0, jchunk};
    if (nsplit > 1) {
        if (!work || work_doubles < nsplit * na * 16)
            return ital_fail(-22, "ital_kernel_matvec: work smaller than ital_kernel_matvec_workspace(na, nb)");
        a.out = work;
        a.ldo = 16;
        a.split_stride = na * 16;
    }
    ITAL_LAUNCH(kernel_w_kernel, dim3((unsigned)gx, (unsigned)nsplit), dim3(256), 0, stream, a);
    int rc = ital_check_launch("ital_kernel_matvec");
    if (rc || nsplit == 1) return rc;
    ITAL_LAUNCH(kernel_w_reduce, dim3((unsigned)((na * F + 255) / 256)), dim3(256), 0, stream, work, na, (int)nsplit, F, out,
                ldo);
    return ital_check_launch("ital_kernel_matvec(reduce)");
}
