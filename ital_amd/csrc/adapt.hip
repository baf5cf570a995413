// Device side of the AdaptAL learner (ital_amd/adapt_al.py), the reference's ital/adapt_al.py:
//
//   ital_chol_inv_diag   out[i] = (K^-1)_ii = sum_j (L^-1)[j][i]^2 from the Cholesky factor of the candidate Gram; its
//                        reciprocal is the Schur complement that information_density gets from one reduced_inv per candidate
//   ital_adapt_scores    entropy and information density of every candidate, elementwise
//   ital_adapt_error     expected classification error of the short-listed candidates (closed-form rank-one update)
//
// The triangular inverse M = L^-1 is built by recursive doubling: the 64 x 64 diagonal blocks (one wave each, forward
// substitution in LDS), then for s = 64, 128, ... every pair of neighbouring inverted diagonal blocks of size s,
// [a0, a0 + s) and [a0 + s, min(a0 + 2 s, n)), gets its off-diagonal block M21 = -M22 (L21 M11) in two launches: T = L21 M11
// and M21 = -M22 T.  Both products run on v_mfma_f64_16x16x4_f64 through a 128 x 128 LDS-staged tile (tile_mm below: the LDS
// layout, schedule and MFMA stage of mfma_tile.h's tile_nt, with the second operand read k-major and every element behind a
// predicate, which is what makes the triangular k-ranges and ragged edges exact: nothing outside the computed part of M is
// ever read).  The squared column sums leave the second product's accumulators as one partial per (64-row block, column); a
// last kernel adds a column's partials top-down.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.h"
#include "ital_adapt.h"
#include "ital_internal.h"
#include "mfma_tile.h"

namespace ital {
namespace adapt {

using namespace ital::tile;

constexpr int NB = 64;         // diagonal block

// acc[p][q] += sum over kbeg <= k < kend of A(r, k) B(k, c) for the 128 x 128 tile of a workgroup of 256 threads: wave
// (wy, wx) owns tile rows 64 wy + 16 p + (kg + 4 reg) and tile columns 64 wx + 16 q + col (D layout of the f64 MFMA).
// fa(r, k): element of A at tile row r; fb(k, c): element of B at tile column c; both return 0 outside their operand (k at
// or past kend included).  A is staged as k-pairs of rows (stage_role), B as runs of 16 columns of one k, into the layout
// mfma_stage reads.  Register + LDS double buffer, one barrier per stage; ends with a barrier.
template <class FA, class FB>
__device__ inline void tile_mm(FA fa, FB fb, int kbeg, int kend, StageLds& lds, d4 acc[4][4]) {
    int ska, arow;
    stage_role(ska, arow);
    const int kb = threadIdx.x >> 4, bcol = threadIdx.x & 15;
    double ra[8], rb[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            ra[2 * u] = fa(arow + 8 * u, k0 + ska);
            ra[2 * u + 1] = fa(arow + 8 * u, k0 + ska + 1);
        }
#pragma unroll
        for (int u = 0; u < 8; u++) rb[u] = fb(k0 + kb, bcol + 16 * u);
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            lds[buf][0][ska][arow + 8 * u] = ra[2 * u];
            lds[buf][0][ska + 1][arow + 8 * u] = ra[2 * u + 1];
        }
#pragma unroll
        for (int u = 0; u < 8; u++) lds[buf][1][kb][bcol + 16 * u] = rb[u];
    };
    const int nstep = (kend - kbeg + KS - 1) / KS;
    if (nstep <= 0) return;
    fetch(kbeg);
    stage(0);
    __syncthreads();
    for (int s_ = 0; s_ < nstep; s_++) {
        const int buf = s_ & 1;
        if (s_ + 1 < nstep) fetch(kbeg + (s_ + 1) * KS);
        mfma_stage(lds, buf, acc);
        if (s_ + 1 < nstep) stage(buf ^ 1);
        __syncthreads();
    }
}

struct InvArgs {
    const double* L; int n; int64_t ld;
    double* M;        // L^-1, lower triangle, n x ldw
    double* Tm;       // L21 M11 of the current level, at the place of M21
    double* part;     // [64-row block][column]: sum of squares of that block's rows of the column
    int64_t ldw;
    const int* info;
    int s;            // block size of the level
};

__device__ inline bool skipped(const InvArgs& a) { return a.info && *a.info != 0; }

// Inverse of the diagonal block b (forward substitution, column c by thread c) and the block's own squared column sums.
// One wave and 65 KB of LDS per block (fits gfx950's 160 KB per CU): 64 us per call at n = 9292, 0.8 % of the whole inverse
// (profiles/adapt_kernel_stats.csv).
__global__ __launch_bounds__(64) void inv_diag_block_kernel(InvArgs a) {
    __shared__ double l[NB][NB + 1];
    __shared__ double x[NB][NB + 1];
    if (skipped(a)) return;
    const int b = blockIdx.x, k0 = b * NB, m = min(NB, a.n - k0), c = threadIdx.x;
    for (int e = c; e < NB * NB; e += 64) {
        const int r = e / NB, cc = e % NB;
        l[r][cc] = (r < m && cc <= r) ? a.L[(int64_t)(k0 + r) * a.ld + k0 + cc] : 0.0;
    }
    __syncthreads();
    if (c >= m) return;
    double ss = 0.0;
    for (int r = c; r < m; r++) {
        double v = r == c ? 1.0 : 0.0;
        for (int p = c; p < r; p++) v -= l[r][p] * x[p][c];
        v /= l[r][r];
        x[r][c] = v;                         // column c is read by thread c alone
        a.M[(int64_t)(k0 + r) * a.ldw + k0 + c] = v;
        ss += v * v;
    }
    a.part[(int64_t)b * a.ldw + k0 + c] = ss;
}

// Geometry of a workgroup at level s: pair blockIdx.y = rows / columns [a0, c0) and [c0, c1); tile (ti, tj) of the
// (c1 - c0) x s block below the diagonal.  False: nothing to do.
__device__ inline bool pair_tile(const InvArgs& a, int& a0, int& c0, int& c1, int& i0, int& j0) {
    const int64_t A0 = (int64_t)blockIdx.y * 2 * a.s;
    if (A0 + a.s >= a.n) return false;
    a0 = (int)A0;
    c0 = a0 + a.s;
    c1 = (int)min((int64_t)c0 + a.s, (int64_t)a.n);
    const int nt = (a.s + T - 1) / T;
    i0 = c0 + (int)(blockIdx.x / nt) * T;
    j0 = a0 + (int)(blockIdx.x % nt) * T;
    return i0 < c1;
}

// T[i][j] = sum_{k = j}^{c0 - 1} L[i][k] M[k][j], i in [c0, c1), j in [a0, c0): M11 is lower triangular.
__global__ __launch_bounds__(256, 2) void inv_lm_kernel(InvArgs a) {
    __shared__ StageLds lds;
    if (skipped(a)) return;
    int a0, c0, c1, i0, j0;
    if (!pair_tile(a, a0, c0, c1, i0, j0)) return;
    auto fa = [&](int r, int k) {
        const int i = i0 + r;
        return (i < c1 && k < c0) ? a.L[(int64_t)i * a.ld + k] : 0.0;
    };
    auto fb = [&](int k, int c) {
        const int j = j0 + c;
        return (k < c0 && j < c0 && j <= k) ? a.M[(int64_t)k * a.ldw + j] : 0.0;
    };
    d4 acc[4][4];
    zero_acc(acc);
    tile_mm(fa, fb, j0, c0, lds, acc);
    const DLane dl = d_lane();
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int j = j0 + dl.column(q);
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int i = i0 + dl.row(p, reg);
                if (i < c1 && j < c0) a.Tm[(int64_t)i * a.ldw + j] = acc[p][q][reg];
            }
    }
}

// M[i][j] = -sum_{k = c0}^{i} M[i][k] T[k][j], i in [c0, c1), j in [a0, c0): M22 is lower triangular.  The squares of the
// results are summed per column over each wave's 64 rows (one global 64-row block: c0 and the tile origin are multiples
// of 64) in a fixed order: registers, then the four lane groups.
__global__ __launch_bounds__(256, 2) void inv_mt_kernel(InvArgs a) {
    __shared__ StageLds lds;
    if (skipped(a)) return;
    int a0, c0, c1, i0, j0;
    if (!pair_tile(a, a0, c0, c1, i0, j0)) return;
    auto fa = [&](int r, int k) {
        const int i = i0 + r;
        return (i < c1 && k <= i) ? a.M[(int64_t)i * a.ldw + k] : 0.0;
    };
    auto fb = [&](int k, int c) {
        const int j = j0 + c;
        return (k < c1 && j < c0) ? a.Tm[(int64_t)k * a.ldw + j] : 0.0;
    };
    d4 acc[4][4];
    zero_acc(acc);
    tile_mm(fa, fb, c0, min(i0 + T, c1), lds, acc);
    const DLane dl = d_lane();
    const int iw = i0 + 64 * dl.wy;     // first row of the wave's 64-row block
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int j = j0 + dl.column(q);
        double ss = 0.0;
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int i = i0 + dl.row(p, reg);
                const double v = -acc[p][q][reg];
                if (i < c1 && j < c0) {
                    a.M[(int64_t)i * a.ldw + j] = v;
                    ss += v * v;
                }
            }
        ss += __shfl_xor(ss, 16, 64);
        ss += __shfl_xor(ss, 32, 64);
        if (dl.kg == 0 && iw < c1 && j < c0) a.part[(int64_t)(iw / NB) * a.ldw + j] = ss;
    }
}

// out[j] = sum of the column's partials, from its diagonal block downwards
__global__ __launch_bounds__(256) void inv_colsum_kernel(InvArgs a, double* out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n) return;
    if (skipped(a)) {
        out[j] = __builtin_nan("");
        return;
    }
    const int nblk = (a.n + NB - 1) / NB;
    double v = 0.0;
    for (int b = j / NB; b < nblk; b++) v += a.part[(int64_t)b * a.ldw + j];
    out[j] = v;
}

__host__ inline int64_t pad16(int64_t v) { return (v + 15) / 16 * 16; }

// clip(norm.cdf(0, mean, sd), 1e-8, 1 - 1e-8) as np.maximum(1e-8, np.minimum(1 - 1e-8, .)): NaN stays NaN
__device__ inline double prob_irrelevant(double mean, double var) {
    double p = norm_cdf0(mean, sqrt(var));
    p = p > 1.0 - 1e-8 ? 1.0 - 1e-8 : p;
    p = p < 1e-8 ? 1e-8 : p;
    return p;
}

__global__ __launch_bounds__(256) void adapt_scores_kernel(const double* mu, const double* s2, const double* inv_diag, int64_t n,
                                                           double kdiag, double* entropy, double* density) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double p = prob_irrelevant(mu[i], fmax(s2[i], 0.0));
    entropy[i] = -1.0 * (p * log(p) + (1.0 - p) * log(1.0 - p));
    const double sigma = 1.0 / inv_diag[i];
    density[i] = log(kdiag / (sigma < 1e-6 ? 1e-6 : sigma)) / 2;
}

// grid (r, 2): row a, fb = True (blockIdx.y == 0) or False
__global__ __launch_bounds__(256) void adapt_error_kernel(const double* C, int64_t ldc, const int* rows, int64_t nc,
                                                          const double* mu, const double* s2, double noise, double* work) {
    __shared__ double red[256];
    const int a = blockIdx.x;
    const bool fb = blockIdx.y == 0;
    const int i = rows[a];
    const double mui = mu[i], s2i = s2[i];
    const double g = 1.0 / (s2i + noise);
    const double d = g * ((fb ? 1.0 : 0.0) - mui);
    const double* c = C + (int64_t)a * ldc;
    double sum = 0.0;
    for (int64_t j = threadIdx.x; j < nc; j += 256) {
        if (j == i) continue;
        const double cj = c[j];
        const double p = prob_irrelevant(mu[j] + cj * d, fmax(0.0, s2[j] - cj * cj * g));
        sum += mu[j] > 0 ? p : 1.0 - p;
    }
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double pi = prob_irrelevant(mui, fmax(s2i, 0.0));
        work[2 * a + (fb ? 0 : 1)] = (fb ? 1.0 - pi : pi) * red[0];
    }
}

__global__ __launch_bounds__(256) void adapt_error_add_kernel(const double* work, int r, double* err) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a < r) err[a] = (0.0 + work[2 * a]) + work[2 * a + 1];     // err = 0; err += True term; err += False term
}

}  // namespace adapt
}  // namespace ital

using namespace ital::adapt;

extern "C" int64_t ital_chol_inv_diag_workspace(int n) {
    if (n <= 0) return 0;
    const int64_t ldw = pad16(n), nblk = ((int64_t)n + NB - 1) / NB;
    return 2 * (int64_t)n * ldw + nblk * ldw;
}

extern "C" int ital_chol_inv_diag(const double* L, int n, int64_t ld, double* out, double* work, int64_t work_doubles,
                                  const int* info, hipStream_t stream) {
    if (n == 0) return 0;
    if (n < 0) return ital_fail(-22, "ital_chol_inv_diag: n must not be negative");
    if (!L || !out) return ital_fail(-22, "ital_chol_inv_diag: L and out are required");
    if (ld < n) return ital_fail(-22, "ital_chol_inv_diag: ld smaller than n");
    if (!work || work_doubles < ital_chol_inv_diag_workspace(n))
        return ital_fail(-22, "ital_chol_inv_diag: work smaller than ital_chol_inv_diag_workspace(n)");
    const int64_t ldw = pad16(n);
    const int nblk = (n + NB - 1) / NB;
    InvArgs a = {L, n, ld, work, work + (int64_t)n * ldw, work + 2 * (int64_t)n * ldw, ldw, info, NB};
    ITAL_LAUNCH(inv_diag_block_kernel, dim3((unsigned)nblk), dim3(64), 0, stream, a);
    for (int64_t s = NB; s < n; s *= 2) {
        a.s = (int)s;
        const int64_t nt = (s + T - 1) / T, pairs = ((int64_t)n + 2 * s - 1) / (2 * s);
        ITAL_LAUNCH(inv_lm_kernel, dim3((unsigned)(nt * nt), (unsigned)pairs), dim3(256), 0, stream, a);
        ITAL_LAUNCH(inv_mt_kernel, dim3((unsigned)(nt * nt), (unsigned)pairs), dim3(256), 0, stream, a);
    }
    ITAL_LAUNCH(inv_colsum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a, out);
    return ital_check_launch("ital_chol_inv_diag");
}

extern "C" int ital_adapt_scores(const double* mu, const double* s2, const double* inv_diag, int64_t n, double kdiag,
                                 double* entropy, double* density, hipStream_t stream) {
    if (n == 0) return 0;
    if (n < 0 || n > ((int64_t)1 << 31)) return ital_fail(-22, "ital_adapt_scores: n outside 0 .. 2^31");
    if (!mu || !s2 || !inv_diag || !entropy || !density) return ital_fail(-22, "ital_adapt_scores: null buffer");
    ITAL_LAUNCH(adapt_scores_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, mu, s2, inv_diag, n, kdiag,
                entropy, density);
    return ital_check_launch("ital_adapt_scores");
}

extern "C" int ital_adapt_error(const double* C, int64_t ldc, const int* rows, int r, int64_t nc, const double* mu,
                                const double* s2, double noise, double* work, double* err, hipStream_t stream) {
    if (r == 0) return 0;
    if (r < 0 || nc <= 0) return ital_fail(-22, "ital_adapt_error: r must not be negative and nc must be positive");
    if (r > nc) return ital_fail(-22, "ital_adapt_error: more rows than candidates");
    if (ldc < nc) return ital_fail(-22, "ital_adapt_error: ldc smaller than nc");
    if (!C || !rows || !mu || !s2 || !work || !err) return ital_fail(-22, "ital_adapt_error: null buffer");
    ITAL_LAUNCH(adapt_error_kernel, dim3((unsigned)r, 2), dim3(256), 0, stream, C, ldc, rows, nc, mu, s2, noise, work);
    ITAL_LAUNCH(adapt_error_add_kernel, dim3((unsigned)((r + 255) / 256)), dim3(256), 0, stream, work, r, err);
    return ital_check_launch("ital_adapt_error");
}
