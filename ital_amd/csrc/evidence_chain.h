// What ital_gp_evidence (evidence.hip), ital_gp_evidence_grad (evidence_grad.hip) and ital_gp_loo_grad (loo_grad.hip) share,
// in one place: the workspace layout, the prologue of five launches, the squared-distance tile, the walk over a wave's
// lower-triangle elements, the serial sums that close the chains and the per-sample terms of lml and the leave-one-out
// scores (the k-major product tile, tile_tn, is in mfma_tile.h).  evidence_grad's factor, alpha, inverse diagonal, M and lml, and loo_grad's loo_logp and loo_mse,
// have evidence's bits because all run this code, not because files are kept in step.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "ital_internal.h"
#include "mfma_tile.h"

namespace ital {
namespace evidence {

using namespace ital::tile;

// ------------------------------------------------------------------------------------------------------- workspace
struct Layout {          // of the workspace of ital_gp_evidence, in doubles from its start; ital_gp_evidence_grad appends to it
    int64_t alpha, cdiag, M, Kp, yp, ldv, nv, total;
};

__host__ __device__ inline Layout layout(int64_t m, int64_t G) {
    Layout w;
    w.alpha = 0;
    w.cdiag = w.alpha + G * m;
    w.M = w.cdiag + G * m;          // the inverse-diagonal kernel's workspace: M_g = L_g^-1 at M + g m m
    w.Kp = w.M + G * m * m;
    w.yp = w.Kp + G;
    w.ldv = w.yp + G;
    w.nv = w.ldv + G;
    w.total = w.nv + G;             // n as int: half of it used
    return w;
}

// -------------------------------------------------------------------------------------------------------- prologue
struct ChainArgs {       // the fields ital_evidence_desc, ital_evidence_grad_desc and ital_loo_grad_desc share
    const double* XT; const double* XTn; int ldx; const double* y; int m; const double* params; int G;
    double* K; int64_t ld; int* info; int* status; double* work; void* const* ev;
};

inline int chain_fail(int code, const char* who, const char* what) {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return ital_fail(code, msg);
}

inline int chain_launched(const char* who, const char* stage) {
    char name[128];
    snprintf(name, sizeof(name), "%s(%s)", who, stage);
    return ital_check_launch(name);
}

// Records event k of the caller's array, if it gave one.
inline int chain_mark(void* const* ev, int k, hipStream_t stream, const char* who) {
    return (ev && hipEventRecord((hipEvent_t)ev[k], stream) != hipSuccess) ? chain_fail(-5, who, "hipEventRecord failed") : 0;
}

// 0, or -22 with `who` in the message for a shared field that is out of range.  An entry point calls it before the checks
// of its own fields, so that refusals keep their order; chain_prologue calls it in any case.
int chain_check(const ChainArgs& c, const char* who);

// chain_check, then setup, the Gram grid, ital_chol_batched, ital_chol_solve_batched and the inverse diagonals on `stream`,
// recording events 0 .. 4: K holds the factors, the workspace alpha, the inverse diagonals and M.  Both are defined in
// evidence.hip, next to the kernels the prologue launches.
int chain_prologue(const ChainArgs& c, const char* who, hipStream_t stream);

// ------------------------------------------------------------------------------------------- squared-distance tile
// The 128 x 128 tile of lower tile pair blockIdx.x of D_ij = |x_i|^2 + |x_j|^2 - 2 x_i . x_j (the expansion of
// ital_gram_rows), left in the accumulators; (iw, jw): the origin of the calling wave's 64 x 64 quarter.  Rows past m are
// the last row (computed, never stored).  False, before any barrier, when the tile lies outside the matrix.  The Gram grid
// and ital_sqdist_lower both get their distances here, so var exp(D / s) from the stored D has the bits of the Gram's entry.
__device__ inline bool sqdist_tile(const double* XT, const double* xn, int64_t m, int ldx, StageLds& lds, d4 acc[4][4],
                                   int64_t& iw, int64_t& jw) {
    int ti, tj;
    tri_pair(blockIdx.x, ti, tj);
    const int64_t i0 = (int64_t)ti * T, j0 = (int64_t)tj * T;
    if (i0 >= m) return false;
    int sk, srow;
    stage_role(sk, srow);
    const double* pa[4];
    const double* pb[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        pa[u] = XT + min(i0 + srow + 8 * u, m - 1) * ldx + sk;
        pb[u] = XT + min(j0 + srow + 8 * u, m - 1) * ldx + sk;
    }
    zero_acc(acc);
    tile_nt(pa, pb, ldx, lds, acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, kg = lane >> 4;
    iw = i0 + 64 * (wave >> 1);
    jw = j0 + 64 * (wave & 1);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const double bnj = xn[min(jw + 16 * q + col, m - 1)];
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const double ani = xn[min(iw + 16 * p + kg + 4 * reg, m - 1)];
                acc[p][q][reg] = rbf_sqdist(ani, bnj, acc[p][q][reg]);
            }
    }
    return true;
}

// ------------------------------------------------------------------------------------------- lower-triangle walker
// f(p, q, reg, i, j) for the elements (i, j), j <= i < n, of the calling lane in its wave's 64 x 64 quarter at (iw, jw),
// acc[p][q][reg] being the lane's value there: q, then p, then reg ascending.  A 16 x 16 sub-tile with nothing at or below
// the diagonal inside the matrix is skipped by the whole wave.  The stored and the fused epilogue of gram_inverse_kernel walk
// through it; gram_grid_kernel and sqdist_lower_kernel write the same walk out, because through it they take a register
// more than before (see there).
template <class I, class F>
__device__ inline void for_each_lower(I iw, I jw, I n, F f) {
    const int lane = threadIdx.x & 63;
    const int col = lane & 15, kg = lane >> 4;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const I j = jw + 16 * q + col;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            if (iw + 16 * p >= n || jw + 16 * q > iw + 16 * p + 15) continue;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const I i = iw + 16 * p + kg + 4 * reg;
                if (i < n && j <= i) f(p, q, reg, i, j);
            }
        }
    }
}

// The k-major product tile (tile_tn) of gram_inverse_kernel and loo_grad lives in mfma_tile.h, next to tile_nt.

// ----------------------------------------------------------------------------------------------------- serial sums
constexpr double LOG2PI = 1.8378770664093454836;

// Four sums over i < m in a workgroup of 256 threads: fill(i) writes the four terms of sample i to term[0..3][threadIdx.x],
// 256 samples at a time, then threads 0 .. 3 add one kind each, i ascending.  Thread k < 4 returns sum k.
template <class F>
__device__ inline double serial_sums(int m, double (*term)[256], F fill) {
    const int tid = threadIdx.x;
    double sum = 0.0;
    for (int i0 = 0; i0 < m; i0 += 256) {
        if (i0 + tid < m) fill(i0 + tid);
        __syncthreads();
        if (tid < 4) {
            const int cnt = min(256, m - i0);
            for (int e = 0; e < cnt; e++) sum += term[tid][e];
        }
        __syncthreads();
    }
    return sum;
}

// lml from y.alpha and sum log L_ii (R&W 2.30).
__device__ inline double lml_value(double ya, double logdet, int m) { return -0.5 * ya - logdet - 0.5 * (double)m * LOG2PI; }

// The leave-one-out quantities of sample i from its target, alpha_i and c_i = (K^-1)_ii (R&W 5.10 - 5.12): predictive mean
// and variance, log predictive density, squared residual.
struct LooSample {
    double mean, var, logp, sq;
};

__device__ inline LooSample loo_sample(double yi, double al, double c) {
    const double r = al / c, mean = yi - r, var = 1.0 / c, d = yi - mean;
    return {mean, var, -0.5 * log(var) - d * d / (2.0 * var) - 0.5 * LOG2PI, r * r};
}

// loo_mse from the sum of the squared residuals.
__device__ inline double loo_mse_value(double sq, int m) { return sq / (double)m; }

}  // namespace evidence
}  // namespace ital
