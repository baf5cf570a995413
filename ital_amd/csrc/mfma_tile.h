// The 128 x 128 LDS-staged v_mfma_f64_16x16x4_f64 tile of the dense FP64 kernels, in one place.  Used by
//
//   dense.hip     gram_kernel, chol_syrk_kernel, kernel_w_kernel   (tile_nt: both operands row-major, read through row pointers)
//   evidence.hip  gram_grid_kernel                                 (tile_nt)
//   adapt.hip     inv_lm_kernel, inv_mt_kernel                     (its own tile_mm: predicated element functors, second operand
//                                                                   k-major; it shares the constants, the LDS layout and mfma_stage)
//   evidence_grad.hip, loo_grad.hip   gram_inverse_kernel and the W products   (tile_tn: both operands k-major behind predicates)
//   influence.hip influence_tile_kernel                            (tile_tn: M^T V, both stored k-major)
//
// cov_block_lds_kernel (mcmi.hip), which this tile was taken from, keeps its own copy: its unit is in the include closures
// that tools/stamp.py hashes and its code generation is pinned by goldens and stamped profiles.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ital {
namespace tile {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int T = 128;         // output tile edge of the MFMA kernels
constexpr int KS = 16;         // k-elements per LDS stage
constexpr int LDT = T + 4;     // padded row stride of a staged tile (doubles)

typedef double StageLds[2][2][KS][LDT];   // [buffer][A / B][k][row]; 66 KB: relies on gfx950's 160 KB of LDS per CU

// Lower-triangular tile pair (ti >= tj) of a linear block index t = ti (ti + 1) / 2 + tj.
__device__ inline void tri_pair(int64_t t, int& ti, int& tj) {
    int r = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((int64_t)(r + 1) * (r + 2) / 2 <= t) r++;
    while ((int64_t)r * (r + 1) / 2 > t) r--;
    ti = r;
    tj = (int)(t - (int64_t)r * (r + 1) / 2);
}

// Staging role of a thread (as in cov_block_lds_kernel): k-pair sk, sk + 1 of the tile rows srow + 8 u, u = 0..3.
__device__ inline void stage_role(int& sk, int& srow) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    sk = 2 * ((lane & 3) + 4 * (lane >> 5));
    srow = 32 * wave + ((lane >> 2) & 7);
}

// Where the calling lane's accumulators sit in the 128 x 128 tile (D layout of the f64 MFMA): wave (wy, wx) owns the
// 64 x 64 quarter at (64 wy, 64 wx); acc[p][q][reg] is the element at tile row row(p, reg), tile column column(q).
// The epilogues of dense.hip and evidence.hip add the same terms to a 64-bit tile origin one by one instead: through row()
// and column() the compiler spends more registers there (gram_grid_kernel 214 -> 218 VGPRs, kernel_w_kernel spills more).
struct DLane {
    int col, kg, wy, wx;
    __device__ int row(int p, int reg) const { return 64 * wy + 16 * p + kg + 4 * reg; }
    __device__ int column(int q) const { return 64 * wx + 16 * q + col; }
};

__device__ inline DLane d_lane() {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    return {lane & 15, lane >> 4, wave >> 1, wave & 1};
}

// One staged k-step (KS elements of k from lds[buf]) for the calling wave's 64 x 64 quarter: 16 LDS reads, 16 MFMAs.
__device__ inline void mfma_stage(StageLds& lds, int buf, d4 acc[4][4]) {
    const DLane dl = d_lane();
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double av[4], bv[4];
#pragma unroll
        for (int p = 0; p < 4; p++) av[p] = lds[buf][0][4 * dl.kg + j][64 * dl.wy + 16 * p + dl.col];
#pragma unroll
        for (int q = 0; q < 4; q++) bv[q] = lds[buf][1][4 * dl.kg + j][dl.column(q)];
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int q = 0; q < 4; q++) acc[p][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[p], bv[q], acc[p][q], 0, 0, 0);
    }
}

// acc[p][q] += sum_k A_r[k] B_c[k] over k < K (a multiple of KS) for the 128 x 128 tile of a workgroup of 256 threads: wave
// (wy, wx) owns rows 64 wy + 16 p + (kg + 4 reg) of A and columns 64 wx + 16 q + col of B (D layout of the f64 MFMA).
// pa[u] / pb[u]: this thread's staged rows srow + 8 u of A / B, already offset by sk.  Register + LDS double buffer, one
// barrier per stage; ends with a barrier, so the caller may reuse `lds`.
__device__ inline void tile_nt(const double* const pa[4], const double* const pb[4], int K, StageLds& lds, d4 acc[4][4]) {
    int sk, srow;
    stage_role(sk, srow);
    double2 ra[4], rb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            ra[u].x = pa[u][k0];
            ra[u].y = pa[u][k0 + 1];
            rb[u].x = pb[u][k0];
            rb[u].y = pb[u][k0 + 1];
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            lds[buf][0][sk][srow + 8 * u] = ra[u].x;
            lds[buf][0][sk + 1][srow + 8 * u] = ra[u].y;
            lds[buf][1][sk][srow + 8 * u] = rb[u].x;
            lds[buf][1][sk + 1][srow + 8 * u] = rb[u].y;
        }
    };
    fetch(0);
    stage(0);
    __syncthreads();
    const int nstep = K / KS;
    for (int s_ = 0; s_ < nstep; s_++) {
        const int buf = s_ & 1;
        if (s_ + 1 < nstep) fetch((s_ + 1) * KS);
        mfma_stage(lds, buf, acc);
        if (s_ + 1 < nstep) stage(buf ^ 1);
        __syncthreads();
    }
}

// acc[p][q] += sum over kbeg <= k < kend of A(k, r) B(k, c) for the 128 x 128 tile of a workgroup of 256 threads: wave
// (wy, wx) owns tile rows 64 wy + 16 p + (kg + 4 reg) and tile columns 64 wx + 16 q + col (D layout of the f64 MFMA).
// fa(k, r) / fb(k, c): the element of A at tile row r / of B at tile column c, both k-major; they return 0 outside their
// operand (k at or past kend included).  Thread (k = tid / 16, tid % 16) stages eight runs of 16 columns of its k for each
// operand, into the layout mfma_stage reads.  Register + LDS double buffer, one barrier per stage; ends with a barrier.
template <class FA, class FB>
__device__ inline void tile_tn(FA fa, FB fb, int kbeg, int kend, StageLds& lds, d4 acc[4][4]) {
    const int kb = threadIdx.x >> 4, c16 = threadIdx.x & 15;
    double ra[8], rb[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 8; u++) {
            ra[u] = fa(k0 + kb, c16 + 16 * u);
            rb[u] = fb(k0 + kb, c16 + 16 * u);
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 8; u++) {
            lds[buf][0][kb][c16 + 16 * u] = ra[u];
            lds[buf][1][kb][c16 + 16 * u] = rb[u];
        }
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

__device__ inline void zero_acc(d4 acc[4][4]) {
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[p][q] = (d4){0, 0, 0, 0};
}

// Squared distance from the squared norms and the dot product, the reference's expansion A + B - 2 C (gp.py:410-416); like
// the reference's it is not clamped at 0.
__device__ inline double rbf_sqdist(double na, double nb, double dot) { return na + nb - 2 * dot; }

}  // namespace tile
}  // namespace ital
