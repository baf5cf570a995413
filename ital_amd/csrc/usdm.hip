// Device side of the USDM learner (ital_amd/usdm.py), the reference's ital/baseline_methods.py:575-658:
//
//   ital_usdm_laplacian  M = D_uu - W_uu and rhs = W_ul y of the harmonic label propagation, from the neighbour lists
//   ital_lu_factor       blocked right-looking LU without pivoting of that (row diagonally dominant) matrix, in place
//   ital_lu_solve        p = U^-1 L^-1 rhs
//   ital_usdm_shift      K + mu 11^T + mu I of one iteration of the augmented-Lagrangian loop (lower triangle)
//   ital_symv_lower      K f from the lower triangle, for the loop's objective
//
// The LU is laid out as the Cholesky of dense.hip: 64 x 64 diagonal blocks (one workgroup, LDS), the two panels as VALU
// work (L21 = A21 U11^-1 one row per thread, U12 = L11^-1 A12 one column per thread, so a wave's loads run along a row),
// and the trailing update A22 -= L21 U12 over all 128 x 128 tiles on v_mfma_f64_16x16x4_f64 through the LDS-staged tile of
// mfma_tile.h.  tile_mm below is the A * B tile loop of adapt.hip (second operand k-major, every element behind a
// predicate), kept here as knn.hip and adapt.hip keep theirs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ital_internal.h"
#include "ital_usdm.h"
#include "mfma_tile.h"

namespace ital {
namespace usdm {

using namespace ital::tile;

constexpr int NB = 64;          // LU block, and the block edge of the symmetric matrix-vector product
constexpr int MAX_K = 32;       // ITAL_KNN_MAX_K

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

// ----------------------------------------------------------------------------------------------------------- Laplacian
struct LapArgs {
    const int64_t* idx; int k; int64_t n;
    const int64_t* u; int64_t n_u; const int64_t* pos; const unsigned char* rel; int64_t n_rel;
    double eps; double* M; int64_t ld; double* rhs;
};

// One row of M per workgroup pass.  The positions in u of the row's neighbours sit in LDS; every element of the row is
// compared against them, so one thread writes one element once and a list with a repeated entry gives the same bits.
__global__ __launch_bounds__(256) void laplacian_kernel(LapArgs a) {
    __shared__ int64_t nb[MAX_K];
    const int tid = threadIdx.x;
    const double w1 = __dadd_rn(1.0, a.eps);
    const double deg = __dadd_rn((double)a.k, __dmul_rn((double)a.n, a.eps));
    const double diag = __dadd_rn(deg, -a.eps);
    const double base = __dmul_rn((double)a.n_rel, a.eps);
    for (int64_t r = blockIdx.x; r < a.n_u; r += gridDim.x) {
        const int64_t i = a.u[r];
        if (tid < 64) {                                    // k <= 32: the lists are read by the first wave
            int64_t p = -1;
            bool relevant = false;
            if (tid < a.k && i >= 0 && i < a.n) {
                const int64_t j = a.idx[i * a.k + tid];
                if (j >= 0 && j < a.n) {
                    p = a.pos[j];
                    relevant = a.rel[j] != 0;
                }
            }
            if (tid < a.k) nb[tid] = p;
            const int c = __popcll(__ballot(relevant));
            if (tid == 0) a.rhs[r] = __dadd_rn((double)c, base);
        }
        __syncthreads();
        double* row = a.M + r * a.ld;
        for (int64_t b = tid; b < a.n_u; b += 256) {
            double v = -a.eps;
            for (int s_ = 0; s_ < a.k; s_++)
                if (nb[s_] == b) v = -w1;
            if (b == r) v = diag;
            row[b] = v;
        }
        __syncthreads();                                   // nb is rewritten by the next pass
    }
}

// ------------------------------------------------------------------------------------------------------------------ LU
struct LuArgs {
    double* A; int n; int64_t ld; int* info; int* status; int k0;
};

// Unblocked right-looking factor of the diagonal block at (k0, k0), staged in LDS; one workgroup.  A pivot that is not > 0
// (NaN included) records info = column + 1, sets status bit 1 and stops: the later kernels of the call do nothing.
__global__ __launch_bounds__(256) void lu_diag_kernel(LuArgs a) {
    __shared__ double s[NB][NB + 1];
    const int n = a.n, k0 = a.k0;
    if (k0 >= n || *a.info != 0) return;
    const int m = min(NB, n - k0);
    double* A = a.A + (int64_t)k0 * a.ld + k0;
    const int tid = threadIdx.x;
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e / NB, c = e % NB;
        if (r < m && c < m) s[r][c] = A[(int64_t)r * a.ld + c];
    }
    __syncthreads();
    for (int j = 0; j < m; j++) {
        const double d = s[j][j];
        if (!(d > 0)) {                     // the same value in every thread: the whole workgroup leaves
            if (tid == 0) {
                *a.info = k0 + j + 1;
                atomicOr(a.status, 1);
            }
            return;
        }
        for (int r = j + 1 + tid; r < m; r += 256) s[r][j] /= d;
        __syncthreads();
        const int w = m - j - 1;
        for (int e = tid; e < w * w; e += 256) {
            const int r = j + 1 + e / w, c = j + 1 + e % w;
            s[r][c] -= s[r][j] * s[j][c];
        }
        __syncthreads();
    }
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e / NB, c = e % NB;
        if (r < m && c < m) A[(int64_t)r * a.ld + c] = s[r][c];
    }
}

// The two panels of a full diagonal block (only those have rows below and columns to the right).  blockIdx.y == 0:
// L21 = A21 U11^-1, one row per thread (substitution against the columns of U11); blockIdx.y == 1: U12 = L11^-1 A12, one
// column per thread (substitution against the rows of the unit lower L11), the loads of a wave contiguous along the row.
__global__ __launch_bounds__(256) void lu_panel_kernel(LuArgs a) {
    __shared__ double f[NB][NB + 1];
    const int n = a.n, k0 = a.k0;
    if (k0 + NB >= n || *a.info != 0) return;
    double* A = a.A;
    const int64_t ld = a.ld;
    for (int e = threadIdx.x; e < NB * NB; e += 256) {
        const int r = e / NB, c = e % NB;
        f[r][c] = A[(int64_t)(k0 + r) * ld + k0 + c];
    }
    __syncthreads();
    const int64_t t = (int64_t)k0 + NB + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    double x[NB];
    if (blockIdx.y == 0) {
        double* row = A + t * ld + k0;
#pragma unroll
        for (int c = 0; c < NB; c++) x[c] = row[c];
#pragma unroll
        for (int c = 0; c < NB; c++) {
            double v = x[c];
#pragma unroll
            for (int p = 0; p < c; p++) v -= x[p] * f[p][c];
            x[c] = v / f[c][c];
        }
#pragma unroll
        for (int c = 0; c < NB; c++) row[c] = x[c];
    } else {
        double* col = A + (int64_t)k0 * ld + t;
#pragma unroll
        for (int r = 0; r < NB; r++) x[r] = col[(int64_t)r * ld];
#pragma unroll
        for (int r = 1; r < NB; r++) {
            double v = x[r];
#pragma unroll
            for (int p = 0; p < r; p++) v -= f[r][p] * x[p];
            x[r] = v;
        }
#pragma unroll
        for (int r = 1; r < NB; r++) col[(int64_t)r * ld] = x[r];
    }
}

// Trailing update A22 -= L21 U12 over all 128 x 128 tiles of the (n - k1) x (n - k1) block, k1 = k0 + 64.
__global__ __launch_bounds__(256, 2) void lu_gemm_kernel(LuArgs a, int tiles) {
    __shared__ StageLds lds;
    const int n = a.n, k0 = a.k0, k1 = k0 + NB;
    if (k1 >= n || *a.info != 0) return;
    const int64_t i0 = (int64_t)k1 + (int64_t)(blockIdx.x / tiles) * T, j0 = (int64_t)k1 + (int64_t)(blockIdx.x % tiles) * T;
    if (i0 >= n || j0 >= n) return;
    const int64_t ld = a.ld;
    double* A = a.A;
    auto fa = [&](int r, int k) {
        const int64_t i = i0 + r;
        return (i < n && k < NB) ? A[i * ld + k0 + k] : 0.0;
    };
    auto fb = [&](int k, int c) {
        const int64_t j = j0 + c;
        return (j < n && k < NB) ? A[(int64_t)(k0 + k) * ld + j] : 0.0;
    };
    d4 acc[4][4];
    zero_acc(acc);
    tile_mm(fa, fb, 0, NB, lds, acc);
    const DLane dl = d_lane();
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int64_t j = j0 + dl.column(q);
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int64_t i = i0 + dl.row(p, reg);
                if (i < n && j < n) A[i * ld + j] -= acc[p][q][reg];
            }
    }
}

// y <- U^-1 L^-1 y, one workgroup: blocks of NB unknowns, the diagonal block by wave 0 (one unknown per lane), the rest of
// the vector updated by all threads (chol_solve_kernel of dense.hip with a unit lower and a separate upper factor).
__global__ __launch_bounds__(256) void lu_solve_kernel(const double* LU, int n, int64_t ld, double* y, const int* info) {
    __shared__ double xs[NB];
    if (n <= 0 || (info && *info != 0)) return;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int kb = 0; kb < n; kb += NB) {                // L z = y, L unit lower
        const int m = min(NB, n - kb);
        if (tid < 64) {
            double v = lane < m ? y[kb + lane] : 0.0;
            for (int c = 0; c < m; c++) {
                const double xc = __shfl(v, c, 64);
                if (lane > c && lane < m) v -= LU[(int64_t)(kb + lane) * ld + kb + c] * xc;
            }
            if (lane < m) {
                y[kb + lane] = v;
                xs[lane] = v;
            }
        }
        __syncthreads();
        for (int64_t i = (int64_t)kb + m + tid; i < n; i += 256) {
            const double* row = LU + i * ld + kb;
            double v = y[i];
            for (int c = 0; c < m; c++) v -= row[c] * xs[c];
            y[i] = v;
        }
        __syncthreads();
    }
    for (int kb = ((n - 1) / NB) * NB; kb >= 0; kb -= NB) {     // U x = z
        const int m = min(NB, n - kb);
        if (tid < 64) {
            double v = lane < m ? y[kb + lane] : 0.0;
            for (int r = m - 1; r >= 0; r--) {
                const double xr = __shfl(v, r, 64) / LU[(int64_t)(kb + r) * ld + kb + r];
                if (lane == r) v = xr;
                if (lane < r) v -= LU[(int64_t)(kb + lane) * ld + kb + r] * xr;
            }
            if (lane < m) {
                y[kb + lane] = v;
                xs[lane] = v;
            }
        }
        __syncthreads();
        for (int64_t i = tid; i < kb; i += 256) {
            const double* row = LU + i * ld + kb;
            double v = y[i];
            for (int c = 0; c < m; c++) v -= row[c] * xs[c];
            y[i] = v;
        }
        __syncthreads();
    }
}

// --------------------------------------------------------------------------------------------------------------- shift
// grid: (column chunks of 256, rows); a chunk that starts right of the diagonal has nothing to write.
__global__ __launch_bounds__(256) void shift_kernel(const double* K, int64_t n, int64_t ldk, double mu, double* B, int64_t ldb) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t i = blockIdx.y; i < n; i += gridDim.y) {
        if (j > i) continue;
        double v = __dadd_rn(K[i * ldk + j], mu);
        if (i == j) v = __dadd_rn(v, mu);
        B[i * ldb + j] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- symv
// One 64 x 64 block (ti, tj), tj <= ti, of the lower triangle per workgroup, staged in LDS (a diagonal block is mirrored
// there).  Its products with x give 64 partial sums for the outputs of block row ti, written to work[tj][64 ti ..], and,
// off the diagonal, 64 for the outputs of block row tj, written to work[ti][64 tj ..]: slot [t][I] of the workspace has
// exactly one writer.  Sixteen products per thread, then the four sixteenths in ascending order.
__global__ __launch_bounds__(256) void symv_block_kernel(const double* K, int64_t n, int64_t ld, const double* x, double* work,
                                                         int64_t npad) {
    __shared__ double s[NB][NB + 1];
    __shared__ double xs[2][NB];
    __shared__ double red[2][4][NB];
    int ti, tj;
    tri_pair(blockIdx.x, ti, tj);
    const int64_t i0 = (int64_t)ti * NB, j0 = (int64_t)tj * NB;
    if (i0 >= n) return;
    const int tid = threadIdx.x, c = tid & 63, g = tid >> 6;
    for (int rr = 0; rr < 16; rr++) {
        const int r = 16 * g + rr;
        const int64_t i = i0 + r, j = j0 + c;
        s[r][c] = (i < n && j <= i) ? K[i * ld + j] : 0.0;
    }
    if (g == 0) xs[0][c] = j0 + c < n ? x[j0 + c] : 0.0;
    if (g == 1) xs[1][c] = i0 + c < n ? x[i0 + c] : 0.0;
    __syncthreads();
    if (ti == tj) {
        for (int rr = 0; rr < 16; rr++) {
            const int r = 16 * g + rr;
            if (r < c) s[r][c] = s[c][r];     // reads below the diagonal, writes above it
        }
        __syncthreads();
    }
    {
        double v = 0.0;                       // row c of the block, columns 16 g .. 16 g + 15
        for (int q = 0; q < 16; q++) v += s[c][16 * g + q] * xs[0][16 * g + q];
        red[0][g][c] = v;
        double w = 0.0;                       // column c of the block, rows 16 g .. 16 g + 15
        for (int q = 0; q < 16; q++) w += s[16 * g + q][c] * xs[1][16 * g + q];
        red[1][g][c] = w;
    }
    __syncthreads();
    if (g == 0) work[(int64_t)tj * npad + i0 + c] = ((red[0][0][c] + red[0][1][c]) + red[0][2][c]) + red[0][3][c];
    if (g == 1 && ti != tj) work[(int64_t)ti * npad + j0 + c] = ((red[1][0][c] + red[1][1][c]) + red[1][2][c]) + red[1][3][c];
}

// out[i] = sum_t work[t][i], t ascending
__global__ __launch_bounds__(256) void symv_sum_kernel(const double* work, int64_t n, int64_t npad, int nt, double* out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v = 0.0;
    for (int t = 0; t < nt; t++) v += work[(int64_t)t * npad + i];
    out[i] = v;
}

constexpr int64_t MAX_N = (int64_t)INT32_MAX - 128;

__host__ inline bool misaligned(const void* p) { return ((uintptr_t)p & 7) != 0; }

}  // namespace usdm
}  // namespace ital

using namespace ital::usdm;

extern "C" int ital_usdm_laplacian(const int64_t* idx, int k, int64_t n, const int64_t* u, int64_t n_u, const int64_t* pos,
                                   const unsigned char* rel, int64_t n_rel, double eps, double* M, int64_t ld, double* rhs,
                                   hipStream_t stream) {
    if (k < 1 || k > MAX_K) return ital_fail(-22, "ital_usdm_laplacian: k must be between 1 and 32");
    if (n < 0 || n > MAX_N) return ital_fail(-22, "ital_usdm_laplacian: n out of range");
    if (n_u < 0 || n_u > n) return ital_fail(-22, "ital_usdm_laplacian: n_u must be between 0 and n");
    if (n_rel < 0 || n_rel > n) return ital_fail(-22, "ital_usdm_laplacian: n_rel must be between 0 and n");
    if (ld < n_u) return ital_fail(-22, "ital_usdm_laplacian: ld must be at least n_u");
    if (n_u == 0) return 0;
    if (!idx || !u || !pos || !rel || !M || !rhs) return ital_fail(-22, "ital_usdm_laplacian: NULL pointer");
    if (misaligned(idx) || misaligned(u) || misaligned(pos) || misaligned(M) || misaligned(rhs))
        return ital_fail(-22, "ital_usdm_laplacian: idx, u, pos, M and rhs must be aligned to 8 bytes");
    LapArgs a = {idx, k, n, u, n_u, pos, rel, n_rel, eps, M, ld, rhs};
    const int64_t grid = n_u < (1 << 20) ? n_u : (1 << 20);
    ITAL_LAUNCH(laplacian_kernel, dim3((unsigned)grid), dim3(256), 0, stream, a);
    return ital_check_launch("ital_usdm_laplacian");
}

extern "C" int ital_lu_factor(double* A, int64_t n, int64_t ld, int* info, int* status, hipStream_t stream) {
    if (n < 0 || n > MAX_N) return ital_fail(-22, "ital_lu_factor: n out of range");
    if (ld < n) return ital_fail(-22, "ital_lu_factor: ld must be at least n");
    if (n == 0) return 0;
    if (!A || !info || !status) return ital_fail(-22, "ital_lu_factor: A, info and status are required");
    if (misaligned(A) || ((uintptr_t)info & 3) || ((uintptr_t)status & 3))
        return ital_fail(-22, "ital_lu_factor: A must be aligned to 8 bytes, info and status to 4");
    const int64_t tr0 = (n + T - 1) / T;
    if (tr0 * tr0 > INT32_MAX) return ital_fail(-22, "ital_lu_factor: matrix too large");
    if (hipMemsetAsync(info, 0, sizeof(int), stream) != hipSuccess) return ital_fail(-5, "ital_lu_factor: hipMemsetAsync failed");
    LuArgs a = {A, (int)n, ld, info, status, 0};
    for (int64_t k0 = 0; k0 < n; k0 += NB) {
        a.k0 = (int)k0;
        ITAL_LAUNCH(lu_diag_kernel, dim3(1), dim3(256), 0, stream, a);
        const int64_t below = n - k0 - NB;
        if (below > 0) {
            ITAL_LAUNCH(lu_panel_kernel, dim3((unsigned)((below + 255) / 256), 2), dim3(256), 0, stream, a);
            const int64_t tr = (below + T - 1) / T;
            ITAL_LAUNCH(lu_gemm_kernel, dim3((unsigned)(tr * tr)), dim3(256), 0, stream, a, (int)tr);
        }
        const int rc = ital_check_launch("ital_lu_factor");
        if (rc) return rc;
    }
    return 0;
}

extern "C" int ital_lu_solve(const double* LU, int64_t n, int64_t ld, double* y, const int* info, hipStream_t stream) {
    if (n < 0 || n > MAX_N) return ital_fail(-22, "ital_lu_solve: n out of range");
    if (ld < n) return ital_fail(-22, "ital_lu_solve: ld must be at least n");
    if (n == 0) return 0;
    if (!LU || !y) return ital_fail(-22, "ital_lu_solve: LU and y are required");
    if (misaligned(LU) || misaligned(y) || ((uintptr_t)info & 3))
        return ital_fail(-22, "ital_lu_solve: LU and y must be aligned to 8 bytes, info to 4");
    ITAL_LAUNCH(lu_solve_kernel, dim3(1), dim3(256), 0, stream, LU, (int)n, ld, y, info);
    return ital_check_launch("ital_lu_solve");
}

extern "C" int ital_usdm_shift(const double* K, int64_t n, int64_t ldk, double mu, double* B, int64_t ldb,
                               hipStream_t stream) {
    if (n < 0 || n > MAX_N) return ital_fail(-22, "ital_usdm_shift: n out of range");
    if (ldk < n || ldb < n) return ital_fail(-22, "ital_usdm_shift: ldk and ldb must be at least n");
    if (n == 0) return 0;
    if (!K || !B) return ital_fail(-22, "ital_usdm_shift: K and B are required");
    if (misaligned(K) || misaligned(B)) return ital_fail(-22, "ital_usdm_shift: K and B must be aligned to 8 bytes");
    const int64_t gy = n < 65535 ? n : 65535;
    ITAL_LAUNCH(shift_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)gy), dim3(256), 0, stream, K, n, ldk, mu, B, ldb);
    return ital_check_launch("ital_usdm_shift");
}

extern "C" int64_t ital_symv_lower_workspace(int64_t n) {
    if (n <= 0 || n > MAX_N) return 0;
    const int64_t nt = (n + NB - 1) / NB;
    return nt * nt * NB;
}

extern "C" int ital_symv_lower(const double* K, int64_t n, int64_t ld, const double* x, double* out, double* work,
                               int64_t work_doubles, hipStream_t stream) {
    if (n < 0 || n > MAX_N) return ital_fail(-22, "ital_symv_lower: n out of range");
    if (ld < n) return ital_fail(-22, "ital_symv_lower: ld must be at least n");
    if (n == 0) return 0;
    if (!K || !x || !out || !work) return ital_fail(-22, "ital_symv_lower: K, x, out and work are required");
    if (misaligned(K) || misaligned(x) || misaligned(out) || misaligned(work))
        return ital_fail(-22, "ital_symv_lower: K, x, out and work must be aligned to 8 bytes");
    if (work_doubles < ital_symv_lower_workspace(n))
        return ital_fail(-22, "ital_symv_lower: work smaller than ital_symv_lower_workspace(n)");
    const int64_t nt = (n + NB - 1) / NB, pairs = nt * (nt + 1) / 2, npad = nt * NB;
    if (pairs > INT32_MAX) return ital_fail(-22, "ital_symv_lower: matrix too large");
    ITAL_LAUNCH(symv_block_kernel, dim3((unsigned)pairs), dim3(256), 0, stream, K, n, ld, x, work, npad);
    int rc = ital_check_launch("ital_symv_lower");
    if (rc) return rc;
    ITAL_LAUNCH(symv_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const double*)work, n, npad, (int)nt,
                out);
    return ital_check_launch("ital_symv_lower(sum)");
}
