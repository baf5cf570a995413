// Trusting a label less: a signed change of diagonal entries of the labelled Gram, carried through the Cholesky-whitened GP
// state (include/ital_reweigh.h).
//
// K_pp + delta is the rank-one update (delta > 0) or downdate (delta < 0) of the trailing block of L with x = sqrt(|delta|) e_p.
// Top-down, k = p .. m-1:  r = sqrt(L_kk^2 +- x_k^2), c = r / L_kk, s = x_k / L_kk, L_kk <- r; rows i > k:
// L_ik <- (L_ik +- s x_i) / c, x_i <- c x_i - s L_ik (the new one) -- Givens rotations for the update, the mixed form of the
// hyperbolic rotations (Bojanczyk, Brent, Van Dooren, de Hoog 1987) for the downdate.  alpha = L^-1 y and every column of
// V = L^-1 K_T,: go through the same recurrence as one more row of L would, with a carry that starts at 0; what is left in the
// carry corrects the means and variances.  Only the pair (row k, carry of chain j) is touched by rotation (j, k), so up to eight
// chains run in ONE pass over V: at row k the rotations of the chains in chain order.
//
// reweigh_factor_kernel: one workgroup, latency-bound, the panel scheme of remove_factor_kernel (csrc/revoke.hip) on a COPY of
// the trailing block in the workspace, chain after chain; alpha rides along as the row below the last one.  The copy is written
// back only if every pivot of every chain was positive and finite; otherwise the "refused" word of the workspace is set.
// reweigh_sweep_kernel: a stream over rows pos[0] .. m-1 of V, in place; it returns before its first store when refused.
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>

#include "ital_hip.h"
#include "ital_internal.h"
#include "ital_reweigh.h"

namespace ital {

constexpr int kPass = ITAL_REWEIGH_PASS;
constexpr int kRwThreads = 512;

// one rotation as the sweep uses it: v <- (v + sk u) ic, u <- c u - s v  (ic = 1 / c, sk = +s: update, -s: downdate)
struct alignas(16) Rot {
    double ic, sk, c, s;
};

struct Chains {
    int pos[kPass];
    double delta[kPass];
};

// work: [0] refused (0.0 / 1.0); [kRwHdr + 2 j, + 1] (g, h) of chain j: mu += g u_j, s2 += h u_j^2; then Rot[r][m] indexed by
// (chain, row); then the carries of the rows (n3 + 1 <= m + 1); then the trailing block with alpha as its last row,
// [n3 + 1][n3], n3 = m - pos[0]
constexpr int kRwHdr = 8;
__host__ __device__ inline int64_t rw_rot_off(int r) { return kRwHdr + 2 * (int64_t)r; }
__host__ __device__ inline int64_t rw_x_off(int m, int r) { return rw_rot_off(r) + 4 * (int64_t)r * m; }
__host__ __device__ inline int64_t rw_s_off(int m, int r) { return rw_x_off(m, r) + (m + 2) + (m & 1); }

__device__ __forceinline__ double rw_bcast(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

__global__ __launch_bounds__(kRwThreads) void reweigh_factor_kernel(double* __restrict__ L, int ldl, double* __restrict__ alpha,
                                                                    double* __restrict__ ws, int m, int p0, int r, int j0, int nc,
                                                                    Chains ch, int first, int last, int* __restrict__ status) {
    __shared__ double Lb[64][65];    // one 64 x 64 diagonal block of the trailing factor at a time
    __shared__ double xb[64];        // the carries of its rows
    __shared__ Rot rb[64];           // the rotations it fixes
    __shared__ int bad_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n3 = m - p0;           // rows from the first position of the call on
    double* gh = ws + kRwHdr;
    Rot* rot = reinterpret_cast<Rot*>(ws + rw_rot_off(r));
    double* xv = ws + rw_x_off(m, r);
    double* S = ws + rw_s_off(m, r);                 // S[t][k] = L[p0 + t][p0 + k]; S[n3][k] = alpha[p0 + k]

    if (tid == 0) bad_s = 0;
    if (first) {
        for (int idx = tid; idx < n3 * n3; idx += kRwThreads) {
            const int t = idx / n3, k = idx - t * n3;
            S[idx] = k <= t ? L[(int64_t)(p0 + t) * ldl + p0 + k] : 0.0;
        }
        for (int k = tid; k < n3; k += kRwThreads) S[(int64_t)n3 * n3 + k] = alpha[p0 + k];
        if (tid == 0) ws[0] = 0.0;
    } else if (ws[0] != 0.0) {
        return;                      // an earlier group of this call was refused (the whole workgroup reads the same word)
    }
    __threadfence_block();
    __syncthreads();

    const int qg = ch.pos[0];        // the sweep of this group starts here: the later chains are the identity above their row
    for (int jj = 0; jj < nc; jj++) {
        const int p = ch.pos[jj];
        const double kind = ch.delta[jj] < 0 ? -1.0 : 1.0;
        const double x0 = sqrt(fabs(ch.delta[jj]));
        Rot* rj = rot + (int64_t)(j0 + jj) * m;
        for (int q = qg + tid; q < p; q += kRwThreads) rj[q] = Rot{1.0, 0.0, 1.0, 0.0};
        for (int t = tid; t <= n3; t += kRwThreads) xv[t] = t == p - p0 ? x0 : 0.0;
        __threadfence_block();
        __syncthreads();

        for (int k0 = p - p0; k0 < n3; k0 += 64) {
            const int nb = n3 - k0 < 64 ? n3 - k0 : 64;
            for (int idx = tid; idx < nb * nb; idx += kRwThreads) {
                const int i = idx / nb, q = idx - i * nb;
                Lb[i][q] = q <= i ? S[(int64_t)(k0 + i) * n3 + k0 + q] : 0.0;
            }
            if (tid < nb) xb[tid] = xv[k0 + tid];
            __syncthreads();
            if (wave == 0) {
                // diagonal block: lane i carries row k0 + i; column k fixes rotation k0 + k from lane k's carry and diagonal
                const bool in = lane < nb;
                double xi = in ? xb[lane] : 0.0;
                double* Srow = S + (int64_t)(k0 + (in ? lane : 0)) * n3 + k0;
                bool bad = false;
                double tik = in ? Lb[lane][0] : 0.0;
                for (int k = 0; k < nb; k++) {
                    const double tnext = in ? Lb[lane][k + 1 < nb ? k + 1 : k] : 0.0;   // next column, off the dependent chain
                    const double d = Lb[k][k];
                    const double xk = rw_bcast(xi, k);
                    const double rr = kind > 0 ? sqrt(fma(xk, xk, d * d)) : sqrt((d - xk) * (d + xk));
                    if (!(rr > 0) || !(rr < INFINITY) || !(d > 0)) bad = true;
                    const Rot g = Rot{d / rr, kind * (xk / d), rr / d, xk / d};
                    if (lane == k) {
                        Srow[k] = rr;
                        rb[k] = g;
                        rj[p0 + k0 + k] = g;
                    } else if (in && lane > k) {
                        const double tn = (tik + g.sk * xi) * g.ic;
                        Srow[k] = tn;
                        xi = g.c * xi - g.s * tn;
                    }
                    tik = tnext;
                }
                if (bad && lane == 0) bad_s = 1;
            }
            __syncthreads();
            // rows below the panel, alpha (row n3) among them: one thread per row, the panel's rotations on its carry
            for (int t = k0 + nb + tid; t <= n3; t += kRwThreads) {
                double xi = xv[t];
                double* Sr = S + (int64_t)t * n3 + k0;
                int kk = 0;
                for (; kk + 16 <= nb; kk += 16) {
                    double tv[16];
#pragma unroll
                    for (int u = 0; u < 16; u++) tv[u] = Sr[kk + u];
#pragma unroll
                    for (int u = 0; u < 16; u++) {
                        const Rot g = rb[kk + u];
                        const double tn = (tv[u] + g.sk * xi) * g.ic;
                        Sr[kk + u] = tn;
                        xi = g.c * xi - g.s * tn;
                    }
                }
                for (; kk < nb; kk++) {
                    const Rot g = rb[kk];
                    const double tn = (Sr[kk] + g.sk * xi) * g.ic;
                    Sr[kk] = tn;
                    xi = g.c * xi - g.s * tn;
                }
                xv[t] = xi;
            }
            __threadfence_block();
            __syncthreads();
        }
        if (tid == 0) {
            gh[2 * (j0 + jj)] = -kind * xv[n3];      // update: mu' = mu - u a_u; downdate: mu' = mu + u a_u
            gh[2 * (j0 + jj) + 1] = kind;            // update: s2' = s2 + u^2;   downdate: s2' = s2 - u^2
        }
        __syncthreads();
    }

    if (bad_s) {
        if (tid == 0) {
            ws[0] = 1.0;
            atomicOr(status, 1);
        }
        return;
    }
    if (!last) return;
    for (int idx = tid; idx < n3 * n3; idx += kRwThreads) {
        const int t = idx / n3, k = idx - t * n3;
        if (k <= t) L[(int64_t)(p0 + t) * ldl + p0 + k] = S[idx];
    }
    for (int k = tid; k < n3; k += kRwThreads) alpha[p0 + k] = S[(int64_t)n3 * n3 + k];
}

// Rows q0 .. m-1 of V through the NC chains of one group, in place; then mu += sum g_j u_j, s2 += sum h_j u_j^2.  A lane owns
// two adjacent columns (16-byte loads and stores) and their 2 NC carries; a row is read and written by that lane alone.  Only
// the FMAs depend on the carries: the loads of eight rows are in flight together.  The coefficients are the same for the whole
// wave (scalar loads).
constexpr int kRwRows = 8;

template <int NC>
__device__ __forceinline__ double2 rw_row(double2 v, double2 (&u)[NC], const Rot* __restrict__ rot, int m, int q) {
#pragma unroll
    for (int j = 0; j < NC; j++) {
        const Rot g = rot[(int64_t)j * m + q];
        v.x = (v.x + g.sk * u[j].x) * g.ic;
        v.y = (v.y + g.sk * u[j].y) * g.ic;
        u[j].x = g.c * u[j].x - g.s * v.x;
        u[j].y = g.c * u[j].y - g.s * v.y;
    }
    return v;
}

template <int NC>
__global__ __launch_bounds__(256) void reweigh_sweep_kernel(double* __restrict__ V, int64_t ldv, int64_t n, double* __restrict__ mu,
                                                            double* __restrict__ s2, const double* __restrict__ ws, int m, int r,
                                                            int j0, int q0) {
    const int64_t j = 2 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
    if (j >= ldv) return;            // ldv is even: a pair never straddles the end
    if (ws[0] != 0.0) return;        // refused: nothing is stored
    const double* __restrict__ gh = ws + kRwHdr + 2 * j0;
    const Rot* __restrict__ rot = reinterpret_cast<const Rot*>(ws + rw_rot_off(r)) + (int64_t)j0 * m;
    double* col = V + j;
    double2 u[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) u[c] = double2{0.0, 0.0};
    int q = q0;
    for (; q + kRwRows <= m; q += kRwRows) {
        double2 y[kRwRows];
#pragma unroll
        for (int t = 0; t < kRwRows; t++) y[t] = *reinterpret_cast<const double2*>(col + (int64_t)(q + t) * ldv);
#pragma unroll
        for (int t = 0; t < kRwRows; t++)
            *reinterpret_cast<double2*>(col + (int64_t)(q + t) * ldv) = rw_row<NC>(y[t], u, rot, m, q + t);
    }
    for (; q < m; q++) {
        const double2 y = *reinterpret_cast<const double2*>(col + (int64_t)q * ldv);
        *reinterpret_cast<double2*>(col + (int64_t)q * ldv) = rw_row<NC>(y, u, rot, m, q);
    }
    double dm0 = 0.0, dm1 = 0.0, ds0 = 0.0, ds1 = 0.0;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const double g = gh[2 * c], h = gh[2 * c + 1];
        dm0 = fma(g, u[c].x, dm0);
        dm1 = fma(g, u[c].y, dm1);
        ds0 = fma(h * u[c].x, u[c].x, ds0);
        ds1 = fma(h * u[c].y, u[c].y, ds1);
    }
    if (j < n) {
        mu[j] += dm0;
        s2[j] += ds0;
    }
    if (j + 1 < n) {
        mu[j + 1] += dm1;
        s2[j + 1] += ds1;
    }
}

template <int NC>
static void launch_sweep(const ital_reweigh_desc* a, int j0, int q0, hipStream_t stream) {
    const int64_t blocks = (a->ldv / 2 + 255) / 256;
    ITAL_LAUNCH(reweigh_sweep_kernel<NC>, dim3((unsigned)blocks), dim3(256), 0, stream, a->V, a->ldv, a->n, a->mu, a->s2, a->work,
                a->m, a->r, j0, q0);
}

}  // namespace ital

extern "C" int64_t ital_gp_reweigh_workspace(int m, int r) {
    if (m <= 0 || r <= 0) return 0;
    return ital::rw_s_off(m, r) + ((int64_t)m + 1) * m;
}

extern "C" int ital_gp_reweigh(const ital_reweigh_desc* a, hipStream_t stream) {
    using namespace ital;
    if (!a) return ital_fail(-22, "ital_gp_reweigh: null descriptor");
    if (a->m <= 0) return ital_fail(-22, "ital_gp_reweigh: no labelled sample (m <= 0)");
    if (a->r < 1) return ital_fail(-22, "ital_gp_reweigh: no position listed (r < 1)");
    if (a->ldl < a->m) return ital_fail(-22, "ital_gp_reweigh: ldl smaller than m");
    if (a->n < 0 || a->ldv < a->n || (a->ldv & 1)) return ital_fail(-22, "ital_gp_reweigh: ldv must be even and at least n >= 0");
    if (!a->L || !a->alpha || !a->work || !a->status || !a->pos || !a->delta) return ital_fail(-22, "ital_gp_reweigh: null buffer");
    if (a->n > 0 && (!a->V || !a->mu || !a->s2)) return ital_fail(-22, "ital_gp_reweigh: null buffer (V, mu, s2)");
    for (int j = 0; j < a->r; j++) {
        if (a->pos[j] < 0 || a->pos[j] >= a->m || (j && a->pos[j] <= a->pos[j - 1]))
            return ital_fail(-22, "ital_gp_reweigh: pos must be strictly increasing inside [0, m)");
        if (!std::isfinite(a->delta[j])) return ital_fail(-22, "ital_gp_reweigh: delta must be finite");
    }
    if (a->work_doubles < ital_gp_reweigh_workspace(a->m, a->r) || ((uintptr_t)a->work & 15))
        return ital_fail(-22, "ital_gp_reweigh: work smaller than ital_gp_reweigh_workspace(m, r), or not 16-byte aligned");
    const int p0 = a->pos[0];
    for (int j0 = 0; j0 < a->r; j0 += kPass) {
        Chains ch = {};
        const int nc = a->r - j0 < kPass ? a->r - j0 : kPass;
        for (int j = 0; j < nc; j++) {
            ch.pos[j] = a->pos[j0 + j];
            ch.delta[j] = a->delta[j0 + j];
        }
        ITAL_LAUNCH(reweigh_factor_kernel, dim3(1), dim3(kRwThreads), 0, stream, a->L, a->ldl, a->alpha, a->work, a->m, p0, a->r, j0,
                    nc, ch, j0 == 0 ? 1 : 0, j0 + kPass >= a->r ? 1 : 0, a->status);
        int rc = ital_check_launch("ital_gp_reweigh(factor)");
        if (rc) return rc;
    }
    if (a->n == 0) return 0;
    for (int j0 = 0; j0 < a->r; j0 += kPass) {
        const int nc = a->r - j0 < kPass ? a->r - j0 : kPass;
        const int q0 = a->pos[j0];
        switch (nc) {
            case 1: launch_sweep<1>(a, j0, q0, stream); break;
            case 2: launch_sweep<2>(a, j0, q0, stream); break;
            case 3: launch_sweep<3>(a, j0, q0, stream); break;
            case 4: launch_sweep<4>(a, j0, q0, stream); break;
            case 5: launch_sweep<5>(a, j0, q0, stream); break;
            case 6: launch_sweep<6>(a, j0, q0, stream); break;
            case 7: launch_sweep<7>(a, j0, q0, stream); break;
            default: launch_sweep<8>(a, j0, q0, stream); break;
        }
        int rc = ital_check_launch("ital_gp_reweigh(sweep)");
        if (rc) return rc;
    }
    return 0;
}
