// Taking a label back: removal of one labelled sample from the Cholesky-whitened GP state (include/ital_revoke.h).
//
// The reference cannot do this (RuntimeError 'Cannot change feedback once given.', ital/retrieval_base.py:183-189); its
// way back is a fit from scratch on the survivors (ital/gp.py:141-161).  Here L without row p -- lower Hessenberg from row p
// on -- is brought back to triangular form by Givens rotations of the column pairs (q, q + 1), q = p .. m-2: per row a running
// carry x = L[i][p]; y = L[i][q+1]; L'[i-1][q] = c_q x + s_q y; x = -s_q x + c_q y, where rotation q is fixed by the row whose
// diagonal it meets (c_q = x / r, s_q = y / r, r = hypot(x, y) the new, positive diagonal).  That is the rank-one UPDATE
// L33' L33'^T = L33 L33^T + l32 l32^T of the trailing block.  The same rotations run down every column of V (the sweep, the
// hot path at scale) and down alpha; what is left in the carry corrects the means and variances.
//
// remove_factor_kernel: one workgroup, latency-bound like chol_append_kernel; the trailing block goes through in panels of 64
// columns (diagonal block in LDS, the recurrence over its columns in one wave with the pivot broadcast by readlane, every row
// below a panel owned by one thread), so the dependent memory round trips are O((m - p) / 64).
// remove_sweep_kernel: a stream over rows p .. m-1 of V, in place.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ital_hip.h"
#include "ital_internal.h"
#include "ital_revoke.h"

namespace ital {

// work: [0] a_last, [kCoef + 2 i, + 1] (c, s) of rotation p + i, then the carries of the rows (m), then the compacted rows
// p .. m-2 of the factor, [m - 1 - p][m]
constexpr int kCoef = 8;
constexpr int kFactorThreads = 512;    // eight waves: 256 registers a lane, the panel's sixteen loads in flight do not spill
__host__ __device__ inline int64_t remove_carry_off(int m) { return kCoef + 2 * (int64_t)m; }
__host__ __device__ inline int64_t remove_rows_off(int m) { return kCoef + 4 * (int64_t)m; }

__device__ __forceinline__ double bcast_f64(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

__global__ __launch_bounds__(kFactorThreads) void remove_factor_kernel(double* __restrict__ L, int ldl, double* __restrict__ alpha,
                                                             double* __restrict__ XT, double* __restrict__ XTn, int ldx,
                                                             double* __restrict__ ws, int m, int p, int* __restrict__ status) {
    __shared__ double Lb[64][65];    // one 64 x 64 diagonal block of the trailing factor at a time
    __shared__ double xb[64];        // the carries of its rows
    __shared__ double2 csb[64];      // the rotations it fixes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n3 = m - 1 - p;        // rows below the one that leaves
    double2* cs = reinterpret_cast<double2*>(ws + kCoef);
    double* xv = ws + remove_carry_off(m);
    double* S = ws + remove_rows_off(m);                            // S[t][j]: new row p + t
    const double* T = L + (int64_t)(p + 1) * ldl + (p + 1);         // T[t][k] = L[p+1+t][p+1+k], the trailing block L33

    // the carries start as column p (l32); columns 0 .. p-1 of the rows below only move up
    for (int t = tid; t < n3; t += kFactorThreads) xv[t] = L[(int64_t)(p + 1 + t) * ldl + p];
    for (int idx = tid; idx < n3 * p; idx += kFactorThreads) {
        const int t = idx / p, j = idx - t * p;
        S[(int64_t)t * m + j] = L[(int64_t)(p + 1 + t) * ldl + j];
    }
    __threadfence_block();
    __syncthreads();

    for (int k0 = 0; k0 < n3; k0 += 64) {
        const int nb = n3 - k0 < 64 ? n3 - k0 : 64;
        for (int idx = tid; idx < nb * nb; idx += kFactorThreads) {
            const int i = idx / nb, q = idx - i * nb;
            Lb[i][q] = q <= i ? T[(int64_t)(k0 + i) * ldl + k0 + q] : 0.0;
        }
        if (tid < nb) xb[tid] = xv[k0 + tid];
        __syncthreads();
        if (wave == 0) {
            // diagonal block: lane i carries row k0 + i; column k fixes rotation k0 + k from lane k's carry and diagonal
            const bool in = lane < nb;
            double xi = in ? xb[lane] : 0.0;
            double* Srow = S + (int64_t)(k0 + (in ? lane : 0)) * m + p + k0;
            bool bad = false;
            double tik = in ? Lb[lane][0] : 0.0;
            for (int k = 0; k < nb; k++) {
                const double tnext = in ? Lb[lane][k + 1 < nb ? k + 1 : k] : 0.0;   // next column, off the dependent chain
                const double d = Lb[k][k];
                const double xk = bcast_f64(xi, k);
                const double r = sqrt(fma(xk, xk, d * d));
                if (!(r > 0) || !(d > 0)) bad = true;
                const double c = xk / r, s = d / r;
                if (lane == k) {
                    Srow[k] = r;
                    csb[k] = double2{c, s};
                    cs[k0 + k] = double2{c, s};
                } else if (in && lane > k) {
                    Srow[k] = fma(c, xi, s * tik);
                    xi = fma(c, tik, -s * xi);
                }
                tik = tnext;
            }
            if (bad && lane == 0) atomicOr(status, 1);
        }
        __syncthreads();
        // rows below the panel (there are some only when the panel is full): one thread per row, 64 rotations on its carry;
        // the loads do not depend on the carry, sixteen of them are in flight
        for (int t = k0 + 64 + tid; t < n3; t += kFactorThreads) {
            double xi = xv[t];
            const double* Tr = T + (int64_t)t * ldl + k0;
            double* Sr = S + (int64_t)t * m + p + k0;
            for (int kk = 0; kk < 64; kk += 16) {
                double tv[16];
#pragma unroll
                for (int u = 0; u < 16; u++) tv[u] = Tr[kk + u];
#pragma unroll
                for (int u = 0; u < 16; u++) {
                    const double2 c = csb[kk + u];
                    Sr[kk + u] = fma(c.x, xi, c.y * tv[u]);
                    xi = fma(c.x, tv[u], -c.y * xi);
                }
            }
            xv[t] = xi;
        }
        __threadfence_block();
        __syncthreads();
    }

    // the compacted rows back into L (strict upper triangle and the row that fell free: zero, as a fresh factor has them)
    for (int idx = tid; idx < n3 * m; idx += kFactorThreads) {
        const int t = idx / m, j = idx - t * m;
        L[(int64_t)(p + t) * ldl + j] = j <= p + t ? S[(int64_t)t * m + j] : 0.0;
    }
    for (int j = tid; j < m; j += kFactorThreads) L[(int64_t)(m - 1) * ldl + j] = 0.0;

    if (wave == 0) {
        // alpha' = (G^T alpha)[0 : m-1]: the same carry, 64 rotations per trip to memory; XTn moves up alongside
        double xa = alpha[p];
        for (int q0 = 0; q0 < n3; q0 += 64) {
            const int nb = n3 - q0 < 64 ? n3 - q0 : 64;
            const bool in = lane < nb;
            const double y = in ? alpha[p + 1 + q0 + lane] : 0.0;
            const double xn = in ? XTn[p + 1 + q0 + lane] : 0.0;
            const double2 c = in ? cs[q0 + lane] : double2{1.0, 0.0};
            double out = 0.0;
            for (int k = 0; k < nb; k++) {
                const double ck = bcast_f64(c.x, k), sk = bcast_f64(c.y, k), yk = bcast_f64(y, k);
                const double o = fma(ck, xa, sk * yk);
                xa = fma(ck, yk, -sk * xa);
                if (lane == k) out = o;
            }
            if (in) {
                alpha[p + q0 + lane] = out;
                XTn[p + q0 + lane] = xn;
            }
        }
        if (lane == 0) {
            ws[0] = xa;              // a_last
            alpha[m - 1] = 0.0;
            XTn[m - 1] = 0.0;
        }
    } else {
        // XT rows p+1 .. m-1 move up by one.  The move overlaps itself: every column belongs to one thread, which walks the
        // rows upwards, eight loads ahead of the eight stores that overwrite what was read before
        for (int col = tid - 64; col < ldx; col += kFactorThreads - 64) {
            double* c0 = XT + col;
            int r = p;
            for (; r + 8 <= m - 1; r += 8) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; u++) v[u] = c0[(int64_t)(r + 1 + u) * ldx];
#pragma unroll
                for (int u = 0; u < 8; u++) c0[(int64_t)(r + u) * ldx] = v[u];
            }
            for (; r < m - 1; r++) c0[(int64_t)r * ldx] = c0[(int64_t)(r + 1) * ldx];
            c0[(int64_t)(m - 1) * ldx] = 0.0;
        }
    }
}

// V' = (G^T V)[0 : m-1] in place, then mu' = mu - w a_last, s2' = s2 + w^2 with w the carry that is left.  A lane owns two
// adjacent columns (16-byte loads and stores); row q is written after rows q and q + 1 were read by that lane alone, so there
// is no hazard between lanes.  Only the FMAs depend on the carry: the loads of eight rows are in flight together.  The
// coefficients are the same for the whole wave (scalar loads).
constexpr int kSweepRows = 8;

__global__ __launch_bounds__(256) void remove_sweep_kernel(double* __restrict__ V, int64_t ldv, int64_t n,
                                                           double* __restrict__ mu, double* __restrict__ s2,
                                                           const double* __restrict__ ws, int m, int p) {
    const int64_t j = 2 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
    if (j >= ldv) return;            // ldv is even: a pair never straddles the end
    const double2* __restrict__ cs = reinterpret_cast<const double2*>(ws + kCoef);   // cs[q - p]: rotation q
    double* col = V + j;
    double2 x = *reinterpret_cast<const double2*>(col + (int64_t)p * ldv);
    int q = p;
    for (; q + kSweepRows <= m - 1; q += kSweepRows) {
        double2 y[kSweepRows];
#pragma unroll
        for (int u = 0; u < kSweepRows; u++) y[u] = *reinterpret_cast<const double2*>(col + (int64_t)(q + 1 + u) * ldv);
#pragma unroll
        for (int u = 0; u < kSweepRows; u++) {
            const double2 c = cs[q - p + u];
            double2 o;
            o.x = fma(c.x, x.x, c.y * y[u].x);
            o.y = fma(c.x, x.y, c.y * y[u].y);
            x.x = fma(c.x, y[u].x, -c.y * x.x);
            x.y = fma(c.x, y[u].y, -c.y * x.y);
            *reinterpret_cast<double2*>(col + (int64_t)(q + u) * ldv) = o;
        }
    }
    for (; q < m - 1; q++) {
        const double2 y = *reinterpret_cast<const double2*>(col + (int64_t)(q + 1) * ldv);
        const double2 c = cs[q - p];
        double2 o;
        o.x = fma(c.x, x.x, c.y * y.x);
        o.y = fma(c.x, x.y, c.y * y.y);
        x.x = fma(c.x, y.x, -c.y * x.x);
        x.y = fma(c.x, y.y, -c.y * x.y);
        *reinterpret_cast<double2*>(col + (int64_t)q * ldv) = o;
    }
    *reinterpret_cast<double2*>(col + (int64_t)(m - 1) * ldv) = double2{0.0, 0.0};
    const double a_last = ws[0];
    if (j < n) {
        mu[j] = fma(-x.x, a_last, mu[j]);
        s2[j] = fma(x.x, x.x, s2[j]);
    }
    if (j + 1 < n) {
        mu[j + 1] = fma(-x.y, a_last, mu[j + 1]);
        s2[j + 1] = fma(x.y, x.y, s2[j + 1]);
    }
}

}  // namespace ital

extern "C" int64_t ital_gp_remove_workspace(int m) {
    if (m <= 0) return 0;
    return ital::remove_rows_off(m) + (int64_t)m * m;
}

// Stands in for the refusal of reference ital/retrieval_base.py:183-189 and for the refit on the survivors, reference
// ital/gp.py:141-161: see include/ital_revoke.h.
extern "C" int ital_gp_remove(const ital_remove_desc* a, hipStream_t stream) {
    if (!a) return ital_fail(-22, "ital_gp_remove: null descriptor");
    if (a->m <= 0) return ital_fail(-22, "ital_gp_remove: no labelled sample (m <= 0)");
    if (a->p < 0 || a->p >= a->m) return ital_fail(-22, "ital_gp_remove: p outside [0, m)");
    if (a->ldl < a->m) return ital_fail(-22, "ital_gp_remove: ldl smaller than m");
    if (a->ldx < 1) return ital_fail(-22, "ital_gp_remove: ldx must be positive");
    if (a->n < 0 || a->ldv < a->n || (a->ldv & 1)) return ital_fail(-22, "ital_gp_remove: ldv must be even and at least n >= 0");
    if (!a->XT || !a->XTn || !a->L || !a->alpha || !a->work || !a->status) return ital_fail(-22, "ital_gp_remove: null buffer");
    if (a->n > 0 && (!a->V || !a->mu || !a->s2)) return ital_fail(-22, "ital_gp_remove: null buffer (V, mu, s2)");
    if (a->work_doubles < ital_gp_remove_workspace(a->m) || ((uintptr_t)a->work & 15))
        return ital_fail(-22, "ital_gp_remove: work smaller than ital_gp_remove_workspace(m), or not 16-byte aligned");
    ITAL_LAUNCH(ital::remove_factor_kernel, dim3(1), dim3(ital::kFactorThreads), 0, stream, a->L, a->ldl, a->alpha, a->XT, a->XTn, a->ldx,
                a->work, a->m, a->p, a->status);
    int rc = ital_check_launch("ital_gp_remove(factor)");
    if (rc || a->n == 0) return rc;
    const int64_t blocks = (a->ldv / 2 + 255) / 256;
    ITAL_LAUNCH(ital::remove_sweep_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a->V, a->ldv, a->n, a->mu, a->s2,
                a->work, a->m, a->p);
    return ital_check_launch("ital_gp_remove(sweep)");
}
