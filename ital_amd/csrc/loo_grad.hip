// The closed-form leave-one-out scores loo_logp and loo_mse of G hyper-parameter candidates and their gradients in
// (log l, log var, log noise), for fitting a live session's kernel to a criterion that holds up where the evidence over-fits
// (include/ital_loo_grad.h; GaussianProcess.loo_grad, tune.fit_session_params(criterion=...), ActiveRetrievalBase.fit_params).
//
//   ital_gp_loo_grad   chain_prologue (evidence_chain.h: setup, Gram grid, ital_chol_batched, ital_chol_solve_batched, inverse
//                      diagonals), ital_sqdist_lower, ital_chol_gram_inverse_batched (the stored W), the product, the reduction
//
// With A = dK / d log theta, P = W A, r = P alpha and s_i = (P W)_ii, both gradients are sums over the samples of terms in
// alpha_i, c_i, r_i and s_i.  The product kernel forms P for A_l l^2 = Kf o D and A_var = Kf on the 128 x 128 LDS-staged
// v_mfma_f64_16x16x4_f64 tile of mfma_tile.h through tile_tn (evidence_chain.h) and reduces every tile to its rows' partial
// r and s; no tile of P reaches memory.  W and D exist as lower triangles only: the fetch functions read them mirrored, at
// (max(i, k), min(i, k)), so the chain needs no second copy of either.  The values come from loo_sample and serial_sums, the
// code evidence_reduce_kernel runs: they have ital_gp_evidence's bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "evidence_chain.h"
#include "ital_loo_grad.h"

namespace ital {
namespace loo_grad {

using namespace ital::evidence;

constexpr int SLOTS = 33;      // 32 column slots of a tile row in the epilogue's LDS, padded against bank conflicts

struct LooLayout {       // of the workspace of ital_gp_loo_grad: that of ital_gp_evidence, then D, W, the partials and r, s
    Layout ev;
    int64_t D, W, part, rs, tn, total;
};

__host__ __device__ inline LooLayout loo_layout(int64_t m, int64_t G) {
    LooLayout w;
    w.tn = (m + T - 1) / T;
    w.ev = layout(m, G);
    w.D = w.ev.total;               // [m][m], shared by the candidates, lower triangle
    w.W = w.D + m * m;              // [G][m][m], lower triangle
    w.part = w.W + G * m * m;       // [G][2 operands][tn column tiles][m rows][2]: partial r_i, s_i
    w.rs = w.part + G * 2 * w.tn * m * 2;     // [G][m][6]: r_i, s_i of A_l, A_var, A_noise
    w.total = w.rs + G * m * 6;
    return w;
}

// Element (r, c) of a symmetric matrix stored as its lower triangle with row stride n.
__device__ inline double sym(const double* S, int64_t n, int r, int c) {
    return r >= c ? S[(int64_t)r * n + c] : S[(int64_t)c * n + r];
}

// ------------------------------------------------------------------------------------------------------- P = W A
struct ProdArgs {
    const double* W; const double* D; int n; int tn; const int* info;     // W_g at W + g n n; D shared; both row stride n
    const double* alpha;                           // alpha_g at alpha + g n
    const double* params;                          // [G][3]
    double* part;                                  // out [G][2][tn][n][2]
};

// grid: (tn x tn tiles, candidates, operands).  Tile (ti, tj) of P = W A for A = Kf o D (blockIdx.z = 0) or A = Kf
// (blockIdx.z = 1), Kf_kj = var exp(D_kj / (-2 l^2)) recomputed from the stored D: k runs over all of 0 .. n.  P is not
// symmetric, so every tile is visited; W and D are read mirrored from their lower triangles, and the predicates k < n, i < n,
// j < n keep every read inside them.  Epilogue: for tile row i the lane adds P_ij alpha_j and P_ij W_ij over its four columns
// (q ascending); thread (kind, row) then adds the row's 32 lane sums in LDS, slot ascending, and writes one partial.
__global__ __launch_bounds__(256, 2) void loo_product_kernel(ProdArgs a) {
    __shared__ StageLds lds;
    static_assert(sizeof(StageLds) >= sizeof(double) * 2 * T * SLOTS, "the epilogue's sums fit the stage buffers");
    const int g = blockIdx.y, n = a.n;
    const bool with_d = blockIdx.z == 0;
    if (a.info[g] != 0) return;
    const int ti = blockIdx.x / a.tn, tj = blockIdx.x % a.tn;
    const int i0 = ti * T, j0 = tj * T;
    const double* W = a.W + (int64_t)g * n * n;
    const double l = a.params[3 * (int64_t)g], var = a.params[3 * (int64_t)g + 1];
    const double s = -2.0 * l * l;
    d4 acc[4][4];
    zero_acc(acc);
    auto fa = [&](int k, int r) {
        const int i = i0 + r;
        return (k < n && i < n) ? sym(W, n, i, k) : 0.0;
    };
    auto fb = [&](int k, int c) {
        const int j = j0 + c;
        if (k >= n || j >= n) return 0.0;
        const double d = sym(a.D, n, k, j);
        const double kf = var * exp(d / s);
        return with_d ? kf * d : kf;
    };
    tile_tn(fa, fb, 0, n, lds, acc);
    // tile_tn ended with a barrier: the stage buffers are free
    double (*red)[T][SLOTS] = (double (*)[T][SLOTS]) & lds[0][0][0][0];
    const DLane dl = d_lane();
    const double* alpha = a.alpha + (int64_t)g * n;
    double aj[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int j = j0 + dl.column(q);
        aj[q] = j < n ? alpha[j] : 0.0;
    }
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int row = dl.row(p, reg), i = i0 + row;
            double sr = 0.0, ss = 0.0;
            if (i < n) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int j = j0 + dl.column(q);
                    if (j < n) {
                        sr += acc[p][q][reg] * aj[q];
                        ss += acc[p][q][reg] * sym(W, n, i, j);
                    }
                }
            }
            red[0][row][16 * dl.wx + dl.col] = sr;
            red[1][row][16 * dl.wx + dl.col] = ss;
        }
    __syncthreads();
    const int kind = threadIdx.x >> 7, row = threadIdx.x & (T - 1);
    if (i0 + row < n) {
        double sum = 0.0;
        for (int e = 0; e < 32; e++) sum += red[kind][row][e];
        a.part[((((int64_t)g * 2 + blockIdx.z) * a.tn + tj) * n + i0 + row) * 2 + kind] = sum;
    }
}

// ------------------------------------------------------------------------------------------------------- the reduction
struct LooArgs {
    const double* y; int m; int G;
    const double* params;
    double* values; double* grad; const int* info;
    double* work;
};

// The terms of sample i in d loo_logp / d log theta and, without its factor 2 / m, in d loo_mse / d log theta.
__device__ inline double logp_term(double al, double c, double r, double s) { return (al * r - 0.5 * (1.0 + al * al / c) * s) / c; }
__device__ inline double mse_term(double al, double c, double r, double s) { return (al / c) * (al * s / c - r) / c; }

// Workgroup g: the two scores and six gradient components of candidate g.  First every thread forms r_i and s_i of its rows
// i = tid, tid + 256, ...: the product's partials in ascending column-tile order (A_l's divided by l^2), and the noise row
// sums noise sum_j W_ij alpha_j and noise sum_j W_ij^2, j ascending.  serial_sums then closes the eight sums, i ascending,
// four at a time; loo_logp and loo_mse are the terms and sums of evidence_reduce_kernel.
__global__ __launch_bounds__(256) void loo_reduce_kernel(LooArgs a) {
    __shared__ double term[4][256];
    __shared__ double tot[8];
    const int g = blockIdx.x, m = a.m, tid = threadIdx.x;
    double* val = a.values + 2 * (int64_t)g;
    double* gr = a.grad + 6 * (int64_t)g;
    if (a.info[g] != 0) {
        if (tid == 0) {
            val[0] = -__builtin_inf();
            val[1] = __builtin_inf();
        }
        if (tid < 6) gr[tid] = __builtin_nan("");
        return;
    }
    const LooLayout w = loo_layout(m, a.G);
    const double* alpha = a.work + w.ev.alpha + (int64_t)g * m;
    const double* cd = a.work + w.ev.cdiag + (int64_t)g * m;
    const double* W = a.work + w.W + (int64_t)g * m * m;
    const double* part = a.work + w.part + (int64_t)g * 2 * w.tn * m * 2;
    double* rs = a.work + w.rs + (int64_t)g * m * 6;
    const double l = a.params[3 * (int64_t)g], noise = a.params[3 * (int64_t)g + 2];
    for (int i = tid; i < m; i += 256) {
        double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int op = 0; op < 2; op++)
            for (int64_t t = 0; t < w.tn; t++) {
                const double* p = part + ((op * w.tn + t) * m + i) * 2;
                v[2 * op] += p[0];
                v[2 * op + 1] += p[1];
            }
        for (int j = 0; j < m; j++) {
            const double wij = sym(W, m, i, j);
            v[4] += wij * alpha[j];
            v[5] += wij * wij;
        }
        v[0] /= l * l;
        v[1] /= l * l;
        v[4] *= noise;
        v[5] *= noise;
        for (int e = 0; e < 6; e++) rs[(int64_t)i * 6 + e] = v[e];      // read back below by this thread alone
    }
    // threads 0..3: loo_logp, sum (alpha / c)^2, d loo_logp / d log l, d log var
    double sum = serial_sums(m, term, [&](int i) {
        const double al = alpha[i], c = cd[i];
        const double* v = rs + (int64_t)i * 6;
        const LooSample t = loo_sample(a.y[i], al, c);
        term[0][tid] = t.logp;
        term[1][tid] = t.sq;
        term[2][tid] = logp_term(al, c, v[0], v[1]);
        term[3][tid] = logp_term(al, c, v[2], v[3]);
    });
    if (tid < 4) tot[tid] = sum;
    // threads 0..3: d loo_logp / d log noise, then the three sums of d loo_mse
    sum = serial_sums(m, term, [&](int i) {
        const double al = alpha[i], c = cd[i];
        const double* v = rs + (int64_t)i * 6;
        term[0][tid] = logp_term(al, c, v[4], v[5]);
        term[1][tid] = mse_term(al, c, v[0], v[1]);
        term[2][tid] = mse_term(al, c, v[2], v[3]);
        term[3][tid] = mse_term(al, c, v[4], v[5]);
    });
    if (tid < 4) tot[4 + tid] = sum;
    __syncthreads();
    if (tid == 0) val[0] = tot[0];
    if (tid == 1) val[1] = loo_mse_value(tot[1], m);
    if (tid == 2) gr[0] = tot[2];
    if (tid == 3) gr[1] = tot[3];
    if (tid == 4) gr[2] = tot[4];
    if (tid >= 5 && tid < 8) gr[tid - 2] = 2.0 / (double)m * tot[tid];
}

}  // namespace loo_grad
}  // namespace ital

using namespace ital::loo_grad;

extern "C" int64_t ital_gp_loo_grad_workspace(int m, int G) {
    if (m < 1 || G < 1) return 0;
    return loo_layout(m, G).total;
}

extern "C" int ital_gp_loo_grad(const ital_loo_grad_desc* d, hipStream_t stream) {
    const char* who = "ital_gp_loo_grad";
    if (!d) return chain_fail(-22, who, "NULL descriptor");
    if (!d->values || !d->grad) return chain_fail(-22, who, "NULL pointer");
    const int m = d->m, G = d->G;
    const ChainArgs c = {d->XT, d->XTn, d->ldx, d->y, m, d->params, G, d->K, d->ld, d->info, d->status, d->work, d->ev};
    int rc;
    if ((rc = chain_check(c, who))) return rc;
    const LooLayout w = loo_layout(m, G);
    if (d->work_doubles < w.total) return chain_fail(-22, who, "work smaller than ital_gp_loo_grad_workspace(m, G)");
    if ((rc = chain_prologue(c, who, stream))) return rc;
    if ((rc = ital_sqdist_lower(d->XT, d->XTn, m, d->ldx, d->work + w.D, m, stream))) return rc;
    if ((rc = chain_mark(d->ev, 5, stream, who))) return rc;
    if ((rc = ital_chol_gram_inverse_batched(d->work + w.ev.M, m, G, d->info, d->work + w.W, m, stream))) return rc;
    if ((rc = chain_mark(d->ev, 6, stream, who))) return rc;
    ProdArgs p = {d->work + w.W, d->work + w.D, m, (int)w.tn, d->info, d->work + w.ev.alpha, d->params, d->work + w.part};
    ITAL_LAUNCH(loo_product_kernel, dim3((unsigned)(w.tn * w.tn), (unsigned)G, 2), dim3(256), 0, stream, p);
    if ((rc = chain_launched(who, "product"))) return rc;
    if ((rc = chain_mark(d->ev, 7, stream, who))) return rc;
    LooArgs a = {d->y, m, G, d->params, d->values, d->grad, d->info, d->work};
    ITAL_LAUNCH(loo_reduce_kernel, dim3((unsigned)G), dim3(256), 0, stream, a);
    if ((rc = chain_launched(who, "reduction"))) return rc;
    return chain_mark(d->ev, 8, stream, who);
}
