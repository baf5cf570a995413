// The log marginal likelihood of G hyper-parameter candidates and its gradient in (log l, log var, log noise), for fitting a
// live session's kernel by gradient ascent (include/ital_evidence_grad.h; GaussianProcess.evidence_grad, tune.maximize_lml,
// ActiveRetrievalBase.fit_params).
//
//   ital_sqdist_lower               the squared distances every candidate shares, with the bits ital_gram_grid forms
//   ital_chol_gram_inverse_batched  W = M^T M, the lower triangle of K^-1, from the inverse factors M = L^-1
//   ital_gp_evidence_grad           the prologue of ital_gp_evidence (setup, Gram grid, ital_chol_batched,
//                                   ital_chol_solve_batched, inverse diagonals), squared distances, fused product, reduction
//
// The five leading launches are chain_prologue (evidence_chain.h), the host function ital_gp_evidence runs, and the reduction
// adds y.alpha and sum log L_ii through the same serial_sums and lml_value: factor, alpha, inverse diagonal and lml have its
// bits because they come from the same code.  The product is the 128 x 128 LDS-staged v_mfma_f64_16x16x4_f64 tile of
// mfma_tile.h (its LDS layout and mfma_stage) with BOTH operands read k-major behind predicates (tile_tn, evidence_chain.h):
// M is stored [k][i], W_ij = sum_k M[k][i] M[k][j] runs down its columns, and a run of 16 neighbouring columns of one row k is
// one 128-byte read.  In the chain W never reaches memory: the epilogue turns a tile into two numbers.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "evidence_chain.h"
#include "ital_evidence_grad.h"

namespace ital {
namespace evidence_grad {

using namespace ital::evidence;

// ------------------------------------------------------------------------------------------------- squared distances
struct DistArgs {
    const double* XT; const double* xn; int m; int ldx;
    double* D; int64_t ld;
};

// grid: lower tile pairs.  The tile gram_grid_kernel forms before its candidate loop (sqdist_tile), stored.
__global__ __launch_bounds__(256, 2) void sqdist_lower_kernel(DistArgs a) {
    __shared__ StageLds lds;
    const int64_t m = a.m;
    d4 acc[4][4];
    int64_t iw, jw;
    if (!sqdist_tile(a.XT, a.xn, m, a.ldx, lds, acc, iw, jw)) return;
    const int lane = threadIdx.x & 63;
    const int col = lane & 15, kg = lane >> 4;
    // for_each_lower's walk, written out: through the helper the kernel takes 32 SGPRs instead of 30
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int64_t j = jw + 16 * q + col;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            if (iw + 16 * p >= m || jw + 16 * q > iw + 16 * p + 15) continue;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int64_t i = iw + 16 * p + kg + 4 * reg;
                if (i < m && j <= i) a.D[i * a.ld + j] = acc[p][q][reg];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- W = M^T M
struct ProdArgs {
    const double* M; int n; const int* info;       // inverse factor g at M + g n n, row stride n, lower triangle
    double* W; int64_t ldw;                        // stored form: W_g at W + g n ldw
    const double* D; int64_t ldd;                  // fused form: the shared squared distances,
    const double* alpha;                           //   alpha_g at alpha + g n,
    const double* params;                          //   [G][3],
    double* part;                                  //   out [G][pairs][2]: sum of t, sum of t D over the tile pair's lower elements
};

// grid: (lower tile pairs, matrices).  Tile (ti, tj), ti >= tj, of W_g = M_g^T M_g: k runs from the tile's first row (M is
// lower triangular: M[k][i] = 0 for k < i) to n; the predicates i <= k, j <= k keep every read inside the lower triangle.
// FUSED: t_ij = (alpha_i alpha_j - W_ij) var exp(D_ij / (-2 l^2)), counted twice below the diagonal, and t_ij D_ij are
// summed per lane (q, p, reg ascending), then over the workgroup by a fixed binary tree in LDS.
template <bool FUSED>
__global__ __launch_bounds__(256, 2) void gram_inverse_kernel(ProdArgs a) {
    __shared__ StageLds lds;
    const int g = blockIdx.y, n = a.n;
    const bool skip = a.info && a.info[g] != 0;
    if (FUSED && skip) return;
    int ti, tj;
    tri_pair(blockIdx.x, ti, tj);
    const int i0 = ti * T, j0 = tj * T;
    if (i0 >= n) return;
    const double* M = a.M + (int64_t)g * n * n;
    d4 acc[4][4];
    zero_acc(acc);
    if (!skip) {
        auto fa = [&](int k, int r) {
            const int i = i0 + r;
            return (k < n && i <= k) ? M[(int64_t)k * n + i] : 0.0;
        };
        auto fb = [&](int k, int c) {
            const int j = j0 + c;
            return (k < n && j <= k) ? M[(int64_t)k * n + j] : 0.0;
        };
        tile_tn(fa, fb, i0, n, lds, acc);
    }
    const int wave = threadIdx.x >> 6;
    const int iw = i0 + 64 * (wave >> 1), jw = j0 + 64 * (wave & 1);
    if (!FUSED) {
        double* W = a.W + (int64_t)g * n * a.ldw;
        for_each_lower(iw, jw, n, [&](int p, int q, int reg, int i, int j) {
            W[(int64_t)i * a.ldw + j] = skip ? __builtin_nan("") : acc[p][q][reg];
        });
        return;
    }
    const double l = a.params[3 * (int64_t)g], var = a.params[3 * (int64_t)g + 1];
    const double s = -2.0 * l * l;
    const double* alpha = a.alpha + (int64_t)g * n;
    double sv = 0.0, sd = 0.0, aj[4];
#pragma unroll
    for (int q = 0; q < 4; q++) aj[q] = alpha[min(jw + 16 * q + (int)(threadIdx.x & 15), n - 1)];
    for_each_lower(iw, jw, n, [&](int p, int q, int reg, int i, int j) {
        const double d = a.D[(int64_t)i * a.ldd + j];
        double t = (alpha[i] * aj[q] - acc[p][q][reg]) * (var * exp(d / s));
        if (j < i) t += t;
        sv += t;
        sd += t * d;
    });
    double (*red)[256] = (double (*)[256]) & lds[0][0][0][0];     // tile_tn ended with a barrier: the stage buffers are free
    const int tid = threadIdx.x;
    red[0][tid] = sv;
    red[1][tid] = sd;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            red[0][tid] += red[0][tid + h];
            red[1][tid] += red[1][tid + h];
        }
        __syncthreads();
    }
    if (tid < 2) a.part[((int64_t)g * gridDim.x + blockIdx.x) * 2 + tid] = red[tid][0];
}

// --------------------------------------------------------------------------------------------- setup and the reduction
struct GradLayout {      // of the workspace of ital_gp_evidence_grad: that of ital_gp_evidence, then D and the partials
    Layout ev;
    int64_t D, part, pairs, total;
};

__host__ __device__ inline GradLayout grad_layout(int64_t m, int64_t G) {
    GradLayout w;
    const int64_t tn = (m + T - 1) / T;
    w.pairs = tn * (tn + 1) / 2;
    w.ev = layout(m, G);
    w.D = w.ev.total;               // [m][m], shared by the candidates
    w.part = w.D + m * m;           // [G][pairs][2]
    w.total = w.part + G * w.pairs * 2;
    return w;
}

struct GradArgs {
    const double* y; int m; int G;
    const double* params;
    double* K; int64_t ld;
    double* values; double* grad; const int* info;
    double* work;
};

// Workgroup g: lml and the three gradient components of candidate g.  y.alpha, sum log L_ii, alpha.alpha and sum c_i are
// serial_sums, the first two and lml_value as evidence_reduce_kernel calls them.  Thread 4 adds the tile pairs' partials in
// ascending tile order.
__global__ __launch_bounds__(256) void grad_reduce_kernel(GradArgs a) {
    __shared__ double term[4][256];
    __shared__ double tot[6];
    const int g = blockIdx.x, m = a.m, tid = threadIdx.x;
    double* gr = a.grad + 3 * (int64_t)g;
    if (a.info[g] != 0) {
        if (tid == 0) a.values[g] = -__builtin_inf();
        if (tid < 3) gr[tid] = __builtin_nan("");
        return;
    }
    const GradLayout w = grad_layout(m, a.G);
    const double* alpha = a.work + w.ev.alpha + (int64_t)g * m;
    const double* cd = a.work + w.ev.cdiag + (int64_t)g * m;
    const double* L = a.K + (int64_t)g * m * a.ld;
    // threads 0..3: y.alpha, sum log L_ii, alpha.alpha, sum c_i
    const double sum = serial_sums(m, term, [&](int i) {
        const double yi = a.y[i], al = alpha[i];
        term[0][tid] = yi * al;
        term[1][tid] = log(L[(int64_t)i * a.ld + i]);
        term[2][tid] = al * al;
        term[3][tid] = cd[i];
    });
    if (tid == 4) {
        const double* part = a.work + w.part + (int64_t)g * w.pairs * 2;
        double sv = 0.0, sd = 0.0;
        for (int64_t t = 0; t < w.pairs; t++) {
            sv += part[2 * t];
            sd += part[2 * t + 1];
        }
        tot[4] = sv;
        tot[5] = sd;
    }
    if (tid == 0) term[0][0] = sum;
    if (tid == 1) term[1][0] = sum;
    if (tid == 2) tot[2] = sum;
    if (tid == 3) tot[3] = sum;
    __syncthreads();
    if (tid == 0) a.values[g] = lml_value(term[0][0], term[1][0], m);
    if (tid == 1) {
        const double l = a.params[3 * (int64_t)g], noise = a.params[3 * (int64_t)g + 2];
        gr[0] = 0.5 * tot[5] / (l * l);
        gr[1] = 0.5 * tot[4];
        gr[2] = 0.5 * noise * (tot[2] - tot[3]);
    }
}

}  // namespace evidence_grad
}  // namespace ital

using namespace ital::evidence_grad;

static int launch_sqdist(const double* XT, const double* XTn, int m, int ldx, double* D, int64_t ld, hipStream_t stream) {
    const int64_t tn = ((int64_t)m + T - 1) / T, pairs = tn * (tn + 1) / 2;
    DistArgs a = {XT, XTn, m, ldx, D, ld};
    ITAL_LAUNCH(sqdist_lower_kernel, dim3((unsigned)pairs), dim3(256), 0, stream, a);
    return ital_check_launch("ital_sqdist_lower");
}

extern "C" int ital_sqdist_lower(const double* XT, const double* XTn, int m, int ldx, double* D, int64_t ld,
                                 hipStream_t stream) {
    if (!XT || !XTn || !D) return ital_fail(-22, "ital_sqdist_lower: NULL pointer");
    if (m < 1) return ital_fail(-22, "ital_sqdist_lower: m must be at least 1");
    if (ldx <= 0 || ldx % 16 != 0) return ital_fail(-22, "ital_sqdist_lower: ldx must be a positive multiple of 16");
    if (ld < m) return ital_fail(-22, "ital_sqdist_lower: ld must be at least m");
    if (m > (1 << 22)) return ital_fail(-22, "ital_sqdist_lower: matrix too large");
    return launch_sqdist(XT, XTn, m, ldx, D, ld, stream);
}

extern "C" int ital_chol_gram_inverse_batched(const double* M, int n, int count, const int* info, double* W, int64_t ldw,
                                              hipStream_t stream) {
    if (!M || !W) return ital_fail(-22, "ital_chol_gram_inverse_batched: NULL pointer");
    if (n < 1 || count < 1) return ital_fail(-22, "ital_chol_gram_inverse_batched: n and count must be at least 1");
    if (count > 65535) return ital_fail(-22, "ital_chol_gram_inverse_batched: more than 65535 matrices per call");
    if (ldw < n) return ital_fail(-22, "ital_chol_gram_inverse_batched: ldw must be at least n");
    if (n > (1 << 22)) return ital_fail(-22, "ital_chol_gram_inverse_batched: matrix too large");
    const int64_t tn = ((int64_t)n + T - 1) / T, pairs = tn * (tn + 1) / 2;
    ProdArgs a = {M, n, info, W, ldw, nullptr, 0, nullptr, nullptr, nullptr};
    ITAL_LAUNCH(gram_inverse_kernel<false>, dim3((unsigned)pairs, (unsigned)count), dim3(256), 0, stream, a);
    return ital_check_launch("ital_chol_gram_inverse_batched");
}

extern "C" int64_t ital_gp_evidence_grad_workspace(int m, int G) {
    if (m < 1 || G < 1) return 0;
    return grad_layout(m, G).total;
}

extern "C" int ital_gp_evidence_grad(const ital_evidence_grad_desc* d, hipStream_t stream) {
    const char* who = "ital_gp_evidence_grad";
    if (!d) return chain_fail(-22, who, "NULL descriptor");
    if (!d->values || !d->grad) return chain_fail(-22, who, "NULL pointer");
    const int m = d->m, G = d->G;
    const ChainArgs c = {d->XT, d->XTn, d->ldx, d->y, m, d->params, G, d->K, d->ld, d->info, d->status, d->work, d->ev};
    int rc;
    if ((rc = chain_check(c, who))) return rc;
    const GradLayout w = grad_layout(m, G);
    if (d->work_doubles < w.total) return chain_fail(-22, who, "work smaller than ital_gp_evidence_grad_workspace(m, G)");
    if ((rc = chain_prologue(c, who, stream))) return rc;
    if ((rc = launch_sqdist(d->XT, d->XTn, m, d->ldx, d->work + w.D, m, stream))) return rc;
    if ((rc = chain_mark(d->ev, 5, stream, who))) return rc;
    ProdArgs p = {d->work + w.ev.M, m, d->info, nullptr, 0, d->work + w.D, m, d->work + w.ev.alpha, d->params, d->work + w.part};
    ITAL_LAUNCH(gram_inverse_kernel<true>, dim3((unsigned)w.pairs, (unsigned)G), dim3(256), 0, stream, p);
    if ((rc = chain_launched(who, "product"))) return rc;
    if ((rc = chain_mark(d->ev, 6, stream, who))) return rc;
    GradArgs a = {d->y, m, G, d->params, d->K, d->ld, d->values, d->grad, d->info, d->work};
    ITAL_LAUNCH(grad_reduce_kernel, dim3((unsigned)G), dim3(256), 0, stream, a);
    if ((rc = chain_launched(who, "reduction"))) return rc;
    return chain_mark(d->ev, 7, stream, who);
}
