// Scoring many hyper-parameter candidates against the labelled set of a live session (include/ital_evidence.h;
// GaussianProcess.evidence, tune.session_scores, ActiveRetrievalBase.tune_params): the log marginal likelihood and the
// closed-form leave-one-out quantities of Rasmussen & Williams (2.30), (5.10), (5.12) for G candidates at once.
//
//   ital_gram_grid              lower triangles of G Grams from one set of feature dot products per workgroup
//   ital_chol_inv_diag_batched  (K_g^-1)_ii = sum_{j >= i} (L_g^-1)[j][i]^2 of G factors, one workgroup per matrix
//   ital_gp_evidence            setup, Gram grid, ital_chol_batched, ital_chol_solve_batched, inverse diagonals, reduction
//
// All but the reduction is chain_prologue, which ital_gp_evidence_grad (evidence_grad.hip) runs too; evidence_chain.h holds
// what the two chains share.
// The Gram tile is the 128 x 128 LDS-staged v_mfma_f64_16x16x4_f64 tile of mfma_tile.h, the one ital_gram_rows runs on; the
// Cholesky and the solves are dense.hip's own entry points.  Every sum has a fixed order and no kernel lets one matrix see
// another: a candidate gets the same bits alone or in any batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "evidence_chain.h"
#include "ital_evidence.h"

namespace ital {
namespace evidence {

constexpr int CH = 1024;       // columns of a factor row staged per step of the inverse-diagonal kernel
constexpr int64_t GRID_TARGET_BLOCKS = 512;   // workgroups the Gram grid aims at: 256 CUs x 2

// ----------------------------------------------------------------------------------------------------------- Gram grid
struct GridArgs {
    const double* XT; const double* xn; int m; int ldx;
    const double* params; int G;
    double* K; int64_t ld;
};

// grid: (lower tile pairs, groups of candidates).  The tile's squared distances are formed once; candidate g = blockIdx.y,
// blockIdx.y + gridDim.y, ... each run their own epilogue over them.
__global__ __launch_bounds__(256, 2) void gram_grid_kernel(GridArgs a) {
    __shared__ StageLds lds;
    const int64_t m = a.m;
    d4 acc[4][4];
    int64_t iw, jw;
    if (!sqdist_tile(a.XT, a.xn, m, a.ldx, lds, acc, iw, jw)) return;
    const int lane = threadIdx.x & 63;
    const int col = lane & 15, kg = lane >> 4;
    for (int g = blockIdx.y; g < a.G; g += gridDim.y) {
        const double l = a.params[3 * (int64_t)g], var = a.params[3 * (int64_t)g + 1], noise = a.params[3 * (int64_t)g + 2];
        const double s = -2.0 * l * l;
        double* K = a.K + (int64_t)g * m * a.ld;
        // for_each_lower's walk, written out: through the helper exp() moves under the element test and the kernel takes
        // 215 VGPRs instead of 214
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int64_t j = jw + 16 * q + col;
#pragma unroll
            for (int p = 0; p < 4; p++) {
                if (iw + 16 * p >= m || jw + 16 * q > iw + 16 * p + 15) continue;
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const int64_t i = iw + 16 * p + kg + 4 * reg;
                    double v = var * exp(acc[p][q][reg] / s);
                    if (i == j) v += noise;
                    if (i < m && j <= i) K[i * a.ld + j] = v;
                }
            }
        }
    }
}

// --------------------------------------------------------------------------------------------------- inverse diagonals
struct InvdArgs {
    const double* const* L; const int64_t* ld; int n; const int* info;
    double* out; int64_t ldo;
    double* work;          // M = L^-1 of matrix g at work + g n n, row-major [j][i], lower triangle
};

// One workgroup per matrix.  Column i of M belongs to thread i % 256 alone: it writes M[j][i] row by row and is the only
// one to read it again, so the only data shared between threads is the staged row of L (double-buffered: one barrier per
// staged piece).  A row longer than CH is taken in pieces; a column's partial sum then waits in M[j][i] itself.  Within a
// wave the k-loop starts at the wave's first column, so that at every step the lanes read neighbouring elements of one row
// of M; a lane joins at k = i.
__global__ __launch_bounds__(256) void inv_diag_batched_kernel(InvdArgs a) {
    __shared__ double lrow[2][CH];
    const int g = blockIdx.x, n = a.n, tid = threadIdx.x;
    double* out = a.out + (int64_t)g * a.ldo;
    if (a.info && a.info[g] != 0) {
        for (int i = tid; i < n; i += 256) out[i] = __builtin_nan("");
        return;
    }
    const double* L = a.L[g];
    const int64_t ld = a.ld[g];
    double* M = a.work + (int64_t)g * n * n;
    int it = 0;
    for (int j = 0; j < n; j++) {
        const double* Lj = L + (int64_t)j * ld;
        double* Mj = M + (int64_t)j * n;
        const double ljj = Lj[j];
        for (int c0 = 0; c0 < j; c0 += CH, it++) {
            const int c1 = min(j, c0 + CH), buf = it & 1;
            for (int k = c0 + tid; k < c1; k += 256) lrow[buf][k - c0] = Lj[k];
            __syncthreads();
            for (int i = tid; i < c1; i += 256) {
                double acc = i >= c0 ? 0.0 : Mj[i];
                const int kb = max(c0, i & ~63);
                const double* Mk = M + (int64_t)kb * n + i;
#pragma unroll 4
                for (int k = kb; k < c1; k++, Mk += n)
                    if (k >= i) acc += lrow[buf][k - c0] * *Mk;
                Mj[i] = c1 == j ? -acc / ljj : acc;
            }
        }
        if (tid == (j & 255)) Mj[j] = 1.0 / ljj;
    }
    for (int i = tid; i < n; i += 256) {
        double ss = 0.0;
        const int jb = i & ~63;
        const double* Mk = M + (int64_t)jb * n + i;
        for (int j = jb; j < n; j++, Mk += n)
            if (j >= i) {
                const double v = *Mk;
                ss += v * v;
            }
        out[i] = ss;
    }
}

// --------------------------------------------------------------------------------------------- setup and the reduction
struct SetupArgs {
    const double* y; int m; int G; double* K; int64_t ld; double* work;
};

// Workgroup g: the entries of the batched calls' argument arrays for candidate g, and y as the solve's right-hand side.
__global__ __launch_bounds__(256) void chain_setup_kernel(SetupArgs a) {
    const int g = blockIdx.x;
    const Layout w = layout(a.m, a.G);
    double* alpha = a.work + w.alpha + (int64_t)g * a.m;
    if (threadIdx.x == 0) {
        ((double**)(a.work + w.Kp))[g] = a.K + (int64_t)g * a.m * a.ld;
        ((double**)(a.work + w.yp))[g] = alpha;
        ((int64_t*)(a.work + w.ldv))[g] = a.ld;
        ((int*)(a.work + w.nv))[g] = a.m;
    }
    for (int i = threadIdx.x; i < a.m; i += 256) alpha[i] = a.y[i];
}

struct EvArgs {
    const double* y; int m; int G;
    double* K; int64_t ld;
    double* scores; const int* info; double* loo_mean; double* loo_var; int64_t ldm;
    double* work;
};

// Workgroup g: loo_mean, loo_var and the four sums of candidate g (serial_sums).
__global__ __launch_bounds__(256) void evidence_reduce_kernel(EvArgs a) {
    __shared__ double term[4][256];
    const int g = blockIdx.x, m = a.m, tid = threadIdx.x;
    double* lm = a.loo_mean + (int64_t)g * a.ldm;
    double* lv = a.loo_var + (int64_t)g * a.ldm;
    double* sc = a.scores + 3 * (int64_t)g;
    if (a.info[g] != 0) {
        for (int i = tid; i < m; i += 256) lm[i] = lv[i] = __builtin_nan("");
        if (tid == 0) {
            sc[0] = sc[1] = -__builtin_inf();
            sc[2] = __builtin_inf();
        }
        return;
    }
    const Layout w = layout(m, a.G);
    const double* alpha = a.work + w.alpha + (int64_t)g * m;
    const double* cd = a.work + w.cdiag + (int64_t)g * m;
    const double* L = a.K + (int64_t)g * m * a.ld;
    // threads 0..3: y.alpha, sum log L_ii, loo_logp, sum (alpha / c)^2
    const double sum = serial_sums(m, term, [&](int i) {
        const double yi = a.y[i], al = alpha[i];
        const LooSample t = loo_sample(yi, al, cd[i]);
        lm[i] = t.mean;
        lv[i] = t.var;
        term[0][tid] = yi * al;
        term[1][tid] = log(L[(int64_t)i * a.ld + i]);
        term[2][tid] = t.logp;
        term[3][tid] = t.sq;
    });
    if (tid == 0) term[0][0] = sum;
    if (tid == 1) term[1][0] = sum;
    __syncthreads();
    if (tid == 0) sc[0] = lml_value(term[0][0], term[1][0], m);
    if (tid == 2) sc[1] = sum;
    if (tid == 3) sc[2] = loo_mse_value(sum, m);
}

}  // namespace evidence
}  // namespace ital

using namespace ital::evidence;

static int launch_gram_grid(const double* XT, const double* XTn, int m, int ldx, const double* params, int G, double* K,
                            int64_t ld, hipStream_t stream) {
    const int64_t tn = ((int64_t)m + T - 1) / T, pairs = tn * (tn + 1) / 2;
    int64_t groups = (GRID_TARGET_BLOCKS + pairs - 1) / pairs;
    groups = groups > G ? G : groups;
    groups = groups > 65535 ? 65535 : groups;
    GridArgs a = {XT, XTn, m, ldx, params, G, K, ld};
    ITAL_LAUNCH(gram_grid_kernel, dim3((unsigned)pairs, (unsigned)groups), dim3(256), 0, stream, a);
    return ital_check_launch("ital_gram_grid");
}

extern "C" int ital_gram_grid(const double* XT, const double* XTn, int m, int ldx, const double* params, int G, double* K,
                              int64_t ld, hipStream_t stream) {
    if (!XT || !XTn || !params || !K) return ital_fail(-22, "ital_gram_grid: NULL pointer");
    if (m < 1 || G < 1) return ital_fail(-22, "ital_gram_grid: m and G must be at least 1");
    if (ldx <= 0 || ldx % 16 != 0) return ital_fail(-22, "ital_gram_grid: ldx must be a positive multiple of 16");
    if (ld < m) return ital_fail(-22, "ital_gram_grid: ld must be at least m");
    if (m > (1 << 22)) return ital_fail(-22, "ital_gram_grid: matrix too large");
    return launch_gram_grid(XT, XTn, m, ldx, params, G, K, ld, stream);
}

extern "C" int64_t ital_chol_inv_diag_batched_workspace(int n, int count) {
    if (n < 1 || count < 1) return 0;
    return (int64_t)count * n * n;
}

extern "C" int ital_chol_inv_diag_batched(const double* const* L, const int64_t* ld, int n, int count, const int* info,
                                          double* out, int64_t ldo, double* work, int64_t work_doubles, hipStream_t stream) {
    if (!L || !ld || !out || !work) return ital_fail(-22, "ital_chol_inv_diag_batched: NULL pointer");
    if (n < 1 || count < 1) return ital_fail(-22, "ital_chol_inv_diag_batched: n and count must be at least 1");
    if (ldo < n) return ital_fail(-22, "ital_chol_inv_diag_batched: ldo must be at least n");
    if (work_doubles < ital_chol_inv_diag_batched_workspace(n, count))
        return ital_fail(-22, "ital_chol_inv_diag_batched: work smaller than ital_chol_inv_diag_batched_workspace(n, count)");
    InvdArgs a = {L, ld, n, info, out, ldo, work};
    ITAL_LAUNCH(inv_diag_batched_kernel, dim3((unsigned)count), dim3(256), 0, stream, a);
    return ital_check_launch("ital_chol_inv_diag_batched");
}

extern "C" int64_t ital_gp_evidence_workspace(int m, int G) {
    if (m < 1 || G < 1) return 0;
    return layout(m, G).total;
}

// The checks and the prologue of both chains (evidence_chain.h).
int ital::evidence::chain_check(const ChainArgs& c, const char* who) {
    if (!c.XT || !c.XTn || !c.y || !c.params || !c.K || !c.info || !c.status || !c.work) return chain_fail(-22, who, "NULL pointer");
    if (c.m < 1 || c.G < 1) return chain_fail(-22, who, "m and G must be at least 1");
    if (c.G > 65535) return chain_fail(-22, who, "more than 65535 candidates per call");
    if (c.m > (1 << 22)) return chain_fail(-22, who, "matrix too large");
    if (c.ldx <= 0 || c.ldx % 16 != 0) return chain_fail(-22, who, "ldx must be a positive multiple of 16");
    if (c.ld < c.m) return chain_fail(-22, who, "ld must be at least m");
    return 0;
}

int ital::evidence::chain_prologue(const ChainArgs& c, const char* who, hipStream_t stream) {
    int rc;
    if ((rc = chain_check(c, who))) return rc;
    const int m = c.m, G = c.G;
    const Layout w = layout(m, G);
    double* const* Kp = (double* const*)(c.work + w.Kp);
    double* const* yp = (double* const*)(c.work + w.yp);
    const int64_t* ldv = (const int64_t*)(c.work + w.ldv);
    const int* nv = (const int*)(c.work + w.nv);
    SetupArgs s = {c.y, m, G, c.K, c.ld, c.work};
    ITAL_LAUNCH(chain_setup_kernel, dim3((unsigned)G), dim3(256), 0, stream, s);
    if ((rc = chain_launched(who, "setup"))) return rc;
    if ((rc = chain_mark(c.ev, 0, stream, who))) return rc;
    if ((rc = launch_gram_grid(c.XT, c.XTn, m, c.ldx, c.params, G, c.K, c.ld, stream))) return rc;
    if ((rc = chain_mark(c.ev, 1, stream, who))) return rc;
    if ((rc = ital_chol_batched(Kp, nv, ldv, G, m, c.info, c.status, stream))) return rc;
    if ((rc = chain_mark(c.ev, 2, stream, who))) return rc;
    if ((rc = ital_chol_solve_batched(Kp, nv, ldv, yp, G, c.info, stream))) return rc;
    if ((rc = chain_mark(c.ev, 3, stream, who))) return rc;
    InvdArgs v = {Kp, ldv, m, c.info, c.work + w.cdiag, m, c.work + w.M};
    ITAL_LAUNCH(inv_diag_batched_kernel, dim3((unsigned)G), dim3(256), 0, stream, v);
    if ((rc = chain_launched(who, "inverse diagonals"))) return rc;
    return chain_mark(c.ev, 4, stream, who);
}

extern "C" int ital_gp_evidence(const ital_evidence_desc* d, hipStream_t stream) {
    const char* who = "ital_gp_evidence";
    if (!d) return chain_fail(-22, who, "NULL descriptor");
    if (!d->scores || !d->loo_mean || !d->loo_var) return chain_fail(-22, who, "NULL pointer");
    const ChainArgs c = {d->XT, d->XTn, d->ldx, d->y, d->m, d->params, d->G, d->K, d->ld, d->info, d->status, d->work, d->ev};
    int rc;
    if ((rc = chain_check(c, who))) return rc;
    if (d->ldm < d->m) return chain_fail(-22, who, "ldm must be at least m");
    if (d->work_doubles < layout(d->m, d->G).total)
        return chain_fail(-22, who, "work smaller than ital_gp_evidence_workspace(m, G)");
    if ((rc = chain_prologue(c, who, stream))) return rc;
    EvArgs a = {d->y, d->m, d->G, d->K, d->ld, d->scores, d->info, d->loo_mean, d->loo_var, d->ldm, d->work};
    ITAL_LAUNCH(evidence_reduce_kernel, dim3((unsigned)d->G), dim3(256), 0, stream, a);
    if ((rc = chain_launched(who, "reduction"))) return rc;
    return chain_mark(d->ev, 5, stream, who);
}
