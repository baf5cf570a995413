// What taking each label back would change, without doing it (include/ital_influence.h): with M = L^-1, B = M^T V holds the
// effect of every single removal on every row, mu'_ij = mu_j - (w_i / c_i) B_ij and s2'_ij = s2_j + B_ij^2 / c_i.
//
// Stage 1 is the existing ital_chol_inv_diag_batched (count = 1: M into the workspace, c = diag K^-1) and a small kernel for
// w = M^T alpha.  Stage 2, the hot path, is the 128 x 128 tile product M^T V on v_mfma_f64_16x16x4_f64 through tile_tn of
// mfma_tile.h: M is stored row-major [p][i] and V [p][j], so BOTH operands are k-major (k = labelled position p) and the
// fetches of both run along contiguous runs of 16 doubles.  M^T is upper triangular: tile row block i0 starts its k-loop at
// i0, and within the first block the predicate k >= i supplies the zeros, so the strict upper triangle of the workspace
// (never written by stage 1) is never read.  Nothing of the product is stored: influence_tile_kernel<false> reduces a tile to
// three numbers per row (sum B^2, max |B|, sign flips of the mean), influence_combine_kernel adds the column tiles in
// ascending order (one workgroup per label) and scales; influence_tile_kernel<true> (preview of a few removals) takes the listed rows of M^T as its
// first operand and writes mu' and s2'.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "ital_evidence.h"
#include "ital_influence.h"
#include "ital_internal.h"
#include "mfma_tile.h"

namespace ital {
namespace influence {

using namespace ital::tile;

// work, in doubles: M [m][m], c [m], w [m], the one-entry pointer and leading-dimension arrays of the batched inverse, then
// the partials [column tile][m][3]
struct Layout {
    int64_t M, c, w, slot, part, total;
};

__host__ __device__ inline int64_t col_tiles(int64_t n) { return (n + T - 1) / T; }

__host__ __device__ inline Layout layout(int64_t m, int64_t n) {
    Layout w;
    w.M = 0;
    w.c = m * m;
    w.w = w.c + m;
    w.slot = w.w + m;
    w.part = w.slot + 2;
    w.total = w.part + col_tiles(n) * m * 3;
    return w;
}

__device__ inline bool bad_c(double c) { return !(c > 0.0) || !(c < __builtin_inf()); }

__global__ void influence_setup_kernel(const double* L, int64_t ldl, double* slot) {
    ((const double**)slot)[0] = L;
    ((int64_t*)slot)[1] = ldl;
}

// w_i = sum_{p >= i} M[p][i] alpha_p, p ascending; coef[i] = (c_i, w_i), NaN and the status bit for a broken c_i.
__global__ __launch_bounds__(256) void influence_coef_kernel(const double* M, const double* alpha, int m, const double* c,
                                                             double* w, double* coef, int* status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    double s = 0.0;
    for (int p = i; p < m; p++) s = fma(M[(int64_t)p * m + i], alpha[p], s);
    w[i] = s;
    const double ci = c[i];
    if (bad_c(ci)) {
        coef[2 * i] = coef[2 * i + 1] = __builtin_nan("");
        atomicOr(status, 1);
    } else {
        coef[2 * i] = ci;
        coef[2 * i + 1] = s;
    }
}

struct Sel {                 // the listed labelled positions of one preview launch, by value
    int idx[T];
};

struct TileArgs {
    const double* M; const double* c; const double* w; int m;
    const double* V; int64_t ldv, n;
    const double* mu; const double* s2; const uint8_t* mask;
    double* part;                                   // reducing epilogue
    double* mu_out; double* s2_out; int64_t ldo;    // writing epilogue: row 0 of this launch
    int rows;                                       // writing epilogue: listed positions of this launch
    int kbeg;                                       // writing epilogue: first k-block that any listed row needs
};

// grid (column tiles, row tiles).  WRITE = false: tile rows are the labelled positions i0 + r.  WRITE = true: tile row r is
// the listed position sel.idx[r], r < a.rows.
template <bool WRITE>
__global__ __launch_bounds__(256, 2) void influence_tile_kernel(TileArgs a, Sel sel) {
    __shared__ StageLds lds;
    const int m = a.m;
    const int i0 = WRITE ? 0 : (int)blockIdx.y * T;
    const int64_t j0 = (int64_t)blockIdx.x * T;
    const int c16 = threadIdx.x & 15;
    int ai[8];               // the labelled position behind each tile row this thread stages, -1: none
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const int r = c16 + 16 * u;
        if (WRITE) ai[u] = r < a.rows ? sel.idx[r] : -1;
        else ai[u] = i0 + r < m ? i0 + r : -1;
    }
    auto fa = [&](int k, int r) {
        const int i = ai[r >> 4];
        return (i >= 0 && k >= i && k < m) ? a.M[(int64_t)k * m + i] : 0.0;
    };
    auto fb = [&](int k, int c) {
        const int64_t j = j0 + c;
        return (k < m && j < a.n) ? a.V[(int64_t)k * a.ldv + j] : 0.0;
    };
    d4 acc[4][4];
    zero_acc(acc);
    tile_tn(fa, fb, WRITE ? a.kbeg : i0, m, lds, acc);
    const DLane dl = d_lane();
    if (WRITE) {
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int rr = dl.row(p, reg);
                if (rr >= a.rows) continue;
                const int i = sel.idx[rr];
                const double ci = a.c[i], ri = a.w[i] / ci;
                const bool bad = bad_c(ci);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int64_t j = j0 + dl.column(q);
                    if (j >= a.n) continue;
                    const double b = acc[p][q][reg];
                    a.mu_out[(int64_t)rr * a.ldo + j] = bad ? __builtin_nan("") : fma(-ri, b, a.mu[j]);
                    a.s2_out[(int64_t)rr * a.ldo + j] = bad ? __builtin_nan("") : a.s2[j] + b * b / ci;
                }
            }
        return;
    }
    // per row: sum B^2, max |B| and the sign flips over the counted columns of this tile.  Fixed order: the lane's four
    // columns, the sixteen lanes of a row (xor tree), then the two waves side by side through LDS.
    double (*red)[T][3] = reinterpret_cast<double (*)[T][3]>(&lds);     // [wx][tile row][3]; tile_tn ended with a barrier
    double muq[4];
    bool on[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int64_t j = j0 + dl.column(q);
        on[q] = j < a.n && (!a.mask || a.mask[j] != 0);
        muq[q] = on[q] ? a.mu[j] : 0.0;
    }
#pragma unroll
    for (int p = 0; p < 4; p++) {
        if (i0 + 64 * dl.wy + 16 * p >= m) continue;     // sixteen rows past the last label (the whole wave agrees): never read
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int rr = dl.row(p, reg), i = i0 + rr;
            const double ri = i < m ? a.w[i] / a.c[i] : 0.0;
            double ss = 0.0, mx = 0.0, fl = 0.0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (!on[q]) continue;
                const double b = acc[p][q][reg];
                ss = fma(b, b, ss);
                mx = fmax(mx, fabs(b));
                fl += ((muq[q] > 0.0) != (fma(-ri, b, muq[q]) > 0.0)) ? 1.0 : 0.0;
            }
#pragma unroll
            for (int s = 1; s < 16; s <<= 1) {
                ss += __shfl_xor(ss, s, 64);
                mx = fmax(mx, __shfl_xor(mx, s, 64));
                fl += __shfl_xor(fl, s, 64);
            }
            if (dl.col == 0) {
                red[dl.wx][rr][0] = ss;
                red[dl.wx][rr][1] = mx;
                red[dl.wx][rr][2] = fl;
            }
        }
    }
    __syncthreads();
    const int rr = threadIdx.x, i = i0 + rr;
    if (rr < T && i < m) {
        double* out = a.part + ((int64_t)blockIdx.x * m + i) * 3;
        out[0] = red[0][rr][0] + red[1][rr][0];
        out[1] = fmax(red[0][rr][1], red[1][rr][1]);
        out[2] = red[0][rr][2] + red[1][rr][2];
    }
}

// stats[i] from the partials of the column tiles, one workgroup per label: thread q adds the tiles [q len, (q + 1) len),
// len = ceil(tiles / 256), in ascending order, thread 0 then the 256 chunk sums in ascending order -- the tiles in ascending
// order throughout (up to 256 tiles: one plain ascending sum), with a grouping that depends on the tile count alone.
__global__ __launch_bounds__(256) void influence_combine_kernel(const double* part, int64_t tiles, const double* c, const double* w,
                                                                int m, double* stats) {
    __shared__ double red[3][256];
    const int i = blockIdx.x, q = threadIdx.x;
    const int64_t len = (tiles + 255) / 256, t0 = q * len, t1 = min(tiles, t0 + len);
    double ss = 0.0, mx = 0.0, fl = 0.0;
    const double* pi = part + 3 * (t0 * m + i);
    for (int64_t t = t0; t < t1; t++, pi += 3 * (int64_t)m) {
        ss += pi[0];
        mx = fmax(mx, pi[1]);
        fl += pi[2];
    }
    red[0][q] = ss;
    red[1][q] = mx;
    red[2][q] = fl;
    __syncthreads();
    if (q != 0) return;
    double* out = stats + 4 * (int64_t)i;
    const double ci = c[i];
    if (bad_c(ci)) {
        out[0] = out[1] = out[2] = out[3] = __builtin_nan("");
        return;
    }
    ss = 0.0, mx = 0.0, fl = 0.0;
    for (int k = 0; k < 256; k++) {
        ss += red[0][k];
        mx = fmax(mx, red[1][k]);
        fl += red[2][k];
    }
    const double ri = w[i] / ci;
    out[0] = ri * ri * ss;
    out[1] = fabs(ri) * mx;
    out[2] = fl;
    out[3] = ss / ci;
}

static int check(const ital_influence_desc* a, const char* who, bool preview) {
    char msg[160];
    const char* what = nullptr;
    if (!a) what = "null descriptor";
    else if (a->m < 1) what = "no labelled sample (m < 1)";
    else if (a->n < 0) what = "n must not be negative";
    else if (a->ldl < a->m) what = "ldl smaller than m";
    else if (a->ldv < a->n) what = "ldv smaller than n";
    else if (!a->L || !a->alpha || !a->coef || !a->work || !a->status) what = "null buffer";
    else if (!preview && !a->stats) what = "null buffer (stats)";
    else if (a->n > 0 && (!a->V || !a->mu)) what = "null buffer (V, mu)";
    else if (preview && a->n > 0 && !a->s2) what = "null buffer (s2)";
    else if (a->work_doubles < ital_gp_influence_workspace(a->m, a->n)) what = "work smaller than ital_gp_influence_workspace(m, n)";
    if (!what) return 0;
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return ital_fail(-22, msg);
}

// M, c, w into the workspace and coef out.
static int stage1(const ital_influence_desc* a, const Layout& w, const char* who, hipStream_t stream) {
    double* ws = a->work;
    ITAL_LAUNCH(influence_setup_kernel, dim3(1), dim3(1), 0, stream, a->L, (int64_t)a->ldl, ws + w.slot);
    int rc = ital_check_launch(who);
    if (rc) return rc;
    rc = ital_chol_inv_diag_batched((const double* const*)(ws + w.slot), (const int64_t*)(ws + w.slot + 1), a->m, 1, nullptr,
                                    ws + w.c, a->m, ws + w.M, (int64_t)a->m * a->m, stream);
    if (rc) return rc;
    ITAL_LAUNCH(influence_coef_kernel, dim3((unsigned)((a->m + 255) / 256)), dim3(256), 0, stream, ws + w.M, a->alpha, a->m,
                ws + w.c, ws + w.w, a->coef, a->status);
    return ital_check_launch(who);
}

static TileArgs tile_args(const ital_influence_desc* a, const Layout& w) {
    double* ws = a->work;
    TileArgs t = {};
    t.M = ws + w.M;
    t.c = ws + w.c;
    t.w = ws + w.w;
    t.m = a->m;
    t.V = a->V;
    t.ldv = a->ldv;
    t.n = a->n;
    t.mu = a->mu;
    t.s2 = a->s2;
    t.mask = a->mask;
    t.part = ws + w.part;
    return t;
}

}  // namespace influence
}  // namespace ital

using namespace ital::influence;

extern "C" int64_t ital_gp_influence_workspace(int m, int64_t n) {
    if (m < 1 || n < 0) return 0;
    return layout(m, n).total;
}

extern "C" int ital_gp_influence(const ital_influence_desc* a, hipStream_t stream) {
    int rc = check(a, "ital_gp_influence", false);
    if (rc) return rc;
    const Layout w = layout(a->m, a->n);
    rc = stage1(a, w, "ital_gp_influence(stage 1)", stream);
    if (rc) return rc;
    const int64_t tiles = col_tiles(a->n);
    const TileArgs t = tile_args(a, w);
    if (tiles > 0) {
        ITAL_LAUNCH(influence_tile_kernel<false>, dim3((unsigned)tiles, (unsigned)((a->m + T - 1) / T)), dim3(256), 0, stream, t,
                    Sel{});
        rc = ital_check_launch("ital_gp_influence(tile)");
        if (rc) return rc;
    }
    ITAL_LAUNCH(influence_combine_kernel, dim3((unsigned)a->m), dim3(256), 0, stream, t.part, tiles, t.c, t.w, a->m, a->stats);
    return ital_check_launch("ital_gp_influence(combine)");
}

extern "C" int ital_gp_preview_remove(const ital_influence_desc* a, const int* sel, int r, double* mu_out, double* s2_out,
                                      int64_t ldo, hipStream_t stream) {
    int rc = check(a, "ital_gp_preview_remove", true);
    if (rc) return rc;
    if (!sel || !mu_out || !s2_out) return ital_fail(-22, "ital_gp_preview_remove: null buffer (sel, mu_out, s2_out)");
    if (r < 1) return ital_fail(-22, "ital_gp_preview_remove: no position listed (r < 1)");
    if (ldo < a->n) return ital_fail(-22, "ital_gp_preview_remove: ldo smaller than n");
    for (int q = 0; q < r; q++)
        if (sel[q] < 0 || sel[q] >= a->m) return ital_fail(-22, "ital_gp_preview_remove: sel entry outside [0, m)");
    const Layout w = layout(a->m, a->n);
    rc = stage1(a, w, "ital_gp_preview_remove(stage 1)", stream);
    if (rc || a->n == 0) return rc;
    const int64_t tiles = col_tiles(a->n);
    TileArgs t = tile_args(a, w);
    t.ldo = ldo;
    for (int q0 = 0; q0 < r; q0 += T) {
        Sel s = {};
        t.rows = r - q0 < T ? r - q0 : T;
        int lo = a->m;
        for (int q = 0; q < t.rows; q++) {
            s.idx[q] = sel[q0 + q];
            lo = s.idx[q] < lo ? s.idx[q] : lo;
        }
        t.kbeg = lo / KS * KS;
        t.mu_out = mu_out + (int64_t)q0 * ldo;
        t.s2_out = s2_out + (int64_t)q0 * ldo;
        ITAL_LAUNCH(influence_tile_kernel<true>, dim3((unsigned)tiles, 1), dim3(256), 0, stream, t, s);
        rc = ital_check_launch("ital_gp_preview_remove(tile)");
        if (rc) return rc;
    }
    return 0;
}
