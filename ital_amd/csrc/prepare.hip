// Preparing feature rows on the device (include/ital_prepare.h, where every result is defined).
//
// col_stats_kernel / col_stats_combine_kernel: a workgroup owns one row range and 64 columns; lane = column, wave = chain
// (rows of the range at distance 4), so a wave reads 64 consecutive elements of a row.  The four chains meet in LDS in a
// fixed order, the ranges in the second kernel in ascending order.
//
// scale_rows_kernel: workgroup = 64 rows x 64 columns, lane = column; subtract then divide.
//
// col_cov_kernel: the hot path.  Workgroup (t, r) owns the lower-triangular tile pair t = (ti, tj) of 128 x 128 columns and
// the row range r; both operands are k-major (k = the row of X), so the product is tile::tile_tn with fetch functors that
// widen an element, subtract its column's mean and mask rows past the range and columns past d AFTER that.  Its tile goes
// to the range's partial matrix in the workspace; col_cov_combine_kernel adds the partials in ascending order and writes
// every number to (a, b) and (b, a).
//
// project_rows_kernel: workgroup (rows, columns) owns 128 x 128 of Y, or 128 x 64 when k <= 64.  The first operand is read as
// rows of X (the staging roles of tile::tile_nt, widened and shifted when fetched), the second as k-major rows of W (the roles
// of tile::tile_tn); both land in the LDS layout of mfma_tile.h.  Each wave owns 32 rows and ALL the tile's columns
// (project_stage), in the k order of tile::mfma_stage.  The epilogue narrows and stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "ital_hip.h"
#include "ital_internal.h"
#include "ital_prepare.h"
#include "mfma_tile.h"
#include "rows_elem.h"

namespace ital {

using tile::d4;

// ------------------------------------------------------------------------------------------------------ the range rule
struct Ranges {
    int64_t count, rows;      // number of ranges, rows per range (the last may be shorter)
};

static Ranges prepare_ranges(int64_t n, int unit, int cap) {
    if (n <= 0 || unit < 1 || cap < 1) return {0, 0};
    const int64_t units = (n + unit - 1) / unit;
    const int64_t per = (units + std::min<int64_t>(cap, units) - 1) / std::min<int64_t>(cap, units);
    return {(units + per - 1) / per, per * unit};
}

static int cov_cap(int d) {
    if (d < 1) return 0;
    const int64_t c = ((int64_t)1 << 24) / ((int64_t)d * d);
    return (int)std::max<int64_t>(1, std::min<int64_t>(c, ITAL_PREPARE_COV_CAP));
}

// ------------------------------------------------------------------------------------------------------ narrowing
// v rounded to nearest, ties to even, onto the numbers with `mbits` fraction bits and least normal exponent `emin`, as a
// double; `over` = the largest finite number plus half a unit in its last place.  ONE rounding: v is scaled by a power of two
// (exact), rounded to an integer by v_rndne_f64 and scaled back (exact).
__device__ __forceinline__ double round_to(double v, int mbits, int emin, double over) {
    if (v != v) return v;
    const double a = fabs(v);
    if (a >= over) return copysign((double)INFINITY, v);
    if (a == 0) return v;
    int e = ((__double2hiint(a) >> 20) & 0x7ff) - 1023;       // a subnormal double: -1023, below every emin
    if (e < emin) e = emin;
    const int q = e - mbits;
    return copysign(ldexp(rint(ldexp(a, -q)), q), v);
}

__device__ __forceinline__ void store_elem(void* Y, int ytype, int64_t at, double v) {
    if (ytype == ITAL_INGEST_F64) {
        static_cast<double*>(Y)[at] = v;
    } else if (ytype == ITAL_INGEST_F32) {
        static_cast<float*>(Y)[at] = (float)v;                 // v_cvt_f32_f64: to nearest even, overflow to infinity
    } else if (ytype == ITAL_INGEST_F16) {
        const _Float16 h = (_Float16)(float)round_to(v, 10, -14, 65520.0);      // both conversions exact
        uint16_t u;
        __builtin_memcpy(&u, &h, 2);
        static_cast<uint16_t*>(Y)[at] = u;
    } else {
        const float f = (float)round_to(v, 7, -126, 0x1.ffp127);                // exact: bf16 is the upper half of an f32
        uint32_t u;
        __builtin_memcpy(&u, &f, 4);
        static_cast<uint16_t*>(Y)[at] = (uint16_t)(u >> 16);
    }
}

// ------------------------------------------------------------------------------------------------------ column statistics
struct StatsArgs {
    const void* X;
    int64_t n, rows, count;   // rows per range, number of ranges
    int d, ldx;
    double *cmin, *cmax, *csum;
    double* part;             // workspace: [count][3][d]
};

template <class E>
__global__ __launch_bounds__(256) void col_stats_kernel(StatsArgs a) {
    typedef typename E::raw raw;
    __shared__ double sh[3][4][64];
    const int lane = threadIdx.x & 63, chain = threadIdx.x >> 6;
    const int col = 64 * blockIdx.y + lane;
    const int64_t r0 = (int64_t)blockIdx.x * a.rows, r1 = min(a.n, r0 + a.rows);
    double mn = INFINITY, mx = -INFINITY, sum = 0.0;
    bool bad = false;
    if (col < a.d) {
        const raw* p = static_cast<const raw*>(a.X) + col;
        for (int64_t i = r0 + chain; i < r1; i += 4) {
            const double v = E::cv(p[i * a.ldx]);
            bad |= v != v;
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
            sum += v;
        }
    }
    sh[0][chain][lane] = bad ? __builtin_nan("") : mn;
    sh[1][chain][lane] = mx;
    sh[2][chain][lane] = sum;
    __syncthreads();
    if (chain == 0 && col < a.d) {
        mn = sh[0][0][lane];
        mx = sh[1][0][lane];
        sum = sh[2][0][lane];
        bad = mn != mn;
#pragma unroll
        for (int c = 1; c < 4; c++) {
            const double m = sh[0][c][lane], x = sh[1][c][lane];
            bad |= m != m;
            mn = m < mn ? m : mn;
            mx = x > mx ? x : mx;
            sum += sh[2][c][lane];
        }
        double* out = a.part + (int64_t)blockIdx.x * 3 * a.d + col;
        out[0] = bad ? __builtin_nan("") : mn;
        out[a.d] = mx;
        out[2 * (int64_t)a.d] = sum;
    }
}

__global__ __launch_bounds__(256) void col_stats_combine_kernel(StatsArgs a) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= a.d) return;
    const double* in = a.part + col;
    double mn = in[0], mx = in[a.d], sum = in[2 * (int64_t)a.d];
    bool bad = mn != mn;
    for (int64_t r = 1; r < a.count; r++) {
        in += 3 * (int64_t)a.d;
        const double m = in[0], x = in[a.d];
        bad |= m != m;
        mn = m < mn ? m : mn;
        mx = x > mx ? x : mx;
        sum += in[2 * (int64_t)a.d];
    }
    const double nan = __builtin_nan("");
    a.cmin[col] = bad ? nan : mn;
    a.cmax[col] = bad ? nan : mx;
    a.csum[col] = bad ? nan : sum;
}

// ------------------------------------------------------------------------------------------------------ scaling
struct ScaleArgs {
    const void* X;
    int64_t n;
    int d, ldx;
    const double *lo, *span;
    void* Y;
    int ytype, ldy;
};

constexpr int SCALE_ROWS = 64;        // rows per workgroup of scale_rows_kernel

// Workgroup (x, y): SCALE_ROWS rows and 64 columns of Y.  Lane = column, so lo and span are read once per thread and a wave
// reads and writes 64 consecutive elements of a row; wave w takes every fourth row.  No index is divided.
template <class E>
__global__ __launch_bounds__(256) void scale_rows_kernel(ScaleArgs a) {
    typedef typename E::raw raw;
    const int j = 64 * blockIdx.y + (threadIdx.x & 63);
    if (j >= a.ldy) return;
    const bool on = j < a.d;
    const double lo = on ? a.lo[j] : 0.0, span = on ? a.span[j] : 1.0;
    const int64_t r0 = (int64_t)SCALE_ROWS * blockIdx.x, r1 = min(a.n, r0 + SCALE_ROWS);
    for (int64_t i = r0 + (threadIdx.x >> 6); i < r1; i += 4) {
        double v = 0.0;
        if (on) v = (E::cv(static_cast<const raw*>(a.X)[i * a.ldx + j]) - lo) / span;
        store_elem(a.Y, a.ytype, i * a.ldy + j, v);
    }
}

// ------------------------------------------------------------------------------------------------------ scatter matrix
struct CovArgs {
    const void* X;
    int64_t n, rows, count;   // rows per range, number of ranges
    int d, ldx;
    const double* mean;
    double* C;
    int64_t ldc;
    double* part;             // workspace: [count][d][d]
};

template <class E>
__global__ __launch_bounds__(256) void col_cov_kernel(CovArgs a) {
    typedef typename E::raw raw;
    __shared__ tile::StageLds lds;
    int ti, tj;
    tile::tri_pair(blockIdx.x, ti, tj);
    const int64_t r0 = (int64_t)blockIdx.y * a.rows;
    const int len = (int)min(a.n - r0, a.rows);                       // >= 1
    const raw* X = static_cast<const raw*>(a.X) + r0 * a.ldx;
    const int ca = tile::T * ti, cb = tile::T * tj, c16 = threadIdx.x & 15;
    double ma[8], mb[8];                                              // the means of the 2 x 8 columns this thread stages
    bool oa[8], ob[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
        oa[u] = ca + c16 + 16 * u < a.d;
        ob[u] = cb + c16 + 16 * u < a.d;
        ma[u] = oa[u] ? a.mean[ca + c16 + 16 * u] : 0.0;
        mb[u] = ob[u] ? a.mean[cb + c16 + 16 * u] : 0.0;
    }
    auto fa = [&](int k, int r) {
        const int u = r >> 4;
        return (k < len && oa[u]) ? E::cv(X[(int64_t)k * a.ldx + ca + r]) - ma[u] : 0.0;
    };
    auto fb = [&](int k, int c) {
        const int u = c >> 4;
        return (k < len && ob[u]) ? E::cv(X[(int64_t)k * a.ldx + cb + c]) - mb[u] : 0.0;
    };
    d4 acc[4][4];
    tile::zero_acc(acc);
    tile::tile_tn(fa, fb, 0, len, lds, acc);
    const tile::DLane dl = tile::d_lane();
    double* P = a.part + (int64_t)blockIdx.y * a.d * a.d;
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int row = ca + dl.row(p, reg);
            if (row >= a.d) continue;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int col = cb + dl.column(q);
                if (col < a.d) P[(int64_t)row * a.d + col] = acc[p][q][reg];
            }
        }
}

// Element (i, j), j <= i, of every partial (all in lower-triangular tiles, which col_cov_kernel wrote whole) -> C[i][j], C[j][i].
__global__ __launch_bounds__(256) void col_cov_combine_kernel(CovArgs a) {
    const int64_t dd = (int64_t)a.d * a.d;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= dd) return;
    const int64_t i = e / a.d, j = e - i * a.d;
    if (j > i) return;
    double s = a.part[e];
    for (int64_t r = 1; r < a.count; r++) s += a.part[r * dd + e];
    a.C[i * a.ldc + j] = s;
    a.C[j * a.ldc + i] = s;
}

// ------------------------------------------------------------------------------------------------------ projection
struct ProjectArgs {
    const void* X;
    int64_t n;
    int d, ldx;
    const double *shift, *W;
    int64_t ldw;
    int k;
    void* Y;
    int ytype, ldy;
};

// One staged step of 16 columns of X for the calling wave's 32 rows x 16 NQ columns of Y: the k order of tile::mfma_stage
// (j = 0..3, the lane's group kg reads k = 4 kg + j), another split of the tile among the waves -- every wave spans all its
// columns, so a narrow Y (k <= 64: NQ = 4) costs half the MFMAs instead of idling two waves.
template <int NQ>
__device__ __forceinline__ void project_stage(tile::StageLds& lds, int buf, d4 (&acc)[2][NQ]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, kg = lane >> 4;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double av[2], bv[NQ];
#pragma unroll
        for (int p = 0; p < 2; p++) av[p] = lds[buf][0][4 * kg + j][32 * wave + 16 * p + col];
#pragma unroll
        for (int q = 0; q < NQ; q++) bv[q] = lds[buf][1][4 * kg + j][16 * q + col];
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int q = 0; q < NQ; q++) acc[p][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[p], bv[q], acc[p][q], 0, 0, 0);
    }
}

// NQ = 8: 128 x 128 of Y per workgroup; NQ = 4: 128 x 64.
template <class E, int NQ>
__global__ __launch_bounds__(256) void project_rows_kernel(ProjectArgs a) {
    typedef typename E::raw raw;
    constexpr int T = tile::T, KS = tile::KS, TW = 16 * NQ;
    __shared__ tile::StageLds lds;
    const int64_t row0 = (int64_t)T * blockIdx.x;
    const int c0 = TW * blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    d4 acc[2][NQ];
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
        for (int q = 0; q < NQ; q++) acc[p][q] = (d4){0, 0, 0, 0};
    if (c0 < a.k) {                                                   // uniform in the workgroup; else the tile is all pad
        int sk, srow;
        tile::stage_role(sk, srow);
        const int kb = threadIdx.x >> 4, c16 = threadIdx.x & 15;
        const raw* pa[4];
#pragma unroll
        for (int u = 0; u < 4; u++) pa[u] = static_cast<const raw*>(a.X) + min(row0 + srow + 8 * u, a.n - 1) * a.ldx + sk;
        double2 ra[4];
        double rb[NQ];
        auto fetch = [&](int k0) {
            const bool on0 = k0 + sk < a.d, on1 = k0 + sk + 1 < a.d;
            const double s0 = on0 ? a.shift[k0 + sk] : 0.0, s1 = on1 ? a.shift[k0 + sk + 1] : 0.0;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                ra[u].x = on0 ? E::cv(pa[u][k0]) - s0 : 0.0;
                ra[u].y = on1 ? E::cv(pa[u][k0 + 1]) - s1 : 0.0;
            }
            const bool onk = k0 + kb < a.d;
#pragma unroll
            for (int u = 0; u < NQ; u++) {
                const int c = c0 + c16 + 16 * u;
                rb[u] = (onk && c < a.k) ? a.W[(int64_t)(k0 + kb) * a.ldw + c] : 0.0;
            }
        };
        auto stage = [&](int buf) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                lds[buf][0][sk][srow + 8 * u] = ra[u].x;
                lds[buf][0][sk + 1][srow + 8 * u] = ra[u].y;
            }
#pragma unroll
            for (int u = 0; u < NQ; u++) lds[buf][1][kb][c16 + 16 * u] = rb[u];
        };
        fetch(0);
        stage(0);
        __syncthreads();
        const int nstep = a.ldx / KS;
        for (int s_ = 0; s_ < nstep; s_++) {
            const int buf = s_ & 1;
            if (s_ + 1 < nstep) fetch((s_ + 1) * KS);
            project_stage<NQ>(lds, buf, acc);
            if (s_ + 1 < nstep) stage(buf ^ 1);
            __syncthreads();
        }
    }
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int64_t row = row0 + 32 * wave + 16 * p + (lane >> 4) + 4 * reg;      // D layout of the f64 MFMA
            if (row >= a.n) continue;
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                const int col = c0 + 16 * q + (lane & 15);
                if (col < a.ldy) store_elem(a.Y, a.ytype, row * a.ldy + col, col < a.k ? acc[p][q][reg] : 0.0);
            }
        }
}

template <class E>
static void launch_project(const ProjectArgs& a, hipStream_t stream) {
    const unsigned rows = (unsigned)((a.n + tile::T - 1) / tile::T);
    if (a.k <= 64)
        ITAL_LAUNCH((project_rows_kernel<E, 4>), dim3(rows, (unsigned)((a.ldy + 63) / 64)), dim3(256), 0, stream, a);
    else
        ITAL_LAUNCH((project_rows_kernel<E, 8>), dim3(rows, (unsigned)((a.ldy + 127) / 128)), dim3(256), 0, stream, a);
}

// ------------------------------------------------------------------------------------------------------ launches
#define PREPARE_DISPATCH(xtype, KERNEL, grid, stream, args)                                                  \
    do {                                                                                                     \
        switch (xtype) {                                                                                     \
            case ITAL_INGEST_F64: ITAL_LAUNCH(KERNEL<IngestF64>, grid, dim3(256), 0, stream, args); break;   \
            case ITAL_INGEST_F32: ITAL_LAUNCH(KERNEL<IngestF32>, grid, dim3(256), 0, stream, args); break;   \
            case ITAL_INGEST_F16: ITAL_LAUNCH(KERNEL<IngestF16>, grid, dim3(256), 0, stream, args); break;   \
            default: ITAL_LAUNCH(KERNEL<IngestBF16>, grid, dim3(256), 0, stream, args); break;               \
        }                                                                                                    \
    } while (0)

static bool misaligned(const void* p, uintptr_t to) { return reinterpret_cast<uintptr_t>(p) % to != 0; }

}  // namespace ital

using namespace ital;

extern "C" int64_t ital_prepare_ranges(int64_t n, int unit, int cap) { return prepare_ranges(n, unit, cap).count; }

extern "C" int ital_col_cov_cap(int d) { return cov_cap(d); }

extern "C" size_t ital_col_stats_workspace(int64_t n, int d) {
    if (n < 0 || n > INT32_MAX || d < 1) return 0;
    return (size_t)prepare_ranges(n, ITAL_PREPARE_STATS_UNIT, ITAL_PREPARE_STATS_CAP).count * 3 * (size_t)d * sizeof(double);
}

extern "C" size_t ital_col_cov_workspace(int64_t n, int d) {
    if (n < 0 || n > INT32_MAX || d < 1) return 0;
    return (size_t)prepare_ranges(n, ITAL_PREPARE_COV_UNIT, cov_cap(d)).count * (size_t)d * (size_t)d * sizeof(double);
}

extern "C" int ital_col_stats(const void* X, int xtype, int64_t n, int d, int ldx, double* cmin, double* cmax, double* csum,
                              void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (n < 0 || n > INT32_MAX) return ital_fail(-22, "ital_col_stats: the number of rows must be in [0, 2^31 - 1]");
    if (d < 1) return ital_fail(-22, "ital_col_stats: d must be positive");
    if (ldx <= 0 || ldx % 16 != 0 || ldx < d) return ital_fail(-22, "ital_col_stats: ldx must be a multiple of 16, at least d");
    if (rows_elem_size(xtype) == 0) return ital_fail(-22, "ital_col_stats: unknown element type of X");
    if (n == 0) return 0;
    if (!X || !cmin || !cmax || !csum || !workspace) return ital_fail(-22, "ital_col_stats: X, the outputs and the workspace must be given");
    if (misaligned(X, 16)) return ital_fail(-22, "ital_col_stats: X must be aligned to 16 B");
    if (misaligned(cmin, 8) || misaligned(cmax, 8) || misaligned(csum, 8) || misaligned(workspace, 8))
        return ital_fail(-22, "ital_col_stats: the outputs and the workspace must be aligned to 8 B");
    if (workspace_bytes < ital_col_stats_workspace(n, d)) return ital_fail(-22, "ital_col_stats: the workspace is too small");
    const Ranges rg = prepare_ranges(n, ITAL_PREPARE_STATS_UNIT, ITAL_PREPARE_STATS_CAP);
    StatsArgs a = {X, n, rg.rows, rg.count, d, ldx, cmin, cmax, csum, static_cast<double*>(workspace)};
    const dim3 grid((unsigned)rg.count, (unsigned)((d + 63) / 64));
    PREPARE_DISPATCH(xtype, col_stats_kernel, grid, stream, a);
    if (int rc = ital_check_launch("ital_col_stats")) return rc;
    ITAL_LAUNCH(col_stats_combine_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, stream, a);
    return ital_check_launch("ital_col_stats");
}

extern "C" int ital_scale_rows(const void* X, int xtype, int64_t n, int d, int ldx, const double* lo, const double* span, void* Y,
                               int ytype, int ldy, hipStream_t stream) {
    if (n < 0 || n > INT32_MAX) return ital_fail(-22, "ital_scale_rows: the number of rows must be in [0, 2^31 - 1]");
    if (d < 1) return ital_fail(-22, "ital_scale_rows: d must be positive");
    if (ldx <= 0 || ldx % 16 != 0 || ldx < d) return ital_fail(-22, "ital_scale_rows: ldx must be a multiple of 16, at least d");
    if (ldy <= 0 || ldy % 16 != 0 || ldy < d) return ital_fail(-22, "ital_scale_rows: ldy must be a multiple of 16, at least d");
    if (rows_elem_size(xtype) == 0) return ital_fail(-22, "ital_scale_rows: unknown element type of X");
    if (rows_elem_size(ytype) == 0) return ital_fail(-22, "ital_scale_rows: unknown element type of Y");
    if (n == 0) return 0;
    if (!X || !lo || !span || !Y) return ital_fail(-22, "ital_scale_rows: X, lo, span and Y must be given");
    if (misaligned(X, 16) || misaligned(Y, 16)) return ital_fail(-22, "ital_scale_rows: X and Y must be aligned to 16 B");
    if (misaligned(lo, 8) || misaligned(span, 8)) return ital_fail(-22, "ital_scale_rows: lo and span must be aligned to 8 B");
    ScaleArgs a = {X, n, d, ldx, lo, span, Y, ytype, ldy};
    const dim3 grid((unsigned)((n + SCALE_ROWS - 1) / SCALE_ROWS), (unsigned)((ldy + 63) / 64));
    PREPARE_DISPATCH(xtype, scale_rows_kernel, grid, stream, a);
    return ital_check_launch("ital_scale_rows");
}

extern "C" int ital_col_cov(const void* X, int xtype, int64_t n, int d, int ldx, const double* mean, double* C, int64_t ldc,
                            void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (n < 0 || n > INT32_MAX) return ital_fail(-22, "ital_col_cov: the number of rows must be in [0, 2^31 - 1]");
    if (d < 1) return ital_fail(-22, "ital_col_cov: d must be positive");
    if (ldx <= 0 || ldx % 16 != 0 || ldx < d) return ital_fail(-22, "ital_col_cov: ldx must be a multiple of 16, at least d");
    if (ldc < d) return ital_fail(-22, "ital_col_cov: ldc must be at least d");
    if (rows_elem_size(xtype) == 0) return ital_fail(-22, "ital_col_cov: unknown element type of X");
    if (n == 0) return 0;
    if (!X || !mean || !C || !workspace) return ital_fail(-22, "ital_col_cov: X, mean, C and the workspace must be given");
    if (misaligned(X, 16)) return ital_fail(-22, "ital_col_cov: X must be aligned to 16 B");
    if (misaligned(mean, 8) || misaligned(C, 8) || misaligned(workspace, 8))
        return ital_fail(-22, "ital_col_cov: mean, C and the workspace must be aligned to 8 B");
    if (workspace_bytes < ital_col_cov_workspace(n, d)) return ital_fail(-22, "ital_col_cov: the workspace is too small");
    const Ranges rg = prepare_ranges(n, ITAL_PREPARE_COV_UNIT, cov_cap(d));
    CovArgs a = {X, n, rg.rows, rg.count, d, ldx, mean, C, ldc, static_cast<double*>(workspace)};
    const int64_t nt = (d + tile::T - 1) / tile::T;
    const dim3 grid((unsigned)(nt * (nt + 1) / 2), (unsigned)rg.count);
    PREPARE_DISPATCH(xtype, col_cov_kernel, grid, stream, a);
    if (int rc = ital_check_launch("ital_col_cov")) return rc;
    ITAL_LAUNCH(col_cov_combine_kernel, dim3((unsigned)(((int64_t)d * d + 255) / 256)), dim3(256), 0, stream, a);
    return ital_check_launch("ital_col_cov");
}

extern "C" int ital_project_rows(const void* X, int xtype, int64_t n, int d, int ldx, const double* shift, const double* W,
                                 int64_t ldw, int k, void* Y, int ytype, int ldy, hipStream_t stream) {
    if (n < 0 || n > INT32_MAX) return ital_fail(-22, "ital_project_rows: the number of rows must be in [0, 2^31 - 1]");
    if (d < 1) return ital_fail(-22, "ital_project_rows: d must be positive");
    if (k < 1 || k > ITAL_PREPARE_MAX_K) return ital_fail(-22, "ital_project_rows: k must be in [1, 512]");
    if (ldx <= 0 || ldx % 16 != 0 || ldx < d) return ital_fail(-22, "ital_project_rows: ldx must be a multiple of 16, at least d");
    if (ldy <= 0 || ldy % 16 != 0 || ldy < k) return ital_fail(-22, "ital_project_rows: ldy must be a multiple of 16, at least k");
    if (ldw < k) return ital_fail(-22, "ital_project_rows: ldw must be at least k");
    if (rows_elem_size(xtype) == 0) return ital_fail(-22, "ital_project_rows: unknown element type of X");
    if (rows_elem_size(ytype) == 0) return ital_fail(-22, "ital_project_rows: unknown element type of Y");
    if (n == 0) return 0;
    if (!X || !shift || !W || !Y) return ital_fail(-22, "ital_project_rows: X, shift, W and Y must be given");
    if (misaligned(X, 16) || misaligned(Y, 16)) return ital_fail(-22, "ital_project_rows: X and Y must be aligned to 16 B");
    if (misaligned(shift, 8) || misaligned(W, 8)) return ital_fail(-22, "ital_project_rows: shift and W must be aligned to 8 B");
    ProjectArgs a = {X, n, d, ldx, shift, W, ldw, k, Y, ytype, ldy};
    switch (xtype) {
        case ITAL_INGEST_F64: launch_project<IngestF64>(a, stream); break;
        case ITAL_INGEST_F32: launch_project<IngestF32>(a, stream); break;
        case ITAL_INGEST_F16: launch_project<IngestF16>(a, stream); break;
        default: launch_project<IngestBF16>(a, stream); break;
    }
    return ital_check_launch("ital_project_rows");
}
