// Whitening a range of data rows against the whole labelled set (include/ital_rewhiten.h): the transpose of the rank-c append
// of rbf.hip.  Per 16-row tile of X and per block of 16 labelled rows the arithmetic is kcols_body's MODE_WHITEN, operation
// for operation (the result is DEFINED as the composition of those sweeps, bit for bit); what differs is where the operands
// come from:
//   - the feature tile is read once per launch and feeds the dot products of a whole chunk of 16*G labelled rows
//     (G accumulators of v_mfma_f64_16x16x4_f64, 4 registers each) instead of being read again for every 16 of them;
//   - the whitened values of the chunk's earlier blocks are read back from LDS ([labelled row][16] per wave), not from V;
//     only the rows of earlier CHUNKS (earlier launches) come from global memory -- no launch reads what it wrote itself;
//   - mu and s2 stay in registers over the blocks of a launch.
// The expressions below restate kcols_body's (same order, same shapes, so that the compiler contracts them alike); rbf.hip
// itself is left as it is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ital_hip.h"
#include "ital_internal.h"
#include "ital_rewhiten.h"
#include "ital_rows.h"
#include "rows_elem.h"

namespace ital {

typedef double d4 __attribute__((ext_vector_type(4)));

struct RewhitenArgs {
    const void* X;        // [n][ldx] the range, of the element type the kernel is instantiated for (rows_elem.h)
    const double* xnorm;  // [n] (FP64 rows: written by ital_row_norms before the first launch; narrower: the store's)
    int64_t n;
    int ldx;
    const double* XT;     // [m][ldx]
    const double* XTn;    // [m]
    const double* L;      // [m][ldl]
    int ldl;
    const double* alpha;  // [m]
    int c0, c1;           // labelled rows of this launch: [c0, c1), c0 a multiple of the chunk
    double* V;            // [..][ldv]
    int64_t ldv;
    int z0, z1;           // rows of V this launch zeroes: [z0, z1) (the last launch: m .. capacity)
    double var, s;        // s = -2 l^2
    double* mu;
    double* s2;
};

constexpr int REWHITEN_DEFAULT_CHUNK = 64;
constexpr int REWHITEN_TILE = 16 * 17;         // the R[j][i] transpose buffer of kcols_body

// LDS doubles per wave: the chunk's whitened values [16 G][16], then the transpose buffer.
template <int G> constexpr int rewhiten_wave_doubles() { return 16 * G * 16 + REWHITEN_TILE; }

// E: element type of X.  As in kcols_body only the fetch of the data rows depends on it (one vector load of a lane's four
// features in X's type, widened exactly when the MFMA takes them).
template <int G, class E>
__device__ __forceinline__ void whiten_rows_body(const RewhitenArgs& a) {
    extern __shared__ double rewhiten_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int col = lane & 15;   // MFMA: A row / B column / D column
    const int kg = lane >> 4;    // MFMA: k index / D row group
    const int64_t i0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    if (i0 >= a.n) return;
    double* vl = rewhiten_lds + wave * rewhiten_wave_doubles<G>();   // vl[(r - c0) * 16 + i]
    double* tile = vl + 16 * G * 16;                                  // tile[j * 17 + i]
    const int64_t irow = i0 + col;
    const bool row_ok = irow < a.n;
    const typename E::raw* xrow = static_cast<const typename E::raw*>(a.X) + (row_ok ? irow : 0) * a.ldx;
    const int nb = (a.c1 - a.c0 + 15) >> 4;       // blocks of 16 labelled rows in this launch, 0..G

    // ---- dot products of the tile with every labelled row of the chunk: k ascending, 16 k-values per step; per element
    // the MFMA sequence of kcols_body (a trailing step of zero operands there adds +0 to an accumulator that is never -0)
    d4 acc_dot[G];
#pragma unroll
    for (int g = 0; g < G; g++) acc_dot[g] = d4{0, 0, 0, 0};
    for (int k0 = 0; k0 < a.ldx; k0 += 32) {
        Quads<E, 2> b;
        double2 a01[2][G], a23[2][G];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int kk = k0 + 16 * u + 4 * kg;
            const bool in = k0 + 16 * u < a.ldx;           // ldx is a multiple of 16
            b.zero(u);
            if (in && row_ok) b.load(u, xrow + kk);
#pragma unroll
            for (int g = 0; g < G; g++) {
                a01[u][g] = a23[u][g] = double2{0, 0};
                const int r = a.c0 + 16 * g + col;
                if (in && r < a.c1) {
                    const double* srow = a.XT + (int64_t)r * a.ldx;
                    a01[u][g] = *reinterpret_cast<const double2*>(srow + kk);
                    a23[u][g] = *reinterpret_cast<const double2*>(srow + kk + 2);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
#pragma unroll
            for (int g = 0; g < G; g++) {
                if (g < nb) {
                    acc_dot[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a01[u][g].x, b.get(u, 0), acc_dot[g], 0, 0, 0);
                    acc_dot[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a01[u][g].y, b.get(u, 1), acc_dot[g], 0, 0, 0);
                    acc_dot[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a23[u][g].x, b.get(u, 2), acc_dot[g], 0, 0, 0);
                    acc_dot[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a23[u][g].y, b.get(u, 3), acc_dot[g], 0, 0, 0);
                }
            }
        }
    }

    const double xn = row_ok ? a.xnorm[irow] : 0.0;
    // lanes 0..15 own one data row each in the substitution: its mean and variance over the blocks of the launch
    double muv = 0.0, s2v = a.var;
    if (lane < 16 && row_ok && a.c0 > 0) {
        muv = a.mu[irow];
        s2v = a.s2[irow];
    }

#pragma unroll
    for (int g = 0; g < G; g++) {
        if (g < nb) {
            const int b0 = a.c0 + 16 * g;                  // first labelled row of the block = rows whitened before it
            const int c = a.c1 - b0 < 16 ? a.c1 - b0 : 16;
            const bool sel_ok = col < c;
            // ---- S = L21 V over the rows before the block, from a zero accumulator, r ascending
            d4 acc_s = {0, 0, 0, 0};
            for (int r0 = 0; r0 < b0; r0 += 16) {
                double av[4], bv[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int r = r0 + 4 * u + kg;
                    av[u] = bv[u] = 0;
                    if (sel_ok) av[u] = a.L[(int64_t)(b0 + col) * a.ldl + r];
                    if (r0 < a.c0) {                       // an earlier launch's rows
                        if (row_ok) bv[u] = a.V[(int64_t)r * a.ldv + irow];
                    } else {                               // this launch's: LDS (0 in the columns past the last row)
                        bv[u] = vl[(r - a.c0) * 16 + col];
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; u++) acc_s = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc_s, 0, 0, 0);
            }
            // ---- epilogue.  D layout (f64 16x16x4): element reg -> row j = kg + 4*reg, column i = col.
            double R[4];
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int j = kg + 4 * reg;
                double v = 0;
                if (j < c) {
                    const double snj = a.XTn[b0 + j];
                    v = a.var * exp((snj + xn - 2 * acc_dot[g][reg]) / a.s) - acc_s[reg];
                }
                R[reg] = v;
            }
#pragma unroll
            for (int reg = 0; reg < 4; reg++) tile[(kg + 4 * reg) * 17 + col] = R[reg];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (lane < 16) {
                if (row_ok) {
                    const double* L22 = a.L + (int64_t)b0 * a.ldl + b0;
                    double vn[16];
                    double dvar = 0, dmu = 0;
#pragma unroll
                    for (int j = 0; j < 16; j++) {
                        if (j < c) {
                            double acc = tile[j * 17 + lane];
#pragma unroll
                            for (int q = 0; q < j; q++) acc -= L22[j * a.ldl + q] * vn[q];
                            vn[j] = acc / L22[j * a.ldl + j];
                            dvar += vn[j] * vn[j];
                            dmu += vn[j] * a.alpha[b0 + j];
                            a.V[(int64_t)(b0 + j) * a.ldv + irow] = vn[j];
                            vl[(16 * g + j) * 16 + lane] = vn[j];
                        } else {
                            vn[j] = 0;
                        }
                    }
                    s2v -= dvar;
                    muv += dmu;
                } else {
#pragma unroll
                    for (int j = 0; j < 16; j++) vl[(16 * g + j) * 16 + lane] = 0;
                }
            }
            // the next block reads vl (all lanes) and overwrites tile
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    if (lane < 16 && row_ok) {
        a.mu[irow] = muv;
        a.s2[irow] = s2v;
    }
    if (row_ok)
        for (int r = a.z0 + kg; r < a.z1; r += 4) a.V[(int64_t)r * a.ldv + irow] = 0.0;
}

template <int G>
__global__ __launch_bounds__(256) void whiten_rows_kernel(RewhitenArgs a) { whiten_rows_body<G, IngestF64>(a); }

// The same sweep over rows kept in their source precision (include/ital_rows.h); the FP64 kernel above keeps its name.
template <int G, class E>
__global__ __launch_bounds__(256) void whiten_typed_rows_kernel(RewhitenArgs a) { whiten_rows_body<G, E>(a); }

template <int G, class E>
static int launch_whiten_rows_of(const RewhitenArgs& a, void (*kernel)(RewhitenArgs), hipStream_t stream) {
    static ItalLdsFlags flags;                    // one set per kernel: the attribute belongs to the function
    const int lds = 4 * rewhiten_wave_doubles<G>() * (int)sizeof(double);
    if (lds > 48 * 1024) {
        const int rc = ital_raise_lds_limit(reinterpret_cast<const void*>(kernel), lds, flags, "ital_whiten_rows");
        if (rc) return rc;
    }
    const int64_t blocks = (a.n + 63) / 64;
    ITAL_LAUNCH(kernel, dim3((unsigned)blocks), dim3(256), lds, stream, a);
    return ital_check_launch("ital_whiten_rows");
}

template <int G>
static int launch_whiten_rows(const RewhitenArgs& a, int xtype, hipStream_t stream) {
    switch (xtype) {
        case ITAL_INGEST_F64: return launch_whiten_rows_of<G, IngestF64>(a, whiten_rows_kernel<G>, stream);
        case ITAL_INGEST_F32: return launch_whiten_rows_of<G, IngestF32>(a, whiten_typed_rows_kernel<G, IngestF32>, stream);
        case ITAL_INGEST_F16: return launch_whiten_rows_of<G, IngestF16>(a, whiten_typed_rows_kernel<G, IngestF16>, stream);
        default: return launch_whiten_rows_of<G, IngestBF16>(a, whiten_typed_rows_kernel<G, IngestBF16>, stream);
    }
}

}  // namespace ital

using namespace ital;

extern "C" int ital_whiten_rows_chunk(void) { return REWHITEN_DEFAULT_CHUNK; }

extern "C" int ital_whiten_rows(const ital_rewhiten_desc* d, hipStream_t stream) {
    return ital_whiten_rows_t(d, ITAL_INGEST_F64, stream);
}

extern "C" int ital_whiten_rows_t(const ital_rewhiten_desc* d, int xtype, hipStream_t stream) {
    if (!d) return ital_fail(-22, "ital_whiten_rows: NULL descriptor");
    if (rows_elem_size(xtype) == 0) return ital_fail(-22, "ital_whiten_rows: unknown element type of X");
    if (!d->X || !d->xnorm || !d->V || !d->mu || !d->s2) return ital_fail(-22, "ital_whiten_rows: X / xnorm / V / mu / s2 must all be given");
    if (d->n_rows < 0 || d->m < 0 || d->v_rows < 0) return ital_fail(-22, "ital_whiten_rows: negative size");
    if (d->n_rows > ((int64_t)1 << 36)) return ital_fail(-22, "ital_whiten_rows: more rows than one launch covers");
    if (d->ldx <= 0 || d->ldx % 16 != 0) return ital_fail(-22, "ital_whiten_rows: ldx must be a positive multiple of 16");
    if (d->m > 0 && (!d->XT || !d->XTn || !d->L || !d->alpha)) return ital_fail(-22, "ital_whiten_rows: XT / XTn / L / alpha missing");
    if (d->ldl < d->m) return ital_fail(-22, "ital_whiten_rows: ldl smaller than the labelled set");
    if (d->ldv < d->n_rows) return ital_fail(-22, "ital_whiten_rows: ldv smaller than the number of rows");
    if (d->v_rows < d->m) return ital_fail(-22, "ital_whiten_rows: v_rows smaller than the labelled set");
    const int chunk = d->chunk ? d->chunk : REWHITEN_DEFAULT_CHUNK;
    if (chunk != 32 && chunk != 64 && chunk != 128) return ital_fail(-22, "ital_whiten_rows: chunk must be 0, 32, 64 or 128");
    if (reinterpret_cast<uintptr_t>(d->X) % 16 != 0) return ital_fail(-22, "ital_whiten_rows: X must be aligned to 16 B");
    if (d->n_rows == 0) return 0;
    int rc = 0;
    // FP64 rows: the norms are part of the result.  Narrower rows: the store's xnorm already holds these bits (input only).
    if (xtype == ITAL_INGEST_F64 && (rc = ital_row_norms(d->X, d->n_rows, d->ldx, d->xnorm, stream))) return rc;
    RewhitenArgs a = {};
    a.X = d->X; a.xnorm = d->xnorm; a.n = d->n_rows; a.ldx = d->ldx;
    a.XT = d->XT; a.XTn = d->XTn; a.L = d->L; a.ldl = d->ldl; a.alpha = d->alpha;
    a.V = d->V; a.ldv = d->ldv; a.var = d->var; a.s = -2.0 * d->length_scale * d->length_scale;
    a.mu = d->mu; a.s2 = d->s2;
    int c0 = 0;
    do {
        a.c0 = c0;
        a.c1 = d->m - c0 < chunk ? d->m : c0 + chunk;
        const bool last = a.c1 >= d->m;
        a.z0 = last ? d->m : 0;
        a.z1 = last ? d->v_rows : 0;
        rc = chunk == 32 ? launch_whiten_rows<2>(a, xtype, stream) : chunk == 64 ? launch_whiten_rows<4>(a, xtype, stream)
                                                                                  : launch_whiten_rows<8>(a, xtype, stream);
        if (rc) return rc;
        c0 = a.c1;
    } while (c0 < d->m);
    return 0;
}
