// Cosine distance of every data row to its nearest labelled row (include/ital_cosine.h): the N x m x d product of the RBMAL
// learner.  The dot products are formed as in whiten_rows_body (rewhiten.hip): a wave owns a tile of 16 data rows, reads it
// once per chunk of 64 labelled rows and feeds four accumulators of v_mfma_f64_16x16x4_f64 (16 labelled rows each); the data
// rows are read in the store's element type and widened in registers (rows_elem.h).  What follows the dot product is one
// division, two roots and a running minimum per pair, in registers: nothing but out[] is written.
//
// Order of the sum of one pair: k ascending in steps of 16, within a step the four MFMAs of the lane's features 0..3, within
// an MFMA the hardware's fixed order over its four k-groups.  The trip count is ldx / 16 rounded up to even, the odd trip
// feeding zeros: a function of ldx alone.  Every element of an MFMA result is computed from its own row and column only, so
// neither the position of a row in its tile nor the other rows of the tile enter.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ital_cosine.h"
#include "ital_hip.h"
#include "ital_internal.h"
#include "rows_elem.h"

namespace ital {

typedef double d4 __attribute__((ext_vector_type(4)));

struct CosineArgs {
    const void* X;        // [n][ldx] of the element type the kernel is instantiated for
    const double* xnorm;  // [n]
    int64_t n;
    int ldx;
    const double* T;      // [c][ldx]
    const double* tnorm;  // [c]
    int c;
    int accumulate;
    double* out;          // [n]
};

constexpr int COSINE_G = 4;               // accumulators per wave: 16 G labelled rows per pass over the data rows

// min(a, b) that keeps a NaN, as np.min; the order of the operands does not matter for anything but a NaN's payload, which
// the kernel replaces at its end.
__device__ __forceinline__ double nan_min(double a, double b) { return (a != a) ? a : (b != b) ? b : (b < a ? b : a); }

template <class E>
__global__ __launch_bounds__(256) void cosine_min_kernel(CosineArgs a) {
    constexpr int G = COSINE_G;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int col = lane & 15;   // MFMA: A row / B column / D column
    const int kg = lane >> 4;    // MFMA: k index / D row group
    const int64_t i0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    if (i0 >= a.n) return;       // whole waves only: the shuffles below see all 64 lanes
    const int64_t irow = i0 + col;
    const bool row_ok = irow < a.n;
    const typename E::raw* xrow = static_cast<const typename E::raw*>(a.X) + (row_ok ? irow : 0) * a.ldx;
    const double xroot = row_ok ? sqrt(a.xnorm[irow]) : 1.0;
    double best = INFINITY;

    for (int c0 = 0; c0 < a.c; c0 += 16 * G) {
        const int nb = (min(a.c, c0 + 16 * G) - c0 + 15) >> 4;    // blocks of 16 labelled rows in this pass, 1..G
        d4 acc[G];
#pragma unroll
        for (int g = 0; g < G; g++) acc[g] = d4{0, 0, 0, 0};
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
                    const int r = c0 + 16 * g + col;
                    if (in && r < a.c) {
                        const double* trow = a.T + (int64_t)r * a.ldx;
                        a01[u][g] = *reinterpret_cast<const double2*>(trow + kk);
                        a23[u][g] = *reinterpret_cast<const double2*>(trow + kk + 2);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 2; u++) {
#pragma unroll
                for (int g = 0; g < G; g++) {
                    if (g < nb) {
                        acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a01[u][g].x, b.get(u, 0), acc[g], 0, 0, 0);
                        acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a01[u][g].y, b.get(u, 1), acc[g], 0, 0, 0);
                        acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a23[u][g].x, b.get(u, 2), acc[g], 0, 0, 0);
                        acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a23[u][g].y, b.get(u, 3), acc[g], 0, 0, 0);
                    }
                }
            }
        }
        // D layout (f64 16x16x4): element reg -> labelled row j = kg + 4 reg of the block, data row i = col
#pragma unroll
        for (int g = 0; g < G; g++) {
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int j = c0 + 16 * g + kg + 4 * reg;
                if (g < nb && j < a.c) {
                    double cs = acc[g][reg] / (xroot * sqrt(a.tnorm[j]));
                    if (fabs(cs) > 1.0) cs = copysign(1.0, cs);
                    best = nan_min(best, 1.0 - cs);
                }
            }
        }
    }
    // the four k-groups hold the labelled rows j = kg (mod 4) of data row `col`
    best = nan_min(best, __shfl_xor(best, 16));
    best = nan_min(best, __shfl_xor(best, 32));
    if (kg == 0 && row_ok) {
        if (a.accumulate) best = nan_min(a.out[irow], best);
        a.out[irow] = (best != best) ? __builtin_nan("") : best;
    }
}

template <class E>
static int launch_cosine_min(const CosineArgs& a, hipStream_t stream) {
    const int64_t blocks = (a.n + 63) / 64;
    ITAL_LAUNCH(cosine_min_kernel<E>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    return ital_check_launch("ital_cosine_min");
}

}  // namespace ital

using namespace ital;

extern "C" int ital_cosine_min(const void* X, int xtype, const double* xnorm, int64_t n, int ldx, const double* T,
                               const double* tnorm, int c, int accumulate, double* out, hipStream_t stream) {
    if (n < 0) return ital_fail(-22, "ital_cosine_min: negative number of rows");
    if (n > ((int64_t)1 << 36)) return ital_fail(-22, "ital_cosine_min: more rows than one launch covers");
    if (c < 1) return ital_fail(-22, "ital_cosine_min: needs at least one labelled row");
    if (ldx <= 0 || ldx % 16 != 0) return ital_fail(-22, "ital_cosine_min: ldx must be a positive multiple of 16");
    if (rows_elem_size(xtype) == 0) return ital_fail(-22, "ital_cosine_min: unknown element type of X");
    if (n == 0) return 0;
    if (!X || !xnorm || !T || !tnorm || !out) return ital_fail(-22, "ital_cosine_min: X / xnorm / T / tnorm / out must all be given");
    if (reinterpret_cast<uintptr_t>(X) % 16 != 0) return ital_fail(-22, "ital_cosine_min: X must be aligned to 16 B");
    if (reinterpret_cast<uintptr_t>(T) % 16 != 0) return ital_fail(-22, "ital_cosine_min: T must be aligned to 16 B");
    CosineArgs a = {X, xnorm, n, ldx, T, tnorm, c, accumulate, out};
    switch (xtype) {
        case ITAL_INGEST_F64: return launch_cosine_min<IngestF64>(a, stream);
        case ITAL_INGEST_F32: return launch_cosine_min<IngestF32>(a, stream);
        case ITAL_INGEST_F16: return launch_cosine_min<IngestF16>(a, stream);
        default: return launch_cosine_min<IngestBF16>(a, stream);
    }
}
