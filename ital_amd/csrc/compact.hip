// Deleting data rows: the survivors' feature rows and norms, and their columns of V, mu and s2, gathered into fresh buffers
// (include/ital_compact.h).  No arithmetic: every survivor keeps its bits.
//
// HBM-bound: each kept byte is read once and written once, plus one 8-B index per kept row; the zero rows and pad columns of
// V_dst are written only.
//
//   rows: one wave per DESTINATION row, bounded grid-stride over the rows (as ingest_rows_kernel).  keep[j] is read once per
//         row (every lane loads the same address: one request), then a lane moves 16 B of the row per step -- a padded row is
//         a multiple of 32 B in every element type, and rows start on 16-B boundaries of a 16-B aligned matrix.
//   cols: a thread owns one destination column, a workgroup 256 neighbouring ones.  The thread loads its keep[j] ONCE into a
//         register and walks the m rows of V, then the zero rows m .. v_rows_dst, then mu and s2: the index array is read
//         once, not m + 2 times.  Removed rows are sparse, so neighbouring lanes read neighbouring addresses of a row of V
//         almost everywhere (a wave's 512 B split where a row was removed) and write 512 contiguous bytes.
//
// An index outside [0, n) is never turned into an address: its destination entries become +0.0 and bit 0 of the status word is
// set by an atomicOr of the lane that saw it.  No LDS, no other atomics, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ital_compact.h"
#include "ital_hip.h"
#include "ital_ingest.h"
#include "ital_internal.h"
#include "rows_elem.h"

namespace ital {

template <class E>
__global__ __launch_bounds__(256) void compact_rows_kernel(const typename E::raw* __restrict__ X,
                                                           const double* __restrict__ xnorm, int64_t n, int ldx,
                                                           const int64_t* __restrict__ keep, int64_t n_keep,
                                                           typename E::raw* __restrict__ X_dst,
                                                           double* __restrict__ xnorm_dst, int* __restrict__ status) {
    typedef typename E::raw raw;
    constexpr int PER = 16 / (int)sizeof(raw);             // elements in 16 B; ldx is a multiple of 16, so of PER
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int vecs = ldx / PER;
    for (int64_t j = wave; j < n_keep; j += nwaves) {
        const int64_t i = keep[j];
        uint4* dst = reinterpret_cast<uint4*>(X_dst + j * ldx);
        if (i >= 0 && i < n) {                              // the same for the whole wave
            const uint4* src = reinterpret_cast<const uint4*>(X + i * ldx);
            for (int q = lane; q < vecs; q += 64) dst[q] = src[q];
            if (lane == 0) xnorm_dst[j] = xnorm[i];
        } else {
            for (int q = lane; q < vecs; q += 64) dst[q] = uint4{0u, 0u, 0u, 0u};
            if (lane == 0) {
                xnorm_dst[j] = 0.0;
                if (status) atomicOr(status, 1);
            }
        }
    }
}

template <class E>
static int launch_compact_rows(const void* X, const double* xnorm, int64_t n, int ldx, const int64_t* keep, int64_t n_keep,
                               void* X_dst, double* xnorm_dst, int* status, hipStream_t stream) {
    typedef typename E::raw raw;
    int64_t blocks = (n_keep + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    ITAL_LAUNCH(compact_rows_kernel<E>, dim3((unsigned)blocks), dim3(256), 0, stream, static_cast<const raw*>(X), xnorm, n, ldx,
                keep, n_keep, static_cast<raw*>(X_dst), xnorm_dst, status);
    return ital_check_launch("ital_compact_rows");
}

__global__ __launch_bounds__(256) void compact_cols_kernel(const double* __restrict__ V, int64_t ldv, int m,
                                                           const double* __restrict__ mu, const double* __restrict__ s2,
                                                           int64_t n, const int64_t* __restrict__ keep, int64_t n_keep,
                                                           double* __restrict__ V_dst, int64_t ldv_dst, int v_rows_dst,
                                                           double* __restrict__ mu_dst, double* __restrict__ s2_dst,
                                                           int* __restrict__ status) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= ldv_dst) return;
    const bool live = j < n_keep;                           // a destination column that holds a survivor; beyond: pad
    int64_t i = 0;
    bool ok = false;
    if (live) {
        i = keep[j];
        ok = i >= 0 && i < n;
        if (!ok && status) atomicOr(status, 1);
    }
    double* dst = V_dst + j;
    int r = 0;
    if (ok) {
        const double* src = V + i;
        for (; r + 4 <= m; r += 4) {                        // four independent loads in flight per lane
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = src[(int64_t)(r + u) * ldv];
#pragma unroll
            for (int u = 0; u < 4; u++) dst[(int64_t)(r + u) * ldv_dst] = v[u];
        }
        for (; r < m; r++) dst[(int64_t)r * ldv_dst] = src[(int64_t)r * ldv];
    }
    for (; r < v_rows_dst; r++) dst[(int64_t)r * ldv_dst] = 0.0;      // pad columns, a refused index, rows m .. v_rows_dst
    if (live) {
        mu_dst[j] = ok ? mu[i] : 0.0;
        s2_dst[j] = ok ? s2[i] : 0.0;
    }
}

// [a, a + na) and [b, b + nb) as byte ranges: do they share a byte?
static bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return na > 0 && nb > 0 && pa < pb + nb && pb < pa + na;
}

}  // namespace ital

using namespace ital;

extern "C" int ital_compact_rows(const void* X, const double* xnorm, int64_t n, int ldx, int xtype, const int64_t* keep,
                                 int64_t n_keep, void* X_dst, double* xnorm_dst, int* status, hipStream_t stream) {
    if (n < 0) return ital_fail(-22, "ital_compact_rows: negative number of rows");
    if (n_keep < 0 || n_keep > n) return ital_fail(-22, "ital_compact_rows: n_keep outside 0..n");
    if (ldx < 16 || ldx % 16 != 0) return ital_fail(-22, "ital_compact_rows: ldx must be a positive multiple of 16");
    const uint64_t es = (uint64_t)rows_elem_size(xtype);
    if (es == 0) return ital_fail(-22, "ital_compact_rows: xtype must be 0 (f64), 1 (f32), 2 (f16) or 3 (bf16)");
    if (n_keep > 0 && (!X || !xnorm || !keep || !X_dst || !xnorm_dst))
        return ital_fail(-22, "ital_compact_rows: X / xnorm / keep / X_dst / xnorm_dst must all be given");
    if (reinterpret_cast<uintptr_t>(X) % 16 != 0 || reinterpret_cast<uintptr_t>(X_dst) % 16 != 0)
        return ital_fail(-22, "ital_compact_rows: X and X_dst must be aligned to 16 B");
    const uint64_t row = (uint64_t)ldx * es;
    if (overlap(X, (uint64_t)n * row, X_dst, (uint64_t)n_keep * row) || overlap(xnorm, (uint64_t)n * 8, xnorm_dst, (uint64_t)n_keep * 8))
        return ital_fail(-22, "ital_compact_rows: a destination overlaps its source (the call is out of place)");
    if (n_keep == 0) return 0;
    switch (xtype) {
        case ITAL_INGEST_F64: return launch_compact_rows<IngestF64>(X, xnorm, n, ldx, keep, n_keep, X_dst, xnorm_dst, status, stream);
        case ITAL_INGEST_F32: return launch_compact_rows<IngestF32>(X, xnorm, n, ldx, keep, n_keep, X_dst, xnorm_dst, status, stream);
        case ITAL_INGEST_F16: return launch_compact_rows<IngestF16>(X, xnorm, n, ldx, keep, n_keep, X_dst, xnorm_dst, status, stream);
        default: return launch_compact_rows<IngestBF16>(X, xnorm, n, ldx, keep, n_keep, X_dst, xnorm_dst, status, stream);
    }
}

extern "C" int ital_compact_cols(const double* V, int64_t ldv, int m, const double* mu, const double* s2, int64_t n,
                                 const int64_t* keep, int64_t n_keep, double* V_dst, int64_t ldv_dst, int v_rows_dst,
                                 double* mu_dst, double* s2_dst, int* status, hipStream_t stream) {
    if (n < 0) return ital_fail(-22, "ital_compact_cols: negative number of rows");
    if (n_keep < 0 || n_keep > n) return ital_fail(-22, "ital_compact_cols: n_keep outside 0..n");
    if (m < 0 || v_rows_dst < m) return ital_fail(-22, "ital_compact_cols: m must be in 0..v_rows_dst");
    if (ldv_dst < 0 || ldv_dst % 16 != 0) return ital_fail(-22, "ital_compact_cols: ldv_dst must be a multiple of 16");
    if (ldv_dst < n_keep) return ital_fail(-22, "ital_compact_cols: ldv_dst smaller than n_keep");
    if (m > 0 && ldv < n) return ital_fail(-22, "ital_compact_cols: ldv smaller than n");
    if (n_keep > 0 && (!mu || !s2 || !keep || !mu_dst || !s2_dst || (m > 0 && !V)))
        return ital_fail(-22, "ital_compact_cols: V / mu / s2 / keep / mu_dst / s2_dst must all be given");
    if (v_rows_dst > 0 && ldv_dst > 0 && !V_dst) return ital_fail(-22, "ital_compact_cols: V_dst must be given");
    const uint64_t v_src = m > 0 ? ((uint64_t)(m - 1) * (uint64_t)ldv + (uint64_t)n) * 8 : 0;
    if (overlap(V, v_src, V_dst, (uint64_t)v_rows_dst * (uint64_t)ldv_dst * 8) ||
        overlap(mu, (uint64_t)n * 8, mu_dst, (uint64_t)n_keep * 8) || overlap(s2, (uint64_t)n * 8, s2_dst, (uint64_t)n_keep * 8))
        return ital_fail(-22, "ital_compact_cols: a destination overlaps its source (the call is out of place)");
    if (ldv_dst == 0 || (n_keep == 0 && v_rows_dst == 0)) return 0;
    const int64_t blocks = (ldv_dst + 255) / 256;
    if (blocks > 0x7fffffff) return ital_fail(-22, "ital_compact_cols: too many columns per call");
    ITAL_LAUNCH(compact_cols_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, V, ldv, m, mu, s2, n, keep, n_keep, V_dst, ldv_dst,
                v_rows_dst, mu_dst, s2_dst, status);
    return ital_check_launch("ital_compact_cols");
}
