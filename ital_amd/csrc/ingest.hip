// Feature rows in the caller's type and stride -> padded FP64 rows and their squared norms (include/ital_ingest.h).
//
// HBM-bound: per element one load of the source type and one 8-B store (12 B at f32, 16 B at f64), then the norms read the
// written rows once more.  The norms are a launch of ital_row_norms itself, not fused: xnorm is DEFINED by that kernel's bits,
// and a second copy of `acc += v.x * v.x + v.y * v.y` is only the same number as long as the compiler contracts both alike
// (rewhiten.hip calls ital_row_norms for the same reason).
//
// One wave per row, bounded grid-stride over the rows (as row_norms_kernel).  Two load paths, chosen on the host per call:
//   wide:    a lane loads 16 B of the row (2 f64, 4 f32, 8 f16 / bf16) and stores 1, 2 or 4 times 16 B;
//   element: a lane loads two single elements and stores 16 B -- for a source whose address or row stride is no multiple of 16 B.
// A vector that straddles column d is read element by element in both paths, so nothing behind a row's last element is
// touched.  No LDS, no atomics, no scratch.  The element types and their converters live in rows_elem.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ital_hip.h"
#include "ital_ingest.h"
#include "ital_internal.h"
#include "ital_rows.h"
#include "rows_elem.h"

namespace ital {

template <class E, bool WIDE>
__global__ __launch_bounds__(256) void ingest_rows_kernel(const typename E::raw* __restrict__ src, int64_t n, int d,
                                                          int64_t ld_src, double* __restrict__ X, int ldx) {
    typedef typename E::raw raw;
    // elements a lane converts per step: ldx is a multiple of 16 and PER divides 16, so k + PER <= ldx for every k below
    constexpr int PER = WIDE ? 16 / (int)sizeof(raw) : 2;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i = wave; i < n; i += nwaves) {
        const raw* s = src + i * ld_src;
        double* x = X + i * ldx;
        for (int k = lane * PER; k < ldx; k += 64 * PER) {
            double v[PER];
            if (WIDE && k + PER <= d) {
                const uint4 w = *reinterpret_cast<const uint4*>(s + k);
                raw r[PER];
                __builtin_memcpy(r, &w, 16);
#pragma unroll
                for (int e = 0; e < PER; e++) v[e] = E::cv(r[e]);
            } else {
#pragma unroll
                for (int e = 0; e < PER; e++) v[e] = k + e < d ? E::cv(s[k + e]) : 0.0;
            }
#pragma unroll
            for (int e = 0; e < PER; e += 2) *reinterpret_cast<double2*>(x + k + e) = double2{v[e], v[e + 1]};
        }
    }
}

template <class E>
static int launch_ingest(const void* src, bool wide, int64_t n, int d, int64_t ld_src, double* X, int ldx, hipStream_t stream) {
    typedef typename E::raw raw;
    int64_t blocks = (n + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    const raw* s = static_cast<const raw*>(src);
    if (wide)
        ITAL_LAUNCH((ingest_rows_kernel<E, true>), dim3((unsigned)blocks), dim3(256), 0, stream, s, n, d, ld_src, X, ldx);
    else
        ITAL_LAUNCH((ingest_rows_kernel<E, false>), dim3((unsigned)blocks), dim3(256), 0, stream, s, n, d, ld_src, X, ldx);
    return ital_check_launch("ital_ingest_rows");
}

// The same rows WITHOUT a conversion: padded rows of the source's own type (include/ital_rows.h).  A lane copies 8 B of the
// row per step (4 f16 / bf16, 2 f32): ldx elements are a multiple of 32 B, so every step stays inside the padded row.  WIDE:
// the source rows start on 8-B boundaries and a step that lies wholly before column d is one 8-B load; every other step --
// and every step of an unaligned or odd-strided source -- reads single elements and never one at or behind column d.
template <class R, bool WIDE>
__global__ __launch_bounds__(256) void ingest_same_kernel(const R* __restrict__ src, int64_t n, int d, int64_t ld_src,
                                                          R* __restrict__ X, int ldx) {
    constexpr int PER = 8 / (int)sizeof(R);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i = wave; i < n; i += nwaves) {
        const R* s = src + i * ld_src;
        R* x = X + i * ldx;
        for (int k = lane * PER; k < ldx; k += 64 * PER) {
            uint2 w;
            if (WIDE && k + PER <= d) {
                w = *reinterpret_cast<const uint2*>(s + k);
            } else {
                R r[PER];
#pragma unroll
                for (int e = 0; e < PER; e++) r[e] = k + e < d ? s[k + e] : (R)0;      // all bits 0: +0 of every type
                __builtin_memcpy(&w, r, 8);
            }
            *reinterpret_cast<uint2*>(x + k) = w;
        }
    }
}

template <class R>
static int launch_ingest_same(const void* src, int64_t n, int d, int64_t ld_src, void* X, int ldx, hipStream_t stream) {
    int64_t blocks = (n + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    const R* s = static_cast<const R*>(src);
    const bool wide = reinterpret_cast<uintptr_t>(src) % 8 == 0 && ((uint64_t)ld_src * sizeof(R)) % 8 == 0;
    if (wide)
        ITAL_LAUNCH((ingest_same_kernel<R, true>), dim3((unsigned)blocks), dim3(256), 0, stream, s, n, d, ld_src, static_cast<R*>(X), ldx);
    else
        ITAL_LAUNCH((ingest_same_kernel<R, false>), dim3((unsigned)blocks), dim3(256), 0, stream, s, n, d, ld_src, static_cast<R*>(X), ldx);
    return ital_check_launch("ital_ingest_rows_t");
}

}  // namespace ital

using namespace ital;

extern "C" int ital_ingest_rows_t(const void* src, int dtype, int64_t n, int d, int64_t ld_src, void* X, int ldx, double* xnorm,
                                  double* scratch, int64_t scratch_rows, hipStream_t stream) {
    if (n < 0) return ital_fail(-22, "ital_ingest_rows_t: negative number of rows");
    if (d < 1) return ital_fail(-22, "ital_ingest_rows_t: d must be at least 1");
    if (ldx % 16 != 0) return ital_fail(-22, "ital_ingest_rows_t: ldx must be a multiple of 16");
    if (ldx < d) return ital_fail(-22, "ital_ingest_rows_t: ldx smaller than d");
    if (ld_src < d) return ital_fail(-22, "ital_ingest_rows_t: ld_src smaller than d");
    if (dtype < ITAL_INGEST_F64 || dtype > ITAL_INGEST_BF16) return ital_fail(-22, "ital_ingest_rows_t: dtype must be 0 (f64), 1 (f32), 2 (f16) or 3 (bf16)");
    if (n > 0 && (!src || !X || !xnorm)) return ital_fail(-22, "ital_ingest_rows_t: src / X / xnorm must all be given");
    const uintptr_t es = (uintptr_t)rows_elem_size(dtype);
    if (reinterpret_cast<uintptr_t>(src) % es != 0) return ital_fail(-22, "ital_ingest_rows_t: src is not aligned to its element size");
    if (reinterpret_cast<uintptr_t>(X) % 16 != 0 || reinterpret_cast<uintptr_t>(xnorm) % 8 != 0)
        return ital_fail(-22, "ital_ingest_rows_t: X must be aligned to 16 B and xnorm to 8 B");
    const bool narrow = dtype != ITAL_INGEST_F64;
    if (narrow && n > 0 && (!scratch || scratch_rows < 1)) return ital_fail(-22, "ital_ingest_rows_t: a scratch block of at least one FP64 row is needed");
    if (reinterpret_cast<uintptr_t>(scratch) % 16 != 0) return ital_fail(-22, "ital_ingest_rows_t: scratch must be aligned to 16 B");
    if (n == 0) return 0;
    if (!narrow) return ital_ingest_rows(src, dtype, n, d, ld_src, static_cast<double*>(X), ldx, xnorm, stream);
    // the norms: ital_ingest_rows itself on one bounded block after the other, its xnorm written straight to its place
    for (int64_t r0 = 0; r0 < n; r0 += scratch_rows) {
        const int64_t k = n - r0 < scratch_rows ? n - r0 : scratch_rows;
        const int rc = ital_ingest_rows(static_cast<const char*>(src) + (size_t)r0 * (size_t)ld_src * es, dtype, k, d, ld_src, scratch,
                                        ldx, xnorm + r0, stream);
        if (rc) return rc;
    }
    return dtype == ITAL_INGEST_F32 ? launch_ingest_same<uint32_t>(src, n, d, ld_src, X, ldx, stream)
                                    : launch_ingest_same<uint16_t>(src, n, d, ld_src, X, ldx, stream);
}

extern "C" int ital_ingest_rows(const void* src, int dtype, int64_t n, int d, int64_t ld_src, double* X, int ldx, double* xnorm,
                                hipStream_t stream) {
    if (n < 0) return ital_fail(-22, "ital_ingest_rows: negative number of rows");
    if (d < 1) return ital_fail(-22, "ital_ingest_rows: d must be at least 1");
    if (ldx % 16 != 0) return ital_fail(-22, "ital_ingest_rows: ldx must be a multiple of 16");
    if (ldx < d) return ital_fail(-22, "ital_ingest_rows: ldx smaller than d");
    if (ld_src < d) return ital_fail(-22, "ital_ingest_rows: ld_src smaller than d");
    if (dtype < ITAL_INGEST_F64 || dtype > ITAL_INGEST_BF16) return ital_fail(-22, "ital_ingest_rows: dtype must be 0 (f64), 1 (f32), 2 (f16) or 3 (bf16)");
    if (n > 0 && (!src || !X || !xnorm)) return ital_fail(-22, "ital_ingest_rows: src / X / xnorm must all be given");
    const uintptr_t es = dtype == ITAL_INGEST_F64 ? 8 : dtype == ITAL_INGEST_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(src) % es != 0) return ital_fail(-22, "ital_ingest_rows: src is not aligned to its element size");
    if (reinterpret_cast<uintptr_t>(X) % 16 != 0 || reinterpret_cast<uintptr_t>(xnorm) % 8 != 0)
        return ital_fail(-22, "ital_ingest_rows: X must be aligned to 16 B and xnorm to 8 B");
    if (n == 0) return 0;
    // the wide path: every row starts on a 16-B boundary
    const bool wide = reinterpret_cast<uintptr_t>(src) % 16 == 0 && ((uint64_t)ld_src * es) % 16 == 0;
    int rc;
    switch (dtype) {
        case ITAL_INGEST_F64: rc = launch_ingest<IngestF64>(src, wide, n, d, ld_src, X, ldx, stream); break;
        case ITAL_INGEST_F32: rc = launch_ingest<IngestF32>(src, wide, n, d, ld_src, X, ldx, stream); break;
        case ITAL_INGEST_F16: rc = launch_ingest<IngestF16>(src, wide, n, d, ld_src, X, ldx, stream); break;
        default: rc = launch_ingest<IngestBF16>(src, wide, n, d, ld_src, X, ldx, stream); break;
    }
    if (rc) return rc;
    return ital_row_norms(X, n, ldx, xnorm, stream);
}
