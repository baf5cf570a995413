// Element types of feature rows (the ITAL_INGEST_* codes of include/ital_ingest.h): the raw storage type and its EXACT
// widening conversion to FP64.  Shared by the ingest kernels (ingest.hip) and by every kernel that reads whole feature rows
// of a store kept in its source precision (include/ital_rows.h: rbf.hip, rewhiten.hip, select_common.h, mcmi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The check every entry point over typed feature rows (include/ital_rows.h) makes before any HIP call (rows.hip): -22 with
// `who_type` for an unknown element type code, with `who_align` for an X that is not aligned to 16 B; 0 otherwise.
int ital_rows_check(const void* X, int xtype, const char* who_type, const char* who_align);

namespace ital {

struct IngestF64 {
    typedef double raw;
    static __device__ __forceinline__ double cv(raw v) { return v; }
};
struct IngestF32 {
    typedef float raw;
    static __device__ __forceinline__ double cv(raw v) { return (double)v; }
};
struct IngestF16 {
    typedef uint16_t raw;
    static __device__ __forceinline__ double cv(raw v) {
        _Float16 h;
        __builtin_memcpy(&h, &v, 2);
        return (double)h;
    }
};
struct IngestBF16 {
    typedef uint16_t raw;
    static __device__ __forceinline__ double cv(raw v) {       // bf16 is the upper half of the f32 with the same value
        const uint32_t u = (uint32_t)v << 16;
        float f;
        __builtin_memcpy(&f, &u, 4);
        return (double)f;
    }
};

// The data-row operands of one trip of an FP64 MFMA dot-product loop: N steps, four consecutive features per lane and step.
// A step's four features are loaded as ONE vector of 4 * sizeof(raw) bytes (8 B at f16 / bf16, 16 B at f32; FP64 keeps the
// two 16-B halves it always had) and widened in registers when the MFMA takes them.  p must be aligned to the vector: rows
// start on multiples of 16 elements of a 16-B aligned matrix.
template <class E, int N>
struct Quads {
    typedef typename E::raw raw;
    typedef raw vec __attribute__((ext_vector_type(4)));
    vec v[N];
    __device__ __forceinline__ void zero(int u) { v[u] = vec{0, 0, 0, 0}; }
    __device__ __forceinline__ void load(int u, const raw* p) { v[u] = *reinterpret_cast<const vec*>(p); }
    __device__ __forceinline__ double get(int u, int i) const { return E::cv(v[u][i]); }
};
template <int N>
struct Quads<IngestF64, N> {
    double2 b01[N], b23[N];
    __device__ __forceinline__ void zero(int u) { b01[u] = b23[u] = double2{0, 0}; }
    __device__ __forceinline__ void load(int u, const double* p) {
        b01[u] = *reinterpret_cast<const double2*>(p);
        b23[u] = *reinterpret_cast<const double2*>(p + 2);
    }
    __device__ __forceinline__ double get(int u, int i) const {
        return i == 0 ? b01[u].x : i == 1 ? b01[u].y : i == 2 ? b23[u].x : b23[u].y;
    }
};

// One feature row widened into an FP64 destination by the calling workgroup (the record of a selection, a gathered block).
template <class E>
__device__ __forceinline__ void widen_row(double* __restrict__ dst, const void* X, int64_t row, int ldx) {
    const typename E::raw* src = static_cast<const typename E::raw*>(X) + row * ldx;
    for (int k = threadIdx.x; k < ldx; k += blockDim.x) dst[k] = E::cv(src[k]);
}

// Bytes of one element of type code `xtype`; 0 for an unknown code.
static inline int rows_elem_size(int xtype) { return xtype == 0 ? 8 : xtype == 1 ? 4 : (xtype == 2 || xtype == 3) ? 2 : 0; }

}  // namespace ital
