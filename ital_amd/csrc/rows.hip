// What the entry points over typed feature rows (include/ital_rows.h) share and what has no better home: their common
// argument check, and the candidate-block gather of mcmi.hip for rows kept in their source precision.  mcmi.hip itself is
// left as it is: its FP64 gather stays the code behind ital_gather_block, and ital_gather_block_t hands FP64 rows to it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ital_hip.h"
#include "ital_internal.h"
#include "ital_rows.h"
#include "rows_elem.h"

namespace ital {

// gather_block_kernel of mcmi.hip with the feature row widened (exactly) while it is copied: Xc is FP64 whatever X is.
// Workgroup per candidate; a sample that lives on another rank contributes zeros.
template <class E>
__global__ __launch_bounds__(128) void gather_block_rows_kernel(const int64_t* __restrict__ cand, int64_t nc, int64_t row0,
                                                                int64_t n_rows, const void* __restrict__ X,
                                                                const double* __restrict__ xnorm, int ldx,
                                                                const double* __restrict__ V, int64_t ldv, int m,
                                                                const double* __restrict__ mu, const double* __restrict__ s2,
                                                                double* __restrict__ Xc, double* __restrict__ Vc, int64_t ldc,
                                                                double* __restrict__ xnc, double* __restrict__ muc,
                                                                double* __restrict__ s2c) {
    const int64_t j = blockIdx.x;
    if (j >= nc) return;
    const int64_t loc = cand[j] - row0;
    const bool own = loc >= 0 && loc < n_rows;
    const typename E::raw* src = static_cast<const typename E::raw*>(X) + (own ? loc : 0) * (int64_t)ldx;
    double* dst = Xc + j * (int64_t)ldx;
    for (int q = threadIdx.x; q < ldx; q += blockDim.x) dst[q] = own ? E::cv(src[q]) : 0.0;
    for (int r = threadIdx.x; r < m; r += blockDim.x) Vc[(int64_t)r * ldc + j] = own ? V[(int64_t)r * ldv + loc] : 0.0;
    if (threadIdx.x == 0) {
        xnc[j] = own ? xnorm[loc] : 0.0;
        muc[j] = own ? mu[loc] : 0.0;
        s2c[j] = own ? s2[loc] : 0.0;
    }
}

}  // namespace ital

using namespace ital;

int ital_rows_check(const void* X, int xtype, const char* who_type, const char* who_align) {
    if (rows_elem_size(xtype) == 0) return ital_fail(-22, who_type);
    if (reinterpret_cast<uintptr_t>(X) % 16 != 0) return ital_fail(-22, who_align);
    return 0;
}

extern "C" int ital_gather_block_t(const int64_t* cand, int64_t nc, int64_t row0, int64_t n_rows, const void* X,
                                   const double* xnorm, int ldx, const double* V, int64_t ldv, int m, const double* mu,
                                   const double* s2, double* Xc, double* Vc, int64_t ldc, double* xnc, double* muc,
                                   double* s2c, int xtype, hipStream_t stream) {
    const int trc = ital_rows_check(X, xtype, "ital_gather_block: unknown element type of X",
                                    "ital_gather_block: X must be aligned to 16 B");
    if (trc) return trc;
    if (xtype == ITAL_INGEST_F64)
        return ital_gather_block(cand, nc, row0, n_rows, static_cast<const double*>(X), xnorm, ldx, V, ldv, m, mu, s2, Xc, Vc, ldc,
                                 xnc, muc, s2c, stream);
    if (nc <= 0) return 0;
    if (!cand || !X || !xnorm || !mu || !s2 || !Xc || !xnc || !muc || !s2c || (m > 0 && (!V || !Vc)))
        return ital_fail(-22, "ital_gather_block: null argument");
    if (ldx <= 0 || m < 0 || ldc < nc || n_rows < 0) return ital_fail(-22, "ital_gather_block: bad sizes");
    if (nc > 0x7fffffff) return ital_fail(-22, "ital_gather_block: too many candidates per call");
#define ITAL_GATHER(E) ITAL_LAUNCH(gather_block_rows_kernel<E>, dim3((unsigned)nc), dim3(128), 0, stream, cand, nc, row0, n_rows, \
                                   X, xnorm, ldx, V, ldv, m, mu, s2, Xc, Vc, ldc, xnc, muc, s2c)
    switch (xtype) {
        case ITAL_INGEST_F32: ITAL_GATHER(IngestF32); break;
        case ITAL_INGEST_F16: ITAL_GATHER(IngestF16); break;
        default: ITAL_GATHER(IngestBF16); break;
    }
#undef ITAL_GATHER
    return ital_check_launch("ital_gather_block");
}
