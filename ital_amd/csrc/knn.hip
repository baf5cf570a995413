// The k nearest neighbours of rows of a store among rows of the same store (include/ital_knn.h): a tiled self-join.
//
// knn_tile_kernel: a workgroup of 256 threads owns 128 query rows and walks its share of the data rows in tiles of 128.  The
// dot products of a tile come from the staged tile of mfma_tile.h (its constants, its LDS layout and mfma_stage; the staging
// loop below is tile_nt's with the elements widened from the store's type as they are fetched).  The tile loop ends on a
// barrier, so the 66 KB stage buffer is free for the epilogue: the 128 x 128 dot products are written into it in two halves
// of 64 x 132, and a wave takes 16 rows of each half.  The 64 lanes of the wave hold the row's sorted list (lane s: slot s) in
// registers, form the distances of two columns each and compare them against the row's k-th best; the few pairs that pass
// are inserted one by one (a ballot for the position, a shuffle for the shift).  After the first tiles almost every pair
// fails that one comparison -- and for the cosine a cheap estimate in front of it, so that the IEEE division of the
// definition is left to the pairs that can enter the list.
// The lists of the 128 rows live in LDS between tiles.  Nothing is written to memory until the workgroup's last tile: then
// its lists go to the workspace as the partial lists of its split of the data range.
//
// knn_merge_kernel: a wave per query row merges the partial lists of the splits -- and with `accumulate` the entries already
// in dist / idx -- by the same order with the same insertion, and forms rowsum.
//
// Order of the sum of one pair: k ascending in stages of 16, within a stage the four MFMAs j = 0..3 (features 4 kg + j), within
// an MFMA the hardware's fixed order over its four k-groups: a function of ldx alone.  An element of an MFMA result depends on
// its own row and column only, and the two operands enter each product symmetrically, so d(i, j) and d(j, i) are equal in bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ital_hip.h"
#include "ital_internal.h"
#include "ital_knn.h"
#include "mfma_tile.h"
#include "rows_elem.h"

namespace ital {

using tile::d4;

struct KnnArgs {
    const void* X;         // [n][ldx] of the element type the kernel is instantiated for
    const double* xnorm;   // [n]
    int ldx;
    int64_t q0, q1, c0, c1;
    int metric, k, skip_self, accumulate, splits;
    double* dist;          // [nq][k]
    int64_t* idx;          // [nq][k]
    double* rowsum;        // [nq] or null
    double* pdist;         // workspace: [splits][nq][k]
    int* pidx;             // workspace: [splits][nq][k]
};

// The total order of the pairs of one query row: numbers ascending, equal numbers by ascending j, NaN after every number by
// ascending j, an empty slot (j < 0) after everything.
__device__ __forceinline__ bool knn_before(double a, int ja, double b, int jb) {
    const int ra = ja < 0 ? 2 : (a != a ? 1 : 0), rb = jb < 0 ? 2 : (b != b ? 1 : 0);
    if (ra != rb) return ra < rb;
    if (ra == 2) return false;
    if (ra == 0 && a != b) return a < b;
    return ja < jb;
}

// Lane `l` (uniform in the wave) of v: a v_readlane, not a trip through the LDS crossbar as __shfl is.
__device__ __forceinline__ int knn_lane(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ double knn_lane(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// The calling wave holds the sorted list of one query row, lane s < k its slot s (ed, ej).  Every lane offers one pair (d, j)
// if `offer`; the list becomes the first k of the union.  A pair whose j is in the list already is dropped.  All 64 lanes
// call this together.  Returns whether the list changed.
__device__ __forceinline__ bool knn_wave_offer(double& ed, int& ej, int k, double d, int j, bool offer) {
    const int lane = threadIdx.x & 63;
    const bool slot = lane < k;
    bool changed = false;
    double td = knn_lane(ed, k - 1);
    int tj = knn_lane(ej, k - 1);
    bool pass = offer && knn_before(d, j, td, tj);
    unsigned long long mask = __ballot(pass);
    while (mask) {
        const int leader = __builtin_ctzll(mask);
        const double nd = knn_lane(d, leader);
        const int nj = knn_lane(j, leader);
        pass = pass && lane != leader;
        if (!__ballot(slot && ej == nj)) {
            const double ud = __shfl_up(ed, 1);
            const int uj = __shfl_up(ej, 1);
            const int pos = __popcll(__ballot(slot && knn_before(ed, ej, nd, nj)));   // the list is sorted: a prefix
            if (slot && lane > pos) {
                ed = ud;
                ej = uj;
            } else if (lane == pos) {
                ed = nd;
                ej = nj;
            }
            changed = true;
            td = knn_lane(ed, k - 1);
            tj = knn_lane(ej, k - 1);
            pass = pass && knn_before(d, j, td, tj);
        }
        mask = __ballot(pass);
    }
    return changed;
}

// tile::tile_nt with the two operands read as rows of the element type E and widened when they are fetched.
template <class E>
__device__ __forceinline__ void knn_tile_rows(const typename E::raw* const pa[4], const typename E::raw* const pb[4], int K,
                                              tile::StageLds& lds, d4 acc[4][4]) {
    int sk, srow;
    tile::stage_role(sk, srow);
    double2 ra[4], rb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            ra[u].x = E::cv(pa[u][k0]);
            ra[u].y = E::cv(pa[u][k0 + 1]);
            rb[u].x = E::cv(pb[u][k0]);
            rb[u].y = E::cv(pb[u][k0 + 1]);
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            lds[buf][0][sk][srow + 8 * u] = ra[u].x;
            lds[buf][0][sk + 1][srow + 8 * u] = ra[u].y;
            lds[buf][1][sk][srow + 8 * u] = rb[u].x;
            lds[buf][1][sk + 1][srow + 8 * u] = rb[u].y;
        }
    };
    fetch(0);
    stage(0);
    __syncthreads();
    const int nstep = K / tile::KS;
    for (int s_ = 0; s_ < nstep; s_++) {
        const int buf = s_ & 1;
        if (s_ + 1 < nstep) fetch((s_ + 1) * tile::KS);
        tile::mfma_stage(lds, buf, acc);
        if (s_ + 1 < nstep) stage(buf ^ 1);
        __syncthreads();
    }
}

// The list rows in LDS are padded by one slot against bank conflicts.  (A variant with 8 slots for k <= 8 gains nothing: the
// registers of the tile hold the kernel to one workgroup per compute unit whatever its LDS.)
template <class E>
__global__ __launch_bounds__(256) void knn_tile_kernel(KnnArgs a) {
    typedef typename E::raw raw;
    constexpr int T = tile::T, KCAP = ITAL_KNN_MAX_K;
    __shared__ tile::StageLds lds;
    __shared__ double list_d[T][KCAP + 1];
    __shared__ int list_j[T][KCAP + 1];
    __shared__ double qs[T], cs[T];       // metric 0: the roots of the norms of the tile's query / data rows; metric 1: the norms
    __shared__ double rqs[T], rcs[T];     // metric 0: their reciprocals, for the filter in front of the division
    double (*dt)[tile::LDT] = reinterpret_cast<double (*)[tile::LDT]>(&lds);   // [64][132]: half a tile of dot products

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = a.k;
    const int64_t nq = a.q1 - a.q0, nc = a.c1 - a.c0;
    const int64_t qbase = a.q0 + (int64_t)T * blockIdx.x;
    const int qrows = (int)min((int64_t)T, a.q1 - qbase);               // >= 1
    const int64_t ntile = (nc + T - 1) / T;
    const int64_t t0 = ntile * blockIdx.y / a.splits, t1 = ntile * (blockIdx.y + 1) / a.splits;

    for (int e = tid; e < T * k; e += 256) {
        list_d[e / k][e % k] = INFINITY;
        list_j[e / k][e % k] = -1;
    }
    if (tid < T) {
        const double v = a.xnorm[min(qbase + tid, a.q1 - 1)];
        qs[tid] = a.metric == ITAL_KNN_COSINE ? sqrt(v) : v;
        rqs[tid] = 1.0 / qs[tid];
    }
    int sk, srow;
    tile::stage_role(sk, srow);
    const raw* pa[4];
#pragma unroll
    for (int u = 0; u < 4; u++) pa[u] = static_cast<const raw*>(a.X) + min(qbase + srow + 8 * u, a.q1 - 1) * a.ldx + sk;
    const tile::DLane dl = tile::d_lane();

    for (int64_t t = t0; t < t1; t++) {
        const int64_t cbase = a.c0 + T * t;
        const raw* pb[4];
#pragma unroll
        for (int u = 0; u < 4; u++) pb[u] = static_cast<const raw*>(a.X) + min(cbase + srow + 8 * u, a.c1 - 1) * a.ldx + sk;
        if (tid < T) {      // read after the barriers of the tile loop; the last reader of the old values is behind a barrier
            const double v = a.xnorm[min(cbase + tid, a.c1 - 1)];
            cs[tid] = a.metric == ITAL_KNN_COSINE ? sqrt(v) : v;
            rcs[tid] = 1.0 / cs[tid];
        }
        d4 acc[4][4];
        tile::zero_acc(acc);
        knn_tile_rows<E>(pa, pb, a.ldx, lds, acc);
        double cv[2], rcv[2];                                             // of the two columns this lane scans in every row
#pragma unroll
        for (int h = 0; h < 2; h++) {
            cv[h] = cs[lane + 64 * h];
            rcv[h] = rcs[lane + 64 * h];
        }
#pragma unroll 1
        for (int half = 0; half < 2; half++) {
            if (dl.wy == half) {
#pragma unroll
                for (int p = 0; p < 4; p++)
#pragma unroll
                    for (int reg = 0; reg < 4; reg++)
#pragma unroll
                        for (int q = 0; q < 4; q++) dt[16 * p + dl.kg + 4 * reg][dl.column(q)] = acc[p][q][reg];
            }
            __syncthreads();
            for (int r16 = 0; r16 < 16; r16++) {
                const int lr = 16 * wave + r16, row = 64 * half + lr;
                if (row >= qrows) break;                                  // uniform in the wave
                const int64_t i = qbase + row;
                const double qv = qs[row], rqv = rqs[row];
                double ed = INFINITY;
                int ej = -1;
                if (lane < k) {
                    ed = list_d[row][lane];
                    ej = list_j[row][lane];
                }
                const double td = knn_lane(ed, k - 1);                    // NaN or +inf while the list is not full of numbers
                bool changed = false;
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int c = lane + 64 * h;
                    const int64_t j = cbase + c;
                    const double dot = dt[lr][c];
                    bool offer = j < a.c1 && !(a.skip_self && j == i);
                    double d;
                    if (a.metric == ITAL_KNN_COSINE) {
                        // The division is for the pairs that can enter the list.  dot * (1 / root) * (1 / root) is the cosine
                        // to 4 roundings where the definition has 2, and |cos| <= 1 + ldx 2^-53: the two distances differ by
                        // less than 1e-15, so a pair this estimate puts 1e-12 behind the row's k-th best is behind it by the
                        // definition too.  An estimate that is not finite (a zero norm) decides nothing.
                        const double est = dot * rqv * rcv[h];
                        offer = offer && !(1.0 - est > td + 1e-12 && fabs(est) < INFINITY);
                        d = 0;
                        if (__ballot(offer)) {
                            double co = dot / (qv * cv[h]);
                            if (fabs(co) > 1.0) co = copysign(1.0, co);
                            d = 1.0 - co;
                            if (d != d) d = __builtin_nan("");
                        }
                    } else {
                        d = tile::rbf_sqdist(qv, cv[h], dot);
                    }
                    changed |= knn_wave_offer(ed, ej, k, d, (int)j, offer);
                }
                if (changed && lane < k) {
                    list_d[row][lane] = ed;
                    list_j[row][lane] = ej;
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    double* pd = a.pdist + ((int64_t)blockIdx.y * nq + (qbase - a.q0)) * k;
    int* pj = a.pidx + ((int64_t)blockIdx.y * nq + (qbase - a.q0)) * k;
    for (int e = tid; e < qrows * k; e += 256) {
        pd[e] = list_d[e / k][e % k];
        pj[e] = list_j[e / k][e % k];
    }
}

// One wave per query row: the partial lists of the `splits` splits (and the row's own entries with `accumulate`) -> dist, idx,
// rowsum.  splits may be 0 (an empty data range).
__global__ __launch_bounds__(256) void knn_merge_kernel(KnnArgs a) {
    const int lane = threadIdx.x & 63;
    const int k = a.k;
    const int64_t nq = a.q1 - a.q0;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= nq) return;                                                  // whole waves only
    double ed = INFINITY;
    int ej = -1;
    if (a.accumulate && lane < k) {
        ed = a.dist[r * k + lane];
        const int64_t j = a.idx[r * k + lane];
        ej = j < 0 ? -1 : (int)j;
    }
    for (int s = 0; s < a.splits; s++) {
        double d = 0;
        int j = -1;
        if (lane < k) {
            d = a.pdist[((int64_t)s * nq + r) * k + lane];
            j = a.pidx[((int64_t)s * nq + r) * k + lane];
        }
        knn_wave_offer(ed, ej, k, d, j, j >= 0);
    }
    if (lane < k) {
        a.dist[r * k + lane] = ej < 0 ? INFINITY : ed;
        a.idx[r * k + lane] = ej;
    }
    if (a.rowsum) {
        double sum = 0;
        for (int s = 0; s < k; s++) sum += __shfl(ej < 0 ? INFINITY : ed, s);
        if (lane == 0) a.rowsum[r] = sum;
    }
}

template <class E>
static int launch_knn_tiles(const KnnArgs& a, hipStream_t stream) {
    const int64_t nqt = (a.q1 - a.q0 + tile::T - 1) / tile::T;
    const dim3 grid((unsigned)nqt, (unsigned)a.splits);
    ITAL_LAUNCH(knn_tile_kernel<E>, grid, dim3(256), 0, stream, a);
    return ital_check_launch("ital_knn_rows");
}

static bool knn_sizes_ok(int64_t nq, int k, int splits) {
    return nq >= 0 && nq <= INT32_MAX && k >= 1 && k <= ITAL_KNN_MAX_K && splits >= 0 && splits <= ITAL_KNN_MAX_SPLITS;
}

}  // namespace ital

using namespace ital;

extern "C" size_t ital_knn_workspace(int64_t nq, int k, int splits) {
    if (!knn_sizes_ok(nq, k, splits)) return 0;
    const size_t entries = (size_t)(splits == 0 ? ITAL_KNN_AUTO_SPLITS : splits) * (size_t)nq * (size_t)k;
    return (entries * (sizeof(double) + sizeof(int)) + 15) / 16 * 16;
}

extern "C" int ital_knn_rows(const void* X, int xtype, const double* xnorm, int64_t n, int ldx, int64_t q0, int64_t q1, int64_t c0,
                             int64_t c1, int metric, int k, int skip_self, int accumulate, int splits, double* dist, int64_t* idx,
                             double* rowsum, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (n < 0 || n > INT32_MAX) return ital_fail(-22, "ital_knn_rows: the number of rows must be in [0, 2^31 - 1]");
    if (q0 < 0 || q1 < q0 || q1 > n) return ital_fail(-22, "ital_knn_rows: the query range must lie inside [0, n]");
    if (c0 < 0 || c1 < c0 || c1 > n) return ital_fail(-22, "ital_knn_rows: the data range must lie inside [0, n]");
    if (ldx <= 0 || ldx % 16 != 0) return ital_fail(-22, "ital_knn_rows: ldx must be a positive multiple of 16");
    if (rows_elem_size(xtype) == 0) return ital_fail(-22, "ital_knn_rows: unknown element type of X");
    if (metric != ITAL_KNN_COSINE && metric != ITAL_KNN_SQEUCLIDEAN) return ital_fail(-22, "ital_knn_rows: unknown metric");
    if (k < 1 || k > ITAL_KNN_MAX_K) return ital_fail(-22, "ital_knn_rows: k must be in [1, 32]");
    if (splits < 0 || splits > ITAL_KNN_MAX_SPLITS) return ital_fail(-22, "ital_knn_rows: splits must be in [0, 64]");
    const int64_t nq = q1 - q0, nc = c1 - c0;
    if (workspace_bytes < ital_knn_workspace(nq, k, splits)) return ital_fail(-22, "ital_knn_rows: the workspace is too small");
    if (nq == 0) return 0;
    if (!dist || !idx || !workspace) return ital_fail(-22, "ital_knn_rows: dist / idx / workspace must all be given");
    if (reinterpret_cast<uintptr_t>(workspace) % 8 != 0) return ital_fail(-22, "ital_knn_rows: the workspace must be aligned to 8 B");
    if (nc > 0) {
        if (!X || !xnorm) return ital_fail(-22, "ital_knn_rows: X / xnorm must be given");
        if (reinterpret_cast<uintptr_t>(X) % 16 != 0) return ital_fail(-22, "ital_knn_rows: X must be aligned to 16 B");
    }
    const int64_t nqt = (nq + tile::T - 1) / tile::T, nct = (nc + tile::T - 1) / tile::T;
    if (splits == 0 && nc > 0) {
        // as many workgroups as the device has compute units and no more: a workgroup of the k <= 32 kernel fills the LDS of one
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            return ital_fail(-5, "ital_knn_rows: cannot read the number of compute units");
        splits = (int)max((int64_t)1, min(min((int64_t)cus / nqt, nct), (int64_t)ITAL_KNN_AUTO_SPLITS));
    }
    if (nc == 0) splits = 0;
    KnnArgs a = {X, xnorm, ldx, q0, q1, c0, c1, metric, k, skip_self, accumulate, splits, dist, idx, rowsum,
                 static_cast<double*>(workspace), nullptr};
    a.pidx = reinterpret_cast<int*>(a.pdist + (int64_t)splits * nq * k);
    if (nc > 0) {
        int rc;
        switch (xtype) {
            case ITAL_INGEST_F64: rc = launch_knn_tiles<IngestF64>(a, stream); break;
            case ITAL_INGEST_F32: rc = launch_knn_tiles<IngestF32>(a, stream); break;
            case ITAL_INGEST_F16: rc = launch_knn_tiles<IngestF16>(a, stream); break;
            default: rc = launch_knn_tiles<IngestBF16>(a, stream); break;
        }
        if (rc) return rc;
    }
    ITAL_LAUNCH(knn_merge_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, stream, a);
    return ital_check_launch("ital_knn_rows");
}
