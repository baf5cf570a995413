// The complete ranking of a score vector and its evaluation on the device (include/ital_rank.h): the ranking of
// `top_results` beyond ITAL_TOPK_MAX (reference ital/retrieval_base.py:64-75) and the two metrics of the experiment loop
// (reference utils.py:174-200 `ndcg`, scikit-learn's average_precision_score; run_experiment.py:154-168).
//
// Ranking: the pair (order key of topk.hip, position) is one composite key, all of them distinct.  Tiles of 2048 pairs are
// sorted in LDS (bitonic); sorted runs are merged pairwise, one launch per doubling of the run length: a workgroup finds the
// part of the two runs that makes its 2048 outputs by a binary search along its diagonals (merge path) and merges it in LDS.
// A launch only reads what the launch before it wrote: no workgroup waits on another, no atomics.
//
// Evaluation: the known samples in rank order carry (known so far, positives so far, does a group of equal scores start
// here, positives before the last such start).  Per tile of 2048 ranks these are integer scans in LDS; the carries between
// tiles are scanned by one workgroup in a launch of its own; the floating-point sums have a shape fixed by n.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ital_internal.h"
#include "ital_rank.h"

namespace ital {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int RT = ITAL_RANK_TILE;     // pairs per tile
constexpr int RB = 256;                // threads per workgroup
constexpr int RE = RT / RB;            // consecutive pairs per thread
constexpr u64 KEY_NAN = ~0ull;

// topk.hip's order_key: ascending doubles <-> ascending keys, NaN above every number, the two zeros equal.  No number maps
// to key 0 (-inf gives 0x000fffffffffffff), which pads a tile below every real entry.
__device__ __forceinline__ u64 rank_key(double x) {
    if (x != x) return KEY_NAN;
    if (x == 0.0) return 0x8000000000000000ull;
    const u64 b = (u64)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// Does (ka, ia) stand before (kb, ib) in the ranking?
__device__ __forceinline__ bool rank_first(u64 ka, u32 ia, u64 kb, u32 ib) { return ka > kb || (ka == kb && ia > ib); }

// How many of the first d entries of the merge of the descending runs a[0..na) and b[0..nb) come from a.
__device__ __forceinline__ int64_t merge_path(const u64* ak, const u32* ai, int64_t na, const u64* bk, const u32* bi, int64_t nb,
                                              int64_t d) {
    int64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (rank_first(ak[mid], ai[mid], bk[d - 1 - mid], bi[d - 1 - mid])) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One tile of up to RT values: keys, a bitonic sort in LDS, descending by (key, position).  EMIT: the tile is the whole
// vector and the result goes out as it is; else the sorted pairs go to the workspace.
template <bool EMIT>
__global__ __launch_bounds__(RB) void rank_tile_kernel(const double* __restrict__ v, int64_t n, int64_t index_offset,
                                                       u64* __restrict__ keys, u32* __restrict__ idx,
                                                       int64_t* __restrict__ out_idx, double* __restrict__ out_vals) {
    __shared__ u64 skey[RT];
    __shared__ u32 sidx[RT];
    const int64_t base = (int64_t)blockIdx.x * RT;
    const int cnt = (int)(n - base < RT ? n - base : RT);
    int P = 1;
    while (P < cnt) P <<= 1;
    for (int i = threadIdx.x; i < P; i += RB) {
        if (i < cnt) { skey[i] = rank_key(v[base + i]); sidx[i] = (u32)(base + i); }
        else { skey[i] = 0; sidx[i] = 0xffffffffu; }       // below every real entry
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < P / 2; i += RB) {
                const int lo = 2 * i - (i & (stride - 1));
                const int hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const u64 ka = skey[lo], kb = skey[hi];
                const u32 ia = sidx[lo], ib = sidx[hi];
                if (rank_first(ka, ia, kb, ib) != desc) { skey[lo] = kb; skey[hi] = ka; sidx[lo] = ib; sidx[hi] = ia; }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < cnt; i += RB) {
        if (EMIT) {
            out_idx[base + i] = index_offset + (int64_t)sidx[i];
            if (out_vals && sidx[i] < n) out_vals[base + i] = v[sidx[i]];
        } else {
            keys[base + i] = skey[i];
            idx[base + i] = sidx[i];
        }
    }
}

// One merge pass: the sorted runs [2jL, 2jL + L) and [2jL + L, 2jL + 2L) of src (cut off at n) become one run of dst.
// Workgroup t makes the outputs [t RT, t RT + RT); L is a multiple of RT, so they belong to one pair of runs.
__global__ __launch_bounds__(RB) void rank_merge_kernel(const u64* __restrict__ src_k, const u32* __restrict__ src_i,
                                                        u64* __restrict__ dst_k, u32* __restrict__ dst_i, int64_t n, int64_t L) {
    __shared__ u64 skey[RT];
    __shared__ u32 sidx[RT];
    __shared__ int64_t cut[2];
    const int64_t out0 = (int64_t)blockIdx.x * RT;
    const int64_t base = out0 / (2 * L) * (2 * L);
    const int64_t na = n - base < L ? n - base : L;
    const int64_t rest = n - base - na;
    const int64_t nb = rest < L ? rest : L;                 // 0: a lone run, copied
    const int64_t d0 = out0 - base;
    const int64_t d1 = d0 + RT < na + nb ? d0 + RT : na + nb;
    const u64* ak = src_k + base;
    const u32* ai = src_i + base;
    const u64* bk = ak + na;
    const u32* bi = ai + na;
    if (threadIdx.x < 2) cut[threadIdx.x] = merge_path(ak, ai, na, bk, bi, nb, threadIdx.x == 0 ? d0 : d1);
    __syncthreads();
    const int64_t a0 = cut[0], b0 = d0 - a0;
    const int ca = (int)(cut[1] - a0), cb = (int)((d1 - cut[1]) - b0), cnt = ca + cb;     // cnt = d1 - d0 <= RT
    for (int i = threadIdx.x; i < cnt; i += RB) {
        if (i < ca) { skey[i] = ak[a0 + i]; sidx[i] = ai[a0 + i]; }
        else { skey[i] = bk[b0 + (i - ca)]; sidx[i] = bi[b0 + (i - ca)]; }
    }
    __syncthreads();
    const int d = (int)threadIdx.x * RE < cnt ? (int)threadIdx.x * RE : cnt;
    const int e = d + RE < cnt ? d + RE : cnt;
    int i = (int)merge_path(skey, sidx, ca, skey + ca, sidx + ca, cb, d);
    int j = d - i;
    u64 rk[RE];
    u32 ri[RE];
#pragma unroll
    for (int q = 0; q < RE; q++) {
        rk[q] = 0;
        ri[q] = 0;
        if (d + q < e) {
            const bool take_a = j >= cb || (i < ca && rank_first(skey[i], sidx[i], skey[ca + j], sidx[ca + j]));
            const int at = take_a ? i : ca + j;
            rk[q] = skey[at];
            ri[q] = sidx[at];
            if (take_a) i++; else j++;
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < RE; q++)
        if (d + q < e) { skey[d + q] = rk[q]; sidx[d + q] = ri[q]; }
    __syncthreads();
    for (int x = threadIdx.x; x < cnt; x += RB) { dst_k[out0 + x] = skey[x]; dst_i[out0 + x] = sidx[x]; }
}

__global__ __launch_bounds__(RB) void rank_emit_kernel(const double* __restrict__ v, const u32* __restrict__ idx, int64_t n,
                                                       int64_t index_offset, int64_t* __restrict__ out_idx,
                                                       double* __restrict__ out_vals) {
    const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
    if (i >= n) return;
    const u32 at = idx[i];
    out_idx[i] = index_offset + (int64_t)at;
    if (out_vals && at < n) out_vals[i] = v[at];
}

// ---------------------------------------------------------------------------------------------------------- evaluation
constexpr int EV_HDR = 8;       // int64 words of the header: known, positives, NaNs among the known, positives before the last start
constexpr int EV_SUM = 8;       // int64 words of a tile's record
constexpr int EV_CARRY = 8;     // int64 words of a tile's carry
constexpr int EV_PART = 4;      // doubles of a tile's sums

struct EvalWork {
    long long* hdr;             // [EV_HDR]
    u64* gk;                    // [tiles * RT] keys in rank order (0 for an unknown sample)
    long long* sum;             // [tiles][EV_SUM]: known, positives, NaNs, first key, last key, positives before the last start
                                //                  that the tile decides itself (-1: none)
    long long* carry;           // [tiles][EV_CARRY]: known before, positives before, is there a known sample before, its key,
                                //                    positives before the last start before the tile
    double* part;               // [tiles][EV_PART]: ap, dcg, ideal dcg
    signed char* gr;            // [tiles * RT] relevance in rank order
};

__host__ __device__ inline size_t eval_bytes(int64_t tiles) {
    return (size_t)EV_HDR * 8 + (size_t)tiles * ((size_t)RT * 8 + EV_SUM * 8 + EV_CARRY * 8 + EV_PART * 8 + RT);
}

__host__ __device__ inline EvalWork eval_carve(void* work, int64_t tiles) {
    EvalWork w;
    w.hdr = static_cast<long long*>(work);
    w.gk = reinterpret_cast<u64*>(w.hdr + EV_HDR);
    w.sum = reinterpret_cast<long long*>(w.gk + tiles * RT);
    w.carry = w.sum + tiles * EV_SUM;
    w.part = reinterpret_cast<double*>(w.carry + tiles * EV_CARRY);
    w.gr = reinterpret_cast<signed char*>(w.part + tiles * EV_PART);
    return w;
}

// Exclusive scan of one int per thread over the workgroup (sum, or maximum with `identity` below every value); *total: the
// scan over all threads.  sh: RB ints of LDS, free again on return.
template <bool MAX>
__device__ __forceinline__ int block_scan_excl(int val, int* sh, int identity, int* total) {
    const int t = threadIdx.x;
    sh[t] = val;
    __syncthreads();
    for (int off = 1; off < RB; off <<= 1) {
        const int other = t >= off ? sh[t - off] : identity;
        __syncthreads();
        const int mine = sh[t];
        sh[t] = MAX ? (mine > other ? mine : other) : mine + other;
        __syncthreads();
    }
    const int before = t > 0 ? sh[t - 1] : identity;
    *total = sh[RB - 1];
    __syncthreads();
    return before;
}

// A fixed tree over the workgroup's doubles (the same shape on every call); the sum is returned to thread 0.
__device__ __forceinline__ double block_sum(double val, double* sh) {
    const int t = threadIdx.x;
    sh[t] = val;
    __syncthreads();
    for (int off = RB / 2; off > 0; off >>= 1) {
        if (t < off) sh[t] += sh[t + off];
        __syncthreads();
    }
    const double s = sh[0];
    __syncthreads();
    return s;
}

// What both tile kernels need of a tile whose keys and relevance a thread holds for its RE consecutive ranks.
struct TileScan {
    int kex, pex;       // known samples / positives of the tile before this thread's ranks
    int prev;           // tile position of the last known sample before this thread's ranks, -1: none in the tile
    int K, P, last;     // of the whole tile: known samples, positives, position of the last known sample (-1: none)
};

__device__ __forceinline__ TileScan tile_scan(const u64 (&key)[RE], const int (&rel)[RE], u64* skey, int* sh) {
    TileScan s;
    int k = 0, p = 0, last = -1;
#pragma unroll
    for (int e = 0; e < RE; e++) {
        const int i = (int)threadIdx.x * RE + e;
        skey[i] = key[e];
        if (rel[e] != 0) { k++; last = i; }
        if (rel[e] > 0) p++;
    }
    s.kex = block_scan_excl<false>(k, sh, 0, &s.K);
    s.pex = block_scan_excl<false>(p, sh, 0, &s.P);
    s.prev = block_scan_excl<true>(last, sh, -1, &s.last);
    return s;
}

// Launch 1, one workgroup per tile of RT ranks: gathers key and relevance into rank order and writes the tile's record.
__global__ __launch_bounds__(RB) void eval_tile_kernel(const int64_t* __restrict__ order, const double* __restrict__ v,
                                                       const signed char* __restrict__ relv, int64_t n, int64_t index_offset,
                                                       void* work, int64_t tiles) {
    __shared__ u64 skey[RT];
    __shared__ int sh[RB];
    __shared__ int s_first, s_lh, s_nan;
    const EvalWork w = eval_carve(work, tiles);
    const int64_t base = (int64_t)blockIdx.x * RT;
    if (threadIdx.x == 0) { s_first = RT; s_lh = -1; s_nan = 0; }
    u64 key[RE];
    int rel[RE];
#pragma unroll
    for (int e = 0; e < RE; e++) {
        const int64_t p = base + (int64_t)threadIdx.x * RE + e;
        key[e] = 0;
        rel[e] = 0;
        if (p < n) {
            const int64_t at = order[p] - index_offset;
            if (at >= 0 && at < n) {
                rel[e] = (int)relv[at];
                if (rel[e] != 0) key[e] = rank_key(v[at]);
            }
        }
        w.gk[p] = key[e];
        w.gr[p] = (signed char)(rel[e] > 0 ? 1 : rel[e] < 0 ? -1 : 0);
    }
    const TileScan s = tile_scan(key, rel, skey, sh);      // its barriers also cover the three words initialised above
    int prev = s.prev, tp = s.pex, lh = -1, nan = 0, first = RT;
#pragma unroll
    for (int e = 0; e < RE; e++) {
        const int i = (int)threadIdx.x * RE + e;
        if (rel[e] != 0) {
            if (prev >= 0) { if (skey[prev] != key[e]) lh = tp; }     // a start the tile decides itself
            else first = i;
            if (key[e] == KEY_NAN) nan++;
            prev = i;
            if (rel[e] > 0) tp++;
        }
    }
    if (first < RT) atomicMin(&s_first, first);
    if (lh >= 0) atomicMax(&s_lh, lh);
    if (nan) atomicAdd(&s_nan, nan);
    __syncthreads();
    if (threadIdx.x == 0) {
        long long* r = w.sum + (int64_t)blockIdx.x * EV_SUM;
        r[0] = s.K;
        r[1] = s.P;
        r[2] = s_nan;
        r[3] = s.K > 0 ? (long long)skey[s_first] : 0;
        r[4] = s.K > 0 ? (long long)skey[s.last] : 0;
        r[5] = s_lh;
    }
}

// Launch 2, one workgroup: the carries of the tiles in order.  RB records at a time are staged in LDS; one thread walks them.
__global__ __launch_bounds__(RB) void eval_carry_kernel(void* work, int64_t tiles) {
    __shared__ long long rec[RB][6];
    __shared__ long long out[RB][5];
    __shared__ long long st[5];         // known, positives, is there a known sample, its key, positives before the last start
    __shared__ long long s_nan;
    const EvalWork w = eval_carve(work, tiles);
    if (threadIdx.x == 0) { st[0] = st[1] = st[2] = st[3] = st[4] = 0; s_nan = 0; }
    for (int64_t c = 0; c < tiles; c += RB) {
        const int64_t b = c + threadIdx.x;
        if (b < tiles)
            for (int q = 0; q < 6; q++) rec[threadIdx.x][q] = w.sum[b * EV_SUM + q];
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = (int)(tiles - c < RB ? tiles - c : RB);
            for (int t = 0; t < m; t++) {
                for (int q = 0; q < 5; q++) out[t][q] = st[q];
                if (rec[t][0] > 0) {
                    const bool starts = st[2] == 0 || st[3] != rec[t][3];      // the tile's first known sample starts a group
                    if (rec[t][5] >= 0) st[4] = st[1] + rec[t][5];
                    else if (starts) st[4] = st[1];
                    st[0] += rec[t][0];
                    st[1] += rec[t][1];
                    st[2] = 1;
                    st[3] = rec[t][4];
                    s_nan += rec[t][2];
                }
            }
        }
        __syncthreads();
        if (b < tiles)
            for (int q = 0; q < 5; q++) w.carry[b * EV_CARRY + q] = out[threadIdx.x][q];
        __syncthreads();
    }
    if (threadIdx.x == 0) { w.hdr[0] = st[0]; w.hdr[1] = st[1]; w.hdr[2] = s_nan; w.hdr[3] = st[4]; }
}

// Launch 3, one workgroup per tile: the summands of the tile.  A group of equal scores is closed where the next one starts:
// at a start of rank R > 1 the closed group ends at rank R - 1 with tp positives so far, tp - g of them its own, where g
// counts the positives before the start before this one.  The last group is closed by launch 4.
__global__ __launch_bounds__(RB) void eval_sum_kernel(void* work, int64_t tiles) {
    __shared__ u64 skey[RT];
    __shared__ int sh[RB];
    __shared__ double shd[RB];
    const EvalWork w = eval_carve(work, tiles);
    const int64_t base = (int64_t)blockIdx.x * RT;
    const long long* cr = w.carry + (int64_t)blockIdx.x * EV_CARRY;
    const long long known_before = cr[0], pos_before = cr[1], g_in = cr[4];
    const bool prev_valid = cr[2] != 0;
    const u64 prev_key = (u64)cr[3];
    const long long n_pos = w.hdr[1];
    u64 key[RE];
    int rel[RE];
#pragma unroll
    for (int e = 0; e < RE; e++) {
        const int64_t p = base + (int64_t)threadIdx.x * RE + e;
        key[e] = w.gk[p];
        rel[e] = (int)w.gr[p];
    }
    const TileScan s = tile_scan(key, rel, skey, sh);
    // pass 1: which of this thread's known samples start a group, and the positives (of the tile) before the last of them
    unsigned starts = 0;
    int prev = s.prev, tp = s.pex, lh = -1;
#pragma unroll
    for (int e = 0; e < RE; e++) {
        if (rel[e] != 0) {
            const bool st = prev >= 0 ? skey[prev] != key[e] : (!prev_valid || prev_key != key[e]);
            if (st) { starts |= 1u << e; lh = tp; }
            prev = (int)threadIdx.x * RE + e;
            if (rel[e] > 0) tp++;
        }
    }
    int unused;
    int g_tile = block_scan_excl<true>(lh, sh, -1, &unused);     // positives of the tile before the last start before this thread
    // pass 2
    double ap = 0.0, dcg = 0.0, ideal = 0.0;
    long long R = known_before + s.kex;
    tp = s.pex;
#pragma unroll
    for (int e = 0; e < RE; e++) {
        if (rel[e] != 0) {
            R++;
            if (starts & (1u << e)) {
                if (R > 1) {
                    const long long tpe = pos_before + tp;
                    const long long own = tpe - (g_tile >= 0 ? pos_before + g_tile : g_in);
                    if (own > 0) ap += ((double)own / (double)n_pos) * ((double)tpe / (double)(R - 1));
                }
                g_tile = tp;
            }
            if (rel[e] > 0 || R <= n_pos) {
                const double gain = 1.0 / log2((double)(R + 1));
                if (rel[e] > 0) dcg += gain;
                if (R <= n_pos) ideal += gain;
            }
            if (rel[e] > 0) tp++;
        }
    }
    const double a = block_sum(ap, shd), d = block_sum(dcg, shd), i = block_sum(ideal, shd);
    if (threadIdx.x == 0) {
        double* r = w.part + (int64_t)blockIdx.x * EV_PART;
        r[0] = a;
        r[1] = d;
        r[2] = i;
    }
}

// Launch 4, one workgroup: thread t adds the sums of the tiles t, t + RB, ... in that order, a tree adds the threads; the
// last group is closed and the record written.
__global__ __launch_bounds__(RB) void eval_finish_kernel(void* work, int64_t tiles, int64_t n, double* __restrict__ out) {
    __shared__ double shd[RB];
    const EvalWork w = eval_carve(work, tiles);
    double ap = 0.0, dcg = 0.0, ideal = 0.0;
    for (int64_t b = threadIdx.x; b < tiles; b += RB) {
        ap += w.part[b * EV_PART];
        dcg += w.part[b * EV_PART + 1];
        ideal += w.part[b * EV_PART + 2];
    }
    ap = block_sum(ap, shd);
    dcg = block_sum(dcg, shd);
    ideal = block_sum(ideal, shd);
    if (threadIdx.x == 0) {
        const long long K = w.hdr[0], P = w.hdr[1], nan = w.hdr[2], g = w.hdr[3];
        const double qnan = __longlong_as_double(0x7ff8000000000000ll);
        double ndcg = qnan;
        if (P > 0 && nan == 0) {
            const long long own = P - g;
            if (own > 0) ap += ((double)own / (double)P) * ((double)P / (double)K);
            ndcg = dcg / ideal;
        } else {
            ap = qnan;
        }
        out[ITAL_RANK_AP] = ap;
        out[ITAL_RANK_NDCG] = ndcg;
        out[ITAL_RANK_N_POS] = (double)P;
        out[ITAL_RANK_N_NEG] = (double)(K - P);
        out[ITAL_RANK_N_UNKNOWN] = (double)(n - K);
        out[ITAL_RANK_N_NAN] = (double)nan;
    }
}

}  // namespace ital

using namespace ital;

static bool rank_n_ok(int64_t n) { return n >= 1 && n < ((int64_t)1 << 31); }

extern "C" size_t ital_rank_workspace(int64_t n) {
    if (!rank_n_ok(n)) return 0;
    return ((size_t)n * 24 + 15) / 16 * 16;        // two buffers of (key, position): 2 * (8 + 4) bytes per value
}

extern "C" size_t ital_rank_eval_workspace(int64_t n) {
    if (!rank_n_ok(n)) return 0;
    return eval_bytes((n + RT - 1) / RT);
}

extern "C" int ital_rank_desc(const double* v, int64_t n, int64_t index_offset, int64_t* out_idx, double* out_vals,
                              void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (!rank_n_ok(n)) return ital_fail(-22, "ital_rank_desc: n must be in 1 .. 2^31 - 1");
    if (!v || !out_idx) return ital_fail(-22, "ital_rank_desc: v or out_idx missing");
    if (!workspace || ((uintptr_t)workspace & 7)) return ital_fail(-22, "ital_rank_desc: workspace missing or not aligned to 8 B");
    if (workspace_bytes < ital_rank_workspace(n)) return ital_fail(-22, "ital_rank_desc: workspace below ital_rank_workspace(n)");
    u64* ka = static_cast<u64*>(workspace);
    u64* kb = ka + n;
    u32* ia = reinterpret_cast<u32*>(kb + n);
    u32* ib = ia + n;
    if (n <= RT) {
        ITAL_LAUNCH(rank_tile_kernel<true>, dim3(1), dim3(RB), 0, stream, v, n, index_offset, ka, ia, out_idx, out_vals);
        return ital_check_launch("ital_rank_desc");
    }
    const unsigned tiles = (unsigned)((n + RT - 1) / RT);
    ITAL_LAUNCH(rank_tile_kernel<false>, dim3(tiles), dim3(RB), 0, stream, v, n, index_offset, ka, ia, out_idx, out_vals);
    for (int64_t L = RT; L < n; L *= 2) {
        ITAL_LAUNCH(rank_merge_kernel, dim3(tiles), dim3(RB), 0, stream, (const u64*)ka, (const u32*)ia, kb, ib, n, L);
        u64* tk = ka; ka = kb; kb = tk;
        u32* ti = ia; ia = ib; ib = ti;
    }
    ITAL_LAUNCH(rank_emit_kernel, dim3((unsigned)((n + RB - 1) / RB)), dim3(RB), 0, stream, v, (const u32*)ia, n, index_offset,
                out_idx, out_vals);
    return ital_check_launch("ital_rank_desc");
}

extern "C" int ital_rank_eval(const int64_t* order, const double* v, const signed char* rel, int64_t n, int64_t index_offset,
                              double* out, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (!rank_n_ok(n)) return ital_fail(-22, "ital_rank_eval: n must be in 1 .. 2^31 - 1");
    if (!order || !v || !rel || !out) return ital_fail(-22, "ital_rank_eval: order, v, rel or out missing");
    if (!workspace || ((uintptr_t)workspace & 7)) return ital_fail(-22, "ital_rank_eval: workspace missing or not aligned to 8 B");
    if (workspace_bytes < ital_rank_eval_workspace(n))
        return ital_fail(-22, "ital_rank_eval: workspace below ital_rank_eval_workspace(n)");
    const int64_t tiles = (n + RT - 1) / RT;
    ITAL_LAUNCH(eval_tile_kernel, dim3((unsigned)tiles), dim3(RB), 0, stream, order, v, rel, n, index_offset, workspace, tiles);
    ITAL_LAUNCH(eval_carry_kernel, dim3(1), dim3(RB), 0, stream, workspace, tiles);
    ITAL_LAUNCH(eval_sum_kernel, dim3((unsigned)tiles), dim3(RB), 0, stream, workspace, tiles);
    ITAL_LAUNCH(eval_finish_kernel, dim3(1), dim3(RB), 0, stream, workspace, tiles, n, out);
    return ital_check_launch("ital_rank_eval");
}
