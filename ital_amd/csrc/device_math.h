// Device-side scalar math for the ITAL hot path on gfx950 (fp64 throughout).
//
// Phi / Phi^-1 / bivariate-normal routines follow the published algorithms that SciPy's
// `mvndst` (A. Genz) is built from, because the reference's orthant probabilities are defined by
// them (reference ital/ital.py:380-381 -> scipy.stats.mvn.mvndst):
//   mvn_phi   : Hart et al. algorithm 5666 (rational, |z| < 10/sqrt2; continued fraction beyond)
//   mvn_phinv : Wichura AS241 PPND16
//   mvn_bvu   : Genz BVU, Gauss-Legendre 6/12/20 point rules
//   ndtr      : erfc form of the normal cdf used by scipy.stats.norm.cdf (ital.py:367-369)
#pragma once
#include <hip/hip_runtime.h>

namespace ital {

// Horner step acc * x + K.  Spelling the instruction out by inline asm was measured and rejected on MI355X: with K in a
// scalar register pair the scalar unit becomes the co-bottleneck (two s_mov_b32 per step), with K in a vector register
// pair the register file spills; the compiler's v_fmac + v_mov_b64 form (coefficients parked in VGPRs) is the fastest.
__device__ __forceinline__ double fma_k(double acc, double x, double K) { return fma(acc, x, K); }

// n / d for well-scaled d (polynomial denominators, no zero / inf / subnormal): hardware reciprocal seed, one Newton
// step and one residual correction -- ~1 ulp, about half the instructions of the IEEE division expansion.
// Cost on MI355X (tools/ubench/inst_rate.hip, per wave-instruction and SIMD): the seed 7.0 ns, as much as 3.5 simple
// instructions, the five that follow 2.0 - 2.4 ns each -- about 18 ns per quotient, 7 of them the seed.  Chains that divide
// at the same point of the program share the seed: fast_div_group below.
__device__ __forceinline__ double fast_div(double n, double d) {
    // v_rcp_f64 is good to ~2^-23; one Newton step on the reciprocal (2^-46), then the residual correction of the quotient
    // squares the error once more: <= 1 ulp without a second step on the reciprocal
    double r = __builtin_amdgcn_rcp(d);
#ifdef ITAL_DIV_TWO_STEPS
    r = fma(fma(-d, r, 1.0), r, r);
#endif
    r = fma(fma(-d, r, 1.0), r, r);
    double q = n * r;
    return fma(fma(-d, q, n), r, q);
}

// n[k] / d[k] for the first `len` of GM independent pairs with ONE reciprocal seed: v_rcp_f64 is the most expensive
// instruction of fast_div (7.0 ns against 2.0 - 2.4 ns for a multiplication or an FMA on MI355X), and chains that divide at
// the same point of the program can share it -- prefix products of the denominators, the seed and its Newton step on the
// product of all, then each reciprocal by back-substitution: 3 (len - 1) multiplications instead of len - 1 seeds and
// 2 (len - 1) FMAs.  The recovered reciprocals carry the Newton step's 2^-46 plus a few roundings; the residual correction
// per quotient is fast_div's own and squares that error, so the quotients are fast_div's (checked over 1.2e7 random pairs
// per range by tools/batch_div_check.cpp: equal in every case, both within 0.5 ulp of the long-double quotient).
// The product must stay in range: here at most six factors from [0.0022, 1.5e10].  A non-finite or zero denominator
// reaches every quotient of its group, so a group holds only chains whose values are added up together anyway.
// len, GM: compile-time constants after unrolling; len == 1 is fast_div itself.
template <int GM>
__device__ __forceinline__ void fast_div_group(const double (&n)[GM], const double (&d)[GM], double (&out)[GM], int len) {
    if (len == 1) {
        out[0] = fast_div(n[0], d[0]);
        return;
    }
    double pre[GM], r[GM];
    pre[0] = d[0];
#pragma unroll
    for (int k = 1; k < GM; k++)
        if (k < len) pre[k] = pre[k - 1] * d[k];
    const double dall = pre[len - 1];
    double ra = __builtin_amdgcn_rcp(dall);
#ifdef ITAL_DIV_TWO_STEPS
    ra = fma(fma(-dall, ra, 1.0), ra, ra);
#endif
    ra = fma(fma(-dall, ra, 1.0), ra, ra);
#pragma unroll
    for (int k = GM - 1; k >= 1; k--)
        if (k < len) {
            r[k] = ra * pre[k - 1];     // 1 / d[k] = (1 / (d[0] .. d[k])) (d[0] .. d[k-1])
            ra = ra * d[k];             // 1 / (d[0] .. d[k-1])
        }
    r[0] = ra;
#pragma unroll
    for (int k = 0; k < GM; k++)
        if (k < len) {
            const double q = n[k] * r[k];
            out[k] = fma(fma(-d[k], q, n[k]), r[k], q);
        }
}

// N independent quotients in groups of G (the last group takes what is left); G <= 1: N times fast_div.
template <int N, int G>
__device__ __forceinline__ void fast_div_batch(const double (&n)[N], const double (&d)[N], double (&out)[N]) {
    constexpr int GM = G > 1 ? G : 1;
#pragma unroll
    for (int g0 = 0; g0 < N; g0 += GM) {
        double gn[GM], gd[GM], go[GM];
        const int len = N - g0 < GM ? N - g0 : GM;
#pragma unroll
        for (int k = 0; k < GM; k++)
            if (k < len) { gn[k] = n[g0 + k]; gd[k] = d[g0 + k]; }
        fast_div_group<GM>(gn, gd, go, len);
#pragma unroll
        for (int k = 0; k < GM; k++)
            if (k < len) out[g0 + k] = go[k];
    }
}

// Polynomial coefficients as operands.  With literals (LitK) the compiler materialises every coefficient next to its use:
// in a loop that already fills the scalar register file it parks them in vector registers and emits `v_mov_b64 acc, K;
// v_fmac_f64 acc, p, r` per Horner step -- the copy is a full-rate FP64 issue slot, 12 % of the lattice loop's vector
// instructions.  HotK holds the coefficients of exp and log as opaque vector-register values instead: the steps become
// three-operand `v_fma_f64 p, p, r, K` with no copy (same 20 + 18 registers the parked literals took).
struct LitK {};
// A literal that is materialised WHERE IT IS USED, in a scalar register pair (two s_mov_b32 next to the consumer, which takes
// it as its one scalar operand).  For coefficients of rarely executed branches inside hot loops -- the log / sqrt tail of
// Phi^-1 runs once per stage and wave: left to itself the compiler treats its 39 coefficients as loop invariants, finds the
// scalar file full and parks them in 78 vector registers for the whole kernel (and copies each into the accumulator of a
// two-address v_fmac: 27 v_mov_b64 per pass).
__device__ __forceinline__ double lit_s(double k) { asm volatile("" : "+s"(k)); return k; }
__device__ __forceinline__ double opaque_v(double k) { asm volatile("" : "+v"(k)); return k; }
struct HotK {
    double e[10];   // exp_neg: q(r) of exp(r) = 1 + r + r^2 q(r)
    double l[9];    // log_pos: odd atanh series 2/19 .. 2/3
    __device__ __forceinline__ void load() {
        e[0] = opaque_v(2.5100375832561321544e-8); e[1] = opaque_v(2.7620075879983480862e-7);
        e[2] = opaque_v(2.7557268480310025341e-6); e[3] = opaque_v(0.000024801521322368693026);
        e[4] = opaque_v(0.00019841269863040545271); e[5] = opaque_v(0.0013888888917196719077);
        e[6] = opaque_v(0.0083333333333300644495); e[7] = opaque_v(0.041666666666624161903);
        e[8] = opaque_v(0.16666666666666667452); e[9] = opaque_v(0.50000000000000010211);
#pragma unroll
        for (int i = 0; i < 9; i++) l[i] = opaque_v(2.0 / (19 - 2 * i));
    }
};

// Only the exp coefficients as register operands (every chain evaluates exp once per stage; the logarithm only runs in the
// compacted tail branch of Phi^-1, once per stage and wave): 18 vector registers less than HotK.
struct HotKE {
    double e[10];
    __device__ __forceinline__ void load() {
        e[0] = opaque_v(2.5100375832561321544e-8); e[1] = opaque_v(2.7620075879983480862e-7);
        e[2] = opaque_v(2.7557268480310025341e-6); e[3] = opaque_v(0.000024801521322368693026);
        e[4] = opaque_v(0.00019841269863040545271); e[5] = opaque_v(0.0013888888917196719077);
        e[6] = opaque_v(0.0083333333333300644495); e[7] = opaque_v(0.041666666666624161903);
        e[8] = opaque_v(0.16666666666666667452); e[9] = opaque_v(0.50000000000000010211);
    }
};

// Six of the ten exp coefficients as register operands, the other four materialised in place (lit_s): 8 vector registers
// less than HotKE for 8 scalar moves per evaluation -- what lets the t = 8 lattice sums fit three waves per SIMD without scratch.
struct HotKE6 {
    double e[6];
    __device__ __forceinline__ void load() {
        e[0] = opaque_v(2.5100375832561321544e-8); e[1] = opaque_v(2.7620075879983480862e-7);
        e[2] = opaque_v(2.7557268480310025341e-6); e[3] = opaque_v(0.000024801521322368693026);
        e[4] = opaque_v(0.00019841269863040545271); e[5] = opaque_v(0.0013888888917196719077);
    }
};

// N of the ten exp coefficients (the leading ones) as register operands, the rest in place: where HotKE6 still spills.
template <int N>
struct HotKEn {
    double e[N > 0 ? N : 1];
    __device__ __forceinline__ void load() {
        const double c[10] = {2.5100375832561321544e-8, 2.7620075879983480862e-7, 2.7557268480310025341e-6,
                              0.000024801521322368693026, 0.00019841269863040545271, 0.0013888888917196719077,
                              0.0083333333333300644495, 0.041666666666624161903, 0.16666666666666667452,
                              0.50000000000000010211};
#pragma unroll
        for (int i = 0; i < N; i++) e[i] = opaque_v(c[i]);
    }
};

// The same coefficients as opaque SCALAR-register values: for the kernels that read their factor from LDS (T >= 7 of
// the perfect-user scorer) the scalar file has room for them, and the 38 vector registers go to the chains instead
// (one scalar operand per v_fma_f64 is what gfx9 encodes).
__device__ __forceinline__ double opaque_s(double k) { asm volatile("" : "+s"(k)); return k; }
struct HotKS {
    double e[10], l[9];
    __device__ __forceinline__ void load() {
        e[0] = opaque_s(2.5100375832561321544e-8); e[1] = opaque_s(2.7620075879983480862e-7);
        e[2] = opaque_s(2.7557268480310025341e-6); e[3] = opaque_s(0.000024801521322368693026);
        e[4] = opaque_s(0.00019841269863040545271); e[5] = opaque_s(0.0013888888917196719077);
        e[6] = opaque_s(0.0083333333333300644495); e[7] = opaque_s(0.041666666666624161903);
        e[8] = opaque_s(0.16666666666666667452); e[9] = opaque_s(0.50000000000000010211);
#pragma unroll
        for (int i = 0; i < 9; i++) l[i] = opaque_s(2.0 / (19 - 2 * i));
    }
};

// exp(x) for x in [-745, 0]: Cody-Waite reduction by ln2, degree-13 Taylor polynomial on |r| <= ln2/2 (relative error
// < 1e-16), scaling by v_ldexp_f64.  19 VALU instructions against ~42 for the general-purpose library routine.
__device__ __forceinline__ double exp_neg(double x) {
    const double LOG2E = 1.4426950408889634074, LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    const double n = rint(x * LOG2E);
    double r = fma(-n, LN2_HI, x);
    r = fma(-n, LN2_LO, r);
#ifdef ITAL_EXP_TAYLOR13
    double p = 1.0 / 6227020800.0;
    p = fma_k(p, r, 1.0 / 479001600.0);
    p = fma_k(p, r, 1.0 / 39916800.0);
    p = fma_k(p, r, 1.0 / 3628800.0);
    p = fma_k(p, r, 1.0 / 362880.0);
    p = fma_k(p, r, 1.0 / 40320.0);
    p = fma_k(p, r, 1.0 / 5040.0);
    p = fma_k(p, r, 1.0 / 720.0);
    p = fma_k(p, r, 1.0 / 120.0);
    p = fma_k(p, r, 1.0 / 24.0);
    p = fma_k(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
#else
    // exp(r) = 1 + r + r^2 q(r), q of degree 9 fitted on |r| <= ln2/2 (Chebyshev fit, error 1.8e-17 relative to exp)
    double p = 2.5100375832561321544e-8;
    p = fma_k(p, r, 2.7620075879983480862e-7);
    p = fma_k(p, r, 2.7557268480310025341e-6);
    p = fma_k(p, r, 0.000024801521322368693026);
    p = fma_k(p, r, 0.00019841269863040545271);
    p = fma_k(p, r, 0.0013888888917196719077);
    p = fma_k(p, r, 0.0083333333333300644495);
    p = fma_k(p, r, 0.041666666666624161903);
    p = fma_k(p, r, 0.16666666666666667452);
    p = fma_k(p, r, 0.50000000000000010211);
#endif
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}

__device__ __forceinline__ double exp_neg(double x, const LitK&) { return exp_neg(x); }
template <class KT>
__device__ __forceinline__ double exp_neg(double x, const KT& k) {
    const double LOG2E = 1.4426950408889634074, LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    const double n = rint(x * LOG2E);
    double r = fma(-n, LN2_HI, x);
    r = fma(-n, LN2_LO, r);
    double p = k.e[0];
#pragma unroll
    for (int i = 1; i < 10; i++) p = fma(p, r, k.e[i]);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}

__device__ __forceinline__ double exp_neg(double x, const HotKE6& k) {
    const double LOG2E = 1.4426950408889634074, LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    const double n = rint(x * LOG2E);
    double r = fma(-n, LN2_HI, x);
    r = fma(-n, LN2_LO, r);
    double p = k.e[0];
#pragma unroll
    for (int i = 1; i < 6; i++) p = fma(p, r, k.e[i]);
    p = fma(p, r, lit_s(0.0083333333333300644495));
    p = fma(p, r, lit_s(0.041666666666624161903));
    p = fma(p, r, lit_s(0.16666666666666667452));
    p = fma(p, r, lit_s(0.50000000000000010211));
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}

template <int N>
__device__ __forceinline__ double exp_neg(double x, const HotKEn<N>& k) {
    const double LOG2E = 1.4426950408889634074, LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    const double c[10] = {2.5100375832561321544e-8, 2.7620075879983480862e-7, 2.7557268480310025341e-6,
                          0.000024801521322368693026, 0.00019841269863040545271, 0.0013888888917196719077,
                          0.0083333333333300644495, 0.041666666666624161903, 0.16666666666666667452,
                          0.50000000000000010211};
    const double n = rint(x * LOG2E);
    double r = fma(-n, LN2_HI, x);
    r = fma(-n, LN2_LO, r);
    double p = N > 0 ? k.e[0] : lit_s(c[0]);
#pragma unroll
    for (int i = 1; i < 10; i++) p = fma(p, r, i < N ? k.e[i < N ? i : 0] : lit_s(c[i]));
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}

// log(x) for finite x > 0: x = 2^e * m, m in [sqrt(1/2), sqrt(2)), log m = 2 atanh(s), s = (m-1)/(m+1), odd series to s^19
// (|s| <= 0.1716: truncation < 3e-17 relative).  ~30 VALU instructions against ~98 for the library routine.
__device__ __forceinline__ double log_pos(double x) {
    const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    int e = __builtin_amdgcn_frexp_exp(x);
    double m = __builtin_amdgcn_frexp_mant(x);  // [0.5, 1)
    const bool lowm = m < 0.70710678118654752440;
    m = lowm ? m + m : m;
    e = lowm ? e - 1 : e;
    const double f = m - 1.0;
    const double s = fast_div(f, 2.0 + f);
    const double z = s * s;
    double p = 2.0 / 19.0;
    p = fma_k(p, z, 2.0 / 17.0);
    p = fma_k(p, z, 2.0 / 15.0);
    p = fma_k(p, z, 2.0 / 13.0);
    p = fma_k(p, z, 2.0 / 11.0);
    p = fma_k(p, z, 2.0 / 9.0);
    p = fma_k(p, z, 2.0 / 7.0);
    p = fma_k(p, z, 2.0 / 5.0);
    p = fma_k(p, z, 2.0 / 3.0);
    const double lm = fma(s * z, p, s + s);
    const double de = (double)e;
    return fma(de, LN2_HI, fma(de, LN2_LO, lm));
}

__device__ __forceinline__ double log_pos(double x, const LitK&) { return log_pos(x); }
__device__ __forceinline__ double log_pos(double x, const HotKE&) { return log_pos(x); }
__device__ __forceinline__ double log_pos(double x, const HotKE6&) { return log_pos(x); }
template <int N>
__device__ __forceinline__ double log_pos(double x, const HotKEn<N>&) { return log_pos(x); }
template <class KT>
__device__ __forceinline__ double log_pos(double x, const KT& k) {
    const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    int e = __builtin_amdgcn_frexp_exp(x);
    double m = __builtin_amdgcn_frexp_mant(x);  // [0.5, 1)
    const bool lowm = m < 0.70710678118654752440;
    m = lowm ? m + m : m;
    e = lowm ? e - 1 : e;
    const double f = m - 1.0;
    const double s = fast_div(f, 2.0 + f);
    const double z = s * s;
    double p = k.l[0];
#pragma unroll
    for (int i = 1; i < 9; i++) p = fma(p, z, k.l[i]);
    const double lm = fma(s * z, p, s + s);
    const double de = (double)e;
    return fma(de, LN2_HI, fma(de, LN2_LO, lm));
}

// sqrt(a) for a in a normal, well-scaled range (here [1e-3, 1e3]): reciprocal-square-root seed (~2^-23), one Goldschmidt step (2^-46)
// and a final residual correction that squares the error again (~1 ulp).
__device__ __forceinline__ double sqrt_pos(double a) {
    double y = __builtin_amdgcn_rsq(a);
    double g = a * y, h = 0.5 * y;
    double r = fma(-h, g, 0.5);
    g = fma(g, r, g);
    h = fma(h, r, h);
#ifdef ITAL_SQRT_TWO_STEPS
    r = fma(-h, g, 0.5);
    g = fma(g, r, g);
    h = fma(h, r, h);
#endif
    const double d = fma(-g, g, a);
    return fma(d, h, g);
}

// MVNPHI (Hart 5666).  The far-tail continued fraction z + 1/(z + 2/(z + 3/(z + 4/(z + 0.65)))) is evaluated as the
// ratio of its convergents' numerators N1/N2 (one division instead of six).
//
// CF = false (the lattice loops, mvn_phi_lat below): the rational on the whole range |z| <= 37.  MVNPHI itself is a 1e-9
// RELATIVE approximation out there (vs the exact tail: rational +2.9e-9 at the cut-off 7.07, its continued fraction -3.6e-9,
// -8.7e-9 at 8); beyond the cut-off the rational drifts to +4e-8 at |z| = 10, +3.5e-6 at 37 -- on values below 7.7e-13, an
// absolute difference to MVNPHI below 5e-21 (Phi(z) for z > 0 is 1 - p: unchanged to the last bit).  The reference adds
// eps = 1e-12 to every probability before its logarithms (ital.py:208-222).  In a wave of 64 chains some |z| lies beyond
// the cut-off often enough that the branch cost 3.5 % (t = 4) to 4.6 % (t = 8) of the lattice sums.
// Hart's rational P(|z|) / Q(|z|) as numerator and denominator (Q in [440, 1.42e10] on |z| <= 37).
__device__ __forceinline__ void hart_pq(double zabs, double& num, double& den) {
    const double P0 = 220.2068679123761, P1 = 221.2135961699311, P2 = 112.0792914978709, P3 = 33.91286607838300,
                 P4 = 6.373962203531650, P5 = .7003830644436881, P6 = .03526249659989109;
    const double Q0 = 440.4137358247522, Q1 = 793.8265125199484, Q2 = 637.3336333788311, Q3 = 296.5642487796737,
                 Q4 = 86.78073220294608, Q5 = 16.06417757920695, Q6 = 1.755667163182642, Q7 = .08838834764831844;
    num = fma_k(fma_k(fma_k(fma_k(fma_k(fma_k(P6, zabs, P5), zabs, P4), zabs, P3), zabs, P2), zabs, P1), zabs, P0);
    den = fma_k(fma_k(fma_k(fma_k(fma_k(fma_k(fma_k(Q7, zabs, Q6), zabs, Q5), zabs, Q4), zabs, Q3), zabs, Q2), zabs, Q1), zabs, Q0);
}

template <class K, bool CF = true>
__device__ __forceinline__ double mvn_phi(double z, const K& kk) {
    const double ROOTPI = 2.506628274631001, CUTOFF = 7.071067811865475;
    const double zabs = fabs(z);
    double p;
    if (zabs > 37.0) {
        p = 0.0;
    } else {
        const double expntl = exp_neg(-zabs * zabs / 2, kk);
        if (!CF || zabs < CUTOFF) {
            double num, den;
            hart_pq(zabs, num, den);
            p = fast_div(expntl * num, den);
        } else {
            const double n5 = zabs + 0.65;
            const double n4 = fma(zabs, n5, 4.0);
            const double n3 = fma(zabs, n4, 3.0 * n5);
            const double n2 = fma(zabs, n3, 2.0 * n4);
            const double n1 = fma(zabs, n2, n3);
            p = fast_div(expntl * n2, n1 * ROOTPI);
        }
    }
    if (z > 0) p = 1 - p;
    return p;
}

__device__ __forceinline__ double mvn_phi(double z) { return mvn_phi(z, LitK()); }

#ifndef ITAL_LATTICE_PHI_CF
#define ITAL_LATTICE_PHI_CF 0
#endif
template <class K>
__device__ __forceinline__ double mvn_phi_lat(double z, const K& kk) { return mvn_phi<K, ITAL_LATTICE_PHI_CF != 0>(z, kk); }
// A coefficient policy marked "MVNPHI as published, continued fraction beyond |z| = 7.07": the lattice loops instantiated with
// WithCF<K> take the far-tail branch.  Needed where a tiny orthant probability enters an objective with a weight of order 1:
// with a change-estimation subset the reference weighs log(p_U + eps) -- the joint probability over subset + batch +
// candidate -- with the probability of the enumerated variables alone (ital.py:227-275).  For a candidate that nearly
// duplicates a subset member p_U is ~1e-10 .. 1e-12, a product with a far-tail Phi among its factors, and the rational's
// 1e-8 .. 1e-6 RELATIVE drift out there reaches the score (golden iris_ce5, candidate 97: 6e-8 at step 2, 1.6e-5 at step 4).
// Everywhere else a probability is weighted by itself and the absolute 5e-21 is all that matters.
template <class K>
struct WithCF : K {};
template <class K>
__device__ __forceinline__ double mvn_phi_lat(double z, const WithCF<K>& kk) { return mvn_phi<K, true>(z, static_cast<const K&>(kk)); }

// mvn_phi's rational form (CF = false) split around its division, for chains that share a reciprocal seed (fast_div_group):
// with q = n / d formed by fast_div's arithmetic, mvn_phi_finish(z, q) is mvn_phi(z) bit for bit.
// The denominator is Q(min(|z|, 37)): the same value on |z| <= 37, and finite -- Q(37) = 1.42e10 -- for every other z, a NaN
// included, so that no chain can spoil the product its group takes the seed of.  The numerator keeps |z| itself: beyond 37 it
// may be anything (the quotient is replaced by 0, as in mvn_phi), and a NaN z still gives a NaN Phi -- its own, not its
// neighbours'.  One v_min_f64 per chain.  (Measured and rejected, docs/HISTORY.md: numerator 0 over denominator 1 chosen by
// selects, and a wave-uniform branch to the unbatched form where any |z| > 37 -- both cost more than the seeds they save.)
template <class K>
__device__ __forceinline__ void mvn_phi_nd(double z, const K& kk, double& n, double& d) {
    const double zabs = fabs(z);
    const double expntl = exp_neg(-zabs * zabs / 2, kk);
    double num, unused;
    hart_pq(zabs, num, unused);
    hart_pq(fmin(zabs, 37.0), unused, d);
    n = expntl * num;
}
__device__ __forceinline__ double mvn_phi_finish(double z, double q) {
    const double p = fabs(z) > 37.0 ? 0.0 : q;
    return z > 0 ? 1 - p : p;
}

#ifndef ITAL_TAIL_LIT_S
#define ITAL_TAIL_LIT_S 1     // coefficients of the Phi^-1 tail branch as in-place scalars (lit_s above)
#endif
#if ITAL_TAIL_LIT_S
#define TK(x) lit_s(x)
#else
#define TK(x) (x)
#endif

// PHINV (Wichura AS241 PPND16), split so that a wave can run the cheap central branch on every lane and the
// log/sqrt tail branch only on the (compacted) lanes that need it.
__device__ __forceinline__ bool phinv_is_central(double p) { return fabs(p - 0.5) <= 0.425; }

// central branch on q = p - 1/2 (bit-identical to AS241's (2p - 1)/2: doubling and halving are exact)
// (numerator and denominator: phinv_central_q(q) = fast_div(n, d).  d lies in [1, 94] on |q| <= 0.425, and in [0.0022, 1]
// -- never zero -- for the tail arguments 0.425 < |q| <= 0.5 whose quotient is discarded)
__device__ __forceinline__ void phinv_central_nd(double q, double& n, double& d) {
    const double A0 = 3.3871328727963666080E0, A1 = 1.3314166789178437745E+2, A2 = 1.9715909503065514427E+3,
                 A3 = 1.3731693765509461125E+4, A4 = 4.5921953931549871457E+4, A5 = 6.7265770927008700853E+4,
                 A6 = 3.3430575583588128105E+4, A7 = 2.5090809287301226727E+3, B1 = 4.2313330701600911252E+1,
                 B2 = 6.8718700749205790830E+2, B3 = 5.3941960214247511077E+3, B4 = 2.1213794301586595867E+4,
                 B5 = 3.9307895800092710610E+4, B6 = 2.8729085735721942674E+4, B7 = 5.2264952788528545610E+3;
    const double r = 0.180625 - q * q;
    const double num = fma_k(fma_k(fma_k(fma_k(fma_k(fma_k(fma_k(A7, r, A6), r, A5), r, A4), r, A3), r, A2), r, A1), r, A0);
    d = fma(fma_k(fma_k(fma_k(fma_k(fma_k(fma_k(B7, r, B6), r, B5), r, B4), r, B3), r, B2), r, B1), r, 1.0);
    n = q * num;
}

__device__ __forceinline__ double phinv_central_q(double q) {
    double n, d;
    phinv_central_nd(q, n, d);
    return fast_div(n, d);
}

__device__ __forceinline__ double phinv_central(double p) { return phinv_central_q(p - 0.5); }

// log(x) for the tail branch: the coefficients as in-place scalars (lit_s), whatever the caller's coefficient policy
__device__ __forceinline__ double log_pos_tail(double x) {
    const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    int e = __builtin_amdgcn_frexp_exp(x);
    double m = __builtin_amdgcn_frexp_mant(x);  // [0.5, 1)
    const bool lowm = m < 0.70710678118654752440;
    m = lowm ? m + m : m;
    e = lowm ? e - 1 : e;
    const double f = m - 1.0;
    const double s = fast_div(f, 2.0 + f);
    const double z = s * s;
    double p = lit_s(2.0 / 19.0);
    p = fma(p, z, lit_s(2.0 / 17.0));
    p = fma(p, z, lit_s(2.0 / 15.0));
    p = fma(p, z, lit_s(2.0 / 13.0));
    p = fma(p, z, lit_s(2.0 / 11.0));
    p = fma(p, z, lit_s(2.0 / 9.0));
    p = fma(p, z, lit_s(2.0 / 7.0));
    p = fma(p, z, lit_s(2.0 / 5.0));
    p = fma(p, z, lit_s(2.0 / 3.0));
    const double lm = fma(s * z, p, s + s);
    const double de = (double)e;
    return fma(de, LN2_HI, fma(de, LN2_LO, lm));
}

template <class K>
__device__ __forceinline__ double phinv_tail(double p, const K& kk) {
    const double q = p - 0.5;
    double r = fmin(p, 1 - p);
    double v;
    if (r > 0) {
#if ITAL_TAIL_LIT_S
        r = sqrt_pos(-log_pos_tail(r));
#else
        r = sqrt_pos(-log_pos(r, kk));
#endif
        if (r <= 5.0) {
            const double C0 = 1.42343711074968357734E0, C1 = 4.63033784615654529590E0, C2 = 5.76949722146069140550E0,
                         C3 = 3.64784832476320460504E0, C4 = 1.27045825245236838258E0, C5 = 2.41780725177450611770E-1,
                         C6 = 2.27238449892691845833E-2, C7 = 7.74545014278341407640E-4, D1 = 2.05319162663775882187E0,
                         D2 = 1.67638483018380384940E0, D3 = 6.89767334985100004550E-1, D4 = 1.48103976427480074590E-1,
                         D5 = 1.51986665636164571966E-2, D6 = 5.47593808499534494600E-4, D7 = 1.05075007164441684324E-9;
            r = r - 1.6;
            v = fast_div(fma_k(fma_k(fma_k(fma_k(fma_k(fma_k(fma_k(TK(C7), r, TK(C6)), r, TK(C5)), r, TK(C4)), r, TK(C3)), r, TK(C2)), r, TK(C1)), r, TK(C0)),
                         fma(fma_k(fma_k(fma_k(fma_k(fma_k(fma_k(TK(D7), r, TK(D6)), r, TK(D5)), r, TK(D4)), r, TK(D3)), r, TK(D2)), r, TK(D1)), r, 1.0));
        } else {
            const double E0 = 6.65790464350110377720E0, E1 = 5.46378491116411436990E0, E2 = 1.78482653991729133580E0,
                         E3 = 2.96560571828504891230E-1, E4 = 2.65321895265761230930E-2, E5 = 1.24266094738807843860E-3,
                         E6 = 2.71155556874348757815E-5, E7 = 2.01033439929228813265E-7, F1 = 5.99832206555887937690E-1,
                         F2 = 1.36929880922735805310E-1, F3 = 1.48753612908506148525E-2, F4 = 7.86869131145613259100E-4,
                         F5 = 1.84631831751005468180E-5, F6 = 1.42151175831644588870E-7, F7 = 2.04426310338993978564E-15;
            r = r - 5.0;
            v = fast_div(fma_k(fma_k(fma_k(fma_k(fma_k(fma_k(fma_k(TK(E7), r, TK(E6)), r, TK(E5)), r, TK(E4)), r, TK(E3)), r, TK(E2)), r, TK(E1)), r, TK(E0)),
                         fma(fma_k(fma_k(fma_k(fma_k(fma_k(fma_k(TK(F7), r, TK(F6)), r, TK(F5)), r, TK(F4)), r, TK(F3)), r, TK(F2)), r, TK(F1)), r, 1.0));
        }
    } else {
        v = 9;
    }
    return q < 0 ? -v : v;
}

__device__ __forceinline__ double phinv_tail(double p) { return phinv_tail(p, LitK()); }

__device__ __forceinline__ double mvn_phinv(double p) {
    return phinv_is_central(p) ? phinv_central(p) : phinv_tail(p);
}

// scipy.special.ndtr (Cephes): the function behind scipy.stats.norm.cdf.
__device__ __forceinline__ double ndtr(double a) {
    const double SQRTH = 7.07106781186547524401E-1;
    if (isnan(a)) return a;
    double x = a * SQRTH;
    double z = fabs(x);
    double y;
    if (z < SQRTH) {
        y = 0.5 + 0.5 * erf(x);
    } else {
        y = 0.5 * erfc(z);
        if (x > 0) y = 1.0 - y;
    }
    return y;
}

// norm.cdf(0, mean, sd): NaN unless sd > 0 (scipy's scale check).
__device__ __forceinline__ double norm_cdf0(double mean, double sd) {
    if (!(sd > 0)) return __builtin_nan("");
    return ndtr((0.0 - mean) / sd);
}

// Gauss-Legendre nodes / weights of Genz's BVU (constant memory: indexed at run time).
__constant__ const double BVU_W6[3] = {0.1713244923791705, 0.3607615730481384, 0.4679139345726904};
__constant__ const double BVU_X6[3] = {-0.9324695142031522, -0.6612093864662647, -0.2386191860831970};
__constant__ const double BVU_W12[6] = {0.4717533638651177e-01, 0.1069393259953183, 0.1600783285433464,
                       0.2031674267230659, 0.2334925365383547, 0.2491470458134029};
__constant__ const double BVU_X12[6] = {-0.9815606342467191, -0.9041172563704750, -0.7699026741943050,
                       -0.5873179542866171, -0.3678314989981802, -0.1252334085114692};
__constant__ const double BVU_W20[10] = {0.1761400713915212e-01, 0.4060142980038694e-01, 0.6267204833410906e-01,
                        0.8327674157670475e-01, 0.1019301198172404, 0.1181945319615184, 0.1316886384491766,
                        0.1420961093183821, 0.1491729864726037, 0.1527533871307259};
__constant__ const double BVU_X20[10] = {-0.9931285991850949, -0.9639719272779138, -0.9122344282513259, -0.8391169718222188,
                        -0.7463319064601508, -0.6360536807265150, -0.5108670019508271, -0.3737060887154196,
                        -0.2277858511416451, -0.7652652113349733e-01};

// sin(x) for |x| <= pi/2 (the arguments of Genz's BVU: asin(r) times a Gauss-Legendre node in (0, 1)): the odd Taylor
// polynomial through x^23 (truncation 1e-18 at pi/2), Horner in x^2 -- 13 fused operations, no argument reduction, no
// tables.  The library routine carries its large-argument reduction along: inlined into a kernel it is what fills the
// scalar register file (score_t2_kernel: 72 spilled SGPRs with it).
#ifndef ITAL_BVU_OWN_MATH
#define ITAL_BVU_OWN_MATH 1
#endif
__device__ __forceinline__ double sin_halfpi(double x) {
    const double z = x * x;
    double p = -1.0 / 25852016738884976640000.0;          // -1/23!
    p = fma(p, z, 1.0 / 51090942171709440000.0);           //  1/21!
    p = fma(p, z, -1.0 / 121645100408832000.0);            // -1/19!
    p = fma(p, z, 1.0 / 355687428096000.0);                //  1/17!
    p = fma(p, z, -1.0 / 1307674368000.0);                 // -1/15!
    p = fma(p, z, 1.0 / 6227020800.0);                     //  1/13!
    p = fma(p, z, -1.0 / 39916800.0);                      // -1/11!
    p = fma(p, z, 1.0 / 362880.0);                         //  1/9!
    p = fma(p, z, -1.0 / 5040.0);                          // -1/7!
    p = fma(p, z, 1.0 / 120.0);                            //  1/5!
    p = fma(p, z, -1.0 / 6.0);                             // -1/3!
    return fma(p * z, x, x);
}
#if ITAL_BVU_OWN_MATH
#define BVU_SIN(x) sin_halfpi(x)
#define BVU_EXP(x) exp_neg(x)      // (Cody-Waite + fitted polynomial, 0.93 ulp; valid for the positive arguments below too: <= 50)
#else
#define BVU_SIN(x) sin(x)
#define BVU_EXP(x) exp(x)
#endif

// P(X > sh, Y > sk), correlation r.
__device__ inline double mvn_bvu(double sh, double sk, double r) {
    const double TWOPI = 6.283185307179586;
    int lg;
    const double *W, *X;
    if (fabs(r) < 0.3) { lg = 3; W = BVU_W6; X = BVU_X6; }
    else if (fabs(r) < 0.75) { lg = 6; W = BVU_W12; X = BVU_X12; }
    else { lg = 10; W = BVU_W20; X = BVU_X20; }
    double h = sh, k = sk, hk = h * k, bvn = 0;
    if (fabs(r) < 0.925) {
        double hs = (h * h + k * k) / 2;
        double asr = asin(r);
        for (int i = 0; i < lg; i++) {
            double sn = BVU_SIN(asr * (X[i] + 1) / 2);
            bvn += W[i] * BVU_EXP((sn * hk - hs) / (1 - sn * sn));
            sn = BVU_SIN(asr * (-X[i] + 1) / 2);
            bvn += W[i] * BVU_EXP((sn * hk - hs) / (1 - sn * sn));
        }
        bvn = bvn * asr / (2 * TWOPI) + mvn_phi(-h) * mvn_phi(-k);
    } else {
        if (r < 0) { k = -k; hk = -hk; }
        if (fabs(r) < 1) {
            double as = (1 - r) * (1 + r);
            double a = sqrt(as);
            double bs = (h - k) * (h - k);
            double c = (4 - hk) / 8;
            double d = (12 - hk) / 16;
            double asr = -(bs / as + hk) / 2;
            if (asr > -100) bvn = a * BVU_EXP(asr) * (1 - c * (bs - as) * (1 - d * bs / 5) / 3 + c * d * as * as / 5);
            if (-hk < 100) {
                double b = sqrt(bs);
                bvn = bvn - BVU_EXP(-hk / 2) * sqrt(TWOPI) * mvn_phi(-b / a) * b * (1 - c * bs * (1 - d * bs / 5) / 3);
            }
            a = a / 2;
            for (int i = 0; i < lg; i++) {
                for (int is = -1; is <= 1; is += 2) {
                    double xs = (a + a * is * X[i]) * (a + a * is * X[i]);
                    double rs = sqrt(1 - xs);
                    double asr2 = -(bs / xs + hk) / 2;
                    if (asr2 > -100) {
                        double sp = (1 + c * xs * (1 + d * xs));
                        double ep = BVU_EXP(-hk * (1 - rs) / (2 * (1 + rs))) / rs;
                        bvn = bvn + a * W[i] * BVU_EXP(asr2) * (ep - sp);
                    }
                }
            }
            bvn = -bvn / TWOPI;
        }
        if (r > 0) {
            bvn = bvn + mvn_phi(-fmax(h, k));
        } else {
            bvn = -bvn;
            if (k > h) {
                if (h < 0) bvn = bvn + mvn_phi(k) - mvn_phi(h);
                else bvn = bvn + mvn_phi(-h) - mvn_phi(-k);
            }
        }
    }
    return bvn;
}

// Orthant probability of a standardised bivariate normal: variable j is > pivot_j when rel_j, else <= pivot_j.
__device__ inline double bvn_orthant(double p0, double p1, bool rel0, bool rel1, double r) {
    if (rel0 && rel1) return mvn_bvu(p0, p1, r);
    if (!rel0 && rel1) return mvn_bvu(-p0, p1, -r);
    if (rel0 && !rel1) return mvn_bvu(p0, -p1, -r);
    return mvn_bvu(-p0, -p1, r);
}

// ---------------------------------------------------------------------------------------------
// MVNUNI: L'Ecuyer (1996) combined multiple-recursive generator, the stream SciPy's mvndst draws
// its lattice shifts from.  State = (x10,x11,x12 mod m1; x20,x21,x22 mod m2).
struct MrgState {
    int x10, x11, x12, x20, x21, x22;
};
constexpr long long MRG_M1 = 2147483647LL, MRG_M2 = 2145483479LL;

__device__ __forceinline__ double mrg_next(MrgState& s) {
    // x12' = (63308*x11 - 183326*x10) mod m1 ; x22' = (86098*x22 - 539608*x20) mod m2
    long long p1 = (63308LL * s.x11 - 183326LL * s.x10) % MRG_M1;
    if (p1 < 0) p1 += MRG_M1;
    long long p2 = (86098LL * s.x22 - 539608LL * s.x20) % MRG_M2;
    if (p2 < 0) p2 += MRG_M2;
    s.x10 = s.x11; s.x11 = s.x12; s.x12 = (int)p1;
    s.x20 = s.x21; s.x21 = s.x22; s.x22 = (int)p2;
    int z = s.x12 - s.x22;
    if (z <= 0) z += (int)MRG_M1;
    return z * 4.656612873077392578125e-10;
}

// The same generator stepped in FP64: the recurrence multipliers are below 2^20 and the state below 2^31, so every
// product and difference is an exactly represented integer (< 2^52); the reduction is an approximate quotient, an exact
// remainder by FMA and one correction each way.  ~22 vector instructions per draw against ~80 for the 64-bit integer
// remainder -- this is what the lanes that generate a call's lattice shifts execute 40-200 times per call.
struct MrgStateF {
    double x10, x11, x12, x20, x21, x22;
};

__device__ __forceinline__ MrgStateF mrg_to_f(const MrgState& s) {
    return {(double)s.x10, (double)s.x11, (double)s.x12, (double)s.x20, (double)s.x21, (double)s.x22};
}

__device__ __forceinline__ double mod_exact(double p, double m, double inv_m) {
    const double q = floor(p * inv_m);
    double r = fma(-q, m, p);
    r = r < 0 ? r + m : r;
    r = r >= m ? r - m : r;
    return r;
}

// MVNUNI's integer z in [1, 2^31 - 1] (as a double); the uniform is z * MRG_INVMP1 -- a prepared call may store the 32-bit
// integer and the consumer form the identical double.
constexpr double MRG_INVMP1 = 4.656612873077392578125e-10;
__device__ __forceinline__ double mrg_next_z(MrgStateF& s) {
    const double M1 = 2147483647.0, M2 = 2145483479.0;
    const double p1 = mod_exact(fma(63308.0, s.x11, -183326.0 * s.x10), M1, 1.0 / 2147483647.0);
    const double p2 = mod_exact(fma(86098.0, s.x22, -539608.0 * s.x20), M2, 1.0 / 2145483479.0);
    s.x10 = s.x11; s.x11 = s.x12; s.x12 = p1;
    s.x20 = s.x21; s.x21 = s.x22; s.x22 = p2;
    double z = p1 - p2;
    z = z <= 0 ? z + M1 : z;
    return z;
}
__device__ __forceinline__ double mrg_next_f(MrgStateF& s) { return mrg_next_z(s) * MRG_INVMP1; }

// state <- J * state, J = two 3x3 matrices (row-major, entries already reduced): jump-ahead by a fixed count.
__device__ __forceinline__ void mrg_apply(MrgState& s, const long long* __restrict__ J) {
    unsigned long long a0 = s.x10, a1 = s.x11, a2 = s.x12;
    unsigned long long b0 = s.x20, b1 = s.x21, b2 = s.x22;
    unsigned long long r[3], q[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        // entries and state are below 2^31: three products sum to less than 3 * 2^62 < 2^64 -- one reduction per row
        r[i] = ((unsigned long long)J[3 * i] * a0 + (unsigned long long)J[3 * i + 1] * a1 +
                (unsigned long long)J[3 * i + 2] * a2) % MRG_M1;
        q[i] = ((unsigned long long)J[9 + 3 * i] * b0 + (unsigned long long)J[9 + 3 * i + 1] * b1 +
                (unsigned long long)J[9 + 3 * i + 2] * b2) % MRG_M2;
    }
    s.x10 = (int)r[0]; s.x11 = (int)r[1]; s.x12 = (int)r[2];
    s.x20 = (int)q[0]; s.x21 = (int)q[1]; s.x22 = (int)q[2];
}

// the same with every product reduced on its own (what the general scorer uses, see score_generic.hip)
__device__ __forceinline__ void mrg_apply_each(MrgState& s, const long long* __restrict__ J) {
    unsigned long long a0 = s.x10, a1 = s.x11, a2 = s.x12;
    unsigned long long b0 = s.x20, b1 = s.x21, b2 = s.x22;
    unsigned long long r[3], q[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        r[i] = ((unsigned long long)J[3 * i] * a0 % MRG_M1 + (unsigned long long)J[3 * i + 1] * a1 % MRG_M1 +
                (unsigned long long)J[3 * i + 2] * a2 % MRG_M1) % MRG_M1;
        q[i] = ((unsigned long long)J[9 + 3 * i] * b0 % MRG_M2 + (unsigned long long)J[9 + 3 * i + 1] * b1 % MRG_M2 +
                (unsigned long long)J[9 + 3 * i + 2] * b2 % MRG_M2) % MRG_M2;
    }
    s.x10 = (int)r[0]; s.x11 = (int)r[1]; s.x12 = (int)r[2];
    s.x20 = (int)q[0]; s.x21 = (int)q[1]; s.x22 = (int)q[2];
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

}  // namespace ital
