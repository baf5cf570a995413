// Host check of the shared reciprocal seed (ital_amd/csrc/device_math.h, fast_div_group): over random (numerator,
// denominator) pairs in the ranges the lattice sums divide in, the quotients formed with one seed per group of G equal
// fast_div's own (one seed per quotient) bit for bit, and both lie within 0.5 ulp of the long-double quotient.
//   g++ -O2 -std=c++17 -ffp-contract=off tools/batch_div_check.cpp -o batch_div_check && ./batch_div_check [pairs per case]
// The arithmetic is the device's, spelled with fma(); the hardware seed v_rcp_f64 (good to ~2^-23) is emulated as 1/d with
// its mantissa cut to 24 bits.  Exit status 1 on any difference.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

static double seed_rcp(double d) {
    double r = 1.0 / d;
    uint64_t u;
    memcpy(&u, &r, 8);
    u &= ~((1ull << 29) - 1);      // 52 - 23 mantissa bits dropped
    memcpy(&r, &u, 8);
    return r;
}

static double fast_div(double n, double d) {
    double r = seed_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    const double q = n * r;
    return fma(fma(-d, q, n), r, q);
}

static void fast_div_group(const double* n, const double* d, double* out, int len) {
    if (len == 1) { out[0] = fast_div(n[0], d[0]); return; }
    double pre[8], r[8];
    pre[0] = d[0];
    for (int k = 1; k < len; k++) pre[k] = pre[k - 1] * d[k];
    const double dall = pre[len - 1];
    double ra = seed_rcp(dall);
    ra = fma(fma(-dall, ra, 1.0), ra, ra);
    for (int k = len - 1; k >= 1; k--) {
        r[k] = ra * pre[k - 1];
        ra = ra * d[k];
    }
    r[0] = ra;
    for (int k = 0; k < len; k++) {
        const double q = n[k] * r[k];
        out[k] = fma(fma(-d[k], q, n[k]), r[k], q);
    }
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {      // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double unif() { return (double)(rng() >> 11) * 0x1p-53; }
static double logunif(double lo, double hi) { return exp(log(lo) + unif() * (log(hi) - log(lo))); }

struct Range {
    const char* name;
    double dlo, dhi;      // denominators, log-uniform
    double qlo, qhi;      // |quotient| aimed at, log-uniform; the numerator is d * q rounded
    bool both_signs;
    double sat;           // share of saturated chains mixed in: denominator 1, numerator 0 or -2^-600 (mvn_phi_nd, |z| > 37)
};

// error of q against the long-double quotient, in units of the last place of the double next to that quotient
static double ulp_err(double q, double n, double d) {
    const long double t = (long double)n / (long double)d;
    if (t == 0) return q == 0 ? 0.0 : INFINITY;
    int e;
    frexpl(fabsl(t), &e);                                  // |t| in [2^(e-1), 2^e): ulp = 2^(e - 53)
    return (double)(fabsl((long double)q - t) * ldexpl(1.0L, 53 - e));
}

int main(int argc, char** argv) {
    const long pairs = argc > 1 ? atol(argv[1]) : 12000000;
    const Range ranges[] = {
        {"Hart Q, |z| <= 37", 440.0, 1.42e10, 1e-290, 0.5, true, 0.0},
        {"Hart Q with saturated chains", 440.0, 1.42e10, 1e-290, 0.5, true, 0.25},
        {"AS241 central, |q| <= 0.425", 1.0, 94.0, 1e-12, 1.44, true, 0.0},
        {"AS241 central incl. discarded tail arguments", 0.0022, 94.0, 1e-12, 240.0, true, 0.0},
    };
    long bad = 0;
    for (const Range& R : ranges)
        for (int G : {2, 3, 6}) {
            long differ = 0, beyond = 0;
            double worst_b = 0, worst_s = 0;
            for (long i = 0; i < pairs; i += G) {
                double n[8], d[8], qb[8];
                for (int k = 0; k < G; k++) {
                    if (unif() < R.sat) {
                        d[k] = 1.0;
                        n[k] = (rng() & 1) ? -0x1p-600 : 0.0;
                    } else {
                        d[k] = logunif(R.dlo, R.dhi);
                        n[k] = d[k] * logunif(R.qlo, R.qhi);
                        if (R.both_signs && (rng() & 1)) n[k] = -n[k];
                    }
                }
                fast_div_group(n, d, qb, G);
                for (int k = 0; k < G; k++) {
                    const double qs = fast_div(n[k], d[k]);
                    if (memcmp(&qs, &qb[k], 8) != 0) {
                        if (differ++ < 5) printf("  differ: n %a d %a single %a batched %a\n", n[k], d[k], qs, qb[k]);
                    }
                    const double eb = ulp_err(qb[k], n[k], d[k]), es = ulp_err(qs, n[k], d[k]);
                    if (eb > worst_b) worst_b = eb;
                    if (es > worst_s) worst_s = es;
                    if (eb > 0.5 || es > 0.5) beyond++;
                }
            }
            printf("%-46s G %d: %ld pairs, %ld differ, worst error batched %.6f ulp, one seed %.6f ulp, %ld beyond 0.5 ulp\n",
                   R.name, G, pairs / G * G, differ, worst_b, worst_s, beyond);
            bad += differ + beyond;
        }
    printf(bad ? "FAILED\n" : "all quotients equal and within 0.5 ulp\n");
    return bad ? 1 : 0;
}
