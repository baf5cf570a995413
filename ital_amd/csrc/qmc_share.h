// The left-over chains of a lattice sum evaluated for several records in one round (score.hip, qmc_main_kernel<4>).
//
// A call at t = 4 has 16 x 73 = 1168 chains: three rounds of six chains per lane and 16 chains left over.  qmc_lane_sum
// (qmc_common.h) runs those 16 as a fourth round of one chain per lane on all 64 lanes -- 48 of them on a dead copy of item
// 0, and three Phi^-1 tail passes at 121 instructions each whatever their fill.  Here a wave takes four records: their
// 4 x 16 left-over chains fill exactly one round (eval_chain_lanes: factor, limits and flip bits per lane), and per record
// only the full rounds remain (qmc_lane_sum_full).  Per record the additions are the ones qmc_lane_sum makes, in its order:
// the same bits.
#pragma once
#include "qmc_common.h"

namespace ital {

// Chains of the lattice sum of dimension T with NH items per lane and round: full rounds, chains left over, chains per lane
// of the last round (as qmc_lane_sum lays them out).
template <int T, int NH>
struct QmcRounds {
    static constexpr int NDIM = T - 1, PRIME = P_TAB[(NDIM < 10 ? NDIM : 10) - 1];
    static constexpr int NC = 2 * NH, NITEM = 8 * PRIME;
    static constexpr int FULL = (2 * NITEM) / (64 * NC), REST = 2 * NITEM - FULL * 64 * NC;
    static constexpr int NCL = ITAL_QMC_TRIM_LAST ? (REST + 63) / 64 : (REST > 0 ? NC : 0);
};

// eval_chains (all-upper form) with the first variable's interval width given: it does not depend on the lattice point, and
// the round of the left-over chains has formed it already (w0: wave-uniform, flip_width applied).
// BPHI / BINV: seed groups of Phi and of the central Phi^-1 (eval_chains).
template <int T, int NCB, class K, int BPHI = 0, int BINV = 0>
__device__ __forceinline__ double eval_chains_w0(const double (&xx)[NCB][(T - 1 > 0 ? T - 1 : 1)], double w0,
                                                 const double (&cf)[(T * (T - 1) / 2 > 0 ? T * (T - 1) / 2 : 1)],
                                                 const double (&lm)[T], unsigned infi_c, double* tailq, int lane, const K& kk) {
    double yy[NCB][(T - 1 > 0 ? T - 1 : 1)], ff[NCB];
#pragma unroll
    for (int c = 0; c < NCB; c++) ff[c] = 1.0;
#pragma unroll
    for (int i = 0; i < T; i++) {
        const bool lower = (infi_c >> i) & 1u;
        double pin[NCB], ph[NCB];
        if (BPHI > 1 && i > 0) {
            if constexpr (BPHI > 1)
                phi_lat_grouped<NCB, (T - 1 > 0 ? T - 1 : 1), (T * (T - 1) / 2 > 0 ? T * (T - 1) / 2 : 1), BPHI>(yy, cf, i, lm[i], kk, ph);
        } else {
#pragma unroll
            for (int c = 0; c < NCB; c++) {
                if (i == 0) {
                    ph[c] = w0;
                } else {
                    double sc = 0;
#pragma unroll
                    for (int j = 0; j < i; j++) sc = fma(cf[i * (i - 1) / 2 + j], yy[c][j], sc);
                    ph[c] = mvn_phi_lat(lm[i] - sc, kk);
                }
            }
        }
        if (i > 0) flip_width<NCB>(ph, lower);
#pragma unroll
        for (int c = 0; c < NCB; c++) {
            const double w = ph[c];
            ff[c] *= w;
            if (ITAL_QMC_PIN_FF) __asm__ volatile("" : "+v"(ff[c]));
            if (i < T - 1) pin[c] = xx[c][i] * w;
        }
        if (i < T - 1) {
            double out[NCB];
            phinv_wave<NCB, K, 0, BINV>(pin, out, tailq, lane, kk);
#pragma unroll
            for (int c = 0; c < NCB; c++) yy[c][i] = out[c];
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < NCB; c++) acc += ff[c];
    return acc;
}

// qmc_lane_sum without its left-over round: the lane's sum over the FULL rounds of 2 NH chains.
template <int T, class K, int NH, int BPHI = 0, int BINV = 0>
__device__ __forceinline__ double qmc_lane_sum_full(const double* __restrict__ lat, double w0,
                                                    const double (&cf)[(T * (T - 1) / 2 > 0 ? T * (T - 1) / 2 : 1)],
                                                    const double (&lm)[T], unsigned infi_c, double* __restrict__ tailq, int lane,
                                                    const K& kk) {
    using R = QmcRounds<T, NH>;
    constexpr int NDIM = R::NDIM, PRIME = R::PRIME, NC = R::NC;
    double acc = 0.0;
    for (int base = 0; base < R::FULL * 64 * NH; base += 64 * NH) {
        double xx[NC][NDIM];
#pragma unroll
        for (int h = 0; h < NH; h++) {
            const int it = base + 64 * h + lane;
            const int sft = it / PRIME;
            const int k = it - sft * PRIME + 1;
#pragma unroll
            for (int j = 0; j < NDIM; j++) {
                const double v = k * lat[sft * NDIM + j] + lat[8 * NDIM + sft * NDIM + j];
                const double fr = v - floor(v);
                xx[2 * h][j] = fabs(2 * fr - 1);
                xx[2 * h + 1][j] = 1 - xx[2 * h][j];
            }
        }
        acc += eval_chains_w0<T, NC, K, BPHI, BINV>(xx, w0, cf, lm, infi_c, tailq, lane, kk);
    }
    return acc;
}

// eval_chains (all-upper form) with ONE chain per lane whose call differs from lane to lane: factor, limits and the bits of
// the negated variables are vector values.  flip_width becomes a select, applied only where the variable is negated.
// w0: the first variable's interval width of the lane's call (the same at every lattice point: eval_chains_w0).
template <int T, class K>
__device__ __forceinline__ double eval_chain_lanes(const double (&xx)[(T - 1 > 0 ? T - 1 : 1)], bool dead,
                                                   const double (&cf)[(T * (T - 1) / 2 > 0 ? T * (T - 1) / 2 : 1)],
                                                   const double (&lm)[T], unsigned flips, double* tailq, int lane, const K& kk,
                                                   double& w0) {
    double yy[(T - 1 > 0 ? T - 1 : 1)], ff = dead ? 0.0 : 1.0;
#pragma unroll
    for (int i = 0; i < T; i++) {
        double sc = 0;
#pragma unroll
        for (int j = 0; j < i; j++) sc = fma(cf[i * (i - 1) / 2 + j], yy[j], sc);
        const double ph = mvn_phi_lat(lm[i] - sc, kk);
        const double w = ((flips >> i) & 1u) ? 1.0 - (1.0 - ph) : ph;
        if (i == 0) w0 = w;
        ff *= w;
        if (i < T - 1) {
            double pin[1] = {xx[i] * w}, out[1];
            phinv_wave<1>(pin, out, tailq, lane, kk);
            yy[i] = out[0];
        }
    }
    double acc = 0.0;
    acc += ff;
    return acc;
}

}  // namespace ital
