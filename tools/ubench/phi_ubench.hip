// Micro-benchmark: throughput of the (Phi, Phi^-1) chain of the lattice integrand in isolation, NC independent chains
// per lane, to separate the cost of the arithmetic itself from the kernel's bookkeeping (compaction, LDS, scalar work).
//   hipcc --offload-arch=gfx950 -O3 -I ital_amd/csrc -I include tools/ubench/phi_ubench.hip -o /tmp/phi_ubench
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include "device_math.h"
using namespace ital;

template <int NC, int MODE>
__global__ __launch_bounds__(256) void k(double* out, int iters, double a0) {
    double y[NC], acc[NC];
    for (int c = 0; c < NC; c++) { y[c] = 0.001 * (threadIdx.x + 7 * c) - 0.1; acc[c] = 0; }
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const double ph = mvn_phi(a0 - 0.3 * y[c]);
            const double w = 1.0 - ph;
            acc[c] += w;
            double p = fma(0.37 + 0.001 * c, w, ph);
            if (MODE == 0) y[c] = phinv_central(p);        // central branch only
            else y[c] = mvn_phinv(p);                      // with the divergent tail branch
        }
    }
    double s = 0;
    for (int c = 0; c < NC; c++) s += acc[c] + y[c];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// The same chain (central branch) with the NC chains of a lane sharing reciprocal seeds in groups of G, in Phi and in Phi^-1
// (device_math.h fast_div_group; G = 1: one seed per quotient through the same code).  NC a multiple of G.
template <int NC, int G>
__global__ __launch_bounds__(256) void kb(double* out, int iters, double a0) {
    double y[NC], acc[NC];
    for (int c = 0; c < NC; c++) { y[c] = 0.001 * (threadIdx.x + 7 * c) - 0.1; acc[c] = 0; }
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int g0 = 0; g0 < NC; g0 += G) {
            double z[G], n[G], d[G], q[G], p[G];
#pragma unroll
            for (int k = 0; k < G; k++) { z[k] = a0 - 0.3 * y[g0 + k]; mvn_phi_nd(z[k], LitK(), n[k], d[k]); }
            fast_div_group<G>(n, d, q, G);
#pragma unroll
            for (int k = 0; k < G; k++) {
                const double ph = mvn_phi_finish(z[k], q[k]);
                const double w = 1.0 - ph;
                acc[g0 + k] += w;
                p[k] = fma(0.37 + 0.001 * (g0 + k), w, ph);
                phinv_central_nd(p[k] - 0.5, n[k], d[k]);
            }
            fast_div_group<G>(n, d, q, G);
#pragma unroll
            for (int k = 0; k < G; k++) y[g0 + k] = q[k];
        }
    }
    double s = 0;
    for (int c = 0; c < NC; c++) s += acc[c] + y[c];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <int NC, int G>
void run_batched(const char* name, int blocks) {
    double* out;
    hipMalloc(&out, sizeof(double) * blocks * 256);
    const int iters = 2000;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL((kb<NC, G>), dim3(blocks), dim3(256), 0, 0, out, 10, 0.2);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    hipLaunchKernelGGL((kb<NC, G>), dim3(blocks), dim3(256), 0, 0, out, iters, 0.2);
    hipEventRecord(e1);
    hipDeviceSynchronize();
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    double sum = 0;
    double* h = (double*)malloc(sizeof(double) * blocks * 256);
    hipMemcpy(h, out, sizeof(double) * blocks * 256, hipMemcpyDeviceToHost);
    for (int i = 0; i < blocks * 256; i++) sum += h[i];
    free(h);
    double pairs = (double)blocks * 256 * NC * iters;
    printf("%-28s blocks %5d  %8.3f ms  %8.2f G pairs/s  checksum %.17g\n", name, blocks, ms, pairs / ms / 1e6, sum);
    hipFree(out);
}

template <int NC, int MODE>
void run(const char* name, int blocks) {
    double* out;
    hipMalloc(&out, sizeof(double) * blocks * 256);
    const int iters = 2000;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL((k<NC, MODE>), dim3(blocks), dim3(256), 0, 0, out, 10, 0.2);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    hipLaunchKernelGGL((k<NC, MODE>), dim3(blocks), dim3(256), 0, 0, out, iters, 0.2);
    hipEventRecord(e1);
    hipDeviceSynchronize();
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    double pairs = (double)blocks * 256 * NC * iters;
    printf("%-28s blocks %5d  %8.3f ms  %8.2f G pairs/s\n", name, blocks, ms, pairs / ms / 1e6);
    hipFree(out);
}

int main() {
    for (int blocks : {256 * 2, 256 * 3, 256 * 4, 256 * 8}) {
        run<1, 0>("1 chain central", blocks);
        run<2, 0>("2 chains central", blocks);
        run<4, 0>("4 chains central", blocks);
        run<8, 0>("8 chains central", blocks);
        run<4, 1>("4 chains with tail branch", blocks);
    }
    // six chains per lane as in the t <= 4 lattice sums, four waves per SIMD: seeds shared by groups of G (same checksum)
    run<6, 0>("6 chains central", 256 * 4);
    run_batched<6, 1>("6 chains, seed groups of 1", 256 * 4);
    run_batched<6, 2>("6 chains, seed groups of 2", 256 * 4);
    run_batched<6, 3>("6 chains, seed groups of 3", 256 * 4);
    run_batched<6, 6>("6 chains, seed groups of 6", 256 * 4);
    return 0;
}
