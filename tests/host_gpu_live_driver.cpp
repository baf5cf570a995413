// A host that is not Python drives a live session (include/ital_ctx_live.h) from C++ alone: create, fit, label; rows arrive;
// a grid of hyper-parameter candidates is scored against the session's own labels and the best one applied; rows leave;
// fetch.  Only the library's headers -- no device buffer of the host's own.  Built and run by
// tests/test_gpu_host_cpp_live.py (-m gpu), which makes the same calls through ctypes and compares what is printed:
//
//     host_gpu_live_driver <X.f64> <n> <d> <length_scale> <Xnew.f64> <k_new> <grid.f64> <G> <k>
//                          <n_labels> <id> <y> ... <n_removed> <id> ...
//
// X.f64 / Xnew.f64: n x d and k_new x d raw little-endian doubles; grid.f64: G x 3 (length_scale, var, noise).
// Prints "best", "map", "picks" and "means" lines.  Exit code 0, or 2 when a call failed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ital_ctx_live.h"

#define ITAL_OK(call)                                                                         \
    do {                                                                                      \
        int rc_ = (call);                                                                     \
        if (rc_ != 0) {                                                                       \
            fprintf(stderr, "%s:%d: %s -> %d: %s\n", __FILE__, __LINE__, #call, rc_, ital_last_error()); \
            return 2;                                                                         \
        }                                                                                     \
    } while (0)

static bool read_doubles(const char* path, std::vector<double>& out) {
    FILE* f = fopen(path, "rb");
    const bool ok = f && fread(out.data(), sizeof(double), out.size(), f) == out.size();
    if (f) fclose(f);
    if (!ok) fprintf(stderr, "cannot read %s\n", path);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 12) {
        fprintf(stderr, "usage: %s X.f64 n d length_scale Xnew.f64 k_new grid.f64 G k n_labels (id y)... n_removed id...\n", argv[0]);
        return 2;
    }
    const int64_t n = atoll(argv[2]);
    const int d = atoi(argv[3]);
    const double ls = atof(argv[4]);
    const int64_t k_new = atoll(argv[6]);
    const int G = atoi(argv[8]), k = atoi(argv[9]), n_lab = atoi(argv[10]);
    if (n < 1 || d < 1 || k_new < 1 || G < 1 || k < 1 || k > ITAL_MAX_T || n_lab < 1 || argc < 12 + 2 * n_lab) return 2;
    std::vector<int64_t> ids(n_lab), gone;
    std::vector<double> y(n_lab);
    for (int j = 0; j < n_lab; j++) {
        ids[j] = atoll(argv[11 + 2 * j]);
        y[j] = atof(argv[12 + 2 * j]);
    }
    const int n_gone = atoi(argv[11 + 2 * n_lab]);
    if (n_gone < 1 || argc != 12 + 2 * n_lab + n_gone) return 2;
    for (int j = 0; j < n_gone; j++) gone.push_back(atoll(argv[12 + 2 * n_lab + j]));
    std::vector<double> X((size_t)n * d), Xnew((size_t)k_new * d), grid((size_t)G * 3);
    if (!read_doubles(argv[1], X) || !read_doubles(argv[5], Xnew) || !read_doubles(argv[7], grid)) return 2;

    // 1. create, fit, label (a capacity that the labels outgrow: reserve)
    ital_ctx* ctx = nullptr;
    ITAL_OK(ital_ctx_create(n, d, ls, 1.0, 1e-6, 16, 0, 1, nullptr, &ctx));
    ITAL_OK(ital_ctx_fit(ctx, X.data(), 0, nullptr));
    ITAL_OK(ital_ctx_reserve(ctx, n_lab + k, nullptr));
    ITAL_OK(ital_ctx_update(ctx, ids.data(), y.data(), n_lab, nullptr));
    // 2. rows arrive
    ITAL_OK(ital_ctx_add_rows(ctx, Xnew.data(), k_new, 0, nullptr));
    // 3. score the grid, apply the candidate of largest log marginal likelihood (the first one among equals)
    std::vector<double> scores((size_t)G * 3);
    std::vector<int> ok(G);
    ITAL_OK(ital_ctx_evidence(ctx, grid.data(), G, scores.data(), ok.data(), nullptr));
    int best = -1;
    for (int g = 0; g < G; g++)
        if (ok[g] && (best < 0 || scores[3 * g] > scores[3 * best])) best = g;
    if (best < 0) {
        fprintf(stderr, "no candidate has a positive definite kernel matrix\n");
        return 2;
    }
    printf("best: %d %.17g\n", best, scores[3 * best]);
    ITAL_OK(ital_ctx_set_params(ctx, grid[3 * best], grid[3 * best + 1], grid[3 * best + 2], nullptr));
    // 4. rows leave
    std::vector<int64_t> map((size_t)(n + k_new));
    ITAL_OK(ital_ctx_remove_rows(ctx, gone.data(), n_gone, map.data(), nullptr));
    printf("map:");
    for (int64_t v : map) printf(" %lld", (long long)v);
    printf("\n");
    // 5. fetch
    std::vector<int64_t> picks(k);
    const int got = ital_ctx_fetch(ctx, k, picks.data(), nullptr);
    if (got != k) {
        fprintf(stderr, "ital_ctx_fetch -> %d: %s\n", got, ital_last_error());
        return 2;
    }
    printf("picks:");
    for (int t = 0; t < k; t++) printf(" %lld", (long long)picks[t]);
    printf("\n");
    const int64_t rows = ital_ctx_local_rows(ctx, nullptr);
    std::vector<double> mean(rows);
    ITAL_OK(ital_ctx_predict_stored(ctx, mean.data(), nullptr, nullptr));
    printf("means:");
    for (double v : mean) printf(" %.17g", v);
    printf("\n");
    ITAL_OK(ital_ctx_destroy(ctx));
    return 0;
}
