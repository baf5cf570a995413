// A host that is not Python, beyond the perfect user: a whole golden session of the reference -- every round's update and
// fetch, then top_results and predict -- through the context layer of libital_hip.so (include/ital_ctx.h) from C++ alone.
// Built and run by tests/test_gpu_host_cpp_models.py (-m gpu):
//
//     host_gpu_driver_models <X.f64> <session.txt>
//
// X.f64: the n x d feature matrix as raw little-endian doubles.  session.txt: whitespace-separated numbers --
//     mode n d length_scale var noise k rounds label_prob mistake_prob label_estimation
//     per round: c idx[c] y[c]   n_cand cand[n_cand]   picks[k]        (the labels given before the fetch; its candidate
//                                                                         list, 0 = all unlabelled; the reference's batch)
//     c idx[c] y[c]                                                    (the labels of the last batch)
//     top[10]   nt Xt[nt * d] mean[nt] var[nt]
// mode 0: ITAL with the user model (ital_ctx_set_model + ital_ctx_fetch); mode 1: MCMI_min (ital_ctx_mcmi_fetch).
// Exit code 0: everything is the reference's; 1: a result differs; 2: a call failed.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ital_ctx.h"

#define ITAL_OK(call)                                                                                  \
    do {                                                                                               \
        int rc_ = (call);                                                                              \
        if (rc_ < 0) {                                                                                 \
            fprintf(stderr, "%s:%d: %s -> %d: %s\n", __FILE__, __LINE__, #call, rc_, ital_last_error()); \
            return 2;                                                                                  \
        }                                                                                              \
    } while (0)

static FILE* g_in = nullptr;

static double next_num() {
    double v = 0;
    if (fscanf(g_in, "%lf", &v) != 1) {
        fprintf(stderr, "session file ended early\n");
        exit(2);
    }
    return v;
}

static void read_labels(std::vector<int64_t>& idx, std::vector<double>& y) {
    const int c = (int)next_num();
    idx.resize(c);
    y.resize(c);
    for (int j = 0; j < c; j++) idx[j] = (int64_t)next_num();
    for (int j = 0; j < c; j++) y[j] = next_num();
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s X.f64 session.txt\n", argv[0]);
        return 2;
    }
    g_in = fopen(argv[2], "r");
    if (!g_in) return 2;
    const int mode = (int)next_num();
    const int64_t n = (int64_t)next_num();
    const int d = (int)next_num();
    const double ls = next_num(), var = next_num(), noise = next_num();
    const int k = (int)next_num(), rounds = (int)next_num();
    ital_ctx_model model = {};
    model.label_prob = next_num();
    model.mistake_prob = next_num();
    model.label_estimation = (int)next_num();
    std::vector<double> X((size_t)n * d);
    FILE* fx = fopen(argv[1], "rb");
    if (!fx || fread(X.data(), sizeof(double), X.size(), fx) != X.size()) return 2;
    fclose(fx);

    ital_ctx* ctx = nullptr;
    ITAL_OK(ital_ctx_create(n, d, ls, var, noise, 64, 0, 1, nullptr, &ctx));
    ITAL_OK(ital_ctx_fit(ctx, X.data(), 0, nullptr));
    if (mode == 0) ITAL_OK(ital_ctx_set_model(ctx, &model));
    int bad = 0;
    std::vector<int64_t> idx, picks(k), cand;
    std::vector<double> y;
    for (int r = 0; r < rounds; r++) {
        read_labels(idx, y);
        ITAL_OK(ital_ctx_update(ctx, idx.data(), y.data(), (int)idx.size(), nullptr));
        cand.resize((size_t)next_num());
        for (auto& c : cand) c = (int64_t)next_num();
        const int64_t* list = cand.empty() ? nullptr : cand.data();
        const int got = mode == 0 ? ital_ctx_fetch(ctx, k, picks.data(), nullptr)
                                  : ital_ctx_mcmi_fetch(ctx, k, list, (int64_t)cand.size(), picks.data(), nullptr);
        ITAL_OK(got);
        printf("round %d picks:", r);
        for (int t = 0; t < k; t++) {
            const int64_t want = (int64_t)next_num();
            printf(" %lld", (long long)picks[t]);
            bad |= got != k || picks[t] != want;
        }
        printf("\n");
    }
    read_labels(idx, y);
    ITAL_OK(ital_ctx_update(ctx, idx.data(), y.data(), (int)idx.size(), nullptr));
    std::vector<int64_t> top(10);
    ITAL_OK(ital_ctx_top_results(ctx, 10, top.data(), nullptr));
    printf("top_results(10):");
    for (int j = 0; j < 10; j++) {
        printf(" %lld", (long long)top[j]);
        bad |= top[j] != (int64_t)next_num();
    }
    printf("\n");
    const int64_t nt = (int64_t)next_num();
    std::vector<double> Xt((size_t)nt * d), mean(nt), pvar(nt);
    for (auto& v : Xt) v = next_num();
    ITAL_OK(ital_ctx_predict(ctx, Xt.data(), nt, mean.data(), pvar.data(), nullptr));
    double err = 0;
    for (int64_t i = 0; i < nt; i++) err = std::fmax(err, std::fabs(mean[i] - next_num()));
    for (int64_t i = 0; i < nt; i++) err = std::fmax(err, std::fabs(pvar[i] - next_num()));
    printf("predict: largest deviation %.3g\n", err);
    bad |= !(err <= 1e-9);
    ITAL_OK(ital_ctx_destroy(ctx));
    fclose(g_in);
    printf(bad ? "MISMATCH\n" : "ok (the reference's session)\n");
    return bad ? 1 : 0;
}
