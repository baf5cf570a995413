// The library-owned context (include/ital_hip.h, ital_ctx.h, ital_ctx_live.h) as its two translation units see it: ctx.hip
// (create / fit / update / revoke / the fetches / predictions) and ctx_live.hip (reserve / add_rows / remove_rows /
// set_params / evidence).  Private: no host includes this.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <initializer_list>
#include <vector>

#include "ital_ctx.h"
#include "ital_hip.h"
#include "ital_internal.h"

struct ital_ctx {
    int64_t n_total = 0, row0 = 0, row1 = 0, n = 0, ldv = 0;
    int d = 0, ldx = 0, cap = 0, kmax = ITAL_MAX_T, rank = 0, world = 1, m = 0;
    double length_scale = 1, var = 1, noise = 1e-6;
    void* comm = nullptr;
    bool fitted = false;
    // device memory (all owned here)
    double *X = nullptr, *xn = nullptr, *L = nullptr, *alpha = nullptr, *XT = nullptr, *XTn = nullptr, *V = nullptr, *mu = nullptr,
           *s2 = nullptr, *ybuf = nullptr, *C = nullptr, *mi = nullptr, *rec = nullptr, *rec_all = nullptr, *work3k = nullptr,
           *qwork = nullptr, *stage = nullptr;
    int64_t qwork_doubles = 0, cand_cap = 0;
    int* status = nullptr;
    int32_t* cand = nullptr;
    uint8_t* alive = nullptr;
    int64_t* ret = nullptr;
    ital_batch batch = {};
    long long* jump[ITAL_MAX_T + 1] = {};
    long long* jumppat[ITAL_MAX_T + 1] = {};
    double* vk[ITAL_MAX_T + 1] = {};
    // host bookkeeping
    int mvn_state[6] = {};
    std::vector<uint8_t> seen;          // [n_total] labelled (the reference's relevant / irrelevant ids)
    int64_t n_seen = 0;
    std::vector<int64_t> order;         // the labelled samples in insertion order: order[p] sits at position p of L / V / XT
    std::vector<double> ylab;           // their labels, parallel to `order` (ital_ctx_set_params / _evidence rebuild from them)
    double* rwork = nullptr;            // ital_gp_remove_workspace(cap) doubles, allocated by the first ital_ctx_revoke
    std::vector<int64_t> last_picks;    // the batch of the last fetch (its feature rows sit in batch.XB on every rank)
    std::vector<void*> owned;
    // user model (ital_ctx_set_model); without one ital_ctx_fetch is the perfect-user layer above (-71 and all)
    bool has_model = false;
    ital_ctx_model model = {1.0, 0.0, 0, 0, 0, 0.0};
    // general scorer: stream tables, pick positions 0, 1, 2, ..., one zero, explicit list positions of this rank's
    // candidates, the subset-mode base set (E_idx, E_sort, E_mu, E_sig, pick_pos, in_pos, dead_pos)
    long long* jump1 = nullptr;
    double* vk_all = nullptr;
    int32_t* iota = nullptr;
    int64_t* zero64 = nullptr;
    int64_t* gpos = nullptr;
    int64_t gpos_cap = 0;
    char* sub = nullptr;
    int64_t sub_bytes = 0;
    // MCMI_min candidate block (ital_amd/mcmi.py: _gather_block / _fetch_bufs)
    double *Xc = nullptr, *Vc = nullptr, *vec = nullptr, *cov = nullptr, *ce = nullptr, *mwork = nullptr;
    int64_t* cand64 = nullptr;
    int32_t* bpos = nullptr;
    uint8_t* balive = nullptr;
    int64_t block_cap = 0, cov_cap = 0, mwork_doubles = 0;
    // top_results (ital_topk + the (value, index) exchange) and predict at external points (chunks of kPredictChunk)
    void* tk_work = nullptr;
    double *tk_send = nullptr, *tk_all = nullptr;
    int tk_cap = 0;
    double *pXt = nullptr, *pxtn = nullptr, *pVt = nullptr, *pmean = nullptr, *pvar = nullptr;
};

namespace {

template <class T>
T* dalloc(ital_ctx* c, size_t count) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T) + 64) != hipSuccess) return nullptr;
    if (hipMemset(p, 0, std::max<size_t>(count, 1) * sizeof(T) + 64) != hipSuccess) {
        (void)hipFree(p);
        return nullptr;
    }
    c->owned.push_back(p);
    return static_cast<T*>(p);
}

// Gives a buffer of the context back: nothing may still be using it (release() drains the stream first).
void dfree(ital_ctx* c, void* p) {
    if (!p) return;
    const auto it = std::find(c->owned.begin(), c->owned.end(), p);
    if (it != c->owned.end()) c->owned.erase(it);
    (void)hipFree(p);
}

// Every regrow path: work enqueued earlier on `stream` may still read the buffers being replaced, so the stream is drained
// before they are given back.
int release(ital_ctx* c, hipStream_t stream, std::initializer_list<void*> bufs) {
    if (hipStreamSynchronize(stream) != hipSuccess) return ital_fail(-5, "ital_ctx: stream error");
    for (void* p : bufs) dfree(c, p);
    return 0;
}

int pad16(int64_t v) { return (int)((v + 15) / 16 * 16); }

}  // namespace
