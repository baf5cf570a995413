// ital_ctx_audit (include/ital_ctx_audit.h): which labels of a context's session deserve a second look, and what taking each
// of them back would change.  Host code over ital_gp_influence with the context's buffers as inputs and temporaries that the
// call owns (Staged, ctx_internal.h), the way ital_ctx_evidence stands over ital_gp_evidence; no kernel of its own, and the
// context is only read.  What ital_amd's ActiveRetrievalBase.audit does in Python.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx_internal.h"
#include "ital_ctx_audit.h"
#include "ital_influence.h"

extern "C" int ital_ctx_audit(ital_ctx* c, int unseen_only, int64_t* ids, double* table, int* count, hipStream_t stream) {
    if (!c || !c->fitted) return ital_fail(-22, "ital_ctx_audit: needs a context after ital_ctx_fit");
    if (!ids || !table || !count) return ital_fail(-22, "ital_ctx_audit: a NULL pointer");
    if (c->m == 0) return ital_fail(-22, "ital_ctx_audit: needs a fitted relevance model: call ital_ctx_update first");
    if (c->world > 1) return ital_fail(-38, "ital_ctx_audit: the per-rank tables are not exchanged: all rows must be on one rank");
    const int m = c->m;
    const int64_t n = c->n, need = ital_gp_influence_workspace(m, n);
    struct Tmp {
        DevBuf<double> work, coef, stats;
        DevBuf<uint8_t> mask;
        DevBuf<int> st;                              // the call's own word: the context's is not touched
    };
    Staged<Tmp> t(stream);
    if (!t.work.alloc(need) || !t.coef.alloc(2 * (int64_t)m) || !t.stats.alloc(4 * (int64_t)m) || !t.st.alloc(1) ||
        (unseen_only && !t.mask.alloc(n)))
        return ital_fail(-12, "ital_ctx_audit: out of device memory");
    std::vector<uint8_t> unseen;
    int64_t counted = n;
    if (unseen_only) {
        unseen.resize((size_t)std::max<int64_t>(n, 1));
        counted = 0;
        for (int64_t j = 0; j < n; j++) counted += unseen[(size_t)j] = !c->seen[(size_t)j];
        if (hipMemcpyAsync(t.mask, unseen.data(), (size_t)n, hipMemcpyHostToDevice, stream) != hipSuccess)
            return ital_fail(-5, "ital_ctx_audit: upload of the row mask failed");
    }
    ital_influence_desc d;
    memset(&d, 0, sizeof(d));
    d.L = c->L; d.ldl = c->cap; d.alpha = c->alpha; d.m = m; d.V = c->V; d.ldv = c->ldv; d.n = n; d.mu = c->mu; d.s2 = c->s2;
    d.mask = unseen_only ? t.mask.p : nullptr; d.coef = t.coef; d.stats = t.stats; d.work = t.work; d.work_doubles = need;
    d.status = t.st;
    const int rc = ital_gp_influence(&d, stream);
    if (rc) return rc;
    std::vector<double> coef(2 * (size_t)m), stats(4 * (size_t)m);
    if (hipMemcpyAsync(coef.data(), t.coef, coef.size() * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipMemcpyAsync(stats.data(), t.stats, stats.size() * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_audit: download of the tables failed");
    for (int p = 0; p < m; p++) {
        const double y = c->ylab[(size_t)p], ci = coef[2 * (size_t)p], w = coef[2 * (size_t)p + 1];
        const double loo_mean = y - w / ci, loo_var = 1.0 / ci;
        double* row = table + 8 * (size_t)p;
        ids[p] = c->order[(size_t)p];
        row[0] = y;
        row[1] = loo_mean;
        row[2] = loo_var;
        row[3] = 0.5 * erfc(y * loo_mean / sqrt(loo_var) * M_SQRT1_2);       // ndtr(-y loo_mean / sd)
        row[4] = counted ? sqrt(stats[4 * (size_t)p] / (double)counted) : 0.0;
        row[5] = stats[4 * (size_t)p + 1];
        row[6] = stats[4 * (size_t)p + 2];
        row[7] = stats[4 * (size_t)p + 3];
    }
    *count = m;
    return 0;
}
