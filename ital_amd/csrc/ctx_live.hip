// A live session in a context that the library owns (include/ital_ctx_live.h): ital_ctx_reserve / _add_rows / _remove_rows /
// _set_params / _evidence.  Host code over the descriptor entry points of this same library, the way ital_amd's Python
// learners drive them (ital_amd/gp.py: extend, drop_rows, set_params, evidence); no kernel of its own.
//
// Every entry point builds the new state in locals (Staged, ctx_internal.h), enqueues its work, drains the stream, checks,
// and only then commits by moving the buffers into the context, which gives the old ones back: a call that fails leaves the
// context as it was.  A call that changes the rows or the capacity resets the lazily grown scratch with its commit.
//
// The reference has none of this (its dense K_all, ital/gp.py:128, is built once; a label, once given, stays,
// ital/retrieval_base.py:183-189).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx_internal.h"
#include "ital_compact.h"
#include "ital_ctx_live.h"
#include "ital_evidence.h"
#include "ital_revoke.h"
#include "ital_rewhiten.h"

namespace {

constexpr int64_t kEvidenceBytes = (int64_t)1 << 30;   // Grams, workspace and outputs of one ital_gp_evidence chunk

int d2d(void* dst, const void* src, size_t bytes, hipStream_t stream) {
    if (bytes == 0) return 0;
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream) == hipSuccess ? 0 : -1;
}

// rows x width doubles between matrices of leading dimensions ld_dst, ld_src (doubles).
int d2d_2d(double* dst, size_t ld_dst, const double* src, size_t ld_src, size_t width, size_t rows, hipStream_t stream) {
    if (width == 0 || rows == 0) return 0;
    return hipMemcpy2DAsync(dst, ld_dst * sizeof(double), src, ld_src * sizeof(double), width * sizeof(double), rows,
                            hipMemcpyDeviceToDevice, stream) == hipSuccess ? 0 : -1;
}

int whiten(const ital_ctx* c, const double* X, int64_t n_rows, const double* L, const double* alpha, int m, double var,
           double length_scale, double* xnorm, double* V, int64_t ldv, double* mu, double* s2, hipStream_t stream) {
    ital_rewhiten_desc r;
    memset(&r, 0, sizeof(r));
    r.X = X; r.n_rows = n_rows; r.ldx = c->ldx; r.XT = c->XT; r.XTn = c->XTn; r.L = L; r.ldl = c->cap; r.alpha = alpha; r.m = m;
    r.var = var; r.length_scale = length_scale; r.xnorm = xnorm; r.V = V; r.ldv = ldv; r.v_rows = c->cap; r.mu = mu; r.s2 = s2;
    r.chunk = 0;
    return ital_whiten_rows(&r, stream);
}

}  // namespace

extern "C" int ital_ctx_reserve(ital_ctx* c, int capacity, hipStream_t stream) {
    if (!c || !c->fitted) return ital_fail(-22, "ital_ctx_reserve: needs a context after ital_ctx_fit");
    if (capacity <= c->cap) return 0;
    if (capacity > (1 << 20)) return ital_fail(-22, "ital_ctx_reserve: capacity above 2^20");
    const int cap = c->cap, ncap = pad16(capacity), ldx = c->ldx, kmax = c->kmax;
    ital_dims nd = *c;
    nd.cap = ncap;
    Staged<ital_state> nw(stream);
    if (!nw.alloc(nd, BY_CAP)) return ital_fail(-12, "ital_ctx_reserve: out of device memory");
    // (the new buffers are zero: the padding of L beyond column cap, and every row from cap on, stay zero)
    if (d2d_2d(nw.L, ncap, c->L, cap, cap, cap, stream) || d2d(nw.alpha, c->alpha, (size_t)cap * sizeof(double), stream) ||
        d2d(nw.XT, c->XT, (size_t)cap * ldx * sizeof(double), stream) || d2d(nw.XTn, c->XTn, (size_t)cap * sizeof(double), stream) ||
        d2d(nw.V, c->V, (size_t)cap * c->ldv * sizeof(double), stream) || d2d_2d(nw.VB, ncap, c->VB, cap, cap, kmax, stream))
        return ital_fail(-5, "ital_ctx_reserve: a device-to-device copy failed");
    if (hipStreamSynchronize(stream) != hipSuccess) return ital_fail(-5, "ital_ctx_reserve: stream error");
    c->commit(nd, std::move(nw));
    c->drop_scratch();
    return 0;
}

extern "C" int ital_ctx_add_rows(ital_ctx* c, const double* rows, int64_t k, int on_device, hipStream_t stream) {
    if (!c || !c->fitted) return ital_fail(-22, "ital_ctx_add_rows: needs a context after ital_ctx_fit");
    if (k == 0) return 0;
    if (k < 0 || !rows) return ital_fail(-22, "ital_ctx_add_rows: rows missing or a negative count");
    if (c->world > 1) return ital_fail(-38, "ital_ctx_add_rows: row sharding cannot grow yet: all rows must be on one rank");
    if (c->n_total + k > 0x7fffffff) return ital_fail(-22, "ital_ctx_add_rows: more than 2^31 - 1 rows");
    const int64_t n = c->n, n_new = n + k, ldv = pad16(n_new);
    const int ldx = c->ldx, m = c->m;
    ital_dims nd = *c;
    nd.n = n_new;
    nd.ldv = ldv;
    std::vector<double> pad;
    Staged<ital_state> nw(stream);
    if (!nw.alloc(nd, BY_ROWS)) return ital_fail(-12, "ital_ctx_add_rows: out of device memory");
    // (the new buffers are zero: the pad columns of the new feature rows, V outside [0:m, 0:n_new) and the means' padding)
    if (d2d(nw.X, c->X, (size_t)n * ldx * sizeof(double), stream) || d2d(nw.xn, c->xn, (size_t)n * sizeof(double), stream) ||
        d2d(nw.mu, c->mu, (size_t)n * sizeof(double), stream) || d2d(nw.s2, c->s2, (size_t)n * sizeof(double), stream) ||
        d2d_2d(nw.V, ldv, c->V, c->ldv, n, m, stream) || !fill_var(nw.s2, n_new, ldv, c->var, pad, stream))
        return ital_fail(-5, "ital_ctx_add_rows: a device-to-device copy failed");
    if (!copy_rows(nw.X + (size_t)n * ldx, ldx, rows, c->d, k, on_device != 0, stream))
        return ital_fail(-5, "ital_ctx_add_rows: copy of the rows failed");
    const int rc = whiten(c, nw.X + (size_t)n * ldx, k, c->L, c->alpha, m, c->var, c->length_scale, nw.xn + n, nw.V + n, ldv,
                          nw.mu + n, nw.s2 + n, stream);
    if (rc) return rc;
    if (hipStreamSynchronize(stream) != hipSuccess) return ital_fail(-5, "ital_ctx_add_rows: stream error");
    c->commit(nd, std::move(nw));
    c->drop_scratch();
    c->n_total += k;
    c->row1 = c->row0 + n_new;
    c->seen.resize((size_t)c->n_total, 0);
    c->last_picks.clear();
    return 0;
}

extern "C" int ital_ctx_remove_rows(ital_ctx* c, const int64_t* idx, int64_t cnt, int64_t* index_map, hipStream_t stream) {
    if (!c || !c->fitted) return ital_fail(-22, "ital_ctx_remove_rows: needs a context after ital_ctx_fit");
    if (!idx || cnt < 1) return ital_fail(-22, "ital_ctx_remove_rows: idx missing or fewer than one index");
    if (c->world > 1) return ital_fail(-38, "ital_ctx_remove_rows: row sharding cannot shrink yet: all rows must be on one rank");
    const int64_t n_old = c->n_total;
    std::vector<uint8_t> gone((size_t)n_old, 0);
    for (int64_t j = 0; j < cnt; j++) {
        if (idx[j] < 0 || idx[j] >= n_old) return ital_fail(-22, "ital_ctx_remove_rows: index outside the data");
        if (gone[(size_t)idx[j]]) return ital_fail(-22, "ital_ctx_remove_rows: an index named twice");
        gone[(size_t)idx[j]] = 1;
    }
    if (cnt == n_old) return ital_fail(-22, "ital_ctx_remove_rows: no row would be left");
    // labelled positions that leave, highest first (the order of ital_ctx_revoke)
    std::vector<int> pos;
    for (int p = c->m - 1; p >= 0; p--)
        if (gone[(size_t)c->order[(size_t)p]]) pos.push_back(p);
    std::vector<int64_t> keep, map((size_t)n_old, -1);
    keep.reserve((size_t)(n_old - cnt));
    for (int64_t i = 0; i < n_old; i++)
        if (!gone[(size_t)i]) {
            map[(size_t)i] = (int64_t)keep.size();
            keep.push_back(i);
        }
    const int64_t n_keep = (int64_t)keep.size(), ldv = pad16(n_keep);
    const int ldx = c->ldx, cap = c->cap;
    ital_dims nd = *c;
    nd.n = n_keep;
    nd.ldv = ldv;
    std::vector<double> pad;
    // the labelled rows leave copies (`old`) of what ital_gp_remove rewrites: the context's own stays as it is until the commit
    struct Build {
        ital_state nw, old;
        DevBuf<int64_t> keep;
        DevBuf<int> st;
    };
    Staged<Build> b(stream);
    const bool labelled = !pos.empty();
    const ital_state& src = labelled ? b.old : static_cast<const ital_state&>(*c);
    if (!b.nw.alloc(nd, BY_ROWS) || !b.keep.alloc(n_keep) || !b.st.alloc(1) ||
        (labelled && (!b.old.alloc(*c, BY_LABEL) || c->rwork.ensure(ital_gp_remove_workspace(cap)) < 0)))
        return ital_fail(-12, "ital_ctx_remove_rows: out of device memory");
    if (hipMemcpyAsync(b.keep, keep.data(), (size_t)n_keep * sizeof(int64_t), hipMemcpyHostToDevice, stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_remove_rows: upload of the surviving rows' indices failed");
    int m = c->m;
    if (labelled) {
        if (!b.old.copy(*c, *c, BY_LABEL, stream)) return ital_fail(-5, "ital_ctx_remove_rows: a device-to-device copy failed");
        for (int p : pos) {
            const ital_remove_desc r = remove_desc(*c, b.old, m, p, c->rwork, b.st);
            const int rc = ital_gp_remove(&r, stream);
            if (rc) return rc;
            m--;
        }
    }
    int rc = ital_compact_rows(c->X, c->xn, c->n, ldx, ITAL_INGEST_F64, b.keep, n_keep, b.nw.X, b.nw.xn, b.st, stream);
    if (!rc) rc = ital_compact_cols(src.V, c->ldv, m, src.mu, src.s2, c->n, b.keep, n_keep, b.nw.V, ldv, cap, b.nw.mu, b.nw.s2, b.st, stream);
    if (rc) return rc;
    if (!fill_var(b.nw.s2, n_keep, ldv, c->var, pad, stream)) return ital_fail(-5, "ital_ctx_remove_rows: upload failed");
    int flagged = 0;
    if (hipMemcpyAsync(&flagged, b.st, sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_remove_rows: stream error");
    if (flagged) {
        char msg[256];
        snprintf(msg, sizeof(msg), "ital_ctx_remove_rows: the kernels flagged the call (status %d): a surviving row's index outside "
                 "the rows (ital_compact_rows / ital_compact_cols), or a factor that was broken before (ital_gp_remove)", flagged);
        return ital_fail(-22, msg);
    }
    // the commit (nothing can fail from here on): the new row state, over the labelled-set state the removals left in `old`
    b.old.take(std::move(b.nw));
    c->commit(nd, std::move(b.old));
    c->drop_scratch();
    for (int p : pos) {
        c->order.erase(c->order.begin() + p);
        c->ylab.erase(c->ylab.begin() + p);
    }
    for (int64_t& g : c->order) g = map[(size_t)g];
    c->m = m;
    c->n_seen -= (int64_t)pos.size();
    std::vector<uint8_t> seen((size_t)n_keep, 0);
    for (int64_t g : c->order) seen[(size_t)g] = 1;
    c->seen.swap(seen);
    c->n_total = n_keep;
    c->row1 = c->row0 + n_keep;
    c->last_picks.clear();
    if (index_map) memcpy(index_map, map.data(), (size_t)n_old * sizeof(int64_t));
    return 0;
}

extern "C" int ital_ctx_set_params(ital_ctx* c, double length_scale, double var, double noise, hipStream_t stream) {
    if (!c || !c->fitted) return ital_fail(-22, "ital_ctx_set_params: needs a context after ital_ctx_fit");
    const double ls = isnan(length_scale) ? c->length_scale : length_scale;
    const double v = isnan(var) ? c->var : var;
    const double nz = isnan(noise) ? c->noise : noise;
    if (!(ls > 0) || !(v > 0) || !(nz >= 0))
        return ital_fail(-22, "ital_ctx_set_params: length_scale and var must be positive, noise must not be negative");
    const int m = c->m, cap = c->cap;
    const int64_t n = c->n, ldv = c->ldv;
    std::vector<double> pad;
    struct Build {
        ital_state nw;
        DevBuf<double> yd;
        DevBuf<int> st;
    };
    Staged<Build> b(stream);
    if (m == 0) {
        // prior: mean 0, variance var (ital_ctx_fit); a variance vector like the one it replaces
        if (!b.nw.s2.alloc(c->s2.count)) return ital_fail(-12, "ital_ctx_set_params: out of device memory");
        if (!fill_var(b.nw.s2, 0, ldv, v, pad, stream) || hipStreamSynchronize(stream) != hipSuccess)
            return ital_fail(-5, "ital_ctx_set_params: upload failed");
        c->commit(*c, std::move(b.nw));
        c->length_scale = ls; c->var = v; c->noise = nz;
        return 0;
    }
    if (!b.nw.alloc(*c, BY_PARAMS) || !b.yd.alloc(m) || !b.st.alloc(1)) return ital_fail(-12, "ital_ctx_set_params: out of device memory");
    if (hipMemcpyAsync(b.yd, c->ylab.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice, stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_set_params: upload of the labels failed");
    for (int c0 = 0; c0 < m; c0 += 16) {
        const int rc = ital_chol_append(c->XT, c->XTn, c->ldx, b.nw.L, cap, b.nw.alpha, b.yd + c0, c0, std::min(16, m - c0), v, ls, nz,
                                        b.st, stream);
        if (rc) return rc;
    }
    int rc = whiten(c, c->X, n, b.nw.L, b.nw.alpha, m, v, ls, b.nw.xn, b.nw.V, ldv, b.nw.mu, b.nw.s2, stream);
    if (rc) return rc;
    if (!fill_var(b.nw.s2, n, ldv, v, pad, stream)) return ital_fail(-5, "ital_ctx_set_params: upload failed");
    int flagged = 0;
    if (hipMemcpyAsync(&flagged, b.st, sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_set_params: stream error");
    if (flagged & 1)
        return ital_fail(-33, "ital_ctx_set_params: kernel matrix of the labelled samples is not positive definite with these "
                              "parameters (the context keeps its own)");
    c->commit(*c, std::move(b.nw));
    c->length_scale = ls; c->var = v; c->noise = nz;
    return 0;
}

extern "C" int ital_ctx_evidence(ital_ctx* c, const double* params, int G, double* scores, int* ok, hipStream_t stream) {
    if (!c || !c->fitted) return ital_fail(-22, "ital_ctx_evidence: needs a context after ital_ctx_fit");
    if (!params || !scores || !ok || G < 1) return ital_fail(-22, "ital_ctx_evidence: a NULL pointer or fewer than one candidate");
    if (c->m == 0) return ital_fail(-22, "ital_ctx_evidence: needs a fitted relevance model: call ital_ctx_update first");
    const int m = c->m;
    // the rule of GaussianProcess.evidence_chunk (ital_amd/gp.py): Grams, workspace and outputs of a chunk below 1 GiB
    const int64_t per = 8 * ((int64_t)m * m + ital_gp_evidence_workspace(m, 1) + 2 * (int64_t)m + 4);
    if (per > kEvidenceBytes) return ital_fail(-12, "ital_ctx_evidence: one candidate alone takes more than 1 GiB");
    const int chunk = (int)std::min<int64_t>(G, std::min<int64_t>(kEvidenceBytes / per, 65535));
    const int64_t need = ital_gp_evidence_workspace(m, chunk);
    struct Tmp {
        DevBuf<double> yd, pd, K, work, sc, lm, lv;
        DevBuf<int> info, st;                        // st: the call's own word: the context's is not touched
    };
    Staged<Tmp> t(stream);
    if (!t.yd.alloc(m) || !t.pd.alloc((int64_t)G * 3) || !t.K.alloc((int64_t)chunk * m * m) || !t.work.alloc(need) ||
        !t.info.alloc(chunk) || !t.st.alloc(1) || !t.sc.alloc((int64_t)chunk * 3) || !t.lm.alloc((int64_t)chunk * m) ||
        !t.lv.alloc((int64_t)chunk * m))
        return ital_fail(-12, "ital_ctx_evidence: out of device memory");
    if (hipMemcpyAsync(t.yd, c->ylab.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipMemcpyAsync(t.pd, params, (size_t)G * 3 * sizeof(double), hipMemcpyHostToDevice, stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_evidence: upload of the labels and candidates failed");
    ital_evidence_desc d;
    memset(&d, 0, sizeof(d));
    d.XT = c->XT; d.XTn = c->XTn; d.ldx = c->ldx; d.y = t.yd; d.m = m; d.K = t.K; d.ld = m; d.scores = t.sc; d.info = t.info;
    d.loo_mean = t.lm; d.loo_var = t.lv; d.ldm = m; d.status = t.st; d.work = t.work; d.work_doubles = need; d.ev = nullptr;
    std::vector<int> info_h((size_t)chunk);
    for (int g0 = 0; g0 < G; g0 += chunk) {
        const int cc = std::min(chunk, G - g0);
        d.params = t.pd + (size_t)3 * g0;
        d.G = cc;
        const int rc = ital_gp_evidence(&d, stream);
        if (rc) return rc;
        if (hipMemcpyAsync(scores + (size_t)3 * g0, t.sc, (size_t)cc * 3 * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipMemcpyAsync(info_h.data(), t.info, (size_t)cc * sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)       // (the chunk's buffers are free again)
            return ital_fail(-5, "ital_ctx_evidence: download of the scores failed");
        for (int g = 0; g < cc; g++) ok[g0 + g] = info_h[(size_t)g] == 0;
    }
    return 0;
}
