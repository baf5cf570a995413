// A live session in a library-owned context (include/ital_ctx_live.h): ital_ctx_reserve / _add_rows / _remove_rows /
// _set_params / _evidence.  Host code over the descriptor entry points of this same library, the way ital_amd's Python
// learners drive them (ital_amd/gp.py: extend, drop_rows, set_params, evidence); no kernel of its own.
//
// Every entry point builds the new state in fresh buffers (Fresh below), drains the stream, checks, and only then swaps the
// buffers into the context and gives the old ones back: a call that fails leaves the context as it was.
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

// Buffers a call allocates.  Those still listed when the object goes out of scope are given back, after the stream has
// drained; keep() hands them to the context for good.
struct Fresh {
    ital_ctx* c;
    hipStream_t stream;
    std::vector<void*> bufs;
    bool ok = true;
    Fresh(ital_ctx* ctx, hipStream_t s) : c(ctx), stream(s) {}
    Fresh(const Fresh&) = delete;
    Fresh& operator=(const Fresh&) = delete;
    template <class T>
    T* get(size_t count) {
        T* p = dalloc<T>(c, count);
        if (p) bufs.push_back(p);
        else ok = false;
        return p;
    }
    void keep() { bufs.clear(); }
    ~Fresh() {
        if (bufs.empty()) return;
        (void)hipStreamSynchronize(stream);
        for (void* p : bufs) dfree(c, p);
    }
};

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

// Entries [n, ld) of a variance vector <- var, as ital_ctx_fit leaves them (`pad` must outlive the stream's work).
int pad_s2(double* s2, int64_t n, int64_t ld, double var, std::vector<double>& pad, hipStream_t stream) {
    if (ld <= n) return 0;
    pad.assign((size_t)(ld - n), var);
    return hipMemcpyAsync(s2 + n, pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice, stream) == hipSuccess ? 0 : -1;
}

// The lazily grown scratch whose size follows the number of rows (n, ldv): given back and its recorded capacities zeroed,
// so that the paths of ctx.hip allocate it again on next use.  The stream has drained.
void drop_row_scratch(ital_ctx* c) {
    for (void* p : {(void*)c->cand, (void*)c->alive, (void*)c->mi, (void*)c->gpos, (void*)c->sub, (void*)c->Xc, (void*)c->Vc,
                    (void*)c->vec, (void*)c->cov, (void*)c->ce, (void*)c->mwork, (void*)c->cand64, (void*)c->bpos,
                    (void*)c->balive, (void*)c->tk_work, (void*)c->tk_send, (void*)c->tk_all, (void*)c->pXt, (void*)c->pxtn,
                    (void*)c->pVt, (void*)c->pmean, (void*)c->pvar, (void*)c->qwork})
        dfree(c, p);
    c->cand = nullptr; c->alive = nullptr; c->mi = nullptr; c->cand_cap = 0;
    c->gpos = nullptr; c->gpos_cap = 0;
    c->sub = nullptr; c->sub_bytes = 0;
    c->Xc = c->Vc = c->vec = c->cov = c->ce = c->mwork = nullptr;
    c->cand64 = nullptr; c->bpos = nullptr; c->balive = nullptr;
    c->block_cap = c->cov_cap = c->mwork_doubles = 0;
    c->tk_work = nullptr; c->tk_send = c->tk_all = nullptr; c->tk_cap = 0;
    c->pXt = c->pxtn = c->pVt = c->pmean = c->pvar = nullptr;
    c->qwork = nullptr; c->qwork_doubles = 0;
}

// The lazily grown scratch whose size follows the labelled-set capacity: Vc [cap][ldc] of the MCMI block (with the
// covariance block, which shares its recorded capacity), pVt [cap][chunk] of predict, the workspace of ital_gp_remove.
void drop_cap_scratch(ital_ctx* c) {
    for (void* p : {(void*)c->Vc, (void*)c->cov, (void*)c->pXt, (void*)c->pxtn, (void*)c->pVt, (void*)c->pmean, (void*)c->pvar,
                    (void*)c->rwork})
        dfree(c, p);
    c->Vc = c->cov = nullptr; c->cov_cap = 0;
    c->pXt = c->pxtn = c->pVt = c->pmean = c->pvar = nullptr;
    c->rwork = nullptr;
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
    const int rec_len = ital_record_len(ldx, ncap, kmax);
    Fresh nw(c, stream);
    double* L = nw.get<double>((size_t)ncap * ncap);
    double* alpha = nw.get<double>(ncap);
    double* XT = nw.get<double>((size_t)ncap * ldx);
    double* XTn = nw.get<double>(ncap);
    double* V = nw.get<double>((size_t)ncap * c->ldv);
    double* VB = nw.get<double>((size_t)kmax * ncap);
    double* rec = nw.get<double>(rec_len);
    double* rec_all = nw.get<double>((size_t)c->world * rec_len);
    if (!nw.ok) return ital_fail(-12, "ital_ctx_reserve: out of device memory");
    // (the new buffers are zero: the padding of L beyond column cap, and every row from cap on, stay zero)
    if (d2d_2d(L, ncap, c->L, cap, cap, cap, stream) || d2d(alpha, c->alpha, (size_t)cap * sizeof(double), stream) ||
        d2d(XT, c->XT, (size_t)cap * ldx * sizeof(double), stream) || d2d(XTn, c->XTn, (size_t)cap * sizeof(double), stream) ||
        d2d(V, c->V, (size_t)cap * c->ldv * sizeof(double), stream) || d2d_2d(VB, ncap, c->batch.VB, cap, cap, kmax, stream))
        return ital_fail(-5, "ital_ctx_reserve: a device-to-device copy failed");
    if (hipStreamSynchronize(stream) != hipSuccess) return ital_fail(-5, "ital_ctx_reserve: stream error");
    for (void* p : {(void*)c->L, (void*)c->alpha, (void*)c->XT, (void*)c->XTn, (void*)c->V, (void*)c->batch.VB, (void*)c->rec,
                    (void*)c->rec_all})
        dfree(c, p);
    drop_cap_scratch(c);
    nw.keep();
    c->L = L; c->alpha = alpha; c->XT = XT; c->XTn = XTn; c->V = V; c->batch.VB = VB; c->rec = rec; c->rec_all = rec_all;
    c->cap = ncap;
    c->batch.ldw = ncap;
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
    Fresh nw(c, stream);
    double* X = nw.get<double>((size_t)n_new * ldx);
    double* xn = nw.get<double>(n_new);
    double* V = nw.get<double>((size_t)c->cap * ldv);
    double* mu = nw.get<double>(ldv);
    double* s2 = nw.get<double>(ldv);
    double* C = nw.get<double>((size_t)c->kmax * ldv);
    if (!nw.ok) return ital_fail(-12, "ital_ctx_add_rows: out of device memory");
    std::vector<double> pad;
    // (the new buffers are zero: the pad columns of the new feature rows, V outside [0:m, 0:n_new) and the means' padding)
    if (d2d(X, c->X, (size_t)n * ldx * sizeof(double), stream) || d2d(xn, c->xn, (size_t)n * sizeof(double), stream) ||
        d2d(mu, c->mu, (size_t)n * sizeof(double), stream) || d2d(s2, c->s2, (size_t)n * sizeof(double), stream) ||
        d2d_2d(V, ldv, c->V, c->ldv, n, m, stream) || pad_s2(s2, n_new, ldv, c->var, pad, stream))
        return ital_fail(-5, "ital_ctx_add_rows: a device-to-device copy failed");
    if (hipMemcpy2DAsync(X + (size_t)n * ldx, (size_t)ldx * sizeof(double), rows, (size_t)c->d * sizeof(double),
                         (size_t)c->d * sizeof(double), (size_t)k, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                         stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_add_rows: copy of the rows failed");
    const int rc = whiten(c, X + (size_t)n * ldx, k, c->L, c->alpha, m, c->var, c->length_scale, xn + n, V + n, ldv, mu + n, s2 + n,
                          stream);
    if (rc) return rc;
    if (hipStreamSynchronize(stream) != hipSuccess) return ital_fail(-5, "ital_ctx_add_rows: stream error");
    for (void* p : {(void*)c->X, (void*)c->xn, (void*)c->V, (void*)c->mu, (void*)c->s2, (void*)c->C}) dfree(c, p);
    drop_row_scratch(c);
    nw.keep();
    c->X = X; c->xn = xn; c->V = V; c->mu = mu; c->s2 = s2; c->C = C;
    c->n = n_new; c->ldv = ldv;
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
    Fresh nw(c, stream), tmp(c, stream);
    double* X = nw.get<double>((size_t)n_keep * ldx);
    double* xn = nw.get<double>(n_keep);
    double* V = nw.get<double>((size_t)cap * ldv);
    double* mu = nw.get<double>(ldv);
    double* s2 = nw.get<double>(ldv);
    double* C = nw.get<double>((size_t)c->kmax * ldv);
    int64_t* keep_d = tmp.get<int64_t>(n_keep);
    int* st = tmp.get<int>(1);
    // the labelled rows leave copies of the model's state: the context's own stays as it is until the swap
    double *L = c->L, *alpha = c->alpha, *XT = c->XT, *XTn = c->XTn, *V_src = c->V, *mu_src = c->mu, *s2_src = c->s2, *rwork = c->rwork;
    if (!pos.empty()) {
        L = nw.get<double>((size_t)cap * cap);
        alpha = nw.get<double>(cap);
        XT = nw.get<double>((size_t)cap * ldx);
        XTn = nw.get<double>(cap);
        V_src = tmp.get<double>((size_t)cap * c->ldv);
        mu_src = tmp.get<double>(c->ldv);
        s2_src = tmp.get<double>(c->ldv);
        if (!rwork) rwork = nw.get<double>((size_t)ital_gp_remove_workspace(cap));
    }
    if (!nw.ok || !tmp.ok) return ital_fail(-12, "ital_ctx_remove_rows: out of device memory");
    if (hipMemcpyAsync(keep_d, keep.data(), (size_t)n_keep * sizeof(int64_t), hipMemcpyHostToDevice, stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_remove_rows: upload of the surviving rows' indices failed");
    int m = c->m;
    if (!pos.empty()) {
        if (d2d(L, c->L, (size_t)cap * cap * sizeof(double), stream) || d2d(alpha, c->alpha, (size_t)cap * sizeof(double), stream) ||
            d2d(XT, c->XT, (size_t)cap * ldx * sizeof(double), stream) || d2d(XTn, c->XTn, (size_t)cap * sizeof(double), stream) ||
            d2d(V_src, c->V, (size_t)cap * c->ldv * sizeof(double), stream) ||
            d2d(mu_src, c->mu, (size_t)c->ldv * sizeof(double), stream) || d2d(s2_src, c->s2, (size_t)c->ldv * sizeof(double), stream))
            return ital_fail(-5, "ital_ctx_remove_rows: a device-to-device copy failed");
        for (int p : pos) {
            ital_remove_desc r = {};
            r.XT = XT; r.XTn = XTn; r.ldx = ldx; r.L = L; r.ldl = cap; r.alpha = alpha;
            r.V = V_src; r.ldv = c->ldv; r.n = c->n; r.mu = mu_src; r.s2 = s2_src; r.m = m; r.p = p;
            r.work = rwork; r.work_doubles = ital_gp_remove_workspace(cap); r.status = st;
            const int rc = ital_gp_remove(&r, stream);
            if (rc) return rc;
            m--;
        }
    }
    std::vector<double> pad;
    int rc = ital_compact_rows(c->X, c->xn, c->n, ldx, ITAL_INGEST_F64, keep_d, n_keep, X, xn, st, stream);
    if (!rc) rc = ital_compact_cols(V_src, c->ldv, m, mu_src, s2_src, c->n, keep_d, n_keep, V, ldv, cap, mu, s2, st, stream);
    if (rc) return rc;
    if (pad_s2(s2, n_keep, ldv, c->var, pad, stream)) return ital_fail(-5, "ital_ctx_remove_rows: upload failed");
    int flagged = 0;
    if (hipMemcpyAsync(&flagged, st, sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_remove_rows: stream error");
    if (flagged) {
        char msg[256];
        snprintf(msg, sizeof(msg), "ital_ctx_remove_rows: the kernels flagged the call (status %d): a surviving row's index outside "
                 "the rows (ital_compact_rows / ital_compact_cols), or a factor that was broken before (ital_gp_remove)", flagged);
        return ital_fail(-22, msg);
    }
    // the swap: nothing can fail from here on
    for (void* p : {(void*)c->X, (void*)c->xn, (void*)c->V, (void*)c->mu, (void*)c->s2, (void*)c->C}) dfree(c, p);
    if (!pos.empty()) {
        for (void* p : {(void*)c->L, (void*)c->alpha, (void*)c->XT, (void*)c->XTn}) dfree(c, p);
        c->L = L; c->alpha = alpha; c->XT = XT; c->XTn = XTn; c->rwork = rwork;
    }
    drop_row_scratch(c);
    nw.keep();
    c->X = X; c->xn = xn; c->V = V; c->mu = mu; c->s2 = s2; c->C = C;
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
    c->n = n_keep; c->ldv = ldv;
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
    Fresh nw(c, stream), tmp(c, stream);
    double* s2 = nw.get<double>(ldv);
    if (m == 0) {
        // prior: mean 0, variance var (ital_ctx_fit)
        std::vector<double> prior((size_t)ldv, v);
        if (!nw.ok) return ital_fail(-12, "ital_ctx_set_params: out of device memory");
        if (hipMemcpyAsync(s2, prior.data(), prior.size() * sizeof(double), hipMemcpyHostToDevice, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            return ital_fail(-5, "ital_ctx_set_params: upload failed");
        dfree(c, c->s2);
        nw.keep();
        c->s2 = s2;
        c->length_scale = ls; c->var = v; c->noise = nz;
        return 0;
    }
    double* L = nw.get<double>((size_t)cap * cap);
    double* alpha = nw.get<double>(cap);
    double* V = nw.get<double>((size_t)cap * ldv);
    double* mu = nw.get<double>(ldv);
    double* xn = nw.get<double>(std::max<int64_t>(n, 1));
    double* yd = tmp.get<double>(m);
    int* st = tmp.get<int>(1);
    if (!nw.ok || !tmp.ok) return ital_fail(-12, "ital_ctx_set_params: out of device memory");
    if (hipMemcpyAsync(yd, c->ylab.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice, stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_set_params: upload of the labels failed");
    for (int c0 = 0; c0 < m; c0 += 16) {
        const int rc = ital_chol_append(c->XT, c->XTn, c->ldx, L, cap, alpha, yd + c0, c0, std::min(16, m - c0), v, ls, nz, st, stream);
        if (rc) return rc;
    }
    std::vector<double> pad;
    int rc = whiten(c, c->X, n, L, alpha, m, v, ls, xn, V, ldv, mu, s2, stream);
    if (rc) return rc;
    if (pad_s2(s2, n, ldv, v, pad, stream)) return ital_fail(-5, "ital_ctx_set_params: upload failed");
    int flagged = 0;
    if (hipMemcpyAsync(&flagged, st, sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_set_params: stream error");
    if (flagged & 1)
        return ital_fail(-33, "ital_ctx_set_params: kernel matrix of the labelled samples is not positive definite with these "
                              "parameters (the context keeps its own)");
    for (void* p : {(void*)c->L, (void*)c->alpha, (void*)c->V, (void*)c->mu, (void*)c->s2, (void*)c->xn}) dfree(c, p);
    nw.keep();
    c->L = L; c->alpha = alpha; c->V = V; c->mu = mu; c->s2 = s2; c->xn = xn;
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
    Fresh tmp(c, stream);
    double* yd = tmp.get<double>(m);
    double* pd = tmp.get<double>((size_t)G * 3);
    double* K = tmp.get<double>((size_t)chunk * m * m);
    double* work = tmp.get<double>((size_t)need);
    int* info = tmp.get<int>(chunk);
    int* st = tmp.get<int>(1);                       // the call's own word: the context's is not touched
    double* sc = tmp.get<double>((size_t)chunk * 3);
    double* lm = tmp.get<double>((size_t)chunk * m);
    double* lv = tmp.get<double>((size_t)chunk * m);
    if (!tmp.ok) return ital_fail(-12, "ital_ctx_evidence: out of device memory");
    if (hipMemcpyAsync(yd, c->ylab.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipMemcpyAsync(pd, params, (size_t)G * 3 * sizeof(double), hipMemcpyHostToDevice, stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_evidence: upload of the labels and candidates failed");
    ital_evidence_desc d;
    memset(&d, 0, sizeof(d));
    d.XT = c->XT; d.XTn = c->XTn; d.ldx = c->ldx; d.y = yd; d.m = m; d.K = K; d.ld = m; d.scores = sc; d.info = info;
    d.loo_mean = lm; d.loo_var = lv; d.ldm = m; d.status = st; d.work = work; d.work_doubles = need; d.ev = nullptr;
    std::vector<int> info_h((size_t)chunk);
    for (int g0 = 0; g0 < G; g0 += chunk) {
        const int cc = std::min(chunk, G - g0);
        d.params = pd + (size_t)3 * g0;
        d.G = cc;
        const int rc = ital_gp_evidence(&d, stream);
        if (rc) return rc;
        if (hipMemcpyAsync(scores + (size_t)3 * g0, sc, (size_t)cc * 3 * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipMemcpyAsync(info_h.data(), info, (size_t)cc * sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)       // (the chunk's buffers are free again)
            return ital_fail(-5, "ital_ctx_evidence: download of the scores failed");
        for (int g = 0; g < cc; g++) ok[g0 + g] = info_h[(size_t)g] == 0;
    }
    return 0;
}
