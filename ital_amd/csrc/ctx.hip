// Context-style entry points of the C ABI (ital_ctx_create / _fit / _update / _fetch / ...): a learner
// whose device buffers the LIBRARY owns, for hosts that do not want to manage the ~20 buffers of the descriptor API
// themselves (tests/host_gpu_driver.cpp is that host; ital_amd's own Python learners stay on the descriptor API, whose
// buffers are torch tensors).  Everything here is host code over the descriptor entry points of this same library: the
// perfect-user path of ITAL -- fit, update (Cholesky append + whitening sweep), fetch_unlabelled(k <= 8) with full
// sign-pattern enumeration, predict_stored -- on one rank, or on several with one ncclAllGather of a record per greedy step
// (ital_select_local -> ital_select_exchange -> ital_select_resolve).
//
// Reference: ital/retrieval_base.py:34-61 (fit / reset), :105-126 (update), ital/ital.py:84-134 (fetch_unlabelled),
// ital/gp.py:141-232 (fit / update / predict_stored).
//
// Beyond the perfect user (include/ital_ctx.h): a user model (ital_ctx_set_model) routes the rounds as ITAL._select /
// _fetch_generic do in ital_amd/ital.py -- the lattice scorer for the perfect user with its fall-back to the general scorer,
// ital_score_generic for every other model, with or without a change-estimation subset; a caller-given candidate list
// (ital_ctx_fetch_list); MCMI_min (ital_ctx_mcmi_fetch, ital_amd/mcmi.py); top_results and predict at external points.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <unordered_map>
#include <vector>

#include "ctx_internal.h"
#include "ital_ctx.h"
#include "ital_hip.h"
#include "ital_internal.h"
#include "ital_revoke.h"

namespace {

constexpr int64_t kQworkCap = (int64_t)1 << 27;   // doubles: the 1 GiB cap of the lattice / pipeline workspace
constexpr int64_t kPredictChunk = 4096;           // external points per ital_predict call (bounds Vt)

// Rank holding global row gi: rows [n r / w, n (r + 1) / w) (ital_amd.sharding.row_range).
int owner_of(const ital_ctx* c, int64_t gi) {
    int owner = 0;
    while (owner + 1 < c->world && c->n_total * (owner + 1) / c->world <= gi) owner++;
    return owner;
}

// All unlabelled samples, ascending: the candidate list of a fetch that is given none.
std::vector<int64_t> unlabelled(const ital_ctx* c) {
    std::vector<int64_t> list;
    list.reserve((size_t)(c->n_total - c->n_seen));
    for (int64_t i = 0; i < c->n_total; i++)
        if (!c->seen[(size_t)i]) list.push_back(i);
    return list;
}

// The device status word, read and written by blocking copies.
int read_status(const ital_ctx* c, int* s) {
    return hipMemcpy(s, c->status, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess ? 0 : ital_fail(-5, "ital_ctx_fetch: stream error");
}
int write_status(ital_ctx* c, int s) {
    return hipMemcpy(c->status, &s, sizeof(int), hipMemcpyHostToDevice) == hipSuccess ? 0 : ital_fail(-5, "ital_ctx_fetch: stream error");
}

// A host table into a buffer of its own, by a blocking copy (the stream tables: made once per context).
template <class T>
int upload_table(DevBuf<T>& buf, const std::vector<T>& host) {
    if (!buf.alloc((int64_t)host.size())) return ital_fail(-12, "ital_ctx_fetch: out of device memory");
    if (hipMemcpy(buf, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
        return ital_fail(-5, "ital_ctx_fetch: upload of the stream tables failed");
    return 0;
}

}  // namespace

extern "C" int ital_ctx_destroy(ital_ctx* c) {
    if (!c) return 0;
    (void)hipDeviceSynchronize();
    delete c;
    return 0;
}

extern "C" int ital_ctx_create(int64_t n_total, int d, double length_scale, double var, double noise, int capacity, int rank,
                               int world, void* nccl_comm, ital_ctx** out) {
    if (!out) return ital_fail(-22, "ital_ctx_create: out missing");
    *out = nullptr;
    if (n_total < 1 || d < 1 || world < 1 || rank < 0 || rank >= world || !(length_scale > 0) || !(var > 0) || !(noise >= 0))
        return ital_fail(-22, "ital_ctx_create: bad arguments");
    if (world > 1 && !nccl_comm) return ital_fail(-22, "ital_ctx_create: several ranks need this rank's ncclComm_t");
    ital_ctx* c = new ital_ctx();
    c->n_total = n_total;
    c->row0 = n_total * rank / world;                      // contiguous row blocks (ital_amd.sharding.row_range)
    c->row1 = n_total * (rank + 1) / world;
    c->n = c->row1 - c->row0;
    c->d = d;
    c->ldx = pad16(d);
    c->ldv = pad16(std::max<int64_t>(c->n, 1));
    c->cap = pad16(capacity > 0 ? capacity : 256);
    c->length_scale = length_scale; c->var = var; c->noise = noise;
    c->rank = rank; c->world = world; c->comm = nccl_comm;
    ital_state st;
    if (!st.alloc(*c, ALL)) {
        ital_ctx_destroy(c);
        return ital_fail(-12, "ital_ctx_create: out of device memory");
    }
    c->commit(*c, std::move(st));
    c->seen.assign((size_t)n_total, 0);
    ital_mvn_seed(c->mvn_state);
    *out = c;
    return 0;
}

// This rank's rows [row0, row1) of the n_total x d matrix, row-major with leading dimension d; host memory, or device memory
// when on_device != 0.  Resets the labelled set (reference retrieval_base.py:34-61).
extern "C" int ital_ctx_fit(ital_ctx* c, const double* rows, int on_device, hipStream_t stream) {
    if (!c || (!rows && c->n > 0)) return ital_fail(-22, "ital_ctx_fit: bad arguments");
    if (c->n > 0 && !copy_rows(c->X, c->ldx, rows, c->d, c->n, on_device != 0, stream))
        return ital_fail(-5, "ital_ctx_fit: copy of the rows failed");
    if (c->n > 0) {
        const int rc = ital_row_norms(c->X, c->n, c->ldx, c->xn, stream);
        if (rc) return rc;
    }
    // prior: mean 0, variance var; no labelled sample
    if (hipMemsetAsync(c->mu, 0, (size_t)c->ldv * sizeof(double), stream) != hipSuccess) return ital_fail(-5, "ital_ctx_fit: memset failed");
    std::vector<double> v;
    if (!fill_var(c->s2, 0, c->ldv, c->var, v, stream) || hipStreamSynchronize(stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_fit: upload failed");
    (void)hipMemsetAsync(c->status, 0, sizeof(int), stream);
    c->m = 0;
    std::fill(c->seen.begin(), c->seen.end(), 0);
    c->n_seen = 0;
    c->order.clear();
    c->ylab.clear();
    c->last_picks.clear();
    c->fitted = true;
    return 0;
}

// Labels c_new samples (global indices idx, labels y = +-1): rank-c Cholesky append + whitened rows + refresh of the means and
// variances (reference retrieval_base.py:105-126, gp.py:164-200).  The feature rows come from this rank's own rows, or --
// several ranks -- from the replicated batch state when the samples are (a subset of) the batch just fetched, which is the
// retrieval loop; anything else on several ranks is -38.
extern "C" int ital_ctx_update(ital_ctx* c, const int64_t* idx, const double* y, int c_new, hipStream_t stream) {
    if (!c || !c->fitted || !idx || !y || c_new < 1) return ital_fail(-22, "ital_ctx_update: bad arguments");
    if (c->m + c_new > c->cap) return ital_fail(-12, "ital_ctx_update: labelled-set capacity exceeded (ital_ctx_create: capacity)");
    for (int j = 0; j < c_new; j++) {
        if (idx[j] < 0 || idx[j] >= c->n_total) return ital_fail(-22, "ital_ctx_update: index outside the data");
        if (c->seen[(size_t)idx[j]]) return ital_fail(-22, "ital_ctx_update: Cannot change feedback once given.");
    }
    bool all_batch = !c->last_picks.empty(), all_local = true;
    std::vector<int> slot(c_new);
    for (int j = 0; j < c_new; j++) {
        const auto it = std::find(c->last_picks.begin(), c->last_picks.end(), idx[j]);
        if (it == c->last_picks.end()) all_batch = false;
        else slot[j] = (int)(it - c->last_picks.begin());
        if (idx[j] < c->row0 || idx[j] >= c->row1) all_local = false;
    }
    // Samples outside the batch just fetched (the first labels of a session: a query) on a communicator: their feature rows
    // are replicated through the exchange the greedy steps use -- one all-gather of a record-sized buffer per sample, the
    // owner contributes the row, everybody keeps the owner's part (the reference slices the rows out of the matrix every
    // worker holds, gp.py:185-190).
    const bool via_comm = !all_batch && c->comm != nullptr;
    if (!all_batch && !all_local && !via_comm)
        return ital_fail(-38, "ital_ctx_update: rows of other ranks need the communicator (ital_ctx_create: nccl_comm)");
    const int rec_len = record_len(c);
    for (int j0 = 0; j0 < c_new; j0 += 16) {
        const int cc = std::min(16, c_new - j0);
        ital_label_batch lb;
        memset(&lb, 0, sizeof(lb));
        lb.c = cc;
        for (int j = 0; j < cc; j++) {
            lb.slot[j] = all_batch ? slot[j0 + j] : (via_comm ? j : (int)(idx[j0 + j] - c->row0));
            lb.y[j] = y[j0 + j];
        }
        if (via_comm) {
            if (c->stage.ensure((int64_t)16 * c->ldx) < 0) return ital_fail(-12, "ital_ctx_update: out of device memory");
            for (int j = 0; j < cc; j++) {
                const int64_t gi = idx[j0 + j];
                const int owner = owner_of(c, gi);
                if (hipMemsetAsync(c->rec, 0, (size_t)rec_len * sizeof(double), stream) != hipSuccess) return ital_fail(-5, "ital_ctx_update: memset failed");
                if (owner == c->rank &&
                    hipMemcpyAsync(c->rec, c->X + (size_t)(gi - c->row0) * c->ldx, (size_t)c->ldx * sizeof(double), hipMemcpyDeviceToDevice,
                                   stream) != hipSuccess)
                    return ital_fail(-5, "ital_ctx_update: copy of the row failed");
                const int rc_x = ital_select_exchange(c->rec, c->rec_all, rec_len, c->comm, stream);
                if (rc_x) return rc_x;
                if (hipMemcpyAsync(c->stage + (size_t)j * c->ldx, c->rec_all + (size_t)owner * rec_len, (size_t)c->ldx * sizeof(double),
                                   hipMemcpyDeviceToDevice, stream) != hipSuccess)
                    return ital_fail(-5, "ital_ctx_update: copy of the replicated row failed");
            }
        }
        const int m = c->m;
        int rc = ital_stage_labelled(all_batch ? c->batch.XB : (via_comm ? c->stage : c->X), c->ldx, lb, c->XT + (size_t)m * c->ldx, c->XTn + m, c->ybuf, stream);
        if (!rc) rc = ital_chol_append(c->XT, c->XTn, c->ldx, c->L, c->cap, c->alpha, c->ybuf, m, cc, c->var, c->length_scale, c->noise,
                                       c->status, stream);
        if (!rc) rc = ital_whiten_append(c->X, c->xn, c->n, c->ldx, c->XT + (size_t)m * c->ldx, c->XTn + m, cc, c->L + (size_t)m * c->cap,
                                         c->cap, c->L + (size_t)m * c->cap + m, c->alpha + m, c->V, c->ldv, m, c->var, c->length_scale,
                                         c->mu, c->s2, stream);
        if (rc) return rc;
        c->m += cc;
    }
    for (int j = 0; j < c_new; j++) c->seen[(size_t)idx[j]] = 1;
    c->order.insert(c->order.end(), idx, idx + c_new);
    c->ylab.insert(c->ylab.end(), y, y + c_new);
    c->n_seen += c_new;
    c->last_picks.clear();
    return 0;
}

// Takes labels back (include/ital_ctx.h): stands in for the RuntimeError of reference retrieval_base.py:183-189 and the fit
// from scratch on the survivors, reference gp.py:141-161.  One ital_gp_remove per sample, highest position first: those
// sweeps are the shortest and shift nothing below them.
extern "C" int ital_ctx_revoke(ital_ctx* c, const int64_t* idx, int c_rev, hipStream_t stream) {
    if (!c || !c->fitted || !idx || c_rev < 1) return ital_fail(-22, "ital_ctx_revoke: bad arguments");
    std::vector<int> pos(c_rev);
    for (int j = 0; j < c_rev; j++) {
        if (idx[j] < 0 || idx[j] >= c->n_total || !c->seen[(size_t)idx[j]])
            return ital_fail(-22, "ital_ctx_revoke: a sample that has no label");
        const auto it = std::find(c->order.begin(), c->order.end(), idx[j]);
        if (it == c->order.end()) return ital_fail(-22, "ital_ctx_revoke: a sample that has no label");
        pos[j] = (int)(it - c->order.begin());
    }
    std::sort(pos.begin(), pos.end(), [](int a, int b) { return a > b; });
    if (std::adjacent_find(pos.begin(), pos.end()) != pos.end()) return ital_fail(-22, "ital_ctx_revoke: a sample named twice");
    if (c->rwork.ensure(ital_gp_remove_workspace(c->cap)) < 0) return ital_fail(-12, "ital_ctx_revoke: out of device memory");
    for (int p : pos) {
        const ital_remove_desc r = remove_desc(*c, *c, c->m, p, c->rwork, c->status);
        const int rc = ital_gp_remove(&r, stream);
        if (rc) return rc;
        c->seen[(size_t)c->order[(size_t)p]] = 0;
        c->order.erase(c->order.begin() + p);
        c->ylab.erase(c->ylab.begin() + p);
        c->n_seen--;
        c->m--;
    }
    if (hipStreamSynchronize(stream) != hipSuccess) return ital_fail(-5, "ital_ctx_revoke: stream error");
    return 0;
}

namespace {

// This rank's share of a candidate list (global sample indices in list order): the local rows of its entries into c->cand,
// their alive flags set, and -- when they are not one contiguous run of the list (a caller's list on several ranks) -- their
// list positions into c->gpos (ital_amd.sharding.shard_candidates).  *pos_offset: list position of the first one.
int load_list(ital_ctx* c, const std::vector<int64_t>& list, int64_t* nc_out, int64_t* pos_offset, const int64_t** gpos_out,
              hipStream_t stream) {
    std::vector<int32_t> rows;
    std::vector<int64_t> pos;
    for (int64_t p = 0; p < (int64_t)list.size(); p++)
        if (list[(size_t)p] >= c->row0 && list[(size_t)p] < c->row1) {
            rows.push_back((int32_t)(list[(size_t)p] - c->row0));
            pos.push_back(p);
        }
    const int64_t nc = (int64_t)rows.size();
    const bool contiguous = nc == 0 || pos.back() - pos.front() == nc - 1;
    // (sized for all of this rank's rows at once: grows at most once per context)
    const int64_t room = nc > 0 ? std::max<int64_t>(nc, c->n) : 0;
    int rc = grow(stream, "ital_ctx_fetch: out of device memory", want(c->cand, room), want(c->alive, room), want(c->mi, room));
    if (rc >= 0 && !contiguous) rc = grow(stream, "ital_ctx_fetch: out of device memory", want(c->gpos, room));
    if (rc < 0) return rc;
    if (nc > 0 && (hipMemcpyAsync(c->cand, rows.data(), nc * sizeof(int32_t), hipMemcpyHostToDevice, stream) != hipSuccess ||
                   hipMemsetAsync(c->alive, 1, nc, stream) != hipSuccess ||
                   (!contiguous && hipMemcpyAsync(c->gpos, pos.data(), nc * sizeof(int64_t), hipMemcpyHostToDevice, stream) != hipSuccess)))
        return ital_fail(-5, "ital_ctx_fetch: upload of the candidate list failed");
    if (hipStreamSynchronize(stream) != hipSuccess) return ital_fail(-5, "ital_ctx_fetch: stream error");   // (rows, pos leave scope)
    *nc_out = nc;
    *pos_offset = nc > 0 ? pos.front() : 0;
    *gpos_out = contiguous ? nullptr : c->gpos.p;
    return 0;
}

// Grows everything whose size follows the batch capacity kmax -- the cross-covariance rows C, the batch state, the picks and
// the selection records -- to `kmax` (general-scorer rounds: batches up to ITAL_GENERIC_MAX_REL, a change-estimation subset
// plus the picks up to ITAL_GENERIC_MAX_DIM rows of C).  The rows of the last batch go with the old batch state.
int ensure_kmax(ital_ctx* c, int kmax, hipStream_t stream) {
    if (kmax <= c->kmax) return 0;
    ital_dims nd = *c;
    nd.kmax = kmax;
    ital_state nw;
    if (!drain(stream)) return ital_fail(-5, "ital_ctx: stream error");
    if (!nw.alloc(nd, BY_KMAX)) return ital_fail(-12, "ital_ctx_fetch: out of device memory (batch state)");
    c->last_picks.clear();
    c->commit(nd, std::move(nw));
    return 0;
}

// The lattice scorer's workspace (ital_round_workspace) or the general scorer's pipeline workspace: grown to `doubles`.
int ensure_qwork(ital_ctx* c, int64_t doubles, hipStream_t stream) {
    const int rc = grow(stream, "ital_ctx_fetch: out of device memory (workspace)", want(c->qwork, doubles));
    return rc < 0 ? rc : 0;
}

// Selection of greedy step t (member slot t - 1) out of the scores c->mi: arg-max, record, append to the batch state.
int select_step(ital_ctx* c, int t, int64_t nc, int64_t pos_offset, const int64_t* gpos, hipStream_t stream) {
    const int rec_len = record_len(c);
    if (c->world == 1 && !c->comm)
        return ital_select_fused(c->mi, c->cand, c->alive, nc, pos_offset, gpos, c->row0, c->rank, 0, c->mu, c->s2, c->X, c->xn,
                                 c->ldx, c->V, c->ldv, c->m, c->cap, c->C, c->ldv, t - 1, t - 1, c->batch, c->status, c->rec, c->ret,
                                 stream);
    int rc = ital_select_local(c->mi, c->cand, c->alive, nc, pos_offset, gpos, c->row0, c->rank, 0, c->mu, c->s2, c->X, c->xn,
                               c->ldx, c->V, c->ldv, c->m, c->cap, c->C, c->ldv, t - 1, c->kmax, c->status, c->work3k, c->rec,
                               stream);
    if (!rc) rc = ital_select_exchange(c->rec, c->rec_all, rec_len, c->comm, stream);
    if (!rc) rc = ital_select_resolve(c->rec_all, c->world, rec_len, c->rank, 0, t - 1, c->batch, c->alive, c->ret, stream);
    return rc;
}

// Cross-covariance row of batch member `slot` with every row (the next greedy step's C[slot]).
int member_column(ital_ctx* c, int slot, hipStream_t stream) {
    return ital_cross_cov_cols(c->X, c->xn, c->n, c->ldx, c->batch.XB + (size_t)slot * c->ldx, c->batch.XBn + slot, 1,
                               c->batch.VB + (size_t)slot * c->cap, c->cap, c->V, c->ldv, c->m, c->var, c->length_scale,
                               c->C + (size_t)slot * c->ldv, c->ldv, stream);
}

// ret[0 .. kmax] of the round (picks, status word) to the host.
int download_ret(ital_ctx* c, std::vector<int64_t>& host, hipStream_t stream) {
    host.assign((size_t)c->kmax + 1, 0);
    if (hipMemcpyAsync(host.data(), c->ret, host.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_fetch: download of the picks failed");
    return 0;
}

// k greedy steps of the perfect user on the lattice scorer (ital_score_step, full enumeration of the 2^t sign patterns) over
// the list loaded by load_list (n_list entries on all ranks); ret -> host.  (ital_amd/ital.py: ITAL._select)
int lattice_round(ital_ctx* c, int k, int64_t nc, int64_t pos_offset, const int64_t* gpos, int64_t n_list, int label_mode,
                  std::vector<int64_t>& host, hipStream_t stream) {
    // the lattice scorer's workspace, ONCE for the whole round: what its largest step (t = k) needs, capped at 1 GiB (slabs
    // beyond) -- ital_round_workspace is documented for exactly this (sized per step, each of the steps t = 3 .. k would grow it
    // again).
    if (k >= 3) {
        const int rc = ensure_qwork(c, ital_round_workspace(k, std::max<int64_t>(nc, 1), kQworkCap), stream);
        if (rc) return rc;
    }
    (void)hipMemsetAsync(c->ret, 0, (c->kmax + 1) * sizeof(int64_t), stream);
    int64_t n_alive = n_list;
    for (int t = 1; t <= k; t++) {
        ital_score_desc desc;
        memset(&desc, 0, sizeof(desc));
        desc.t = t; desc.n_cand = nc; desc.cand = c->cand; desc.alive = c->alive; desc.mu = c->mu; desc.s2 = c->s2;
        desc.C = c->C; desc.ldc = c->ldv; desc.row_offset = c->row0; desc.pos_offset = pos_offset; desc.gpos = gpos;
        desc.batch = c->batch; desc.noise = c->noise; desc.eps = 1e-12; desc.label_mode = label_mode; desc.mi = c->mi;
        desc.status = c->status;
        if (t >= 3) {
            if (!c->jump[t]) {
                std::vector<long long> jump((size_t)ITAL_JUMP_BITS * 18), pat((size_t)(1 << t) * 18);
                std::vector<double> vk(t - 1);
                int rc = ital_mvn_tables(t, jump.data(), pat.data(), vk.data());
                if (rc) return rc;
                DevBuf<long long> d_jump, d_pat;
                DevBuf<double> d_vk;
                if ((rc = upload_table(d_jump, jump)) || (rc = upload_table(d_pat, pat)) || (rc = upload_table(d_vk, vk))) return rc;
                c->jump[t] = std::move(d_jump); c->jumppat[t] = std::move(d_pat); c->vk[t] = std::move(d_vk);
            }
            desc.jump = c->jump[t]; desc.jumppat = c->jumppat[t]; desc.vk = c->vk[t];
            desc.work = c->qwork; desc.work_doubles = c->qwork.count;
            for (int j = 0; j < 6; j++) desc.seed[j] = c->mvn_state[j];
        }
        int rc = nc > 0 ? ital_score_step(&desc, stream) : 0;
        if (!rc) rc = select_step(c, t, nc, pos_offset, gpos, stream);
        if (!rc && t < k) rc = member_column(c, t - 1, stream);
        if (rc) return rc;
        // the serial reference has now made 2 * 2^t mvndst calls per live candidate of the WHOLE list (ital.py:191-206)
        ital_mvn_advance(c->mvn_state, n_alive * (int64_t)(2 << t) * ital_mvn_draws_per_call(t));
        n_alive--;
    }
    return download_ret(c, host, stream);
}

bool perfect_user(const ital_ctx_model& m) { return m.label_prob >= 1 && m.mistake_prob <= 0; }

// fb_mode of ital_gscore_desc (ITAL._fb_mode): 0 perfect user, 1 label_prob >= 1 with mistakes, 2 general.
int fb_mode_of(const ital_ctx_model& m) { return perfect_user(m) ? 0 : (m.label_prob >= 1 ? 1 : 2); }

// Sign patterns and simulated feedback configurations per pattern at a step with nr enumerated variables, full enumeration
// (ITAL._mc_plan without the Monte-Carlo switches).
void enum_plan(int nr, int fb_mode, int64_t* npat, int64_t* nfb) {
    *npat = (int64_t)1 << nr;
    int64_t p3 = 1;
    for (int i = 0; i < nr; i++) p3 *= 3;
    *nfb = fb_mode == 0 ? 1 : (fb_mode == 1 ? (int64_t)1 << nr : p3 - 1);
}

// Device tables of the general scorer (ITAL._fetch_generic: jump1, vk_all, iota, zero64), made once per context.
int generic_tables(ital_ctx* c) {
    if (c->jump1) return 0;
    const int GN = ITAL_GENERIC_MAX_DIM;
    std::vector<long long> jump1((size_t)ITAL_JUMP_BITS * 18);
    std::vector<double> vk((size_t)(GN + 1) * GN);
    std::vector<int32_t> iota(64);
    for (int i = 0; i < 64; i++) iota[(size_t)i] = i;
    int rc = ital_mvn_generic_tables(GN, jump1.data(), vk.data());
    if (rc) return rc;
    DevBuf<long long> d_jump1;                                  // (c->jump1 says that all four are there)
    if ((rc = upload_table(d_jump1, jump1)) || (rc = upload_table(c->vk_all, vk)) || (rc = upload_table(c->iota, iota))) return rc;
    if (!c->zero64.alloc(1)) return ital_fail(-12, "ital_ctx_fetch: out of device memory");
    c->jump1 = std::move(d_jump1);
    return 0;
}

// The fields of a general-scorer step that do not depend on the base set.
void gscore_common(const ital_ctx* c, ital_gscore_desc& d, int64_t nc, int64_t pos_offset, const int64_t* gpos, int fb_mode) {
    memset(&d, 0, sizeof(d));
    d.n_cand = nc; d.cand = c->cand; d.alive = c->alive; d.mu = c->mu; d.s2 = c->s2; d.C = c->C; d.ldc = c->ldv;
    d.row_offset = c->row0; d.pos_offset = pos_offset; d.gpos = gpos;
    d.fb_mode = fb_mode; d.label_prob = c->model.label_prob; d.mistake_prob = c->model.mistake_prob;
    d.label_mode = c->model.label_estimation; d.noise = c->noise; d.eps = 1e-12; d.clip_cov = 0;
    for (int j = 0; j < 6; j++) d.seed[j] = c->mvn_state[j];
    d.jump1 = c->jump1; d.vk = c->vk_all; d.mi = c->mi; d.status = c->status;
}

// The pipeline's workspace for the step of `d` (all candidates in one slab, capped at 1 GiB) when it runs as the pipeline.
int gscore_workspace(ital_ctx* c, ital_gscore_desc& d, hipStream_t stream) {
    const int64_t want = std::min<int64_t>(ital_score_generic_workspace(&d), kQworkCap);
    const int rc = ensure_qwork(c, want, stream);
    if (rc) return rc;
    d.work = c->qwork; d.work_doubles = c->qwork.count;
    return 0;
}

// k greedy steps on the general scorer with the device batch state as the base set (ITAL._fetch_generic without a subset and
// without the Monte-Carlo switches, ital_amd/ital.py:702-1050): no host round trip until the picks; ret -> host.
int generic_round(ital_ctx* c, int k, int64_t nc, int64_t pos_offset, const int64_t* gpos, int64_t n_list,
                  std::vector<int64_t>& host, hipStream_t stream) {
    int rc = generic_tables(c);
    if (rc) return rc;
    const int fb_mode = fb_mode_of(c->model);
    (void)hipMemsetAsync(c->ret, 0, (c->kmax + 1) * sizeof(int64_t), stream);
    int64_t n_alive = n_list;
    for (int t = 1; t <= k; t++) {
        const int nE = t - 1, nr = t;
        int64_t npat, nfb;
        enum_plan(nr, fb_mode, &npat, &nfb);
        ital_gscore_desc d;
        gscore_common(c, d, nc, pos_offset, gpos, fb_mode);
        // the base set is the batch so far: members, their order by data index, means, covariances and list positions are
        // the device batch state itself
        d.nE = nE; d.E_idx = c->batch.bidx; d.E_sort = c->batch.bsort; d.E_mu = c->batch.bmu; d.E_sig = c->batch.sig;
        d.ldE = c->kmax; d.n_picks = nE; d.pick_pos = c->iota;
        d.subset_mode = 0;
        d.draws_out = npat * (1 + nfb) * ital_mvn_draws_per_call(nr); d.draws_in = 0;
        d.n_in = 0; d.in_pos = c->zero64; d.n_dead = nE; d.dead_pos = c->batch.bgpos;
        if (nE + 1 <= 16 && (rc = gscore_workspace(c, d, stream))) return rc;
        rc = nc > 0 ? ital_score_generic(&d, stream) : 0;
        if (rc) return rc;
        ital_mvn_advance(c->mvn_state, n_alive * d.draws_out);
        n_alive--;
        rc = select_step(c, t, nc, pos_offset, gpos, stream);
        if (!rc && t < k) rc = member_column(c, t - 1, stream);
        if (rc) return rc;
    }
    return download_ret(c, host, stream);
}

// Record of global sample gi packed by its owner -- [3] mu, [4] s2, [5] |x|^2, the feature row at ITAL_REC_HEADER, its
// whitened column behind it, and (n_cc > 0) C[0 .. n_cc)[gi] behind that -- and replicated: the address of the owner's record
// on this rank (c->rec itself without a communicator).
int share_sample(ital_ctx* c, int64_t gi, int n_cc, const double** out, hipStream_t stream) {
    const int h = ITAL_REC_HEADER, rec_len = record_len(c);
    const int owner = owner_of(c, gi);
    if (hipMemsetAsync(c->rec, 0, (size_t)rec_len * sizeof(double), stream) != hipSuccess) return ital_fail(-5, "ital_ctx_fetch: memset failed");
    if (owner == c->rank) {
        const int64_t l = gi - c->row0;
        bool ok = hipMemcpyAsync(c->rec + 3, c->mu + l, sizeof(double), hipMemcpyDeviceToDevice, stream) == hipSuccess &&
                  hipMemcpyAsync(c->rec + 4, c->s2 + l, sizeof(double), hipMemcpyDeviceToDevice, stream) == hipSuccess &&
                  hipMemcpyAsync(c->rec + 5, c->xn + l, sizeof(double), hipMemcpyDeviceToDevice, stream) == hipSuccess &&
                  hipMemcpyAsync(c->rec + h, c->X + (size_t)l * c->ldx, (size_t)c->ldx * sizeof(double), hipMemcpyDeviceToDevice,
                                 stream) == hipSuccess;
        if (ok && c->m > 0)
            ok = hipMemcpy2DAsync(c->rec + h + c->ldx, sizeof(double), c->V + l, (size_t)c->ldv * sizeof(double), sizeof(double),
                                  (size_t)c->m, hipMemcpyDeviceToDevice, stream) == hipSuccess;
        if (ok && n_cc > 0)
            ok = hipMemcpy2DAsync(c->rec + h + c->ldx + c->cap, sizeof(double), c->C + l, (size_t)c->ldv * sizeof(double),
                                  sizeof(double), (size_t)n_cc, hipMemcpyDeviceToDevice, stream) == hipSuccess;
        if (!ok) return ital_fail(-5, "ital_ctx_fetch: copy of a sample's record failed");
    }
    if (!c->comm) {
        *out = c->rec;
        return 0;
    }
    const int rc = ital_select_exchange(c->rec, c->rec_all, rec_len, c->comm, stream);
    if (rc) return rc;
    *out = c->rec_all + (size_t)owner * rec_len;
    return 0;
}

// Same rule as ital_select_resolve (ital_amd.sharding.winner, mode 0): first maximum over the list positions, NaN first.
int host_winner(const std::vector<double>& recs, int world, int rec_len) {
    int best = -1;
    for (int w = 0; w < world; w++) {
        const double v = recs[(size_t)w * rec_len], p = recs[(size_t)w * rec_len + 1];
        if (p < 0) continue;
        if (best < 0) {
            best = w;
            continue;
        }
        const double bv = recs[(size_t)best * rec_len], bp = recs[(size_t)best * rec_len + 1];
        const bool vn = isnan(v), bn = isnan(bv);
        const bool better = vn != bn ? vn : ((vn || v == bv) ? p < bp : v > bv);
        if (better) best = w;
    }
    return best;
}

// k greedy steps with a change-estimation subset (ITAL._fetch_generic, subset mode, ital_amd/ital.py:743-760, :1008-1040):
// the base set E starts as the subset and grows when a pick lies outside it; that bookkeeping stays on the host (one
// synchronisation per greedy step).  list: the whole candidate list (all ranks), E: the subset in the caller's order.
int subset_round(ital_ctx* c, int k, const std::vector<int64_t>& list, std::vector<int64_t> E, int64_t nc, int64_t pos_offset,
                 const int64_t* gpos, std::vector<int64_t>& picks, hipStream_t stream) {
    int rc = generic_tables(c);
    if (rc) return rc;
    const int h = ITAL_REC_HEADER, rec_len = record_len(c);
    const int fb_mode = fb_mode_of(c->model);
    const int kmax_e = (int)E.size() + k;
    std::unordered_map<int64_t, int64_t> pos_of;
    for (int64_t p = 0; p < (int64_t)list.size(); p++) pos_of[list[(size_t)p]] = p;
    // staging of the base set on the device: E_idx, in_pos, dead_pos [kmax_e] int64, E_mu [kmax_e], E_sig [kmax_e]^2,
    // E_sort, pick_pos [kmax_e] int32
    const int64_t bytes = (int64_t)8 * (4 * kmax_e + (int64_t)kmax_e * kmax_e) + 8 * kmax_e + 64;
    if ((rc = grow(stream, "ital_ctx_fetch: out of device memory", want(c->sub, bytes))) < 0) return rc;
    int64_t* d_eidx = reinterpret_cast<int64_t*>(c->sub.p);
    int64_t* d_in = d_eidx + kmax_e;
    int64_t* d_dead = d_in + kmax_e;
    double* d_emu = reinterpret_cast<double*>(d_dead + kmax_e);
    double* d_esig = d_emu + kmax_e;
    int32_t* d_esort = reinterpret_cast<int32_t*>(d_esig + (size_t)kmax_e * kmax_e);
    int32_t* d_ppos = d_esort + kmax_e;
    std::vector<double> e_mu((size_t)kmax_e, 0.0), e_sig((size_t)kmax_e * kmax_e, 0.0);
    // covariance rows of the subset members with every row, then their covariances among themselves (C[a][E[b]]) and means
    const int n0 = (int)E.size();
    for (int j = 0; j < n0; j++) {
        const double* r = nullptr;
        if ((rc = share_sample(c, E[(size_t)j], 0, &r, stream))) return rc;
        rc = ital_cross_cov_cols(c->X, c->xn, c->n, c->ldx, r + h, r + 5, 1, r + h + c->ldx, c->cap, c->V, c->ldv, c->m, c->var,
                                 c->length_scale, c->C + (size_t)j * c->ldv, c->ldv, stream);
        if (rc) return rc;
    }
    std::vector<double> col((size_t)rec_len);
    for (int b = 0; b < n0; b++) {
        const double* r = nullptr;
        if ((rc = share_sample(c, E[(size_t)b], n0, &r, stream))) return rc;
        if (hipMemcpyAsync(col.data(), r, (size_t)rec_len * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            return ital_fail(-5, "ital_ctx_fetch: download of the subset's covariances failed");
        e_mu[(size_t)b] = col[3];
        for (int a = 0; a < n0; a++) e_sig[(size_t)a * kmax_e + b] = col[(size_t)(h + c->ldx + c->cap + a)];
    }
    std::vector<int32_t> pick_pos;
    std::vector<double> recs((size_t)c->world * rec_len);
    int64_t n_alive = (int64_t)list.size();
    for (int t = 1; t <= k; t++) {
        const int nE = (int)E.size(), nr = t;
        int64_t npat, nfb;
        enum_plan(nr, fb_mode, &npat, &nfb);
        const int64_t draws_out = npat * (ital_mvn_draws_per_call(nr) + (1 + nfb) * ital_mvn_draws_per_call(nE + 1));
        const int64_t draws_in = npat * (ital_mvn_draws_per_call(nr) + (1 + nfb) * ital_mvn_draws_per_call(nE));
        std::vector<int64_t> in_pos, dead_pos;
        for (int64_t e : E)
            if (pos_of.count(e) && std::find(picks.begin(), picks.end(), e) == picks.end()) in_pos.push_back(pos_of[e]);
        std::sort(in_pos.begin(), in_pos.end());
        for (int64_t q : picks) dead_pos.push_back(pos_of[q]);
        std::vector<int32_t> esort((size_t)nE);
        for (int i = 0; i < nE; i++) esort[(size_t)i] = i;
        std::stable_sort(esort.begin(), esort.end(), [&](int32_t a, int32_t b) { return E[(size_t)a] < E[(size_t)b]; });
        bool ok = hipMemcpyAsync(d_eidx, E.data(), nE * sizeof(int64_t), hipMemcpyHostToDevice, stream) == hipSuccess &&
                  hipMemcpyAsync(d_esort, esort.data(), nE * sizeof(int32_t), hipMemcpyHostToDevice, stream) == hipSuccess &&
                  hipMemcpyAsync(d_emu, e_mu.data(), e_mu.size() * sizeof(double), hipMemcpyHostToDevice, stream) == hipSuccess &&
                  hipMemcpyAsync(d_esig, e_sig.data(), e_sig.size() * sizeof(double), hipMemcpyHostToDevice, stream) == hipSuccess;
        if (ok && !pick_pos.empty())
            ok = hipMemcpyAsync(d_ppos, pick_pos.data(), pick_pos.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream) == hipSuccess;
        if (ok && !in_pos.empty())
            ok = hipMemcpyAsync(d_in, in_pos.data(), in_pos.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream) == hipSuccess;
        if (ok && !dead_pos.empty())
            ok = hipMemcpyAsync(d_dead, dead_pos.data(), dead_pos.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream) == hipSuccess;
        if (!ok) return ital_fail(-5, "ital_ctx_fetch: upload of the base set failed");
        ital_gscore_desc d;
        gscore_common(c, d, nc, pos_offset, gpos, fb_mode);
        d.nE = nE; d.E_idx = d_eidx; d.E_sort = d_esort; d.E_mu = d_emu; d.E_sig = d_esig; d.ldE = kmax_e;
        d.n_picks = (int)picks.size(); d.pick_pos = d_ppos;
        d.subset_mode = 1;
        d.draws_out = draws_out; d.draws_in = draws_in;
        d.n_in = (int)in_pos.size(); d.in_pos = d_in; d.n_dead = (int)dead_pos.size(); d.dead_pos = d_dead;
        if (nE + 1 <= 13 && (rc = gscore_workspace(c, d, stream))) return rc;
        rc = nc > 0 ? ital_score_generic(&d, stream) : 0;
        if (rc) return rc;
        const int64_t n_in_alive = (int64_t)in_pos.size();
        ital_mvn_advance(c->mvn_state, (n_alive - n_in_alive) * draws_out + n_in_alive * draws_in);
        n_alive--;
        // the winner is resolved on the host: it may or may not extend the base set
        rc = ital_select_local(c->mi, c->cand, c->alive, nc, pos_offset, gpos, c->row0, c->rank, 0, c->mu, c->s2, c->X, c->xn,
                               c->ldx, c->V, c->ldv, c->m, c->cap, c->C, c->ldv, nE, c->kmax, c->status, c->work3k, c->rec, stream);
        if (!rc && c->comm) rc = ital_select_exchange(c->rec, c->rec_all, rec_len, c->comm, stream);
        if (rc) return rc;
        const double* recs_d = c->comm ? c->rec_all : c->rec;
        const int nrec = c->comm ? c->world : 1;
        if (hipMemcpyAsync(recs.data(), recs_d, (size_t)nrec * rec_len * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            return ital_fail(-5, "ital_ctx_fetch: download of the records failed");
        const int w = host_winner(recs, nrec, rec_len);
        if (w < 0) return ital_fail(-5, "ital_ctx_fetch: no rank had a live candidate");
        const double* rec = recs.data() + (size_t)w * rec_len;
        const int64_t pick = (int64_t)rec[2];
        if ((int)rec[6] == c->rank && hipMemsetAsync(c->alive + (int64_t)rec[7], 0, 1, stream) != hipSuccess)
            return ital_fail(-5, "ital_ctx_fetch: memset failed");
        picks.push_back(pick);
        const auto in_e = std::find(E.begin(), E.end(), pick);
        if (in_e != E.end()) {
            pick_pos.push_back((int32_t)(in_e - E.begin()));
            continue;
        }
        // new member of the base set: its covariance row, mean and covariances with the members so far
        e_mu[(size_t)nE] = rec[3];
        e_sig[(size_t)nE * kmax_e + nE] = rec[4];
        for (int a = 0; a < nE; a++) {
            e_sig[(size_t)nE * kmax_e + a] = rec[h + c->ldx + c->cap + a];
            e_sig[(size_t)a * kmax_e + nE] = rec[h + c->ldx + c->cap + a];
        }
        if (t < k) {
            const double* rd = recs_d + (size_t)w * rec_len;
            rc = ital_cross_cov_cols(c->X, c->xn, c->n, c->ldx, rd + h, rd + 5, 1, rd + h + c->ldx, c->cap, c->V, c->ldv, c->m,
                                     c->var, c->length_scale, c->C + (size_t)nE * c->ldv, c->ldv, stream);
            if (rc) return rc;
        }
        pick_pos.push_back(nE);
        E.push_back(pick);
    }
    return hipStreamSynchronize(stream) == hipSuccess ? 0 : ital_fail(-5, "ital_ctx_fetch: stream error");
}

// Status word of a round: bit 1 (Cholesky append) and bit 2 (orthant integrator) end it (ital_amd.gp.check_status).
int round_status(int64_t st, const char* who) {
    char msg[256];
    if (st & 1) {
        snprintf(msg, sizeof(msg), "%s: kernel matrix of the labelled samples is not positive definite", who);
        return ital_fail(-33, msg);
    }
    if (st & 2) {
        snprintf(msg, sizeof(msg), "%s: singular conditional covariance in the orthant integrator (duplicate samples in the batch?)", who);
        return ital_fail(-33, msg);
    }
    return 0;
}

// Checks a caller's list of global sample indices: inside the data, unlabelled, no repeats (-22).
int check_list(const ital_ctx* c, const int64_t* v, int64_t n, const char* who, const char* what) {
    std::vector<uint8_t> mark((size_t)c->n_total, 0);
    char msg[256];
    for (int64_t i = 0; i < n; i++) {
        const int64_t g = v[i];
        const char* why = (g < 0 || g >= c->n_total) ? "an index outside the data"
                          : c->seen[(size_t)g]        ? "a labelled sample"
                          : mark[(size_t)g]           ? "a repeated sample"
                                                      : nullptr;
        if (why) {
            snprintf(msg, sizeof(msg), "%s: %s holds %s (%lld at %lld)", who, what, why, (long long)g, (long long)i);
            return ital_fail(-22, msg);
        }
        mark[(size_t)g] = 1;
    }
    return 0;
}

// ITAL._unsupported for the context's model (ital_amd/ital.py:132-159): why the device scorers cannot run this round, or
// nullptr.  whole_list_subset: the subset is the candidate list itself (change_estimation_subset=None).
const char* unsupported(const ital_ctx* c, int k, int n_subset, bool whole_list_subset, char* buf, size_t len) {
    const bool subset = n_subset > 0;
    const int max_dim = subset ? (whole_list_subset ? n_subset : n_subset + k) : k;
    if (whole_list_subset && n_subset > ITAL_GENERIC_MAX_DIM) {
        snprintf(buf, len, "change_estimation_subset=None with %d candidates: orthants of that dimension (limit %d)", n_subset,
                 ITAL_GENERIC_MAX_DIM);
        return buf;
    }
    if (subset || !perfect_user(c->model)) {
        if (max_dim > ITAL_GENERIC_MAX_DIM) {
            snprintf(buf, len, "orthant dimension %d (subset + batch) above %d", max_dim, ITAL_GENERIC_MAX_DIM);
            return buf;
        }
        if (k > ITAL_GENERIC_MAX_REL) {
            snprintf(buf, len, "batches larger than %d with the general scorer", ITAL_GENERIC_MAX_REL);
            return buf;
        }
        const int fb_mode = fb_mode_of(c->model);
        for (int nr = 1; nr <= k; nr++) {
            int64_t npat, nfb;
            enum_plan(nr, fb_mode, &npat, &nfb);
            if (npat * (2 + nfb) > ITAL_GENERIC_MAX_CALLS) {
                snprintf(buf, len, "%lld orthant probabilities per candidate at greedy step %d: set monte_carlo_num_rel / "
                         "monte_carlo_num_fb (reference ital.py:293-297)", (long long)(npat * (2 + nfb)), nr);
                return buf;
            }
        }
    } else if (k > ITAL_MAX_T) {
        snprintf(buf, len, "batches larger than %d with full enumeration: set monte_carlo_num_rel (reference ital.py:293-297)",
                 ITAL_MAX_T);
        return buf;
    }
    return nullptr;
}

// fetch_unlabelled(k) with the context's model over `cand` (NULL: all unlabelled samples ascending), optionally with a
// change-estimation subset: ITAL.fetch_unlabelled -> _select / _fetch_generic (ital_amd/ital.py:223-253, :300-421, :702-1050).
int model_fetch(ital_ctx* c, const char* who, int k, const int64_t* cand, int64_t n_cand, const int64_t* subset, int n_subset,
                int64_t* picks, hipStream_t stream) {
    char msg[320];
    if (!c || !c->fitted || !picks || n_subset < 0 || (n_subset > 0 && !subset) || (cand && n_cand < 0)) {
        snprintf(msg, sizeof(msg), "%s: bad arguments", who);
        return ital_fail(-22, msg);
    }
    if (c->m == 0) {
        snprintf(msg, sizeof(msg), "%s: needs a fitted relevance model: call ital_ctx_update first", who);
        return ital_fail(-22, msg);
    }
    const int64_t n_unseen = c->n_total - c->n_seen;
    if (k > n_unseen) k = (int)n_unseen;
    if (k < 1) return 0;
    std::vector<int64_t> list;
    if (cand) {
        int rc = check_list(c, cand, n_cand, who, "the candidate list");
        if (rc) return rc;
        list.assign(cand, cand + n_cand);
    } else {
        list = unlabelled(c);
    }
    std::vector<int64_t> E;
    bool whole_list = false;
    if (n_subset > 0) {
        int rc = check_list(c, subset, n_subset, who, "the change-estimation subset");
        if (rc) return rc;
        E.assign(subset, subset + n_subset);
        if ((int64_t)n_subset == (int64_t)list.size()) {
            std::vector<int64_t> a(list), b(E);
            std::sort(a.begin(), a.end());
            std::sort(b.begin(), b.end());
            whole_list = a == b;
        }
    }
    char why_buf[256];
    if (const char* why = unsupported(c, k, n_subset, whole_list, why_buf, sizeof(why_buf))) {
        snprintf(msg, sizeof(msg), "%s: %s is not implemented", who, why);
        return ital_fail(-95, msg);
    }
    int rc = ensure_kmax(c, n_subset > 0 ? n_subset + k : k, stream);
    if (rc) return rc;
    c->last_picks.clear();
    // k was clamped to the unlabelled samples BEFORE the list: the reference picks until the list is empty, then np.argmax([])
    // raises (ital.py:130) -- with the random stream advanced by the steps it did run, so those are run here too
    const int steps = (int)std::min<int64_t>(k, (int64_t)list.size());
    const int64_t n_list = (int64_t)list.size();
    std::vector<int64_t> got, host;
    int64_t st = 0;
    if (steps > 0) {
        int64_t nc = 0, pos_offset = 0;
        const int64_t* gpos = nullptr;
        if ((rc = load_list(c, list, &nc, &pos_offset, &gpos, stream))) return rc;
        if (n_subset > 0) {
            if ((rc = subset_round(c, steps, list, E, nc, pos_offset, gpos, got, stream))) return rc;
            int s = 0;
            if ((rc = read_status(c, &s))) return rc;
            st = s;
        } else {
            bool generic = !perfect_user(c->model);
            if (!generic) {
                int saved[6];
                memcpy(saved, c->mvn_state, sizeof(saved));
                if ((rc = lattice_round(c, steps, nc, pos_offset, gpos, n_list, c->model.label_estimation, host, stream))) return rc;
                if (host[(size_t)c->kmax] & 6) {
                    // linearly dependent variables inside the batch (duplicate samples), or a simulated update that does not pin
                    // the labels (large noise): the round again through the general scorer from the same stream position
                    // (ital.py:411-417)
                    int s = 0;
                    if ((rc = read_status(c, &s)) || (rc = write_status(c, s & ~6))) return rc;
                    memcpy(c->mvn_state, saved, sizeof(saved));
                    if ((rc = load_list(c, list, &nc, &pos_offset, &gpos, stream))) return rc;
                    generic = true;
                }
            }
            if (generic && (rc = generic_round(c, steps, nc, pos_offset, gpos, n_list, host, stream))) return rc;
            st = host[(size_t)c->kmax];
            got.assign(host.begin(), host.begin() + steps);
        }
    }
    if (steps < k) {
        snprintf(msg, sizeof(msg), "%s: attempt to get argmax of an empty sequence (k = %d, %lld candidates)", who, k, (long long)n_list);
        return ital_fail(-61, msg);
    }
    if ((rc = round_status(st, who))) return rc;
    if (n_subset == 0) c->last_picks = got;          // (subset mode leaves the batch state alone: update() reads rows itself)
    for (int t = 0; t < k; t++) picks[t] = got[(size_t)t];
    return k;
}

}  // namespace

// fetch_unlabelled(k): the k picks in selection order into picks[0 .. k) (host memory).  Perfect user, full enumeration of
// the 2^t sign patterns (k <= ITAL_MAX_T), candidates = all unlabelled samples in ascending order
// (reference ital.py:84-134, retrieval_base.py:78-87).  Synchronises `stream` (the picks are its result).
// -71: the round met a batch the fast scorer does not cover (duplicate samples, large noise: status bits 2 / 4) -- such a
// round belongs to ital_score_generic, which this layer drives only once a user model is set (ital_ctx_set_model: then the
// round follows ITAL._select, fall-back included).
extern "C" int ital_ctx_fetch(ital_ctx* c, int k, int64_t* picks, hipStream_t stream) {
    if (c && c->has_model) return model_fetch(c, "ital_ctx_fetch", k, nullptr, 0, nullptr, 0, picks, stream);
    if (!c || !c->fitted || !picks) return ital_fail(-22, "ital_ctx_fetch: bad arguments");
    if (c->m == 0) return ital_fail(-22, "ital_ctx_fetch: needs a fitted relevance model: call ital_ctx_update first");
    const int64_t n_unseen = c->n_total - c->n_seen;
    if (k > n_unseen) k = (int)n_unseen;
    if (k < 1) return 0;
    if (k > ITAL_MAX_T) return ital_fail(-22, "ital_ctx_fetch: batches larger than ITAL_MAX_T need the Monte-Carlo switch (ital_score_generic)");
    // candidate list: ascending unseen samples; this rank's share is one run of it
    const std::vector<int64_t> list = unlabelled(c);
    int64_t nc = 0, pos_offset = 0;
    const int64_t* gpos = nullptr;
    std::vector<int64_t> host;
    int rc = load_list(c, list, &nc, &pos_offset, &gpos, stream);
    if (!rc) rc = lattice_round(c, k, nc, pos_offset, gpos, n_unseen, 0, host, stream);
    if (rc) return rc;
    const int64_t st = host[(size_t)c->kmax];
    if (st & 1) return ital_fail(-33, "ital_ctx_fetch: kernel matrix of the labelled samples is not positive definite");
    if (st & 6) {
        (void)write_status(c, 0);
        return ital_fail(-71, "ital_ctx_fetch: the round needs the general scorer (duplicate samples in the batch or large noise)");
    }
    c->last_picks.assign(host.begin(), host.begin() + k);
    for (int t = 0; t < k; t++) picks[t] = host[(size_t)t];
    return k;
}

extern "C" int ital_ctx_set_model(ital_ctx* c, const ital_ctx_model* model) {
    if (!c || !model) return ital_fail(-22, "ital_ctx_set_model: bad arguments");
    char msg[256];
    if (model->label_estimation < 0 || model->label_estimation > 2) {
        snprintf(msg, sizeof(msg), "ital_ctx_set_model: label_estimation=%d is not implemented (0 'mean', 1 'optimistic', 2 'pessimistic')",
                 model->label_estimation);
        return ital_fail(-95, msg);
    }
    if (model->monte_carlo_num_rel != 0 || model->monte_carlo_num_fb != 0)
        return ital_fail(-95, "ital_ctx_set_model: the Monte-Carlo switches (monte_carlo_num_rel / monte_carlo_num_fb) are not "
                              "implemented in the context layer");
    if (model->clip_cov > 0 && model->clip_cov < 1) return ital_fail(-95, "ital_ctx_set_model: clip_cov is not implemented in the context layer");
    if (!(model->label_prob >= 0 && model->label_prob <= 1) || !(model->mistake_prob >= 0 && model->mistake_prob <= 1))
        return ital_fail(-22, "ital_ctx_set_model: label_prob and mistake_prob are probabilities");
    c->model = *model;
    c->model.clip_cov = 0;
    c->has_model = true;
    return 0;
}

extern "C" int ital_ctx_fetch_list(ital_ctx* c, int k, const int64_t* cand, int64_t n_cand, const int64_t* ce_subset, int n_subset,
                                   int64_t* picks, hipStream_t stream) {
    return model_fetch(c, "ital_ctx_fetch_list", k, cand, n_cand, ce_subset, n_subset, picks, stream);
}

// MCMI_min.fetch_unlabelled(k) on one rank (ital_amd/mcmi.py:134-229): the candidate block gathered out of the rows, then
// ital_mcmi_round (k <= nc <= 2^18) or the step loop; the picks' feature rows stay in the batch state for ital_ctx_update.
extern "C" int ital_ctx_mcmi_fetch(ital_ctx* c, int k, const int64_t* cand, int64_t n_cand, int64_t* picks, hipStream_t stream) {
    if (!c || !c->fitted || !picks || (cand && n_cand < 0)) return ital_fail(-22, "ital_ctx_mcmi_fetch: bad arguments");
    if (c->world > 1) return ital_fail(-38, "ital_ctx_mcmi_fetch: MCMI_min on several ranks needs an all-reduce of the candidate block");
    if (c->m == 0) return ital_fail(-22, "ital_ctx_mcmi_fetch: needs a fitted relevance model: call ital_ctx_update first");
    std::vector<int64_t> list;
    if (cand) {
        int rc = check_list(c, cand, n_cand, "ital_ctx_mcmi_fetch", "the candidate list");
        if (rc) return rc;
        list.assign(cand, cand + n_cand);
    } else {
        list = unlabelled(c);
    }
    const int64_t nc = (int64_t)list.size();
    if (nc < k) k = (int)nc;
    if (k < 1) return 0;
    if (k > ITAL_MAX_T) return ital_fail(-95, "ital_ctx_mcmi_fetch: batches larger than 8 are not enumerated on the device");
    c->last_picks.clear();
    const int ldc = pad16(nc), ldx = c->ldx, cap = c->cap;
    const char* oom = "ital_ctx_mcmi_fetch: out of device memory";
    int rc = grow(stream, oom, want(c->Xc, nc * ldx), want(c->vec, 3 * nc), want(c->ce, nc), want(c->cand64, nc), want(c->bpos, nc),
                  want(c->balive, nc));
    if (rc < 0) return rc;
    if (rc > 0) {
        // (a grown bpos is zero again: block positions 0, 1, 2, ...)
        std::vector<int32_t> pos((size_t)nc);
        for (int64_t i = 0; i < nc; i++) pos[(size_t)i] = (int32_t)i;
        if (hipMemcpy(c->bpos, pos.data(), pos.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
            return ital_fail(-5, "ital_ctx_mcmi_fetch: upload failed");
    }
    // Vc [cap][ldc] and the covariance block [nc][ldc] follow the block's padded width
    if ((rc = grow(stream, oom, want(c->Vc, (int64_t)cap * ldc), want(c->cov, (int64_t)ldc * nc))) < 0) return rc;
    const bool round = nc <= ((int64_t)1 << 18);
    if (k >= 5 && (rc = grow(stream, "ital_ctx_mcmi_fetch: out of device memory (workspace)",
                             want(c->mwork, ital_mcmi_workspace(ITAL_MAX_T, nc)))) < 0)
        return rc;
    double *xnc = c->vec, *muc = c->vec + nc, *s2c = c->vec + 2 * nc;
    // (the padding columns of Vc stay zero: cleared before every gather, the block width may have changed)
    if (hipMemcpyAsync(c->cand64, list.data(), nc * sizeof(int64_t), hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipMemsetAsync(c->Vc, 0, (size_t)cap * ldc * sizeof(double), stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_mcmi_fetch: upload of the candidate list failed");
    rc = ital_gather_block(c->cand64, nc, c->row0, c->n, c->X, c->xn, ldx, c->V, c->ldv, c->m, c->mu, c->s2, c->Xc, c->Vc, ldc, xnc,
                           muc, s2c, stream);
    if (rc) return rc;
    ital_mcmi_desc step;
    memset(&step, 0, sizeof(step));
    step.n_i = nc; step.pos_offset = 0; step.n_all = nc; step.alive = c->balive; step.mu = muc; step.s2 = s2c;
    step.cov = c->cov; step.ld_cov = ldc; step.C = c->C; step.ldc = ldc; step.batch = c->batch; step.noise = c->noise;
    step.eps = 1e-12; step.ce = c->ce;
    if (k >= 5) { step.work = c->mwork; step.work_doubles = c->mwork.count; }
    if (round) {
        ital_mcmi_round_desc r;
        memset(&r, 0, sizeof(r));
        r.k = k; r.step = step; r.Xc = c->Xc; r.xnc = xnc; r.ldx = ldx; r.Vc = c->Vc; r.ldv = ldc; r.m = c->m; r.ldw = cap;
        r.var = c->var; r.length_scale = c->length_scale; r.pos = c->bpos; r.status = c->status; r.record = c->rec; r.ret = c->ret;
        r.begin = 1;
        rc = ital_mcmi_round(&r, stream);
        if (rc) return rc;
    } else {
        if (hipMemsetAsync(c->balive, 1, nc, stream) != hipSuccess ||
            hipMemsetAsync(c->ret, 0, (c->kmax + 1) * sizeof(int64_t), stream) != hipSuccess)
            return ital_fail(-5, "ital_ctx_mcmi_fetch: memset failed");
        rc = ital_cov_block(c->Xc, xnc, nc, c->Xc, xnc, nc, ldx, c->Vc, ldc, c->Vc, ldc, c->m, c->var, c->length_scale, c->cov, ldc,
                            stream);
        const int rec_len = record_len(c);
        for (int t = 1; t <= k && !rc; t++) {
            step.t = t;
            rc = ital_mcmi_score_step(&step, stream);
            if (!rc) rc = ital_select_local(c->ce, c->bpos, c->balive, nc, 0, nullptr, 0, c->rank, 1, muc, s2c, c->Xc, xnc, ldx, c->Vc,
                                            ldc, c->m, cap, c->C, ldc, t - 1, c->kmax, c->status, c->work3k, c->rec, stream);
            if (!rc) rc = ital_select_resolve(c->rec, 1, rec_len, c->rank, 1, t - 1, c->batch, c->balive, c->ret, stream);
            if (!rc && t < k)
                rc = ital_cross_cov_cols(c->Xc, xnc, nc, ldx, c->batch.XB + (size_t)(t - 1) * ldx, c->batch.XBn + (t - 1), 1,
                                         c->batch.VB + (size_t)(t - 1) * cap, cap, c->Vc, ldc, c->m, c->var, c->length_scale,
                                         c->C + (size_t)(t - 1) * ldc, ldc, stream);
        }
        if (rc) return rc;
    }
    std::vector<int64_t> host;
    if ((rc = download_ret(c, host, stream))) return rc;       // block positions + status word
    if ((rc = round_status(host[(size_t)c->kmax], "ital_ctx_mcmi_fetch"))) return rc;
    for (int t = 0; t < k; t++) picks[t] = list[(size_t)host[(size_t)t]];
    c->last_picks.assign(picks, picks + k);
    return k;
}

// top_results(k): ital_topk over this rank's means; several ranks exchange their (value, index) pairs once and merge on the
// host by the same rule (NaN first, larger first, ties by the larger index), so every rank returns the same list.
extern "C" int ital_ctx_top_results(ital_ctx* c, int k, int64_t* idx, hipStream_t stream) {
    if (!c || !c->fitted || !idx) return ital_fail(-22, "ital_ctx_top_results: bad arguments");
    if (c->m == 0) return ital_fail(-22, "ital_ctx_top_results: needs a fitted relevance model: call ital_ctx_update first");
    if (k < 1 || k > std::min<int64_t>(ITAL_TOPK_MAX, c->n_total))
        return ital_fail(-22, "ital_ctx_top_results: k outside 1..min(ITAL_TOPK_MAX, number of samples)");
    int rc = 0;
    const char* oom = "ital_ctx_top_results: out of device memory";
    if (c->tk_work.ensure((int64_t)ital_topk_workspace()) < 0) return ital_fail(-12, oom);
    // per rank: [k values][k indices (int64 bits)], all ranks' behind each other
    if ((rc = grow(stream, oom, want(c->tk_send, 2 * k), want(c->tk_all, 2 * k * c->world))) < 0) return rc;
    const int k_loc = (int)std::min<int64_t>(k, c->n);
    if (k_loc > 0 && (rc = ital_topk(c->mu, c->n, c->row0, k_loc, c->tk_send, reinterpret_cast<int64_t*>(c->tk_send + k), c->tk_work,
                                     stream)))
        return rc;
    const bool several = c->comm != nullptr;
    if (several && (rc = ital_select_exchange(c->tk_send, c->tk_all, 2 * k, c->comm, stream))) return rc;
    const int nw = several ? c->world : 1;
    std::vector<double> all((size_t)2 * k * nw);
    if (hipMemcpyAsync(all.data(), several ? c->tk_all : c->tk_send, all.size() * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_top_results: download failed");
    struct Cand { double v; int64_t i; };
    std::vector<Cand> pool;
    for (int w = 0; w < nw; w++) {
        const int64_t rows = several ? c->n_total * (w + 1) / c->world - c->n_total * w / c->world : c->n;
        const int kw = (int)std::min<int64_t>(k, rows);
        const double* base = all.data() + (size_t)2 * k * w;
        for (int j = 0; j < kw; j++) {
            int64_t i;
            memcpy(&i, base + k + j, sizeof(i));
            pool.push_back({base[j], i});
        }
    }
    std::sort(pool.begin(), pool.end(), [](const Cand& a, const Cand& b) {
        const bool an = isnan(a.v), bn = isnan(b.v);
        if (an != bn) return an;
        if (an || a.v == b.v) return a.i > b.i;
        return a.v > b.v;
    });
    for (int j = 0; j < k; j++) idx[j] = pool[(size_t)j].i;
    return 0;
}

// gp.predict(Xt, cov_mode='diag') at external points (ital_amd/gp.py:467-488): ital_predict in chunks of kPredictChunk points.
extern "C" int ital_ctx_predict(ital_ctx* c, const double* Xt, int64_t nt, double* mean, double* variance, hipStream_t stream) {
    if (!c || !c->fitted || nt < 0 || (nt > 0 && !Xt)) return ital_fail(-22, "ital_ctx_predict: bad arguments");
    if (c->m == 0) return ital_fail(-22, "ital_ctx_predict: needs a fitted relevance model: call ital_ctx_update first");
    // (the padding columns of pXt stay zero: the uploads write d of ldx columns)
    if (c->pXt.ensure(kPredictChunk * c->ldx) < 0 || c->pxtn.ensure(kPredictChunk) < 0 || c->pVt.ensure(c->cap * kPredictChunk) < 0 ||
        c->pmean.ensure(kPredictChunk) < 0 || c->pvar.ensure(kPredictChunk) < 0)
        return ital_fail(-12, "ital_ctx_predict: out of device memory");
    for (int64_t i0 = 0; i0 < nt; i0 += kPredictChunk) {
        const int64_t cnt = std::min<int64_t>(kPredictChunk, nt - i0);
        const int64_t ldvt = pad16(cnt);
        if (!copy_rows(c->pXt, c->ldx, Xt + (size_t)i0 * c->d, c->d, cnt, false, stream))
            return ital_fail(-5, "ital_ctx_predict: upload of the points failed");
        int rc = ital_predict(c->pXt, cnt, c->ldx, c->XT, c->XTn, c->m, c->L, c->cap, c->alpha, c->var, c->length_scale, c->pmean,
                              c->pvar, c->pxtn, c->pVt, ldvt, 1, stream);
        if (rc) return rc;
        if ((mean && hipMemcpyAsync(mean + i0, c->pmean, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess) ||
            (variance && hipMemcpyAsync(variance + i0, c->pvar, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess) ||
            hipStreamSynchronize(stream) != hipSuccess)
            return ital_fail(-5, "ital_ctx_predict: download failed");
    }
    return 0;
}

// Predictive mean and variance of this rank's rows (n_local doubles each, host memory; either may be NULL); the variance
// clamped at 0 as predict_stored(cov_mode='diag') does (reference gp.py:203-232).  Synchronises `stream`.
extern "C" int ital_ctx_predict_stored(ital_ctx* c, double* mean, double* variance, hipStream_t stream) {
    if (!c || !c->fitted) return ital_fail(-22, "ital_ctx_predict_stored: bad arguments");
    if (mean && hipMemcpyAsync(mean, c->mu, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_predict_stored: download failed");
    if (variance && hipMemcpyAsync(variance, c->s2, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess)
        return ital_fail(-5, "ital_ctx_predict_stored: download failed");
    if (hipStreamSynchronize(stream) != hipSuccess) return ital_fail(-5, "ital_ctx_predict_stored: stream error");
    if (variance)
        for (int64_t i = 0; i < c->n; i++) variance[i] = variance[i] > 0 ? variance[i] : 0;
    return 0;
}

extern "C" int64_t ital_ctx_local_rows(const ital_ctx* c, int64_t* row0) {
    if (!c) return 0;
    if (row0) *row0 = c->row0;
    return c->n;
}
