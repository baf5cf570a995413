// The context that the library owns (include/ital_hip.h, ital_ctx.h, ital_ctx_live.h) as its two translation units see it: ctx.hip
// (create / fit / update / revoke / the fetches / predictions) and ctx_live.hip (reserve / add_rows / remove_rows /
// set_params / evidence).  Private: no host includes this.
//
// Every device buffer has an owner (DevBuf): the context's are members of the groups below, a call's are locals of the call.
// ital_state::each is the one place that writes a size formula of the model state; a call whose sizes change allocates the
// buffers that follow the changed size in a local ital_state, enqueues and checks its work, and commits by move.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>

#include "ital_ctx.h"
#include "ital_hip.h"
#include "ital_internal.h"
#include "ital_revoke.h"

namespace {

int pad16(int64_t v) { return (int)((v + 15) / 16 * 16); }

// THE rule of giving device memory back: work enqueued earlier on `stream` may still touch it, so the stream is drained
// first.  grow() and ~Staged, the two places that free memory a kernel may have seen, go through here; a commit frees what
// it replaces after the call's own synchronisation.
bool drain(hipStream_t stream) { return hipStreamSynchronize(stream) == hipSuccess; }

// A device buffer and the element count it was allocated for.  Move-only; the memory goes back when the owner goes out of
// scope, is reset or is assigned to.
template <class T>
struct DevBuf {
    T* p = nullptr;
    int64_t count = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), count(std::exchange(o.count, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p = std::exchange(o.p, nullptr);
            count = std::exchange(o.count, 0);
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    operator T*() const { return p; }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        count = 0;
    }
    // n elements (at least one), zero-filled, 64 bytes of slack behind the end; what was held is given back first.
    // (An unchecked failure would surface as a device fault in the first kernel that touches the buffer.)
    bool alloc(int64_t n) {
        reset();
        const size_t bytes = (size_t)std::max<int64_t>(n, 1) * sizeof(T) + 64;
        void* q = nullptr;
        if (hipMalloc(&q, bytes) != hipSuccess) return false;
        if (hipMemset(q, 0, bytes) != hipSuccess) {
            (void)hipFree(q);
            return false;
        }
        p = static_cast<T*>(q);
        count = n;
        return true;
    }
    // Grows to n elements when fewer are held: 1 grown (zero-filled: the caller refills what it keeps there), 0 large
    // enough as it is, -1 out of memory (nothing held).
    int ensure(int64_t n) { return n <= count ? 0 : (alloc(n) ? 1 : -1); }
};

template <class T>
struct Want {
    DevBuf<T>& buf;
    int64_t count;
};
template <class T>
Want<T> want(DevBuf<T>& buf, int64_t count) { return {buf, count}; }

// The lazy growth of buffers that grow together: when a request exceeds what its buffer holds, the stream is drained and
// the buffers grow.  1 grown, 0 nothing to do, or the failure's code with `oom` as the text of -12.
template <class... T>
int grow(hipStream_t stream, const char* oom, Want<T>... w) {
    if (!((w.count > w.buf.count) || ...)) return 0;
    if (!drain(stream)) return ital_fail(-5, "ital_ctx: stream error");
    if (!((w.buf.ensure(w.count) >= 0) && ...)) return ital_fail(-12, oom);
    return 1;
}

// What a call holds while it runs: the state it builds before it commits and its temporaries.  Whatever is still here
// when the call returns -- everything after a failure, which leaves the context as it was -- is given back once the
// stream has drained.
template <class G>
struct Staged : G {
    hipStream_t stream;
    explicit Staged(hipStream_t s) : stream(s) {}
    ~Staged() { (void)drain(stream); }
};

}  // namespace

// The sizes every buffer of the model state follows.
struct ital_dims {
    int64_t n = 0, ldv = 0;            // local rows; leading dimension of V and C, length of mu and s2
    int ldx = 0, cap = 0, kmax = ITAL_MAX_T, world = 1;
};

// What sizes a buffer or decides its contents: a call allocates the buffers that carry the bit of what it changes.
enum : unsigned {
    BY_ROWS = 1,     // n, ldv
    BY_CAP = 2,      // the labelled-set capacity
    BY_KMAX = 4,     // the batch capacity
    BY_PARAMS = 8,   // written again under other kernel parameters (xn: ital_whiten_rows writes it with the rest)
    BY_LABEL = 16,   // rewritten when a label leaves (ital_gp_remove)
    ALL = ~0u,       // ital_ctx_create; nothing but it makes ybuf, status, work3k
};

// The model state on the device.
struct ital_state {
    DevBuf<double> L, alpha, XT, XTn;                       // labelled-set state
    DevBuf<double> X, xn, V, mu, s2, C;                     // row state
    DevBuf<int64_t> ret, bidx, bgpos;                       // picks + status word of a round; then the batch state, which
    DevBuf<int32_t> bsort;                                  //   kernels see through the view ital_ctx::batch
    DevBuf<double> rec, rec_all, bmu, sig, XB, XBn, VB;
    DevBuf<double> ybuf, work3k;
    DevBuf<int> status;

    // f(member, what it follows, elements) for every buffer: THE size formulas.
    template <class F>
    static void each(const ital_dims& d, F&& f) {
        using S = ital_state;
        const int64_t n = std::max<int64_t>(d.n, 1), ldv = d.ldv, ldx = d.ldx, cap = d.cap, kmax = d.kmax;
        const int64_t rec_len = ital_record_len(d.ldx, d.cap, d.kmax);
        f(&S::L, BY_CAP | BY_PARAMS | BY_LABEL, cap * cap);
        f(&S::alpha, BY_CAP | BY_PARAMS | BY_LABEL, cap);
        f(&S::XT, BY_CAP | BY_LABEL, cap * ldx);
        f(&S::XTn, BY_CAP | BY_LABEL, cap);
        f(&S::X, BY_ROWS, n * ldx);
        f(&S::xn, BY_ROWS | BY_PARAMS, n);
        f(&S::V, BY_ROWS | BY_CAP | BY_PARAMS | BY_LABEL, cap * ldv);
        f(&S::mu, BY_ROWS | BY_PARAMS | BY_LABEL, ldv);
        f(&S::s2, BY_ROWS | BY_PARAMS | BY_LABEL, ldv);
        f(&S::C, BY_ROWS | BY_KMAX, kmax * ldv);
        f(&S::ret, BY_KMAX, kmax + 1);
        f(&S::rec, BY_KMAX | BY_CAP, rec_len);
        f(&S::rec_all, BY_KMAX | BY_CAP, d.world * rec_len);
        f(&S::bidx, BY_KMAX, kmax);
        f(&S::bgpos, BY_KMAX, kmax);
        f(&S::bsort, BY_KMAX, kmax);
        f(&S::bmu, BY_KMAX, kmax);
        f(&S::sig, BY_KMAX, kmax * kmax);
        f(&S::XB, BY_KMAX, kmax * ldx);
        f(&S::XBn, BY_KMAX, kmax);
        f(&S::VB, BY_KMAX | BY_CAP, kmax * cap);
        f(&S::ybuf, 0u, 16);
        f(&S::status, 0u, 1);
        f(&S::work3k, 0u, 3 * 1024);
    }
    // The buffers that follow `what`, at the sizes of `d`: false when one could not be allocated.
    bool alloc(const ital_dims& d, unsigned what) {
        bool ok = true;
        each(d, [&](auto m, unsigned follows, int64_t count) {
            if (ok && (what == ALL || (follows & what))) ok = (this->*m).alloc(count);
        });
        return ok;
    }
    // The buffers that follow `what` <- those of `src`, both of the sizes `d`, by copies on the stream in the order of each().
    bool copy(const ital_state& src, const ital_dims& d, unsigned what, hipStream_t stream) {
        bool ok = true;
        each(d, [&](auto m, unsigned follows, int64_t count) {
            using T = std::remove_reference_t<decltype(*(this->*m).p)>;
            if (ok && (follows & what))
                ok = hipMemcpyAsync(this->*m, src.*m, (size_t)count * sizeof(T), hipMemcpyDeviceToDevice, stream) == hipSuccess;
        });
        return ok;
    }
    // Every buffer `nw` holds replaces this state's, which is given back: the stream has drained.
    void take(ital_state&& nw) {
        each(ital_dims(), [&](auto m, unsigned, int64_t) {
            if ((nw.*m).p) this->*m = std::move(nw.*m);
        });
    }
};

// Lazily grown scratch, each buffer with the count it was grown to; every size here follows the rows or the capacity, so
// a call that changes either resets the group and the paths of ctx.hip allocate again, zeroed, on next use.
struct ital_scratch {
    DevBuf<int32_t> cand;               // this rank's share of a candidate list, its alive flags and scores
    DevBuf<uint8_t> alive;
    DevBuf<double> mi;
    DevBuf<int64_t> gpos;               // explicit list positions of this rank's candidates
    DevBuf<double> qwork;               // workspace of the lattice scorer / the general scorer's pipeline
    DevBuf<char> sub;                   // subset mode's base set (E_idx, E_sort, E_mu, E_sig, pick_pos, in_pos, dead_pos)
    // MCMI_min candidate block (ital_amd/mcmi.py: _gather_block / _fetch_bufs)
    DevBuf<double> Xc, Vc, vec, cov, ce, mwork;
    DevBuf<int64_t> cand64;
    DevBuf<int32_t> bpos;
    DevBuf<uint8_t> balive;
    // top_results (ital_topk + the (value, index) exchange) and predict at external points (chunks of kPredictChunk)
    DevBuf<char> tk_work;
    DevBuf<double> tk_send, tk_all;
    DevBuf<double> pXt, pxtn, pVt, pmean, pvar;
    DevBuf<double> rwork;               // ital_gp_remove_workspace(cap) doubles
};

// Made once per context, sizes fixed: the lattice scorer's stream tables per batch dimension, the general scorer's
// (jump1, vk_all, pick positions 0, 1, 2, ..., one zero), the staging of replicated rows in ital_ctx_update.
struct ital_tables {
    DevBuf<long long> jump[ITAL_MAX_T + 1], jumppat[ITAL_MAX_T + 1], jump1;
    DevBuf<double> vk[ITAL_MAX_T + 1], vk_all, stage;
    DevBuf<int32_t> iota;
    DevBuf<int64_t> zero64;
};

struct ital_ctx : ital_dims, ital_state, ital_scratch, ital_tables {
    int64_t n_total = 0, row0 = 0, row1 = 0;
    int d = 0, rank = 0, m = 0;
    double length_scale = 1, var = 1, noise = 1e-6;
    void* comm = nullptr;
    bool fitted = false;
    ital_batch batch = {};              // the ABI's view of the batch state
    // host bookkeeping
    int mvn_state[6] = {};
    std::vector<uint8_t> seen;          // [n_total] labelled (the reference's relevant / irrelevant ids)
    int64_t n_seen = 0;
    std::vector<int64_t> order;         // the labelled samples in insertion order: order[p] sits at position p of L / V / XT
    std::vector<double> ylab;           // their labels, parallel to `order` (ital_ctx_set_params / _evidence rebuild from them)
    std::vector<int64_t> last_picks;    // the batch of the last fetch (its feature rows sit in batch.XB on every rank)
    // user model (ital_ctx_set_model); without one ital_ctx_fetch is the perfect-user layer above (-71 and all)
    bool has_model = false;
    ital_ctx_model model = {1.0, 0.0, 0, 0, 0, 0.0};

    // The commit of a call that built in locals: the sizes become `nd`, the buffers of `nw` replace the context's, the
    // batch view follows.  The stream has drained.
    void commit(const ital_dims& nd, ital_state&& nw) {
        static_cast<ital_dims&>(*this) = nd;
        take(std::move(nw));
        batch = {kmax, ldx, cap, bidx, bgpos, bsort, bmu, sig, XB, XBn, VB};
    }
    void drop_scratch() { static_cast<ital_scratch&>(*this) = ital_scratch(); }
};

namespace {

int record_len(const ital_ctx* c) { return ital_record_len(c->ldx, c->cap, c->kmax); }

// count rows of d doubles (row-major, host memory or -- on_device -- device memory) into rows of leading dimension ldx.
bool copy_rows(double* dst, int ldx, const double* rows, int d, int64_t count, bool on_device, hipStream_t stream) {
    return hipMemcpy2DAsync(dst, (size_t)ldx * sizeof(double), rows, (size_t)d * sizeof(double), (size_t)d * sizeof(double),
                            (size_t)count, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream) == hipSuccess;
}

// Entries [from, to) of a variance vector <- the prior variance (`host` must outlive the stream's work).
bool fill_var(double* s2, int64_t from, int64_t to, double var, std::vector<double>& host, hipStream_t stream) {
    if (to <= from) return true;
    host.assign((size_t)(to - from), var);
    return hipMemcpyAsync(s2 + from, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, stream) == hipSuccess;
}

// One ital_gp_remove of position p out of m labelled samples, on the model state `s` of sizes `d`.
ital_remove_desc remove_desc(const ital_dims& d, const ital_state& s, int m, int p, double* work, int* status) {
    ital_remove_desc r = {};
    r.XT = s.XT; r.XTn = s.XTn; r.ldx = d.ldx; r.L = s.L; r.ldl = d.cap; r.alpha = s.alpha;
    r.V = s.V; r.ldv = d.ldv; r.n = d.n; r.mu = s.mu; r.s2 = s.s2; r.m = m; r.p = p;
    r.work = work; r.work_doubles = ital_gp_remove_workspace(d.cap); r.status = status;
    return r;
}

}  // namespace
