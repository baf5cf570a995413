"""The context layer beyond the perfect user (include/ital_ctx.h, csrc/ctx.hip): user models, caller-given candidate lists
with a change-estimation subset, MCMI_min, top_results and predict -- the golden sessions of the real reference replayed
through ctypes (host arrays only; the library owns every device buffer), cross-checks against the Python learners, and the
error codes.  Reference: ital/ital.py:84-134, :183-481, ital/mcmi.py:48-124, ital/retrieval_base.py:64-75, ital/gp.py:264-292."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import _ranks  # noqa: E402
import make_golden  # noqa: E402  (fixture table only)

_LABEL_MODES = {"mean": 0, "optimistic": 1, "pessimistic": 2}


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ital_amd import _lib
    torch.cuda.init()
    return _lib.load()


def _i64(v):
    return np.ascontiguousarray(v, dtype=np.int64)


class Ctx:
    """One context through ctypes; every call returns the library's code (the caller asserts)."""

    def __init__(self, lib, X, ls, var=1.0, noise=1e-6, capacity=64, rank=0, world=1, comm=None, n_total=None):
        self.lib = lib
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        self.n_total = len(X) if n_total is None else n_total
        self.h = ctypes.c_void_p()
        rc = lib.ital_ctx_create(self.n_total, self.X.shape[1], float(ls), float(var), float(noise), capacity, rank, world, comm,
                                 ctypes.byref(self.h))
        assert rc == 0, self.err()
        assert lib.ital_ctx_fit(self.h, self.X.ctypes.data, 0, None) == 0, self.err()

    def err(self):
        return self.lib.ital_last_error().decode()

    def close(self):
        assert self.lib.ital_ctx_destroy(self.h) == 0

    def set_model(self, label_prob=1.0, mistake_prob=0.0, label_estimation="mean", mc_rel=0, mc_fb=0, clip_cov=0.0):
        from ital_amd import _lib
        m = _lib.ItalCtxModel(float(label_prob), float(mistake_prob), _LABEL_MODES.get(label_estimation, label_estimation),
                              mc_rel, mc_fb, float(clip_cov))
        return self.lib.ital_ctx_set_model(self.h, ctypes.byref(m))

    def update(self, idx, y):
        idx, y = _i64(idx), np.ascontiguousarray(y, dtype=np.float64)
        assert self.lib.ital_ctx_update(self.h, idx.ctypes.data, y.ctypes.data, len(idx), None) == 0, self.err()

    def fetch(self, k):
        p = np.zeros(max(k, 1), dtype=np.int64)
        rc = self.lib.ital_ctx_fetch(self.h, k, p.ctypes.data, None)
        return rc, p[: max(rc, 0)].tolist()

    def fetch_list(self, k, cand=None, subset=None):
        p = np.zeros(max(k, 1), dtype=np.int64)
        c = None if cand is None else _i64(cand)
        s = None if subset is None else _i64(subset)
        rc = self.lib.ital_ctx_fetch_list(self.h, k, None if c is None else c.ctypes.data, 0 if c is None else len(c),
                                          None if s is None else s.ctypes.data, 0 if s is None else len(s), p.ctypes.data, None)
        return rc, p[: max(rc, 0)].tolist()

    def mcmi_fetch(self, k, cand=None):
        p = np.zeros(max(k, 1), dtype=np.int64)
        c = None if cand is None else _i64(cand)
        rc = self.lib.ital_ctx_mcmi_fetch(self.h, k, None if c is None else c.ctypes.data, 0 if c is None else len(c),
                                          p.ctypes.data, None)
        return rc, p[: max(rc, 0)].tolist()

    def predict_stored(self):
        n = self.lib.ital_ctx_local_rows(self.h, None)
        mean, var = np.empty(n), np.empty(n)
        assert self.lib.ital_ctx_predict_stored(self.h, mean.ctypes.data, var.ctypes.data, None) == 0, self.err()
        return mean, var

    def top_results(self, k):
        idx = np.zeros(max(k, 1), dtype=np.int64)
        rc = self.lib.ital_ctx_top_results(self.h, k, idx.ctypes.data, None)
        return rc, idx[:k].tolist()

    def predict(self, Xt):
        Xt = np.ascontiguousarray(Xt, dtype=np.float64)
        mean, var = np.empty(len(Xt)), np.empty(len(Xt))
        rc = self.lib.ital_ctx_predict(self.h, Xt.ctypes.data, len(Xt), mean.ctypes.data, var.ctypes.data, None)
        return rc, mean, var


def replay(lib, name, how, comm=None):
    """All rounds of golden fixture `name` through one context; `how` names the call that fetches (see the table below)."""
    z = np.load(os.path.join(HERE, "golden", name + ".npz"))
    spec = make_golden.FIXTURES[name]
    k = int(z["k"])
    ctx = Ctx(lib, z["X"], z["length_scale"], z["var"], z["noise"], comm=comm)
    try:
        if how == "model":
            assert ctx.set_model(**spec["kw"]) == 0, ctx.err()
        elif how == "perfect":
            assert ctx.set_model() == 0, ctx.err()
        prev = 0
        for r in range(int(z["rounds"])):
            ind, y = z["r%d_ind" % r], z["r%d_y" % r]
            ctx.update(ind[prev:], y[prev:])
            prev = len(ind)
            mean, var = ctx.predict_stored()
            np.testing.assert_allclose(mean, z["r%d_rel_mean" % r], rtol=0, atol=2e-9)
            np.testing.assert_allclose(var, z["r%d_var" % r], rtol=0, atol=2e-9)
            if how in ("model", "perfect"):
                rc, got = ctx.fetch(k)
            elif how == "list":
                rc, got = ctx.fetch_list(k, z["r%d_s0_cand" % r])
            elif how == "subset":
                rc, got = ctx.fetch_list(k, None, z["r%d_ce_subset" % r])
            else:
                rc, got = ctx.mcmi_fetch(k, z["r%d_s0_cand" % r])
            assert rc == k, ctx.err()
            assert got == z["r%d_ret" % r].tolist(), (name, r)
        ctx.update(got, z["rel"][got])
        mean, _ = ctx.predict_stored()
        np.testing.assert_allclose(mean, z["final_rel_mean"], rtol=0, atol=1e-9)
        rc, top = ctx.top_results(10)
        assert rc == 0 and top == z["top_results_10"].tolist()
        rc, pm, pv = ctx.predict(z["predict_X"])
        assert rc == 0, ctx.err()
        np.testing.assert_allclose(pm, z["predict_mean"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(pv, z["predict_var"], rtol=0, atol=1e-9)
    finally:
        ctx.close()


@pytest.mark.parametrize("name,how", [("synth200_noisy", "model"), ("synth200_motivated", "model"),
                                      ("synth200_optimistic", "model"), ("synth200_topcand", "list"),
                                      ("synth200_topcand_float", "list"), ("iris_ce5", "subset"), ("usps500_mcmi", "mcmi"),
                                      ("synth300_mcmi", "mcmi"), ("usps500", "perfect")])
def test_golden_session_through_the_context(lib, name, how):
    replay(lib, name, how)


def test_duplicate_rows_fall_back_to_the_general_scorer(lib):
    """A round the lattice scorer flags (every row twice: the batch meets a sample's twin) is -71 on a plain context and
    ITAL's own fall-back round on a context with a model (ital.py:411-417: same stream position, general scorer)."""
    from ital_amd import ITAL, mvn_stream
    B = np.random.default_rng(21).random((30, 5))
    X = np.concatenate([B, B])
    ls = float(np.sqrt(5 / 12.0))
    plain = Ctx(lib, X, ls)
    try:
        plain.update([4], [1.0])
        rc, _ = plain.fetch(3)
        assert rc == -71, plain.err()
    finally:
        plain.close()
    mvn_stream.GLOBAL.reset()
    L = ITAL(X, length_scale=ls, device="cuda:0")
    L.update({4: 1})
    want = L.fetch_unlabelled(3)
    ctx = Ctx(lib, X, ls)
    try:
        assert ctx.set_model() == 0
        ctx.update([4], [1.0])
        rc, got = ctx.fetch(3)
        assert rc == 3, ctx.err()
        assert got == want
        # the next round continues from the same stream position as the learner's
        L.update({i: 1.0 if X[i, 0] > 0.5 else -1.0 for i in want})
        ctx.update(want, [1.0 if X[i, 0] > 0.5 else -1.0 for i in want])
        rc, got = ctx.fetch(3)
        assert rc == 3 and got == L.fetch_unlabelled(3)
    finally:
        ctx.close()


def test_noisy_pessimistic_user_equals_the_python_learner(lib):
    from ital_amd import ITAL, mvn_stream
    rng = np.random.default_rng(5)
    X = rng.random((150, 8))
    ls = float(np.sqrt(8 / 12.0))
    kw = dict(label_prob=0.6, mistake_prob=0.2, label_estimation="pessimistic")
    mvn_stream.GLOBAL.reset()
    L = ITAL(X, length_scale=ls, device="cuda:0", **kw)
    ctx = Ctx(lib, X, ls)
    try:
        assert ctx.set_model(**kw) == 0
        labels = {3: 1.0}
        for r in range(3):
            L.update(labels)
            ctx.update(list(labels), list(labels.values()))
            want = L.fetch_unlabelled(3)
            rc, got = ctx.fetch(3)
            assert rc == 3, ctx.err()
            assert got == want, r
            labels = {i: 1.0 if X[i, 1] > 0.5 else -1.0 for i in want}
    finally:
        ctx.close()


def test_mcmi_equals_the_python_learner(lib):
    from ital_amd import MCMI_min
    rng = np.random.default_rng(8)
    X = rng.random((120, 6))
    ls = float(np.sqrt(6 / 12.0))
    L = MCMI_min(X, length_scale=ls, device="cuda:0")
    ctx = Ctx(lib, X, ls)
    try:
        labels = {0: 1.0, 1: -1.0}
        for k in (3, 5):                       # k = 5: the MCMI workspace
            L.update(labels)
            ctx.update(list(labels), list(labels.values()))
            want = L.fetch_unlabelled(k)
            rc, got = ctx.mcmi_fetch(k)
            assert rc == k, ctx.err()
            assert got == want, k
            labels = {i: 1.0 if X[i, 2] > 0.5 else -1.0 for i in want}
        L.update(labels)
        ctx.update(list(labels), list(labels.values()))
        rc, top = ctx.top_results(7)
        assert rc == 0 and top == L.top_results(7).tolist()
    finally:
        ctx.close()


def test_error_codes(lib):
    from ital_amd import ITAL, mvn_stream
    rng = np.random.default_rng(3)
    X = rng.random((60, 4))
    ls = 0.7
    ctx = Ctx(lib, X, ls)
    try:
        # before the first label
        assert ctx.top_results(3)[0] == -22 and "fitted relevance model" in ctx.err()
        assert ctx.predict(X[:2])[0] == -22 and "fitted relevance model" in ctx.err()
        assert ctx.fetch_list(2)[0] == -22 and ctx.mcmi_fetch(2)[0] == -22
        # models the context does not drive
        assert ctx.set_model(mc_rel=2) == -95 and "Monte-Carlo" in ctx.err()
        assert ctx.set_model(mc_fb=1) == -95 and "Monte-Carlo" in ctx.err()
        assert ctx.set_model(clip_cov=0.35) == -95 and "clip_cov" in ctx.err()
        assert ctx.set_model(label_estimation=3) == -95 and "label_estimation=3" in ctx.err()
        ctx.update([0, 1], [1.0, -1.0])
        # bad lists
        assert ctx.fetch_list(2, [5, 0, 7])[0] == -22 and "a labelled sample" in ctx.err()
        assert ctx.fetch_list(2, [5, 6, 5])[0] == -22 and "a repeated sample" in ctx.err()
        assert ctx.fetch_list(2, [5, 60])[0] == -22 and "outside the data" in ctx.err()
        assert ctx.fetch_list(2, None, [3, 3])[0] == -22 and "a repeated sample" in ctx.err()
        assert ctx.mcmi_fetch(2, [9, 1])[0] == -22 and "a labelled sample" in ctx.err()
        # beyond the device scorers (the words of ITAL._unsupported)
        assert ctx.fetch_list(3, None, list(range(2, 20)))[0] == -95
        assert "orthant dimension 21 (subset + batch) above 20" in ctx.err()
        assert ctx.fetch_list(2, list(range(2, 23)), list(range(2, 23)))[0] == -95
        assert "change_estimation_subset=None with 21 candidates" in ctx.err()
        assert ctx.fetch_list(9)[0] == -95 and "batches larger than 8 with full enumeration" in ctx.err()
        assert ctx.set_model(label_prob=0.6, mistake_prob=0.2) == 0
        assert ctx.fetch(17)[0] == -95 and "batches larger than 16 with the general scorer" in ctx.err()
        assert ctx.fetch(9)[0] == -95 and "10078208 orthant probabilities per candidate at greedy step 9" in ctx.err()
        assert ctx.mcmi_fetch(9)[0] == -95 and "larger than 8" in ctx.err()
        # top_results / predict arguments
        assert ctx.top_results(0)[0] == -22 and ctx.top_results(61)[0] == -22
        assert ctx.top_results(60)[0] == 0
    finally:
        ctx.close()
    # k larger than the list: the reference's steps run (the stream advances), then np.argmax([]) raises
    mvn_stream.GLOBAL.reset()
    L = ITAL(X, length_scale=ls, top_candidates=2, device="cuda:0")
    L.update({0: 1})
    with pytest.raises(ValueError, match="empty sequence"):
        L.fetch_unlabelled(3)
    L.top_candidates = None
    want = L.fetch_unlabelled(3)
    ctx = Ctx(lib, X, ls)
    try:
        ctx.update([0], [1.0])
        assert ctx.fetch_list(3, [10, 20])[0] == -61 and "attempt to get argmax of an empty sequence" in ctx.err()
        rc, got = ctx.fetch_list(3)
        assert rc == 3 and got == want
    finally:
        ctx.close()


def _comm_worker(rank, world, port, name, out):
    dev, group = _ranks.join(rank, world, port, "rccl1")
    try:
        from ital_amd import _lib, sharding
        lib = _lib.load()
        comm = sharding.raw_comm(group, dev)            # the process group's own ncclComm_t (one rank)
        if comm is None:
            out[rank] = ("no raw communicator", sharding.raw_comm_reason(group, dev))
            return
        replay(lib, name, "model", comm=comm)
        torch.cuda.synchronize()
        out[rank] = ("ok", None)
    finally:
        _ranks.leave(group)


def test_noisy_golden_through_the_exchange_path(golden_dir):
    """synth200_noisy with a communicator: every greedy step of the general scorer goes ital_select_local -> ncclAllGather ->
    ital_select_resolve, top_results through the (value, index) exchange (a one-rank RCCL group)."""
    res = _ranks.spawn(_comm_worker, 1, "synth200_noisy")[0]
    assert res[0] == "ok", res
