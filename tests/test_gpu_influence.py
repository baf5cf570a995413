"""What taking a label back would change, on the device (include/ital_influence.h, csrc/influence.hip): the two C entries
against the extended-precision model and a-priori bounds of tests/_influence_ref.py, GaussianProcess.influence /
preview_remove and ActiveRetrievalBase.audit / preview_revoke against clone() + revoke([i]) -- what they replace -- on a
plain array, a DeviceData and a compact store, on two ranks, and ital_ctx_audit against the Python learner."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _influence_ref as ref  # noqa: E402
import _ranks  # noqa: E402

U = 2.0 ** -53


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


# ------------------------------------------------------------------------------------------------------ the C entries
def _run(case, sel, dev):
    """Both entries on the case's arrays as they are (cap > m, ldv > n, poison outside m x n), the workspace and the outputs
    starting as NaN; entry 1 twice.  Returns a result as ref.evaluate does, and the second run's (coef, stats)."""
    from ital_amd import _lib
    lib = _lib.load()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    m, n = case.m, case.n
    L, alpha, V, mu, s2 = t(case.L), t(case.alpha), t(case.V), t(case.mu), t(case.s2)
    mask = t(case.mask) if case.mask is not None else None
    need = int(lib.ital_gp_influence_workspace(m, n))
    runs = []
    for _ in range(2):
        work = torch.full((need,), float("nan"), dtype=torch.float64, device=dev)
        coef = torch.full((m, 2), float("nan"), dtype=torch.float64, device=dev)
        stats = torch.full((m, 4), float("nan"), dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        d = _lib.ItalInfluenceDesc()
        d.L, d.ldl, d.alpha, d.m, d.V, d.ldv, d.n = L.data_ptr(), case.cap, alpha.data_ptr(), m, V.data_ptr(), case.ldv, n
        d.mu, d.s2, d.mask = mu.data_ptr(), s2.data_ptr(), mask.data_ptr() if mask is not None else None
        d.coef, d.stats, d.work, d.work_doubles, d.status = coef.data_ptr(), stats.data_ptr(), work.data_ptr(), need, status.data_ptr()
        _lib.check(lib.ital_gp_influence(ctypes.byref(d), None))
        torch.cuda.synchronize()
        runs.append((coef.cpu().numpy(), stats.cpu().numpy(), int(status.item()), work.cpu().numpy()))
    coef_h, stats_h, st, work_h = runs[0]
    res = dict(M=work_h[: m * m].reshape(m, m), c=work_h[m * m: m * m + m], w=work_h[m * m + m: m * m + 2 * m], coef=coef_h,
               stats=stats_h, status=st)
    if sel is not None:
        r, ldo = len(sel), n + 3
        mu_out = torch.full((r, ldo), float("nan"), dtype=torch.float64, device=dev)
        s2_out = torch.full((r, ldo), float("nan"), dtype=torch.float64, device=dev)
        work = torch.full((need,), float("nan"), dtype=torch.float64, device=dev)
        d.work, d.mask, d.stats = work.data_ptr(), None, None
        _lib.check(lib.ital_gp_preview_remove(ctypes.byref(d), (ctypes.c_int * r)(*sel), r, mu_out.data_ptr(), s2_out.data_ptr(),
                                              ldo, None))
        torch.cuda.synchronize()
        res["mu_out"], res["s2_out"] = mu_out.cpu().numpy(), s2_out.cpu().numpy()
        assert np.isnan(res["mu_out"][:, n:]).all() and np.isnan(res["s2_out"][:, n:]).all()     # nothing written past n
        # stage 1 of the second entry left the same M, c, w
        w2 = work.cpu().numpy()
        assert np.array_equal(np.tril(w2[: m * m].reshape(m, m)), np.tril(res["M"]), equal_nan=True)
        assert np.array_equal(w2[m * m: m * m + 2 * m], work_h[m * m: m * m + 2 * m], equal_nan=True)
    return res, runs[1]


@pytest.mark.parametrize("m,n,mask", ref.grid())
def test_entries_against_the_model(dev, m, n, mask):
    case = ref.Case(m, n, mask=mask)
    sel = ref.selection(m)
    res, again = _run(case, sel, dev)
    assert np.array_equal(res["coef"], again[0]) and np.array_equal(res["stats"], again[1])       # two runs, equal bits
    s = ref.check(case, res, sel)
    if m >= 2:
        assert s["ambiguous"].sum() == 0
        assert np.array_equal(res["stats"][:, 2], s["certain"].astype(np.float64))                # then the flips are exact
    assert np.array_equal(res["mu_out"][1, :n], res["mu_out"][3, :n])                             # the repeated position
    assert np.array_equal(res["s2_out"][1, :n], res["s2_out"][3, :n])
    if mask == "zero":
        assert not res["stats"].any()


def test_more_than_one_launch_of_listed_positions(dev):
    """130 listed positions: two launches of the writing tile, the second with one ragged row block."""
    case = ref.Case(17, 129)
    sel = [int(i) for i in np.random.default_rng(5).integers(0, 17, 130)]
    res, _ = _run(case, sel, dev)
    ref.check(case, res, sel)


@pytest.mark.parametrize("m,n,pivot", [(17, 40, 5), (129, 300, 70)])
def test_a_zero_pivot_breaks_its_rows_only(dev, m, n, pivot):
    case = ref.Case(m, n, zero_pivot=pivot, mask="random")
    sel = [0, pivot, pivot + 1, m - 1]
    res, again = _run(case, sel, dev)
    assert np.array_equal(res["stats"], again[1], equal_nan=True)
    ref.check(case, res, sel)
    assert res["status"] & 1
    assert np.isnan(res["coef"][: pivot + 1]).all() and np.isnan(res["stats"][: pivot + 1]).all()
    assert np.isfinite(res["coef"][pivot + 1:]).all() and np.isfinite(res["stats"][pivot + 1:]).all()
    assert np.isnan(res["mu_out"][:2, :n]).all() and np.isfinite(res["mu_out"][2:, :n]).all()


def test_no_rows(dev):
    """n == 0: stage 1 only; the coefficients are there, the statistics are zero."""
    case = ref.Case(5, 0)
    res, _ = _run(case, None, dev)
    ref.check(case, res)
    assert not res["stats"].any() and np.isfinite(res["coef"]).all()


# ---------------------------------------------------------------------------------------------------------- end to end
N, D, NOISE = 60, 6, 1e-2
LS = float(np.sqrt(D / 12.0))
SEED = 23


def _rows():
    """Rows that a float16 holds exactly: the plain-array learner on them is the learner on the widened compact store."""
    t16 = torch.from_numpy(np.random.default_rng(SEED).random((N + 1, D))).to(torch.float16)
    return t16, t16.to(torch.float64).numpy()


def _labels(X):
    rng = np.random.default_rng(SEED + 1)
    ids = [int(i) for i in rng.choice(N, 20, replace=False)]
    fb = {i: (1 if X[i, 0] + X[i, 1] > 1.0 else -1) for i in ids}
    fb[ids[0]], fb[ids[1]] = 1, -1                                       # both signs, whatever the draw
    fb[ids[2]] = -fb[ids[2]]                                              # and one slip for audit() to find
    return fb


def _learner(data, query, dev, **kw):
    from ital_amd import ITAL
    L = ITAL(data, queries=[query], length_scale=LS, noise=NOISE, device=dev, **kw)
    fb = _labels(_rows()[1])
    ids = list(fb)
    L.update({i: fb[i] for i in ids[:12]})
    L.update({i: fb[i] for i in ids[12:]})
    return L


def _snapshot(L):
    a = L.audit()
    ids = [int(i) for i in a["ids"]]
    mean, var = L.preview_revoke(ids)
    return a, mean, var


@pytest.fixture(scope="module")
def session(dev):
    """The learner on a DeviceData (clone() shares the rows of one), its audit and previews, and what clone() + revoke([i])
    gives for every labelled i."""
    from ital_amd import DeviceData
    _, X = _rows()
    L = _learner(DeviceData(torch.from_numpy(X[:N]).to(dev), device=dev), X[N], dev)
    a, mean, var = _snapshot(L)
    clones = []
    for i in a["ids"]:
        C = L.clone()
        C.revoke([int(i)])
        clones.append((np.asarray(C.rel_mean).copy(), C.gp.predict_stored(cov_mode='diag')[1].copy(), C.gp._full(C.gp.s2).copy()))
    K = L.gp.K
    tol = 64 * L.gp.m * U * np.linalg.cond(K)
    return dict(L=L, audit=a, mean=mean, var=var, clones=clones, tol=tol, X=X)


def test_preview_revoke_equals_clone_and_revoke(session):
    s = session
    a, tol = s["audit"], s["tol"]
    assert len(a["ids"]) == 20 and s["L"].gp.m == 21 and set(a["label"]) == {1.0, -1.0}
    assert tol < 1e-9
    for q in range(20):
        cm, cv, _ = s["clones"][q]
        dm, dv = np.abs(s["mean"][q] - cm), np.abs(s["var"][q] - cv)
        print("label %d: |mean - clone| %.3e, |var - clone| %.3e, bound %.3e" % (a["ids"][q], dm.max(), dv.max(), tol))
        assert np.all(dm <= tol * np.maximum(1, np.abs(cm)))
        assert np.all(dv <= tol * np.maximum(1, np.abs(cv)))
    # nothing changed in the session, and the calls repeat in bits
    a2, mean2, var2 = _snapshot(s["L"])
    assert all(np.array_equal(a[k], a2[k]) for k in a if a[k] is not None)
    assert np.array_equal(mean2, s["mean"]) and np.array_equal(var2, s["var"])


def test_audit_equals_what_the_clones_say(session):
    s = session
    L, a, tol = s["L"], s["audit"], s["tol"]
    unseen = np.asarray(L.get_unseen())
    assert len(unseen) == N - 20
    mean0, s20 = np.asarray(L.rel_mean), L.gp._full(L.gp.s2)
    y = a["label"]
    for q in range(20):
        cm, _, cs2 = s["clones"][q]
        dmu = (cm - mean0)[unseen]
        tq = tol * np.maximum(1, np.abs(cm[unseen]))
        assert abs(a["dmu_max"][q] - np.abs(dmu).max()) <= tq.max()
        assert abs(a["dmu_rms"][q] - np.sqrt((dmu ** 2).mean())) <= tq.max()
        assert abs(a["ds2"][q] - (cs2 - s20)[unseen].sum()) <= len(unseen) * tol * max(1.0, np.abs(cs2).max())
        ambiguous = np.abs(cm[unseen]) <= tq
        certain = (((mean0[unseen] > 0) != (cm[unseen] > 0)) & ~ambiguous).sum()
        assert ambiguous.sum() == 0                                       # the seed was chosen so
        assert certain <= a["flips"][q] <= certain + ambiguous.sum()
    # the leave-one-out prediction of a label is the clone's prediction AT the sample (variance of the noisy target)
    for q, i in enumerate(a["ids"]):
        cm, cv, _ = s["clones"][q]
        assert abs(a["loo_mean"][q] - cm[i]) <= tol * max(1, abs(cm[i]))
        assert abs(a["loo_var"][q] - (cv[i] + NOISE)) <= tol * max(1, cv[i])
    from scipy.special import ndtr
    d = ndtr(-y * a["loo_mean"] / np.sqrt(a["loo_var"]))
    assert np.array_equal(a["disagreement"], d) and a["p_mistake"] is None
    assert a["order"].tolist() == sorted(range(20), key=lambda q: (-d[q], q))
    b = L.audit(mistake_prob=0.1, unseen_only=False)
    assert np.allclose(b["p_mistake"], 0.1 * d / (0.1 * d + 0.9 * (1 - d)), rtol=1e-15, atol=0)
    assert np.all(b["flips"] >= a["flips"]) and np.all(b["ds2"] >= a["ds2"]) and np.all(b["dmu_max"] >= a["dmu_max"])
    for k in ("ids", "label", "loo_mean", "loo_var", "disagreement", "order"):
        assert np.array_equal(a[k], b[k])


def test_refusals_and_unnameable(session, dev):
    from ital_amd import ITAL
    L = session["L"]
    labelled = int(session["audit"]["ids"][0])
    unseen = L.get_unseen()
    with pytest.raises(ValueError):
        L.preview_revoke([unseen[0]])
    with pytest.raises(ValueError):
        L.gp.preview_remove([unseen[0]])
    with pytest.raises(ValueError):
        L.gp.preview_remove([N])                                          # the query row
    fresh = ITAL(session["X"][:N], length_scale=LS, noise=NOISE, device=dev)
    with pytest.raises(RuntimeError):
        fresh.audit()
    C = L.clone()
    C.update({unseen[0]: 0})                                              # unnameable: no label to lose
    mean, var = C.preview_revoke([unseen[0], labelled])
    assert np.array_equal(mean[0], np.asarray(C.rel_mean)) and np.array_equal(var[0], C.gp.predict_stored(cov_mode='diag')[1])
    assert np.array_equal(mean[1], session["mean"][0]) and np.array_equal(var[1], session["var"][0])
    assert C.audit(unseen_only=False)["ids"].tolist() == session["audit"]["ids"].tolist()
    noisy = ITAL(session["X"][:N], length_scale=LS, noise=NOISE, device=dev, label_prob=0.8, mistake_prob=0.05)
    noisy.update({int(i): int(v) for i, v in zip(session["audit"]["ids"], session["audit"]["label"])})
    p = noisy.audit()
    d = p["disagreement"]
    assert np.allclose(p["p_mistake"], 0.05 * d / (0.05 * d + 0.95 * (1 - d)), rtol=1e-15, atol=0)


@pytest.mark.parametrize("kind", ["plain_array", "compact_f16"])
def test_plain_array_and_compact_store_agree_in_bits_with_the_device_data(session, dev, kind):
    from ital_amd import DeviceData
    t16, X = _rows()
    if kind == "plain_array":
        store = X[:N]
    else:
        store = DeviceData(t16[:N].to(dev), device=dev, storage="source")
        assert store.storage is torch.float16
    a, mean, var = _snapshot(_learner(store, X[N], dev))
    for k, v in session["audit"].items():
        assert (v is None and a[k] is None) or np.array_equal(a[k], v), k
    assert np.array_equal(mean, session["mean"]) and np.array_equal(var, session["var"])


# ------------------------------------------------------------------------------------------------------------ two ranks
def _rank_influence(rank, world, port, mode, out):
    dev, group = _ranks.join(rank, world, port, mode)
    try:
        _, X = _rows()
        L = _learner(X[:N], X[N], dev, rank=rank, world=world, group=group)
        mask = np.zeros(N, dtype=bool)
        mask[L.get_unseen()] = True
        inf = L.gp.influence(mask)                                        # every rank makes the calls
        ids = [i for i in L.gp.ind if i < N][:3]
        mean, var = L.gp.preview_remove(ids)
        tol = 64 * L.gp.m * U * np.linalg.cond(L.gp.K)
        out[rank] = (inf, mean, var, L.audit(), tol)
    finally:
        _ranks.leave(group)


def test_two_ranks_like_one():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    one = _ranks.spawn(_rank_influence, 1, None)[0]
    two = _ranks.spawn(_rank_influence, 2, "gloo")
    # B has the same bits wherever its column lies (the k-order of the tile does not depend on it), so a sum differs from
    # the one-rank sum by the order of its N terms alone: both are within gamma_N of the exact sum of the same positive terms
    g = 2 * float(ref.gamma(N + 2))
    for inf, mean, var, audit, tol in two:
        for k in ("c", "w", "loo_mean", "loo_var", "dmu_max", "flips"):
            assert np.array_equal(inf[k], one[0][k]), k
        for k in ("dmu_sq", "ds2"):
            assert np.all(np.abs(inf[k] - one[0][k]) <= g * np.abs(one[0][k])), k
        assert mean.shape == (3, N) and var.shape == (3, N)
        assert np.all(np.abs(mean - one[1]) <= tol * np.maximum(1, np.abs(one[1])))
        assert np.all(np.abs(var - one[2]) <= tol * np.maximum(1, np.abs(one[2])))
        assert np.array_equal(audit["order"], one[3]["order"]) and np.array_equal(audit["flips"], one[3]["flips"])
    for k in two[0][0]:
        assert np.array_equal(two[0][0][k], two[1][0][k]), k
    assert np.array_equal(two[0][1], two[1][1]) and np.array_equal(two[0][2], two[1][2])     # full length, the same on both


# -------------------------------------------------------------------------------------------------------- context layer
def test_ctx_audit_against_the_python_learner(dev):
    from ital_amd import ITAL, _lib
    lib = _lib.load()
    _, X = _rows()
    X = np.ascontiguousarray(X[:N])
    fb = _labels(_rows()[1])
    ids = list(fb)
    blocks = [ids[:16], ids[16:]]                                         # appends of 16 and 4: the blocks ital_ctx_update makes
    L = ITAL(X, length_scale=LS, noise=NOISE, device=dev)
    h = ctypes.c_void_p()
    assert lib.ital_ctx_create(N, D, LS, 1.0, NOISE, 64, 0, 1, None, ctypes.byref(h)) == 0
    try:
        assert lib.ital_ctx_fit(h, X.ctypes.data, 0, None) == 0
        for blk in blocks:
            L.update({i: fb[i] for i in blk})
            order = [int(i) for i in L.gp.ind[-len(blk):]]                # relevant first, as the learner hands them on
            idx, y = np.asarray(order, dtype=np.int64), np.asarray([fb[i] for i in order], dtype=np.float64)
            assert lib.ital_ctx_update(h, idx.ctypes.data, y.ctypes.data, len(idx), None) == 0, lib.ital_last_error()
        params = np.array([[LS, 1.0, NOISE], [0.5, 1.0, 1e-3]])

        def evidence():
            scores, ok = np.zeros((2, 3)), np.zeros(2, dtype=np.int32)
            assert lib.ital_ctx_evidence(h, params.ctypes.data, 2, scores.ctypes.data, ok.ctypes.data, None) == 0
            return scores

        before = evidence()
        out_ids, table, count = np.full(64, -1, dtype=np.int64), np.full((64, 8), np.nan), ctypes.c_int(-1)
        assert lib.ital_ctx_audit(h, 1, None, table.ctypes.data, ctypes.byref(count), None) == -22        # refused ...
        assert lib.ital_ctx_audit(h, 1, out_ids.ctypes.data, table.ctypes.data, None, None) == -22
        assert count.value == -1 and np.isnan(table).all() and np.array_equal(evidence(), before)        # ... nothing changed
        for unseen_only in (1, 0):
            assert lib.ital_ctx_audit(h, unseen_only, out_ids.ctypes.data, table.ctypes.data, ctypes.byref(count), None) == 0, \
                lib.ital_last_error()
            a = L.audit(unseen_only=bool(unseen_only))
            m = count.value
            assert m == 20 and out_ids[:m].tolist() == a["ids"].tolist() and np.isnan(table[m:]).all()
            t = table[:m]
            # the two sessions hold the same state (tests/test_gpu_ctx_live.py) and run the same kernels: equal bits, except
            # for the normal distribution function, which each side takes from its own library
            for col, k in ((0, "label"), (1, "loo_mean"), (2, "loo_var"), (4, "dmu_rms"), (5, "dmu_max"), (6, "flips"), (7, "ds2")):
                assert np.array_equal(t[:, col], a[k]), (k, np.abs(t[:, col] - a[k]).max())
            assert np.all(np.abs(t[:, 3] - a["disagreement"]) <= 8 * U * np.maximum(a["disagreement"], 2.0 ** -1022))
        assert np.array_equal(evidence(), before)
    finally:
        assert lib.ital_ctx_destroy(h) == 0
