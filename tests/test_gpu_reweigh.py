"""Per-label noise on the device (GaussianProcess.reweigh, ActiveRetrievalBase.set_label_noise, ital_gp_reweigh;
csrc/reweigh.hip) against the dense model of tests/_reweigh_ref.py: the GP on K_TT + noise I + diag(e) in numpy float64.

Bound for mean, variance, a full covariance block of 12 rows, K and w (tests/test_gpu_revoke.py):
|device - model| <= max(1e-10, 1e-15 cond) * max(1, max|model|),  cond the dpocon estimate of the worse-conditioned of the
labelled Gram before and after the call.  Run: python -m pytest tests -m gpu."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ranks  # noqa: E402
import _reweigh_ref as ref  # noqa: E402

LS = 0.7


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


@pytest.fixture(scope="module")
def X():
    return np.random.default_rng(1).random((301, 5))        # 301 rows: ldv = 304, three pad columns


def _gp(X, ls, dev, sizes, seed, capacity=None):
    from ital_amd import GaussianProcess
    rng = np.random.default_rng(seed)
    ind = [int(i) for i in rng.choice(len(X), sum(sizes), replace=False)]
    y = rng.choice([-1.0, 1.0], size=len(ind))
    gp = GaussianProcess(X, ls, device=dev, capacity=capacity)
    at = 0
    for c in sizes:
        gp.update(ind[at:at + c], y[at:at + c])
        at += c
    return gp, ind, y


def _model(gp, X, ls, e=None):
    """The dense model of what the session holds now: its labelled rows, labels and per-label noise (or `e` instead)."""
    XT = gp.XT[: gp.m, : gp.d].cpu().numpy()          # data rows and query rows alike
    return ref.Dense(X, XT, gp.y, gp.label_noise if e is None else e, ls, float(gp.var), float(gp.noise))


def _check(gp, X, ls, cond, e=None):
    D = _model(gp, X, ls, e)
    cond = max(cond, D.cond)
    ref.within(gp.predict_stored(), D.mean, cond, "mean")
    ref.within(gp.predict_stored(cov_mode="diag")[1], np.maximum(0, D.var), cond, "variance")
    ref.within(gp.predict_stored(D.rows, cov_mode="full")[1], D.cov, cond, "covariance")
    ref.within(gp.K, D.K, cond, "K")
    ref.within(gp.w, D.w, cond, "w")
    return D


def _check_structure(gp):
    """As tests/test_gpu_revoke.py::_check_structure: L lower triangular with a positive diagonal, rows >= m of L and V zero,
    the pad columns finite, status 0; label_noise in step with ind."""
    m = gp.m
    L = gp.L.cpu().numpy()
    assert np.all(np.triu(L[:m, :m], 1) == 0)
    assert np.all(np.diag(L[:m, :m]) > 0)
    assert np.all(L[m:] == 0) and np.all(L[:, m:] == 0)
    assert np.all(gp.V[m:].cpu().numpy() == 0)
    assert np.all(gp.alpha[m:].cpu().numpy() == 0)
    assert np.all(np.isfinite(gp.V.cpu().numpy()))                   # the pad columns included
    assert int(gp.status.item()) == 0
    assert len(gp.ind) == m == len(gp.y) == len(gp.label_noise) and sum(abs(c) for c in gp.appends) == m


def _state(gp):
    return [t.cpu().numpy().copy() for t in (gp.L, gp.alpha, gp.V, gp.mu, gp.s2)]


# ------------------------------------------------------------------------------------------------------ GP level
def test_one_label_up_and_down_again(dev, X):
    """130 labels from updates of 1, 16 x 8, 1 into a capacity of 64 (it grows twice); one label at a time, at the first
    position, 63, 64, the middle and the last: up from 0, checked, down to 0 again, checked against the model with e = 0."""
    gp, ind, y = _gp(X, LS, dev, [1] + [16] * 8 + [1], 2, capacity=64)
    assert gp.m == 130 and gp.cap > 64
    appends = list(gp.appends)
    for p, extra in ((0, 0.3), (63, 0.05), (64, 2.0), (65, 0.3), (129, 0.7)):
        cond = _model(gp, X, LS).cond
        assert gp.reweigh([ind[p]], extra) is gp
        want = np.zeros(130)
        want[p] = extra
        assert np.array_equal(gp.label_noise, want) and gp.ind == ind and gp.appends == appends
        _check_structure(gp)
        _check(gp, X, LS, cond)
        gp.reweigh([ind[p]], 0.0)
        assert np.array_equal(gp.label_noise, np.zeros(130))
        _check_structure(gp)
        _check(gp, X, LS, cond, e=np.zeros(130))
    print("worst ratio: %.3g" % ref.WORST[0])


def test_zero_deltas_change_no_bit(dev, X):
    gp, ind, y = _gp(X, LS, dev, [1, 16, 7], 3)
    gp.reweigh([ind[4], ind[20]], [0.2, 0.4])
    before = _state(gp)
    launches = gp._lib.ital_launch_count()
    gp.reweigh([ind[4], ind[20], ind[7]], [0.2, 0.4, 0.0])
    gp.reweigh([], 1.0)
    assert gp._lib.ital_launch_count() == launches               # no launch at all
    for a, b in zip(_state(gp), before):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("r", [8, 9])
def test_many_labels_in_one_call_equal_single_calls(dev, X, r):
    """Eight labels are one sweep, nine are two; increases and decreases mixed, adjacent positions and position 0 among them."""
    a, ind, y = _gp(X, LS, dev, [1, 16, 16, 16, 16, 5], 4)
    b, _, _ = _gp(X, LS, dev, [1, 16, 16, 16, 16, 5], 4)
    pos = [0, 1, 17, 31, 32, 63, 64, 69, 40][:r]
    start = {ind[p]: 0.25 for p in pos[1::2]}                      # every other one comes down, the rest go up
    for gp in (a, b):
        gp.reweigh(list(start), list(start.values()))
    cond = _model(a, X, LS).cond
    target = {ind[p]: (0.0 if t % 4 == 1 else 0.1 if t % 4 == 3 else 0.2 + 0.1 * t) for t, p in enumerate(pos)}
    launches = a._lib.ital_launch_count()
    a.reweigh(list(target), list(target.values()))
    assert a._lib.ital_launch_count() - launches == (2 if r <= 8 else 4)      # factor and sweep per group of eight
    for i, v in target.items():
        b.reweigh([i], v)
    assert np.array_equal(a.label_noise, b.label_noise)
    assert sorted(np.flatnonzero(a.label_noise)) == sorted(p for p in pos if target[ind[p]] > 0)
    for gp in (a, b):
        _check_structure(gp)
        D = _check(gp, X, LS, cond)
    ref.within(a.predict_stored(), b.predict_stored(), max(cond, D.cond), "one vs %d" % r)
    ref.within(a.predict_stored(cov_mode="diag")[1], b.predict_stored(cov_mode="diag")[1], max(cond, D.cond), "one vs %d, var" % r)
    print("worst ratio: %.3g" % ref.WORST[0])


def test_reweigh_over_three_blocks_at_cond_1e8(dev):
    """The conditioned case of test_gpu_revoke.py::test_remove_over_three_blocks_at_cond_1e8: 301 x 3, length scale 1.0, 130
    labels, cond about 1e8 -- the cond-scaled branch of the bound is the one that holds."""
    X3 = np.random.default_rng(3).random((301, 3))
    gp, ind, y = _gp(X3, 1.0, dev, [16] * 8 + [2], 4)
    cond0 = _model(gp, X3, 1.0).cond
    print("cond of the 130-label Gram: %.3g" % cond0)
    assert 1e-15 * cond0 > 1e-10
    gp.reweigh([ind[0]], 1e-4)
    _check(gp, X3, 1.0, cond0)
    gp.reweigh([ind[1], ind[60], ind[129]], [1e-3, 1e-5, 1e-4])
    _check_structure(gp)
    _check(gp, X3, 1.0, cond0)
    gp.reweigh([ind[0], ind[60]], 0.0)                              # downdates at this conditioning
    _check_structure(gp)
    _check(gp, X3, 1.0, cond0)
    print("worst ratio: %.3g" % ref.WORST[0])


def _raw_call(gp, pos, delta, status):
    from ital_amd import _lib
    lib = gp._lib
    r = len(pos)
    work = torch.empty(int(lib.ital_gp_reweigh_workspace(gp.m, r)), dtype=torch.float64, device=gp.device)
    d = _lib.ItalReweighDesc()
    d.L, d.ldl, d.alpha, d.m = gp.L.data_ptr(), gp.cap, gp.alpha.data_ptr(), gp.m
    d.V, d.ldv, d.n, d.mu, d.s2 = gp.V.data_ptr(), gp.ldv, gp.n, gp.mu.data_ptr(), gp.s2.data_ptr()
    d.work, d.work_doubles, d.status, d.r = work.data_ptr(), work.numel(), status.data_ptr(), r
    cpos, cdelta = (ctypes.c_int * r)(*pos), (ctypes.c_double * r)(*delta)
    d.pos, d.delta = ctypes.cast(cpos, ctypes.c_void_p), ctypes.cast(cdelta, ctypes.c_void_p)
    rc = lib.ital_gp_reweigh(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def test_refusal_changes_nothing(dev, X):
    """A delta below -(e_p + noise) -- here below -K_pp, so the changed Gram has a negative diagonal entry and a pivot goes
    non-positive by construction -- on a well-conditioned m = 20: the status bit, and every byte as it was.  As the only
    label, as the second of two (the first chain ran on the workspace copy), as the last and as the first of nine (the
    second group's kernels return early)."""
    gp, ind, y = _gp(X, 0.3, dev, [1, 16, 3], 5)
    assert gp.m == 20 and _model(gp, X, 0.3).cond < 1e4
    gp.reweigh([ind[6]], 0.5)
    before = _state(gp)
    ok = [0.1, 0.2, 0.3, 0.1, 0.1, 0.2, -0.3, 0.3, 0.1]            # position 6 carries 0.5: -0.3 is a sound downdate
    for pos, delta in (([6], [-2.0]), ([2, 6], [0.3, -2.0]), (list(range(9)), ok[:8] + [-2.0]),
                       (list(range(9)), [-2.0] + ok[1:]), ([19], [-1.5])):
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        assert _raw_call(gp, pos, delta, status) == 0
        assert int(status.item()) & 1
        for a, b in zip(_state(gp), before):
            assert a.tobytes() == b.tobytes()
    assert int(gp.status.item()) == 0
    status = torch.zeros(1, dtype=torch.int32, device=dev)          # and the same route accepts a sound call
    assert _raw_call(gp, [2, 6], [0.3, -0.3], status) == 0 and int(status.item()) == 0
    gp.label_noise[2], gp.label_noise[6] = 0.3, 0.2
    _check(gp, X, 0.3, 1.0)


def test_reweigh_then_remove_and_update(dev, X):
    gp, ind, y = _gp(X, LS, dev, [1, 16, 16, 3], 6)
    rest = [i for i in range(301) if i not in ind]
    gp.reweigh([ind[3], ind[20], ind[30]], [0.4, 0.1, 0.2])
    cond = _model(gp, X, LS).cond
    gp.remove([ind[10]])                                            # another label: e moves up with the positions
    assert gp.label_noise[3] == 0.4 and gp.label_noise[19] == 0.1 and gp.label_noise[29] == 0.2
    _check_structure(gp)
    _check(gp, X, LS, cond)
    gp.remove([ind[20]])                                            # a reweighed label itself
    assert gp.label_noise[3] == 0.4 and gp.label_noise[28] == 0.2 and np.count_nonzero(gp.label_noise) == 2
    _check_structure(gp)
    _check(gp, X, LS, cond)
    gp.update(rest[:5], [1, -1, 1, 1, -1])                          # an append onto a reweighed factor
    assert len(gp.label_noise) == gp.m == 39 and np.all(gp.label_noise[-5:] == 0)
    _check_structure(gp)
    _check(gp, X, LS, cond)
    gp.update([ind[20]], [y[20]])                                   # back with its full weight
    assert gp.label_noise[-1] == 0
    gp.reweigh([rest[2], ind[3]], [0.3, 0.0])
    _check(gp, X, LS, cond)


def test_set_params_keeps_the_label_noise(dev, X):
    gp, ind, y = _gp(X, LS, dev, [1, 16, 16, 3], 7)
    gp.reweigh([ind[0], ind[17], ind[35]], [0.3, 0.1, 0.6])
    e = gp.label_noise.copy()
    cond = _model(gp, X, LS).cond
    gp.set_params(length_scale=0.55, var=1.3, noise=1e-4)
    assert np.array_equal(gp.label_noise, e)
    _check_structure(gp)
    D = _check(gp, X, 0.55, cond)
    assert abs(D.K[17, 17] - (1.3 + 1e-4 + 0.1)) < 1e-12            # the model really is the one at the new parameters
    gp.reweigh([ind[17]], 0.0)                                      # and the session goes on from there
    _check(gp, X, 0.55, cond)


# ------------------------------------------------------------------------------------------------------ learner level
def _truth(X, i):
    return 1 if X[i, 0] > 0.5 else -1


def _gaps(scores, cand, picks):
    """(best - second best) / max|MI| of every greedy step over the list positions that were still live in it."""
    out = []
    for t, s in enumerate(scores):
        live = s[: len(cand)][~np.isin(cand, picks[:t])]
        live = np.sort(live)[::-1]
        out.append((live[0] - live[1]) / np.max(np.abs(live)))
    return out


def test_ital_round_on_weighted_labels_equals_a_reloaded_session(dev):
    """ITAL, 120 x 4, k = 3: two labels are softened, then a round is fetched; a second learner reaches the same weights by
    load_state_dict (a replay of the appends followed by reweigh) and fetches the same round."""
    from ital_amd import ITAL, mvn_stream
    rng = np.random.default_rng(2)
    X4 = rng.random((120, 4))
    ls = float(np.sqrt(4 / 12.0))
    mvn_stream.GLOBAL.reset()
    A = ITAL(X4, length_scale=ls, device=dev)
    first = {int(i): _truth(X4, i) for i in rng.choice(120, 5, replace=False)}
    A.update(first)
    got = A.fetch_unlabelled(3)
    A.update({i: _truth(X4, i) for i in got})
    unseen = A.get_unseen()
    with pytest.raises(ValueError):
        A.set_label_noise({unseen[0]: 0.1})
    A.set_label_noise({got[1]: 0.5, list(first)[2]: 0.05})
    assert A.label_noise() == {got[1]: 0.5, list(first)[2]: 0.05}
    assert A.get_unseen() == unseen and A.rounds == 2
    D = _model(A.gp, X4, ls)
    ref.within(A.rel_mean, D.mean, D.cond, "rel_mean")
    for call in (lambda: A.gp.evidence([dict(length_scale=0.5)]), lambda: A.gp.evidence_grad([dict(length_scale=0.5)]),
                 lambda: A.gp.loo_grad([dict(length_scale=0.5)]), lambda: A.tune_params(), lambda: A.fit_params()):
        with pytest.raises(ValueError, match="set_label_noise"):
            call()
    sd = A.state_dict()
    assert sd["version"] == 1 and np.count_nonzero(sd["label_noise"]) == 2
    B = ITAL(X4, length_scale=ls, device=dev).load_state_dict(sd)
    assert B.gp.ind == A.gp.ind and np.array_equal(B.gp.label_noise, A.gp.label_noise) and B.label_noise() == A.label_noise()
    ref.within(B.rel_mean, D.mean, D.cond, "reloaded")
    A.keep_scores = B.keep_scores = True
    cand = np.asarray(A.get_unseen())
    mvn_stream.GLOBAL.reset()
    pa = A.fetch_unlabelled(3)
    sa = [s.cpu().numpy().copy() for s in A.last_scores]
    mvn_stream.GLOBAL.reset()
    pb = B.fetch_unlabelled(3)
    sb = [s.cpu().numpy() for s in B.last_scores]
    gaps = _gaps(sa, cand, pa)
    print("MI gaps (best - second) / max|MI|:", gaps)
    assert min(gaps) > 1e-6                          # no tie: a differing pick would be this feature's fault, not rounding's
    assert pa == pb and len(pa) == 3
    for t in range(3):
        np.testing.assert_allclose(sa[t], sb[t], rtol=1e-8, atol=1e-10, err_msg="step %d" % t)
    A.keep_scores = False
    A.update({i: _truth(X4, i) for i in pa})         # and the loop goes on; the weights stay with their labels
    assert A.label_noise() == {got[1]: 0.5, list(first)[2]: 0.05}
    A.set_label_noise({got[1]: 0.0})
    assert A.label_noise() == {list(first)[2]: 0.05} and "label_noise" in A.state_dict()
    A.set_label_noise({list(first)[2]: 0.0})
    assert "label_noise" not in A.state_dict()
    A.gp.evidence([dict(length_scale=0.5)])          # no weight is left: the evidence family answers again


def test_audit_on_weighted_labels(dev):
    from ital_amd import ITAL
    rng = np.random.default_rng(8)
    X4 = rng.random((120, 4))
    A = ITAL(X4, length_scale=0.6, device=dev)
    fb = {int(i): _truth(X4, i) for i in rng.choice(120, 24, replace=False)}
    A.update(fb)
    ids = list(A.gp.ind)                              # labelled order: the relevant ones of the call first
    A.set_label_noise({ids[0]: 0.3, ids[7]: 0.05, ids[23]: 1.0})
    D = _model(A.gp, X4, 0.6)
    lm, lv = D.loo(A.gp.y)
    au = A.audit()
    assert au["ids"].tolist() == ids
    ref.within(au["loo_mean"], lm, D.cond, "loo_mean")
    ref.within(au["loo_var"], lv, D.cond, "loo_var")
    mean, var = A.preview_revoke([ids[7]])           # reads L, alpha, V only: the state without that label, e carried along
    keep = [t for t in range(24) if t != 7]
    W = ref.Dense(X4, X4[[ids[t] for t in keep]], A.gp.y[keep], A.gp.label_noise[keep], 0.6)
    ref.within(mean[0], W.mean, D.cond, "preview mean")
    ref.within(var[0], np.maximum(0, W.var), D.cond, "preview var")


def test_emoc_and_the_evidence_family_on_weighted_labels(dev):
    """EMOC reads the factor to whiten its query columns: with queries, after a reweigh, against the dense formula
    (P(+) |1 - mu| + P(-) |-1 - mu|) / (s2 + noise) * mean_j |Sigma_ij| over the data rows and the queries."""
    from scipy.special import ndtr
    import scipy.linalg
    from ital_amd import tune
    from ital_amd.baselines import EMOC
    rng = np.random.default_rng(9)
    X4 = rng.random((120, 4))
    Q = X4[:2] + 0.01
    A = EMOC(X4, queries=Q, length_scale=0.6, device=dev)
    fb = {int(i): _truth(X4, i) for i in rng.choice(120, 10, replace=False)}
    A.update(fb)
    A.set_label_noise({list(fb)[1]: 0.4, list(fb)[8]: 0.1})
    gp = A.gp
    XT = gp.XT[: gp.m, :4].cpu().numpy()
    Z = np.concatenate((X4, Q))
    K = ref.gram(XT, gp.label_noise, 0.6)
    c = scipy.linalg.cho_factor(K, lower=True)
    KXT, KTZ = ref.rbf(X4, XT, 0.6), ref.rbf(XT, Z, 0.6)
    mean = KXT @ scipy.linalg.cho_solve(c, gp.y)
    Sigma = ref.rbf(X4, Z, 0.6) - KXT @ scipy.linalg.cho_solve(c, KTZ)
    ind = np.asarray(A.get_unseen()[:40])
    var = np.maximum(0, np.diag(Sigma[:, :120]))
    spread = np.abs(Sigma).mean(axis=1)
    prob_neg = ndtr((0.0 - mean) / np.sqrt(var))
    want = ((1 - prob_neg) * np.abs((1 - mean) / (var + 1e-6)) + prob_neg * np.abs((-1 - mean) / (var + 1e-6))) * spread
    ref.within(A.emoc_scores(ind), want[ind], ref.cond(K), "EMOC")
    for call in (lambda: tune.session_scores(A, [dict(length_scale=0.5)]), lambda: A.tune_params(apply=False),
                 lambda: A.fit_params(apply=False), lambda: gp.evidence([dict(length_scale=0.5)])):
        with pytest.raises(ValueError, match="set_label_noise"):
            call()


# ------------------------------------------------------------------------------------------------------ two ranks
def _rank_session(rank, world, port, X, mode, out):
    dev, group = _ranks.join(rank, world, port, mode)
    try:
        from ital_amd import ITAL, mvn_stream
        mvn_stream.GLOBAL.reset()
        L = ITAL(X, length_scale=0.6, device=dev, rank=rank, world=world, group=group)
        L.update({5: 1, 77: -1, 140: 1})
        got = L.fetch_unlabelled(3)
        L.update({i: _truth(X, i) for i in got})
        L.set_label_noise({77: 0.4, got[0]: 0.1})    # both ranks make the same call
        L.set_label_noise({77: 0.2, 5: 0.3})
        picks = L.fetch_unlabelled(3)
        out[rank] = (got, picks, np.asarray(L.rel_mean).copy(), list(L.gp.ind), L.label_noise(), np.asarray(L.gp.y).copy())
    finally:
        _ranks.leave(group)


def test_two_ranks_reweigh_like_one():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    X = np.random.default_rng(41).random((151, 4))
    one = _ranks.spawn(_rank_session, 1, X, None)[0]
    two = _ranks.spawn(_rank_session, 2, X, "gloo")
    ids = one[3]
    e = np.asarray([one[4].get(i, 0.0) for i in ids])
    assert one[4] == {77: 0.2, 5: 0.3, one[0][0]: 0.1}
    D = ref.Dense(X, X[ids], one[5], e, 0.6)
    ref.within(one[2], D.mean, D.cond, "one rank")
    for r in two:
        assert r[0] == one[0] and r[1] == one[1] and r[3] == one[3] and r[4] == one[4] and np.array_equal(r[5], one[5])
        ref.within(r[2], one[2], D.cond, "two ranks")
    np.testing.assert_array_equal(two[0][2], two[1][2])
