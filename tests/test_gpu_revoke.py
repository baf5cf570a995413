"""Taking feedback back on the device (GaussianProcess.remove, ActiveRetrievalBase.revoke / relabel, ital_ctx_revoke;
csrc/revoke.hip) against the reference's own model of the SURVIVING labels: oracle.gp.OracleGP / oracle.ital.OracleITAL
fitted to the survivors in their original order and grouping -- what the reference could only reach by reset() and a replay
(ital/retrieval_base.py:183-189, ital/gp.py:141-161).

Bound for mean, variance, a full covariance block of 12 rows, K and w (the form of section 10 for
solves against a factor):  |device - oracle| <= max(1e-10, 1e-15 cond) * max(1, max|oracle|),  cond the dpocon estimate of
the labelled Gram before the removal.  Both sides carry that conditioning error.  Run: python -m pytest tests -m gpu."""
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

ROWS12 = [0, 3, 17, 64, 65, 100, 128, 199, 255, 256, 299, 300]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


def _cond(A):
    """The dpocon estimate, as tests/test_gpu_adapt.py computes it."""
    from scipy.linalg import lapack
    c, info = lapack.dpotrf(A, lower=1)
    assert info == 0
    rcond, _ = lapack.dpocon(c, np.abs(A).sum(axis=0).max(), uplo="L")
    return 1.0 / rcond


WORST = [0.0]        # the largest |device - oracle| / bound seen by this module (printed; DESIGN.md section 12 quotes it)


def _within(got, want, cond, what):
    bound = max(1e-10, 1e-15 * cond) * max(1.0, float(np.max(np.abs(want))))
    err = float(np.max(np.abs(np.asarray(got) - np.asarray(want))))
    WORST[0] = max(WORST[0], err / bound)
    print("%-10s err %.3g  bound %.3g  ratio %.3g  (cond %.3g; worst ratio so far %.3g)" % (what, err, bound, err / bound, cond,
                                                                                             WORST[0]))
    assert err <= bound, (what, err, bound, cond)


def _oracle(X, ls, gp):
    from oracle.gp import OracleGP
    return OracleGP(X, ls).fit(list(gp.ind), np.asarray(gp.y))


def _check_against_survivors(gp, X, ls, cond, rows=ROWS12):
    """The device state against the reference's model of what is labelled now; `cond`: of the Gram BEFORE the removal."""
    O = _oracle(X, ls, gp)
    rows = [r for r in rows if r < len(X)]
    _within(gp.predict_stored(), O.predict_stored(), cond, "mean")
    _within(gp.predict_stored(cov_mode="diag")[1], O.predict_stored(cov_mode="diag")[1], cond, "variance")
    _within(gp.predict_stored(rows, cov_mode="full")[1], O.predict_stored(rows, cov_mode="full")[1], cond, "covariance")
    _within(gp.K, O.K, cond, "K")
    _within(gp.w, O.w, cond, "w")


def _check_structure(gp):
    """L lower triangular with a positive diagonal; rows >= m of L, V and XT zero, as _alloc leaves them."""
    m = gp.m
    L = gp.L.cpu().numpy()
    assert np.all(np.triu(L[:m, :m], 1) == 0)
    assert np.all(np.diag(L[:m, :m]) > 0)
    assert np.all(L[m:] == 0) and np.all(L[:, m:] == 0)
    assert np.all(gp.V[m:].cpu().numpy() == 0)
    assert np.all(gp.XT[m:].cpu().numpy() == 0)
    assert np.all(gp.XTn[m:].cpu().numpy() == 0) and np.all(gp.alpha[m:].cpu().numpy() == 0)
    assert np.all(np.isfinite(gp.V.cpu().numpy()))                   # the pad columns included
    assert int(gp.status.item()) == 0
    assert len(gp.ind) == m == (0 if gp.y is None else len(gp.y)) and sum(abs(c) for c in gp.appends) == m


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


def _cond_now(X, ls, gp):
    return _cond(_oracle(X, ls, gp).K)


# ------------------------------------------------------------------------------------------------------ GP level
def test_remove_first_63_64_last_middle(dev):
    """301 x 6 (N no multiple of 16 or 64), 70 labels from updates of 1, 16, 16, 16, 16, 5; checked after every removal."""
    X = np.random.default_rng(1).random((301, 6))
    gp, ind, y = _gp(X, 0.7, dev, [1, 16, 16, 16, 16, 5], 2)
    assert gp.appends == [1, 16, 16, 16, 16, 5]
    want_appends = [[0, 16, 16, 16, 16, 5], [0, 16, 16, 16, 15, 5], [0, 16, 16, 16, 15, 4], [0, 16, 16, 16, 15, 3]]
    for step, pos in enumerate([0, 63, 64, "last", "middle"]):
        p = gp.m - 1 if pos == "last" else gp.m // 2 if pos == "middle" else pos
        cond = _cond_now(X, 0.7, gp)
        victim = gp.ind[p]
        survivors = [i for i in gp.ind if i != victim]
        gp.remove([victim])
        assert gp.ind == survivors
        if step < len(want_appends):
            assert gp.appends == want_appends[step]
        _check_structure(gp)
        _check_against_survivors(gp, X, 0.7, cond)
    assert gp.m == 65


def test_remove_over_three_blocks_at_cond_1e8(dev):
    """301 x 3, length scale 1.0, 130 labels: the trailing block spans three 64-column panels (129 rows, then exactly 128),
    and cond is about 1e8 -- the cond-scaled branch of the bound is the one that holds."""
    X = np.random.default_rng(3).random((301, 3))
    gp, ind, y = _gp(X, 1.0, dev, [16] * 8 + [2], 4)
    cond0 = _cond_now(X, 1.0, gp)
    print("cond of the 130-label Gram: %.3g" % cond0)
    assert 1e-15 * cond0 > 1e-10
    for p in (0, 0, 60):
        cond = _cond_now(X, 1.0, gp)
        gp.remove([gp.ind[p]])
        _check_structure(gp)
        _check_against_survivors(gp, X, 1.0, cond)
    assert gp.m == 127


def test_three_ids_in_one_call_equal_three_calls(dev):
    X = np.random.default_rng(5).random((301, 6))
    a, ind, y = _gp(X, 0.7, dev, [1, 16, 16, 7], 6)
    b, _, _ = _gp(X, 0.7, dev, [1, 16, 16, 7], 6)
    cond = _cond_now(X, 0.7, a)
    ids = [ind[20], ind[0], ind[21]]                 # two adjacent positions and position 0
    a.remove(ids)
    for i in ids:
        b.remove([i])
    assert a.ind == b.ind == [i for i in ind if i not in ids]
    assert a.appends == b.appends == [0, 16, 14, 7]
    assert np.array_equal(a.y, b.y)
    for gp in (a, b):
        _check_structure(gp)
        _check_against_survivors(gp, X, 0.7, cond)
    want = _oracle(X, 0.7, a).predict_stored()
    _within(a.predict_stored(), b.predict_stored(), cond, "one vs three")
    assert np.max(np.abs(want)) > 0


def test_remove_append_remove(dev):
    X = np.random.default_rng(7).random((301, 6))
    gp, ind, y = _gp(X, 0.7, dev, [1, 16, 3], 8)
    rest = [i for i in range(301) if i not in ind]
    cond = _cond_now(X, 0.7, gp)
    gp.remove([ind[5]])
    _check_against_survivors(gp, X, 0.7, cond)
    gp.update(rest[:5], [1, -1, 1, 1, -1])
    assert gp.appends == [1, 15, 3, 5]
    cond = _cond_now(X, 0.7, gp)
    _check_against_survivors(gp, X, 0.7, cond)       # an append onto a factor that a removal left
    gp.remove([rest[1], ind[0]])
    assert gp.appends == [0, 15, 3, 4]
    _check_structure(gp)
    _check_against_survivors(gp, X, 0.7, cond)
    gp.update([ind[5]], [y[5]])                      # the sample that left may be labelled again
    _check_against_survivors(gp, X, 0.7, _cond_now(X, 0.7, gp))


def test_remove_across_a_capacity_growth(dev):
    X = np.random.default_rng(9).random((301, 6))
    gp, ind, y = _gp(X, 0.7, dev, [1, 15], 10, capacity=16)
    assert gp.cap == 16
    rest = [i for i in range(301) if i not in ind]
    cond = _cond_now(X, 0.7, gp)
    gp.remove([ind[3]])                              # at full capacity
    _check_structure(gp)
    _check_against_survivors(gp, X, 0.7, cond)
    gp.update(rest[:6], [1, 1, -1, 1, -1, -1])       # 15 + 6: the buffers grow
    assert gp.cap > 16
    cond = _cond_now(X, 0.7, gp)
    gp.remove([ind[0], rest[2]])                     # in the grown buffers (leading dimension and workspace changed)
    _check_structure(gp)
    _check_against_survivors(gp, X, 0.7, cond)


def test_remove_all_equals_reset(dev):
    X = np.random.default_rng(11).random((301, 6))
    gp, ind, y = _gp(X, 0.7, dev, [1, 16, 4], 12)
    gp.remove(list(reversed(ind)))
    assert gp.m == 0 and gp.ind == [] and gp.y is None and gp.appends == []
    assert np.all(gp.mu.cpu().numpy() == 0) and np.all(gp.s2.cpu().numpy() == gp.var)
    assert np.all(gp.mu_all.cpu().numpy() == 0)
    _check_structure(gp)
    for t in (gp.L, gp.V, gp.XT, gp.XTn, gp.alpha):
        assert np.all(t.cpu().numpy() == 0)
    assert gp.K is None
    gp.update(ind[:7], y[:7])                        # and goes on as a fresh one does
    _check_against_survivors(gp, X, 0.7, _cond_now(X, 0.7, gp))


def test_remove_refuses(dev):
    from ital_amd import ITAL
    X = np.random.default_rng(13).random((40, 4))
    gp, ind, y = _gp(X, 0.8, dev, [5], 14)
    before = gp.predict_stored().copy()
    other = [i for i in range(40) if i not in ind][0]
    with pytest.raises(ValueError):
        gp.remove([other])
    with pytest.raises(ValueError):
        gp.remove([ind[0], other])
    with pytest.raises(ValueError):
        gp.remove([ind[0], ind[0]])
    with pytest.raises(ValueError):
        gp.remove([40])
    assert gp.remove([]) is gp
    assert gp.ind == ind and np.array_equal(gp.predict_stored(), before)
    L = ITAL(X, queries=X[:2] + 0.01, length_scale=0.8, device=dev)
    L.update({7: 1})
    assert L.gp.ind == [40, 41, 7] and L.gp.appends == [-2, 1]
    with pytest.raises(ValueError):
        L.gp.remove([40])                            # a query row: part of the learner's construction
    with pytest.raises(ValueError):
        L.revoke([8])                                # never got feedback
    L.revoke([7])
    assert L.gp.ind == [40, 41] and L.gp.appends == [-2, 0] and L.rel_mean is not None


# ------------------------------------------------------------------------------------------------------ learner level
def _truth(X, i):
    return 1 if X[i, 0] > 0.5 else -1


def _mi_gaps(trace):
    out = []
    for cand, vals, _ in trace:
        s = np.sort(vals)[::-1]
        out.append((s[0] - s[1]) / np.max(np.abs(vals)))
    return out


def test_ital_revoke_equals_a_fresh_session_on_the_survivors(dev):
    """ITAL, perfect user, 200 x 5, k = 4: two rounds, then one sample of round 1 is revoked.  Seed 1: OracleITAL's best and
    second best MI differ by >= 6e-4 of max|MI| at every step of the compared fetch (chosen on the CPU; asserted below)."""
    from oracle import mvn as omvn
    from oracle.ital import OracleITAL
    from ital_amd import ITAL, mvn_stream
    rng = np.random.default_rng(1)
    X = rng.random((200, 5))
    ls = float(np.sqrt(5 / 12.0))
    groups = [{int(i): _truth(X, i) for i in rng.choice(200, 5, replace=False)}]
    mvn_stream.GLOBAL.reset()
    A = ITAL(X, length_scale=ls, device=dev)
    A.update(groups[0])
    for _ in range(2):
        got = A.fetch_unlabelled(4)
        groups.append({i: _truth(X, i) for i in got})
        A.update(groups[-1])
    assert A.last_round[0] == 2                      # the retrieval loop: the device compacted its own list
    victim = list(groups[1])[1]
    cond = _cond_now(X, ls, A.gp)
    rounds = A.rounds
    assert victim not in A.get_unseen()
    A.revoke([victim])
    del groups[1][victim]
    assert victim in A.get_unseen() and A.rounds == rounds
    assert victim not in A.relevant_ids and victim not in A.irrelevant_ids
    assert A.gp.appends == [5, 3, 4]

    B = ITAL(X, length_scale=ls, device=dev)         # a fresh learner fed the surviving feedback
    O = OracleITAL(X, length_scale=ls)
    for g in groups:
        B.update(g)
        O.update(g)
    assert A.gp.ind == B.gp.ind == O.gp.ind
    _within(A.rel_mean, O.gp.predict_stored(), cond, "rel_mean")

    A.keep_scores = B.keep_scores = True
    mvn_stream.GLOBAL.reset()                        # one stream position for both
    pa = A.fetch_unlabelled(4)
    assert A.last_round[0] == 1                      # the list was uploaded, not compacted
    sa = [s.cpu().numpy().copy() for s in A.last_scores]
    mvn_stream.GLOBAL.reset()
    pb = B.fetch_unlabelled(4)
    sb = [s.cpu().numpy() for s in B.last_scores]
    omvn.rng_reset()
    po = [int(i) for i in O.fetch_unlabelled(4)]
    gaps = _mi_gaps(O.trace)
    print("oracle MI gaps (best - second) / max|MI|:", gaps)
    assert min(gaps) > 1e-6                          # no tie: a differing pick would be this feature's fault, not rounding's
    assert pa == pb == po
    for t in range(4):
        np.testing.assert_allclose(sa[t], sb[t], rtol=1e-8, atol=1e-10, err_msg="step %d" % t)
    A.keep_scores = False
    A.update({i: _truth(X, i) for i in pa})
    A.fetch_unlabelled(4)
    assert A.last_round[0] == 2                      # and the loop is back on the device list


def test_relabel_equals_a_fresh_session_with_the_corrected_label(dev):
    """Noisy user (label_prob 0.75, mistake_prob 0.25), 120 x 4, k = 3 (seed 2: the oracle's MI gaps are >= 1e-4)."""
    from ital_amd import ITAL, mvn_stream
    kw = dict(label_prob=0.75, mistake_prob=0.25)
    rng = np.random.default_rng(2)
    X = rng.random((120, 4))
    ls = float(np.sqrt(4 / 12.0))
    groups = [{int(i): _truth(X, i) for i in rng.choice(120, 5, replace=False)}]
    mvn_stream.GLOBAL.reset()
    A = ITAL(X, length_scale=ls, device=dev, **kw)
    A.update(groups[0])
    for _ in range(2):
        got = A.fetch_unlabelled(3)
        groups.append({i: _truth(X, i) for i in got})
        A.update(groups[-1])
    positive = [i for i, fb in groups[1].items() if fb > 0]
    assert positive
    i = positive[0]
    with pytest.raises(RuntimeError, match="Cannot change feedback once given."):
        A.update({i: -1})                            # update() refuses as before, and as the reference does
    assert i in A.relevant_ids
    cond = _cond_now(X, ls, A.gp)
    A.relabel({i: -1})
    assert i in A.irrelevant_ids and i not in A.relevant_ids and i not in A.get_unseen()
    groups[1] = {j: fb for j, fb in groups[1].items() if j != i}
    groups.append({i: -1})                           # the corrected label is the newest one
    assert A.gp.appends == [5, 2, 3, 1]
    B = ITAL(X, length_scale=ls, device=dev, **kw)
    for g in groups:
        B.update(g)
    assert A.gp.ind == B.gp.ind and np.array_equal(A.gp.y, B.gp.y)
    _within(A.rel_mean, _oracle(X, ls, A.gp).predict_stored(), cond, "rel_mean")
    A.keep_scores = B.keep_scores = True
    mvn_stream.GLOBAL.reset()
    pa = A.fetch_unlabelled(3)
    sa = [s.cpu().numpy().copy() for s in A.last_scores]
    mvn_stream.GLOBAL.reset()
    pb = B.fetch_unlabelled(3)
    assert pa == pb
    for t in range(3):
        np.testing.assert_allclose(sa[t], B.last_scores[t].cpu().numpy(), rtol=1e-8, atol=1e-10, err_msg="step %d" % t)
    A.relabel({i: -1, pa[0]: 1})                     # nothing differs for i: a plain update of the rest
    assert A.gp.ind[-1] == pa[0] and A.gp.ind.count(i) == 1


@pytest.mark.parametrize("name", ["MCMI_min", "AdaptAL", "BorderlineSampling"])
def test_other_learners_after_a_revoke(dev, name):
    import ital_amd
    from ital_amd import baselines, mvn_stream
    cls = getattr(ital_amd, name, None) or getattr(baselines, name)
    kw = dict(subsample=60) if name in ("MCMI_min", "AdaptAL") else {}
    rng = np.random.default_rng(21)
    X = rng.random((150, 4))
    groups = [{int(i): _truth(X, i) for i in rng.choice(150, 6, replace=False)}]
    A = cls(X, length_scale=0.6, device=dev, **kw)
    A.update(groups[0])
    np.random.seed(3)
    got = A.fetch_unlabelled(3)
    groups.append({i: _truth(X, i) for i in got})
    A.update(groups[-1])
    A.revoke([got[0], list(groups[0])[2]])
    del groups[1][got[0]]
    del groups[0][list(groups[0])[2]]
    B = cls(X, length_scale=0.6, device=dev, **kw)
    for g in groups:
        B.update(g)
    assert A.gp.ind == B.gp.ind and got[0] in A.get_unseen()
    np.random.seed(4)
    mvn_stream.GLOBAL.reset()
    pa = A.fetch_unlabelled(3)
    np.random.seed(4)
    mvn_stream.GLOBAL.reset()
    pb = B.fetch_unlabelled(3)
    assert pa == pb and len(pa) == 3


def test_state_round_trip_after_a_revoke(dev):
    from ital_amd import ITAL, mvn_stream
    rng = np.random.default_rng(31)
    X = rng.random((90, 4))
    mvn_stream.GLOBAL.reset()
    A = ITAL(X, length_scale=0.6, device=dev)
    first = {int(i): _truth(X, i) for i in rng.choice(90, 3, replace=False)}
    A.update(first)
    got = A.fetch_unlabelled(3)
    A.update({i: _truth(X, i) for i in got})
    A.revoke([list(first)[0], got[1]])
    sd = A.state_dict()
    assert sd["appends"] == [2, 2]
    B = ITAL(X, length_scale=0.6, device=dev).load_state_dict(sd)
    assert B.gp.ind == A.gp.ind and B.gp.appends == [2, 2]
    assert B.relevant_ids == A.relevant_ids and B.irrelevant_ids == A.irrelevant_ids
    np.testing.assert_allclose(B.rel_mean, A.rel_mean, rtol=0, atol=1e-12)
    A.revoke(list(A.relevant_ids | A.irrelevant_ids))
    assert A.rel_mean is None and A.gp.m == 0        # nothing is left: as before the first update
    sd = A.state_dict()
    assert sd["ind"] == [] and ITAL(X, length_scale=0.6, device=dev).load_state_dict(sd).gp.m == 0


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
        L.revoke([77, got[0]])                       # both ranks make the same call
        picks = L.fetch_unlabelled(3)
        out[rank] = (got, picks, np.asarray(L.rel_mean).copy(), list(L.gp.ind), L.get_unseen())
    finally:
        _ranks.leave(group)


def test_two_ranks_revoke_like_one():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle.gp import OracleGP
    X = np.random.default_rng(41).random((151, 4))
    one = _ranks.spawn(_rank_session, 1, X, None)[0]
    two = _ranks.spawn(_rank_session, 2, X, "gloo")
    before = [5, 77, 140] + list(one[0])
    cond = _cond(OracleGP(X, 0.6).fit(before, np.ones(len(before))).K)
    for r in two:
        assert r[0] == one[0] and r[1] == one[1] and r[3] == one[3] and r[4] == one[4]
        _within(r[2], one[2], cond, "two ranks")
    np.testing.assert_array_equal(two[0][2], two[1][2])


# ------------------------------------------------------------------------------------------------------ context layer
def test_ctx_revoke_against_the_python_learner(dev):
    from ital_amd import ITAL, _lib, mvn_stream
    lib, chk = _lib.load(), _lib.check
    rng = np.random.default_rng(51)
    X = np.ascontiguousarray(rng.random((130, 5)))
    ls = 0.65
    first = {int(i): float(_truth(X, i)) for i in rng.choice(130, 4, replace=False)}
    mvn_stream.GLOBAL.reset()
    A = ITAL(X, length_scale=ls, device=dev)
    A.update(first)
    got = A.fetch_unlabelled(4)
    A.update({i: _truth(X, i) for i in got})
    cond = _cond_now(X, ls, A.gp)
    A.revoke([got[1], list(first)[0]])
    after = A.fetch_unlabelled(4)

    ctx = ctypes.c_void_p()
    chk(lib.ital_ctx_create(130, 5, ls, 1.0, 1e-6, 32, 0, 1, None, ctypes.byref(ctx)))
    try:
        chk(lib.ital_ctx_fit(ctx, X.ctypes.data, 0, None))
        i0 = np.asarray(list(first), dtype=np.int64)
        y0 = np.asarray(list(first.values()), dtype=np.float64)
        chk(lib.ital_ctx_update(ctx, i0.ctypes.data, y0.ctypes.data, len(i0), None))
        picks = np.zeros(8, dtype=np.int64)
        assert lib.ital_ctx_fetch(ctx, 4, picks.ctypes.data, None) == 4
        assert picks[:4].tolist() == got
        y1 = np.asarray([_truth(X, i) for i in got], dtype=np.float64)
        chk(lib.ital_ctx_update(ctx, picks.ctypes.data, y1.ctypes.data, 4, None))
        never = np.asarray([after[0]], dtype=np.int64)
        assert lib.ital_ctx_revoke(ctx, never.ctypes.data, 1, None) == -22          # no label
        assert b"ital_ctx_revoke" in lib.ital_last_error()
        twice = np.asarray([got[1], got[1]], dtype=np.int64)
        assert lib.ital_ctx_revoke(ctx, twice.ctypes.data, 2, None) == -22
        rev = np.asarray([got[1], list(first)[0]], dtype=np.int64)
        chk(lib.ital_ctx_revoke(ctx, rev.ctypes.data, 2, None))
        assert lib.ital_ctx_revoke(ctx, rev.ctypes.data, 1, None) == -22            # it has no label any more
        mean, var = np.empty(130), np.empty(130)
        chk(lib.ital_ctx_predict_stored(ctx, mean.ctypes.data, var.ctypes.data, None))
        O = _oracle(X, ls, A.gp)
        _within(mean, O.predict_stored(), cond, "ctx mean")
        _within(var, O.predict_stored(cov_mode="diag")[1], cond, "ctx variance")
        _within(mean, A.rel_mean, cond, "ctx vs python")
        assert lib.ital_ctx_fetch(ctx, 4, picks.ctypes.data, None) == 4
        assert picks[:4].tolist() == after                                            # the revoked samples are candidates again
        again = np.asarray([got[1]], dtype=np.int64)
        chk(lib.ital_ctx_update(ctx, again.ctypes.data, np.ones(1).ctypes.data, 1, None))   # and may be labelled anew
    finally:
        chk(lib.ital_ctx_destroy(ctx))
