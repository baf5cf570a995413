"""AdaptAL on the device (ital_amd/adapt_al.py, csrc/adapt.hip) against numpy / scipy restatements of its kernels and
against the reference's ital/adapt_al.py (goldens of tests/golden/make_golden_adapt.py).  Run: python -m pytest tests -m gpu."""
import io
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
import _ranks  # noqa: E402

FIXTURES = ["adapt_usps600_q3", "adapt_usps600_q17", "adapt_usps2007_sub500", "adapt_synth300_k6", "adapt_synth300_betas",
            "adapt_synth300_b1"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


def _lib():
    from ital_amd import _lib
    return _lib.lib(), _lib.check


def _st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------ kernel level
def _spd(n, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, n))
    return B @ B.T / n + np.eye(n)


def _cond(A):
    from scipy.linalg import lapack
    c, info = lapack.dpotrf(A, lower=1)
    assert info == 0
    rcond, _ = lapack.dpocon(c, np.abs(A).sum(axis=0).max(), uplo="L")
    return 1.0 / rcond


def _factor_and_inv_diag(A, pad=3):
    """Cholesky on the device (ital_chol_batched), then ital_chol_inv_diag on that factor; (factor, out, info)."""
    lib, check = _lib()
    n = A.shape[0]
    ld = n + pad
    B = np.full((n, ld), 7.25)
    B[:, :n] = A
    buf = torch.from_numpy(B).cuda()
    P = lambda v, dt: torch.tensor(v, dtype=dt, device="cuda")  # noqa: E731
    ptrs, ns, lds = P([buf.data_ptr()], torch.int64), P([n], torch.int32), P([ld], torch.int64)
    info = torch.zeros(2, dtype=torch.int32, device="cuda")
    check(lib.ital_chol_batched(ptrs.data_ptr(), ns.data_ptr(), lds.data_ptr(), 1, n, info.data_ptr(), info.data_ptr() + 4,
                                _st()))
    wl = int(lib.ital_chol_inv_diag_workspace(n))
    work = torch.full((wl,), float("nan"), dtype=torch.float64, device="cuda")     # nothing unwritten may be read
    out = torch.full((n + 1,), -3.0, dtype=torch.float64, device="cuda")
    check(lib.ital_chol_inv_diag(buf.data_ptr(), n, ld, out.data_ptr(), work.data_ptr(), wl, info.data_ptr(), _st()))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert o[n] == -3.0
    return np.tril(buf.cpu().numpy()[:, :n]), o[:n], info.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000, 3001])
def test_chol_inv_diag_matches_dtrtri(dev, n):
    from scipy.linalg import lapack
    A = _spd(n, 11 * n + 1)
    L, got, info = _factor_and_inv_diag(A)
    assert info[0] == 0
    li, rc = lapack.dtrtri(L, lower=1)
    assert rc == 0
    want = (np.tril(li) ** 2).sum(axis=0)
    dev_rel = np.max(np.abs(got - want) / want)
    print("inv_diag n=%d: max relative deviation %.3g (bar %.3g)" % (n, dev_rel, 1e-14 * _cond(A)))
    assert dev_rel <= 1e-14 * _cond(A)


def test_chol_inv_diag_reports_a_failed_factorisation(dev):
    A = _spd(200, 5)
    A[150, 150] = -1.0
    _, got, info = _factor_and_inv_diag(A)
    assert info[0] == 151
    assert np.all(np.isnan(got))


def _clip_p(mean, var):
    from scipy.stats import norm
    with np.errstate(all="ignore"):
        return np.maximum(1e-8, np.minimum(1.0 - 1e-8, norm.cdf(0, mean, np.sqrt(var))))


def _scores_np(mu, s2, inv, kdiag):
    p = _clip_p(mu, np.maximum(0, s2))
    with np.errstate(all="ignore"):
        ent = -1 * (p * np.log(p) + (1.0 - p) * np.log(1.0 - p))
    return ent, np.log(kdiag / np.maximum(1e-6, 1.0 / inv)) / 2


def _scores_dev(mu, s2, inv, kdiag):
    lib, check = _lib()
    n = len(mu)
    t = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (mu, s2, inv)]
    out = torch.empty((2, n), dtype=torch.float64, device="cuda")
    check(lib.ital_adapt_scores(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n, kdiag, out[0].data_ptr(),
                                out[1].data_ptr(), _st()))
    o = out.cpu().numpy()
    return o[0], o[1]


def test_adapt_scores_formula(dev):
    rng = np.random.default_rng(3)
    n = 1000
    s2 = rng.uniform(0.05, 1.0, n)
    mu = rng.uniform(-1.5, 1.5, n) * np.sqrt(s2)
    inv = 1.0 / rng.uniform(1e-3, 1.0, n)
    mu[0], s2[0] = 0.3, -1e-12                  # a variance clamped to 0: NaN, as scipy's scale check
    inv[1] = 1e9                                # sigma = 1e-9 under the 1e-6 floor
    mu[2], s2[2] = 10.0, 1.0                    # probability at the lower clip
    mu[3], s2[3] = -10.0, 1.0                   # ... and at the upper clip
    kdiag = 1.3 + 1e-4
    ent, den = _scores_dev(mu, s2, inv, kdiag)
    want_e, want_d = _scores_np(mu, s2, inv, kdiag)
    assert np.isnan(ent[0]) and np.isnan(want_e[0])
    assert den[1] == pytest.approx(np.log(kdiag / 1e-6) / 2, rel=1e-14)
    p_lo = 1e-8
    h_clip = -(p_lo * np.log(p_lo) + (1 - p_lo) * np.log(1 - p_lo))
    assert ent[2] == pytest.approx(h_clip, rel=1e-12) and ent[3] == pytest.approx(h_clip, rel=1e-12)
    np.testing.assert_allclose(ent[1:], want_e[1:], rtol=1e-12, atol=0)
    np.testing.assert_allclose(den, want_d, rtol=1e-12, atol=0)
    e1, d1 = _scores_dev(mu[5:6], s2[5:6], inv[5:6], kdiag)          # one candidate only
    np.testing.assert_allclose([e1[0], d1[0]], [want_e[5], want_d[5]], rtol=1e-12)


def _error_np(C, rows, mu, s2, noise, y_false=0.0):
    nc = len(mu)
    out = []
    for a, i in enumerate(rows):
        p_i = _clip_p(mu[i], max(s2[i], 0))
        others = np.setdiff1d(np.arange(nc), [i])
        g = 1.0 / (s2[i] + noise)
        err = 0
        for fb in (True, False):
            y = 1.0 if fb else y_false
            m = mu[others] + C[a, others] * g * (y - mu[i])
            v = np.maximum(0, s2[others] - C[a, others] ** 2 * g)
            p = _clip_p(m, v)
            err += (1 - p_i if fb else p_i) * np.sum(np.where(mu[others] > 0, p, 1. - p))
        out.append(err)
    return np.array(out, dtype=np.float64)


def _error_dev(C, rows, mu, s2, noise, ldc):
    lib, check = _lib()
    r, nc = C.shape
    Cp = np.full((r, ldc), 1e30)
    Cp[:, :nc] = C
    t = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (Cp, mu, s2)]
    rows_d = torch.tensor(rows, dtype=torch.int32, device="cuda")
    out = torch.empty(3 * r, dtype=torch.float64, device="cuda")
    check(lib.ital_adapt_error(t[0].data_ptr(), ldc, rows_d.data_ptr(), r, nc, t[1].data_ptr(), t[2].data_ptr(), noise,
                               out.data_ptr() + 8 * r, out.data_ptr(), _st()))
    return out[:r].cpu().numpy()


def test_adapt_error_formula(dev):
    rng = np.random.default_rng(4)
    nc, noise = 777, 1e-4
    s2 = rng.uniform(0.2, 1.0, nc)
    mu = rng.uniform(-1.0, 1.0, nc) * np.sqrt(s2)
    rows = [0, 5, 300, 776, 41]
    C = rng.uniform(-0.3, 0.3, (len(rows), nc)) * np.sqrt(s2)[None, :]
    mu[7], s2[7] = 9.0, 0.5                      # updated probabilities at the clips
    mu[8], s2[8] = -9.0, 0.5
    mu[41], s2[41] = 6.5, 1.0                    # p_i of a short-listed row at the lower clip
    got = _error_dev(C, rows, mu, s2, noise, nc + 7)
    want = _error_np(C, rows, mu, s2, noise)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    # the target of fb = False is 0.0 (float(False)), not -1: the restatement with -1 is far away (rows whose own
    # probability is not clipped: at the clip the False term weighs 1e-8)
    wrong = _error_np(C, rows, mu, s2, noise, y_false=-1.0)
    assert np.min(np.abs(wrong - want)[:4] / want[:4]) > 1e-6
    # a simulated variance clamped to 0 is NaN in both (scipy's scale check inside norm.cdf)
    C2 = C.copy()
    C2[1, 9] = 10.0
    got2, want2 = _error_dev(C2, rows, mu, s2, noise, nc), _error_np(C2, rows, mu, s2, noise)
    assert np.isnan(got2[1]) and np.isnan(want2[1])
    np.testing.assert_allclose(np.delete(got2, 1), np.delete(want2, 1), rtol=1e-12, atol=0)
    # one candidate only: nothing else to misclassify
    one = _error_dev(np.array([[0.4]]), [0], np.array([0.2]), np.array([0.4]), noise, 1)
    assert one.tolist() == [0.0]


# ----------------------------------------------------------------------------------------------------- session level
def _load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    X = z["X"] if "X" in z.files else np.load(os.path.join(GOLD, str(z["source"])))["X"][:int(z["rows"])]
    return z, X


def _learner(z, X, **placement):
    from ital_amd import AdaptAL
    L = AdaptAL(X, length_scale=float(z["length_scale"]), var=float(z["var"]), noise=float(z["noise"]),
                subsample=int(z["subsample"]) or None, betas=z["betas"].tolist(), **placement)
    L.update({int(z["query"]): 1})
    return L


@pytest.mark.parametrize("name", FIXTURES)
def test_session_reproduces_reference(dev, name):
    z, X = _load(name)
    rel = z["rel"]
    np.random.seed(int(z["seed"]))
    L = _learner(z, X, device=dev)
    worst = dict(entropy=0.0, density=0.0, err=0.0)
    for r in range(int(z["rounds"])):
        p = "r%d_" % r
        unseen = np.asarray(L.get_unseen())
        before = np.random.get_state()
        ret = L.fetch_unlabelled(int(z["k"]))
        after = np.random.get_state()
        last = L.last
        assert np.array_equal(last["candidates"], z[p + "cand"])
        if int(z["subsample"]):
            # the global generator stands where the reference's single choice() call leaves it
            np.random.set_state(before)
            assert np.array_equal(np.random.choice(unseen, int(z["subsample"]), replace=False), z[p + "cand"])
            mine = np.random.get_state()
            assert mine[0] == after[0] and np.array_equal(mine[1], after[1]) and mine[2:] == after[2:]
            np.random.set_state(after)
        d_ent = np.max(np.abs(last["entropy"] - z[p + "entropy"]))
        d_den = np.max(np.abs(last["density"] - z[p + "density"]))
        tol_den = max(1e-14 * float(z[p + "cond"]), 10 * float(z[p + "den_ref_vs_lapack"]))
        worst["entropy"], worst["density"] = max(worst["entropy"], d_ent), max(worst["density"], d_den)
        print("%s round %d: |entropy| %.3g (bar 4e-9), |density| %.3g (bar %.3g)" % (name, r, d_ent, d_den, tol_den))
        assert d_ent <= 4e-9
        assert d_den <= tol_den
        assert np.array_equal(last["max_ind"], z[p + "max_ind"])
        want_err = z[p + "err"]
        if len(want_err):
            d_err = np.max(np.abs(last["err"] - want_err) / np.maximum(np.abs(want_err), 1))
            worst["err"] = max(worst["err"], d_err)
            print("%s round %d: |err| %.3g (bar 1e-8)" % (name, r, d_err))
            assert d_err <= 1e-8
        else:
            assert last["err"] is None
        assert ret == z[p + "ret"].tolist()
        assert all(type(i) is int for i in ret)
        L.update({int(i): (1 if rel[i] > 0 else -1) for i in ret})
    print("%s worst: entropy %.3g density %.3g err %.3g" % (name, worst["entropy"], worst["density"], worst["err"]))


def test_limits_and_empty_requests(dev):
    from ital_amd import AdaptAL
    rng = np.random.default_rng(9)
    X = rng.random((20, 4))
    L = AdaptAL(X, length_scale=0.5, device=dev)
    with pytest.raises(RuntimeError, match="fitted relevance model"):
        L.fetch_unlabelled(2)
    L.update({0: 1, 1: -1, 2: 1})
    assert L.fetch_unlabelled(0) == []
    assert L.fetch_unlabelled(-1) == []
    got = L.fetch_unlabelled(50)                 # k larger than the candidate count: every unseen sample
    assert sorted(got) == list(range(3, 20))
    L.max_gram_bytes = 1000
    with pytest.raises(MemoryError, match="subsample"):
        L.fetch_unlabelled(2)
    L.update({i: -1 for i in range(3, 20)})      # no candidates left
    assert L.fetch_unlabelled(3) == []


def test_harness_builds_and_runs_the_learner(dev):
    from ital_amd import AdaptAL, harness
    config, dataset, learner = harness.load_config(os.path.join(GOLD, "conf", "harness_adapt.conf"))
    assert isinstance(learner, AdaptAL) and learner.subsample == 40
    trace, buf = [], io.StringIO()
    harness.run_retrieval_experiment(config, dataset, learner, out=buf, trace=trace)
    assert len(trace) == 3                       # three classes, one repetition, one round
    for _, query, _, ret, _ in trace:
        assert len(ret) == 3 and len(set(ret)) == 3 and not set(ret) & set(query)
    assert buf.getvalue().splitlines()[0].startswith("Round;Median_AP")


def _rank_worker(rank, world, port, name, mode, out):
    dev, group = _ranks.join(rank, world, port, mode)
    try:
        z, X = _load(name)
        rel = z["rel"]
        np.random.seed(int(z["seed"]))
        L = _learner(z, X, device=dev, rank=rank, world=world, group=group)
        assert L.gp.collective
        picks = []
        for r in range(int(z["rounds"])):
            ret = L.fetch_unlabelled(int(z["k"]))
            picks.append(ret)
            L.update({int(i): (1 if rel[i] > 0 else -1) for i in ret})
        out[rank] = picks
    finally:
        _ranks.leave(group)


def test_two_ranks_return_the_one_rank_list(dev):
    name = "adapt_usps2007_sub500"
    z, _ = _load(name)
    want = [z["r%d_ret" % r].tolist() for r in range(int(z["rounds"]))]     # == the one-rank lists (test above)
    res = _ranks.spawn(_rank_worker, 2, name, "gloo")
    assert res[0] == want and res[1] == want


def test_full_size_9298x256_without_subsample(dev):
    """No golden (the reference takes too long here): runs, returns 4 distinct unseen ids, and the density equals the
    scipy dpotrf + dtrtri value on the downloaded Gram to 1e-14 cond."""
    from scipy.linalg import lapack
    from ital_amd import AdaptAL
    lib, check = _lib()
    rng = np.random.default_rng(21)
    n, d = 9298, 256
    X = rng.random((n, d))
    ls = float(np.sqrt(d / 12.0))
    L = AdaptAL(X, length_scale=ls, device=dev)
    labels = {int(i): (1 if j % 2 == 0 else -1) for j, i in enumerate(rng.choice(n, 6, replace=False))}
    L.update(labels)
    ret = L.fetch_unlabelled(4)
    assert len(ret) == 4 and len(set(ret)) == 4 and not set(ret) & set(labels)
    assert all(0 <= i < n for i in ret)
    nc = n - len(labels)
    assert len(L.last["density"]) == nc
    # the same Gram once more (the factorisation overwrote it), downloaded
    _, Xc, _, vec = L._block_bufs
    _, K, idx, work, v3, idx_p, n_p, K_p, ld_p, info = L._gram_bufs
    check(lib.ital_gram_rows(Xc.data_ptr(), vec[0].data_ptr(), L.gp.ldx, idx_p.data_ptr(), n_p.data_ptr(), K_p.data_ptr(),
                             ld_p.data_ptr(), 1, nc, 1.0, ls, 1e-6, _st()))
    A = np.tril(K.cpu().numpy()[:, :nc])
    A = A + np.tril(A, -1).T
    c, rc = lapack.dpotrf(A, lower=1)
    assert rc == 0
    rcond, _ = lapack.dpocon(c, np.abs(A).sum(axis=0).max(), uplo="L")
    li, rc = lapack.dtrtri(c, lower=1)
    assert rc == 0
    want = np.log(np.diag(A) / np.maximum(1e-6, 1 / (np.tril(li) ** 2).sum(axis=0))) / 2
    dev_abs = np.max(np.abs(L.last["density"] - want))
    print("full size: cond %.3g, |density - lapack| %.3g (bar %.3g)" % (1 / rcond, dev_abs, 1e-14 / rcond))
    assert dev_abs <= 1e-14 / rcond
