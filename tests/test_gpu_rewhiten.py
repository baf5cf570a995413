"""Whitening a row range against the whole labelled set on the device (ital_whiten_rows, csrc/rewhiten.hip) and what is built
on it: GaussianProcess.extend / ActiveRetrievalBase.add_data and set_params.

The kernel is DEFINED as the composition of the existing entry points -- ital_row_norms, then one ital_whiten_append per block
of 16 labelled rows from row 0 up -- and is compared with that composition bit for bit (torch.equal).  add_data / set_params
are compared with a learner constructed on the final data / hyper-parameters and given the same feedback: 2e-9, the project's
bound for append against re-inversion (tests/test_gpu_mcmi.py, tests/test_gpu_parity.py), and with the oracle in the form of
tests/test_gpu_revoke.py: |device - oracle| <= max(1e-10, 1e-15 cond) * max(1, max|oracle|).  Run: python -m pytest tests -m gpu."""
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

APPEND_ATOL = 2e-9


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


def _cond(A):
    """The dpocon estimate, as tests/test_gpu_revoke.py computes it."""
    from scipy.linalg import lapack
    c, info = lapack.dpotrf(A, lower=1)
    assert info == 0
    rcond, _ = lapack.dpocon(c, np.abs(A).sum(axis=0).max(), uplo="L")
    return 1.0 / rcond


def _within(got, want, cond, what):
    bound = max(1e-10, 1e-15 * cond) * max(1.0, float(np.max(np.abs(want))))
    err = float(np.max(np.abs(np.asarray(got) - np.asarray(want))))
    print("%-22s err %.3g  bound %.3g  (cond %.3g)" % (what, err, bound, cond))
    assert err <= bound, (what, err, bound, cond)


def _close(got, want, what, atol=APPEND_ATOL):
    err = float(np.max(np.abs(np.asarray(got) - np.asarray(want))))
    print("%-22s err %.3g  bound %.3g" % (what, err, atol))
    assert err <= atol, (what, err)


# ------------------------------------------------------------------------------------------------ the kernel
OFFSET = 5            # the row range of the kernel tests starts at this row of the data matrix, not at row 0
GUARD = -7.0          # what the output buffers hold before a call: nothing outside the range may change


def _fitted_gp(dev, n, d, m, seed):
    """A GaussianProcess on n x d rows whose m labels came through a real sequence of update() calls of mixed sizes."""
    from ital_amd import GaussianProcess
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    gp = GaussianProcess(X, 0.7 * float(np.sqrt(d / 12.0)), var=1.3, noise=1e-5, device=dev, capacity=16)
    ind = [int(i) for i in rng.choice(n, m, replace=False)]
    y = rng.choice([-1.0, 1.0], size=m)
    sizes, at = [1, 16, 5, 16, 3, 16, 16, 7], 0
    while at < m:
        c = min(sizes[len(gp.appends) % len(sizes)], m - at)
        gp.update(ind[at:at + c], y[at:at + c])
        at += c
    assert gp.m == m and int(gp.status.item()) == 0
    return gp


class _Out(object):
    """Output buffers of one whitening of `rows` data rows: xnorm, V (capacity x ldv), mu, s2, pre-filled with GUARD."""

    def __init__(self, gp, rows, fill):
        dev = gp.device
        self.rows, self.ldv = rows, (rows + 15) // 16 * 16 + 16
        self.xnorm = torch.full((rows + 4,), GUARD, dtype=torch.float64, device=dev)
        self.mu = torch.full((rows + 4,), GUARD, dtype=torch.float64, device=dev)
        self.s2 = torch.full((rows + 4,), GUARD, dtype=torch.float64, device=dev)
        self.V = torch.full((gp.cap, self.ldv), fill, dtype=torch.float64, device=dev)

    def untouched_outside(self):
        r = self.rows
        return bool((self.xnorm[r:] == GUARD).all() and (self.mu[r:] == GUARD).all() and (self.s2[r:] == GUARD).all())


def _composed(gp, rows):
    """The definition: ital_row_norms, then ital_whiten_append per block of 16 labelled rows, from mu = 0, s2 = var."""
    from ital_amd import _lib
    from ital_amd.gp import _stream
    lib, st, o = _lib.lib(), _stream(), _Out(gp, rows, 0.0)
    X = gp.Xd.data_ptr() + 8 * OFFSET * gp.ldx
    o.mu[:rows] = 0.0
    o.s2[:rows] = float(gp.var)
    _lib.check(lib.ital_row_norms(X, rows, gp.ldx, o.xnorm.data_ptr(), st))
    for b0 in range(0, gp.m, 16):
        c = min(16, gp.m - b0)
        _lib.check(lib.ital_whiten_append(X, o.xnorm.data_ptr(), rows, gp.ldx, gp.XT.data_ptr() + 8 * b0 * gp.ldx,
                                          gp.XTn.data_ptr() + 8 * b0, c, gp.L.data_ptr() + 8 * b0 * gp.cap, gp.cap,
                                          gp.L.data_ptr() + 8 * (b0 * gp.cap + b0), gp.alpha.data_ptr() + 8 * b0,
                                          o.V.data_ptr(), o.ldv, b0, float(gp.var), float(gp.length_scale), o.mu.data_ptr(),
                                          o.s2.data_ptr(), st))
    return o


def _kernel(gp, rows, chunk=0):
    from ital_amd import _lib
    from ital_amd.gp import _stream
    o = _Out(gp, rows, GUARD)
    r = _lib.ItalRewhitenDesc()
    r.X, r.n_rows, r.ldx = gp.Xd.data_ptr() + 8 * OFFSET * gp.ldx, rows, gp.ldx
    r.XT, r.XTn, r.L, r.ldl, r.alpha, r.m = gp.XT.data_ptr(), gp.XTn.data_ptr(), gp.L.data_ptr(), gp.cap, gp.alpha.data_ptr(), gp.m
    r.var, r.length_scale = float(gp.var), float(gp.length_scale)
    r.xnorm, r.V, r.ldv, r.v_rows, r.mu, r.s2 = o.xnorm.data_ptr(), o.V.data_ptr(), o.ldv, gp.cap, o.mu.data_ptr(), o.s2.data_ptr()
    r.chunk = chunk
    _lib.check(_lib.lib().ital_whiten_rows(ctypes.byref(r), _stream()))
    return o


def _chunk():
    from ital_amd import _lib
    return int(_lib.lib().ital_whiten_rows_chunk())


def _kernel_cases():
    # (rows, d, m): ragged last tiles, ldx no multiple of 64, m across a block boundary and across the chunk boundary, m = 0
    cases = [(1, 3, 1), (17, 3, 0), (70, 21, 17), (257, 40, 65), (1000, 16, 130), (300, 256, 45)]
    cases += [(100, 5, "chunk-1"), (100, 5, "chunk"), (100, 5, "chunk+1")]
    return cases


@pytest.mark.parametrize("rows,d,m", _kernel_cases())
def test_kernel_equals_the_composed_sweeps_bit_for_bit(dev, rows, d, m):
    if isinstance(m, str):
        m = _chunk() + {"chunk-1": -1, "chunk": 0, "chunk+1": 1}[m]
    gp = _fitted_gp(dev, max(rows + OFFSET + 3, m + 1), d, m, seed=rows + 7 * d + m)
    want = _composed(gp, rows)
    got = _kernel(gp, rows)
    again = _kernel(gp, rows)
    for name in ("xnorm", "mu", "s2"):
        assert torch.equal(getattr(got, name)[:rows], getattr(want, name)[:rows]), name
        assert torch.equal(getattr(got, name), getattr(again, name)), name       # two launches: identical bits
    assert torch.equal(got.V[:, :rows], want.V[:, :rows])
    assert torch.equal(got.V, again.V)
    assert bool((got.V[gp.m:, :rows] == 0).all())                                # rows m .. capacity are zeroed
    assert bool((got.V[:, rows:] == GUARD).all()) and got.untouched_outside()    # nothing outside the range is written
    if m == 0:
        assert bool((got.mu[:rows] == 0).all()) and bool((got.s2[:rows] == float(gp.var)).all())
    else:
        assert bool(torch.isfinite(got.V[:, :rows]).all()) and float(got.V[: gp.m, :rows].abs().max()) > 0


@pytest.mark.parametrize("chunk", [32, 64, 128])
def test_every_chunk_size_gives_the_same_bits(dev, chunk):
    """The definition does not depend on the chunk: 130 labelled rows are 5, 3 and 2 launches."""
    gp = _fitted_gp(dev, 1008, 16, 130, seed=3)
    want = _composed(gp, 1000)
    got = _kernel(gp, 1000, chunk)
    for name in ("xnorm", "mu", "s2"):
        assert torch.equal(getattr(got, name)[:1000], getattr(want, name)[:1000]), name
    assert torch.equal(got.V[:, :1000], want.V[:, :1000])


# ------------------------------------------------------------------------------------------------ add_data, golden fixtures
@pytest.mark.parametrize("n0", [480, 333])
def test_add_data_before_the_first_fetch_gives_the_golden_rounds(dev, golden_dir, n0):
    """usps500: the learner is built on the first n0 rows (a multiple of 16, and not), the query is labelled, the other
    rows are added, then the fixture's rounds: picks bit-exact, MI and means within the bounds of tests/test_gpu_parity.py."""
    from ital_amd import ITAL, mvn_stream
    z = np.load(os.path.join(golden_dir, "usps500.npz"))
    X, q, rel = z["X"], int(z["query"]), z["rel"]
    assert q < n0 < len(X)
    mvn_stream.GLOBAL.reset()
    np.random.seed(0)
    L = ITAL(X[:n0], length_scale=float(z["length_scale"]), device=dev, **make_golden.FIXTURES["usps500"]["kw"])
    L.keep_scores = True
    L.update({q: 1})
    L.add_data(X[n0:])
    assert len(L.data) == len(X) == L.gp.n == L.gp.n_total and L.get_unseen() == [i for i in range(len(X)) if i != q]
    for r in range(int(z["rounds"])):
        m, v = L.gp.predict_stored(cov_mode="diag")
        np.testing.assert_allclose(m, z[f"r{r}_rel_mean"], rtol=0, atol=1e-10)
        np.testing.assert_allclose(v, z[f"r{r}_var"], rtol=0, atol=1e-9)
        ret = L.fetch_unlabelled(int(z["k"]))
        cand0 = z[f"r{r}_s0_cand"].tolist()
        pos = {c: i for i, c in enumerate(cand0)}
        for t in range(len(ret)):
            cand = z[f"r{r}_s{t}_cand"].tolist()
            mine = L.last_scores[t].cpu().numpy()[[pos[c] for c in cand]]
            np.testing.assert_allclose(mine, z[f"r{r}_s{t}_mi"], rtol=1e-8, atol=1e-10, err_msg=f"r{r} step {t}")
        assert ret == z[f"r{r}_ret"].tolist(), r
        L.update({int(i): float(rel[i]) for i in ret})
    np.testing.assert_allclose(L.rel_mean, z["final_rel_mean"], rtol=0, atol=1e-9)


def test_add_data_before_the_first_fetch_mcmi(dev, golden_dir):
    from ital_amd import MCMI_min
    z = np.load(os.path.join(golden_dir, "usps500_mcmi.npz"))
    X, q, rel, n0 = z["X"], int(z["query"]), z["rel"], 333
    assert q < n0
    np.random.seed(0)
    L = MCMI_min(X[:n0], length_scale=float(z["length_scale"]), device=dev, **make_golden.FIXTURES["usps500_mcmi"]["kw"])
    L.keep_scores = True
    L.update({q: 1})
    L.add_data(X[n0:])
    assert L.candidates == []
    for r in range(int(z["rounds"])):
        ret = L.fetch_unlabelled(int(z["k"]))
        cand0 = z[f"r{r}_s0_cand"].tolist()
        pos = {c: i for i, c in enumerate(cand0)}
        for t in range(len(ret)):
            cand = z[f"r{r}_s{t}_cand"].tolist()
            mine = L.last_scores[t].cpu().numpy()[[pos[c] for c in cand]]
            np.testing.assert_allclose(mine, z[f"r{r}_s{t}_mi"], rtol=1e-8, atol=0, err_msg=f"r{r} step {t}")
        assert ret == z[f"r{r}_ret"].tolist(), r
        L.update({int(i): float(rel[i]) for i in ret})
    np.testing.assert_allclose(L.rel_mean, z["final_rel_mean"], rtol=0, atol=1e-9)


# ------------------------------------------------------------------------------------------------ add_data in mid-session
def _truth(X, i):
    return 1 if X[i, 0] > 0.5 else -1


def _oracle(X, Q, ls, gp, **kw):
    """The reference's model of what `gp` holds: queries are extra rows behind the data (retrieval_base.py:40)."""
    from oracle.gp import OracleGP
    rows = np.vstack((X, Q)) if len(Q) else X
    return OracleGP(rows, ls, **kw).fit(list(gp.ind), np.asarray(gp.y))


def _session(cls, X, Q, ls, dev, k, **kw):
    """Two rounds of k on a fresh learner (after a first update without queries); returns it and the feedback history."""
    from ital_amd import mvn_stream
    mvn_stream.GLOBAL.reset()
    L = cls(X, queries=Q, length_scale=ls, device=dev, **kw)
    history = []
    if not len(Q):
        history.append({i: _truth(X, i) for i in (3, 11, 40, 77)})
        L.update(history[-1])
    for _ in range(2):
        got = L.fetch_unlabelled(k)
        history.append({i: _truth(X, i) for i in got})
        L.update(history[-1])
    return L, history


@pytest.mark.parametrize("case", ["plain", "two_queries", "after_revoke"])
def test_add_data_in_mid_session_equals_a_learner_built_on_all_rows(dev, case):
    from ital_amd import ITAL, mvn_stream
    rng = np.random.default_rng(17)
    X = rng.random((120, 6))
    ls = float(np.sqrt(6 / 12.0))
    Q = X[[100, 110]] + 0.01 if case == "two_queries" else []
    nq = len(Q)
    B, history = _session(ITAL, X[:90], Q, ls, dev, 4)
    cond = None
    if case == "after_revoke":
        cond = _cond(_oracle(X[:90], Q, ls, B.gp).K)
        victim = list(history[1])[1]
        B.revoke([victim])
        del history[1][victim]
    rounds, m = B.rounds, B.gp.m
    if nq:
        assert B.gp.ind[:2] == [90, 91]
    B.add_data(X[90:])
    assert B.rounds == rounds and B.gp.m == m and len(B.data) == 120 == B.gp.n == B.gp.n_total == B.gp.row1
    assert B.gp.X_host.shape == (120, 6) and B.gp.mu_all.shape[0] == 120 and B.state_dict()["n"] == 120
    if nq:
        assert B.gp.ind[:2] == [120, 121]            # queries are labelled rows numbered from n_total on: shifted
    A = ITAL(X, queries=Q, length_scale=ls, device=dev)
    for g in history:
        A.update(g)
    assert A.gp.ind == B.gp.ind and np.array_equal(A.gp.y, B.gp.y)
    ma, va = A.gp.predict_stored(cov_mode="diag")
    mb, vb = B.gp.predict_stored(cov_mode="diag")
    O = _oracle(X, Q, ls, B.gp)
    mo, vo = O.predict_stored(cov_mode="diag")
    mo, vo = mo[:120], vo[:120]
    if cond is None:
        _close(B.rel_mean, A.rel_mean, "rel_mean B vs A")
        _close(vb, va, "variance B vs A")
        for name, (mm, vv) in dict(A=(ma, va), B=(mb, vb)).items():
            _close(mm, mo, "mean %s vs oracle" % name)
            _close(vv, vo, "variance %s vs oracle" % name)
    else:                                            # a factor that a row deletion left: the bound of tests/test_gpu_revoke.py
        _within(B.rel_mean, A.rel_mean, cond, "rel_mean B vs A")
        _within(vb, va, cond, "variance B vs A")
        for name, (mm, vv) in dict(A=(ma, va), B=(mb, vb)).items():
            _within(mm, mo, cond, "mean %s vs oracle" % name)
            _within(vv, vo, cond, "variance %s vs oracle" % name)
    seen = set().union(*history)
    assert B.get_unseen() == A.get_unseen() == [i for i in range(120) if i not in seen]
    assert sorted(B.top_results().tolist()) == list(range(120))
    assert B.top_results(5).tolist() == A.top_results(5).tolist()
    mvn_stream.GLOBAL.reset()
    pa = A.fetch_unlabelled(4)
    mvn_stream.GLOBAL.reset()
    pb = B.fetch_unlabelled(4)
    assert pa == pb and len(set(pb)) == 4 and not set(pb) & seen
    B.update({i: _truth(X, i) for i in pb})          # and the retrieval loop goes on, over all 120 rows
    nxt = B.fetch_unlabelled(4)
    assert len(set(nxt)) == 4 and not set(nxt) & (seen | set(pb)) and B.rounds == rounds + 1


@pytest.mark.parametrize("name", ["MCMI_min", "AdaptAL", "BorderlineSampling"])
def test_other_learners_after_add_data(dev, name):
    import ital_amd
    from ital_amd import baselines
    cls = getattr(ital_amd, name, None) or getattr(baselines, name)
    kw = dict(subsample=60) if name in ("MCMI_min", "AdaptAL") else {}
    X = np.random.default_rng(23).random((150, 4))
    np.random.seed(3)
    B, history = _session(cls, X[:101], [], 0.6, dev, 3, **kw)
    B.add_data(X[101:])
    A = cls(X, length_scale=0.6, device=dev, **kw)
    for g in history:
        A.update(g)
    assert A.gp.ind == B.gp.ind and A.get_unseen() == B.get_unseen() and 149 in B.get_unseen()
    _close(B.rel_mean, A.rel_mean, "rel_mean B vs A")
    np.random.seed(4)
    pa = A.fetch_unlabelled(3)
    np.random.seed(4)
    pb = B.fetch_unlabelled(3)
    assert pa == pb and len(pb) == 3


# ------------------------------------------------------------------------------------------------ set_params
def test_set_params_equals_a_fresh_learner_with_those_values(dev):
    from ital_amd import ITAL, mvn_stream
    X = np.random.default_rng(29).random((120, 6))
    ls = float(np.sqrt(6 / 12.0))
    new = dict(length_scale=1.3 * ls, var=1.4, noise=1e-4)
    A, history = _session(ITAL, X, [], ls, dev, 4)
    mean0, var0 = [np.array(t) for t in A.gp.predict_stored(cov_mode="diag")]
    rounds = A.rounds
    assert A.set_params(**new) is A
    assert (A.length_scale, A.var, A.noise) == (new["length_scale"], 1.4, 1e-4) == (A.gp.length_scale, A.gp.var, A.gp.noise)
    assert A.rounds == rounds and int(A.gp.status.item()) == 0
    B = ITAL(X, device=dev, **new)
    for g in history:
        B.update(g)
    ma, va = A.gp.predict_stored(cov_mode="diag")
    mb, vb = B.gp.predict_stored(cov_mode="diag")
    _close(A.rel_mean, B.rel_mean, "rel_mean vs fresh")
    _close(va, vb, "variance vs fresh")
    O = _oracle(X, [], new["length_scale"], A.gp, var=1.4, noise=1e-4)
    cond = _cond(O.K)
    mo, vo = O.predict_stored(cov_mode="diag")
    _within(ma, mo, cond, "mean vs oracle")
    _within(va, vo, cond, "variance vs oracle")
    mvn_stream.GLOBAL.reset()
    pa = A.fetch_unlabelled(4)
    mvn_stream.GLOBAL.reset()
    pb = B.fetch_unlabelled(4)
    assert pa == pb and len(set(pa)) == 4
    A.set_params(length_scale=ls, var=1.0, noise=1e-6)       # and back
    m1, v1 = A.gp.predict_stored(cov_mode="diag")
    _close(m1, mean0, "means after the old values")
    _close(v1, var0, "variances after the old values")
    A.set_params(var=1.4)                                    # None: as it is
    assert (A.length_scale, A.var, A.noise) == (ls, 1.4, 1e-6)


def test_set_params_refuses_an_indefinite_gram_and_changes_nothing(dev):
    from ital_amd import ITAL
    X = np.random.default_rng(31).random((120, 6))
    ls = float(np.sqrt(6 / 12.0))
    A, _ = _session(ITAL, X, [], ls, dev, 4)
    mean, L, alpha, V = np.array(A.rel_mean), A.gp.L.clone(), A.gp.alpha.clone(), A.gp.V.clone()
    mu, s2 = A.gp.mu.clone(), A.gp.s2.clone()
    with pytest.raises(np.linalg.LinAlgError):
        A.set_params(noise=-2.0)                             # K - 2 I has a negative diagonal
    assert (A.length_scale, A.var, A.noise) == (ls, 1.0, 1e-6) == (A.gp.length_scale, A.gp.var, A.gp.noise)
    assert np.array_equal(A.rel_mean, mean) and torch.equal(A.gp.L, L) and torch.equal(A.gp.alpha, alpha)
    assert torch.equal(A.gp.V, V) and torch.equal(A.gp.mu, mu) and torch.equal(A.gp.s2, s2)
    assert int(A.gp.status.item()) == 0
    assert len(A.fetch_unlabelled(4)) == 4                   # the session goes on


def test_set_params_and_add_data_before_any_label(dev):
    from ital_amd import ITAL
    X = np.random.default_rng(37).random((60, 5))
    A = ITAL(X[:40], length_scale=0.6, device=dev)
    A.set_params(var=2.0, length_scale=0.7)
    assert (A.length_scale, A.var, A.noise) == (0.7, 2.0, 1e-6) and A.rel_mean is None and A.gp.m == 0
    assert bool((A.gp.s2 == 2.0).all()) and bool((A.gp.mu == 0).all())
    A.add_data(X[40:])
    assert bool((A.gp.s2 == 2.0).all()) and bool((A.gp.mu == 0).all()) and A.gp.s2.shape[0] == 60 and bool((A.gp.V == 0).all())
    B = ITAL(X, length_scale=0.7, var=2.0, device=dev)
    for L in (A, B):
        L.update({5: 1, 50: -1})
    assert np.array_equal(A.rel_mean, B.rel_mean)            # the same appends on the same state


# ------------------------------------------------------------------------------------------------ errors
def test_add_data_errors_and_no_op(dev):
    from ital_amd import ITAL
    X = np.random.default_rng(41).random((50, 4))
    A = ITAL(X, length_scale=0.6, device=dev)
    A.update({3: 1, 9: -1})
    mean, ptr = np.array(A.rel_mean), A.gp.V.data_ptr()
    with pytest.raises(ValueError):
        A.add_data(np.zeros((3, 5)))
    with pytest.raises(ValueError):
        A.gp.extend(np.zeros((3, 5)))
    assert A.add_data(np.zeros((0, 4))) is A and A.gp.extend([]) is A.gp
    assert len(A.data) == 50 == A.gp.n and A.gp.V.data_ptr() == ptr and np.array_equal(A.rel_mean, mean)


def _rank_session(rank, world, port, X, mode, out):
    dev, group = _ranks.join(rank, world, port, mode)
    try:
        from ital_amd import ITAL, mvn_stream
        mvn_stream.GLOBAL.reset()
        L = ITAL(X, length_scale=0.6, device=dev, rank=rank, world=world, group=group)
        L.update({5: 1, 77: -1, 140: 1})
        got = L.fetch_unlabelled(3)
        L.update({i: _truth(X, i) for i in got})
        refused = None
        if world > 1:
            try:
                L.add_data(X[:4])
            except NotImplementedError as e:
                refused = str(e)
            try:
                L.gp.extend(X[:4])
            except NotImplementedError as e:
                refused = refused and str(e)
        L.set_params(length_scale=0.75, var=1.2, noise=1e-5)     # every rank makes the same call
        picks = L.fetch_unlabelled(3)
        out[rank] = (got, picks, np.asarray(L.rel_mean).copy(), refused, len(L.data))
    finally:
        _ranks.leave(group)


def test_two_ranks_set_params_like_one_and_refuse_add_data():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    X = np.random.default_rng(43).random((151, 4))
    one = _ranks.spawn(_rank_session, 1, X, None)[0]
    two = _ranks.spawn(_rank_session, 2, X, "gloo")
    for r in two:
        assert r[0] == one[0] and r[1] == one[1] and r[4] == 151
        assert r[3] and "row sharding cannot grow" in r[3]
        _close(r[2], one[2], "two ranks vs one")
    np.testing.assert_array_equal(two[0][2], two[1][2])
