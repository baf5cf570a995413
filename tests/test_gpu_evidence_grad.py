"""The log marginal likelihood's gradient in the log-parameters on the device (include/ital_evidence_grad.h,
csrc/evidence_grad.hip) and what is built on it: GaussianProcess.evidence_grad, tune.fit_session_params and
ActiveRetrievalBase.fit_params.

Inputs are those of tests/test_gpu_evidence.py (tests/_evidence_inputs.py holds them for both).  The references are computed
here with numpy / scipy in float64 (tests/_evidence_grad_ref.py), D from the same expansion |x_i|^2 + |x_j|^2 - 2 x_i.x_j.
No bound comes from a measurement on the device:

- D within rtol 1e-12 of the host's where |D| > 1e-9, else atol 1e-12 (the project's bar for RBF values);
- W = K^-1 within 100 * cond(K) * 2^-52 of max(1, |inv|) of numpy.linalg.inv, cond < 1e5 (the bar of test_gpu_evidence.py);
- every gradient component within 100 * cond(K) * 2^-52 * max(1, S_theta) of the host's, S_theta = 1/2 sum_ij
  |(alpha alpha^T - W)_ij dK_ij| being the forward-error scale of the sum.  Two float64 routes on the host (explicit inverse;
  Cholesky plus the closed forms) stay below 0.012 of that bound against a long-double reference on these cases;
- against the central difference of the device's own lml (ital_gp_evidence) at h = 1e-4 in each log-parameter: 1e-6 *
  max(1, |g|); the host model of that comparison gives 4.3e-8, nearly all of it truncation ~ h^2.

Every comparison prints its figure before it asserts (run with -s to see them).  Run: python -m pytest tests -m gpu."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _evidence_grad_ref as ref  # noqa: E402
from _evidence_inputs import CANDS, GUARD, _case, _evidence, _labels, _lib, _params, _stream, _upload  # noqa: E402

EPS = 2.0 ** -52
WORST = {"grad": 0.0, "W": 0.0, "fd": 0.0}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


def _evidence_lml(X, y, cands, dev, pad=0):
    """ital_gp_evidence, the entry point this one extends, on G candidates: the device tensor of its lml."""
    return _evidence(X, y, cands, dev, pad=pad)["scores"][:, 0].clone()


def _grad(X, y, cands, dev, pad=0):
    """ital_gp_evidence_grad on G candidates; leading dimension m + pad; one guard element behind every output."""
    L, lib = _lib()
    XT, XTn, ldx = _upload(X, dev)
    m, G = len(X), len(cands)
    ld = m + pad
    yd = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).to(dev)
    prm = _params(cands, dev)
    K = torch.full((G, m, ld), GUARD, dtype=torch.float64, device=dev)
    need = int(lib.ital_gp_evidence_grad_workspace(m, G))
    work = torch.full((need + 1,), GUARD, dtype=torch.float64, device=dev)
    values = torch.full((G + 1,), GUARD, dtype=torch.float64, device=dev)
    grad = torch.full((G + 1, 3), GUARD, dtype=torch.float64, device=dev)
    info = torch.full((G + 1,), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    d = L.ItalEvidenceGradDesc()
    d.XT, d.XTn, d.ldx, d.y, d.m, d.params, d.G = XT.data_ptr(), XTn.data_ptr(), ldx, yd.data_ptr(), m, prm.data_ptr(), G
    d.K, d.ld, d.values, d.grad, d.info = K.data_ptr(), ld, values.data_ptr(), grad.data_ptr(), info.data_ptr()
    d.status, d.work, d.work_doubles, d.ev = status.data_ptr(), work.data_ptr(), need, None
    before = int(lib.ital_launch_count())
    L.check(lib.ital_gp_evidence_grad(ctypes.byref(d), _stream()))
    launches = int(lib.ital_launch_count()) - before
    torch.cuda.synchronize()
    assert float(values[G]) == GUARD and bool((grad[G] == GUARD).all()) and int(info[G]) == -1 and int(status[1]) == 0
    assert float(work[need]) == GUARD
    assert bool((K[:, :, m:] == GUARD).all())                           # nothing beyond column m of the Grams
    up = torch.triu(torch.ones((m, m), dtype=torch.bool, device=dev), 1)
    assert bool((K[:, :, :m][:, up] == GUARD).all())                    # nothing above their diagonals
    return dict(values=values[:G], grad=grad[:G], info=info[:G], status=int(status[0].item()), K=K, work=work, launches=launches)


SHAPES = [(m, d, G) for m in (1, 2, 17, 63, 64, 65, 127, 128, 129, 200, 257) for d in (3, 40) for G in (1, 3)]


@functools.lru_cache(maxsize=None)
def _ref(m, d, g):
    """The host's values for candidate g of the shape's inputs: computed once, shared by the tests, never written to."""
    X, y, _ = _case(m, d, 1)
    h = ref.host_grad(ref.sqdist(X), y, *CANDS[d][g])
    assert h is not None and h["cond"] < 1e5, (m, d, g)
    return h


# ------------------------------------------------------------------------------------------------ D and W
@pytest.mark.parametrize("m,d", sorted(set((m, d) for m, d, _ in SHAPES)))
def test_squared_distances_equal_the_hosts_expansion(dev, m, d):
    L, lib = _lib()
    X, _, _ = _case(m, d, 1)
    XT, XTn, ldx = _upload(X, dev)
    low = np.tril(np.ones((m, m), dtype=bool))
    want = ref.sqdist(X)
    for ld in (m, m + 3):
        D = torch.full((m, ld), GUARD, dtype=torch.float64, device=dev)
        L.check(lib.ital_sqdist_lower(XT.data_ptr(), XTn.data_ptr(), m, ldx, D.data_ptr(), ld, _stream()))
        got = D.cpu().numpy()
        big = low & (np.abs(want) > 1e-9)
        small = low & ~big
        rel = float(np.max(np.abs(got[:, :m][big] - want[big]) / np.abs(want[big]))) if big.any() else 0.0
        ab = float(np.max(np.abs(got[:, :m][small] - want[small]))) if small.any() else 0.0
        print("GRAD D m %d d %d ld %d: rel %.3g (bound 1e-12)  abs near 0 %.3g (bound 1e-12)" % (m, d, ld, rel, ab))
        assert rel <= 1e-12 and ab <= 1e-12
        assert np.all(got[:, :m][~low] == GUARD) and np.all(got[:, m:] == GUARD)      # the lower triangle and nothing else


@pytest.mark.parametrize("m,d,G", SHAPES)
def test_the_inverse_from_the_inverse_factors(dev, m, d, G):
    """ital_chol_inv_diag_batched leaves M = L^-1 in its workspace; W = M^T M.  The workspace starts as NaN and the upper
    triangle of M stays so: a read above the diagonal would show in W."""
    L, lib = _lib()
    refs = [_ref(m, d, g) for g in range(G)]
    X, _, cands = _case(m, d, G)
    Dh = ref.sqdist(X)
    mats = []
    for g, (ls, var, noise) in enumerate(cands):
        Lh = np.linalg.cholesky(var * np.exp(Dh / (-2.0 * ls * ls)) + noise * np.eye(m))
        A = torch.full((m, m), float("nan"), dtype=torch.float64, device=dev)
        A[:, :] = torch.from_numpy(np.tril(Lh) + np.triu(np.full((m, m), np.nan), 1)).to(dev)
        mats.append(A)
    ptrs = torch.tensor([A.data_ptr() for A in mats], dtype=torch.int64, device=dev)
    ldd = torch.full((G,), m, dtype=torch.int64, device=dev)
    cdiag = torch.empty((G, m), dtype=torch.float64, device=dev)
    need = int(lib.ital_chol_inv_diag_batched_workspace(m, G))
    work = torch.full((need,), float("nan"), dtype=torch.float64, device=dev)
    L.check(lib.ital_chol_inv_diag_batched(ptrs.data_ptr(), ldd.data_ptr(), m, G, None, cdiag.data_ptr(), m, work.data_ptr(),
                                           need, _stream()))
    low = np.tril(np.ones((m, m), dtype=bool))
    for ldw in (m, m + 3):
        W = torch.full((G, m, ldw), GUARD, dtype=torch.float64, device=dev)
        L.check(lib.ital_chol_gram_inverse_batched(work.data_ptr(), m, G, None, W.data_ptr(), ldw, _stream()))
        Wh = W.cpu().numpy()
        for g in range(G):
            ls, var, noise = cands[g]
            inv = np.linalg.inv(var * np.exp(Dh / (-2.0 * ls * ls)) + noise * np.eye(m))
            got = Wh[g, :, :m]
            err = float(np.max(np.abs(got[low] - inv[low]) / np.maximum(1.0, np.abs(inv[low]))))
            bound = 100.0 * refs[g]["cond"] * EPS
            WORST["W"] = max(WORST["W"], err / bound)
            print("GRAD W m %d d %d g %d: err %.3g  bound %.3g  (cond %.3g; worst ratio so far %.3g)"
                  % (m, d, g, err, bound, refs[g]["cond"], WORST["W"]))
            assert err <= bound
            assert np.all(got[~low] == GUARD) and np.all(Wh[g, :, m:] == GUARD)
    # a flagged matrix is skipped and gets NaN; the others do not notice
    if G == 3:
        info = torch.tensor([0, 5, 0], dtype=torch.int32, device=dev)
        W2 = torch.full((G, m, m), GUARD, dtype=torch.float64, device=dev)
        L.check(lib.ital_chol_gram_inverse_batched(work.data_ptr(), m, G, info.data_ptr(), W2.data_ptr(), m, _stream()))
        lowd = torch.from_numpy(low).to(dev)
        assert bool(torch.isnan(W2[1][lowd]).all()) and bool((W2[1][~lowd] == GUARD).all())
        assert torch.equal(W2[0], W[0, :, :m]) and torch.equal(W2[2], W[2, :, :m])


# ------------------------------------------------------------------------------------------------ the gradient
@pytest.mark.parametrize("m,d,G", SHAPES)
def test_gradient_equals_the_host_and_the_value_has_the_bits_of_the_evidence(dev, m, d, G):
    X, y, cands = _case(m, d, G)
    for pad in (0, 3):
        r = _grad(X, y, cands, dev, pad=pad)
        assert r["status"] == 0 and not r["info"].any()
        assert torch.equal(r["values"], _evidence_lml(X, y, cands, dev, pad=pad))          # bit for bit
        gh = r["grad"].cpu().numpy()
        for g in range(G):
            h = _ref(m, d, g)
            bound = 100.0 * h["cond"] * EPS * np.maximum(1.0, h["scale"])
            err = np.abs(gh[g] - h["grad"])
            WORST["grad"] = max(WORST["grad"], float(np.max(err / bound)))
            print("GRAD m %d d %d g %d pad %d: err %s  bound %s  (worst ratio so far %.3g)"
                  % (m, d, g, pad, np.array2string(err, precision=3), np.array2string(bound, precision=3), WORST["grad"]))
            assert np.all(err <= bound), (g, err, bound)
            lml_err = abs(float(r["values"][g]) - h["lml"]) / max(1.0, abs(h["lml"]))
            assert lml_err <= 100.0 * h["cond"] * EPS


@pytest.mark.parametrize("m,d,G", SHAPES)
def test_gradient_equals_the_central_difference_of_the_devices_own_evidence(dev, m, d, G):
    X, y, cands = _case(m, d, G)
    hstep = 1e-4
    moved = []
    for c in cands:
        for k in range(3):
            for sgn in (1.0, -1.0):
                t = list(c)
                t[k] = t[k] * float(np.exp(sgn * hstep))
                moved.append(tuple(t))
    lml = _evidence_lml(X, y, moved, dev).cpu().numpy().reshape(len(cands), 3, 2)
    fd = (lml[:, :, 0] - lml[:, :, 1]) / (2 * hstep)
    got = _grad(X, y, cands, dev)["grad"].cpu().numpy()
    dev_ = np.abs(got - fd) / np.maximum(1.0, np.abs(got))
    WORST["fd"] = max(WORST["fd"], float(dev_.max()))
    print("GRAD fd m %d d %d G %d: deviation %s  bound 1e-06  (worst so far %.3g)"
          % (m, d, G, np.array2string(dev_.max(axis=0), precision=3), WORST["fd"]))
    assert np.all(dev_ <= 1e-6), (got, fd)


# ------------------------------------------------------------------------------------------------ batch independence
def _same(a, g, b, h):
    return all(torch.equal(a[k][g], b[k][h]) for k in ("values", "grad", "info"))


def test_a_candidate_gets_the_same_bits_alone_and_anywhere_in_a_batch(dev):
    rng = np.random.default_rng(5)
    m = 129
    X, y = rng.random((m, 10)), _labels(rng, m)
    five = [(1.0, 1.0, 1e-6), (0.7, 1.3, 1e-4), (1.5, 0.8, 1e-3), (0.9, 1.1, 1e-5), (2.0, 1.0, 1e-2)]
    alone = _grad(X, y, [five[2]], dev)
    middle = _grad(X, y, five, dev)
    first = _grad(X, y, five[2:] + five[:2], dev)
    last = _grad(X, y, five[3:] + five[:3], dev)
    assert _same(alone, 0, middle, 2) and _same(alone, 0, first, 0) and _same(alone, 0, last, 4)
    for g in range(5):
        assert _same(middle, g, first, (g - 2) % 5) and _same(middle, g, last, (g - 3) % 5)
    assert bool(torch.isfinite(middle["grad"]).all())


# ------------------------------------------------------------------------------------------------ the shared prologue
@pytest.mark.parametrize("m,d,G", [(1, 3, 1), (64, 3, 3), (65, 40, 3), (129, 3, 3)])
def test_both_chains_leave_the_same_prologue_state(dev, m, d, G):
    """ital_gp_evidence and ital_gp_evidence_grad on the same inputs, K and the workspaces filled with the guard value, both
    with leading dimension m: the same factors in K (and the same untouched rest of it), the same info, and the same alpha,
    inverse diagonals and M at the head of the workspace.  The pointer tables behind M hold addresses and are not compared."""
    X, y, cands = _case(m, d, G)
    e, g = _evidence(X, y, cands, dev), _grad(X, y, cands, dev)
    assert e["status"] == 0 and g["status"] == 0
    assert torch.equal(e["K"], g["K"])
    assert torch.equal(e["info"], g["info"])
    head = 2 * G * m + G * m * m
    assert torch.equal(e["work"][:head], g["work"][:head])
    assert not bool((e["work"][:2 * G * m] == GUARD).any())             # alpha and the inverse diagonals were written
    assert float(e["work"][e["need"]]) == GUARD                         # nothing behind ital_gp_evidence's workspace


@pytest.mark.parametrize("m", [1, 65, 129])
def test_the_gradient_costs_two_launches_more_and_neither_count_depends_on_G(dev, m):
    counts = {}
    for G in (1, 3):
        X, y, cands = _case(m, 3, G)
        counts[G] = (_evidence(X, y, cands, dev)["launches"], _grad(X, y, cands, dev)["launches"])
        print("GRAD launches m %d G %d: evidence %d  evidence_grad %d" % ((m, G) + counts[G]))
        assert counts[G][1] - counts[G][0] == 2
    assert counts[1] == counts[3]


def _gp(dev, X, ind, y, ls, **kw):
    from ital_amd import GaussianProcess
    gp = GaussianProcess(X, ls, device=dev, **kw)
    for a in range(0, len(ind), 16):
        gp.update(ind[a:a + 16], y[a:a + 16])
    return gp


def test_chunking_gives_the_same_arrays(dev):
    rng = np.random.default_rng(6)
    X = rng.random((90, 10))
    ind = [int(i) for i in rng.choice(90, 65, replace=False)]
    gp = _gp(dev, X, ind, _labels(rng, 65), 1.0)
    cands = [dict(length_scale=0.6 + 0.02 * g, var=1.0 + 0.01 * (g % 5), noise=10.0 ** -(2 + g % 5)) for g in range(7)]
    before = [t.clone() for t in (gp.L, gp.alpha, gp.V, gp.mu, gp.s2, gp.status)]
    one = gp.evidence_grad(cands)
    lib = _lib()[1]
    w1, w2 = (int(lib.ital_gp_evidence_grad_workspace(gp.m, c)) for c in (1, 2))
    per, shared = 8 * (gp.m * gp.m + (w2 - w1) + 5), 8 * (2 * w1 - w2)
    small = shared + 2 * per + per // 2
    assert gp.evidence_grad_chunk(small) == 2 and gp.evidence_grad_chunk() >= 7
    four = gp.evidence_grad(cands, max_bytes=small)                       # chunks of 2, 2, 2, 1
    assert one["ok"].all() and set(one) == {"lml", "grad", "ok"} and one["grad"].shape == (7, 3)
    for k in one:
        assert np.array_equal(one[k], four[k]), k
    assert np.array_equal(one["lml"], gp.evidence(cands)["lml"])          # the bits of evidence()
    assert all(torch.equal(a, b) for a, b in zip(before, (gp.L, gp.alpha, gp.V, gp.mu, gp.s2, gp.status)))
    with pytest.raises(MemoryError):
        gp.evidence_grad(cands, max_bytes=per // 2)
    with pytest.raises(ValueError):
        gp.evidence_grad([dict(length_scale=0.0)])
    with pytest.raises(ValueError):
        gp.evidence_grad([dict(length_scale=1.0, var=-1.0)])
    with pytest.raises(TypeError):
        gp.evidence_grad([dict(lengthscale=1.0)])
    from ital_amd import GaussianProcess
    with pytest.raises(RuntimeError):
        GaussianProcess(X, 0.5, device=dev).evidence_grad([dict(length_scale=1.0)])


# ------------------------------------------------------------------------------------ a Gram that is not positive definite
def _twins(rng, n, d):
    """Rows whose first two are identical and made of eighths: their squared norms, their dot product and so their distance 0
    are exact in floating point, and with var = 1, noise = 0 the second pivot is exactly 1 - 1 * 1 = 0."""
    X = rng.random((n, d))
    X[0] = X[1] = rng.integers(0, 8, d) / 8.0
    return X


def test_an_indefinite_candidate_among_good_ones(dev):
    rng = np.random.default_rng(7)
    m = 65
    X, y = _twins(rng, m, 10), _labels(rng, m)
    good = [(1.0, 1.0, 1e-3), (0.8, 1.2, 1e-2), (1.3, 0.9, 1e-3)]
    bad = (1.0, 1.0, 0.0)
    mixed = _grad(X, y, [good[0], bad, good[1], good[2]], dev)
    clean = _grad(X, y, good, dev)
    assert clean["status"] == 0 and mixed["status"] & 1
    assert mixed["info"].cpu().tolist() == [0, 2, 0, 0]
    assert (mixed["info"] == 0).cpu().tolist() == [True, False, True, True]
    assert float(mixed["values"][1]) == -np.inf and bool(torch.isnan(mixed["grad"][1]).all())
    for g, h in ((0, 0), (2, 1), (3, 2)):
        assert _same(mixed, g, clean, h)
    assert bool(torch.isfinite(clean["grad"]).all())


def test_fit_params_refuses_when_nothing_is_positive_definite(dev):
    from ital_amd import ITAL
    rng = np.random.default_rng(8)
    X = _twins(rng, 80, 10)
    A = ITAL(X, length_scale=1.0, var=1.0, noise=1e-3, device=dev)
    A.update({0: 1, 1: 1})                                   # the twins are labelled rows 0 and 1
    A.update({int(i): (1 if i % 3 else -1) for i in range(5, 25)})
    ev = A.gp.evidence_grad([dict(noise=1e-3), dict(noise=0.0), dict(length_scale=0.7), dict(var=2.0)])
    assert ev["ok"].tolist() == [True, False, True, True]
    assert ev["lml"][1] == -np.inf and np.isnan(ev["grad"][1]).all() and np.isfinite(ev["grad"][[0, 2, 3]]).all()
    gp = A.gp
    before = [t.clone() for t in (gp.L, gp.alpha, gp.V, gp.mu, gp.s2)]
    rounds = A.rounds
    with pytest.raises(np.linalg.LinAlgError):               # only the length scale moves: every start keeps noise = 0
        A.fit_params(params=("length_scale",), init=dict(noise=0.0), restarts=4)
    assert all(torch.equal(a, b) for a, b in zip(before, (gp.L, gp.alpha, gp.V, gp.mu, gp.s2)))
    assert (A.length_scale, A.var, A.noise) == (1.0, 1.0, 1e-3) == (gp.length_scale, gp.var, gp.noise)
    assert A.rounds == rounds and int(gp.status.item()) == 0
    assert len(A.fetch_unlabelled(4)) == 4                   # the session goes on


# ------------------------------------------------------------------------------------------------ a session
def _two_clusters():
    rng = np.random.default_rng(64)
    X = np.concatenate((rng.normal(0, 0.5, (150, 8)), rng.normal(0, 0.5, (150, 8)) + 0.35))
    truth = np.where(np.arange(300) < 150, 1, -1)
    ids = [int(i) for i in rng.choice(300, 36, replace=False)]
    return X, [{i: int(truth[i]) for i in ids[a:a + 12]} for a in range(0, 36, 12)]


def _session(cls, dev, store=True, **kw):
    from ital_amd import DeviceData, mvn_stream
    X, history = _two_clusters()
    mvn_stream.GLOBAL.reset()
    np.random.seed(1)
    A = cls(DeviceData(X, device=dev) if store else X, length_scale=0.5, var=1.0, noise=1e-2, device=dev, **kw)
    for g in history:
        A.update(g)
    return A, X, history


def test_fit_params_on_a_live_session(dev, capsys):
    from ital_amd import ITAL, mvn_stream, tune
    A, X, history = _session(ITAL, dev)
    gp = A.gp
    current = dict(length_scale=0.5, var=1.0, noise=1e-2)
    before = [t.clone() for t in (gp.L, gp.alpha, gp.V, gp.mu, gp.s2, gp.status)]
    np_state, rounds = np.random.get_state(), A.rounds
    mvn_state = (tuple(mvn_stream.GLOBAL.state), int(mvn_stream.GLOBAL.draws))

    best, lml = A.fit_params(apply=False)
    assert all(torch.equal(a, b) for a, b in zip(before, (gp.L, gp.alpha, gp.V, gp.mu, gp.s2, gp.status)))
    assert (gp.length_scale, gp.var, gp.noise) == (0.5, 1.0, 1e-2) == (A.length_scale, A.var, A.noise)
    now = np.random.get_state()
    assert A.rounds == rounds and now[0] == np_state[0] and np.array_equal(now[1], np_state[1]) and now[2:] == np_state[2:]
    assert (tuple(mvn_stream.GLOBAL.state), int(mvn_stream.GLOBAL.draws)) == mvn_state
    assert capsys.readouterr().out == ""                                  # verbose = 0 prints nothing
    here = tune.session_scores(A, [current], "lml")[0]
    assert set(best) == {"length_scale", "var", "noise"} and lml >= here

    # the same search with the host's evaluator on the same starts
    host_best, host_lml, _ = tune.maximize_lml(ref.evaluator(X[gp.ind], gp.y), tune.session_starts(current, 8))
    print("GRAD fit_params: device %.10g at %r; host %.10g at %r; session now %.10g" % (lml, best, host_lml, host_best, here))
    assert abs(lml - host_lml) <= 1e-6 * max(1.0, abs(host_lml))

    # applied: what set_params(**best) gives on a clone
    twin = A.clone()
    twin.set_params(**best)
    best2, lml2 = A.fit_params()
    assert (best2, lml2) == (best, lml)
    assert (A.length_scale, A.var, A.noise) == (best["length_scale"], best["var"], best["noise"]) == \
        (gp.length_scale, gp.var, gp.noise)
    assert torch.equal(A.gp.mu, twin.gp.mu) and torch.equal(A.gp.s2, twin.gp.s2)
    now = np.random.get_state()
    assert A.rounds == rounds and np.array_equal(now[1], np_state[1]) and now[2:] == np_state[2:]
    assert (tuple(mvn_stream.GLOBAL.state), int(mvn_stream.GLOBAL.draws)) == mvn_state
    assert len(set(A.fetch_unlabelled(4))) == 4                           # the session goes on


def test_fit_params_of_the_length_scale_alone(dev):
    from ital_amd import ITAL, tune
    A, X, history = _session(ITAL, dev)
    var, noise = 1.2345678901234567, 0.012345678901234567
    A.set_params(var=var, noise=noise)
    here = tune.session_scores(A, [dict()], "lml")[0]
    best, lml = A.fit_params(params=("length_scale",))
    assert set(best) == {"length_scale"} and lml >= here
    assert (A.var, A.noise) == (var, noise) == (A.gp.var, A.gp.noise)     # bit-identical
    assert A.length_scale == best["length_scale"] == A.gp.length_scale != 0.5
    grid = [dict(length_scale=best["length_scale"] * f) for f in (0.9, 1.0, 1.1)]
    around = tune.session_scores(A, grid, "lml")
    print("GRAD ls only: lml %.10g at %g; 10 %% below %.10g, above %.10g" % (lml, best["length_scale"], around[0], around[2]))
    assert around[1] == lml and around[1] > around[0] and around[1] > around[2]      # a maximum along the one free axis


def test_fit_params_through_mcmi(dev):
    """The inherited method beyond ITAL: the same fit, and the learner goes on with the new parameters."""
    from ital_amd import MCMI_min, tune
    A, X, history = _session(MCMI_min, dev, store=False, subsample=60)
    current = dict(length_scale=0.5, var=1.0, noise=1e-2)
    host_best, host_lml, _ = tune.maximize_lml(ref.evaluator(X[A.gp.ind], A.gp.y), tune.session_starts(current, 8))
    best, lml = A.fit_params()
    assert abs(lml - host_lml) <= 1e-6 * max(1.0, abs(host_lml))
    assert (A.gp.length_scale, A.gp.var, A.gp.noise) == (best["length_scale"], best["var"], best["noise"])
    assert (A.length_scale, A.var, A.noise) == (A.gp.length_scale, A.gp.var, A.gp.noise)
    np.random.seed(4)
    picks = A.fetch_unlabelled(3)
    assert len(set(picks)) == 3
