"""The leave-one-out scores' gradients in the log-parameters on the device (include/ital_loo_grad.h, csrc/loo_grad.hip) and
what is built on them: GaussianProcess.loo_grad, tune.fit_session_params(criterion=...) and ActiveRetrievalBase.fit_params.

Inputs are those of tests/test_gpu_evidence.py (tests/_evidence_inputs.py).  Every shape gets three candidates: the shape's
first candidate there, its second with noise = 10 var (the noise dominates: W Kf = I - noise W would cancel) and its third
with noise = 1e-8 (the floor of the fit's box).  The references are computed here with numpy / scipy in float64
(tests/_loo_grad_ref.py).  No bound comes from a measurement on the device:

- every gradient component within 100 * cond(K) * 2^-52 * max(1, S) of the host's, S being the forward-error scale of the
  component's sum (S_logp, S_mse of the reference): the form of the bound of tests/test_gpu_evidence_grad.py.  A float64
  evaluation on the host stays below 0.022 of it against an 80-bit long-double one, cond up to 4e9;
- against the central difference of the device's own loo_logp and loo_mse (ital_gp_evidence) at h = 1e-4 in each
  log-parameter: 1e-6 * max(1, |g|), the project's bound for lml;
- d loo_logp / d log var + d loo_logp / d log noise = -m / 2 + 1/2 sum_i alpha_i^2 / c_i with the right side from
  ital_gp_evidence's loo_mean and loo_var (alpha_i / c_i = y_i - mean_i, 1 / c_i = var_i): the same bound.

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

import _loo_grad_ref as ref  # noqa: E402
from _evidence_inputs import CANDS, GUARD, _case, _evidence, _labels, _lib, _params, _stream, _upload  # noqa: E402

EPS = 2.0 ** -52
NAN = float("nan")
WORST = {"grad": 0.0, "fd": 0.0, "scale": 0.0}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


def _cands(d):
    """The three candidates of every shape with d features (see the module's docstring)."""
    a, b, c = CANDS[d]
    return [a, (b[0], b[1], 10.0 * b[1]), (c[0], c[1], 1e-8)]


def _desc(XT, XTn, ldx, yd, m, prm, G, K, ld, values, grad, info, status, work, need):
    L, _ = _lib()
    d = L.ItalLooGradDesc()
    d.XT, d.XTn, d.ldx, d.y, d.m, d.params, d.G = XT.data_ptr(), XTn.data_ptr(), ldx, yd.data_ptr(), m, prm.data_ptr(), G
    d.K, d.ld, d.values, d.grad, d.info = K.data_ptr(), ld, values.data_ptr(), grad.data_ptr(), info.data_ptr()
    d.status, d.work, d.work_doubles, d.ev = status.data_ptr(), work.data_ptr(), need, None
    return d


def _loo(X, y, cands, dev, pad=0, fill=GUARD):
    """ital_gp_loo_grad on G candidates; leading dimension m + pad; K and the workspace start as `fill`; one guard element
    behind every output and behind the workspace."""
    L, lib = _lib()
    XT, XTn, ldx = _upload(X, dev)
    m, G = len(X), len(cands)
    ld = m + pad
    yd = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).to(dev)
    prm = _params(cands, dev)
    K = torch.full((G, m, ld), fill, dtype=torch.float64, device=dev)
    need = int(lib.ital_gp_loo_grad_workspace(m, G))
    work = torch.full((need + 1,), fill, dtype=torch.float64, device=dev)
    work[need] = GUARD
    values = torch.full((G + 1, 2), GUARD, dtype=torch.float64, device=dev)
    grad = torch.full((G + 1, 2, 3), GUARD, dtype=torch.float64, device=dev)
    info = torch.full((G + 1,), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    d = _desc(XT, XTn, ldx, yd, m, prm, G, K, ld, values, grad, info, status, work, need)
    before = int(lib.ital_launch_count())
    L.check(lib.ital_gp_loo_grad(ctypes.byref(d), _stream()))
    launches = int(lib.ital_launch_count()) - before
    torch.cuda.synchronize()
    assert bool((values[G] == GUARD).all()) and bool((grad[G] == GUARD).all()) and int(info[G]) == -1 and int(status[1]) == 0
    assert float(work[need]) == GUARD
    if fill == GUARD:
        assert bool((K[:, :, m:] == GUARD).all())                           # nothing beyond column m of the Grams
        up = torch.triu(torch.ones((m, m), dtype=torch.bool, device=dev), 1)
        assert bool((K[:, :, :m][:, up] == GUARD).all())                    # nothing above their diagonals
    return dict(values=values[:G], grad=grad[:G], info=info[:G], status=int(status[0].item()), launches=launches)


def _same(a, g, b, h):
    return all(torch.equal(a[k][g], b[k][h]) for k in ("values", "grad", "info"))


SHAPES = [(m, d) for m in (1, 2, 17, 63, 64, 65, 127, 128, 129, 200, 257) for d in (3, 40)]


@functools.lru_cache(maxsize=None)
def _ref(m, d, g):
    """The host's values for candidate g of the shape's inputs: computed once, shared by the tests, never written to."""
    X, y, _ = _case(m, d, 1)
    h = ref.host_loo(ref.sqdist(X), y, *_cands(d)[g])
    assert h is not None, (m, d, g)
    return h


# ------------------------------------------------------------------------------------------------ the gradient
@pytest.mark.parametrize("m,d", SHAPES)
def test_gradients_equal_the_host_and_the_values_have_the_bits_of_the_evidence(dev, m, d):
    """G = 3 and each candidate alone (G = 1), leading dimensions m and m + 3."""
    X, y, _ = _case(m, d, 1)
    cands = _cands(d)
    for pad in (0, 3):
        ev = _evidence(X, y, cands, dev, pad=pad)
        three = _loo(X, y, cands, dev, pad=pad)
        assert three["status"] == 0 and not three["info"].any()
        assert torch.equal(three["values"], ev["scores"][:, 1:3])                   # bit for bit
        got = three["grad"].cpu().numpy()
        assert np.all(np.isfinite(got))
        for g in range(3):
            one = _loo(X, y, cands[g:g + 1], dev, pad=pad)
            assert one["status"] == 0 and _same(one, 0, three, g)                  # G = 1: the same bits
            h = _ref(m, d, g)
            for k, name in enumerate(("logp", "mse")):
                bound = 100.0 * h["cond"] * EPS * np.maximum(1.0, h["scale_" + name])
                err = np.abs(got[g, k] - h["grad_" + name])
                WORST["grad"] = max(WORST["grad"], float(np.max(err / bound)))
                print("LOO %s m %d d %d g %d pad %d: err %s  bound %s  cond %.3g  (worst ratio so far %.3g)"
                      % (name, m, d, g, pad, np.array2string(err, precision=3), np.array2string(bound, precision=3),
                         h["cond"], WORST["grad"]))
                assert np.all(err <= bound), (g, name, err, bound)


@pytest.mark.parametrize("m,d", SHAPES)
def test_nothing_unwritten_is_read(dev, m, d):
    """K and the whole workspace start as NaN: the outputs are finite and have the bits of a run that starts from zeros."""
    X, y, _ = _case(m, d, 1)
    cands = _cands(d)
    for pad in (0, 3):
        nan, zero = _loo(X, y, cands, dev, pad=pad, fill=NAN), _loo(X, y, cands, dev, pad=pad, fill=0.0)
        assert nan["status"] == 0 and zero["status"] == 0
        assert bool(torch.isfinite(nan["values"]).all()) and bool(torch.isfinite(nan["grad"]).all())
        assert all(torch.equal(nan[k], zero[k]) for k in ("values", "grad", "info"))


@pytest.mark.parametrize("m", [64, 129])
def test_gradients_equal_the_central_difference_of_the_devices_own_evidence(dev, m):
    d = 40
    X, y, _ = _case(m, d, 1)
    cands = _cands(d)
    hstep = 1e-4
    moved = []
    for c in cands:
        for k in range(3):
            for sgn in (1.0, -1.0):
                t = list(c)
                t[k] = t[k] * float(np.exp(sgn * hstep))
                moved.append(tuple(t))
    sc = _evidence(X, y, moved, dev)["scores"][:, 1:3].cpu().numpy().reshape(len(cands), 3, 2, 2)    # [g][param][+/-][criterion]
    fd = np.transpose((sc[:, :, 0, :] - sc[:, :, 1, :]) / (2 * hstep), (0, 2, 1))                     # [g][criterion][param]
    got = _loo(X, y, cands, dev)["grad"].cpu().numpy()
    dev_ = np.abs(got - fd) / np.maximum(1.0, np.abs(got))
    WORST["fd"] = max(WORST["fd"], float(dev_.max()))
    print("LOO fd m %d: deviation per candidate and criterion %s  bound 1e-06  (worst so far %.3g)"
          % (m, np.array2string(dev_.max(axis=2), precision=3), WORST["fd"]))
    assert np.all(dev_ <= 1e-6), (got, fd)


@pytest.mark.parametrize("m,d", [(2, 3), (64, 40), (129, 40), (257, 3)])
def test_scaling_var_and_noise_together_on_the_device_alone(dev, m, d):
    X, y, _ = _case(m, d, 1)
    cands = _cands(d)
    ev = _evidence(X, y, cands, dev)
    lm, lv = ev["loo_mean"][:, :m].cpu().numpy(), ev["loo_var"][:, :m].cpu().numpy()
    want = -m / 2.0 + 0.5 * np.sum((y[None, :] - lm) ** 2 / lv, axis=1)          # alpha_i^2 / c_i = (y_i - mean_i)^2 / var_i
    got = _loo(X, y, cands, dev)["grad"].cpu().numpy()
    for g in range(3):
        h = _ref(m, d, g)
        bound = 100.0 * h["cond"] * EPS * max(1.0, h["scale_logp"][1] + h["scale_logp"][2])
        err = abs(got[g, 0, 1] + got[g, 0, 2] - want[g])
        WORST["scale"] = max(WORST["scale"], err / bound)
        print("LOO scale identity m %d d %d g %d: err %.3g  bound %.3g  (worst ratio so far %.3g)"
              % (m, d, g, err, bound, WORST["scale"]))
        assert err <= bound


# ------------------------------------------------------------------------------------------------ batch independence
def test_a_candidate_gets_the_same_bits_alone_and_anywhere_in_a_batch(dev):
    rng = np.random.default_rng(5)
    m = 257
    X, y = rng.random((m, 10)), _labels(rng, m)
    five = [(1.0, 1.0, 1e-6), (0.7, 1.3, 1e-4), (1.5, 0.8, 8.0), (0.9, 1.1, 1e-8), (2.0, 1.0, 1e-2)]
    alone = _loo(X, y, [five[2]], dev)
    middle = _loo(X, y, five, dev)
    first = _loo(X, y, five[2:] + five[:2], dev)
    last = _loo(X, y, five[3:] + five[:3], dev)
    assert _same(alone, 0, middle, 2) and _same(alone, 0, first, 0) and _same(alone, 0, last, 4)
    for g in range(5):
        assert _same(middle, g, first, (g - 2) % 5) and _same(middle, g, last, (g - 3) % 5)
    assert bool(torch.isfinite(middle["grad"]).all())


@pytest.mark.parametrize("m", [1, 65, 129, 257])
def test_the_chain_costs_three_launches_more_than_the_evidence_whatever_G(dev, m):
    counts = {}
    for G in (1, 3):
        X, y, _ = _case(m, 3, 1)
        cands = _cands(3)[:G]
        counts[G] = (_evidence(X, y, cands, dev)["launches"], _loo(X, y, cands, dev)["launches"])
        print("LOO launches m %d G %d: evidence %d  loo_grad %d" % ((m, G) + counts[G]))
        assert counts[G][1] - counts[G][0] == 3          # distances, W, product, and the reduction in place of evidence's
    assert counts[1] == counts[3]


def _gp(dev, X, ind, y, ls, **kw):
    from ital_amd import GaussianProcess
    gp = GaussianProcess(X, ls, device=dev, **kw)
    for a in range(0, len(ind), 16):
        gp.update(ind[a:a + 16], y[a:a + 16])
    return gp


def test_chunking_gives_the_same_arrays(dev):
    rng = np.random.default_rng(6)
    X = rng.random((200, 10))
    ind = [int(i) for i in rng.choice(200, 130, replace=False)]
    gp = _gp(dev, X, ind, _labels(rng, 130), 1.0)
    cands = [dict(length_scale=0.6 + 0.02 * g, var=1.0 + 0.01 * (g % 5), noise=10.0 ** -(2 + g % 5)) for g in range(7)]
    before = [t.clone() for t in (gp.L, gp.alpha, gp.V, gp.mu, gp.s2, gp.status)]
    one = gp.loo_grad(cands)
    lib = _lib()[1]
    w1, w2 = (int(lib.ital_gp_loo_grad_workspace(gp.m, c)) for c in (1, 2))
    per, shared = 8 * (gp.m * gp.m + (w2 - w1) + 9), 8 * (2 * w1 - w2)
    small = shared + 2 * per + per // 2
    assert gp.loo_grad_chunk(small) == 2 and gp.loo_grad_chunk() >= 7
    four = gp.loo_grad(cands, max_bytes=small)                            # chunks of 2, 2, 2, 1
    assert one["ok"].all() and set(one) == {"loo_logp", "loo_mse", "grad_logp", "grad_mse", "ok"}
    assert one["grad_logp"].shape == (7, 3) == one["grad_mse"].shape
    for k in one:
        assert np.array_equal(one[k], four[k]), k
    ev = gp.evidence(cands)
    assert np.array_equal(one["loo_logp"], ev["loo_logp"]) and np.array_equal(one["loo_mse"], ev["loo_mse"])
    assert all(torch.equal(a, b) for a, b in zip(before, (gp.L, gp.alpha, gp.V, gp.mu, gp.s2, gp.status)))
    with pytest.raises(MemoryError):
        gp.loo_grad(cands, max_bytes=per // 2)
    with pytest.raises(ValueError):
        gp.loo_grad([dict(length_scale=0.0)])
    with pytest.raises(TypeError):
        gp.loo_grad([dict(lengthscale=1.0)])
    from ital_amd import GaussianProcess
    with pytest.raises(RuntimeError):
        GaussianProcess(X, 0.5, device=dev).loo_grad([dict(length_scale=1.0)])


# ------------------------------------------------------------------------------------ a Gram that is not positive definite
def _twins(rng, n, d):
    """Rows whose first two are identical and made of eighths: their squared norms, their dot product and so their distance 0
    are exact in floating point, and with var = 1, noise = 0 the second pivot is exactly 1 - 1 * 1 = 0."""
    X = rng.random((n, d))
    X[0] = X[1] = rng.integers(0, 8, d) / 8.0
    return X


def test_an_indefinite_candidate_among_good_ones(dev):
    rng = np.random.default_rng(7)
    m = 130
    X, y = _twins(rng, m, 10), _labels(rng, m)
    good = [(1.0, 1.0, 1e-3), (0.8, 1.2, 1e-2), (1.3, 0.9, 1e-3)]
    bad = (1.0, 1.0, 0.0)
    mixed = _loo(X, y, [good[0], bad, good[1], good[2]], dev)
    clean = _loo(X, y, good, dev)
    assert clean["status"] == 0 and mixed["status"] & 1
    assert mixed["info"].cpu().tolist() == [0, 2, 0, 0]
    assert float(mixed["values"][1, 0]) == -np.inf and float(mixed["values"][1, 1]) == np.inf
    assert bool(torch.isnan(mixed["grad"][1]).all())
    for g, h in ((0, 0), (2, 1), (3, 2)):
        assert _same(mixed, g, clean, h)
    assert bool(torch.isfinite(clean["grad"]).all())


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_before_any_launch(dev):
    L, lib = _lib()
    X, y, _ = _case(17, 3, 1)
    XT, XTn, ldx = _upload(X, dev)
    m, G = 17, 3
    yd = torch.from_numpy(y).to(dev)
    prm = _params(_cands(3), dev)
    K = torch.full((G, m, m), GUARD, dtype=torch.float64, device=dev)
    need = int(lib.ital_gp_loo_grad_workspace(m, G))
    work = torch.full((need,), GUARD, dtype=torch.float64, device=dev)
    values = torch.full((G, 2), GUARD, dtype=torch.float64, device=dev)
    grad = torch.full((G, 2, 3), GUARD, dtype=torch.float64, device=dev)
    info = torch.full((G,), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    before = int(lib.ital_launch_count())
    bads = [dict(XT=None), dict(XTn=None), dict(y=None), dict(params=None), dict(K=None), dict(values=None), dict(grad=None),
            dict(info=None), dict(status=None), dict(work=None), dict(ldx=0), dict(ldx=8), dict(ldx=24), dict(ld=m - 1),
            dict(m=0), dict(G=0), dict(G=65536), dict(work_doubles=need - 1)]
    for bad in bads:
        d = _desc(XT, XTn, ldx, yd, m, prm, G, K, m, values, grad, info, status, work, need)
        for k, v in bad.items():
            setattr(d, k, v)
        assert lib.ital_gp_loo_grad(ctypes.byref(d), _stream()) == -22, bad
        assert "ital_gp_loo_grad" in lib.ital_last_error().decode()
    assert lib.ital_gp_loo_grad(None, _stream()) == -22
    assert int(lib.ital_launch_count()) == before
    torch.cuda.synchronize()
    assert bool((values == GUARD).all()) and bool((grad == GUARD).all()) and bool((work == GUARD).all())
    assert bool((info == -1).all()) and int(status.item()) == 0 and bool((K == GUARD).all())
    # and the good descriptor goes through
    d = _desc(XT, XTn, ldx, yd, m, prm, G, K, m, values, grad, info, status, work, need)
    L.check(lib.ital_gp_loo_grad(ctypes.byref(d), _stream()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad).all()) and not info.any()


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


CURRENT = dict(length_scale=0.5, var=1.0, noise=1e-2)


def test_fit_params_by_loo_logp_on_a_live_session(dev, capsys):
    from ital_amd import ITAL, mvn_stream, tune
    A, X, history = _session(ITAL, dev)
    gp = A.gp
    before = [t.clone() for t in (gp.L, gp.alpha, gp.V, gp.mu, gp.s2, gp.status)]
    np_state, rounds = np.random.get_state(), A.rounds
    mvn_state = (tuple(mvn_stream.GLOBAL.state), int(mvn_stream.GLOBAL.draws))

    best, score = A.fit_params(apply=False, criterion="loo_logp")
    assert all(torch.equal(a, b) for a, b in zip(before, (gp.L, gp.alpha, gp.V, gp.mu, gp.s2, gp.status)))
    assert (gp.length_scale, gp.var, gp.noise) == (0.5, 1.0, 1e-2) == (A.length_scale, A.var, A.noise)
    now = np.random.get_state()
    assert A.rounds == rounds and now[0] == np_state[0] and np.array_equal(now[1], np_state[1]) and now[2:] == np_state[2:]
    assert (tuple(mvn_stream.GLOBAL.state), int(mvn_stream.GLOBAL.draws)) == mvn_state
    assert capsys.readouterr().out == ""                                  # verbose = 0 prints nothing
    here = tune.session_scores(A, [CURRENT], "loo_logp")[0]
    assert set(best) == {"length_scale", "var", "noise"} and score >= here

    # the same search with the host's evaluator on the same starts
    host_best, host_score, _ = tune.maximize_lml(ref.evaluator(X[gp.ind], gp.y), tune.session_starts(CURRENT, 8))
    print("LOO fit_params: device %.10g at %r; host %.10g at %r; session now %.10g" % (score, best, host_score, host_best, here))
    assert abs(score - host_score) <= 1e-6 * max(1.0, abs(host_score))

    # applied: what set_params(**best) gives on a clone
    twin = A.clone()
    twin.set_params(**best)
    best2, score2 = A.fit_params(criterion="loo_logp")
    assert (best2, score2) == (best, score)
    assert (A.length_scale, A.var, A.noise) == (best["length_scale"], best["var"], best["noise"]) == \
        (gp.length_scale, gp.var, gp.noise)
    assert torch.equal(A.gp.mu, twin.gp.mu) and torch.equal(A.gp.s2, twin.gp.s2)
    now = np.random.get_state()
    assert A.rounds == rounds and np.array_equal(now[1], np_state[1]) and now[2:] == np_state[2:]
    assert (tuple(mvn_stream.GLOBAL.state), int(mvn_stream.GLOBAL.draws)) == mvn_state
    assert len(set(A.fetch_unlabelled(4))) == 4                           # the session goes on


def test_fit_params_by_loo_mse_leaves_var_untouched(dev):
    from ital_amd import ITAL, tune
    A, X, history = _session(ITAL, dev)
    var = 1.2345678901234567
    A.set_params(var=var)
    here = tune.session_scores(A, [dict()], "loo_mse")[0]
    best, score = A.fit_params(params=("length_scale", "noise"), criterion="loo_mse")
    print("LOO fit_params loo_mse: %.10g at %r; session before %.10g" % (score, best, here))
    assert set(best) == {"length_scale", "noise"} and score >= here and score < 0        # minus the mse
    assert A.var == var == A.gp.var                                       # bit-identical
    assert (A.length_scale, A.noise) == (best["length_scale"], best["noise"]) == (A.gp.length_scale, A.gp.noise)
    assert tune.session_scores(A, [dict()], "loo_mse")[0] == score
    with pytest.raises(ValueError, match="fit at most one of var and noise"):
        A.fit_params(criterion="loo_mse")
    with pytest.raises(ValueError, match="loo_ap"):
        A.fit_params(criterion="loo_ap")


def test_fit_params_by_loo_logp_through_mcmi(dev):
    """The inherited method beyond ITAL: the same fit, and the learner goes on with the new parameters."""
    from ital_amd import MCMI_min, tune
    A, X, history = _session(MCMI_min, dev, store=False, subsample=60)
    host_best, host_score, _ = tune.maximize_lml(ref.evaluator(X[A.gp.ind], A.gp.y), tune.session_starts(CURRENT, 8))
    best, score = A.fit_params(criterion="loo_logp")
    assert abs(score - host_score) <= 1e-6 * max(1.0, abs(host_score))
    assert (A.gp.length_scale, A.gp.var, A.gp.noise) == (best["length_scale"], best["var"], best["noise"])
    assert (A.length_scale, A.var, A.noise) == (A.gp.length_scale, A.gp.var, A.gp.noise)
    np.random.seed(4)
    picks = A.fetch_unlabelled(3)
    assert len(set(picks)) == 3
