"""GP evidence and closed-form leave-one-out scores of many hyper-parameter candidates on the device (include/ital_evidence.h,
csrc/evidence.hip) and what is built on them: GaussianProcess.evidence, tune.session_scores / optimize_session_params and
ActiveRetrievalBase.tune_params.

The references are computed here with numpy / scipy in float64, K from the same expansion |x_i|^2 + |x_j|^2 - 2 x_i.x_j.  Two
bounds need no measurement: K entries within rtol 1e-12 (the project's bar for RBF values, tests/test_gpu_parity.py), and
every score, loo_mean, loo_var and inverse diagonal within 100 * cond(K) * 2^-52 of max(1, |value|) -- cond times epsilon of
a backward-stable solve, the factor 100 for the growth with m and d; cond from numpy.linalg.cond, kept below 1e5, so the bar
is at most 2e-9, the project's GP bar.  Every comparison prints its figure before it asserts (run with -s to see them).
Run: python -m pytest tests -m gpu."""
import functools
import os
import sys
import warnings
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from _evidence_inputs import CANDS, GUARD, _case, _evidence, _labels, _lib, _params, _stream, _upload  # noqa: E402

EPS = 2.0 ** -52
K_RTOL = 1e-12
APPEND_ATOL = 2e-9       # set_params' bar (tests/test_gpu_rewhiten.py)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


# ------------------------------------------------------------------------------------------------ host reference
def _host(X, y, ls, var, noise):
    """The quantities of include/ital_evidence.h in float64 on the host."""
    import scipy.linalg as sl
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    m = len(X)
    sn = (X * X).sum(axis=1)
    D = sn[:, None] + sn[None, :] - 2.0 * (X @ X.T)
    K = var * np.exp(D / (-2.0 * ls * ls)) + noise * np.eye(m)
    L = np.linalg.cholesky(K)
    alpha = sl.cho_solve((L, True), y)
    Minv = sl.solve_triangular(L, np.eye(m), lower=True)
    c = (Minv * Minv).sum(axis=0)
    mean, v = y - alpha / c, 1.0 / c
    return dict(K=K, L=L, cdiag=c, cond=float(np.linalg.cond(K)),
                lml=-0.5 * float(y @ alpha) - float(np.log(np.diag(L)).sum()) - 0.5 * m * np.log(2 * np.pi),
                loo_logp=float((-0.5 * np.log(v) - (y - mean) ** 2 / (2 * v) - 0.5 * np.log(2 * np.pi)).sum()),
                loo_mse=float(np.mean((alpha / c) ** 2)), loo_mean=mean, loo_var=v)


def _within(got, want, cond, what):
    assert cond < 1e5, (what, cond)
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
    bound = 100.0 * cond * EPS
    print("EVID %-10s err %.3g  bound %.3g  (cond %.3g)" % (what, err, bound, cond))
    assert err <= bound, (what, err, bound, cond)


# ------------------------------------------------------------------------------------------------ the C ABI, directly
SHAPES = [(m, d, G) for m in (1, 2, 17, 63, 64, 65, 129, 200) for d in (3, 40) for G in (1, 3)]


@functools.lru_cache(maxsize=None)
def _ref(m, d, g):
    """The host's values for candidate g of the shape's inputs: computed once, shared by the tests, never written to."""
    X, y, _ = _case(m, d, 1)
    return _host(X, y, *CANDS[d][g])


@pytest.mark.parametrize("m,d,G", SHAPES)
def test_gram_grid_equals_the_host_kernel_matrix(dev, m, d, G):
    L, lib = _lib()
    X, _, cands = _case(m, d, G)
    XT, XTn, ldx = _upload(X, dev)
    ld = m + 3
    K = torch.full((G, m, ld), GUARD, dtype=torch.float64, device=dev)
    L.check(lib.ital_gram_grid(XT.data_ptr(), XTn.data_ptr(), m, ldx, _params(cands, dev).data_ptr(), G, K.data_ptr(), ld,
                               _stream()))
    Kh = K.cpu().numpy()
    low = np.tril(np.ones((m, m), dtype=bool))
    for g, c in enumerate(cands):
        want = _ref(m, d, g)["K"]
        got = Kh[g, :, :m]
        err = float(np.max(np.abs(got[low] - want[low]) / np.abs(want[low])))
        print("EVID %-10s err %.3g  bound %.3g" % ("K", err, K_RTOL))
        assert err <= K_RTOL, (g, err)
        assert np.all(got[~low] == GUARD) and np.all(Kh[g, :, m:] == GUARD)      # the lower triangle and nothing else


@pytest.mark.parametrize("d", [5, 20, 40])            # ldx 16, 32, 48: one k-stage; both LDS buffers; an odd count of stages
@pytest.mark.parametrize("m", [1, 128, 129, 257])     # one tile pair; the exact edge; three pairs, ragged; six pairs
def test_gram_grid_of_one_candidate_has_the_bits_of_gram_rows(dev, m, d):
    """ital_gram_grid at G = 1 and ital_gram_rows over rows 0 .. m-1 (identity index) run the same tile (csrc/mfma_tile.h) and
    the same distance expression: the same bits in the lower triangle, and neither writes anything else."""
    L, lib = _lib()
    ls, var, noise = 0.7, 1.3, 1e-3
    X = np.random.default_rng(77).random((m, d))
    XT, XTn, ldx = _upload(X, dev)
    ld = m + 3
    grid = torch.full((1, m, ld), GUARD, dtype=torch.float64, device=dev)
    L.check(lib.ital_gram_grid(XT.data_ptr(), XTn.data_ptr(), m, ldx, _params([(ls, var, noise)], dev).data_ptr(), 1,
                               grid.data_ptr(), ld, _stream()))
    rows = torch.full((m, ld), GUARD, dtype=torch.float64, device=dev)
    idx = torch.arange(m, dtype=torch.int64, device=dev)
    ip, kp, ldp = (torch.tensor([v], dtype=torch.int64, device=dev) for v in (idx.data_ptr(), rows.data_ptr(), ld))
    npt = torch.tensor([m], dtype=torch.int32, device=dev)
    L.check(lib.ital_gram_rows(XT.data_ptr(), XTn.data_ptr(), ldx, ip.data_ptr(), npt.data_ptr(), kp.data_ptr(), ldp.data_ptr(),
                               1, m, var, ls, noise, _stream()))
    a, b = grid.cpu().numpy()[0], rows.cpu().numpy()
    low = np.tril(np.ones((m, m), dtype=bool))
    diff = np.abs(a[:, :m][low] - b[:, :m][low])
    print("EVID grid vs rows m %d d %d: largest difference %.3g in %d of %d" % (m, d, diff.max(), int((diff > 0).sum()), diff.size))
    assert not np.any(a[:, :m][low] == GUARD)
    assert np.array_equal(a[:, :m][low], b[:, :m][low])
    for got in (a, b):
        assert np.all(got[:, :m][~low] == GUARD) and np.all(got[:, m:] == GUARD)


@pytest.mark.parametrize("m,d,G", SHAPES)
def test_inverse_diagonals_of_a_batch_of_factors(dev, m, d, G):
    L, lib = _lib()
    X, _, cands = _case(m, d, G)
    refs = [_ref(m, d, g) for g in range(G)]
    lds = [m + g for g in range(G)]                        # their own pointers and leading dimensions
    mats = []
    for g in range(G):
        A = torch.full((m, lds[g]), float("nan"), dtype=torch.float64, device=dev)      # NaN wherever nothing may be read
        A[:, :m] = torch.from_numpy(np.tril(refs[g]["L"]) + np.triu(np.full((m, m), np.nan), 1)).to(dev)
        mats.append(A)
    ptrs = torch.tensor([A.data_ptr() for A in mats], dtype=torch.int64, device=dev)
    ldd = torch.tensor(lds, dtype=torch.int64, device=dev)
    ldo = m + 2
    out = torch.full((G, ldo), GUARD, dtype=torch.float64, device=dev)
    need = int(lib.ital_chol_inv_diag_batched_workspace(m, G))
    work = torch.empty(need, dtype=torch.float64, device=dev)
    L.check(lib.ital_chol_inv_diag_batched(ptrs.data_ptr(), ldd.data_ptr(), m, G, None, out.data_ptr(), ldo, work.data_ptr(),
                                           need, _stream()))
    oh = out.cpu().numpy()
    for g in range(G):
        _within(oh[g, :m], refs[g]["cdiag"], refs[g]["cond"], "inv_diag")
        assert np.all(oh[g, m:] == GUARD)


@pytest.mark.parametrize("m,d,G", SHAPES)
def test_evidence_end_to_end_equals_the_host(dev, m, d, G):
    X, y, cands = _case(m, d, G)
    r = _evidence(X, y, cands, dev, pad=2)
    assert r["status"] == 0 and not r["info"].any()
    sc, lm, lv = r["scores"].cpu().numpy(), r["loo_mean"].cpu().numpy(), r["loo_var"].cpu().numpy()
    for g in range(G):
        h = _ref(m, d, g)
        for j, name in enumerate(("lml", "loo_logp", "loo_mse")):
            _within(sc[g, j], h[name], h["cond"], name)
        _within(lm[g, :m], h["loo_mean"], h["cond"], "loo_mean")
        _within(lv[g, :m], h["loo_var"], h["cond"], "loo_var")
        assert np.all(lm[g, m:] == GUARD) and np.all(lv[g, m:] == GUARD)


# ------------------------------------------------------------------------------------------------ batch independence
def _same(a, g, b, h):
    return all(torch.equal(a[k][g], b[k][h]) for k in ("scores", "info", "loo_mean", "loo_var", "K"))


def test_a_candidate_gets_the_same_bits_alone_and_anywhere_in_a_batch(dev):
    rng = np.random.default_rng(5)
    m = 129
    X, y = rng.random((m, 10)), _labels(rng, m)
    seven = [(1.0, 1.0, 1e-6), (0.7, 1.3, 1e-4), (1.5, 0.8, 1e-3), (0.9, 1.1, 1e-5), (2.0, 1.0, 1e-2), (0.5, 2.0, 1e-6),
             (1.2, 0.5, 1e-4)]
    alone = _evidence(X, y, [seven[3]], dev)
    batch = _evidence(X, y, seven, dev)
    moved = _evidence(X, y, seven[4:] + seven[:4], dev)          # candidate 3 is now the last one
    assert _same(alone, 0, batch, 3) and _same(alone, 0, moved, 6)
    for g in range(7):
        assert _same(batch, g, moved, (g + 3) % 7)
    h = _host(X, y, *seven[3])
    _within(alone["scores"][0].cpu().numpy(), [h["lml"], h["loo_logp"], h["loo_mse"]], h["cond"], "scores")


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
    cands = [dict(length_scale=0.6 + 0.02 * g, var=1.0 + 0.01 * (g % 5), noise=10.0 ** -(2 + g % 5)) for g in range(70)]
    one = gp.evidence(cands)
    per = (1 << 30) // gp.evidence_chunk(1 << 30)
    small = 32 * per + per // 2
    assert gp.evidence_chunk(small) == 32 and gp.evidence_chunk() >= 70
    three = gp.evidence(cands, max_bytes=small)
    assert one["ok"].all()
    for k in one:
        assert np.array_equal(one[k], three[k]), k
    with pytest.raises(MemoryError):
        gp.evidence(cands, max_bytes=per // 2)
    with pytest.raises(ValueError):
        gp.evidence([dict(length_scale=0.0)])
    with pytest.raises(ValueError):
        gp.evidence([dict(length_scale=1.0, var=-1.0)])


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
    mixed = _evidence(X, y, [good[0], bad, good[1], good[2]], dev)
    clean = _evidence(X, y, good, dev)
    assert clean["status"] == 0 and mixed["status"] & 1
    assert mixed["info"].cpu().tolist() == [0, 2, 0, 0]
    sc = mixed["scores"][1].cpu().numpy()
    assert sc[0] == -np.inf and sc[1] == -np.inf and sc[2] == np.inf
    assert torch.isnan(mixed["loo_mean"][1]).all() and torch.isnan(mixed["loo_var"][1]).all()
    for g, h in ((0, 0), (2, 1), (3, 2)):
        assert _same(mixed, g, clean, h)

    # the inverse diagonals on their own: a flagged matrix is skipped and gets NaN
    L, lib = _lib()
    ptrs = torch.tensor([mixed["K"][g].data_ptr() for g in range(4)], dtype=torch.int64, device=dev)
    ldd = torch.full((4,), m, dtype=torch.int64, device=dev)
    out = torch.full((4, m), GUARD, dtype=torch.float64, device=dev)
    need = int(lib.ital_chol_inv_diag_batched_workspace(m, 4))
    work = torch.empty(need, dtype=torch.float64, device=dev)
    L.check(lib.ital_chol_inv_diag_batched(ptrs.data_ptr(), ldd.data_ptr(), m, 4, mixed["info"].data_ptr(), out.data_ptr(), m,
                                           work.data_ptr(), need, _stream()))
    assert torch.isnan(out[1]).all() and not torch.isnan(out[[0, 2, 3]]).any()
    assert torch.equal(1.0 / out[0], mixed["loo_var"][0])


def test_session_scores_warns_and_tune_params_refuses_when_nothing_is_positive_definite(dev):
    from ital_amd import ITAL, tune
    rng = np.random.default_rng(8)
    X = _twins(rng, 80, 10)
    A = ITAL(X, length_scale=1.0, var=1.0, noise=1e-3, device=dev)
    A.update({0: 1, 1: 1})                                   # the twins are labelled rows 0 and 1
    A.update({int(i): (1 if i % 3 else -1) for i in range(5, 25)})
    with pytest.warns(UserWarning, match="Matrix is not positive semi-definite."):
        got = tune.session_scores(A, [dict(noise=1e-3), dict(noise=0.0), dict(length_scale=0.7)], "loo_logp")
    assert got[1] == -np.inf and np.isfinite(got[0]) and np.isfinite(got[2])
    gp = A.gp
    before = [t.clone() for t in (gp.L, gp.alpha, gp.V, gp.mu, gp.s2)]
    rounds = A.rounds
    grid = OrderedDict((("noise", [0.0]), ("length_scale", [0.5, 1.0, 2.0])))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(np.linalg.LinAlgError):
            A.tune_params(grid=grid)
    assert all(torch.equal(a, b) for a, b in zip(before, (gp.L, gp.alpha, gp.V, gp.mu, gp.s2)))
    assert (A.length_scale, A.var, A.noise) == (1.0, 1.0, 1e-3) == (gp.length_scale, gp.var, gp.noise)
    assert A.rounds == rounds and int(gp.status.item()) == 0
    assert len(A.fetch_unlabelled(4)) == 4                   # the session goes on


# ------------------------------------------------------------------------------------------------ a real session
def _real_session(dev, call_evidence):
    from ital_amd import ITAL, mvn_stream
    rng = np.random.default_rng(9)
    X = rng.random((140, 10))
    Q = rng.random((2, 10))
    mvn_stream.GLOBAL.reset()
    np.random.seed(0)
    A = ITAL(X, queries=Q, length_scale=1.0, device=dev)
    truth = np.where(X[:, 0] + X[:, 1] > 1.0, 1, -1)
    for _ in range(3):
        A.update({int(i): int(truth[i]) for i in A.fetch_unlabelled(4)})
    A.revoke([A.gp.ind[4]])
    A.update({int(i): int(truth[i]) for i in A.fetch_unlabelled(4)})
    result = None
    if call_evidence:
        gp = A.gp
        before = [t.clone() for t in (gp.L, gp.alpha, gp.V, gp.mu, gp.s2, gp.status)]
        np_state, mvn_state = np.random.get_state(), (tuple(mvn_stream.GLOBAL.state), int(mvn_stream.GLOBAL.draws))
        last = A._last_batch
        cands = [dict(length_scale=1.0), dict(length_scale=0.8, var=1.2), dict(length_scale=1.3, noise=1e-4)]
        result = (cands, gp.evidence(cands))
        assert all(torch.equal(a, b) for a, b in zip(before, (gp.L, gp.alpha, gp.V, gp.mu, gp.s2, gp.status)))
        now = np.random.get_state()
        assert now[0] == np_state[0] and np.array_equal(now[1], np_state[1]) and now[2:] == np_state[2:]
        assert (tuple(mvn_stream.GLOBAL.state), int(mvn_stream.GLOBAL.draws)) == mvn_state
        assert A._last_batch is last
    return A, np.vstack((X, Q)), result, A.fetch_unlabelled(4)


def test_evidence_on_a_real_session_equals_the_host_and_leaves_the_session_alone(dev):
    A, rows, (cands, ev), picks = _real_session(dev, True)
    gp = A.gp
    assert gp.m == 2 + 15 and ev["ok"].all() and ev["loo_mean"].shape == (3, gp.m)
    for g, c in enumerate(cands):
        h = _host(rows[gp.ind], gp.y, c.get("length_scale", gp.length_scale), c.get("var", gp.var), c.get("noise", gp.noise))
        for name in ("lml", "loo_logp", "loo_mse", "loo_mean", "loo_var"):
            _within(ev[name][g], h[name], h["cond"], name)
    _, _, _, twin_picks = _real_session(dev, False)
    assert picks == twin_picks and len(set(picks)) == 4


def test_evidence_needs_a_fitted_model(dev):
    from ital_amd import GaussianProcess
    gp = GaussianProcess(np.random.default_rng(1).random((20, 4)), 0.5, device=dev)
    with pytest.raises(RuntimeError):
        gp.evidence([dict(length_scale=1.0)])


# ------------------------------------------------------------------------------------------------ tune_params end to end
TUNE_GRID = OrderedDict((("length_scale", [0.35, 0.5, 0.7, 1.0, 1.4, 2.0, 3.0, 5.0]),))


def _two_clusters():
    rng = np.random.default_rng(64)
    X = np.concatenate((rng.normal(0, 0.5, (150, 8)), rng.normal(0, 0.5, (150, 8)) + 0.35))
    truth = np.where(np.arange(300) < 150, 1, -1)
    ids = [int(i) for i in rng.choice(300, 36, replace=False)]
    return X, [{i: int(truth[i]) for i in ids[a:a + 12]} for a in range(0, 36, 12)]


def _tuned_session(cls, dev, **kw):
    from ital_amd import mvn_stream
    X, history = _two_clusters()
    mvn_stream.GLOBAL.reset()
    np.random.seed(1)
    A = cls(X, length_scale=0.5, var=1.0, noise=1e-2, device=dev, **kw)
    for g in history:
        A.update(g)
    return A, X, history


def _host_criterion(h, y, criterion):
    from sklearn.metrics import average_precision_score
    if criterion == "loo_ap":
        return float(average_precision_score(y > 0, h["loo_mean"]))
    return -h["loo_mse"] if criterion == "loo_mse" else h[criterion]


def _close(got, want, what, atol=APPEND_ATOL):
    err = float(np.max(np.abs(np.asarray(got) - np.asarray(want))))
    print("EVID %-22s err %.3g  bound %.3g" % (what, err, atol))
    assert err <= atol, (what, err)


@pytest.mark.parametrize("criterion", ["lml", "loo_logp", "loo_mse", "loo_ap"])
def test_tune_params_selects_the_hosts_best_and_applies_it(dev, criterion, capsys):
    from ital_amd import ITAL, mvn_stream, tune
    A, X, history = _tuned_session(ITAL, dev)
    gp = A.gp
    values = TUNE_GRID["length_scale"]
    host = [_host_criterion(_host(X[gp.ind], gp.y, ls, 1.0, 1e-2), gp.y, criterion) for ls in values]
    order = np.argsort(host)[::-1]
    margin = (host[order[0]] - host[order[1]]) / abs(host[order[0]])
    print("EVID %s host best %g margin %.3g" % (criterion, values[order[0]], margin))
    assert margin > 1e-6                                      # no tie decides what follows
    got = tune.session_scores(A, [dict(length_scale=ls) for ls in values], criterion)
    assert int(np.argmax(got)) == int(order[0])

    before = [t.clone() for t in (gp.L, gp.alpha, gp.V, gp.mu, gp.s2)]
    np_state, rounds = np.random.get_state(), A.rounds
    mvn_state = (tuple(mvn_stream.GLOBAL.state), int(mvn_stream.GLOBAL.draws))
    best, score = A.tune_params(grid=TUNE_GRID, criterion=criterion, apply=False)
    assert best == {"length_scale": values[order[0]]} and score == got[order[0]]
    shown = capsys.readouterr().out
    assert shown.count("length_scale = ") == 0                # verbose = 0 prints nothing
    assert all(torch.equal(a, b) for a, b in zip(before, (A.gp.L, A.gp.alpha, A.gp.V, A.gp.mu, A.gp.s2)))
    assert (A.length_scale, A.gp.length_scale) == (0.5, 0.5)

    best2, score2 = A.tune_params(grid=TUNE_GRID, criterion=criterion, verbose=1)
    assert (best2, score2) == (best, score)
    assert capsys.readouterr().out == "length_scale = {} : {:.4f}\n".format(best["length_scale"], score)
    assert (A.length_scale, A.var, A.noise) == (best["length_scale"], 1.0, 1e-2) == (gp.length_scale, gp.var, gp.noise)
    now = np.random.get_state()
    assert A.rounds == rounds and np.array_equal(now[1], np_state[1]) and now[2:] == np_state[2:]
    assert (tuple(mvn_stream.GLOBAL.state), int(mvn_stream.GLOBAL.draws)) == mvn_state
    B = ITAL(X, length_scale=best["length_scale"], var=1.0, noise=1e-2, device=dev)
    for g in history:
        B.update(g)
    _close(A.rel_mean, B.rel_mean, "rel_mean vs fresh")
    _close(A.gp.predict_stored(cov_mode="diag")[1], B.gp.predict_stored(cov_mode="diag")[1], "variance vs fresh")
    mvn_stream.GLOBAL.reset()
    pa = A.fetch_unlabelled(4)
    mvn_stream.GLOBAL.reset()
    pb = B.fetch_unlabelled(4)
    assert pa == pb and len(set(pa)) == 4
    shown += capsys.readouterr().out
    with capsys.disabled():
        sys.stdout.write(shown)                               # the figures, for a run with -s


def test_loo_ap_needs_both_signs(dev):
    from ital_amd import ITAL
    X, _ = _two_clusters()
    A = ITAL(X, length_scale=0.5, noise=1e-2, device=dev)
    A.update({3: 1, 10: 1, 40: 1})
    with pytest.raises(ValueError, match="both signs"):
        A.tune_params(grid=TUNE_GRID, criterion="loo_ap")
    assert A.length_scale == 0.5
    best, _ = A.tune_params(grid=TUNE_GRID, criterion="lml")             # the other criteria do not mind
    assert A.length_scale == best["length_scale"]


def test_tune_params_through_mcmi(dev):
    """The inherited method beyond ITAL: the same selection, and the learner goes on with the new parameters."""
    from ital_amd import MCMI_min
    A, X, history = _tuned_session(MCMI_min, dev, subsample=60)
    host = [_host(X[A.gp.ind], A.gp.y, ls, 1.0, 1e-2)["lml"] for ls in TUNE_GRID["length_scale"]]
    best, score = A.tune_params(grid=TUNE_GRID)
    assert best == {"length_scale": TUNE_GRID["length_scale"][int(np.argmax(host))]} and A.gp.length_scale == best["length_scale"]
    assert abs(score - max(host)) <= 2e-9 * max(1.0, abs(max(host)))
    B = MCMI_min(X, length_scale=best["length_scale"], var=1.0, noise=1e-2, device=dev, subsample=60)
    for g in history:
        B.update(g)
    _close(A.rel_mean, B.rel_mean, "rel_mean vs fresh")
    np.random.seed(4)
    pa = A.fetch_unlabelled(3)
    np.random.seed(4)
    pb = B.fetch_unlabelled(3)
    assert pa == pb and len(pb) == 3
