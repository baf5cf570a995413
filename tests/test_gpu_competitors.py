"""TCAL and RBMAL on the device (ital_amd/competitors.py): ital_cosine_min against the extended-precision model of its
DEFINITION (tests/_competitors_ref.py, where the bound is derived) and the equalities it holds in bits; the two learners
against the golden vectors of the real reference (tests/golden/make_golden_competitors.py), on the stores and on two ranks;
the harness tables.  Run on the GPU box: python -m pytest tests -m gpu."""
import io
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _competitors_ref as ref  # noqa: E402
import _ranks  # noqa: E402

NS = (1, 15, 16, 17, 63, 64, 65, 257)
CS = (1, 15, 16, 17, 63, 64, 65, 130)
DTYPES = (torch.float64, torch.float32, torch.float16, torch.bfloat16)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


def _padded(rows, dev, dtype=torch.float64, extra=0, fill=0.0):
    """(padded device matrix of len(rows) + extra rows, the extra ones filled with `fill`; FP64 squared norms of all rows as
    ital_row_norms gives them on the widened rows)."""
    from ital_amd import _lib
    from ital_amd.gp import _pad16, _ptr, _stream
    n, d = rows.shape
    ldx = _pad16(d)
    M = torch.full((n + extra, ldx), fill, dtype=torch.float64, device=dev)
    M[:n] = 0.0
    M[:n, :d] = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float64)).to(dev)
    nrm = torch.full((n + extra,), fill, dtype=torch.float64, device=dev)
    if n:
        _lib.check(_lib.lib().ital_row_norms(_ptr(M), n, ldx, _ptr(nrm), _stream()))
    return M.to(dtype), nrm


def _cosine(X, xn, n, T, tn, c, accumulate=0, out=None):
    from ital_amd import _lib
    from ital_amd.device_data import DTYPE_CODES
    from ital_amd.gp import _ptr, _stream
    if out is None:
        out = torch.full((n + 3,), 7.0, dtype=torch.float64, device=X.device)
    _lib.check(_lib.lib().ital_cosine_min(_ptr(X), DTYPE_CODES[X.dtype], _ptr(xn), n, X.shape[1], _ptr(T), _ptr(tn), c,
                                          accumulate, _ptr(out), _stream()))
    return out


def _bits(t):
    return t.contiguous().view(torch.int64)


# ------------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("d", [1, 3, 16, 17, 40])
def test_cosine_min_against_the_model(dev, d):
    """Every n x c of the tile, block and pass boundaries at this d (ldx 16, 32, 48): NaN positions equal, values within
    (2 ldx + 10) 2^-53 of the np.longdouble model (the bound is derived in tests/_competitors_ref.py, not tuned); rows >= n of
    `out` keep their bits and NaN-poisoned rows >= c of T play no part."""
    rng = np.random.default_rng(100 + d)
    ldx = (d + 15) // 16 * 16
    rows = rng.normal(size=(max(NS), d))
    rows[3] = 0.0                                          # a zero row: NaN (n > 3)
    train = rng.normal(size=(max(CS), d))
    rows[5] = train[0] * 1.5                               # a multiple of a train row: distance 0 up to rounding (n > 5)
    worst = 0.0
    for c in CS:
        T, tn = _padded(train[:c], dev, extra=3, fill=float("nan"))
        for n in NS:
            X, xn = _padded(rows[:n], dev)
            out = _cosine(X, xn, n, T, tn, c)
            got = out.cpu().numpy()
            assert (got[n:] == 7.0).all()
            worst = max(worst, ref.check(got[:n], rows[:n], xn[:n].cpu().numpy(), train[:c], tn[:c].cpu().numpy(), ldx))
    print("d = %d: largest error / bound = %.3f" % (d, worst))


def _f16_values(rng, shape):
    return rng.integers(-16, 17, size=shape) / 8.0          # exact in f16 and bf16; every dot product is exact in FP64


@pytest.mark.parametrize("n,d,c", [(16, 3, 1), (65, 17, 17), (257, 40, 130)])
def test_every_element_type_gives_the_fp64_bits(dev, n, d, c):
    rng = np.random.default_rng(n + c)
    rows, train = _f16_values(rng, (n, d)), _f16_values(rng, (c, d))
    rows[n // 2] = 0.0
    T, tn = _padded(train, dev)
    want = None
    for dtype in DTYPES:
        X, xn = _padded(rows, dev, dtype)
        assert X.dtype is dtype
        got = _cosine(X, xn, n, T, tn, c)
        if want is None:
            want = got
            ref.check(got[:n].cpu().numpy(), rows, xn.cpu().numpy(), train, tn.cpu().numpy(), X.shape[1])
            assert torch.isnan(got[n // 2])
        assert torch.equal(_bits(got), _bits(want)), dtype


def test_order_of_train_rows_calls_and_position_change_no_bit(dev):
    """A permutation of T, T cut into two calls at 1, 16 or 64 (the second accumulating), and a row computed alone or
    inside a larger call: the same bits."""
    rng = np.random.default_rng(77)
    n, d, c = 257, 40, 130
    rows, train = rng.normal(size=(n, d)), rng.normal(size=(c, d))
    rows[9] = 0.0
    X, xn = _padded(rows, dev)
    T, tn = _padded(train, dev)
    want = _cosine(X, xn, n, T, tn, c)
    perm = torch.from_numpy(rng.permutation(c)).to(dev)
    assert torch.equal(_bits(_cosine(X, xn, n, T[perm].contiguous(), tn[perm].contiguous(), c)), _bits(want))
    for cut in (1, 16, 64):
        out = _cosine(X, xn, n, T, tn, cut)
        out = _cosine(X, xn, n, T[cut:], tn[cut:], c - cut, accumulate=1, out=out)
        assert torch.equal(_bits(out), _bits(want)), cut
    for i in (0, 9, 63, 64, 200, 256):
        alone = _cosine(X[i:i + 1], xn[i:i + 1], 1, T, tn, c)
        assert torch.equal(_bits(alone[:1]), _bits(want[i:i + 1])), i
    part = _cosine(X[64:], xn[64:], 100, T, tn, c)
    assert torch.equal(_bits(part[:100]), _bits(want[64:164]))
    # accumulate keeps a NaN that is already there and a smaller value
    prev = torch.full((n + 3,), 7.0, dtype=torch.float64, device=dev)
    prev[:n] = want[:n]
    prev[4], prev[6] = float("nan"), -1.0
    acc = _cosine(X, xn, n, T, tn, c, accumulate=1, out=prev.clone())
    assert torch.isnan(acc[4]) and acc[6] == -1.0
    keep = torch.ones(n + 3, dtype=torch.bool, device=dev)
    keep[4] = keep[6] = False
    assert torch.equal(_bits(acc[keep]), _bits(prev[keep]))


# ------------------------------------------------------------------------------------------------------ learners
def _params(z):
    kw = dict(length_scale=float(z["length_scale"]), var=float(z["var"]), noise=float(z["noise"]))
    if "kw_unc_factor" in z.files:
        kw["unc_factor"] = int(z["kw_unc_factor"])
    return kw


def _run_rbmal(z, data, n_cols, check=True, **placement):
    from ital_amd import RBMAL
    L = RBMAL(data, **_params(z), **placement)
    L.update({int(z["query"]): 1})
    k, picks = int(z["k"]), []
    ldx = (n_cols + 15) // 16 * 16
    for r in range(int(z["rounds"])):
        p = "r%d_" % r
        ret = L.fetch_unlabelled(k)
        picks.append(ret)
        if check:
            cand = z[p + "cand"]
            assert ret == z[p + "ret"].tolist() and all(type(i) is int for i in ret)
            assert np.array_equal(L.last["candidates"], cand) and sorted(L.last["train"]) == sorted(z[p + "train"].tolist())
            assert L.last["folded"] == (1 if r == 0 else k - 1)          # only the rows labelled since the last fetch
            err = np.abs(L.last["dist"] - z[p + "dist"][cand]).max()
            print("round %d: dist differs from scipy's by %.3g (bound %.3g)" % (r, err, ref.bound(ldx) + ref.bound(n_cols)))
            assert err <= ref.bound(ldx) + ref.bound(n_cols)              # the device's bound plus scipy's
            np.testing.assert_allclose(L.last["unc"], z[p + "unc"][cand], rtol=0, atol=1e-12)
            assert L.last["alpha"] == z[p + "alpha"][0]
            np.testing.assert_allclose(L.last["scores"], z[p + "s0_scores"], rtol=0, atol=1e-12)
        L.update({int(i): float(z["rel"][i]) for i in ret})
    if check:
        np.testing.assert_allclose(L.rel_mean, z["final_rel_mean"], rtol=0, atol=1e-10)
    return L, picks


def _run_tcal(z, data, check=True, **placement):
    from ital_amd import TCAL
    np.random.seed(0)
    L = TCAL(data, **_params(z), **placement)
    L.update({int(z["query"]): 1})
    k, picks = int(z["k"]), []
    for r in range(int(z["rounds"])):
        p = "r%d_" % r
        ret = L.fetch_unlabelled(k)
        picks.append(ret)
        if check:
            assert ret == z[p + "ret"].tolist() and all(type(i) is int for i in ret)
            assert np.array_equal(L.last["unc"], z[p + "unc"])
            assert np.array_equal(L.last["K"], L.last["K"].T)
            np.testing.assert_allclose(L.last["K"], z[p + "K"], rtol=0, atol=1e-12)
            assert np.array_equal(L.last["labels"], z[p + "labels"]) and L.last["clusterings"] == int(z[p + "clusterings"])
            for i, dens in enumerate(L.last["densities"]):
                np.testing.assert_allclose(dens, z[p + "dens%d" % i], rtol=0, atol=1e-11)
            assert ref.same_rng_state(z, p + "rng_after")
        L.update({int(i): float(z["rel"][i]) for i in ret})
    if check:
        np.testing.assert_allclose(L.rel_mean, z["final_rel_mean"], rtol=0, atol=1e-10)
    return L, picks


@pytest.mark.parametrize("name", ref.RBMAL_FIXTURES)
def test_rbmal_golden(dev, name):
    z, X = ref.load(name)
    _run_rbmal(z, X, X.shape[1], device=dev)


@pytest.mark.parametrize("name", ref.TCAL_FIXTURES)
def test_tcal_golden(dev, name):
    z, X = ref.load(name)
    saved = np.random.get_state()
    try:
        _run_tcal(z, X, device=dev)
    finally:
        np.random.set_state(saved)


def test_learner_errors_and_short_requests(dev):
    from ital_amd import RBMAL, TCAL
    z, X = ref.load("rbmal_synth150")
    for cls in (RBMAL, TCAL):
        L = cls(X, **_params(z), device=dev)
        with pytest.raises(RuntimeError):
            L.fetch_unlabelled(3)                                      # nothing fitted
    q = X[7] * 0.9
    R = RBMAL(X, [q], **_params(z), device=dev)
    assert R.fetch_unlabelled(1) == [] and R.fetch_unlabelled(0) == []
    with pytest.raises(ValueError):
        R.fetch_unlabelled(3)                                          # fitted by a query only: no labelled data sample
    R.update({4: 1})
    assert len(R.fetch_unlabelled(4)) == 3 and R.last["train"] == [4]  # the query is not a train sample
    T = TCAL(X, [q], **_params(z), device=dev)
    assert T.fetch_unlabelled(0) == [] and T.fetch_unlabelled(-2) == []
    with pytest.raises(ValueError):
        T.fetch_unlabelled(40)                                         # m = 160 > 150 candidates: numpy's own error


def test_rbmal_kept_distances_equal_a_fresh_learners_in_bits(dev):
    from ital_amd import RBMAL
    z, X = ref.load("rbmal_synth150")
    L, picks = _run_rbmal(z, X, X.shape[1], check=False, device=dev)
    labels = {int(z["query"]): 1}
    for ret in picks:
        labels.update({int(i): float(z["rel"][i]) for i in ret})

    def fresh(lab):
        F = RBMAL(X, **_params(z), device=dev)
        F.update(lab)
        F.fetch_unlabelled(2)
        assert F.last["folded"] == len(lab)
        return F

    L.fetch_unlabelled(2)
    assert L.last["folded"] == int(z["k"]) - 1                         # folded round by round, never rebuilt
    assert torch.equal(_bits(L._dist[2]), _bits(fresh(labels)._dist[2]))
    gone = picks[1][0]
    L.revoke([gone])
    del labels[gone]
    L.fetch_unlabelled(2)
    assert L.last["folded"] == len(labels)                             # not a suffix of the kept list: built again
    assert torch.equal(_bits(L._dist[2]), _bits(fresh(labels)._dist[2]))
    L.reset()
    L.update({3: 1})
    L.fetch_unlabelled(2)
    assert L.last["folded"] == 1 and L.last["train"] == [3]


def test_stores(dev):
    """The same picks on a DeviceData; on an f32 compact store the bits of the FP64 store of the f32-rounded rows."""
    from ital_amd import DeviceData
    z, X = ref.load("rbmal_synth150")
    _run_rbmal(z, DeviceData(X, device=dev), X.shape[1], device=dev)
    zt, Xt = ref.load("tcal_synth150")
    saved = np.random.get_state()
    try:
        _run_tcal(zt, DeviceData(Xt, device=dev), device=dev)
        t32 = torch.from_numpy(X).to(torch.float32)
        compact = DeviceData(t32, device=dev, storage="source")
        assert compact.X.dtype is torch.float32
        wide = DeviceData(t32.to(torch.float64), device=dev)
        A, pa = _run_rbmal(z, compact, X.shape[1], check=False, device=dev)
        B, pb = _run_rbmal(z, wide, X.shape[1], check=False, device=dev)
        assert pa == pb and A.gp.xtype == 1 and B.gp.xtype == 0
        assert torch.equal(_bits(A._dist[2]), _bits(B._dist[2]))
        _, ta = _run_tcal(zt, DeviceData(torch.from_numpy(Xt).to(torch.float32), device=dev, storage="source"), check=False,
                          device=dev)
        _, tb = _run_tcal(zt, DeviceData(torch.from_numpy(Xt).to(torch.float32).to(torch.float64), device=dev), check=False,
                          device=dev)
        assert ta == tb
    finally:
        np.random.set_state(saved)


def _rank_worker(rank, world, port, mode, out):
    dev, group = _ranks.join(rank, world, port, mode)
    try:
        z, X = ref.load("rbmal_synth150")
        L, rb = _run_rbmal(z, X, X.shape[1], check=False, device=dev, rank=rank, world=world, group=group)
        assert L.gp.collective
        z, X = ref.load("tcal_synth150")
        _, tc = _run_tcal(z, X, check=False, device=dev, rank=rank, world=world, group=group)
        out[rank] = (rb, tc)
    finally:
        _ranks.leave(group)


def test_two_ranks_return_the_one_rank_lists(dev):
    want = tuple([ref.load(name)[0]["r%d_ret" % r].tolist() for r in range(3)] for name in ("rbmal_synth150", "tcal_synth150"))
    res = _ranks.spawn(_rank_worker, 2, "gloo")
    assert res[0] == want and res[1] == want


# ------------------------------------------------------------------------------------------------------ harness
@pytest.mark.parametrize("name", ["harness_tcal", "harness_rbmal"])
def test_harness_tables(dev, name):
    """The reference's printed AP / NDCG table, every fetched batch and every simulated feedback, in order."""
    from ital_amd import harness
    with open(os.path.join(ref.GOLD, name + ".json")) as fh:
        g = json.load(fh)
    cfg = harness.read_config_file(os.path.join(ref.GOLD, "conf", name + ".conf"), "EXPERIMENT", {})
    kw = dict(cfg["Stored"])
    kw["data_file"] = os.path.join(ref.GOLD, kw["data_file"])
    ds = harness.load_dataset("Stored", **kw)
    assert len(ds.X_train_norm) == g["n_train"]
    assert all(gap >= ref.MARGIN for gap in g["smallest_margins"].values())
    method = cfg["EXPERIMENT"]["method"]
    lkw = dict(cfg["METHOD_DEFAULTS"])
    if method in cfg:
        lkw.update(cfg[method])
    learner = harness.make_learner(method, ds.X_train_norm, lkw, device=dev)
    trace, buf = [], io.StringIO()
    saved = np.random.get_state()
    try:
        harness.run_retrieval_experiment(cfg, ds, learner, out=buf, trace=trace)
    finally:
        np.random.set_state(saved)
    assert [t[3] for t in trace] == [t["ret"] for t in g["trace"]]
    assert [t[4] for t in trace] == [t["fb"] for t in g["trace"]]
    assert buf.getvalue() == g["table"]


def test_cli_runs_a_competitor(dev, capsys):
    from ital_amd import harness
    saved = np.random.get_state()
    try:
        harness.main([os.path.join(ref.GOLD, "conf", "harness_border.conf"), "--method=TCAL", "--rounds=1", "--repetitions=1"])
    finally:
        np.random.set_state(saved)
    out = capsys.readouterr().out.strip().splitlines()
    assert out[0] == "Round;Median_AP;Mean_AP;AP_SD;Median_NDCG;Mean_NDCG;NDCG_SD" and len(out) == 3
