"""ital_knn_rows on the device (include/ital_knn.h) against the extended-precision model of its DEFINITION and the checker of
tests/_knn_ref.py (where the bounds are derived) and the equalities it holds in bits; DeviceData.knn / neighbour_density and
their cache; SUD against the golden vectors of the real reference (tests/golden/make_golden_sud.py).  Run on the GPU box:
python -m pytest tests -m gpu."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _knn_ref as ref  # noqa: E402

NS = (1, 2, 17, 127, 128, 129, 300)
KS = (1, 2, 21, 32)
GUARD = 64
DTYPES = (torch.float64, torch.float32, torch.float16, torch.bfloat16)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


def _padded(rows, dev, dtype=torch.float64):
    """(padded device matrix of the rows, FP64 squared norms as ital_row_norms gives them on the widened rows)."""
    from ital_amd import _lib
    from ital_amd.gp import _pad16, _ptr, _stream
    n, d = rows.shape
    M = torch.zeros((n, _pad16(d)), dtype=torch.float64, device=dev)
    M[:, :d] = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float64)).to(dev)
    nrm = torch.empty(n, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().ital_row_norms(_ptr(M), n, M.shape[1], _ptr(nrm), _stream()))
    return M.to(dtype), nrm


class Out(object):
    """dist / idx / rowsum for nq rows between guard bytes."""

    def __init__(self, nq, k, dev):
        self.nq, self.k = nq, k
        self.d = torch.full((nq * k + 2 * GUARD,), -7.0, dtype=torch.float64, device=dev)
        self.i = torch.full((nq * k + 2 * GUARD,), -77, dtype=torch.int64, device=dev)
        self.s = torch.full((nq + 2 * GUARD,), -7.0, dtype=torch.float64, device=dev)

    @property
    def dist(self):
        return self.d[GUARD:GUARD + self.nq * self.k].view(self.nq, self.k)

    @property
    def idx(self):
        return self.i[GUARD:GUARD + self.nq * self.k].view(self.nq, self.k)

    @property
    def rowsum(self):
        return self.s[GUARD:GUARD + self.nq]

    def guards_untouched(self):
        for t, fill, m in ((self.d, -7.0, self.nq * self.k), (self.i, -77, self.nq * self.k), (self.s, -7.0, self.nq)):
            assert (t[:GUARD] == fill).all() and (t[GUARD + m:] == fill).all()


def _knn(X, xn, metric, k, skip_self, q=None, c=None, accumulate=0, splits=1, out=None, row0=0, rowsum=True):
    """One call of ital_knn_rows; `out` (an Out of at least row0 + nq rows) receives the query rows from its row `row0`."""
    from ital_amd import _lib
    from ital_amd.device_data import DTYPE_CODES
    from ital_amd.gp import _ptr, _stream
    n = X.shape[0]
    q, c = q or (0, n), c or (0, n)
    nq = q[1] - q[0]
    if out is None:
        out = Out(nq, k, X.device)
    lib = _lib.lib()
    need = lib.ital_knn_workspace(nq, k, splits)
    work = torch.full((need + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=X.device)
    _lib.check(lib.ital_knn_rows(_ptr(X), DTYPE_CODES[X.dtype], _ptr(xn), n, X.shape[1], q[0], q[1], c[0], c[1], metric, k, skip_self,
                                 accumulate, splits, out.dist[row0:].data_ptr(), out.idx[row0:].data_ptr(),
                                 out.rowsum[row0:].data_ptr() if rowsum else 0, work[GUARD:].data_ptr(), need, _stream()))
    out.guards_untouched()
    assert (work[:GUARD] == 0x5A).all() and (work[GUARD + need:] == 0x5A).all()
    return out


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same(a, b):
    return torch.equal(_bits(a.dist), _bits(b.dist)) and torch.equal(a.idx, b.idx) and torch.equal(_bits(a.rowsum), _bits(b.rowsum))


def _rows(n, d, seed):
    """Rows with exact duplicates (index ties), a zero row (NaN under the cosine) and a row scaled by 1e-200."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d))
    if n > 1:
        X[1] = 0.0
    if n > 11:
        X[7] = X[3]
        X[11] = X[3]
        X[9] = X[8] * 1e-200
    return X


def _sequential_sum(dist):
    s = np.zeros(len(dist))
    with np.errstate(invalid="ignore"):
        for slot in range(dist.shape[1]):
            s = s + dist[:, slot]
    return s


# ------------------------------------------------------------------------------------------------------ against the model
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d", [1, 5, 16, 20, 40])
def test_lists_against_the_model(dev, d, metric):
    """Every n of the tile boundaries, every k (k >= n: the +inf / -1 fill), skip_self 0 and 1 at this d (ldx 16, 32, 48: one,
    two and three LDS stages): (a) .. (e) of tests/_knn_ref.py, guard bytes, rowsum."""
    rows = _rows(max(NS), d, 200 + d)
    X, xn = _padded(rows, dev)
    xn_h = xn.cpu().numpy()
    if metric == 0:
        assert xn_h[1] == 0.0 and xn_h[9] == 0.0           # the scaled row's squared norm underflows: its dots do not
    pairs = ref.pair_model(rows, xn_h, metric, (0, max(NS)), (0, max(NS)))
    worst = 0.0
    for n in NS:
        for k in KS:
            for skip in (0, 1):
                out = _knn(X[:n], xn[:n], metric, k, skip, splits=0 if (n + k) % 2 else 1)
                idx, dist = out.idx.cpu().numpy(), out.dist.cpu().numpy()
                worst = max(worst, ref.check(idx, dist, rows[:n], xn_h[:n], metric, k, skip, pairs=pairs))
                np.testing.assert_array_equal(out.rowsum.cpu().numpy(), _sequential_sum(dist))
    print("d = %d, metric %d: largest error / bound = %.3f" % (d, metric, worst))


def test_ranges_and_empty_ranges(dev):
    rows = _rows(300, 20, 7)
    X, xn = _padded(rows, dev)
    xn_h = xn.cpu().numpy()
    out = _knn(X, xn, 0, 5, 1, q=(100, 231), c=(17, 290))
    ref.check(out.idx.cpu().numpy(), out.dist.cpu().numpy(), rows, xn_h, 0, 5, 1, q=(100, 231), c=(17, 290))
    empty = _knn(X, xn, 0, 5, 1, q=(100, 231), c=(40, 40))
    assert (empty.idx == -1).all() and torch.isposinf(empty.dist).all() and torch.isposinf(empty.rowsum).all()
    kept = _knn(X, xn, 0, 5, 1, q=(100, 231), c=(40, 40), accumulate=1, out=_knn(X, xn, 0, 5, 1, q=(100, 231), c=(17, 290)))
    assert _same(kept, out)
    none = _knn(X, xn, 0, 5, 1, q=(100, 100), c=(0, 300))          # an empty query range: nothing is written (the guards)
    assert none.dist.numel() == 0
    without = _knn(X, xn, 0, 5, 1, q=(100, 231), c=(17, 290), rowsum=False)
    assert torch.equal(_bits(without.dist), _bits(out.dist)) and (without.rowsum == -7.0).all()


# ------------------------------------------------------------------------------------------------------ equal bits
@pytest.mark.parametrize("metric", [0, 1])
def test_splits_cuts_and_ranges_change_no_bit(dev, metric):
    rows = _rows(300, 20, 11)
    X, xn = _padded(rows, dev)
    n, k = 300, 21
    for skip in (0, 1):
        want = _knn(X, xn, metric, k, skip, splits=1)
        for splits in (2, 3, 0):
            assert _same(_knn(X, xn, metric, k, skip, splits=splits), want), splits
        for cut in (64, 128, 129):
            out = _knn(X, xn, metric, k, skip, c=(0, cut), splits=2)
            out = _knn(X, xn, metric, k, skip, c=(cut, n), accumulate=1, out=out)
            assert _same(out, want), cut
        out = _knn(X, xn, metric, k, skip, c=(0, 130))
        out = _knn(X, xn, metric, k, skip, c=(100, n), accumulate=1, splits=3, out=out)     # rows 100 .. 129 come twice
        assert _same(out, want)
        out = Out(n, k, dev)
        _knn(X, xn, metric, k, skip, q=(0, 150), out=out)
        _knn(X, xn, metric, k, skip, q=(150, n), out=out, row0=150, splits=2)
        assert _same(out, want)


@pytest.mark.parametrize("n,d,k", [(17, 3, 2), (129, 17, 21), (300, 40, 32)])
def test_every_element_type_gives_the_fp64_bits(dev, n, d, k):
    rng = np.random.default_rng(n + d)
    rows = rng.integers(-16, 17, size=(n, d)) / 8.0          # exact in f16 and bf16
    rows[n // 2] = 0.0
    for metric in (0, 1):
        want = None
        for dtype in DTYPES:
            X, xn = _padded(rows, dev, dtype)
            assert X.dtype is dtype
            got = _knn(X, xn, metric, k, 1, splits=0)
            if want is None:
                want = got
                ref.check(got.idx.cpu().numpy(), got.dist.cpu().numpy(), rows, xn.cpu().numpy(), metric, k, 1)
            assert _same(got, want), dtype


@pytest.mark.parametrize("metric", [0, 1])
def test_distance_is_symmetric_in_bits(dev, metric):
    """All pairs of 33 rows with k = n - 1 = 32; all pairs of 129 rows (two tiles each way) from data ranges of 32 rows."""
    for n in (33, 129):
        rows = _rows(n, 20, 13)
        X, xn = _padded(rows, dev)
        D = np.zeros((n, n), dtype=np.int64)
        seen = np.zeros((n, n), dtype=bool)
        for c0 in range(0, n, 32 if n > 33 else n):
            out = _knn(X, xn, metric, 32, 1, c=(c0, min(n, c0 + (32 if n > 33 else n))))
            i, b = out.idx.cpu().numpy(), _bits(out.dist).cpu().numpy()
            for r in range(n):
                real = i[r] >= 0
                D[r, i[r][real]] = b[r][real]
                seen[r, i[r][real]] = True
        assert seen.sum() == n * (n - 1)
        assert np.array_equal(D, D.T)


# ------------------------------------------------------------------------------------------------------ the store
def test_store_lists_follow_append_and_remove(dev):
    from ital_amd import DeviceData
    rows = _rows(300, 20, 17)
    fresh = DeviceData(rows, device=dev)
    want_i, want_d = fresh.knn(5)
    want_dens = fresh.neighbour_density(20)
    X, xn = _padded(rows, dev)
    direct = _knn(X, xn, 0, 5, 1)
    assert torch.equal(want_i, direct.idx) and torch.equal(_bits(want_d), _bits(direct.dist))
    k21 = _knn(X, xn, 0, 21, 0)
    assert torch.equal(_bits(want_dens), _bits((k21.rowsum - 1.0) / 20.0))
    assert fresh.knn(5)[1].data_ptr() == want_d.data_ptr()                     # served from the cache
    for capacity in (300, None):                              # in place, and through a reallocation
        grown = DeviceData(rows[:263], device=dev, capacity=capacity)
        first = grown.knn(5)
        grown.knn(3, metric="sqeuclidean", skip_self=False)
        grown.neighbour_density(20)
        assert grown.append(rows[263:]) == 37
        kept = grown._knn[("cosine", 5, True)]
        assert kept.n == 263
        got_i, got_d = grown.knn(5)
        assert kept is grown._knn[("cosine", 5, True)] and kept.n == 300           # extended, not rebuilt
        assert torch.equal(got_i, want_i) and torch.equal(_bits(got_d), _bits(want_d))
        assert torch.equal(_bits(grown.neighbour_density(20)), _bits(want_dens))
        sq = _knn(X, xn, 1, 3, 0)
        got = grown.knn(3, metric="sqeuclidean", skip_self=False)
        assert torch.equal(got[0], sq.idx) and torch.equal(_bits(got[1]), _bits(sq.dist))
        assert first[0].shape == (263, 5)
    sel = grown.knn(5, rows=[299, 0, 4])
    assert torch.equal(sel[0], want_i[[299, 0, 4]]) and torch.equal(_bits(sel[1]), _bits(want_d[[299, 0, 4]]))
    rng_ = grown.knn(5, rows=range(10, 20))
    assert torch.equal(rng_[0], want_i[10:20])
    grown.remove([3, 10])
    assert grown._knn == {}
    after = DeviceData(np.delete(rows, [3, 10], axis=0), device=dev)
    assert torch.equal(grown.knn(5)[0], after.knn(5)[0]) and torch.equal(_bits(grown.knn(5)[1]), _bits(after.knn(5)[1]))
    for bad in (dict(k=0), dict(k=33), dict(k=5, metric="l1")):
        with pytest.raises(ValueError):
            fresh.knn(**bad)
    with pytest.raises(ValueError):
        fresh.neighbour_density(32)
    with pytest.raises(ValueError):
        DeviceData(rows[:10], device=dev).neighbour_density(10)


# ------------------------------------------------------------------------------------------------------ SUD
def _params(z):
    return dict(length_scale=float(z["length_scale"]), var=float(z["var"]), noise=float(z["noise"]), K=int(z["K"]))


def _run_sud(z, data, n_cols, check=True, **placement):
    from ital_amd import SUD
    L = SUD(data, **_params(z), **placement)
    L.update({int(z["query"]): 1})
    k, K, picks = int(z["k"]), int(z["K"]), []
    ldx = (n_cols + 15) // 16 * 16
    for r in range(int(z["rounds"])):
        p = "r%d_" % r
        ret = L.fetch_unlabelled(k)
        picks.append(ret)
        assert ret == z[p + "ret"].tolist() and all(type(i) is int for i in ret)
        if check:
            assert np.array_equal(L.last["candidates"], z[p + "cand"])
            bound = ref.density_bound(K, ldx, z[p + "dens"]) + ref.density_bound(K, n_cols, z[p + "dens"])   # ours plus scipy's
            err = np.abs(L.last["densities"] - z[p + "dens"])
            print("round %d: densities differ from the reference's by %.3g (bound %.3g)" % (r, err.max(), bound.min()))
            assert (err <= bound).all()
            np.testing.assert_allclose(L.last["unc"], z[p + "unc"], rtol=0, atol=1e-12)
            np.testing.assert_allclose(L.last["scores"], z[p + "scores"], rtol=0, atol=1e-12)
        L.update({int(i): float(z["rel"][i]) for i in ret})
    if check:
        np.testing.assert_allclose(L.rel_mean, z["final_rel_mean"], rtol=0, atol=1e-10)
    return L, picks


@pytest.mark.parametrize("name", ref.SUD_FIXTURES)
def test_sud_golden(dev, name):
    from ital_amd import DeviceData
    z, X = ref.load(name)
    K = int(z["K"])
    L, _ = _run_sud(z, X, X.shape[1], device=dev)
    S, _ = _run_sud(z, DeviceData(X, device=dev), X.shape[1], device=dev)
    assert S.gp.store is not None and L.gp.store is None
    for learner in (L, S):                                  # every density of the data set against the model, not the candidates' alone
        model = ref.model_density(X, learner.gp.xnorm.cpu().numpy(), K)
        err = np.abs(learner._densities()[1] - model).astype(np.float64)
        assert (err <= ref.density_bound(K, learner.gp.ldx, model.astype(np.float64))).all()


def test_sud_stores_share_and_stay_behind(dev):
    """An f32 compact store gives the reference's picks and the bits of the FP64 store of the same values; two learners on
    a store share one density vector; a learner that has not called sync_data() gets the densities of the rows it knows."""
    from ital_amd import SUD, DeviceData
    z, X = ref.load("sud_synth150")
    t32 = torch.from_numpy(X).to(torch.float32)
    compact = DeviceData(t32, device=dev, storage="source")
    assert compact.X.dtype is torch.float32
    wide = DeviceData(t32.to(torch.float64), device=dev)
    A, pa = _run_sud(z, compact, X.shape[1], check=False, device=dev)
    B, pb = _run_sud(z, wide, X.shape[1], check=False, device=dev)
    assert pa == pb and A.gp.xtype == 1 and B.gp.xtype == 0
    assert torch.equal(_bits(A._densities()[0]), _bits(B._densities()[0]))
    C, _ = _run_sud(z, wide, X.shape[1], check=False, device=dev)
    assert C._densities()[0] is B._densities()[0] and len(wide._knn) == 1
    before = B._densities()[0].clone()
    wide.append(X[:5] * 1.01)
    assert torch.equal(_bits(B._densities()[0]), _bits(before)) and B._densities()[0].shape == (150,)
    assert wide.neighbour_density(20).shape == (155,)
    assert torch.equal(_bits(B._densities()[0]), _bits(before))                  # rebuilt for its 150 rows, never longer
    B.sync_data()
    assert torch.equal(_bits(B._densities()[0]), _bits(DeviceData(wide.rows(), device=dev).neighbour_density(20)))
    with pytest.raises(RuntimeError):
        SUD(X, **_params(z), device=dev).fetch_unlabelled(4)                      # nothing fitted
    with pytest.raises(ValueError):
        L = SUD(X[:15], **_params(z), device=dev)
        L.update({0: 1})
        L.fetch_unlabelled(2)                                                     # K + 1 = 21 neighbours of 15 rows
