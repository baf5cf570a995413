"""The kernels of include/ital_usdm.h on the device against the model and the checkers of tests/_usdm_ref.py (where the bounds
are stated), and the USDM learner against the golden vectors of the real reference (tests/golden/make_golden_usdm.py).  Run on
the GPU box: python -m pytest tests -m gpu."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _usdm_ref as ref  # noqa: E402

GUARD = 64
ALL_FIXTURES = ref.FIXTURES + ("usdm_usps500_tol",)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


def _lib():
    from ital_amd import _lib as L
    return L.lib(), L.check


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded(object):
    """An n x m block with leading dimension ld between NaN guards, NaN in the padding; `a`: its initial values or None (NaN)."""

    def __init__(self, n, m, ld, dev, a=None):
        self.n, self.m, self.ld = n, m, ld
        host = np.full(2 * GUARD + n * ld, np.nan)
        if a is not None:
            host[GUARD:GUARD + n * ld].reshape(n, ld)[:, :m] = a
        self.before = host.copy()
        self.t = torch.from_numpy(host).to(dev)

    @property
    def ptr(self):
        return self.t.data_ptr() + 8 * GUARD

    def read(self, written=None):
        """The block now; asserts that every double outside it and outside `written` (a bool [n][m], default all) has its
        bits."""
        host = self.t.cpu().numpy()
        mask = np.zeros(len(host), dtype=bool)
        mask[GUARD:GUARD + self.n * self.ld].reshape(self.n, self.ld)[:, :self.m] = True if written is None else written
        assert np.array_equal(host.view(np.int64)[~mask], self.before.view(np.int64)[~mask]), "a byte outside the write set changed"
        return host[GUARD:GUARD + self.n * self.ld].reshape(self.n, self.ld)[:, :self.m].copy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.int64), np.ascontiguousarray(b, dtype=np.float64).view(np.int64))


# ----------------------------------------------------------------------------------------------------------- Laplacian
def _label_cases(n, rng):
    """(unlabelled u, relevant rows): a mixed case with unnameable rows, one with a single unlabelled row."""
    perm = rng.permutation(n)
    n_lab = max(1, n // 4)
    lab, unnameable = perm[:n_lab], perm[n_lab:n_lab + n // 8]
    yield np.setdiff1d(np.arange(n), np.concatenate([lab, unnameable])), lab[::2]
    yield perm[-1:], perm[:-1][::3]


@pytest.mark.parametrize("k", [1, 5, 32])
@pytest.mark.parametrize("n", [6, 17, 129, 300])
def test_laplacian_bits(dev, n, k):
    lib, check = _lib()
    rng = np.random.default_rng(100 * n + k)
    idx = ref.random_graph(n, k, rng)
    assert (idx == -1).any() == (n <= k)
    idx_d = torch.from_numpy(idx).to(dev)
    for u, relevant in _label_cases(n, rng):
        n_u = len(u)
        pos = np.full(n, -1, dtype=np.int64)
        pos[u] = np.arange(n_u)
        rel = np.zeros(n, dtype=np.uint8)
        rel[relevant] = 1
        M = Guarded(n_u, n_u, n_u + 3, dev)
        rhs = Guarded(1, n_u, n_u, dev)
        u_d, pos_d, rel_d = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (u.astype(np.int64), pos, rel))
        check(lib.ital_usdm_laplacian(idx_d.data_ptr(), k, n, u_d.data_ptr(), n_u, pos_d.data_ptr(), rel_d.data_ptr(),
                                      int(rel.sum()), ref.EPS, M.ptr, n_u + 3, rhs.ptr, _stream()))
        want_M, want_rhs = ref.model_laplacian(idx, k, n, u, pos, rel, int(rel.sum()))
        assert _same_bits(M.read(), want_M)
        assert _same_bits(rhs.read()[0], want_rhs)


# ------------------------------------------------------------------------------------------------------------------ LU
def _factor(dev, A, status0=0):
    lib, check = _lib()
    n = len(A)
    G = Guarded(n, n, n + 5, dev, A)
    flags = torch.tensor([-9, status0], dtype=torch.int32, device=dev)
    check(lib.ital_lu_factor(G.ptr, n, n + 5, flags[0:].data_ptr(), flags[1:].data_ptr(), _stream()))
    info, status = flags.cpu().tolist()
    return G, flags, info, status


def _laplacian_shaped(n, rng):
    k = min(5, max(1, n - 1))
    total = n + max(2, n // 5)                      # the labelled rows give the margin (total - n) eps
    idx = ref.random_graph(total, k, rng)
    u = np.arange(n)
    pos = np.full(total, -1, dtype=np.int64)
    pos[u] = u
    return ref.model_laplacian(idx, k, total, u, pos, np.zeros(total, dtype=np.uint8), 0)[0]


WORST = {}


@pytest.mark.parametrize("kind", ["laplacian", "dominant"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 200, 300, 517])
def test_lu_factor_and_solve_within_the_bounds(dev, n, kind):
    lib, check = _lib()
    rng = np.random.default_rng(7 * n + len(kind))
    A = _laplacian_shaped(n, rng) if kind == "laplacian" else ref.dominant_matrix(n, rng, 10.0 ** -rng.integers(1, 7) if n % 2 else 1e-6)
    G, flags, info, status = _factor(dev, A)
    LU = G.read()
    r_factor = ref.check_lu(A, LU, info, 0, status)
    b = rng.normal(size=n)
    y = Guarded(1, n, n, dev, b)
    check(lib.ital_lu_solve(G.ptr, n, n + 5, y.ptr, flags.data_ptr(), _stream()))
    r_solve = ref.check_lu_solve(A, LU, b, y.read()[0])
    assert _same_bits(G.read(), LU)                                   # the solve writes nothing but y
    WORST[(kind, n)] = (r_factor, r_solve)
    print("lu %-9s n = %3d: |A - LU| at %.3g of its bound, |b - Ax| at %.3g" % (kind, n, r_factor, r_solve))


def _zero_cross(A, j):
    A = A.copy()
    A[j, :] = 0.0
    A[:, j] = 0.0
    return A


def test_lu_failure_paths(dev):
    lib, check = _lib()
    rng = np.random.default_rng(5)
    base = ref.dominant_matrix(130, rng, 1e-2)
    nan = base.copy()
    nan[70, 70] = np.nan
    cases = [(_zero_cross(base, 0), 1, 0), (_zero_cross(base, 64), 65, 0), (_zero_cross(base, 129), 130, 2), (nan, 71, 0),
             (_zero_cross(base[:64, :64], 63), 64, 4)]
    for A, column, status0 in cases:
        G, flags, info, status = _factor(dev, A, status0)
        G.read()
        ref.check_lu(A, None, info, status0, status, expect_info=column)
        b = rng.normal(size=len(A))
        y = Guarded(1, len(A), len(A), dev, b)
        check(lib.ital_lu_solve(G.ptr, len(A), len(A) + 5, y.ptr, flags.data_ptr(), _stream()))
        assert _same_bits(y.read()[0], b)                              # skipped: y unchanged in bits
    G, flags, info, status = _factor(dev, base, 2)                     # a status word already set stays as it is
    ref.check_lu(base, G.read(), info, 2, status)


# ------------------------------------------------------------------------------------------------------ shift and symv
@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_shift_bits(dev, n):
    lib, check = _lib()
    rng = np.random.default_rng(n)
    K = rng.normal(size=(n, n))
    mu = 1e-6 * 1.1 ** 7
    Kd = Guarded(n, n, n + 2, dev, K)
    B = Guarded(n, n, n + 3, dev)
    check(lib.ital_usdm_shift(Kd.ptr, n, n + 2, mu, B.ptr, n + 3, _stream()))
    got = B.read(written=np.tril(np.ones((n, n), dtype=bool)))           # the strict upper triangle keeps its NaN guards
    assert _same_bits(got, ref.model_shift(K, mu))
    assert _same_bits(Kd.read(), K)


@pytest.mark.parametrize("n", [1, 64, 129, 300, 517])
def test_symv_lower(dev, n):
    lib, check = _lib()
    rng = np.random.default_rng(n)
    K = rng.normal(size=(n, n))
    K[np.triu_indices(n, 1)] = np.nan                                    # never read
    x = rng.normal(size=n)
    Kd, xd = Guarded(n, n, n + 1, dev, K), Guarded(1, n, n, dev, x)
    wl = int(lib.ital_symv_lower_workspace(n))
    outs = []
    for _ in range(2):
        out = Guarded(1, n, n, dev)
        work = torch.full((wl,), np.nan, dtype=torch.float64, device=dev)
        check(lib.ital_symv_lower(Kd.ptr, n, n + 1, xd.ptr, out.ptr, work.data_ptr(), wl, _stream()))
        outs.append(out.read()[0])
    assert _same_bits(outs[0], outs[1])
    print("symv n = %3d: %.3g of its bound" % (n, ref.check_symv(K, x, outs[0])))
    Kd.read()
    xd.read()


# ------------------------------------------------------------------------------------------------------ the learner
def _run(z, data, dev, rounds=None):
    from ital_amd import USDM
    L = USDM(data, **ref.options(z), device=dev)
    L.update({int(z["query"]): 1})
    lasts, picks = [], []
    for r in range(int(z["rounds"]) if rounds is None else rounds):
        picks.append(L.fetch_unlabelled(int(z["k"])))
        lasts.append(L.last)
        L.update(ref.feedback(z, r))
    return L, lasts, picks


@pytest.mark.parametrize("store", [False, True], ids=["numpy", "DeviceData"])
@pytest.mark.parametrize("name", ALL_FIXTURES)
def test_usdm_golden(dev, name, store):
    from ital_amd import DeviceData
    z = ref.load(name)
    X = z["X"]
    L, lasts, picks = _run(z, DeviceData(X, device=dev) if store else X, dev)
    nb = np.sort(L._graph().idx.cpu().numpy(), axis=1)
    assert np.array_equal(nb, z["r0_neighbours"])
    for r, (last, pick) in enumerate(zip(lasts, picks)):
        p = "r%d_" % r
        assert all(type(i) is int for i in pick)
        assert np.array_equal(last["candidates"], z[p + "u"])
        assert last["iterations"] == int(z[p + "iterations"]) == len(last["objectives"])
        for key, zkey, spread in (("prob", "prob", "spread_prob"), ("f", "f", "spread_f"), ("objectives", "objectives", "spread_obj")):
            err = float(np.max(np.abs(last[key] - z[p + zkey])))
            floor = 8 * ref.U * float(np.max(np.abs(z[p + zkey])))
            print("%s round %d %-10s: error %.3g = %.3g of 100 spread + floor" % (name, r, key, err, err / (100 * float(z[p + spread]) + floor)))
            assert err <= 100 * float(z[p + spread]) + floor, (r, key)
        assert set(pick) == set(z[p + "ret"].tolist())


def _state(z, rounds):
    """(relevant, irrelevant, unnameable) of the fixture after `rounds` rounds of feedback."""
    ids = ({int(z["query"])}, set(), set())
    for r in range(rounds):
        for i, v in ref.feedback(z, r).items():
            ids[0 if v > 0 else 1 if v < 0 else 2].add(i)
    return ids


def _fresh(z, X, ids, dev):
    from ital_amd import USDM
    L = USDM(X, **ref.options(z), device=dev)
    fb = {i: 1 for i in ids[0]}
    fb.update({i: -1 for i in ids[1]})
    fb.update({i: 0 for i in ids[2]})
    L.update(fb)
    return L


def test_live_session(dev):
    from ital_amd import USDM, DeviceData
    z = ref.load("usdm_synth150_knn3_r2")
    X, k = z["X"], int(z["k"])
    store = DeviceData(X[:140], device=dev)
    A = USDM(store, **ref.options(z), device=dev)
    B = USDM(store, **ref.options(z), device=dev)
    ids = _state(z, 1)
    ids = tuple({i for i in s if i < 140} for s in ids)
    for L in (A, B):
        L.update({**{i: 1 for i in ids[0]}, **{i: -1 for i in ids[1]}, **{i: 0 for i in ids[2]}})
    first = A.fetch_unlabelled(k)
    assert A._graph() is B._graph()                                       # one graph per store
    assert (A.knn, A.r, A.max_iter, A.tol) == (3, 2.0, 100, 1e-6)
    C = A.clone()
    assert (C.knn, C.r, C.max_iter, C.tol) == (A.knn, A.r, A.max_iter, A.tol)
    assert set(C.fetch_unlabelled(k)) == set(first) == set(_fresh(z, X[:140], ids, dev).fetch_unlabelled(k))
    A.add_data(X[140:])
    assert A.last is None
    assert set(A.fetch_unlabelled(k)) == set(_fresh(z, X, ids, dev).fetch_unlabelled(k))
    gone = [2, 77, 141]
    index_map = A.remove_data(gone)
    ids2 = tuple({int(index_map[i]) for i in s if index_map[i] >= 0} for s in ids)
    assert set(A.fetch_unlabelled(k)) == set(_fresh(z, np.delete(X, gone, axis=0), ids2, dev).fetch_unlabelled(k))
    N = USDM(X[:140], **ref.options(z), device=dev)                       # plain numpy data: the learner's own lists
    N.update({**{i: 1 for i in ids[0]}, **{i: -1 for i in ids[1]}, **{i: 0 for i in ids[2]}})
    assert set(N.fetch_unlabelled(k)) == set(first)
    lists = N._graph()
    assert N._graph() is lists
    N.set_params(length_scale=2.0)
    assert N._lists == {} and N.last is None


def test_device_side_refusals(dev):
    from ital_amd import USDM, DeviceData
    z = ref.load("usdm_synth150")
    X = z["X"]
    with pytest.raises(NotImplementedError, match="FP64 rows"):
        USDM(DeviceData(torch.from_numpy(X).to(torch.float32), device=dev, storage="source"), device=dev)
    with pytest.raises(NotImplementedError, match="row shards"):
        USDM(X, device=dev, world=2)
    with pytest.raises(NotImplementedError, match="queries"):
        USDM(X, queries=X[:1], device=dev)
    L = USDM(X[:20], length_scale=1.0, device=dev)
    with pytest.raises(RuntimeError, match="update"):
        L.fetch_unlabelled(4)
    L.update({0: 1, 1: 0})
    with pytest.raises(ValueError):
        L.fetch_unlabelled(19)                                            # 18 unlabelled rows
    assert len(L.fetch_unlabelled(18)) == 18
