"""DeviceData on the device: ital_ingest_rows (csrc/ingest.hip) against the same conversion written with tensor operations and
ital_row_norms, and what is built on it -- learners on a shared store, sync_data, clone, predict on a tensor.

The conversion to FP64 is exact for f16 / bf16 / f32 / f64 and the norms are ital_row_norms' own, so a learner on a store holds
the bits a learner built from the equivalent float64 numpy array holds: every comparison below is torch.equal / == unless it
says otherwise (a clone against a REPLAYED history: 2e-9, the bound tests/test_gpu_rewhiten.py uses against a rebuilt learner).
Run: python -m pytest tests -m gpu."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden  # noqa: E402  (fixture table only)

APPEND_ATOL = 2e-9


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


def _pad16(v):
    return (v + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------ the kernel
DTYPES = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
NS = (1, 63, 64, 65, 257)
DS = (1, 15, 16, 17, 130)


def _values(n, d, dtype, seed):
    """n x d host values of `dtype`, among them -0.0, the type's smallest subnormal and its largest finite value."""
    g = torch.Generator().manual_seed(seed)
    v = (torch.randn((n, d), generator=g, dtype=torch.float64) * 3).to(dtype)
    flat = v.view(-1)
    info = torch.finfo(dtype)
    specials = [-0.0, 0.0, 1.0]
    for at, s in enumerate(specials):
        if at < flat.numel():
            flat[at] = s
    if flat.numel() > 5:          # the smallest subnormal and the largest magnitude
        flat[3] = torch.tensor(info.smallest_normal, dtype=dtype) * torch.tensor(info.eps, dtype=dtype)
        flat[4] = -info.max if dtype is not torch.float64 else -1e150        # its square is finite in FP64
        assert flat[3] != 0
    return v


def _source(layout, vals, dev):
    """The values as a device tensor view of the asked layout; returns (view, element stride of its rows)."""
    n, d = vals.shape
    es = vals.element_size()
    if layout == "contiguous":
        t = vals.to(dev)
        return t, d
    if layout == "row_strided":
        buf = torch.zeros((n, d + 5), dtype=vals.dtype, device=dev)
        buf[:, :d] = vals.to(dev)
        return buf[:, :d], d + 5
    if layout == "offset_one":            # one element into an allocation: never on a 16-B boundary -> the element-wise loads
        buf = torch.zeros(n * d + 1, dtype=vals.dtype, device=dev)
        t = buf[1:].view(n, d)
        t.copy_(vals.to(dev))
        assert t.data_ptr() % 16 != 0 and t.data_ptr() % es == 0
        return t, d
    if layout == "aligned16":             # pointer and row stride multiples of 16 B -> the wide loads
        ld = _pad16(d) + 16
        buf = torch.zeros((n, ld), dtype=vals.dtype, device=dev)
        buf[:, :d] = vals.to(dev)
        assert buf.data_ptr() % 16 == 0 and (ld * es) % 16 == 0
        return buf[:, :d], ld
    raise AssertionError(layout)


@pytest.mark.parametrize("layout", ["contiguous", "row_strided", "offset_one", "aligned16"])
@pytest.mark.parametrize("name", list(DTYPES))
def test_ingest_rows_equals_conversion_and_row_norms(dev, name, layout):
    from ital_amd import _lib
    from ital_amd.gp import _stream
    lib, dtype = _lib.lib(), DTYPES[name]
    code = {"f64": 0, "f32": 1, "f16": 2, "bf16": 3}[name]
    nan = float("nan")
    for n in NS:
        for d in DS:
            vals = _values(n, d, dtype, 1000 * n + d)
            src, ld = _source(layout, vals, dev)
            ldx = _pad16(d)
            X = torch.full((n + 3, ldx), nan, dtype=torch.float64, device=dev)
            xnorm = torch.full((n + 3,), nan, dtype=torch.float64, device=dev)
            _lib.check(lib.ital_ingest_rows(src.data_ptr(), code, n, d, ld, X.data_ptr(), ldx, xnorm.data_ptr(), _stream()))
            want = vals.to(torch.float64).to(dev)          # exact, converted on the host
            what = (name, layout, n, d)
            assert torch.equal(X[:n, :d], want), what
            assert torch.equal(X[:n, :d].contiguous().view(torch.int64), want.view(torch.int64)), what     # also the sign of -0.0
            assert bool((X[:n, d:].contiguous().view(torch.int64) == 0).all()), what        # pad columns: +0.0
            assert bool(torch.isnan(X[n:]).all()) and bool(torch.isnan(xnorm[n:]).all()), what   # rows >= n: not touched
            norms = torch.full((n + 3,), nan, dtype=torch.float64, device=dev)
            _lib.check(lib.ital_row_norms(X.data_ptr(), n, ldx, norms.data_ptr(), _stream()))
            assert torch.equal(xnorm[:n], norms[:n]), what
            assert bool(torch.isfinite(xnorm[:n]).all()), what


def test_device_data_input_kinds_chunks_and_no_alias(dev):
    from ital_amd import DeviceData
    rng = np.random.default_rng(3)
    A = rng.standard_normal((257, 140)).astype(np.float32)
    want = torch.from_numpy(A.astype(np.float64)).to(dev)
    one = DeviceData(A, device=dev)
    assert (one.n, one.d, one.ldx, one.shape, one.ndim, len(one), np.shape(one)) == (257, 140, 144, (257, 140), 2, 257, (257, 140))
    assert one.X.shape == (257, 144) and one.xnorm.shape == (257,) and one.device == torch.device(dev) and one.capacity == 257
    assert torch.equal(one.X[:, :140], want) and bool((one.X[:, 140:] == 0).all())
    pieces = DeviceData(A, device=dev, chunk_bytes=3000)          # 5 rows per upload
    assert torch.equal(pieces.X, one.X) and torch.equal(pieces.xnorm, one.xnorm)
    T = torch.from_numpy(A)
    for src in (T.to(dev), T, T.to(dev).to(torch.float64), A.astype(np.float64)):
        s = DeviceData(src, device=dev)
        assert torch.equal(s.X, one.X) and torch.equal(s.xnorm, one.xnorm)
    for view in (T[:, 3:131], T.to(dev)[:, 3:131], A[:, 3:131], T.to(dev).t().contiguous().t()[:, 3:131]):
        s = DeviceData(view, device=dev)
        assert s.shape == (257, 128) and torch.equal(s.X, want[:, 3:131])
    for dt in (torch.float16, torch.bfloat16):
        s = DeviceData(T.to(dt), device=dev, chunk_bytes=1 << 12)
        assert torch.equal(s.X[:, :140], T.to(dt).to(torch.float64).to(dev))
    assert torch.equal(DeviceData(A.astype(np.float16), device=dev).X[:, :140], torch.from_numpy(A.astype(np.float16).astype(np.float64)).to(dev))
    ints = np.arange(12, dtype=np.int32).reshape(3, 4)
    assert np.array_equal(DeviceData(ints, device=dev).rows(), ints.astype(np.float64))
    # the source is not aliased: overwriting it afterwards changes nothing
    D = T.to(dev).to(torch.float64)
    s = DeviceData(D, device=dev)
    D.fill_(7.0)
    torch.cuda.synchronize()
    assert torch.equal(s.X, one.X)
    assert np.array_equal(s.rows(), A.astype(np.float64)) and np.array_equal(s.rows([5, 0, 256, -1]), A.astype(np.float64)[[5, 0, 256, -1]])
    with pytest.raises(IndexError):
        s.rows([257])
    # capacity and append: in place, then by reallocation
    c = DeviceData(A[:200], device=dev, capacity=230)
    ptr = c.X.data_ptr()
    assert c.capacity == 230 and c.n == 200
    assert c.append(T[200:230].to(dev)) == 30 and c.X.data_ptr() == ptr and c.n == 230
    old = c.X
    assert c.append(A[230:].astype(np.float16).astype(np.float32)) == 27 and c.X.data_ptr() != ptr and c.capacity == 460
    assert torch.equal(c.X[:230], one.X[:230]) and torch.equal(c.xnorm[:230], one.xnorm[:230]) and torch.equal(old, one.X[:230])
    assert c.append(np.zeros((0, 140))) == 0 and c.append([]) == 0 and c.n == 257


# ------------------------------------------------------------------------------------------------ same model
def _golden_session(cls, name, z, data, dev):
    """The fixture's session on `data`: the learner afterwards and its picks per round."""
    from ital_amd import mvn_stream
    mvn_stream.GLOBAL.reset()
    np.random.seed(0)
    L = cls(data, length_scale=float(z["length_scale"]), device=dev, **make_golden.FIXTURES[name]["kw"])
    L.update({int(z["query"]): 1})
    rel, picks = z["rel"], []
    for r in range(int(z["rounds"])):
        ret = L.fetch_unlabelled(int(z["k"]))
        picks.append(ret)
        L.update({int(i): float(rel[i]) for i in ret})
    return L, picks


_reference_sessions = {}


def _reference(name, golden_dir, dev, rounded):
    """The numpy-built learner of a fixture (on X, or on X rounded to float32), run once per module and left unchanged."""
    import ital_amd
    key = (name, rounded)
    if key not in _reference_sessions:
        z = np.load(os.path.join(golden_dir, name + ".npz"))
        X = z["X"].astype(np.float32).astype(np.float64) if rounded else z["X"]
        cls = getattr(ital_amd, make_golden.FIXTURES[name]["learner"])
        _reference_sessions[key] = (z, cls) + _golden_session(cls, name, z, X, dev)
    return _reference_sessions[key]


def _same_state(A, B):
    m = A.gp.m
    assert m == B.gp.m and A.gp.ind == B.gp.ind and np.array_equal(A.gp.y, B.gp.y)
    assert torch.equal(A.gp.mu, B.gp.mu) and torch.equal(A.gp.s2, B.gp.s2) and torch.equal(A.gp.V[:m], B.gp.V[:m])


@pytest.mark.parametrize("source", ["store_of_numpy_f64", "device_f64_tensor", "host_f32_tensor"])
@pytest.mark.parametrize("name", ["usps500", "usps500_mcmi"])
def test_a_learner_on_a_store_is_the_numpy_built_learner(dev, golden_dir, name, source):
    from ital_amd import DeviceData
    rounded = source == "host_f32_tensor"
    z, cls, ref, ref_picks = _reference(name, golden_dir, dev, rounded)
    if source == "store_of_numpy_f64":
        data = DeviceData(z["X"], device=dev)
    elif source == "device_f64_tensor":
        data = torch.from_numpy(z["X"]).to(dev)
    else:
        data = torch.from_numpy(z["X"].astype(np.float32))
    L, picks = _golden_session(cls, name, z, data, dev)
    assert isinstance(L.data, DeviceData) and L.gp.store is L.data and len(L.data) == len(z["X"]) and L.gp.X_host is None
    assert picks == ref_picks
    if not rounded:
        assert picks == [z[f"r{r}_ret"].tolist() for r in range(int(z["rounds"]))]       # the golden picks
        assert ref_picks == picks
        assert np.array_equal(L.gp.X, z["X"])
    _same_state(L, ref)
    assert torch.equal(L.gp.Xd, ref.gp.Xd) and torch.equal(L.gp.xnorm, ref.gp.xnorm)
    sd = L.state_dict()
    assert sd["n"] == len(z["X"]) and sd["ind"] == ref.state_dict()["ind"]


# ------------------------------------------------------------------------------------------------ sharing
def _truth(X, i):
    return 1 if X[i, 0] > 0.5 else -1


def _fetch(L, k, seed=4):
    """fetch_unlabelled from a defined position of the two process-wide random streams."""
    from ital_amd import mvn_stream
    mvn_stream.GLOBAL.reset()
    np.random.seed(seed)
    return L.fetch_unlabelled(k)


def _interleaved(A, B, X):
    """update A, update B, fetch A, fetch B, update A, fetch B, update B, fetch A, fetch B: the picks in call order."""
    from ital_amd import mvn_stream
    mvn_stream.GLOBAL.reset()
    out = []
    A.update({3: 1, 11: -1, 40: 1})
    B.update({5: -1, 77: 1})
    pa = A.fetch_unlabelled(4)
    pb = B.fetch_unlabelled(3)
    A.update({i: _truth(X, i) for i in pa})
    pb2 = B.fetch_unlabelled(3)                   # a second fetch without an update in between
    B.update({i: -_truth(X, i) for i in pb2})    # other feedback than A's rule
    pa2 = A.fetch_unlabelled(4)
    pb3 = B.fetch_unlabelled(4)
    out += [pa, pb, pb2, pa2, pb3]
    return out


def test_two_learners_share_one_store(dev):
    from ital_amd import ITAL, DeviceData
    X = np.random.default_rng(51).random((150, 6))
    ls = float(np.sqrt(6 / 12.0))
    store = DeviceData(X, device=dev)
    A, B = ITAL(store, length_scale=ls, device=dev), ITAL(store, length_scale=ls, device=dev)
    assert A.data is B.data is store
    assert A.gp.Xd.data_ptr() == B.gp.Xd.data_ptr() == store.X.data_ptr()
    assert A.gp.xnorm.data_ptr() == B.gp.xnorm.data_ptr() == store.xnorm.data_ptr()
    shared = _interleaved(A, B, X)
    C, D = ITAL(X, length_scale=ls, device=dev), ITAL(X, length_scale=ls, device=dev)
    private = _interleaved(C, D, X)
    assert shared == private and all(len(set(p)) == len(p) for p in shared)
    _same_state(A, C)
    _same_state(B, D)
    assert not torch.equal(A.gp.mu, B.gp.mu)
    assert torch.equal(store.X[:, :6], torch.from_numpy(X).to(dev))       # nobody wrote to the shared rows


class _SmallITAL(object):
    """ITAL with room for 16 labelled samples (the class attribute the learners read at construction)."""
    _cls = None

    @classmethod
    def get(cls):
        if cls._cls is None:
            from ital_amd import ITAL
            cls._cls = type("SmallITAL", (ITAL,), dict(gp_capacity=16))
        return cls._cls


def _second_learner_bytes(make_data, dev):
    """memory_allocated of a second learner: read immediately before its construction and after its one update.  Garbage that
    earlier tests left in reference cycles is collected before either reading: what it frees is not the learner's."""
    import gc
    cls = _SmallITAL.get()
    first = cls(make_data(), length_scale=5.0, device=dev)
    first.update({3: 1, 70: -1})
    gc.collect()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    second = cls(make_data(), length_scale=5.0, device=dev)
    second.update({9: 1, 400: -1})
    gc.collect()
    torch.cuda.synchronize()
    return torch.cuda.memory_allocated(dev) - before, first, second


def test_a_second_learner_on_a_store_costs_no_second_copy_of_the_rows(dev):
    from ital_amd import DeviceData
    n, d = 4096, 512
    X = np.random.default_rng(61).random((n, d))
    x_bytes = n * d * 8
    store = DeviceData(X, device=dev)
    shared, a, b = _second_learner_bytes(lambda: store, dev)
    print("second learner on the store: %.2f MiB" % (shared / 2.0 ** 20))
    assert a.gp.Xd.data_ptr() == b.gp.Xd.data_ptr()
    assert 0 < shared < x_bytes // 4, shared
    del a, b
    private, a, b = _second_learner_bytes(lambda: X, dev)
    print("second learner on its own copy: %.2f MiB" % (private / 2.0 ** 20))
    assert private >= x_bytes, private


# ------------------------------------------------------------------------------------------------ growth
def _history(L, X, Q, k, revoke):
    """Labels, one round of k and (optionally) a revoke on a fresh learner; returns the feedback given, in order."""
    history = []
    if not len(Q):
        history.append({i: _truth(X, i) for i in (3, 11, 40, 77)})
        L.update(history[-1])
    got = _fetch(L, k)
    history.append({i: _truth(X, i) for i in got})
    L.update(history[-1])
    if revoke:
        L.revoke([list(history[-1])[1]])
    return history


def _learner_class(name):
    import ital_amd
    return getattr(ital_amd, name)


GROWTH_CASES = [("ITAL", "plain"), ("ITAL", "two_queries"), ("ITAL", "after_revoke"), ("MCMI_min", "plain"), ("AdaptAL", "plain")]


@pytest.mark.parametrize("spare", [0, 64], ids=["reallocates", "in_place"])
@pytest.mark.parametrize("name,case", GROWTH_CASES)
def test_growth_reaches_the_learner_that_syncs_and_no_other(dev, name, case, spare):
    from ital_amd import DeviceData
    cls = _learner_class(name)
    kw = dict(subsample=60) if name in ("MCMI_min", "AdaptAL") else {}
    X = np.random.default_rng(17).random((120, 6))
    ls = float(np.sqrt(6 / 12.0))
    Q = X[[100, 110]] + 0.01 if case == "two_queries" else []
    store = DeviceData(X[:90], device=dev, capacity=90 + spare)
    alone = DeviceData(X[:90], device=dev)
    A, B = cls(store, queries=Q, length_scale=ls, device=dev, **kw), cls(store, queries=Q, length_scale=ls, device=dev, **kw)
    C = cls(alone, queries=Q, length_scale=ls, device=dev, **kw)          # the control: its store never grows
    N = cls(X[:90], queries=Q, length_scale=ls, device=dev, **kw)         # built from numpy: add_data() at the same point
    histories = [_history(L, X, Q, 4, case == "after_revoke") for L in (A, B, C, N)]
    assert histories[0] == histories[1] == histories[2] == histories[3]
    for L in (A, B, C):
        _same_state(L, N)
    if len(Q):
        assert A.gp.ind[:2] == [90, 91]
    assert A.sync_data() == 0 and B.gp.sync_data() == 0
    before = (store.X.data_ptr(), A.gp.Xd.data_ptr(), A.gp.V.data_ptr(), A.gp.mu.data_ptr())
    assert A.sync_data() == 0 and before == (store.X.data_ptr(), A.gp.Xd.data_ptr(), A.gp.V.data_ptr(), A.gp.mu.data_ptr())

    assert store.append(X[90:]) == 30 and len(store) == 120
    assert (store.X.data_ptr() == before[0]) == (spare > 0)
    rounds = A.rounds
    assert A.sync_data() == 30 and A.sync_data() == 0
    # the learner's own _start_afresh fired: what the last fetch left behind was sized for 90 rows
    assert A._last_batch is None
    if name == "ITAL":
        assert A._fetch_bufs is None and A._round_bufs is None
    elif name == "MCMI_min":
        assert A.candidates == [] and A._block_bufs is None and A._fetch_bufs is None and B.candidates != []
    else:
        assert A.last is None and A._block_bufs is None and A._gram_bufs is None and B.last is not None
    N.add_data(X[90:])
    # A: what the numpy-built learner holds after add_data(), bit for bit
    assert A.rounds == rounds and len(A.data) == 120 == A.gp.n == A.gp.n_total and A.gp.Xd.data_ptr() == store.X.data_ptr()
    _same_state(A, N)
    assert torch.equal(A.gp.Xd, N.gp.Xd) and torch.equal(A.gp.xnorm, N.gp.xnorm) and A.gp.mu_all.shape[0] == 120
    if len(Q):
        assert A.gp.ind[:2] == [120, 121]
    assert A.get_unseen() == N.get_unseen() and 119 in A.get_unseen()
    assert A.top_results(5).tolist() == N.top_results(5).tolist()
    pa, pn = _fetch(A, 4), _fetch(N, 4)
    assert pa == pn and len(set(pa)) == 4
    # B has not synced: it goes on on its 90 rows, like the control
    assert B.gp.n == 90 == B.gp.n_total and B.gp.Xd.shape[0] == 90 and (B.gp.Xd.data_ptr() == store.X.data_ptr()) == (spare > 0)
    _same_state(B, C)
    assert B.get_unseen() == C.get_unseen() and max(B.get_unseen()) == 89 and B.state_dict()["n"] == 90
    assert B.top_results(5).tolist() == C.top_results(5).tolist()
    assert sorted(B.top_results().tolist()) == list(range(90))
    pb, pc = _fetch(B, 4), _fetch(C, 4)
    assert pb == pc and max(pb) < 90
    for L in (B, C):
        L.update({i: _truth(X, i) for i in pb})
    _same_state(B, C)
    assert np.array_equal(B.rel_mean, C.rel_mean) and len(B.rel_mean) == 90
    # and it catches up when it chooses to; add_data() on a store learner is append + sync
    assert B.sync_data() == 30 and B.gp.n == 120 and B.gp.Xd.data_ptr() == store.X.data_ptr() and 119 in B.get_unseen()
    assert A.add_data(torch.from_numpy(X[:7]).to(dev)) is A and len(store) == 127 == A.gp.n and B.gp.n == 120
    assert len(_fetch(A, 4)) == 4 and len(_fetch(B, 4)) == 4


# ------------------------------------------------------------------------------------------------ clone
def test_clone_branches_a_session(dev, golden_dir):
    from ital_amd import ITAL, DeviceData
    z = np.load(os.path.join(golden_dir, "usps500.npz"))
    X, rel, k = z["X"], z["rel"], int(z["k"])
    L, picks = _golden_session(ITAL, "usps500", z, DeviceData(X, device=dev), dev)
    history = [{int(z["query"]): 1}] + [{int(i): float(rel[i]) for i in p} for p in picks]
    nxt = _fetch(L, k)
    twin = L.clone()
    assert type(twin) is ITAL and twin.data is L.data and twin.gp is not L.gp and twin.gp.Xd.data_ptr() == L.gp.Xd.data_ptr()
    assert twin.gp.V.data_ptr() != L.gp.V.data_ptr() and twin.gp.mu.data_ptr() != L.gp.mu.data_ptr()
    assert twin.rounds == L.rounds and twin.relevant_ids == L.relevant_ids and twin.relevant_ids is not L.relevant_ids
    assert twin.irrelevant_ids == L.irrelevant_ids and twin.get_unseen() == L.get_unseen()
    assert twin._last_batch is None and twin._fetch_bufs is None and twin._round_bufs is None
    _same_state(twin, L)
    assert torch.equal(twin.gp.L, L.gp.L) and torch.equal(twin.gp.alpha, L.gp.alpha) and torch.equal(twin.gp.XT, L.gp.XT)
    assert _fetch(twin, k) == nxt
    keep = [t.clone() for t in (L.gp.mu, L.gp.s2, L.gp.V, L.gp.L, L.gp.alpha, L.gp.XT, L.gp.XTn)]
    ids = (set(L.relevant_ids), set(L.irrelevant_ids), L.rounds, list(L.gp.ind))
    # the clone takes the opposite feedback and goes on: the original does not move
    other = {int(i): -float(rel[i]) for i in nxt}
    twin.update(other)
    twin_next = _fetch(twin, k)
    for was, now in zip(keep, (L.gp.mu, L.gp.s2, L.gp.V, L.gp.L, L.gp.alpha, L.gp.XT, L.gp.XTn)):
        assert torch.equal(was, now)
    assert ids == (set(L.relevant_ids), set(L.irrelevant_ids), L.rounds, list(L.gp.ind))
    own = {int(i): float(rel[i]) for i in nxt}
    L.update(own)
    orig_next = _fetch(L, k)
    assert twin.rounds == L.rounds and twin.relevant_ids != L.relevant_ids
    # each branch against a learner that replayed the branch's history on a store of its own
    for branch, last, then in ((L, own, orig_next), (twin, other, twin_next)):
        R = ITAL(DeviceData(X, device=dev), length_scale=float(z["length_scale"]), device=dev)
        for g in history + [last]:
            R.update(g)
        assert R.gp.ind == branch.gp.ind
        for a, b, what in ((branch.gp.mu, R.gp.mu, "mu"), (branch.gp.s2, R.gp.s2, "s2")):
            err = float((a - b).abs().max())
            print("%-4s vs replay: %.3g (bound %.3g)" % (what, err, APPEND_ATOL))
            assert err <= APPEND_ATOL, (what, err)
        assert _fetch(R, k) == then and R.get_unseen() == branch.get_unseen()


# ------------------------------------------------------------------------------------------------ predict
@pytest.mark.parametrize("cov_mode", [None, "diag", "full"])
def test_predict_takes_a_tensor(dev, cov_mode):
    from ital_amd import GaussianProcess
    rng = np.random.default_rng(5)
    X = rng.random((300, 33))
    gp = GaussianProcess(X, 0.8 * float(np.sqrt(33 / 12.0)), device=dev, capacity=16)
    idx = rng.permutation(300)[:21].tolist()
    gp.update(idx, np.where(rng.random(21) > 0.5, 1.0, -1.0))
    T32 = torch.from_numpy(rng.random((37, 33)).astype(np.float32))
    for t in (T32.to(dev), T32, T32.to(torch.bfloat16).to(dev), T32.to(torch.float16), T32.to(dev)[5], T32.to(dev).to(torch.float64)):
        want = gp.predict(t.cpu().to(torch.float64).numpy(), cov_mode=cov_mode)
        got = gp.predict(t, cov_mode=cov_mode)
        if cov_mode is None:
            want, got = (want,), (got,)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a.shape == b.shape and np.array_equal(a, b)
    with pytest.raises(ValueError):
        gp.predict(torch.zeros((3, 32), device=dev))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(dev):
    from ital_amd import ITAL, DeviceData, GaussianProcess
    X = np.random.default_rng(71).random((50, 4))
    with pytest.raises(ValueError):
        DeviceData(X[0], device=dev)
    with pytest.raises(ValueError):
        DeviceData(torch.zeros(5, device=dev), device=dev)
    with pytest.raises(TypeError):
        DeviceData(X.astype(np.complex128), device=dev)
    with pytest.raises(TypeError):
        DeviceData(torch.zeros((3, 2), dtype=torch.complex64, device=dev), device=dev)
    store = DeviceData(X, device=dev, capacity=60)
    A = ITAL(store, length_scale=0.6, device=dev)
    A.update({3: 1, 9: -1})
    mean, ptrs = np.array(A.rel_mean), (store.X.data_ptr(), A.gp.Xd.data_ptr(), A.gp.V.data_ptr())
    rows = store.X.clone()
    for bad in (np.zeros((3, 5)), torch.zeros((3, 3), device=dev), np.zeros(4)):
        with pytest.raises(ValueError):
            store.append(bad)
        with pytest.raises(ValueError):
            A.add_data(bad)
    assert len(store) == 50 == len(A.data) == A.gp.n and store.capacity == 60 and A.sync_data() == 0
    assert ptrs == (store.X.data_ptr(), A.gp.Xd.data_ptr(), A.gp.V.data_ptr())
    assert torch.equal(store.X, rows) and np.array_equal(A.rel_mean, mean)
    assert A.add_data(np.zeros((0, 4))) is A and len(store) == 50
    for data in (store, torch.from_numpy(X)):
        with pytest.raises(NotImplementedError):
            GaussianProcess(data, 0.6, device=dev, rank=0, world=2)
        with pytest.raises(NotImplementedError):
            ITAL(data, length_scale=0.6, device=dev, rank=1, world=2)
    N = ITAL(X, length_scale=0.6, device=dev)
    with pytest.raises(ValueError, match="DeviceData"):
        N.clone()
    with pytest.raises(ValueError, match="DeviceData"):
        N.gp.clone()
    with pytest.raises(ValueError, match="DeviceData"):
        N.sync_data()
    assert N.add_data(X[:3]) is N and len(N.data) == 53 and isinstance(N.data, np.ndarray)       # as before on a numpy learner
