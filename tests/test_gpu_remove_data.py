"""remove_data() on the device: the two gathers of csrc/compact.hip against tensor indexing, bit for bit, and what is built on
them -- GaussianProcess.drop_rows, DeviceData.remove with the change log, sync_data over removals, learner.remove_data.

A removal of unlabelled rows is a gather without arithmetic, so every comparison against the state before it is by bit pattern.
A labelled row leaves through the Cholesky row deletion revoke() has, so a removal is compared, bit for bit, with revoke()
followed by the removal.  Against a REBUILT session (a new learner on np.delete(X, ids, 0) that replays the history) the bound
is 2e-9, the one tests/test_gpu_device_data.py uses for a clone against a replay.
Run: python -m pytest tests -m gpu."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REPLAY_ATOL = 2e-9


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


def _pad16(v):
    return (v + 15) // 16 * 16


def _bits(t):
    """The bytes of a tensor: equality of bit patterns (-0.0 != +0.0, a NaN equals itself)."""
    return t.contiguous().view(torch.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ the kernels
DTYPES = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CODES = {"f64": 0, "f32": 1, "f16": 2, "bf16": 3}
NS = (1, 17, 63, 64, 65, 257, 1025)
DS = (1, 16, 17, 130)
MS = (0, 1, 16, 17)


def _keep_patterns(n):
    """name -> ascending survivors of n rows."""
    if n > 64:
        lo, hi = 60, min(70, n)                  # the removed block straddles row 64
    else:
        lo = n // 3
        hi = max(lo + 1, n - n // 3)
    return {"all": np.arange(n), "first": np.array([0]), "last": np.array([n - 1]), "every_other": np.arange(0, n, 2),
            "all_but_a_block": np.concatenate((np.arange(lo), np.arange(hi, n))), "one_left": np.array([n // 2])}


def _random_bits(shape, dtype, dev, seed):
    """A tensor of `dtype` whose every byte is random (NaN patterns and subnormals among the values), with -0.0 and +0.0 in front."""
    g = torch.Generator().manual_seed(seed)
    es = torch.empty(0, dtype=dtype).element_size()
    raw = torch.randint(0, 256, tuple(shape[:-1]) + (shape[-1] * es,), dtype=torch.uint8, generator=g)
    t = raw.view(dtype).clone()
    flat = t.view(-1)
    flat[0] = -0.0
    if flat.numel() > 1:
        flat[1] = 0.0
    return t.to(dev)


def _compact_rows(lib, X, xnorm, n, code, keep_d, X_dst, xnorm_dst, status):
    from ital_amd.gp import _stream
    return lib.ital_compact_rows(X.data_ptr(), xnorm.data_ptr(), n, X.shape[1], code, keep_d.data_ptr(), keep_d.shape[0],
                                 X_dst.data_ptr(), xnorm_dst.data_ptr(), status.data_ptr(), _stream())


def _compact_cols(lib, V, m, mu, s2, n, keep_d, V_dst, mu_dst, s2_dst, status):
    from ital_amd.gp import _stream
    return lib.ital_compact_cols(V.data_ptr(), V.shape[1], m, mu.data_ptr(), s2.data_ptr(), n, keep_d.data_ptr(), keep_d.shape[0],
                                 V_dst.data_ptr(), V_dst.shape[1], V_dst.shape[0], mu_dst.data_ptr(), s2_dst.data_ptr(),
                                 status.data_ptr(), _stream())


def _bad_keeps(n):
    """Index lists with an entry equal to n and one equal to -1 (n_keep <= n: one list each where n == 1)."""
    if n == 1:
        return [np.array([1]), np.array([-1])]
    k = np.arange(n)
    k[0], k[-1] = -1, n
    return [k]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", list(DTYPES))
def test_compact_rows_moves_the_bits_of_the_kept_rows(dev, name, n):
    from ital_amd import _lib
    lib, dtype, code = _lib.lib(), DTYPES[name], CODES[name]
    nan = float("nan")
    for d in DS:
        ldx = _pad16(d)
        X = _random_bits((n, ldx), dtype, dev, 1000 * n + d)             # pad columns hold random bits too
        xnorm = _random_bits((n,), torch.float64, dev, 7000 * n + d)
        for pattern, keep in _keep_patterns(n).items():
            what = (name, n, d, pattern)
            nk = len(keep)
            keep_d = torch.from_numpy(keep.astype(np.int64)).to(dev)
            out = []
            for _ in range(2):                                           # two identical launches
                X_dst = torch.full((nk + 2, ldx), nan, dtype=dtype, device=dev)
                xnorm_dst = torch.full((nk + 2,), nan, dtype=torch.float64, device=dev)
                status = torch.zeros(1, dtype=torch.int32, device=dev)
                assert _compact_rows(lib, X, xnorm, n, code, keep_d, X_dst, xnorm_dst, status) == 0, what
                assert int(status.item()) == 0, what
                out.append((X_dst, xnorm_dst))
            X_dst, xnorm_dst = out[0]
            assert _same_bits(X_dst[:nk], X[keep_d]), what               # pad columns and -0.0 included
            assert _same_bits(xnorm_dst[:nk], xnorm[keep_d]), what
            assert bool(torch.isnan(X_dst[nk:]).all()) and bool(torch.isnan(xnorm_dst[nk:]).all()), what    # not touched
            assert _same_bits(out[0][0], out[1][0]) and _same_bits(out[0][1], out[1][1]), what
        # an index outside [0, n) is never followed: +0.0 rows, bit 0 of the status word, every other row correct
        for keep in _bad_keeps(n):
            what = (name, n, d, keep[[0, -1]].tolist())
            nk = len(keep)
            bad = torch.from_numpy((keep < 0) | (keep >= n)).to(dev)
            keep_d = torch.from_numpy(keep.astype(np.int64)).to(dev)
            X_dst = torch.full((nk + 2, ldx), nan, dtype=dtype, device=dev)
            xnorm_dst = torch.full((nk + 2,), nan, dtype=torch.float64, device=dev)
            status = torch.full((1,), 4, dtype=torch.int32, device=dev)
            assert _compact_rows(lib, X, xnorm, n, code, keep_d, X_dst, xnorm_dst, status) == 0, what
            assert int(status.item()) == 5, what                         # bit 0 set, the rest of the word as it was
            assert bool((_bits(X_dst[:nk][bad]) == 0).all()) and bool((_bits(xnorm_dst[:nk][bad]) == 0).all()), what
            good = keep_d[~bad]
            assert _same_bits(X_dst[:nk][~bad], X[good]) and _same_bits(xnorm_dst[:nk][~bad], xnorm[good]), what
            assert bool(torch.isnan(X_dst[nk:]).all()) and bool(torch.isnan(xnorm_dst[nk:]).all()), what


@pytest.mark.parametrize("n", NS)
def test_compact_cols_moves_the_bits_of_the_kept_columns_and_zeroes_the_rest(dev, n):
    from ital_amd import _lib
    lib = _lib.lib()
    nan = float("nan")
    ldv = _pad16(n) + 16
    for m in MS:
        V = _random_bits((max(m, 1), ldv), torch.float64, dev, 31 * n + m)
        mu = _random_bits((n,), torch.float64, dev, 37 * n + m)
        s2 = _random_bits((n,), torch.float64, dev, 41 * n + m)
        cases = [(p, k) for p, k in _keep_patterns(n).items()] + [("bad", k) for k in _bad_keeps(n)]
        for pattern, keep in cases:
            what = (n, m, pattern)
            nk = len(keep)
            bad = torch.from_numpy((keep < 0) | (keep >= n)).to(dev)
            keep_d = torch.from_numpy(keep.astype(np.int64)).to(dev)
            good = keep_d[~bad]
            ldd = _pad16(nk) + (16 if pattern in ("every_other", "first") else 0)     # with and without whole pad blocks
            out = []
            for _ in range(2):
                V_dst = torch.full((m + 3, ldd), nan, dtype=torch.float64, device=dev)
                mu_dst = torch.full((nk + 2,), nan, dtype=torch.float64, device=dev)
                s2_dst = torch.full((nk + 2,), nan, dtype=torch.float64, device=dev)
                status = torch.zeros(1, dtype=torch.int32, device=dev)
                assert _compact_cols(lib, V, m, mu, s2, n, keep_d, V_dst, mu_dst, s2_dst, status) == 0, what
                assert int(status.item()) == (1 if pattern == "bad" else 0), what
                out.append((V_dst, mu_dst, s2_dst))
            V_dst, mu_dst, s2_dst = out[0]
            assert _same_bits(V_dst[:m, :nk][:, ~bad], V[:m][:, good]), what
            assert _same_bits(mu_dst[:nk][~bad], mu[good]) and _same_bits(s2_dst[:nk][~bad], s2[good]), what
            assert bool((_bits(V_dst[:m, :nk][:, bad]) == 0).all()), what             # a refused index: +0.0
            assert bool((_bits(mu_dst[:nk][bad]) == 0).all()) and bool((_bits(s2_dst[:nk][bad]) == 0).all()), what
            assert bool((_bits(V_dst[:m, nk:]) == 0).all()), what                     # pad columns: +0.0 by bits
            assert bool((_bits(V_dst[m:]) == 0).all()), what                          # rows m .. v_rows_dst: +0.0 by bits
            assert bool(torch.isnan(mu_dst[nk:]).all()) and bool(torch.isnan(s2_dst[nk:]).all()), what
            for a, b in zip(out[0], out[1]):
                assert _same_bits(a, b), what
    # no survivor: V_dst is still zero-filled
    keep_d = torch.zeros(0, dtype=torch.int64, device=dev)
    V = _random_bits((4, ldv), torch.float64, dev, n)
    V_dst = torch.full((6, 16), nan, dtype=torch.float64, device=dev)
    one = torch.full((1,), nan, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    assert lib.ital_compact_cols(V.data_ptr(), ldv, 4, mu.data_ptr(), s2.data_ptr(), n, 0, 0, V_dst.data_ptr(), 16, 6,
                                 one.data_ptr(), one.data_ptr(), status.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool((_bits(V_dst) == 0).all()) and bool(torch.isnan(one).all()) and int(status.item()) == 0


# ------------------------------------------------------------------------------------------------ sessions
def _truth(X, i):
    return 1 if X[i, 0] > 0.5 else -1


def _fetch(L, k, seed=4):
    """fetch_unlabelled from a defined position of the two process-wide random streams."""
    from ital_amd import mvn_stream
    mvn_stream.GLOBAL.reset()
    np.random.seed(seed)
    return [int(i) for i in L.fetch_unlabelled(k)]


def _drive(L, X, k, rounds, first=(3, 11, 40, 77), unnameable=()):
    """First labels (none for a learner with queries), `rounds` rounds of k and unnameable feedback; the feedback given."""
    history = []
    if first:
        history.append({i: _truth(X, i) for i in first})
        L.update(history[-1])
    for _ in range(rounds):
        history.append({i: _truth(X, i) for i in _fetch(L, k)})
        L.update(history[-1])
    if unnameable:
        history.append({i: 0 for i in unnameable})
        L.update(history[-1])
    return history


def _replay(L, history, index_map):
    """The history on a learner over the reduced matrix: removed ids dropped, the others under their new numbers."""
    for fb in history:
        fb = {int(index_map[i]): v for i, v in fb.items() if index_map[i] >= 0}
        if fb:
            L.update(fb)


def _snapshot(gp):
    m = gp.m
    return dict(m=m, mu=gp.mu[: gp.n].clone(), s2=gp.s2[: gp.n].clone(), V=gp.V[:m, : gp.n].clone(), L=gp.L.clone(),
                alpha=gp.alpha.clone(), XT=gp.XT.clone(), ind=list(gp.ind))


def _same_state(A, B):
    m = A.gp.m
    assert m == B.gp.m and A.gp.ind == B.gp.ind and np.array_equal(A.gp.y, B.gp.y) and A.gp.n == B.gp.n
    assert A.gp.n_total == B.gp.n_total and A.gp.ldv == B.gp.ldv and A.gp.appends == B.gp.appends
    for name in ("mu", "s2", "L", "alpha"):
        assert _same_bits(getattr(A.gp, name), getattr(B.gp, name)), name
    assert _same_bits(A.gp.V[:m], B.gp.V[:m])
    assert A.relevant_ids == B.relevant_ids and A.irrelevant_ids == B.irrelevant_ids and A.unnameable_ids == B.unnameable_ids
    assert A.rounds == B.rounds and A._fitted == B._fitted


def _scattered(n, seen, count, seed, must=()):
    """`count` ascending ids of the n rows, `must` among them, none of `seen`."""
    rng = np.random.default_rng(seed)
    free = [i for i in rng.permutation(n).tolist() if i not in seen and i not in must]
    return sorted(list(must) + free[: count - len(must)])


def _np_map(n, ids):
    left = np.delete(np.arange(n), ids)
    out = np.full(n, -1, dtype=np.int64)
    out[left] = np.arange(len(left))
    return out


_ital_300 = {}


def _ital_session(dev):
    """ITAL on 300 x 16 rows after three rounds of k = 3 and one unnameable sample, then remove_data of 40 unlabelled ids:
    run once per module and left unchanged.  Returns everything the tests compare."""
    if not _ital_300:
        from ital_amd import ITAL
        X = np.random.default_rng(71).random((300, 16))
        ls = float(np.sqrt(16 / 12.0))
        L = ITAL(X, length_scale=ls, device=dev)
        history = _drive(L, X, 3, 3)
        un = [i for i in L.get_unseen() if i >= 150][:2]         # two samples the user cannot name
        history.append({i: 0 for i in un})
        L.update(history[-1])
        labelled = set(L.relevant_ids) | set(L.irrelevant_ids)
        assert len(labelled) == 13 and L.gp.m == 13 and not {0, 299} & labelled
        ids = _scattered(300, labelled | set(un), 40, 5, must=(0, 299, un[1]))
        before = _snapshot(L.gp)
        before.update(unseen=L.get_unseen(), ranking=L.top_results(300).tolist(), rel=set(L.relevant_ids),
                      irr=set(L.irrelevant_ids), unn=set(L.unnameable_ids), rounds=L.rounds, Xd=L.gp.Xd.clone(),
                      xnorm=L.gp.xnorm.clone())
        got = L.remove_data(ids[::-1] + [ids[3], ids[0] - 300])          # any order, duplicates, from the end
        _ital_300.update(X=X, ls=ls, L=L, history=history, ids=ids, before=before, map=got, un=un)
    return _ital_300


def test_removing_unlabelled_rows_is_a_gather(dev):
    s = _ital_session(dev)
    L, b, ids, X = s["L"], s["before"], s["ids"], s["X"]
    want = _np_map(300, ids)
    assert s["map"].dtype == np.int64 and np.array_equal(s["map"], want)
    keep = torch.from_numpy(np.delete(np.arange(300), ids)).to(dev)
    gp, m = L.gp, b["m"]
    assert (gp.n, gp.n_total, gp.row1, gp.ldv, gp.m) == (260, 260, 260, 272, m) and len(L.data) == 260
    assert np.array_equal(L.data, np.delete(X, ids, 0)) and L.data is gp.X_host
    assert _same_bits(gp.mu, b["mu"][keep]) and _same_bits(gp.s2, b["s2"][keep])
    assert _same_bits(gp.V[:m, :260], b["V"][:, keep])
    assert bool((_bits(gp.V[:m, 260:]) == 0).all()) and bool((_bits(gp.V[m:]) == 0).all())
    assert _same_bits(gp.L, b["L"]) and _same_bits(gp.alpha, b["alpha"]) and _same_bits(gp.XT, b["XT"])
    assert _same_bits(gp.Xd, b["Xd"][keep]) and _same_bits(gp.xnorm, b["xnorm"][keep])
    assert int(gp.status.item()) == 0 and gp.mu_all.shape[0] == 260
    remap = lambda q: set(int(want[i]) for i in q if want[i] >= 0)      # noqa: E731
    assert L.relevant_ids == remap(b["rel"]) and L.irrelevant_ids == remap(b["irr"])
    assert L.unnameable_ids == remap(b["unn"]) == {int(want[s["un"][0]])} and L.rounds == b["rounds"] and L._fitted
    assert gp.ind == [int(want[i]) for i in b["ind"]]
    assert L.get_unseen() == [int(want[i]) for i in b["unseen"] if want[i] >= 0]
    ranking = [int(want[i]) for i in b["ranking"] if want[i] >= 0]
    assert L.top_results(10).tolist() == ranking[:10] and L.top_results(260).tolist() == ranking
    assert np.array_equal(L.rel_mean, b["mu"].cpu().numpy()[keep.cpu().numpy()])
    assert L.state_dict()["n"] == 260


def test_after_the_removal_the_session_is_the_rebuilt_one(dev):
    from ital_amd import ITAL
    s = _ital_session(dev)
    L, X, ids = s["L"], s["X"], s["ids"]
    R = ITAL(np.delete(X, ids, 0), length_scale=s["ls"], device=dev)
    _replay(R, s["history"], s["map"])
    assert R.gp.ind == L.gp.ind and R.get_unseen() == L.get_unseen() and R.unnameable_ids == L.unnameable_ids
    dmu = float((R.gp.mu - L.gp.mu).abs().max())
    ds2 = float((R.gp.s2 - L.gp.s2).abs().max())
    print("ITAL removed vs rebuilt: max |dmu| = %.3g, max |ds2| = %.3g, bit-equal: %s"
          % (dmu, ds2, _same_bits(R.gp.mu, L.gp.mu) and _same_bits(R.gp.s2, L.gp.s2)))
    assert dmu <= REPLAY_ATOL and ds2 <= REPLAY_ATOL
    # the picks of the next round (the shared session is left as it is: a clone of its state is not needed to fetch)
    pl, pr = _fetch(L, 3), _fetch(R, 3)
    assert pl == pr and len(set(pl)) == 3 and not set(pl) & (L.relevant_ids | L.irrelevant_ids | L.unnameable_ids)
    # round trip: the state after a removal loads into a fresh learner over the reduced matrix
    F = ITAL(np.delete(X, ids, 0), length_scale=s["ls"], device=dev)
    F.load_state_dict(L.state_dict(), restore_stream=False)
    assert F.gp.ind == L.gp.ind and F.relevant_ids == L.relevant_ids and F.unnameable_ids == L.unnameable_ids
    np.testing.assert_allclose(F.rel_mean, L.rel_mean, rtol=0, atol=REPLAY_ATOL)


OTHERS = {"ITAL_general": ("ITAL", dict(label_prob=0.9, mistake_prob=0.05), 3), "MCMI_min": ("MCMI_min", dict(subsample=60), 2),
          "AdaptAL": ("AdaptAL", dict(subsample=60), 3), "BorderlineSampling": ("BorderlineSampling", {}, 3),
          "EntropySampling": ("EntropySampling", {}, 2)}


@pytest.mark.parametrize("case", list(OTHERS))
def test_other_learners_after_remove_data_equal_the_rebuilt_session(dev, case):
    import ital_amd
    from ital_amd import baselines
    name, kw, k = OTHERS[case]
    cls = getattr(ital_amd, name, None) or getattr(baselines, name)
    X = np.random.default_rng(23).random((150, 4))           # the shapes of the growth tests (tests/test_gpu_rewhiten.py)
    A = cls(X, length_scale=0.6, device=dev, **kw)
    history = _drive(A, X, k, 2, unnameable=(90,))
    seen = set().union(*history)
    ids = _scattered(150, seen - {90}, 31, 9, must=(0, 149, 90))
    snap = _snapshot(A.gp)
    got = A.remove_data(ids)
    assert np.array_equal(got, _np_map(150, ids)) and A.gp.n == 119 == len(A.data)
    keep = torch.from_numpy(np.delete(np.arange(150), ids)).to(dev)
    assert _same_bits(A.gp.mu, snap["mu"][keep]) and _same_bits(A.gp.s2, snap["s2"][keep])
    assert _same_bits(A.gp.V[: snap["m"], :119], snap["V"][:, keep]) and _same_bits(A.gp.L, snap["L"])
    R = cls(np.delete(X, ids, 0), length_scale=0.6, device=dev, **kw)
    _replay(R, history, got)
    assert R.gp.ind == A.gp.ind and R.get_unseen() == A.get_unseen() and A.unnameable_ids == set()
    dmu = float((R.gp.mu - A.gp.mu).abs().max())
    ds2 = float((R.gp.s2 - A.gp.s2).abs().max())
    print("%s removed vs rebuilt: max |dmu| = %.3g, max |ds2| = %.3g" % (case, dmu, ds2))
    assert dmu <= REPLAY_ATOL and ds2 <= REPLAY_ATOL
    pa, pr = _fetch(A, k), _fetch(R, k)
    assert pa == pr and len(set(pa)) == k and max(pa) < 119
    A.update({i: _truth(A.data, i) for i in pa})              # and the retrieval loop goes on
    assert len(_fetch(A, k)) == k


# ------------------------------------------------------------------------------------------------ labelled rows
def _pair(dev, X, ls, **kw):
    from ital_amd import ITAL
    out = []
    for _ in range(2):
        L = ITAL(X, length_scale=ls, device=dev, **kw)
        _drive(L, X, 3, 2, first=() if "queries" in kw else (3, 11, 40, 77))
        out.append(L)
    assert out[0].gp.ind == out[1].gp.ind and _same_bits(out[0].gp.mu, out[1].gp.mu)
    return out


def test_a_labelled_row_leaves_as_revoke_then_removal(dev):
    X = np.random.default_rng(83).random((120, 6))
    ls = float(np.sqrt(6 / 12.0))
    A, B = _pair(dev, X, ls)
    i = A.gp.ind[5]                                           # labelled, from a fetched round
    j = next(q for q in range(50, 120) if q not in A.gp.ind)
    m = A.gp.m
    got = A.remove_data([i, j])
    B.revoke([i])
    assert B.gp.m == m - 1
    snap = _snapshot(B.gp)
    assert np.array_equal(B.remove_data([i, j]), got) and np.array_equal(got, _np_map(120, sorted((i, j))))
    _same_state(A, B)
    assert A.gp.m == m - 1 and A.gp.n == 118 and i not in (A.relevant_ids | A.irrelevant_ids)
    # for B the removal was a gather of unlabelled rows again
    keep = torch.from_numpy(np.delete(np.arange(120), [i, j])).to(dev)
    assert _same_bits(B.gp.mu, snap["mu"][keep]) and _same_bits(B.gp.V[: m - 1, :118], snap["V"][:, keep])
    assert _same_bits(B.gp.L, snap["L"]) and _same_bits(B.gp.alpha, snap["alpha"])
    assert sum(c for c in A.gp.appends) == m - 1 and A.state_dict()["n"] == 118


def test_removing_the_only_labelled_sample_leaves_the_prior(dev):
    from ital_amd import ITAL
    X = np.random.default_rng(89).random((70, 5))
    L = ITAL(X, length_scale=0.6, var=1.5, device=dev)
    L.update({5: 1})
    assert L._fitted and L.rel_mean is not None
    L.remove_data([5, 60])
    assert L.gp.m == 0 and not L._fitted and L.rel_mean is None and L.relevant_ids == set() and L.gp.n == 68
    assert bool((L.gp.mu == 0).all()) and bool((L.gp.s2 == 1.5).all()) and bool((L.gp.V == 0).all())
    assert L.gp.mu.shape[0] == 68 and L.gp.ind == [] and L.get_unseen() == list(range(68))
    L.update({5: 1, 9: -1})                                   # and the session goes on, as a fresh learner's would
    F = ITAL(np.delete(X, [5, 60], 0), length_scale=0.6, var=1.5, device=dev)
    F.update({5: 1, 9: -1})
    assert np.array_equal(L.rel_mean, F.rel_mean)


def test_query_rows_move_down_and_predictions_stay(dev):
    X = np.random.default_rng(97).random((120, 6))
    ls = float(np.sqrt(6 / 12.0))
    Q = X[[100, 110]] + 0.01
    A, B = _pair(dev, X, ls, queries=Q)
    assert A.gp.ind[:2] == [120, 121]
    i = A.gp.ind[3]
    free = [q for q in range(120) if q not in A.gp.ind]
    ids = [free[0], free[7], free[-1]]
    mean, var = [np.array(t) for t in A.gp.predict_stored(cov_mode="diag")]
    got = A.remove_data(ids)
    keep = np.delete(np.arange(120), ids)
    assert A.gp.ind[:2] == [117, 118] and A.gp.ind[2:] == [int(got[q]) for q in B.gp.ind[2:]]
    m2, v2 = A.gp.predict_stored(cov_mode="diag")
    np.testing.assert_allclose(m2, mean[keep], rtol=0, atol=REPLAY_ATOL)
    np.testing.assert_allclose(v2, var[keep], rtol=0, atol=REPLAY_ATOL)
    assert np.array_equal(m2, mean[keep]) and np.array_equal(v2, var[keep])          # a gather: in fact the same bits
    # a labelled row next to the queries: revoke then removal, as without queries
    A.remove_data([int(got[i])])
    B.revoke([i])
    B.remove_data(ids + [i])
    _same_state(A, B)
    assert A.gp.ind[:2] == [116, 117] and A._fitted
    with pytest.raises(ValueError):
        A.remove_data([116])                                  # a query row
    assert len(_fetch(A, 3)) == 3


# ------------------------------------------------------------------------------------------------ a shared store
STORES = {"f64": (np.float64, "f64"), "source_f16": (np.float16, "source"), "source_f32": (np.float32, "source")}


@pytest.mark.parametrize("kind", list(STORES))
def test_a_removal_reaches_the_learner_that_syncs_and_no_other(dev, kind):
    from ital_amd import ITAL, DeviceData
    np_type, storage = STORES[kind]
    X = np.random.default_rng(17).random((150, 6)).astype(np_type)
    X64 = X.astype(np.float64)
    ls = float(np.sqrt(6 / 12.0))
    store = DeviceData(X, device=dev, storage=storage)
    own = DeviceData(X, device=dev, storage=storage)          # N's: it removes the rows itself
    alone = DeviceData(X, device=dev, storage=storage)        # the control's: it never changes
    wide = DeviceData(X64, device=dev)                        # the FP64 store of the same values
    A, B, N, C, W = [ITAL(s, length_scale=ls, device=dev) for s in (store, store, own, alone, wide)]
    histories = [_drive(L, X64, 3, 2) for L in (A, B, N, C, W)]
    assert all(h == histories[0] for h in histories)
    K = A.clone()                                             # a clone taken before the removal
    labelled = A.gp.ind[4]
    seen = set(A.gp.ind)
    ids = _scattered(150, seen, 20, 3, must=(0, 149)) + [labelled]
    old_ptr, epoch = store.X.data_ptr(), store.epoch
    want = _np_map(150, sorted(ids))
    assert np.array_equal(store.remove(ids), want) and store.n == 129 and store.epoch == epoch + 1
    assert store.X.data_ptr() != old_ptr and store.capacity == alone.capacity
    assert _same_bits(store.X, alone.X[torch.from_numpy(np.delete(np.arange(150), ids)).to(dev)])
    # B has not synced: its views keep the old tensors, and it goes on as the control does, bit for bit
    assert B.gp.Xd.data_ptr() == old_ptr and B.gp.n == 150 == B._num_samples() and _same_bits(B.gp.Xd, alone.X)
    assert np.array_equal(B.rel_mean, C.rel_mean)
    pb, pc = _fetch(B, 3), _fetch(C, 3)
    assert pb == pc
    for L in (B, C):
        L.update({i: _truth(X64, i) for i in pb})
    assert np.array_equal(B.rel_mean, C.rel_mean) and len(B.rel_mean) == 150
    # A syncs: what a learner that removed the rows itself holds, bit for bit
    assert N.remove_data(ids) is not None and np.array_equal(N.last_index_map, want)
    assert A.sync_data() == 0 and np.array_equal(A.last_index_map, want) and np.array_equal(A.gp.last_index_map, want)
    _same_state(A, N)
    assert A.gp.Xd.data_ptr() == store.X.data_ptr() and _same_bits(A.gp.Xd, N.gp.Xd) and _same_bits(A.gp.xnorm, N.gp.xnorm)
    assert A.gp.m == len(seen) - 1 and int(want[labelled]) == -1 and A.gp.n == 129 == len(A.data)
    assert A.sync_data() == 0 and A.last_index_map is None    # nothing new: nothing applied
    # the clone taken before the removal catches up the same way
    assert K.gp.n == 150 and K.sync_data() == 0
    _same_state(K, A)
    # a compact store gives the bits of the FP64 store
    W.remove_data(ids)
    _same_state(A, W)
    assert A.get_unseen() == W.get_unseen()
    pa, pn, pw = _fetch(A, 3), _fetch(N, 3), _fetch(W, 3)
    assert pa == pn == pw and len(set(pa)) == 3 and max(pa) < 129
    # B catches up later, with its extra round: the labelled rows among the removed ones leave it too
    assert B.sync_data() == 0 and B.gp.n == 129 and not (set(int(want[i]) for i in pb) - {-1}) - set(B.gp.ind)
    # add_data() after remove_data() numbers the new rows from the new n_total
    A.add_data(X[:5])
    assert len(store) == 134 == A.gp.n == A.gp.n_total and A.get_unseen()[-5:] == [129, 130, 131, 132, 133]
    assert store.log[-2:] == [("remove", sorted(ids), 150), ("append", 5)]


def test_a_log_of_remove_append_remove_synced_at_once_equals_three_syncs(dev):
    from ital_amd import ITAL, DeviceData
    X = np.random.default_rng(19).random((140, 6))
    ls = float(np.sqrt(6 / 12.0))
    one, three = DeviceData(X[:120], device=dev), DeviceData(X[:120], device=dev)
    E, F = ITAL(one, length_scale=ls, device=dev), ITAL(three, length_scale=ls, device=dev)
    assert _drive(E, X, 3, 2) == _drive(F, X, 3, 2)
    lab1, lab2 = E.gp.ind[2], E.gp.ind[7]
    seen = set(E.gp.ind)
    first = _scattered(120, seen, 15, 11, must=(0,)) + [lab1]
    m1 = _np_map(120, sorted(first))
    n1 = 120 - len(first)
    # the second removal: rows of the first 120, a labelled one, and rows that were appended in between
    second = sorted([int(m1[i]) for i in _scattered(120, seen | set(first), 10, 13)] + [int(m1[lab2]), n1 + 2, n1 + 19])
    maps = []
    for store, L in ((one, E), (three, F)):
        store.remove(first)
        if L is F:
            assert L.sync_data() == 0
            maps.append(L.last_index_map)
        store.append(X[120:])
        if L is F:
            assert L.sync_data() == 20 and L.last_index_map is None
        store.remove(second)
        if L is F:
            assert L.sync_data() == 0
            maps.append(L.last_index_map)
    assert E.gp.n == 120 and E.sync_data() == 18              # two of the 20 appended rows never entered the model
    _same_state(E, F)
    assert _same_bits(E.gp.Xd, F.gp.Xd) and _same_bits(E.gp.xnorm, F.gp.xnorm) and E.gp.n == one.n == n1 + 20 - len(second)
    composed = np.where(maps[0] >= 0, maps[1][np.maximum(maps[0], 0)], -1)
    assert np.array_equal(E.last_index_map, composed) and len(E.last_index_map) == 120
    from ital_amd.device_data import log_index_map
    assert np.array_equal(log_index_map(one.log, 120)[0], composed)
    assert E.get_unseen() == F.get_unseen() and _fetch(E, 3) == _fetch(F, 3)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_change_nothing(dev):
    from ital_amd import ITAL, DeviceData
    X = np.random.default_rng(41).random((50, 4))
    Q = X[[7]] + 0.01
    for data in (X, DeviceData(X, device=dev)):
        A = ITAL(data, queries=Q, length_scale=0.6, device=dev)
        A.update({3: 1, 9: -1})
        mu, V, ind = A.gp.mu.clone(), A.gp.V.clone(), list(A.gp.ind)
        ptr = A.gp.mu.data_ptr()
        for bad in ([50], [2, 51], [-51], [50 + 0]):          # outside the rows; 50 is the query row
            with pytest.raises((ValueError, IndexError)):
                A.remove_data(bad)
        with pytest.raises((ValueError, IndexError)):
            A.remove_data(range(50))                          # every row
        A.world = 2
        with pytest.raises(NotImplementedError, match="cannot shrink"):
            A.remove_data([1])
        A.world = 1
        assert np.array_equal(A.remove_data([]), np.arange(50))
        assert _same_bits(A.gp.mu, mu) and _same_bits(A.gp.V, V) and A.gp.ind == ind and A.gp.mu.data_ptr() == ptr
        assert A.gp.n == 50 == len(A.data) and A.relevant_ids == {3} and A.irrelevant_ids == {9}
        if isinstance(data, DeviceData):
            assert data.n == 50 and data.log == [] and data.epoch == 0
        else:
            with pytest.raises(ValueError):
                A.gp.drop_rows([50])                          # the query row, as remove() refuses it
            assert A.gp.drop_rows([]) is A.gp
    g = ITAL(X, length_scale=0.6, device=dev).gp
    g.world = 2
    with pytest.raises(NotImplementedError, match="cannot shrink"):
        g.drop_rows([1])
