"""Host side of per-label noise (no device): the C declarations of include/ital_reweigh.h against their bindings, the argument
checks that come before any HIP call, a numpy emulation of exactly the recurrences of csrc/reweigh.hip against the dense
model of tests/_reweigh_ref.py within the bound of DESIGN.md section 12 -- and against three injected mistakes, so the
checker is known to be able to fail -- and the Python layer's refusals and state_dict shape on bare objects.
The GPU side is tests/test_gpu_reweigh.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _reweigh_ref as ref  # noqa: E402

REWEIGH = ["ital_gp_reweigh", "ital_gp_reweigh_workspace"]


# ------------------------------------------------------------------------------------------------------ the C boundary
def test_reweigh_declarations_equal_bindings_and_are_exported():
    from ital_amd import _lib
    header = open(os.path.join(ROOT, "include", "ital_reweigh.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", code))
    assert declared == set(REWEIGH) == set(_lib.REWEIGH_SIGNATURES), declared ^ set(_lib.REWEIGH_SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in REWEIGH:
        assert hasattr(raw, name), name
    lib = _lib.load()
    for name, (res, args) in _lib.REWEIGH_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert "ital_ctx" in header                      # the header says that the context layer is out of scope
    assert "ital_gp_reweigh" not in open(os.path.join(ROOT, "include", "ital_hip.h")).read()


def test_reweigh_desc_fields_follow_the_header():
    """Same field names in the same order as the struct in the header, pointers as pointers."""
    from ital_amd import _lib
    header = open(os.path.join(ROOT, "include", "ital_reweigh.h")).read()
    body = re.search(r"typedef struct ital_reweigh_desc \{(.*?)\} ital_reweigh_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.search(r"([A-Za-z_0-9]+)$", d).group(1) for d in fields]
    assert names == [f[0] for f in _lib.ItalReweighDesc._fields_]
    assert names[:12] == ["L", "ldl", "alpha", "V", "ldv", "n", "mu", "s2", "m", "work", "work_doubles", "status"]
    assert names[12:] == ["r", "pos", "delta"]
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    for d, (name, ctype) in zip(fields, _lib.ItalReweighDesc._fields_):
        assert ctype is (ctypes.c_void_p if "*" in d else kinds[d.split()[0]]), name


def _desc(pos=(1, 3), delta=(0.5, -0.25), **kw):
    from ital_amd import _lib
    d = _lib.ItalReweighDesc()
    r = len(pos)
    ws = int(_lib.load().ital_gp_reweigh_workspace(8, r))
    cpos, cdelta = (ctypes.c_int * max(r, 1))(*pos), (ctypes.c_double * max(r, 1))(*delta)
    base = dict(L=64, ldl=16, alpha=64, V=64, ldv=32, n=20, mu=64, s2=64, m=8, work=64, work_doubles=ws, status=64, r=r,
                pos=ctypes.cast(cpos, ctypes.c_void_p), delta=ctypes.cast(cdelta, ctypes.c_void_p))
    base.update(kw)
    for k, v in base.items():
        setattr(d, k[:-4] if k.endswith("_ptr") else k, v)
    d._keep = (cpos, cdelta)
    return d


def test_entry_point_refuses_bad_arguments_without_a_device():
    """-22 before any HIP call, with the entry point's name in ital_last_error."""
    from ital_amd import _lib
    lib = _lib.load()

    def refused(rc):
        assert rc == -22
        assert "ital_gp_reweigh" in lib.ital_last_error().decode()

    assert lib.ital_gp_reweigh_workspace(0, 1) == 0 and lib.ital_gp_reweigh_workspace(8, 0) == 0
    assert lib.ital_gp_reweigh_workspace(-1, 3) == 0
    # the refused word and its header, (g, h) and four coefficients per (label, row), the carries, the block with alpha's row
    assert lib.ital_gp_reweigh_workspace(8, 2) == 8 + 2 * 2 + 4 * 2 * 8 + (8 + 2) + (8 + 1) * 8
    assert lib.ital_gp_reweigh_workspace(256, 9) >= 4 * 9 * 256 + 257 * 256
    refused(lib.ital_gp_reweigh(None, None))
    ws = int(lib.ital_gp_reweigh_workspace(8, 2))
    for bad in (dict(m=0), dict(m=-1), dict(ldl=7), dict(ldv=19), dict(ldv=33), dict(n=-1), dict(L=None), dict(alpha=None),
                dict(work=None), dict(status=None), dict(V=None), dict(mu=None), dict(s2=None), dict(pos_ptr=None),
                dict(delta_ptr=None), dict(work_doubles=ws - 1), dict(work=72), dict(r=0)):
        refused(lib.ital_gp_reweigh(ctypes.byref(_desc(**bad)), None))
    for pos in ((3, 1), (1, 1), (-1, 2), (2, 8)):
        refused(lib.ital_gp_reweigh(ctypes.byref(_desc(pos=pos)), None))
    for delta in ((0.5, float("nan")), (float("inf"), 0.1)):
        refused(lib.ital_gp_reweigh(ctypes.byref(_desc(delta=delta)), None))
    refused(lib.ital_gp_reweigh(ctypes.byref(_desc(V=None, n=5)), None))     # V == NULL is the factor-only call: n == 0 only


# ------------------------------------------------------------------------------------------------------ the recurrences
def _case(m, r, seed):
    """A labelled set of m samples among n = 40 rows, r of them changing: some up from 0, some down to 0, some between two
    non-zero values.  Returns (X, XT, y, e before, e after, pos, delta)."""
    rng = np.random.default_rng(seed)
    X = rng.random((40, 5))
    XT = np.concatenate((X[rng.choice(40, min(m, 30), replace=False)], rng.random((max(0, m - 30), 5))))
    y = rng.choice([-1.0, 1.0], size=m)
    pos = sorted(int(p) for p in rng.choice(m, r, replace=False))
    e0 = np.zeros(m)
    e0[rng.choice(m, m // 3, replace=False)] = 0.2            # labels outside the call carry noise too
    e1 = e0.copy()
    for t, p in enumerate(pos):
        kind = t % 3
        if kind == 0:
            e0[p], e1[p] = 0.0, 0.05 + 0.3 * rng.random()     # update
        elif kind == 1:
            e0[p], e1[p] = 0.05 + 0.3 * rng.random(), 0.0     # downdate, back to full weight
        else:
            e0[p], e1[p] = 0.4, 0.1                           # downdate between two values
    return X, XT, y, e0, e1, pos, [e1[p] - e0[p] for p in pos]


LS = 0.7
CASES = [(m, r) for m in (1, 2, 63, 64, 65, 130) for r in (1, 2, 8, 9) if r <= m]


def _check(state, X, XT, y, e1, cnd):
    L, alpha, V, mu, s2 = state
    D = ref.Dense(X, XT, y, e1, LS)
    import scipy.linalg
    ref.within(mu, D.mean, cnd, "mean")
    ref.within(s2, D.var, cnd, "variance")
    rows = D.rows
    ref.within(ref.rbf(X[rows], X[rows], LS) - V[:, rows].T @ V[:, rows], D.cov, cnd, "covariance")
    ref.within(L @ L.T, D.K, cnd, "K")
    ref.within(scipy.linalg.solve_triangular(L, alpha, lower=True, trans="T"), D.w, cnd, "w")
    ref.within(V.T @ alpha, D.mean, cnd, "V^T alpha")
    assert np.all(np.triu(L, 1) == 0) and np.all(np.diag(L) > 0)


@pytest.mark.parametrize("m,r", CASES)
def test_emulated_recurrences_reproduce_the_dense_model(m, r):
    X, XT, y, e0, e1, pos, delta = _case(m, r, 100 * m + r)
    cnd = max(ref.cond(ref.gram(XT, e0, LS)), ref.cond(ref.gram(XT, e1, LS)))
    state = ref.whitened(X, XT, y, e0, LS)
    before = [a.copy() for a in state]
    out = ref.emulate(*state, pos, delta)
    for a, b in zip(state, before):
        assert np.array_equal(a, b)                  # the emulation works on copies
    _check(out, X, XT, y, e1, cnd)
    p0 = pos[0]
    assert np.array_equal(out[0][:p0], before[0][:p0]) and np.array_equal(out[2][:p0], before[2][:p0])   # rows above: not touched


def _rejects(m, r, seed, **mistake):
    X, XT, y, e0, e1, pos, delta = _case(m, r, seed)
    cnd = max(ref.cond(ref.gram(XT, e0, LS)), ref.cond(ref.gram(XT, e1, LS)))
    state = ref.whitened(X, XT, y, e0, LS)
    _check(ref.emulate(*state, pos, delta), X, XT, y, e1, cnd)             # the case itself is sound
    with pytest.raises((AssertionError, ref.Refused)):
        _check(ref.emulate(*state, pos, delta, **mistake), X, XT, y, e1, cnd)


def test_the_checker_rejects_a_flipped_sign_in_the_downdate():
    _rejects(65, 2, 1, flip=True)
    _rejects(130, 8, 2, flip=True)


def test_the_checker_rejects_chains_in_the_wrong_order():
    _rejects(65, 2, 3, reverse=True)
    _rejects(130, 8, 4, reverse=True)


def test_the_checker_rejects_a_carry_kept_between_passes():
    _rejects(65, 9, 5, keep_carry=True)
    _rejects(130, 9, 6, keep_carry=True)


def test_emulation_refuses_an_indefinite_downdate_and_changes_nothing():
    X, XT, y, e0, e1, pos, delta = _case(20, 2, 7)
    state = ref.whitened(X, XT, y, e0, LS)
    before = [a.copy() for a in state]
    p = pos[1]
    with pytest.raises(ref.Refused):
        ref.emulate(*state, pos, [delta[0], -(e0[p] + 1e-6) - 2.0])     # K_pp would go below zero
    for a, b in zip(state, before):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------ the Python layer
def _bare_gp(ind, n_total=50):
    from ital_amd import GaussianProcess, _lib
    gp = object.__new__(GaussianProcess)             # no device: the refusals come before any device work
    gp._lib = _lib.lib()
    gp.ind, gp.n_total, gp.m = list(ind), n_total, len(ind)
    gp.y = np.ones(len(ind))
    gp.appends = [len(ind)]
    gp.label_noise = np.zeros(len(ind))
    gp.store = None
    gp.length_scale, gp.var, gp.noise = 0.5, 1.0, 1e-6
    return gp


def test_reweigh_refuses_bad_arguments_and_changes_nothing():
    gp = _bare_gp([4, 9, 50, 17])                    # 50: a query row
    for ind, extra in (([5], 0.1), ([4, 4], 0.1), ([50], 0.1), ([4], -0.1), ([4], float("nan")), ([4], float("inf")),
                       ([4, 9], [0.1]), ([4, 9], [0.1, -1.0]), ([4, 5], [0.1, 0.1])):
        with pytest.raises(ValueError):
            gp.reweigh(ind, extra)
    assert np.array_equal(gp.label_noise, np.zeros(4)) and gp.ind == [4, 9, 50, 17]
    assert gp.reweigh([], 0.3) is gp                 # no-ops without a launch: a bare object has no device to launch on
    assert gp.reweigh([], []) is gp
    assert gp.reweigh([4, 17], 0.0) is gp
    gp.label_noise[1] = 0.25
    assert gp.reweigh([9], 0.25) is gp and gp.reweigh([9, 4], [0.25, 0.0]) is gp


def test_evidence_family_refuses_a_reweighed_model():
    gp = _bare_gp([4, 9])
    gp.label_noise[0] = 0.5
    for call in (gp.evidence, gp.evidence_grad, gp.loo_grad):
        with pytest.raises(ValueError, match="set_label_noise"):
            call([dict(length_scale=0.5)])
    from ital_amd import tune
    with pytest.raises(ValueError, match="set_label_noise"):
        tune.session_scores(gp, [dict(length_scale=0.5)])


def _bare_learner(gp):
    from ital_amd.retrieval_base import ActiveRetrievalBase
    L = object.__new__(ActiveRetrievalBase)
    L.__dict__.update(gp=gp, data=np.zeros((50, 3)), length_scale=0.5, var=1.0, noise=1e-6, rounds=2)
    L.relevant_ids, L.irrelevant_ids, L.unnameable_ids = {4, 9}, {17}, {30}
    return L


def test_state_dict_has_label_noise_only_when_there_is_some():
    gp = _bare_gp([4, 9, 17])
    L = _bare_learner(gp)
    sd = L.state_dict()
    assert "label_noise" not in sd and sd["version"] == 1
    assert sorted(sd) == sorted(["version", "n", "hyper", "ind", "y", "appends", "relevant_ids", "irrelevant_ids",
                                 "unnameable_ids", "rounds", "mvn_stream", "np_random"])     # what a session wrote before
    assert L.label_noise() == {}
    gp.label_noise[1] = 0.75
    sd = L.state_dict()
    assert sd["version"] == 1 and np.array_equal(sd["label_noise"], [0.0, 0.75, 0.0])
    assert sd["label_noise"] is not gp.label_noise
    assert L.label_noise() == {9: 0.75}
    for bad in ({30: 0.1}, {5: 0.1}, {4: 0.1, 31: 0.2}):     # unnameable, never seen, one good one bad
        with pytest.raises(ValueError):
            L.set_label_noise(bad)
    with pytest.raises(ValueError):
        L.set_label_noise({4: -1.0})
    assert np.array_equal(gp.label_noise, [0.0, 0.75, 0.0])
