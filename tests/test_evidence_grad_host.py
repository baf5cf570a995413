"""Host side of fitting a session's kernel parameters by evidence gradients (no device): the C declarations of
include/ital_evidence_grad.h against their bindings, the descriptor's fields, the argument checks that come before any HIP
call, and tune.maximize_lml / session_starts / fit_session_params against a numpy evaluator (tests/_evidence_grad_ref.py).
The GPU side is tests/test_gpu_evidence_grad.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import _evidence_grad_ref as ref  # noqa: E402

GRAD = ["ital_sqdist_lower", "ital_chol_gram_inverse_batched", "ital_gp_evidence_grad", "ital_gp_evidence_grad_workspace"]


def _header():
    header = open(os.path.join(ROOT, "include", "ital_evidence_grad.h")).read()
    return header, re.sub(r"/\*.*?\*/", "", header, flags=re.S)


def test_evidence_grad_declarations_equal_bindings_and_are_exported():
    from ital_amd import _lib
    _, code = _header()
    declared = set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", code))
    assert declared == set(GRAD) == set(_lib.EVIDENCE_GRAD_SIGNATURES), declared ^ set(_lib.EVIDENCE_GRAD_SIGNATURES)
    for other in (_lib.SIGNATURES, _lib.CTX_SIGNATURES, _lib.DENSE_SIGNATURES, _lib.ADAPT_SIGNATURES, _lib.REVOKE_SIGNATURES,
                  _lib.REWHITEN_SIGNATURES, _lib.EVIDENCE_SIGNATURES, _lib.INGEST_SIGNATURES, _lib.ROWS_SIGNATURES,
                  _lib.COMPACT_SIGNATURES):
        assert not declared & set(other)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in GRAD:
        assert hasattr(raw, name), name
    lib = _lib.load()
    for name, (res, args) in _lib.EVIDENCE_GRAD_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    # every declaration, argument by argument: pointers and the stream as void*, scalars by their C type
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    seen = set()
    for res_c, name, arglist in re.findall(r"\b(int|int64_t)\s+(ital_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", code):
        want_res, want_args = _lib.EVIDENCE_GRAD_SIGNATURES[name]
        assert want_res is kinds[res_c], name
        got = []
        for arg in [a.strip() for a in arglist.split(",")]:
            if "ital_evidence_grad_desc" in arg:
                got.append(ctypes.POINTER(_lib.ItalEvidenceGradDesc))
            elif "*" in arg or arg.startswith("hipStream_t"):
                got.append(ctypes.c_void_p)
            else:
                got.append(kinds[arg.split()[0]])
        assert got == want_args, name
        seen.add(name)
    assert seen == set(GRAD)
    for untouched in ("ital_hip.h", "ital_ctx.h", "ital_evidence.h"):
        text = open(os.path.join(ROOT, "include", untouched)).read()
        assert not any(name in text for name in GRAD)
    from ital_amd import build
    assert "evidence_grad.hip" in build.SOURCES
    assert os.path.realpath(os.path.join(ROOT, "include", "ital_evidence_grad.h")) in \
        [os.path.realpath(h) for h in build.headers()]


def test_evidence_grad_desc_fields_follow_the_header():
    """Same field names in the same order as the struct in the header, pointers as pointers, scalars by their C type."""
    from ital_amd import _lib
    header, _ = _header()
    body = re.search(r"typedef struct ital_evidence_grad_desc \{(.*?)\} ital_evidence_grad_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.search(r"([A-Za-z_0-9]+)$", d).group(1) for d in fields]
    assert names == [f[0] for f in _lib.ItalEvidenceGradDesc._fields_]
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for d, (name, ctype) in zip(fields, _lib.ItalEvidenceGradDesc._fields_):
        assert ctype is (ctypes.c_void_p if "*" in d else kinds[d.split()[0]]), name


def _desc(**kw):
    from ital_amd import _lib
    d = _lib.ItalEvidenceGradDesc()
    base = dict(XT=64, XTn=64, ldx=16, y=64, m=8, params=64, G=3, K=64, ld=8, values=64, grad=64, info=64, status=64, work=64,
                work_doubles=1 << 20, ev=None)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def test_entry_points_refuse_bad_arguments_without_a_device():
    """-22 before any HIP call, naming the entry point: NULL pointers, ldx % 16 != 0, ld < m, m < 1, G < 1 or > 65535, a
    workspace one double short."""
    from ital_amd import _lib
    lib = _lib.load()

    def refused(rc, who):
        assert rc == -22
        assert who in lib.ital_last_error().decode()

    need = lib.ital_gp_evidence_grad_workspace(8, 3)
    # M, alpha and the inverse diagonal of every candidate, the shared distances, two partials per candidate: at least
    assert need >= 3 * (8 * 8 + 2 * 8) + 8 * 8 + 3 * 2
    assert need > lib.ital_gp_evidence_workspace(8, 3)
    assert lib.ital_gp_evidence_grad_workspace(0, 3) == 0 and lib.ital_gp_evidence_grad_workspace(8, 0) == 0
    assert lib.ital_gp_evidence_grad_workspace(256, 1176) >= 1176 * 256 * 256       # no 32-bit overflow
    refused(lib.ital_gp_evidence_grad(None, None), "ital_gp_evidence_grad")
    for bad in (dict(XT=None), dict(XTn=None), dict(y=None), dict(params=None), dict(K=None), dict(values=None),
                dict(grad=None), dict(info=None), dict(status=None), dict(work=None), dict(ldx=0), dict(ldx=-16),
                dict(ldx=8), dict(ldx=24), dict(ld=7), dict(m=0), dict(m=-1), dict(G=0), dict(G=-2), dict(G=65536),
                dict(work_doubles=need - 1), dict(work_doubles=0)):
        refused(lib.ital_gp_evidence_grad(ctypes.byref(_desc(**bad)), None), "ital_gp_evidence_grad")

    good = dict(XT=64, XTn=64, m=8, ldx=16, D=64, ld=8)
    order = ("XT", "XTn", "m", "ldx", "D", "ld")
    for bad in (dict(XT=None), dict(XTn=None), dict(D=None), dict(ldx=0), dict(ldx=8), dict(ldx=24), dict(ld=7), dict(m=0),
                dict(m=-3)):
        a = dict(good, **bad)
        refused(lib.ital_sqdist_lower(*[a[k] for k in order], None), "ital_sqdist_lower")

    good = dict(M=64, n=8, count=3, info=None, W=64, ldw=8)
    order = ("M", "n", "count", "info", "W", "ldw")
    for bad in (dict(M=None), dict(W=None), dict(n=0), dict(count=0), dict(count=65536), dict(ldw=7)):
        a = dict(good, **bad)
        refused(lib.ital_chol_gram_inverse_batched(*[a[k] for k in order], None), "ital_chol_gram_inverse_batched")


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("m", [1, 127, 128, 129, 257])
def test_the_gradients_workspace_is_the_evidences_plus_distances_and_partials(m, G):
    """ital_gp_evidence's workspace: alpha and the inverse diagonals [G][m] each, M [G][m][m], four tables of G entries.
    ital_gp_evidence_grad's: that, then D [m][m] and two partials per candidate and lower pair of 128 x 128 tiles."""
    from ital_amd import _lib
    lib = _lib.load()
    tn = (m + 127) // 128
    pairs = tn * (tn + 1) // 2
    assert lib.ital_gp_evidence_workspace(m, G) == 2 * G * m + G * m * m + 4 * G
    assert lib.ital_gp_evidence_grad_workspace(m, G) - lib.ital_gp_evidence_workspace(m, G) == m * m + 2 * G * pairs


def test_every_learner_has_fit_params():
    import ital_amd
    from ital_amd import baselines
    from ital_amd.retrieval_base import ActiveRetrievalBase
    assert callable(ital_amd.GaussianProcess.evidence_grad)
    for cls in (ital_amd.ITAL, ital_amd.MCMI_min, ital_amd.AdaptAL, baselines.BorderlineSampling, baselines.EntropySampling):
        assert cls.fit_params is ActiveRetrievalBase.fit_params


# ------------------------------------------------------------------------------------------------------ maximize_lml
INIT = dict(length_scale=1.0, var=1.0, noise=1e-2)
CASES = [(40, 5), (120, 16), (200, 40)]


def _problem(m, d):
    X, y = ref.two_clusters(m, d, 100 * d + m)
    scale = float(np.sqrt(d / 12.0))
    init = dict(INIT, length_scale=scale)
    bounds = dict(length_scale=(0.05 * scale, 20.0 * scale), var=(0.1, 10.0), noise=(1e-6, 1.0))
    return X, y, init, bounds


def test_the_host_evaluators_gradient_is_the_derivative_of_its_value():
    """The reference itself, before anything is measured against it: central differences of its lml at h = 1e-5 in each
    log-parameter (truncation ~ h^2, rounding ~ eps |lml| / h: both below 1e-6 of the scale here)."""
    X, y, init, _ = _problem(40, 5)
    ev = ref.evaluator(X, y)
    theta = np.array([[init["length_scale"], 1.3, 0.05]])
    _, grad, ok = ev(theta)
    assert ok.all()
    h = 1e-5
    for k in range(3):
        up, dn = theta.copy(), theta.copy()
        up[0, k] *= np.exp(h)
        dn[0, k] *= np.exp(-h)
        fd = (ev(up)[0][0] - ev(dn)[0][0]) / (2 * h)
        assert abs(fd - grad[0, k]) <= 1e-6 * max(1.0, abs(grad[0, k])), (k, fd, grad[0, k])


@pytest.mark.parametrize("m,d", CASES)
def test_one_run_over_all_restarts_is_as_good_as_separate_runs(m, d):
    from scipy.optimize import minimize
    from ital_amd import tune
    X, y, init, bounds = _problem(m, d)
    starts = tune.session_starts(init, 8, bounds)
    assert starts.shape == (8, 3) and tuple(starts[0]) == (init["length_scale"], init["var"], init["noise"])
    calls = []
    ev = ref.evaluator(X, y, calls)
    best, lml, records = tune.maximize_lml(ev, starts, bounds, maxiter=100)
    assert len(records) == 8 and all(c <= 8 for c in calls)          # one call serves every restart
    assert records[0]["evaluations"] == len(calls)

    box = np.log(np.array([bounds[k] for k in tune.PARAM_NAMES]))
    separate = []
    for s in starts:
        def f(x):
            v, g, ok = ev(np.exp(x)[None, :])
            return (-v[0], -g[0]) if ok[0] else (np.inf, np.zeros(3))
        if not ev(s[None, :])[2][0]:
            continue
        r = minimize(f, np.log(s), jac=True, method="L-BFGS-B", bounds=[tuple(b) for b in box],
                     options=dict(tune.LBFGSB_OPTIONS, maxiter=100))
        separate.append(-float(r.fun))
    want = max(separate)
    lml0 = float(ev(starts[:1])[0][0])
    print("FIT m %d d %d: joint %.10g  separate %.10g  difference %.3g  init %.10g  best %r"
          % (m, d, lml, want, lml - want, lml0, best))
    assert lml >= want - 1e-6 * max(1.0, abs(want))
    assert lml >= lml0
    assert records[0]["lml"] >= lml0                                  # no restart reports less than its start
    got = ev(np.array([[best[k] for k in tune.PARAM_NAMES]]))[0][0]
    assert got == lml                                                 # the parameters returned are the ones that scored it
    for k, name in enumerate(tune.PARAM_NAMES):
        assert bounds[name][0] <= best[name] <= bounds[name][1]


@pytest.mark.parametrize("free", [("length_scale",), ("length_scale", "noise"), ("var",)])
def test_a_frozen_parameter_comes_back_bit_identical(free):
    from ital_amd import tune
    X, y, init, bounds = _problem(40, 5)
    init = dict(init, var=1.2345678901234567, noise=0.012345678901234567)
    starts = tune.session_starts(init, 8, bounds, free)
    seen = []

    def ev(theta, inner=ref.evaluator(X, y)):
        seen.append(np.array(theta))
        lml, grad, ok = inner(theta)
        grad = grad.copy()
        for k, name in enumerate(tune.PARAM_NAMES):
            if name not in free:
                grad[:, k] = np.nan                                   # a frozen component must be ignored
        return lml, grad, ok

    best, lml, records = tune.maximize_lml(ev, starts, bounds, free, maxiter=40)
    assert np.isfinite(lml)
    for k, name in enumerate(tune.PARAM_NAMES):
        if name not in free:
            assert best[name] == init[name]
            assert all(rec["params"][name] == rec["start"][name] for rec in records)
            assert all(np.array_equal(t[:, k], np.full(len(t), init[name])) for t in seen)
    assert lml >= ev(starts[:1])[0][0]


def test_a_restart_that_leaves_the_positive_definite_region_is_dropped():
    """A stub surface: lml = -sum (log theta - target)^2, whose region length_scale < 0.3 reports ok = False.  Restarts
    that start there, or walk into it, are dropped; the result comes from the survivors."""
    from ital_amd import tune
    target = np.log(np.array([2.0, 1.5, 0.1]))

    def stub(theta, wall=0.3):
        x = np.log(theta)
        lml = -((x - target) ** 2).sum(axis=1)
        grad = -2.0 * (x - target)
        ok = theta[:, 0] >= wall
        return np.where(ok, lml, -np.inf), np.where(ok[:, None], grad, np.nan), ok

    starts = np.array([[1.0, 1.0, 0.01], [0.1, 1.0, 0.01], [5.0, 2.0, 0.5], [0.2, 0.5, 0.1]])
    best, lml, records = tune.maximize_lml(stub, starts, maxiter=60)
    assert [r["dropped"] for r in records] == [False, True, False, True]
    assert lml > -1e-12 and abs(best["length_scale"] - 2.0) < 1e-5 and abs(best["noise"] - 0.1) < 1e-5
    assert records[1]["params"] is None and records[1]["lml"] == -np.inf

    # a restart that is fine where it starts and is dropped on its way: the optimum lies behind the wall for everyone
    far = lambda theta: stub(theta, wall=3.0)
    starts = np.array([[4.0, 1.0, 0.01], [10.0, 1.0, 0.01]])
    best, lml, records = tune.maximize_lml(far, starts, maxiter=60)
    assert all(r["dropped"] for r in records) and best is None and lml == -np.inf
    assert all(np.isfinite(r["lml"]) for r in records)               # what they reached before is still on record

    # all of them outside from the start
    best, lml, records = tune.maximize_lml(stub, np.array([[0.1, 1.0, 0.01], [0.2, 1.0, 0.1]]))
    assert best is None and lml == -np.inf and all(r["dropped"] for r in records)

    # one walks into the wall, the other one's hill is inside: the survivor resumes and arrives
    def two_hills(theta):
        x = np.log(theta)
        goal = np.where(theta[:, :1] > 1.0, np.log(np.array([[5.0, 1.0, 0.1]])), np.log(np.array([[0.1, 1.0, 0.1]])))
        ok = theta[:, 0] >= 0.3
        return np.where(ok, -((x - goal) ** 2).sum(axis=1), -np.inf), np.where(ok[:, None], -2.0 * (x - goal), np.nan), ok

    best, lml, records = tune.maximize_lml(two_hills, np.array([[0.9, 1.0, 0.01], [2.0, 2.0, 0.5]]), maxiter=60)
    assert [r["dropped"] for r in records] == [True, False]
    assert lml > -1e-10 and abs(best["length_scale"] - 5.0) < 1e-4


def test_session_starts_are_a_fixed_design_inside_the_bounds():
    from ital_amd import tune
    init = dict(length_scale=0.7, var=1.3, noise=1e-3)
    a, b = tune.session_starts(init, 8), tune.session_starts(init, 8)
    assert np.array_equal(a, b) and a.shape == (8, 3)
    lo, hi = (np.array([tune.DEFAULT_FIT_BOUNDS[k][j] for k in tune.PARAM_NAMES]) for j in (0, 1))
    assert tune.DEFAULT_FIT_BOUNDS["noise"][0] > 0
    assert np.all(a[1:] > lo) and np.all(a[1:] < hi) and np.all(a[:, 1] == 1.3)
    assert len(set(a[1:, 0])) == 4 and len(set(a[1:, 2])) == 2        # four length scales crossed with two noise levels
    ratios = np.sort(np.array(list(set(a[1:, 0]))))
    assert np.allclose(ratios[1:] / ratios[:-1], ratios[1] / ratios[0])      # log-spaced
    assert tune.session_starts(init, 1).shape == (1, 3)
    only_ls = tune.session_starts(init, 5, free=("length_scale",))
    assert only_ls.shape == (5, 3) and np.all(only_ls[:, 1] == 1.3) and np.all(only_ls[:, 2] == 1e-3)


class _StubSession(object):
    """Stands where a GaussianProcess would: evidence_grad from the host reference."""

    def __init__(self, X, y, **prm):
        self.length_scale, self.var, self.noise = prm["length_scale"], prm["var"], prm["noise"]
        self._ev = ref.evaluator(X, y)
        self.asked = 0

    def evidence_grad(self, params_list):
        self.asked += 1
        theta = np.array([[p["length_scale"], p["var"], p["noise"]] for p in params_list])
        lml, grad, ok = self._ev(theta)
        return dict(lml=lml, grad=grad, ok=ok)


def test_fit_session_params_touches_no_random_generator(capsys):
    from ital_amd import mvn_stream, tune
    X, y, init, bounds = _problem(40, 5)
    gp = _StubSession(X, y, **init)
    np.random.seed(3)
    np_state = np.random.get_state()
    mvn_state = (tuple(mvn_stream.GLOBAL.state), int(mvn_stream.GLOBAL.draws))
    recs = []
    best, lml = tune.fit_session_params(gp, bounds=bounds, maxiter=30, records=recs)
    now = np.random.get_state()
    assert now[0] == np_state[0] and np.array_equal(now[1], np_state[1]) and now[2:] == np_state[2:]
    assert (tuple(mvn_stream.GLOBAL.state), int(mvn_stream.GLOBAL.draws)) == mvn_state
    assert set(best) == set(tune.PARAM_NAMES) and len(recs) == 8 and gp.asked == recs[0]["evaluations"]
    assert recs[0]["start"] == init                                   # restart 0 is the session's current point
    assert lml >= gp.evidence_grad([init])["lml"][0]
    assert (gp.length_scale, gp.var, gp.noise) == (init["length_scale"], init["var"], init["noise"])
    assert capsys.readouterr().out == ""                              # verbose = 0 prints nothing
    # the same call twice: the same result
    assert tune.fit_session_params(gp, bounds=bounds, maxiter=30) == (best, lml)
    # a subset: only its names come back, and a learner is unwrapped
    holder = type("Learner", (), {"gp": gp})()
    part, lml1 = tune.fit_session_params(holder, ("length_scale",), bounds=bounds, maxiter=30, verbose=1)
    assert set(part) == {"length_scale"} and lml1 <= lml + 1e-9 * abs(lml)
    assert capsys.readouterr().out == "length_scale = {} : {:.4f}\n".format(part["length_scale"], lml1)
    with pytest.raises(TypeError, match="lengthscale"):
        tune.fit_session_params(gp, ("lengthscale",))
    with pytest.raises(ValueError):
        tune.fit_session_params(gp, ())
