"""Host side of fitting a session's kernel parameters by leave-one-out gradients (no device): the C declarations of
include/ital_loo_grad.h against their bindings, the descriptor's fields, the argument checks that come before any HIP call,
the host reference (tests/_loo_grad_ref.py) against central differences and two identities of its own, and
tune.fit_session_params / maximize_lml with the new criteria.  The GPU side is tests/test_gpu_loo_grad.py.

The reference is checked on two_clusters(m, 8, 3) -- the generator, dimension and seed of the session the fit is shown on --
for m in 17, 36, 64, 129 at the data's natural length scale sqrt(d / 12), var = 1 and noise = 1e-8, 1e-6, 1e-4, 1e-2."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import _loo_grad_ref as ref  # noqa: E402

LOO = ["ital_gp_loo_grad", "ital_gp_loo_grad_workspace"]


def _header():
    header = open(os.path.join(ROOT, "include", "ital_loo_grad.h")).read()
    return header, re.sub(r"/\*.*?\*/", "", header, flags=re.S)


def test_loo_grad_declarations_equal_bindings_and_are_exported():
    from ital_amd import _lib
    _, code = _header()
    declared = set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", code))
    assert declared == set(LOO) == set(_lib.LOO_GRAD_SIGNATURES), declared ^ set(_lib.LOO_GRAD_SIGNATURES)
    others = [getattr(_lib, name) for name in dir(_lib) if name.endswith("SIGNATURES") and name != "LOO_GRAD_SIGNATURES"]
    assert len(others) >= 11
    for other in others:
        assert not declared & set(other)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in LOO:
        assert hasattr(raw, name), name
    lib = _lib.load()
    for name, (res, args) in _lib.LOO_GRAD_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    # every declaration, argument by argument: pointers and the stream as void*, scalars by their C type
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    seen = set()
    for res_c, name, arglist in re.findall(r"\b(int|int64_t)\s+(ital_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", code):
        want_res, want_args = _lib.LOO_GRAD_SIGNATURES[name]
        assert want_res is kinds[res_c], name
        got = []
        for arg in [a.strip() for a in arglist.split(",")]:
            if "ital_loo_grad_desc" in arg:
                got.append(ctypes.POINTER(_lib.ItalLooGradDesc))
            elif "*" in arg or arg.startswith("hipStream_t"):
                got.append(ctypes.c_void_p)
            else:
                got.append(kinds[arg.split()[0]])
        assert got == want_args, name
        seen.add(name)
    assert seen == set(LOO)
    for untouched in ("ital_hip.h", "ital_ctx.h", "ital_evidence.h", "ital_evidence_grad.h"):
        text = open(os.path.join(ROOT, "include", untouched)).read()
        assert not any(name in text for name in LOO)
    from ital_amd import build
    assert "loo_grad.hip" in build.SOURCES
    assert os.path.realpath(os.path.join(ROOT, "include", "ital_loo_grad.h")) in \
        [os.path.realpath(h) for h in build.headers()]


def test_loo_grad_desc_fields_follow_the_header():
    """Same field names in the same order as the struct in the header, pointers as pointers, scalars by their C type."""
    from ital_amd import _lib
    header, _ = _header()
    body = re.search(r"typedef struct ital_loo_grad_desc \{(.*?)\} ital_loo_grad_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.search(r"([A-Za-z_0-9]+)$", d).group(1) for d in fields]
    assert names == [f[0] for f in _lib.ItalLooGradDesc._fields_]
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for d, (name, ctype) in zip(fields, _lib.ItalLooGradDesc._fields_):
        assert ctype is (ctypes.c_void_p if "*" in d else kinds[d.split()[0]]), name


def _desc(**kw):
    from ital_amd import _lib
    d = _lib.ItalLooGradDesc()
    base = dict(XT=64, XTn=64, ldx=16, y=64, m=8, params=64, G=3, K=64, ld=8, values=64, grad=64, info=64, status=64, work=64,
                work_doubles=1 << 20, ev=None)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def test_the_entry_point_refuses_bad_arguments_without_a_device():
    """-22 before any HIP call, naming the entry point: NULL pointers, ldx % 16 != 0, ld < m, m < 1, G < 1 or > 65535, a
    workspace one double short."""
    from ital_amd import _lib
    lib = _lib.load()
    need = lib.ital_gp_loo_grad_workspace(8, 3)
    assert lib.ital_gp_loo_grad_workspace(0, 3) == 0 and lib.ital_gp_loo_grad_workspace(8, 0) == 0
    assert lib.ital_gp_loo_grad_workspace(256, 1176) >= 2 * 1176 * 256 * 256       # no 32-bit overflow
    before = lib.ital_launch_count()
    bads = [None] + [_desc(**bad) for bad in (
        dict(XT=None), dict(XTn=None), dict(y=None), dict(params=None), dict(K=None), dict(values=None), dict(grad=None),
        dict(info=None), dict(status=None), dict(work=None), dict(ldx=0), dict(ldx=-16), dict(ldx=8), dict(ldx=24), dict(ld=7),
        dict(m=0), dict(m=-1), dict(G=0), dict(G=-2), dict(G=65536), dict(work_doubles=need - 1), dict(work_doubles=0))]
    for d in bads:
        assert lib.ital_gp_loo_grad(ctypes.byref(d) if d is not None else None, None) == -22
        assert "ital_gp_loo_grad" in lib.ital_last_error().decode()
    assert lib.ital_launch_count() == before


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("m", [1, 127, 128, 129, 257])
def test_the_workspace_is_the_evidences_plus_distances_inverse_partials_and_row_sums(m, G):
    """ital_gp_evidence's workspace, then D [m][m], W [G][m][m], two partials per candidate, operand, column tile and row,
    and r_i, s_i of the three parameters per candidate and row."""
    from ital_amd import _lib
    lib = _lib.load()
    tn = (m + 127) // 128
    assert lib.ital_gp_loo_grad_workspace(m, G) - lib.ital_gp_evidence_workspace(m, G) == \
        m * m + G * m * m + G * 2 * tn * m * 2 + G * m * 6


def test_every_learner_takes_a_criterion():
    import inspect
    import ital_amd
    from ital_amd import baselines, tune
    from ital_amd.retrieval_base import ActiveRetrievalBase
    assert callable(ital_amd.GaussianProcess.loo_grad) and callable(ital_amd.GaussianProcess.loo_grad_chunk)
    for cls in (ital_amd.ITAL, ital_amd.MCMI_min, ital_amd.AdaptAL, baselines.BorderlineSampling, baselines.EntropySampling):
        assert cls.fit_params is ActiveRetrievalBase.fit_params
    # appended after the existing keywords: every existing positional call means what it meant
    for fn in (tune.fit_session_params, ActiveRetrievalBase.fit_params):
        prm = list(inspect.signature(fn).parameters.values())
        assert prm[-1].name == "criterion" and prm[-1].default == "lml"


# ------------------------------------------------------------------------------------------------------ the reference
LS = float(np.sqrt(8 / 12.0))
REF_CASES = [(m, noise) for m in (17, 36, 64, 129) for noise in (1e-8, 1e-6, 1e-4, 1e-2)]


@pytest.mark.parametrize("m,noise", REF_CASES)
def test_the_reference_is_the_derivative_of_the_closed_form_criteria(m, noise):
    """Central differences of loo_logp and loo_mse at h = 1e-4 in each log-parameter: 1e-6 max(1, |g|), the project's bound
    for lml."""
    X, y = ref.two_clusters(m, 8, 3)
    D = ref.sqdist(X)
    theta = np.array([LS, 1.0, noise])
    got = ref.host_loo(D, y, *theta)
    h = 1e-4
    for k in range(3):
        up, dn = theta.copy(), theta.copy()
        up[k] *= np.exp(h)
        dn[k] *= np.exp(-h)
        a, b = ref.host_loo(D, y, *up, full=False), ref.host_loo(D, y, *dn, full=False)
        for name in ("logp", "mse"):
            fd = (a["loo_" + name] - b["loo_" + name]) / (2 * h)
            g = got["grad_" + name][k]
            print("LOO ref m %d noise %g %s[%d]: fd %.10g  closed form %.10g  deviation %.3g (bound 1e-06)"
                  % (m, noise, name, k, fd, g, abs(fd - g) / max(1.0, abs(g))))
            assert abs(fd - g) <= 1e-6 * max(1.0, abs(g)), (name, k, fd, g)


@pytest.mark.parametrize("m,noise", REF_CASES + [(36, 10.0)])
def test_scaling_var_and_noise_together(m, noise):
    """K -> t K scales c and alpha by 1 / t: d loo_logp / d log t = -m / 2 + 1/2 sum alpha_i^2 / c_i, and loo_mse does not
    move.  Both sides are sums of m terms of the size of the scales S: a few hundred roundings of them at the most."""
    X, y = ref.two_clusters(m, 8, 3)
    h = ref.host_loo(ref.sqdist(X), y, LS, 1.0, noise)
    want = -m / 2.0 + 0.5 * float(np.sum(h["alpha"] ** 2 / h["c"]))
    tol_logp = 1000 * 2.0 ** -52 * h["cond"] * max(1.0, h["scale_logp"][1] + h["scale_logp"][2])
    tol_mse = 1000 * 2.0 ** -52 * h["cond"] * max(1.0, h["scale_mse"][1] + h["scale_mse"][2])
    got_logp, got_mse = h["grad_logp"][1] + h["grad_logp"][2], h["grad_mse"][1] + h["grad_mse"][2]
    print("LOO ref identities m %d noise %g: logp %.3g (tol %.3g)  mse %.3g (tol %.3g)"
          % (m, noise, abs(got_logp - want), tol_logp, abs(got_mse), tol_mse))
    assert abs(got_logp - want) <= tol_logp
    assert abs(got_mse) <= tol_mse


# ------------------------------------------------------------------------------------------------- fit_session_params
class _NoDevice(object):
    """Stands where a GaussianProcess would: fit_session_params must refuse before it asks it for anything."""
    length_scale, var, noise = 0.5, 1.0, 1e-2

    def _asked(self, *args, **kw):
        raise AssertionError("the device was asked")

    evidence = evidence_grad = loo_grad = _asked


def test_fit_session_params_refuses_a_criterion_without_a_gradient_before_any_device_work():
    from ital_amd import tune
    with pytest.raises(ValueError, match="loo_ap"):
        tune.fit_session_params(_NoDevice(), criterion="loo_ap")
    with pytest.raises(ValueError, match="criterion"):
        tune.fit_session_params(_NoDevice(), criterion="ap")
    with pytest.raises(ValueError, match="fit at most one of var and noise"):
        tune.fit_session_params(_NoDevice(), criterion="loo_mse")
    with pytest.raises(ValueError, match="fit at most one of var and noise"):
        tune.fit_session_params(_NoDevice(), ("noise", "var"), criterion="loo_mse")
    holder = type("Learner", (), {"gp": _NoDevice()})()
    with pytest.raises(ValueError, match="fit at most one of var and noise"):
        tune.fit_session_params(holder, criterion="loo_mse")
    # the other checks keep their places
    with pytest.raises(TypeError, match="lengthscale"):
        tune.fit_session_params(_NoDevice(), ("lengthscale",), criterion="loo_logp")
    with pytest.raises(ValueError, match="no parameter"):
        tune.fit_session_params(_NoDevice(), (), criterion="loo_mse")


class _StubSession(object):
    """Stands where a GaussianProcess would: loo_grad from the host reference; evidence_grad must not be asked."""

    def __init__(self, X, y, **prm):
        self.length_scale, self.var, self.noise = prm["length_scale"], prm["var"], prm["noise"]
        self._D, self._y = ref.sqdist(X), y
        self.asked = 0

    def loo_grad(self, params_list):
        self.asked += 1
        rows = [ref.host_loo(self._D, self._y, p["length_scale"], p["var"], p["noise"], full=False) for p in params_list]
        out = {k: np.array([r[k] for r in rows]) for k in ("loo_logp", "loo_mse", "grad_logp", "grad_mse")}
        out["ok"] = np.ones(len(rows), dtype=bool)
        return out


def test_fit_session_params_climbs_the_criterion_it_is_given():
    from ital_amd import tune
    X, y = ref.two_clusters(36, 8, 3)
    init = dict(length_scale=LS, var=1.0, noise=1e-2)
    here = ref.host_loo(ref.sqdist(X), y, LS, 1.0, 1e-2, full=False)
    gp = _StubSession(X, y, **init)
    best, score = tune.fit_session_params(gp, restarts=4, maxiter=40, criterion="loo_logp")
    assert set(best) == set(tune.PARAM_NAMES) and gp.asked > 0 and score >= here["loo_logp"]
    assert score == ref.host_loo(ref.sqdist(X), y, best["length_scale"], best["var"], best["noise"], full=False)["loo_logp"]
    # loo_mse: minus the mse comes back, and var stays where it was
    best, score = tune.fit_session_params(gp, ("length_scale", "noise"), restarts=4, maxiter=40, criterion="loo_mse")
    assert set(best) == {"length_scale", "noise"} and score >= -here["loo_mse"] and score < 0
    assert score == -ref.host_loo(ref.sqdist(X), y, best["length_scale"], 1.0, best["noise"], full=False)["loo_mse"]
    assert (gp.length_scale, gp.var, gp.noise) == (LS, 1.0, 1e-2)


def test_maximize_lml_on_loo_logp_never_ends_below_its_start_and_is_stable():
    """The host's own margin for the device comparison of tests/test_gpu_loo_grad.py: with every output of the evaluator
    perturbed by 1e-12 relative the result moves by less than 1e-7 (1e-10 measured on a CPU)."""
    from ital_amd import tune
    X, y = ref.two_clusters(36, 8, 3)
    starts = tune.session_starts(dict(length_scale=LS, var=1.0, noise=1e-2), 8)
    ev = ref.evaluator(X, y)
    best, score, records = tune.maximize_lml(ev, starts)
    start_scores = ev(starts)[0]
    for r, rec in enumerate(records):
        assert rec["dropped"] or rec["lml"] >= start_scores[r]
    assert score >= start_scores[0] and score == max(rec["lml"] for rec in records if not rec["dropped"])
    assert tune.DEFAULT_FIT_BOUNDS["noise"][0] < best["noise"] < tune.DEFAULT_FIT_BOUNDS["noise"][1]      # an interior point
    _, moved, _ = tune.maximize_lml(ref.evaluator(X, y, perturb=1e-12), starts)
    print("LOO fit on the host: %.10g at %r from %.10g; perturbed by 1e-12: moves by %.3g (bound 1e-07)"
          % (score, best, start_scores[0], abs(moved - score)))
    assert abs(moved - score) < 1e-7
