"""What taking a label back would change (include/ital_influence.h, include/ital_ctx_audit.h; GaussianProcess.influence,
ActiveRetrievalBase.audit): everything that needs no GPU -- the model of tests/_influence_ref.py against itself, its checker
against planted mistakes, the declarations, their bindings and the refusals that come before any HIP call, and the arithmetic
of audit()'s probabilities.  The GPU side is tests/test_gpu_influence.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import _influence_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = {"ital_gp_influence", "ital_gp_influence_workspace", "ital_gp_preview_remove"}
DECL = r"\b(ital_[a-z_0-9]+)\s*\("


# ------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("m,n,seed", [(1, 9, 0), (2, 9, 1), (7, 23, 2), (12, 40, 3)])
def test_closed_form_equals_brute_force(m, n, seed):
    g = ref.gp_case(m, n, seed)
    c, w, B, mu1, s21 = ref.closed_form(g["L"], g["alpha"], g["V"], g["mu"], g["s2"])
    loo_mean, loo_var, bmu, bs2 = ref.brute_force(g["K"], g["Ks"], g["y"])
    K = g["K"].astype(np.float64)
    tol = 64 * m * float(np.finfo(np.longdouble).eps) * np.linalg.cond(K)
    assert np.abs(mu1 - bmu).max() <= tol * max(1.0, float(np.abs(bmu).max()))
    assert np.abs(s21 - bs2).max() <= tol
    assert np.abs((g["y"] - w / c) - loo_mean).max() <= tol * max(1.0, float(np.abs(loo_mean).max()))
    assert np.abs(1 / c - loo_var).max() <= tol
    if m == 1:
        assert np.abs(mu1).max() <= tol and np.abs(s21 - 1).max() <= tol      # the prior again


@pytest.fixture(scope="module")
def judged():
    """The float64 statement of the algorithm on one case per mask, with a selection: judged once, shared."""
    out = {}
    for mask in ref.MASKS:
        case = ref.Case(17, 129, mask=mask, poison=3.0)     # a finite poison, so that a planted out-of-range read shows as a number
        sel = ref.selection(case.m)
        out[mask] = (case, sel, ref.evaluate(case, sel))
    return out


@pytest.mark.parametrize("mask", ref.MASKS)
def test_checker_accepts_the_float64_evaluation(judged, mask):
    case, sel, res = judged[mask]
    ref.check(case, res, sel)


@pytest.mark.parametrize("m,n,mask", ref.grid())
def test_fixtures_have_no_ambiguous_flip(m, n, mask):
    """The condition under which the GPU test may demand the flips exactly."""
    case = ref.Case(m, n, mask=mask)
    res = ref.evaluate(case, ref.selection(m))
    ref.check(case, res, ref.selection(m))
    if m >= 2:
        assert ref.ambiguous_rows(case, res) == 0


@pytest.mark.parametrize("mistake", ref.MISTAKES)
def test_checker_rejects_a_planted_mistake(judged, mistake):
    mask = "random"
    case, sel, good = judged[mask]
    bad = ref.evaluate(case, sel, mistake=mistake)
    assert any(not np.array_equal(bad[k], good[k]) for k in ("stats", "mu_out", "s2_out")), "the mistake changed nothing"
    with pytest.raises(ref.Mismatch):
        ref.check(case, bad, sel)


def test_checker_judges_a_zero_pivot():
    case = ref.Case(17, 40, zero_pivot=5)
    res = ref.evaluate(case, [0, 5, 6, 16])
    ref.check(case, res, [0, 5, 6, 16])
    assert res["status"] == 1 and np.isnan(res["stats"][:6]).all() and np.isfinite(res["stats"][6:]).all()
    res["stats"][3] = 0.0                                   # a broken row that is not NaN
    with pytest.raises(ref.Mismatch):
        ref.check(case, res, [0, 5, 6, 16])


# --------------------------------------------------------------------------------------------------------------- the ABI
def test_influence_declarations_equal_bindings_and_are_exported():
    from ital_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "ital_influence.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(DECL, code)) == NAMES == set(_lib.INFLUENCE_SIGNATURES)
    audit = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ital_ctx_audit.h")).read(), flags=re.S)
    assert set(re.findall(DECL, audit)) == {"ital_ctx_audit"} == set(_lib.CTX_AUDIT_SIGNATURES)
    for name in dir(_lib):
        if name.endswith("SIGNATURES") and name not in ("INFLUENCE_SIGNATURES", "CTX_AUDIT_SIGNATURES"):
            assert not (NAMES | {"ital_ctx_audit"}) & set(getattr(_lib, name)), name
    assert "influence.hip" in build.SOURCES and "ctx_audit.hip" in build.SOURCES
    lib = _lib.lib()                                        # load() binds every table: the library exports the symbols
    for name, (res, args) in list(_lib.INFLUENCE_SIGNATURES.items()) + list(_lib.CTX_AUDIT_SIGNATURES.items()):
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    # the descriptor, field by field, against the header
    body = re.search(r"typedef struct ital_influence_desc \{(.*?)\} ital_influence_desc;", code, flags=re.S).group(1)
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    want = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            want.append((decl.split()[-1].lstrip("*"), ctypes.c_void_p if "*" in decl else kinds[decl.split()[0]]))
    assert want == list(_lib.ItalInfluenceDesc._fields_)


def _desc(**kw):
    """A descriptor of fake pointers that are never followed, sound except for what `kw` breaks."""
    from ital_amd import _lib
    P = 4096
    lib = _lib.lib()
    d = _lib.ItalInfluenceDesc()
    d.L, d.ldl, d.alpha, d.m, d.V, d.ldv, d.n, d.mu, d.s2, d.mask = P, 8, P, 5, P, 40, 33, P, P, None
    d.coef, d.stats, d.work, d.status = P, P, P, P
    d.work_doubles = lib.ital_gp_influence_workspace(5, 33)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


BROKEN = [dict(m=0), dict(m=-2), dict(n=-1), dict(ldl=4), dict(ldv=32), dict(L=None), dict(alpha=None), dict(V=None),
          dict(mu=None), dict(coef=None), dict(work=None), dict(status=None), dict(work_doubles=0)]


def test_influence_refuses_bad_arguments_without_touching_the_device():
    """Every case is decided before any HIP call: this test runs where there is no device at all."""
    from ital_amd import _lib
    lib = _lib.lib()
    assert lib.ital_gp_influence_workspace(5, 33) == 25 + 10 + 2 + 1 * 5 * 3
    assert lib.ital_gp_influence_workspace(5, 129) == 25 + 10 + 2 + 2 * 5 * 3
    assert lib.ital_gp_influence_workspace(0, 33) == 0 and lib.ital_gp_influence_workspace(5, -1) == 0
    assert lib.ital_gp_influence_workspace(5, 0) == 37

    def refused(rc, who):
        assert rc == -22
        assert who in lib.ital_last_error().decode()

    refused(lib.ital_gp_influence(None, None), "ital_gp_influence")
    for kw in BROKEN + [dict(stats=None), dict(work_doubles=lib.ital_gp_influence_workspace(5, 33) - 1)]:
        refused(lib.ital_gp_influence(ctypes.byref(_desc(**kw)), None), "ital_gp_influence")
    sel = (ctypes.c_int * 3)(0, 4, 2)
    P = 4096
    refused(lib.ital_gp_preview_remove(None, sel, 3, P, P, 40, None), "ital_gp_preview_remove")
    for kw in BROKEN + [dict(s2=None)]:
        refused(lib.ital_gp_preview_remove(ctypes.byref(_desc(**kw)), sel, 3, P, P, 40, None), "ital_gp_preview_remove")
    d = _desc()
    refused(lib.ital_gp_preview_remove(ctypes.byref(d), None, 3, P, P, 40, None), "ital_gp_preview_remove")
    refused(lib.ital_gp_preview_remove(ctypes.byref(d), sel, 3, None, P, 40, None), "ital_gp_preview_remove")
    refused(lib.ital_gp_preview_remove(ctypes.byref(d), sel, 3, P, None, 40, None), "ital_gp_preview_remove")
    refused(lib.ital_gp_preview_remove(ctypes.byref(d), sel, 0, P, P, 40, None), "ital_gp_preview_remove")
    refused(lib.ital_gp_preview_remove(ctypes.byref(d), sel, -1, P, P, 40, None), "ital_gp_preview_remove")
    refused(lib.ital_gp_preview_remove(ctypes.byref(d), sel, 3, P, P, 32, None), "ital_gp_preview_remove")       # ldo < n
    for entry in (5, -1):
        refused(lib.ital_gp_preview_remove(ctypes.byref(d), (ctypes.c_int * 3)(0, entry, 2), 3, P, P, 40, None),
                "sel entry outside")
    ids, table, count = (ctypes.c_int64 * 4)(), (ctypes.c_double * 32)(), ctypes.c_int(0)
    refused(lib.ital_ctx_audit(None, 1, ids, table, ctypes.byref(count), None), "ital_ctx_audit")


# ------------------------------------------------------------------------------------------- the probabilities of audit()
def test_disagreement_and_mistake_posterior_on_canned_arrays():
    from scipy.special import ndtr

    from ital_amd.retrieval_base import label_disagreement, mistake_posterior
    label = np.array([1.0, 1.0, -1.0, -1.0, 1.0])
    loo_mean = np.array([2.0, -2.0, 0.5, -0.5, 0.0])
    loo_var = np.array([1.0, 4.0, 0.25, 0.25, 9.0])
    d = label_disagreement(label, loo_mean, loo_var)
    assert np.allclose(d, [ndtr(-2.0), ndtr(1.0), ndtr(1.0), ndtr(-1.0), 0.5], rtol=0, atol=1e-16)
    assert d[1] == d[2] and d[0] < d[3] < d[4] < d[1]
    assert mistake_posterior(d, None) is None and mistake_posterior(d, 0.0) is None and mistake_posterior(d, 1.0) is None
    q = 0.1
    p = mistake_posterior(d, q)
    assert np.allclose(p, q * d / (q * d + (1 - q) * (1 - d)), rtol=1e-15, atol=0)
    assert p[4] == pytest.approx(q)                         # no evidence either way: the prior
    assert np.all(np.diff(p[np.argsort(d)]) >= 0)           # monotone in the disagreement
    assert mistake_posterior(np.array([0.0, 1.0]), q).tolist() == [0.0, 1.0]
    assert np.allclose(mistake_posterior(d, 0.5), d)        # an even prior returns the disagreement


def test_audit_and_preview_exist_on_the_base_class():
    from ital_amd.gp import GaussianProcess
    from ital_amd.retrieval_base import ActiveRetrievalBase
    for cls, names in ((GaussianProcess, ("influence", "preview_remove")), (ActiveRetrievalBase, ("audit", "preview_revoke"))):
        for name in names:
            assert callable(getattr(cls, name))
