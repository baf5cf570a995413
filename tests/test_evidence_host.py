"""Host side of scoring hyper-parameter candidates against a session's own labels (no device): the C declarations of
include/ital_evidence.h against their bindings, the descriptor's fields, the argument checks that come before any HIP call,
and the parts of tune.session_scores / optimize_session_params / tune_params that need no GPU.  The GPU side is
tests/test_gpu_evidence.py."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")

EVIDENCE = ["ital_gram_grid", "ital_chol_inv_diag_batched", "ital_chol_inv_diag_batched_workspace", "ital_gp_evidence",
            "ital_gp_evidence_workspace"]


def test_evidence_declarations_equal_bindings_and_are_exported():
    from ital_amd import _lib
    header = open(os.path.join(ROOT, "include", "ital_evidence.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", code))
    assert declared == set(EVIDENCE) == set(_lib.EVIDENCE_SIGNATURES), declared ^ set(_lib.EVIDENCE_SIGNATURES)
    for other in (_lib.SIGNATURES, _lib.CTX_SIGNATURES, _lib.DENSE_SIGNATURES, _lib.ADAPT_SIGNATURES, _lib.REVOKE_SIGNATURES,
                  _lib.REWHITEN_SIGNATURES):
        assert not declared & set(other)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in EVIDENCE:
        assert hasattr(raw, name), name
    lib = _lib.load()
    for name, (res, args) in _lib.EVIDENCE_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    # every declaration, argument by argument: pointers and the stream as void*, scalars by their C type
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for res_c, name, arglist in re.findall(r"\b(int|int64_t)\s+(ital_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", code):
        want_res, want_args = _lib.EVIDENCE_SIGNATURES[name]
        assert want_res is kinds[res_c], name
        got = []
        for arg in [a.strip() for a in arglist.split(",")]:
            if "ital_evidence_desc" in arg:
                got.append(ctypes.POINTER(_lib.ItalEvidenceDesc))
            elif "*" in arg or arg.startswith("hipStream_t"):
                got.append(ctypes.c_void_p)
            else:
                got.append(kinds[arg.split()[0]])
        assert got == want_args, name
    for untouched in ("ital_hip.h", "ital_ctx.h"):
        text = open(os.path.join(ROOT, "include", untouched)).read()
        assert not any(name in text for name in EVIDENCE)
    from ital_amd import build
    assert "evidence.hip" in build.SOURCES
    assert os.path.realpath(os.path.join(ROOT, "include", "ital_evidence.h")) in [os.path.realpath(h) for h in build.headers()]


def test_evidence_desc_fields_follow_the_header():
    """Same field names in the same order as the struct in the header, pointers as pointers, scalars by their C type."""
    from ital_amd import _lib
    header = open(os.path.join(ROOT, "include", "ital_evidence.h")).read()
    body = re.search(r"typedef struct ital_evidence_desc \{(.*?)\} ital_evidence_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.search(r"([A-Za-z_0-9]+)$", d).group(1) for d in fields]
    assert names == [f[0] for f in _lib.ItalEvidenceDesc._fields_]
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for d, (name, ctype) in zip(fields, _lib.ItalEvidenceDesc._fields_):
        assert ctype is (ctypes.c_void_p if "*" in d else kinds[d.split()[0]]), name


def _desc(**kw):
    from ital_amd import _lib
    d = _lib.ItalEvidenceDesc()
    base = dict(XT=64, XTn=64, ldx=16, y=64, m=8, params=64, G=3, K=64, ld=8, scores=64, info=64, loo_mean=64, loo_var=64,
                ldm=8, status=64, work=64, work_doubles=1 << 20, ev=None)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def test_entry_points_refuse_bad_arguments_without_a_device():
    """-22 before any HIP call, naming the entry point: NULL pointers, ldx % 16 != 0, ld < m, ldm < m, m < 1, G < 1, a
    workspace that is too small."""
    from ital_amd import _lib
    lib = _lib.load()

    def refused(rc, who):
        assert rc == -22
        assert who in lib.ital_last_error().decode()

    need = lib.ital_gp_evidence_workspace(8, 3)
    assert need >= 3 * (8 * 8 + 2 * 8)            # M, alpha and the inverse diagonal of every candidate, at least
    assert lib.ital_gp_evidence_workspace(0, 3) == 0 and lib.ital_gp_evidence_workspace(8, 0) == 0
    assert lib.ital_gp_evidence_workspace(256, 1176) >= 1176 * 256 * 256       # no 32-bit overflow
    refused(lib.ital_gp_evidence(None, None), "ital_gp_evidence")
    for bad in (dict(XT=None), dict(XTn=None), dict(y=None), dict(params=None), dict(K=None), dict(scores=None),
                dict(info=None), dict(loo_mean=None), dict(loo_var=None), dict(status=None), dict(work=None), dict(ldx=0),
                dict(ldx=-16), dict(ldx=8), dict(ldx=24), dict(ld=7), dict(ldm=7), dict(m=0), dict(m=-1), dict(G=0),
                dict(G=-2), dict(G=65536), dict(work_doubles=need - 1), dict(work_doubles=0)):
        refused(lib.ital_gp_evidence(ctypes.byref(_desc(**bad)), None), "ital_gp_evidence")

    good = dict(XT=64, XTn=64, m=8, ldx=16, params=64, G=3, K=64, ld=8)
    order = ("XT", "XTn", "m", "ldx", "params", "G", "K", "ld")
    for bad in (dict(XT=None), dict(XTn=None), dict(params=None), dict(K=None), dict(ldx=0), dict(ldx=8), dict(ldx=24),
                dict(ld=7), dict(m=0), dict(G=0)):
        a = dict(good, **bad)
        refused(lib.ital_gram_grid(*[a[k] for k in order], None), "ital_gram_grid")

    wneed = lib.ital_chol_inv_diag_batched_workspace(8, 3)
    assert wneed == 3 * 8 * 8 and lib.ital_chol_inv_diag_batched_workspace(0, 3) == 0
    good = dict(L=64, ld=64, n=8, count=3, info=None, out=64, ldo=8, work=64, work_doubles=wneed)
    order = ("L", "ld", "n", "count", "info", "out", "ldo", "work", "work_doubles")
    for bad in (dict(L=None), dict(ld=None), dict(out=None), dict(work=None), dict(n=0), dict(count=0), dict(ldo=7),
                dict(work_doubles=wneed - 1)):
        a = dict(good, **bad)
        refused(lib.ital_chol_inv_diag_batched(*[a[k] for k in order], None), "ital_chol_inv_diag_batched")


def test_every_learner_has_tune_params():
    import ital_amd
    from ital_amd import baselines
    from ital_amd.retrieval_base import ActiveRetrievalBase
    assert callable(ital_amd.GaussianProcess.evidence)
    for cls in (ital_amd.ITAL, ital_amd.MCMI_min, ital_amd.AdaptAL, baselines.BorderlineSampling, baselines.EntropySampling):
        assert cls.tune_params is ActiveRetrievalBase.tune_params


class _NoDevice(object):
    """Stands where a GaussianProcess would: session_scores must refuse before it asks it for anything."""
    length_scale, var, noise = 0.1, 1.0, 1e-6

    def evidence(self, params_list):
        raise AssertionError("the device was asked")


def test_session_scores_argument_errors():
    from ital_amd import tune
    with pytest.raises(ValueError, match="criterion"):
        tune.session_scores(_NoDevice(), [{"length_scale": 1.0}], criterion="ap")
    with pytest.raises(TypeError, match="pdist"):
        tune.session_scores(_NoDevice(), [{"length_scale": 1.0, "pdist": None}])
    with pytest.raises(TypeError, match="lengthscale"):
        tune.session_scores(_NoDevice(), [{"length_scale": 1.0}, {"lengthscale": 2.0}], criterion="loo_mse")
    gp = _NoDevice()
    gp.y = np.ones(5)
    with pytest.raises(ValueError, match="both signs"):
        tune.session_scores(gp, [{"length_scale": 1.0}], criterion="loo_ap")


def test_session_search_follows_the_reference_trace(monkeypatch, capsys):
    """optimize_session_params over a stubbed scorer: the calls, the printed lines, the tie rule and the result are those of
    optimize_gp_params for the same score table (tests/golden/tune_trace.json, recorded from the reference's search)."""
    from ital_amd import tune
    with open(os.path.join(GOLD, "tune_trace.json")) as fh:
        trace = json.load(fh)
    table = {(r[0], r[1], r[2]): r[3] for r in trace["table"]}
    session = _NoDevice()
    for case in trace["cases"]:
        calls = []

        def stub(gp_or_learner, params_list, criterion="lml"):
            assert gp_or_learner is session and criterion == "loo_logp"
            keys = [(p["length_scale"], p.get("var", 1.0), p.get("noise", 1e-6)) for p in params_list]
            calls.extend(list(k) for k in keys)
            return [table[k] for k in keys]

        monkeypatch.setattr(tune, "session_scores", stub)
        best, perf = tune.optimize_session_params(session, tune.default_grids[case["grid"]], init=case["init"],
                                                  criterion="loo_logp", verbose=2)
        assert calls == case["calls"]
        assert capsys.readouterr().out == case["stdout"]
        assert best == case["best"] and perf == case["perf"]
        # the same table through optimize_gp_params: the same lines
        monkeypatch.setattr(tune, "cross_validate_gp", lambda dataset, relevance, p, n_folds=10:
                            table[(p["length_scale"], p.get("var", 1.0), p.get("noise", 1e-6))])
        assert tune.optimize_gp_params(np.eye(3), np.array([1, -1, 1]), tune.default_grids[case["grid"]], init=case["init"],
                                       verbose=2) == (best, perf)
        assert capsys.readouterr().out == case["stdout"]


def test_session_search_starts_from_the_session_and_takes_the_first_best(monkeypatch, capsys):
    from ital_amd import tune
    session = _NoDevice()
    session.length_scale = 2.0
    seen = []

    def stub(gp_or_learner, params_list, criterion="lml"):
        seen.append([dict(p) for p in params_list])
        return [5.0 if p["length_scale"] in (1.0, 3.0) else 1.0 for p in params_list]      # a tie between 1.0 and 3.0

    monkeypatch.setattr(tune, "session_scores", stub)
    grid = {"length_scale": [0.5, 1.0, 2.0, 3.0], "noise": [1e-6, 1e-4]}
    best, perf = tune.optimize_session_params(session, grid, verbose=0)
    assert best == {"length_scale": 1.0, "noise": 1e-6} and perf == 5.0
    # init = None: the first sweep holds the noise at the session's own value; `var`, which the grid does not name, is left out
    assert seen[0] == [{"length_scale": v, "noise": 1e-6} for v in grid["length_scale"]]
    assert seen[1] == [{"length_scale": 1.0, "noise": v} for v in grid["noise"]]
    assert capsys.readouterr().out == ""
