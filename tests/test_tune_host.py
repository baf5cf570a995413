"""Host-side logic of ital_amd.tune (no device): the alternating search against the reference's control flow, the folds,
the C declarations of the dense kernels against their bindings, the CLI arguments, pdist refusal."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")


def test_alternating_search_reproduces_reference_trace(monkeypatch, capsys):
    from ital_amd import tune
    with open(os.path.join(GOLD, "tune_trace.json")) as fh:
        trace = json.load(fh)
    table = {(r[0], r[1], r[2]): r[3] for r in trace["table"]}
    for case in trace["cases"]:
        calls = []

        def stub(dataset, relevance, gp_params, n_folds=10):
            key = (gp_params["length_scale"], gp_params.get("var", 1.0), gp_params.get("noise", 1e-6))
            calls.append(list(key))
            return table[key]

        monkeypatch.setattr(tune, "cross_validate_gp", stub)
        best, perf = tune.optimize_gp_params(np.eye(3), np.array([1, -1, 1]), tune.default_grids[case["grid"]],
                                             init=case["init"], verbose=2)
        assert calls == case["calls"]
        assert capsys.readouterr().out == case["stdout"]
        assert best == case["best"] and perf == case["perf"]


def test_folds_equal_reference_folds():
    from ital_amd import tune
    z = np.load(os.path.join(GOLD, "tune_iris.npz"))
    for c in (0, 1, 2):
        rel = 2 * (z["y"] == c) - 1
        rows, folds = tune.fold_split(z["X"], rel, 10)
        fid = np.full(len(rel), -1)
        for f, (tr, te) in enumerate(folds):
            fid[rows[te]] = f
        assert np.array_equal(fid, z["c%d_folds" % c])
    s = np.load(os.path.join(GOLD, "tune_synth.npz"))
    rows, folds = tune.fold_split(s["X"], s["rel"], 10)
    assert np.array_equal(rows, np.nonzero(s["rel"] != 0)[0])
    fid = np.full(len(s["rel"]), -1)
    for f, (tr, te) in enumerate(folds):
        fid[rows[te]] = f
    assert np.array_equal(fid, s["folds"])
    rows, folds = tune.fold_split(s["X"], None, 10)
    fid = np.full(len(s["rel"]), -1)
    for f, (tr, te) in enumerate(folds):
        fid[rows[te]] = f
    assert np.array_equal(fid, s["reg_folds"])


DENSE = ["ital_gram_rows", "ital_chol_batched", "ital_chol_solve_batched", "ital_kernel_matvec",
         "ital_kernel_matvec_workspace"]


def _ctype_of(decl):
    decl = decl.strip()
    if "*" in decl:
        return ctypes.c_void_p
    base = " ".join(w for w in decl.split()[:-1] if w != "const")
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "hipStream_t": ctypes.c_void_p}[base]


def test_dense_declarations_equal_bindings():
    from ital_amd import _lib
    header = open(os.path.join(ROOT, "include", "ital_dense.h")).read()
    assert set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", header)) == set(DENSE) == set(_lib.DENSE_SIGNATURES)
    assert not set(DENSE) & set(_lib.SIGNATURES)
    for name in DENSE:
        m = re.search(r"\b(int|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        res = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}[m.group(1)]
        args = [_ctype_of(a) for a in m.group(2).split(",")]
        want_res, want_args = _lib.DENSE_SIGNATURES[name]
        assert res is want_res, name
        assert args == want_args, name


def test_cli_arguments_parse_as_reference(capsys):
    from ital_amd import tune
    assert tune.parse_args(["a.conf", "--grid=ls_only", "--n_folds=5"]) == ("a.conf", {"grid": "ls_only", "n_folds": "5"})
    assert tune.parse_args(["--few_shot=yes", "b.conf"]) == ("b.conf", {"few_shot": "yes"})
    assert tune.parse_args(["a.conf", "--HELP"]) == (None, {})
    assert tune.parse_args(["--query_classes=1 2=3"]) == (None, {"query_classes": "1 2=3"})
    with pytest.raises(SystemExit):
        tune.parse_args(["a.conf", "b.conf"])
    assert "Unexpected argument: b.conf" in capsys.readouterr().out
    assert tune.main([]) is None
    assert "Usage:" in capsys.readouterr().out


def test_defaults_equal_reference():
    from ital_amd import tune
    assert list(tune.default_grids) == ["full", "ls_only"]
    assert list(tune.default_grids["full"]) == ["length_scale", "var", "noise"]
    assert len(tune.default_grids["full"]["length_scale"]) == 21 and tune.default_grids["full"]["noise"][0] == 1e-8
    assert tune.default_init == {"length_scale": 0.1, "var": 1.0, "noise": 1e-6}


def test_pdist_is_refused():
    from ital_amd import tune
    X = np.random.default_rng(0).random((20, 3))
    rel = np.where(X[:, 0] > 0.5, 1, -1)
    with pytest.raises(NotImplementedError):
        tune.cross_validate_gp(X, rel, dict(length_scale=1.0, pdist=np.zeros((20, 20))))
    with pytest.raises(NotImplementedError):
        tune.cross_validate_fewshot(X, rel, dict(length_scale=1.0, pdist=None))
