#!/usr/bin/env python3
"""Generates the golden vectors of the hyper-parameter search (tests/test_tune_host.py, tests/test_gpu_tune.py) by running
the REAL reference's optimize_parameters.py (/root/reference) -- in the build container only, like make_golden.py, whose
shims it reuses (numexpr -> numpy eval, ...), plus `np.infty = np.inf` (removed in NumPy 2) and the `warnings` module the
reference's gp.py uses without importing it.  The reference itself is not modified.

    python tests/golden/make_golden_tune.py          # every fixture

Fixtures:
  tune_iris.npz      Iris (reference datasets.py split), classes 0, 1, 2: ls_only and full grids at verbose=2
  tune_usps.npz      usps2007.npz (X, rel): ls_only, normal and fewshot
  tune_synth.npz     400 x 12 synthetic set with ~10 % relevance 0 (ls_only), and one regression cross_validate_gp call
  tune_trace.json    the reference's optimize_gp_params with cross_validate_gp replaced by a fixed table (control flow)
Stored per case: the test fold of every row, the AP of every evaluated grid value (in evaluation order), the per-fold
held-out scores and a per-fold condition estimate (dpocon) for at most three grid values, the chosen params, the best
perf and the captured stdout.
"""
import contextlib
import io
import json
import os
import sys
import warnings

os.environ.setdefault("OMP_NUM_THREADS", "8")

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

make_golden.install_shims()
np.infty = np.inf
import ital.gp as ref_gp  # noqa: E402

ref_gp.warnings = warnings
import optimize_parameters as ref  # noqa: E402
from scipy.linalg import lapack  # noqa: E402


def iris_dataset():
    from sklearn.datasets import load_iris
    from sklearn.model_selection import train_test_split
    d = load_iris()
    Xtr, _, ytr, _ = train_test_split(d.data, d.target, test_size=0.2, random_state=0)  # datasets.py:92
    return Xtr, ytr


class DS(object):
    def __init__(self, X, y=None):
        self.X_train = np.asarray(X, dtype=np.float64)
        self.X_train_norm = self.X_train
        self.y_train = y


def fold_ids(n, relevance, n_folds=10):
    from sklearn.model_selection import KFold, StratifiedKFold
    rows = np.arange(n)
    if relevance is not None:
        rows = rows[np.asarray(relevance) != 0]
        split = StratifiedKFold(n_folds, shuffle=True, random_state=0).split(np.zeros((len(rows), 1)), np.asarray(relevance)[rows])
    else:
        split = KFold(n_folds, shuffle=True, random_state=0).split(np.zeros((n, 1)))
    fid = np.full(n, -1, dtype=np.int32)
    for f, (_, test) in enumerate(split):
        fid[rows[test]] = f
    return fid


def per_fold(ds, relevance, params, fewshot=False, n_folds=10):
    """Held-out scores of every fold (rows by fold) and the dpocon condition estimate of every fold Gram, reference GP."""
    rows = np.arange(len(ds.X_train))
    rel = np.asarray(relevance)
    rows = rows[rel != 0]
    from sklearn.model_selection import StratifiedKFold
    gp = ref_gp.GaussianProcess(ds.X_train_norm, **params)
    scores = np.zeros(len(ds.X_train))
    conds = []
    fscore = []
    for f, (train, test) in enumerate(StratifiedKFold(n_folds, shuffle=True, random_state=0).split(ds.X_train_norm[rows], rel[rows])):
        fit, pred = (test, train) if fewshot else (train, test)
        gp.fit(rows[fit], rel[rows[fit]])
        s = gp.predict_stored(rows[pred])
        if fewshot:
            fscore.append(s)
        else:
            scores[rows[pred]] = s
        c, info = lapack.dpotrf(gp.K, True, False)
        anorm = np.abs(gp.K).sum(axis=0).max()
        rcond, _ = lapack.dpocon(c, anorm, uplo="L") if info == 0 else (0.0, 0)
        conds.append(1.0 / rcond if rcond > 0 else np.inf)
    return (np.concatenate(fscore) if fewshot else scores), np.array(conds)


def run_case(ds, relevance, grid, fewshot, verbose=2, n_folds=10, keep_scores=3):
    evaluated = []
    orig_gp, orig_fs = ref.cross_validate_gp, ref.cross_validate_fewshot

    def rec(fn):
        def wrapped(dataset, relevance, gp_params, n_folds=10):
            v = fn(dataset, relevance, gp_params, n_folds=n_folds)
            evaluated.append([gp_params['length_scale'], gp_params.get('var', 1.0), gp_params.get('noise', 1e-6), v])
            return v
        return wrapped

    ref.cross_validate_gp, ref.cross_validate_fewshot = rec(orig_gp), rec(orig_fs)
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            best, perf = ref.optimize_gp_params(ds, relevance, grid, n_folds=n_folds, fewshot=fewshot, verbose=verbose)
    finally:
        ref.cross_validate_gp, ref.cross_validate_fewshot = orig_gp, orig_fs
    ev = np.array(evaluated, dtype=np.float64)
    out = dict(evaluated=ev, best=np.array([best.get('length_scale'), best.get('var', np.nan), best.get('noise', np.nan)]),
               best_perf=np.float64(perf), stdout=np.array(buf.getvalue()))
    # per-fold scores for the best value and its two neighbours in evaluation order (at most three values)
    order = np.argsort(-ev[:, 3], kind="stable")[:keep_scores]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for r, i in enumerate(order):
            prm = dict(length_scale=ev[i, 0], var=ev[i, 1], noise=ev[i, 2])
            s, c = per_fold(ds, relevance, prm, fewshot=fewshot, n_folds=n_folds)
            out["scores%d_params" % r] = ev[i, :3]
            out["scores%d" % r] = s
            out["cond%d" % r] = c
    return out


def save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    print(name, os.path.getsize(path), "bytes")


def main():
    # (a) Iris
    X, y = iris_dataset()
    Xn = (X - X.min()) / (X.max() - X.min())
    ds = DS(Xn)
    arrays = dict(X=Xn, y=y)
    for lbl in (0, 1, 2):
        rel = 2 * (y == lbl) - 1
        arrays["c%d_folds" % lbl] = fold_ids(len(y), rel)
        for gname in ("ls_only", "full"):
            for k, v in run_case(ds, rel, ref.default_grids[gname], False).items():
                arrays["c%d_%s_%s" % (lbl, gname, k)] = v
    save("tune_iris.npz", **arrays)

    # (b) USPS, 2007 rows
    z = np.load(os.path.join(HERE, "usps2007.npz"))
    ds = DS(z["X"])
    rel = z["rel"]
    arrays = dict(folds=fold_ids(len(rel), rel))
    for tag, fs in (("normal", False), ("fewshot", True)):
        for k, v in run_case(ds, rel, ref.default_grids["ls_only"], fs, verbose=2).items():
            arrays["%s_%s" % (tag, k)] = v
    save("tune_usps.npz", **arrays)

    # (c) synthetic with relevance 0, plus regression
    rng = np.random.default_rng(400)
    Xs = rng.random((400, 12))
    rel = np.where(Xs[:, 0] + 0.3 * Xs[:, 1] > 0.8, 1, -1)
    rel[rng.random(400) < 0.1] = 0
    ds = DS(Xs, y=np.sin(3 * Xs[:, 0]) + Xs[:, 2])
    arrays = dict(X=Xs, rel=rel, y=ds.y_train, folds=fold_ids(400, rel))
    for k, v in run_case(ds, rel, ref.default_grids["ls_only"], False, verbose=2).items():
        arrays["ls_" + k] = v
    reg_params = dict(length_scale=0.5, var=1.0, noise=1e-3)
    arrays["reg_params"] = np.array([0.5, 1.0, 1e-3])
    arrays["reg_value"] = np.float64(ref.cross_validate_gp(ds, None, reg_params))
    arrays["reg_folds"] = fold_ids(400, None)
    save("tune_synth.npz", **arrays)

    # (d) control-flow trace: cross_validate_gp replaced by a fixed table (ties included)
    grid = ref.default_grids["full"]
    table = {}
    rs = np.random.RandomState(7)
    for ls in grid["length_scale"]:
        for var in grid["var"]:
            for noise in grid["noise"]:
                table[(ls, var, noise)] = float(np.round(rs.rand() * 0.5 + 0.1 * (ls in (2.0, 2.5)), 2))
    cases = []
    for gname, init in (("full", dict(ref.default_init)), ("ls_only", dict(ref.default_init)),
                        ("full", dict(length_scale=2.0, var=0.5, noise=1e-3))):
        calls = []

        def stub(dataset, relevance, gp_params, n_folds=10):
            key = (gp_params["length_scale"], gp_params.get("var", 1.0), gp_params.get("noise", 1e-6))
            calls.append(list(key))
            return table[key]

        orig = ref.cross_validate_gp
        ref.cross_validate_gp = stub
        buf = io.StringIO()
        try:
            with contextlib.redirect_stdout(buf):
                best, perf = ref.optimize_gp_params(DS(np.eye(3)), np.array([1, -1, 1]), ref.default_grids[gname],
                                                    init=init, verbose=2)
        finally:
            ref.cross_validate_gp = orig
        cases.append(dict(grid=gname, init=init, calls=calls, stdout=buf.getvalue(), best=best, perf=perf))
    with open(os.path.join(HERE, "tune_trace.json"), "w") as fh:
        json.dump(dict(table=[[k[0], k[1], k[2], v] for k, v in table.items()], cases=cases), fh)
    print("tune_trace.json", os.path.getsize(os.path.join(HERE, "tune_trace.json")), "bytes")


if __name__ == "__main__":
    main()
