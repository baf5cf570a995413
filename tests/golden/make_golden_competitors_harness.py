#!/usr/bin/env python3
"""End-to-end golden tables for TCAL and RBMAL: runs the REAL reference harness (utils.load_config +
run_experiment.run_retrieval_experiment) on tests/golden/conf/harness_tcal.conf and harness_rbmal.conf and stores the printed
AP / NDCG table plus every fetched batch and simulated feedback, like make_golden_harness.py.  Build container only.

    python tests/golden/make_golden_competitors_harness.py                    (finds a data seed, one process per run)
    python tests/golden/make_golden_competitors_harness.py harness_tcal       (one fixture on the data set as it is)

The data set is a small duplicate-free `Stored` one that this script writes (harness_competitors_data.npz: 160 x 6 train,
40 test, 3 classes) -- not Iris, whose duplicate rows tie.  Every fetch of a run has to meet the margin condition of
make_golden_competitors.py; a run that misses it exits with status 3 and the next data seed is tried.
"""
import io
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402
import make_golden_competitors as mc  # noqa: E402

NAMES = ["harness_tcal", "harness_rbmal"]
DATA = os.path.join(HERE, "harness_competitors_data.npz")


def write_data(seed):
    """Three overlapping classes in 6 dimensions, continuous features: no two rows are equal."""
    rng = np.random.default_rng(seed)
    centres = rng.random((3, 6))
    y = np.arange(200) % 3
    X = centres[y] + 0.35 * rng.normal(size=(200, 6))
    order = rng.permutation(200)
    X, y = X[order], y[order]
    assert len(np.unique(X, axis=0)) == 200
    np.savez_compressed(DATA, X_train=X[:160], y_train=y[:160], X_test=X[160:], y_test=y[160:], seed=seed)


def run(name):
    make_golden.install_shims()
    import matplotlib
    matplotlib.use("Agg")
    os.chdir(HERE)                                   # the conf names the data file relative to this directory
    import utils as ref_utils
    import run_experiment as ref_run
    conf = os.path.join(HERE, "conf", name + ".conf")
    km_log = mc.KMeansLog()
    config, dataset, learner = ref_utils.load_config(conf, "EXPERIMENT", {})
    trace, smallest = [], {}
    update = learner.update
    is_tcal = type(learner).__name__ == "TCAL"

    def logged_fetch(k):
        del learner.fetch_unlabelled                 # the instrumented round calls the learner's own method
        try:
            scratch = {}
            ret, margins = mc.tcal_round(learner, k, km_log, scratch, "") if is_tcal else mc.rbmal_round(learner, k, scratch, "")
        finally:
            learner.fetch_unlabelled = logged_fetch
        for what, gap in margins.items():
            if not (gap == 0.0 or gap >= mc.MARGIN):
                print("%s: fetch %d misses the %s margin: %g" % (name, len(trace), what, gap))
                sys.exit(3)
            if gap > 0:
                smallest[what] = min(smallest.get(what, np.inf), gap)
        trace.append(dict(ret=[int(i) for i in ret]))
        return ret

    def logged_update(fb):
        if trace and "fb" not in trace[-1] and len(fb) == len(trace[-1]["ret"]) and list(fb.keys()) == trace[-1]["ret"]:
            trace[-1]["fb"] = [int(v) for v in fb.values()]
        return update(fb)

    learner.fetch_unlabelled, learner.update = logged_fetch, logged_update
    buf = io.StringIO()
    stdout = sys.stdout
    sys.stdout = buf
    try:
        ref_run.run_retrieval_experiment(config, dataset, learner)
    finally:
        sys.stdout = stdout
    out = dict(table=buf.getvalue(), trace=trace, n_train=int(len(dataset.X_train_norm)),
               smallest_margins={w: float(g) for w, g in smallest.items()})
    with open(os.path.join(HERE, name + ".json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(name, "ok:", len(trace), "fetches, smallest non-zero margins", out["smallest_margins"])
    print(buf.getvalue())


if __name__ == "__main__":
    if len(sys.argv) > 1:
        run(sys.argv[1])
    else:
        for seed in range(100):
            write_data(seed)
            codes = [subprocess.call([sys.executable, os.path.abspath(__file__), n]) for n in NAMES]
            if codes == [0, 0]:
                print("data seed", seed)
                break
            if any(c != 3 for c in codes if c):
                raise SystemExit("a run failed for another reason than a margin")
        else:
            raise SystemExit("no data seed meets the margin condition")
