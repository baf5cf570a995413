#!/usr/bin/env python3
"""ital_gp_loo_grad -- the leave-one-out scores of G candidates with their gradients -- against ital_gp_evidence_grad, the
chain it stands next to (the yardstick: the six stages they share are the same launches), in one process, and
learner.fit_params(criterion='loo_logp') against learner.fit_params() end to end.

    python tools/loo_grad_bench.py [--repeats R] [--json FILE]

For m in (45, 256, 1024) and G in (1, 8, 64): both chains through GaussianProcess.evidence_grad / loo_grad with all G
candidates in one chunk, timed by the HIP events the library records between its stages (setup excluded for both: it comes
before the first event), medians of repeats that alternate between the two after a warm-up.  For m in (45, 256): the two
session-level fits end to end (apply=False), host wall clock after a synchronise, alternated likewise.  --json: every repeat."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ital_amd import ITAL, GaussianProcess, _lib, tune

GRAD_STAGES = ("gram_grid", "chol_batched", "chol_solve_batched", "inv_diag_batched", "sqdist", "product", "reduce")
LOO_STAGES = ("gram_grid", "chol_batched", "chol_solve_batched", "inv_diag_batched", "sqdist", "gram_inverse", "product", "reduce")


def candidates(d, G):
    scale = float(np.sqrt(d / 12.0))
    return [dict(length_scale=scale * (0.6 + 0.9 * g / max(1, G - 1)), var=1.0 + 0.25 * (g % 3), noise=10.0 ** -(1 + g % 3))
            for g in range(G)]


def marks(n):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
    for e in ev:
        e.record()                            # an event has a handle once it has been recorded
    return ev


def launches(fn):
    lib = _lib.lib()
    before = int(lib.ital_launch_count())
    fn()
    return int(lib.ital_launch_count()) - before


def chains(m, d, G, repeats):
    rng = np.random.default_rng(0)
    n = max(2 * m, 64)
    X = rng.random((n, d))
    ind = [int(i) for i in rng.choice(n, m, replace=False)]
    y = np.where(rng.random(m) < 0.4, 1.0, -1.0)
    gp = GaussianProcess(X, float(np.sqrt(d / 12.0)), noise=1e-2, device="cuda:0", capacity=m + 16)
    for at in range(0, m, 16):
        gp.update(ind[at:at + 16], y[at:at + 16])
    gp.check_status()
    cands = candidates(d, G)
    mg, ml = marks(len(GRAD_STAGES) + 1), marks(len(LOO_STAGES) + 1)
    big = 1 << 36
    a, b, e = gp.evidence_grad(cands, max_bytes=big), gp.loo_grad(cands, max_bytes=big), gp.evidence(cands, max_bytes=big)
    assert a["ok"].all() and b["ok"].all()                                          # warm-up, and the comparison
    assert np.array_equal(b["loo_logp"], e["loo_logp"]) and np.array_equal(b["loo_mse"], e["loo_mse"])
    gr = {s: [] for s in GRAD_STAGES}
    lo = {s: [] for s in LOO_STAGES}
    for _ in range(repeats):
        gp.evidence_grad(cands, max_bytes=big, events=mg)
        torch.cuda.synchronize()
        for k, s in enumerate(GRAD_STAGES):
            gr[s].append(mg[k].elapsed_time(mg[k + 1]))
        gp.loo_grad(cands, max_bytes=big, events=ml)
        torch.cuda.synchronize()
        for k, s in enumerate(LOO_STAGES):
            lo[s].append(ml[k].elapsed_time(ml[k + 1]))
    med = lambda xs: float(np.median(np.asarray(xs)))
    total = lambda st: [float(sum(st[s][r] for s in st)) for r in range(repeats)]
    return dict(m=m, d=d, G=G, repeats=repeats,
                evidence_grad_ms=med(total(gr)), loo_grad_ms=med(total(lo)),
                evidence_grad_stage_ms={s: med(gr[s]) for s in GRAD_STAGES}, loo_grad_stage_ms={s: med(lo[s]) for s in LOO_STAGES},
                evidence_grad_all_ms=gr, loo_grad_all_ms=lo,
                launches=dict(evidence_grad=launches(lambda: gp.evidence_grad(cands, max_bytes=big)),
                              loo_grad=launches(lambda: gp.loo_grad(cands, max_bytes=big)),
                              loo_grad_one_candidate=launches(lambda: gp.loo_grad(cands[:1], max_bytes=big))))


def session(m, d, repeats):
    rng = np.random.default_rng(1)
    n = max(4 * m, 256)
    X = np.concatenate((rng.normal(0, 0.5, (n // 2, d)), rng.normal(0, 0.5, (n - n // 2, d)) + 0.35))
    truth = np.where(np.arange(n) < n // 2, 1, -1)
    ids = [int(i) for i in rng.choice(n, m, replace=False)]
    A = ITAL(X, length_scale=float(np.sqrt(d / 12.0)), var=1.0, noise=1e-2, device="cuda:0")
    for at in range(0, m, 15):
        A.update({i: int(truth[i]) for i in ids[at:at + 15]})
    recs = []
    tune.fit_session_params(A, records=recs, criterion="loo_logp")
    by_lml, by_loo = A.fit_params(apply=False), A.fit_params(apply=False, criterion="loo_logp")
    at_lml = tune.session_scores(A, [by_lml[0]], "loo_logp")[0]
    tl, tf = [], []
    for _ in range(repeats):
        for fn, out in ((lambda: A.fit_params(apply=False), tl), (lambda: A.fit_params(apply=False, criterion="loo_logp"), tf)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
    return dict(m=m, d=d, repeats=repeats, fit_lml_ms=float(np.median(tl)), fit_loo_logp_ms=float(np.median(tf)),
                fit_lml_all_ms=tl, fit_loo_logp_all_ms=tf, fit_lml_best=by_lml[0], fit_lml_score=by_lml[1],
                loo_logp_at_fit_lml=at_lml, fit_loo_logp_best=by_loo[0], fit_loo_logp_score=by_loo[1],
                evaluations=recs[0]["evaluations"], iterations=recs[0]["iterations"],
                restarts_dropped=sum(r["dropped"] for r in recs))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loo_grad_bench needs a HIP device: nothing is timed without one")
    res = dict(chains=[], sessions=[])
    print("%5s %4s | %10s %10s %6s | %s" % ("m", "G", "lml grad", "loo grad", "ratio", "stages of loo_grad (ms)"))
    for m in (45, 256, 1024):
        for G in (1, 8, 64):
            r = chains(m, 64, G, a.repeats)
            res["chains"].append(r)
            print("%5d %4d | %8.3fms %8.3fms %6.2f | %s | launches %d / %d"
                  % (m, G, r["evidence_grad_ms"], r["loo_grad_ms"], r["loo_grad_ms"] / r["evidence_grad_ms"],
                     "  ".join("%s %.3f" % (s, r["loo_grad_stage_ms"][s]) for s in LOO_STAGES),
                     r["launches"]["evidence_grad"], r["launches"]["loo_grad"]), flush=True)
            assert r["launches"]["loo_grad"] == r["launches"]["loo_grad_one_candidate"]
    for m in (45, 256):
        r = session(m, 64, max(3, a.repeats // 2))
        res["sessions"].append(r)
        print("m %d: fit_params() %.2f ms -> lml %.4f at %r (loo_logp there %.4f); fit_params(criterion='loo_logp') %.2f ms "
              "(%d evaluations, %d dropped) -> loo_logp %.4f at %r"
              % (m, r["fit_lml_ms"], r["fit_lml_score"], r["fit_lml_best"], r["loo_logp_at_fit_lml"], r["fit_loo_logp_ms"],
                 r["evaluations"], r["restarts_dropped"], r["fit_loo_logp_score"], r["fit_loo_logp_best"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
