#!/usr/bin/env python3
"""GaussianProcess.evidence -- log marginal likelihood and leave-one-out scores of G hyper-parameter candidates against the
m labels of a session -- on the device, against a host evaluation of the same quantities (scipy cho_factor / cho_solve /
solve_triangular on the downloaded XT and y, with the threads the BLAS takes): the only way to get these numbers without
ital_gp_evidence.  Device time is measured with HIP events around the whole call (uploads, every chunk, downloads), after a
warm-up, as the median of repeats alternated with the host's; the host wall clock around the call is printed next to it.

Also reported: the kernel launches of one ital_gp_evidence call at G = 21 and at G = 1176 for this m (they must be equal),
and the time of each of the five stages from events the library records between them (one chunk holding all G).

    python tools/evidence_bench.py m d G [--repeats R] [--host-repeats H] [--json FILE]

The grid is the first G values of the product grid of tune.default_grids['full'] (length scale fastest), the length scales
scaled by sqrt(d / 12) so that they bracket the data's own scale.  --json appends the run, with every repeat, to FILE."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ital_amd import GaussianProcess, _lib, tune

STAGES = ("gram_grid", "chol_batched", "chol_solve_batched", "inv_diag_batched", "reduce")


def candidates(d, G):
    full = tune.default_grids['full']
    scale = float(np.sqrt(d / 12.0))
    out = []
    for noise in full['noise']:
        for var in full['var']:
            for ls in full['length_scale']:
                out.append(dict(length_scale=ls * scale, var=var, noise=noise))
    if G > len(out):
        sys.exit("the full product grid has %d candidates" % len(out))
    return out[:G]


def host_evidence(X, y, cands):
    """What gp.evidence returns, on the host."""
    import scipy.linalg as sl
    m = len(X)
    sn = (X * X).sum(axis=1)
    D = sn[:, None] + sn[None, :] - 2.0 * (X @ X.T)
    eye = np.eye(m)
    out = dict(lml=np.empty(len(cands)), loo_logp=np.empty(len(cands)), loo_mse=np.empty(len(cands)),
               ok=np.zeros(len(cands), dtype=bool))
    for g, c in enumerate(cands):
        K = c['var'] * np.exp(D / (-2.0 * c['length_scale'] ** 2)) + c['noise'] * eye
        try:
            cf = sl.cho_factor(K, lower=True)
        except np.linalg.LinAlgError:
            out['lml'][g] = out['loo_logp'][g] = -np.inf
            out['loo_mse'][g] = np.inf
            continue
        alpha = sl.cho_solve(cf, y)
        Minv = sl.solve_triangular(cf[0], eye, lower=True)
        cd = (Minv * Minv).sum(axis=0)
        r, v = alpha / cd, 1.0 / cd
        out['ok'][g] = True
        out['lml'][g] = -0.5 * (y @ alpha) - np.log(np.diag(cf[0])).sum() - 0.5 * m * np.log(2 * np.pi)
        out['loo_logp'][g] = (-0.5 * np.log(v) - r * r / (2 * v) - 0.5 * np.log(2 * np.pi)).sum()
        out['loo_mse'][g] = np.mean(r * r)
    return out


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    res = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0, res


def launches(gp, cands):
    lib = _lib.lib()
    before = int(lib.ital_launch_count())
    gp.evidence(cands, max_bytes=1 << 36)
    return int(lib.ital_launch_count()) - before


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("m", type=int)
    ap.add_argument("d", type=int)
    ap.add_argument("G", type=int)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("evidence_bench needs a HIP device: nothing is timed without one")
    m, d, G = a.m, a.d, a.G
    rng = np.random.default_rng(0)
    n = max(2 * m, 64)
    X = rng.random((n, d))
    ind = [int(i) for i in rng.choice(n, m, replace=False)]
    y = np.where(rng.random(m) < 0.4, 1.0, -1.0)
    gp = GaussianProcess(X, float(np.sqrt(d / 12.0)), noise=1e-4, device="cuda:0", capacity=m + 16)
    for at in range(0, m, 16):
        gp.update(ind[at:at + 16], y[at:at + 16])
    gp.check_status()
    cands = candidates(d, G)
    Xh = gp.XT[:m, :d].cpu().numpy()

    dev = gp.evidence(cands)                  # warm-up of both sides, and the comparison
    host = host_evidence(Xh, gp.y, cands)
    both = dev['ok'] & host['ok']
    dev_rel = {k: float(np.max(np.abs(dev[k][both] - host[k][both]) / np.maximum(1.0, np.abs(host[k][both]))))
               if both.any() else None for k in ('lml', 'loo_logp', 'loo_mse')}

    td, wd, th = [], [], []
    for r in range(a.repeats):
        ev, wall, _ = timed(lambda: gp.evidence(cands))
        td.append(ev)
        wd.append(wall)
        if r < a.host_repeats:
            t0 = time.perf_counter()
            host_evidence(Xh, gp.y, cands)
            th.append(time.perf_counter() - t0)

    # the five stages of one call that holds all G candidates
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    for e in marks:
        e.record()                            # an event has a handle once it has been recorded
    stages = {s: [] for s in STAGES}
    for _ in range(a.repeats):
        gp.evidence(cands, max_bytes=1 << 36, events=marks)
        torch.cuda.synchronize()
        for k, s in enumerate(STAGES):
            stages[s].append(marks[k].elapsed_time(marks[k + 1]) * 1e-3)
    n21, n1176 = launches(gp, candidates(d, 21)), launches(gp, candidates(d, 1176))

    med = lambda xs: float(np.median(np.asarray(xs)))
    res = dict(m=m, d=d, ldx=gp.ldx, G=G, repeats=a.repeats, host_repeats=len(th), chunk=min(G, gp.evidence_chunk()),
               positive_definite=int(dev['ok'].sum()), host_positive_definite=int(host['ok'].sum()),
               max_deviation_from_host=dev_rel,
               device_ms=med(td) * 1e3, device_all_ms=[t * 1e3 for t in td], device_wall_ms=med(wd) * 1e3,
               host_ms=med(th) * 1e3, host_all_ms=[t * 1e3 for t in th], host_threads=int(os.environ.get("OMP_NUM_THREADS", 0)),
               stage_ms={s: med(stages[s]) * 1e3 for s in STAGES}, stage_all_ms={s: [t * 1e3 for t in stages[s]] for s in STAGES},
               launches_per_call={"G=21": n21, "G=1176": n1176})
    print("m=%d d=%d (ldx %d) G=%d, %d candidates positive definite; chunks of %d" % (m, d, gp.ldx, G, res["positive_definite"],
                                                                                     res["chunk"]))
    print("gp.evidence      %10.3f ms (events; min %.3f max %.3f)  %10.3f ms (host wall)"
          % (res["device_ms"], min(td) * 1e3, max(td) * 1e3, res["device_wall_ms"]))
    print("host evaluation  %10.3f ms (wall; min %.3f max %.3f)   host / device = %.2fx"
          % (res["host_ms"], min(th) * 1e3, max(th) * 1e3, res["host_ms"] / res["device_ms"]))
    for s in STAGES:
        print("  stage %-20s %10.3f ms" % (s, res["stage_ms"][s]))
    print("launches per ital_gp_evidence call: %d at G = 21, %d at G = 1176" % (n21, n1176))
    print("largest deviation from the host, relative to max(1, |value|): %r" % (dev_rel,))
    if a.json:
        runs = []
        if os.path.exists(a.json):
            with open(a.json) as f:
                runs = json.load(f)
        runs.append(res)
        with open(a.json, "w") as f:
            json.dump(runs, f, indent=1)


if __name__ == "__main__":
    main()
