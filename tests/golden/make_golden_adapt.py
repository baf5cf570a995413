#!/usr/bin/env python3
"""Generates the golden vectors of the AdaptAL learner (tests/test_adapt_host.py, tests/test_gpu_adapt.py) by running the
REAL reference's ital/adapt_al.py (/root/reference) -- in the build container only, like make_golden.py, whose shims it
reuses, plus the `warnings` module the reference's gp.py uses without importing it.  The reference itself is not modified;
its learner runs with parallelized=False (the serial path of information_density, the same arithmetic as the pool).

    python tests/golden/make_golden_adapt.py          # every fixture
    python tests/golden/make_golden_adapt.py NAME     # one fixture

Sessions: a query, then `rounds` times fetch_unlabelled(k) and update() with the fixture's own relevance as feedback.
Stored per fixture: hyper-parameters, the relevance vector, the feature rows unless a committed fixture has them
(`source`, `rows`), the reference's wall time of its fetches on the CPU that generated the file (for the record).
Stored per round r (`r<r>_*`): the candidate array after the subsample draw, predictive mean and variance at the
candidates, entropy, density, max_ind, the expected-error vector (empty on the early return), the returned list, `cond`
(LAPACK dpocon estimate of the candidate Gram) and `den_ref_vs_lapack`, the largest |density_ref - density_f| where
density_f comes from 1 / diag(inv) through LAPACK dpotrf + dtrtri on the same Gram.

A pick is only well defined where the reference's own boundaries are wider than arithmetic noise.  `accept_round` is the
condition every stored round meets (the generator refuses to write a fixture otherwise; tests/test_adapt_host.py restates
it on the stored vectors):
 (a) for every beta, with s the scores, S the k selected positions, R the rest:
     min_S (s - 100 e) > max_R (s + 100 e),  e = s (beta dH / H + (1 - beta) tol_den / density),
     dH = 2e-9 (|dH/dmean| + |dH/dvar|),  tol_den = max(1e-14 cond, 10 den_ref_vs_lapack);
 (b) every gap between neighbouring values of the sorted error vector exceeds 1e-6 relative;
 (c) max (|dH/dmean| + |dH/dvar|) <= 2.
"""
import os
import sys
import time
import warnings

os.environ.setdefault("OMP_NUM_THREADS", "8")

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

DEFAULT_BETAS = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0]

FIXTURES = {
    # name: data, rows, query, length scale, k, rounds, subsample, seed of numpy's global generator, learner kwargs
    "adapt_usps600_q3": dict(data="usps2007", rows=600, query=3, ls=3.0, k=4, rounds=3, subsample=None, seed=0, kw={}),
    "adapt_usps600_q17": dict(data="usps2007", rows=600, query=17, ls=3.0, k=4, rounds=3, subsample=None, seed=0, kw={}),
    "adapt_usps2007_sub500": dict(data="usps2007", rows=2007, query=5, ls=3.0, k=4, rounds=3, subsample=500, seed=0, kw={}),
    "adapt_synth300_k6": dict(data="synth", rows=300, query=None, ls=0.4, k=6, rounds=3, subsample=None, seed=0, kw={}),
    "adapt_synth300_betas": dict(data="synth", rows=300, query=None, ls=0.4, k=4, rounds=3, subsample=None, seed=0,
                                 kw=dict(betas=[0.25, 0.5, 0.75], var=2.0, noise=1e-4)),
    "adapt_synth300_b1": dict(data="synth", rows=300, query=None, ls=0.4, k=4, rounds=3, subsample=None, seed=0,
                              kw=dict(betas=[1.0])),
}


def sensitivities(mean, var):
    """|dH/dmean| and |dH/dvar| of the entropy of step 2 (analytic, clipping ignored)."""
    from scipy.stats import norm
    sd = np.sqrt(var)
    z = -mean / sd
    p = np.clip(norm.cdf(z), 1e-8, 1 - 1e-8)
    dHdp = np.log((1 - p) / p)
    return np.abs(dHdp * norm.pdf(z) / sd), np.abs(dHdp * norm.pdf(z) * mean / (2 * sd ** 3))


def accept_round(k, betas, mean, var, entropy, density, err, cond, den_ref_vs_lapack):
    """None if the round meets (a), (b), (c) of the module docstring, else the reason."""
    tol_den = max(1e-14 * cond, 10 * den_ref_vs_lapack)
    dm, dv = sensitivities(mean, var)
    if not (dm + dv).max() <= 2:
        return "(c) entropy sensitivity %.3g" % (dm + dv).max()
    dH = 2e-9 * (dm + dv)
    k = min(k, len(entropy))
    for beta in betas:
        s = (entropy ** beta) * (density ** (1. - beta))
        e = s * (beta * dH / entropy + (1 - beta) * tol_den / density)
        sel = np.argpartition(-s, k - 1)[:k]
        rest = np.setdiff1d(np.arange(len(s)), sel)
        if len(rest) and not (s[sel] - 100 * e[sel]).min() > (s[rest] + 100 * e[rest]).max():
            return "(a) beta %g: margin %.3g" % (beta, (s[sel] - 100 * e[sel]).min() - (s[rest] + 100 * e[rest]).max())
    if len(err) > 1:
        srt = np.sort(err)
        gap = (np.diff(srt) / np.abs(srt[:-1])).min()
        if not gap > 1e-6:
            return "(b) error gap %.3g" % gap
    return None


def synth():
    rng = np.random.RandomState(3)
    Z = rng.rand(300, 8)
    return Z, np.where(Z[:, 0] > 0.6, 1, -1)


def run_fixture(name):
    import make_golden
    make_golden.install_shims()
    import ital.gp as ref_gp
    ref_gp.warnings = warnings
    from ital.adapt_al import AdaptAL
    from scipy.linalg import lapack

    class Rec(AdaptAL):
        def fetch_unlabelled(self, k):
            self.log = {"ece": []}
            e0, d0, x0 = self.entropy, self.information_density, self.expected_classification_error

            def e(m, v):
                r = e0(m, v)
                self.log["ent"], self.log["mv"] = r, (m, v)
                return r

            def d(c):
                r = d0(c)
                self.log["den"], self.log["cand"] = r, c
                return r

            def x(*a):
                r = x0(*a)
                self.log["ece"].append(r)
                return r

            self.entropy, self.information_density, self.expected_classification_error = e, d, x
            try:
                return AdaptAL.fetch_unlabelled(self, k)
            finally:
                del self.entropy, self.information_density, self.expected_classification_error

    spec = FIXTURES[name]
    if spec["data"] == "usps2007":
        z = np.load(os.path.join(HERE, "usps2007.npz"))
        X, rel = z["X"][:spec["rows"]], z["rel"][:spec["rows"]]
        arrays = dict(source=np.array("usps2007.npz"), rows=np.int64(spec["rows"]))
    else:
        X, rel = synth()
        arrays = dict(X=X)
    query = int(np.argmax(rel)) if spec["query"] is None else spec["query"]
    kw = dict(spec["kw"])
    betas = kw.get("betas", DEFAULT_BETAS)
    np.random.seed(spec["seed"])
    learner = Rec(X, length_scale=spec["ls"], subsample=spec["subsample"], parallelized=False, **kw)
    learner.update({query: 1})
    arrays.update(rel=rel.astype(np.int8), query=np.int64(query), length_scale=np.float64(spec["ls"]),
                  var=np.float64(kw.get("var", 1.0)), noise=np.float64(kw.get("noise", 1e-6)), k=np.int64(spec["k"]),
                  subsample=np.int64(spec["subsample"] or 0), seed=np.int64(spec["seed"]), betas=np.array(betas, dtype=np.float64),
                  rounds=np.int64(spec["rounds"]))
    seconds = []
    for r in range(spec["rounds"]):
        t0 = time.perf_counter()
        ret = learner.fetch_unlabelled(spec["k"])
        seconds.append(time.perf_counter() - t0)
        log = learner.log
        cand = np.asarray(log["cand"])
        mean, var = log["mv"]
        K = learner.gp.K_all[np.ix_(cand, cand)] + learner.gp.noise * np.eye(len(cand))
        c, info = lapack.dpotrf(K, lower=1)
        assert info == 0
        rcond, _ = lapack.dpocon(c, np.abs(K).sum(axis=0).max(), uplo="L")
        li, info = lapack.dtrtri(c, lower=1)
        assert info == 0
        li = np.tril(li)
        den_f = np.log(np.diag(K) / np.maximum(1e-6, 1 / (li * li).sum(axis=0))) / 2
        dd = np.abs(log["den"] - den_f).max()
        cond = 1.0 / rcond
        k = min(spec["k"], len(cand))
        scores = np.stack([(log["ent"] ** b) * (log["den"] ** (1. - b)) for b in betas])
        max_ind = np.unique(np.argpartition(-scores, k - 1, axis=-1)[:, :k].ravel())
        err = np.array(log["ece"], dtype=np.float64)
        assert len(err) == (len(max_ind) if len(max_ind) > k else 0)
        why = accept_round(k, betas, mean, var, log["ent"], log["den"], err, cond, dd)
        print("%s round %d: nc %d, |max_ind| %d, cond %.2g, den_ref_vs_lapack %.2g, %.2f s: %s"
              % (name, r, len(cand), len(max_ind), cond, dd, seconds[-1], why or "accepted"), flush=True)
        if why:
            raise SystemExit("%s round %d refused: %s (change the query or the seed)" % (name, r, why))
        p = "r%d_" % r
        arrays.update({p + "cand": cand.astype(np.int64), p + "mean": mean, p + "var": var, p + "entropy": log["ent"],
                       p + "density": log["den"], p + "max_ind": max_ind.astype(np.int64), p + "err": err,
                       p + "ret": np.array(ret, dtype=np.int64), p + "cond": np.float64(cond),
                       p + "den_ref_vs_lapack": np.float64(dd)})
        learner.update({i: (1 if rel[i] > 0 else -1) for i in ret})
    arrays["ref_fetch_seconds"] = np.array(seconds)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(name + ".npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    for fixture in (sys.argv[1:] or list(FIXTURES)):
        run_fixture(fixture)
