#!/usr/bin/env python3
"""The live-session calls of the context layer (include/ital_ctx_live.h) against the only route a C host had before them:
a new context on the resulting rows (ital_ctx_create + ital_ctx_fit, every row uploaded again) and a replay of the labels
(ital_ctx_update: one sweep over all rows per 16 labels).  One process, host wall clock -- every call of either route
synchronises before it returns -- one warm-up of each route, then medians of alternated repeats:

  add_rows(r)      r new rows                         vs  rebuild on n + r rows
  remove_rows(r)   r scattered unlabelled rows        vs  rebuild on n - r rows
  set_params       other length scale, variance, noise vs rebuild on n rows with those parameters
  evidence(G)      G candidates scored                 (no counterpart: a rebuild per candidate yields a model, not a score;
                                                        the rebuild on n rows is printed next to it for scale)

    python tools/ctx_live_bench.py [n d labels r G] [--repeats R]        (default 9298 256 45 64 21)

Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ital_amd import _lib


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("shape", type=int, nargs="*", default=[9298, 256, 45, 64, 21])
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if len(a.shape) != 5:
        ap.error("n d labels r G")
    if not torch.cuda.is_available():
        sys.exit("ctx_live_bench needs a HIP device: nothing is timed without one")
    n, d, m, r, G = a.shape
    torch.cuda.init()
    lib = _lib.load()
    rng = np.random.default_rng(0)
    X = rng.random((n + r, d))
    ls = float(np.sqrt(d / 12.0))
    labelled = rng.choice(n, m, replace=False).astype(np.int64)
    y = np.where(X[labelled, 0] > 0.5, 1.0, -1.0)
    gone = np.sort(rng.choice(np.setdiff1d(np.arange(n), labelled), r, replace=False)).astype(np.int64)
    keep = np.delete(np.arange(n), gone)
    new_id = np.full(n, -1, dtype=np.int64)
    new_id[keep] = np.arange(len(keep))
    other = (ls * 1.5, 0.7, 1e-4)
    grid = np.ascontiguousarray([[ls * f, 1.0, 1e-6] for f in np.geomspace(0.25, 4.0, G)])

    def check(rc):
        if rc != 0:
            sys.exit("%d: %s" % (rc, lib.ital_last_error().decode()))

    def build(rows, ids, params=(ls, 1.0, 1e-6)):
        """create + fit + the labels in calls of 16: the rebuild route, and the starting point of every live call."""
        rows = np.ascontiguousarray(rows)
        h = ctypes.c_void_p()
        check(lib.ital_ctx_create(len(rows), d, params[0], params[1], params[2], max(64, m + 16), 0, 1, None, ctypes.byref(h)))
        check(lib.ital_ctx_fit(h, rows.ctypes.data, 0, None))
        for j0 in range(0, m, 16):
            i, t = np.ascontiguousarray(ids[j0:j0 + 16]), np.ascontiguousarray(y[j0:j0 + 16])
            check(lib.ital_ctx_update(h, i.ctypes.data, t.ctypes.data, len(i), None))
        return h

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    new_rows = np.ascontiguousarray(X[n:])
    scores, ok = np.empty((G, 3)), np.empty(G, dtype=np.int32)
    live = {
        "add_rows": lambda h: lib.ital_ctx_add_rows(h, new_rows.ctypes.data, r, 0, None),
        "remove_rows": lambda h: lib.ital_ctx_remove_rows(h, gone.ctypes.data, r, None, None),
        "set_params": lambda h: lib.ital_ctx_set_params(h, other[0], other[1], other[2], None),
        "evidence": lambda h: lib.ital_ctx_evidence(h, grid.ctypes.data, G, scores.ctypes.data, ok.ctypes.data, None),
    }
    rebuild = {
        "add_rows": lambda: build(X, labelled),
        "remove_rows": lambda: build(X[keep], new_id[labelled]),
        "set_params": lambda: build(X[:n], labelled, other),
        "evidence": lambda: build(X[:n], labelled),
    }
    res = dict(n=n, d=d, labels=m, rows=r, candidates=G, repeats=a.repeats)
    for name in live:
        t_live, t_new = [], []
        for rep in range(a.repeats + 1):                  # (repeat 0 warms both routes up)
            h = build(X[:n], labelled)
            ms, rc = wall(lambda: live[name](h))
            check(rc)
            check(lib.ital_ctx_destroy(h))
            ms2, h2 = wall(rebuild[name])
            check(lib.ital_ctx_destroy(h2))
            if rep:
                t_live.append(ms)
                t_new.append(ms2)
        res[name + "_ms"] = float(np.median(t_live))
        res[name + "_rebuild_ms"] = float(np.median(t_new))
        res[name + "_all_ms"] = t_live
        res[name + "_rebuild_all_ms"] = t_new
    res["evidence_ok"] = int(ok.sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
