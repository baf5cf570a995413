#!/usr/bin/env python3
"""Taking one label back: GaussianProcess.remove (ital_gp_remove: factor kernel + sweep over V) against the only way back
there was before -- reset() and a replay of the surviving labels in their original groups.  Both timed with HIP events in
this process; the factor kernel is also timed alone (on copies of L, alpha, XT, with no columns), which gives the sweep's
share and its bytes/s: it reads and writes rows p .. m-1 of V, 16 (m - p) ldv bytes.

    python tools/revoke_bench.py n d m [p]          (p: labelled position that leaves, default 0 = the longest sweep)"""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ital_amd import GaussianProcess, _lib
from ital_amd.gp import _ptr, _stream


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0


def factor_alone(gp, p):
    """The factor kernel on copies of the replicated state (n = 0: no sweep is launched)."""
    lib = _lib.lib()
    L, alpha, XT, XTn = gp.L.clone(), gp.alpha.clone(), gp.XT.clone(), gp.XTn.clone()
    work = torch.empty(int(lib.ital_gp_remove_workspace(gp.cap)), dtype=torch.float64, device=gp.device)
    r = _lib.ItalRemoveDesc()
    r.XT, r.XTn, r.ldx, r.L, r.ldl, r.alpha = _ptr(XT), _ptr(XTn), gp.ldx, _ptr(L), gp.cap, _ptr(alpha)
    r.V, r.ldv, r.n, r.mu, r.s2, r.m, r.p = None, gp.ldv, 0, None, None, gp.m, p
    r.work, r.work_doubles, r.status = _ptr(work), work.numel(), _ptr(gp.status)
    return timed(lambda: _lib.check(lib.ital_gp_remove(ctypes.byref(r), _stream())))[0]


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    n, d, m = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    p = int(sys.argv[4]) if len(sys.argv) > 4 else 0
    rng = np.random.default_rng(0)
    X = rng.random((n, d))
    ind = [int(i) for i in rng.choice(n, m, replace=False)]
    y = rng.choice([-1.0, 1.0], size=m)
    gp = GaussianProcess(X, float(np.sqrt(d / 12.0)), device="cuda:0", capacity=m + 16)

    def feed(ids, labels, groups):
        at = 0
        for c in groups:
            if c:
                gp.update(ids[at:at + c], labels[at:at + c])
            at += c

    groups = [1] + [16] * ((m - 1) // 16) + ([(m - 1) % 16] if (m - 1) % 16 else [])
    feed(ind, y, groups)
    gp.check_status()
    # warm-up: the last label leaves and comes back (first launches, the workspace)
    gp.remove([ind[-1]])
    gp.update([ind[-1]], y[-1:])
    groups = list(gp.appends)
    t_factor = factor_alone(gp, p)
    t_factor = min(t_factor, factor_alone(gp, p))
    mean_before = gp.mu.clone()
    t_rev, w_rev = timed(lambda: gp.remove([ind[p]]))
    survivors, labels, left = list(gp.ind), gp.y.copy(), list(gp.appends)
    mean_revoked = gp.mu.clone()

    def replay():
        gp.reset()
        feed(survivors, labels, left)

    t_rep, w_rep = timed(replay)
    gp.check_status()
    diff = float((gp.mu - mean_revoked).abs().max())
    moved = float((mean_before - mean_revoked).abs().max())
    sweep = max(t_rev - t_factor, 1e-9)
    nbytes = 16.0 * (m - p) * gp.ldv
    print("n=%d d=%d m=%d p=%d" % (n, d, m, p))
    print("revoke          %10.3f ms (events)  %10.3f ms (host wall)" % (t_rev * 1e3, w_rev * 1e3))
    print("  factor alone  %10.3f ms" % (t_factor * 1e3))
    print("  sweep         %10.3f ms  %.1f MB  %.1f GB/s" % (sweep * 1e3, nbytes / 1e6, nbytes / sweep / 1e9))
    print("reset + replay  %10.3f ms (events)  %10.3f ms (host wall)   %d appends" % (t_rep * 1e3, w_rep * 1e3,
                                                                                   sum(1 for c in left if c)))
    print("speed-up %.1fx; max |mean(revoke) - mean(replay)| = %.3g (the revoke moved the means by up to %.3g)"
          % (t_rep / t_rev, diff, moved))


if __name__ == "__main__":
    main()
