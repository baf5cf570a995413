#!/usr/bin/env python3
"""Softening labels: GaussianProcess.reweigh (ital_gp_reweigh: factor kernel + ONE sweep over V for up to eight labels) for
r = 1, 4, 8 labels at the median labelled position, against the same labels in r single calls (what the shared pass buys) and
against the only route to a changed label there was before: remove(ids) + update(ids).  All timed with HIP events in this
process, best of three.  The factor kernels are also timed alone (factor-only call on copies of L and alpha), which gives
the sweep's share and its bytes/s against the 8 TB/s peak: a pass reads and writes rows p_min .. m-1 of V,
16 (m - p_min) ldv bytes.  remove()'s sweep at the same position is timed the same way for comparison.

    python tools/reweigh_bench.py n d m"""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ital_amd import GaussianProcess, _lib
from ital_amd.gp import _ptr, _stream

PEAK = 8e12


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def reweigh_factor_alone(gp, pos, delta):
    """The factor kernels on copies of the replicated state (V == NULL, n = 0: no sweep is launched)."""
    L, alpha = gp.L.clone(), gp.alpha.clone()
    status = torch.zeros(1, dtype=torch.int32, device=gp.device)
    return timed(lambda: gp._reweigh_call(L, alpha, status, pos, delta, factor_only=True))


def remove_factor_alone(gp, p):
    lib = _lib.lib()
    L, alpha, XT, XTn = gp.L.clone(), gp.alpha.clone(), gp.XT.clone(), gp.XTn.clone()
    work = torch.empty(int(lib.ital_gp_remove_workspace(gp.cap)), dtype=torch.float64, device=gp.device)
    r = _lib.ItalRemoveDesc()
    r.XT, r.XTn, r.ldx, r.L, r.ldl, r.alpha = _ptr(XT), _ptr(XTn), gp.ldx, _ptr(L), gp.cap, _ptr(alpha)
    r.V, r.ldv, r.n, r.mu, r.s2, r.m, r.p = None, gp.ldv, 0, None, None, gp.m, p
    r.work, r.work_doubles, r.status = _ptr(work), work.numel(), _ptr(gp.status)
    return timed(lambda: _lib.check(lib.ital_gp_remove(ctypes.byref(r), _stream())))


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    n, d, m = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    rng = np.random.default_rng(0)
    X = rng.random((n, d))
    ind = [int(i) for i in rng.choice(n, m, replace=False)]
    y = rng.choice([-1.0, 1.0], size=m)
    gp = GaussianProcess(X, float(np.sqrt(d / 12.0)), device="cuda:0", capacity=m + 16)
    gp.update(ind[:1], y[:1])
    for c0 in range(1, m, 16):
        gp.update(ind[c0:c0 + 16], y[c0:c0 + 16])
    gp.check_status()
    p0 = m // 2
    gp.reweigh([gp.ind[p0]], 0.3)                      # warm-up: first launches, the workspace
    gp.reweigh([gp.ind[p0]], 0.0)
    print("n=%d d=%d m=%d ldv=%d, labels from position %d on" % (n, d, m, gp.ldv, p0))
    for r in (1, 4, 8):
        pos = list(range(p0, p0 + r))
        ids = [gp.ind[p] for p in pos]
        nbytes = 16.0 * (m - p0) * gp.ldv
        t_one = t_single = t_factor = 1e9
        for _ in range(3):
            t_factor = min(t_factor, reweigh_factor_alone(gp, pos, [0.3] * r))
            t_one = min(t_one, timed(lambda: gp.reweigh(ids, 0.3)))
            gp.reweigh(ids, 0.0)

            def singles():
                for i in ids:
                    gp.reweigh([i], 0.3)
            t_single = min(t_single, timed(singles))
            gp.reweigh(ids, 0.0)
        sweep = max(t_one - t_factor, 1e-9)
        print("r=%d  one call %8.3f ms   (factor alone %7.3f ms, sweep %7.3f ms: %.1f MB, %.0f GB/s = %.0f%% of peak)"
              % (r, t_one * 1e3, t_factor * 1e3, sweep * 1e3, nbytes / 1e6, nbytes / sweep / 1e9, 100 * nbytes / sweep / PEAK))
        print("     %d single calls %8.3f ms   (%.2fx the one call)" % (r, t_single * 1e3, t_single / t_one))
        labels = [float(gp.y[p]) for p in pos]
        mean_before = gp.mu.clone()

        def old_route():
            gp.remove(ids)
            gp.update(ids, labels)
        t_old = timed(old_route)
        drift = float((gp.mu - mean_before).abs().max())
        print("     remove + update %8.3f ms   (%.2fx the one call; the labels end up last, means moved by %.2g)"
              % (t_old * 1e3, t_old / t_one, drift))
    p = p0
    t_rf = min(remove_factor_alone(gp, p) for _ in range(2))
    victim, label = gp.ind[p], float(gp.y[p])
    t_rm = timed(lambda: gp.remove([victim]))
    gp.update([victim], [label])
    sweep = max(t_rm - t_rf, 1e-9)
    nbytes = 16.0 * (m - p) * gp.ldv
    print("remove() at p=%d  %8.3f ms   (factor alone %7.3f ms, sweep %7.3f ms: %.0f GB/s = %.0f%% of peak)"
          % (p, t_rm * 1e3, t_rf * 1e3, sweep * 1e3, nbytes / sweep / 1e9, 100 * nbytes / sweep / PEAK))
    gp.check_status()


if __name__ == "__main__":
    main()
