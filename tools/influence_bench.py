#!/usr/bin/env python3
"""What revoking each label would change: GaussianProcess.influence (ital_gp_influence: one product L^-1^T V on FP64 MFMA,
reduced per label) against what there was before -- per label, clone() the learner, revoke([i]) and take the difference of
rel_mean.  Both sides are timed with a host clock around work that ends in a device synchronise, after a warm-up of the same
shape; the C entry is also timed with device events, whole and with no columns (stage 1 alone), which gives the time of the
tile kernel with its combine and from it

    flop/s       = m (m + 1) n / t           (what the upper-triangular product needs; the tile executes up to one 128-row
                                              block more per row tile, and 16 k-steps at a time)
    bytes/s      = 8 n sum_t (m - 128 t) / t  (V streamed once per 128-row tile of labels, rows from the tile's first on)
    share of peak = max(flop / 78.6 TFLOP/s, bytes / 6.3 TB/s) / t, with the bound named.

    python tools/influence_bench.py                 the headline shape 9298 x 256 with m = 64, then 1 000 000 x 512 with
                                                    m = 64 and m = 256
    python tools/influence_bench.py n d m [...]     one shape, several m

For m > 64 the baseline is timed on 8 labels spread over the positions and multiplied by m / 8 (said in the output)."""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ital_amd import ITAL, DeviceData, _lib
from ital_amd.gp import _stream

PEAK_FLOPS, PEAK_BYTES = 78.6e12, 6.3e12


def wall(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def events(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def entry_times(gp, reps):
    """(whole C entry, stage 1 alone) by device events."""
    lib = _lib.lib()
    d, keep = gp._influence_desc()
    whole = events(lambda: _lib.check(lib.ital_gp_influence(ctypes.byref(d), _stream())), reps)
    d.n, d.V, d.mu = 0, None, None
    stage1 = events(lambda: _lib.check(lib.ital_gp_influence(ctypes.byref(d), _stream())), reps)
    return whole, stage1


def baseline(L, ids):
    """clone() + revoke([i]) + the difference of rel_mean, per listed label; returns the largest |difference| per label."""
    base = np.asarray(L.rel_mean)
    out = []
    for i in ids:
        C = L.clone()
        C.revoke([int(i)])
        out.append(float(np.abs(np.asarray(C.rel_mean) - base).max()))
    return out


def run(n, d, ms):
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    store = DeviceData(torch.rand((n, d), dtype=torch.float64, device=dev, generator=gen), device=dev)
    L = ITAL(store, length_scale=float(np.sqrt(d / 12.0)), noise=1e-2, device=dev)
    L.gp_capacity = max(ms) + 16
    rng = np.random.default_rng(0)
    ids = [int(i) for i in rng.choice(n, max(ms), replace=False)]
    y = rng.choice([-1, 1], size=max(ms))
    fed = 0
    for m in sorted(ms):
        while fed < m:
            c = min(16, m - fed)
            L.update({ids[q]: int(y[q]) for q in range(fed, fed + c)})
            fed += c
        gp = L.gp
        gp.check_status()
        gp.influence()                                                    # warm-up: first launches, the workspace
        reps = 50 if n * m < 10 ** 8 else 5
        t_inf, inf = wall(gp.influence, reps)
        t_c, t_s1 = entry_times(gp, reps)
        t_tile = max(t_c - t_s1, 1e-9)
        flop = float(m) * (m + 1) * n
        nbytes = 8.0 * n * sum(m - 128 * t for t in range((m + 127) // 128))
        floor_f, floor_b = flop / PEAK_FLOPS, nbytes / PEAK_BYTES
        labelled = list(gp.ind)
        some = labelled if m <= 64 else [labelled[int(q)] for q in np.linspace(0, m - 1, 8).round()]
        baseline(L, some[:1])                                             # warm-up
        t_base, moved = wall(lambda: baseline(L, some))
        scale = m / len(some)
        pos = [labelled.index(i) for i in some]
        err = max(abs(inf["dmu_max"][p] - mv) for p, mv in zip(pos, moved))
        print("n=%d d=%d m=%d" % (n, d, m))
        print("  influence()            %10.3f ms (host wall, mean of %d)" % (t_inf * 1e3, reps))
        print("  ital_gp_influence      %10.3f ms (events)   stage 1 alone %8.3f ms   tile + combine %8.3f ms"
              % (t_c * 1e3, t_s1 * 1e3, t_tile * 1e3))
        print("  tile + combine         %8.2f TFLOP/s  %8.2f TB/s  %.3f of peak (%s bound)"
              % (flop / t_tile / 1e12, nbytes / t_tile / 1e12, max(floor_f, floor_b) / t_tile,
                 "FP64 MFMA" if floor_f > floor_b else "HBM"))
        print("  clone + revoke + diff  %10.3f ms for %d labels%s" % (t_base * 1e3, len(some), "" if scale == 1 else
              " -> %.3f ms SCALED by m / %d to all %d labels" % (t_base * scale * 1e3, len(some), m)))
        print("  ratio %.1fx; max |dmu_max - max |clone mean - mean|| over those labels = %.3g" % (t_base * scale / t_inf, err))


def main():
    if len(sys.argv) == 1:
        run(9298, 256, [64])
        run(1000000, 512, [64, 256])
    elif len(sys.argv) >= 4:
        run(int(sys.argv[1]), int(sys.argv[2]), [int(a) for a in sys.argv[3:]])
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
