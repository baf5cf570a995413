#!/usr/bin/env python3
"""Measures the AdaptAL learner (ital_amd/adapt_al.py, csrc/adapt.hip) on one device.

    python tools/adapt_bench.py [--out FILE] [--quick]

Prints one JSON object (also written to --out): ms per fetch_unlabelled(4) at 9298 x 256 with subsample = 1000 (the
setting of the reference's configs) and without subsample (nc = 9292); ital_chol_inv_diag alone at n = 1000 and n = 9292:
ms, TFLOP/s with n^3 / 3 flop as the work count and its share of the FP64 matrix peak; and, for the record, the wall time
of the reference's own fetches as stored in the golden fixtures (the CPU of the machine that generated them).  Times: a
host clock around a fetch (it ends in a download) and device events around the kernel, after one warm-up.  --quick: one
timed repetition each (the run that is traced with `rocprofv3 --kernel-trace --stats`).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_MFMA_PEAK_TFLOPS = 78.6


def fetch_ms(torch, X, ls, labels, subsample, reps):
    from ital_amd import AdaptAL
    np.random.seed(0)
    L = AdaptAL(X, length_scale=ls, subsample=subsample, device="cuda:0")
    L.update(labels)
    times = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ret = L.fetch_unlabelled(4)
        times.append((time.perf_counter() - t0) * 1e3)
    assert len(set(ret)) == 4
    return dict(nc=len(L.last["candidates"]), short_list=len(L.last["max_ind"]), ms_first=round(times[0], 3),
                ms=round(min(times[1:]), 3), ms_all=[round(t, 3) for t in times[1:]])


def inv_diag_rate(torch, lib, check, n, reps):
    g = torch.Generator(device="cuda").manual_seed(n)
    B = torch.rand((n, 64), generator=g, dtype=torch.float64, device="cuda")
    A = B @ B.T / 64
    A.diagonal().add_(1.0)
    P = lambda v, dt: torch.tensor(v, dtype=dt, device="cuda")  # noqa: E731
    ptrs, ns, lds = P([A.data_ptr()], torch.int64), P([n], torch.int32), P([n], torch.int64)
    info = torch.zeros(2, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    check(lib.ital_chol_batched(ptrs.data_ptr(), ns.data_ptr(), lds.data_ptr(), 1, n, info.data_ptr(), info.data_ptr() + 4, st))
    wl = int(lib.ital_chol_inv_diag_workspace(n))
    work = torch.empty(wl, dtype=torch.float64, device="cuda")
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    times = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.ital_chol_inv_diag(A.data_ptr(), n, n, out.data_ptr(), work.data_ptr(), wl, info.data_ptr(), st))
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    assert int(info[0].item()) == 0 and bool(torch.isfinite(out).all())
    ms = min(times)
    tf = float(n) ** 3 / 3 / (ms * 1e-3) / 1e12
    return dict(n=n, ms=round(ms, 3), tflops=round(tf, 2), frac_peak=round(tf / FP64_MFMA_PEAK_TFLOPS, 3))


def reference_seconds():
    gold = os.path.join(ROOT, "tests", "golden")
    out = {}
    for name in sorted(os.listdir(gold)):
        if name.startswith("adapt_") and name.endswith(".npz"):
            z = np.load(os.path.join(gold, name))
            out[name[:-4]] = dict(nc=int(len(z["r0_cand"])), seconds_per_fetch=[round(float(s), 2) for s in z["ref_fetch_seconds"]])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("adapt_bench needs a HIP device (nothing is measured without one)")
    from ital_amd import _lib
    lib, check = _lib.lib(), _lib.check
    rng = np.random.default_rng(21)
    n, d = 9298, 256
    X = rng.random((n, d))
    ls = float(np.sqrt(d / 12.0))
    labels = {int(i): (1 if j % 2 == 0 else -1) for j, i in enumerate(rng.choice(n, 6, replace=False))}
    reps = 1 if args.quick else 5
    res = dict(shape=[n, d], k=4, fp64_mfma_peak_tflops=FP64_MFMA_PEAK_TFLOPS,
               fetch_subsample_1000=fetch_ms(torch, X, ls, labels, 1000, reps),
               fetch_all_candidates=fetch_ms(torch, X, ls, labels, None, 1 if args.quick else 2),
               chol_inv_diag=[inv_diag_rate(torch, lib, check, m, reps) for m in (1000, 9292)],
               reference_cpu_fetch_seconds=reference_seconds())
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
