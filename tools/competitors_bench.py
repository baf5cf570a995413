#!/usr/bin/env python3
"""Measures the RBMAL / TCAL learners (ital_amd/competitors.py) and ital_cosine_min (csrc/cosine.hip) on one device.

    python tools/competitors_bench.py [--out FILE] [--quick]

Prints one JSON object (also written to --out):
  - ital_cosine_min at 9298 x 256 with c = 45 (FP64 rows) and at 1M x 512 with c = 256 (FP64 rows and an f16 store): ms per
    call from device events after a warm-up, and the two lower bounds of that time -- the traffic bound
    ceil(c / 64) * n * ldx * sizeof(element) over the 6.3 TB/s of HBM that are achievable, and 2 n c ldx flop over the FP64
    matrix peak -- with the measured time as a multiple of the larger one;
  - scipy's cdist(..., 'cosine').min(-1), the reference's path (baseline_methods.py:500), on this machine's CPUs for the same
    shapes: measured on a slice of the rows (cdist is one thread; the slice is split over 16 threads) and scaled to n;
  - a whole RBMAL.fetch_unlabelled(4) at 9298 x 256 with 45 labelled samples, with the folded cache (3 new rows) and with a
    full recompute, and a whole TCAL.fetch_unlabelled(4): host clock around the call (it ends in a download).
--quick: small shapes, one repetition (a rehearsal of the script, not a measurement).
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_MFMA_PEAK_TFLOPS = 78.6
HBM_ACHIEVABLE_TBS = 6.3
CPU_THREADS = 16


def cosine_case(torch, lib, check, n, d, c, dtype, reps, launches):
    from ital_amd.device_data import DTYPE_CODES
    g = torch.Generator(device="cuda").manual_seed(n + c)
    X = torch.rand((n, d), generator=g, dtype=torch.float32, device="cuda").to(dtype)       # d is a multiple of 16: no padding
    T = torch.rand((c, d), generator=g, dtype=torch.float64, device="cuda")
    xn = torch.empty(n, dtype=torch.float64, device="cuda")
    for r0 in range(0, n, 1 << 16):                          # the norms of the widened rows, without a widened copy of X
        blk = X[r0:r0 + (1 << 16)].to(torch.float64)
        xn[r0:r0 + (1 << 16)] = (blk * blk).sum(1)
    tn = (T * T).sum(1)
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    times = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            check(lib.ital_cosine_min(X.data_ptr(), DTYPE_CODES[dtype], xn.data_ptr(), n, d, T.data_ptr(), tn.data_ptr(), c, 0,
                                      out.data_ptr(), st))
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1) / launches)
    assert bool(torch.isfinite(out).all()) and float(out.min()) >= 0.0
    ms = min(times)
    passes = (c + 63) // 64
    traffic_ms = passes * n * d * X.element_size() / (HBM_ACHIEVABLE_TBS * 1e12) * 1e3
    flop_ms = 2.0 * n * c * d / (FP64_MFMA_PEAK_TFLOPS * 1e12) * 1e3
    lower = max(traffic_ms, flop_ms)
    return dict(n=n, d=d, c=c, rows=str(dtype).replace("torch.", ""), ms=round(ms, 4), ms_all=[round(t, 4) for t in times],
                passes=passes, traffic_bound_ms=round(traffic_ms, 4), flop_bound_ms=round(flop_ms, 4),
                bound_by="traffic" if traffic_ms >= flop_ms else "flop", times_the_bound=round(ms / lower, 2),
                tflops=round(2.0 * n * c * d / (ms * 1e-3) / 1e12, 2),
                x_tbs=round(passes * n * d * X.element_size() / (ms * 1e-3) / 1e12, 3))


def cdist_case(n, d, c, slice_rows):
    """scipy's path for n x d against c rows: seconds, scaled from `slice_rows` rows split over CPU_THREADS threads."""
    from scipy.spatial.distance import cdist
    rng = np.random.default_rng(n + c)
    rows = min(n, slice_rows)
    X, T = rng.random((rows, d)), rng.random((c, d))
    parts = np.array_split(np.arange(rows), CPU_THREADS)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(CPU_THREADS) as ex:
        list(ex.map(lambda p: cdist(X[p], T, "cosine").min(axis=-1), parts))
    sec = time.perf_counter() - t0
    return dict(n=n, d=d, c=c, rows_measured=rows, threads=CPU_THREADS, seconds_measured=round(sec, 4),
                seconds_scaled_to_n=round(sec * n / rows, 3))


def fetch_case(torch, X, ls, labels, extra, reps):
    from ital_amd import RBMAL, TCAL

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ret = fn()
        return (time.perf_counter() - t0) * 1e3, ret

    L = RBMAL(X, length_scale=ls, device="cuda:0")
    L.update(labels)
    L.fetch_unlabelled(4)                                    # warm-up, builds the kept distances
    folded, full = [], []
    for r in range(reps):
        L.update(extra[r])                                   # three more labelled rows: the next fetch folds them in
        ms, ret = clock(lambda: L.fetch_unlabelled(4))
        assert len(ret) == 3 and L.last["folded"] == len(extra[r])
        folded.append(ms)
        L._dist = None                                       # what any other change of the labelled set leads to
        ms, ret = clock(lambda: L.fetch_unlabelled(4))
        assert L.last["folded"] == len(L.last["train"])
        full.append(ms)
    np.random.seed(0)
    C = TCAL(X, length_scale=ls, device="cuda:0")
    C.update(labels)
    C.fetch_unlabelled(4)
    tcal = [clock(lambda: C.fetch_unlabelled(4))[0] for _ in range(reps)]
    return dict(n=len(X), d=X.shape[1], labelled=len(labels), k=4,
                rbmal_folded_ms=round(min(folded), 3), rbmal_folded_ms_all=[round(t, 3) for t in folded],
                rbmal_full_ms=round(min(full), 3), rbmal_full_ms_all=[round(t, 3) for t in full],
                tcal_ms=round(min(tcal), 3), tcal_ms_all=[round(t, 3) for t in tcal])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("competitors_bench needs a HIP device (nothing is measured without one)")
    from ital_amd import _lib
    lib, check = _lib.lib(), _lib.check
    reps = 1 if args.quick else 5
    big = 1 << 14 if args.quick else 1 << 20
    small = (2048, 64) if args.quick else (9298, 256)
    kernel = [cosine_case(torch, lib, check, small[0], small[1], 45, torch.float64, reps, 20),
              cosine_case(torch, lib, check, big, 512, 256, torch.float64, reps, 1),
              cosine_case(torch, lib, check, big, 512, 256, torch.float16, reps, 1),
              cosine_case(torch, lib, check, big, 512, 64, torch.float64, reps, 1),
              cosine_case(torch, lib, check, big, 512, 64, torch.float16, reps, 1)]
    cpu = [cdist_case(small[0], small[1], 45, small[0]), cdist_case(big, 512, 256, 1 << 14)]
    rng = np.random.default_rng(21)
    n, d = small
    X = rng.random((n, d))
    chosen = rng.choice(n, 45 + 3 * reps, replace=False)
    labels = {int(i): (1 if j % 2 == 0 else -1) for j, i in enumerate(chosen[:45])}
    extra = [{int(i): 1 for i in chosen[45 + 3 * r:48 + 3 * r]} for r in range(reps)]
    res = dict(fp64_mfma_peak_tflops=FP64_MFMA_PEAK_TFLOPS, hbm_achievable_tbs=HBM_ACHIEVABLE_TBS, cosine_min=kernel,
               cdist_cpu=cpu, fetch=fetch_case(torch, X, float(np.sqrt(d / 12.0)), labels, extra, reps))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
