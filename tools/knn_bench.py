#!/usr/bin/env python3
"""Measures ital_knn_rows (csrc/knn.hip) on one device against the two things a user could do before it.

    python tools/knn_bench.py [--out FILE] [--quick]

Prints one JSON object (also written to --out).  Shapes 9298 x 256 and 100 000 x 512 (FP64 rows, cosine, skip_self), k = 21
and k = 5; from the same run
  - ital_knn_rows with splits = 0: ms per call from device events after a warm-up, and 2 n^2 ldx flop over that time in
    TFLOP/s and as a fraction of the FP64 matrix peak (the flops of the whole self-join: the kernel forms every tile);
  - the device-side path of before: an FP64 torch matmul of a block of query rows with a chunk of data rows, the cosine
    distance formed from it, torch.topk of the chunk, merged into the running k best by a second topk (what a chunked
    ital_cosine_min-style pass over all rows plus a top-k comes to); blocks sized to about 1 GiB of distances;
  - scipy's cdist(X, X, 'cosine') + np.partition on the host, for the small shape only (one thread, as the reference runs it).
The torch path's lists are compared with the kernel's (same indices where the k-th gap is not a near-tie).
--quick: small shapes, one repetition (a rehearsal of the script, not a measurement).
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


def events(torch, fn, reps, launches):
    """ms per call of `fn`, `launches` calls per timed window, `reps` windows after a warm-up window."""
    times = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            ret = fn()
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1) / launches)
    return times, ret


def torch_knn(torch, X, xn, k, qblock, cchunk):
    n = X.shape[0]
    root = xn.sqrt()
    out_d = torch.empty((n, k), dtype=torch.float64, device=X.device)
    out_i = torch.empty((n, k), dtype=torch.int64, device=X.device)
    for q0 in range(0, n, qblock):
        q1 = min(n, q0 + qblock)
        best_d = best_i = None
        for c0 in range(0, n, cchunk):
            c1 = min(n, c0 + cchunk)
            cos = (X[q0:q1] @ X[c0:c1].T) / (root[q0:q1, None] * root[None, c0:c1])
            dist = 1.0 - cos.clamp_(-1.0, 1.0)
            lo, hi = max(q0, c0), min(q1, c1)
            if lo < hi:                                                   # skip_self
                r = torch.arange(lo, hi, device=X.device)
                dist[r - q0, r - c0] = float("inf")
            d, i = torch.topk(dist, min(k, c1 - c0), dim=1, largest=False)
            i = i + c0
            if best_d is not None:
                d, i = torch.cat([best_d, d], 1), torch.cat([best_i, i], 1)
                d, pos = torch.topk(d, k, dim=1, largest=False)
                i = i.gather(1, pos)
            best_d, best_i = d, i
        out_d[q0:q1], out_i[q0:q1] = best_d, best_i
    return out_i, out_d


def case(torch, n, d, k, reps, host):
    from ital_amd.device_data import knn_rows
    g = torch.Generator(device="cuda").manual_seed(n + k)
    X = torch.rand((n, d), generator=g, dtype=torch.float64, device="cuda")          # d is a multiple of 16: no padding
    xn = (X * X).sum(1)
    idx = torch.empty((n, k), dtype=torch.int64, device="cuda")
    dist = torch.empty((n, k), dtype=torch.float64, device="cuda")
    rowsum = torch.empty(n, dtype=torch.float64, device="cuda")
    launches = 20 if n < 20000 else 1                                     # a timed window of a fraction of a second at least
    t_knn, _ = events(torch, lambda: knn_rows(X, xn, n, (0, n), (0, n), "cosine", k, True, idx, dist, rowsum), reps, launches)
    qblock = min(n, 8192)
    cchunk = min(n, max(1024, (1 << 27) // qblock))                       # qblock x cchunk doubles: 1 GiB
    t_torch, (ti, td) = events(torch, lambda: torch_knn(torch, X, xn, k, qblock, cchunk), reps, launches)
    agree = float((ti == idx).all(dim=1).double().mean())
    worst = float((td - dist).abs().max())
    flop = 2.0 * n * n * d
    ms = min(t_knn)
    res = dict(n=n, d=d, k=k, calls_per_window=launches, knn_ms=round(ms, 3), knn_ms_all=[round(t, 3) for t in t_knn],
               knn_tflops=round(flop / (ms * 1e-3) / 1e12, 2), of_fp64_mfma_peak=round(flop / (ms * 1e-3) / 1e12 / FP64_MFMA_PEAK_TFLOPS, 3),
               torch_ms=round(min(t_torch), 3), torch_ms_all=[round(t, 3) for t in t_torch], torch_qblock=qblock, torch_cchunk=cchunk,
               torch_over_knn=round(min(t_torch) / ms, 2), rows_with_equal_lists=round(agree, 4), largest_distance_difference=worst)
    if host:
        from scipy.spatial.distance import cdist
        Xh = X.cpu().numpy()
        t0 = time.perf_counter()
        D = cdist(Xh, Xh, "cosine")
        np.fill_diagonal(D, np.inf)
        part = np.partition(D, k - 1, axis=-1)[:, :k]
        res["scipy_cdist_partition_s"] = round(time.perf_counter() - t0, 3)
        res["scipy_largest_kth_difference"] = float(np.abs(part.max(axis=1) - dist[:, -1].cpu().numpy()).max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench needs a HIP device (nothing is measured without one)")
    reps = 1 if args.quick else 3
    shapes = [(1500, 64, True), (5000, 128, False)] if args.quick else [(9298, 256, True), (100000, 512, False)]
    res = dict(fp64_mfma_peak_tflops=FP64_MFMA_PEAK_TFLOPS,
               cases=[case(torch, n, d, k, reps, host and k == 21) for n, d, host in shapes for k in (21, 5)])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
