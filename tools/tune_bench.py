#!/usr/bin/env python3
"""Measures the dense kernels of the hyper-parameter search (csrc/dense.hip) and ital_amd.tune end to end on one device.

    python tools/tune_bench.py [--out FILE] [--quick] [--no-cpu]

Prints one JSON object (also written to --out): Cholesky TFLOP/s (n^3 / 3 flop) and its share of the FP64 matrix peak,
single matrices and a batch of 10 x 8368; ital_kernel_matvec at 9298 x 9298 x 256, F = 10; ms per grid value of
cross_validate_gp at 9298 x 256 and 25 000 x 512 (10 folds); a whole ls_only sweep (21 values) per class at 9298 x 256;
and the reference's per-fold arithmetic (scipy dpotrf + dpotri + the dense predictions) for one fold at 9298, times 10 as
an extrapolated grid value.  Times: device events around work that ends in a synchronise, after one warm-up.
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


def _spd_device(torch, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    B = torch.rand((n, 64), generator=g, dtype=torch.float64, device="cuda")
    A = B @ B.T / 64
    A.diagonal().add_(1.0)
    return A


def chol_rate(torch, lib, check, sizes, reps=2):
    mats = [_spd_device(torch, n, i) for i, n in enumerate(sizes)]
    work = [m.clone() for m in mats]
    P = lambda v, dt: torch.tensor(v, dtype=dt, device="cuda")  # noqa: E731
    ptrs = P([w.data_ptr() for w in work], torch.int64)
    ns, lds = P(sizes, torch.int32), P(sizes, torch.int64)
    info = torch.zeros(len(sizes), dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    times = []
    for r in range(reps + 1):
        for w, m in zip(work, mats):
            w.copy_(m)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.ital_chol_batched(ptrs.data_ptr(), ns.data_ptr(), lds.data_ptr(), len(sizes), max(sizes), info.data_ptr(),
                                    status.data_ptr(), st))
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    assert int(info.abs().sum()) == 0
    ms = min(times)
    flop = sum(float(n) ** 3 / 3 for n in sizes)
    tf = flop / (ms * 1e-3) / 1e12
    return dict(sizes=sizes, ms=round(ms, 3), tflops=round(tf, 2), frac_peak=round(tf / FP64_MFMA_PEAK_TFLOPS, 3))


def matvec_rate(torch, lib, check, n=9298, d=256, F=10):
    from ital_amd import tune
    X = np.random.default_rng(1).random((n, d))
    dev = tune._DeviceRows(X, None)
    W = torch.rand((n, F), dtype=torch.float64, device="cuda")
    out = torch.empty((n, F), dtype=torch.float64, device="cuda")
    wl = int(lib.ital_kernel_matvec_workspace(n, n))
    work = torch.empty(max(wl, 1), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    times = []
    for r in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.ital_kernel_matvec(dev.Xd.data_ptr(), dev.xnorm.data_ptr(), n, dev.Xd.data_ptr(), dev.xnorm.data_ptr(), n,
                                     dev.ldx, W.data_ptr(), F, F, 1.0, 5.0, out.data_ptr(), F, work.data_ptr(), wl, st))
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    ms = min(times)
    flop = 2.0 * n * n * (d + F)
    return dict(shape=[n, n, d, F], ms=round(ms, 3), tflops=round(flop / (ms * 1e-3) / 1e12, 2))


def grid_value_ms(torch, n, d, values, seed=2):
    from ital_amd import tune
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    rel = np.where(X[:, 0] + X[:, 1] > 1.0, 1, -1)
    dev = tune._DeviceRows(X, None)
    plist = [dict(length_scale=v, var=1.0, noise=1e-6) for v in values]
    tune._scores(X, rel, plist[:1], 10, False, None, tune.DEFAULT_MAX_BYTES, dev=dev)     # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    aps = tune._scores(X, rel, plist, 10, False, None, tune.DEFAULT_MAX_BYTES, dev=dev)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return dict(shape=[n, d], values=len(values), ms_total=round(ms, 1), ms_per_value=round(ms / len(values), 1),
                ap=[round(a, 6) for a in aps])


def cpu_fold(n=9298, d=256):
    """One fold of the reference's procedure in float64 on the host: Gram, dpotrf + dpotri, w = K^-1 y, predictions."""
    from scipy.linalg import lapack
    rng = np.random.default_rng(2)
    X = rng.random((n, d))
    rel = np.where(X[:, 0] + X[:, 1] > 1.0, 1.0, -1.0)
    tr = np.arange(n) % 10 != 0
    te = ~tr
    t0 = time.perf_counter()
    A, B = X[tr], X[te]
    na = (A ** 2).sum(1)
    K = np.exp(((na[:, None] + na[None, :]) - 2 * A @ A.T) / (-2 * 25.0)) + 1e-6 * np.eye(len(A))
    c, info = lapack.dpotrf(K, False, False)
    inv, info2 = lapack.dpotri(c)
    iu = np.triu_indices_from(inv, 1)
    inv[iu[1], iu[0]] = inv[iu]
    w = inv @ rel[tr]
    nb = (B ** 2).sum(1)
    s = np.exp(((na[:, None] + nb[None, :]) - 2 * A @ B.T) / (-2 * 25.0)).T @ w
    ms = (time.perf_counter() - t0) * 1e3
    return dict(shape=[n, d], threads=os.environ.get("OMP_NUM_THREADS"), ms_one_fold=round(ms, 1),
                ms_per_value_extrapolated=round(10 * ms, 1), info=int(info), finite=bool(np.all(np.isfinite(s))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="skip the 25 000 x 512 and 22 500 Cholesky figures")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tune_bench needs a HIP device")
    from ital_amd import _lib
    lib, check = _lib.lib(), _lib.check
    res = dict(device=torch.cuda.get_device_name(0), fp64_mfma_peak_tflops=FP64_MFMA_PEAK_TFLOPS)
    sizes = [2048, 8192, 16384] + ([] if args.quick else [22500])
    res["chol_single"] = [chol_rate(torch, lib, check, [n]) for n in sizes]
    res["chol_batched"] = chol_rate(torch, lib, check, [8368] * 10)
    res["kernel_matvec"] = matvec_rate(torch, lib, check)
    res["cv_9298x256"] = grid_value_ms(torch, 9298, 256, [4.0, 6.0, 9.0])
    ls = [0.001, 0.005, 0.01, 0.05, 0.1, 0.5, 1.0, 1.5, 2.0, 2.5, 3., 4., 5., 6., 7., 8., 9., 10., 15., 20., 25.]
    res["ls_only_sweep_9298x256"] = grid_value_ms(torch, 9298, 256, ls)
    if not args.quick:
        res["cv_25000x512"] = grid_value_ms(torch, 25000, 512, [9.0])
    if not args.no_cpu:
        res["cpu_reference_9298"] = cpu_fold()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
