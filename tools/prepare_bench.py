#!/usr/bin/env python3
"""Measures the kernels of include/ital_prepare.h (csrc/prepare.hip) on one device against what a user could do before them.

    python tools/prepare_bench.py [--out FILE] [--quick]

Prints one JSON object (also written to --out).  Shapes 9298 x 256 f64, 100 000 x 512 f64 and f16, 1 000 000 x 512 f16; k = 50
axes (the reference's PCA-50).  From the same run, per shape
  - ital_col_stats, ital_col_cov and ital_project_rows (output in the store's own type): ms per call from device events, the
    best of three windows after a warm-up window.  For ital_col_cov the flop it executes (2 n 128^2 per lower-triangular
    tile pair) over that time in TFLOP/s and as a fraction of the FP64 matrix peak, and the nominal 2 n d^2 next to it; for
    ital_project_rows the bytes of X over the time in GB/s;
  - PCA.fit + apply as a user calls them (wall time around a device synchronisation: uploads, the eigh on the host and the
    norms of the new store included), and the peak device memory beyond the store;
  - the torch path on the same device: X.double() centred by its column means, Z.T @ Z, Z @ W -- ms for the scatter matrix
    and for the projection, and its peak device memory beyond the store;
  - numpy on the host (centre, Z.T @ Z, eigh, Z @ W), at the smallest shape only.
--quick: small shapes, one window (a rehearsal of the script, not a measurement).
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
            fn()
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1) / launches)
    return min(times)


def peak_beyond(torch, fn):
    """(result, wall seconds, peak bytes allocated beyond what was there before) of one call of fn."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    ret = fn()
    torch.cuda.synchronize()
    return ret, time.perf_counter() - t0, torch.cuda.max_memory_allocated() - base


def case(torch, n, d, dtype, k, reps, host):
    from ital_amd import _lib, DeviceData, PCA
    from ital_amd.device_data import DTYPE_CODES
    lib = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(n + d)
    X = (torch.randn((n, d), generator=g, dtype=torch.float32, device="cuda") * 2 + 1).to(dtype)      # d is a multiple of 16
    store = DeviceData(X, storage="source", device="cuda:0")
    del X
    Xs, code, name = store.X, DTYPE_CODES[dtype], str(dtype).replace("torch.", "")
    launches = 10 if n < 20000 else 1
    out3 = torch.empty((3, d), dtype=torch.float64, device="cuda")
    nb = lib.ital_col_stats_workspace(n, d)
    work = torch.empty(max(nb, 8), dtype=torch.uint8, device="cuda")
    t_stats = events(torch, lambda: _lib.check(lib.ital_col_stats(Xs.data_ptr(), code, n, d, d, out3[0].data_ptr(), out3[1].data_ptr(),
                                                                  out3[2].data_ptr(), work.data_ptr(), nb, stream)), reps, launches)
    mean = out3[2] / n
    C = torch.empty((d, d), dtype=torch.float64, device="cuda")
    nb = lib.ital_col_cov_workspace(n, d)
    work = torch.empty(max(nb, 8), dtype=torch.uint8, device="cuda")
    t_cov = events(torch, lambda: _lib.check(lib.ital_col_cov(Xs.data_ptr(), code, n, d, d, mean.data_ptr(), C.data_ptr(), d,
                                                              work.data_ptr(), nb, stream)), reps, launches)
    tiles = (d + 127) // 128
    executed, nominal = 2.0 * n * 128 * 128 * tiles * (tiles + 1) / 2, 2.0 * n * d * d
    W = torch.linalg.qr(torch.randn((d, k), dtype=torch.float64, device="cuda"))[0].contiguous()
    ldy = (k + 15) // 16 * 16
    Y = torch.empty((n, ldy), dtype=dtype, device="cuda")
    t_proj = events(torch, lambda: _lib.check(lib.ital_project_rows(Xs.data_ptr(), code, n, d, d, mean.data_ptr(), W.data_ptr(), k, k,
                                                                    Y.data_ptr(), code, ldy, stream)), reps, launches)
    del work, Y
    storage = {"float64": "f64", "float32": "f32", "float16": "f16", "bfloat16": "bf16"}[name]
    out, fit_s, fit_peak = peak_beyond(torch, lambda: PCA.fit(store, k).apply(store, storage=storage))
    del out

    def torch_cov():
        Z = Xs.double()
        Z = Z - Z.mean(dim=0)                    # out of place: an FP64 store is not to be centred where it lies
        return Z, Z.T @ Z

    def torch_all():
        Z, Ct = torch_cov()
        return Ct, (Z @ W).to(dtype)

    (Ct, _), _, torch_peak = peak_beyond(torch, torch_all)
    rel = float(((Ct - C).abs().max() / Ct.abs().max()))
    del Ct
    t_torch_cov = events(torch, torch_cov, reps, launches)
    Z = Xs.double()
    Z = Z - Z.mean(dim=0)
    t_torch_mm = events(torch, lambda: Z.T @ Z, reps, launches)
    t_torch_proj = events(torch, lambda: (Z @ W).to(dtype), reps, launches)
    del Z
    res = dict(n=n, d=d, dtype=name, k=k, calls_per_window=launches, col_stats_ms=round(t_stats, 3), col_cov_ms=round(t_cov, 3),
               col_cov_ranges=int(lib.ital_prepare_ranges(n, _lib.PREPARE_COV_UNIT, lib.ital_col_cov_cap(d))),
               col_cov_executed_tflops=round(executed / t_cov / 1e9, 2),
               col_cov_of_fp64_mfma_peak=round(executed / t_cov / 1e9 / FP64_MFMA_PEAK_TFLOPS, 3),
               col_cov_nominal_tflops=round(nominal / t_cov / 1e9, 2), project_ms=round(t_proj, 3),
               project_x_gbps=round(n * d * Xs.element_size() / t_proj / 1e6, 1), pca_fit_apply_s=round(fit_s, 4),
               pca_fit_apply_peak_bytes=int(fit_peak), torch_cov_with_widening_ms=round(t_torch_cov, 3),
               torch_cov_matmul_only_ms=round(t_torch_mm, 3), torch_project_ms=round(t_torch_proj, 3), torch_peak_bytes=int(torch_peak),
               torch_cov_over_col_cov=round(t_torch_cov / t_cov, 2), torch_project_over_project=round(t_torch_proj / t_proj, 2),
               largest_relative_difference_of_c=rel)
    if host:
        Xh = store.rows()
        t0 = time.perf_counter()
        Zh = Xh - Xh.mean(axis=0)
        lam, V = np.linalg.eigh(Zh.T @ Zh / (n - 1))
        Zh @ V[:, ::-1][:, :k]
        res["numpy_host_s"] = round(time.perf_counter() - t0, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prepare_bench needs a HIP device (nothing is measured without one)")
    reps = 1 if args.quick else 3
    f64, f16 = torch.float64, torch.float16
    shapes = [(1500, 64, f64, True), (5000, 128, f16, False)] if args.quick else \
        [(9298, 256, f64, True), (100000, 512, f64, False), (100000, 512, f16, False), (1000000, 512, f16, False)]
    res = dict(fp64_mfma_peak_tflops=FP64_MFMA_PEAK_TFLOPS,
               cases=[case(torch, n, d, dtype, min(50, d), reps, host) for n, d, dtype, host in shapes])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
