#!/usr/bin/env python3
"""DeviceData at one shape, three measurements in one process (HIP events, medians of alternated repeats after a warm-up of
every variant; the host wall clock around a synchronise next to them where the host takes part):

  (a) constructing a learner: from a float64 numpy array (the path of a numpy caller, unchanged), from a host array of `dtype`
      through a DeviceData, from a device tensor of `dtype`, and on a store that exists already;
  (b) ital_ingest_rows alone (the conversion and the ital_row_norms launch behind it), in bytes moved per second, on both load
      paths -- 16-B loads (an aligned source) and single elements (the same source one element into its allocation) -- next to
      what the same process gets from ital_row_norms alone (tools/stream_bench.py's first line) and from a plain device-to-device
      copy of the FP64 rows (torch's copy_: 16 B per element);
  (c) torch.cuda.memory_allocated of a second learner after one update: on the store, and on a private copy.

Bytes are the algorithm's, from the shapes: the conversion reads n d elements and writes n ldx doubles, the norms read those
doubles again and write n.

    python tools/device_data_bench.py n d dtype [--repeats R] [--json FILE]      (dtype: f64, f32, f16 or bf16)

--json merges the result into FILE under the key "<n>x<d>_<dtype>"."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ital_amd import ITAL, DeviceData, _lib
from ital_amd.gp import _stream

DTYPES = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
DEV = "cuda:0"


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0, out


def median(xs):
    return float(np.median(np.asarray(xs)))


class Learner(ITAL):
    gp_capacity = 16


def construct(data, ls):
    L = Learner(data, length_scale=ls, device=DEV)
    return L


def allocated():
    gc.collect()
    torch.cuda.synchronize()
    return torch.cuda.memory_allocated(DEV)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("n", type=int)
    ap.add_argument("d", type=int)
    ap.add_argument("dtype", choices=sorted(DTYPES))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("device_data_bench needs a HIP device: nothing is timed without one")
    n, d, dtype = a.n, a.d, DTYPES[a.dtype]
    es = torch.empty(0, dtype=dtype).element_size()
    ldx = (d + 15) // 16 * 16
    ls = float(np.sqrt(d / 12.0))
    lib = _lib.lib()
    rng = np.random.default_rng(0)
    X64 = rng.random((n, d))
    # the caller's rows in their own type, on the host: a numpy array that numpy allocated, like X64 (the rate of an upload
    # from pageable memory depends on who allocated it); numpy has no bf16: a torch tensor then
    if dtype is torch.bfloat16:
        host_in = torch.from_numpy(X64).to(dtype)
        device_in = host_in.to(DEV)
    else:
        host_in = X64.astype({"f64": np.float64, "f32": np.float32, "f16": np.float16}[a.dtype])
        device_in = torch.from_numpy(host_in).to(DEV)
    store = DeviceData(device_in, device=DEV)

    # ---- (a) construction, alternated: every variant once as a warm-up, then `repeats` rounds
    # a numpy array handed to a learner directly keeps the path it always took (float64 on the host, FP64 staging tensor):
    # "numpy_f64" is that path, "numpy_<dtype>_direct" the same for the caller's own type; "host_<dtype>" goes through a store
    variants = [("numpy_f64", lambda: construct(X64, ls)),
                ("host_" + a.dtype, lambda: construct(DeviceData(host_in, device=DEV), ls)),
                ("device_" + a.dtype, lambda: construct(device_in, ls)), ("existing_store", lambda: construct(store, ls))]
    if isinstance(host_in, np.ndarray) and a.dtype != "f64":
        variants.insert(1, ("numpy_%s_direct" % a.dtype, lambda: construct(host_in, ls)))
    for _, fn in variants:
        fn()
    gc.collect()
    ta = {name: [] for name, _ in variants}
    wa = {name: [] for name, _ in variants}
    for _ in range(a.repeats):
        for name, fn in variants:
            ev, wall, L = timed(fn)
            ta[name].append(ev)
            wa[name].append(wall)
            del L
            gc.collect()

    # ---- (b) the entry point alone, both load paths, next to row norms alone and a plain copy
    X = torch.empty((n, ldx), dtype=torch.float64, device=DEV)
    X2 = torch.empty((n, ldx), dtype=torch.float64, device=DEV)
    xn = torch.empty(n, dtype=torch.float64, device=DEV)
    code = {"f64": 0, "f32": 1, "f16": 2, "bf16": 3}[a.dtype]
    shifted_buf = torch.empty(n * d + 1, dtype=dtype, device=DEV)
    shifted = shifted_buf[1:].view(n, d)
    shifted.copy_(device_in)
    wide_ran = device_in.data_ptr() % 16 == 0 and (d * es) % 16 == 0     # the rule of csrc/ingest.hip
    assert shifted.data_ptr() % 16 != 0
    st = _stream()

    def ingest(src):
        _lib.check(lib.ital_ingest_rows(src.data_ptr(), code, n, d, d, X.data_ptr(), ldx, xn.data_ptr(), st))

    kernels = [("ingest_aligned", lambda: ingest(device_in)), ("ingest_shifted", lambda: ingest(shifted)),
               ("row_norms", lambda: _lib.check(lib.ital_row_norms(X.data_ptr(), n, ldx, xn.data_ptr(), st))),
               ("copy_f64", lambda: X2.copy_(X))]
    ingest(shifted)
    keep = (X.clone(), xn.clone())
    ingest(device_in)
    torch.cuda.synchronize()
    if not (torch.equal(X, keep[0]) and torch.equal(xn, keep[1])):
        sys.exit("the two load paths wrote different bits")
    del keep
    for _, fn in kernels:
        fn()
    tb = {name: [] for name, _ in kernels}
    for _ in range(a.repeats):
        for name, fn in kernels:
            tb[name].append(timed(fn)[0])
    conv_bytes = float(n) * d * es + 8.0 * n * ldx
    norm_bytes = 8.0 * n * ldx + 8.0 * n
    bytes_b = dict(ingest_aligned=conv_bytes + norm_bytes, ingest_shifted=conv_bytes + norm_bytes, row_norms=norm_bytes,
                   copy_f64=16.0 * n * ldx)
    del X, X2, xn, shifted, shifted_buf
    torch.cuda.empty_cache()

    # ---- (c) what a second learner adds
    def second(make):
        first = construct(make(), ls)
        first.update({3: 1, n // 2: -1})
        before = allocated()
        other = construct(make(), ls)
        other.update({5: 1, n // 3: -1})
        return allocated() - before

    mem_store = second(lambda: store)
    mem_private = second(lambda: device_in)

    res = dict(n=n, d=d, ldx=ldx, dtype=a.dtype, repeats=a.repeats,
               a_construct_event_ms={k: median(v) * 1e3 for k, v in ta.items()},
               a_construct_wall_ms={k: median(v) * 1e3 for k, v in wa.items()},
               a_construct_event_all_ms={k: [t * 1e3 for t in v] for k, v in ta.items()},
               a_construct_wall_all_ms={k: [t * 1e3 for t in v] for k, v in wa.items()},
               b_ms={k: median(v) * 1e3 for k, v in tb.items()}, b_all_ms={k: [t * 1e3 for t in v] for k, v in tb.items()},
               b_gbytes={k: v / 1e9 for k, v in bytes_b.items()},
               b_gbytes_per_s={k: bytes_b[k] / median(tb[k]) / 1e9 for k in tb},
               b_contiguous_source_takes="16-B loads" if wide_ran else "single elements", b_paths_bit_identical=True,
               c_second_learner_bytes=dict(on_the_store=int(mem_store), private_copy=int(mem_private)),
               x_bytes=8 * n * ldx)
    print("n=%d d=%d (ldx %d) %s, %d repeats, medians" % (n, d, ldx, a.dtype, a.repeats))
    for name, _ in variants:
        print("(a) learner from %-18s %10.3f ms (events)  %10.3f ms (host wall)   (wall min %.3f max %.3f)"
              % (name, res["a_construct_event_ms"][name], res["a_construct_wall_ms"][name], min(wa[name]) * 1e3, max(wa[name]) * 1e3))
    for name, _ in kernels:
        print("(b) %-16s %10.3f ms  %7.3f GB  %7.1f GB/s   (min %.3f max %.3f)"
              % (name, res["b_ms"][name], res["b_gbytes"][name], res["b_gbytes_per_s"][name], min(tb[name]) * 1e3, max(tb[name]) * 1e3))
    print("    a contiguous %s source of this shape takes the %s" % (a.dtype, res["b_contiguous_source_takes"]))
    print("(c) a second learner: %.2f MiB on the store, %.2f MiB on a private copy (X itself: %.2f MiB)"
          % (mem_store / 2.0 ** 20, mem_private / 2.0 ** 20, res["x_bytes"] / 2.0 ** 20))
    if a.json:
        merged = {}
        if os.path.exists(a.json):
            with open(a.json) as f:
                merged = json.load(f)
        merged["%dx%d_%s" % (n, d, a.dtype)] = res
        with open(a.json, "w") as f:
            json.dump(merged, f, indent=1)


if __name__ == "__main__":
    main()
