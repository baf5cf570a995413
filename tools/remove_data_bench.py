#!/usr/bin/env python3
"""remove_data() at one shape, in one process (HIP events next to the host wall clock around a synchronise; a warm-up of every
variant, then medians of alternated repeats):

  (a) learner.remove_data(ids) end to end, on a learner with 40 labels (10 updates of 4) over a DeviceData of `dtype` rows
      (storage="source": f64 rows are the FP64 store), r scattered unlabelled rows removed;
  (b) the only route there was before: the reduced matrix (index_select on the device), a new store and learner on it and a
      replay of the labels in the same rounds;
  (c) each gather alone -- ital_compact_rows (X, xnorm) and ital_compact_cols (V, mu, s2 at the learner's m and capacity) -- in
      GB/s of the algorithm's bytes;
  (d) the same gathers written with torch: index_select plus a copy into the padded buffers (and a zero fill of V);
  (e) a device-to-device copy_ that moves the same number of bytes: the ceiling.

Bytes are the algorithm's, from the shapes: the row gather reads and writes n_keep padded rows and norms and reads n_keep 8-B
indices; the column gather reads m x n_keep doubles of V, mu and s2 and the indices, and writes the whole cap x ldv_dst block
(zero rows and pad columns included), mu and s2.

    python tools/remove_data_bench.py n d dtype r [--repeats R] [--json FILE]      (dtype: f64, f32, f16 or bf16)

--json merges the result, every repeat included, into FILE under the key "<n>x<d>_<dtype>_r<r>"."""
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
ROUNDS, PER_ROUND = 10, 4


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


def pad16(v):
    return (v + 15) // 16 * 16


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("n", type=int)
    ap.add_argument("d", type=int)
    ap.add_argument("dtype", choices=sorted(DTYPES))
    ap.add_argument("r", type=int)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("remove_data_bench needs a HIP device: nothing is timed without one")
    n, d, r, dtype = a.n, a.d, a.r, DTYPES[a.dtype]
    es = torch.empty(0, dtype=dtype).element_size()
    ldx = pad16(d)
    ls = float(np.sqrt(d / 12.0))
    lib = _lib.lib()
    g = torch.Generator(device=DEV).manual_seed(0)
    rows = torch.rand((n, d), generator=g, dtype=torch.float64, device=DEV).to(dtype)
    rng = np.random.default_rng(0)
    labelled = rng.choice(n, ROUNDS * PER_ROUND, replace=False)
    first_col = rows[torch.from_numpy(labelled).to(DEV), 0].to(torch.float64).cpu().numpy()
    rounds = [{int(i): (1 if first_col[q * PER_ROUND + t] > 0.5 else -1) for t, i in enumerate(labelled[q * PER_ROUND:(q + 1) * PER_ROUND])}
              for q in range(ROUNDS)]
    free = np.setdiff1d(np.arange(n), labelled)
    ids = np.sort(rng.choice(free, r, replace=False))
    keep = np.delete(np.arange(n, dtype=np.int64), ids)
    new_id = np.full(n, -1, dtype=np.int64)
    new_id[keep] = np.arange(len(keep))
    reduced_rounds = [{int(new_id[i]): y for i, y in fb.items()} for fb in rounds]
    keep_d = torch.from_numpy(keep).to(DEV)
    nk = len(keep)

    def session(data, history):
        L = ITAL(DeviceData(data, device=DEV, storage="source"), length_scale=ls, device=DEV)
        for fb in history:
            L.update(fb)
        return L

    def removed():
        L = session(rows, rounds)
        return timed(lambda: L.remove_data(ids)) + (L,)

    def rebuilt():
        return timed(lambda: session(rows.index_select(0, keep_d), reduced_rounds))

    # ---- (a), (b): alternated; one warm-up each, which also shows that both routes end in the same model
    _, _, _, A = removed()
    _, _, B = rebuilt()
    diff = float((A.gp.mu - B.gp.mu).abs().max())
    m, cap = A.gp.m, A.gp.cap
    del A, B
    gc.collect()
    ta, wa, tb, wb = [], [], [], []
    for _ in range(a.repeats):
        ev, wall, _, L = removed()
        ta.append(ev)
        wa.append(wall)
        del L
        gc.collect()
        ev, wall, L = rebuilt()
        tb.append(ev)
        wb.append(wall)
        del L
        gc.collect()
    torch.cuda.empty_cache()

    # ---- (c), (d), (e): the gathers alone
    store = DeviceData(rows, device=DEV, storage="source")
    X, xnorm = store.X, store.xnorm
    ldv, ldd = pad16(n), pad16(nk)
    V = torch.rand((cap, ldv), generator=g, dtype=torch.float64, device=DEV)
    mu = torch.rand(n, generator=g, dtype=torch.float64, device=DEV)
    s2 = torch.rand(n, generator=g, dtype=torch.float64, device=DEV)
    X_dst = torch.empty((nk, ldx), dtype=dtype, device=DEV)
    xnorm_dst = torch.empty(nk, dtype=torch.float64, device=DEV)
    V_dst = torch.empty((cap, ldd), dtype=torch.float64, device=DEV)
    mu_dst = torch.empty(nk, dtype=torch.float64, device=DEV)
    s2_dst = torch.empty(nk, dtype=torch.float64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    code = {"f64": 0, "f32": 1, "f16": 2, "bf16": 3}[a.dtype]
    st = _stream()
    bytes_rows = 2.0 * nk * ldx * es + 16.0 * nk + 8.0 * nk
    bytes_cols = 8.0 * m * nk + 8.0 * cap * ldd + 32.0 * nk + 8.0 * nk
    flat_rows = (torch.empty(int(bytes_rows) // 16, dtype=torch.float64, device=DEV), torch.empty(int(bytes_rows) // 16, dtype=torch.float64, device=DEV))
    flat_cols = (torch.empty(int(bytes_cols) // 16, dtype=torch.float64, device=DEV), torch.empty(int(bytes_cols) // 16, dtype=torch.float64, device=DEV))

    def rows_kernel():
        _lib.check(lib.ital_compact_rows(X.data_ptr(), xnorm.data_ptr(), n, ldx, code, keep_d.data_ptr(), nk, X_dst.data_ptr(),
                                         xnorm_dst.data_ptr(), status.data_ptr(), st))

    def cols_kernel():
        _lib.check(lib.ital_compact_cols(V.data_ptr(), ldv, m, mu.data_ptr(), s2.data_ptr(), n, keep_d.data_ptr(), nk,
                                         V_dst.data_ptr(), ldd, cap, mu_dst.data_ptr(), s2_dst.data_ptr(), status.data_ptr(), st))

    def rows_torch():
        X_dst.copy_(X.index_select(0, keep_d))
        xnorm_dst.copy_(xnorm.index_select(0, keep_d))

    def cols_torch():
        V_dst.zero_()
        V_dst[:m, :nk] = V[:m].index_select(1, keep_d)
        mu_dst.copy_(mu.index_select(0, keep_d))
        s2_dst.copy_(s2.index_select(0, keep_d))

    # the two writings of each gather give the same bits
    rows_kernel()
    cols_kernel()
    got = [t.clone() for t in (X_dst, xnorm_dst, V_dst, mu_dst, s2_dst)]
    rows_torch()
    cols_torch()
    torch.cuda.synchronize()
    same = all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(got, (X_dst, xnorm_dst, V_dst, mu_dst, s2_dst)))
    if not same or int(status.item()) != 0:
        sys.exit("the kernels and the torch gathers wrote different bits")
    del got
    kernels = [("rows_kernel", rows_kernel, bytes_rows), ("rows_torch", rows_torch, bytes_rows),
               ("rows_copy", lambda: flat_rows[1].copy_(flat_rows[0]), bytes_rows), ("cols_kernel", cols_kernel, bytes_cols),
               ("cols_torch", cols_torch, bytes_cols), ("cols_copy", lambda: flat_cols[1].copy_(flat_cols[0]), bytes_cols)]
    for _, fn, _ in kernels:
        fn()
    tc = {name: [] for name, _, _ in kernels}
    for _ in range(max(a.repeats, 7)):
        for name, fn, _ in kernels:
            tc[name].append(timed(fn)[0])

    res = dict(n=n, d=d, ldx=ldx, dtype=a.dtype, removed=r, labels=m, capacity=cap, repeats=a.repeats,
               a_remove_data_event_ms=median(ta) * 1e3, a_remove_data_wall_ms=median(wa) * 1e3,
               b_rebuild_event_ms=median(tb) * 1e3, b_rebuild_wall_ms=median(wb) * 1e3,
               a_all_event_ms=[t * 1e3 for t in ta], a_all_wall_ms=[t * 1e3 for t in wa],
               b_all_event_ms=[t * 1e3 for t in tb], b_all_wall_ms=[t * 1e3 for t in wb],
               max_abs_mean_difference_a_vs_b=diff,
               gather_ms={k: median(v) * 1e3 for k, v in tc.items()}, gather_all_ms={k: [t * 1e3 for t in v] for k, v in tc.items()},
               gather_gbytes={name: b / 1e9 for name, _, b in kernels},
               gather_gbytes_per_s={name: b / median(tc[name]) / 1e9 for name, _, b in kernels}, gathers_bit_identical=True)
    print("n=%d d=%d (ldx %d) %s, %d rows removed, m=%d cap=%d, %d repeats, medians" % (n, d, ldx, a.dtype, r, m, cap, a.repeats))
    print("(a) remove_data            %10.3f ms (events)  %10.3f ms (host wall)   (wall min %.3f max %.3f)"
          % (res["a_remove_data_event_ms"], res["a_remove_data_wall_ms"], min(wa) * 1e3, max(wa) * 1e3))
    print("(b) new learner and replay %10.3f ms (events)  %10.3f ms (host wall)   (wall min %.3f max %.3f)"
          % (res["b_rebuild_event_ms"], res["b_rebuild_wall_ms"], min(wb) * 1e3, max(wb) * 1e3))
    print("    max |mean(a) - mean(b)| = %.3g" % diff)
    for name, _, b in kernels:
        print("(c-e) %-12s %10.3f ms  %7.3f GB  %7.1f GB/s   (min %.3f max %.3f)"
              % (name, res["gather_ms"][name], b / 1e9, res["gather_gbytes_per_s"][name], min(tc[name]) * 1e3, max(tc[name]) * 1e3))
    if a.json:
        merged = {}
        if os.path.exists(a.json):
            with open(a.json) as f:
                merged = json.load(f)
        merged["%dx%d_%s_r%d" % (n, d, a.dtype, r)] = res
        with open(a.json, "w") as f:
            json.dump(merged, f, indent=1)


if __name__ == "__main__":
    main()
