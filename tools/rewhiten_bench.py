#!/usr/bin/env python3
"""Whitening all n data rows against the m labelled samples, three ways in one process, timed with HIP events (median of
repeated, alternated runs after a warm-up; the host wall clock around a synchronise is printed next to it):

  (a) ital_whiten_rows over all rows, at every chunk size (32 / 64 / 128 labelled rows per launch);
  (b) the composed sweeps that define it: ital_row_norms, then ital_whiten_append per block of 16 labelled rows;
  (c) GaussianProcess.set_params end to end against what there was before: set the attributes and gp.fit(gp.ind, gp.y).

(a) and (b) write to buffers of their own and are compared bit for bit at the measured size.  Bytes are the algorithm's,
from the shapes: the feature rows once per launch, the earlier rows of V each launch reads from memory, V written once.

    python tools/rewhiten_bench.py n d m [--repeats R] [--json FILE]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ital_amd import GaussianProcess, _lib
from ital_amd.gp import _ptr, _stream

CHUNKS = (32, 64, 128)


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0


class Out(object):
    def __init__(self, gp):
        dev = gp.device
        self.xnorm = torch.empty(gp.n, dtype=torch.float64, device=dev)
        self.mu = torch.empty(gp.n, dtype=torch.float64, device=dev)
        self.s2 = torch.empty(gp.n, dtype=torch.float64, device=dev)
        self.V = torch.zeros((gp.cap, gp.ldv), dtype=torch.float64, device=dev)


def kernel(gp, o, chunk):
    r = _lib.ItalRewhitenDesc()
    r.X, r.n_rows, r.ldx = _ptr(gp.Xd), gp.n, gp.ldx
    r.XT, r.XTn, r.L, r.ldl, r.alpha, r.m = _ptr(gp.XT), _ptr(gp.XTn), _ptr(gp.L), gp.cap, _ptr(gp.alpha), gp.m
    r.var, r.length_scale = float(gp.var), float(gp.length_scale)
    r.xnorm, r.V, r.ldv, r.v_rows, r.mu, r.s2, r.chunk = _ptr(o.xnorm), _ptr(o.V), gp.ldv, gp.cap, _ptr(o.mu), _ptr(o.s2), chunk
    _lib.check(_lib.lib().ital_whiten_rows(ctypes.byref(r), _stream()))


def composed(gp, o):
    lib, st = _lib.lib(), _stream()
    o.mu.zero_()
    o.s2.fill_(float(gp.var))
    _lib.check(lib.ital_row_norms(_ptr(gp.Xd), gp.n, gp.ldx, _ptr(o.xnorm), st))
    for b0 in range(0, gp.m, 16):
        c = min(16, gp.m - b0)
        _lib.check(lib.ital_whiten_append(_ptr(gp.Xd), _ptr(o.xnorm), gp.n, gp.ldx, gp.XT.data_ptr() + 8 * b0 * gp.ldx,
                                          gp.XTn.data_ptr() + 8 * b0, c, gp.L.data_ptr() + 8 * b0 * gp.cap, gp.cap,
                                          gp.L.data_ptr() + 8 * (b0 * gp.cap + b0), gp.alpha.data_ptr() + 8 * b0, _ptr(o.V),
                                          gp.ldv, b0, float(gp.var), float(gp.length_scale), _ptr(o.mu), _ptr(o.s2), st))


def algorithm_bytes(n, ldx, m, step):
    """Feature rows once per launch (plus once for the norms), V rows of earlier launches read, V written once."""
    launches = (m + step - 1) // step
    earlier = sum(c0 for c0 in range(0, m, step))
    return 8.0 * n * (ldx * (launches + 1) + earlier + m)


def median(xs):
    return float(np.median(np.asarray(xs)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("n", type=int)
    ap.add_argument("d", type=int)
    ap.add_argument("m", type=int)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rewhiten_bench needs a HIP device: nothing is timed without one")
    n, d, m = a.n, a.d, a.m
    rng = np.random.default_rng(0)
    X = rng.random((n, d))
    ind = [int(i) for i in rng.choice(n, m, replace=False)]
    y = rng.choice([-1.0, 1.0], size=m)
    ls = float(np.sqrt(d / 12.0))
    gp = GaussianProcess(X, ls, device="cuda:0", capacity=m + 16)
    at = 0
    for c in [1] + [16] * ((m + 14) // 16):
        c = min(c, m - at)
        if c:
            gp.update(ind[at:at + c], y[at:at + c])
        at += c
    gp.check_status()
    default_chunk = int(_lib.lib().ital_whiten_rows_chunk())

    # ---- (a) and (b): warm-up of every shape, bit-for-bit comparison, then alternated timed runs
    oa, ob = Out(gp), Out(gp)
    composed(gp, ob)
    for chunk in CHUNKS:
        oa.V.fill_(-1.0)
        kernel(gp, oa, chunk)
        torch.cuda.synchronize()
        same = all(torch.equal(getattr(oa, k)[: gp.n], getattr(ob, k)[: gp.n]) for k in ("xnorm", "mu", "s2")) and \
            torch.equal(oa.V[:, : gp.n], ob.V[:, : gp.n])
        if not same:
            sys.exit("chunk %d: ital_whiten_rows differs from the composed sweeps" % chunk)
    ta = {chunk: [] for chunk in CHUNKS}
    tb, wa, wb = [], [], []
    for _ in range(a.repeats):
        for chunk in CHUNKS:
            ev, wall = timed(lambda: kernel(gp, oa, chunk))
            ta[chunk].append(ev)
            if chunk == default_chunk:
                wa.append(wall)
        ev, wall = timed(lambda: composed(gp, ob))
        tb.append(ev)
        wb.append(wall)

    # ---- (c): set_params against attributes + fit(), toggling between two settings so that both always have work to do
    settings = [(1.3 * ls, 1.4, 1e-4), (ls, 1.0, 1e-6)]
    ind0, y0 = list(gp.ind), gp.y.copy()

    def by_fit(ls_, var_, noise_):
        gp.length_scale, gp.length_scale_sq, gp.var, gp.noise = ls_, ls_ * ls_, var_, noise_
        gp.fit(ind0, y0)

    gp.set_params(*settings[0])
    by_fit(*settings[1])
    tc_new, tc_old, wc_new, wc_old = [], [], [], []
    for r in range(a.repeats):
        ev, wall = timed(lambda: gp.set_params(*settings[r % 2]))
        tc_new.append(ev)
        wc_new.append(wall)
        mean_new = gp.mu.clone()
        ev, wall = timed(lambda: by_fit(*settings[r % 2]))
        tc_old.append(ev)
        wc_old.append(wall)
        diff = float((gp.mu - mean_new).abs().max())
    gp.check_status()

    res = dict(n=n, d=d, ldx=gp.ldx, m=m, repeats=a.repeats, default_chunk=default_chunk, bit_identical=True,
               a_whiten_rows_ms={str(c): median(ta[c]) * 1e3 for c in CHUNKS},
               a_whiten_rows_all_ms={str(c): [t * 1e3 for t in ta[c]] for c in CHUNKS},
               a_host_wall_ms=median(wa) * 1e3,
               b_composed_ms=median(tb) * 1e3, b_composed_all_ms=[t * 1e3 for t in tb], b_host_wall_ms=median(wb) * 1e3,
               a_gbytes={str(c): algorithm_bytes(n, gp.ldx, m, c) / 1e9 for c in CHUNKS},
               b_gbytes=algorithm_bytes(n, gp.ldx, m, 16) / 1e9,
               c_set_params_ms=median(tc_new) * 1e3, c_set_params_wall_ms=median(wc_new) * 1e3,
               c_attributes_and_fit_ms=median(tc_old) * 1e3, c_attributes_and_fit_wall_ms=median(wc_old) * 1e3,
               c_max_mean_difference=diff)
    print("n=%d d=%d (ldx %d) m=%d, %d repeats, medians; default chunk %d" % (n, d, gp.ldx, m, a.repeats, default_chunk))
    for c in CHUNKS:
        t = res["a_whiten_rows_ms"][str(c)]
        print("(a) ital_whiten_rows chunk %3d  %10.3f ms  %7.2f GB  %7.1f GB/s   (min %.3f max %.3f)"
              % (c, t, res["a_gbytes"][str(c)], res["a_gbytes"][str(c)] / t * 1e3, min(ta[c]) * 1e3, max(ta[c]) * 1e3))
    t = res["b_composed_ms"]
    print("(b) composed sweeps             %10.3f ms  %7.2f GB  %7.1f GB/s   (min %.3f max %.3f)"
          % (t, res["b_gbytes"], res["b_gbytes"] / t * 1e3, min(tb) * 1e3, max(tb) * 1e3))
    print("    (b) / (a, default chunk) = %.2fx; host wall (a) %.3f ms, (b) %.3f ms"
          % (t / res["a_whiten_rows_ms"][str(default_chunk)], res["a_host_wall_ms"], res["b_host_wall_ms"]))
    print("(c) set_params                  %10.3f ms (events)  %10.3f ms (host wall)" % (res["c_set_params_ms"], res["c_set_params_wall_ms"]))
    print("    attributes + fit(ind, y)    %10.3f ms (events)  %10.3f ms (host wall)   max |mean difference| %.3g"
          % (res["c_attributes_and_fit_ms"], res["c_attributes_and_fit_wall_ms"], diff))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
