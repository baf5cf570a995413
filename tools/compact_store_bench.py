#!/usr/bin/env python3
"""A compact store (DeviceData(storage="source")) next to the FP64 store of the same values, at one shape, in one process:
HIP events, a warm-up of every variant, alternated repeats, medians.

  (a) the ital_whiten_append sweep (c = 16 new labelled rows against m = 64);
  (b) one ital_cross_cov_cols column (m = 64);
  (c) ital_whiten_rows over all rows (m = 64, one chunk);
  (d) a fetch_unlabelled(4) + update round of an ITAL learner on the store (--no-round skips it);
  (e) torch.cuda.memory_allocated of the store.

Bytes are the algorithm's, from the shapes: per row the kernels read d elements of the store's type and the m whitened
values (8 m bytes) and write what the entry point's contract says (a: 8 c + 16 read-modify-write of mu, s2; b: 8; c: 8 m + 16).
Before any time is printed the compact store's outputs are compared with the FP64 store's, bit for bit, at this very size.

    python tools/compact_store_bench.py n d dtype [--repeats R] [--no-round] [--json FILE]     (dtype: f32, f16 or bf16)

--json merges every repeat into FILE (default profiles/compact_store_bench.json) under the key "<n>x<d>_<dtype>"."""
import argparse
import ctypes
import gc
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from ital_amd import ITAL, DeviceData, _lib, mvn_stream
from ital_amd.gp import _stream

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
DEV = "cuda:0"
M, C = 64, 16


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


class State(object):
    """A labelled-set state of M + C rows that both stores are run against (the factor need not come from a Gram: the kernels
    are timed and compared, not interpreted), and each store's own outputs."""

    def __init__(self, wide, n, ldx, ls):
        g = torch.Generator().manual_seed(1)
        cap = M + C
        self.n, self.ldx, self.ldv, self.cap, self.ls = n, ldx, (n + 15) // 16 * 16, cap, ls
        pick = torch.randperm(n, generator=g)[:cap].to(DEV)
        self.XT = wide.X.index_select(0, pick).contiguous()
        self.XTn = wide.xnorm.index_select(0, pick).contiguous()
        L = torch.tril(torch.randn((cap, cap), generator=g, dtype=torch.float64) * 0.05) + 2.0 * torch.eye(cap, dtype=torch.float64)
        self.L = L.to(DEV)
        self.alpha = torch.randn(cap, generator=g, dtype=torch.float64).to(DEV)
        self.W = (torch.randn((1, cap), generator=g, dtype=torch.float64) * 0.1).to(DEV)

    def outputs(self):
        f = dict(dtype=torch.float64, device=DEV)
        return dict(V=torch.zeros((self.cap, self.ldv), **f), mu=torch.zeros(self.n, **f), s2=torch.ones(self.n, **f),
                    col=torch.zeros(self.ldv, **f))


def run_rows(st, store, o):
    r = _lib.ItalRewhitenDesc()
    r.X, r.n_rows, r.ldx = store.X.data_ptr(), st.n, st.ldx
    r.XT, r.XTn, r.L, r.ldl, r.alpha, r.m = st.XT.data_ptr(), st.XTn.data_ptr(), st.L.data_ptr(), st.cap, st.alpha.data_ptr(), M
    r.var, r.length_scale = 1.0, st.ls
    r.xnorm, r.V, r.ldv, r.v_rows = store.xnorm.data_ptr(), o["V"].data_ptr(), st.ldv, st.cap
    r.mu, r.s2, r.chunk = o["mu"].data_ptr(), o["s2"].data_ptr(), 64
    _lib.check(_lib.rows_fn("ital_whiten_rows", _lib_code(store))(ctypes.byref(r), _stream()))


def run_sweep(st, store, o):
    L21 = st.L[M:]
    _lib.check(_lib.rows_fn("ital_whiten_append", _lib_code(store))(
        store.X.data_ptr(), store.xnorm.data_ptr(), st.n, st.ldx, st.XT[M:].data_ptr(), st.XTn[M:].data_ptr(), C, L21.data_ptr(),
        st.cap, L21.data_ptr() + 8 * M, st.alpha[M:].data_ptr(), o["V"].data_ptr(), st.ldv, M, 1.0, st.ls, o["mu"].data_ptr(),
        o["s2"].data_ptr(), _stream()))


def run_column(st, store, o):
    _lib.check(_lib.rows_fn("ital_cross_cov_cols", _lib_code(store))(
        store.X.data_ptr(), store.xnorm.data_ptr(), st.n, st.ldx, st.XT.data_ptr(), st.XTn.data_ptr(), 1, st.W.data_ptr(), st.cap,
        o["V"].data_ptr(), st.ldv, M, 1.0, st.ls, o["col"].data_ptr(), st.ldv, _stream()))


def _lib_code(store):
    from ital_amd.device_data import DTYPE_CODES
    return DTYPE_CODES[store.storage]


class Learner(ITAL):
    gp_capacity = 32


def round_of(store, ls, X0):
    """A fresh learner with four labels: the time of one fetch_unlabelled(4) + update, and what it picked and holds."""
    mvn_stream.GLOBAL.reset()
    np.random.seed(0)
    L = Learner(store, length_scale=ls, device=DEV)
    L.update({3: 1, 11: -1, 40: 1, 50: -1})
    got = []

    def go():
        got.extend(L.fetch_unlabelled(4))
        L.update({int(i): (1 if X0[int(i)] > 0 else -1) for i in got})
    t = timed(go)
    return t, got, L.gp.mu.clone(), L.gp.V[: L.gp.m].clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("d", type=int)
    ap.add_argument("dtype", choices=sorted(DTYPES))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-round", action="store_true")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "compact_store_bench.json"))
    a = ap.parse_args()
    n, d, dt = a.n, a.d, DTYPES[a.dtype]
    es = torch.empty(0, dtype=dt).element_size()
    t = torch.randn((n, d), generator=torch.Generator().manual_seed(0), dtype=torch.float32).to(dt)
    ls = float(np.sqrt(2.0 * d))
    mem = {}
    stores = {}
    for name, kw in (("f64", {}), (a.dtype, dict(storage="source"))):
        gc.collect()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(DEV)
        stores[name] = DeviceData(t, device=DEV, **kw)
        torch.cuda.synchronize()
        mem[name] = torch.cuda.memory_allocated(DEV) - before
    wide, compact = stores["f64"], stores[a.dtype]
    assert same_bits(wide.xnorm, compact.xnorm) and same_bits(wide.X, compact.X.to(torch.float64))
    st = State(wide, n, wide.ldx, ls)
    outs = {name: st.outputs() for name in stores}
    kernels = (("whiten_rows", run_rows, lambda e: (e * d + 8 * M) + (8 * M + 16)),
               ("whiten_append", run_sweep, lambda e: (e * d + 8 * M + 16) + (8 * C + 16)),
               ("cross_cov_col", run_column, lambda e: (e * d + 8 * M) + 8))
    times = {k: {name: [] for name in stores} for k, _, _ in kernels}
    for k, fn, _ in kernels:                         # whiten_rows first: it leaves V[:M], mu, s2 of a consistent state
        for rep in range(a.repeats + 1):             # repeat 0: the warm-up of both variants
            for name in stores:
                o = outs[name]                       # both variants run the same sequence of calls on their own outputs
                sec = timed(lambda: fn(st, stores[name], o))
                if rep:
                    times[k][name].append(sec)
        for key in ("V", "mu", "s2", "col"):
            assert same_bits(outs["f64"][key], outs[a.dtype][key]), (k, key)
    result = dict(n=n, d=d, dtype=a.dtype, m=M, c=C, store_bytes=mem, kernels={})
    print("%d x %d, %s store next to the FP64 store (m = %d, c = %d); outputs equal bit for bit" % (n, d, a.dtype, M, C))
    print("store: f64 %.1f MiB, %s %.1f MiB" % (mem["f64"] / 2.0 ** 20, a.dtype, mem[a.dtype] / 2.0 ** 20))
    for k, _, nbytes in kernels:
        row = {}
        for name, e in (("f64", 8), (a.dtype, es)):
            med = float(np.median(times[k][name]))
            total = n * nbytes(e)
            row[name] = dict(seconds=times[k][name], median_s=med, bytes=total, gbs=total / med * 1e-9)
            print("%-14s %-5s %9.1f us  %8.1f MB  %7.1f GB/s" % (k, name, med * 1e6, total * 1e-6, total / med * 1e-9))
        result["kernels"][k] = row
    if not a.no_round:
        X0 = t[:, 0].to(torch.float64).numpy()
        rounds = {name: [] for name in stores}
        kept = {}
        for rep in range(a.repeats + 1):
            for name in stores:
                sec, got, mu, V = round_of(stores[name], ls, X0)
                kept[name] = (got, mu, V)
                if rep:
                    rounds[name].append(sec)
            assert kept["f64"][0] == kept[a.dtype][0] and same_bits(kept["f64"][1], kept[a.dtype][1]) and \
                same_bits(kept["f64"][2], kept[a.dtype][2])
        result["round_k4"] = {name: dict(seconds=v, median_s=float(np.median(v))) for name, v in rounds.items()}
        print("fetch(4)+update: f64 %.2f ms, %s %.2f ms (same picks, same state)"
              % (result["round_k4"]["f64"]["median_s"] * 1e3, a.dtype, result["round_k4"][a.dtype]["median_s"] * 1e3))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        merged = json.load(open(a.json)) if os.path.exists(a.json) else {}
        merged["%dx%d_%s" % (n, d, a.dtype)] = result
        json.dump(merged, open(a.json, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
