#!/usr/bin/env python3
"""Measures the USDM learner (ital_amd/usdm.py, csrc/usdm.hip) on one device.

    python tools/usdm_bench.py [--out FILE] [--quick]

Prints one JSON object (also written to --out).  Data: uniform random rows, 9298 x 256, length scale 3, one relevant and one
irrelevant label, k = 4.  From the same run
  - one whole fetch_unlabelled (host clock around the call, which ends in a download), with the default options and with
    tol = 0, max_iter = 10 (ten iterations of the loop); the graph is built before and timed on its own;
  - every part of a fetch on its own, from device events after a warm-up, best of three windows: Laplacian assembly, LU
    factor, LU solve, Gram, and per iteration shift, Cholesky, Cholesky solve, symv and the vector updates in torch;
  - ital_lu_factor alone at n = 2048 and n = 9298 against torch.linalg.lu_factor (pivoted, the vendor library) on the same
    Laplacian-shaped matrix: ms and (2/3) n^3 / t in TFLOP/s;
  - the whole fetch against the NumPy restatement of the reference's fetch (tests/_usdm_ref.py, whatever threads the BLAS of
    this process has) at n = 1000, 2000 and 4000, and that host time extrapolated by n^3 to 9298 (labelled as such).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def events(torch, fn, reps, before=None):
    """ms of `fn` per window, `reps` windows after a warm-up window; `before` (untimed) prepares each window."""
    times = []
    for r in range(reps + 1):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    return round(min(times), 3)


def learner_on(X, labels, **kw):
    from ital_amd import USDM
    L = USDM(X, length_scale=3.0, **kw)
    L.update(labels)
    return L


def whole_fetch(torch, L, k, reps):
    times = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        L.fetch_unlabelled(k)
        if r:
            times.append((time.perf_counter() - t0) * 1e3)
    return round(min(times), 3), L.last["iterations"]


def parts(torch, L, k, reps):
    """The calls of USDM.fetch_unlabelled, one by one, on buffers of their own."""
    from ital_amd import _lib
    from ital_amd.gp import _pad16, _ptr, _stream
    from ital_amd.usdm import EPS, usdm_entropy_term
    lib, check, gp, dev = _lib.lib(), _lib.check, L.gp, L.gp.device
    u = np.asarray(L._unseen_array(), dtype=np.int64)
    n, n_u = int(gp.n), len(u)
    ld = _pad16(n_u)
    pos = np.full(n, -1, dtype=np.int64)
    pos[u] = np.arange(n_u)
    rel = np.zeros(n, dtype=np.uint8)
    rel[list(L.relevant_ids)] = 1
    u_d, pos_d, rel_d = (torch.from_numpy(a).to(dev) for a in (u, pos, rel))
    idx = L._graph().idx
    M = torch.empty((n_u, ld), dtype=torch.float64, device=dev)
    Kuu = torch.empty((n_u, ld), dtype=torch.float64, device=dev)
    p = torch.empty(n_u, dtype=torch.float64, device=dev)
    flags = torch.zeros(4, dtype=torch.int32, device=dev)
    ptrs = torch.tensor([u_d.data_ptr(), Kuu.data_ptr(), M.data_ptr(), ld], dtype=torch.int64, device=dev)
    n_p = torch.tensor([n_u], dtype=torch.int32, device=dev)
    wl = int(lib.ital_symv_lower_workspace(n_u))
    work = torch.empty(wl, dtype=torch.float64, device=dev)
    st = _stream()

    def laplacian():
        check(lib.ital_usdm_laplacian(_ptr(idx), L.knn, n, _ptr(u_d), n_u, _ptr(pos_d), _ptr(rel_d), len(L.relevant_ids), EPS,
                                      _ptr(M), ld, _ptr(p), st))

    def lu_factor():
        check(lib.ital_lu_factor(_ptr(M), n_u, ld, _ptr(flags[0:]), _ptr(flags[1:]), st))

    def lu_solve():
        check(lib.ital_lu_solve(_ptr(M), n_u, ld, _ptr(p), _ptr(flags[0:]), st))

    def gram():
        check(lib.ital_gram_rows(_ptr(gp.Xd), _ptr(gp.xnorm), gp.ldx, _ptr(ptrs[0:]), _ptr(n_p), _ptr(ptrs[1:]), _ptr(ptrs[3:]), 1,
                                 n_u, float(L.var), float(L.length_scale), 0.0, st))

    res = dict(n_u=n_u, laplacian_ms=events(torch, laplacian, reps), lu_factor_ms=events(torch, lu_factor, reps, laplacian),
               lu_solve_ms=events(torch, lu_solve, reps), gram_ms=events(torch, gram, reps))
    b = usdm_entropy_term(torch.clamp(p, 1e-8, 1 - 1e-8), L.r)
    f = torch.full((n_u,), 1.0 / n_u, dtype=torch.float64, device=dev)
    Kf = torch.empty_like(f)
    y_p = torch.tensor([f.data_ptr()], dtype=torch.int64, device=dev)
    state = dict(v=f.clone(), l1=torch.zeros((), dtype=torch.float64, device=dev), l2=torch.zeros_like(f))
    mu = 1e-6

    def shift():
        check(lib.ital_usdm_shift(_ptr(Kuu), n_u, ld, mu, _ptr(M), ld, st))

    def chol():
        check(lib.ital_chol_batched(_ptr(ptrs[2:]), _ptr(n_p), _ptr(ptrs[3:]), 1, n_u, _ptr(flags[2:]), _ptr(flags[3:]), st))

    def chol_solve():
        check(lib.ital_chol_solve_batched(_ptr(ptrs[2:]), _ptr(n_p), _ptr(ptrs[3:]), _ptr(y_p), 1, _ptr(flags[2:]), st))

    def symv():
        check(lib.ital_symv_lower(_ptr(Kuu), n_u, ld, _ptr(f), _ptr(Kf), _ptr(work), wl, st))

    def vectors():
        f.copy_(mu * (state["v"] + 1.0) - (state["l2"] + state["l1"]) - b)
        v = f + state["l2"] / mu
        v[v < 0] = 0
        l1 = state["l1"] + mu * (f.sum() - k)
        l2 = state["l2"] + mu * (f - v)
        return torch.dot(f, Kf) / 2 + torch.dot(f, b), v, l1, l2

    res.update(shift_ms=events(torch, shift, reps), chol_ms=events(torch, chol, reps, shift),
               chol_solve_ms=events(torch, chol_solve, reps), symv_ms=events(torch, symv, reps),
               vector_updates_ms=events(torch, vectors, reps))
    res["flags"] = flags.cpu().tolist()
    res["iteration_ms"] = round(sum(res[key] for key in ("shift_ms", "chol_ms", "chol_solve_ms", "symv_ms", "vector_updates_ms")), 3)
    res["solves_share_of_default_fetch"] = None
    return res


def lu_against_torch(torch, n, reps):
    import _usdm_ref as ref
    from ital_amd import _lib
    from ital_amd.gp import _ptr, _stream
    lib, check = _lib.lib(), _lib.check
    rng = np.random.default_rng(n)
    total = n + n // 5
    idx = rng.integers(0, total, size=(n, 5))
    A = np.full((n, n), -ref.EPS)
    rows = np.repeat(np.arange(n), 5)
    inside = idx.ravel() < n
    A[rows[inside], idx.ravel()[inside]] = -(1.0 + ref.EPS)
    A[np.arange(n), np.arange(n)] = 5 + total * ref.EPS - ref.EPS
    src = torch.from_numpy(A).cuda()
    work = torch.empty_like(src)
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    st = _stream()

    def mine():
        check(lib.ital_lu_factor(_ptr(work), n, n, _ptr(flags[0:]), _ptr(flags[1:]), st))

    def theirs():
        torch.linalg.lu_factor(work)

    def fill():
        work.copy_(src)

    t_mine, t_torch = events(torch, mine, reps, fill), events(torch, theirs, reps, fill)
    flop = 2.0 / 3.0 * n ** 3
    return dict(n=n, ital_lu_factor_ms=t_mine, ital_tflops=round(flop / (t_mine * 1e-3) / 1e12, 3), torch_lu_factor_ms=t_torch,
                torch_tflops=round(flop / (t_torch * 1e-3) / 1e12, 3), flags=flags.cpu().tolist())


def host_restatement(X, labels, k):
    import _usdm_ref as ref
    t0 = time.perf_counter()
    K = ref.kernel(X, 3.0, 1.0)
    A = ref.laplacian_matrix(ref.neighbours(K, 5), len(X))
    t1 = time.perf_counter()
    out = ref.fetch(K, A, {i for i, v in labels.items() if v > 0}, {i for i, v in labels.items() if v < 0}, set(), k, 1.0, 100, 1e-6)
    return time.perf_counter() - t1, t1 - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("usdm_bench needs a HIP device (nothing is measured without one)")
    reps = 1 if args.quick else 3
    n, d, k = (700, 32, 4) if args.quick else (9298, 256, 4)
    X = np.random.default_rng(0).random((n, d))
    labels = {0: 1, 1: -1}
    res = dict(n=n, d=d, k=k, blas_threads=os.environ.get("OMP_NUM_THREADS"))
    L = learner_on(X, labels)
    t0 = time.perf_counter()
    L._graph()
    torch.cuda.synchronize()
    res["graph_first_call_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    res["fetch_ms"], res["fetch_iterations"] = whole_fetch(torch, L, k, reps)
    L10 = learner_on(X, labels, tol=0.0, max_iter=10)
    res["fetch_10_iterations_ms"], res["fetch_10_iterations"] = whole_fetch(torch, L10, k, reps)
    res["parts"] = parts(torch, L, k, reps)
    pr = res["parts"]
    res["parts"]["solves_share_of_default_fetch"] = round(
        (pr["lu_solve_ms"] + res["fetch_iterations"] * pr["chol_solve_ms"]) / res["fetch_ms"], 3)
    res["lu_factor"] = [lu_against_torch(torch, m, reps) for m in ((256, 700) if args.quick else (2048, 9298))]
    host = []
    for m in ((300, 500) if args.quick else (1000, 2000, 4000)):
        Lm = learner_on(X[:m], labels)
        Lm._graph()
        dev_ms, _ = whole_fetch(torch, Lm, k, reps)
        fetch_s, setup_s, out = host_restatement(X[:m], labels, k)
        host.append(dict(n=m, device_fetch_ms=dev_ms, numpy_fetch_s=round(fetch_s, 3), numpy_kernel_and_graph_s=round(setup_s, 3),
                         numpy_over_device=round(fetch_s * 1e3 / dev_ms, 1), iterations=(Lm.last["iterations"], out["iterations"]),
                         same_picks=set(out["picks"].tolist()) == set(Lm.fetch_unlabelled(k))))
    res["against_numpy"] = host
    last = host[-1]
    res["numpy_fetch_s_extrapolated_by_n3_to_%d" % n] = round(last["numpy_fetch_s"] * (n / last["n"]) ** 3, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
