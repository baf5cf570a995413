#!/usr/bin/env python3
"""Measures the device ranking and evaluation (csrc/rank.hip, ital_amd/metrics.py) against the host path they replace.

    python tools/rank_bench.py [--out FILE] [--quick]

Prints one JSON object (also written to --out).  N = 9 298 and N = 1 000 000 scores (normal; harness.ndcg is defined on
distinct scores only) on the device, relevance +1 / -1 / 0 with probabilities 0.1 / 0.7 / 0.2; from the same run
  - ital_rank_desc alone: ms per call from device events after a warm-up, and its number of kernel launches;
  - ranking + evaluation as learner.evaluate() runs them (metrics.evaluate on device tensors, the download of the 48-byte
    record included): ms per call on the host clock around the call, which ends in that download, and the launches;
  - the path of before on the same inputs, each part on the host clock: the download of the N scores,
    np.argsort(kind="stable")[::-1] (top_results(None)), sklearn's average_precision_score on the known samples and
    harness.ndcg (a Python loop over the N samples): what one evaluation of the experiment loop came to;
  - the two results side by side (the ranking must be equal, the metrics agree to rounding).
--quick: small sizes, one repetition (a rehearsal of the script, not a measurement).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_ms(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ret = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return times, ret


def case(torch, n, reps):
    from sklearn.metrics import average_precision_score
    from ital_amd import _lib, harness, metrics
    lib = _lib.lib()
    rng = np.random.default_rng(n)
    s_host = rng.normal(size=n)
    rel_host = rng.choice(np.array([1, -1, 0], dtype=np.int8), size=n, p=[0.1, 0.7, 0.2])
    s = torch.from_numpy(s_host).to("cuda")
    rel = torch.from_numpy(rel_host).to("cuda")
    calls = 200 if n < 100000 else 20                              # a timed window of device work, not of one launch

    # the ranking alone, device events
    c0 = lib.ital_launch_count()
    order = metrics.rank(s)
    rank_launches = int(lib.ital_launch_count() - c0)
    torch.cuda.synchronize()
    t_rank = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            order = metrics.rank(s)
        e1.record()
        torch.cuda.synchronize()
        if r:
            t_rank.append(e0.elapsed_time(e1) / calls)

    # ranking + evaluation, ends in the download of the record
    c0 = lib.ital_launch_count()
    got = metrics.evaluate(s, rel)
    eval_launches = int(lib.ital_launch_count() - c0)

    def device_path():
        for _ in range(calls):
            res = metrics.evaluate(s, rel)
        return res
    t_eval, got = host_ms(device_path, reps)
    t_eval = [t / calls for t in t_eval]

    # the host path of before
    t_down, s_down = host_ms(lambda: s.cpu().numpy(), reps)
    t_sort, order_host = host_ms(lambda: np.argsort(s_down, kind="stable")[::-1], reps)
    known = rel_host != 0
    t_ap, ap_host = host_ms(lambda: average_precision_score(rel_host[known], s_down[known]), reps)
    t_ndcg, ndcg_host = host_ms(lambda: harness.ndcg(rel_host, s_down), 1 if n > 100000 else reps)
    host_total = min(t_down) + min(t_ap) + min(t_ndcg)
    r3 = lambda ts: [round(t, 4) for t in ts]
    return dict(n=n, calls_per_window=calls,
                rank_ms=round(min(t_rank), 4), rank_ms_all=r3(t_rank), rank_launches=rank_launches,
                rank_eval_ms=round(min(t_eval), 4), rank_eval_ms_all=r3(t_eval), rank_eval_launches=eval_launches,
                host_download_ms=round(min(t_down), 4), host_argsort_stable_ms=round(min(t_sort), 4), host_argsort_stable_ms_all=r3(t_sort),
                host_average_precision_ms=round(min(t_ap), 4), host_ndcg_ms=round(min(t_ndcg), 4),
                host_evaluation_ms=round(host_total, 4), host_evaluation_over_device=round(host_total / min(t_eval), 1),
                host_argsort_over_device_rank=round((min(t_down) + min(t_sort)) / min(t_rank), 1),
                ranking_equal=bool(np.array_equal(order.cpu().numpy(), order_host)),
                ap_device=got["ap"], ap_host=float(ap_host), ndcg_device=got["ndcg"], ndcg_host=float(ndcg_host))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rank_bench needs a HIP device (nothing is measured without one)")
    reps = 1 if args.quick else 3
    sizes = [3000, 20000] if args.quick else [9298, 1000000]
    res = dict(cases=[case(torch, n, reps) for n in sizes])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
