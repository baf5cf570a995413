"""Ranking and evaluation on the device (include/ital_rank.h, csrc/rank.hip): the complete descending ranking of a score
vector, and scikit-learn's average precision and the reference's NDCG (utils.py:174-200) of it against relevance labels
+1 / -1 / 0 (0: unknown, left out).  What the reference's experiment loop does on the host after every round
(run_experiment.py:154-168) and `top_results` beyond ITAL_TOPK_MAX results.

    order = metrics.rank(scores)                 # int64 device tensor, np.argsort(scores, kind="stable")[::-1]
    metrics.evaluate(scores, relevance)          # {"ap", "ndcg", "n_pos", "n_neg", "n_unknown"}

Scores and relevance are numpy arrays or torch tensors, on the host or on the device; a float64 (int8 for the relevance)
contiguous device tensor is used in place, anything else is converted on the device.
"""
import numpy as np

from . import _lib
from ._lib import check


def _torch():
    import torch
    return torch


def _device_of(*arrays):
    torch = _torch()
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    return torch.device("cuda", torch.cuda.current_device())


def _scores(scores, device):
    torch = _torch()
    t = scores if isinstance(scores, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(scores, dtype=np.float64)))
    if t.ndim != 1 or t.numel() < 1:
        raise ValueError("scores must be a non-empty vector")
    return t.to(device=device, dtype=torch.float64).contiguous()


def _relevance(relevance, device):
    torch = _torch()
    if isinstance(relevance, torch.Tensor):
        t = relevance.to(device)
        if t.dtype != torch.int8:
            t = torch.sign(t).to(torch.int8)
    else:
        t = torch.from_numpy(np.sign(np.asarray(relevance)).astype(np.int8)).to(device)
    return t.contiguous()


def _stream():
    torch = _torch()
    return torch.cuda.current_stream().cuda_stream


def _rank_device(v, index_offset=0, values=False):
    """(order, ranked values or None) of a float64 contiguous device vector."""
    torch = _torch()
    lib = _lib.lib()
    n = v.numel()
    with torch.cuda.device(v.device):
        work = torch.empty(int(lib.ital_rank_workspace(n)), dtype=torch.uint8, device=v.device)
        order = torch.empty(n, dtype=torch.int64, device=v.device)
        vals = torch.empty(n, dtype=torch.float64, device=v.device) if values else None
        check(lib.ital_rank_desc(v.data_ptr(), n, int(index_offset), order.data_ptr(), vals.data_ptr() if values else 0,
                                 work.data_ptr(), work.numel(), _stream()))
    return order, vals


def rank(scores, index_offset=0, values=False):
    """The complete ranking of `scores` as an int64 device tensor of index_offset + position: value descending, NaN before
    every number, equal values (and -0.0 / +0.0) by descending position -- np.argsort(scores, kind="stable")[::-1], the order
    of top_results.  values=True: (ranking, the ranked scores with their own bits)."""
    v = _scores(scores, _device_of(scores))
    order, vals = _rank_device(v, index_offset, values)
    return (order, vals) if values else order


def evaluate_record(scores, relevance):
    """All six entries of the device record (_lib.RANK_EVAL_FIELDS) as a dict of floats; the metrics are NaN when no sample is
    relevant or a known sample's score is NaN.  One download of 48 bytes."""
    torch = _torch()
    lib = _lib.lib()
    device = _device_of(scores, relevance)
    v = _scores(scores, device)
    rel = _relevance(relevance, device)
    n = v.numel()
    if rel.ndim != 1 or rel.numel() != n:
        raise ValueError("scores and relevance must have the same length")
    order, _ = _rank_device(v)
    with torch.cuda.device(device):
        work = torch.empty(int(lib.ital_rank_eval_workspace(n)), dtype=torch.uint8, device=device)
        out = torch.empty(_lib.RANK_EVAL_LEN, dtype=torch.float64, device=device)
        check(lib.ital_rank_eval(order.data_ptr(), v.data_ptr(), rel.data_ptr(), n, 0, out.data_ptr(), work.data_ptr(),
                                 work.numel(), _stream()))
    return dict(zip(_lib.RANK_EVAL_FIELDS, out.cpu().tolist()))


def _refuse(n_pos, n_nan):
    if n_nan:
        raise ValueError("Input contains NaN.")
    if not n_pos:
        raise ValueError("no sample is relevant: average precision and NDCG are undefined")


def evaluate(scores, relevance):
    """{"ap", "ndcg", "n_pos", "n_neg", "n_unknown"} of `scores` against `relevance` (+1 / -1 / 0), computed on the device:
    ap = sklearn.metrics.average_precision_score(relevance[relevance != 0], scores[relevance != 0]), ndcg = the reference's
    utils.ndcg(relevance, scores) with ties ranked as rank() ranks them.  ValueError for a NaN score of a known sample (as
    scikit-learn) and when no sample is relevant; host inputs are refused before anything goes to the device."""
    torch = _torch()
    if not isinstance(scores, torch.Tensor) and not isinstance(relevance, torch.Tensor):
        scores, relevance = np.asarray(scores, dtype=np.float64), np.asarray(relevance)
        if scores.ndim != 1 or scores.shape != relevance.shape or scores.size < 1:
            raise ValueError("scores and relevance must be non-empty vectors of the same length")
        _refuse(int(np.count_nonzero(relevance > 0)), int(np.count_nonzero(np.isnan(scores[relevance != 0]))))
    rec = evaluate_record(scores, relevance)
    _refuse(rec["n_pos"], rec["n_nan"])
    return {"ap": rec["ap"], "ndcg": rec["ndcg"], "n_pos": int(rec["n_pos"]), "n_neg": int(rec["n_neg"]),
            "n_unknown": int(rec["n_unknown"])}
