"""Host model of include/ital_rank.h in plain NumPy: the order of the complete ranking, the tie-grouped average precision
(scikit-learn's average_precision_score on the known samples) and the NDCG walk of the reference (utils.py:174-200,
ital_amd.harness.ndcg) with ties ranked by that order."""
import math

import numpy as np


def order(s):
    """Value descending, NaN before every number, equal values (-0.0 == +0.0) and NaNs by descending position."""
    return np.argsort(np.asarray(s, dtype=np.float64), kind="stable")[::-1]


def counts(s, rel):
    s, rel = np.asarray(s, dtype=np.float64), np.asarray(rel)
    known = rel != 0
    return dict(n_pos=int(np.sum(rel > 0)), n_neg=int(np.sum(rel < 0)), n_unknown=int(np.sum(~known)),
                n_nan=int(np.sum(np.isnan(s[known]))))


def ap(s, rel):
    """Sum over the groups of equal score among the known samples, in rank order, of
    (positives in the group / n_pos) * (positives so far / known samples so far), taken at the group's last sample."""
    s, rel = np.asarray(s, dtype=np.float64), np.asarray(rel)
    o = order(s)
    o = o[rel[o] != 0]
    n_pos = int(np.sum(rel > 0))
    if n_pos == 0 or np.isnan(s[o]).any():
        return float("nan")
    total, tp, in_group = 0.0, 0, 0
    for r, j in enumerate(o, start=1):
        if rel[j] > 0:
            tp += 1
            in_group += 1
        if r == len(o) or s[o[r]] != s[j]:          # the group's last sample (0.0 == -0.0)
            total += (in_group / n_pos) * (tp / r)
            in_group = 0
    return total


def ndcg(s, rel):
    """The known sample of rank r has gain 1 / log2(r + 1); the summed gain of the positives over that of the first n_pos
    ranks."""
    s, rel = np.asarray(s, dtype=np.float64), np.asarray(rel)
    n_pos = int(np.sum(rel > 0))
    if n_pos == 0 or np.isnan(s[rel != 0]).any():
        return float("nan")
    rank, gain_sum, best = 0, 0.0, 0.0
    for j in order(s):
        if rel[j] != 0:
            rank += 1
            g = 1.0 / math.log2(rank + 1)
            if rel[j] > 0:
                gain_sum += g
            if rank <= n_pos:
                best += g
    return gain_sum / best


def evaluate(s, rel):
    out = counts(s, rel)
    out.update(ap=ap(s, rel), ndcg=ndcg(s, rel))
    return out
