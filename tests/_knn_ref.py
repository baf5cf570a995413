"""What the tests of the neighbour lists and of SUD share (tests/test_knn_host.py, tests/test_gpu_knn.py): the golden fixtures
of tests/golden/make_golden_sud.py, an extended-precision host model of the DEFINITION of ital_knn_rows (include/ital_knn.h)
and the checker that compares a result against it.

THE CHECKER does not depend on how near-ties fall.  The r-th order statistic of a row is 1-Lipschitz in the sup norm: if every
device distance of a row is within B of the model's, so is the r-th smallest.  Hence
    (a) |dist[i][r] - sorted_model_row_i[r]| <= B_i                 B_i: the largest bound of a pair of the row;
    (b) |dist[i][r] - model[i][idx[i][r]]|   <= B_(i, idx[i][r])    the value belongs to the index next to it;
    (c) the indices of a row are distinct, inside the data range, never i under skip_self, and -1 exactly where dist is +inf;
    (d) a row is sorted by the total order (numbers ascending, equal numbers by ascending index, NaN after every number by
        ascending index, empty slots last) on the device's own values;
    (e) NaN slots are exactly where the model has them, and empty slots exactly beyond the available pairs.

THE BOUNDS.  u = 2^-53 is the largest relative error of one correctly rounded FP64 operation.

metric 0 (cosine): the derivation of tests/_competitors_ref.py holds word for word -- the same quantities are formed in the
same way -- so B = (2 ldx + 10) u, absolute (|d| <= 2).

metric 1 (squared Euclidean, d = xnorm[i] + xnorm[j] - 2 dot): with S = sum_k |x_k y_k| and W = xnorm[i] + xnorm[j] + 2 S >= |d|
the device value collects
    the dot product      (ldx + 1) u S, as above; it enters twice: (ldx + 1) u 2 S <= (ldx + 1) u W    (doubling is exact)
    xnorm[i] + xnorm[j]  u (xnorm[i] + xnorm[j])                                     <= u W
    the difference       u |d|                                                        <= u W
(a fused multiply-add for the last step rounds once where two roundings are counted).  The norms themselves are inputs of the
definition and of the model alike.  One more unit covers the second-order terms and the model's own error (np.longdouble,
ldx 2^-64 S for its dot product):
    |d_dev - d_model| <= (ldx + 4) u W + ldx 2^-1073.
The last term is gradual underflow: a product or partial sum below the normal range is rounded absolutely, by at most 2^-1075,
not relatively; ldx of them, doubled, and the model (whose exponent range is wider) does not underflow there.  It matters for
the row scaled by 1e-200 alone.

rowsum of k kept distances, against the sum of the model's first k (every slot a number): every term is within B of the
model's by (a): k B; the k - 1 additions round partial sums of at most k D, D the largest |distance| of the row (2 for the
cosine): (k - 1) k D u.  The density (rowsum - 1) / K of the cosine lists with k = K + 1 adds its two operations: the difference
rounds a value of at most 2 k, the quotient its own value.  In all
    |dens_dev - dens_model| <= (k B + (k - 1) 2 k u + 2 k u) / K + u |dens|.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _competitors_ref as cref  # noqa: E402

GOLD = cref.GOLD
MARGIN = cref.MARGIN
SUD_FIXTURES = ["sud_usps500", "sud_synth150", "sud_synth150_K3"]
U = 2.0 ** -53
LD = np.longdouble

load = cref.load


def pair_model(X, xnorm, metric, q, c):
    """(d[i][j] of the DEFINITION in np.longdouble, the bound of every pair) for the query rows q = (q0, q1) and the data
    rows c = (c0, c1).  The norms are the FP64 inputs, as the kernel gets them."""
    X = np.asarray(X, dtype=np.float64)
    ldx = (X.shape[1] + 15) // 16 * 16
    Q, C = X[q[0]:q[1]], X[c[0]:c[1]]
    qn, cn = np.asarray(xnorm, dtype=np.float64)[q[0]:q[1]], np.asarray(xnorm, dtype=np.float64)[c[0]:c[1]]
    if metric == 0:
        return cref.pair_model(Q, qn, C, cn), np.full((len(Q), len(C)), cref.bound(ldx))
    dot = np.asarray(Q, dtype=LD) @ np.asarray(C, dtype=LD).T
    d = np.asarray(qn, dtype=LD)[:, None] + np.asarray(cn, dtype=LD)[None, :] - 2 * dot
    W = qn[:, None] + cn[None, :] + 2 * (np.abs(Q) @ np.abs(C).T)
    return d, (ldx + 4) * U * W * (1 + 1e-12) + ldx * 2.0 ** -1073       # W is itself an FP64 sum of positive terms: good to (d + 3) u relative


def order(values, ids):
    """The positions of `values` (any float type) in the total order, `ids` their indices."""
    nan = np.isnan(values)
    return np.lexsort((ids, np.where(nan, 0, values), nan))


def model_lists(X, xnorm, metric, k, skip_self, q=None, c=None):
    """The model's own answer: (idx int64 [nq][k], dist longdouble [nq][k]) by the total order, +inf / -1 beyond the pairs."""
    n = len(X)
    q, c = q or (0, n), c or (0, n)
    d, _ = pair_model(X, xnorm, metric, q, c)
    nq = q[1] - q[0]
    idx = np.full((nq, k), -1, dtype=np.int64)
    dist = np.full((nq, k), np.inf, dtype=LD)
    ids = np.arange(c[0], c[1])
    for r in range(nq):
        ok = ids != q[0] + r if skip_self else np.ones(len(ids), dtype=bool)
        o = order(d[r][ok], ids[ok])[:k]
        idx[r, :len(o)], dist[r, :len(o)] = ids[ok][o], d[r][ok][o]
    return idx, dist


def check(idx, dist, X, xnorm, metric, k, skip_self, q=None, c=None, pairs=None):
    """Raises AssertionError unless (idx, dist) -- numpy, [nq][k] -- pass (a) .. (e) of the module docstring.  Returns the
    largest ratio of an error to its bound.  pairs: pair_model(X, xnorm, metric, (0, n), (0, n)) of at least these rows,
    computed once by a caller that checks several results on the same rows."""
    n = len(X)
    q, c = q or (0, n), c or (0, n)
    idx, dist = np.asarray(idx), np.asarray(dist)
    nq = q[1] - q[0]
    assert idx.shape == dist.shape == (nq, k), (idx.shape, dist.shape)
    if pairs is None:
        d, B = pair_model(X, xnorm, metric, q, c)
    else:
        d, B = pairs[0][q[0]:q[1], c[0]:c[1]], pairs[1][q[0]:q[1], c[0]:c[1]]
    ids = np.arange(c[0], c[1])
    worst = 0.0
    for r in range(nq):
        i = q[0] + r
        ok = ids != i if skip_self else np.ones(len(ids), dtype=bool)
        avail = int(ok.sum())
        gi, gd = idx[r], dist[r]
        # (c) and the empty slots of (e)
        assert np.array_equal(gi == -1, np.isposinf(gd)), "row %d: -1 and +inf do not go together: %s %s" % (i, gi, gd)
        assert np.array_equal(gi == -1, np.arange(k) >= avail), "row %d: empty slots %s with %d pairs" % (i, gi, avail)
        real = gi[gi >= 0]
        assert ((real >= c[0]) & (real < c[1])).all(), "row %d: an index outside the data range: %s" % (i, gi)
        assert len(set(real.tolist())) == len(real), "row %d: an index twice: %s" % (i, gi)
        assert not (skip_self and (real == i).any()), "row %d: the row itself is in its list" % i
        # (d)
        rank = np.where(gi < 0, 2, np.where(np.isnan(gd), 1, 0))
        key = list(zip(rank.tolist(), np.where(rank == 0, gd, 0.0).tolist(), np.where(rank == 2, 0, gi).tolist()))
        for s in range(k - 1):
            assert key[s] < key[s + 1] or rank[s] == rank[s + 1] == 2, "row %d: slots %d, %d are not in order: %s %s" % (i, s, s + 1, gi, gd)
        # (e) and (a)
        o = order(d[r][ok], ids[ok])[:k]
        want = d[r][ok][o]
        m = len(want)
        assert np.array_equal(np.isnan(gd[:m]), np.isnan(want)), "row %d: NaN slots %s, the model's %s" % (i, gd, want)
        num = ~np.isnan(want)
        if num.any():
            Bi = B[r][ok].max()
            with np.errstate(invalid="ignore"):
                err = np.abs(gd[:m][num].astype(LD) - want[num])
            err = np.where(gd[:m][num].astype(LD) == want[num], 0, np.where(np.isnan(err), np.inf, err))     # inf - inf
            assert (err <= Bi).all(), "row %d: (a) an order statistic is off by %g, bound %g" % (i, float(err.max()), Bi)
            worst = max(worst, float(err.max() / Bi) if Bi > 0 else 0.0)
            # (b)
            at = real[:m][num] - c[0]
            err = np.abs(gd[:m][num].astype(LD) - d[r][at])
            err = np.where(np.isnan(err), np.inf, err)
            assert (err <= B[r][at]).all(), "row %d: (b) a value does not belong to its index: off by %g" % (i, float(err.max()))
    return worst


def rowsum_bound(k, B, D=2.0):
    return k * B + (k - 1) * k * D * U


def density_bound(K, ldx, dens):
    k = K + 1
    return (rowsum_bound(k, cref.bound(ldx)) + 2 * k * U) / K + U * np.abs(dens)


def model_density(X, xnorm, K):
    """The reference's expression on the model's lists (np.longdouble)."""
    _, dist = model_lists(X, xnorm, 0, K + 1, False)
    return (dist.sum(axis=1) - 1) / K
