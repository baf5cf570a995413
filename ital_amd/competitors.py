"""TCAL and RBMAL on the device GP state: the two comparison learners of the reference (ital/baseline_methods.py:477-571)
that need nothing beyond what a session already holds -- the GP state, the feature rows and the labelled rows.

RBMAL (Cardoso et al., ranked batch-mode active learning) trades the uncertainty of a candidate against its cosine distance
to the nearest labelled sample.  The reference forms that distance with scipy's cdist over all candidates and all labelled
samples in every greedy step; here it is `ital_cosine_min` (include/ital_cosine.h: FP64 MFMA over the rows in the store's
element type), its result stays on the device between fetches, and a fetch folds in only the rows labelled since the last.

TCAL (Demir & Bruzzone, triple criteria active learning) clusters the unc_factor * k samples nearest the decision boundary
into k groups by kernel k-means and returns the densest sample of every group.  It works on a few dozen samples: the prior
kernel among them comes from `ital_cov_block`, the rest is host numpy (ital_amd/_kernel_kmeans.py).

The selection rules are functions of arrays (`rbmal_uncertainty`, `rbmal_select`, `tcal_uncertain`, `tcal_select`), so that
they are tested without a device against what the reference recorded.
"""
import numpy as np
import torch
from scipy.special import ndtr

from . import _lib
from ._kernel_kmeans import kernel_kmeans
from ._lib import check
from .gp import _pad16, _ptr, _stream
from .retrieval_base import ActiveRetrievalBase


# ------------------------------------------------------------------------------------------------------ RBMAL
def rbmal_uncertainty(mean, var, noise):
    """1 - |1 - 2 P(irrelevant)| with P(irrelevant) = norm.cdf(0, mean, sqrt(var + noise)) (baseline_methods.py:489-491)."""
    irr = ndtr((0 - mean) / np.sqrt(var + noise))
    return 1.0 - np.abs(1.0 - 2 * irr)


def rbmal_select(dist, unc, n_train, k, steps=None):
    """The greedy loop of reference baseline_methods.py:496-513 over the candidates' distances and uncertainties (arrays in
    candidate order): positions of the picks in that order.  k - 1 picks, as the reference's `range(1, k)` makes them, and
    the same `dist` in every step (the reference's train list does not grow inside the loop): only alpha moves.  `steps`, if
    a list, receives (alpha, scores, positions still in the list) of every step."""
    dist, unc = np.asarray(dist, dtype=np.float64), np.asarray(unc, dtype=np.float64)
    left = np.arange(len(dist))
    ret = []
    for _ in range(1, k):
        alpha = len(left) / (len(left) + n_train + len(ret))
        scores = alpha * dist[left] + (1 - alpha) * unc[left]
        if steps is not None:
            steps.append((alpha, scores, left))
        best = int(np.argmax(scores))            # ValueError on an empty list, as in the reference
        ret.append(int(left[best]))
        left = np.delete(left, best)
        if len(left) == 0:
            break
    return ret


class RBMAL(ActiveRetrievalBase):
    """Ranked batch-mode active learning (reference ital/baseline_methods.py:477-513); constructor arguments as the
    reference's plus the keyword-only placement arguments.

    Two properties of the reference are part of the drop-in and kept: `fetch_unlabelled(k)` returns k - 1 samples (its loop
    is `range(1, k)`; `fetch_unlabelled(1)` returns []), and the labelled set does not grow inside the loop, so the distance
    to the nearest labelled sample is one vector for all steps of a fetch and only the weight alpha moves.

    That vector lives on the device, one value per local row, together with the list of labelled samples it was built from.
    A fetch whose list extends the kept one by a suffix folds in the new rows only (`ital_cosine_min` with accumulate = 1);
    any other change -- a revoked or changed label, rows added or removed, a reset -- builds it again.  A minimum is exact:
    the folded and the rebuilt vector are equal in bits."""

    def __init__(self, data=None, queries=[], length_scale=0.1, var=1.0, noise=1e-6, **placement):
        self._dist = None
        ActiveRetrievalBase.__init__(self, data, queries, length_scale, var, noise, **placement)
        #: what the last fetch computed (numpy): candidates, their dist and unc, the train list, alpha and scores of the first
        #: step, and `folded`: how many labelled rows the kernel read (all of them after a rebuild)
        self.last = None

    def _start_afresh(self):
        """add_data() / remove_data() / sync_data() / set_params(): the kept distances are dropped."""
        ActiveRetrievalBase._start_afresh(self)
        self._dist = None
        self.last = None

    def _nearest_labelled(self):
        """(cosine distance of every sample to its nearest labelled data sample as a full-length numpy array, the train
        list, labelled rows read).  Collective on several ranks: every rank runs the kernel on its own rows."""
        gp = self.gp
        pos = [p for p, i in enumerate(gp.ind) if i < gp.n_total]
        train = [gp.ind[p] for p in pos]
        if not train:
            raise ValueError("zero-size array to reduction operation minimum which has no identity (no labelled data sample: "
                             "the model was fitted by queries only)")
        key = (gp, gp.Xd.data_ptr(), gp.n, gp.n_total)
        kept = self._dist
        if kept is not None and kept[0][0] is gp and kept[0][1:] == key[1:] and kept[1] == train[:len(kept[1])]:
            dist, new = kept[2], pos[len(kept[1]):]
        else:
            dist, new = torch.empty(max(gp.n, 1), dtype=torch.float64, device=gp.device), pos
        if new:
            with torch.cuda.device(gp.device):
                sel = torch.as_tensor(new, dtype=torch.int64, device=gp.device)
                T, tn = gp.XT.index_select(0, sel), gp.XTn.index_select(0, sel)
                check(_lib.lib().ital_cosine_min(_ptr(gp.Xd), gp.xtype, _ptr(gp.xnorm), gp.n, gp.ldx, _ptr(T), _ptr(tn), len(new),
                                                 int(len(new) < len(pos)), _ptr(dist), _stream()))
        self._dist = (key, train, dist)
        return gp._full(dist), train, len(new)

    def fetch_unlabelled(self, k):
        """Fetches a batch of unlabelled samples (reference baseline_methods.py:486-513); list of k - 1 python ints."""
        gp = self.gp
        if gp.m == 0:
            raise RuntimeError("fetch_unlabelled() needs a fitted relevance model: call update() first or pass queries")
        mean, var = gp.predict_stored(cov_mode="diag")
        unc = rbmal_uncertainty(mean, var, gp.noise)
        self._last_batch = None
        self.last = None
        if k <= 1:
            return []
        dist, train, folded = self._nearest_labelled()
        cand = self._unseen_array()
        steps = []
        picks = rbmal_select(dist[cand], unc[cand], len(train), k, steps)
        self.last = dict(candidates=cand, dist=dist[cand], unc=unc[cand], train=train, alpha=steps[0][0], scores=steps[0][1],
                         folded=folded)
        return cand[picks].tolist()


# ------------------------------------------------------------------------------------------------------ TCAL
def tcal_uncertain(rel_mean, cand, m):
    """The m candidates of smallest |mean| in the order numpy's argpartition leaves them (baseline_methods.py:545-547): the
    order is part of the result, the initial cluster labels are assigned by position.  numpy's ValueError for m > len(cand)."""
    cand = np.asarray(cand)
    return cand[np.argpartition(np.abs(np.asarray(rel_mean)[cand]), m - 1)[:m]]


def tcal_select(K, k, rng=None, info=None):
    """Clusters the samples of the kernel matrix `K` into k groups and returns the position of the densest member of every
    group, in group order (baseline_methods.py:549-571).  When a cluster runs empty the clustering is repeated with one
    cluster fewer (the list is then shorter than k); the ValueError is passed on when no cluster is left.  The density of a
    member is its mean squared kernel distance K_aa + K_bb - 2 K_ab to the members of its group; a group of two is an exact
    tie on a symmetric K and goes to its first member.  `info`, if a dict, receives the labels of the clustering that
    succeeded, the number of clusterings and the densities of every group."""
    K = np.asarray(K, dtype=np.float64)
    clusterings = 0
    while True:
        clusterings += 1
        try:
            labels = kernel_kmeans(K, k, rng=rng)
            break
        except ValueError:
            k -= 1
            if k == 0:
                raise
    ret, densities = [], []
    for i in range(k):
        members = np.flatnonzero(labels == i)
        Kc = K[np.ix_(members, members)]
        d = np.diag(Kc)
        dens = np.mean(d[:, None] + d[None, :] - 2 * Kc, axis=-1)
        densities.append(dens)
        ret.append(int(members[np.argmin(dens)]))
    if info is not None:
        info.update(labels=labels, clusterings=clusterings, densities=densities)
    return ret


class TCAL(ActiveRetrievalBase):
    """Triple criteria active learning (reference ital/baseline_methods.py:517-571); constructor arguments as the
    reference's plus the keyword-only placement arguments.  `unc_factor` sets the number of samples that are clustered,
    m = unc_factor * k.  The initial cluster labels come from numpy's global legacy generator, exactly the reference's draw.
    `fetch_unlabelled(k)` with k <= 0 returns [] (the reference does not return there)."""

    def __init__(self, data=None, queries=[], length_scale=0.1, var=1.0, noise=1e-6, unc_factor=4, **placement):
        ActiveRetrievalBase.__init__(self, data, queries, length_scale, var, noise, **placement)
        self.unc_factor = unc_factor
        #: what the last fetch computed (numpy): the clustered samples `unc`, their prior kernel matrix K, the labels, the
        #: number of clusterings and the densities of every cluster
        self.last = None

    def _start_afresh(self):
        ActiveRetrievalBase._start_afresh(self)
        self.last = None

    def _prior_kernel(self, ind):
        """The prior kernel among the samples `ind` (numpy, symmetric in bits: the lower triangle of ital_cov_block's block
        with an empty whitened part, mirrored).  Collective on several ranks: the rows are gathered to every rank."""
        gp = self.gp
        ns = len(ind)
        with torch.cuda.device(gp.device):
            rows = gp._gather_rows([int(i) for i in ind])
            norms = torch.empty(ns, dtype=torch.float64, device=gp.device)
            check(gp._lib.ital_row_norms(_ptr(rows), ns, gp.ldx, _ptr(norms), _stream()))
            out = torch.empty((ns, _pad16(ns)), dtype=torch.float64, device=gp.device)
            check(gp._lib.ital_cov_block(_ptr(rows), _ptr(norms), ns, _ptr(rows), _ptr(norms), ns, gp.ldx, 0, 0, 0, 0, 0,
                                         float(self.var), float(self.length_scale), _ptr(out), out.shape[1], _stream()))
            K = out[:, :ns].cpu().numpy()
        low = np.tril(K)
        return low + np.tril(K, -1).T

    def fetch_unlabelled(self, k):
        """Fetches a batch of unlabelled samples (reference baseline_methods.py:540-571); list of python ints, shorter than
        k when the clustering had to be repeated with fewer clusters."""
        if self.gp.m == 0:
            raise RuntimeError("fetch_unlabelled() needs a fitted relevance model: call update() first or pass queries")
        self._last_batch = None
        self.last = None
        if k <= 0:
            return []
        unc = tcal_uncertain(self.rel_mean, self._unseen_array(), self.unc_factor * k)
        K = self._prior_kernel(unc)
        info = {}
        picks = tcal_select(K, k, info=info)
        self.last = dict(unc=unc, K=K, **info)
        return unc[picks].tolist()


LEARNERS = {"TCAL": TCAL, "RBMAL": RBMAL}
