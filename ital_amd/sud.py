"""SUD on the device GP state: sampling by uncertainty and density (Zhu et al., COLING 2008), the reference's
ital/baseline_methods.py:440-473.

A candidate's score is the entropy of its predicted label times its density: the mean cosine distance to its K nearest
neighbours in the WHOLE data set.  The reference forms that with scipy's cdist over all candidates and all samples in every
fetch, an N x N product per round; but the density of a sample depends on the data alone.  Here it is one vector per store,
computed once by `ital_knn_rows` (include/ital_knn.h: a tiled FP64 MFMA self-join that keeps the K + 1 best per row and never
stores a distance tile), kept on the device and shared by every session on that store (`DeviceData.neighbour_density`).  A
learner on plain numpy data computes the same vector from the GP's own rows and keeps it itself.

The selection rule is two functions of arrays (`sud_uncertainty`, `sud_select`), tested without a device against what the
reference recorded.
"""
import numpy as np
from scipy.special import ndtr

from .device_data import check_density_k, neighbour_lists
from .retrieval_base import ActiveRetrievalBase


def sud_uncertainty(mean, var, noise):
    """The binary entropy of P(irrelevant) = norm.cdf(0, mean, sqrt(var + noise)) clipped to [1e-8, 1 - 1e-8]
    (baseline_methods.py:464-466)."""
    irr = np.maximum(1e-8, np.minimum(1.0 - 1e-8, ndtr((0 - np.asarray(mean)) / np.sqrt(np.asarray(var) + noise))))
    rel = 1.0 - irr
    return -1 * (rel * np.log(rel) + irr * np.log(irr))


def sud_select(unc, dens, k):
    """Positions of the k largest products of uncertainty and density, largest first (baseline_methods.py:472-473): numpy's
    argsort reversed, so a NaN score (the density of a zero row) is taken first, as in the reference."""
    return np.argsort(np.asarray(unc) * np.asarray(dens))[::-1][:k]


class SUD(ActiveRetrievalBase):
    """Sampling by uncertainty and density (reference ital/baseline_methods.py:440-473); constructor arguments as the
    reference's plus the keyword-only placement arguments.  `K`: the number of nearest neighbours of the density, at most 31.

    The densities are the reference's expression, its `- 1.0` included (the K + 1 nearest of a sample contain the sample
    itself at distance 0; the reference subtracts 1 where 0 would remove it), so tight neighbourhoods have negative densities.
    Row sharding is not supported: neighbour lists across the shards of several ranks are not built."""

    def __init__(self, data=None, queries=[], length_scale=0.1, var=1.0, noise=1e-6, K=20, **placement):
        if int(placement.get("world", 1)) > 1:
            raise NotImplementedError("SUD needs neighbour lists over all rows: they are not built across row shards")
        self.K = K
        self._lists = {}              # a learner on plain numpy data keeps its neighbour lists itself
        self._dens_host = None
        ActiveRetrievalBase.__init__(self, data, queries, length_scale, var, noise, **placement)
        #: what the last fetch computed (numpy): candidates, their unc, densities and scores
        self.last = None

    def _start_afresh(self):
        """add_data() / remove_data() / sync_data() / set_params(): what the learner keeps is dropped."""
        ActiveRetrievalBase._start_afresh(self)
        self._lists = {}
        self._dens_host = None
        self.last = None

    def _densities(self):
        """The density of every sample this learner knows: (device vector, its numpy copy).  The copy is kept while the
        device vector is the same one."""
        gp = self.gp
        if gp.store is not None:
            dens = gp.store.neighbour_density(self.K, view=(gp.Xd, gp.xnorm, gp.n))
        else:
            K = check_density_k(self.K, gp.n)
            dens = neighbour_lists(self._lists, gp.Xd, gp.xnorm, gp.n, "cosine", K + 1, False).densities()
        if self._dens_host is None or self._dens_host[0] is not dens:
            self._dens_host = (dens, dens.cpu().numpy())
        return self._dens_host

    def fetch_unlabelled(self, k):
        """Fetches a batch of unlabelled samples (reference baseline_methods.py:458-473); list of python ints."""
        gp = self.gp
        if gp.m == 0:
            raise RuntimeError("fetch_unlabelled() needs a fitted relevance model: call update() first or pass queries")
        self._last_batch = None
        self.last = None
        cand = self._unseen_array()
        mean, var = gp.predict_stored(cand, cov_mode="diag")
        unc = sud_uncertainty(mean, var, gp.noise)
        dens = self._densities()[1][cand]
        picks = sud_select(unc, dens, k)
        self.last = dict(candidates=cand, unc=unc, densities=dens, scores=unc * dens)
        return cand[picks].tolist()
