"""Learner API -- the drop-in boundary (mirror of reference ital/retrieval_base.py `ActiveRetrievalBase`).

Same constructor arguments, methods (fit / reset / top_results / get_unseen / fetch_unlabelled / update /
partition_feedback), attributes (gp, rel_mean, relevant_ids, irrelevant_ids, unnameable_ids, rounds, data,
queries) and error behaviour; the GP behind it is the streaming MI355X one (ital_amd.gp).
Keyword-only extras: device, rank, world, group (row sharding over GPUs).

This file IS the drop-in boundary: `partition_feedback` and `updated_prediction` have one correct form -- the reference's
(retrieval_base.py:129-193: same branches, same error message, same ordering of the ids) -- and restate it; everything
below them (GP state, candidate bookkeeping, the device path) is this package's own.
"""
import numpy as np

import copy

from . import tune
from .device_data import DeviceData
from .gp import GaussianProcess


class IdSet(set):
    """A set that counts its in-place changes (`changes`): what the learners keep their relevant / irrelevant / unnameable
    ids in (public attributes of the reference, retrieval_base.py:50-52).  Behaves as a set everywhere else."""

    _serial = 0      # process-wide: a freshly wrapped set never starts at a token value an earlier wrapper held

    def __init__(self, *a):
        set.__init__(self, *a)
        IdSet._serial += 1 << 20
        self.changes = IdSet._serial


def _counting(name):
    base = getattr(set, name)

    def method(self, *a, **kw):
        self.changes += 1
        return base(self, *a, **kw)
    method.__name__ = name
    method.__doc__ = base.__doc__
    return method


for _name in ("add", "discard", "remove", "pop", "clear", "update", "difference_update", "intersection_update",
              "symmetric_difference_update", "__ior__", "__iand__", "__isub__", "__ixor__"):
    setattr(IdSet, _name, _counting(_name))
del _name


class UnseenList(object):
    """The ascending list of samples without feedback (reference retrieval_base.py:78-87) as an ascending base array plus a
    short sorted list of ids taken out of it since: what a round of the retrieval loop needs from the list -- its length,
    the number of entries below a row boundary, the entries of one rank's rows -- costs O(k log N) per round instead of a
    copy of the N-sized array (8 MB at a million samples, on the critical path of every rank whatever the number of ranks).
    The array itself is only formed for callers that read it (get_unseen(), the options that restrict or subsample the
    list).  `version` counts the removals: the candidate list a device holds is described by the version it was built
    from (ital.py)."""

    REBASE_AT = 4096         # removed ids from which a materialisation also becomes the new base

    def __init__(self, base):
        self.base = base                     # ascending int64 array, never written to
        self.removed = []                    # ascending python ints, all members of base
        self.version = 0
        self.last_removed = ()               # the ids of the last remove() (version - 1 -> version)
        self._flat = base                    # the list as an array (None: not formed since the last removal)
        self._prev_flat = None               # (array before the last removal, the ids it lost): one pass forms the next one

    def __len__(self):
        return len(self.base) - len(self.removed)

    def count_below(self, x):
        """Number of list entries < x (= list position of the first entry >= x)."""
        import bisect
        return int(np.searchsorted(self.base, x)) - bisect.bisect_left(self.removed, x)

    def remove(self, ids):
        """Takes `ids` (distinct) out of the list; False (list unchanged) when one of them is not on it."""
        import bisect
        ids = sorted(set(int(i) for i in ids))
        if not ids:
            return True
        arr = np.asarray(ids, dtype=np.int64)
        at = np.searchsorted(self.base, arr)
        if np.any(at >= len(self.base)) or np.any(self.base[np.minimum(at, len(self.base) - 1)] != arr):
            return False
        for i in ids:
            j = bisect.bisect_left(self.removed, i)
            if j < len(self.removed) and self.removed[j] == i:
                return False
        prev = self._flat
        for i in ids:
            bisect.insort(self.removed, i)
        self.version += 1
        self.last_removed = tuple(ids)
        self._flat, self._prev_flat = None, (prev, arr) if prev is not None else None
        return True

    def in_rows(self, row0, row1):
        """The list entries in [row0, row1) as an array: O(entries returned)."""
        import bisect
        a, b = int(np.searchsorted(self.base, row0)), int(np.searchsorted(self.base, row1))
        part = self.base[a:b]
        r0, r1 = bisect.bisect_left(self.removed, row0), bisect.bisect_left(self.removed, row1)
        if r1 > r0:
            part = np.delete(part, np.searchsorted(part, np.asarray(self.removed[r0:r1], dtype=np.int64)))
        return part

    def array(self):
        """The whole list as an int64 array (treat as read-only; the same object until the next removal)."""
        if self._flat is None:
            prev = self._prev_flat
            if prev is not None:             # the array before the last removal is at hand: one pass over it
                self._flat = np.delete(prev[0], np.searchsorted(prev[0], prev[1]))
            else:
                self._flat = np.delete(self.base, np.searchsorted(self.base, np.asarray(self.removed, dtype=np.int64)))
            self._prev_flat = None
            if len(self.removed) >= self.REBASE_AT:
                self.base, self.removed = self._flat, []
        return self._flat


def label_disagreement(label, loo_mean, loo_var):
    """Probability that the model, fitted to all the OTHER labels, gives a labelled sample the opposite sign:
    ndtr(-y * loo_mean / sqrt(loo_var)) of the leave-one-out predictive distribution (R&W 5.12)."""
    from scipy.special import ndtr
    label, loo_mean, loo_var = (np.asarray(a, dtype=np.float64) for a in (label, loo_mean, loo_var))
    with np.errstate(invalid="ignore", divide="ignore"):
        return ndtr(-label * loo_mean / np.sqrt(loo_var))


def mistake_posterior(disagreement, q):
    """Posterior probability that a label is a slip, from the prior flip probability q and the disagreement d of the other
    labels with it: q d / (q d + (1 - q)(1 - d)).  None without a prior in (0, 1)."""
    if q is None or not (0.0 < float(q) < 1.0):
        return None
    q, d = float(q), np.asarray(disagreement, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return q * d / (q * d + (1.0 - q) * (1.0 - d))


class ActiveRetrievalBase(object):

    #: initial capacity of the labelled set on the device (None: GaussianProcess picks it; it grows on demand)
    gp_capacity = None

    def __init__(self, data=None, queries=[], length_scale=0.1, var=1.0, noise=1e-6, *, device=None, rank=0,
                 world=1, group=None):
        self.length_scale = length_scale
        self.var = var
        self.noise = noise
        self.device, self.rank, self.world, self.group = device, rank, world, group
        self.fit(data, queries)

    def fit(self, data, queries=[]):
        """reference retrieval_base.py:34-45.  `data`: an array; or a DeviceData (rows on the device, shared by every learner
        built on it), or a torch tensor, which becomes a DeviceData of this learner's own -- `self.data` is then that store."""
        if data is not None and not isinstance(data, DeviceData):
            import torch
            if isinstance(data, torch.Tensor):
                if self.world > 1:
                    raise NotImplementedError("a tensor is kept as a DeviceData, which is not sharded: pass ShardedRows to several ranks")
                data = DeviceData(data, device=self.device)
        self.data = data
        self.queries = queries
        if self.data is not None:
            self.gp = GaussianProcess(self.data, self.length_scale, self.var, self.noise, device=self.device,
                                      rank=self.rank, world=self.world, group=self.group, capacity=self.gp_capacity)
            self.reset()
        else:
            self.gp = None

    def _num_samples(self):
        """len(self.data) -- except on a DeviceData that has grown since this learner last called sync_data(): the learner
        goes on on the rows it knows."""
        gp = self.__dict__.get("gp")
        return gp.n_total if gp is not None and gp.store is not None else len(self.data)

    def reset(self):
        """reference retrieval_base.py:48-61"""
        self.rounds = 0
        self.relevant_ids = set()
        self.irrelevant_ids = set()
        self.unnameable_ids = set()
        self._last_batch = None
        self.gp.reset()
        if len(self.queries) > 0:
            n = self._num_samples()
            self.gp.update_points(self.queries, [1] * len(self.queries), ind=list(range(n, n + len(self.queries))))
            self._fitted = True
        else:
            self._fitted = False

    # ------------------------------------------------------------------ checkpoint / resume (the
    # reference has none: its state dies with the process)
    def state_dict(self):
        """Everything needed to continue a retrieval session in another process: the labelled set in insertion order with
        the sizes of the update() calls that built it, the id sets, the round counter and the position of the replayed
        mvndst stream and the state of numpy's global legacy generator (what MCMI_min(subsample), the change-estimation
        subset and the Monte-Carlo switches draw from, as the reference does).  Small (O(labelled samples)): the whitened
        block V is rebuilt on load, not stored -- the replay appends sample by sample where the session appended staged
        batches, so the means agree to ~1e-15, not bit for bit (a pick at an exact numerical tie may differ).  The entry
        `label_noise` (set_label_noise; aligned with `ind`) is there only when some label carries extra noise."""
        from . import mvn_stream
        gp = self.gp
        sd = dict(version=1, n=self._num_samples(), hyper=(float(self.length_scale), float(self.var), float(self.noise)),
                  ind=[int(i) for i in gp.ind], y=(gp.y.copy() if gp.y is not None else np.zeros(0)),
                  appends=list(gp.appends), relevant_ids=sorted(self.relevant_ids),
                  irrelevant_ids=sorted(self.irrelevant_ids), unnameable_ids=sorted(self.unnameable_ids),
                  rounds=int(self.rounds), mvn_stream=(tuple(mvn_stream.GLOBAL.state), int(mvn_stream.GLOBAL.draws)),
                  np_random=np.random.get_state())
        if np.any(gp.label_noise != 0):
            # only a session with weighted labels has the entry: every other dict is what it was before there were any
            sd["label_noise"] = gp.label_noise.copy()          # aligned with ind
        return sd

    def load_state_dict(self, sd, restore_stream=True):
        """Restores a session saved by state_dict() on a learner constructed over the same data (and queries) with the same
        hyper-parameters: reset(), then the same sequence of appends to the GP (same kernels, same order: the predictive
        means equal the saved session's to ~1e-15), the id sets, the round counter and -- unless told otherwise -- the
        process-wide positions of the two random streams (mvndst's, numpy's global generator).  Collective on several ranks,
        like update()."""
        from . import mvn_stream
        if sd.get("version") != 1 or sd["n"] != self._num_samples():
            raise ValueError("state_dict of another data set / version")
        if tuple(sd["hyper"]) != (float(self.length_scale), float(self.var), float(self.noise)):
            raise ValueError("state_dict was saved with other hyper-parameters: %r" % (sd["hyper"],))
        self.reset()
        at = self.gp.m                       # queries, if any, are back in place after reset()
        ind, y = list(sd["ind"]), np.asarray(sd["y"], dtype=np.float64)
        for c in sd["appends"]:
            if c < 0:
                continue                     # the queries' own append: done by reset()
            if c:
                self.gp.update(ind[at:at + c], y[at:at + c])
            at += c
        if self.gp.ind != ind:
            raise ValueError("state_dict does not match this learner's queries")
        extra = sd.get("label_noise")
        if extra is not None:
            extra = np.asarray(extra, dtype=np.float64).reshape(-1)
            if len(extra) != len(ind):
                raise ValueError("state_dict's label_noise does not match its labelled set")
            pos = np.flatnonzero(extra)
            self.gp.reweigh([ind[p] for p in pos], extra[pos])
        self.relevant_ids = set(sd["relevant_ids"])
        self.irrelevant_ids = set(sd["irrelevant_ids"])
        self.unnameable_ids = set(sd["unnameable_ids"])
        self.rounds = int(sd["rounds"])
        self._fitted = self.gp.m > 0
        if restore_stream:
            mvn_stream.GLOBAL.state, mvn_stream.GLOBAL.draws = tuple(sd["mvn_stream"][0]), int(sd["mvn_stream"][1])
            if sd.get("np_random") is not None:
                np.random.set_state(sd["np_random"])
        return self

    @property
    def rel_mean(self):
        """Predictive mean of every sample (numpy; None before the first update, as reference retrieval_base.py:61).
        gp.update() replicates the means on every rank's device (asynchronously, all ranks take part in update()); this
        attribute only downloads that vector when somebody reads it -- a local operation, safe to read on one rank."""
        return self.gp.mean_host() if self._fitted else None

    def top_results(self, k=None):
        """reference retrieval_base.py:64-75.  On a fitted learner the ranking is made on the device, exact, ties by descending
        index as the reversal of a stable ascending sort gives: up to ITAL_TOPK_MAX results by a selection (ital_topk), more
        of them and the complete ranking (k = None) by a sort (ital_rank_desc); only the indices returned are downloaded."""
        from ._lib import ITAL_TOPK_MAX
        if k is not None and self._fitted and 1 <= int(k) <= min(ITAL_TOPK_MAX, self._num_samples()):
            return self.gp.topk_mean(int(k))
        if self._fitted and (k is None or int(k) > ITAL_TOPK_MAX):
            return self.gp.rank_mean(None if k is None else min(int(k), self._num_samples()))
        ind = np.argsort(self.rel_mean, kind="stable")[::-1]
        return ind[:k] if k is not None else ind

    def evaluate(self, relevance, X=None):
        """Average precision and NDCG of the current model against `relevance` (+1 / -1 per sample, 0: unknown, left out),
        computed on the device (metrics.evaluate: ranking, tie groups and sums; 48 bytes come back): the scores are the
        predictive means of the stored samples, or, with `X`, those of external points (gp.predict on the device; relevance
        then has one entry per row of X) -- what the reference's experiment loop computes on the host after every round
        (run_experiment.py:154-168).  Returns {"ap", "ndcg", "n_pos", "n_neg", "n_unknown"}.  RuntimeError before any feedback;
        ValueError when no sample is relevant or a score is NaN.  Local operation on the replicated state."""
        from . import metrics
        if not self._fitted:
            raise RuntimeError("evaluate() needs a fitted model: call update() first")
        import torch
        with torch.cuda.device(self.gp.device):
            scores = self.gp.mu_all[: self._num_samples()] if X is None else self.gp.predict(X, on_device=True)
            return metrics.evaluate(scores, relevance)

    def get_unseen(self):
        """reference retrieval_base.py:78-87 (ascending sample indices, python ints)."""
        return self._unseen_array().tolist()

    # the three id sets are public attributes, as in the reference; assigning a new set to one of them (rather than going
    # through update()) invalidates the derived candidate bookkeeping
    def _set_ids(self, name, value):
        # kept as a set that counts its in-place changes (`IdSet`): the candidate bookkeeping notices ANY change made behind
        # update()'s back, also one that leaves the sizes as they were (an id swapped for another)
        # NOTE (differs from the reference, which stores the caller's object, retrieval_base.py:50-52): a plain set is COPIED
        # into an IdSet -- later changes of the caller's own set object are not seen by the learner; change `learner.<name>`
        # itself (in place, or by assigning again).  INTEGRATION.md, "id sets".
        self.__dict__[name] = value if isinstance(value, IdSet) else IdSet(value)
        self.__dict__["_unseen"] = None

    def _get_ids(self, name):
        try:
            return self.__dict__[name]
        except KeyError:
            raise AttributeError(name[1:]) from None       # before fit() / reset(), as an attribute never assigned

    relevant_ids = property(lambda self: self._get_ids("_relevant_ids"), lambda self, v: self._set_ids("_relevant_ids", v))
    irrelevant_ids = property(lambda self: self._get_ids("_irrelevant_ids"), lambda self, v: self._set_ids("_irrelevant_ids", v))
    unnameable_ids = property(lambda self: self._get_ids("_unnameable_ids"), lambda self, v: self._set_ids("_unnameable_ids", v))

    def _id_sizes(self):
        """Token of the three id sets' state: sizes and change counters."""
        sets = (self.relevant_ids, self.irrelevant_ids, self.unnameable_ids)
        return tuple(len(q) for q in sets) + tuple(getattr(q, "changes", -1) for q in sets)

    def _unseen_list(self):
        """The samples without feedback as an UnseenList, kept between calls: update() takes the newly seen samples out of
        it (O(k log N)).  Rebuilt from the three id sets (N-sized work) when they were changed behind update()'s back:
        a set assigned anew, or sizes that no longer match what update() left."""
        u = self.__dict__.get("_unseen")
        if u is not None and u[1] == self._id_sizes():
            return u[0]
        seen = self.relevant_ids | self.irrelevant_ids | self.unnameable_ids
        if not seen:
            arr = np.arange(self._num_samples(), dtype=np.int64)
        else:
            mask = np.ones(self._num_samples(), dtype=bool)
            mask[np.fromiter(seen, dtype=np.int64, count=len(seen))] = False
            arr = np.flatnonzero(mask)
        lst = UnseenList(arr)
        self.__dict__["_unseen"] = (lst, self._id_sizes())
        return lst

    def _unseen_array(self):
        """Ascending indices of the samples without feedback (int64 array; treat as read-only)."""
        return self._unseen_list().array()

    def _unseen_after(self, new_ids, sizes_before):
        """Called by update() once the id sets hold `new_ids` (samples that had no feedback before): the kept list loses
        them (the device keeps its candidate list the same way, ital.py)."""
        u = self.__dict__.get("_unseen")
        if u is None or u[1] != sizes_before:
            self.__dict__["_unseen"] = None
            return
        ids = set(int(i) for i in new_ids)
        if not u[0].remove(ids):
            self.__dict__["_unseen"] = None        # feedback for something that was not a candidate: rebuild next time
            return
        self.__dict__["_unseen"] = (u[0], self._id_sizes())

    def fetch_unlabelled(self, k):
        raise NotImplementedError('fetch_unlabelled() has to be implemented in a derived class.')

    def update(self, feedback):
        """reference retrieval_base.py:105-126"""
        rel, irr, unnameable = self.partition_feedback(feedback)
        sizes_before = self._id_sizes()
        if len(rel) + len(irr) > 0:
            self.gp.update(rel + irr, np.concatenate((np.ones(len(rel)), -1 * np.ones(len(irr)))),
                           row_cache=self._batch_rows())
            self._fitted = True
            self.relevant_ids.update(rel)
            self.irrelevant_ids.update(irr)
            self.rounds += 1
        new_unnameable = [i for i in unnameable if i not in self.unnameable_ids]
        self.unnameable_ids.update(unnameable)
        self._unseen_after(rel + irr + new_unnameable, sizes_before)

    def revoke(self, ids):
        """Takes the feedback for `ids` back: they leave the relevant / irrelevant / unnameable ids and -- the labelled ones
        -- the GP (GaussianProcess.remove: a Cholesky row deletion and one sweep on the device), and are candidates again.
        The reference has no way back from a label (RuntimeError 'Cannot change feedback once given.',
        retrieval_base.py:183-189) short of reset() and a replay of the surviving feedback, gp.py:141-161.  `rounds` stays
        as it is.  ValueError for an id that never got feedback (nothing is changed then).  Several ranks: every rank makes
        the same call, like update()."""
        ids = list(dict.fromkeys(int(i) for i in ids))
        for i in ids:
            if not (i in self.relevant_ids or i in self.irrelevant_ids or i in self.unnameable_ids):
                raise ValueError("sample %d never got feedback" % i)
        labelled = [i for i in ids if i in self.relevant_ids or i in self.irrelevant_ids]
        if labelled:
            self.gp.remove(labelled)
        for i in ids:
            # in-place changes of the three IdSets: the unseen list and a device candidate list rebuild on their next use
            self.relevant_ids.discard(i)
            self.irrelevant_ids.discard(i)
            self.unnameable_ids.discard(i)
        self.__dict__["_unseen"] = None
        self._fitted = self.gp.m > 0

    def set_label_noise(self, noise_by_id):
        """Keeps labels but trusts them less: `noise_by_id` maps ids with feedback to the extra noise variance (>= 0) their
        label carries from now on (GaussianProcess.reweigh: Cholesky up- and downdates and one sweep on the device).  The
        value is absolute; 0 gives a label its full weight back, a large one approaches revoke([id]).  The id sets, the unseen
        list, `rounds` and both random streams stay as they are; the prepared next round and the batch state of the last
        fetch are dropped.  ValueError (nothing changed) for an id that is neither relevant nor irrelevant -- an unnameable
        one has no label -- and for a negative or non-finite value.  Several ranks: every rank makes the same call."""
        ids = [int(i) for i in noise_by_id]
        for i in ids:
            if not (i in self.relevant_ids or i in self.irrelevant_ids):
                raise ValueError("sample %d has no label" % i)
        self.gp.reweigh(ids, [float(noise_by_id[i]) for i in noise_by_id])
        self._last_batch = None
        rb = getattr(self, "_round_bufs", None)
        if rb is not None:
            rb.drop_prepared()

    def label_noise(self):
        """{id: extra noise variance} of the labels that carry some (set_label_noise)."""
        gp = self.gp
        return {int(gp.ind[p]): float(gp.label_noise[p]) for p in np.flatnonzero(gp.label_noise)}

    def audit(self, mistake_prob=None, unseen_only=True):
        """Which labels deserve a second look, and what taking each of them back would change -- for all labelled data
        samples in one pass on the device (GaussianProcess.influence), with no change of state; what clone() + revoke([i])
        per label answers with m copies of the whitened block.  Query rows are left out: they cannot be revoked.  Returns a
        dict of arrays over the labelled data samples in labelled order: ids; label (+1 / -1); loo_mean, loo_var, the
        prediction for the sample from all the other labels; disagreement, the probability that this prediction has the
        opposite sign; p_mistake, its posterior with the prior flip probability `mistake_prob` (default: the learner's own
        `mistake_prob` when it has one in (0, 1); else None); dmu_rms, dmu_max, flips, ds2: root mean square and maximum
        of the change of the predictive mean, number of rows whose mean changes sign and total variance the label removes,
        over the unseen samples (`unseen_only`, the rows a user still acts on) or over every data row; order, the positions
        sorted by disagreement, largest first, ties by position.  RuntimeError before any feedback.  Several ranks: every
        rank makes the call."""
        gp = self.gp
        n = self._num_samples()
        pos = [p for p, i in enumerate(gp.ind) if i < n] if self._fitted else []
        if not pos:
            raise RuntimeError("audit() needs feedback: call update() first")
        mask = None
        counted = n
        if unseen_only:
            unseen = self._unseen_array()
            mask = np.zeros(n, dtype=bool)
            mask[unseen] = True
            counted = len(unseen)
        inf = gp.influence(mask)
        pos = np.asarray(pos, dtype=np.int64)
        label = np.asarray(gp.y, dtype=np.float64)[pos]
        loo_mean, loo_var = inf["loo_mean"][pos], inf["loo_var"][pos]
        d = label_disagreement(label, loo_mean, loo_var)
        q = mistake_prob if mistake_prob is not None else getattr(self, "mistake_prob", None)
        with np.errstate(invalid="ignore", divide="ignore"):
            rms = np.sqrt(inf["dmu_sq"][pos] / counted) if counted else np.zeros(len(pos))
        return dict(ids=np.asarray(gp.ind, dtype=np.int64)[pos], label=label, loo_mean=loo_mean, loo_var=loo_var,
                    disagreement=d, p_mistake=mistake_posterior(d, q), dmu_rms=rms, dmu_max=inf["dmu_max"][pos],
                    flips=inf["flips"][pos], ds2=inf["ds2"][pos], order=np.argsort(-d, kind="stable"))

    def preview_revoke(self, ids):
        """(rel_mean, var) of every sample as they would be after revoke([i]), one row per id (each row takes that id alone
        back), with no change of state (GaussianProcess.preview_remove).  ValueError for an id that never got feedback; an
        unnameable id has no label to lose, its row is the current state."""
        ids = [int(i) for i in ids]
        for i in ids:
            if not (i in self.relevant_ids or i in self.irrelevant_ids or i in self.unnameable_ids):
                raise ValueError("sample %d never got feedback" % i)
        labelled = [i for i in ids if i in self.relevant_ids or i in self.irrelevant_ids]
        n = self._num_samples()
        mean, var = np.empty((len(ids), n)), np.empty((len(ids), n))
        if labelled:
            lm, lv = self.gp.preview_remove(labelled)
        if len(labelled) < len(ids):
            if self._fitted:
                cm, cv = self.gp.predict_stored(cov_mode='diag')
            else:
                cm, cv = np.zeros(n), np.full(n, float(self.var))
        at = 0
        for q, i in enumerate(ids):
            if i in self.relevant_ids or i in self.irrelevant_ids:
                mean[q], var[q] = lm[at], lv[at]
                at += 1
            else:
                mean[q], var[q] = cm, cv
        return mean, var

    def _start_afresh(self):
        """What a learner derives from the data matrix or the hyper-parameters and keeps between rounds -- the cached list of
        unseen samples, the batch state of the last fetch, device buffers sized by the number of rows -- is dropped and built
        again on its next use.  The derived learners add their own."""
        self.__dict__["_unseen"] = None
        self._last_batch = None

    def add_data(self, rows):
        """Appends samples to a live session (GaussianProcess.extend): the new ones get the ids len(data) .. and are unseen;
        feedback, `rounds` and both random streams stay as they are.  The reference would need a new learner (and a new
        dense K_all, gp.py:128).  An empty array is a no-op; ValueError (nothing changed) for another number of columns;
        NotImplementedError on several ranks: row sharding cannot grow yet.  A learner on a DeviceData: store.append(rows)
        -- any input kind the store takes -- followed by sync_data(); other learners on the store catch up when they call
        sync_data() themselves."""
        if isinstance(self.data, DeviceData):
            if self.data.append(rows):
                self.sync_data()
            return self
        rows = np.asarray(rows, dtype=np.float64)
        if rows.size == 0:
            return self
        if rows.ndim != 2 or rows.shape[1] != np.shape(self.data)[1]:
            raise ValueError("rows must be a k-by-%d array" % np.shape(self.data)[1])
        if self.world > 1:
            raise NotImplementedError("row sharding cannot grow yet: add_data() needs all rows on one rank")
        self.gp.extend(rows)
        self.data = self.gp.X_host
        self._start_afresh()
        return self

    def sync_data(self):
        """A learner on a DeviceData takes in the rows the store has gained since its construction or its last sync_data()
        (GaussianProcess.sync_data: only the new range is whitened): they get the ids that follow and are unseen; feedback,
        `rounds` and both random streams stay as they are.  Rows the store has lost since (DeviceData.remove) leave the
        learner too, in the order of the store's change log: a labelled one as revoke() takes it out, the others by a gather;
        removed ids vanish from the three id sets, the surviving ids are renumbered, and `last_index_map` is the composed
        map.  Returns the number of rows gained (0 and no removal: nothing is touched).  ValueError for a learner that owns
        its rows."""
        if not isinstance(self.data, DeviceData):
            raise ValueError("this learner owns its rows: build it on a DeviceData to share and grow them")
        k = self.gp.sync_data()
        for removed in self.gp.last_removals:
            self._ids_after_removal(removed)
        if k or self.gp.last_removals:
            self._fitted = self.gp.m > 0
            self._start_afresh()
        return k

    @property
    def last_index_map(self):
        """The composed index map of the removals the last sync_data() applied (int64 array of the length the learner had:
        the new index of every sample, -1 for a removed one); None if it applied none."""
        return self.gp.last_index_map

    def _ids_after_removal(self, removed):
        """The three id sets once the samples `removed` (ascending) have left: they vanish from the sets, the surviving ids
        move down (bisection on `removed`: nothing N-sized).  New sets are assigned: the unseen list and a device candidate
        list rebuild on their next use."""
        from .device_data import remap_ids
        self.relevant_ids = remap_ids(self.relevant_ids, removed)
        self.irrelevant_ids = remap_ids(self.irrelevant_ids, removed)
        self.unnameable_ids = remap_ids(self.unnameable_ids, removed)

    def remove_data(self, ids):
        """Deletes samples from a live session, like np.delete(data, ids, axis=0): the survivors keep their order and get the
        ids 0 .. n - r - 1; returns the index map (int64 array of the old length: the new id of every sample, -1 for a
        removed one).  Removed ids vanish from the relevant / irrelevant / unnameable ids, the surviving ids are renumbered;
        a labelled sample among `ids` first leaves the GP as revoke() takes it out (a Cholesky row deletion and one sweep),
        everything else is a gather on the device that changes no bit of a survivor (GaussianProcess.drop_rows).  `rounds` and
        both random streams stay as they are.  The reference would need a new learner (and a new dense K_all, gp.py:128).

        `ids`: any iterable of ints; duplicates are collapsed, negative ones count from the end; an empty list is a no-op
        that returns the identity.  ValueError / IndexError (nothing changed) for a query row or an id outside the samples and
        for removing every sample; NotImplementedError on several ranks: row sharding cannot shrink yet.  A learner on a
        DeviceData: store.remove(ids) followed by sync_data(); other learners on the store go on on the rows they know until
        they call sync_data() themselves."""
        from .device_data import normalize_ids, removal_map
        if self.world > 1:
            raise NotImplementedError("row sharding cannot shrink yet: remove_data() needs all rows on one rank")
        n = self._num_samples()
        if isinstance(self.data, DeviceData):
            self.data.remove(ids)
            self.sync_data()
            return self.last_index_map if self.last_index_map is not None else np.arange(n, dtype=np.int64)
        ids = [int(i) for i in ids]
        for i in ids:
            if i >= n:
                raise ValueError("%d is a query row or outside the %d samples: it cannot be removed" % (i, n))
        removed = normalize_ids(ids, n)
        if not removed:
            return np.arange(n, dtype=np.int64)
        self.gp.drop_rows(removed)
        self.data = self.gp.X_host
        self._ids_after_removal(removed)
        self._fitted = self.gp.m > 0
        self._start_afresh()
        return removal_map(n, removed)

    #: attributes that hold buffers or caches of one learner's last fetch: a clone starts without them
    _FETCH_STATE = ("_unseen", "_last_batch", "_fetch_bufs", "_round_bufs", "_block_bufs", "_gram_bufs", "_err_bufs",
                    "_ce_subset", "_transport", "last", "last_scores", "last_round", "profile", "pair_counter", "host_clock")

    def clone(self):
        """A second learner of the same class and options on the same DeviceData, in this learner's state: the GP's device
        state is copied device to device (GaussianProcess.clone), the labelled set, the three id sets and `rounds` on the
        host; the buffers of the last fetch are not carried over -- the clone builds its own on its next fetch.  The two
        branches then take different feedback without a second copy of the rows: a what-if, or a session handed on.  The two
        random streams are process-wide and are not touched.  ValueError for a learner built from a numpy array."""
        if not isinstance(self.data, DeviceData):
            raise ValueError("clone() shares the rows between the two learners: build the learner on a DeviceData "
                             "(ital_amd.DeviceData(data)) instead of a numpy array")
        new = object.__new__(type(self))
        for name, value in self.__dict__.items():
            if name in self._FETCH_STATE:
                value = None
            elif isinstance(value, (list, dict)) and not isinstance(value, IdSet):
                value = copy.copy(value)
            new.__dict__[name] = value
        if "_pinned" in new.__dict__:
            new._pinned = {}
        if "event_pool" in new.__dict__:
            new.event_pool = []
        new.gp = self.gp.clone()
        new.relevant_ids, new.irrelevant_ids, new.unnameable_ids = set(self.relevant_ids), set(self.irrelevant_ids), \
            set(self.unnameable_ids)
        return new

    def set_params(self, length_scale=None, var=None, noise=None):
        """Other kernel hyper-parameters for a live session (None: as it is), e.g. the result of ital_amd.tune
        (GaussianProcess.set_params: the factor is built anew and every row whitened again in one pass per chunk of labelled
        samples).  LinAlgError for a Gram that is not positive definite; the session is then exactly as it was.  Several
        ranks: every rank makes the same call."""
        self.gp.set_params(length_scale, var, noise)
        self.length_scale, self.var, self.noise = self.gp.length_scale, self.gp.var, self.gp.noise
        self._start_afresh()
        return self

    def tune_params(self, grid=tune.default_grids['ls_only'], criterion='lml', apply=True, verbose=0):
        """Finds kernel hyper-parameters for a live session from its own labels (tune.optimize_session_params: alternating
        grid search over `grid`, every sweep scored on the device by `criterion` -- 'lml', 'loo_logp', 'loo_mse' or 'loo_ap',
        see tune.session_scores) and, with `apply`, makes them the session's (set_params).  The reference can only tune
        offline against the ground truth of the whole data set (optimize_parameters.py).  Returns (best parameters, their
        score).  LinAlgError when no candidate's Gram is positive definite; the session is then exactly as it was.
        `rounds` and both random streams stay as they are.  Several ranks: every rank makes the same call."""
        best, score = tune.optimize_session_params(self, grid, criterion=criterion, verbose=verbose)
        if score == -np.inf:
            raise np.linalg.LinAlgError("no candidate of the grid has a positive definite kernel matrix of the labelled samples")
        if apply:
            self.set_params(**best)
        return best, score

    def fit_params(self, params=tune.PARAM_NAMES, init=None, restarts=8, bounds=None, maxiter=100, apply=True, verbose=0,
                   criterion='lml'):
        """Fits kernel hyper-parameters of a live session to its own labels by maximising the log marginal likelihood from
        its gradient on the device (tune.fit_session_params: L-BFGS-B over the logarithms of `params` from `restarts`
        deterministic starting points at once, restart 0 being `init` or the session's current values) and, with `apply`,
        makes them the session's (set_params).  The continuous counterpart of tune_params(), which only finds what lies on
        its grid.  `criterion`: 'lml', or 'loo_logp' / 'loo_mse', the leave-one-out scores of tune_params, climbed from
        their gradients (GaussianProcess.loo_grad); 'loo_mse' fits at most one of var and noise.  Returns (fitted parameters,
        their score: the log marginal likelihood, loo_logp or minus loo_mse).  LinAlgError when no starting point has a
        positive definite Gram; the session is then exactly as it was.  `rounds` and both random streams stay as they are.
        Several ranks: every rank makes the same call."""
        best, lml = tune.fit_session_params(self, params, init=init, restarts=restarts, bounds=bounds, maxiter=maxiter,
                                            verbose=verbose, criterion=criterion)
        if best is None:
            raise np.linalg.LinAlgError("no starting point has a positive definite kernel matrix of the labelled samples")
        if apply:
            self.set_params(**best)
        return best, lml

    def relabel(self, feedback):
        """update(feedback) for a user who corrects themselves: the ids of `feedback` whose stored feedback differs from the
        new one are revoked first, then `feedback` is applied as update() applies it.  update() itself keeps refusing a
        changed label, as the reference does (retrieval_base.py:183-189)."""
        changed = []
        for i, fb in feedback.items():
            old = 1 if i in self.relevant_ids else -1 if i in self.irrelevant_ids else 0 if i in self.unnameable_ids else None
            new = 1 if fb > 0 else -1 if fb < 0 else 0
            if old is not None and old != new:
                changed.append(i)
        if changed:
            self.revoke(changed)
        self.update(feedback)

    def _batch_rows(self):
        """Feature rows of the last fetched batch as kept (replicated) in the device batch state, or None."""
        last = getattr(self, "_last_batch", None)
        if not last:
            return None
        b, picks = last
        return b["XB"], {int(i): slot for slot, i in enumerate(picks)}

    def updated_prediction(self, feedback, test_ind, cov_mode='full'):
        """Prediction after a simulated update with `feedback`, without performing it (reference
        retrieval_base.py:129-164)."""
        rel, irr, _ = self.partition_feedback(feedback)
        if len(rel) + len(irr) == 0:
            return self.gp.predict_stored(test_ind, cov_mode=cov_mode)
        rel.sort()
        irr.sort()
        return self.gp.updated_prediction(rel + irr, np.concatenate((np.ones(len(rel)), -1 * np.ones(len(irr)))),
                                          test_ind, cov_mode=cov_mode)

    def partition_feedback(self, feedback):
        """reference retrieval_base.py:167-193"""
        rel, irr, unnameable = [], [], []
        for i, fb in feedback.items():
            if fb > 0:
                if i in self.irrelevant_ids:
                    raise RuntimeError('Cannot change feedback once given.')
                elif i not in self.relevant_ids:
                    rel.append(i)
            elif fb < 0:
                if i in self.relevant_ids:
                    raise RuntimeError('Cannot change feedback once given.')
                elif i not in self.irrelevant_ids:
                    irr.append(i)
            else:
                unnameable.append(i)
        return rel, irr, unnameable
