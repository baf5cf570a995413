"""ITAL on MI355X: host-side mirror of reference ital/ital.py `ITAL` (drop-in learner).

`fetch_unlabelled(k)` keeps the reference's greedy batch construction (ital.py:84-134) but every stage is a HIP
kernel enqueued on one stream, with no host round trip inside a round:

    for step t = 1..k:   score all live candidates   ital_score_step      (replaces Pool.map of ital.py:124-128)
                         local arg-max + record      ital_select_local    (np.argmax, ital.py:130)
                         [all-gather of one record per rank over RCCL when world > 1]
                         winner -> batch state       ital_select_resolve  (append + del, ital.py:131-132)
                         next cross-covariance col.  ital_cross_cov_cols  (predict_cov_batch, ital.py:586)

Candidates are sharded by rows across ranks; the per-step exchange is ONE fixed-size record per rank.

This module holds the learner, the dispatch between its paths and the step-by-step fast path (`_select_steps`).  A whole
round as one call below the C ABI (`_select_round`) is `_fast_round.FastRound`, which also keeps that path's state between
rounds (`_fast_round.RoundBuffers`: the candidate list on the device, the prepared next round); the round of every other
option (`_fetch_generic`) is `_generic_round.GenericRound`, the host sampling of the Monte-Carlo switches `_mc_sampler`,
the launches and buffers all greedy loops share (selection of a step, the new member's covariance column, lattice tables,
workspace, alive flags and selection partials) `_batch`.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib, _mc_sampler, mvn_stream, sharding
from ._lib import ITAL_GENERIC_MAX_CALLS, ITAL_GENERIC_MAX_DIM, ITAL_GENERIC_MAX_REL, ITAL_MAX_T, ItalScoreDesc, check
from ._batch import (FUSED_LAUNCH_MAX as _FUSED_LAUNCH_MAX, LABEL_MODES as _LABEL_MODES, Scored, ensure_step_buffers,
                     fill_score_desc, fill_score_select, gp_model, lattice_label, lattice_tables, make_batch_buffers,
                     member_column, qmc_work, select_step)
from ._fast_round import FastRound
from ._generic_round import GenericRound
from ._mc_sampler import range_cuts as _range_cuts   # noqa: F401 -- tests/test_host_logic.py imports it from here
from .gp import _ptr, _stream
from .retrieval_base import ActiveRetrievalBase, UnseenList

_FUSED_SELECT_MAX = _lib.ITAL_ROUND_MAX_CAND   # per rank, up to this many candidates: arg-max + record (+ resolve) inside the scoring launch


class ITAL(ActiveRetrievalBase):
    """Information-theoretic Active Learning for information retrieval (reference ital/ital.py:12-134).

    Constructor arguments are the reference's (ital.py:15-81).  The perfect-user default runs on the specialised
    scorer (`ital_score_step`); every other option (user models, change-estimation subset, clip_cov, label_estimation,
    the Monte-Carlo switches) on the general one (`ital_score_generic`).  Configurations beyond the device limits
    (`_unsupported`) raise NotImplementedError at fetch time instead of silently taking another path.  `parallelized`
    is accepted and ignored (the GPU is the parallelism).
    """

    def __init__(self, data=None, queries=[], length_scale=0.1, var=1.0, noise=1e-6, label_prob=1.0,
                 mistake_prob=0.0, top_candidates=None, change_estimation_subset=0, clip_cov=0,
                 label_estimation='mean', monte_carlo_num_rel=None, monte_carlo_num_fb=None, parallelized=True, *,
                 device=None, rank=0, world=1, group=None):
        ActiveRetrievalBase.__init__(self, data, queries, length_scale, var, noise, device=device, rank=rank,
                                     world=world, group=group)
        self.label_prob = label_prob
        self.mistake_prob = mistake_prob
        self.top_candidates = top_candidates
        self.change_estimation_subset = change_estimation_subset
        self.clip_cov = clip_cov
        self.label_estimation = label_estimation
        self.monte_carlo_num_rel = monte_carlo_num_rel
        self.monte_carlo_num_fb = monte_carlo_num_fb
        self.parallelized = parallelized
        self.eps = 1e-12  # reference ital/ital.py:144
        self.last_scores = None  # per greedy step: device tensor of MI per list position (diagnostics/tests)
        self.keep_scores = False
        self.force_generic = False  # route the perfect-user case through the general scorer too (cross-check in tests)
        self._ce_subset = None
        self.qmc_work_bytes = int(os.environ.get("ITAL_QMC_WORK_BYTES", 1 << 30))   # cap of the lattice scorer's workspace
        self._last_batch = None  # (batch buffers, picks) of the last fast-path round: update() reuses the winners' rows
        self.pair_counter = None  # optional int64 device tensor [1]: the general scorer adds its evaluated (Phi, Phi^-1) pairs
        self.generic_pipeline = True   # False: the general scorer always runs as its single kernel (cross-check in tests)
        self.event_pool = []     # pre-created timing events (bench.py)
        self.profile = None      # list to receive (stage, t, size, start_event, end_event) per launch (bench.py)
        self._fetch_bufs = None
        self.profile_steps = None      # round path: greedy steps whose lattice sums are bracketed by events (None: all)
        self.round_call = True        # up to ITAL_ROUND_MAX_CAND candidates per rank: a whole round through ital_fetch_round (False: step by step from Python)
        self._round_bufs = None       # _fast_round.RoundBuffers of _fetch_bufs: what only the one-call round keeps between rounds
        self.last_round = None        # (begin, descriptor slot) of the last one-call round: how its candidate list reached the device (diagnostics / tests)
        self._transport = None        # (process group, _round_transport() for it)
        self._pinned = {}             # page-locked landing buffers of _download on several ranks
        self.select_in_scorer = True  # False: the selection of a greedy step always runs as a launch of its own (cross-check in tests)
        self.mc_walk = [0, 0, 0.0]   # Monte-Carlo pattern sampling: standard normals computed / skipped, host seconds
        self.host_clock = None       # dict(gap_s=0.0, gaps=0, enqueue_s=0.0, t_download=None): host time of the round path (bench.py)

    # ------------------------------------------------------------------ helpers
    def _perfect_user(self):
        return self.label_prob >= 1 and self.mistake_prob <= 0

    def _fb_mode(self):
        """fb_mode of ital_gscore_desc: which simulated feedback the scorer enumerates (reference ital.py:300-342)."""
        return 0 if self._perfect_user() else (1 if self.label_prob >= 1 else 2)

    def _subset_mode(self):
        return self.change_estimation_subset is None or self.change_estimation_subset > 0

    def _mc_plan(self, nr, fb_mode):
        """Which enumerations the reference replaces by sampling at a step with nr enumerated variables
        (ital.py:293-297, :318-337): (rel sampled?, patterns, feedback sampled?, feedback configurations)."""
        return _mc_sampler.mc_plan(nr, fb_mode, self.monte_carlo_num_rel, self.monte_carlo_num_fb)

    def _unsupported(self, k, n_unseen=0):
        """Reason why the device scorers cannot run this configuration (None if they can)."""
        if self.label_estimation not in _LABEL_MODES:
            return "label_estimation=%r" % (self.label_estimation,)
        if self.change_estimation_subset is None:
            # the whole candidate set is the estimation subset (ital.py:103-104): every orthant spans all candidates
            if n_unseen > ITAL_GENERIC_MAX_DIM:
                return ("change_estimation_subset=None with %d candidates: orthants of that dimension (limit %d)"
                        % (n_unseen, ITAL_GENERIC_MAX_DIM))
            sub, max_dim = n_unseen, n_unseen
        else:
            sub = self.change_estimation_subset if self.change_estimation_subset > 0 else 0
            max_dim = sub + k
        if self._needs_generic():
            if max_dim > ITAL_GENERIC_MAX_DIM:
                return "orthant dimension %d (subset + batch) above %d" % (max_dim, ITAL_GENERIC_MAX_DIM)
            if k > ITAL_GENERIC_MAX_REL:
                return "batches larger than %d with the general scorer" % ITAL_GENERIC_MAX_REL
            fb_mode = self._fb_mode()
            for nr in range(1, k + 1):
                _, npat, _, nfb = self._mc_plan(nr, fb_mode)
                if npat * (2 + nfb) > ITAL_GENERIC_MAX_CALLS:
                    return ("%d orthant probabilities per candidate at greedy step %d: set monte_carlo_num_rel / "
                            "monte_carlo_num_fb (reference ital.py:293-297)" % (npat * (2 + nfb), nr))
        elif k > ITAL_MAX_T:
            return ("batches larger than %d with full enumeration: set monte_carlo_num_rel (reference ital.py:293-297)"
                    % ITAL_MAX_T)
        return None

    def _needs_generic(self):
        return (self._subset_mode() or not self._perfect_user() or self.force_generic or self._clip_active()
                or self.monte_carlo_num_rel is not None or self.monte_carlo_num_fb is not None)

    def _clip_active(self):
        """clip_cov only ever acts on orthants of more than 5 dimensions, between 0 and 1 (reference ital.py:360)."""
        return bool(self.clip_cov) and 0 < self.clip_cov < 1

    def _mark(self, stage=None, t=0, size=0, start=None):
        """HIP event on the launch stream (only when bench.py asked for per-kernel timings).  Events come from
        `event_pool` when the caller filled it (creating a timing event costs ~0.3 ms on a loaded host)."""
        if self.profile is None:
            return None
        ev = self.event_pool.pop() if self.event_pool else torch.cuda.Event(enable_timing=True)
        ev.record()
        if start is not None:
            self.profile.append((stage, t, size, start, ev))
        return ev

    def _event(self):
        """A timing event for the library to record (handle must exist: pool events are recorded once when the pool is
        made; a fresh one is recorded here)."""
        if self.event_pool:
            return self.event_pool.pop()
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def _buffers(self, kmax):
        gp = self.gp
        b = self._fetch_bufs
        if b is not None and b["kmax"] >= kmax and b["ldw"] == gp.cap and b["gp"] is gp:
            return b
        b = make_batch_buffers(gp.device, kmax, gp.ldx, gp.cap, gp.ldv, gp.world)
        b["gp"] = gp              # fit() on an existing learner builds a new GP (other row count / dimension): new buffers
        self._fetch_bufs = b
        self._round_bufs = None
        return b

    def _start_afresh(self):
        """add_data() / set_params(): the batch buffers (keyed by the row count's ldv), the device's candidate list and the
        prepared next round start afresh."""
        ActiveRetrievalBase._start_afresh(self)
        if self._round_bufs is not None:
            self._round_bufs.drop_prepared()
            self._round_bufs.invalidate()
        self._fetch_bufs = None
        self._round_bufs = None
        self._ce_subset = None

    @property
    def _dev_list(self):
        """The candidate list the device holds (_fast_round.DeviceList); None unless the next round may follow it."""
        return None if self._round_bufs is None else self._round_bufs.device_list

    def _candidate_list(self, candidates=None):
        """Candidate list in the reference's order (ital.py:98, :111-117) as an int64 array."""
        if candidates is None:
            candidates = self._unseen_array()
        # change-estimation subset: drawn from the unrestricted candidate list on the global numpy RNG (ital.py:103-108)
        if self.change_estimation_subset is None:
            self._ce_subset = [int(i) for i in candidates]
        elif self.change_estimation_subset > 0:
            self._ce_subset = sorted(int(i) for i in np.random.choice(
                candidates, min(len(candidates), self.change_estimation_subset), replace=False))
        else:
            self._ce_subset = None
        if self.top_candidates is not None:
            top_candidates = self.top_candidates
            if isinstance(self.top_candidates, float):
                labelled = len(self.queries) + len(self.relevant_ids) + len(self.irrelevant_ids)
                top_candidates = min(len(candidates), int(self.top_candidates * labelled))
            if (top_candidates > 0) and (top_candidates < len(candidates)):
                top_ind = np.argpartition(self.rel_mean[candidates], -top_candidates)[-top_candidates:]
                candidates = candidates[top_ind]
        return candidates

    # ------------------------------------------------------------------ the hot path
    def fetch_unlabelled(self, k, show_progress=False):
        """Selects k unlabelled samples by greedy maximisation of mutual information (reference ital.py:84-134).

        Returns the list of selected sample indices (python ints, selection order)."""
        gp = self.gp
        if gp.m == 0:
            raise RuntimeError("fetch_unlabelled() needs a fitted relevance model: call update() first or pass queries "
                               "(the reference fails with an AttributeError at gp.py:222)")
        unseen = self._unseen_list()
        k = min(int(k), len(unseen))
        if k <= 0:
            return []
        why = self._unsupported(k, len(unseen))
        if why is not None:
            raise NotImplementedError("ital_amd device scorer: %s is not implemented" % why)
        if (self.top_candidates is None and not self._needs_generic() and self.round_call and self.select_in_scorer
                and self._round_possible(k, unseen)):
            # the retrieval loop's own case: the candidate list is get_unseen() itself.  Nothing of its size is touched on
            # the host -- the list lives on the device, the host keeps (base, removed ids) (retrieval_base.UnseenList)
            self._ce_subset = None
            self._last_batch = None
            return self._select_round(k, unseen)
        candidates = self._candidate_list(unseen.array())
        if len(candidates) < k:
            # k was clamped to the number of unseen samples BEFORE the top_candidates restriction (ital.py:99-117): the
            # reference picks until the list is empty and np.argmax([]) then raises exactly this (ital.py:130) -- with
            # the random streams advanced by the steps it did run, so those are run here too
            if len(candidates) > 0:
                self._select(len(candidates), candidates)
            raise ValueError("attempt to get argmax of an empty sequence")
        return self._select(k, candidates)

    def _shard(self, candidates, b=None):
        """Candidate shard of this rank as device arrays: local rows, alive flags, explicit list positions (or None when
        the local positions are one contiguous run of the list), and the list position of the first one.  `b`: batch
        buffers whose cached alive-flag array is reused (the fetch prologue sits between two rounds with the GPU idle)."""
        gp = self.gp
        dev = gp.device
        cand = np.asarray(candidates, dtype=np.int64)
        if gp.world == 1:
            loc_rows, pos_offset, gpos = cand, 0, None          # every candidate is local, in list order
        else:
            loc_rows, pos_offset, gpos = sharding.shard_candidates(cand, gp.row0, gp.row1, self._ascending(candidates))
        n_loc = len(loc_rows)
        cand_d = torch.from_numpy((loc_rows - gp.row0).astype(np.int32)).to(dev) if n_loc else \
            torch.zeros(1, dtype=torch.int32, device=dev)
        gpos_d = torch.from_numpy(gpos).to(dev) if gpos is not None else None
        if b is not None:
            ensure_step_buffers(b, n_loc, 0, dev)
            alive = b["alive"]
            alive.fill_(1)
        else:
            alive = torch.ones(max(n_loc, 1), dtype=torch.uint8, device=dev)
        return cand, n_loc, pos_offset, cand_d, gpos_d, alive

    def _ascending(self, candidates):
        """The candidate list is the get_unseen() array itself (ascending by construction): lets the sharding arithmetic
        use binary searches instead of passes over a list of up to millions of entries."""
        u = self.__dict__.get("_unseen")
        return u is not None and candidates is u[0]._flat

    def _qmc_workspace(self, b, t, n_loc):
        """Workspace of the lattice scorer (prepared calls of a slab of candidates), grown on demand up to `qmc_work_bytes`."""
        want = int(_lib.lib().ital_round_workspace(t, max(n_loc, 1), max(self.qmc_work_bytes // 8, 1 << 16)))
        return qmc_work(b, want, self.gp.device)

    def _sel_parts_doubles(self, k, n_loc):
        """Doubles of the block partials of the selection inside the scoring launches of a round of k steps: three per
        scoring block -- n/256 blocks at t = 1, n/32 at t = 2, n/256 plus one per slab of the lattice workspace from t = 3 on
        (with a small workspace cap, `qmc_work_bytes`, a step of t = 7, 8 runs in slabs of a few candidates each)."""
        return int(_lib.lib().ital_sel_parts_len(k, n_loc, max(self.qmc_work_bytes // 8, 1 << 16)))

    def _select(self, k, candidates):
        """Greedy construction of a batch of k out of `candidates` (k <= len(candidates))."""
        # (published only after the round's final successful download: update() pairs its sample ids with rows of the batch buffers)
        self._last_batch = None
        generic = self._needs_generic()
        if not generic and self.round_call and self.select_in_scorer and self._round_possible(k, candidates):
            return self._select_round(k, candidates)
        if self._round_bufs is not None:
            self._round_bufs.invalidate()      # the other paths leave the device's list behind
        return self._fetch_generic(k, candidates) if generic else self._select_steps(k, candidates)

    def _user(self):
        """(noise, eps, label mode) of ital_score_desc."""
        return float(self.noise), float(self.eps), _LABEL_MODES[self.label_estimation]

    def _step_desc(self, b, scored, t, k, n_alive, tail, fused):
        """ital_score_desc of greedy step t of the step-by-step path (tail: the scoring launch ends with the selection)."""
        gp = self.gp
        n_loc = scored.n
        desc = ItalScoreDesc()
        desc.t = t
        fill_score_desc(desc, gp, b, scored, self._user())
        if t >= 3:
            jump, jumppat, vk = lattice_tables(b, t, gp.device)
            desc.jump, desc.jumppat, desc.vk = _ptr(jump), _ptr(jumppat), _ptr(vk)
            for j in range(6):
                desc.seed[j] = mvn_stream.GLOBAL.state[j]
            work = self._qmc_workspace(b, t, n_loc)
            desc.work, desc.work_doubles = _ptr(work), work.numel()
            if self.profile is not None and n_loc > 0:
                # the lattice-sum kernel alone, bracketed by events the library records on the launch stream (an
                # event has to be recorded once before its handle exists: the pool's events are, see bench.py).
                # Every record is a barrier packet in the queue (~4 us of idle GPU in a 3 ms round), so the step
                # as a whole is only bracketed where no kernel-level pair exists
                k0, k1 = self._event(), self._event()
                desc.ev_start, desc.ev_stop = k0.cuda_event, k1.cuda_event
                # several slabs: the pair spans first .. last lattice sum incl. the launches between them
                self.profile.append((lattice_label(work, t, n_loc), t, n_alive if not gp.collective else n_loc, k0, k1))
        if tail:
            # the scoring launch ends with the selection itself (the block that finishes last selects): one rank --
            # arg-max, record and batch bookkeeping, no selection launch at all; several ranks -- arg-max and record
            # (what ital_select_local does in a single-workgroup launch of its own), exchange and resolve follow
            ensure_step_buffers(b, n_loc, self._sel_parts_doubles(k, n_loc), gp.device)
            fill_score_select(desc, gp, b, gp.m, b["ret"] if fused else None)
        return desc

    def _select_steps(self, k, candidates):
        """_select step by step from Python: per greedy step the scoring launch, the selection (inside it, or as launches
        of its own with the ranks' exchange between them) and the new member's covariance column."""
        gp = self.gp
        lib = _lib.lib()
        with torch.cuda.device(gp.device):
            b = self._buffers(k)
            st = _stream()
            # ---- candidate shard of this rank (list positions keep their global numbering)
            cand, n_loc, pos_offset, cand_d, gpos_d, alive = self._shard(candidates, b)
            mi = b["mi"]                                   # every live position is written by the scorer
            scored = Scored(mi, cand_d, alive, n_loc, pos_offset, gpos_d, gp.row0)
            self.last_scores = []
            stream = mvn_stream.GLOBAL
            saved_stream = (stream.state, stream.draws)
            n_alive = len(candidates)
            b["ret"][b["kmax"]:].zero_()      # the resolve steps OR every rank's status word into this slot
            for t in range(1, k + 1):
                tail = self.select_in_scorer and 0 < n_loc <= _FUSED_SELECT_MAX
                fused = not gp.collective and 0 < n_loc <= (_FUSED_SELECT_MAX if tail else _FUSED_LAUNCH_MAX)
                desc = self._step_desc(b, scored, t, k, n_alive, tail, fused)
                ev0 = self._mark() if t < 3 else None
                check(_lib.rows_fn("ital_score_step", gp.xtype)(ctypes.byref(desc), st))
                if t < 3:
                    self._mark("score", t, n_alive, ev0)
                if self.keep_scores:
                    self.last_scores.append(mi.clone())
                if not (tail and fused):
                    select_step(gp, b, scored, gp_model(gp), t - 1, st, fused=fused, local=not tail, mark=self._mark)
                if t < k:
                    ev0 = self._mark() if t == 1 else None           # one sample of the streaming kernel per round
                    member_column(self, gp_model(gp), b, t - 1, st)
                    if t == 1:
                        self._mark("cross_cov", t, gp.m, ev0)
                # the reference's serial loop has now consumed this many uniforms of mvndst's stream
                stream.advance(mvn_stream.step_draws(t, n_alive))
                n_alive -= 1
            host = self._download(b["ret"], "the picks of the round", self._step_estimate_s(k, n_loc)).tolist()     # the only synchronisation of the round: the picks and the status word
            ret, status = host[:k], host[b["kmax"]]   # status: OR over the greedy steps and over all ranks (same everywhere)
            if status & 6:
                # linearly dependent variables inside a batch (duplicate samples), or a simulated update that does not pin the
                # labels (large noise): the fast scorer carries neither MVNDFN's limit-intersection logic nor the updated
                # integrals; redo the round with the general scorer from the same stream position -- on every rank alike
                gp.status.bitwise_and_(~6)
                stream.state, stream.draws = saved_stream
                return self._fetch_generic(k, candidates)
        if status:
            gp.check_status(status)
        self._last_batch = (b, list(ret))
        return [int(i) for i in ret]

    def _round_possible(self, k, candidates):
        """Can this round run as one ital_fetch_round call?  One rank: any list of up to ITAL_ROUND_MAX_CAND candidates.
        Several ranks: the ascending get_unseen() list (an UnseenList: every rank's share is one run of it), at least one
        and at most that many candidates on every rank, and a transport for the per-step record exchange.  Decided from
        the list and the process group alone: the same on every rank."""
        gp = self.gp
        n = len(candidates)
        if n < k:
            return False
        if not gp.collective:
            return n <= _FUSED_SELECT_MAX
        if not isinstance(candidates, UnseenList) or self._round_transport() is None:
            return False
        bounds = [sharding.row_range(gp.n_total, gp.world, r)[0] for r in range(gp.world)] + [gp.n_total]
        sizes = np.diff([candidates.count_below(x) for x in bounds])
        return bool(sizes.min() >= 1 and sizes.max() <= _FUSED_SELECT_MAX)

    @staticmethod
    def _step_estimate_s(k, n_loc):
        """Upper estimate of the compute time of ONE greedy step of the full enumeration on this rank (the last step of a batch
        of k dominates): its (Phi, Phi^-1) pairs at 1e11 pairs/s, less than half the measured rate of the lattice sums -- what
        the exchange deadline must not mistake for a stalled collective (sharding.await_download)."""
        if k < 3:
            return 0.0
        prime = (31, 47, 73, 113, 173, 263, 397, 593, 907, 1361)[min(k - 1, 10) - 1]
        return float(n_loc) * (2 ** k) * 16 * prime * (k - 1) / 1e11

    def _download(self, tensor, what, step_estimate_s=0.0):
        """Device -> host copy of a round's result.  On several ranks it is the point where this rank waits for the round's
        collectives: bounded (no resolved greedy step for ITAL_EXCHANGE_TIMEOUT_S, or for three times the estimated compute
        time of one step if that is longer) and with the raw communicator's asynchronous errors polled
        (sharding.await_download) -- a rank that dies mid-round must not leave the others waiting for ever."""
        gp = self.gp
        if not gp.collective:
            return tensor.cpu()
        kind = self._transport[1] if self._transport else None
        comm = kind[1] if kind and kind[0] == "nccl" else None
        if comm is None:
            e = sharding._RAW_COMMS.get((id(gp.group), str(gp.device)))      # the step path uses the raw communicator as well
            comm = e[1] if e else None
        name = {"nccl": "raw_nccl", "host": "host"}[kind[0]] if kind else ("raw_nccl (per step)" if comm else "torch_dist")
        return sharding.await_download(tensor, what, gp.group, gp.device, comm, gp.rank, gp.world, name, pinned=self._pinned,
                                       step_estimate_s=step_estimate_s)

    def _round_transport(self):
        """How ital_fetch_round exchanges the ranks' records: ("nccl", ncclComm_t of the process group -- the communicator
        torch.distributed itself uses, ProcessGroupNCCL._comm_ptr) over RCCL, ("host", None) through torch.distributed from
        a callback (backends that move host memory: the gloo rehearsals and tests), or None (the round is enqueued step by
        step with torch.distributed's all-gather between the launches)."""
        gp = self.gp
        cached = self._transport
        if cached is not None and cached[0] is gp.group:
            return cached[1]
        kind = None
        import torch.distributed as dist
        if gp.group is not None and dist.is_initialized():
            if dist.get_backend(gp.group) == "nccl":
                comm = sharding.raw_comm(gp.group, gp.device)      # None: the step path (torch.distributed between launches)
                kind = ("nccl", comm) if comm else None
            else:
                kind = ("host", None)
        if os.environ.get("ITAL_ROUND_TRANSPORT") == "none":
            kind = None
        elif os.environ.get("ITAL_ROUND_TRANSPORT") == "host" and kind is not None:
            kind = ("host", None)
        if kind is not None:
            self._transport = (gp.group, kind)
        return kind

    def _select_round(self, k, candidates):
        """_select as ONE call below the C ABI (ital_fetch_round); the candidate list stays on the device between rounds.
        The round itself is _fast_round.FastRound."""
        round_ = FastRound(self, k, candidates)            # (the host clock of the round's prologue starts here)
        with torch.cuda.device(self.gp.device):
            return round_.run()

    # ------------------------------------------------------------------ general scorer (noisy users, estimation subset)
    def _fetch_generic(self, k, candidates):
        """Greedy batch construction through ital_score_generic: any user model (reference ital.py:300-342), with or
        without a change-estimation subset (ital.py:227-275, 541-582), the Monte-Carlo switches, clip_cov, label
        estimation; also every fallback of the fast paths.  The round itself is _generic_round.GenericRound."""
        self._last_batch = None
        with torch.cuda.device(self.gp.device):
            return GenericRound(self, k, candidates).run()
