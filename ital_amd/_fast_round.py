"""One greedy batch construction as ONE call below the C ABI (`ital_fetch_round`): what ITAL._select_round runs.

Candidate-list upkeep, k scoring steps that end with their selection (several ranks: with the rank's record, then the
exchange issued from C and the resolve launch), k - 1 covariance columns -- enqueued from C (a Python host needs 10 - 17 us
per launch, the first greedy steps are shorter than that).  Several ranks work on their own share of the list.  The
candidate list stays on the device between rounds: when the list is the previous one minus the previous batch (the
retrieval loop: fetch, label the batch, fetch), it is compacted there by its alive flags instead of being rebuilt and
uploaded; and the descriptor of such a next round is filled in while the GPU still works on the current one.

`RoundBuffers` is the state only this path keeps between rounds (one per batch-buffer set), `Prepared` a filled-in round
descriptor and what goes with it, `plan_round` the decision how the candidate list reaches the device, and
`FastRound.run()` the round; every stage of it is a method of its own."""
import collections
import ctypes
import time

import numpy as np
import torch

from . import _lib, mvn_stream, sharding
from ._batch import (Scored, ensure_step_buffers, fill_score_desc, fill_score_select, lattice_label, lattice_tables)
from ._lib import check
from .gp import _ptr, _stream
from .retrieval_base import UnseenList

# how the candidate list reaches the device (plan_round): the descriptor the previous round prepared runs as it is (it
# compacts the previous list on the device); a fresh descriptor compacts that list (begin = 2); a fresh one after an upload
# (begin = 1)
PREPARED, COMPACT, UPLOAD = "prepared", "compact", "upload"

# what the device's candidate list corresponds to: the list of `unseen` (an UnseenList) as of `version` with `picks` flagged
# dead, n_loc entries of it on this rank, in the list tensors of `buffers`
DeviceList = collections.namedtuple("DeviceList", "buffers unseen version picks n_loc")


class Prepared(collections.namedtuple("Prepared", "desc slot k n n_loc m begin cur state_before state_after draws events sig")):
    """Round descriptor `desc` (slot `slot` of its buffer set), filled for a round of k steps over n candidates (n_loc of
    them this rank's) with m labelled samples from stream state `state_before`, the list in device buffer `cur`; the
    stream position after the round (state_after, draws), the profile tuples of the events it records, and the
    signature of everything else the descriptor points to or copies."""
    __slots__ = ()

    def matches(self, k, n, m, stream_state, signature):
        """Is this the descriptor of a round of k out of n with m labelled samples at that stream state and signature?"""
        return (self.k == k and self.n == n and self.m == m and self.state_before == tuple(stream_state)
                and self.sig == signature)

    def patch_share(self, n_loc, pos_offset):
        """Several ranks: the descriptor was prepared before the picks of the round before were known -- how many of them
        lay in this rank's rows (n_loc) and before them (pos_offset) goes in when the round comes.  Returns the patched one."""
        d = self.desc.step
        d.n_cand, d.pos_offset = n_loc, pos_offset
        return self._replace(n_loc=n_loc, events=[ev[:2] + (n_loc,) + ev[3:] for ev in self.events])


def plan_round(candidates, buffers, record, prepared, keep_scores, k, n, m, stream_state, signature):
    """PREPARED, COMPACT or UPLOAD for a round of k out of the n `candidates` with m labelled samples.  The device holds
    the list as of `record.version` with the picks of that round flagged dead: it follows the host's when the host's list
    is that version minus exactly those picks (same buffer set, same UnseenList object)."""
    follows = (isinstance(candidates, UnseenList) and record is not None and record.buffers is buffers
               and record.unseen is candidates and record.version == candidates.version - 1
               and tuple(sorted(record.picks)) == candidates.last_removed)
    if not follows:
        return UPLOAD
    if prepared is not None and not keep_scores and prepared.matches(k, n, m, stream_state, signature):
        return PREPARED
    return COMPACT


class RoundBuffers(object):
    """What only the one-call round keeps with batch buffers `b` of `learner`: two candidate-list tensors (the compaction
    reads one, writes the other) and which is current, two round descriptors, the prepared next round, the host
    transport's callback, and the record of the list the device holds."""

    def __init__(self, learner, b):
        self.L, self.b = learner, b
        self.lists, self.cur = None, 0
        self.descs = None
        self.next = None                 # Prepared: the round that follows in the retrieval loop
        self.exchange_cb = None
        self.exchange_exc = None         # what the callback caught: re-raised by the caller of ital_fetch_round
        self.device_list = None          # DeviceList, or None: the next round uploads its list

    def invalidate(self):
        """The device's list is no longer known to be the host's minus a batch."""
        self.device_list = None

    def drop_prepared(self):
        """The prepared round did not come: its events go back to the pool."""
        if self.next is not None:
            for ev in self.next.events:
                self.L.event_pool += [ev[3], ev[4]]
            self.next = None

    def ensure(self, n_loc, k):
        """Room for a round of k steps over n_loc candidates of this rank.  A buffer that a descriptor or the device list
        lives in is replaced: both start afresh."""
        L, b = self.L, self.b
        dev = L.gp.device
        grown = ensure_step_buffers(b, n_loc, L._sel_parts_doubles(k, n_loc), dev)
        if grown or self.lists is None or self.lists[0].numel() < n_loc:
            self.lists = [torch.empty(max(n_loc, 1), dtype=torch.int32, device=dev) for _ in range(2)]
            self.cur = 0
            self.descs = [_lib.ItalRoundDesc(), _lib.ItalRoundDesc()]
            self.drop_prepared()
            self.invalidate()

    def host_exchange(self):
        """The record exchange as a callback of ital_fetch_round (transport "host"): torch.distributed's all-gather of this
        rank's record buffer, issued from inside the C call at the place the RCCL transport issues ncclAllGather."""
        if self.exchange_cb is None:
            b, group = self.b, self.L.gp.group

            def exchange(ctx, record, records_all, rec_len, stream):
                try:
                    sharding.gather_records(b["rec"], b["rec_all"], group)
                    return 0
                except Exception as e:      # noqa: BLE001 -- must not unwind through the C frames
                    self.exchange_exc = e   # (an ExchangeError: deadline / lost peer)
                    return -5
            self.exchange_cb = _lib.EXCHANGE_FN(exchange)
        return self.exchange_cb

    def signature(self, k):
        """Everything a descriptor of a round of k steps points to or copies besides (n, m, stream state)."""
        L, b = self.L, self.b
        gp = L.gp
        w = b.get("qmc_work")
        return (id(b), k, gp.cap, gp.ldv, gp.V.data_ptr(), gp.mu.data_ptr(), 0 if w is None else w.data_ptr(),
                float(L.noise), float(L.eps), float(L.var), float(L.length_scale), L.label_estimation, L.qmc_work_bytes,
                L.profile is not None, repr(L.profile_steps))

    def prepare(self, slot, k, n, m, begin, cur, state_before, *, n_prev=0, n_loc=None, pos_offset=0):
        """Fills round descriptor `slot` (one of two) for a round of k steps over n candidates with m labelled samples, the
        candidate list in device buffer `cur` (begin = 2: compacted out of the other buffer, which holds n_prev entries).
        Several ranks: n_loc of the n candidates are this rank's, the first of them at list position pos_offset.
        Nothing here depends on the picks of the round before: the descriptor of the NEXT round is prepared while the GPU
        works on the current one, off the critical path of the retrieval loop."""
        L, b = self.L, self.b
        gp = L.gp
        r = self.descs[slot]
        d = r.step
        r.k, r.n_rows, r.var, r.length_scale = k, gp.n, float(L.var), float(L.length_scale)
        r.begin, r.cand_prev, r.n_prev = begin, (_ptr(self.lists[cur ^ 1]) if begin == 2 else None), (n_prev if begin == 2 else 0)
        n_loc = n if n_loc is None else n_loc
        fill_score_desc(d, gp, b, Scored(b["mi"], self.lists[cur], b["alive"], n_loc, pos_offset, None, gp.row0), L._user())
        r.world, r.records_all, r.nccl_comm, r.exchange = 0, None, None, _lib.EXCHANGE_FN(0)
        if gp.collective:
            kind, comm = L._round_transport()
            r.world, r.records_all = gp.world, _ptr(b["rec_all"])
            if kind == "nccl":
                r.nccl_comm = comm
            else:
                r.exchange = self.host_exchange()
        fill_score_select(d, gp, b, m, b["ret"])
        r.mi_keep = None
        work = None
        if k >= 3:
            work = L._qmc_workspace(b, k, n_loc)
            d.work, d.work_doubles = _ptr(work), work.numel()
        events = self._lattice_steps(r, k, n, n_loc, work)
        # the reference's serial loop consumes n_alive * 2 * 2^t calls of mvndst's stream at step t: states before every step
        st6 = (ctypes.c_int * 6)(*state_before)
        check(_lib.lib().ital_mvn_round_seeds(st6, n, k, ctypes.byref(r.seeds)))
        draws = sum(mvn_stream.step_draws(t, n - (t - 1)) for t in range(3, k + 1))
        return Prepared(r, slot, k, n, n_loc, m, begin, cur, tuple(state_before), tuple(int(v) for v in st6), draws, events,
                        self.signature(k))

    def _lattice_steps(self, r, k, n, n_loc, work):
        """Lattice tables of the steps t >= 3 of descriptor r (their workspace: `work`) and, when bench.py asked for
        per-kernel timings, the events that bracket their lattice sums; returns the profile tuples of those events."""
        L, b = self.L, self.b
        gp = L.gp
        events = []
        for t in range(1, k + 1):
            r.ev_start[t] = r.ev_stop[t] = None
            if t >= 3:
                r.jump[t], r.jumppat[t], r.vk[t] = [_ptr(x) for x in lattice_tables(b, t, gp.device)]
                if L.profile is not None and (L.profile_steps is None or t in L.profile_steps):
                    k0, k1 = L._event(), L._event()
                    r.ev_start[t], r.ev_stop[t] = k0.cuda_event, k1.cuda_event
                    # (candidates the bracketed launches score: the whole list on one rank; this rank's share otherwise --
                    # which rank the earlier picks of the round come from is not known when the descriptor is built)
                    events.append((lattice_label(work, t, n_loc), t,
                                   n - (t - 1) if not gp.collective else n_loc, k0, k1))
        return events


class FastRound(object):
    def __init__(self, learner, k, candidates):
        self.t_enter = time.perf_counter()
        self.L, self.k, self.candidates, self.gp = learner, k, candidates, learner.gp
        self.n = len(candidates)
        self.listed = isinstance(candidates, UnseenList)      # (several ranks: always, see ITAL._round_possible)
        self.stream = mvn_stream.GLOBAL
        self.lo = self.n_loc = self.rb = self.p = self.keep = self.t_call = None

    def run(self):
        L = self.L
        self._share()
        self._buffers()
        self.p = p = self._descriptor()
        L.last_round = (p.begin, p.slot)          # diagnostics / tests: how the candidate list reached the device
        self._keep_scores()
        saved_stream = (self.stream.state, self.stream.draws)
        self._stamp_call()
        self._call()
        self.stream.state, self.stream.draws = p.state_after, self.stream.draws + p.draws
        if L.profile is not None:
            L.profile += p.events
        self._prepare_next()
        ret, status = self._download()
        return self._finish(ret, status, saved_stream)

    def _share(self):
        """This rank's share of the ascending list: one run of it, list positions lo .. lo + n_loc."""
        gp, c = self.gp, self.candidates
        lo, hi = (c.count_below(gp.row0), c.count_below(gp.row1)) if gp.collective else (0, self.n)
        self.lo, self.n_loc = lo, hi - lo

    def _buffers(self):
        """The path's own state with the learner's batch buffers (which drop it when they are replaced), with room for
        this round."""
        L = self.L
        b = L._buffers(self.k)
        if L._round_bufs is None:
            L._round_bufs = RoundBuffers(L, b)
        self.rb = L._round_bufs
        self.rb.ensure(self.n_loc, self.k)

    def _descriptor(self):
        """The round's descriptor: the one the previous round prepared, or -- its events returned -- a fresh one over the
        list compacted on the device or uploaded.  The device-list record is cleared here and published again after the
        round's successful download."""
        L, gp, rb, k, n, n_loc = self.L, self.gp, self.rb, self.k, self.n, self.n_loc
        dl, p = rb.device_list, rb.next
        plan = plan_round(self.candidates, rb, dl, p, L.keep_scores, k, n, gp.m, self.stream.state,
                          rb.signature(k) if p is not None else None)
        rb.invalidate()
        if plan == PREPARED:
            rb.next = None
            rb.cur = p.cur                                     # the round the previous one prepared for
            return p.patch_share(n_loc, self.lo) if gp.collective else p
        rb.drop_prepared()
        if plan == COMPACT:
            begin, n_prev = 2, dl.n_loc                        # the device holds the parent list with exactly those picks flagged
            rb.cur ^= 1
        else:
            begin, n_prev = 1, 0
            c = self.candidates
            share = c.in_rows(gp.row0, gp.row1) if self.listed else np.asarray(c, dtype=np.int64)
            rb.lists[rb.cur][:n_loc].copy_(torch.from_numpy((share - gp.row0).astype(np.int32)))
        return rb.prepare(0, k, n, gp.m, begin, rb.cur, self.stream.state, n_prev=n_prev, n_loc=n_loc, pos_offset=self.lo)

    def _keep_scores(self):
        if self.L.keep_scores:
            self.keep = torch.zeros((self.k, self.n_loc), dtype=torch.float64, device=self.gp.device)
            self.p.desc.mi_keep = _ptr(self.keep)

    def _stamp_call(self):
        """Host time on the critical path of the retrieval loop: from the download of the previous round's picks (the
        caller's feedback, update(), this prologue) to the call that enqueues the next round."""
        hc = self.L.host_clock
        if hc is not None:
            self.t_call = t_call = time.perf_counter()
            if hc.get("t_download") is not None:
                hc["gap_s"] += t_call - hc["t_download"]
                hc["gaps"] += 1
                hc["prologue_s"] = hc.get("prologue_s", 0.0) + (t_call - self.t_enter)

    def _call(self):
        rb = self.rb
        rc = _lib.rows_fn("ital_fetch_round", self.gp.xtype)(ctypes.byref(self.p.desc), _stream())
        if rc and rb.exchange_exc is not None:      # the host transport's callback failed: its own error, not the C one
            exc, rb.exchange_exc = rb.exchange_exc, None
            raise exc
        check(rc)

    def _prepare_next(self):
        """While the GPU works: the descriptor of the round that follows in the retrieval loop (this batch labelled, then
        the next fetch of k): nothing in it depends on which samples this round picks."""
        L, gp, rb, p, k, n, n_loc = self.L, self.gp, self.rb, self.p, self.k, self.n, self.n_loc
        if n - k >= k and gp.m + k <= gp.cap and not L.keep_scores:
            # (several ranks: this rank's share of that list is known only with the picks -- patched in when the round comes)
            rb.next = rb.prepare(p.slot ^ 1, k, n - k, gp.m + k, 2, rb.cur ^ 1, self.stream.state, n_prev=n_loc,
                                 n_loc=n_loc if gp.collective else n - k, pos_offset=self.lo)

    def _download(self):
        """The only synchronisation of the round: the picks and the status word."""
        L, k, hc = self.L, self.k, self.L.host_clock
        if hc is not None:
            hc["enqueue_s"] += time.perf_counter() - self.t_call     # the call itself + the next round's descriptor (GPU busy)
        host = L._download(self.rb.b["ret"], "the picks of the round", L._step_estimate_s(k, self.n_loc)).tolist()
        if hc is not None:
            hc["t_download"] = time.perf_counter()
        keep = self.keep
        L.last_scores = [keep[t, :self.n_loc] for t in range(k)] if keep is not None else []
        return host[:k], host[self.rb.b["kmax"]]

    def _finish(self, ret, status, saved_stream):
        """Status word (OR over the greedy steps and all ranks), then the batch and the device's list are published."""
        L, gp, c = self.L, self.gp, self.candidates
        if status & 8:
            raise RuntimeError("ital_amd: the candidate list kept on the device lost track of the host's (internal error)")
        if status & 6:
            # see ITAL._select_steps: duplicates inside the batch / a simulated update that does not pin the labels
            gp.status.bitwise_and_(~6)
            self.stream.state, self.stream.draws = saved_stream
            return L._fetch_generic(self.k, c.array() if self.listed else c)
        if status:
            gp.check_status(status)
        ret = [int(i) for i in ret]
        L._last_batch = (self.rb.b, list(ret))
        if self.listed:
            self.rb.device_list = DeviceList(self.rb, c, c.version, ret, self.n_loc)
        return ret
