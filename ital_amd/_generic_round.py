"""One greedy batch construction through the general scorer (`ital_score_generic`): what ITAL._fetch_generic runs.

Without a change-estimation subset the base set of the scorer IS the batch so far: it lives in the replicated device batch
state that the selection launches maintain, and a round is enqueued without any host round trip (one download of the
picks at the end) unless an option needs the host between the steps (Monte-Carlo sampling on numpy's generator, the
counting pass of clip_cov).  With a subset the base set also holds the subset members and grows only when a pick lies
outside it: that bookkeeping stays on the host (one synchronisation per greedy step).

`GenericRound.run()` is the loop; every stage of a step is a method of its own, the step's values travel in `Step`."""
import ctypes
import os
import time

import numpy as np
import torch

from . import _lib, _mc_sampler, mvn_stream, sharding
from ._batch import FUSED_LAUNCH_MAX, LABEL_MODES, Scored, gp_model, member_column, qmc_work, select_step
from ._lib import ITAL_GENERIC_MAX_DIM, ITAL_GENERIC_MAX_REL, ITAL_JUMP_BITS, ITAL_REC_HEADER, ItalGscoreDesc, check
from .gp import _ptr, _stream


class Step(object):
    """Values of one greedy step t: nE members of the base set, nr enumerated variables, the Monte-Carlo plan, uniforms
    of mvndst's stream per candidate outside / inside the base set, list positions of the live members of the base set,
    whether clip_cov needs the counting pass; then what the stages add (desc, samples, ranges, total_draws)."""

    def __init__(self, t, nE, plan, clip_count):
        self.t, self.nE, self.nr, self.plan, self.clip_count = t, nE, t, plan, clip_count
        self.draws_out = self.draws_in = 0
        self.in_pos = []
        self.samples = self.ranges = self.total_draws = self.desc = None


class GenericRound(object):
    def __init__(self, learner, k, candidates):
        """Set-up: shard, buffers, constant tables, the subset members' covariance columns."""
        self.L, self.k, self.gp = learner, k, learner.gp
        gp = self.gp
        self.dev = dev = gp.device
        self.lib = _lib.lib()
        self.subset_mode = learner._ce_subset is not None
        self.fb_mode = learner._fb_mode()
        self.E = list(learner._ce_subset) if self.subset_mode else []
        self.kmax_e = len(self.E) + k
        self.stream = mvn_stream.GLOBAL
        self.st = _stream()
        self.b = b = learner._buffers(max(self.kmax_e, 4))
        self.kmax = kmax = b["kmax"]
        self.cand, self.n_loc, self.pos_offset, self.cand_d, self.gpos_d, self.alive = learner._shard(candidates)
        # every rank's candidates one contiguous run of the list (the ascending get_unseen() order; not after the
        # argpartition order of top_candidates on several ranks)?  Decided from the list alone: the same on every rank
        self.runs = sharding.contiguous_runs(self.cand, gp.n_total, gp.world, learner._ascending(candidates))
        self.pos_of = {int(c): i for i, c in enumerate(self.cand.tolist())}
        self.mi = torch.zeros(max(self.n_loc, 1), dtype=torch.float64, device=dev)
        self.scored = Scored(self.mi, self.cand_d, self.alive, self.n_loc, self.pos_offset, self.gpos_d, gp.row0)
        if "jump1" not in b:
            b["jump1"] = torch.from_numpy(mvn_stream.jump1_table(ITAL_JUMP_BITS)).to(dev)
            b["vk_all"] = torch.from_numpy(mvn_stream.vk_table(ITAL_GENERIC_MAX_DIM)).to(dev)
            b["iota"] = torch.arange(kmax, dtype=torch.int32, device=dev)
            b["zero64"] = torch.zeros(1, dtype=torch.int64, device=dev)
        self.C = b["C"]
        self.e_mu = np.zeros(self.kmax_e)
        self.e_sig = np.zeros((self.kmax_e, self.kmax_e))
        self.keep = []                # device temporaries of the enqueued work (released after the round's synchronisation)
        b["ret"][kmax:].zero_()
        if self.E:
            self._subset_columns()
        self.picks, self.pick_pos = [], []
        self.mc_cache = {}            # host copies of this rank's variances / covariance columns (pattern sampling)
        learner.last_scores = []
        learner.last_patterns = []    # keep_scores: the sampled sign patterns of every Monte-Carlo step (diagnostics/tests)
        self.n_alive = len(candidates)
        self.z_next = None

    def _subset_columns(self):
        """Covariance columns of the subset members with every row, and among themselves."""
        gp, E, C, dev = self.gp, self.E, self.C, self.dev
        rows = gp._gather_rows(E)
        norms = torch.empty(len(E), dtype=torch.float64, device=dev)
        check(self.lib.ital_row_norms(_ptr(rows), len(E), gp.ldx, _ptr(norms), self.st))
        vcols = gp.gather_columns(gp.V[: max(gp.m, 1)], E)          # [m, |E|]
        for c0 in range(0, len(E), 16):
            c = min(16, len(E) - c0)
            Wt = torch.zeros((c, gp.cap), dtype=torch.float64, device=dev)
            Wt[:, : gp.m] = vcols[: gp.m, c0:c0 + c].t()
            check(_lib.rows_fn("ital_cross_cov_cols", gp.xtype)(_ptr(gp.Xd), _ptr(gp.xnorm), gp.n, gp.ldx, _ptr(rows[c0:c0 + c]),
                                               _ptr(norms[c0:c0 + c]), c, _ptr(Wt), gp.cap, _ptr(gp.V), gp.ldv, gp.m,
                                               float(self.L.var), float(self.L.length_scale), _ptr(C[c0:c0 + c]), gp.ldv,
                                               self.st))
            self.keep.append(Wt)
        self.keep += [rows, norms, vcols]
        self.e_sig[: len(E), : len(E)] = gp.gather_columns(C[: len(E)], E).cpu().numpy()
        self.e_mu[: len(E)] = self.L.rel_mean[np.asarray(E)]

    # ------------------------------------------------------------------ the round
    def run(self):
        L, k = self.L, self.k
        for t in range(1, k + 1):
            s = self._plan_step(t)
            if s.plan[0] or s.plan[2]:
                self._sample(s)
            self.z_next = None
            self._descriptor(s)
            self._attach_samples(s)
            if s.clip_count:
                self._count_clip_draws(s)
            ev0 = L._mark()
            if s.ranges is None:
                check(self.lib.ital_score_generic(ctypes.byref(s.desc), self.st))
            else:
                self._score_ranged(s)
            L._mark("score_generic", t, self.n_alive, ev0)
            if L.keep_scores:
                L.last_scores.append(self.mi.clone())
            self._advance(s)
            if self.subset_mode:
                self._select_host(s)
            else:
                self._select_device(s)
        return self._finish()

    def _plan_step(self, t):
        L = self.L
        nE = len(self.E) if self.subset_mode else t - 1
        s = Step(t, nE, L._mc_plan(t, self.fb_mode), L._clip_active() and nE + 1 > 5)
        dpc = mvn_stream.draws_per_call
        npat, nfb = s.plan[1], s.plan[3]
        if self.subset_mode:
            s.draws_out = npat * (dpc(s.nr) + (1 + nfb) * dpc(nE + 1))
            s.draws_in = npat * (dpc(s.nr) + (1 + nfb) * dpc(nE))
            s.in_pos = sorted(self.pos_of[e] for e in self.E if e in self.pos_of and e not in self.picks)
        else:
            s.draws_out = npat * (1 + nfb) * dpc(s.nr)
        return s

    def _sample(self, s):
        """Host sampling for the step: the device batch state comes down, the patterns / feedback configurations are
        drawn -- as arrays, or, for pattern sampling alone on a large shard, as a generator over ranges of candidates (the
        SVDs of the next range run on the host under the lattice sums of the current one)."""
        b, t, kmax = self.b, s.t, self.kmax
        rel_mc, npat, fb_mc, nfb = s.plan
        t_host0 = t_host1 = time.perf_counter()
        if not self.subset_mode and t > 1:
            # batch state kept by the device: the members' means / covariances for the pattern sampler
            self.picks = [int(i) for i in b["ret"][: t - 1].cpu().tolist()]
            t_host1 = time.perf_counter()          # (the wait for the step before: GPU time, not host time)
            self.pick_pos = list(range(t - 1))
            self.e_mu[: t - 1] = b["bmu"][: t - 1].cpu().numpy()
            self.e_sig[: t - 1, : t - 1] = b["sig"].view(kmax, kmax)[: t - 1, : t - 1].cpu().numpy()
        n_chunks = _mc_sampler.range_count(s.nr, self.n_loc, rel_mc and not fb_mc and not self.subset_mode
                                           and not s.clip_count and bool(self.runs) and self.gpos_d is None)
        pos_of = self.pos_of
        local = (self.pos_offset, self.pos_offset + self.n_loc) if self.runs else None
        var, cov_cols, row0 = self._moment_tables(rel_mc and not fb_mc and local is not None) if rel_mc else (None, None, 0)
        sampler = _mc_sampler.PatternSampler(
            rows=self.cand, dead=[pos_of[q] for q in self.picks], pick_members=self.pick_pos, e_mu=self.e_mu,
            e_sig=self.e_sig, plan=s.plan, nr=s.nr, fb_mode=self.fb_mode, user=(self.L.label_prob, self.L.mistake_prob),
            base_pos=[pos_of.get(e, -1) for e in self.E] if self.subset_mode else None,
            mean=np.asarray(self.L.rel_mean, dtype=np.float64) if rel_mc else None, var=var, cov_cols=cov_cols, row0=row0,
            local=local, z_ahead=self.z_next, walk=self.L.mc_walk)
        if n_chunks > 0 and sampler.jl1 > sampler.jl0:
            s.ranges, s.samples = sampler.ranges(n_chunks), (None, None, sampler.enumerated_draws())
        else:
            s.samples = sampler.arrays()
        if os.environ.get("ITAL_MC_TIMING"):
            print("t=%d: waited %.1f ms for the step before; batch state + sampler set-up%s %.1f ms" % (
                t, (t_host1 - t_host0) * 1e3, "" if n_chunks else " + ALL decompositions",
                (time.perf_counter() - t_host1) * 1e3), flush=True)

    def _moment_tables(self, local_only):
        """Variances and the picks' covariance columns on the host, and the data index of their entry 0.  local_only:
        the sampler reads rows of this rank alone (PatternSampler.local_only)."""
        gp, C, pp, cache = self.gp, self.C, self.pick_pos, self.mc_cache
        if local_only:
            # every row read is a row of this rank: variances and covariance columns come from the local shard
            # (a column is downloaded once per fetch, when its member joins the batch) -- no collective, nothing N-sized
            if "s2" not in cache:
                cache["s2"] = gp.s2[: gp.n].cpu().numpy()
            for c in pp:
                if ("C", c) not in cache:
                    cache[("C", c)] = C[c][: gp.n].cpu().numpy()
            return cache["s2"], (np.stack([cache[("C", c)] for c in pp]) if pp else np.zeros((0, gp.n))), gp.row0
        return gp._full(gp.s2), (np.stack([gp._full(C[c]) for c in pp]) if pp else np.zeros((0, gp.n_total))), 0

    def _descriptor(self, s):
        """ItalGscoreDesc of the step; the base set is either the host's (subset mode: uploaded) or the device batch
        state itself.  Sizes the pipeline's workspace."""
        L, gp, b, dev = self.L, self.gp, self.b, self.dev
        s.desc = desc = ItalGscoreDesc()
        desc.n_cand = self.n_loc
        desc.cand, desc.alive, desc.mu, desc.s2 = _ptr(self.cand_d), _ptr(self.alive), _ptr(gp.mu), _ptr(gp.s2)
        desc.C, desc.ldc = _ptr(self.C), gp.ldv
        desc.row_offset, desc.pos_offset, desc.gpos = gp.row0, self.pos_offset, _ptr(self.gpos_d)
        if self.subset_mode:
            E = self.E
            i32, i64 = torch.int32, torch.int64
            dead_pos = [self.pos_of[q] for q in self.picks]
            up = [torch.as_tensor(E if E else [0], dtype=i64, device=dev),
                  torch.as_tensor(np.argsort(np.asarray(E, dtype=np.int64), kind="stable") if E else [0], dtype=i32, device=dev),
                  torch.from_numpy(np.ascontiguousarray(self.e_mu)).to(dev),
                  torch.from_numpy(np.ascontiguousarray(self.e_sig)).to(dev),
                  torch.as_tensor(self.pick_pos if self.pick_pos else [0], dtype=i32, device=dev),
                  torch.as_tensor(s.in_pos if s.in_pos else [0], dtype=i64, device=dev),
                  torch.as_tensor(dead_pos if dead_pos else [0], dtype=i64, device=dev)]
            self.keep += up
            self._base_set(desc, s.nE, up[:4], self.kmax_e, (len(self.picks), up[4]), (len(s.in_pos), up[5]),
                           (len(dead_pos), up[6]))
        else:
            # the base set is the batch so far: members, their order by data index, means, covariances and list
            # positions are the device batch state itself
            self._base_set(desc, s.nE, (b["bidx"], b["bsort"], b["bmu"], b["sig"]), self.kmax, (s.nE, b["iota"]),
                           (0, b["zero64"]), (s.nE, b["bgpos"]))
        desc.subset_mode, desc.fb_mode = int(self.subset_mode), self.fb_mode
        desc.label_prob, desc.mistake_prob = float(L.label_prob), float(L.mistake_prob)
        desc.label_mode = LABEL_MODES[L.label_estimation]
        desc.noise, desc.eps = float(L.noise), float(L.eps)
        desc.clip_cov = float(L.clip_cov) if L._clip_active() else 0.0
        for j in range(6):
            desc.seed[j] = self.stream.state[j]
        desc.jump1, desc.vk = _ptr(b["jump1"]), _ptr(b["vk_all"])
        desc.draws_out, desc.draws_in = s.draws_out, s.draws_in
        desc.mi, desc.status = _ptr(self.mi), _ptr(gp.status)
        desc.pair_count = _ptr(L.pair_counter)
        if L.generic_pipeline and not L._clip_active() and s.nE + 1 <= (13 if self.subset_mode else 16):
            # workspace of the pipeline of kernels (verdicts, records of the calls to integrate; with a change-estimation
            # subset the pipeline's wide form, one lattice-sum launch per dimension that occurs among the step's calls):
            # what one slab of all candidates takes, capped (the library then walks the candidates in several slabs)
            rel_mc, npat, fb_mc, nfb = s.plan
            desc.mc_rel, desc.mc_fb = (npat if rel_mc else 0), (nfb if fb_mc else 0)     # (read by the size query)
            want = int(self.lib.ital_score_generic_workspace(ctypes.byref(desc)))
            desc.mc_rel, desc.mc_fb = 0, 0
            w = qmc_work(b, min(want, max(L.qmc_work_bytes // 8, 1 << 16)), dev)
            desc.work, desc.work_doubles = _ptr(w), w.numel()

    @staticmethod
    def _base_set(desc, nE, members, ldE, picks, inside, dead):
        """The base set of the descriptor: members = (data indices, their sort order, means, covariances [ldE, ldE]);
        picks / inside / dead = (count, device list) of the picks' positions in the base set and of the list positions
        of live members and of dead candidates."""
        desc.nE, desc.ldE = nE, ldE
        desc.E_idx, desc.E_sort, desc.E_mu, desc.E_sig = [_ptr(m) for m in members]
        desc.n_picks, desc.pick_pos = picks[0], _ptr(picks[1])
        desc.n_in, desc.in_pos = inside[0], _ptr(inside[1])
        desc.n_dead, desc.dead_pos = dead[0], _ptr(dead[1])

    def _attach_samples(self, s):
        """Uploads the step's sampled patterns / feedback configurations (this rank's list positions) and the offsets of
        its candidates in mvndst's stream."""
        L, desc, dev = self.L, s.desc, self.dev
        if s.samples is None:
            if L.keep_scores:
                L.last_patterns.append(None)          # this step enumerates its patterns
            return
        rel_arr, fb_arr, draws_pp = s.samples       # per list position (dead positions hold zeros)
        if L.keep_scores and s.ranges is None:
            L.last_patterns.append(rel_arr)
        if self.gpos_d is None:
            mine = slice(self.pos_offset, self.pos_offset + max(self.n_loc, 1))
        else:
            mine = self.gpos_d.cpu().numpy()
        if rel_arr is not None:
            t_rel = torch.from_numpy(np.ascontiguousarray(rel_arr[mine])).to(dev)
            desc.mc_rel, desc.rel_samples = s.plan[1], _ptr(t_rel)
            self.keep.append(t_rel)
        if fb_arr is not None:
            t_fb = torch.from_numpy(np.ascontiguousarray(fb_arr[mine])).to(dev)
            desc.mc_fb, desc.fb_samples = s.plan[3], _ptr(t_fb)
            self.keep.append(t_fb)
        off = np.concatenate(([0], np.cumsum(draws_pp)[:-1])).astype(np.int64)
        t_off = torch.from_numpy(np.ascontiguousarray(off[mine])).to(dev)
        self.keep.append(t_off)
        desc.draw_off = _ptr(t_off)
        s.total_draws = int(draws_pp.sum())

    def _count_clip_draws(self, s):
        """With clip_cov the number of mvndst calls (one per group of correlated variables) and hence the stream
        consumption depends on the data: a counting pass of the same kernel reports it per candidate."""
        gp, desc, dev, n_loc, pos_offset, gpos_d = self.gp, s.desc, self.dev, self.n_loc, self.pos_offset, self.gpos_d
        counts = torch.zeros(max(n_loc, 1), dtype=torch.int64, device=dev)
        desc.draw_count = _ptr(counts)
        check(self.lib.ital_score_generic(ctypes.byref(desc), self.st))
        desc.draw_count = None
        if gp.collective:
            # uniforms consumed before each of this rank's candidates: prefix over the whole list
            full = torch.zeros(len(self.cand), dtype=torch.int64, device=dev)
            if n_loc:
                if gpos_d is None:
                    full[pos_offset:pos_offset + n_loc] = counts[:n_loc]
                else:
                    full[gpos_d] = counts[:n_loc]
            sharding.all_reduce_sum(full, gp.group)
            excl = torch.cumsum(full, 0) - full
            t_off = (excl[pos_offset:pos_offset + max(n_loc, 1)] if gpos_d is None else excl[gpos_d]).contiguous()
            s.total_draws = int(full.sum().item())
        else:
            t_off = torch.cumsum(counts, 0) - counts
            s.total_draws = int(counts.sum().item())
        self.keep += [counts, t_off]
        desc.draw_off = _ptr(t_off)

    def _score_ranged(self, s):
        """One call per range of candidates: patterns of range r + 1 are decomposed on the host (LAPACK, thread pool)
        while the GPU integrates range r; the uploads go through page-locked memory on a stream of their own (a pageable
        copy would wait for the scorer in front of it)."""
        L, b, desc, dev, n_loc, pos_offset, t = self.L, self.b, s.desc, self.dev, self.n_loc, self.pos_offset, s.t
        npat = s.plan[1]
        if b.get("mc_pin") is None or b["mc_pin"].shape[0] < n_loc or b["mc_pin"].shape[1] < npat:
            b["mc_pin"] = torch.empty((n_loc, ITAL_GENERIC_MAX_REL), dtype=torch.int32).pin_memory()
            b["mc_dev"] = torch.empty((n_loc, ITAL_GENERIC_MAX_REL), dtype=torch.int32, device=dev)
            b["mc_stream"] = torch.cuda.Stream(device=dev)
        pin, t_rel, side = b["mc_pin"], b["mc_dev"], b["mc_stream"]
        main = torch.cuda.current_stream(dev)
        side.wait_stream(main)                   # earlier readers of the device buffer (the step before) are done
        kept = np.zeros((len(self.cand), npat), dtype=np.uint32) if L.keep_scores else None
        base = {f: getattr(desc, f) for f in ("cand", "alive", "mi", "draw_off", "pos_offset")}
        dbg = os.environ.get("ITAL_MC_TIMING")
        tq = time.perf_counter()
        # (try / finally around the WHOLE loop, not only the C call: the generator runs host LAPACK and thread-pool
        # work between the ranges -- if that raises while a deferred range is still running on the library's internal
        # streams, the join below is what orders those kernels, which write `mi` and the workspace, before anything
        # the caller's stream does next with these torch buffers)
        try:
            for lo, hi, rows, last_range in s.ranges:
                if dbg:
                    t_rows = time.perf_counter() - tq
                    tq = time.perf_counter()
                a, e = lo - pos_offset, hi - pos_offset
                flat = pin.view(-1)[a * npat:e * npat]
                flat.copy_(torch.from_numpy(rows.view(np.int32).reshape(-1)))
                dflat = t_rel.view(-1)[a * npat:e * npat]
                with torch.cuda.stream(side):
                    dflat.copy_(flat, non_blocking=True)
                up = torch.cuda.Event()
                up.record(side)
                main.wait_event(up)
                desc.n_cand = e - a
                desc.cand, desc.alive = base["cand"] + 4 * a, base["alive"] + a
                desc.mi, desc.draw_off = base["mi"] + 8 * a, base["draw_off"] + 8 * a
                desc.pos_offset = base["pos_offset"] + a
                desc.mc_rel, desc.rel_samples = npat, dflat.data_ptr()
                # all but the last range leave the library's streams unjoined: the preparation of the next range's
                # first slab then runs under this range's lattice sums (ital_gscore_desc.defer_join)
                desc.defer_join = 0 if last_range else 1
                check(self.lib.ital_score_generic(ctypes.byref(desc), self.st))
                if dbg:
                    print("t=%d range %d..%d: patterns %.1f ms, upload + launch %.1f ms" % (
                        t, lo, hi, t_rows * 1e3, (time.perf_counter() - tq) * 1e3), flush=True)
                    tq = time.perf_counter()
                if kept is not None:
                    kept[lo:hi] = rows
        finally:
            desc.defer_join = 0
            rc_join = self.lib.ital_score_generic_join(self.st)      # (nothing pending after a last range; cheap)
        check(rc_join)
        if kept is not None:
            L.last_patterns.append(kept)

    def _advance(self, s):
        """mvndst's stream past the step; then the standard normals of the next step's pattern sampling: they depend on
        nothing but their count, so drawn now, while the scorer runs, they are off the critical path (same order on
        numpy's global generator).  Only this rank's candidates' normals are computed; the generator is walked past the
        others' (ital_np_legacy_normals).  The next step's live ranks of the local positions [lo, hi) depend on the pick
        this step is about to make: lo - t <= first, last <= hi covers every outcome."""
        n_in_alive = len(s.in_pos)
        self.stream.advance(s.total_draws if s.total_draws is not None else
                            (self.n_alive - n_in_alive) * s.draws_out + n_in_alive * s.draws_in)
        self.n_alive -= 1
        if s.t < self.k:
            rel_nx, npat_nx, fb_nx, _ = self.L._mc_plan(s.nr + 1, self.fb_mode)
            if rel_nx and not fb_nx:
                g0, g1 = (0, self.n_alive) if not self.runs else \
                    (max(self.pos_offset - s.t, 0), min(self.pos_offset + self.n_loc, self.n_alive))
                z = _mc_sampler.walk_normals(self.n_alive, g0, g1, npat_nx * (s.nr + 1), self.L.mc_walk)
                self.z_next = (g0, z.reshape(-1, npat_nx, s.nr + 1))

    def _select_device(self, s):
        """The pick joins the device batch state; its covariance column for the next step."""
        gp, slot = self.gp, s.t - 1
        select_step(gp, self.b, self.scored, gp_model(gp), slot, self.st,
                    fused=not gp.collective and self.n_loc <= FUSED_LAUNCH_MAX)
        if s.t < self.k:
            ev0 = self.L._mark()
            member_column(self.L, gp_model(gp), self.b, slot, self.st)
            self.L._mark("cross_cov", s.t, gp.m, ev0)

    def _select_host(self, s):
        """Subset mode: the winner is resolved on the host (it may or may not extend the base set)."""
        gp, b, E, nE, h = self.gp, self.b, self.E, s.nE, ITAL_REC_HEADER
        recs = select_step(gp, b, self.scored, gp_model(gp), nE, self.st, resolve=False)
        if not gp.collective:
            recs = recs.unsqueeze(0)
        recs_h = self.L._download(recs, "the records of greedy step %d" % s.t).numpy()    # host synchronisation of this greedy step
        self.keep.clear()
        w = sharding.winner(recs_h, 0)
        rec = recs_h[w]
        pick = int(rec[2])
        if int(rec[6]) == gp.rank:
            self.alive[int(rec[7])] = 0
        self.picks.append(pick)
        if pick in E:
            self.pick_pos.append(E.index(pick))
            return
        # new member of the base set: its covariance column, mean and covariances with the members so far
        e_mu, e_sig = self.e_mu, self.e_sig
        e_mu[nE] = rec[3]
        e_sig[nE, nE] = rec[4]
        e_sig[nE, :nE] = rec[h + gp.ldx + gp.cap: h + gp.ldx + gp.cap + nE]
        e_sig[:nE, nE] = e_sig[nE, :nE]
        if s.t < self.k:
            rec_d = recs[w]
            member = (rec_d[h:h + gp.ldx].contiguous(), rec_d[5:6].contiguous(),
                      rec_d[h + gp.ldx:h + gp.ldx + gp.cap].contiguous())
            member_column(self.L, gp_model(gp), b, nE, self.st, member)
            self.keep += member
        self.pick_pos.append(nE)
        E.append(pick)

    def _finish(self):
        """Download of the picks and the status word (OR over steps and ranks); publishes the batch for update()."""
        picks, status = self.picks, None          # subset mode: only the replicated Cholesky append reports: same on all ranks
        if not self.subset_mode:
            host = self.L._download(self.b["ret"], "the picks of the round").tolist()
            picks, status = host[:self.k], host[self.kmax]
        self.keep.clear()
        self.gp.check_status(status)
        picks = [int(i) for i in picks]
        if not self.subset_mode:
            self.L._last_batch = (self.b, picks)
        return picks
