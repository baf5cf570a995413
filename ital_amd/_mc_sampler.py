"""Host side of the Monte-Carlo switches (reference ital/ital.py:293-297, :318-337): which enumerations a greedy step
replaces by sampling (`mc_plan`), the sign patterns / feedback configurations themselves, drawn from numpy's global
generator in the reference's serial order (`PatternSampler`), and the ranges of candidates a step of sampled patterns is
scored in (`range_count`, `range_cuts`).  Pure numpy on host arrays: the learner downloads what the sampler reads.
"""
import collections
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from .mvn_stream import draws_per_call

HOST_THREADS = max(1, min(int(os.environ.get("ITAL_HOST_THREADS", 16)), os.cpu_count() or 1))   # host share of one GPU
# pattern sampling: ranges of candidates per greedy step (host / GPU overlap), their minimum size, and the number of
# variables from which a step is split at all (below, the step's lattice sums are shorter than the host's decompositions:
# measured at 125 000 x 512, nothing to hide behind; on shards of 262 144 candidates and more from 7 variables on).
# Read where they are used, so an experiment or a test may set them on this module (environment: experiments only)
MC_CHUNKS = int(os.environ.get("ITAL_MC_CHUNKS", 4))
MC_CHUNK_MIN = int(os.environ.get("ITAL_MC_CHUNK_MIN", 8192))
MC_CHUNK_FROM = int(os.environ.get("ITAL_MC_CHUNK_FROM", 10))
_POOL = None

McPlan = collections.namedtuple("McPlan", "rel_mc npat fb_mc nfb")


def mc_plan(nr, fb_mode, monte_carlo_num_rel, monte_carlo_num_fb):
    """Which enumerations the reference replaces by sampling at a step with nr enumerated variables
    (ital.py:293-297, :318-337): (rel sampled?, patterns, feedback sampled?, feedback configurations)."""
    num_rel = nr * monte_carlo_num_rel if monte_carlo_num_rel is not None else None
    rel_mc = num_rel is not None and not (2 ** (nr - 1) < num_rel)
    npat = num_rel if rel_mc else 2 ** nr
    num_fb = nr * monte_carlo_num_fb if monte_carlo_num_fb is not None else None
    if fb_mode == 3:                 # entropy objective: no simulated feedback at all
        fb_mc, nfb = False, 0
    elif fb_mode == 0:
        fb_mc, nfb = False, 1
    elif fb_mode == 1:
        fb_mc = num_fb is not None and not (2 ** (nr - 1) < num_fb)
        nfb = num_fb if fb_mc else 2 ** nr
    else:
        fb_mc = num_fb is not None and not (3 ** nr < 2 * num_fb)
        nfb = num_fb if fb_mc else 3 ** nr - 1
    return McPlan(rel_mc, npat, fb_mc, nfb)


def range_count(nr, n_loc, eligible=True):
    """In how many ranges of candidates a step of nr variables over a shard of n_loc candidates is scored (0: in one call).
    `eligible`: pattern sampling alone, on a shard that is one run of the list (the caller's part of the decision)."""
    big = n_loc >= 32 * MC_CHUNK_MIN
    if eligible and MC_CHUNKS > 0 and (nr >= MC_CHUNK_FROM or (nr >= 7 and big)) and n_loc >= MC_CHUNK_MIN * MC_CHUNKS:
        return MC_CHUNKS + (2 if big else 0)
    return 0


def range_cuts(lo, hi, chunks, smallest=None):
    """Boundaries of the ranges a step of sampled patterns is scored in: sizes 1 : 2 : 4 : ... over [lo, hi) (the first range is
    decomposed while the GPU idles, every later one under the lattice sums of the range before), none shorter than `smallest`
    (default MC_CHUNK_MIN) unless the whole span is.  Ascending int64 array, first entry lo, last entry hi."""
    smallest = MC_CHUNK_MIN if smallest is None else smallest
    span = hi - lo
    cuts = lo + (span * ((1 << np.arange(chunks + 1)) - 1)) // ((1 << chunks) - 1)
    return np.unique(np.concatenate(([lo], cuts[cuts - lo >= min(smallest, span)], [hi])).astype(np.int64))


def host_pool():
    global _POOL
    if _POOL is None:
        _POOL = ThreadPoolExecutor(HOST_THREADS)
    return _POOL


def walk_normals(n_live, j0, j1, per_cand, walk=None):
    """numpy's global generator walked over the `per_cand` standard normals of each of `n_live` candidates
    (multivariate_normal.rvs per candidate, reference ital.py:297); returns those of candidates j0 .. j1-1 (flat).
    `walk` accumulates [normals computed, normals skipped, seconds] (ITAL.mc_walk: diagnostics / tests)."""
    j0, j1 = max(int(j0), 0), min(int(j1), int(n_live))
    j1 = max(j1, j0)
    t0 = time.perf_counter()
    z = _lib.legacy_normals(j0 * per_cand, (j1 - j0) * per_cand, HOST_THREADS)
    _lib.legacy_normals((n_live - j1) * per_cand, 0)
    if walk is not None:
        walk[0] += (j1 - j0) * per_cand
        walk[1] += (n_live - (j1 - j0)) * per_cand
        walk[2] += time.perf_counter() - t0
    return z


class PatternSampler(object):
    """The samples of ONE greedy step: per live candidate one multivariate_normal.rvs (ital.py:297), per pattern one
    np.random.choice (ital.py:323-337), in list order on numpy's global generator.

    rows         data index of every list position [P]
    dead         list positions already picked
    pick_members positions in the base set (indices into e_mu / e_sig) of the picks so far: the enumerated variables
    base_pos     change-estimation subset: list position of every member of the base set (-1: not in the list); None
                 when the base set is the batch so far
    e_mu, e_sig  mean / covariance of the base set
    mean         relevance mean by data index; var, cov_cols [len(pick_members), .]: variance and covariance with every
                 pick by (data index - row0).  Only read with sampled patterns
    plan, nr     mc_plan(nr, fb_mode, ...) of the step; user = (label_prob, mistake_prob)
    local        list positions [lo, hi) whose patterns this rank reads (pattern sampling alone: the others are skipped)
    z_ahead      (first live rank, normals [., npat, nr]) when the caller drew this step's normals ahead
    walk         see walk_normals
    """

    def __init__(self, *, rows, dead, pick_members, e_mu, e_sig, plan, nr, fb_mode=0, user=(1.0, 0.0), base_pos=None,
                 mean=None, var=None, cov_cols=None, row0=0, local=None, z_ahead=None, walk=None):
        self.rows, self.pp, self.e_mu, self.e_sig = np.asarray(rows), list(pick_members), e_mu, e_sig
        self.plan, self.nr, self.fb_mode, self.user = McPlan(*plan), nr, fb_mode, user
        self.mean, self.var, self.cov_cols, self.row0 = mean, var, cov_cols, row0
        self.local, self.z_ahead, self.walk = local, z_ahead, walk
        self.subset_mode = base_pos is not None
        self.P = P = len(self.rows)
        alive = np.ones(P, dtype=bool)
        alive[np.asarray(list(dead), dtype=np.int64)] = False
        self.live = np.flatnonzero(alive)
        self.in_e = np.full(P, -1, dtype=np.int64)                 # member of the base set: its position there
        nE = len(base_pos) if self.subset_mode else len(self.pp)
        if self.subset_mode:
            bp = np.asarray(base_pos, dtype=np.int64).reshape(-1)
            self.in_e[bp[bp >= 0]] = np.flatnonzero(bp >= 0)
        n_full = np.where(self.in_e >= 0, nE, nE + 1)               # orthant dimension of the full-dimension calls
        self.d_full = np.array([draws_per_call(int(v)) for v in range(nE + 2)], dtype=np.int64)[n_full]
        self.npre_draws = (draws_per_call(nr) + self.d_full) if self.subset_mode else self.d_full
        # with pattern sampling alone only the candidates this rank scores (live[jl0:jl1]) are decomposed
        self.jl0, self.jl1 = 0, len(self.live)
        if self.local_only():
            self.jl0, self.jl1 = (int(np.searchsorted(self.live, local[0])), int(np.searchsorted(self.live, local[1])))
        self.weights = (1 << np.arange(nr - 1, -1, -1)).astype(np.uint32)   # variable v at bit nr-1-v

    def local_only(self):
        """Pattern sampling alone with `local` given: only this rank's rows are read (the same decision on every rank:
        `local` is set for all of them or for none)."""
        return self.plan.rel_mc and not self.plan.fb_mc and self.local is not None

    def _moments(self, j0, j1):
        """Mean [n, nr] and covariance [n, nr, nr] of (members so far, candidate) for live candidates j0 .. j1-1
        (ital.py:247-248, :529)."""
        nr, pp, e_mu, e_sig = self.nr, self.pp, self.e_mu, self.e_sig
        rw = self.rows[self.live[j0:j1]]
        rl = rw - self.row0
        mean = np.empty((len(rw), nr))
        cov = np.empty((len(rw), nr, nr))
        mean[:, : nr - 1] = e_mu[pp][None, :] if pp else 0
        cov[:, : nr - 1, : nr - 1] = e_sig[np.ix_(pp, pp)][None] if pp else 0
        mean[:, nr - 1] = self.mean[rw]
        cov[:, nr - 1, nr - 1] = self.var[rl]
        if pp:
            cov[:, : nr - 1, nr - 1] = self.cov_cols[:, rl].T
            cov[:, nr - 1, : nr - 1] = cov[:, : nr - 1, nr - 1]
        if self.subset_mode:
            in_e = self.in_e[self.live[j0:j1]]
            for j in np.flatnonzero(in_e >= 0):                     # members of the base set: covariances from E itself
                idx = pp + [int(in_e[j])]
                mean[j] = e_mu[idx]
                cov[j] = e_sig[np.ix_(idx, idx)]
        elif nr == 1:
            cov[:, 0, 0] = np.maximum(0, cov[:, 0, 0])     # first step: predict_stored(cov_mode='diag') (ital.py:558)
        return mean, cov

    def _transform(self, z, j0, j1):
        mean, cov = self._moments(j0, j1)
        _, sv, vt = np.linalg.svd(cov)
        x = z @ (np.sqrt(sv)[:, :, None] * vt) + mean[:, None, :]
        return ((x > 0) * self.weights).sum(axis=2).astype(np.uint32)

    def _draw_rel(self, j0, j1, z=None):
        """multivariate_normal.rvs for live candidates j0..j1-1: numpy's legacy generator = standard normals in
        order, then x = z . (sqrt(s) v) + mean with (u, s, v) = svd(cov).  The per-candidate LAPACK calls are
        independent of each other: large stacks are cut into slices for a thread pool (numpy's gufuncs release the
        GIL; the result is the same bits as one call)."""
        nr = self.nr
        if z is None:
            z = np.random.standard_normal((j1 - j0, self.plan.npat, nr))
        n = j1 - j0
        workers = min(HOST_THREADS, n * nr * nr // 65536)
        if workers < 2:
            return self._transform(z, j0, j1)
        cuts = np.linspace(0, n, 2 * workers + 1).astype(np.int64)
        parts = list(host_pool().map(lambda ab: self._transform(z[ab[0]:ab[1]], j0 + ab[0], j0 + ab[1]),
                                     zip(cuts[:-1], cuts[1:])))
        return np.concatenate(parts)

    def _draw_fb(self, pats):
        """np.random.choice(vals, (nfb, nr), p) for every pattern of `pats` [..., npat]: uniforms in order."""
        nr = self.nr
        label_prob, mistake_prob = self.user
        if self.fb_mode == 1:
            vals = np.array([1, -1])
            pr = np.array([1.0 - mistake_prob, mistake_prob])
        else:
            vals = np.array([0, 1, -1])
            pr = np.array([1.0 - label_prob, label_prob * (1.0 - mistake_prob), label_prob * mistake_prob])
        cdf = pr.cumsum()
        cdf /= cdf[-1]
        u = np.random.random_sample(pats.shape + (self.plan.nfb, nr))
        smp = vals[cdf.searchsorted(u, side="right")]
        relv = ((pats[..., None] >> np.arange(nr - 1, -1, -1)) & 1).astype(bool)     # [..., npat, nr]
        smp = np.where(relv[..., None, :], smp, -smp)
        vbit = (1 << np.arange(nr)).astype(np.uint32)
        nz = ((smp != 0) * vbit).sum(axis=-1).astype(np.uint32)
        ps = ((smp > 0) * vbit).sum(axis=-1).astype(np.uint32)
        return nz | (ps << np.uint32(16))

    def _local_normals(self):
        """Pattern sampling alone: the legacy generator cannot jump, so every rank walks the whole stream of normals -- but
        only its own candidates' are computed (the others are skipped: raw draws and accept tests,
        ital_np_legacy_normals), and the decompositions are done for those alone."""
        npat, nr = self.plan.npat, self.nr
        if self.z_ahead is None:
            return walk_normals(len(self.live), self.jl0, self.jl1, npat * nr, self.walk).reshape(-1, npat, nr)
        g0, z = self.z_ahead                                       # drawn ahead for live ranks g0 .. g0 + len(z) - 1
        return z[self.jl0 - g0:self.jl1 - g0]

    def enumerated_draws(self):
        """Uniforms of mvndst's stream consumed per list position [P] int64 when the feedback is enumerated."""
        draws = np.zeros(self.P, dtype=np.int64)
        live = self.live
        draws[live] = self.plan.npat * (self.npre_draws[live] + self.plan.nfb * self.d_full[live])
        return draws

    def ranges(self, chunks):
        """Pattern sampling alone, `local` given and not empty: the patterns as a generator of (lo, hi, rows, last) over up
        to `chunks` consecutive ranges of the local list positions -- the per-candidate decompositions of a range are only
        done when it is asked for, so the caller can score one range on the GPU while the host prepares the next.  The
        normals are taken off the generator here, before the first range."""
        live, local, jl0, jl1 = self.live, self.local, self.jl0, self.jl1
        z_loc = self._local_normals()

        def ranges():
            # a SHORT first range: the GPU idles while the host decomposes it (the pick of the step before, the new
            # member's covariance column and the SVDs of its candidates: 0.17 s per step at 1M x 512 with four equal
            # ranges, 2.8 s of a 101 s round), every later range is decomposed under the lattice sums of the one before
            # -- as long as a range is not much longer than the one before (the host decomposes ~1.4 M candidates per
            # second on 16 threads, the GPU integrates 1.6 M (7 variables) .. 47 k (16) per second): sizes 1 : 2 : 4 : ...
            cuts = range_cuts(jl0, jl1, chunks)
            for a, b in zip(cuts[:-1], cuts[1:]):
                lo = local[0] if a == jl0 else int(live[a])
                hi = local[1] if b == jl1 else int(live[b])
                rows = np.zeros((hi - lo, self.plan.npat), dtype=np.uint32)
                rows[live[a:b] - lo] = self._draw_rel(int(a), int(b), z_loc[a - jl0:b - jl0])
                yield lo, hi, rows, bool(b == cuts[-1])
        return ranges()

    def arrays(self):
        """Per list position (dead positions hold zeros): patterns [P, npat] uint32 (or None), feedback [P, npat, nfb]
        uint32 (or None), uniforms of mvndst's stream consumed [P] int64."""
        rel_mc, npat, fb_mc, nfb = self.plan
        live, P, L = self.live, self.P, len(self.live)
        rel_arr = fb_arr = None
        if rel_mc and not fb_mc:
            rel_live = np.zeros((L, npat), dtype=np.uint32)
            z_loc = self._local_normals()
            if self.jl1 > self.jl0:
                rel_live[self.jl0:self.jl1] = self._draw_rel(self.jl0, self.jl1, z_loc)
        elif fb_mc and not rel_mc:
            fb_live = self._draw_fb(np.broadcast_to(np.arange(npat, dtype=np.uint32), (L, npat)))
        else:
            rel_live = np.empty((L, npat), dtype=np.uint32)
            fb_live = np.empty((L, npat, nfb), dtype=np.uint32)
            for j in range(L):                                       # the two samplers interleave per candidate
                rel_live[j] = self._draw_rel(j, j + 1)[0]
                fb_live[j] = self._draw_fb(rel_live[j])
        if rel_mc:
            rel_arr = np.zeros((P, npat), dtype=np.uint32)
            rel_arr[live] = rel_live
        if not fb_mc:
            return rel_arr, None, self.enumerated_draws()
        fb_arr = np.zeros((P, npat, nfb), dtype=np.uint32)
        fb_arr[live] = fb_live
        calls = ((fb_live & 0xffff) != 0).sum(axis=(1, 2))      # all-zero feedback samples make no call
        draws = np.zeros(P, dtype=np.int64)
        draws[live] = npat * self.npre_draws[live] + calls * self.d_full[live]
        return rel_arr, fb_arr, draws
