"""The host side of the Monte-Carlo switches (ital_amd/_mc_sampler.py) against numpy's own calls, in the reference's order
(reference ital/ital.py:293-297 `multivariate_normal.rvs` per live candidate, :323-337 `np.random.choice` per pattern):
the samples AND the position numpy's global generator is left at are equal, exactly.  Random SPD covariances (every 17th
candidate repeats a member of the batch: a singular one); no GPU."""
import warnings

import numpy as np
import pytest

from ital_amd import _mc_sampler
from ital_amd._mc_sampler import McPlan, PatternSampler
from ital_amd.mvn_stream import draws_per_call as dpc

P, DEAD = 257, (3, 100, 256)


def _state(nr, seed, n_members=None):
    """A greedy step with nr enumerated variables: members of the base set and P candidates as latent vectors."""
    rng = np.random.default_rng(seed)
    nm = nr - 1 if n_members is None else n_members
    d = nm + 3
    M, Cv = rng.standard_normal((nm, d)), rng.standard_normal((P, d))
    if nm:
        Cv[::17] = M[0]                                   # the candidate duplicates a variable of the batch
    return dict(rows=rng.permutation(1000)[:P], e_mu=rng.standard_normal(nm), e_sig=M @ M.T, mean=rng.standard_normal(1000),
                var=(Cv * Cv).sum(1), cov=M @ Cv.T)


def _sampler(s, plan, nr, **kw):
    table = np.zeros(1000)
    table[s["rows"]] = s["var"]
    cols = np.zeros((len(s["cov"]), 1000))
    cols[:, s["rows"]] = s["cov"]
    kw.setdefault("pick_members", list(range(nr - 1)))
    return PatternSampler(rows=s["rows"], dead=DEAD, e_mu=s["e_mu"], e_sig=s["e_sig"], plan=plan, nr=nr, mean=s["mean"],
                          var=table, cov_cols=cols[kw["pick_members"]], **kw)


def _moments(s, i, pp):
    mean = np.concatenate((s["e_mu"][pp], [s["mean"][s["rows"][i]]]))
    n = len(pp)
    cov = np.empty((n + 1, n + 1))
    cov[:n, :n] = s["e_sig"][np.ix_(pp, pp)]
    cov[:n, n] = cov[n, :n] = s["cov"][pp, i]
    cov[n, n] = s["var"][i]
    return mean, cov


def _pack(x):
    nr = x.shape[-1]
    return ((x > 0) * (1 << np.arange(nr - 1, -1, -1))).sum(axis=-1).astype(np.uint32)     # variable v at bit nr - 1 - v


def _numpy_patterns(s, nr, npat, pp=None, moments=None):
    pp = list(range(nr - 1)) if pp is None else pp
    want = np.zeros((P, npat), dtype=np.uint32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # (singular covariances: numpy's positive-semidefinite check)
        for i in range(P):
            if i not in DEAD:
                mean, cov = (moments or _moments)(s, i, pp)
                want[i] = _pack(np.random.multivariate_normal(mean, cov, npat))
    return want


@pytest.fixture(scope="module")
def rel_cases():
    """Per (nr, monte_carlo_num_rel): numpy's patterns from seed 7 and the generator's next draws afterwards."""
    out = {}
    for nr in range(1, 9):
        for mc in (1, 3):
            s = _state(nr, 100 * nr + mc)
            np.random.seed(7)
            out[nr, mc] = (s, _numpy_patterns(s, nr, nr * mc), np.random.random_sample(3))
    return out


@pytest.mark.parametrize("mc", (1, 3))
@pytest.mark.parametrize("nr", range(1, 9))
def test_patterns_equal_numpy(rel_cases, nr, mc):
    s, want, after = rel_cases[nr, mc]
    npat = nr * mc
    np.random.seed(7)
    rel, fb, draws = _sampler(s, McPlan(True, npat, False, 1), nr).arrays()
    assert fb is None and rel.dtype == np.uint32 and rel.shape == (P, npat)
    assert np.array_equal(rel, want)                       # every live candidate, exactly
    assert not rel[list(DEAD)].any()
    assert np.array_equal(np.random.random_sample(3), after)
    live = np.ones(P, dtype=bool)
    live[list(DEAD)] = False
    assert np.array_equal(draws, live * (npat * 2 * dpc(nr)))


@pytest.mark.parametrize("world", (1, 2, 4))
@pytest.mark.parametrize("nr,mc", [(1, 1), (4, 3), (8, 1)])
def test_local_slices_and_ranges(rel_cases, monkeypatch, nr, mc, world):
    s, want, after = rel_cases[nr, mc]
    npat = nr * mc
    monkeypatch.setattr(_mc_sampler, "MC_CHUNK_MIN", 16)
    bounds = [P * r // world for r in range(world + 1)]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        np.random.seed(7)
        rel = _sampler(s, McPlan(True, npat, False, 1), nr, local=(lo, hi)).arrays()[0]
        assert np.array_equal(rel[lo:hi], want[lo:hi])
        assert np.array_equal(np.random.random_sample(3), after)
        np.random.seed(7)
        sampler = _sampler(s, McPlan(True, npat, False, 1), nr, local=(lo, hi))
        got, at = list(sampler.ranges(4)), lo
        assert np.array_equal(np.random.random_sample(3), after)       # the normals leave the generator before the first range
        assert len(got) > 1
        for a, b, rows, last in got:
            assert a == at and b > a and rows.shape == (b - a, npat)
            assert np.array_equal(rows, want[a:b])
            assert last == (b == hi)
            at = b
        assert at == hi


@pytest.mark.parametrize("nr", (1, 2, 4, 6))
@pytest.mark.parametrize("fb_mode", (1, 2))
def test_feedback_interleave_equals_numpy(fb_mode, nr):
    label_prob, mistake_prob = (1.0, 0.2) if fb_mode == 1 else (0.6, 0.25)
    npat, nfb = 2 * nr, 3 * nr
    s = _state(nr, 40 + nr)
    vals, pr = ([1, -1], [1.0 - mistake_prob, mistake_prob]) if fb_mode == 1 else \
        ([0, 1, -1], [1.0 - label_prob, label_prob * (1.0 - mistake_prob), label_prob * mistake_prob])
    np.random.seed(9)
    want_rel = np.zeros((P, npat), dtype=np.uint32)
    want_fb = np.zeros((P, npat, nfb), dtype=np.uint32)
    want_draws = np.zeros(P, dtype=np.int64)
    bit = 1 << np.arange(nr)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(P):
            if i in DEAD:
                continue
            rel = np.random.multivariate_normal(*_moments(s, i, list(range(nr - 1))), npat) > 0
            want_rel[i] = _pack(rel)
            calls = 0
            for p in range(npat):
                smp = np.random.choice(vals, (nfb, nr), p=pr)
                smp[:, [v for v in range(nr) if not rel[p, v]]] *= -1          # reference ital.py:327, :341
                want_fb[i, p] = ((smp != 0) * bit).sum(1) | (((smp > 0) * bit).sum(1) << 16)
                calls += int((smp != 0).any(axis=1).sum())                      # all-zero feedback rows make no call
            want_draws[i] = npat * dpc(nr) + calls * dpc(nr)                    # npat * npre + calls * d_full
    after = np.random.random_sample(3)
    np.random.seed(9)
    rel, fb, draws = _sampler(s, McPlan(True, npat, True, nfb), nr, fb_mode=fb_mode, user=(label_prob, mistake_prob)).arrays()
    assert np.array_equal(rel, want_rel)
    assert np.array_equal(fb & 0xffff, want_fb & 0xffff) and np.array_equal(fb >> 16, want_fb >> 16)
    assert np.array_equal(draws, want_draws)
    assert np.array_equal(np.random.random_sample(3), after)


def test_subset_members_take_the_base_sets_moments():
    """Change-estimation subset: a candidate that is a member of the base set is described by e_mu / e_sig alone, and its
    full-dimension calls have nE variables, not nE + 1."""
    nr, nE, npat, pp = 3, 5, 6, [0, 3]
    s = _state(nr, 77, n_members=nE)
    base_pos = [10, -1, 42, 3, 200]                       # list positions of the members (3: a pick, dead)
    member_at = {p: e for e, p in enumerate(base_pos) if p >= 0}

    def moments(s, i, pp):
        if i in member_at:
            idx = pp + [member_at[i]]
            return s["e_mu"][idx], s["e_sig"][np.ix_(idx, idx)]
        return _moments(s, i, pp)
    np.random.seed(3)
    want = _numpy_patterns(s, nr, npat, pp, moments)
    after = np.random.random_sample(3)
    np.random.seed(3)
    rel, _, draws = _sampler(s, McPlan(True, npat, False, 1), nr, pick_members=pp, base_pos=base_pos).arrays()
    assert np.array_equal(rel, want)
    assert np.array_equal(np.random.random_sample(3), after)
    assert dpc(nE) != dpc(nE + 1)
    for i in range(P):
        full = dpc(nE) if i in member_at else dpc(nE + 1)
        assert draws[i] == (0 if i in DEAD else npat * (dpc(nr) + 2 * full)), i


def test_mc_plan_and_range_count(monkeypatch):
    assert _mc_sampler.mc_plan(4, 0, 1, None) == (True, 4, False, 1)
    assert _mc_sampler.mc_plan(4, 0, 3, None) == (False, 16, False, 1)
    assert [_mc_sampler.range_count(nr, 125_000) for nr in (6, 9, 10, 16)] == [0, 0, 4, 4]
    assert [_mc_sampler.range_count(nr, 262_144) for nr in (6, 7, 16)] == [0, 6, 6]
    assert _mc_sampler.range_count(12, 32_767) == 0 and _mc_sampler.range_count(12, 125_000, False) == 0
    monkeypatch.setattr(_mc_sampler, "MC_CHUNK_MIN", 64)             # read at call time
    assert _mc_sampler.range_count(10, 597) == 4
    assert _mc_sampler.range_cuts(0, 597, 4).tolist() == [0, 119, 278, 597]
