"""The general-scorer round of ITAL (ital_amd/_generic_round.py) and the launch helpers it shares with the fast path and
MCMI_min (ital_amd/_batch.py `select_step`, `member_column`):
  * a greedy step of sampled patterns scored in ranges of candidates (host / GPU overlap, _mc_sampler.PatternSampler.ranges)
    gives what the same step gives in one call -- at 600 candidates, with the sampler's minimum range size lowered;
  * the number of kernel launches of a fetch, per learner configuration, is a recorded constant.
Run on the GPU box: python -m pytest tests -m gpu."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


def _fetch_mc(dev, k):
    from ital_amd import ITAL, mvn_stream
    rng = np.random.default_rng(5)
    X = rng.random((600, 8))
    np.random.seed(11)
    mvn_stream.GLOBAL.reset()
    A = ITAL(X, length_scale=float(np.sqrt(8 / 12.0)), monte_carlo_num_rel=1, device=dev)
    A.keep_scores = True
    A.update({7: 1, 11: -1, 60: 1})
    picks = A.fetch_unlabelled(k)
    return dict(picks=picks, patterns=A.last_patterns, scores=[s.cpu().numpy() for s in A.last_scores],
                stream=(tuple(mvn_stream.GLOBAL.state), mvn_stream.GLOBAL.draws), after=np.random.random_sample(4))


def test_ranged_scoring_equals_unranged(dev, monkeypatch):
    """Steps 10 and 11 (ITAL_MC_CHUNK_FROM = 10, the dimensions production ranges) in ranges of 64 candidates and more (three of them),
    against the same fetch with every step in one call.  MI within the 1e-8 of DESIGN section 6."""
    from ital_amd import _mc_sampler
    k = 11
    assert _mc_sampler.MC_CHUNK_FROM == 10
    monkeypatch.setattr(_mc_sampler, "MC_CHUNK_MIN", 64)
    assert [_mc_sampler.range_count(t, 597) for t in (9, 10, 11)] == [0, 4, 4]
    ranged = _fetch_mc(dev, k)
    monkeypatch.setattr(_mc_sampler, "MC_CHUNKS", 0)               # ranges disabled
    assert _mc_sampler.range_count(11, 597) == 0
    whole = _fetch_mc(dev, k)
    assert ranged["picks"] == whole["picks"]
    assert len(ranged["patterns"]) == len(whole["patterns"]) == k
    for t in range(k):
        assert np.array_equal(ranged["patterns"][t], whole["patterns"][t]), t
        a, b = ranged["scores"][t], whole["scores"][t]
        print("step %d: MI %s, max |difference| %.3g" % (t + 1, "bit-equal" if np.array_equal(a, b) else "differs",
                                                        float(np.abs(a - b).max())))
        np.testing.assert_allclose(a, b, rtol=1e-8, atol=1e-10, err_msg="step %d" % (t + 1))
    assert ranged["stream"] == whole["stream"]
    assert np.array_equal(ranged["after"], whole["after"])


NAMES = ["ITAL", "ITAL noisy user", "ITAL subset 3", "ITAL clip_cov 0.5, subset 4", "ITAL monte_carlo_num_rel 1",
         "EntropySampling", "MCMI_min step by step"]


def _learners():
    from ital_amd import ITAL, MCMI_min
    from ital_amd.baselines import EntropySampling

    def mcmi(*a, **kw):
        L = MCMI_min(*a, **kw)
        L.round_call = False
        return L
    return {
        "ITAL": (ITAL, {}),
        "ITAL noisy user": (ITAL, dict(label_prob=0.5, mistake_prob=0.25)),
        "ITAL subset 3": (ITAL, dict(change_estimation_subset=3)),
        "ITAL clip_cov 0.5, subset 4": (ITAL, dict(clip_cov=0.5, change_estimation_subset=4)),
        "ITAL monte_carlo_num_rel 1": (ITAL, dict(monte_carlo_num_rel=1)),
        "EntropySampling": (EntropySampling, {}),
        "MCMI_min step by step": (mcmi, {}),
    }


# ital_launch_count() around fetch_unlabelled(4), measured on an MI355X at commit 3fe1ce5 ("Add revoke()/relabel(): take
# feedback back by a Cholesky row deletion"), the parent of the split of the general round into named steps
LAUNCHES = {"ITAL": 12, "ITAL noisy user": 23, "ITAL subset 3": 31, "ITAL clip_cov 0.5, subset 4": 16,
            "ITAL monte_carlo_num_rel 1": 23, "EntropySampling": 23, "MCMI_min step by step": 13}


def launches_of_fetch(name, dev):
    """Kernel launches of one fetch_unlabelled(4) on 150 x 8 (a second learner of the same kind has fetched before: tables
    and buffers that are made once per process or device exist)."""
    from ital_amd import _lib, mvn_stream
    make, kw = _learners()[name]
    X = np.random.default_rng(3).random((150, 8))
    labels = {7: 1, 11: -1, 60: 1}
    np.random.seed(4)
    mvn_stream.GLOBAL.reset()
    got = []
    for _ in range(2):
        L = make(X, length_scale=float(np.sqrt(8 / 12.0)), device=dev, **kw)
        L.update(labels)
        torch.cuda.synchronize()
        c0 = _lib.lib().ital_launch_count()
        picks = L.fetch_unlabelled(4)
        torch.cuda.synchronize()
        got.append(int(_lib.lib().ital_launch_count() - c0))
        assert len(picks) == 4
    return got[1]


@pytest.mark.parametrize("name", NAMES)
def test_launch_counts(dev, name):
    n = launches_of_fetch(name, dev)
    print("%s: %d launches" % (name, n))
    assert n == LAUNCHES[name]
