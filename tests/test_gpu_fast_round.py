"""The one-call round of ITAL (ital_amd/_fast_round.py) seen from outside, on one rank: which of its two descriptors a round
runs and how its candidate list reached the device (`last_round` = (begin, slot): begin 1 uploaded, 2 compacted on the
device), that a labelled set outgrowing its capacity inside the loop costs one upload and nothing else, that no timing
event of a prepared round is lost, and MCMI_min's one-call round against its step-by-step form.
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


def _loop(dev, make, ks, round_call):
    """Retrieval loop on 300 x 8 from the stream's start: fetch k, label the whole batch, for every k of `ks` (no feedback
    after the last).  Returns the picks, `last_round` and the stream position after every fetch."""
    from ital_amd import mvn_stream
    X = np.random.default_rng(8).random((300, 8))
    mvn_stream.GLOBAL.reset()
    L = make(X, length_scale=0.8, device=dev)
    L.round_call = round_call
    L.update({5: 1, 9: -1})
    picks, how, draws = [], [], []
    for i, k in enumerate(ks):
        ret = L.fetch_unlabelled(k)
        picks.append(ret)
        how.append(L.last_round if round_call else None)
        draws.append(mvn_stream.GLOBAL.draws)
        if i + 1 < len(ks):
            L.update({j: 1.0 if X[j, 0] > 0.5 else -1.0 for j in ret})
    return picks, how, draws


def test_slot_sequence(dev):
    """Six rounds of the retrieval loop alternate between the two descriptors, each prepared during the round before; a
    seventh of another batch size follows the device's list but not the prepared descriptor: a fresh one in slot 0."""
    from ital_amd import ITAL
    ks = [4] * 6 + [3]
    picks, how, draws = _loop(dev, ITAL, ks, True)
    print("last_round:", how)
    assert how == [(1, 0), (2, 1), (2, 0), (2, 1), (2, 0), (2, 1), (2, 0)]
    picks_s, _, draws_s = _loop(dev, ITAL, ks, False)
    assert picks == picks_s and draws == draws_s


def test_capacity_growth_inside_the_loop(dev):
    """Capacity 16, m = 2, 6, 10, 14: at m = 14 no next round is prepared (m + k > capacity), the update that follows
    grows the GP and with it replaces the batch buffers: that round uploads its list, the loop goes on from there."""
    from ital_amd import ITAL

    class Small(ITAL):
        gp_capacity = 16
    ks = [4] * 6
    picks, how, draws = _loop(dev, Small, ks, True)
    print("last_round:", how)
    assert [h[0] for h in how] == [1, 2, 2, 2, 1, 2]
    picks_s, _, draws_s = _loop(dev, Small, ks, False)
    assert picks == picks_s and draws == draws_s


def test_no_event_is_lost(dev):
    """Every event taken from the pool is either in a profile tuple (two each) or held by the prepared next round, which
    brackets the lattice sums of its steps t >= 3 (k = 4: two tuples, k = 3: one); a prepared round that does not come
    gives its events back.  (The number of tuples the prepared round holds is taken from its definition, not read from
    the learner's private state: an event the prepared round lost and a miscounted tuple look alike here; which events a
    preparation takes and that a dropped one returns them is checked on the host, tests/test_fast_round_host.py.)"""
    from ital_amd import ITAL, mvn_stream
    X = np.random.default_rng(9).random((200, 6))
    mvn_stream.GLOBAL.reset()
    L = ITAL(X, length_scale=0.8, device=dev)
    L.update({5: 1, 9: -1})
    L.profile = []
    L.event_pool = [torch.cuda.Event(enable_timing=True) for _ in range(64)]
    for ev in L.event_pool:
        ev.record()
    torch.cuda.synchronize()
    for rnd in range(3):
        ret = L.fetch_unlabelled(4)
        pending = 2                     # the next round of 4 is prepared (196 - 4 * rnd candidates, capacity 64): t = 3, 4
        print("round %d: %d in the pool, %d profile tuples" % (rnd, len(L.event_pool), len(L.profile)))
        assert len(L.event_pool) + 2 * len(L.profile) + 2 * pending == 64
        L.update({j: 1.0 if X[j, 0] > 0.5 else -1.0 for j in ret})
    assert all(p[0].startswith("qmc_") for p in L.profile)
    L.fetch_unlabelled(3)               # the prepared round of 4 does not come; the next round of 3 is prepared: t = 3
    print("then: %d in the pool, %d profile tuples" % (len(L.event_pool), len(L.profile)))
    assert len(L.profile) == 3 * 2 + 1
    assert len(L.event_pool) + 2 * len(L.profile) + 2 * 1 == 64


def test_mcmi_round_equals_steps(dev):
    """MCMI_min: the one-call round and the step-by-step fetch pick the same samples and leave the same candidates; the
    step-by-step fetch of 4 takes its recorded 13 launches (test_gpu_generic_round.LAUNCHES)."""
    from ital_amd import MCMI_min, _lib
    X = np.random.default_rng(3).random((150, 8))
    out = []
    for round_call in (True, False, False):          # (the second step-by-step learner: tables and buffers exist)
        L = MCMI_min(X, length_scale=float(np.sqrt(8 / 12.0)), device=dev)
        L.round_call = round_call
        L.update({7: 1, 11: -1, 60: 1})
        torch.cuda.synchronize()
        c0 = _lib.lib().ital_launch_count()
        picks = L.fetch_unlabelled(4)
        torch.cuda.synchronize()
        out.append((picks, list(L.candidates), int(_lib.lib().ital_launch_count() - c0)))
    assert len(out[0][0]) == 4
    assert out[0][:2] == out[1][:2] == out[2][:2]
    assert len(out[0][1]) == 150 - 3 - 4
    assert out[2][2] == 13
