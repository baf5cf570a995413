"""Host logic of ITAL's one-call round (ital_amd/_fast_round.py), no GPU: the decision how the candidate list reaches the
device (`plan_round`) over real UnseenList objects, a round descriptor prepared ahead of its round against the one a fresh
preparation builds (CPU tensors, a stand-in for the GP, the library's host-only entry points), and `Prepared.patch_share`."""
import ctypes
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ital_amd import ITAL, _fast_round as fr, mvn_stream                      # noqa: E402
from ital_amd.retrieval_base import UnseenList                               # noqa: E402

STATE = tuple(mvn_stream.SEED)
SIG = ("buffers", 4, 64, 48, 1000, 2000, 3000, 1e-6, 1e-12, 1.0, 0.8, "mean", 1 << 30, False, "None")


def _prepared(**changes):
    fields = dict(desc=None, slot=1, k=4, n=32, n_loc=32, m=6, begin=2, cur=1, state_before=STATE, state_after=STATE, draws=0,
                  events=[], sig=SIG)
    fields.update(changes)
    return fr.Prepared(**fields)


def test_plan_round_follows_exactly_the_previous_list_minus_the_previous_batch():
    """The nine fetches of test_gpu_properties.test_device_candidate_list_follows_arbitrary_feedback on a list of 40 ids:
    what the device holds is published after every round as FastRound does; no round is prepared ahead."""
    bufs = object()
    state = dict(u=UnseenList(np.arange(40, dtype=np.int64)), rec=None)
    follows = []

    def fetch(k):
        u = state["u"]
        plan = fr.plan_round(u, bufs, state["rec"], None, False, k, len(u), 2, STATE, SIG)
        assert plan in (fr.COMPACT, fr.UPLOAD)
        follows.append(plan == fr.COMPACT)
        picks = [int(i) for i in u.array()[[7, 2, 11, 5][:k]]]         # (selection order, not ascending)
        state["rec"] = fr.DeviceList(bufs, u, u.version, picks, len(u))
        return picks

    u = state["u"]
    r = fetch(4); assert u.remove(r)                                    # noqa: E702 -- whole batch
    r = fetch(4); assert u.remove(r[:3])                                # noqa: E702 -- one pick left unlabelled
    r = fetch(3); assert u.remove(r + [int(u.array()[20])])             # noqa: E702 -- an extra id with the batch
    r = fetch(4); assert u.remove(r)                                    # noqa: E702 -- unnameable: the ids are removed all the same
    r = fetch(4); assert u.remove(r)                                    # noqa: E702
    r = fetch(2); assert u.remove(r)                                    # noqa: E702
    r = fetch(4)                                                        # no update; then reset(): a new list object
    state["u"] = u = UnseenList(np.arange(40, dtype=np.int64))
    r = fetch(4); assert u.remove(r)                                    # noqa: E702
    r = fetch(4)
    assert follows == [False, True, False, False, True, True, True, False, True]
    # a fetch with no update in between, on the same list object: the device's list still has the picks flagged
    assert fr.plan_round(u, bufs, state["rec"], None, False, 4, len(u), 2, STATE, SIG) == fr.UPLOAD
    # a plain array as the candidate list is never followed
    assert fr.plan_round(u.array(), bufs, state["rec"], None, False, 4, len(u), 2, STATE, SIG) == fr.UPLOAD


def test_plan_round_uses_the_prepared_round_only_when_everything_matches():
    bufs = object()
    u = UnseenList(np.arange(40, dtype=np.int64))
    picks = [9, 3, 30, 12]
    rec = fr.DeviceList(bufs, u, u.version, picks, 40)
    assert u.remove(picks)
    n = len(u)
    p = _prepared(n=n)
    args = dict(k=4, n=n, m=6, stream_state=STATE, signature=SIG)

    def plan(candidates=u, buffers=bufs, record=rec, prepared=p, keep_scores=False, **changes):
        return fr.plan_round(candidates, buffers, record, prepared, keep_scores, **dict(args, **changes))

    assert plan() == fr.PREPARED
    assert plan(stream_state=list(STATE)) == fr.PREPARED            # (the stream's state as a list or a tuple)
    assert plan(prepared=None) == fr.COMPACT
    assert plan(k=3) == fr.COMPACT
    assert plan(n=n - 1) == fr.COMPACT
    assert plan(m=7) == fr.COMPACT
    assert plan(stream_state=STATE[:3] + (STATE[3] + 1,) + STATE[4:]) == fr.COMPACT
    assert plan(signature=SIG[:6] + (3008,) + SIG[7:]) == fr.COMPACT       # the workspace was replaced
    assert plan(keep_scores=True) == fr.COMPACT
    assert plan(buffers=object()) == fr.UPLOAD
    twin = UnseenList(np.arange(40, dtype=np.int64))
    assert twin.remove(picks) and twin.version == u.version and twin.last_removed == u.last_removed
    assert plan(candidates=twin) == fr.UPLOAD


class _Event(object):
    def __init__(self, handle):
        self.cuda_event = handle


def _learner(n, d, m, world=1):
    """An ITAL without data whose `gp` is a stand-in of CPU tensors: all a round descriptor takes of it is sizes and
    data_ptr()s."""
    f64 = torch.float64
    L = ITAL(length_scale=0.8)
    ldx, ldv, cap = 16 * -(-d // 16), 16 * -(-n // 16), 64
    L.gp = types.SimpleNamespace(
        device="cpu", n=n, n_total=n * world, ldx=ldx, ldv=ldv, cap=cap, m=m, row0=0, row1=n, rank=0, world=world,
        collective=world > 1, group=None, mu=torch.zeros(ldv, dtype=f64), s2=torch.zeros(ldv, dtype=f64),
        V=torch.zeros((cap, ldv), dtype=f64), Xd=torch.zeros((n, ldx), dtype=f64), xnorm=torch.zeros(n, dtype=f64),
        status=torch.zeros(1, dtype=torch.int32))
    if world > 1:
        L._transport = (None, ("host", None))       # the records travel through a callback: nothing of it runs here
    return L


def _bytes(desc):
    return ctypes.string_at(ctypes.addressof(desc), ctypes.sizeof(desc))


def _round(L, k, candidates, stream):
    """A FastRound up to its descriptor, as run() gets there (share, buffers, descriptor)."""
    rnd = fr.FastRound(L, k, candidates)
    rnd.stream = stream
    rnd._share()
    rnd._buffers()
    rnd.p = rnd._descriptor()
    return rnd


def test_descriptor_prepared_ahead_equals_a_fresh_one():
    """FastRound's own steps on CPU tensors: round r (k = 4 of 300 candidates, 2 labelled samples) uploads and prepares
    round r + 1 in the other descriptor slot; when that round comes, the prepared descriptor is adopted -- and, with the
    prepared round taken away, a fresh one is built in slot 0 (begin = 2, the same list buffer): the same bytes."""
    k, n, m = 4, 300, 2
    L = _learner(n, 8, m)
    u = UnseenList(np.arange(n, dtype=np.int64))
    stream = mvn_stream.MvnStream()
    r0 = _round(L, k, u, stream)                                            # round r: the list is uploaded
    rb, p0 = r0.rb, r0.p
    assert (p0.begin, p0.slot, p0.draws) == (1, 0, sum(mvn_stream.step_draws(t, n - (t - 1)) for t in (3, 4)))
    assert rb.lists[rb.cur][:n].tolist() == list(range(n)) and rb.device_list is None
    stream.state, stream.draws = p0.state_after, p0.draws                   # (what run() does after the call)
    r0._prepare_next()
    ahead = rb.next
    assert ahead is not None and (ahead.begin, ahead.slot, ahead.cur) == (2, 1, p0.cur ^ 1)
    picks = [17, 3, 250, 99]
    held = fr.DeviceList(rb, u, u.version, picks, n)                        # (what _finish publishes)
    rb.device_list = held
    assert u.remove(picks)
    L.gp.m = m + k                                                          # the batch was labelled
    r1 = _round(L, k, u, stream)
    assert r1.p is ahead and rb.next is None and rb.cur == ahead.cur and rb.device_list is None
    rb.device_list, rb.cur = held, p0.cur                                   # the same round without a prepared one
    r2 = _round(L, k, u, stream)
    fresh = r2.p
    assert (fresh.begin, fresh.slot, fresh.cur) == (2, 0, ahead.cur)
    assert _bytes(rb.descs[1]) == _bytes(rb.descs[0])
    assert fresh._replace(desc=None, slot=1) == ahead._replace(desc=None)      # stream position, draws, signature alike
    assert rb.descs[0].step.n_cand == n - k and rb.descs[0].n_prev == n and rb.descs[0].step.sel_m == m + k


def test_patch_share_gives_what_a_fresh_preparation_gives():
    """Two ranks, k = 4 with timing events (steps 3 and 4): the share of the list this rank gets is known only with the
    picks of the round before."""
    k, n, m = 4, 200, 6
    L = _learner(100, 8, m, world=2)
    L.profile = []
    L.event_pool = [_Event(0x1000 + 8 * i) for i in range(8)]
    rnd = fr.FastRound(L, k, UnseenList(np.arange(n, dtype=np.int64)))
    rnd._share()
    assert (rnd.lo, rnd.n_loc) == (0, 100)
    rnd._buffers()
    rb = rnd.rb
    ahead = rb.prepare(1, k, n, m, 2, 1, STATE, n_prev=100, n_loc=100, pos_offset=0)
    assert [ev[:3] for ev in ahead.events] == [("qmc_main", 3, 100), ("qmc_main", 4, 100)] and len(L.event_pool) == 4
    ahead = ahead.patch_share(97, 3)
    fresh = rb.prepare(0, k, n, m, 2, 1, STATE, n_prev=100, n_loc=97, pos_offset=3)
    a, f = rb.descs[1].step, rb.descs[0].step
    assert (a.n_cand, a.pos_offset, ahead.n_loc) == (f.n_cand, f.pos_offset, fresh.n_loc) == (97, 3, 97)
    assert [ev[:3] for ev in ahead.events] == [ev[:3] for ev in fresh.events] == [("qmc_main", 3, 97), ("qmc_main", 4, 97)]
    assert all(isinstance(ev[3], _Event) and isinstance(ev[4], _Event) for ev in ahead.events)
    # the prepared round does not come: its events are back in the pool
    rb.next = ahead
    rb.drop_prepared()
    assert rb.next is None and len(L.event_pool) == 4
