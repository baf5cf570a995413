"""The selection model of tests/_select_ref.py and its checker, held on the CPU.

Model agreement: `pick` against np.argmax / np.argmin on the live subset; `resolve_winner` against ital_amd.sharding.winner,
the project's other host statement of the rule.

Checker bite: an emulation of the selection kernels in NumPy, written apart from the model in the device's style -- threads
that stride over the positions four loads per trip, xor butterflies inside waves of 64, wave leaders reduced once more, block
partials stored as doubles and reduced by a second launch, one thread walking the ranks' records -- passes the checker at every
shape tests/test_gpu_select_kernels.py runs on the device.  Each mistake of MISTAKES, injected into that emulation, is rejected;
where a mistake leaves the bits of a case unchanged, the test asserts the reason (`_unseen_because`) instead of passing over
it."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _select_ref as ref  # noqa: E402

H = ref.H


# ---------------------------------------------------------------------------------------------------- model agreement
def _special_vector(rng, n, flavour):
    v = rng.uniform(-1, 1, n)
    if flavour == "specials" and n:
        k = max(1, n // 6)
        for val in (np.nan, np.inf, -np.inf, 0.0, -0.0):
            v[rng.integers(0, n, k)] = val
        a = int(rng.integers(n))
        v[a:a + max(2, n // 5)] = rng.choice([0.5, -0.5, np.inf, -np.inf, 0.0])          # a block of equal values
    elif flavour == "no_nan" and n:
        v[rng.integers(0, n, max(1, n // 4))] = rng.choice([1.0, -1.0, np.inf, -np.inf, 0.0, -0.0], max(1, n // 4))
    return v


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("numbering", ["offset", "gpos"])
def test_pick_is_numpys_first_extreme_over_the_live_positions(mode, numbering):
    rng = np.random.default_rng(11 + mode)
    arg = np.argmax if mode == 0 else np.argmin
    seen_nan = seen_tie = 0
    for trial in range(400):
        n = int(rng.integers(0, 40))
        v = _special_vector(rng, n, ("random", "specials", "no_nan")[trial % 3])
        alive = (rng.random(n) < 0.7).astype(np.uint8)
        if trial % 7 == 0:
            alive[:] = 0
        gpos = 5 * rng.permutation(n).astype(np.int64) + 2
        got = ref.pick(v, alive, gpos if numbering == "gpos" else 1000, mode)
        live = np.flatnonzero(alive)
        if live.size == 0:
            assert got is None
            continue
        lp = gpos[live] if numbering == "gpos" else 1000 + live
        order = np.argsort(lp, kind="stable")
        j = int(arg(v[live[order]]))            # the reference: its list holds the live candidates in list order
        assert got[1] == lp[order[j]] and got[2] == live[order[j]]
        assert np.float64(got[0]).tobytes() == np.float64(v[live[order[j]]]).tobytes()
        seen_nan += bool(np.isnan(got[0]))
        seen_tie += bool((v[live] == got[0]).sum() > 1)
    assert seen_nan > 20 and seen_tie > 20


def test_pick_signed_zeros_and_nothing():
    assert ref.pick(np.array([-1.0, -0.0, 0.0]), np.ones(3), 0, 0)[1:] == (1, 1)
    assert np.signbit(ref.pick(np.array([-1.0, -0.0, 0.0]), np.ones(3), 0, 0)[0])
    assert ref.pick(np.array([1.0, 0.0, -0.0]), np.ones(3), np.array([9, 8, 7]), 1)[1:] == (7, 2)
    assert ref.pick(np.zeros(0), np.zeros(0), 0, 0) is None and ref.pick(np.zeros(3), np.zeros(3), 0, 1) is None


@pytest.mark.parametrize("world", ref.WORLDS)
@pytest.mark.parametrize("mode", [0, 1])
def test_resolve_winner_is_shardings_winner(world, mode):
    from ital_amd import sharding
    rng = np.random.default_rng(100 * world + mode)
    sets = []
    for trial in range(300):
        r = np.zeros((world, H))
        r[:, 0] = _special_vector(rng, world, ("random", "specials", "no_nan")[trial % 3])
        r[:, 1] = rng.permutation(4 * world)[:world]
        r[rng.random(world) < 0.25, 1] = -1.0
        sets.append(r)
    for c in ref.resolve_cases(world):
        sets.append(c.bufs["records"][:world * c.rec_len()].reshape(world, c.rec_len()))
    empties = 0
    for r in sets:
        want = sharding.winner(r, mode)
        got = ref.resolve_winner(r, mode)
        assert (got if got is not None else -1) == want, r[:, :2]
        empties += got is None
    assert empties > 0


def test_first_difference_names_the_buffer_and_compares_bits():
    want = dict(record=np.array([1.0, np.nan, -0.0]), work=np.zeros(2), ret=np.array([3, 4], dtype=np.int64))
    same = {k: v.copy() for k, v in want.items()}
    assert ref.first_difference(want, same) is None
    same["work"][:] = 7.0                                     # scratch: excluded
    assert ref.first_difference(want, same) is None
    assert ref.first_difference(want, same, exclude=()).startswith("work[0]")
    for name, i, value in (("record", 2, 0.0), ("record", 1, 1.0), ("record", 1, -np.nan), ("ret", 1, 5)):
        got = {k: v.copy() for k, v in want.items()}
        got[name][i] = value
        assert ref.first_difference(want, got).startswith("%s[%d]" % (name, i)), (name, i, value)
    got = {k: v.copy() for k, v in want.items()}
    got["ret"][0], got["record"][0] = 9, 2.0                  # the first in the order of `want`
    assert ref.first_difference(want, got).startswith("record[0]")
    got["ret"] = got["ret"].astype(np.int32)
    got["record"][0] = 1.0
    assert ref.first_difference(want, got).startswith("ret: shape/type")


# ------------------------------------------------------------------------------------------------------- the emulation
MISTAKES = ("last_equal", "nan_loses", "later_nan", "dead_considered", "partial_order", "gpos_ignored", "trunc32", "tail_unwritten",
            "stale_empty", "sig_one_side", "bsort_appended", "alive_nonowner", "alive_not_cleared", "status_overwritten",
            "status_dropped_no_winner", "state_touched_no_winner")
COMPARE = MISTAKES[:5]         # mistakes of the comparison: the ranks' records meet them too
SCAN = MISTAKES[:9]            # mistakes ital_select_local can make
RESOLVE = MISTAKES[9:]         # mistakes only the resolve step can make


def _sel(mask, a, b):
    return tuple(np.where(mask, x, y) for x, y in zip(a, b))


def _better(a, b, mode, bug, by_ord=False):
    """a precedes b; a, b: (value, list position, local position, partial or rank number)."""
    av, ap, _, ao = a
    bv, bp, _, bo = b
    an, bn = np.isnan(av), np.isnan(bv)
    tie = ap > bp if bug == "last_equal" else ap < bp
    nans = ap > bp if bug == "later_nan" else ap < bp
    if by_ord and bug == "partial_order":
        tie = nans = ao < bo
    with np.errstate(invalid="ignore"):
        strict = av > bv if mode == 0 else av < bv
    res = np.where(an != bn, bn if bug == "nan_loses" else an, np.where(an, nans, np.where(av != bv, strict, tie)))
    return np.where(ap < 0, False, np.where(bp < 0, True, res))


def _nothing(shape):
    return np.zeros(shape), np.full(shape, -1, dtype=np.int64), np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64)


def _butterfly(v, mode, bug, by_ord):
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        o = tuple(x[..., lanes ^ off] for x in v)
        v = _sel(_better(o, v, mode, bug, by_ord), o, v)
    return v


def _block_best(v, mode, bug, by_ord=False):
    """v: [blocks][threads] each -> [blocks]."""
    B, T = v[0].shape
    nw = T // 64
    w = _butterfly(tuple(x.reshape(B, nw, 64) for x in v), mode, bug, by_ord)
    r = list(_nothing((B, 64)))
    for k in range(4):
        r[k][:, :nw] = w[k][:, :, 0]
    return tuple(x[:, 0] for x in _butterfly(tuple(r), mode, bug, by_ord))


def _scan(case, B, T, bug):
    p, b = case.p, case.bufs
    n, mode = p["n_cand"], p["mode"]
    step = B * T
    tid = np.arange(step, dtype=np.int64)
    v = _nothing(step)
    for p0 in range(0, n, 4 * step):
        loaded = []
        for u in range(4):
            q = p0 + u * step + tid
            inn = q < n
            qc = np.where(inn, q, 0)
            live = inn if bug == "dead_considered" else inn & (b["alive"][qc] != 0)
            loaded.append((q, qc, live, b["mi"][qc]))
        for q, qc, live, val in loaded:
            pos = b["gpos"][qc] if b.get("gpos") is not None and bug != "gpos_ignored" else p["pos_offset"] + q
            if bug == "trunc32":
                pos = pos.astype(np.int32).astype(np.int64)
            c = (val, pos, q, tid // T)
            v = _sel(live & _better(c, v, mode, bug), c, v)
    return tuple(x.reshape(B, T) for x in v)


def _winner(case, bug, two_stage):
    mode = case.p["mode"]
    if not two_stage:
        return tuple(x[0] for x in _block_best(_scan(case, 1, 1024, bug), mode, bug))
    n = case.p["n_cand"]
    B = max(1, min(1024, (n + 255) // 256))
    part = _block_best(_scan(case, B, 256, bug), mode, bug)
    work = np.stack([part[0], part[1].astype(np.float64), part[2].astype(np.float64)], axis=1)     # what the first launch leaves
    trips = (B + 255) // 256
    pad = np.zeros((trips * 256, 3))
    pad[:, 1] = -1.0
    pad[:B] = work
    pad = pad.reshape(trips, 256, 3)
    v = _nothing(256)
    for j in range(trips):
        c = (pad[j, :, 0], pad[j, :, 1].astype(np.int64), pad[j, :, 2].astype(np.int64), j * 256 + np.arange(256))
        v = _sel(_better(c, v, mode, bug, True), c, v)
    return tuple(x[0] for x in _block_best(tuple(x.reshape(1, 256) for x in v), mode, bug, True))


def _pack(case, v, rec, bug):
    p, b = case.p, case.bufs
    val, pos, loc = v[0], int(v[1]), int(v[2])
    n = case.rec_len()
    status = 0.0 if p["status_null"] else float(b["status"][0])
    if pos < 0:
        if bug != "stale_empty":
            rec[:n] = 0.0
        rec[1], rec[8] = -1.0, status
        return
    row = int(b["cand"][loc])
    gidx = p["row_offset"] + row
    if bug == "trunc32":
        gidx = int(np.int64(gidx).astype(np.int32))
    rec[:H] = [val, float(pos), float(gidx), b["mu"][row], b["s2"][row], b["xnorm"][row], float(p["rank"]), float(loc), status, 0.0]
    ldx, ldw, kmax = p["ldx"], p["ldw"], p["kmax"]
    for t0 in range(0, ldx, 256):
        rec[H + t0:H + min(ldx, t0 + 256)] = b["X"][row * ldx + t0:row * ldx + min(ldx, t0 + 256)]
    for r in range(ldw):
        if r < p["m"]:
            rec[H + ldx + r] = b["V"][r * p["ldv"] + row]
        elif bug != "tail_unwritten":
            rec[H + ldx + r] = 0.0
    for q in range(kmax):
        if q < p["nprev"]:
            rec[H + ldx + ldw + q] = b["C"][q * p["ldc"] + row]
        elif bug != "tail_unwritten":
            rec[H + ldx + ldw + q] = 0.0


def _resolve(records, world, case, out, bug):
    p = case.p
    kmax, ldx, ldw = case.dims()
    n, mode, slot, rank = case.rec_len(), p["mode"], p["slot"], p["rank"]
    v, win, word = tuple(x[()] for x in _nothing(())), -1, 0
    for w in range(world):
        r = records[w * n:(w + 1) * n]
        c = (r[0], np.int64(r[1]), np.int64(0), np.int64(w))
        if _better(c, v, mode, bug, True):
            v, win = c, w
        word |= int(r[8])
    if win >= 0 or bug != "status_dropped_no_winner":
        out["ret"][kmax] = word if bug == "status_overwritten" else out["ret"][kmax] | word
    if win < 0:
        out["ret"][slot] = -1
        if bug == "state_touched_no_winner":
            out["bidx"][slot] = -1
        return
    r = records[win * n:(win + 1) * n]
    gidx = int(r[2])
    out["bidx"][slot], out["bgpos"][slot], out["bmu"][slot], out["XBn"][slot] = gidx, int(r[1]), r[3], r[5]
    out["sig"][slot * kmax + slot] = r[4]
    for q in range(slot):
        out["sig"][slot * kmax + q] = r[H + ldx + ldw + q]
        if bug != "sig_one_side":
            out["sig"][q * kmax + slot] = r[H + ldx + ldw + q]
    at = slot
    while bug != "bsort_appended" and at > 0 and out["bidx"][out["bsort"][at - 1]] > gidx:
        out["bsort"][at] = out["bsort"][at - 1]
        at -= 1
    out["bsort"][at] = slot
    out["ret"][slot] = gidx
    owner = int(r[6]) == rank
    if (owner and bug != "alive_not_cleared") or (not owner and bug == "alive_nonowner"):
        out["alive"][int(r[7])] = 0
    for k in range(ldx):
        out["XB"][slot * ldx + k] = r[H + k]
    for k in range(ldw):
        out["VB"][slot * ldw + k] = r[H + ldx + k]


def _copy(case):
    return {k: v.copy() for k, v in case.bufs.items() if v is not None}


def emu_local(case, bug=None):
    out = _copy(case)
    _pack(case, _winner(case, bug, case.p["n_cand"] > ref.SMALL_MAX), out["record"], bug)
    return out


def emu_fused(case, bug=None):
    out = _copy(case)
    _pack(case, _winner(case, bug, False), out["record"], bug)
    _resolve(out["record"], 1, case, out, bug)
    return out


def emu_resolve(case, bug=None):
    out = _copy(case)
    _resolve(case.bufs["records"], case.p["world"], case, out, bug)
    return out


# ------------------------------------------------------------------------------------------------ the cases, built once
_CACHE = {}


def _small():
    if "small" not in _CACHE:
        cases = [c for n in ref.N_SMALL for mode in (0, 1) for c in ref.small_cases(n, mode)]
        _CACHE["small"] = [(c, ref.expect_local(c), ref.expect_fused(c)) for c in cases]
    return _CACHE["small"]


def _two_stage():
    if "two" not in _CACHE:
        cases = [ref.two_stage(n, pl) for n in ref.N_TWO_STAGE + (ref.SMALL_MAX,) for pl in ref.PLACEMENTS]
        _CACHE["two"] = [(c, ref.expect_local(c)) for c in cases]
    return _CACHE["two"]


def _resolves():
    if "res" not in _CACHE:
        _CACHE["res"] = [(c, ref.expect_resolve(c)) for w in ref.WORLDS for c in ref.resolve_cases(w)]
    return _CACHE["res"]


def test_the_cases_cover_what_they_claim():
    small = [c for c, _, _ in _small()]
    assert len(small) == len(ref.N_SMALL) * 2 * len(ref.PATTERNS) * len(ref.POS)
    for key, values in (("row_offset", {0, ref.BIG_ROW}), ("ldx", {16, 144}), ("kmax", {4, 9}), ("status_null", {True, False})):
        for n in ref.N_SMALL:
            assert {c.p[key] for c in small if c.p["n_cand"] == n} == values, (key, n)
    assert {(c.p["m"] == 0, c.p["m"] == c.p["ldw"]) for c in small} == {(True, False), (False, True), (False, False)}
    assert {(c.p["nprev"] == 0, c.p["nprev"] == c.p["kmax"]) for c in small} == {(True, False), (False, True), (False, False)}
    assert {int(c.bufs["status"][0]) for c in small} == {0, 5}
    assert {(c.p["slot"] == 0, c.p["slot"] == c.p["kmax"] - 1) for c in small} == {(True, False), (False, True), (False, False)}
    # two equal extremes whose position order and list order disagree do occur, and so do empty ranks
    crossed = 0
    for c in small:
        if "two_equal" in c.name and c.bufs["gpos"] is not None and c.p["n_cand"] >= 1023:
            n = c.p["n_cand"]
            w = ref.pick(c.bufs["mi"][:n], c.bufs["alive"][:n], c.gpos_or_offset(), c.p["mode"])
            same = np.flatnonzero((c.bufs["mi"][:n] == w[0]) & (c.bufs["alive"][:n] != 0))
            crossed += len(same) == 2 and w[2] == same.max()
    assert crossed >= 4
    two = [c for c, _ in _two_stage()]
    assert sum(c.p["n_cand"] > ref.SMALL_MAX for c in two) == 2 * len(ref.PLACEMENTS)
    for c in two:             # on the two-stage route the first of the two equal values (NaNs) sits in the later partial block
        if c.p["n_cand"] > ref.SMALL_MAX and ("equal_two_blocks" in c.name or "two_nans" in c.name):
            count, first_in_lowest_block = _live_facts(c)[:2]
            assert count == 2 and not first_in_lowest_block, c
    worlds = {c.p["world"] for c, _ in _resolves()}
    assert worlds == set(ref.WORLDS)


def test_the_emulation_passes_the_checker_at_every_shape():
    for c, want_local, want_fused in _small():
        assert ref.first_difference(want_local, emu_local(c)) is None, c
        assert ref.first_difference(want_fused, emu_fused(c)) is None, c
    for c, want in _two_stage():
        assert ref.first_difference(want, emu_local(c)) is None, c
        if c.p["n_cand"] > ref.SMALL_MAX:           # the fused call has no size switch: same record
            assert ref.first_difference({"record": want["record"]}, emu_fused(c)) is None, c
    for c, want in _resolves():
        assert ref.first_difference(want, emu_resolve(c)) is None, c


def test_the_emulation_passes_a_full_sequence_of_resolves():
    for kmax, world in ((4, 2), (9, 3)):
        dims, steps = ref.sequence_records(kmax, world, 77 + kmax)
        for rank in range(world):
            state = ref.empty_state(dims)
            for slot, recs in enumerate(steps):
                p = dict(kmax=kmax, ldx=dims[1], ldw=dims[2], mode=0, slot=slot, rank=rank, world=world)
                c = ref.Case("seq", p, dict(state, records=recs))
                want = ref.expect_resolve(c)
                got = emu_resolve(c)
                assert ref.first_difference(want, got) is None, (kmax, world, rank, slot)
                state = {k: got[k] for k in ref.STATE}
                assert list(state["bsort"][:slot + 1]) == list(np.argsort(state["bidx"][:slot + 1], kind="stable"))
                sig = state["sig"][:kmax * kmax].reshape(kmax, kmax)[:slot + 1, :slot + 1]
                assert np.array_equal(sig, sig.T) and np.isfinite(sig).all()


# ------------------------------------------------------------------------------- why a mistake leaves a case unchanged
def _tie_facts(values, lps, groups, mode):
    """Of the entries that hold the winning value (every NaN when one is there): how many, and whether the first in list order
    also sits in the lowest group (partial block or rank)."""
    nan = np.isnan(values)
    if nan.any():
        same = np.flatnonzero(nan)
    else:
        same = np.flatnonzero(values == (values.max() if mode == 0 else values.min()))
    first = same[np.argmin(lps[same])]
    return len(same), groups[first] == groups[same].min(), nan.sum(), len(values)


def _live_facts(c):
    """_tie_facts over the live positions of a select case (groups: the partial block of the two-stage route), or None."""
    n = c.p["n_cand"]
    live = np.flatnonzero(c.bufs["alive"][:n] != 0)
    if live.size == 0:
        return None
    g = c.gpos_or_offset()
    lps = g[live] if np.ndim(g) else live + g
    B = max(1, min(1024, (n + 255) // 256))
    return _tie_facts(c.bufs["mi"][live], lps, (live % (B * 256)) // 256, c.p["mode"])


def _record_facts(c):
    w = c.p["world"]
    r = c.bufs["records"][:w * c.rec_len()].reshape(w, c.rec_len())
    there = np.flatnonzero(r[:, 1] >= 0)
    return None if there.size == 0 else _tie_facts(r[there, 0], r[there, 1], there, c.p["mode"])


def _unseen_because(bug, c, facts, want, two_stage=False, resolve=False):
    """The reason `bug` cannot change the bits of case c (None: it must)."""
    if bug in COMPARE or bug in ("gpos_ignored", "trunc32", "tail_unwritten") or bug in RESOLVE[:4] or bug == "alive_not_cleared":
        if facts is None and bug != "dead_considered" and bug not in RESOLVE[4:]:
            return "nobody is live: nothing is compared, packed or appended"
    if bug in ("last_equal", "later_nan", "nan_loses", "partial_order"):
        count, first_in_lowest_group, nans, size = facts
        if bug == "last_equal":
            return "the winning value is a NaN or occurs once" if nans or count == 1 else None
        if bug == "later_nan":
            return "fewer than two NaNs" if nans < 2 else None
        if bug == "nan_loses":
            return "no NaN, or nothing but NaNs" if nans in (0, size) else None
        if not (two_stage or resolve):
            return "one workgroup, one rank: there are no partials to order"
        return "the first of the equal values also sits in the lowest partial / rank" if count == 1 or first_in_lowest_group else None
    if bug == "dead_considered":
        n = c.p["n_cand"]
        a = ref.pick(c.bufs["mi"][:n], np.ones(n), c.gpos_or_offset(), c.p["mode"])
        w = ref.pick(c.bufs["mi"][:n], c.bufs["alive"][:n], c.gpos_or_offset(), c.p["mode"])
        return "no dead position would win" if (a is None) == (w is None) and (a is None or a[1:] == w[1:]) else None
    if bug == "gpos_ignored":
        if c.bufs["gpos"] is None:
            return "no gpos"
        n = c.p["n_cand"]
        w = ref.pick(c.bufs["mi"][:n], c.bufs["alive"][:n], c.gpos_or_offset(), c.p["mode"])
        a = ref.pick(c.bufs["mi"][:n], c.bufs["alive"][:n], c.p["pos_offset"], c.p["mode"])
        return "the winner's gpos is its own position and the order agrees" if a[1:] == w[1:] else None
    rec = want["record"] if "record" in want else None
    if bug == "trunc32":
        return "list position and data index fit 31 bits" if rec[1] < 2 ** 31 and rec[2] < 2 ** 31 else None
    if bug == "tail_unwritten":
        return "m = ldw and nprev = kmax: no tail" if c.p["m"] == c.p["ldw"] and c.p["nprev"] == c.p["kmax"] else None
    if bug == "stale_empty":
        return "somebody wins: the record is not the empty one" if facts is not None else None
    # ---- the resolve step: the winner's record
    kmax, slot = c.p["kmax"], c.p["slot"]
    word = want["ret"][kmax]
    before = c.bufs["ret"][kmax]
    if bug == "status_overwritten":
        new = _or_of_records(c, want)
        return "the old word is contained in the records' words" if before | new == new else None
    if bug == "status_dropped_no_winner":
        return "somebody wins, or the records carry no new bit" if facts is not None or word == before else None
    if bug == "state_touched_no_winner":
        return "somebody wins" if facts is not None else None
    if bug == "sig_one_side":
        return "slot 0: no off-diagonal entry" if slot == 0 else None
    gidx = want["bidx"][slot]
    if bug == "bsort_appended":
        return "the new data index is the largest so far" if slot == 0 or gidx >= c.bufs["bidx"][:slot].max() else None
    owner = _owner(c, want)
    if bug == "alive_nonowner":
        return "this rank owns the winner" if owner == c.p["rank"] else None
    if bug == "alive_not_cleared":
        return "another rank owns the winner" if owner != c.p["rank"] else None
    raise AssertionError(bug)


def _records_of(c, want):
    if "records" in c.bufs:
        w = c.p["world"]
        return c.bufs["records"][:w * c.rec_len()].reshape(w, c.rec_len())
    return want["record"][None, :c.rec_len()]


def _or_of_records(c, want):
    word = 0
    for r in _records_of(c, want):
        word |= int(r[8])
    return word


def _owner(c, want):
    r = _records_of(c, want)
    return int(r[ref.resolve_winner(r, c.p["mode"])][6])


@pytest.mark.parametrize("bug", MISTAKES)
def test_the_checker_rejects(bug):
    rejected = {"small": 0, "two": 0, "resolve": 0}

    def judge(family, c, want, got, facts, **kw):
        diff = ref.first_difference(want, got)
        why = _unseen_because(bug, c, facts, want, **kw)
        assert (diff is None) == (why is not None), (bug, c, diff, why)
        rejected[family] += diff is not None

    for c, want_local, want_fused in _small():
        if bug in SCAN:
            judge("small", c, want_local, emu_local(c, bug), _live_facts(c))
        else:
            judge("small", c, want_fused, emu_fused(c, bug), _live_facts(c))
    if bug in SCAN:
        for c, want in _two_stage():
            if c.p["n_cand"] == ref.N_TWO_STAGE[1]:   # the same placements two trips deep: the unmodified emulation runs them above
                continue
            judge("two", c, want, emu_local(c, bug), _live_facts(c), two_stage=c.p["n_cand"] > ref.SMALL_MAX)
    if bug in COMPARE[:3] + ("partial_order",) or bug in RESOLVE:
        for c, want in _resolves():
            judge("resolve", c, want, emu_resolve(c, bug), _record_facts(c), resolve=True)
    # every family the mistake can show in has caught it at least once
    if bug in SCAN:
        assert rejected["two"] > 0, rejected
        assert rejected["small"] > 0 or bug == "partial_order", rejected
    if bug in RESOLVE:
        assert rejected["resolve"] > 0, rejected
        assert rejected["small"] > 0 or bug == "alive_nonowner", rejected
    if bug in COMPARE[:3] + ("partial_order",):
        assert rejected["resolve"] > 0, rejected
