"""Exact host model of the selection rule (ital_select_local, ital_select_resolve, ital_select_fused), the checker that holds
a call to it, and the inputs the host and the device tests share.

The model is written from the reference's statements -- np.argmax (ital/ital.py:130), np.argmin (ital/mcmi.py:77): the FIRST
extreme in candidate-list order, a NaN counting as the extreme; append + del (ital/ital.py:131-132) -- and from the contracts
in include/ital_hip.h, not from the device code: `pick` sorts the live positions by list position and takes the first extreme
of that sequence; `resolve` applies the same `pick` to the ranks' records.  The selection does no arithmetic, so every
comparison is equality of bits; there is no tolerance anywhere in this module.

A call is described by a `Case`: scalars in `p`, flat NumPy buffers (with guard entries behind their last valid element) in
`bufs`.  `expect_*` returns the image of ALL buffers a correct call leaves: the write set from the model, everything else as
it was.  `first_difference` names the first buffer and index where an after-image departs from it.  The `work` scratch of
ital_select_local is scratch: it is the one buffer excluded from every comparison.

NumPy and Python only (no torch): tests/test_select_ref_host.py runs all of it without a GPU."""
import bisect

import numpy as np

H = 10                      # ITAL_REC_HEADER
G = 4                       # guard entries behind every buffer
NAN = float("nan")
S32 = -0x5A5A5A5            # sentinel of int32 buffers
S64 = -0x5A5A5A5A5A5A5      # sentinel of int64 buffers
S8 = 0x5A                   # sentinel of the alive flags' guard (non-zero: a flag read out of range counts as alive)
SMALL_MAX = 1 << 18         # ital_select_local: n_cand above this takes the two-stage route
EXCLUDED = ("work",)


# ----------------------------------------------------------------------------------------------------------- the model
def pick(mi, alive, gpos_or_offset, mode):
    """(value, list position, local position) of the first extreme among the live positions in order of list position, or
    None.  gpos_or_offset: an integer (list position of q = offset + q) or an array (list position of q = gpos[q])."""
    mi = np.asarray(mi, dtype=np.float64)
    n = len(mi)
    live = np.flatnonzero(np.asarray(alive)[:n] != 0)
    if live.size == 0:
        return None
    if np.ndim(gpos_or_offset) == 0:
        lp = live.astype(np.int64) + np.int64(gpos_or_offset)
    else:
        lp = np.asarray(gpos_or_offset, dtype=np.int64)[live]
    order = np.argsort(lp, kind="stable")
    seq = mi[live[order]]                     # the scores as the reference's list would hold them
    isnan = np.isnan(seq)
    if isnan.any():
        j = int(np.flatnonzero(isnan)[0])
    else:
        ext = seq.max() if mode == 0 else seq.min()
        j = int(np.flatnonzero(seq == ext)[0])
    return seq[j], int(lp[order[j]]), int(live[order[j]])


def record(mi, cand, alive, gpos_or_offset, row_offset, rank, mode, mu, s2, X, xnorm, V, m, ldw, C, nprev, kmax, status):
    """The record of ital_select_local.  X: [rows][ldx], V: [>= m][>= rows], C: [>= nprev][>= rows]; status: int or None."""
    ldx = X.shape[1]
    rec = np.zeros(H + ldx + ldw + kmax)
    rec[8] = 0.0 if status is None else float(int(status))
    w = pick(mi, alive, gpos_or_offset, mode)
    if w is None:
        rec[1] = -1.0
        return rec
    val, lp, loc = w
    row = int(cand[loc])
    rec[0], rec[1], rec[2], rec[3], rec[4], rec[5] = val, float(lp), float(int(row_offset) + row), mu[row], s2[row], xnorm[row]
    rec[6], rec[7], rec[9] = float(rank), float(loc), 0.0
    rec[H:H + ldx] = X[row]
    rec[H + ldx:H + ldx + m] = V[:m, row]
    rec[H + ldx + ldw:H + ldx + ldw + nprev] = C[:nprev, row]
    return rec


def resolve_winner(records, mode):
    """Index of the winning record (None: every record is empty): the selection rule over (records[w][0], records[w][1])."""
    records = np.asarray(records, dtype=np.float64)
    w = pick(records[:, 0], records[:, 1] >= 0, records[:, 1].astype(np.int64), mode)
    return None if w is None else w[2]


def resolve(records, rank, mode, slot, state, dims):
    """The batch state, alive flags and ret after ital_select_resolve.  state: flat arrays bidx, bgpos, bsort, bmu, sig, XB,
    XBn, VB, alive, ret (copied, never changed in place); dims = (kmax, ldx, ldw)."""
    kmax, ldx, ldw = dims
    records = np.asarray(records, dtype=np.float64)
    s = {k: v.copy() for k, v in state.items()}
    word = 0
    for r in records:
        word |= int(r[8])
    s["ret"][kmax] |= word
    win = resolve_winner(records, mode)
    if win is None:
        s["ret"][slot] = -1
        return s
    r = records[win]
    gidx = int(r[2])
    s["bidx"][slot], s["bgpos"][slot], s["bmu"][slot], s["XBn"][slot] = gidx, int(r[1]), r[3], r[5]
    s["XB"][slot * ldx:(slot + 1) * ldx] = r[H:H + ldx]
    s["VB"][slot * ldw:(slot + 1) * ldw] = r[H + ldx:H + ldx + ldw]
    s["sig"][slot * kmax + slot] = r[4]
    for q in range(slot):
        s["sig"][slot * kmax + q] = s["sig"][q * kmax + slot] = r[H + ldx + ldw + q]
    members = [int(v) for v in state["bsort"][:slot]]                   # ordered by data index so far
    at = bisect.bisect_right([int(state["bidx"][v]) for v in members], gidx)
    members.insert(at, slot)                                            # behind its equals: stable
    s["bsort"][:slot + 1] = members
    s["ret"][slot] = gidx
    if int(r[6]) == rank:
        s["alive"][int(r[7])] = 0
    return s


STATE = ("bidx", "bgpos", "bsort", "bmu", "sig", "XB", "XBn", "VB", "alive", "ret")


class Case:
    def __init__(self, name, p, bufs):
        self.name, self.p, self.bufs = name, p, bufs

    def __repr__(self):
        return self.name

    def gpos_or_offset(self):
        g = self.bufs.get("gpos")
        return self.p["pos_offset"] if g is None else g[:self.p["n_cand"]]

    def dims(self):
        return self.p["kmax"], self.p["ldx"], self.p["ldw"]

    def rec_len(self):
        return H + self.p["ldx"] + self.p["ldw"] + self.p["kmax"]

    def status(self):
        return None if self.p["status_null"] else int(self.bufs["status"][0])

    def model_record(self):
        p, b = self.p, self.bufs
        n, R = p["n_cand"], p["rows"]
        return record(b["mi"][:n], b["cand"][:n], b["alive"][:n], self.gpos_or_offset(), p["row_offset"], p["rank"], p["mode"],
                      b["mu"], b["s2"], b["X"].reshape(R + 1, p["ldx"]), b["xnorm"], b["V"].reshape(-1, p["ldv"]), p["m"],
                      p["ldw"], b["C"].reshape(-1, p["ldc"]), p["nprev"], p["kmax"], self.status())


def expect_local(case):
    """Every buffer after ital_select_local."""
    e = {k: v.copy() for k, v in case.bufs.items() if v is not None}
    e["record"][:case.rec_len()] = case.model_record()
    return e


def expect_fused(case):
    """Every buffer after ital_select_fused: the record, then the resolve of that one record."""
    e = expect_local(case)
    rec = e["record"][:case.rec_len()]
    e.update(resolve(rec[None, :], case.p["rank"], case.p["mode"], case.p["slot"], {k: case.bufs[k] for k in STATE}, case.dims()))
    return e


def expect_resolve(case):
    """Every buffer after ital_select_resolve (case.bufs['records']: [world][rec_len] and a guard row)."""
    e = {k: v.copy() for k, v in case.bufs.items()}
    recs = case.bufs["records"][:case.p["world"] * case.rec_len()].reshape(case.p["world"], case.rec_len())
    e.update(resolve(recs, case.p["rank"], case.p["mode"], case.p["slot"], {k: case.bufs[k] for k in STATE}, case.dims()))
    return e


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32, 2: np.int16}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def first_difference(expected, after, exclude=EXCLUDED):
    """None, or 'name[i]: got ..., want ...' for the first buffer (in the order of `expected`) and the first index at which
    `after` does not hold the expected bits."""
    for name, want in expected.items():
        if name in exclude:
            continue
        got = after[name]
        if got.shape != want.shape or got.dtype != want.dtype:
            return "%s: shape/type %s %s, want %s %s" % (name, got.shape, got.dtype, want.shape, want.dtype)
        bad = np.flatnonzero(_bits(got) != _bits(want))
        if bad.size:
            i = int(bad[0])
            return "%s[%d]: got %r, want %r" % (name, i, got[i], want[i])
    return None


# ------------------------------------------------------------------------------------------------ inputs: select_local
N_SMALL = (0, 1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 5000)
PATTERNS = ("random", "first", "last", "all_equal", "two_equal", "one_nan", "two_nan", "inf", "zeros", "dead_extreme", "all_dead")
POS = ("zero", "big", "gpos")
ROWS = 23                   # rows of the feature table the candidates point into
BIG_POS = 2 ** 40 + 3
BIG_ROW = 2 ** 33 + 1


def _guard(a, fill, extra=G):
    out = np.full(len(a) + extra, fill, dtype=a.dtype)
    out[:len(a)] = a
    return out


def layout(i):
    """The parameters a case does not name, cycled by a running number so that every listed value of each occurs with every
    n_cand and mode, and the pairs mix."""
    kmax = (4, 9)[(i // 2) % 2]
    ldw = (8, 5)[(i // 3) % 2]
    return dict(row_offset=(0, BIG_ROW)[i % 2], m=(0, 3, ldw)[i % 3], nprev=(0, 2, kmax)[(i // 2) % 3], ldx=(16, 144)[(i // 5) % 2],
                kmax=kmax, ldw=ldw, status=(0, 5, None)[(i // 4) % 3], slot=(0, 1, kmax - 1)[(i // 7) % 3], gbase=(0, 2 ** 35)[(i // 3) % 2])


def _tables(lay, rng, n, mode):
    """Feature table, GP columns, batch state and scratch of a case (everything but mi, cand, alive, gpos)."""
    R, ldx, ldw, kmax, m, nprev, slot = ROWS, lay["ldx"], lay["ldw"], lay["kmax"], lay["m"], lay["nprev"], lay["slot"]
    ldv, ldc = R + 3, R + 5
    X = np.full((R + 1, ldx), NAN)
    X[:R] = rng.standard_normal((R, ldx))
    V = np.full((ldw + 1, ldv), NAN)
    V[:m, :R] = rng.standard_normal((m, R))
    C = np.full((kmax + 1, ldc), NAN)
    C[:nprev, :R] = rng.standard_normal((nprev, R))
    vec = lambda: _guard(rng.standard_normal(R), NAN, 1)     # noqa: E731
    b = dict(mu=vec(), s2=vec(), X=X.ravel(), xnorm=vec(), V=V.ravel(), C=C.ravel(),
             status=np.array([lay["status"] or 0, S32], dtype=np.int32),
             record=np.full(H + ldx + ldw + kmax + G, NAN), work=np.full(3 * 1024 + G, NAN))
    # the batch: members 0 .. slot - 1 hold recognisable values and a bsort that orders them, everything else NaN / sentinel
    bidx = np.full(kmax + G, S64, dtype=np.int64)
    bidx[:slot] = rng.permutation(2 * kmax)[:slot] * 7 + (BIG_ROW if lay["row_offset"] else 0) + 20
    bsort = np.full(kmax + G, S32, dtype=np.int32)
    bsort[:slot] = np.argsort(bidx[:slot], kind="stable")
    bgpos = np.full(kmax + G, S64, dtype=np.int64)
    bgpos[:slot] = 900 + np.arange(slot)
    dbl = lambda size, filled: _guard(np.where(np.arange(size) < filled, 1.0 + np.arange(size) / 64.0, NAN), NAN)    # noqa: E731
    sig = np.full((kmax, kmax), NAN)
    sig[:slot, :slot] = 2.0 + np.arange(slot * slot).reshape(slot, slot) / 32.0
    ret = np.full(kmax + 1 + G, S64, dtype=np.int64)
    ret[:slot] = bidx[:slot]
    ret[kmax] = 2
    b.update(bidx=bidx, bgpos=bgpos, bsort=bsort, bmu=dbl(kmax, slot), sig=_guard(sig.ravel(), NAN), XB=dbl(kmax * ldx, slot * ldx),
             XBn=dbl(kmax, slot), VB=dbl(kmax * ldw, slot * ldw), ret=ret)
    p = dict(n_cand=n, mode=mode, rows=R, ldx=ldx, ldw=ldw, kmax=kmax, m=m, nprev=nprev, slot=slot, ldv=ldv, ldc=ldc, rank=3,
             row_offset=lay["row_offset"], status_null=lay["status"] is None)
    return p, b


def _positions(n, pos, gbase, rng):
    """(pos_offset, gpos or None, list position of every q)."""
    q = np.arange(n, dtype=np.int64)
    if pos == "gpos":
        gpos = gbase + 3 * rng.permutation(n).astype(np.int64) + 1
        return 0, gpos, gpos
    off = BIG_POS if pos == "big" else 0
    return off, None, off + q


def _finish(name, p, b, mi, cand, alive, off, gpos):
    p["pos_offset"] = off
    b.update(mi=_guard(mi, NAN), cand=_guard(cand.astype(np.int32), ROWS), alive=_guard(alive.astype(np.uint8), S8),
             gpos=None if gpos is None else _guard(gpos, S64))
    return Case(name, p, b)


def small_case(n, mode, pattern, pos, i):
    """One input of the single-workgroup route.  About a third of the positions are dead and hold NaN (a dead position that is
    looked at wins); the pattern then places its values on live positions."""
    rng = np.random.default_rng(1000 + i)
    lay = layout(i)
    p, b = _tables(lay, rng, n, mode)
    off, gpos, lp = _positions(n, pos, lay["gbase"], rng)
    sgn = 1.0 if mode == 0 else -1.0
    E = 5.0 * sgn
    alive = (rng.random(n) < 0.7) if n >= 4 else np.ones(n, dtype=bool)
    if n >= 4:
        alive[rng.integers(n)] = True
    mi = rng.uniform(-1.0, 1.0, n)
    live = np.flatnonzero(alive)

    def some(count):
        return rng.choice(live, size=min(count, live.size), replace=False)

    if pattern == "first" and live.size:
        mi[live[0]] = E
    elif pattern == "last" and live.size:
        mi[live[-1]] = E
    elif pattern == "all_equal":
        mi[:] = 0.25
    elif pattern == "two_equal" and live.size:
        pair = some(2)
        for _ in range(64):                       # a pair whose q order and list order disagree, where the map allows one
            if len(pair) == 2 and (pair[0] < pair[1]) != (lp[pair[0]] < lp[pair[1]]):
                break
            pair = some(2)
        mi[pair] = E
    elif pattern == "one_nan":
        mi[some(1)] = NAN
    elif pattern == "two_nan":
        mi[some(2)] = NAN
    elif pattern == "inf":
        at = some(3)
        mi[at] = np.array([sgn * np.inf, -sgn * np.inf, E])[:len(at)]
    elif pattern == "zeros":
        mi[:] = -sgn * rng.uniform(0.5, 1.0, n)
        at = some(2)
        mi[at] = np.array([-0.0, 0.0])[:len(at)]
    elif pattern == "dead_extreme" and n >= 2:
        d = int(rng.integers(n))
        alive[d] = False
        mi[d] = 2.0 * E
    elif pattern == "all_dead":
        alive[:] = False
    dead_nan = ~alive if pattern not in ("dead_extreme", "all_dead") else np.zeros(n, dtype=bool)
    mi[dead_nan] = NAN
    name = "n%d-mode%d-%s-%s-#%d" % (n, mode, pattern, pos, i)
    return _finish(name, p, b, mi, rng.integers(0, ROWS, n), alive, off, gpos)


def small_cases(n, mode):
    """The cases of one n_cand and mode: every pattern with every way of numbering the list."""
    base = (N_SMALL.index(n) * 2 + mode) * len(PATTERNS) * len(POS) if n in N_SMALL else 7 * n
    return [small_case(n, mode, pat, pos, base + j * len(POS) + k) for j, pat in enumerate(PATTERNS) for k, pos in enumerate(POS)]


# ------------------------------------------------------------------------------------- inputs: the two-stage route
N_TWO_STAGE = (SMALL_MAX + 1, SMALL_MAX + 1024 * 256 + 7)
PLACEMENTS = ("pos0", "second_trip", "last", "equal_two_blocks", "equal_one_block", "nan_last_partial", "two_nans", "all_dead", "gpos_equal")


def two_stage_case(n, placement, mode, i=0):
    """n above 1 << 18 (or exactly there: the same input through the single-workgroup route).  The partial launch has 1024 blocks
    of 256 threads; thread t of block b sees positions b * 256 + t + j * (1 << 18)."""
    rng = np.random.default_rng(5000 + i)
    lay = layout(i + 1)
    p, b = _tables(lay, rng, n, mode)
    off, gpos, lp = _positions(n, "gpos" if placement == "gpos_equal" else ("big" if i % 2 else "zero"), lay["gbase"], rng)
    sgn = 1.0 if mode == 0 else -1.0
    E = 5.0 * sgn
    alive = rng.random(n) < 0.75
    mi = rng.uniform(-1.0, 1.0, n)
    stride = 1 << 18
    # position 300 is block 1's; `later` is a higher position that block 0 sees on its second trip (n > stride), so the lower
    # list position sits in the LATER partial -- on the single-workgroup route (n = stride) just another position
    later = stride + 5 if n > stride + 5 else (n - 1 if n > stride else 5 + 256 * 7)
    forced = []
    if placement == "pos0":
        forced = [0]
    elif placement == "second_trip":
        forced = [min(stride, n - 1)]
    elif placement == "last":
        forced = [n - 1]
    elif placement == "equal_two_blocks":
        forced = [300, later]
    elif placement == "equal_one_block":
        forced = [256 * 9 + 17, 256 * 9 + 200]
    elif placement == "gpos_equal":
        forced = [4000, 256 * 700 + 3]            # a permuted list: which of the two comes first is the map's business
    elif placement == "two_nans":
        forced = [300, later]                     # the first NaN of the list in the LATER block
    alive[forced] = True
    mi[forced] = NAN if placement == "two_nans" else E
    if placement == "nan_last_partial":
        at = 1023 * 256 + 77                      # block 1023: the last partial
        alive[at] = True
        mi[~alive] = NAN
        mi[at] = NAN
    elif placement == "all_dead":
        alive[:] = False
    else:
        mi[~alive] = NAN
    name = "n%d-mode%d-%s" % (n, mode, placement)
    return _finish(name, p, b, mi, rng.integers(0, ROWS, n), alive, off, gpos)


def two_stage(n, placement):
    """The case of one size (N_TWO_STAGE, or SMALL_MAX itself) and placement; modes and list numberings alternate."""
    j = PLACEMENTS.index(placement) + (N_TWO_STAGE + (SMALL_MAX,)).index(n)
    return two_stage_case(n, placement, j % 2, j)


# --------------------------------------------------------------------------------------- inputs: ital_select_resolve
WORLDS = (1, 2, 3, 8)
SCENARIOS = ("first", "middle", "last", "tie_low_pos_high_rank", "nan_vs_numbers", "two_nans", "some_empty", "all_empty_status",
             "status_or")
N_ALIVE = 12


def hand_record(val, lp, gidx, rank, loc, status, rng, dims):
    kmax, ldx, ldw = dims
    r = rng.standard_normal(H + ldx + ldw + kmax)
    r[:H] = [val, float(lp), float(gidx), r[3], abs(r[4]) + 0.5, abs(r[5]), float(rank), float(loc), float(status), 0.0]
    return r


def empty_record(status, dims):
    kmax, ldx, ldw = dims
    r = np.zeros(H + ldx + ldw + kmax)
    r[1], r[8] = -1.0, float(status)
    return r


def resolve_case(world, scenario, rank, i):
    """Hand-built records of `world` ranks seen from `rank` (its own alive flags).  None: the scenario needs more ranks."""
    rng = np.random.default_rng(9000 + 131 * world + 17 * SCENARIOS.index(scenario) + i)    # the same records for every rank
    lay = layout(i)
    lay["ldx"] = 16
    mode = i % 2
    p, b = _tables(lay, rng, 0, mode)
    dims = (lay["kmax"], lay["ldx"], lay["ldw"])
    sgn = 1.0 if mode == 0 else -1.0
    E = 5.0 * sgn
    val = rng.uniform(-1.0, 1.0, world)
    lp = 100 * np.arange(world) + rng.integers(0, 50, world)
    st = np.zeros(world, dtype=np.int64)
    empty = np.zeros(world, dtype=bool)
    if scenario in ("first", "middle", "last"):
        val[{"first": 0, "middle": world // 2, "last": world - 1}[scenario]] = E
    elif scenario in ("tie_low_pos_high_rank", "two_nans"):
        if world < 2:
            return None
        a, c = sorted(rng.choice(world, 2, replace=False))
        val[[a, c]] = E if scenario == "tie_low_pos_high_rank" else NAN
        lp[a], lp[c] = lp[c], lp[a]
    elif scenario == "nan_vs_numbers":
        val[rng.integers(world)] = NAN
        val[rng.integers(world)] = E              # may fall on the same rank: then the NaN replaced nothing but itself
        if np.isnan(val).sum() == 0:
            val[0] = NAN
    elif scenario == "some_empty":
        if world < 2:
            return None
        empty[0] = True
        empty[rng.random(world) < 0.4] = True
        empty[rng.integers(1, world)] = False
    elif scenario == "all_empty_status":
        empty[:] = True
        st[rng.integers(world)] = 4
    elif scenario == "status_or":
        st[:min(world, 2)] = [1, 4][:min(world, 2)]
    recs = []
    for w in range(world):
        recs.append(empty_record(st[w], dims) if empty[w] else
                    hand_record(val[w], lp[w], BIG_ROW * (i % 2) + int(rng.integers(0, 400)), w, int(rng.integers(N_ALIVE)), st[w],
                                rng, dims))
    recs.append(np.full(len(recs[0]), NAN))       # the guard row
    p.update(world=world, rank=rank)
    bufs = {k: b[k] for k in STATE if k != "alive"}
    bufs["alive"] = _guard(np.ones(N_ALIVE, dtype=np.uint8), S8)
    bufs["records"] = np.concatenate(recs)
    return Case("world%d-%s-rank%d-#%d" % (world, scenario, rank, i), p, bufs)


def resolve_cases(world):
    out = []
    for j, sc in enumerate(SCENARIOS):
        for rank in range(world):
            c = resolve_case(world, sc, rank, 3 * j + world)
            if c is not None:
                out.append(c)
    return out


def sequence_records(kmax, world, seed):
    """One record set per greedy step of a full batch: data indices in scrambled order (with one repeated index, so that the
    stability of the insertion shows), winners on varying ranks."""
    rng = np.random.default_rng(seed)
    dims = (kmax, 16, 8)
    gidx = rng.permutation(kmax) * 11 + 5
    gidx[-1] = gidx[0]
    steps = []
    for t in range(kmax):
        owner = int(rng.integers(world))
        recs = [hand_record(rng.uniform(-1, 1) + (5.0 if w == owner else 0.0), 10 * w + t, int(gidx[t]) if w == owner else 999,
                            w, (3 * t + w) % N_ALIVE, 0, rng, dims) for w in range(world)]
        steps.append(np.concatenate(recs + [np.full(len(recs[0]), NAN)]))
    return dims, steps


def empty_state(dims, rng=None):
    """A batch nobody has written yet: NaN and sentinels throughout, all flags alive, a clear status word."""
    kmax, ldx, ldw = dims
    ret = np.full(kmax + 1 + G, S64, dtype=np.int64)
    ret[kmax] = 0
    return dict(bidx=np.full(kmax + G, S64, dtype=np.int64), bgpos=np.full(kmax + G, S64, dtype=np.int64),
                bsort=np.full(kmax + G, S32, dtype=np.int32), bmu=np.full(kmax + G, NAN), sig=np.full(kmax * kmax + G, NAN),
                XB=np.full(kmax * ldx + G, NAN), XBn=np.full(kmax + G, NAN), VB=np.full(kmax * ldw + G, NAN),
                alive=_guard(np.ones(N_ALIVE, dtype=np.uint8), S8), ret=ret)
