"""Device buffers of one greedy batch construction (the replicated batch state of include/ital_hip.h `ital_batch`,
the per-member covariance columns, the selection record and its gather target), and the launches every greedy loop of
the package shares: the selection of a step (`select_step`), the new member's covariance column (`member_column`), the
lattice tables and workspace of the scorers, the common fields of `ItalScoreDesc`."""
import collections

import torch

from . import mvn_stream, sharding
from ._lib import ITAL_JUMP_BITS, ItalBatch, check, lib as _lib, rows_fn
from .device_data import DTYPE_CODES

LABEL_MODES = {"mean": 0, "optimistic": 1, "pessimistic": 2}
FUSED_LAUNCH_MAX = 1 << 18   # one rank, up to this many candidates: ital_select_fused (one workgroup) as the separate selection launch

# what a selection ranks: scores, local rows / block positions, alive flags of `n` candidates whose list positions are
# gpos[q] (or pos_offset + q); row_offset: data index of local row 0
Scored = collections.namedtuple("Scored", "scores cand alive n pos_offset gpos row_offset")
# where the winner's record and a member's covariance column are read: the GP's arrays or a gathered candidate block
Model = collections.namedtuple("Model", "mu s2 X xnorm n ldx V ldv m cap")


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def make_batch_buffers(device, kmax, ldx, cap, ldc, world):
    """kmax: batch capacity; ldx: padded feature dimension; cap: labelled-set capacity (leading dimension of the
    whitened columns); ldc: length of one covariance column; world: number of ranks exchanging records."""
    kmax = max(int(kmax), 4)
    f64, i64, i32 = torch.float64, torch.int64, torch.int32
    b = dict(kmax=kmax, ldw=cap, ldc=ldc, ldx=ldx)
    b["bidx"] = torch.zeros(kmax, dtype=i64, device=device)
    b["bgpos"] = torch.zeros(kmax, dtype=i64, device=device)
    b["bsort"] = torch.zeros(kmax, dtype=i32, device=device)
    b["bmu"] = torch.zeros(kmax, dtype=f64, device=device)
    b["sig"] = torch.zeros(kmax * kmax, dtype=f64, device=device)
    b["XB"] = torch.zeros((kmax, ldx), dtype=f64, device=device)
    b["XBn"] = torch.zeros(kmax, dtype=f64, device=device)
    b["VB"] = torch.zeros((kmax, cap), dtype=f64, device=device)
    b["C"] = torch.zeros((kmax, ldc), dtype=f64, device=device)
    b["ret"] = torch.zeros(kmax + 1, dtype=i64, device=device)   # last slot: copy of the status word (one download)
    b["work"] = torch.zeros(3 * 1024, dtype=f64, device=device)
    rec_len = int(_lib().ital_record_len(ldx, cap, kmax))      # = ITAL_REC_HEADER + ldx + cap + kmax
    b["rec_len"] = rec_len
    b["rec"] = torch.zeros(rec_len, dtype=f64, device=device)
    b["rec_all"] = torch.zeros((world, rec_len), dtype=f64, device=device)
    b["jump"] = {}
    b["jumppat"] = {}
    b["vk"] = {}
    b["batch"] = ItalBatch(kmax, ldx, cap, _ptr(b["bidx"]), _ptr(b["bgpos"]), _ptr(b["bsort"]), _ptr(b["bmu"]),
                           _ptr(b["sig"]), _ptr(b["XB"]), _ptr(b["XBn"]), _ptr(b["VB"]))
    return b


def gp_model(gp):
    return Model(gp.mu, gp.s2, gp.Xd, gp.xnorm, gp.n, gp.ldx, gp.V, gp.ldv, gp.m, gp.cap)


def select_step(gp, b, scored, model, slot, st, *, argmin=0, fused=False, local=True, resolve=True, mark=None):
    """Selection of one greedy step: arg-extreme of the scores + the winner's record, the exchange of the ranks' records,
    the winner into batch state `slot` -- `fused`: one launch for one rank (ital_select_fused); otherwise ital_select_local
    (`local` False: the scoring launch has left the record), the all-gather over `gp.group` and ital_select_resolve
    (`resolve` False: the caller resolves on the host; `slot` then only counts the members the record is correlated with).
    `mark`: the learner's profile hook for the exchange.  Returns the records the resolve step read (None when fused)."""
    lib = _lib()
    s, m = scored, model
    head = (_ptr(s.scores), _ptr(s.cand), _ptr(s.alive), s.n, s.pos_offset, _ptr(s.gpos), s.row_offset, gp.rank, argmin,
            _ptr(m.mu), _ptr(m.s2), _ptr(m.X), _ptr(m.xnorm), m.ldx, _ptr(m.V), m.ldv, m.m, m.cap, _ptr(b["C"]), m.ldv, slot)
    xtype = DTYPE_CODES[m.X.dtype]       # the model's rows: FP64, or views of a compact store (the record is FP64 either way)
    if fused:
        check(rows_fn("ital_select_fused", xtype)(*head, slot, b["batch"], _ptr(gp.status), _ptr(b["rec"]), _ptr(b["ret"]), st))
        return None
    if local:
        check(rows_fn("ital_select_local", xtype)(*head, b["kmax"], _ptr(gp.status), _ptr(b["work"]), _ptr(b["rec"]), st))
    recs = b["rec"]
    if gp.collective:
        ev0 = mark() if mark else None
        recs = sharding.gather_records(b["rec"], b["rec_all"], gp.group)
        if mark:
            mark("exchange", slot + 1, gp.world, ev0)
    if resolve:
        check(lib.ital_select_resolve(_ptr(recs), gp.world, b["rec_len"], gp.rank, argmin, slot, b["batch"], _ptr(s.alive),
                                      _ptr(b["ret"]), st))
    return recs


def member_column(learner, model, b, slot, st, member=None):
    """Posterior covariance of batch member `slot` with every row of `model` into b["C"][slot] (ital_cross_cov_cols).
    `member`: its (feature row, squared norm, whitened column) when they are not the batch state's own."""
    x, xn, v = member if member is not None else (b["XB"][slot], b["XBn"][slot:], b["VB"][slot])
    m = model
    check(rows_fn("ital_cross_cov_cols", DTYPE_CODES[m.X.dtype])(
        _ptr(m.X), _ptr(m.xnorm), m.n, m.ldx, _ptr(x), _ptr(xn), 1, _ptr(v), m.cap, _ptr(m.V), m.ldv, m.m, float(learner.var),
        float(learner.length_scale), _ptr(b["C"][slot]), m.ldv, st))


def lattice_tables(b, t, dev):
    """Jump, jump-pattern and Korobov tables of the lattice rule for t variables (device tensors, made once per buffer set)."""
    if t not in b["jump"]:
        b["jump"][t] = torch.from_numpy(mvn_stream.jump_table(t, ITAL_JUMP_BITS)).to(dev)
        b["jumppat"][t] = torch.from_numpy(mvn_stream.jump_pattern_table(t)).to(dev)
        b["vk"][t] = torch.from_numpy(mvn_stream.korobov_vk(t)).to(dev)
    return b["jump"][t], b["jumppat"][t], b["vk"][t]


def qmc_work(b, want, dev):
    """The scorers' workspace b["qmc_work"], grown to `want` doubles."""
    w = b.get("qmc_work")
    if w is None or w.numel() < want:
        b["qmc_work"] = w = torch.empty(want, dtype=torch.float64, device=dev)
    return w


def ensure_step_buffers(b, n_loc, sel_doubles, dev):
    """Buffers of `b` that the fast paths' steps share: alive flags and scores of n_loc candidates (b["alive"], b["mi"]) and,
    for steps that end with their selection, sel_doubles doubles of block partials with their counter (b["sel_parts"],
    b["sel_counter"]).  They grow, never shrink; True when one was replaced (what pointed into it is stale)."""
    grown = False
    n = max(n_loc, 1)
    if b.get("alive") is None or b["alive"].numel() < n:
        b["alive"] = torch.empty(n, dtype=torch.uint8, device=dev)
        b["mi"] = torch.empty(n, dtype=torch.float64, device=dev)
        grown = True
    if sel_doubles and (b.get("sel_parts") is None or b["sel_parts"].numel() < sel_doubles):
        b["sel_parts"] = torch.empty(sel_doubles, dtype=torch.float64, device=dev)
        b["sel_counter"] = torch.zeros(1, dtype=torch.int32, device=dev)
        grown = True
    return grown


def lattice_label(work, t, n_loc):
    """Profile label of the lattice sums of step t over n_loc candidates: they run in as many slabs as workspace `work`
    needs to hold the prepared calls of all of them."""
    slabs = -(-n_loc // max(work.numel() // int(_lib().ital_score_workspace(t, 1)), 1))
    return "qmc_main" if slabs == 1 else "qmc_slabs%d" % slabs


def fill_score_desc(d, gp, b, scored, user):
    """Fields of ital_score_desc that every fast-path step fills alike.  user: (noise, eps, label mode)."""
    s = scored
    d.n_cand = s.n
    d.cand, d.alive, d.mu, d.s2 = _ptr(s.cand), _ptr(s.alive), _ptr(gp.mu), _ptr(gp.s2)
    d.C, d.ldc = _ptr(b["C"]), gp.ldv
    d.row_offset, d.pos_offset, d.gpos = s.row_offset, s.pos_offset, _ptr(s.gpos)
    d.batch = b["batch"]
    d.noise, d.eps, d.label_mode = user
    d.mi, d.status = _ptr(s.scores), _ptr(gp.status)


def fill_score_select(d, gp, b, m, ret):
    """Fields of ital_score_desc for the selection at the end of the scoring launch (m labelled samples; ret: None when
    exchange and resolve follow as launches of their own)."""
    d.sel_X, d.sel_xnorm, d.sel_ldx = _ptr(gp.Xd), _ptr(gp.xnorm), gp.ldx
    d.sel_V, d.sel_ldv, d.sel_m, d.sel_ldw, d.sel_rank = _ptr(gp.V), gp.ldv, m, gp.cap, gp.rank
    d.sel_record, d.sel_ret = _ptr(b["rec"]), _ptr(ret)
    parts = b["sel_parts"]
    d.sel_parts, d.sel_parts_len, d.sel_counter = _ptr(parts), parts.numel(), _ptr(b["sel_counter"])
