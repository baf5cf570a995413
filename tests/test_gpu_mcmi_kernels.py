"""The MCMI kernels of ital_amd/csrc/mcmi.hip, one call each, against the extended-precision reference of tests/_mcmi_ref.py.

ital_cov_block (its three routes), ital_cov_abs_rowsum, ital_mcmi_score_step (single kernel, t <= 4, and split form, t = 5 .. 8)
and ital_gather_block are called through ctypes on buffers built on the host.  Every byte a call must not read or write holds
NaN (padding columns of out, cov and C, rows and columns >= t - 1 of sig, bmu and bgpos with kmax = 8, the row-sum work area;
the scorer's workspace holds 0xFF bytes); afterwards everything outside the write set is compared by its bits with what was
uploaded.  The results are judged by the a-priori bounds of _mcmi_ref.py (operation counts and the published accuracy of
MVNPHI; nothing is fitted): largest residual / bound <= 1.  The tests assert the route they mean to hit (ref.expected_route).
That a plain FP64 emulation passes the same bounds at the same shapes, and that the checker rejects the mistakes these kernels
can make, is tests/test_mcmi_ref_host.py.

Largest residual / bound observed (MI355X / FP64 NumPy emulation on the host), printed again by every run with -s:

    quantity                                            device   emulation
    ital_cov_block, small route                         0.15     0.23
    ital_cov_block, default route (every piece)         0.19     0.17
    ital_cov_block, LDS route (four corners)            0.098    0.12
    ital_cov_abs_rowsum                                 0.018    0.020
    ital_mcmi_score_step, t <= 4 (extended subset)      0.063    0.33
    ital_mcmi_score_step, t >= 5 (extended subset)      0.027    0.083
    ital_mcmi_score_step, NaN rule (t = 3, 6)           0.025    0.063
    the other candidates, device against emulation at twice the bound: 0.29 (t <= 4), 0.076 (t >= 5)

The default and LDS routes gave the bits of the small route on every piece compared.  The conditional-entropy bound is 4e-15 to
7e-14 of the value (it grows with t and with 1 / noise through W); the device stays within 0.063 of it, so it differs from
the exact value by a few 1e-16 relative where the learner tests allow 1e-8, and sits closer to the reference than the
NumPy emulation does (FMA chains, Hart's rational against ndtr).  No ratio above 1, so nothing to trace.

Findings from reading, not from a failing test.  ital_cov_block and ital_cov_abs_rowsum test `ldx % 16 != 0` only, so ldx = 0
is accepted: the register-tiled kernels then read no feature at all, the LDS-staged one would still stage Xa[0 .. 15] and
Xb[0 .. 15] once.  ital_gram_rows and ital_kernel_matvec refuse ldx <= 0, and no caller in the project passes it (gp.ldx >=
16).  The refusal belongs in mcmi.hip; that file and include/ital_hip.h are hashed into the source stamps of the committed MCMI
profiles (tools/stamp.py, units mcmi and mcmiall), which still match, so it waits for a change that voids them anyway -- these
tests found no wrong result that would be one.

Run: python -m pytest tests/test_gpu_mcmi_kernels.py -m gpu."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _mcmi_ref as ref  # noqa: E402

NAN = float("nan")
WORST = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for name, (d, e) in sorted(WORST.items()):
        print("%-44s largest residual/bound: device %.3g, emulation %.3g" % (name, d, e))


def _note(name, device, emulation=0.0):
    d, e = WORST.get(name, (0.0, 0.0))
    WORST[name] = (max(d, device), max(e, emulation))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _down(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b):
    return a.shape == b.shape and bool(np.array_equal(_bits(a), _bits(b)))


def _ld(v):
    """A leading dimension strictly greater than v that is no multiple of 16."""
    ld = v + 3
    while ld % 16 == 0:
        ld += 1
    return ld


def _guarded(a, dev, extra=2):
    """`a` followed by `extra` rows (entries) of NaN, on the host and on the device."""
    host = np.full((a.shape[0] + extra,) + a.shape[1:], NAN)
    host[:a.shape[0]] = a
    return host, _up(host, dev)


def _fresh(shape, dev):
    """A buffer of NaN, on the host and on the device."""
    host = np.full(shape, NAN)
    return host, _up(host, dev)


def _kept(before, after, written=None):
    """Everything outside the boolean mask `written` has the bits it was uploaded with."""
    keep = np.ones(before.shape, dtype=bool) if written is None else ~written
    return before.shape == after.shape and bool(np.array_equal(_bits(before)[keep], _bits(after)[keep]))


def _mask(shape, *index):
    w = np.zeros(shape, dtype=bool)
    w[index] = True
    return w


def _id(case):
    return "-".join(str(v) for v in case)


def _lib():
    from ital_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ ital_cov_block
class _CovBuffers:
    """The inputs of one shape on the device.  V: one [m + 1][wide] array with Va at column offset 3 and Vb behind it at an odd
    offset, NaN everywhere else (the several-rank call of MCMI_min._steps passes windows of one wider V with its row stride)."""

    def __init__(self, s, dev):
        self.s = s
        self.Xa0, self.Xa = _guarded(s.Xa, dev)
        self.Xb0, self.Xb = _guarded(s.Xb, dev)
        self.an0, self.an = _guarded(s.an, dev)
        self.bn0, self.bn = _guarded(s.bn, dev)
        self.offa = 3
        self.offb = (3 + s.na + 2) | 1
        self.wide = self.offb + s.nb + 2
        self.V0 = np.full((s.m + 1, self.wide), NAN)
        self.V0[:s.m, self.offa:self.offa + s.na] = s.Va
        self.V0[:s.m, self.offb:self.offb + s.nb] = s.Vb
        self.V = _up(self.V0, dev)

    def call(self, dev, rows=None, cols=None):
        """ital_cov_block on the sub-block rows x cols (the whole block by default).  Returns out[na'][nb'] after the padding of
        the output has been compared by bits."""
        s = self.s
        i0, i1 = rows or (0, s.na)
        j0, j1 = cols or (0, s.nb)
        na, nb = i1 - i0, j1 - j0
        ldo = _ld(nb)
        out0, out = _fresh((na + 1, ldo), dev)
        va = self.V.data_ptr() + 8 * (self.offa + i0) if s.m else None
        vb = self.V.data_ptr() + 8 * (self.offb + j0) if s.m else None
        lib = _lib()
        lib.check(lib.lib().ital_cov_block(self.Xa.data_ptr() + 8 * i0 * s.ldx, self.an.data_ptr() + 8 * i0, na,
                                           self.Xb.data_ptr() + 8 * j0 * s.ldx, self.bn.data_ptr() + 8 * j0, nb, s.ldx, va,
                                           self.wide, vb, self.wide, s.m, float(s.var), float(s.ls), out.data_ptr(), ldo, _stream()))
        got = _down(out)
        assert _kept(out0, got, _mask(got.shape, slice(0, na), slice(0, nb))) and np.isfinite(got[:na, :nb]).all(), (na, nb)
        return np.ascontiguousarray(got[:na, :nb])

    def untouched(self):
        return _same(self.Xa0, _down(self.Xa)) and _same(self.Xb0, _down(self.Xb)) and _same(self.an0, _down(self.an)) and \
            _same(self.bn0, _down(self.bn)) and _same(self.V0, _down(self.V))

    def ratios(self, out, rows=None, cols=None):
        s = self.s
        i0, i1 = rows or (0, s.na)
        j0, j1 = cols or (0, s.nb)
        args = (s.Xa[i0:i1], s.an[i0:i1], s.Xb[j0:j1], s.bn[j0:j1], s.Va[:, i0:i1], s.Vb[:, j0:j1], s.m, s.var, s.ls)
        return ref.cov_block_check(out, *args), ref.cov_block_check(ref.emu_cov_block(*args), *args)


@pytest.mark.parametrize("case", ref.SMALL_CASES, ids=_id)
def test_cov_block_small_route_against_the_extended_reference(dev, case):
    """Every call passes Va and Vb as windows at odd column offsets of one wider V, ldva = ldvb = its row stride."""
    assert ref.expected_route(case[0], case[1]) == "small"
    b = _CovBuffers(ref.cov_inputs(*case), dev)
    out = b.call(dev)
    assert b.untouched()
    d, e = b.ratios(out)
    _note("ital_cov_block, small route", d, e)
    print(case, "device %.3g emulation %.3g" % (d, e))
    assert d <= 1.0, (case, d)


@pytest.mark.parametrize("case", ref.DEFAULT_CASES + ref.LDS_CASES, ids=_id)
def test_cov_block_default_and_lds_routes_have_the_bits_of_the_small_route(dev, case):
    """The block of one call through the default 32 x 64 tile (or the LDS-staged kernel) against the same block from small-route
    calls on sub-blocks of at most 128 x 2048: every piece of the tiling for the default route, the four corners for the LDS
    route -- (1, 130945): every staged row clamps to row 0; (129, 65409): a ragged second tile row.  `The same bits whichever
    tile` is the claim of mcmi.hip.  The checked pieces are judged in the extended type as well."""
    na, nb = case[0], case[1]
    route = ref.expected_route(na, nb)
    assert route == ("default" if case in ref.DEFAULT_CASES else "lds")
    b = _CovBuffers(ref.cov_inputs(*case), dev)
    full = b.call(dev)
    checked = ref.checked_pieces(na, nb)
    for piece in (ref.pieces(na, nb) if route == "default" else checked):
        i0, i1, j0, j1 = piece
        assert ref.expected_route(i1 - i0, j1 - j0) == "small"
        sub = b.call(dev, (i0, i1), (j0, j1))
        assert _same(sub, np.ascontiguousarray(full[i0:i1, j0:j1])), (case, piece)
        if piece in checked:
            d, e = b.ratios(sub, (i0, i1), (j0, j1))
            _note("ital_cov_block, %s route" % route, d, e)
            print(case, piece, "device %.3g emulation %.3g" % (d, e))
            assert d <= 1.0, (case, piece, d)
    assert b.untouched()


# ------------------------------------------------------------------------------------------------ ital_cov_abs_rowsum
@pytest.mark.parametrize("shape", ref.ROWSUM_SHAPES, ids=_id)
def test_cov_abs_rowsum_against_the_extended_reference(dev, shape):
    na, nb, ldx, m = shape
    b = _CovBuffers(ref.cov_inputs(*shape), dev)
    s = b.s
    lib = _lib()
    prior = np.linspace(0.5, 2.5, na)
    va, vb = b.V.data_ptr() + 8 * b.offa, b.V.data_ptr() + 8 * b.offb

    def call(nb_, mult, accumulate):
        out0, out = _guarded(prior, dev)
        work0, work = _guarded(np.full(mult * na, NAN), dev)
        lib.check(lib.lib().ital_cov_abs_rowsum(b.Xa.data_ptr(), b.an.data_ptr(), na, b.Xb.data_ptr(), b.bn.data_ptr(), nb_, ldx, va,
                                                b.wide, vb, b.wide, m, float(s.var), float(s.ls), work.data_ptr(), mult * na,
                                                accumulate, out.data_ptr(), _stream()))
        got, w = _down(out), _down(work)
        assert _kept(out0, got, _mask(got.shape, slice(0, na))), (shape, nb_, mult, accumulate)
        assert _kept(work0, w, _mask(w.shape, slice(0, mult * na))), (shape, nb_, mult, accumulate)
        return got[:na]

    for mult in ref.ROWSUM_WORK:
        nsplit, ntile = ref.expected_nsplit(na, nb, mult * na)
        for accumulate in (0, 1):
            got = call(nb, mult, accumulate)
            args = (s.Xa, s.an, s.Xb, s.bn, s.Va, s.Vb, m, s.var, s.ls, nsplit)
            before = prior if accumulate else np.zeros(na)
            d = ref.rowsum_check(got, before, *args)
            e = ref.rowsum_check(ref.emu_rowsum(prior, accumulate, *args), before, *args)
            _note("ital_cov_abs_rowsum", d, e)
            print(shape, "nsplit %d of %d tiles, accumulate %d: device %.3g emulation %.3g" % (nsplit, ntile, accumulate, d, e))
            assert d <= 1.0, (shape, mult, accumulate, d)
    assert _same(call(0, 1, 0), np.zeros(na)) and _same(call(0, 1, 1), prior)
    assert b.untouched()


# ------------------------------------------------------------------------------------------------ ital_mcmi_score_step
KMAX = 8


def _score(dev, inp, work=None, spare=3, short=0):
    """One ital_mcmi_score_step on padded, NaN-guarded copies of the arrays of `inp`.  Returns (status, ce[n_i], workspace).
    The workspace (t >= 5) is downloaded before and after the call: a call that ran may have written its first
    ital_mcmi_workspace(t, n_i) doubles and nothing behind them, a refused call nothing at all (a fresh workspace holds 0xFF
    bytes, a used one whatever the call before left)."""
    lib = _lib()
    t, n_i, n = inp.t, inp.n_i, inp.n_all
    ld_cov, ldc = _ld(n), _ld(n + 5)
    host = {}
    host["mu"], host["s2"] = np.full(n + 2, NAN), np.full(n + 2, NAN)
    host["mu"][:n], host["s2"][:n] = inp.mu, inp.s2
    host["cov"] = np.full((n_i + 1, ld_cov), NAN)
    host["cov"][:n_i, :n] = inp.cov
    host["C"] = np.full((KMAX, ldc), NAN)
    host["C"][:t - 1, :n] = inp.C
    host["sig"] = np.full((KMAX, KMAX), NAN)
    host["sig"][:t - 1, :t - 1] = inp.sig
    host["bmu"] = np.full(KMAX, NAN)
    host["bmu"][:t - 1] = inp.bmu
    host["bgpos"] = np.full(KMAX, NAN).view(np.int64).copy()
    host["bgpos"][:t - 1] = inp.bgpos
    host["alive"] = np.full(n_i + 8, 1, dtype=np.uint8)
    host["alive"][:n_i] = inp.alive
    host["ce"] = np.full(n_i + 2, NAN)
    host["ce"][:n_i] = ref.CANARY
    d = {k: _up(v, dev) for k, v in host.items()}
    desc = lib.ItalMcmiDesc()
    desc.t, desc.n_i, desc.pos_offset, desc.n_all = t, n_i, inp.pos_offset, n
    desc.alive, desc.mu, desc.s2 = d["alive"].data_ptr(), d["mu"].data_ptr(), d["s2"].data_ptr()
    desc.cov, desc.ld_cov, desc.C, desc.ldc = d["cov"].data_ptr(), ld_cov, d["C"].data_ptr(), ldc
    desc.batch.kmax = KMAX
    desc.batch.bmu, desc.batch.sig, desc.batch.bgpos = d["bmu"].data_ptr(), d["sig"].data_ptr(), d["bgpos"].data_ptr()
    desc.noise, desc.eps, desc.ce = float(inp.noise), float(inp.eps), d["ce"].data_ptr()
    need = int(lib.lib().ital_mcmi_workspace(t, n_i))
    assert (need > 0) == (t >= 5)
    if t >= 5 and work is None:
        work = torch.full((8 * (need + spare),), 0xFF, dtype=torch.uint8, device=dev).view(torch.float64)
    if t >= 5 and work is not False:
        desc.work, desc.work_doubles = work.data_ptr(), (need - short if short else work.numel())
    work_before = _down(work.view(torch.int64)) if t >= 5 and work is not False else None
    status = lib.lib().ital_mcmi_score_step(ctypes.byref(desc), _stream())
    ce = _down(d["ce"])
    if work_before is not None:
        work_after = _down(work.view(torch.int64))
        assert len(work_after) > need and np.array_equal(work_before[need if status == 0 else 0:],
                                                          work_after[need if status == 0 else 0:]), (t, n_i, status)
    for k, v in host.items():
        if k != "ce":
            assert _same(v, _down(d[k])), k
    assert _kept(host["ce"], ce, _mask(ce.shape, slice(0, n_i)))
    return status, ce[:n_i], work


def _judge(dev, inp, name):
    status, ce, _ = _score(dev, inp)
    assert status == 0
    emu = ref.emu_ce(inp)
    sub = ref.subset(inp, ref.ce_subset_size(inp.t))
    full = ref.ce_ref_cached(inp.t, inp.n_all, inp.noise, inp.n_i, inp.pos_offset)
    d, e = ref.ce_check(ce, inp, sub, full), ref.ce_check(emu, inp, sub, full)
    rest = ref.ce_check_against_emulation(ce, emu, inp, sub)
    _note(name, d, e)
    _note(name + ", others against the emulation", rest)
    print((inp.t, inp.n_all, inp.noise, inp.n_i, inp.pos_offset), "device %.3g emulation %.3g, others %.3g" % (d, e, rest))
    assert d <= 1.0 and rest <= 1.0, (inp.t, inp.n_all, inp.noise, inp.n_i, inp.pos_offset, d, rest)


@pytest.mark.parametrize("case", ref.CE_CASES, ids=_id)
def test_mcmi_score_step_against_the_extended_reference(dev, case):
    """The three slices of the case: the whole block, the last five at pos_offset = n_all - 5, one in the middle.  Members lie in
    the first, a middle and the last stride of the j loop and are dead where the slice holds them, one more candidate is dead
    without being a member; kmax = 8 > t, ld_cov != ldc > n_all.  The extended check looks at 6 (t <= 4) or 3 scored candidates,
    the others are held to the FP64 emulation at twice the bound.  That the minimising patterns of the t >= 5 subsets fall in
    the first, a middle and the last group of 8 is asserted from the reference in tests/test_mcmi_ref_host.py (no device call)."""
    t, n_all, noise = case
    for n_i, pos_offset in ref.slices(t, n_all):
        _judge(dev, ref.ce_inputs(t, n_all, noise, n_i, pos_offset), "ital_mcmi_score_step, t %s" % ("<= 4" if t <= 4 else ">= 5"))


@pytest.mark.parametrize("t", [3, 6])
def test_mcmi_score_step_is_nan_exactly_where_the_reference_says(dev, t):
    """One case per form.  Block entry j* has s2 = 2e-6 and a covariance of 0.5 with every second scored candidate: in the
    reference s'_{j*} <= -1e-6 there and >= +1e-6 for the others."""
    inp = ref.nan_inputs(t)
    full = ref.ce_ref(inp)
    due = sorted(li for li, (val, _, _) in full.items() if val is None)
    lo, hi = ref.sprime_at_jstar(inp)
    assert due == sorted(inp.hit) and max(lo) <= -1e-6 and min(hi) >= 1e-6
    status, ce, _ = _score(dev, inp)
    assert status == 0 and sorted(np.nonzero(np.isnan(ce))[0].tolist()) == due
    d = ref.ce_check(ce, inp, ref=full)
    _note("ital_mcmi_score_step, NaN rule", d, ref.ce_check(ref.emu_ce(inp), inp, ref=full))
    assert d <= 1.0, d


@pytest.mark.parametrize("t", [5, 8])
def test_mcmi_split_form_on_a_used_workspace(dev, t):
    """A workspace of 0xFF bytes, larger than needed, serves a call over the whole block; a second call with n_i = 5 on the same
    workspace then gives the bits of that call on a fresh one.  No workspace, or one a double short, is refused with -22 and
    leaves ce and the whole workspace as they were.  (_score compares the workspace behind the call's share by bits.)"""
    lib = _lib()
    big = ref.ce_inputs(t, 65, 1e-6, 65, 0)
    small = ref.ce_inputs(t, 65, 1e-6, 5, 60)
    status, _, work = _score(dev, big, spare=100)
    assert status == 0
    status, used, _ = _score(dev, small, work=work)
    assert status == 0
    status, fresh, _ = _score(dev, small)
    assert status == 0 and np.isfinite(fresh[small.alive[:5] == 1]).all() and _same(used, fresh)
    for kwargs in (dict(work=False), dict(short=1)):
        status, ce, _ = _score(dev, small, **kwargs)
        assert status == -22 and b"workspace" in lib.lib().ital_last_error()
        assert _same(ce, np.full(5, ref.CANARY))


# ------------------------------------------------------------------------------------------------ ital_gather_block
def test_gather_block_windows_repeats_and_padding(dev):
    """On top of test_gather_block_equals_indexing: m = 0 with null V and Vc; ldc > nc with the NaN padding kept; an index that
    appears twice; row windows that own none and all of the list."""
    lib = _lib()
    rng = np.random.default_rng(77)
    n, ldx, m = 40, 16, 3
    X, xn, mu, s2 = rng.random((n, ldx)), rng.random(n), rng.standard_normal(n), rng.random(n)
    V = rng.standard_normal((m, n + 4))
    cand = np.array([5, 39, 0, 17, 5, 22, 38], dtype=np.int64)
    nc, ldc = len(cand), len(cand) + 4
    dX, dxn, dmu, ds2, dV, dcand = (_up(a, dev) for a in (X, xn, mu, s2, V, cand))

    def call(row0, n_rows, m_):
        fresh = [_fresh(shape, dev) for shape in ((nc + 1, ldx), (m + 1, ldc), (nc + 1,), (nc + 1,), (nc + 1,))]
        Xc, Vc, xnc, muc, s2c = outs = [f[1] for f in fresh]
        # the rank's arrays start at its first row: row0 of the data is local row 0
        lib.check(lib.lib().ital_gather_block(dcand.data_ptr(), nc, row0, n_rows, dX.data_ptr() + 8 * ldx * min(row0, n - 1),
                                              dxn.data_ptr() + 8 * min(row0, n - 1), ldx,
                                              dV.data_ptr() + 8 * min(row0, n - 1) if m_ else None, n + 4, m_,
                                              dmu.data_ptr() + 8 * min(row0, n - 1), ds2.data_ptr() + 8 * min(row0, n - 1),
                                              Xc.data_ptr(), Vc.data_ptr() if m_ else None, ldc, xnc.data_ptr(), muc.data_ptr(),
                                              s2c.data_ptr(), _stream()))
        got = [_down(o) for o in outs]
        written = [_mask(got[0].shape, slice(0, nc)), _mask(got[1].shape, slice(0, m_), slice(0, nc))] + \
                  [_mask(got[2].shape, slice(0, nc))] * 3
        assert all(_kept(f[0], g, w) for f, g, w in zip(fresh, got, written)), (row0, n_rows, m_)
        return got

    for row0, n_rows, m_ in ((0, n, m), (0, n, 0), (n, 0, m), (10, 20, m)):
        Xc, Vc, xnc, muc, s2c = call(row0, n_rows, m_)
        own = (cand >= row0) & (cand < row0 + n_rows)
        assert _same(Xc[:nc], np.where(own[:, None], X[cand], 0.0))
        for got, src in ((xnc, xn), (muc, mu), (s2c, s2)):
            assert _same(got[:nc], np.where(own, src[cand], 0.0))
        if m_:
            assert _same(Vc[:m, :nc], np.where(own[None, :], V[:, cand], 0.0))
    for a, t_ in ((X, dX), (xn, dxn), (mu, dmu), (s2, ds2), (V, dV), (cand, dcand)):
        assert _same(a, _down(t_))
