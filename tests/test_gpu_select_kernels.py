"""The selection kernels of ital_amd/csrc/select.hip and select_common.h, one call each, against the exact host model of
tests/_select_ref.py.

ital_select_local (single-workgroup route and two-stage route), ital_select_fused and ital_select_resolve are called through
ctypes on buffers built on the host.  Every byte a call must not read holds NaN (doubles) or a sentinel (integers), every buffer
a call writes is pre-filled with them, and every buffer carries guard entries behind its last valid element.  After the call ALL
buffers are downloaded: the write set must hold the model's bits, everything else the bits that were uploaded
(ref.first_difference names the first buffer and index that does not).  The selection does no arithmetic: every comparison in
this file is equality of bits.  The `work` scratch of ital_select_local is excluded (tests/_select_ref.py says so once); its
guard is still checked.  The tests assert the route they mean to hit by the number of launches (ital_launch_count).

Calls per entry point: ital_select_local 819 (792 on the single-workgroup route: 12 sizes x 2 modes x 11 score patterns x 3 list
numberings; 18 on the two-stage route, 4 at the threshold with 4 one position above it, 1 with FP32 rows), ital_select_fused 810
(the same 792 and 18 inputs), ital_select_resolve 158 (123 hand-built record sets of 1, 2, 3 and 8 ranks, 35 steps of two full
sequences).  On an MI355X every one of them left the model's bits: no finding, the kernels are unchanged.  Noted from reading
only: ital_select_resolve does not refuse a mode outside 0 / 1 as ital_select_local and ital_select_fused do (it would act as
arg-min); no caller passes one, and the refusal test below asks for what the header promises, no more.

That a NumPy emulation of these kernels passes the same checker on the same inputs, and that the checker rejects the mistakes
such kernels can make, is tests/test_select_ref_host.py.

Run: python -m pytest tests/test_gpu_select_kernels.py -m gpu."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _select_ref as ref  # noqa: E402

LOCAL = ("mi", "cand", "alive", "gpos", "mu", "s2", "X", "xnorm", "V", "C", "status", "work", "record")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


def _L():
    from ital_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _up(bufs, dev, names=None):
    return {k: torch.from_numpy(v).to(dev) for k, v in bufs.items() if v is not None and (names is None or k in names)}


def _down(d):
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in d.items()}


def _p(d, name):
    t = d.get(name)
    return None if t is None else t.data_ptr()


def _batch(case, d):
    L = _L()
    kmax, ldx, ldw = case.dims()
    return L.ItalBatch(kmax, ldx, ldw, *[_p(d, k) for k in ("bidx", "bgpos", "bsort", "bmu", "sig", "XB", "XBn", "VB")])


def _launches(fn):
    lib = _L().lib()
    before = int(lib.ital_launch_count())
    rc = fn()
    return rc, int(lib.ital_launch_count()) - before


def _local_args(case, d):
    p = case.p
    return (_p(d, "mi"), _p(d, "cand"), _p(d, "alive"), p["n_cand"], p["pos_offset"], _p(d, "gpos"), p["row_offset"], p["rank"],
            p["mode"], _p(d, "mu"), _p(d, "s2"), _p(d, "X"), _p(d, "xnorm"), p["ldx"], _p(d, "V"), p["ldv"], p["m"], p["ldw"],
            _p(d, "C"), p["ldc"], p["nprev"])


def call_local(case, dev, xtype=None):
    """ital_select_local on the case's buffers -> (every buffer afterwards, launches)."""
    L = _L()
    d = _up(case.bufs, dev, LOCAL)
    tail = (case.p["kmax"], None if case.p["status_null"] else _p(d, "status"), _p(d, "work"), _p(d, "record"))
    if xtype is None:
        rc, launches = _launches(lambda: L.lib().ital_select_local(*_local_args(case, d), *tail, _stream()))
    else:
        rc, launches = _launches(lambda: L.lib().ital_select_local_t(*_local_args(case, d), *tail, xtype, _stream()))
    L.check(rc)
    return _down(d), launches


def call_fused(case, dev):
    """ital_select_fused on the case's buffers -> (every buffer afterwards, launches)."""
    L = _L()
    d = _up(case.bufs, dev)
    rc, launches = _launches(lambda: L.lib().ital_select_fused(
        *_local_args(case, d), case.p["slot"], _batch(case, d), None if case.p["status_null"] else _p(d, "status"), _p(d, "record"),
        _p(d, "ret"), _stream()))
    L.check(rc)
    return _down(d), launches


def call_resolve(case, dev):
    L = _L()
    d = _up(case.bufs, dev)
    p = case.p
    rc, launches = _launches(lambda: L.lib().ital_select_resolve(_p(d, "records"), p["world"], case.rec_len(), p["rank"], p["mode"],
                                                                 p["slot"], _batch(case, d), _p(d, "alive"), _p(d, "ret"), _stream()))
    L.check(rc)
    return _down(d), launches


def _only(expected, names):
    return {k: v for k, v in expected.items() if k in names}


def _work_guard_kept(case, after):
    return bool(np.isnan(after["work"][3 * 1024:]).all())


# ------------------------------------------------------------------------------------- the single-workgroup route
SMALL = [(n, mode) for n in ref.N_SMALL for mode in (0, 1)]


@pytest.mark.parametrize("n,mode", SMALL)
def test_select_local_single_workgroup_equals_the_model(dev, n, mode):
    """Every score pattern with pos_offset 0, pos_offset 2^40 + 3 and a permuted gpos; row_offset, m, nprev, ldx, kmax and the
    status word cycle through their values (ref.layout)."""
    for case in ref.small_cases(n, mode):
        after, launches = call_local(case, dev)
        assert launches == 1, case
        diff = ref.first_difference(_only(ref.expect_local(case), LOCAL), after)
        assert diff is None, (case, diff)
        assert _work_guard_kept(case, after), case


@pytest.mark.parametrize("n,mode", SMALL)
def test_select_fused_equals_the_model(dev, n, mode):
    """The record, the batch state (slot 0, 1 and kmax - 1 of a pre-filled batch), the alive flags and ret with its status word."""
    for case in ref.small_cases(n, mode):
        after, launches = call_fused(case, dev)
        assert launches == 1, case
        diff = ref.first_difference(ref.expect_fused(case), after)
        assert diff is None, (case, diff)


# -------------------------------------------------------------------------------------------- the two-stage route
TWO = [(n, pl) for n in ref.N_TWO_STAGE for pl in ref.PLACEMENTS]


@pytest.mark.parametrize("n,placement", TWO)
def test_select_local_two_stage_equals_the_model_and_the_fused_call(dev, n, placement):
    case = ref.two_stage(n, placement)
    want = ref.expect_local(case)
    after, launches = call_local(case, dev)
    assert launches == 2, case                                  # select_partial_kernel, select_record_kernel
    diff = ref.first_difference(_only(want, LOCAL), after)
    assert diff is None, (case, diff)
    assert _work_guard_kept(case, after), case
    fused, launches = call_fused(case, dev)                     # no size switch in there: one workgroup whatever n_cand is
    assert launches == 1
    diff = ref.first_difference({"record": after["record"]}, fused)
    assert diff is None, (case, diff)
    diff = ref.first_difference(ref.expect_fused(case), fused)
    assert diff is None, (case, diff)


@pytest.mark.parametrize("placement", ["second_trip", "last", "equal_two_blocks", "two_nans"])
def test_select_local_at_the_threshold_takes_the_single_workgroup(dev, placement):
    """n_cand = 1 << 18 exactly: one launch, and the record the two-stage route gives one candidate later (a dead one)."""
    case = ref.two_stage(ref.SMALL_MAX, placement)
    after, launches = call_local(case, dev)
    assert launches == 1
    diff = ref.first_difference(_only(ref.expect_local(case), LOCAL), after)
    assert diff is None, (case, diff)
    # the same list with one dead position appended goes through the two-stage route and has to leave the same record
    n = case.p["n_cand"]
    more = ref.Case(case.name + "+1", dict(case.p, n_cand=n + 1), dict(case.bufs))
    for k, fill in (("mi", np.inf if case.p["mode"] == 0 else -np.inf), ("alive", 0), ("cand", 0), ("gpos", ref.S64)):
        if case.bufs[k] is not None:
            b = np.concatenate([case.bufs[k][:n], np.array([fill], dtype=case.bufs[k].dtype), case.bufs[k][n:]])
            more.bufs[k] = b
    after2, launches = call_local(more, dev)
    assert launches == 2
    assert ref.first_difference({"record": after["record"]}, after2) is None


def test_select_local_two_stage_reads_fp32_rows(dev):
    """ital_select_local_t on the two-stage route: the FP32 feature row is widened exactly; everything else as for FP64 rows."""
    case = ref.two_stage(ref.N_TWO_STAGE[0], "equal_two_blocks")
    X32 = case.bufs["X"].astype(np.float32)
    want = ref.Case(case.name, case.p, dict(case.bufs, X=X32.astype(np.float64)))
    rec = want.model_record()
    case.bufs["X"] = X32
    after, launches = call_local(case, dev, xtype=_L().INGEST_F32)
    assert launches == 2
    expected = _only({k: v.copy() for k, v in case.bufs.items() if v is not None}, LOCAL)
    expected["record"][:case.rec_len()] = rec
    diff = ref.first_difference(expected, after)
    assert diff is None, diff


# ------------------------------------------------------------------------------------------- ital_select_resolve
@pytest.mark.parametrize("world", ref.WORLDS)
def test_select_resolve_equals_the_model(dev, world):
    """Hand-built records: every scenario once per rank value, each rank with its own alive flags."""
    cases = ref.resolve_cases(world)
    assert {c.p["rank"] for c in cases} == set(range(world))
    for case in cases:
        after, launches = call_resolve(case, dev)
        assert launches == 1
        diff = ref.first_difference(ref.expect_resolve(case), after)
        assert diff is None, (case, diff)


@pytest.mark.parametrize("kmax,world", [(4, 2), (9, 3)])
def test_a_full_sequence_of_resolves_keeps_the_batch_ordered(dev, kmax, world):
    """kmax resolves whose data indices arrive scrambled (one of them twice): after each step bsort[0 .. slot] is the stable
    argsort of bidx[0 .. slot], sig is symmetric on the filled block and everything else is untouched."""
    dims, steps = ref.sequence_records(kmax, world, 77 + kmax)
    for rank in range(world):
        state = ref.empty_state(dims)
        for slot, recs in enumerate(steps):
            p = dict(kmax=kmax, ldx=dims[1], ldw=dims[2], mode=0, slot=slot, rank=rank, world=world)
            case = ref.Case("sequence-rank%d-slot%d" % (rank, slot), p, dict(state, records=recs))
            after, _ = call_resolve(case, dev)
            diff = ref.first_difference(ref.expect_resolve(case), after)
            assert diff is None, (case, diff)
            state = {k: after[k] for k in ref.STATE}
            assert list(state["bsort"][:slot + 1]) == list(np.argsort(state["bidx"][:slot + 1], kind="stable"))
            sig = state["sig"][:kmax * kmax].reshape(kmax, kmax)[:slot + 1, :slot + 1]
            assert np.array_equal(np.ascontiguousarray(sig).view(np.int64), np.ascontiguousarray(sig.T).view(np.int64))
            assert np.isfinite(sig).all()


# -------------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_are_refused_before_any_launch(dev):
    L = _L()
    lib = L.lib()
    case = ref.small_case(5, 0, "random", "zero", 4)
    d = _up(case.bufs, dev)
    p = case.p
    before = int(lib.ital_launch_count())

    def refused(rc, who):
        assert rc == -22, who
        assert who in lib.ital_last_error().decode(), (who, lib.ital_last_error().decode())

    def local(**bad):
        c = ref.Case("bad", dict(p, **bad), case.bufs)
        return lib.ital_select_local(*_local_args(c, d), c.p["kmax"], _p(d, "status"), _p(d, "work"), _p(d, "record"), _stream())

    def fused(batch=None, **bad):
        c = ref.Case("bad", dict(p, **bad), case.bufs)
        return lib.ital_select_fused(*_local_args(c, d), c.p["slot"], batch or _batch(case, d), _p(d, "status"), _p(d, "record"),
                                     _p(d, "ret"), _stream())

    def resolve(rec_len, slot):
        return lib.ital_select_resolve(_p(d, "record"), 1, rec_len, 0, 0, slot, _batch(case, d), _p(d, "alive"), _p(d, "ret"), _stream())

    for mode in (2, -1):
        refused(local(mode=mode), "ital_select_local")
        refused(fused(mode=mode), "ital_select_fused")
    refused(local(m=p["ldw"] + 1), "ital_select_local")
    refused(fused(m=p["ldw"] + 1), "ital_select_fused")
    for slot in (-1, p["kmax"], p["kmax"] + 3):
        refused(fused(slot=slot), "ital_select_fused")
        refused(resolve(case.rec_len(), slot), "ital_select_resolve")
    kmax, ldx, ldw = case.dims()
    for other in (ref.Case("b", dict(p, ldx=ldx + 16), {}), ref.Case("b", dict(p, ldw=ldw + 1), {})):
        refused(fused(batch=_batch(other, d)), "ital_select_fused")       # the batch's layout is not the call's
    for rec_len in (case.rec_len() - 1, case.rec_len() + 1, 0):
        refused(resolve(rec_len, 0), "ital_select_resolve")
    assert int(lib.ital_launch_count()) == before
    after = _down(d)
    diff = ref.first_difference({k: v for k, v in case.bufs.items() if v is not None}, after, exclude=())
    assert diff is None, diff
