"""The checker of tests/_mcmi_ref.py is sound and sharp, shown on the CPU.

Soundness: a plain NumPy FP64 emulation of ital_cov_block, ital_cov_abs_rowsum and ital_mcmi_score_step, written from the
formulas, passes every check at every shape tests/test_gpu_mcmi_kernels.py runs on the device (for the two large covariance
routes: on the pieces that module checks in the extended type).  Largest residual / bound of the emulation (printed again by
every run with -s):

    covariance block, small-route shapes      0.23
    covariance block, default-route pieces    0.17
    covariance block, LDS-route corners       0.12
    absolute row sum                          0.020
    conditional entropy, t <= 4               0.33
    conditional entropy, t >= 5               0.083

Sharpness: the emulation makes, one at a time, the mistakes the kernels can make (`defect=`), each under its own test id, and the
checker rejects each of them wherever the mistake touches the call, with two exceptions that the test asserts to lie below
twice the bound (no sound check can tell such a change from rounding), far inside the allowance of one slice in five:
  - a pattern group left out of the minimum: 7 of the 62 slices it touches, all with n_all = t and noise = 1e-6.  The sum then
    has one term, the candidate itself, whose updated variance is ~noise: its entropy term is ~1e-12 under every pattern.
  - noise left off the diagonal: 2 of 240 slices, (t, n_all) = (4, 4) and (5, 5) at noise = 1e-6, for the same reason.
    Elsewhere that mistake ends in NaN (the candidate's own updated variance is zero up to rounding) or moves the value by
    1e-7 relative and more.
A member that is not skipped in the sum over j moves the value by ~1e-13 relative at the production noise of 1e-6 (its updated
variance is ~noise and its entropy term ~1e-12), so the test holds that mistake to the noise = 0.1 cases.  A covariance row
sum without |.| is tried on blocks with 37 % to 100 % negative entries (asserted: at least 10 %)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _mcmi_ref as ref  # noqa: E402

WORST = {}


def _note(name, r):
    WORST[name] = max(WORST.get(name, 0.0), r)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for name, r in sorted(WORST.items()):
        print("host emulation  %-42s largest residual/bound = %.3g" % (name, r))


def _id(case):
    return "-".join(str(v) for v in case)


# ------------------------------------------------------------------------------------------------ the arithmetic
def _mpf(v):
    import mpmath
    return mpmath.mpf(np.format_float_scientific(v, precision=24, unique=False))


def test_the_extended_phi_agrees_with_mpmath_at_50_digits():
    """Both q and 1 - q, on a grid over [-38, 38] and around the switch between series and continued fraction."""
    import mpmath
    mpmath.mp.dps = 50
    z = np.concatenate((np.linspace(-38.0, 38.0, 457), 2.0 * np.sqrt(2.0) + np.linspace(-1e-3, 1e-3, 9),
                        -2.0 * np.sqrt(2.0) + np.linspace(-1e-3, 1e-3, 9), [0.0, 1e-300, -1e-9]))
    q, p = ref.phi_pair(ref.xp(z))
    tol = float(np.finfo(np.longdouble).eps) if ref.MODE == "longdouble" else 1e-42
    worst = 0.0
    for zz, a, b in zip(z, q, p):
        worst = max(worst, max(abs(_mpf(a) / mpmath.ncdf(zz) - 1), abs(_mpf(b) / mpmath.ncdf(-zz) - 1)) / (40 + 2 * zz * zz))
    print("extended Phi: largest relative error / (40 + 2 z^2) = %.3g (tolerance %.3g)" % (worst, tol))
    assert worst <= tol
    tol *= 40
    x = ref.xp(np.array([1e-3, 0.3, 0.5 - 1e-12, 1.0]))
    for a, b in zip(x, ref.xlog(x)):
        assert abs(_mpf(b) - mpmath.log(_mpf(a))) <= tol * max(1.0, abs(float(b)))


def test_the_fp64_hart_rational_is_accurate_to_the_published_1e_15():
    """PHI_ABS is the published absolute accuracy of MVNPHI; the same rational and far-tail continued fraction in FP64 NumPy stay
    inside it on a grid of 15203 points (largest error printed: some 1e-16)."""
    import mpmath
    mpmath.mp.dps = 50
    z = np.linspace(-38.0, 38.0, 15203)
    got = ref.mvnphi64(z)
    worst = max(abs(mpmath.mpf(float(a)) - mpmath.ncdf(float(b))) for a, b in zip(got, z))
    print("Hart 5666 in FP64: largest absolute error %.3g" % float(worst))
    assert worst <= ref.PHI_ABS


def test_expected_route_restates_the_thresholds():
    assert [ref.expected_route(*s) for s in ((1, 1), (200, 150), (4210, 4230), (3000, 3000), (2050, 2050), (3900, 3900))] == \
        ["small", "small", "lds", "default", "default", "default"]
    assert all(ref.expected_route(na, nb) == "small" for na, nb, _, _ in ref.SMALL_CASES)
    assert all(ref.expected_route(na, nb) == "default" for na, nb, _, _ in ref.DEFAULT_CASES)
    assert all(ref.expected_route(na, nb) == "lds" for na, nb, _, _ in ref.LDS_CASES)
    assert all(ref.expected_route(i1 - i0, j1 - j0) == "small" for c in ref.DEFAULT_CASES + ref.LDS_CASES
               for i0, i1, j0, j1 in ref.pieces(c[0], c[1]))
    assert ref.expected_nsplit(257, 1000, 7 * 257) == (7, 16) and ref.expected_nsplit(130, 4200, 64 * 130) == (64, 66)


# ------------------------------------------------------------------------------------------------ covariance block
def _cov_ratio(s, rows=None, cols=None, defect=None):
    i0, i1 = rows or (0, s.na)
    j0, j1 = cols or (0, s.nb)
    Xa, Xb, Va, Vb = s.Xa[i0:i1], s.Xb[j0:j1], s.Va[:, i0:i1], s.Vb[:, j0:j1]
    out = ref.emu_cov_block(Xa, s.an[i0:i1], Xb, s.bn[j0:j1], Va, Vb, s.m, s.var, s.ls, defect)
    return ref.cov_block_check(out, Xa, s.an[i0:i1], Xb, s.bn[j0:j1], Va, Vb, s.m, s.var, s.ls)


@pytest.mark.parametrize("case", ref.SMALL_CASES, ids=_id)
def test_the_fp64_covariance_block_passes_its_bound(case):
    r = _cov_ratio(ref.cov_inputs(*case))
    _note("covariance block, small-route shapes", r)
    assert r <= 1.0, (case, r)


@pytest.mark.parametrize("case", ref.DEFAULT_CASES + ref.LDS_CASES, ids=_id)
def test_the_fp64_covariance_block_passes_its_bound_on_the_checked_pieces(case):
    s = ref.cov_inputs(*case)
    name = "covariance block, %s" % ("default-route pieces" if case in ref.DEFAULT_CASES else "LDS-route corners")
    for i0, i1, j0, j1 in ref.checked_pieces(case[0], case[1]):
        r = _cov_ratio(s, (i0, i1), (j0, j1))
        _note(name, r)
        assert r <= 1.0, (case, i0, j0, r)


def _cov_applies(defect, na, nb, ldx, m):
    return {"last16": (ldx // 16) % 2 == 1, "mquad": m % 4 != 0, "sign": m > 0, "swap": m > 0 and (na, nb) != (1, 1),
            "ragged_norm": (na % 16 != 0 and na > 1) or (nb % 16 != 0 and nb > 1)}[defect]


@pytest.mark.parametrize("defect", ref.COV_DEFECTS)
def test_a_defect_of_the_covariance_block_is_rejected(defect):
    seen = 0
    for case in ref.SMALL_CASES:
        if _cov_applies(defect, *case):
            r = _cov_ratio(ref.cov_inputs(*case), defect=defect)
            assert r > 1.0, (defect, case, r)
            seen += 1
    assert seen >= 8


# ------------------------------------------------------------------------------------------------ absolute row sum
def _rowsum_ratio(shape, mult, accumulate, defect=None, nb=None):
    na, nb0, ldx, m = shape
    s = ref.cov_inputs(*shape)
    nb = nb0 if nb is None else nb
    nsplit = ref.expected_nsplit(na, nb, mult * na)[0] if nb else 1
    prior = np.linspace(0.5, 2.5, na)
    Xb, bn, Vb = s.Xb[:nb], s.bn[:nb], s.Vb[:, :nb]
    out = ref.emu_rowsum(prior, accumulate, s.Xa, s.an, Xb, bn, s.Va, Vb, m, s.var, s.ls, nsplit, defect)
    return ref.rowsum_check(out, prior if accumulate else np.zeros(na), s.Xa, s.an, Xb, bn, s.Va, Vb, m, s.var, s.ls, nsplit)


@pytest.mark.parametrize("shape", ref.ROWSUM_SHAPES, ids=_id)
def test_the_fp64_row_sum_passes_its_bound(shape):
    for mult in ref.ROWSUM_WORK:
        for accumulate in (0, 1):
            r = _rowsum_ratio(shape, mult, accumulate)
            _note("absolute row sum", r)
            assert r <= 1.0, (shape, mult, accumulate, r)
    assert _rowsum_ratio(shape, 1, 0, nb=0) == 0.0 and _rowsum_ratio(shape, 1, 1, nb=0) == 0.0


def test_the_row_sum_inputs_have_negative_entries():
    for shape in ref.ROWSUM_SHAPES:
        s = ref.cov_inputs(*shape)
        share = ref.negative_share(s.Xa, s.Xb, s.Va, s.Vb, s.m, s.var, s.ls)
        print("negative entries of the reference block", shape, "%.0f %%" % (100 * share))
        assert share >= 0.10, (shape, share)


@pytest.mark.parametrize("defect", ref.ROWSUM_DEFECTS)
def test_a_defect_of_the_row_sum_is_rejected(defect):
    seen = 0
    for shape in ref.ROWSUM_SHAPES:
        na, nb, ldx, m = shape
        for mult in ref.ROWSUM_WORK:
            nsplit, ntile = ref.expected_nsplit(na, nb, mult * na)
            for accumulate in (0, 1):
                applies = {"noabs": True, "skip_tile": ntile % nsplit != 0, "no_accumulate": accumulate == 1}.get(defect)
                if applies is None:
                    applies = _cov_applies(defect, *shape)
                if applies:
                    r = _rowsum_ratio(shape, mult, accumulate, defect)
                    assert r > 1.0, (defect, shape, mult, accumulate, r)
                    seen += 1
    assert seen >= 4


# ------------------------------------------------------------------------------------------------ conditional entropy
def _ce_cases(t, n_all, noise):
    for n_i, pos_offset in ref.slices(t, n_all):
        yield ref.ce_inputs(t, n_all, noise, n_i, pos_offset)


@pytest.mark.parametrize("case", ref.CE_CASES, ids=_id)
def test_the_fp64_scorer_passes_its_bound(case):
    t = case[0]
    for inp in _ce_cases(*case):
        emu = ref.emu_ce(inp)
        sub = ref.subset(inp, ref.ce_subset_size(t))
        r = ref.ce_check(emu, inp, sub, ref.ce_ref_cached(t, case[1], case[2], inp.n_i, inp.pos_offset))
        _note("conditional entropy, t %s" % ("<= 4" if t <= 4 else ">= 5"), r)
        assert r <= 1.0, (case, inp.n_i, inp.pos_offset, r)
        assert ref.ce_check_against_emulation(emu, emu, inp, sub) == 0.0


def _ce_applies(defect, inp):
    """Whether the mistake touches anything the call computes."""
    t, n = inp.t, inp.n_all
    live = int(inp.alive.sum())
    j = np.arange(n)
    lost = {"last_stride": j >= n // 256 * 256 if n % 256 else j < 0, "wave_dropped": (j % 256) // 64 == 1}.get(defect)
    if lost is not None:
        return live > 0 and bool((lost & ref._keep(inp)).any())
    return live > 0 and {"no_noise": True, "member_kept": t > 1 and inp.noise == 0.1, "li_for_gi": inp.pos_offset > 0,
                         "group_dropped": t >= 5, "dead_scored": live < inp.n_i}[defect]


@pytest.mark.parametrize("defect", [d for d in ref.CE_DEFECTS if d != "nanmin"])
def test_a_defect_of_the_scorer_is_rejected(defect):
    """Every mistake at every slice of every case it touches.  A slice may be excused only where the mistake moves no checked
    value by twice its bound (asserted from the two emulations and the reference's bound; such a change cannot be told from
    rounding by any sound check), and at no more than one slice in five; the excused slices are printed."""
    seen, excused = 0, []
    for case in ref.CE_CASES:
        for inp in _ce_cases(*case):
            if not _ce_applies(defect, inp):
                continue
            sub = ref.subset(inp, ref.ce_subset_size(case[0]))
            full = ref.ce_ref_cached(case[0], case[1], case[2], inp.n_i, inp.pos_offset)
            bad = ref.emu_ce(inp, defect)
            seen += 1
            if ref.ce_check(bad, inp, sub, full) > 1.0:
                continue
            good = ref.emu_ce(inp)
            assert all(abs(bad[li] - good[li]) < 2 * float(bound) for li, (_, bound, _) in full.items()), (defect, case, inp.n_i)
            excused.append(case + (inp.n_i, inp.pos_offset))
    print(defect, "touches", seen, "slices; below twice the bound at", excused)
    assert seen >= 20 and 5 * len(excused) <= seen, (seen, excused)


@pytest.mark.parametrize("t", [3, 6])
def test_the_nan_rule_and_a_nanmin_in_its_place(t):
    """s'_{j*} <= -1e-6 for every second scored candidate and >= +1e-6 for the others, in the reference; the emulation gives NaN
    exactly there, and a sum that ignores the NaN term is rejected."""
    inp = ref.nan_inputs(t)
    full = ref.ce_ref(inp)
    due = sorted(li for li, (val, _, _) in full.items() if val is None)
    assert due == sorted(inp.hit) and 0 < len(due) < len(full)
    lo, hi = ref.sprime_at_jstar(inp)
    assert max(lo) <= -1e-6 and min(hi) >= 1e-6
    emu = ref.emu_ce(inp)
    assert sorted(np.nonzero(np.isnan(emu))[0].tolist()) == due
    assert ref.ce_check(emu, inp, ref=full) <= 1.0
    assert ref.ce_check(ref.emu_ce(inp, "nanmin"), inp, ref=full) == float("inf")


def test_the_minimising_patterns_cover_the_first_a_middle_and_the_last_group():
    assert ref.group_coverage() == {"first", "middle", "last"}


def test_both_arithmetics_give_the_same_verdict(monkeypatch):
    """The mpmath path (used where long double is only 64 bits wide) reproduces the ratios of the long double path, up to the
    long double's own rounding: 2^-64 against bounds of a few 2^-53, some 1e-3 of a bound."""
    import mpmath  # noqa: F401
    import _gp_update_ref as base
    s = ref.cov_inputs(17, 33, 32, 5)
    inp = ref.ce_inputs(3, 9, 0.1, 9, 0)
    got = []
    for mode in ("longdouble", "mpmath"):
        if mode == "longdouble" and ref.MODE != "longdouble":
            continue
        monkeypatch.setattr(base, "MODE", mode)
        monkeypatch.setattr(ref, "MODE", mode)
        args = (s.Xa, s.an, s.Xb, s.bn, s.Va, s.Vb, s.m, s.var, s.ls)
        got.append((ref.cov_block_check(ref.emu_cov_block(*args), *args),
                    ref.rowsum_check(ref.emu_rowsum(s.an, 1, *args, 1), s.an, *args, 1),
                    ref.ce_check(ref.emu_ce(inp), inp, [0, 4]),
                    ref.ce_check(ref.emu_ce(inp, "member_kept"), inp, [0, 4])))
    for r in got:
        assert max(r[:3]) <= 1.0 < r[3], r
    if len(got) == 2:
        for a, b in zip(*got):
            assert b == pytest.approx(a, rel=1e-3, abs=1e-3) or a == b
