"""The checker of tests/_gp_update_ref.py is sound and sharp, shown on the CPU.

Soundness: a straightforward NumPy FP64 emulation of every operation (row-by-row append, forward substitution, K - W V) passes
every check at every shape tests/test_gpu_gp_update.py runs on the device, the near-duplicate rows included -- so the a-priori
bounds admit a correct FP64 implementation, with room: the largest ratios are printed at the end of the module (run with -s).
Sharpness: the emulation makes, one at a time, the mistakes the device kernels can make (`defect=`), and the checker rejects each
of them at every shape where the mistake changes anything."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _gp_update_ref as ref  # noqa: E402

NAN = float("nan")
WORST = {}


def _note(entry, kind, ratios):
    for name, r in ratios.items():
        key = (entry, kind, name)
        WORST[key] = max(WORST.get(key, 0.0), r)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (entry, kind, name), r in sorted(WORST.items()):
        print("host emulation  %-12s %-8s %-9s largest residual/bound = %.3g" % (entry, kind, name, r))


def _chol_inputs(s):
    m, M = s.m, s.m + s.c
    L0, a0 = np.full((M, M), NAN), np.full(M, NAN)
    L0[:m, :m] = np.where(np.tri(m, dtype=bool), s.L[:m, :m], NAN)
    a0[:m] = s.alpha[:m]
    return L0, a0


def _run_chol(s, defect=None):
    L0, a0 = _chol_inputs(s)
    L, alpha, status = ref.emu_chol_append(s.XT, ref.row_norms64(s.XT), L0, a0, s.y[s.m:], s.m, s.c, s.var, s.ls, s.noise, defect)
    assert np.array_equal(L[:s.m].view(np.int64), L0[:s.m].view(np.int64))
    ratios = ref.judge_chol(s, L, alpha)
    ratios["status"] = float("inf") if status else 0.0       # a defect may also end in "not positive definite"
    return ratios


def _sweep_inputs(s):
    """NaN wherever the sweep must not read: the strict upper triangle of L22, the pad columns of the factor rows, V rows >= m."""
    m, c, M = s.m, s.c, s.m + s.c
    ldw = M + 3
    Lrows = np.full((c, ldw), NAN)
    Lrows[:, :m] = s.L[m:, :m]
    Lrows[:, m:M] = np.where(np.tri(c, dtype=bool), s.L[m:, m:], NAN)
    V0 = np.full((M, s.n), NAN)
    V0[:m] = s.V[:m]
    if s.kind == "free":
        return Lrows, ldw, V0, s.mu_in, s.s2_in
    return Lrows, ldw, V0, s.V[:m].T @ s.alpha[:m], s.var - (s.V[:m] ** 2).sum(axis=0)


def _run_whiten(s, defect=None):
    m, c = s.m, s.c
    Lrows, ldw, V0, mu0, s20 = _sweep_inputs(s)
    V, mu, s2 = ref.emu_whiten(s.X, ref.row_norms64(s.X), s.XT[m:], ref.row_norms64(s.XT[m:]), Lrows, ldw, s.alpha[m:], V0, mu0,
                               s20, m, c, s.var, s.ls, defect)
    return ref.judge_whiten(s, V, mu0, mu, s20, s2)


def _run_cross(s, defect=None):
    m = s.m
    out = ref.emu_cross_cov(s.X, ref.row_norms64(s.X), s.XT[m:], ref.row_norms64(s.XT[m:]), s.W, s.V, m, s.var, s.ls, defect)
    return ref.judge_cross(s, out)


def _id(case):
    return "-".join(str(v) for v in case)


# ------------------------------------------------------------------------------------------------ soundness
@pytest.mark.parametrize("case", ref.CHOL_CASES, ids=_id)
def test_the_fp64_append_passes_the_factor_and_alpha_bounds(case):
    ratios = _run_chol(ref.state(*case))
    _note("chol_append", case[0], ratios)
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("case", ref.WHITEN_CASES, ids=_id)
def test_the_fp64_whitening_sweep_passes_its_bounds(case):
    n, m, c, ldx = case
    ratios = _run_whiten(ref.state("uniform", m, c, ldx, n))
    _note("whiten", "uniform", ratios)
    assert max(ratios.values()) <= 1.0, ratios


def test_the_fp64_whitening_sweep_passes_its_bounds_on_free_form_inputs():
    ratios = _run_whiten(ref.free_form_whiten())
    _note("whiten", "free", ratios)
    assert max(ratios.values()) <= 1.0, ratios


def test_the_fp64_whitening_sweep_passes_its_bounds_on_near_duplicate_rows():
    for m, c in ((17, 5), (33, 16)):
        ratios = _run_whiten(ref.state("neardup", m, c, 16, 65))
        _note("whiten", "neardup", ratios)
        assert max(ratios.values()) <= 1.0, (m, c, ratios)


@pytest.mark.parametrize("case", ref.CROSS_CASES, ids=_id)
def test_the_fp64_cross_covariance_passes_its_bound(case):
    n, m, c, ldx = case
    ratios = _run_cross(ref.state("uniform", m, c, ldx, n))
    _note("cross_cov", "uniform", ratios)
    assert max(ratios.values()) <= 1.0, (case, ratios)


@pytest.mark.parametrize("case", ref.PREDICT_CASES, ids=_id)
def test_the_fp64_predict_passes_its_bounds(case):
    m, nt = case
    s = ref.state("uniform", m, 0, 16, nt)
    Vt, mean, pvar = ref.emu_predict(s.X, s.XT, ref.row_norms64(s.XT), s.L, s.alpha, m, s.var, s.ls)
    ratios = ref.judge_predict(s, Vt, mean, pvar)
    _note("predict", "uniform", ratios)
    assert max(ratios.values()) <= 1.0, ratios


def test_the_emulated_append_reports_a_matrix_that_is_not_positive_definite():
    XT = np.zeros((2, 16))
    XT[:, :5] = 0.25
    L0, a0 = np.full((2, 2), NAN), np.full(2, NAN)
    L, alpha, status = ref.emu_chol_append(XT, ref.row_norms64(XT), L0, a0, np.array([1.0, -1.0]), 0, 2, 1.0, 0.5, -0.5)
    assert status == 1 and L[0, 0] == np.sqrt(0.5) and np.isnan(L[1, 1])
    assert ref.check_structure(L, 0, 2)


# ------------------------------------------------------------------------------------------------ sharpness
def _applies(defect, m, c, ldx):
    return {"cross_block": m > 64, "last_column": m >= 1, "alpha_l21": m >= 1, "perturb": m >= 1,
            "wv_slice": m >= 1, "partial_step": ldx % 64 != 0, "wrong_ld": c >= 2}[defect]


def _perturbation_is_above_the_rounding_bound(s, rel):
    """Whether a relative change `rel` of L[m][m // 2] moves some residual of row m by more than twice its bound.  A change
    below that cannot be told from the roundings a correct FP64 append may make (the unperturbed residual may sit anywhere
    inside its bound), so no sound componentwise check rejects it; above it every sound check must.  Decided from the
    reference state alone (s.L is the rounded exact factor), not from what the code under test returns."""
    m, p = s.m, s.m // 2
    bound = ref.factor_bound(s.L, m, s.dK_TT, m + s.c + 4)[p:]
    shift = ref.xp(rel) * abs(ref.xp(s.L[m, p])) * np.abs(ref.xp(s.L[p:m + 1, p]))
    return bool((shift > 2 * bound).any())


@pytest.mark.parametrize("defect", ref.CHOL_DEFECTS)
def test_a_defect_of_the_append_is_rejected(defect):
    """Every defect at every shape where it changes anything.  The relative perturbation of 1e-11 of L[m][m // 2] is
    rejected at 26 of the 30 shapes with m >= 1.  It may pass only where it stays below twice the rounding bound of the
    residuals it moves (asserted; L[m][m // 2] decays with the distance of the two rows: 2e-3 to 1e-4 at those four shapes,
    which are printed); there the same entry is perturbed by the first power of ten that does exceed twice the bound
    (1e-6 at the most), and that is rejected."""
    seen, small = 0, []
    for case in ref.CHOL_CASES:
        kind, m, c, ldx = case
        if not _applies(defect, m, c, ldx):
            continue
        s = ref.state(*case)
        ratios = _run_chol(s, defect)
        if defect == "perturb" and max(ratios.values()) <= 1.0:
            assert not _perturbation_is_above_the_rounding_bound(s, 1e-11), case       # else the checker is not sharp
            rel = 1e-10
            while not _perturbation_is_above_the_rounding_bound(s, rel):
                rel *= 10.0
            assert rel <= 1e-6, (case, rel)
            small.append(case + (rel,))
            L0, a0 = _chol_inputs(s)
            L, alpha, _ = ref.emu_chol_append(s.XT, ref.row_norms64(s.XT), L0, a0, s.y[m:], m, c, s.var, s.ls, s.noise)
            L[m, m // 2] *= 1.0 + rel
            ratios = ref.judge_chol(s, L, alpha)
        assert max(ratios.values()) > 1.0, (defect, case, ratios)
        seen += 1
    assert seen >= (15 if defect == "cross_block" else 30)
    if small:
        print("1e-11 of L[m][m // 2] is below twice its rounding bound at", small)
    assert len(small) <= 4


@pytest.mark.parametrize("defect", ref.SWEEP_DEFECTS)
def test_a_defect_of_the_row_sweep_is_rejected(defect):
    seen = 0
    for n, m, c, ldx in ref.WHITEN_CASES:
        if _applies(defect, m, c, ldx):
            ratios = _run_whiten(ref.state("uniform", m, c, ldx, n), defect)
            assert ratios["whiten"] > 1.0, (defect, n, m, c, ldx, ratios)
            seen += 1
    for n, m, c, ldx in ref.CROSS_CASES:
        if defect != "wrong_ld" and _applies(defect, m, c, ldx):
            ratios = _run_cross(ref.state("uniform", m, c, ldx, n), defect)
            assert ratios["cross"] > 1.0, (defect, n, m, c, ldx, ratios)
            seen += 1
    assert seen >= 30


def test_a_wrong_mu_or_s2_is_rejected():
    s = ref.state("uniform", 17, 5, 16, 65)
    Lrows, ldw, V0, mu0, s20 = _sweep_inputs(s)
    V, mu, s2 = ref.emu_whiten(s.X, ref.row_norms64(s.X), s.XT[17:], ref.row_norms64(s.XT[17:]), Lrows, ldw, s.alpha[17:], V0, mu0,
                               s20, 17, 5, s.var, s.ls)
    good = ref.judge_whiten(s, V, mu0, mu, s20, s2)
    assert max(good.values()) <= 1.0
    mu_bad, s2_bad = mu.copy(), s2.copy()
    mu_bad[64] += 1e-13
    s2_bad[0] += 1e-13
    bad = ref.judge_whiten(s, V, mu0, mu_bad, s20, s2_bad)
    assert bad["mu"] > 1.0 and bad["s2"] > 1.0 and bad["whiten"] == good["whiten"]


def test_a_nan_or_a_sign_of_zero_in_the_new_block_is_rejected():
    s = ref.state("uniform", 1, 16, 16)
    L0, a0 = _chol_inputs(s)
    L, alpha, _ = ref.emu_chol_append(s.XT, ref.row_norms64(s.XT), L0, a0, s.y[1:], 1, 16, s.var, s.ls, s.noise)
    assert not ref.check_structure(L, 1, 16)
    for at, v in (((3, 9), -0.0), ((3, 9), NAN), ((5, 5), -L[5, 5]), ((16, 0), NAN)):
        Lb = L.copy()
        Lb[at] = v
        assert ref.check_structure(Lb, 1, 16), (at, v)
    ab = alpha.copy()
    ab[7] = NAN
    assert ref.judge_chol(s, L, ab)["alpha"] == float("inf")


# ------------------------------------------------------------------------------------------------ the arithmetic
def test_the_extended_type_is_what_the_module_says():
    assert ref.MODE in ("longdouble", "mpmath")
    one = ref.xp(1.0)
    tiny = ref.xp(2.0 ** -60)
    assert (one + tiny) - one == tiny              # 2^-60 survives next to 1: more than 53 bits
    assert float(ref.gamma(10)) == pytest.approx(10 * 2.0 ** -53, rel=1e-12)


def test_both_arithmetics_give_the_same_verdict(monkeypatch):
    """The mpmath path (used where long double is only 64 bits wide) reproduces the ratios of the long double path."""
    import mpmath  # noqa: F401
    build = ref.state.__wrapped__
    got = []
    for mode in ("longdouble", "mpmath"):
        if mode == "longdouble" and ref.MODE != "longdouble":
            continue
        monkeypatch.setattr(ref, "MODE", mode)
        s = build("uniform", 5, 3, 16, 4)
        r = dict(_run_chol(s))
        r.update(_run_whiten(s))
        r.update(_run_cross(s))
        got.append(r)
    for r in got:
        assert max(r.values()) <= 1.0, r
    if len(got) == 2:
        for key in got[0]:
            assert got[1][key] == pytest.approx(got[0][key], rel=1e-3, abs=1e-6), key
