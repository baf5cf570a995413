"""The checker of tests/_dense_ref.py is sound and sharp, shown on the CPU.

Soundness: a plain NumPy FP64 emulation of ital_gram_rows, ital_chol_batched (blocked as the kernels are),
ital_chol_solve_batched and ital_kernel_matvec passes every bound at every shape tests/test_gpu_dense_kernels.py runs on the
device, the near-duplicate rows (condition numbers up to 1e8) included -- so the a-priori bounds admit a correct FP64
implementation.  The largest ratios are printed at the end of the module (run with -s); they are the emulation column of the
table in the GPU file's docstring.  Sharpness: the emulation makes, one at a time, mistakes these kernels could make
(`defect=`), and the checker rejects each at every shape where the mistake changes the output."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _dense_ref as ref  # noqa: E402

NAN = float("nan")
WORST = {}
COND = {}


def _note(entry, kind, ratios):
    for name, r in ratios.items():
        key = (entry, kind, name)
        WORST[key] = max(WORST.get(key, 0.0), r)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (entry, kind, name), r in sorted(WORST.items()):
        print("host emulation  %-14s %-8s %-7s largest residual/bound = %.3g" % (entry, kind, name, r))
    for key, (lo, hi) in sorted(COND.items()):
        print("condition numbers of the Grams at n = 129 and 321, %s: %.1e to %.1e" % (key, lo, hi))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _id(case):
    return "-".join(str(v) for v in case)


def _gram(s, defect=None):
    return ref.emu_gram(s.X, ref.row_norms64(s.X), s.idx, s.n, s.var, s.ls, s.noise, defect)


def _factor(A, defect=None):
    """The emulated factor of the lower triangle of A inside a NaN-guarded buffer.  Returns (buffer, ratios): `factor` is
    inf when info != 0, `writes` is inf when anything outside the lower triangle changed."""
    n = A.shape[0]
    buf = ref.guarded(ref.lower_nan(A), n + 3)
    out, info = ref.emu_chol(buf, n, max_n=n + 2, defect=defect)
    written = np.zeros(buf.shape, dtype=bool)
    written[:n, :n] = np.tri(n, dtype=bool)
    same = np.array_equal(_bits(buf)[~written], _bits(out)[~written])
    return out, dict(factor=float("inf") if info else ref.check_factor(out, A, n), writes=0.0 if same else float("inf"))


# ------------------------------------------------------------------------------------------------ soundness
@pytest.mark.parametrize("case", ref.GRAM_CASES, ids=_id)
def test_the_fp64_chain_gram_factor_solve_passes_its_bounds(case):
    """Gram -> factor -> two solves, each step on the FP64 output of the one before, as the evidence prologue chains them."""
    s = ref.gram_case(*case)
    Kref, dK = ref.gram_ref(*case)
    K = _gram(s)
    ratios = dict(gram=ref.check_gram(K, Kref, dK, s.noise))
    L, r = _factor(K)
    assert r["factor"] != float("inf"), "the Gram does not factor in FP64 with info == 0"
    ratios.update(r)
    for name, y in (("solve", s.y), ("solve6", s.y_wide)):
        ratios[name] = ref.check_solve(L, ref.emu_solve(L, s.n, y), y, s.n)
    _note("chain", s.kind, ratios)
    assert max(ratios.values()) <= 1.0, ratios
    if s.n in (129, 321):
        full = np.tril(K) + np.tril(K, -1).T
        c = float(np.linalg.cond(full))
        lo, hi = COND.get(s.kind, (c, c))
        COND[s.kind] = (min(lo, c), max(hi, c))


@pytest.mark.parametrize("n", ref.SIZES)
def test_the_fp64_factor_and_solves_pass_their_bounds_on_host_built_matrices(n):
    A = ref.host_spd(n)
    L, ratios = _factor(A)
    for name, y in zip(("solve", "solve6"), ref.rhs(n)):
        ratios[name] = ref.check_solve(L, ref.emu_solve(L, n, y), y, n)
    _note("chol+solve", "host", ratios)
    assert max(ratios.values()) <= 1.0, ratios


def test_the_conditioning_is_what_the_gpu_file_says():
    """Three decades past the 1e5 the evidence tests allow: the near-duplicate Grams reach 1e7 and more."""
    worst = {}
    for kind, ldx, ls in ref.GRAM_PARAMS:
        for n in (129, 321):
            K = _gram(ref.gram_case(kind, ldx, ls, n))
            worst[kind] = max(worst.get(kind, 0.0), float(np.linalg.cond(np.tril(K) + np.tril(K, -1).T)))
    assert worst["uniform"] >= 1e4 and worst["neardup"] >= 1e7, worst


@pytest.mark.parametrize("case", ref.MATVEC_SMALL_CASES, ids=_id)
def test_the_fp64_kernel_times_w_passes_its_bound(case):
    na, nb, ldx, F = case
    s = ref.matvec_case(*case)
    if (na, nb) in ref.MATVEC_SMALL_SPLITS:
        assert (s.nsplit, s.per) == ref.MATVEC_SMALL_SPLITS[(na, nb)]
    out = ref.emu_matvec(s.Xa, ref.row_norms64(s.Xa), s.Xb, ref.row_norms64(s.Xb), s.W, s.var, s.ls)
    Kref, dK = ref.kernel_ref(s.Xa, s.Xb, s.var, s.ls)
    r = ref.check_matvec(out, Kref, dK, s.W, nb, s.nsplit)
    _note("kernel_matvec", "small", dict(out=r))
    assert r <= 1.0, r


@pytest.fixture(scope="module")
def loop_runs():
    """The FP64 emulation of the two production-loop shapes, computed once."""
    runs = {}
    for na, nb, ldx, F, nsplit, per, last in ref.MATVEC_LOOP:
        s = ref.matvec_case(na, nb, ldx, F)
        runs[(na, nb)] = (s, ref.emu_matvec(s.Xa, ref.row_norms64(s.Xa), s.Xb, ref.row_norms64(s.Xb), s.W, s.var, s.ls))
    return runs


@pytest.mark.parametrize("shape", ref.MATVEC_LOOP, ids=_id)
def test_the_fp64_kernel_times_w_passes_its_bound_in_the_production_loop(shape, loop_runs):
    na, nb, ldx, F, nsplit, per, last = shape
    s, out = loop_runs[(na, nb)]
    assert (s.nsplit, s.per) == (nsplit, per) == ref.expected_split(na, nb)
    assert ref._cdiv(nb - (nsplit - 1) * per * ref.T, ref.T) == last
    rows = ref.loop_rows(na, nb)
    Kref, dK = ref.kernel_ref(s.Xa[rows], s.Xb, s.var, s.ls)
    r = ref.check_matvec(out[rows], Kref, dK, s.W, nb, nsplit)
    _note("kernel_matvec", "loop", dict(out=r))
    assert r <= 1.0, r


def test_expected_split_restates_the_table_of_the_issue():
    assert ref.expected_split(129, 4001) == (32, 1)
    assert ref.expected_split(1000, 1531) == (12, 1)
    assert ref.expected_split(9298, 9298) == (15, 5)
    assert ref.expected_split(4000, 4224) == (17, 2)
    assert ref.expected_split(4200, 4200) == (17, 2)          # the held-out-scores test of tests/test_gpu_tune.py
    assert ref.expected_workspace(300, 77) == 0 and ref.expected_workspace(130, 129) == 2 * 130 * 16


# ------------------------------------------------------------------------------------------------ failure paths
@pytest.mark.parametrize("j", [0, 63, 64, 65, 127, 128, 199])
def test_the_emulated_factor_reports_the_first_pivot_that_is_not_positive(j):
    A = ref.host_spd(200)
    A[j, j] = -1.0
    buf = ref.guarded(ref.lower_nan(A), 203)
    out, info = ref.emu_chol(buf, 200)
    assert info == j + 1
    k0 = j // 64 * 64
    assert ref.check_factor(out, A, 200, ncols=k0) <= 1.0
    outside = ~np.pad(np.tri(200, dtype=bool), ((0, 2), (0, 3)))
    assert np.array_equal(_bits(out)[outside], _bits(buf)[outside])
    assert not np.isnan(out[:200, :k0][np.tril_indices(200, 0, k0)]).any()


@pytest.mark.parametrize("r,c", [(64, 0), (70, 66), (130, 3), (199, 198)])
def test_the_emulated_factor_reports_the_row_of_a_nan_below_the_diagonal(r, c):
    A = ref.host_spd(200)
    A[r, c] = NAN
    out, info = ref.emu_chol(ref.guarded(ref.lower_nan(A), 203), 200)
    assert info == r + 1


# ------------------------------------------------------------------------------------------------ sharpness
def _chol_applies(defect, n):
    return {"syrk_k48": n > 64, "partial_full": n % 64 != 0, "max_n": True, "perturb": True}[defect]


@pytest.mark.parametrize("defect", ref.CHOL_DEFECTS)
def test_a_defect_of_the_factor_is_rejected(defect):
    seen = 0
    mats = [("host", n, ref.host_spd(n)) for n in ref.SIZES]
    for kind, ldx, ls in (ref.GRAM_PARAMS[0], ref.GRAM_PARAMS[3]):
        mats += [(kind, n, _gram(ref.gram_case(kind, ldx, ls, n))) for n in ref.SIZES]
    for kind, n, A in mats:
        if _chol_applies(defect, n):
            _, ratios = _factor(A, defect)
            assert max(ratios.values()) > 1.0, (defect, kind, n, ratios)
            seen += 1
    assert seen >= 27


@pytest.mark.parametrize("defect", ref.SOLVE_DEFECTS)
def test_a_defect_of_the_solve_is_rejected(defect):
    seen = 0
    for n in ref.SIZES:
        if {"backward_forward": n > 64, "tail_skipped": n % 64 != 0}[defect]:
            L, ratios = _factor(ref.host_spd(n))
            assert max(ratios.values()) <= 1.0
            for y in ref.rhs(n):
                r = ref.check_solve(L, ref.emu_solve(L, n, y, defect), y, n)
                assert r > 1.0, (defect, n, r)
                seen += 1
    assert seen >= 18


def _gram_applies(defect, n):
    return {"noise_tile_local": n > 64, "idx_ignored": n >= 2, "clamped_norm": n >= 2}[defect]


@pytest.mark.parametrize("defect", ref.GRAM_DEFECTS)
def test_a_defect_of_the_gram_is_rejected(defect):
    seen = 0
    for case in ref.GRAM_CASES:
        if _gram_applies(defect, case[3]):
            s = ref.gram_case(*case)
            Kref, dK = ref.gram_ref(*case)
            r = ref.check_gram(_gram(s, defect), Kref, dK, s.noise)
            assert r > 1.0, (defect, case, r)
            seen += 1
    assert seen >= 54


def test_a_defect_of_the_kernel_times_w_is_rejected(loop_runs):
    seen = dict.fromkeys(ref.MATVEC_DEFECTS, 0)
    cases = [ref.matvec_case(*c) for c in ref.MATVEC_SMALL_CASES if c[3] == 5]
    cases += [ref.matvec_case(na, nb, ldx, F) for na, nb, ldx, F, _, _, _ in ref.MATVEC_LOOP[:1]]
    for s in cases:
        rows = list(range(s.na)) if s.na <= 300 else ref.loop_rows(s.na, s.nb)
        Kref, dK = ref.kernel_ref(s.Xa[rows], s.Xb, s.var, s.ls)
        an, bn = ref.row_norms64(s.Xa), ref.row_norms64(s.Xb)
        for defect in ref.MATVEC_DEFECTS:
            if {"first_tile_only": s.per > 1, "chunk_overrun": s.nsplit > 1, "clamped_weight": s.nb % 128 != 0}[defect]:
                out = ref.emu_matvec(s.Xa[rows], an[rows], s.Xb, bn, s.W, s.var, s.ls, defect) if s.na <= 300 else \
                    ref.emu_matvec(s.Xa, an, s.Xb, bn, s.W, s.var, s.ls, defect)[rows]
                r = ref.check_matvec(out, Kref, dK, s.W, s.nb, s.nsplit)
                assert r > 1.0, (defect, s.na, s.nb, r)
                seen[defect] += 1
    assert seen["first_tile_only"] >= 1 and seen["chunk_overrun"] >= 3 and seen["clamped_weight"] >= 5, seen


def test_the_emulation_check_of_the_large_shapes_rejects_a_dropped_tile(loop_runs):
    """What the rows outside the extended subset are held to: the device against the FP64 emulation at twice the bound."""
    na, nb = ref.MATVEC_LOOP[0][:2]
    s, good = loop_runs[(na, nb)]
    bound = ref.matvec_bound64(s.Xa, s.Xb, s.W, s.var, s.ls, s.nsplit)
    bad = ref.emu_matvec(s.Xa, ref.row_norms64(s.Xa), s.Xb, ref.row_norms64(s.Xb), s.W, s.var, s.ls, "first_tile_only")
    assert ref.check_matvec_against_emulation(good, good, bound) == 0.0
    assert ref.check_matvec_against_emulation(bad, good, bound) > 1.0
    one = good.copy()
    one[1777, 3] += 3.0 * (bound[1777, 3] + 2.0 ** -53 * abs(good[1777, 3]))
    assert ref.check_matvec_against_emulation(one, good, bound) > 1.0
    nan = good.copy()
    nan[5, 0] = NAN
    assert ref.check_matvec_against_emulation(nan, good, bound) == float("inf")


def test_a_nan_in_an_output_is_rejected():
    s = ref.gram_case("uniform", 16, 1.2, 65)
    Kref, dK = ref.gram_ref("uniform", 16, 1.2, 65)
    K = _gram(s)
    L, ratios = _factor(K)
    x = ref.emu_solve(L, 65, s.y)
    K[40, 3], L[64, 1], x[7] = NAN, NAN, NAN
    assert ref.check_gram(K, Kref, dK, s.noise) == float("inf")
    assert ref.check_factor(L, K, 65) == float("inf")
    assert ref.check_solve(L, x, s.y, 65) == float("inf")
