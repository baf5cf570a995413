"""Preparing feature rows without a device: header against binding, every refusal of the four entry points of
include/ital_prepare.h (they come before any HIP call), the range rule, the checkers of tests/_prepare_ref.py on the model's
own answer and on injected mistakes, principal_axes, Transform, and the min-max rule against what the real reference's
datasets.Dataset recorded (tests/golden/make_golden_prepare.py)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _prepare_ref as ref  # noqa: E402

from ital_amd import _lib, build  # noqa: E402
from ital_amd.prepare import Transform, principal_axes  # noqa: E402


# ------------------------------------------------------------------------------------------------------ ABI
def test_header_matches_the_binding():
    with open(os.path.join(ROOT, "include", "ital_prepare.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    assert set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", header)) == set(_lib.PREPARE_SIGNATURES)
    for name in dir(_lib):
        if name.endswith("SIGNATURES") and name != "PREPARE_SIGNATURES":
            assert not set(_lib.PREPARE_SIGNATURES) & set(getattr(_lib, name)), name
    ctype = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const double*": ctypes.c_void_p, "double*": ctypes.c_void_p,
             "hipStream_t": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}
    lib = _lib.lib()
    for name, (res, args) in _lib.PREPARE_SIGNATURES.items():
        m = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)" % name, header)
        assert ctype[m.group(1)] is res, name
        params = [re.sub(r"\s*\w+$", "", p.strip()).replace(" *", "*") for p in m.group(2).split(",")]
        assert [ctype[p] for p in params] == args == getattr(lib, name).argtypes, (name, params)
    for macro, value in (("ITAL_PREPARE_STATS_UNIT", _lib.PREPARE_STATS_UNIT), ("ITAL_PREPARE_STATS_CAP", _lib.PREPARE_STATS_CAP),
                         ("ITAL_PREPARE_COV_UNIT", _lib.PREPARE_COV_UNIT), ("ITAL_PREPARE_COV_CAP", _lib.PREPARE_COV_CAP),
                         ("ITAL_PREPARE_MAX_K", _lib.PREPARE_MAX_K)):
        assert int(re.search(r"#define %s (\d+)" % macro, header).group(1)) == value
    assert "prepare.hip" in build.SOURCES


P = 4096          # a fake, suitably aligned pointer: a refusal never touches it

CALLS = {
    "ital_col_stats": (("X", "xtype", "n", "d", "ldx", "cmin", "cmax", "csum", "workspace", "workspace_bytes", "stream"),
                       dict(X=P, xtype=0, n=10, d=5, ldx=16, cmin=P, cmax=P, csum=P, workspace=P, workspace_bytes=1 << 20, stream=0)),
    "ital_scale_rows": (("X", "xtype", "n", "d", "ldx", "lo", "span", "Y", "ytype", "ldy", "stream"),
                        dict(X=P, xtype=0, n=10, d=5, ldx=16, lo=P, span=P, Y=P, ytype=0, ldy=16, stream=0)),
    "ital_col_cov": (("X", "xtype", "n", "d", "ldx", "mean", "C", "ldc", "workspace", "workspace_bytes", "stream"),
                     dict(X=P, xtype=0, n=10, d=5, ldx=16, mean=P, C=P, ldc=5, workspace=P, workspace_bytes=1 << 20, stream=0)),
    "ital_project_rows": (("X", "xtype", "n", "d", "ldx", "shift", "W", "ldw", "k", "Y", "ytype", "ldy", "stream"),
                          dict(X=P, xtype=0, n=10, d=5, ldx=16, shift=P, W=P, ldw=3, k=3, Y=P, ytype=0, ldy=16, stream=0)),
}

COMMON = [dict(n=-1), dict(n=1 << 31), dict(d=0), dict(d=-3), dict(ldx=0), dict(ldx=-16), dict(ldx=24), dict(d=17), dict(xtype=4),
          dict(xtype=-1), dict(X=0), dict(X=P + 8)]
REFUSALS = {
    "ital_col_stats": COMMON + [dict(cmin=0), dict(cmax=0), dict(csum=0), dict(workspace=0), dict(cmin=P + 4), dict(cmax=P + 4),
                                dict(csum=P + 4), dict(workspace=P + 4), dict(workspace_bytes=3 * 5 * 8 - 1)],
    "ital_scale_rows": COMMON + [dict(ldy=0), dict(ldy=24), dict(d=20, ldx=32), dict(ytype=4), dict(ytype=-1), dict(lo=0),
                                 dict(span=0), dict(Y=0), dict(Y=P + 8), dict(lo=P + 4), dict(span=P + 4)],
    "ital_col_cov": COMMON + [dict(ldc=4), dict(ldc=-1), dict(mean=0), dict(C=0), dict(workspace=0), dict(mean=P + 4), dict(C=P + 4),
                              dict(workspace=P + 4), dict(workspace_bytes=5 * 5 * 8 - 1)],
    "ital_project_rows": COMMON + [dict(k=0), dict(k=513), dict(k=-1), dict(ldy=0), dict(ldy=24), dict(k=17, ldw=17), dict(ldw=2),
                                   dict(ytype=4), dict(ytype=-1), dict(shift=0), dict(W=0), dict(Y=0), dict(Y=P + 8),
                                   dict(shift=P + 4), dict(W=P + 4)],
}


def _call(name, **over):
    order, a = CALLS[name]
    a = dict(a)
    a.update(over)
    return getattr(_lib.lib(), name)(*[a[key] for key in order])


@pytest.mark.parametrize("name,over", [(name, over) for name in sorted(REFUSALS) for over in REFUSALS[name]],
                         ids=lambda v: v if isinstance(v, str) else ",".join("%s=%s" % kv for kv in v.items()))
def test_refusals_come_before_any_hip_call(name, over):
    assert _call(name, **over) == -22
    assert _lib.lib().ital_last_error().decode().startswith(name + ": ")


@pytest.mark.parametrize("name", sorted(CALLS))
def test_no_rows_is_no_work(name):
    order, _ = CALLS[name]
    nothing = {key: 0 for key in order if key in ("X", "cmin", "cmax", "csum", "workspace", "workspace_bytes", "lo", "span", "Y",
                                                   "mean", "C", "shift", "W")}
    before = _lib.lib().ital_launch_count()
    assert _call(name, n=0, **nothing) == 0
    assert _lib.lib().ital_launch_count() == before


def _ranges(n, unit, cap):
    """The rule as include/ital_prepare.h states it."""
    units = -(-n // unit)
    per = -(-units // min(cap, units))
    return -(-units // per), per * unit


def test_the_range_rule_and_the_workspace_sizes():
    lib = _lib.lib()
    su, sc, cu, cc = _lib.PREPARE_STATS_UNIT, _lib.PREPARE_STATS_CAP, _lib.PREPARE_COV_UNIT, _lib.PREPARE_COV_CAP
    for n in (1, su, su + 1, su * sc, su * sc + 1, 10 ** 6, 2 ** 31 - 1):
        count, rows = _ranges(n, su, sc)
        assert lib.ital_prepare_ranges(n, su, sc) == count <= sc and (count - 1) * rows < n <= count * rows
        assert lib.ital_col_stats_workspace(n, 7) == count * 3 * 7 * 8
    assert _ranges(su + 1, su, sc) == (2, su) and _ranges(su * sc + 1, su, sc) == ((sc + 2) // 2, 2 * su)
    assert [lib.ital_col_cov_cap(d) for d in (1, 512, 724, 725, 1024, 2048, 4096, 4097, 10 ** 4)] == [32, 32, 32, 31, 16, 4, 1, 1, 1]
    for n, d in ((1, 5), (cu + 1, 5), (cu * cc + 1, 3), (10 ** 6, 512), (10 ** 6, 2048)):
        count, _ = _ranges(n, cu, lib.ital_col_cov_cap(d))
        assert lib.ital_col_cov_workspace(n, d) == count * d * d * 8 and count <= 32
    assert lib.ital_col_cov_workspace(10 ** 6, 4096) <= 128 << 20
    for bad in ((-1, 5), (1 << 31, 5), (10, 0)):
        assert lib.ital_col_stats_workspace(*bad) == 0 and lib.ital_col_cov_workspace(*bad) == 0
    assert lib.ital_prepare_ranges(0, 128, 4) == 0 and lib.ital_prepare_ranges(5, 0, 4) == 0 and lib.ital_col_cov_cap(0) == 0


# ------------------------------------------------------------------------------------------------------ the checkers
def _data(n=150, d=20, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)) * (1.0 + np.arange(d) % 4) + 50.0        # a mean far from 0: centring matters
    X[7] = X[3]
    X[:, 2] = 0.375
    return X


def _fp64_answers(X, k=6):
    """What a correct FP64 implementation would give, formed by numpy in float64 (another order of summation)."""
    mean = X.sum(axis=0) / X.shape[0]
    Z = X - mean
    W = np.random.default_rng(4).normal(size=(X.shape[1], k))
    Y = np.zeros((X.shape[0], 16))
    Y[:, :k] = Z @ W
    return mean, Z.T @ Z, W, Y


def test_checkers_accept_a_correct_fp64_answer():
    X = _data()
    mean, C, W, Y = _fp64_answers(X)
    assert ref.check_stats(X.min(axis=0), X.max(axis=0), X.sum(axis=0), X) <= 1.0
    assert ref.check_cov((C + C.T) / 2, X, mean) <= 1.0
    assert ref.check_project(Y, X, mean, W) <= 1.0
    for code in (1, 2, 3):
        assert ref.check_project(ref.round_to(Y, code), X, mean, W, code) <= 1.0
    lo, span = np.full(20, X.min()), np.full(20, X.max() - X.min())
    S = np.zeros((150, 32))
    S[:, :20] = (X - lo) / span
    ref.check_scale(S, X, lo, span)
    ref.check_scale(ref.round_to(S, 2), X, lo, span, 2)
    nan = X.copy()
    nan[5, 1] = np.nan
    with np.errstate(invalid="ignore"):
        ref.check_stats(nan.min(axis=0), nan.max(axis=0), nan.sum(axis=0), nan)


def test_the_rounding_model():
    rng = np.random.default_rng(2)
    v = np.concatenate([rng.normal(size=4000) * np.exp(rng.normal(size=4000) * 9), [0.0, -0.0, np.inf, -np.inf, 65519.99, 65520.0,
                        2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1e-320]])
    with np.errstate(over="ignore"):
        assert ref.same_bits(ref.round_to(v, 2), v.astype(np.float16).astype(np.float64))       # numpy rounds f64 -> f16 once
        assert ref.same_bits(ref.round_to(v, 1), v.astype(np.float32).astype(np.float64))
    torch = pytest.importorskip("torch")
    f = v.astype(np.float32)                                    # f32 -> bf16 is one rounding in torch as well
    want = torch.from_numpy(f).to(torch.bfloat16).to(torch.float64).numpy()
    assert ref.same_bits(ref.round_to(f.astype(np.float64), 3), want)
    assert np.isnan(ref.round_to(np.array([np.nan]), 3)).all()
    assert (ref.half_ulp(np.array([1.0, 1.5, 2.0, 0.0, 1e-9]), 2) == [2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -25, 2.0 ** -25]).all()


def _mistakes():
    X = _data()
    mean, C, W, Y = _fp64_answers(X)
    C = (C + C.T) / 2
    n = X.shape[0]

    def dropped_row():
        z = X[-1] - mean
        ref.check_cov(C - np.outer(z, z), X, mean)

    def dropped_row_in_a_sum():
        ref.check_stats(X.min(axis=0), X.max(axis=0), X[:-1].sum(axis=0), X)

    def uncentred_pad_row():                                    # a masked row entered as 0 - mean
        ref.check_cov(C + np.outer(mean, mean), X, mean)

    def uncentred_moments():                                    # sum x x^T - n m m^T: cancellation, far outside the bound
        big = X + 1e6
        m = big.sum(axis=0) / n
        Cb = big.T @ big - n * np.outer(m, m)
        ref.check_cov((Cb + Cb.T) / 2, big, m)

    def transposed_tile():
        T = Y.copy()
        T[:6, :6] = T[:6, :6].T.copy()
        ref.check_project(T, X, mean, W)

    def transposed_tile_of_c():
        wrong = C.copy()
        wrong[10:, :10] = wrong[10:, :10].T.copy()               # the 10 x 10 block below the diagonal, written transposed
        ref.check_cov(wrong, X, mean)

    def asymmetric_in_the_last_bit():
        wrong = C.copy()
        wrong[5, 3] = np.nextafter(wrong[5, 3], np.inf)
        ref.check_cov(wrong, X, mean)

    def wrong_rounding_mode():
        ref.check_project(ref.trunc_to(Y, 2), X, mean, W, 2)

    def rounded_twice():                                        # through f32 first: off by more than half a unit somewhere
        v = np.zeros((1, 16))
        v[0, 0] = 1.0 + 2.0 ** -11 + 2.0 ** -30                 # f32 rounds it onto the tie, which then goes to even
        twice = ref.round_to(ref.round_to(v, 1), 2)
        ref.check_scale(twice, v[:, :1], np.zeros(1), np.ones(1), 2)

    def non_zero_pad_column():
        wrong = Y.copy()
        wrong[4, 9] = 1e-300
        ref.check_project(wrong, X, mean, W)

    def negative_zero_pad_column():
        wrong = Y.copy()
        wrong[4, 15] = -0.0
        ref.check_project(wrong, X, mean, W)

    def reciprocal_instead_of_division():
        lo, span = np.full(20, X.min()), np.full(20, X.max() - X.min())
        S = np.zeros((150, 32))
        S[:, :20] = (X - lo) * (1.0 / span)
        ref.check_scale(S, X, lo, span)

    def nan_ignored():
        nan = X.copy()
        nan[5, 1] = np.nan
        ref.check_stats(np.nanmin(nan, axis=0), np.nanmax(nan, axis=0), np.nansum(nan, axis=0), nan)

    return [dropped_row, dropped_row_in_a_sum, uncentred_pad_row, uncentred_moments, transposed_tile, transposed_tile_of_c,
            asymmetric_in_the_last_bit, wrong_rounding_mode, rounded_twice, non_zero_pad_column, negative_zero_pad_column,
            reciprocal_instead_of_division, nan_ignored]


@pytest.mark.parametrize("mistake", _mistakes(), ids=lambda fn: fn.__name__)
def test_checkers_reject(mistake):
    with pytest.raises(AssertionError):
        mistake()


# ------------------------------------------------------------------------------------------------------ principal_axes
def _matrices():
    rng = np.random.default_rng(21)
    G = rng.normal(size=(50, 20))
    yield "gram20", G.T @ G
    Q = np.linalg.qr(rng.normal(size=(64, 64)))[0]
    yield "decay64", (Q * 2.0 ** -np.arange(64)) @ Q.T
    Z = rng.normal(size=(300, 129)) * (1 + np.arange(129) % 5)
    Z -= Z.mean(axis=0)
    yield "cov129", Z.T @ Z / 299


# numpy.linalg.eigh's own worst values on these three matrices, measured with all d axes: max |W^T W - I| = 2.22e-15,
# max |C W - W diag(lambda)| / lambda_max = 3.91e-16.  Allowed: 8 x that.  These numbers are LAPACK's, not this project's.
ORTHO_TOL, RESIDUAL_TOL = 8 * 2.22e-15, 8 * 3.91e-16


@pytest.mark.parametrize("name,C", list(_matrices()), ids=lambda v: v if isinstance(v, str) else "")
def test_principal_axes(name, C):
    C = (C + C.T) / 2
    d = C.shape[0]
    for k in (1, 3, d):
        lam, W = principal_axes(C, k)
        assert lam.shape == (k,) and W.shape == (d, k) and W.flags.c_contiguous
        assert (np.diff(lam) <= 0).all() and np.array_equal(lam, np.linalg.eigh(C)[0][::-1][:k])
        assert np.abs(W.T @ W - np.eye(k)).max() <= ORTHO_TOL
        assert np.abs(C @ W - W * lam).max() / lam[0] <= RESIDUAL_TOL
        lead = np.argmax(np.abs(W), axis=0)
        assert (W[lead, np.arange(k)] > 0).all()


def test_principal_axes_sign_rule_ties_and_refusals():
    lam, W = principal_axes(np.diag([1.0, 3.0, 2.0]), 2)
    assert lam.tolist() == [3.0, 2.0] and W.tolist() == [[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]
    # the eigenvector (1, -1) / sqrt 2 has two entries of the same magnitude: the FIRST one decides, so it is made positive
    lam, W = principal_axes(np.array([[2.0, -1.0], [-1.0, 2.0]]), 2)
    assert lam.tolist() == [3.0, 1.0] and W[0, 0] > 0 > W[1, 0] and W[0, 1] > 0 and W[1, 1] > 0
    assert abs(W[0, 0]) == abs(W[1, 0])
    lam, W = principal_axes(-np.array([[2.0, -1.0], [-1.0, 2.0]]), 1)
    assert lam.tolist() == [-1.0] and (W > 0).all()
    lam, W = principal_axes(np.eye(3) * 5.0, 3)                 # a threefold eigenvalue: any orthonormal basis, signs by the rule
    assert lam.tolist() == [5.0] * 3 and np.abs(W.T @ W - np.eye(3)).max() <= ORTHO_TOL and (W.max(axis=0) > 0).all()
    for bad in (0, 4, 1.5, True):
        with pytest.raises(ValueError):
            principal_axes(np.eye(3), bad)
    with pytest.raises(ValueError):
        principal_axes(np.ones((3, 2)), 1)


# ------------------------------------------------------------------------------------------------------ Transform
def test_transform_round_trip_and_composition():
    rng = np.random.default_rng(7)
    X = rng.normal(size=(30, 6))
    S = Transform([(0, X.min(axis=0), X.max(axis=0) - X.min(axis=0))])
    P = Transform([(1, rng.normal(size=6), rng.normal(size=(6, 3)))])
    assert (S.d_in, S.d_out, P.d_in, P.d_out) == (6, 6, 6, 3)
    assert S.W is None and P.span is None and S.span.shape == (6,) and P.W.shape == (6, 3) and P.shift.shape == (6,)
    both = S.then(P)
    assert (both.d_in, both.d_out, len(both.steps)) == (6, 3, 2)
    assert np.array_equal(both.reference(X), P.reference(S.reference(X)))
    assert np.array_equal(S.reference(X), (X - S.shift) / S.span)
    with pytest.raises(AttributeError):
        both.shift
    with pytest.raises(ValueError):
        P.then(S)                                               # 3 columns into a step that reads 6
    for T in (S, P, both):
        state = T.state_dict()
        assert all(type(v) is np.ndarray for v in state.values())
        back = Transform.from_state_dict({key: v.copy() for key, v in state.items()})
        assert (back.d_in, back.d_out, len(back.steps)) == (T.d_in, T.d_out, len(T.steps))
        assert ref.same_bits(back.reference(X), T.reference(X))
    E = Transform(P.steps, eigenvalues=[3.0, 2.0, 0.5])
    back = Transform.from_state_dict(E.state_dict())
    assert back.eigenvalues.tolist() == [3.0, 2.0, 0.5] and P.eigenvalues is None and S.then(E).eigenvalues is None
    assert "eigenvalues" not in P.state_dict() and type(E.state_dict()["eigenvalues"]) is np.ndarray
    for steps, lam in ((P.steps, [1.0, 2.0]), (S.steps, np.ones(6)), (both.steps, np.ones(3))):
        with pytest.raises(ValueError):
            Transform(steps, eigenvalues=lam)
    state = S.state_dict()
    state["shift0"][0] = 99.0                                   # the state is a copy
    assert S.shift[0] != 99.0
    for bad in ([], [(0, np.zeros(3), np.ones(4))], [(1, np.zeros(3), np.ones((4, 2)))], [(2, np.zeros(3), np.ones(3))],
                [(1, np.zeros(600), np.ones((600, 513)))]):
        with pytest.raises(ValueError):
            Transform(bad)


def test_exports():
    import ital_amd
    for name in ("prepare", "column_stats", "MinMax", "PCA", "Transform", "principal_axes"):
        assert name in ital_amd.__all__ and getattr(ital_amd, name) is not None
    assert ital_amd.Transform is Transform and ital_amd.prepare.principal_axes is principal_axes


# ------------------------------------------------------------------------------------------------------ the reference's rule
def test_min_max_fixture_is_the_numpy_expression(golden_dir):
    z = np.load(os.path.join(golden_dir, "prepare_minmax.npz"))
    Xtr, Xte = z["X_train"], z["X_test"]
    assert Xtr.shape == (40, 5) and Xte.shape == (10, 5)
    assert Xte.min() < Xtr.min() and Xte.max() > Xtr.max()              # test rows outside the training range
    lo, hi = Xtr.min(), Xtr.max()
    T = Transform([(0, np.full(5, lo), np.full(5, hi - lo))])
    for src, want in ((Xtr, z["X_train_norm"]), (Xte, z["X_test_norm"])):
        assert ref.same_bits(T.reference(src), want) and ref.same_bits(ref.model_scale(src, T.shift, T.span), want)
    assert z["X_train_norm"].min() == 0.0 and z["X_train_norm"].max() == 1.0
    assert z["X_test_norm"].min() < 0.0 and z["X_test_norm"].max() > 1.0
