"""USDM without a device: header against binding, every refusal of the five entry points of include/ital_usdm.h (they come
before any HIP call), the NumPy restatement of tests/_usdm_ref.py against what the real reference recorded
(tests/golden/make_golden_usdm.py), the conditions of those fixtures, the LU checker on the model's own factor and on injected
mistakes, and the learner's refusals that need no device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _usdm_ref as ref  # noqa: E402

from ital_amd import _lib, build  # noqa: E402

NAMES = {"ital_usdm_laplacian", "ital_lu_factor", "ital_lu_solve", "ital_usdm_shift", "ital_symv_lower",
         "ital_symv_lower_workspace"}
ALL_FIXTURES = ref.FIXTURES + ("usdm_usps500_tol",)


# ------------------------------------------------------------------------------------------------------ ABI
def test_header_matches_the_binding():
    with open(os.path.join(ROOT, "include", "ital_usdm.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    assert set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", header)) == NAMES == set(_lib.USDM_SIGNATURES)
    for name in dir(_lib):
        if name.endswith("SIGNATURES") and name != "USDM_SIGNATURES":
            assert not set(_lib.USDM_SIGNATURES) & set(getattr(_lib, name)), name
    ptr = ctypes.c_void_p
    ctype = {"const double*": ptr, "double*": ptr, "const int64_t*": ptr, "const unsigned char*": ptr, "int*": ptr, "const int*": ptr,
             "hipStream_t": ptr, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for name, (res, args) in _lib.USDM_SIGNATURES.items():
        m = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)" % name, header)
        assert ctype[m.group(1)] is res, name
        params = [re.sub(r"\s*\w+$", "", p.strip()).replace(" *", "*") for p in m.group(2).split(",")]
        assert [ctype[p] for p in params] == args, (name, params)
    assert "usdm.hip" in build.SOURCES
    lib = _lib.lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes == _lib.USDM_SIGNATURES[name][1]


# fake, suitably aligned pointers: a refusal never touches them
P = 4096
VALID = {
    "ital_usdm_laplacian": dict(idx=P, k=5, n=10, u=P, n_u=6, pos=P, rel=P, n_rel=2, eps=1e-6, M=P, ld=6, rhs=P, stream=0),
    "ital_lu_factor": dict(A=P, n=10, ld=10, info=P, status=P, stream=0),
    "ital_lu_solve": dict(LU=P, n=10, ld=10, y=P, info=P, stream=0),
    "ital_usdm_shift": dict(K=P, n=10, ldk=10, mu=1e-6, B=P, ldb=10, stream=0),
    "ital_symv_lower": dict(K=P, n=10, ld=10, x=P, out=P, work=P, work_doubles=64, stream=0),
}
BIG = (1 << 31) - 128
REFUSALS = {
    "ital_usdm_laplacian": [dict(k=0), dict(k=33), dict(n=-1), dict(n=BIG), dict(n_u=-1), dict(n_u=11), dict(n_rel=-1),
                            dict(n_rel=11), dict(ld=5), dict(idx=0), dict(u=0), dict(pos=0), dict(rel=0), dict(M=0), dict(rhs=0),
                            dict(idx=P + 4), dict(u=P + 4), dict(pos=P + 4), dict(M=P + 4), dict(rhs=P + 4)],
    "ital_lu_factor": [dict(n=-1), dict(n=BIG, ld=BIG), dict(ld=9), dict(A=0), dict(info=0), dict(status=0), dict(A=P + 4),
                       dict(info=P + 2), dict(status=P + 2), dict(n=6000000, ld=6000000)],
    "ital_lu_solve": [dict(n=-1), dict(n=BIG, ld=BIG), dict(ld=9), dict(LU=0), dict(y=0), dict(LU=P + 4), dict(y=P + 4),
                      dict(info=P + 2)],
    "ital_usdm_shift": [dict(n=-1), dict(n=BIG, ldk=BIG, ldb=BIG), dict(ldk=9), dict(ldb=9), dict(K=0), dict(B=0), dict(K=P + 4),
                        dict(B=P + 4)],
    "ital_symv_lower": [dict(n=-1), dict(n=BIG, ld=BIG), dict(ld=9), dict(K=0), dict(x=0), dict(out=0), dict(work=0),
                        dict(K=P + 4), dict(x=P + 4), dict(out=P + 4), dict(work=P + 4), dict(work_doubles=63),
                        dict(n=65, ld=65, work_doubles=2 * 2 * 64 - 1)],
}


def _call(name, **over):
    a = dict(VALID[name])
    a.update(over)
    return getattr(_lib.lib(), name)(*a.values())


@pytest.mark.parametrize("name,over", [(n, o) for n in REFUSALS for o in REFUSALS[n]],
                         ids=lambda v: v if isinstance(v, str) else ",".join("%s=%s" % kv for kv in v.items()))
def test_refusals_come_before_any_hip_call(name, over):
    assert _call(name, **over) == -22
    assert _lib.lib().ital_last_error().decode().startswith(name + ": ")


def test_no_rows_is_no_work_and_the_workspace_size():
    assert _call("ital_usdm_laplacian", n_u=0, ld=0, u=0, M=0, rhs=0) == 0
    assert _call("ital_usdm_laplacian", n=0, n_u=0, n_rel=0, ld=0, idx=0, u=0, pos=0, rel=0, M=0, rhs=0) == 0
    assert _call("ital_lu_factor", n=0, ld=0, A=0, info=0, status=0) == 0
    assert _call("ital_lu_solve", n=0, ld=0, LU=0, y=0, info=0) == 0
    assert _call("ital_usdm_shift", n=0, ldk=0, ldb=0, K=0, B=0) == 0
    assert _call("ital_symv_lower", n=0, ld=0, K=0, x=0, out=0, work=0, work_doubles=0) == 0
    ws = _lib.lib().ital_symv_lower_workspace
    assert [ws(n) for n in (-1, 0, 1, 64, 65, 300, BIG)] == [0, 0, 64, 64, 256, 25 * 64, 0]


# ------------------------------------------------------------------------------------------------ the reference's record
@pytest.fixture(scope="module", params=ALL_FIXTURES)
def fixture(request):
    return request.param, ref.load(request.param)


def test_the_fixtures_the_issue_names_exist():
    for name in ref.FIXTURES:
        assert os.path.exists(os.path.join(ref.GOLDEN, name + ".npz")), name


def test_fixture_conditions(fixture):
    name, z = fixture
    ref.check_fixture_conditions(z)
    its = [int(z["r%d_iterations" % r]) for r in range(int(z["rounds"]))]
    assert its == ([100] * 3 if name == "usdm_usps500_tol" else [2] * 3)


def test_restatement_reproduces_the_reference(fixture):
    _, z = fixture
    o = ref.options(z)
    X = z["X"]
    K = ref.kernel(X, o["length_scale"], o["var"])
    nb = ref.neighbours(K, o["knn"])
    assert np.array_equal(nb, z["r0_neighbours"])
    A = ref.laplacian_matrix(nb, len(X))
    ids = ({int(z["query"])}, set(), set())
    for r in range(int(z["rounds"])):
        p = "r%d_" % r
        out = ref.fetch(K, A, *ids, int(z["k"]), o["r"], o["max_iter"], o["tol"])
        assert np.array_equal(out["u"], z[p + "u"])
        assert out["iterations"] == int(z[p + "iterations"])
        # K is formed here by BLAS where the reference's gp.py forms it: alternative (b) of the generator covers that
        for key, spread in (("prob", "spread_prob"), ("f", "spread_f"), ("objectives", "spread_obj")):
            tol = float(z[p + spread]) + 8 * ref.U * np.max(np.abs(z[p + key]))
            assert np.max(np.abs(out[key] - z[p + key])) <= tol, (r, key)
        # |db / dprob| = r |log(prob / (1 - prob))| / log 2 <= r log(1e8) / log 2 < 27 r on the clipped range
        tol_b = 27 * o["r"] * float(z[p + "spread_prob"]) + 8 * ref.U * np.max(np.abs(z[p + "b"]))
        assert np.max(np.abs(out["b"] - z[p + "b"])) <= tol_b, r
        assert set(out["picks"].tolist()) == set(z[p + "ret"].tolist())
        for i, v in ref.feedback(z, r).items():
            ids[0 if v > 0 else 1 if v < 0 else 2].add(i)


# ------------------------------------------------------------------------------------------------------ the checkers
def _lap_case(n=40, k=5, seed=2):
    rng = np.random.default_rng(seed)
    idx = ref.random_graph(n, k, rng)
    lab = rng.permutation(n)[:7]
    u = np.setdiff1d(np.arange(n), lab)
    pos = np.full(n, -1, dtype=np.int64)
    pos[u] = np.arange(len(u))
    rel = np.zeros(n, dtype=np.uint8)
    rel[lab[:3]] = 1
    return idx, k, n, u, pos, rel


def test_model_laplacian_is_the_reference_matrix():
    idx, k, n, u, pos, rel = _lap_case()
    M, rhs = ref.model_laplacian(idx, k, n, u, pos, rel, int(rel.sum()))
    A = ref.laplacian_matrix(idx, n)
    lab = np.flatnonzero(pos < 0)
    assert np.allclose(M, A[np.ix_(u, u)], rtol=1e-15, atol=0)
    assert np.allclose(rhs, -A[np.ix_(u, lab)] @ rel[lab].astype(np.float64), rtol=1e-13, atol=0)
    assert (np.abs(M).sum(axis=1) - 2 * np.diag(M) < 0).all()         # strictly dominant by rows


def test_model_shift_and_symv():
    rng = np.random.default_rng(0)
    K = rng.normal(size=(9, 9))
    B = ref.model_shift(K, 1e-6)
    assert B[4, 2] == K[4, 2] + 1e-6 and B[3, 3] == (K[3, 3] + 1e-6) + 1e-6 and np.isnan(B[2, 4])
    S = np.tril(K) + np.tril(K, -1).T
    x = rng.normal(size=9)
    assert np.allclose(np.asarray(ref.model_symv(K, x), dtype=np.float64), S @ x)
    ref.check_symv(K, x, S @ x)
    bad = S @ x
    bad[3] *= 1 + 1e-10
    with pytest.raises(AssertionError):
        ref.check_symv(K, x, bad)


def test_lu_checker_accepts_the_model_and_rejects_mistakes():
    rng = np.random.default_rng(1)
    A = ref.dominant_matrix(70, rng, 1e-3)
    LU, info = ref.ld_lu(A)
    LU = np.asarray(LU, dtype=np.float64)
    assert info == 0
    assert ref.check_lu(A, LU, 0, 0, 0) <= 1.0
    b = rng.normal(size=70)
    x = np.asarray(ref.ld_lu_apply(LU, b), dtype=np.float64)
    assert ref.check_lu_solve(A, LU, b, x) <= 1.0

    def off(m):
        m[40, 12] *= 1 + 1e-10

    def swapped(m):
        m[5, 9], m[9, 5] = m[9, 5], m[5, 9]

    def stale_upper(m):
        m[np.triu_indices(70, 1)] = A[np.triu_indices(70, 1)]

    for mistake in (off, swapped, stale_upper):
        wrong = LU.copy()
        mistake(wrong)
        with pytest.raises(AssertionError):
            ref.check_lu(A, wrong, 0, 0, 0)
    xw = x.copy()
    xw[11] *= 1 + 1e-10
    with pytest.raises(AssertionError):
        ref.check_lu_solve(A, LU, b, xw)
    # failure paths: the column and the status bit
    Z = A.copy()
    Z[0, 0] = 0.0
    assert ref.ld_lu(Z)[1] == 1
    ref.check_lu(Z, Z, 1, 2, 3, expect_info=1)
    with pytest.raises(AssertionError):
        ref.check_lu(Z, Z, 1, 2, 2, expect_info=1)            # a missing status
    with pytest.raises(AssertionError):
        ref.check_lu(Z, Z, 2, 2, 3, expect_info=1)            # the wrong column
    with pytest.raises(AssertionError):
        ref.check_lu(A, LU, 0, 0, 1)                          # a status set on a matrix that factors


# ------------------------------------------------------------------------------------------------------ the learner
def test_exported_but_not_registered():
    import ital_amd
    from ital_amd import competitors, harness
    assert "USDM" in ital_amd.__all__
    assert ital_amd.USDM.__name__ == "USDM"
    assert "USDM" not in competitors.LEARNERS
    assert "USDM" in harness.BASELINES
    assert "USDM" not in harness._learners()
    with pytest.raises(NotImplementedError, match="baseline") as e:
        harness.make_learner("USDM", None, {})
    assert "SUD and USDM" in str(e.value)


def test_refusals_without_a_device():
    from ital_amd import USDM
    with pytest.raises(NotImplementedError, match="row shards"):
        USDM(None, world=2)
    with pytest.raises(NotImplementedError, match="queries"):
        USDM(None, queries=[np.zeros(3)])
    for knn in (0, 33, 2.5, True):
        with pytest.raises(ValueError, match="1..32"):
            USDM(None, knn=knn)
    learner = USDM(None, knn=3, r=2.0, max_iter=7, tol=1e-3)
    assert (learner.knn, learner.r, learner.max_iter, learner.tol, learner.last) == (3, 2.0, 7, 1e-3, None)


def test_entropy_term_is_the_reference_expression():
    from ital_amd.usdm import usdm_entropy_term
    z = ref.load("usdm_synth150_knn3_r2")
    assert np.array_equal(usdm_entropy_term(z["r1_prob"], float(z["r"])), z["r1_b"])
