"""Host side of TCAL and RBMAL (no device): the C declaration of include/ital_cosine.h against its binding and its argument
checks; kernel k-means and the pure selection functions of ital_amd/competitors.py against what the real reference recorded
(tests/golden/make_golden_competitors.py); the extended-precision model of ital_cosine_min's DEFINITION against scipy, and
the model's checker against injected mistakes; the registration of the two learners."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _competitors_ref as ref  # noqa: E402


# ------------------------------------------------------------------------------------------------------ ABI
def _ctype_of(decl):
    decl = decl.strip()
    if "*" in decl:
        return ctypes.c_void_p
    base = " ".join(w for w in decl.split()[:-1] if w != "const")
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "hipStream_t": ctypes.c_void_p}[base]


def test_cosine_declaration_equals_binding():
    from ital_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "ital_cosine.h")).read()
    assert set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", header)) == {"ital_cosine_min"} == set(_lib.COSINE_SIGNATURES)
    m = re.search(r"\bint\s+ital_cosine_min\s*\(([^)]*)\)\s*;", header)
    assert m
    res, args = _lib.COSINE_SIGNATURES["ital_cosine_min"]
    assert res is ctypes.c_int and [_ctype_of(a) for a in m.group(1).split(",")] == args
    assert "cosine.hip" in build.SOURCES
    fn = _lib.lib().ital_cosine_min                  # load() binds every table: the library exports the symbol
    assert fn.argtypes == args and fn.restype is res
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "ital_cosine.h":
            assert "ital_cosine" not in open(os.path.join(ROOT, "include", name)).read(), name


def test_cosine_header_is_c99_and_cxx11(tmp_path):
    text = ('#include "ital_cosine.h"\n'
            "typedef int (*cos_fn)(const void*, int, const double*, int64_t, int, const double*, const double*, int, int, double*,\n"
            "                      hipStream_t);\n"
            "cos_fn use_cosine = ital_cosine_min;\n"
            "int main(void) { return ITAL_INGEST_F64 == 0 ? 0 : 1; }\n")
    for cc, std, name in (("gcc", "-std=c99", "use_cosine.c"), ("g++", "-std=c++11", "use_cosine.cpp")):
        unit = tmp_path / name
        unit.write_text(text)
        r = subprocess.run([cc, std, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(unit)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_cosine_refuses_bad_arguments_without_touching_the_device():
    """Fake pointers that are never followed: every case is decided before any HIP call."""
    from ital_amd import _lib
    lib = _lib.lib()
    P = 4096

    def refused(rc):
        assert rc == -22
        assert "ital_cosine_min" in lib.ital_last_error().decode()

    call = lib.ital_cosine_min
    refused(call(P, 0, P, -1, 16, P, P, 1, 0, P, None))              # n < 0
    refused(call(P, 0, P, 5, 16, P, P, 0, 0, P, None))               # c < 1
    refused(call(P, 0, P, 5, 16, P, P, -3, 0, P, None))
    refused(call(P, 0, P, 5, 0, P, P, 1, 0, P, None))                # ldx
    refused(call(P, 0, P, 5, -16, P, P, 1, 0, P, None))
    refused(call(P, 0, P, 5, 24, P, P, 1, 0, P, None))
    for slot in (0, 2, 5, 6, 9):                                      # a NULL pointer with n > 0
        a = [P, 0, P, 5, 16, P, P, 1, 0, P, None]
        a[slot] = None
        refused(call(*a))
    refused(call(P, 4, P, 5, 16, P, P, 1, 0, P, None))               # unknown element type
    refused(call(P, -1, P, 5, 16, P, P, 1, 0, P, None))
    refused(call(P + 8, 0, P, 5, 16, P, P, 1, 0, P, None))           # X not aligned to 16 B
    refused(call(P + 2, 2, P, 5, 16, P, P, 1, 0, P, None))
    assert call(None, 0, None, 0, 16, None, None, 1, 0, None, None) == 0       # n == 0: nothing to do, no launch
    assert call(P, 3, P, 0, 32, P, P, 7, 1, P, None) == 0


# ------------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("name", ref.TCAL_FIXTURES + ref.RBMAL_FIXTURES)
def test_committed_fixture_meets_the_generators_condition(name):
    """Every recorded decision margin is an exact tie or at least 1e-9; the picks are those of the real reference."""
    z, X = ref.load(name)
    assert os.path.getsize(os.path.join(ref.GOLD, name + ".npz")) <= 1 << 20
    rounds = int(z["rounds"])
    assert rounds == 3
    margins = [key for key in z.files if "_margin_" in key]
    kinds = {"partition", "kmeans", "density"} if name.startswith("tcal") else {"argmax"}
    assert {key.split("_margin_")[1] for key in margins} == kinds and len(margins) == rounds * len(kinds)
    for key in margins:
        gap = float(z[key])
        assert gap == 0.0 or gap >= ref.MARGIN, (key, gap)
    want = {"tcal_synth150": [[91, 70, 57, 2], [108, 84, 138, 86], [132, 121, 82, 51]],
            "tcal_usps500": [[49, 137, 386, 282], [16, 129, 180, 174], [251, 222, 48, 279]],
            "tcal_synth60_retry": [[35, 34, 47], [55, 4], [15, 10]],
            "rbmal_synth150": [[91, 70, 10], [57, 94, 80], [54, 47, 132]],
            "rbmal_usps500": [[134, 78, 80, 422], [435, 451, 450, 486], [436, 353, 352, 326]],
            "rbmal_butterflies": [[901, 491, 917], [202, 532, 995], [683, 848, 154]]}[name]
    assert [z["r%d_ret" % r].tolist() for r in range(rounds)] == want
    # the margins are what the stored vectors show
    for r in range(rounds):
        p = "r%d_" % r
        if name.startswith("tcal"):
            a = np.sort(np.abs(z[p + "rel_mean"][z[p + "cand"]]))
            m = len(z[p + "unc"])
            assert float(z[p + "margin_partition"]) == a[m] - a[m - 1]
            gaps = [np.diff(np.sort(z[p + "dens%d" % i])[:2]) for i in range(int(z[p + "labels"].max()) + 1)]
            assert float(z[p + "margin_density"]) == min(float(g[0]) for g in gaps if len(g))
        else:
            gaps = [np.diff(np.sort(z[p + "s%d_scores" % t])[-2:])[0] for t in range(len(z[p + "alpha"]))]
            assert float(z[p + "margin_argmax"]) == min(gaps)


# ------------------------------------------------------------------------------------------------------ kernel k-means
@pytest.mark.parametrize("name", ref.TCAL_FIXTURES)
def test_kernel_kmeans_reproduces_the_recorded_clusterings(name):
    """From the recorded K, generator state and k: the recorded labels, a ValueError where the reference raised one, and
    the recorded generator state afterwards."""
    from ital_amd._kernel_kmeans import kernel_kmeans
    z, _ = ref.load(name)
    saved = np.random.get_state()
    try:
        retries = 0
        for r in range(int(z["rounds"])):
            p = "r%d_" % r
            np.random.set_state(ref.rng_state(z, p + "rng_before"))
            k = int(z["k"])
            for _ in range(int(z[p + "clusterings"]) - 1):
                with pytest.raises(ValueError):
                    kernel_kmeans(z[p + "K"], k)
                k -= 1
                retries += 1
            labels = kernel_kmeans(z[p + "K"], k)
            assert np.array_equal(labels, z[p + "labels"])
            assert ref.same_rng_state(z, p + "rng_after")
        assert (retries > 0) == (name == "tcal_synth60_retry")
    finally:
        np.random.set_state(saved)


def test_kernel_kmeans_takes_its_own_generator_and_leaves_the_global_one_alone():
    from ital_amd._kernel_kmeans import kernel_kmeans
    z, _ = ref.load("tcal_synth150")
    before = np.random.get_state()
    a = kernel_kmeans(z["r0_K"], 3, rng=np.random.RandomState(5))
    b = kernel_kmeans(z["r0_K"], 3, rng=np.random.RandomState(5))
    assert np.array_equal(a, b) and set(a) == {0, 1, 2}
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    with pytest.raises(ValueError):
        kernel_kmeans(np.eye(2), 3, rng=np.random.RandomState(0))       # three clusters of two samples: one is empty


# ------------------------------------------------------------------------------------------------------ selection functions
@pytest.mark.parametrize("name", ref.TCAL_FIXTURES)
def test_tcal_selection_reproduces_the_recorded_picks(name):
    from ital_amd.competitors import tcal_select, tcal_uncertain
    z, _ = ref.load(name)
    k = int(z["k"])
    factor = int(z["kw_unc_factor"]) if "kw_unc_factor" in z.files else 4
    saved = np.random.get_state()
    try:
        for r in range(int(z["rounds"])):
            p = "r%d_" % r
            unc = tcal_uncertain(z[p + "rel_mean"], z[p + "cand"], factor * k)
            assert np.array_equal(unc, z[p + "unc"])                     # numpy's own order within the first m
            np.random.set_state(ref.rng_state(z, p + "rng_before"))
            info = {}
            picks = tcal_select(z[p + "K"], k, info=info)
            assert unc[picks].tolist() == z[p + "ret"].tolist()
            assert all(type(i) is int for i in picks)
            assert info["clusterings"] == int(z[p + "clusterings"]) and len(picks) == k - info["clusterings"] + 1
            assert np.array_equal(info["labels"], z[p + "labels"])
            for i, dens in enumerate(info["densities"]):
                np.testing.assert_allclose(dens, z[p + "dens%d" % i], rtol=0, atol=1e-12)
            assert ref.same_rng_state(z, p + "rng_after")
    finally:
        np.random.set_state(saved)


def test_tcal_selection_edge_cases():
    from ital_amd.competitors import tcal_select, tcal_uncertain
    with pytest.raises(ValueError):
        tcal_uncertain(np.linspace(-1, 1, 20), np.arange(7), 8)           # m > len(cand): numpy's own error
    assert sorted(tcal_uncertain(np.array([0.5, -0.1, 0.05, -0.2]), np.array([0, 1, 3]), 2).tolist()) == [1, 3]
    # a cluster of two is an exact tie on a symmetric K: its first member is taken
    K = np.array([[1.0, 0.3], [0.3, 1.0]])
    info = {}
    assert tcal_select(K, 1, rng=np.random.RandomState(0), info=info) == [0]
    assert info["densities"][0][0] == info["densities"][0][1]
    # one sample, asked for two clusters: the second is always empty, one cluster is left
    info = {}
    assert tcal_select(np.array([[1.0]]), 2, rng=np.random.RandomState(1), info=info) == [0]
    assert info["clusterings"] >= 1 and len(info["densities"]) == 1


@pytest.mark.parametrize("name", ref.RBMAL_FIXTURES)
def test_rbmal_selection_reproduces_the_recorded_picks(name):
    from ital_amd.competitors import rbmal_select
    z, _ = ref.load(name)
    k = int(z["k"])
    for r in range(int(z["rounds"])):
        p = "r%d_" % r
        cand = z[p + "cand"]
        steps = []
        picks = rbmal_select(z[p + "dist"][cand], z[p + "unc"][cand], len(z[p + "train"]), k, steps)
        assert cand[picks].tolist() == z[p + "ret"].tolist()
        assert len(picks) == k - 1 and all(type(i) is int for i in picks)              # k - 1, as the reference
        assert [s[0] for s in steps] == z[p + "alpha"].tolist()
        for t, (_, scores, _) in enumerate(steps):
            assert np.array_equal(scores, z[p + "s%d_scores" % t])                      # the same expression on the same inputs


def test_rbmal_selection_edge_cases():
    from ital_amd.competitors import rbmal_select, rbmal_uncertainty
    dist, unc = np.array([0.3, 0.1, 0.7]), np.array([0.2, 0.9, 0.1])
    assert rbmal_select(dist, unc, 2, 1) == [] and rbmal_select(dist, unc, 2, 0) == []
    assert len(rbmal_select(dist, unc, 2, 3)) == 2
    assert sorted(rbmal_select(dist, unc, 2, 9)) == [0, 1, 2]                           # the list runs empty
    with pytest.raises(ValueError):
        rbmal_select(dist[:0], unc[:0], 2, 2)                                            # argmax of an empty sequence
    u = rbmal_uncertainty(np.array([0.0, 5.0, -5.0]), np.array([1.0, 1.0, 1.0]), 1e-6)
    assert u[0] == 1.0 and u[1] < 1e-5 and abs(u[1] - u[2]) < 1e-12


# ------------------------------------------------------------------------------------------------------ model of the kernel
def _cases(seed):
    rng = np.random.default_rng(seed)
    d = 37
    X, T = rng.random((40, d)) - 0.3, rng.random((9, d)) - 0.3
    X[3] = 0.0                       # a zero row: NaN
    X[5] = T[4]                      # a row equal to a train row: distance 0 up to rounding
    X[7] *= 1e-200                   # its squared norm underflows to 0, the dot product does not: inf, clipped to 1
    X[8] = -T[2]
    return X, T


def test_model_of_the_definition_agrees_with_scipy():
    from scipy.spatial.distance import cdist
    for seed, scale_train in ((0, False), (1, True)):
        X, T = _cases(seed)
        if scale_train:
            T[6] *= 1e-200           # both norms and the dot product underflow for row 7: 0 / 0
        d = X.shape[1]
        xn, tn = (X * X).sum(1), (T * T).sum(1)
        want = cdist(X, T, "cosine").min(axis=-1)
        assert np.isnan(want[3]) and want[5] <= ref.bound(d)
        assert np.isnan(want[7]) == scale_train
        ratio = ref.check(want, X, xn, T, tn, d)
        assert ratio <= 1.0
        pair = ref.pair_model(X, xn, T, tn)
        assert pair[7, 0] in (0, 2) and pair[8, 2] >= 2 - ref.bound(d)


def _mistaken(kind, X, xn, T, tn, c, prev):
    """An implementation of ital_cosine_min over the first c rows of T with one mistake built in (float64)."""
    d = ref.pair_model(X, xn, T, tn).astype(np.float64)
    if kind == "extra_row":
        out = d[:, :c + 1].min(axis=1)                       # a row of T past c enters the minimum
    elif kind == "fmin":
        with np.errstate(all="ignore"):
            out = np.fmin.reduce(d[:, :c], axis=1)           # drops NaN instead of keeping it
    elif kind == "no_clip":
        ld = np.longdouble
        with np.errstate(all="ignore"):
            cos = (np.asarray(X, dtype=ld) @ np.asarray(T[:c], dtype=ld).T) / (np.sqrt(xn.astype(ld))[:, None] * np.sqrt(tn[:c].astype(ld)))
            out = (1 - cos).min(axis=1).astype(np.float64)
    elif kind == "no_accumulate":
        return d[:, :c].min(axis=1)
    elif kind == "off_by_1e-12":
        out = d[:, :c].min(axis=1) * (1 + 1e-12)             # an error far above the rounding of any summation order
    else:
        out = d[:, :c].min(axis=1)
    return out if prev is None else np.minimum(prev, out)


def test_checker_rejects_injected_mistakes():
    X, T = _cases(2)
    T[8] = X[11] * 3.0                                       # the row past c is the nearest of row 11
    c = 8
    xn, tn = (X * X).sum(1), (T * T).sum(1)
    prev = np.full(len(X), 2.0)
    prev[20] = 0.0
    prev[21] = np.nan
    for p in (None, prev):
        assert ref.check(_mistaken("none", X, xn, T, tn, c, p), X, xn, T[:c], tn[:c], X.shape[1], p) <= 1.0
    for kind, p in (("extra_row", None), ("no_clip", None), ("no_accumulate", prev), ("off_by_1e-12", None)):
        with pytest.raises(AssertionError):
            ref.check(_mistaken(kind, X, xn, T, tn, c, p), X, xn, T[:c], tn[:c], X.shape[1], p)
    # one NaN pair among finite ones (both norms and the dot product of row 7 with train row 6 underflow): np.min keeps it
    T[6] *= 1e-200
    tn = (T * T).sum(1)
    assert np.isnan(ref.model(X, xn, T[:c], tn[:c])[7])
    assert ref.check(_mistaken("none", X, xn, T, tn, c, None), X, xn, T[:c], tn[:c], X.shape[1]) <= 1.0
    with pytest.raises(AssertionError):
        ref.check(_mistaken("fmin", X, xn, T, tn, c, None), X, xn, T[:c], tn[:c], X.shape[1])
    with pytest.raises(AssertionError):                      # and the accumulated NaN
        ref.check(np.fmin(prev, _mistaken("none", X, xn, T, tn, c, None)), X, xn, T[:c], tn[:c], X.shape[1], prev)


# ------------------------------------------------------------------------------------------------------ registration
def test_learners_are_registered_and_the_rest_stays_refused(tmp_path):
    import ital_amd
    from ital_amd import RBMAL, TCAL, harness
    table = harness._learners()
    assert table["TCAL"] is TCAL and table["RBMAL"] is RBMAL
    assert "TCAL" in ital_amd.__all__ and "RBMAL" in ital_amd.__all__
    assert set(harness.BASELINES) == {"SUD", "RBMAL", "TCAL", "USDM"}
    for method in ("USDM", "SUD"):
        with pytest.raises(NotImplementedError, match="baseline") as e:
            harness.make_learner(method, None, {})
        assert "SUD and USDM" in str(e.value)
    import inspect
    assert "unc_factor" in inspect.signature(TCAL.__init__).parameters
    assert TCAL(None).unc_factor == 4 and RBMAL(None).gp is None                         # no data: no device is touched
