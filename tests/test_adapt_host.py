"""Host side of the AdaptAL learner (no device): the C declarations of include/ital_adapt.h against their bindings, the
argument checks of the three entry points, the learner's registration, and the acceptance rule of
tests/golden/make_golden_adapt.py restated on the stored vectors of every committed fixture."""
import ctypes
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")

ADAPT = ["ital_chol_inv_diag", "ital_chol_inv_diag_workspace", "ital_adapt_scores", "ital_adapt_error"]
FIXTURES = ["adapt_usps600_q3", "adapt_usps600_q17", "adapt_usps2007_sub500", "adapt_synth300_k6", "adapt_synth300_betas",
            "adapt_synth300_b1"]


def _ctype_of(decl):
    decl = decl.strip()
    if "*" in decl:
        return ctypes.c_void_p
    base = " ".join(w for w in decl.split()[:-1] if w != "const")
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "hipStream_t": ctypes.c_void_p}[base]


def test_adapt_declarations_equal_bindings():
    from ital_amd import _lib
    header = open(os.path.join(ROOT, "include", "ital_adapt.h")).read()
    assert set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", header)) == set(ADAPT) == set(_lib.ADAPT_SIGNATURES)
    for other in (_lib.SIGNATURES, _lib.CTX_SIGNATURES, _lib.DENSE_SIGNATURES):
        assert not set(ADAPT) & set(other)
    for name in ADAPT:
        m = re.search(r"\b(int|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        res = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}[m.group(1)]
        args = [_ctype_of(a) for a in m.group(2).split(",")]
        want_res, want_args = _lib.ADAPT_SIGNATURES[name]
        assert res is want_res, name
        assert args == want_args, name
    lib = _lib.lib()                                   # load() resolves every table: the library exports them
    for name in ADAPT:
        assert getattr(lib, name).argtypes == _lib.ADAPT_SIGNATURES[name][1]


def test_entry_points_refuse_bad_arguments_without_touching_the_device():
    """Every refusal is -22 with a message that names the entry point; empty problems return 0."""
    from ital_amd import _lib
    lib = _lib.lib()

    def refused(rc, name):
        assert rc == -22
        assert name in lib.ital_last_error().decode()

    assert lib.ital_chol_inv_diag_workspace(0) == 0 and lib.ital_chol_inv_diag_workspace(-3) == 0
    assert lib.ital_chol_inv_diag_workspace(1) == 2 * 16 + 16
    assert lib.ital_chol_inv_diag_workspace(65) == 2 * 65 * 80 + 2 * 80
    assert lib.ital_chol_inv_diag(None, 0, 0, None, None, 0, None, None) == 0
    refused(lib.ital_chol_inv_diag(None, -1, 0, None, None, 0, None, None), "ital_chol_inv_diag")
    refused(lib.ital_chol_inv_diag(None, 4, 4, None, None, 0, None, None), "ital_chol_inv_diag")          # null L / out
    refused(lib.ital_chol_inv_diag(8, 4, 3, 8, 8, 1 << 20, None, None), "ital_chol_inv_diag")             # ld < n
    refused(lib.ital_chol_inv_diag(8, 4, 4, 8, None, 1 << 20, None, None), "ital_chol_inv_diag")          # no work
    refused(lib.ital_chol_inv_diag(8, 4, 4, 8, 8, 2 * 4 * 16 + 15, None, None), "ital_chol_inv_diag")     # work too small

    assert lib.ital_adapt_scores(None, None, None, 0, 1.0, None, None, None) == 0
    refused(lib.ital_adapt_scores(None, None, None, -1, 1.0, None, None, None), "ital_adapt_scores")
    refused(lib.ital_adapt_scores(8, 8, None, 5, 1.0, 8, 8, None), "ital_adapt_scores")

    assert lib.ital_adapt_error(None, 0, None, 0, 0, None, None, 1e-6, None, None, None) == 0
    refused(lib.ital_adapt_error(8, 16, 8, -1, 10, 8, 8, 1e-6, 8, 8, None), "ital_adapt_error")
    refused(lib.ital_adapt_error(8, 16, 8, 3, 0, 8, 8, 1e-6, 8, 8, None), "ital_adapt_error")             # no candidates
    refused(lib.ital_adapt_error(8, 16, 8, 11, 10, 8, 8, 1e-6, 8, 8, None), "ital_adapt_error")           # r > nc
    refused(lib.ital_adapt_error(8, 9, 8, 3, 10, 8, 8, 1e-6, 8, 8, None), "ital_adapt_error")             # ldc < nc
    refused(lib.ital_adapt_error(8, 16, None, 3, 10, 8, 8, 1e-6, 8, 8, None), "ital_adapt_error")         # null rows


def test_learner_is_registered():
    from ital_amd import harness
    assert "AdaptAL" not in harness.BASELINES
    assert set(harness.BASELINES) == {"SUD", "RBMAL", "TCAL", "USDM"}
    from ital_amd import AdaptAL
    assert harness._learners()["AdaptAL"] is AdaptAL
    import ital_amd
    assert "AdaptAL" in ital_amd.__all__
    assert AdaptAL.max_gram_bytes > 0


def _sensitivities(mean, var):
    from scipy.stats import norm
    sd = np.sqrt(var)
    z = -mean / sd
    p = np.clip(norm.cdf(z), 1e-8, 1 - 1e-8)
    dHdp = np.log((1 - p) / p)
    return np.abs(dHdp * norm.pdf(z) / sd), np.abs(dHdp * norm.pdf(z) * mean / (2 * sd ** 3))


@pytest.mark.parametrize("name", FIXTURES)
def test_committed_fixture_meets_the_generators_condition(name):
    """(a) every beta's top k is separated from the rest by 100 times the first-order effect of the tests' tolerances on
    the scores; (b) neighbouring values of the sorted error vector differ by more than 1e-6 relative; (c) the entropy's
    sensitivity to mean and variance is at most 2.  A fixture written by a loosened generator or edited by hand fails."""
    path = os.path.join(GOLD, name + ".npz")
    assert os.path.getsize(path) <= 1 << 20
    z = np.load(path)
    betas = z["betas"]
    assert int(z["rounds"]) == 3
    early = 0
    for r in range(int(z["rounds"])):
        p = "r%d_" % r
        mean, var, ent, den, err = z[p + "mean"], z[p + "var"], z[p + "entropy"], z[p + "density"], z[p + "err"]
        k = min(int(z["k"]), len(ent))
        tol_den = max(1e-14 * float(z[p + "cond"]), 10 * float(z[p + "den_ref_vs_lapack"]))
        dm, dv = _sensitivities(mean, var)
        assert (dm + dv).max() <= 2                                                         # (c)
        dH = 2e-9 * (dm + dv)
        picked = []
        for beta in betas:                                                                  # (a)
            s = (ent ** beta) * (den ** (1. - beta))
            e = s * (beta * dH / ent + (1 - beta) * tol_den / den)
            sel = np.argpartition(-s, k - 1)[:k]
            rest = np.setdiff1d(np.arange(len(s)), sel)
            assert not len(rest) or (s[sel] - 100 * e[sel]).min() > (s[rest] + 100 * e[rest]).max(), (r, beta)
            picked.append(sel)
        max_ind = np.unique(np.concatenate(picked))
        assert np.array_equal(max_ind, z[p + "max_ind"])
        cand = z[p + "cand"]
        if len(max_ind) <= k:
            early += 1
            assert len(err) == 0 and z[p + "ret"].tolist() == cand[max_ind].tolist()
        else:
            assert len(err) == len(max_ind)
            srt = np.sort(err)
            assert (np.diff(srt) / np.abs(srt[:-1])).min() > 1e-6                          # (b)
            assert z[p + "ret"].tolist() == cand[max_ind[np.argpartition(err, k - 1)[:k]]].tolist()
    if name == "adapt_synth300_b1":
        assert early == 3                       # the early return of reference adapt_al.py:107-108 is covered
