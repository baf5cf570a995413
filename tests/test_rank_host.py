"""Ranking and evaluation without a device: the host model of tests/_rank_ref.py against scikit-learn, harness.ndcg and
np.argsort; header against binding; every refusal of ital_rank_desc / ital_rank_eval (they come before any HIP call); the
refusals of metrics.evaluate on host inputs."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _rank_ref as ref  # noqa: E402

from ital_amd import _lib, build, harness  # noqa: E402


# ------------------------------------------------------------------------------------------------------ the model
def _cases(count=300, seed=11):
    """(scores, relevance, tied): n up to 400; one third heavily tied, with both zeros."""
    rng = np.random.default_rng(seed)
    for c in range(count):
        n = int(rng.integers(2, 401))
        tied = c % 3 == 0
        if tied:
            s = rng.integers(-3, 4, size=n).astype(np.float64) / 2.0
            s[rng.random(n) < 0.1] = -0.0
        else:
            s = rng.normal(size=n)
        rel = rng.choice([-1, 0, 1], size=n, p=[0.5, 0.2, 0.3])
        rel[int(rng.integers(n))] = 1
        yield s, rel, tied


def test_model_against_scikit_learn_and_the_harness():
    from sklearn.metrics import average_precision_score
    worst_ap, worst_ndcg = 0.0, 0.0
    for s, rel, tied in _cases():
        known = rel != 0
        want = average_precision_score(rel[known], s[known])
        worst_ap = max(worst_ap, abs(ref.ap(s, rel) - want) / want)
        if not tied:                        # harness.ndcg sorts with numpy's unstable default: defined on distinct scores only
            assert len(np.unique(s)) == len(s)
            want = harness.ndcg(rel, s)
            worst_ndcg = max(worst_ndcg, abs(ref.ndcg(s, rel) - want) / want)
    print("model: ap within %.3g of scikit-learn, ndcg within %.3g of harness.ndcg" % (worst_ap, worst_ndcg))
    assert worst_ap < 5e-15 and worst_ndcg < 5e-15


def test_model_on_small_cases_by_hand():
    # ranking by score: +, -, (+ unknown), +  ->  known ranks 1, 2, 3
    s, rel = np.array([0.9, 0.5, 0.4, 0.45]), np.array([1, -1, 1, 0])
    assert ref.ap(s, rel) == pytest.approx((1 / 2) * (1 / 1) + (1 / 2) * (2 / 3), rel=1e-15)
    assert ref.ndcg(s, rel) == pytest.approx((1 + 1 / 2) / (1 + 1 / np.log2(3)), rel=1e-15)
    # one group of three equal scores (both zeros in it) with two positives, then a negative
    s, rel = np.array([0.0, -0.0, 0.0, -1.0]), np.array([1, -1, 1, -1])
    assert ref.ap(s, rel) == pytest.approx(2 / 3, rel=1e-15)
    assert ref.evaluate(s, rel) == dict(n_pos=2, n_neg=2, n_unknown=0, n_nan=0, ap=ref.ap(s, rel), ndcg=ref.ndcg(s, rel))
    assert np.isnan(ref.ap(s, -np.abs(rel))) and np.isnan(ref.ndcg(s, -np.abs(rel)))
    assert ref.counts(np.array([np.nan, 1.0, np.nan]), np.array([1, 1, 0]))["n_nan"] == 1


def test_order_with_nans_and_both_zeros():
    nan = np.frombuffer(np.array([0x7ff8000000000000, 0xfff8000000000001, 0x7ff0000000000001, 0xffffffffffffffff],
                                 dtype=np.uint64).tobytes(), dtype=np.float64)
    s = np.array([0.0, nan[0], -0.0, 1.0, nan[1], -np.inf, 0.0, nan[2], np.inf, -0.0, 5e-324, -5e-324, nan[3], 1.0])
    o = ref.order(s)
    assert o.tolist() == np.argsort(s, kind="stable")[::-1].tolist()
    assert o.tolist() == [12, 7, 4, 1, 8, 13, 3, 10, 9, 6, 2, 0, 11, 5]


# ------------------------------------------------------------------------------------------------------ ABI
def test_header_matches_the_binding_and_the_symbols_are_exported():
    with open(os.path.join(ROOT, "include", "ital_rank.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    names = {"ital_rank_desc", "ital_rank_workspace", "ital_rank_eval", "ital_rank_eval_workspace"}
    assert set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", header)) == names == set(_lib.RANK_SIGNATURES)
    for name in dir(_lib):
        if name.endswith("SIGNATURES") and name != "RANK_SIGNATURES":
            assert not names & set(getattr(_lib, name)), name
    ctype = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const double*": ctypes.c_void_p, "double*": ctypes.c_void_p,
             "int64_t*": ctypes.c_void_p, "const int64_t*": ctypes.c_void_p, "const signed char*": ctypes.c_void_p,
             "hipStream_t": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}
    for name, (res, args) in _lib.RANK_SIGNATURES.items():
        m = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)" % name, header)
        assert ctype[m.group(1)] is res, name
        params = [re.sub(r"\s*\w+$", "", p.strip()).replace(" *", "*") for p in m.group(2).split(",")]
        assert [ctype[p] for p in params] == args, (name, params)
    assert int(re.search(r"#define ITAL_RANK_TILE (\d+)", header).group(1)) == _lib.RANK_TILE
    assert int(re.search(r"#define ITAL_RANK_EVAL_LEN (\d+)", header).group(1)) == _lib.RANK_EVAL_LEN == len(_lib.RANK_EVAL_FIELDS)
    for slot, field in enumerate(_lib.RANK_EVAL_FIELDS):
        assert int(re.search(r"#define ITAL_RANK_%s (\d+)" % field.upper(), header).group(1)) == slot
    assert "rank.hip" in build.SOURCES
    lib = _lib.lib()
    for name in names:
        assert getattr(lib, name).argtypes == _lib.RANK_SIGNATURES[name][1]


def test_the_python_surface_is_exported():
    import ital_amd
    from ital_amd import metrics
    from ital_amd.gp import GaussianProcess
    from ital_amd.retrieval_base import ActiveRetrievalBase
    assert "metrics" in ital_amd.__all__ and ital_amd.metrics is metrics
    assert callable(metrics.rank) and callable(metrics.evaluate)
    assert callable(GaussianProcess.rank_mean) and callable(ActiveRetrievalBase.evaluate)
    import inspect
    assert inspect.signature(harness.run_retrieval_experiment).parameters["metrics"].default == "host"
    with pytest.raises(ValueError):
        harness.run_retrieval_experiment(None, None, None, metrics="gpu")


def test_ital_hip_h_does_not_know_the_new_symbols():
    with open(os.path.join(ROOT, "include", "ital_hip.h")) as fh:
        text = fh.read()
    assert "ital_rank" not in text and "ITAL_RANK" not in text
    assert not set(_lib.RANK_SIGNATURES) & set(_lib.SIGNATURES)


# ------------------------------------------------------------------------------------------------------ refusals
N = 5000


def _rank(**over):
    a = dict(v=4096, n=N, index_offset=0, out_idx=4096, out_vals=0, work=4096, work_bytes=_lib.lib().ital_rank_workspace(N), stream=0)
    a.update(over)
    return _lib.lib().ital_rank_desc(*[a[k] for k in ("v", "n", "index_offset", "out_idx", "out_vals", "work", "work_bytes", "stream")])


def _eval(**over):
    a = dict(order=4096, v=4096, rel=4096, n=N, index_offset=0, out=4096, work=4096,
             work_bytes=_lib.lib().ital_rank_eval_workspace(N), stream=0)
    a.update(over)
    return _lib.lib().ital_rank_eval(*[a[k] for k in ("order", "v", "rel", "n", "index_offset", "out", "work", "work_bytes", "stream")])


RANK_REFUSALS = [dict(n=0), dict(n=-1), dict(n=1 << 31, work_bytes=1 << 62), dict(v=0), dict(out_idx=0), dict(work=0),
                 dict(work=4100), dict(work_bytes=24 * N - 1), dict(work_bytes=0)]
EVAL_REFUSALS = [dict(n=0), dict(n=-1), dict(n=1 << 31, work_bytes=1 << 62), dict(order=0), dict(v=0), dict(rel=0), dict(out=0),
                 dict(work=0), dict(work=4100), dict(work_bytes=0)]


@pytest.mark.parametrize("over", RANK_REFUSALS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_rank_refusals_come_before_any_hip_call(over):
    assert _rank(**over) == -22
    assert _lib.lib().ital_last_error().decode().startswith("ital_rank_desc: ")


@pytest.mark.parametrize("over", EVAL_REFUSALS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_eval_refusals_come_before_any_hip_call(over):
    assert _eval(**over) == -22
    assert _lib.lib().ital_last_error().decode().startswith("ital_rank_eval: ")


def test_a_workspace_one_byte_short_is_refused_and_the_sizes():
    lib = _lib.lib()
    for n in (1, 2048, 2049, N, (1 << 31) - 1):
        assert lib.ital_rank_workspace(n) >= 24 * n and lib.ital_rank_workspace(n) % 16 == 0
        assert lib.ital_rank_eval_workspace(n) >= 9 * n and lib.ital_rank_eval_workspace(n) % 8 == 0
    assert _eval(work_bytes=lib.ital_rank_eval_workspace(N) - 1) == -22
    assert _rank(work_bytes=lib.ital_rank_workspace(N) - 1) == -22
    for bad in (0, -5, 1 << 31, 1 << 40):
        assert lib.ital_rank_workspace(bad) == 0 and lib.ital_rank_eval_workspace(bad) == 0


# ------------------------------------------------------------------------------------------------------ metrics.evaluate
def test_evaluate_refuses_nan_scores_and_no_positives_on_host_inputs():
    from ital_amd import metrics
    s = np.array([0.3, np.nan, 0.1, 0.2])
    with pytest.raises(ValueError, match="NaN"):
        metrics.evaluate(s, np.array([1, -1, 1, 0]))
    with pytest.raises(ValueError, match="relevant"):
        metrics.evaluate(np.array([0.3, 0.5, 0.1]), np.array([-1, 0, -1]))
    with pytest.raises(ValueError, match="relevant"):
        metrics.evaluate([0.3, np.nan, 0.1], [-1, 0, -1])           # the NaN belongs to an unknown sample
    with pytest.raises(ValueError):
        metrics.evaluate(np.zeros(3), np.ones(4, dtype=np.int8))
