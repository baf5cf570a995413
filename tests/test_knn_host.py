"""The neighbour lists and SUD without a device: header against binding, every refusal of ital_knn_rows (they come before any
HIP call), the checker of tests/_knn_ref.py on the model's own answer and on injected mistakes, and the array functions of
ital_amd/sud.py against what the real reference recorded (tests/golden/make_golden_sud.py)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _knn_ref as ref  # noqa: E402

from ital_amd import _lib, build  # noqa: E402


# ------------------------------------------------------------------------------------------------------ ABI
def test_header_matches_the_binding():
    with open(os.path.join(ROOT, "include", "ital_knn.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    assert set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", header)) == {"ital_knn_rows", "ital_knn_workspace"} == set(_lib.KNN_SIGNATURES)
    for name in dir(_lib):
        if name.endswith("SIGNATURES") and name != "KNN_SIGNATURES":
            assert not set(_lib.KNN_SIGNATURES) & set(getattr(_lib, name)), name
    ctype = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const double*": ctypes.c_void_p, "double*": ctypes.c_void_p,
             "int64_t*": ctypes.c_void_p, "hipStream_t": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64,
             "size_t": ctypes.c_size_t}
    for name, (res, args) in _lib.KNN_SIGNATURES.items():
        m = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)" % name, header)
        assert ctype[m.group(1)] is res, name
        params = [re.sub(r"\s*\w+$", "", p.strip()).replace(" *", "*") for p in m.group(2).split(",")]
        assert [ctype[p] for p in params] == args, (name, params)
    for macro, value in (("ITAL_KNN_MAX_K", _lib.KNN_MAX_K), ("ITAL_KNN_MAX_SPLITS", _lib.KNN_MAX_SPLITS),
                         ("ITAL_KNN_AUTO_SPLITS", _lib.KNN_AUTO_SPLITS), ("ITAL_KNN_COSINE", _lib.KNN_METRICS["cosine"]),
                         ("ITAL_KNN_SQEUCLIDEAN", _lib.KNN_METRICS["sqeuclidean"])):
        assert int(re.search(r"#define %s (\d+)" % macro, header).group(1)) == value
    assert "knn.hip" in build.SOURCES
    lib = _lib.lib()
    assert lib.ital_knn_rows.argtypes == _lib.KNN_SIGNATURES["ital_knn_rows"][1]


def _call(**over):
    """ital_knn_rows with valid arguments (fake, suitably aligned pointers: a refusal never touches them) but `over`."""
    a = dict(X=4096, xtype=0, xnorm=4096, n=10, ldx=16, q0=0, q1=10, c0=0, c1=10, metric=0, k=3, skip_self=1, accumulate=0,
             splits=1, dist=4096, idx=4096, rowsum=0, workspace=4096, workspace_bytes=1 << 20, stream=0)
    a.update(over)
    return _lib.lib().ital_knn_rows(*[a[name] for name in ("X", "xtype", "xnorm", "n", "ldx", "q0", "q1", "c0", "c1", "metric", "k",
                                                           "skip_self", "accumulate", "splits", "dist", "idx", "rowsum", "workspace",
                                                           "workspace_bytes", "stream")])


REFUSALS = [dict(n=-1, q1=0, c1=0), dict(n=1 << 31), dict(q0=-1), dict(q1=11), dict(q0=5, q1=4), dict(c0=-1), dict(c1=11),
            dict(c0=7, c1=6), dict(ldx=0), dict(ldx=-16), dict(ldx=24), dict(xtype=4), dict(xtype=-1), dict(metric=2),
            dict(metric=-1), dict(k=0), dict(k=33), dict(splits=-1), dict(splits=65), dict(workspace_bytes=10 * 3 * 12 - 1),
            dict(splits=0, workspace_bytes=16 * 10 * 3 * 12 - 1), dict(X=0), dict(xnorm=0), dict(dist=0), dict(idx=0),
            dict(workspace=0), dict(X=4104), dict(workspace=4100)]


@pytest.mark.parametrize("over", REFUSALS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_refusals_come_before_any_hip_call(over):
    assert _call(**over) == -22
    assert _lib.lib().ital_last_error().decode().startswith("ital_knn_rows: ")


def test_an_empty_query_range_is_no_work_and_the_workspace_size():
    lib = _lib.lib()
    assert _call(q0=4, q1=4, dist=0, idx=0, workspace=0, workspace_bytes=0) == 0
    assert _call(q0=4, q1=4, c0=3, c1=3, X=0, xnorm=0, dist=0, idx=0, workspace=0, workspace_bytes=0) == 0
    assert lib.ital_knn_workspace(10, 3, 1) == (10 * 3 * 12 + 15) // 16 * 16
    assert lib.ital_knn_workspace(10, 3, 2) >= 2 * 10 * 3 * 12
    assert lib.ital_knn_workspace(10, 3, 0) == lib.ital_knn_workspace(10, 3, _lib.KNN_AUTO_SPLITS)
    for bad in ((-1, 3, 1), (10, 0, 1), (10, 33, 1), (10, 3, -1), (10, 3, 65)):
        assert lib.ital_knn_workspace(*bad) == 0


# ------------------------------------------------------------------------------------------------------ the checker
def _data(n=40, d=5, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d))
    X[7] = X[3]                       # exact duplicates: index ties
    X[11] = X[3]
    X[20] = 0.0                       # a zero row: NaN under the cosine
    return X, (X * X).sum(axis=1)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("k,skip_self", [(1, 1), (5, 0), (5, 1), (32, 1)])
def test_checker_accepts_the_model(metric, k, skip_self):
    X, xn = _data()
    idx, dist = ref.model_lists(X, xn, metric, k, skip_self)
    assert ref.check(idx, dist.astype(np.float64), X, xn, metric, k, skip_self) <= 1.0
    idx, dist = ref.model_lists(X, xn, metric, k, skip_self, q=(5, 25), c=(2, 30))
    ref.check(idx, dist.astype(np.float64), X, xn, metric, k, skip_self, q=(5, 25), c=(2, 30))
    small = X[:4]
    idx, dist = ref.model_lists(small, xn[:4], metric, k, skip_self)
    assert (idx[:, 4 - skip_self:] == -1).all() and np.isposinf(dist[:, 4 - skip_self:].astype(np.float64)).all()
    ref.check(idx, dist.astype(np.float64), small, xn[:4], metric, k, skip_self)


def test_the_order_of_the_model():
    X, xn = _data()
    idx, dist = ref.model_lists(X, xn, 0, 39, True)
    assert idx[3, :2].tolist() == [7, 11] and idx[7, :2].tolist() == [3, 11]       # equal numbers by ascending index
    assert idx[3, -1] == 20 and np.isnan(dist[3, -1])                             # NaN after every number
    assert np.isnan(dist[20].astype(np.float64)).all() and idx[20].tolist() == [j for j in range(40) if j != 20]


def _mistakes():
    X, xn = _data()
    k = 39
    idx, dist = ref.model_lists(X, xn, 0, k, True)
    dist = dist.astype(np.float64)

    def self_not_skipped(i, d):
        i[5, 0], d[5, 0] = 5, 0.0

    def farther_neighbour(i, d):
        full_i, full_d = ref.model_lists(X, xn, 0, 6, True)   # lists of 5, the last entry replaced by the 6th neighbour
        return full_i[:, [0, 1, 2, 3, 5]], full_d[:, [0, 1, 2, 3, 5]].astype(np.float64), 5

    def unsorted_row(i, d):
        i[9, [2, 3]], d[9, [2, 3]] = i[9, [3, 2]], d[9, [3, 2]]

    def tie_by_larger_index(i, d):
        assert d[3, 0] == d[3, 1]
        i[3, [0, 1]] = i[3, [1, 0]]

    def value_off(i, d):
        d[12, 4] += 1e-12

    def nan_dropped(i, d):
        assert np.isnan(d[4, -1])
        i[4, -1], d[4, -1] = -1, np.inf

    def minus_one_without_inf(i, d):
        i[6, -1] = -1

    for fn in (self_not_skipped, farther_neighbour, unsorted_row, tie_by_larger_index, value_off, nan_dropped, minus_one_without_inf):
        i, d = idx.copy(), dist.copy()
        res = fn(i, d)
        yield (fn.__name__,) + ((res[0], res[1], res[2]) if res else (i, d, k))


@pytest.mark.parametrize("name,idx,dist,k", list(_mistakes()), ids=lambda v: v if isinstance(v, str) else "")
def test_checker_rejects(name, idx, dist, k):
    X, xn = _data()
    with pytest.raises(AssertionError):
        ref.check(idx, dist, X, xn, 0, k, True)


# ------------------------------------------------------------------------------------------------------ SUD
@pytest.mark.parametrize("name", ref.SUD_FIXTURES)
def test_selection_rule_reproduces_the_reference(name):
    from ital_amd.sud import sud_select, sud_uncertainty
    z, X = ref.load(name)
    assert not (np.abs(X).sum(axis=1) == 0).any()
    k = int(z["k"])
    for r in range(int(z["rounds"])):
        p = "r%d_" % r
        unc = sud_uncertainty(z[p + "mean"], z[p + "var"], float(z["noise"]))
        np.testing.assert_allclose(unc, z[p + "unc"], rtol=1e-14, atol=0)
        assert np.array_equal(unc * z[p + "dens"], z[p + "scores"]) or np.allclose(unc * z[p + "dens"], z[p + "scores"], rtol=1e-14, atol=0)
        picks = sud_select(z[p + "unc"], z[p + "dens"], k)
        assert z[p + "cand"][picks].tolist() == z[p + "ret"].tolist()
        assert z[p + "cand"][sud_select(unc, z[p + "dens"], k)].tolist() == z[p + "ret"].tolist()


@pytest.mark.parametrize("name", ref.SUD_FIXTURES)
def test_margin_condition_holds_on_the_files(name):
    z, _ = ref.load(name)
    k = int(z["k"])
    for r in range(int(z["rounds"])):
        top = np.sort(z["r%d_scores" % r])[::-1][:k + 1]
        assert (top[:-1] - top[1:]).min() >= ref.MARGIN
        assert float(z["r%d_margin_scores" % r]) >= ref.MARGIN


def test_sud_select_takes_a_nan_first():
    from ital_amd.sud import sud_select
    assert sud_select(np.array([0.5, 0.6, 0.1]), np.array([1.0, np.nan, 9.0]), 2).tolist() == [1, 2]


def test_sud_is_exported_but_not_registered():
    import ital_amd
    from ital_amd import SUD, competitors
    L = SUD(None)
    assert L.gp is None and L.K == 20 and L.last is None
    assert "SUD" in ital_amd.__all__
    assert "SUD" not in competitors.LEARNERS
    with pytest.raises(NotImplementedError):
        SUD(None, world=2)
