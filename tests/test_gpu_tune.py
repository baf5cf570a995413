"""Cross-validated hyper-parameter search on the device (ital_amd.tune, csrc/dense.hip) against numpy / scipy and against
the reference's optimize_parameters.py (goldens of tests/golden/make_golden_tune.py)."""
import ctypes
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch


def _lib():
    from ital_amd import _lib
    return _lib.lib(), _lib.check


def _chol_device(mats, pad=3):
    """Factor a list of SPD matrices in one batched call; returns (factors, info, status, padded buffers)."""
    torch = _torch()
    lib, check = _lib()
    bufs = []
    for A in mats:
        n = A.shape[0]
        ld = n + pad
        B = np.full((n + 1, ld), 7.25)          # padding past n (columns and one row) must stay untouched
        B[:n, :n] = A
        bufs.append(torch.from_numpy(B).cuda())
    ptrs = torch.tensor([b.data_ptr() for b in bufs], dtype=torch.int64, device="cuda")
    ns = torch.tensor([A.shape[0] for A in mats], dtype=torch.int32, device="cuda")
    lds = torch.tensor([A.shape[0] + pad for A in mats], dtype=torch.int64, device="cuda")
    info = torch.full((len(mats),), -5, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    check(lib.ital_chol_batched(ptrs.data_ptr(), ns.data_ptr(), lds.data_ptr(), len(mats), max(A.shape[0] for A in mats),
                                info.data_ptr(), status.data_ptr(), st))
    torch.cuda.synchronize()
    return [b.cpu().numpy() for b in bufs], info.cpu().numpy(), int(status.item()), (bufs, ptrs, ns, lds, info)


def _spd(n, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, n))
    return B @ B.T / n + np.eye(n)


SIZES = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 500, 1000, 4097]


@pytest.mark.parametrize("n", SIZES)
def test_cholesky_matches_numpy(n):
    A = _spd(n, n)
    outs, info, status, _ = _chol_device([A])
    assert info[0] == 0 and status == 0
    L = np.tril(outs[0][:n, :n])
    want = np.linalg.cholesky(A)
    assert np.max(np.abs(L - want)) <= 1e-12 * np.max(np.abs(want))
    # strict upper triangle and padding untouched
    iu = np.triu_indices(n, 1)
    assert np.array_equal(outs[0][:n, :n][iu], A[iu])
    assert np.all(outs[0][:, n:] == 7.25) and np.all(outs[0][n] == 7.25)


def test_cholesky_batched_equals_single_bit_for_bit():
    sizes = [17, 129, 64, 500, 1, 1000, 65]
    mats = [_spd(n, 100 + n) for n in sizes]
    batch, info, status, _ = _chol_device(mats)
    assert status == 0 and np.all(info == 0)
    for A, got in zip(mats, batch):
        single, _, _, _ = _chol_device([A])
        assert np.array_equal(got, single[0])


def test_cholesky_not_positive_definite_reports_column():
    n = 300
    A = _spd(n, 5)
    A[200, 200] = -1.0                          # pivot 200 is the first that fails
    good = _spd(70, 6)
    outs, info, status, _ = _chol_device([good, A])
    assert status & 1
    assert info[0] == 0 and info[1] == 201
    assert np.max(np.abs(np.tril(outs[0][:70, :70]) - np.linalg.cholesky(good))) <= 1e-12 * 3
    assert not np.any(np.isnan(outs[1][:n, :200]))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 500, 1000, 2049])
def test_solves_match_cho_solve(n):
    from scipy.linalg import cho_factor, cho_solve
    torch = _torch()
    lib, check = _lib()
    A = _spd(n, 7 * n)
    y = np.random.default_rng(n).standard_normal(n)
    outs, info, _, keep = _chol_device([A])
    bufs, ptrs, ns, lds, infod = keep
    yd = torch.from_numpy(y.copy()).cuda()
    yp = torch.tensor([yd.data_ptr()], dtype=torch.int64, device="cuda")
    check(lib.ital_chol_solve_batched(ptrs.data_ptr(), ns.data_ptr(), lds.data_ptr(), yp.data_ptr(), 1, infod.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream))
    want = cho_solve(cho_factor(A, lower=True), y)
    got = yd.cpu().numpy()
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


def _rows(X):
    torch = _torch()
    lib, check = _lib()
    n, d = X.shape
    ldx = (d + 15) // 16 * 16
    Xp = np.zeros((n, ldx))
    Xp[:, :d] = X
    Xd = torch.from_numpy(Xp).cuda()
    xn = torch.empty(n, dtype=torch.float64, device="cuda")
    check(lib.ital_row_norms(Xd.data_ptr(), n, ldx, xn.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return Xd, xn, ldx


def _rbf(A, B, ls, var):
    D = (A ** 2).sum(1)[:, None] + (B ** 2).sum(1)[None, :] - 2 * A @ B.T
    return var * np.exp(D / (-2 * ls * ls))


@pytest.mark.parametrize("na,nb,d,F", [(77, 300, 3, 1), (300, 77, 21, 10), (1000, 1531, 256, 16), (129, 4001, 21, 16),
                                       (5, 9, 3, 10)])
def test_kernel_matvec_matches_dense(na, nb, d, F):
    torch = _torch()
    lib, check = _lib()
    rng = np.random.default_rng(na * nb + d)
    Xa, Xb = rng.random((na, d)), rng.random((nb, d))
    ls, var = 0.3 * np.sqrt(d), 1.7
    W = rng.standard_normal((nb, F))
    Ad, an, ldx = _rows(Xa)
    Bd, bn, _ = _rows(Xb)
    Wd = torch.from_numpy(np.ascontiguousarray(W)).cuda()
    out = torch.full((na, F + 2), 3.5, dtype=torch.float64, device="cuda")
    wl = int(lib.ital_kernel_matvec_workspace(na, nb))
    work = torch.empty(max(wl, 1), dtype=torch.float64, device="cuda")
    check(lib.ital_kernel_matvec(Ad.data_ptr(), an.data_ptr(), na, Bd.data_ptr(), bn.data_ptr(), nb, ldx, Wd.data_ptr(), F,
                                 F, var, ls, out.data_ptr(), F + 2, work.data_ptr(), wl,
                                 torch.cuda.current_stream().cuda_stream))
    got = out.cpu().numpy()
    want = _rbf(Xa, Xb, ls, var) @ W
    assert np.max(np.abs(got[:, :F] - want)) <= 1e-12 * max(1.0, np.max(np.abs(want)))
    assert np.all(got[:, F:] == 3.5)


def test_gram_rows_matches_reference_kernel():
    torch = _torch()
    lib, check = _lib()
    rng = np.random.default_rng(3)
    X = rng.random((700, 21))
    Xd, xn, ldx = _rows(X)
    sets = [np.sort(rng.choice(700, 300, replace=False)), rng.choice(700, 129, replace=False)]
    var, ls, noise = 1.3, 0.9, 1e-3
    bufs = [torch.full((len(s), len(s) + 1), 9.0, dtype=torch.float64, device="cuda") for s in sets]
    idx = [torch.from_numpy(s.astype(np.int64)).cuda() for s in sets]
    P = lambda v, dt: torch.tensor(v, dtype=dt, device="cuda")  # noqa: E731
    ip, npt, kp, ldp = (P([t.data_ptr() for t in idx], torch.int64), P([len(s) for s in sets], torch.int32),
                        P([b.data_ptr() for b in bufs], torch.int64), P([len(s) + 1 for s in sets], torch.int64))
    check(lib.ital_gram_rows(Xd.data_ptr(), xn.data_ptr(), ldx, ip.data_ptr(), npt.data_ptr(), kp.data_ptr(), ldp.data_ptr(),
                             2, 300, var, ls, noise, torch.cuda.current_stream().cuda_stream))
    for s, b in zip(sets, bufs):
        got = b.cpu().numpy()
        want = _rbf(X[s], X[s], ls, var) + noise * np.eye(len(s))
        lo = np.tril_indices(len(s))
        assert np.max(np.abs(got[:, :len(s)][lo] - want[lo])) <= 1e-13
        assert np.all(got[:, :len(s)][np.triu_indices(len(s), 1)] == 9.0) and np.all(got[:, len(s)] == 9.0)


# ------------------------------------------------------------------------------------------------------------- goldens
class _DS(object):
    def __init__(self, X, y=None):
        self.X_train = self.X_train_norm = np.asarray(X, dtype=np.float64)
        self.y_train = y


def _bound(cond, smax):
    # dpocon is a 1-norm estimate; the Gram entries themselves differ in the last bit (MFMA vs BLAS dot products), which
    # the fold's conditioning amplifies: measured up to 1.6e-15 cond max|s| on Iris, so one decade of margin
    return max(1e-10, 1e-14 * cond) * smax


def _tied(evaluated, perf_tol):
    best = evaluated[:, 3].max()
    return evaluated[evaluated[:, 3] >= best - perf_tol]


def _check_case(ds, rel, z, prefix, grid, fewshot, capsys):
    from ital_amd import tune
    # per-fold held-out scores of the stored values
    tol_perf = 0.0
    r = 0
    while prefix + "scores%d" % r in z.files:
        ls, var, noise = z[prefix + "scores%d_params" % r]
        rows, folds, out = tune.held_out_scores(ds, rel, dict(length_scale=ls, var=var, noise=noise), fewshot=fewshot)
        cond = z[prefix + "cond%d" % r]
        want = z[prefix + "scores%d" % r]
        if fewshot:
            got = np.concatenate([out[rows[tr], f] for f, (tr, te) in enumerate(folds)])
            cuts = np.cumsum([0] + [len(tr) for tr, te in folds])
            for f in range(len(folds)):
                w = want[cuts[f]:cuts[f + 1]]
                assert np.max(np.abs(got[cuts[f]:cuts[f + 1]] - w)) <= _bound(cond[f], np.max(np.abs(w)))
        else:
            for f, (tr, te) in enumerate(folds):
                w = want[rows[te]]
                assert np.max(np.abs(out[rows[te], f] - w)) <= _bound(cond[f], np.max(np.abs(w)))
        tol_perf = max(tol_perf, 1e-12)
        r += 1
    # the search itself
    ev = z[prefix + "evaluated"]
    cond_max = max(np.max(z[prefix + "cond%d" % k]) for k in range(r))
    perf_tol = max(1e-12, 1e-15 * cond_max * 100)
    best, perf = tune.optimize_gp_params(ds, rel, grid, fewshot=fewshot, verbose=2)
    out_lines = capsys.readouterr().out.splitlines()
    want_lines = str(z[prefix + "stdout"]).splitlines()
    tied = _tied(ev, perf_tol)
    pick = [best.get("length_scale"), best.get("var", 1.0), best.get("noise", 1e-6)]
    assert any(np.allclose(pick[:len(best)], t[:len(best)]) for t in tied), (best, tied)
    assert abs(perf - float(z[prefix + "best_perf"])) <= perf_tol
    # same lines in the same order; a printed AP may differ in its last digit where the held-out scores are numerically
    # tied (length scales so small that every score underflows towards 0, or values within the bound of the best)
    assert len(out_lines) == len(want_lines)
    for got_ln, want_ln in zip(out_lines, want_lines):
        g, w = got_ln.rsplit(" : ", 1), want_ln.rsplit(" : ", 1)
        assert g[0] == w[0] or len(tied) > 1, (got_ln, want_ln)
        assert abs(float(g[1]) - float(w[1])) <= 2e-4, (got_ln, want_ln)


@pytest.mark.parametrize("cls", [0, 1, 2])
@pytest.mark.parametrize("gname", ["ls_only", "full"])
def test_iris_matches_reference(cls, gname, capsys):
    from ital_amd import tune
    z = np.load(os.path.join(GOLD, "tune_iris.npz"))
    y = z["y"]
    rel = 2 * (y == cls) - 1
    _check_case(_DS(z["X"]), rel, z, "c%d_%s_" % (cls, gname), tune.default_grids[gname], False, capsys)


@pytest.mark.parametrize("tag", ["normal", "fewshot"])
def test_usps2007_matches_reference(tag, capsys):
    from ital_amd import tune
    z = np.load(os.path.join(GOLD, "tune_usps.npz"))
    u = np.load(os.path.join(GOLD, "usps2007.npz"))
    _check_case(_DS(u["X"]), u["rel"], z, tag + "_", tune.default_grids["ls_only"], tag == "fewshot", capsys)


def test_synthetic_with_unnameable_and_regression(capsys):
    from ital_amd import tune
    z = np.load(os.path.join(GOLD, "tune_synth.npz"))
    ds = _DS(z["X"], y=z["y"])
    _check_case(ds, z["rel"], z, "ls_", tune.default_grids["ls_only"], False, capsys)
    ls, var, noise = z["reg_params"]
    got = tune.cross_validate_gp(ds, None, dict(length_scale=ls, var=var, noise=noise))
    assert abs(got - float(z["reg_value"])) <= 1e-9 * abs(float(z["reg_value"]))


def test_full_size_against_scipy():
    """9298 x 256, 10 folds, three length scales; folds 0 and 1 of two of them restated with scipy in float64."""
    from scipy.linalg import cho_factor, cho_solve
    from sklearn.metrics import average_precision_score
    from ital_amd import tune
    rng = np.random.default_rng(9298)
    X = rng.random((9298, 256))
    rel = np.where(X[:, 0] + X[:, 1] > 1.0, 1, -1)
    grid = [4.0, 6.0, 9.0]
    plist = [dict(length_scale=v, var=1.0, noise=1e-6) for v in grid]
    aps = tune._scores(X, rel, plist, 10, False, None, tune.DEFAULT_MAX_BYTES)
    assert all(np.isfinite(aps))
    for v in grid[:2]:
        rows, folds, out = tune.held_out_scores(X, rel, dict(length_scale=v, var=1.0, noise=1e-6))
        for f in (0, 1):
            tr, te = folds[f]
            A, B = X[rows[tr]], X[rows[te]]
            K = _rbf(A, A, v, 1.0) + 1e-6 * np.eye(len(tr))
            alpha = cho_solve(cho_factor(K, lower=True), rel[rows[tr]].astype(np.float64))
            want = _rbf(B, A, v, 1.0) @ alpha
            got = out[rows[te], f]
            assert np.max(np.abs(got - want)) <= 1e-6 * np.max(np.abs(want))
            assert abs(average_precision_score(rel[rows[te]], got) - average_precision_score(rel[rows[te]], want)) <= 1e-9


def test_held_out_scores_where_a_workgroup_walks_two_tiles():
    """4200 rows, d = 5, two folds: the kernel-times-W pass of _predict runs ital_kernel_matvec at (4200, 4200), where kw_split
    gives every workgroup a chunk of two 128-wide tiles (17 splits) -- the loop the Iris-sized goldens never enter."""
    import sys
    from scipy.linalg import cho_factor, cho_solve
    from ital_amd import tune
    sys.path.insert(0, HERE)
    import _dense_ref
    n = 4200
    assert _dense_ref.expected_split(n, n) == (17, 2)
    rng = np.random.default_rng(4200)
    X = rng.random((n, 5))
    rel = np.where(X[:, 0] + 0.3 * rng.standard_normal(n) > 0.5, 1, -1)
    ls, var, noise = 0.5, 1.0, 1e-2
    rows, folds, out = tune.held_out_scores(X, rel, dict(length_scale=ls, var=var, noise=noise), n_folds=2)
    assert out is not None and out.shape == (n, 2) and len(rows) == n
    for f, (tr, te) in enumerate(folds):
        A, B = X[rows[tr]], X[rows[te]]
        K = _rbf(A, A, ls, var) + noise * np.eye(len(tr))
        want = _rbf(B, A, ls, var) @ cho_solve(cho_factor(K, lower=True), rel[rows[tr]].astype(np.float64))
        cond = np.linalg.cond(K, 1)
        err = np.max(np.abs(out[rows[te], f] - want))
        print("fold %d: cond_1 = %.3g, max |score| = %.3g, max error = %.3g, bound = %.3g"
              % (f, cond, np.max(np.abs(want)), err, _bound(cond, np.max(np.abs(want)))))
        assert err <= _bound(cond, np.max(np.abs(want)))


def test_not_positive_definite_scores_minus_inf():
    from ital_amd import tune
    rng = np.random.default_rng(11)
    X = rng.random((60, 5))
    X = np.vstack([X, X])                       # duplicate rows: singular Gram without noise
    rel = np.where(X[:, 0] > 0.5, 1, -1)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        v = tune.cross_validate_gp(X, rel, dict(length_scale=1.0, var=1.0, noise=0.0))
    assert v == -np.inf
    assert any("not positive semi-definite" in str(x.message) for x in w)
    from collections import OrderedDict
    grid = OrderedDict((("length_scale", [1.0]), ("noise", [0.0, 1e-3])))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        best, perf = tune.optimize_gp_params(X, rel, grid, init=dict(length_scale=1.0, var=1.0, noise=0.0), verbose=0)
    assert best == {"length_scale": 1.0, "noise": 1e-3} and np.isfinite(perf)


def test_memory_budget_refuses_a_fold_quickly():
    import time
    from ital_amd import tune
    rng = np.random.default_rng(0)
    X = rng.random((2000, 3))
    rel = np.where(X[:, 0] > 0.5, 1, -1)
    t0 = time.time()
    with pytest.raises(MemoryError, match="n_train = 1800"):
        tune.cross_validate_gp(X, rel, dict(length_scale=1.0), max_bytes=1 << 20)
    assert time.time() - t0 < 30


def test_cli_on_iris_prints_reference_lines(tmp_path, capsys):
    from ital_amd import tune
    z = np.load(os.path.join(GOLD, "tune_iris.npz"))
    conf = tmp_path / "iris.conf"
    conf.write_text("[EXPERIMENT]\ndataset = Iris\nmethod = ITAL\ngrid = ls_only\nverbosity = 1\n\n[Iris]\n")
    tune.main([str(conf)])
    out = capsys.readouterr().out.splitlines()
    best_lines = [ln for ln in out if ln.startswith("Best parameters")]
    want = []
    for c in (0, 1, 2):
        ls = float(z["c%d_ls_only_best" % c][0])
        want.append("Best parameters for dataset 1, class {} (AP: {:.2f}): {!r}".format(c, float(z["c%d_ls_only_best_perf" % c]),
                                                                                  {"length_scale": ls}))
    assert best_lines == want
