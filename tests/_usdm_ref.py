"""What the USDM tests share (tests/test_usdm_host.py, tests/test_gpu_usdm.py, tests/golden/make_golden_usdm.py): the fixture
loader, an np.longdouble model of the five entry points of include/ital_usdm.h, a NumPy restatement of the reference's fetch
(ital/baseline_methods.py:611-658) that takes its solvers as arguments, and the checkers of the device results.

Bounds.  u = 2^-53, gamma_m = m u / (1 - m u).  An LU computed by any ordering of Gaussian elimination without pivoting
satisfies |A - L U| <= gamma_n |L| |U| componentwise, and the solution of the two triangular systems
|b - A x| <= gamma_3n |L| |U| |x| (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 9.3 / 9.4); a sum of n
products in any order |out - K x| <= gamma_n |K| |x|, checked as gamma_(n+2).  The products on the right are formed in
np.longdouble from the device's own L, U and x.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
U = 2.0 ** -53
EPS = 1e-6
LD = np.longdouble

FIXTURES = ("usdm_synth150", "usdm_synth150_ls3", "usdm_synth150_knn3_r2", "usdm_usps500")
MARGIN = 1000.0                 # the conditions of the fixtures, in units of the stored spreads
KNN_GAP = 1e-9


def gamma(m):
    return m * U / (1.0 - m * U)


# ------------------------------------------------------------------------------------------------------------ fixtures
def load(name):
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    if "X_from" in z:
        z["X"] = np.load(os.path.join(GOLDEN, str(z["X_from"]) + ".npz"))["X"]
    return z


def feedback(z, r):
    """The feedback the fixture gave after round r: {id: 1 / -1 / 0}."""
    return {int(i): float(v) for i, v in zip(z["r%d_fb_ids" % r], z["r%d_fb_vals" % r])}


def options(z):
    return dict(length_scale=float(z["length_scale"]), var=float(z["var"]), noise=float(z["noise"]), knn=int(z["knn"]),
                r=float(z["r"]), max_iter=int(z["max_iter"]), tol=float(z["tol"]))


# -------------------------------------------------------------------------------------------------------- restatement
def kernel(X, length_scale, var, dtype=np.float64):
    """K_all of the reference without noise (gp.py:410-416: v * exp((A + B - 2 C) / s), s = -2 l^2), in `dtype`."""
    X = np.asarray(X, dtype=dtype)
    xn = (X * X).sum(axis=1)
    return dtype(var) * np.exp((xn[:, None] + xn[None, :] - 2 * (X @ X.T)) / (dtype(-2.0) * dtype(length_scale) * dtype(length_scale)))


def neighbours(K, knn):
    """[n][knn] neighbour indices of the reference's graph (baseline_methods.py:604), each row ascending."""
    K = np.asarray(K, dtype=np.float64)
    return np.sort(np.argpartition(np.diag(np.diag(K)) - K, knn, axis=-1)[:, :knn], axis=-1)


def laplacian_matrix(nb, n):
    """self.A of the reference (baseline_methods.py:603-608) from the neighbour lists."""
    A = np.zeros((n, n))
    A[np.arange(n)[:, None], nb] = 1
    A += 1e-6
    return np.diag(A.sum(axis=-1)) - A


def harmonic(A, u, labelled, y, solve=np.linalg.solve):
    """p of baseline_methods.py:620 before the clip."""
    return solve(-A[np.ix_(u, u)], np.dot(A[np.ix_(u, labelled)], y))


def clip_entropy(p, r):
    prob = np.maximum(1e-8, np.minimum(1.0 - 1e-8, np.asarray(p, dtype=np.float64)))
    return prob, (r * (prob * np.log(prob) + (1.0 - prob) * np.log(1.0 - prob))) / np.log(0.5)


def alm(K, b, k, max_iter, tol, solve=np.linalg.solve):
    """_alm of the reference (baseline_methods.py:629-658) with `solve` in the place of np.linalg.solve: (f, objectives)."""
    n = len(b)
    mu, rho = 1e-6, 1.1
    f = np.ones(n) / n
    v = f.copy()
    lambda1, lambda2, obj, objs = 0.0, np.zeros(n), None, []
    for it in range(max_iter):
        A = K.copy()
        A += mu
        A[np.arange(n), np.arange(n)] += mu
        e = mu * (v + np.ones(n)) - (lambda2 + lambda1 * np.ones(n)) - b
        f = np.asarray(solve(A, e), dtype=np.float64)
        v = f + lambda2 / mu
        v[v < 0] = 0
        lambda1 += mu * (f.sum() - k)
        lambda2 += mu * (f - v)
        mu *= rho
        obj_prev = obj
        obj = np.dot(f, np.dot(K, f)) / 2 + np.dot(f, b)
        objs.append(obj)
        if (obj_prev is not None) and (abs(obj_prev - obj) < tol):
            break
    return f, np.array(objs, dtype=np.float64)


def fetch(K, A, relevant, irrelevant, unnameable, k, r, max_iter, tol, solve_lu=np.linalg.solve, solve_spd=np.linalg.solve):
    """Steps 2 to 4 of a fetch from the kernel matrix K and the Laplacian A of all samples."""
    n = len(K)
    labelled = np.array(list(set(relevant) | set(irrelevant)), dtype=np.int64)      # the reference's order (:613)
    u = np.setdiff1d(np.arange(n), np.concatenate([labelled, np.array(sorted(unnameable), dtype=np.int64)]))
    y = np.array([1. if i in relevant else 0. for i in labelled])
    p = np.asarray(harmonic(A, u, labelled, y, solve_lu), dtype=np.float64)
    prob, b = clip_entropy(p, r)
    f, objs = alm(K[np.ix_(u, u)], b, k, max_iter, tol, solve_spd)
    return dict(u=u, p=p, prob=prob, b=b, f=f, objectives=objs, iterations=len(objs), picks=u[np.argpartition(-f, k - 1)[:k]])


# ------------------------------------------------------------------------------------------- extended-precision solvers
def ld_lu(A):
    """(LU, info) of Gaussian elimination without pivoting in np.longdouble; info as ital_lu_factor."""
    LU = np.array(A, dtype=LD)
    n = len(LU)
    for j in range(n):
        if not LU[j, j] > 0:
            return LU, j + 1
        LU[j + 1:, j] /= LU[j, j]
        LU[j + 1:, j + 1:] -= np.outer(LU[j + 1:, j], LU[j, j + 1:])
    return LU, 0


def ld_lu_apply(LU, y):
    x = np.array(y, dtype=LD)
    n = len(x)
    for i in range(1, n):
        x[i] -= LU[i, :i] @ x[:i]
    for i in range(n - 1, -1, -1):
        x[i] = (x[i] - LU[i, i + 1:] @ x[i + 1:]) / LU[i, i]
    return x


def ld_solve_lu(A, b):
    if A[0, 0] < 0:                 # the reference passes -(D_uu - W_uu) and -W_ul y: the same system, negated exactly
        A, b = -A, -b
    LU, info = ld_lu(A)
    assert info == 0
    return ld_lu_apply(LU, b)


def ld_solve_chol(A, b):
    """Cholesky solve in np.longdouble (lower triangle of A)."""
    L = np.tril(np.array(A, dtype=LD))
    n = len(L)
    for j in range(n):
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
        L[j + 1:, j + 1:] -= np.tril(np.outer(L[j + 1:, j], L[j + 1:, j]))
    x = np.array(b, dtype=LD)
    for i in range(n):
        x[i] = (x[i] - L[i, :i] @ x[:i]) / L[i, i]
    for i in range(n - 1, -1, -1):
        x[i] = (x[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def scipy_solve_chol(A, b):
    import scipy.linalg
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(A, lower=True), b)


# ------------------------------------------------------------------------------------------ model of the entry points
def model_laplacian(idx, k, n, u, pos, rel, n_rel, eps=EPS):
    """(M, rhs) of ital_usdm_laplacian, in bits: every value is one FP64 operation on FP64 values."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, k)
    w1 = np.float64(1.0) + np.float64(eps)
    deg = np.float64(k) + np.float64(n) * np.float64(eps)
    n_u = len(u)
    M = np.full((n_u, n_u), -np.float64(eps))
    rhs = np.empty(n_u)
    base = np.float64(n_rel) * np.float64(eps)
    for a in range(n_u):
        c = 0
        for j in idx[u[a]]:
            if j < 0:
                continue
            if pos[j] >= 0:
                M[a, pos[j]] = -w1
            if rel[j]:
                c += 1
        M[a, a] = deg - np.float64(eps)
        rhs[a] = np.float64(c) + base
    return M, rhs


def model_shift(K, mu):
    """The lower triangle of ital_usdm_shift's B, in bits (the strict upper triangle: NaN)."""
    K = np.asarray(K, dtype=np.float64)
    B = K + np.float64(mu)
    B[np.diag_indices(len(K))] += np.float64(mu)
    B[np.triu_indices(len(K), 1)] = np.nan
    return B


def model_symv(K, x):
    """K_sym x in np.longdouble from the lower triangle of K."""
    L = np.tril(np.asarray(K, dtype=np.float64)).astype(LD)
    S = L + np.tril(L, -1).T
    return S @ np.asarray(x, dtype=LD)


# ------------------------------------------------------------------------------------------------------------ checkers
def check_lu(A, LU, info, status_before, status_after, expect_info=0):
    """Asserts what ital_lu_factor promises for the input A and returns the worst |A - L U| / (gamma_n |L| |U|).  A
    failing factorisation (expect_info != 0) must report the column and set the status bit and nothing else."""
    A = np.asarray(A, dtype=np.float64)
    n = len(A)
    if expect_info != 0:
        assert info == expect_info, "info %d, expected %d" % (info, expect_info)
        assert status_after == (status_before | 1), "status %d after %d" % (status_after, status_before)
        return 0.0
    assert info == 0, "info %d on a matrix that factors" % info
    assert status_after == status_before, "status changed from %d to %d" % (status_before, status_after)
    LU = np.asarray(LU, dtype=np.float64)
    assert np.isfinite(LU).all()
    L = np.tril(LU, -1).astype(LD) + np.eye(n, dtype=LD)
    Um = np.triu(LU).astype(LD)
    res = np.abs(A.astype(LD) - L @ Um)
    bound = LD(gamma(n)) * (np.abs(L) @ np.abs(Um))
    ratio = float(np.max(res / bound))
    assert ratio <= 1.0, "|A - L U| is %.3g of gamma_n |L| |U|" % ratio
    return ratio


def check_lu_solve(A, LU, b, x):
    """Worst |b - A x| / (gamma_3n |L| |U| |x|) for the device's factor and solution."""
    n = len(A)
    LU = np.asarray(LU, dtype=np.float64)
    L = np.tril(LU, -1).astype(LD) + np.eye(n, dtype=LD)
    Um = np.triu(LU).astype(LD)
    x = np.asarray(x, dtype=np.float64)
    assert np.isfinite(x).all()
    res = np.abs(np.asarray(b, dtype=LD) - np.asarray(A, dtype=np.float64).astype(LD) @ x.astype(LD))
    bound = LD(gamma(3 * n)) * ((np.abs(L) @ np.abs(Um)) @ np.abs(x).astype(LD))
    ratio = float(np.max(res / bound))
    assert ratio <= 1.0, "|b - A x| is %.3g of gamma_3n |L| |U| |x|" % ratio
    return ratio


def check_symv(K, x, out):
    n = len(x)
    L = np.abs(np.tril(np.asarray(K, dtype=np.float64))).astype(LD)
    bound = LD(gamma(n + 2)) * ((L + np.tril(L, -1).T) @ np.abs(np.asarray(x, dtype=LD)))
    res = np.abs(np.asarray(out, dtype=np.float64).astype(LD) - model_symv(K, x))
    ok = res <= bound
    assert ok.all(), "|out - K x| above gamma_(n+2) |K| |x| in %d entries" % int((~ok).sum())
    return float(np.max(np.where(bound > 0, res / np.where(bound > 0, bound, 1), 0)))


def dominant_matrix(n, rng, margin):
    """A random matrix that is strictly diagonally dominant by rows: diagonal = (sum of |off-diagonal|) / (1 - margin)."""
    A = rng.uniform(-1.0, 1.0, size=(n, n))
    np.fill_diagonal(A, 0.0)
    s = np.abs(A).sum(axis=1)
    np.fill_diagonal(A, np.where(s > 0, s, 1.0) / (1.0 - margin))
    return A


def random_graph(n, k, rng):
    """Neighbour lists as ital_knn_rows writes them for skip_self: k distinct other rows, -1 where there are fewer."""
    idx = np.full((n, k), -1, dtype=np.int64)
    for i in range(n):
        others = np.delete(np.arange(n), i)
        take = rng.permutation(others)[:k]
        idx[i, :len(take)] = take
    return idx


def check_fixture_conditions(z):
    """The conditions of tests/golden/make_golden_usdm.py, on a loaded fixture."""
    k, knn, tol = int(z["k"]), int(z["knn"]), float(z["tol"])
    X = z["X"]
    K = kernel(X, float(z["length_scale"]), float(z["var"]))
    off = K - np.diag(np.diag(K))
    assert (np.sort(off, axis=1)[:, -knn] > 0).all()
    xn = (X * X).sum(axis=1)
    sq = xn[:, None] + xn[None, :] - 2 * (X @ X.T)
    sq[np.diag_indices(len(X))] = np.inf
    srt = np.sort(sq, axis=1)
    assert ((srt[:, knn] - srt[:, knn - 1]) >= KNN_GAP * np.abs(srt[:, knn])).all()
    for r in range(int(z["rounds"])):
        p = "r%d_" % r
        f, objs = z[p + "f"], z[p + "objectives"]
        sf, so, sp = float(z[p + "spread_f"]), float(z[p + "spread_obj"]), float(z[p + "spread_prob"])
        top = np.sort(f)[::-1][:k + 1]
        assert (top[:-1] - top[1:] >= MARGIN * sf).all(), (r, top, sf)
        d = np.abs(objs[:-1] - objs[1:])
        assert (np.abs(d - tol) >= MARGIN * so).all(), (r, so)
        assert int(z[p + "iterations"]) == len(objs) == int(z[p + "iterations_a"]) == int(z[p + "iterations_b"])
        pv = z[p + "p"]
        for bound, sign in ((1e-8, -1.0), (1.0 - 1e-8, 1.0)):
            near = np.abs(pv - bound) <= MARGIN * sp
            assert not near.any(), (r, bound, pv[near])
