"""Host reference of include/ital_evidence_grad.h in float64 (numpy / scipy: Cholesky and the closed forms), shared by
tests/test_evidence_grad_host.py and tests/test_gpu_evidence_grad.py.  Not a test module."""
import numpy as np


def sqdist(X):
    """D_ij = |x_i|^2 + |x_j|^2 - 2 x_i . x_j, the expansion of ital_evidence.h (not clamped)."""
    X = np.asarray(X, dtype=np.float64)
    sn = (X * X).sum(axis=1)
    return sn[:, None] + sn[None, :] - 2.0 * (X @ X.T)


def host_grad(D, y, ls, var, noise, full=True):
    """lml and its gradient in (log l, log var, log noise); with `full` also the forward-error scale S_theta of each
    component's sum, K^-1, alpha and cond(K).  None if K is not positive definite."""
    import scipy.linalg as sl
    y = np.asarray(y, dtype=np.float64)
    m = len(y)
    Kf = var * np.exp(D / (-2.0 * ls * ls))
    K = Kf + noise * np.eye(m)
    try:
        L = np.linalg.cholesky(K)
    except np.linalg.LinAlgError:
        return None
    alpha = sl.cho_solve((L, True), y)
    Minv = sl.lapack.dtrtri(L, lower=1)[0]              # K^-1 = L^-T L^-1
    W = Minv.T @ Minv
    A = np.outer(alpha, alpha) - W
    dK = (Kf * D / (ls * ls), Kf, noise * np.eye(m))
    grad = np.array([0.5 * float((A * d).sum()) for d in dK])
    lml = -0.5 * float(y @ alpha) - float(np.log(np.diag(L)).sum()) - 0.5 * m * np.log(2 * np.pi)
    if not full:
        return dict(lml=lml, grad=grad)
    scale = np.array([0.5 * float(np.abs(A * d).sum()) for d in dK])
    return dict(lml=lml, grad=grad, scale=scale, W=W, alpha=alpha, cond=float(np.linalg.cond(K)))


def evaluator(X, y, counter=None):
    """evaluate(theta[R, 3]) -> (lml[R], grad[R, 3], ok[R]) of tune.maximize_lml, on the host."""
    D = sqdist(X)
    try:        # matrices of a few hundred rows: a BLAS that spreads them over many threads is several times slower
        from threadpoolctl import threadpool_limits
    except ImportError:
        import contextlib
        threadpool_limits = lambda limits: contextlib.nullcontext()

    def evaluate(theta):
        theta = np.asarray(theta, dtype=np.float64).reshape(-1, 3)
        lml, grad, ok = np.full(len(theta), -np.inf), np.full((len(theta), 3), np.nan), np.zeros(len(theta), dtype=bool)
        with threadpool_limits(limits=1):
            for r, (ls, var, noise) in enumerate(theta):
                h = host_grad(D, y, ls, var, noise, full=False)
                if h is not None:
                    lml[r], grad[r], ok[r] = h["lml"], h["grad"], True
        if counter is not None:
            counter.append(len(theta))
        return lml, grad, ok

    return evaluate


def two_clusters(m, d, seed):
    """m rows in two clusters of d dimensions with the cluster as the label, a tenth of the labels flipped."""
    rng = np.random.default_rng(seed)
    half = m // 2
    X = np.concatenate((rng.normal(0, 0.5, (half, d)), rng.normal(0, 0.5, (m - half, d)) + 0.6))
    y = np.where(np.arange(m) < half, 1.0, -1.0)
    flip = rng.choice(m, max(1, m // 10), replace=False)
    y[flip] = -y[flip]
    return X, y
