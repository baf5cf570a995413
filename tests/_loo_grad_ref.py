"""Host reference of include/ital_loo_grad.h in float64 (numpy / scipy: Cholesky, dtrtri and the closed forms), shared by
tests/test_loo_grad_host.py and tests/test_gpu_loo_grad.py.  Not a test module."""
import numpy as np

from _evidence_grad_ref import sqdist, two_clusters  # noqa: F401  (re-exported: the tests take their inputs from here)

LOG2PI = float(np.log(2 * np.pi))


def loo_values(alpha, c):
    """loo_logp and loo_mse from alpha and c_i = (K^-1)_ii (R&W 5.10 - 5.12)."""
    r = alpha / c
    var = 1.0 / c
    return float(np.sum(-0.5 * np.log(var) - r * r / (2.0 * var) - 0.5 * LOG2PI)), float(np.mean(r * r))


def host_loo(D, y, ls, var, noise, full=True):
    """loo_logp, loo_mse and their gradients in (log l, log var, log noise); with `full` also the forward-error scales S of
    each component's sum, alpha, c and cond(K).  None if K is not positive definite."""
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
    Minv = np.tril(sl.lapack.dtrtri(L, lower=1)[0])     # K^-1 = L^-T L^-1
    W = Minv.T @ Minv
    c = np.diag(W).copy()
    dK = (Kf * D / (ls * ls), Kf, noise * np.eye(m))
    g_logp, g_mse = np.empty(3), np.empty(3)
    u = 0.5 * (1.0 + alpha * alpha / c)
    for k, A in enumerate(dK):
        P = W @ A
        r = P @ alpha
        s = (P * W).sum(axis=1)                         # (P W)_ii, W symmetric
        g_logp[k] = float(np.sum((alpha * r - u * s) / c))
        g_mse[k] = 2.0 / m * float(np.sum((alpha / c) * (alpha * s / c - r) / c))
    logp, mse = loo_values(alpha, c)
    out = dict(loo_logp=logp, loo_mse=mse, grad_logp=g_logp, grad_mse=g_mse)
    if not full:
        return out
    s_logp, s_mse = np.empty(3), np.empty(3)
    aW, aa = np.abs(W), np.abs(alpha)
    for k, A in enumerate(dK):
        aP = aW @ np.abs(A)
        ar = aP @ aa
        as_ = (aP * aW).sum(axis=1)
        s_logp[k] = float(np.sum((aa * ar + u * as_) / c))
        s_mse[k] = 2.0 / m * float(np.sum((aa / c) * (aa * as_ / c + ar) / c))
    out.update(scale_logp=s_logp, scale_mse=s_mse, alpha=alpha, c=c, cond=float(np.linalg.cond(K)))
    return out


def _single_thread():
    try:        # matrices of a few hundred rows: a BLAS that spreads them over many threads is several times slower
        from threadpoolctl import threadpool_limits
        return threadpool_limits(limits=1)
    except ImportError:
        import contextlib
        return contextlib.nullcontext()


def evaluator(X, y, criterion="loo_logp", perturb=0.0):
    """evaluate(theta[R, 3]) -> (score[R], grad[R, 3], ok[R]) of tune.maximize_lml, on the host, in the orientation of
    tune.session_scores (loo_mse negated).  `perturb`: a relative perturbation of every output, alternating in sign."""
    D = sqdist(X)
    sign = -1.0 if criterion == "loo_mse" else 1.0

    def evaluate(theta):
        theta = np.asarray(theta, dtype=np.float64).reshape(-1, 3)
        val, grad, ok = np.full(len(theta), -np.inf), np.full((len(theta), 3), np.nan), np.zeros(len(theta), dtype=bool)
        with _single_thread():
            for r, (ls, var, noise) in enumerate(theta):
                h = host_loo(D, y, ls, var, noise, full=False)
                if h is not None:
                    val[r], ok[r] = sign * h[criterion], True
                    grad[r] = sign * h["grad_" + criterion[4:]]
        if perturb:
            val = val * (1.0 + perturb * np.where(np.arange(len(theta)) % 2, -1.0, 1.0))
            grad = grad * (1.0 + perturb * np.array([1.0, -1.0, 1.0]))
        return val, grad, ok

    return evaluate
