"""What the reweigh tests share, in plain numpy float64: the dense model of a GP with one extra noise variance per labelled
sample, the bound of DESIGN.md section 12, and a host emulation of exactly the recurrences of csrc/reweigh.hip.

Dense model:  A = rbf(X_T) + noise I + diag(e),  mean = K_NT A^-1 y,  var = v - diag(K_NT A^-1 K_TN), a full covariance block of
the listed rows, K (= A) and w = A^-1 y.  oracle.gp.OracleGP cannot take a vector of noises; its kernel function is used as is."""
import numpy as np

ROWS12 = [0, 3, 17, 64, 65, 100, 128, 199, 255, 256, 299, 300]


def rbf(a, b, ls, var=1.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    an, bn = (a * a).sum(axis=1), (b * b).sum(axis=1)
    return var * np.exp((an[:, None] + bn[None, :] - 2.0 * (a @ b.T)) / (-2.0 * ls * ls))


def cond(A):
    """The dpocon estimate, as tests/test_gpu_revoke.py computes it."""
    from scipy.linalg import lapack
    c, info = lapack.dpotrf(A, lower=1)
    assert info == 0
    rcond, _ = lapack.dpocon(c, np.abs(A).sum(axis=0).max(), uplo="L")
    return 1.0 / rcond


def gram(XT, e, ls, var=1.0, noise=1e-6):
    XT = np.asarray(XT, dtype=np.float64)
    return rbf(XT, XT, ls, var) + noise * np.eye(len(XT)) + np.diag(np.asarray(e, dtype=np.float64))


class Dense(object):
    """The dense model of labelled feature rows XT with labels y and extra noise e, predicting the rows of X."""

    def __init__(self, X, XT, y, e, ls, var=1.0, noise=1e-6, rows=ROWS12):
        import scipy.linalg
        X = np.asarray(X, dtype=np.float64)
        self.K = gram(XT, e, ls, var, noise)
        self.c = scipy.linalg.cho_factor(self.K, lower=True)
        self.w = scipy.linalg.cho_solve(self.c, np.asarray(y, dtype=np.float64))
        KNT = rbf(X, XT, ls, var)
        self.mean = KNT @ self.w
        Z = scipy.linalg.cho_solve(self.c, KNT.T)
        self.var = var - np.einsum("ij,ji->i", KNT, Z)
        self.rows = [r for r in rows if r < len(X)]
        R = X[self.rows]
        self.cov = rbf(R, R, ls, var) - KNT[self.rows] @ Z[:, self.rows]
        self.cond = cond(self.K)

    def loo(self, y):
        """Leave-one-out mean and variance of every label (R&W 5.12) on this Gram."""
        import scipy.linalg
        Ki = scipy.linalg.cho_solve(self.c, np.eye(len(self.K)))
        d = np.diag(Ki)
        return np.asarray(y, dtype=np.float64) - self.w / d, 1.0 / d


WORST = [0.0]        # the largest |got - model| / bound seen in this process (printed; DESIGN.md section 24 quotes it)


def within(got, want, cnd, what):
    """|got - want| <= max(1e-10, 1e-15 cond) * max(1, max|want|): tests/test_gpu_revoke.py::_within."""
    bound = max(1e-10, 1e-15 * cnd) * max(1.0, float(np.max(np.abs(want))))
    err = float(np.max(np.abs(np.asarray(got) - np.asarray(want))))
    WORST[0] = max(WORST[0], err / bound)
    print("%-12s err %.3g  bound %.3g  ratio %.3g  (cond %.3g; worst ratio so far %.3g)" % (what, err, bound, err / bound, cnd,
                                                                                            WORST[0]))
    assert err <= bound, (what, err, bound, cnd)


# ------------------------------------------------------------------------------------------------ the kernel's recurrences
PASS = 8             # ITAL_REWEIGH_PASS


class Refused(Exception):
    pass


def _factor_chain(L, alpha, p, delta, flip=False):
    """One chain on the factor (in place), top-down from row p: returns the rotations [(ic, sk, c, s)] of rows p .. m-1 and
    (g, h), the weights of the carry in mu and s2.  `flip`: the injected mistake of a wrong sign in the downdate."""
    m = len(L)
    kind = -1.0 if delta < 0 else 1.0
    x = np.zeros(m + 1)                  # entry m: the carry of alpha, the row below the last one
    x[p] = np.sqrt(abs(delta))
    rots = []
    for k in range(p, m):
        d, xk = L[k, k], x[k]
        with np.errstate(invalid="ignore"):
            rr = np.sqrt(xk * xk + d * d) if kind > 0 else np.sqrt((d - xk) * (d + xk))
        if not (rr > 0 and np.isfinite(rr) and d > 0):
            raise Refused()
        ic, s, c = d / rr, xk / d, rr / d
        sk = kind * s
        if flip and kind < 0:
            sk = -sk
        L[k, k] = rr
        L[k + 1:, k] = (L[k + 1:, k] + sk * x[k + 1:m]) * ic
        x[k + 1:m] = c * x[k + 1:m] - s * L[k + 1:, k]
        alpha[k] = (alpha[k] + sk * x[m]) * ic
        x[m] = c * x[m] - s * alpha[k]
        rots.append((ic, sk, c, s))
    return rots, (-kind * x[m], kind)


def emulate(L, alpha, V, mu, s2, pos, delta, flip=False, reverse=False, keep_carry=False):
    """ital_gp_reweigh on host copies: the chains one after the other on the factor, then the sweeps of at most PASS chains --
    at row q the rotations of every chain with pos[j] <= q in chain order, carries from 0 -- and mu += sum g u, s2 += sum h u^2.
    Returns the new (L, alpha, V, mu, s2); raises Refused and leaves the inputs alone when a pivot is not positive and finite.
    Injected mistakes: `flip` (sign of the downdate), `reverse` (the sweep applies the chains of a row in the wrong order),
    `keep_carry` (the carries are not reset between two passes)."""
    L, alpha, V, mu, s2 = (np.array(a, dtype=np.float64, copy=True) for a in (L, alpha, V, mu, s2))
    m = len(L)
    assert all(0 <= p < m for p in pos) and all(b > a for a, b in zip(pos, pos[1:]))
    chains = [_factor_chain(L, alpha, p, d, flip) for p, d in zip(pos, delta)]
    u = None
    for j0 in range(0, len(pos), PASS):
        grp = list(range(j0, min(j0 + PASS, len(pos))))
        if u is None or not keep_carry:
            u = np.zeros((PASS, V.shape[1]))
        for q in range(pos[j0], m):
            for j in (reversed(grp) if reverse else grp):
                if q < pos[j]:
                    continue
                ic, sk, c, s = chains[j][0][q - pos[j]]
                V[q] = (V[q] + sk * u[j - j0]) * ic
                u[j - j0] = c * u[j - j0] - s * V[q]
        for j in grp:
            g, h = chains[j][1]
            mu += g * u[j - j0]
            s2 += h * u[j - j0] ** 2
    return L, alpha, V, mu, s2


def whitened(X, XT, y, e, ls, var=1.0, noise=1e-6):
    """The state the device keeps, from a dense factorisation: L, alpha = L^-1 y, V = L^-1 K_TN, mu, s2."""
    import scipy.linalg
    L = np.linalg.cholesky(gram(XT, e, ls, var, noise))
    alpha = scipy.linalg.solve_triangular(L, np.asarray(y, dtype=np.float64), lower=True)
    V = scipy.linalg.solve_triangular(L, rbf(XT, X, ls, var), lower=True)
    return L, alpha, V, V.T @ alpha, var - (V * V).sum(axis=0)
