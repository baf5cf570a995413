"""Extended-precision host reference and checker of the GP update kernels -- ital_chol_append, ital_whiten_append,
ital_cross_cov_cols, ital_predict (include/ital_hip.h) -- shared by tests/test_gp_update_ref_host.py and
tests/test_gpu_gp_update.py.  Plain NumPy, no GPU, no project import.  Not a test module.

Arithmetic: np.longdouble where it is the x87 80-bit type or better (eps <= 2^-63), else mpmath at 50 digits (object arrays of
mpf); with neither the import fails.  Inputs are always the FP64 values the device received; the reference forms norms, dot
products, the kernel values, the Cholesky factor and every residual and bound in the extended type.

The checks are componentwise residuals against a-priori rounding bounds (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., Thm 8.5 for the substitutions, Thm 10.3 for the factor), u = 2^-53, gamma(k) = k u / (1 - k u):

  kernel value   dK_ij = K_ij (dA_ij + 4u),  dA_ij = gamma(ldx + 4) (|x_i|^2 + |x_j|^2 + 2 |x_i|.|x_j|) / (2 l^2)
                 the exponent's numerator is a sum of three ldx-term sums (<= ldx roundings each), two additions, the
                 division and the rounding of s = -2 l^2: ldx + 4; its relative error times |argument| is the relative error
                 of exp.  4u: exp at <= 1 ulp, the scaling by var, the rounding of the stored norms' last bit, one to spare.
  factor rows    |G_gq - sum_r L_gr L_qr| <= gamma(m + c + 4) (|L||L|^T)_gq + dK_gq       g in [m, m + c), q <= g
  alpha          |y_g - sum_{r<=g} L_gr alpha_r| <= gamma(m + c + 4) (|L||alpha|)_g
  whitened rows  |K_gi - sum_{r<=g} L_gr V_ri| <= gamma(m + c + 4) (|L||V|)_gi + dK_gi
  mu, s2         |mu_out - mu_in - V_new^T alpha_new| <= gamma(c + 2) (|mu_in| + |V_new|^T |alpha_new|)
                 |s2_in - s2_out - colsum(V_new^2)| <= gamma(c + 2) (|s2_in| + colsum(V_new^2))
  cross-cov      |K_ji - (W V)_ji - out_ji| <= gamma(m + 4) (|W||V|)_ji + dK_ji + u |out_ji|

An inner product of at most m + c terms and its subtraction from the right-hand side take at most m + c roundings per term; the
`+ 4` covers the reciprocal-then-multiply the substitution uses in place of a division (two roundings for one), the noise added
to the diagonal and the final rounding.  The constants are operation counts, not fitted to any output.  Every check returns its
largest residual / bound ratio (inf for a non-finite output): a result passes with ratio <= 1."""
import functools
import types

import numpy as np

if np.finfo(np.longdouble).eps <= 2.0 ** -63:
    MODE = "longdouble"
else:
    try:
        import mpmath  # noqa: F401
    except ImportError as e:      # no skip: without an extended type nothing here means anything
        raise RuntimeError("tests/_gp_update_ref.py needs an 80-bit np.longdouble or mpmath") from e
    MODE = "mpmath"

DPS = 50

#: feature count behind every padded length the tests use: the last 16-feature step always holds live features
D_OF = {16: 5, 48: 40, 64: 60, 80: 70, 256: 250, 272: 260, 528: 520}


# ------------------------------------------------------------------------------------------------ the extended type
def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


def xp(a):
    """The FP64 values of `a`, exactly, in the extended type."""
    a = np.asarray(a, dtype=np.float64)
    if MODE == "longdouble":
        return a.astype(np.longdouble)
    out = np.frompyfunc(_mp().mpf, 1, 1)(a)
    return out if isinstance(out, np.ndarray) else np.asarray(out, dtype=object)


def xzeros(shape):
    return xp(np.zeros(shape))


def xexp(a):
    if MODE == "longdouble":
        return np.exp(a)
    return np.frompyfunc(_mp().exp, 1, 1)(a)


def xsqrt(a):
    if MODE == "longdouble":
        return np.sqrt(a)
    return np.frompyfunc(_mp().sqrt, 1, 1)(a)


def rnd(a):
    """Rounded to FP64 (what a host hands to the device)."""
    return np.asarray(a).astype(np.float64)


def unit():
    return xp(2.0 ** -53)


def gamma(k):
    ku = xp(float(k)) * unit()
    return ku / (1 - ku)


def _ratio(resid, bound):
    """max |resid| / bound; a zero bound admits only a zero residual."""
    resid = np.abs(np.atleast_1d(resid))
    bound = np.atleast_1d(bound)
    if resid.size == 0:
        return 0.0
    pos = np.asarray(bound > 0, dtype=bool)
    zero = np.asarray(resid == 0, dtype=bool)
    q = resid / np.where(pos, bound, 1)
    worst = 0.0
    if pos.any():
        worst = float(np.max(q[pos]))
    if (~pos & ~zero).any():
        return float("inf")
    return worst


def _finite(*arrays):
    return all(bool(np.isfinite(np.asarray(a, dtype=np.float64)).all()) for a in arrays)


# ------------------------------------------------------------------------------------------------ reference values
def kernel_ref(Xa, Xb, var, ls):
    """K_ref[i][j] = var exp((|a_i|^2 + |b_j|^2 - 2 a_i.b_j) / (-2 l^2)) of padded FP64 rows and the bound dK on what an
    FP64 evaluation that sums over the padded length may differ by."""
    A, B = xp(Xa), xp(Xb)
    ldx = A.shape[1]
    na, nb = (A * A).sum(axis=1), (B * B).sum(axis=1)
    two_l2 = 2 * xp(ls) * xp(ls)
    K = xp(var) * xexp((na[:, None] + nb[None, :] - 2 * (A @ B.T)) / (-two_l2))
    dA = gamma(ldx + 4) * (na[:, None] + nb[None, :] + 2 * (np.abs(A) @ np.abs(B).T)) / two_l2
    return K, K * (dA + 4 * unit())


def chol_x(G):
    """Lower Cholesky factor in the extended type (column by column)."""
    n = G.shape[0]
    L = xzeros((n, n))
    for j in range(n):
        v = G[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise ValueError("the reference Gram matrix is not positive definite")
        L[j:, j] = v / xsqrt(v[0])
    return L


def solve_lower_x(L, B):
    """L^-1 B in the extended type (row by row)."""
    X = xzeros(B.shape)
    for i in range(L.shape[0]):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


# ------------------------------------------------------------------------------------------------ the checks
def check_structure(L, m, c):
    """Rows [m, m + c) of the factor: finite on columns [0, m + c), a positive diagonal, +0.0 by its bits above the diagonal
    of the new c x c block.  Returns the list of violations."""
    L = np.ascontiguousarray(L, dtype=np.float64)
    bad = []
    if not _finite(L[m:m + c, :m + c]):
        bad.append("non-finite entry in the new rows")
    for j in range(c):
        g = m + j
        if not L[g, g] > 0:
            bad.append("L[%d][%d] = %r is not positive" % (g, g, L[g, g]))
        if (L[g, g + 1:m + c].view(np.int64) != 0).any():
            bad.append("row %d is not +0.0 above the diagonal" % g)
    return bad


def _steps(k, rows):
    if np.isscalar(k):
        return {g: k for g in rows}
    return k


def check_factor(L, rows, G, dK, k):
    """Rows `rows` of the lower factor L against G = K_ref + noise I.  k: m + c + 4, or {row: that count}."""
    rows = list(rows)
    top = max(rows) + 1
    Lf = np.tril(np.asarray(L, dtype=np.float64)[:top, :top])
    if not _finite(Lf):
        return float("inf")
    Lx, k = xp(Lf), _steps(k, rows)
    A = np.abs(Lx)
    worst = 0.0
    for g in rows:
        resid = G[g, :g + 1] - Lx[:g + 1, :g + 1] @ Lx[g, :g + 1]
        bound = gamma(k[g]) * (A[:g + 1, :g + 1] @ A[g, :g + 1]) + dK[g, :g + 1]
        worst = max(worst, _ratio(resid, bound))
    return worst


def factor_bound(L, g, dK, k):
    """The bound of check_factor on row g, columns [0, g]."""
    A = np.abs(xp(np.tril(np.asarray(L, dtype=np.float64)[:g + 1, :g + 1])))
    return gamma(k) * (A @ A[g]) + dK[g, :g + 1]


def check_alpha(L, alpha, y, rows, k):
    rows = list(rows)
    top = max(rows) + 1
    Lf, af = np.tril(np.asarray(L, dtype=np.float64)[:top, :top]), np.asarray(alpha, dtype=np.float64)[:top]
    if not _finite(Lf, af):
        return float("inf")
    Lx, ax, yx, k = xp(Lf), xp(af), xp(y), _steps(k, rows)
    resid = np.array([yx[g] - Lx[g, :g + 1] @ ax[:g + 1] for g in rows])
    bound = np.array([gamma(k[g]) * (np.abs(Lx[g, :g + 1]) @ np.abs(ax[:g + 1])) for g in rows])
    return _ratio(resid, bound)


def check_whiten(L, V, rows, K, dK, k):
    """Rows `rows` of V against the lower factor L (indexed by the same row numbers): K[g][i] = sum_{r <= g} L[g][r] V[r][i].
    K, dK: [row][i] reference kernel values of labelled row g with data row i, and their bound."""
    rows = list(rows)
    top = max(rows) + 1
    Lf, Vf = np.tril(np.asarray(L, dtype=np.float64)[:top, :top]), np.asarray(V, dtype=np.float64)[:top]
    if not _finite(Lf[rows], Vf):
        return float("inf")
    Lx, Vx, k = xp(Lf), xp(Vf), _steps(k, rows)
    Va = np.abs(Vx)
    worst = 0.0
    for g in rows:
        resid = K[g] - Lx[g, :g + 1] @ Vx[:g + 1]
        bound = gamma(k[g]) * (np.abs(Lx[g, :g + 1]) @ Va[:g + 1]) + dK[g]
        worst = max(worst, _ratio(resid, bound))
    return worst


def check_mu_s2(mu_in, mu_out, s2_in, s2_out, Vnew, alpha_new, k):
    """mu and s2 from their values before the call.  k: c + 2.  Returns (ratio of mu, ratio of s2)."""
    if not _finite(mu_in, mu_out, s2_in, s2_out, Vnew, alpha_new):
        return float("inf"), float("inf")
    mi, mo, si, so, Vx, ax = (xp(a) for a in (mu_in, mu_out, s2_in, s2_out, Vnew, alpha_new))
    sq = (Vx * Vx).sum(axis=0)
    r_mu = _ratio(mo - mi - Vx.T @ ax, gamma(k) * (np.abs(mi) + np.abs(Vx).T @ np.abs(ax)))
    r_s2 = _ratio(si - so - sq, gamma(k) * (np.abs(si) + sq))
    return r_mu, r_s2


def check_cross_cov(out, W, V, K, dK, m):
    """out[j][i] = K[j][i] - sum_{r < m} W[j][r] V[r][i]."""
    of, Wf, Vf = (np.asarray(a, dtype=np.float64) for a in (out, np.asarray(W)[:, :m], np.asarray(V)[:m]))
    if not _finite(of, Wf, Vf):
        return float("inf")
    ox, Wx, Vx = xp(of), xp(Wf), xp(Vf)
    resid = K - Wx @ Vx - ox
    bound = gamma(m + 4) * (np.abs(Wx) @ np.abs(Vx)) + dK + unit() * np.abs(ox)
    return _ratio(resid, bound)


# ------------------------------------------------------------------------------------------------ inputs
def pad16(v):
    return (v + 15) // 16 * 16


def padded(rows, ldx):
    out = np.zeros((rows.shape[0], ldx))
    out[:, :rows.shape[1]] = rows
    return out


def draw_rows(kind, count, d, rng):
    """uniform: rows in the unit cube.  neardup: every third row is its predecessor plus 1e-6 noise."""
    X = rng.random((count, d))
    if kind == "neardup":
        for i in range(2, count, 3):
            X[i] = X[i - 1] + 1e-6 * rng.standard_normal(d)
    return X


@functools.lru_cache(maxsize=None)
def state(kind, m, c, ldx, n=0, noise=None, twin_rows=False):
    """One step from known inputs: m + c labelled rows XT (the last c are the new ones) with labels y, n data rows X, and
    the state after the first m rows as the host hands it to the device -- every matrix solved in the extended type from
    K_ref, then rounded to FP64:  L = chol(G_ref) (its first m rows are L11, the last c the exact answer of the append),
    alpha = L^-1 y, V = L^-1 K_ref[T, :].  twin_rows: the data rows are the labelled rows, repeated (predictions at
    labelled points)."""
    d = D_OF[ldx]
    M = m + c
    rng = np.random.default_rng(1000003 * m + 10007 * c + 101 * ldx + n + (7 if kind == "neardup" else 0))
    s = types.SimpleNamespace(kind=kind, m=m, c=c, ldx=ldx, n=n, d=d)
    s.var = 1.0 if kind == "neardup" else 1.3
    s.ls = 0.8 * float(np.sqrt(d / 12.0))
    s.noise = 1e-6 if noise is None else noise
    s.XT = padded(draw_rows(kind, M, d, rng), ldx)
    s.y = np.where(rng.random(M) < 0.5, 1.0, -1.0)
    s.K_TT, s.dK_TT = kernel_ref(s.XT, s.XT, s.var, s.ls)
    s.G = s.K_TT + xp(s.noise) * xp(np.eye(M))
    Lx = chol_x(s.G)
    s.L = rnd(Lx)
    s.alpha = rnd(solve_lower_x(Lx, xp(s.y)[:, None])[:, 0])
    if n:
        if twin_rows:
            X = s.XT[np.arange(n) % M]
        else:
            X = padded(rng.random((n, d)), ldx)
            k = min(n, M, 3)
            X[:k] = s.XT[M - k:]             # labelled rows are data rows: the new ones among them
        s.X = np.ascontiguousarray(X)
        s.K_TX, s.dK_TX = kernel_ref(s.XT, s.X, s.var, s.ls)
        s.V = rnd(solve_lower_x(Lx, s.K_TX))
        # the new rows as SELECTED points of a greedy step: their whitened columns against the first m labelled rows
        s.W = rnd(solve_lower_x(Lx[:m, :m], s.K_TT[:m, m:])).T.copy() if m else np.zeros((c, 0))
    return s


def row_norms64(X):
    return (X * X).sum(axis=1)


# ------------------------------------------------------------------------------------------------ the shapes of the issue
CHOL_PAIRS = ((0, 1), (0, 16), (1, 16), (63, 1), (63, 2), (64, 16), (65, 15), (127, 3), (128, 16), (129, 16), (200, 5))
CHOL_CASES = [(kind, m, c, ldx) for kind, ldx in (("uniform", 16), ("uniform", 48), ("neardup", 16)) for m, c in CHOL_PAIRS] + \
             [("uniform", 65, 15, ldx) for ldx in (256, 272, 528)]
WHITEN_NS = (1, 15, 16, 17, 63, 64, 65, 130)
WHITEN_MC = ((0, 1), (0, 16), (1, 5), (15, 16), (16, 1), (17, 5), (33, 16))
WHITEN_CASES = [(n, m, c, 16) for n in WHITEN_NS for m, c in WHITEN_MC] + [(65, 17, 5, ldx) for ldx in (64, 80, 272)]
CROSS_CASES = [(n, m, c, ldx) for ldx in (16, 80) for n in (1, 17, 65, 130) for c in (1, 5, 16) for m in (1, 15, 16, 17, 33)]
PREDICT_CASES = [(m, nt) for m in (1, 16, 17, 33, 65) for nt in (1, 17, 65)]


def free_form_whiten(n=65, m=17, c=5, ldx=16, seed=5):
    """An arbitrary well-conditioned triangular L22 with random L21, V and alpha (the residual form needs no consistent
    state): the inputs of one whitening sweep."""
    rng = np.random.default_rng(seed)
    d = D_OF[ldx]
    s = types.SimpleNamespace(kind="free", n=n, m=m, c=c, ldx=ldx, d=d, var=1.3, ls=3.0 * float(np.sqrt(2 * d)), noise=0.0)
    s.X, s.XT = padded(3.0 * rng.standard_normal((n, d)), ldx), np.zeros((m + c, ldx))
    s.XT[m:] = padded(3.0 * rng.standard_normal((c, d)), ldx)
    s.L = np.zeros((m + c, m + c))
    s.L[m:, :m] = 0.3 * rng.standard_normal((c, m))
    s.L[m:, m:] = np.tril(0.3 * rng.standard_normal((c, c))) + 2.0 * np.eye(c)
    s.alpha = np.concatenate((np.zeros(m), rng.standard_normal(c)))
    s.V = np.zeros((m + c, n))
    s.V[:m] = 0.1 * rng.standard_normal((m, n))
    s.mu_in, s.s2_in = rng.standard_normal(n), rng.standard_normal(n)
    K, dK = kernel_ref(s.XT[m:], s.X, s.var, s.ls)
    s.K_TX, s.dK_TX = np.concatenate((xzeros((m, n)), K)), np.concatenate((xzeros((m, n)), dK))
    return s


# ------------------------------------------------------------------------------------------------ verdicts per entry point
def judge_chol(s, L, alpha):
    """Ratios of one ital_chol_append from state `s`: L and alpha are the (m + c) x (m + c) factor and the vector after it."""
    rows = range(s.m, s.m + s.c)
    k = s.m + s.c + 4
    bad = check_structure(L, s.m, s.c)
    return dict(structure=float("inf") if bad else 0.0, factor=check_factor(L, rows, s.G, s.dK_TT, k),
                alpha=check_alpha(L, alpha, s.y, rows, k))


def judge_whiten(s, Vout, mu_in, mu_out, s2_in, s2_out):
    """Ratios of one ital_whiten_append: Vout holds rows [0, m + c) of V after the call; the factor rows and alpha_new are the
    state's (s.L, s.alpha: what the call was given)."""
    m, c = s.m, s.c
    rows = range(m, m + c)
    r_mu, r_s2 = check_mu_s2(mu_in, mu_out, s2_in, s2_out, Vout[m:m + c], s.alpha[m:m + c], c + 2)
    return dict(whiten=check_whiten(s.L, Vout, rows, s.K_TX, s.dK_TX, m + c + 4), mu=r_mu, s2=r_s2)


def judge_cross(s, out):
    return dict(cross=check_cross_cov(out, s.W, s.V, s.K_TX[s.m:], s.dK_TX[s.m:], s.m))


def predict_steps(m):
    """{row: operation count} of V rows written in sweeps of 16 labelled rows (ital_predict, GaussianProcess._append)."""
    return {g: min(g // 16 * 16 + 16, m) + 4 for g in range(m)}


def judge_predict(s, Vt, mean, pvar):
    """Ratios of ital_predict (clamp = 0) at the state's data rows as test points, against the whole factor."""
    M = s.m + s.c
    r_mu, r_s2 = check_mu_s2(np.zeros(s.n), mean, np.full(s.n, s.var), pvar, Vt[:M], s.alpha, M + 2)
    return dict(whiten=check_whiten(s.L, Vt, range(M), s.K_TX, s.dK_TX, predict_steps(M)), mu=r_mu, s2=r_s2)


# ------------------------------------------------------------------------------------------------ FP64 emulation
# Straightforward NumPy FP64 versions of the three operations: a row-by-row append, a forward substitution, K - W V.  They
# show that the bounds admit a correct FP64 implementation (soundness); with `defect` they make the mistakes the device
# kernels can make, which the checks must reject (sharpness).
CHOL_DEFECTS = ("cross_block", "last_column", "alpha_l21", "perturb")
SWEEP_DEFECTS = ("wv_slice", "partial_step", "wrong_ld")


def emu_kernel(Xa, na, Xb, nb, var, ls, defect=None):
    ldx = Xa.shape[1]
    kk = ldx // 64 * 64 if defect == "partial_step" else ldx      # the last partial trip of four 16-feature steps skipped
    return var * np.exp((na[:, None] + nb[None, :] - 2.0 * (Xa[:, :kk] @ Xb[:, :kk].T)) / (-2.0 * ls * ls))


def emu_chol_append(XT, XTn, L, alpha, ynew, m, c, var, ls, noise, defect=None):
    """Appends rows [m, m + c) to copies of L and alpha.  Reads the lower triangle of rows < m only.  Returns L, alpha, status.
    defect: cross_block  the substitution of an old column q >= 64 forgets the columns solved in earlier 64-column blocks
            last_column  the last column of every 64-column block is left without its division
            alpha_l21    alpha_new without the L21 alpha term
            perturb      L[m][m // 2] off by a relative 1e-11"""
    L, alpha, status = L.copy(), alpha.copy(), 0
    with np.errstate(invalid="ignore"):
        for j in range(c):
            g = m + j
            k = emu_kernel(XT[g:g + 1], XTn[g:g + 1], XT[:g + 1], XTn[:g + 1], var, ls)[0]
            k[g] += noise
            row = np.zeros(g + 1)
            for q in range(g):
                lo = q // 64 * 64 if defect == "cross_block" and q < m else 0
                v = k[q] - row[lo:q] @ L[q, lo:q]
                row[q] = v if defect == "last_column" and q < m and (q % 64 == 63 or q == m - 1) else v / L[q, q]
            dgg = k[g] - row[:g] @ row[:g]
            if not dgg > 0:
                status |= 1
            row[g] = np.sqrt(dgg)
            L[g, :g + 1] = row
            L[g, g + 1:m + c] = 0.0
            lo = m if defect == "alpha_l21" else 0
            alpha[g] = (ynew[j] - row[lo:g] @ alpha[lo:g]) / row[g]
    if defect == "perturb":
        L[m, m // 2] *= 1.0 + 1e-11
    return L, alpha, status


def _wv(W, V, m, defect):
    mm = (m - 1) // 16 * 16 if defect == "wv_slice" and m else m      # the last 16-row slice skipped
    return W[:, :mm] @ V[:mm]


def emu_whiten(X, xn, Xnew, snew, Lrows, ldw, alpha_new, V, mu, s2, m, c, var, ls, defect=None):
    """Lrows: the c new rows of the factor as a flat buffer of leading dimension ldw (L21 = columns [0, m), L22 from column
    m).  Returns copies of V, mu, s2 with rows [m, m + c) appended.  defect: wv_slice, partial_step, or wrong_ld (L22 read
    with leading dimension ldw - 1)."""
    flat = np.asarray(Lrows, dtype=np.float64).ravel()
    ld22 = ldw - 1 if defect == "wrong_ld" else ldw
    W = flat[:c * ldw].reshape(c, ldw)
    R = emu_kernel(Xnew, snew, X, xn, var, ls, defect) - _wv(W, V, m, defect)
    Vn = np.zeros((c, X.shape[0]))
    for j in range(c):
        acc = R[j].copy()
        for q in range(j):
            acc -= flat[m + j * ld22 + q] * Vn[q]
        Vn[j] = acc / flat[m + j * ld22 + j]
    V = V.copy()
    V[m:m + c] = Vn
    return V, mu + Vn.T @ alpha_new, s2 - (Vn * Vn).sum(axis=0)


def emu_cross_cov(X, xn, Xs, sn, W, V, m, var, ls, defect=None):
    return emu_kernel(Xs, sn, X, xn, var, ls, defect) - _wv(W, V, m, defect)


def emu_predict(Xt, XT, XTn, L, alpha, m, var, ls):
    """ital_predict without the clamp: sweeps of 16 labelled rows.  Returns Vt, mean, pvar."""
    nt = Xt.shape[0]
    xtn = row_norms64(Xt)
    Vt, mean, pvar = np.zeros((m, nt)), np.zeros(nt), np.full(nt, float(var))
    for c0 in range(0, m, 16):
        c = min(16, m - c0)
        rows = np.ascontiguousarray(L[c0:c0 + c, :m])
        Vt, mean, pvar = emu_whiten(Xt, xtn, XT[c0:c0 + c], XTn[c0:c0 + c], rows, m, alpha[c0:c0 + c], Vt, mean, pvar, c0, c,
                                    var, ls)
    return Vt, mean, pvar
