"""Extended-precision model of ital_gp_influence / ital_gp_preview_remove (include/ital_influence.h) and a checker whose
bounds are computed from the inputs alone -- no tuned constant.

The model (np.longdouble) computes every output two ways: by the closed forms of the header, and by brute force (delete row
and column i of K and fit again).  The checker judges a result (the device's, or `evaluate`, the float64 statement of the
device algorithm that the host tests feed it) in two stages, u = 2^-53, gamma_k = k u / (1 - k u):

Stage 1 (M = L^-1, c, w) against longdouble from L.  Forward substitution gives (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., section 8.1, Theorem 8.5 applied to the columns of the inverse)  |fl(M) - M| <= E = gamma_m |M||L||M| /
(1 - gamma_m cond(L)), cond(L) = || |L^-1||L| ||_inf computed here on the host.  That is the bound on the ENTRIES of M; c and w
are sums over them and inherit, by the same propagation as stage 2,
    |fl(c_i) - c_i| <= sum_p (2 |M_pi| E_pi + E_pi^2) + gamma_{m+1} sum_p (|M_pi| + E_pi)^2
    |fl(w_i) - w_i| <= sum_p E_pi |alpha_p| + gamma_m sum_p (|M_pi| + E_pi) |alpha_p|.
(The one-line form cond(L) gamma_m |value| cannot hold as it stands: at m = 1, c = fl(fl(1 / L)^2) has two roundings, which
is more than gamma_1 = u allows any implementation.)

Stage 2 against the model fed the result's OWN M, c and w, so that its only error is the dot product:
|fl(B_ij) - B_ij| <= eB_ij = gamma_m sum_p |M_pi| |V_pj| for any summation order, with or without FMA.  Every output then has
an interval: with lo = max(|B| - eB, 0), hi = |B| + eB, r = w / c, n the counted rows and g = (1 + gamma_8)(1 + gamma_{n+1})
(eight roundings cover r, its square, the squares of B and the final products and quotient in either order of evaluation;
gamma_{n+1} covers the sum over j in any order),
    r^2 sum lo^2 / g <= dmu_sq <= g r^2 sum hi^2          |r| max lo / (1 + gamma_8) <= dmu_max <= (1 + gamma_8) |r| max hi
    sum lo^2 / (c g) <= ds2 <= g sum hi^2 / c
    |fl(mu') - mu'| <= bmu = |r| eB + 4 u |r| hi + u (|mu| + |r| hi)
    |fl(s2') - s2'| <= (2 |B| eB + eB^2) / c + 4 u hi^2 / c + u (|s2| + hi^2 / c)
A row j with |mu'_ij| <= bmu_ij is ambiguous for flips_i: the result must lie between the certain flips and the certain flips
plus the ambiguous rows.  A row whose c is not finite or not > 0 must be NaN in all six outputs, with status bit 1 set."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def gamma(k):
    return LD(k) * LD(U) / (1 - LD(k) * LD(U))


# ------------------------------------------------------------------------------------------------ longdouble linear algebra
def tri_inverse(L):
    """L^-1 of a lower triangular matrix, row by row (any float type: the result has L's)."""
    m = len(L)
    M = np.zeros_like(L)
    for j in range(m):
        row = -(L[j, :j] @ M[:j]) if j else np.zeros(m, dtype=L.dtype)
        row[j] = 1
        M[j, :j + 1] = row[:j + 1] / L[j, j]             # the strict upper triangle stays 0 whatever the pivot is
    return M


def cholesky(K):
    K = np.array(K, dtype=LD)
    m = len(K)
    L = np.zeros((m, m), dtype=LD)
    for j in range(m):
        L[j, j] = np.sqrt(K[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_spd(K, B):
    """K^-1 B in longdouble (Cholesky)."""
    M = tri_inverse(cholesky(K))
    return M.T @ (M @ np.asarray(B, dtype=LD))


# ------------------------------------------------------------------------------------------------------------- fixtures
class Case(object):
    """Inputs of one call: the arrays as the device sees them (cap > m rows, ldv > n columns, poisoned outside m x n)."""

    def __init__(self, m, n, seed=0, poison=np.nan, zero_pivot=None, mask="none"):
        rng = np.random.default_rng(1000 * m + n + 7919 * seed)
        self.m, self.n, self.cap, self.ldv = m, n, m + 3, n + 5
        L = np.full((self.cap, self.cap), poison)
        low = np.tril(rng.standard_normal((m, m)), -1) * (0.5 / np.sqrt(m))
        L[:m, :m] = low + np.diag(1.0 + rng.random(m))
        L[:m, :m][np.triu_indices(m, 1)] = poison      # the strict upper triangle is not read either
        if zero_pivot is not None:
            L[zero_pivot, zero_pivot] = 0.0
        self.zero_pivot = zero_pivot
        V = np.full((self.cap, self.ldv), poison)
        V[:m, :n] = rng.standard_normal((m, n))
        self.L, self.V = L, V
        self.alpha = np.concatenate([rng.standard_normal(m), np.full(3, poison)])
        mu = rng.standard_normal(n)
        mu[::7] = 0.0                                  # exact zeros: `>` and `>=` differ there
        self.mu = np.concatenate([mu, np.full(5, poison)])
        self.s2 = np.concatenate([0.1 + rng.random(n), np.full(5, poison)])
        self.mask = {"none": None, "zero": np.zeros(n, dtype=np.uint8),
                     "random": (rng.random(n) < 0.6).astype(np.uint8)}[mask]

    def counted(self):
        return np.ones(self.n, dtype=bool) if self.mask is None else self.mask != 0


def gp_case(m, n, seed=0, noise=1e-2, d=3):
    """A consistent GP state in longdouble -- K, K_S,: , y and the derived L, alpha, V, mu, s2 -- for closed form vs brute force."""
    rng = np.random.default_rng(seed)
    X = rng.random((n, d)).astype(LD)
    S = rng.choice(n, m, replace=False)
    D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    Kall = np.exp(-D / LD(2 * 0.3 ** 2))
    K = Kall[np.ix_(S, S)] + LD(noise) * np.eye(m, dtype=LD)
    Ks = Kall[S]
    y = np.where(rng.random(m) < 0.5, LD(1), LD(-1))
    L = cholesky(K)
    M = tri_inverse(L)
    alpha, V = M @ y, M @ Ks
    return dict(K=K, Ks=Ks, y=y, L=L, alpha=alpha, V=V, mu=V.T @ alpha, s2=1 - (V * V).sum(0), S=S)


# ------------------------------------------------------------------------------------------------- the model, two ways
def closed_form(L, alpha, V, mu, s2):
    """(c, w, B, mu'[m][n], s2'[m][n]) by the closed forms, in the type of the inputs (longdouble in the tests)."""
    M = tri_inverse(L)
    c = (M * M).sum(0)
    w = M.T @ alpha
    B = M.T @ V
    return c, w, B, mu[None, :] - (w / c)[:, None] * B, s2[None, :] + B * B / c[:, None]


def brute_force(K, Ks, y, var=1):
    """(loo_mean, loo_var, mu'[m][n], s2'[m][n]): delete row and column i of K and fit again, for every i."""
    m, n = Ks.shape
    mu1, s21 = np.zeros((m, n), dtype=LD), np.zeros((m, n), dtype=LD)
    loo_mean, loo_var = np.zeros(m, dtype=LD), np.zeros(m, dtype=LD)
    for i in range(m):
        keep = np.delete(np.arange(m), i)
        if len(keep) == 0:
            mu1[i], s21[i] = 0, var
            loo_mean[i], loo_var[i] = 0, K[i, i]
            continue
        Kk, Kr = K[np.ix_(keep, keep)], Ks[keep]
        mu1[i] = Kr.T @ solve_spd(Kk, y[keep])
        s21[i] = var - (Kr * solve_spd(Kk, Kr)).sum(0)
        ki = K[keep, i]
        loo_mean[i] = ki @ solve_spd(Kk, y[keep])
        loo_var[i] = K[i, i] - ki @ solve_spd(Kk, ki)       # variance of the noisy target: K carries the noise
    return loo_mean, loo_var, mu1, s21


# ---------------------------------------------------------------------------- float64 statement of the device algorithm
def evaluate(case, sel=None, mistake=None):
    """What the kernels compute, in float64 numpy, as a dict like the device result (M, c, w, coef, stats, status, and
    mu_out / s2_out for `sel`).  `mistake`: one of MISTAKES, planted."""
    m, n = case.m, case.n
    rows = m + 1 if mistake == "row_m_read" else m
    L = case.L[:m, :m]
    with np.errstate(all="ignore"):
        M = tri_inverse(np.tril(L))
        c = (M * M).sum(0)
        w = np.array([M[i:, i] @ case.alpha[i:m] for i in range(m)])
        Mt = np.zeros((m, rows))
        Mt[:, :m] = np.tril(M, -1).T if mistake == "strict_triangle" else np.tril(M).T
        Vr = case.V[:rows, :n].copy()
        if rows > m:
            Mt[:, m] = 1.0                                # what a kernel that runs k past m picks up: whatever lies there
            Vr[m] = np.where(np.isfinite(Vr[m]), Vr[m], 1.0)
        B = Mt @ Vr
        r = w / c
        on = np.ones(n, dtype=bool) if (mistake == "mask_ignored" or case.mask is None) else case.mask != 0
        mu, s2 = case.mu[:n], case.s2[:n]
        sign = 1.0 if mistake == "wrong_sign" else -1.0
        mu1 = mu[None, :] + sign * r[:, None] * B
        inv_c = np.ones(m) if mistake == "missing_inv_c" else 1.0 / c
        d = sign * r[:, None] * B
        Bo = B[:, on]
        stats = np.zeros((m, 4))
        stats[:, 0] = (d[:, on] ** 2).sum(1)
        if on.any():
            stats[:, 1] = d[:, on].max(1).clip(0) if mistake == "signed_max" else np.abs(d[:, on]).max(1)
        before = mu[on] >= 0 if mistake == "flip_ge" else mu[on] > 0
        after = mu1[:, on] >= 0 if mistake == "flip_ge" else mu1[:, on] > 0
        stats[:, 2] = (before[None, :] != after).sum(1)
        stats[:, 3] = (Bo * Bo).sum(1) * inv_c
        bad = ~(np.isfinite(c) & (c > 0))
        coef = np.stack([c, w], 1)
        coef[bad], stats[bad] = np.nan, np.nan
        out = dict(M=M, c=c, w=w, coef=coef, stats=stats, status=int(bad.any()))
        if sel is not None:
            sel = np.asarray(sel)
            out["mu_out"] = mu1[sel]
            out["s2_out"] = (s2[None, :] + B * B * inv_c[:, None])[sel]
            out["mu_out"][bad[sel]] = np.nan
            out["s2_out"][bad[sel]] = np.nan
    return out


#: the sizes of the kernel tests: both sides of one and two 128-row tiles, of the 16-wide k-stage and of one 128-column tile
M_SIZES = (1, 2, 16, 17, 129, 257)
N_SIZES = (1, 17, 128, 129, 300)
MASKS = ("none", "zero", "random")


def grid():
    """(m, n, mask) over all sizes, the three masks taking turns."""
    return [(m, n, MASKS[(a + b) % 3]) for a, m in enumerate(M_SIZES) for b, n in enumerate(N_SIZES)]


def selection(m):
    """First, last, middle and a repeated position."""
    return [0, m - 1, m // 2, m - 1]


MISTAKES = ("missing_inv_c", "wrong_sign", "mask_ignored", "strict_triangle", "flip_ge", "signed_max", "row_m_read")


# --------------------------------------------------------------------------------------------------------- the checker
class Mismatch(AssertionError):
    pass


def _need(ok, what, *figures):
    if not np.all(ok):
        raise Mismatch("%s: %s" % (what, ", ".join(repr(f) for f in figures)))


def stage1_reference(case):
    """(M, c, w, eM, ec, ew) in longdouble from the case's L and alpha, with the bounds of the module docstring."""
    m = case.m
    L = np.tril(case.L[:m, :m]).astype(LD)
    al = case.alpha[:m].astype(LD)
    with np.errstate(all="ignore"):
        return _stage1(m, L, al)


def _stage1(m, L, al):
    M = tri_inverse(L)
    aM, aL = np.abs(M), np.abs(L)
    cond = (aM @ aL).sum(1).max()
    g = gamma(m)
    E = g * (aM @ aL @ aM) / (1 - g * cond)
    c, w = (M * M).sum(0), M.T @ al
    ec = (2 * aM * E + E * E).sum(0) + gamma(m + 1) * ((aM + E) ** 2).sum(0)
    ew = E.T @ np.abs(al) + g * ((aM + E).T @ np.abs(al))
    return M, c, w, E, ec, ew, cond


def ambiguous_rows(case, res):
    """Number of (i, j), j counted, whose flip the bounds cannot decide, from the result's own M, c, w."""
    return _stage2(case, res)["ambiguous"].sum()


def _stage2(case, res):
    m, n = case.m, case.n
    M = np.tril(np.asarray(res["M"], dtype=np.float64)[:m, :m]).astype(LD)
    c, w = np.asarray(res["c"], dtype=np.float64).astype(LD), np.asarray(res["w"], dtype=np.float64).astype(LD)
    good = np.isfinite(res["c"]) & (np.asarray(res["c"]) > 0)
    V = case.V[:m, :n].astype(LD)
    Mg = np.where(good[None, :], M, 0)                   # columns of broken rows: not judged
    B = Mg.T @ V
    eB = gamma(m) * (np.abs(Mg).T @ np.abs(V))
    with np.errstate(all="ignore"):
        r = np.where(good, w / np.where(good, c, 1), 0)
    lo, hi = np.maximum(np.abs(B) - eB, 0), np.abs(B) + eB
    mu, s2 = case.mu[:n].astype(LD), case.s2[:n].astype(LD)
    ar = np.abs(r)[:, None]
    mu1 = mu[None, :] - r[:, None] * B
    bmu = ar * eB + 4 * LD(U) * ar * hi + LD(U) * (np.abs(mu)[None, :] + ar * hi)
    cc = np.where(good, c, 1)[:, None]
    s21 = s2[None, :] + B * B / cc
    bs2 = (2 * np.abs(B) * eB + eB * eB) / cc + 4 * LD(U) * hi * hi / cc + LD(U) * (np.abs(s2)[None, :] + hi * hi / cc)
    on = case.counted()
    amb = (np.abs(mu1) <= bmu) & on[None, :] & good[:, None]
    flip = ((mu > 0)[None, :] != (mu1 > 0)) & on[None, :]
    return dict(good=good, B=B, lo=lo, hi=hi, r=r, c=cc[:, 0], mu1=mu1, bmu=bmu, s21=s21, bs2=bs2, on=on, ambiguous=amb,
                certain=(flip & ~amb).sum(1), maybe=amb.sum(1))


def check(case, res, sel=None, flips=True):
    """Raises Mismatch unless `res` (M, c, w, coef, stats, status and, with `sel`, mu_out, s2_out) is within the bounds."""
    m, n = case.m, case.n
    M, c, w, E, ec, ew, cond = stage1_reference(case)
    dM = np.tril(np.asarray(res["M"])[:m, :m])
    finite = np.isfinite(c) & (c > 0) if case.zero_pivot is None else np.arange(m) > case.zero_pivot
    # ---- stage 1: rows after a planted zero pivot never meet it (column i of M involves rows >= i of L only)
    if case.zero_pivot is None:
        _need(np.abs(dM - M) <= E, "M outside the triangular-inverse bound", float(np.max(np.abs(dM - M) - E)))
        _need(np.abs(res["c"] - c) <= ec, "c outside its bound", np.abs(res["c"] - c).astype(float), ec.astype(float))
        _need(np.abs(res["w"] - w) <= ew, "w outside its bound", np.abs(res["w"] - w).astype(float), ew.astype(float))
    good = np.isfinite(res["c"]) & (np.asarray(res["c"]) > 0)
    _need(good[finite], "a sound row was flagged", good)
    if case.zero_pivot is not None:
        _need(~good[: case.zero_pivot + 1], "rows at or before the zero pivot must be broken", good)
    _need(int(res["status"]) & 1 == int((~good).any()), "status bit", res["status"])
    coef, stats = np.asarray(res["coef"]), np.asarray(res["stats"])
    _need(np.isnan(coef[~good]).all() and np.isnan(stats[~good]).all(), "a broken row must be NaN in all six outputs")
    _need(coef[good, 0] == np.asarray(res["c"])[good], "coef[:, 0] is c")
    _need(coef[good, 1] == np.asarray(res["w"])[good], "coef[:, 1] is w")
    # ---- stage 2
    s = _stage2(case, res)
    on, r, cc = s["on"], s["r"], s["c"]
    cnt = int(on.sum())
    g8 = 1 + gamma(8)
    g = g8 * (1 + gamma(cnt + 1))
    lo2, hi2 = (s["lo"][:, on] ** 2).sum(1), (s["hi"][:, on] ** 2).sum(1)
    mlo = s["lo"][:, on].max(1) if cnt else np.zeros(m, dtype=LD)
    mhi = s["hi"][:, on].max(1) if cnt else np.zeros(m, dtype=LD)
    st = stats.astype(LD)
    k = good
    _need((st[k, 0] >= r[k] ** 2 * lo2[k] / g) & (st[k, 0] <= g * r[k] ** 2 * hi2[k]), "dmu_sq outside its interval",
          stats[k, 0], (r ** 2 * lo2).astype(float)[k], (r ** 2 * hi2).astype(float)[k])
    _need((st[k, 1] >= np.abs(r[k]) * mlo[k] / g8) & (st[k, 1] <= g8 * np.abs(r[k]) * mhi[k]), "dmu_max outside its interval",
          stats[k, 1], (np.abs(r) * mlo).astype(float)[k], (np.abs(r) * mhi).astype(float)[k])
    _need((st[k, 3] >= lo2[k] / (cc[k] * g)) & (st[k, 3] <= g * hi2[k] / cc[k]), "ds2 outside its interval",
          stats[k, 3], (lo2 / cc).astype(float)[k], (hi2 / cc).astype(float)[k])
    if flips and m >= 2:
        _need((st[k, 2] >= s["certain"][k]) & (st[k, 2] <= s["certain"][k] + s["maybe"][k]), "flips outside its range",
              stats[k, 2], s["certain"][k], s["maybe"][k])
    if sel is not None:
        sel = np.asarray(sel)
        mo, so = np.asarray(res["mu_out"])[:, :n], np.asarray(res["s2_out"])[:, :n]
        gs = good[sel]
        _need(np.isnan(mo[~gs]).all() and np.isnan(so[~gs]).all(), "preview of a broken row must be NaN")
        _need(np.abs(mo[gs] - s["mu1"][sel][gs]) <= s["bmu"][sel][gs], "mu' outside its bound",
              float(np.max(np.abs(mo[gs] - s["mu1"][sel][gs]) - s["bmu"][sel][gs], initial=-np.inf)))
        _need(np.abs(so[gs] - s["s21"][sel][gs]) <= s["bs2"][sel][gs], "s2' outside its bound",
              float(np.max(np.abs(so[gs] - s["s21"][sel][gs]) - s["bs2"][sel][gs], initial=-np.inf)))
    return s
