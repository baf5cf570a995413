"""Extended-precision host reference and checker of the MCMI kernels -- ital_cov_block, ital_cov_abs_rowsum,
ital_mcmi_score_step (include/ital_hip.h, ital_amd/csrc/mcmi.hip) -- shared by tests/test_mcmi_ref_host.py and
tests/test_gpu_mcmi_kernels.py.  Plain NumPy, no GPU, no project import.  Not a test module.

The extended type (long double, mpmath at 50 digits where long double is only 64 bits wide), u = 2^-53, gamma(k) and the kernel
reference with its bound dK are those of tests/_gp_update_ref.py.  Every checker returns its largest residual / bound ratio, inf
for a non-finite output where a finite one is due (and for a finite one where NaN is due): a result passes with ratio <= 1.  The
constants below are operation counts and published accuracies; none is fitted to an output of the device or of the emulation.

Covariance block   out_ij = K_ij - sum_{r<m} Va_ri Vb_rj
    |out - ref| <= dK + gamma(m + 2) (|Va|^T |Vb|) + u |out|
    The m products and their additions into the accumulator that already holds the kernel value are at most m + 1 roundings
    (fewer where the matrix cores fuse them); one more covers the final store.  The norms are inputs: the 4u of dK allow their
    last bit.

Absolute row sum   out_i = prior_i + sum_j |ref_ij|
    |out - ref| <= sum_j (dK + gamma(m + 2) |Va|^T|Vb|)_ij + gamma(nb + nsplit + 1) sum_j |ref_ij| + u |prior_i|
    ||a| - |b|| <= |a - b| carries the block bound through the absolute value; a row sum is nb additions however they are
    split among lanes and column splits, nsplit more in the reduction, one for the prior.

Conditional entropy   ce_i = min_r sum_{j not a member} h(z_jr),  h(z) = q log(q + eps) + (1 - q) log(1 - q + eps),  q = Phi(z)
    A first-order forward bound, T = t, all magnitudes taken from the reference (extended type):
    W    G = Sigma_S + noise I = L L^T, X = L^-1, W = X^T X.  Higham Thm 10.3: L_hat L_hat^T = G + dG, |dG| <= gamma(T + 1)
         |L||L^T|, one more rounding for the noise on the diagonal; the triangular inverse by substitution (ch. 14, Method 1):
         |X_hat - L_hat^-1| <= gamma(T) |X||L||X|; the product X^T X: gamma(T) |X^T||X|.  To first order
         dW = gamma(T + 2) |W|(|L||L^T|)|W| + gamma(T) (|X^T|(|X||L||X|) + transposed) + gamma(T) |X^T||X|
    u    u_j = W c_j, T-term FMAs: du = dW |c| + gamma(T) |W||c|
    s'   quad = c.u: dquad = |c|.du + gamma(T) |c|.|u|;  s' = s2 - quad: ds = dquad + u |s'|
    base mu_j - sum_p u_p mu_S,p: dbase = |mu_S|.du + gamma(T + 1) B,  B = |mu_j| + |mu_S|.|u|
    val  the 2^T pattern values mu_j + u.(y_r - mu_S) are built from base by at most T additions of +-u_p and T of +2u_p, every
         partial sum bounded by B + sum_p |u_p|: dval = dbase + sum_p du_p + gamma(2T) (B + sum_p |u_p|)
    z    z = -val / sqrt(s'): the square root, the reciprocal and the product are 3 roundings, one to spare:
         dz = dval / sqrt(s') + |z| (ds / (2 s') + 4u)
    h    through h'(z) = phi(z) D(z), D = log((q + eps)/(1 - q + eps)) + q/(q + eps) - (1 - q)/(1 - q + eps), and the
         evaluation of h itself: Phi to PHI_ABS = 1e-15 absolute (the published accuracy of MVNPHI, Hart et al. 5666, which the
         host test confirms on the FP64 rational) plus the rounding of 1 - q; each logarithm to 2u relative with its argument
         rounded once, each product and the sum once:
         dh = phi |D| dz + |D| (PHI_ABS + u) + 4u (|q log(q + eps)| + |(1 - q) log(1 - q + eps)|) + 2u
    sum  256 threads stride over j, 6 shuffle levels, 2 levels across the waves: depth = ceil(n_all / 256) + 8
         dce_r = sum_j dh_jr + gamma(depth) sum_j |h_jr|
    min  |min_r a_r - min_r b_r| <= max_r |a_r - b_r|: the verdict is |ce - min_r ref_r| <= max_r dce_r.
    The value is NaN iff some non-member j has s'_j <= 0 (the cases keep |s'_j| >= 1e-6 there, far above ds).  Dead candidates
    must still hold the canary, by bits."""
import functools
import itertools
import math
import types

import numpy as np

from _gp_update_ref import (MODE, DPS, xp, xzeros, xexp, xsqrt, rnd, unit, gamma, _ratio, kernel_ref, chol_x,  # noqa: F401
                            solve_lower_x, padded)

PHI_ABS = 1e-15        # MVNPHI: "normal distribution probabilities accurate to 1e-15" (Genz; Hart et al. algorithm 5666)
CANARY = -12345.678    # what ce[] holds before a call

# ------------------------------------------------------------------------------------------------ routes of ital_cov_block
# Restates the three conditions of ital_cov_block and the split count of ital_cov_abs_rowsum in ital_amd/csrc/mcmi.hip
# (ITAL_COV_SMALL_BELOW = 512, ITAL_COV_LDS_MIN_TILES = 1024, tiles of 128 x 64 and 128 x 128): keep in step with that file.
COV_SMALL_BELOW, COV_LDS_MIN_TILES = 512, 1024


def _cdiv(a, b):
    return -(-a // b)


def expected_route(na, nb):
    if _cdiv(na, 128) * _cdiv(nb, 128) >= COV_LDS_MIN_TILES:
        return "lds"
    if _cdiv(na, 128) * _cdiv(nb, 64) < COV_SMALL_BELOW:
        return "small"
    return "default"


def expected_nsplit(na, nb, work_len):
    """Column splits of ital_cov_abs_rowsum (keep in step with mcmi.hip) and the number of 64-column tiles."""
    ntile = _cdiv(nb, 64)
    return min(_cdiv(4096, _cdiv(na, 128)), ntile, work_len // na, 65535), ntile


# ------------------------------------------------------------------------------------------------ the extended functions
def xlog(a):
    if MODE == "longdouble":
        return np.log(a)
    import mpmath
    return np.frompyfunc(mpmath.log, 1, 1)(a)


def _erfc_pos(x):
    """erfc(x) for an array x >= 0 of long doubles.  Below 1: 1 - erf(x) with erf = 2/sqrt(pi) e^-x^2 sum_n 2^n x^(2n+1) / (2n+1)!!
    (all terms positive; erfc >= 0.157 there, so the subtraction costs under one digit).  From 1 on: the continued fraction
    e^-x^2 / sqrt(pi) / (x + (1/2) / (x + 1 / (x + (3/2) / (x + ...)))) evaluated backwards, 400 levels below 3 and 150 beyond
    (converged to the type's precision; the host test compares with mpmath).  The rounding of x^2 in the exponent leaves a
    relative error of up to 2.5 x^2 eps."""
    x = np.asarray(x, dtype=np.longdouble)
    out = np.empty_like(x)
    root_pi = np.sqrt(4 * np.arctan(np.longdouble(1)))
    lo = x < 1
    if lo.any():
        xs = x[lo]
        term = xs.copy()
        s = xs.copy()
        for n in range(1, 60):
            term = term * (2 * xs * xs) / (2 * n + 1)
            s = s + term
        out[lo] = 1 - 2 / root_pi * np.exp(-xs * xs) * s
    for sel, levels in ((~lo & (x < 3), 400), (x >= 3, 150)):
        if sel.any():
            xb = x[sel]
            f = xb.copy()
            for k in range(levels, 0, -1):
                f = xb + (np.longdouble(k) / 2) / f
            out[sel] = np.exp(-xb * xb) / (root_pi * f)
    return out


def phi_pair(z):
    """(Phi(z), 1 - Phi(z)) in the extended type, each to a relative (40 + 2 z^2) eps of the type.  Where the 80-bit long double
    exists every term takes the vectorised long-double erfc above, whatever the term count -- not mpmath for the small counts
    and the long double for the large ones: one route, pinned as a whole to mpmath.ncdf at 50 digits by
    tests/test_mcmi_ref_host.py.  mpmath evaluates the terms only where long double is 64 bits wide."""
    if MODE != "longdouble":
        import mpmath
        return np.frompyfunc(mpmath.ncdf, 1, 1)(z), np.frompyfunc(lambda v: mpmath.ncdf(-v), 1, 1)(z)
    z = np.asarray(z, dtype=np.longdouble)
    tail = _erfc_pos(np.abs(z).ravel() / np.sqrt(np.longdouble(2))).reshape(z.shape) / 2
    neg = z <= 0
    return np.where(neg, tail, 1 - tail), np.where(neg, 1 - tail, tail)


# Hart et al. 5666 as MVNPHI evaluates it (Genz), in FP64 NumPy: what the host test measures PHI_ABS on.
_HP = (220.2068679123761, 221.2135961699311, 112.0792914978709, 33.91286607838300, 6.373962203531650, .7003830644436881,
       .03526249659989109)
_HQ = (440.4137358247522, 793.8265125199484, 637.3336333788311, 296.5642487796737, 86.78073220294608, 16.06417757920695,
       1.755667163182642, .08838834764831844)


def mvnphi64(z):
    z = np.asarray(z, dtype=np.float64)
    a = np.abs(z)
    num, den = np.full_like(a, _HP[6]), np.full_like(a, _HQ[7])
    for c in _HP[5::-1]:
        num = num * a + c
    for c in _HQ[6::-1]:
        den = den * a + c
    ex = np.exp(-a * a / 2)
    cf = a + 1 / (a + 2 / (a + 3 / (a + 4 / (a + 0.65))))
    p = np.where(a > 37, 0.0, np.where(a < 7.071067811865475, ex * num / den, ex / (cf * 2.506628274631001)))
    return np.where(z > 0, 1 - p, p)


# ------------------------------------------------------------------------------------------------ covariance block, row sum
def block_ref(Xa, Xb, Va, Vb, m, var, ls):
    """(ref, bound without the store term) of K - Va^T Vb in the extended type."""
    K, dK = kernel_ref(Xa, Xb, var, ls)
    if m:
        A, B = xp(np.asarray(Va)[:m]), xp(np.asarray(Vb)[:m])
        return K - A.T @ B, dK + gamma(m + 2) * (np.abs(A).T @ np.abs(B))
    return K, dK


def cov_block_check(out, Xa, an, Xb, bn, Va, Vb, m, var, ls):
    """an, bn are what the device was given beside the rows; the reference forms the norms from the rows itself."""
    out = np.asarray(out, dtype=np.float64)
    if not np.isfinite(out).all():
        return float("inf")
    ref, bound = block_ref(Xa, Xb, Va, Vb, m, var, ls)
    ox = xp(out)
    return _ratio(ox - ref, bound + unit() * np.abs(ox))


def rowsum_check(out, prior, Xa, an, Xb, bn, Va, Vb, m, var, ls, nsplit):
    """prior: what out held before an accumulating call, zeros otherwise."""
    out = np.asarray(out, dtype=np.float64)
    if not np.isfinite(out).all():
        return float("inf")
    nb = np.asarray(Xb).shape[0]
    px = xp(prior)
    if nb == 0:
        return _ratio(xp(out) - px, xzeros(out.shape))
    ref, bound = block_ref(Xa, Xb, Va, Vb, m, var, ls)
    tot = np.abs(ref).sum(axis=1)
    return _ratio(xp(out) - px - tot, bound.sum(axis=1) + gamma(nb + nsplit + 1) * tot + unit() * np.abs(px))


def negative_share(Xa, Xb, Va, Vb, m, var, ls):
    ref, _ = block_ref(Xa, Xb, Va, Vb, m, var, ls)
    return float(np.mean(np.asarray(ref < 0, dtype=bool)))


def _frozen(s):
    """The arrays of a cached namespace made read-only: every test that asks for the same inputs gets the same object."""
    for v in vars(s).values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return s


COV_DEFECTS = ("last16", "mquad", "sign", "swap", "ragged_norm")
ROWSUM_DEFECTS = COV_DEFECTS + ("noabs", "skip_tile", "no_accumulate")


def emu_cov_block(Xa, an, Xb, bn, Va, Vb, m, var, ls, defect=None):
    """Plain FP64: var exp((|a|^2 + |b|^2 - 2 a.b) / (-2 l^2)) - Va^T Vb.
    defect: last16       the last 16-feature step dropped when ldx / 16 is odd
            mquad        the last partial quadruple of the m whitened rows dropped
            sign         the whitened part added
            swap         Va and Vb exchanged (indices wrapped into the other block's width)
            ragged_norm  the last row (column) of a ragged block takes the norm of the row (column) before it"""
    na, nb, ldx = Xa.shape[0], Xb.shape[0], Xa.shape[1]
    kk = ldx - 16 if defect == "last16" and (ldx // 16) % 2 == 1 else ldx
    an, bn = np.array(an[:na], dtype=np.float64), np.array(bn[:nb], dtype=np.float64)
    if defect == "ragged_norm":
        if na % 16 and na > 1:
            an[-1] = an[-2]
        if nb % 16 and nb > 1:
            bn[-1] = bn[-2]
    out = var * np.exp((an[:, None] + bn[None, :] - 2.0 * (Xa[:, :kk] @ Xb[:, :kk].T)) / (-2.0 * ls * ls))
    mm = m // 4 * 4 if defect == "mquad" else m
    if mm:
        A, B = np.asarray(Va)[:mm, :na], np.asarray(Vb)[:mm, :nb]
        if defect == "swap":
            A, B = np.asarray(Vb)[:mm][:, np.arange(na) % nb], np.asarray(Va)[:mm][:, np.arange(nb) % na]
        out = out + A.T @ B if defect == "sign" else out - A.T @ B
    return out


def emu_rowsum(prior, accumulate, Xa, an, Xb, bn, Va, Vb, m, var, ls, nsplit, defect=None):
    """Partial sums per column split (tile jt of 64 columns belongs to split jt % nsplit), added in ascending order onto the
    prior.  defect: those of emu_cov_block, or noabs, skip_tile (the last column tile skipped when ntile % nsplit != 0),
    no_accumulate."""
    na, nb = Xa.shape[0], Xb.shape[0]
    out = np.array(prior, dtype=np.float64) if accumulate and defect != "no_accumulate" else np.zeros(na)
    if nb == 0:
        return out if accumulate else np.zeros(na)
    blk = emu_cov_block(Xa, an, Xb, bn, Va, Vb, m, var, ls, defect if defect in COV_DEFECTS else None)
    if defect != "noabs":
        blk = np.abs(blk)
    ntile = _cdiv(nb, 64)
    if defect == "skip_tile" and ntile % nsplit:
        ntile -= 1
    for s in range(nsplit):
        part = np.zeros(na)
        for jt in range(s, ntile, nsplit):
            part += blk[:, 64 * jt:64 * jt + 64].sum(axis=1)
        out = out + part
    return out


@functools.lru_cache(maxsize=None)
def cov_inputs(na, nb, ldx, m, seed=0, spread=1.0):
    """Rows with d < ldx live features (the last 16-feature step holds live features and zero padding), FP64 norms, and
    whitened blocks with entries of both signs large enough that a good share of K - Va^T Vb is negative."""
    d = ldx - 5
    rng = np.random.default_rng(7919 * na + 104729 * nb + 31 * ldx + m + seed)
    s = types.SimpleNamespace(na=na, nb=nb, ldx=ldx, m=m, d=d, var=1.3, ls=0.8 * float(np.sqrt(d / 12.0)))
    s.Xa, s.Xb = padded(spread * rng.random((na, d)), ldx), padded(spread * rng.random((nb, d)), ldx)
    s.an, s.bn = (s.Xa * s.Xa).sum(axis=1), (s.Xb * s.Xb).sum(axis=1)
    s.Va, s.Vb = 0.8 * rng.standard_normal((m, na)), 0.8 * rng.standard_normal((m, nb))
    if na == nb == 1 and m:
        s.Va[0, 0] = s.Vb[0, 0] = 1.5          # the one entry of a 1 x 1 block is negative: var - 2.25 at the most
    return _frozen(s)


# ------------------------------------------------------------------------------------------------ conditional entropy
def patterns(t):
    """[2^t][t] labels in itertools.product order (variable 0 slowest, -1 before +1)."""
    return np.array(list(itertools.product((-1.0, 1.0), repeat=t))).reshape(1 << t, t)


def _members(inp):
    return [int(p) for p in np.asarray(inp.bgpos)[:inp.t - 1]]


def _keep(inp):
    keep = np.ones(inp.n_all, dtype=bool)
    keep[_members(inp)] = False
    return keep


class _Ext:
    cv, zeros, sqrt, exp, log, phi = staticmethod(xp), staticmethod(xzeros), staticmethod(xsqrt), staticmethod(xexp), \
        staticmethod(xlog), staticmethod(phi_pair)


class _F64:
    """The same formulas in FP64: two digits of the bound for candidates outside the extended subset."""
    cv, zeros, sqrt, exp, log = staticmethod(lambda a: np.asarray(a, dtype=np.float64)), staticmethod(np.zeros), \
        staticmethod(np.sqrt), staticmethod(np.exp), staticmethod(np.log)

    @staticmethod
    def phi(z):
        from scipy.special import ndtr
        return ndtr(z), ndtr(-z)


def _ce_core(inp, li, X, want_sp=False):
    """Per pattern r of candidate li: (sum_j h_jr, its bound dce_r, whether NaN is due), in the arithmetic X.  want_sp: s'
    over the whole block instead."""
    t, n = inp.t, inp.n_all
    gi = inp.pos_offset + li
    cv = X.cv
    S = X.zeros((t, t))
    if t > 1:
        S[:t - 1, :t - 1] = cv(np.asarray(inp.sig)[:t - 1, :t - 1])
        S[:t - 1, t - 1] = S[t - 1, :t - 1] = cv(np.asarray(inp.C)[:t - 1, gi])
    S[t - 1, t - 1] = cv(inp.s2[gi])
    eye = cv(np.eye(t))
    G = S + cv(inp.noise) * eye
    if X is _Ext:
        L = chol_x(G)
        Xi = solve_lower_x(L, eye)
    else:
        L = np.linalg.cholesky(G)
        Xi = np.linalg.inv(L)
    W = Xi.T @ Xi
    c = cv(np.vstack((np.asarray(inp.C)[:t - 1, :n].reshape(t - 1, n), np.asarray(inp.cov)[li, :n][None, :])))
    ms = cv(np.concatenate((np.asarray(inp.bmu)[:t - 1], [inp.mu[gi]])))
    mu, s2 = cv(np.asarray(inp.mu)[:n]), cv(np.asarray(inp.s2)[:n])
    U = W @ c
    sp = s2 - (c * U).sum(axis=0)
    if want_sp:
        return sp
    keep = _keep(inp)
    R = 1 << t
    if np.asarray(sp[keep] <= 0, dtype=bool).any():
        return None, None, True
    c, U, sp, mu = c[:, keep], U[:, keep], sp[keep], mu[keep]
    val = (mu - ms @ U)[None, :] + cv(patterns(t)) @ U
    # ---- the bound
    u = cv(2.0 ** -53)
    g = lambda k: cv(float(k)) * u / (1 - cv(float(k)) * u)
    aL, aX, aW, ac, aU, ams = np.abs(L), np.abs(Xi), np.abs(W), np.abs(c), np.abs(U), np.abs(ms)
    A = aX.T @ (aX @ aL @ aX)
    dW = g(t + 2) * (aW @ (aL @ aL.T) @ aW) + g(t) * (A + A.T) + g(t) * (aX.T @ aX)
    dU = dW @ ac + g(t) * (aW @ ac)
    ds = (ac * dU).sum(axis=0) + g(t) * (ac * aU).sum(axis=0) + u * np.abs(sp)
    B = np.abs(mu) + ams @ aU
    dval = ams @ dU + g(t + 1) * B + dU.sum(axis=0) + g(2 * t) * (B + aU.sum(axis=0))
    sd = X.sqrt(sp)
    z = -val / sd[None, :]
    dz = (dval / sd)[None, :] + np.abs(z) * (ds / (2 * sp) + 4 * u)[None, :]
    q, p = X.phi(z)
    eps = cv(inp.eps)
    lq, lp = X.log(q + eps), X.log(p + eps)
    h = q * lq + p * lp
    D = np.abs(lq - lp + q / (q + eps) - p / (p + eps))
    pdf = X.exp(-z * z / 2) / X.sqrt(cv(2 * math.pi))
    dh = pdf * D * dz + D * (cv(PHI_ABS) + u) + 4 * u * (np.abs(q * lq) + np.abs(p * lp)) + 2 * u
    depth = _cdiv(n, 256) + 8
    assert h.shape == (R, int(keep.sum()))
    return h.sum(axis=1), dh.sum(axis=1) + g(depth) * np.abs(h).sum(axis=1), False


def _first_min(vals):
    """Index of the minimum under `cur < best` in order: the first of equal values."""
    best = 0
    for r in range(1, len(vals)):
        if vals[r] < vals[best]:
            best = r
    return best


def ce_ref(inp, only=None, arith=_Ext):
    """{li: (value, bound, index of the minimising pattern)} of the scored live candidates (all of them, or those in `only`);
    the value is None where NaN is due (the reference's first pattern is NaN and `cur < best` keeps it)."""
    out = {}
    for li in (range(inp.n_i) if only is None else only):
        if not inp.alive[li]:
            continue
        vals, bounds, nan = _ce_core(inp, li, arith)
        if nan:
            out[li] = (None, None, 0)
        else:
            r = _first_min(vals)
            out[li] = (vals[r], max(bounds), r)
    return out


def ce_check(ce, inp, only=None, ref=None):
    """Largest |ce - ref| / bound over the candidates of `only` (all live ones by default); inf for a NaN mismatch or a dead
    candidate that lost its canary (every dead candidate is looked at whatever `only` says)."""
    ce = np.asarray(ce, dtype=np.float64)
    dead = np.asarray(inp.alive)[:inp.n_i] == 0
    if not np.array_equal(ce[:inp.n_i][dead].view(np.int64), np.full(int(dead.sum()), CANARY).view(np.int64)):
        return float("inf")
    ref = ce_ref(inp, only) if ref is None else ref
    worst = 0.0
    for li, (val, bound, _) in ref.items():
        if val is None:
            if not np.isnan(ce[li]):
                return float("inf")
        elif not np.isfinite(ce[li]):
            return float("inf")
        else:
            worst = max(worst, _ratio(xp(ce[li]) - val, bound))
    return worst


def ce_check_against_emulation(ce, emu, inp, skip=()):
    """The candidates outside the extended subset: device and emulation each lie within the bound of the reference, so within
    twice the bound of each other (the bound evaluated in FP64 -- two digits of it are enough)."""
    worst = 0.0
    for li, (val, bound, _) in ce_ref(inp, [i for i in range(inp.n_i) if inp.alive[i] and i not in skip], _F64).items():
        if val is None or not np.isfinite(emu[li]):
            if not (np.isnan(ce[li]) and np.isnan(emu[li])):
                return float("inf")
        elif not np.isfinite(ce[li]):
            return float("inf")
        else:
            worst = max(worst, abs(ce[li] - emu[li]) / (2 * float(bound)))
    return worst


CE_DEFECTS = ("no_noise", "member_kept", "li_for_gi", "last_stride", "wave_dropped", "group_dropped", "nanmin", "dead_scored")


def emu_ce(inp, defect=None):
    """Plain FP64 from the formulas: W by the Cholesky route, Phi by scipy's ndtr, NumPy's log and sum.  Returns ce[n_i] with
    the canary at dead candidates.
    defect: no_noise       noise left off the diagonal of Sigma_S
            member_kept    members not skipped in the sum over j
            li_for_gi      li where pos_offset + li belongs, in C, mu and s2
            last_stride    the last partial stride of 256 of the j loop dropped
            wave_dropped   the second wave's share (j % 256 in [64, 128)) dropped
            group_dropped  the group of 8 patterns that holds the minimum left out of it (t >= 5)
            nanmin         a j with s' <= 0 ignored instead of making the sum NaN
            dead_scored    dead candidates scored like live ones"""
    from scipy.special import ndtr
    t, n = inp.t, inp.n_all
    ce = np.full(inp.n_i, CANARY)
    Y = patterns(t)
    keep = np.ones(n, dtype=bool) if defect == "member_kept" else _keep(inp)
    if defect == "last_stride" and n % 256:
        keep[n // 256 * 256:] = False
    if defect == "wave_dropped":
        keep[(np.arange(n) % 256) // 64 == 1] = False
    C, mu, s2 = np.asarray(inp.C)[:t - 1, :n].reshape(t - 1, n), np.asarray(inp.mu)[:n], np.asarray(inp.s2)[:n]
    for li in range(inp.n_i):
        if not inp.alive[li] and defect != "dead_scored":
            continue
        gi = li if defect == "li_for_gi" else inp.pos_offset + li
        S = np.empty((t, t))
        S[:t - 1, :t - 1] = np.asarray(inp.sig)[:t - 1, :t - 1]
        S[:t - 1, t - 1] = S[t - 1, :t - 1] = C[:, gi]
        S[t - 1, t - 1] = s2[gi]
        if defect != "no_noise":
            S = S + inp.noise * np.eye(t)
        Li = np.linalg.inv(np.linalg.cholesky(S))
        W = Li.T @ Li
        c = np.vstack((C, np.asarray(inp.cov)[li, :n][None, :]))
        U = W @ c
        sp = s2 - (c * U).sum(axis=0)
        ms = np.concatenate((np.asarray(inp.bmu)[:t - 1], [mu[gi]]))
        mean = mu[None, :] + (Y - ms[None, :]) @ U
        with np.errstate(invalid="ignore", divide="ignore"):
            q = ndtr(-mean / np.sqrt(np.where(sp > 0, sp, np.nan))[None, :])
            h = q * np.log(q + inp.eps) + (1 - q) * np.log(1 - q + inp.eps)
        vals = (np.nansum if defect == "nanmin" else np.sum)(h[:, keep], axis=1)
        if defect == "group_dropped" and t >= 5:
            r = _first_min(vals)
            vals = np.delete(vals, np.arange(r // 8 * 8, r // 8 * 8 + 8))
        ce[li] = vals[_first_min(vals)]
    return ce


# ------------------------------------------------------------------------------------------------ host-built state
M_LABELLED, BLOCK_D, BLOCK_LDX = 6, 11, 16


@functools.lru_cache(maxsize=None)
def block_state(n_all, noise):
    """n_all block points and M_LABELLED labelled points in the unit cube: posterior mean mu and covariance Sigma of the block
    given the labels, solved in the extended type from the reference kernel values and rounded to FP64."""
    rng = np.random.default_rng(1000 * n_all + int(round(-np.log10(noise))))
    s = types.SimpleNamespace(n_all=n_all, noise=noise, var=1.0, ls=0.8 * float(np.sqrt(BLOCK_D / 12.0)))
    s.X = padded(rng.random((n_all, BLOCK_D)), BLOCK_LDX)
    XT = padded(rng.random((M_LABELLED, BLOCK_D)), BLOCK_LDX)
    y = xp(np.where(rng.random(M_LABELLED) < 0.5, 1.0, -1.0))
    K_TT, _ = kernel_ref(XT, XT, s.var, s.ls)
    Lx = chol_x(K_TT + xp(noise) * xp(np.eye(M_LABELLED)))
    K_TX, _ = kernel_ref(XT, s.X, s.var, s.ls)
    V = solve_lower_x(Lx, K_TX)
    alpha = solve_lower_x(Lx, y[:, None])[:, 0]
    K_XX, _ = kernel_ref(s.X, s.X, s.var, s.ls)
    s.mu = rnd(V.T @ alpha)
    s.Sigma = rnd(K_XX - V.T @ V)
    s.Sigma = 0.5 * (s.Sigma + s.Sigma.T)
    return _frozen(s)


def member_positions(t, n_all):
    """t - 1 distinct block positions spread over the first, a middle and the last stride of the j loop (where the last stride
    holds a single entry, n_all = 257, the member stays in front of it: that entry is the one a dropped stride would lose)."""
    last = n_all - 2 if n_all % 256 == 1 and n_all > 1 else n_all - 1
    want = [last, 0, n_all // 2, 1, last - 1, n_all // 2 + 1, n_all // 3, 2, 3]
    out = []
    for p in want:
        if len(out) < t - 1 and 0 <= p < n_all and p not in out:
            out.append(p)
    assert len(out) == t - 1
    return out


def slices(t, n_all):
    """(n_i, pos_offset): the whole block, the last five (an odd offset where n_all is even), one in the middle."""
    out = [(n_all, 0)]
    if n_all > 5:
        out.append((5, n_all - 5))
    if n_all > 2:
        out.append((1, n_all // 2 + 2 if n_all // 2 + 2 < n_all else n_all // 2))
    return out


def ce_inputs(t, n_all, noise, n_i, pos_offset, eps=1e-12):
    """The arrays of ital_mcmi_desc from block_state: members dead where they lie in the slice, plus one dead non-member."""
    s = block_state(n_all, noise)
    mem = member_positions(t, n_all)
    inp = types.SimpleNamespace(t=t, n_i=n_i, pos_offset=pos_offset, n_all=n_all, noise=noise, eps=eps)
    inp.mu, inp.s2 = s.mu.copy(), np.diag(s.Sigma).copy()
    inp.cov = s.Sigma[pos_offset:pos_offset + n_i].copy()
    inp.C = s.Sigma[mem].reshape(t - 1, n_all).copy()
    inp.sig = s.Sigma[np.ix_(mem, mem)].reshape(t - 1, t - 1).copy()
    inp.bmu, inp.bgpos = s.mu[mem].copy(), np.array(mem, dtype=np.int64)
    inp.alive = np.ones(n_i, dtype=np.uint8)
    for p in mem:
        if pos_offset <= p < pos_offset + n_i:
            inp.alive[p - pos_offset] = 0
    live = [li for li in range(n_i) if inp.alive[li]]
    inp.dead_extra = None
    if len(live) > 1:
        inp.dead_extra = live[len(live) // 3]
        inp.alive[inp.dead_extra] = 0
    return inp


def subset(inp, count):
    """At most `count` live candidates spread over the slice: the ones the extended check looks at."""
    live = [li for li in range(inp.n_i) if inp.alive[li]]
    if len(live) <= count:
        return live
    return sorted({live[int(round(k * (len(live) - 1) / (count - 1)))] for k in range(count)})


def nan_inputs(t, n_all=65, noise=1e-6, delta=2e-6):
    """The NaN rule: block entry j* has s2 = delta, no covariance with the members, and covariance 0.5 with every second
    scored candidate -- s'_{j*} = delta - 0.25 W_tt there (W_tt >= 1 / (s2_i + noise) > 1), delta elsewhere."""
    inp = ce_inputs(t, n_all, noise, n_all, 0)
    mem = _members(inp)
    jstar = next(j for j in range(7, n_all) if j not in mem and inp.alive[j])
    inp.alive[jstar] = 0                       # j* is a block entry, not a scored candidate
    inp.s2[jstar] = delta
    inp.C[:, jstar] = 0.0
    inp.cov[:, jstar] = 0.0
    hit = [li for li in range(n_all) if inp.alive[li]][::2]
    inp.cov[hit, jstar] = 0.5
    inp.jstar, inp.hit = jstar, hit
    return inp


def sprime_at_jstar(inp):
    """s'_{j*} of nan_inputs in the extended type: (values at the candidates that were hit, values at the others)."""
    lo = [float(_ce_core(inp, li, _Ext, True)[inp.jstar]) for li in inp.hit]
    hi = [float(_ce_core(inp, li, _Ext, True)[inp.jstar]) for li in range(inp.n_i) if inp.alive[li] and li not in inp.hit]
    return lo, hi


# ------------------------------------------------------------------------------------------------ the shapes of the issue
LDX_OF_M = {0: 16, 1: 32, 3: 48, 4: 16, 5: 32, 17: 48}
SMALL_SHAPES = ((1, 1), (17, 33), (64, 32), (65, 33), (200, 150))
SMALL_CASES = [(na, nb, LDX_OF_M[m], m) for na, nb in SMALL_SHAPES for m in (0, 1, 3, 4, 5, 17)] + \
              [(65, 33, ldx, 5) for ldx in (16, 48)] + [(17, 33, 32, 4), (200, 150, 16, 17)]
DEFAULT_CASES = [(130, 16330, 32, 5), (390, 8130, 48, 3)]
LDS_CASES = [(1, 130945, 16, 5), (129, 65409, 48, 4)]
ROWSUM_SHAPES = ((1, 1, 16, 1), (129, 63, 32, 5), (257, 1000, 48, 3), (130, 4200, 16, 4))
ROWSUM_WORK = (1, 2, 7, 64)
CE_CASES = [(t, n, noise) for t in range(1, 5) for n in (t, 63, 64, 65, 255, 256, 257, 300) for noise in (1e-6, 0.1)] + \
           [(t, n, noise) for t in range(5, 9) for n in (t, 65, 257) for noise in (1e-6, 0.1)]


def ce_subset_size(t):
    return 6 if t <= 4 else 3


def pieces(na, nb, rows=128, cols=2048):
    """(i0, i1, j0, j1) sub-blocks of at most 128 x 2048 that tile an na x nb block (each one a small-route call)."""
    return [(i0, min(i0 + rows, na), j0, min(j0 + cols, nb)) for i0 in range(0, na, rows) for j0 in range(0, nb, cols)]


def checked_pieces(na, nb):
    """The pieces compared by bits and checked in the extended type.  Default route: every piece of the tiling.  LDS route:
    the four corners, the right-hand ones at an odd column offset (nb - 2046, nb odd in both cases), the lower ones at an odd
    row offset (na - 126 = 3 for na = 129; a single row has no lower corners)."""
    if expected_route(na, nb) == "default":
        return pieces(na, nb)
    out = []
    for i0, i1 in ((0, min(128, na)), (max(0, na - 126), na)):
        for j0, j1 in ((0, 2048), (nb - 2046, nb)):
            if (i0, i1, j0, j1) not in out:
                out.append((i0, i1, j0, j1))
    return out


@functools.lru_cache(maxsize=None)
def ce_ref_cached(t, n_all, noise, n_i, pos_offset):
    """ce_ref on the extended subset of one slice of a case (the same for every test that needs it)."""
    inp = ce_inputs(t, n_all, noise, n_i, pos_offset)
    return ce_ref(inp, subset(inp, ce_subset_size(t)))


def group_coverage(found=None):
    """Which of the first / a middle / the last group of 8 patterns hold the minimum, over the extended subsets of the t >= 5
    cases (or over `found`: (t, pattern index) pairs)."""
    if found is None:
        found = []
        for t, n, noise in CE_CASES:
            if t >= 5:
                for n_i, off in slices(t, n):
                    found += [(t, r) for _, _, r in ce_ref_cached(t, n, noise, n_i, off).values()]
    out = set()
    for t, r in found:
        last = (1 << t) // 8 - 1
        out.add("first" if r // 8 == 0 else "last" if r // 8 == last else "middle")
    return out
