"""Extended-precision host reference, checker and FP64 emulation of the dense tune kernels -- ital_gram_rows,
ital_chol_batched, ital_chol_solve_batched, ital_kernel_matvec (include/ital_dense.h, ital_amd/csrc/dense.hip) -- shared by
tests/test_dense_ref_host.py and tests/test_gpu_dense_kernels.py.  Plain NumPy, no GPU, no project import.  Not a test module.

The extended type, kernel_ref with its bound dK and the row generators are those of tests/_gp_update_ref.py (the checks
here are residuals, so its chol_x and solve_lower_x are not needed).  Inputs are always the FP64 values the device received; the reference and every residual and bound
are formed in the extended type.  Each check returns its largest residual / bound ratio (inf for a non-finite output): a
result passes with ratio <= 1.

The bounds are a-priori (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 10.3 for the factor, Thm 8.5 for
the substitutions, Lemma 8.4 for one entry's chain of operations), u = 2^-53, gamma(k) = k u / (1 - k u).  The constants are
operation counts of the kernels as written in dense.hip; nothing is fitted to an output.

  Gram     |K_ij - Kref_ij| <= dK_ij  (j < i),   |K_ii - Kref_ii - noise| <= dK_ii + u |K_ii|
           Kref, dK: kernel_ref on the rows X[idx].  dK_ij = Kref_ij (dA_ij + 4u) with dA the error of the exponent's
           argument when norms and dot product are sums of ldx terms in any order: it covers the norm kernel's order, the
           MFMA's order, the distance that is not clamped at 0 (so the device diagonal is var exp(tiny) + noise, not
           var + noise) and an exp of <= 1 ulp.  u |K_ii|: the addition of the noise.

  factor   |A_ij - sum_r L_ir L_jr| <= gamma(c_n) (|L||L|^T)_ij,  j <= i,   c_n = n + ceil(n / 64) + 2
           Entry (i, j) with j = 64 B + jj is formed by this chain.  B trailing updates (chol_syrk_kernel), one per earlier
           block column: a 64-term MFMA sum from a zero accumulator (its terms see at most 64 roundings: the product, unless
           fused, and 63 additions) and ONE subtraction of that sum from the entry: 65 per step, 65 B in all.  Inside its own
           block (chol_diag_kernel for i in the block, chol_trsm_kernel below it) jj multiply-subtract steps, a term seeing its
           product and the subtractions after it, <= jj + 1; then the division by L_jj -- or, for i = j, the square root, whose
           one rounding enters L_jj^2 twice: jj + 3.  By Lemma 8.4 every term of the sum (and A_ij itself) carries at most the
           roundings of the whole chain:  65 B + jj + 3 = j + B + 3 <= (n - 1) + ceil(n / 64) + 3 = c_n.
           (The largest number a single term really sees is 64 + B + jj + 2; c_n is the plain sum the theorem's form uses.)
           A leading factor (columns < k of a matrix whose factoring stopped in the block at k) obeys the same bound on those
           columns, all rows.

  solve    |y - L L^T x| <= (2 gamma(c_n) + gamma(c_n)^2) (|L| (|L|^T |x|)),  componentwise
           chol_solve_kernel: row i of the forward sweep is i multiply-subtracts (in blocks of 64, but one running value per
           unknown, so a plain chain) and a division, i + 1 <= c_n roundings per term (Thm 8.5): (L + D1) z = y, |D1| <=
           gamma |L|; the backward sweep likewise (L + D2)^T x = z.  Composed: y = (L + D1)(L + D2)^T x, and the residual
           y - L L^T x = (D1 L^T + L D2^T + D1 D2^T) x.  L is the device's own factor: the solve is judged apart from it.

  K W      |out_if - sum_j Kref_ij W_jf| <= gamma(nb + nsplit + 3) sum_j |Kref_ij||W_jf| + sum_j dK_ij |W_jf| + u |out_if|
           kernel_w_kernel: each of the four waves adds its share of a chunk's products into one MFMA accumulator, one term
           after the other over the tiles of the chunk (<= nb terms; the product is one more rounding unless fused), the two
           waves that share a row are added once, kernel_w_reduce adds the nsplit partial sums in ascending order:
           nb + nsplit + 2, one to spare.  u |out_if|: the final rounding.  nsplit: expected_split, a host copy of kw_split.

emu_*: plain FP64 NumPy emulations of the four entry points (the Cholesky blocked as the kernels are).  They show that the
bounds admit a correct FP64 implementation; with `defect` they make, one at a time, mistakes these kernels could make, which
the checks must reject (tests/test_dense_ref_host.py)."""
import functools
import types

import numpy as np

import _gp_update_ref as g
from _gp_update_ref import D_OF, draw_rows, gamma, kernel_ref, padded, row_norms64, unit, xp

NB = 64                      # Cholesky block (dense.hip NB)
T = 128                      # MFMA tile edge (mfma_tile.h T)
KW_TARGET_BLOCKS = 1024      # dense.hip KW_TARGET_BLOCKS
NAN = float("nan")


def _cdiv(a, b):
    return (a + b - 1) // b


def expected_split(na, nb):
    """(nsplit, tiles per chunk) of ital_kernel_matvec: keep in step with kw_split of dense.hip."""
    gx, tiles_b = _cdiv(na, T), _cdiv(nb, T)
    want = min(max(_cdiv(KW_TARGET_BLOCKS, gx), 1), tiles_b)
    per = _cdiv(tiles_b, want)
    return _cdiv(nb, per * T), per


def expected_workspace(na, nb):
    nsplit = expected_split(na, nb)[0]
    return nsplit * na * 16 if nsplit > 1 else 0


def c_n(n):
    return n + _cdiv(n, NB) + 2


def mv_count(nb, nsplit):
    return nb + nsplit + 3


# ------------------------------------------------------------------------------------------------ the checks
def check_gram(K, Kref, dK, noise):
    """The lower triangle of the n x n device Gram K against kernel_ref's values of the rows X[idx]."""
    n = Kref.shape[0]
    lo = np.tril_indices(n)
    Kf = np.asarray(K, dtype=np.float64)[:n, :n]
    if not g._finite(Kf[lo]):
        return float("inf")
    Kx = xp(Kf)
    eye = xp(np.eye(n))
    resid = Kx - Kref - xp(noise) * eye
    bound = dK + unit() * np.abs(Kx) * eye
    return g._ratio(resid[lo], bound[lo])


def check_factor(L, A, n, ncols=None):
    """|A_ij - (L L^T)_ij| <= gamma(c_n) (|L||L|^T)_ij on j <= i, j < ncols (default n: the whole lower triangle).  A: the
    FP64 matrix the device was given (its lower triangle is read)."""
    ncols = n if ncols is None else ncols
    if ncols == 0:
        return 0.0
    Lf = np.tril(np.asarray(L, dtype=np.float64)[:n, :n])[:, :ncols]
    if not g._finite(Lf):
        return float("inf")
    Lx = xp(Lf)
    Ax = xp(np.tril(np.asarray(A, dtype=np.float64)[:n, :n])[:, :ncols])
    La = np.abs(Lx)
    P, Pa = Lx @ Lx[:ncols].T, La @ La[:ncols].T          # [i][j] = sum_{r < ncols} L_ir L_jr; L_jr = 0 for r > j
    keep = np.tril(np.ones((n, n), dtype=bool))[:, :ncols]
    return g._ratio((Ax - P)[keep], (gamma(c_n(n)) * Pa)[keep])


def factor_bound(L, n, i, j):
    """The bound of check_factor at entry (i, j), in FP64."""
    La = np.abs(np.tril(np.asarray(L, dtype=np.float64)[:n, :n]))
    return float(gamma(c_n(n))) * float(La[i] @ La[j])


def check_solve(L, x, y, n):
    """|y - L L^T x| <= (2 gamma + gamma^2) |L| (|L|^T |x|) with gamma = gamma(c_n)."""
    if n == 0:
        return 0.0
    Lf, xf = np.tril(np.asarray(L, dtype=np.float64)[:n, :n]), np.asarray(x, dtype=np.float64)[:n]
    if not g._finite(Lf, xf):
        return float("inf")
    Lx, xx, yx = xp(Lf), xp(xf), xp(np.asarray(y, dtype=np.float64)[:n])
    La = np.abs(Lx)
    gm = gamma(c_n(n))
    return g._ratio(yx - Lx @ (Lx.T @ xx), (2 * gm + gm * gm) * (La @ (La.T @ np.abs(xx))))


def check_matvec(out, Kref, dK, W, nb, nsplit):
    """out[rows][:F] against Kref[rows] W for the rows Kref and dK were made for."""
    of, Wf = np.asarray(out, dtype=np.float64), np.asarray(W, dtype=np.float64)
    if not g._finite(of):
        return float("inf")
    ox, Wx = xp(of), xp(Wf)
    Wa = np.abs(Wx)
    bound = gamma(mv_count(nb, nsplit)) * (np.abs(Kref) @ Wa) + dK @ Wa + unit() * np.abs(ox)
    return g._ratio(Kref @ Wx - ox, bound)


def matvec_bound64(Xa, Xb, W, var, ls, nsplit):
    """The bound of check_matvec for every row, evaluated in FP64 chunk by chunk (two digits of a bound are enough); without
    the u |out| term."""
    na, nb = Xa.shape[0], Xb.shape[0]
    ldx = Xa.shape[1]
    u = 2.0 ** -53
    an, bn = row_norms64(Xa), row_norms64(Xb)
    Wa = np.abs(W)
    gm, gk = float(gamma(mv_count(nb, nsplit))), float(gamma(ldx + 4))
    bound = np.zeros((na, W.shape[1]))
    for j0 in range(0, nb, 512):
        B = Xb[j0:j0 + 512]
        K = var * np.exp((an[:, None] + bn[None, j0:j0 + 512] - 2.0 * (Xa @ B.T)) / (-2.0 * ls * ls))
        dA = gk * (an[:, None] + bn[None, j0:j0 + 512] + 2.0 * (np.abs(Xa) @ np.abs(B).T)) / (2.0 * ls * ls)
        bound += (K * (gm + dA + 4 * u)) @ Wa[j0:j0 + 512]
    return bound


def check_matvec_against_emulation(out, emu, bound64):
    """Rows outside the extended subset: device and emulation each lie within the bound of the reference, so within twice
    the bound of each other."""
    out, emu = np.asarray(out, dtype=np.float64), np.asarray(emu, dtype=np.float64)
    if not g._finite(out, emu):
        return float("inf")
    return g._ratio(out - emu, 2.0 * (bound64 + 2.0 ** -53 * np.abs(out)))


# ------------------------------------------------------------------------------------------------ FP64 emulation
GRAM_DEFECTS = ("noise_tile_local", "idx_ignored", "clamped_norm")
CHOL_DEFECTS = ("syrk_k48", "partial_full", "max_n", "perturb")
SOLVE_DEFECTS = ("backward_forward", "tail_skipped")
MATVEC_DEFECTS = ("first_tile_only", "chunk_overrun", "clamped_weight")
PERTURB = 3.0                 # the `perturb` defect moves one entry of L by this multiple of its bound


def emu_gram(X, xn, idx, n, var, ls, noise, defect=None):
    """The n x n Gram of the rows X[idx[:n]] (the kernel writes its lower triangle).
    defect: noise_tile_local  i == j tested on the indices inside a wave's 64 x 64 quarter: noise on (i - j) % 64 == 0
            idx_ignored       rows 0 .. n - 1 taken instead of idx
            clamped_norm      the norm on the row side clamped one row too early: row n - 1 gets the norm of row n - 2"""
    rows = np.arange(n) if defect == "idx_ignored" else np.asarray(idx)[:n]
    R, nc = X[rows], xn[rows]
    nr = nc.copy()
    if defect == "clamped_norm" and n >= 2:
        nr[n - 1] = nr[n - 2]
    K = var * np.exp((nr[:, None] + nc[None, :] - 2.0 * (R @ R.T)) / (-2.0 * ls * ls))
    i, j = np.indices((n, n))
    K[(i - j) % NB == 0 if defect == "noise_tile_local" else i == j] += noise
    return K


def emu_chol(buf, n, max_n=None, defect=None):
    """ital_chol_batched on one matrix held in the 2-D buffer `buf` (at least n rows and columns; what lies past n and above
    the diagonal is never read by a correct factor).  Blocked as the kernels are: a 64 x 64 diagonal block factored
    right-looking, the panel below it by forward substitution, one trailing update per block column.  Returns (a copy of
    buf with the factor in its lower triangle, info); a failing pivot leaves its diagonal block as it was.
    defect: syrk_k48      the last 16-wide stage of the trailing update's 64-wide k dropped
            partial_full  a partial diagonal block treated as a full one (the emulation stays inside its buffer)
            max_n         max_n used where n belongs
            perturb       L[n - 1][n // 2] moved by PERTURB times its bound of check_factor (divided by L[n // 2][n // 2])"""
    A, info = np.array(buf, dtype=np.float64), 0
    nn = min(max_n, A.shape[0], A.shape[1]) if defect == "max_n" and max_n else n
    with np.errstate(invalid="ignore", divide="ignore"):
        for k0 in range(0, nn, NB):
            m = min(NB, nn - k0)
            if defect == "partial_full":
                m = min(NB, A.shape[0] - k0, A.shape[1] - k0)
            S = A[k0:k0 + m, k0:k0 + m].copy()
            for j in range(m):
                if not S[j, j] > 0:
                    info = k0 + j + 1
                    break
                S[j, j] = np.sqrt(S[j, j])
                S[j + 1:, j] /= S[j, j]
                S[j + 1:, j + 1:] -= np.outer(S[j + 1:, j], S[j + 1:, j])
            if info:
                break
            lo = np.tril(np.ones((m, m), dtype=bool))
            A[k0:k0 + m, k0:k0 + m][lo] = S[lo]
            k1 = k0 + NB
            if k1 < nn:
                P = A[k1:nn, k0:k1]
                for c in range(NB):
                    P[:, c] = (P[:, c] - P[:, :c] @ S[c, :c]) / S[c, c]
                kk = NB - 16 if defect == "syrk_k48" else NB
                U = P[:, :kk] @ P[:, :kk].T
                lo = np.tril(np.ones((nn - k1, nn - k1), dtype=bool))
                A[k1:nn, k1:nn][lo] -= U[lo]
    if defect == "perturb" and not info:
        i, j = n - 1, n // 2 if n > 1 else 0
        A[i, j] += PERTURB * factor_bound(A, n, i, j) / abs(A[j, j])
    return A, info


def emu_solve(L, n, y, defect=None):
    """y <- L^-T L^-1 y in blocks of 64 unknowns, as chol_solve_kernel sweeps.
    defect: backward_forward  the backward sweep visits its blocks in forward order
            tail_skipped      the unknowns below the last full block are skipped by both sweeps"""
    x = np.array(y, dtype=np.float64)[:n].copy()
    top = n // NB * NB if defect == "tail_skipped" else n
    blocks = list(range(0, top, NB))
    for kb in blocks:
        m = min(NB, top - kb)
        for c in range(m):
            x[kb + c] = (x[kb + c] - L[kb + c, kb:kb + c] @ x[kb:kb + c]) / L[kb + c, kb + c]
        x[kb + m:top] -= L[kb + m:top, kb:kb + m] @ x[kb:kb + m]
    for kb in (blocks if defect == "backward_forward" else blocks[::-1]):
        m = min(NB, top - kb)
        for r in range(m - 1, -1, -1):
            x[kb + r] = (x[kb + r] - L[kb + r + 1:kb + m, kb + r] @ x[kb + r + 1:kb + m]) / L[kb + r, kb + r]
        x[:kb] -= L[kb:kb + m, :kb].T @ x[kb:kb + m]
    return x


def emu_matvec(Xa, an, Xb, bn, W, var, ls, defect=None):
    """out[na][F] = K(a, b) W: the sum over b split into expected_split's chunks, a chunk walked in tiles of 128 rows of b, the
    partial sums of the splits added in ascending order.  The kernel matrix is formed one tile at a time.
    defect: first_tile_only  only the first tile of a chunk accumulated
            chunk_overrun    the rows of W past the chunk's end not zeroed: the next chunk's first tile counted twice
            clamped_weight   the rows past nb of the last tile (clamped to row nb - 1) given that row's weight"""
    na, nb = Xa.shape[0], Xb.shape[0]
    nsplit, per = expected_split(na, nb)
    out = np.zeros((na, W.shape[1]))
    for s in range(nsplit):
        jbeg = s * per * T
        jend = min(nb, jbeg + per * T)
        tiles = list(range(jbeg, jend, T))
        if defect == "first_tile_only":
            tiles = tiles[:1]
        if defect == "chunk_overrun" and jend < nb:
            tiles.append(jend)
        part = np.zeros_like(out)
        for j0 in tiles:
            rows = np.arange(j0, min(j0 + T, nb))
            if defect == "clamped_weight":
                rows = np.minimum(np.arange(j0, j0 + T), nb - 1)
            K = var * np.exp((an[:, None] + bn[None, rows] - 2.0 * (Xa @ Xb[rows].T)) / (-2.0 * ls * ls))
            part += K @ W[rows]
        out = out + part
    return out


def emu_factor_solve(A, ys):
    """The ratios of the emulated factor of A (its lower triangle, in a NaN-guarded buffer) and of the emulated solves with the
    right-hand sides ys = (labels, six decades) on that factor."""
    n = A.shape[0]
    L, info = emu_chol(guarded(lower_nan(A), n + 3), n)
    out = dict(factor=float("inf") if info else check_factor(L, A, n))
    for name, y in zip(("solve", "solve6"), ys):
        out[name] = check_solve(L, emu_solve(L, n, y), y, n)
    return out


def emu_chain(s, Kref, dK):
    """The ratios of the emulated chain Gram -> factor -> solves of gram_case `s`, each step on the output of the one before."""
    K = emu_gram(s.X, row_norms64(s.X), s.idx, s.n, s.var, s.ls, s.noise)
    out = dict(gram=check_gram(K, Kref, dK, s.noise))
    out.update(emu_factor_solve(K, (s.y, s.y_wide)))
    return out


# ------------------------------------------------------------------------------------------------ inputs and shapes
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 321)
EXTRA_ROWS = 7                # the row set is this much larger than the Gram taken from it
#: (kind, ldx, length scale): d = 5 with a near-flat and a peaked kernel, d = 40 near-flat
GRAM_PARAMS = (("uniform", 16, 1.2), ("uniform", 16, 0.5), ("uniform", 48, 1.2),
               ("neardup", 16, 1.2), ("neardup", 16, 0.5), ("neardup", 48, 1.2))
GRAM_CASES = [p + (n,) for p in GRAM_PARAMS for n in SIZES]
BATCH_SIZES = (65, 0, 129, 1, 64, 193)          # one mixed batch; max_n is larger than all of them
BATCH_MAX_N = 200


@functools.lru_cache(maxsize=None)
def gram_case(kind, ldx, ls, n):
    """n + EXTRA_ROWS padded rows X, a permutation idx of all of them (the Gram takes its first n), var, ls, noise."""
    d = D_OF[ldx]
    rng = np.random.default_rng(7919 * n + 31 * ldx + int(10 * ls) + (3 if kind == "neardup" else 0))
    s = types.SimpleNamespace(kind=kind, ldx=ldx, ls=float(ls), n=n, d=d, var=1.3)
    s.noise = 1e-6 if kind == "neardup" else 1e-3
    s.X = padded(draw_rows(kind, n + EXTRA_ROWS, d, rng), ldx)
    s.idx = rng.permutation(n + EXTRA_ROWS).astype(np.int64)
    assert n < 2 or not np.array_equal(s.idx[:n], np.arange(n))
    s.y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    s.y_wide = s.y * 10.0 ** rng.uniform(-3.0, 3.0, n)
    return s


@functools.lru_cache(maxsize=None)
def gram_ref(kind, ldx, ls, n):
    s = gram_case(kind, ldx, ls, n)
    R = s.X[s.idx[:n]]
    return kernel_ref(R, R, s.var, s.ls)


def host_spd(n, seed=0):
    """A host-built SPD matrix that is not a Gram: B diag(s) B^T / n with s spread over five decades, its rows and columns
    scaled over three more (a componentwise backward error does not see the scaling, a normwise one would)."""
    rng = np.random.default_rng(104729 * n + seed)
    B = rng.standard_normal((n, n))
    A = (B * np.logspace(0.0, -5.0, n)) @ B.T / n + 1e-5 * np.eye(n)
    sc = 10.0 ** rng.uniform(-1.5, 1.5, n)
    A = A * sc[:, None] * sc[None, :]
    return (A + A.T) / 2.0


def rhs(n, seed=0):
    """The two right-hand sides of the solve tests: +-1 labels, and entries spread over six decades."""
    rng = np.random.default_rng(15485863 * (n + 1) + seed)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    return y, y * 10.0 ** rng.uniform(-3.0, 3.0, n)


def lower_nan(A):
    """The lower triangle of a square matrix; NaN above the diagonal."""
    return np.where(np.tri(A.shape[0], dtype=bool), A, NAN)


def guarded(A, ld, extra_rows=2):
    """An n x n matrix in a buffer of n + extra_rows rows and ld columns; NaN wherever the matrix is not."""
    n = A.shape[0]
    out = np.full((n + extra_rows, ld), NAN)
    out[:n, :n] = A
    return out


MATVEC_F = (1, 5, 16)
MATVEC_SMALL = ((1, 1, 16), (5, 9, 16), (130, 129, 16), (129, 300, 16), (300, 77, 16), (300, 77, 48))
MATVEC_SMALL_SPLITS = {(1, 1): (1, 1), (5, 9): (1, 1), (130, 129): (2, 1), (129, 300): (3, 1), (300, 77): (1, 1)}
MATVEC_SMALL_CASES = [shape + (F,) for shape in MATVEC_SMALL for F in MATVEC_F]
#: the production loop: more than one tile per chunk.  (na, nb, ldx, F, nsplit, tiles per chunk, tiles of the last split)
MATVEC_LOOP = ((4000, 4224, 16, 16, 17, 2, 1), (4001, 8250, 16, 5, 22, 3, 2))


@functools.lru_cache(maxsize=None)
def matvec_case(na, nb, ldx, F):
    """Rows a and b in the unit cube and W[nb][F] of mixed signs with about a third of its rows zero (the fold layout: a
    sample outside a fold's training set has weight 0 there); the last row is not zero."""
    d = D_OF[ldx]
    rng = np.random.default_rng(1000003 * na + 101 * nb + 7 * ldx + F)
    s = types.SimpleNamespace(na=na, nb=nb, ldx=ldx, F=F, d=d, var=1.3, ls=0.5 * float(np.sqrt(d / 5.0)))
    s.Xa, s.Xb = padded(rng.random((na, d)), ldx), padded(rng.random((nb, d)), ldx)
    s.W = rng.standard_normal((nb, F)) * (rng.random(nb) < 0.67)[:, None]
    s.W[nb - 1] = rng.standard_normal(F)
    s.nsplit, s.per = expected_split(na, nb)
    return s


def loop_rows(na, nb):
    """The rows of a large shape judged against the extended reference: the first and last, those at the 127 / 128 tile edge
    and the first of the last row tile."""
    return sorted(set(r for r in (0, 127, 128, (na - 1) // T * T - 1, (na - 1) // T * T, na - 1) if 0 <= r < na))
