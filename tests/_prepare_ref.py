"""An np.longdouble model of the four definitions of include/ital_prepare.h, with a-priori componentwise bounds, and the
checkers the host and the GPU tests share.

BOUNDS.  u = 2^-53.  A sum of t FP64 terms formed in ANY order by FP64 additions differs from the exact sum by at most
gamma_(t-1) sum|term| <= (t - 1) u sum|term| (1 + O(t u)) (Higham, Accuracy and Stability, (4.4)); a dot product of t products
whose products are rounded (or fused: fewer roundings) by gamma_t sum|a||b| ((3.5)).  The model itself is a longdouble
(64-bit fraction) pairwise sum: its own error is below t 2^-64 sum|term|.  The small constant absorbs that, the second-order
terms for the sizes used here (t u < 2^-30) and, for C and the projection, the ONE FP64 rounding of each centred operand
(x - m is formed in FP64 on the device, in longdouble here: each factor carries (1 + delta), |delta| <= u):

    column sum            |got - model| <= (n + 4) u sum_i |x_ij|
    C[a][b]               |got - model| <= (n + 8) u sum_i |x_ia - m_a| |x_ib - m_b|
    Y[i][c]               |got - model| <= (d + 8) u sum_j |x_ij - s_j| |W_jc|
    a narrowed Y          on top, half a unit in the last place of the target type at |model| + the bound above (ONE rounding
                          to nearest of a value within the bound of the model).

None of this depends on the order of summation, so the range rule of the header does not enter the model.  min, max and the
scaling are exact: they are compared in bits.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53

#: element type code -> (name, fraction bits, least normal exponent, largest finite + half a unit); None for f64
TYPES = {0: ("f64", 52, -1022, None), 1: ("f32", 23, -126, float(LD(2) ** 128 - LD(2) ** 103)),
         2: ("f16", 10, -14, 65520.0), 3: ("bf16", 7, -126, float(LD(2) ** 128 - LD(2) ** 119))}


# ---------------------------------------------------------------------------------------------------- narrowing
def round_to(v, code):
    """float64 array v rounded ONCE to nearest, ties to even, onto the numbers of the element type `code` (as float64):
    beyond the largest finite number plus half a unit -> infinity, subnormals kept, NaN kept."""
    v = np.asarray(v, dtype=np.float64)
    if code == 0:
        return v.copy()
    _, mbits, emin, over = TYPES[code]
    a = np.abs(v)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e = np.frexp(np.where(np.isfinite(a) & (a > 0), a, 1.0))[1] - 1          # a = f 2^(e+1), f in [0.5, 1)
        q = np.maximum(e, emin) - mbits
        r = np.ldexp(np.rint(np.ldexp(a, -q)), q)                                 # rint: to nearest, ties to even
        r = np.where(a >= over, np.inf, r)
        r = np.where(np.isfinite(a), r, a)
    return np.copysign(r, v)


def trunc_to(v, code):
    """As round_to but rounding toward zero: the WRONG rounding mode, for the checker's own test."""
    _, mbits, emin, _ = TYPES[code]
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.frexp(np.where(a > 0, a, 1.0))[1] - 1
    q = np.maximum(e, emin) - mbits
    return np.copysign(np.ldexp(np.floor(np.ldexp(a, -q)), q), v)


def half_ulp(mag, code):
    """Half a unit in the last place of the element type at the magnitudes `mag` (float64 array); 0 for f64."""
    if code == 0:
        return np.zeros_like(np.asarray(mag, dtype=np.float64))
    _, mbits, emin, _ = TYPES[code]
    mag = np.abs(np.asarray(mag, dtype=np.float64))
    e = np.frexp(np.where(mag > 0, mag, 1.0))[1] - 1
    e = np.where(mag > 0, e, emin)
    return np.ldexp(0.5, np.maximum(e, emin) - mbits)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    """Equal as arrays of bits, any NaN counting as equal to any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------------------------------------------- the model
def model_stats(X):
    """(min, max, sum as longdouble, bound of the sum) per column of the float64 array X; a column with a NaN: NaN."""
    X = np.asarray(X, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return X.min(axis=0), X.max(axis=0), X.astype(LD).sum(axis=0), (X.shape[0] + 4) * U * np.abs(X).astype(LD).sum(axis=0)


def model_scale(X, lo, span, code=0):
    """The bits ital_scale_rows must write: numpy's own FP64 subtraction and division, then one rounding."""
    X = np.asarray(X, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return round_to((X - np.asarray(lo, dtype=np.float64)) / np.asarray(span, dtype=np.float64), code)


def model_cov(X, mean):
    """(C as longdouble [d, d], its bound) for the float64 rows X and the float64 mean the device was given."""
    Z = np.asarray(X, dtype=np.float64).astype(LD) - np.asarray(mean, dtype=np.float64).astype(LD)
    A = np.abs(Z)
    return Z.T @ Z, (X.shape[0] + 8) * U * (A.T @ A)


def model_project(X, shift, W):
    """(Y as longdouble [n, k], its bound) before any narrowing."""
    Z = np.asarray(X, dtype=np.float64).astype(LD) - np.asarray(shift, dtype=np.float64).astype(LD)
    W = np.asarray(W, dtype=np.float64).astype(LD)
    return Z @ W, (X.shape[1] + 8) * U * (np.abs(Z) @ np.abs(W))


# ---------------------------------------------------------------------------------------------------- the checkers
def _worst(err, bound):
    """max err / bound over the entries (0 / 0 counts as 0); asserts it is at most 1 and that no entry is NaN."""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    assert not np.isnan(err).any(), "NaN where a number is due"
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0, LD(0), err / np.where(bound > 0, bound, LD(1e-4900)))
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, "outside the bound: %.3g of it" % worst
    return worst


def check_stats(cmin, cmax, csum, X):
    """The three outputs of ital_col_stats against the float64 rows X.  Returns the worst error of a sum as a fraction of
    its bound."""
    mn, mx, s, bound = model_stats(X)
    nan = np.isnan(np.asarray(X, dtype=np.float64)).any(axis=0)
    for got in (cmin, cmax, csum):
        assert np.array_equal(np.isnan(got), nan), "the NaN rule"
    ok = ~nan
    assert np.array_equal(np.asarray(cmin)[ok], mn[ok]) and np.array_equal(np.asarray(cmax)[ok], mx[ok]), "min / max"
    return _worst(np.abs(np.asarray(csum, dtype=np.float64)[ok].astype(LD) - s[ok]), bound[ok])


def check_cov(C, X, mean):
    """The d x d result of ital_col_cov: symmetric in bits and within the bound of the model."""
    C = np.asarray(C, dtype=np.float64)
    assert same_bits(C, C.T), "C[a][b] and C[b][a] differ in bits"
    want, bound = model_cov(X, mean)
    return _worst(np.abs(C.astype(LD) - want), bound)


def check_project(Y, X, shift, W, code=0):
    """Y: the [n, ldy] result of ital_project_rows as float64 values (exact widening of what was stored).  Columns beyond k
    must hold +0.0; the others lie within the bound of the model plus half a unit of the element type `code`."""
    Y = np.asarray(Y, dtype=np.float64)
    k = np.asarray(W).shape[1]
    assert not bits(Y[:, k:]).any(), "a pad column that is not +0.0"
    want, bound = model_project(X, shift, W)
    if code:
        assert same_bits(Y[:, :k], round_to(Y[:, :k], code)), "a value the element type does not have"
        over = TYPES[code][3]
        assert (np.abs(want) + bound < over).all(), "the checker does not cover overflow"
        bound = bound + half_ulp((np.abs(want) + bound).astype(np.float64), code).astype(LD)
    return _worst(np.abs(Y[:, :k].astype(LD) - want), bound)


def check_scale(Y, X, lo, span, code=0):
    """Y [n, ldy] as float64 values: the bits of model_scale in the first d columns, +0.0 beyond."""
    Y = np.asarray(Y, dtype=np.float64)
    d = np.asarray(X).shape[1]
    assert not bits(Y[:, d:]).any(), "a pad column that is not +0.0"
    assert same_bits(Y[:, :d], model_scale(X, lo, span, code)), "not the bits of (X - lo) / span"


def subspace_sine(U_, V_):
    """|| (I - U U^T) V ||_F for two d x k matrices with orthonormal columns: the Frobenius norm of the sines of the
    canonical angles between their column spaces."""
    U_, V_ = np.asarray(U_, dtype=LD), np.asarray(V_, dtype=LD)
    return float(np.sqrt(((V_ - U_ @ (U_.T @ V_)) ** 2).sum()))
