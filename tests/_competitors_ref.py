"""What the tests of TCAL and RBMAL share (tests/test_competitors_host.py, tests/test_gpu_competitors.py): the golden fixtures
of tests/golden/make_golden_competitors.py, and an extended-precision host model of the DEFINITION of ital_cosine_min
(include/ital_cosine.h) with the checker that compares a result against it.

THE BOUND.  u = 2^-53 is the largest relative error of one correctly rounded FP64 operation.  On the scale of cos (|cos| <= 1
after the clip, and |x . t| <= |x| |t|) the device value of one pair collects
    the dot product      ldx + 1   a chain of ldx multiply-adds, one more rounding if the products are rounded on their own;
                                   relative to sum |x_k t_k| <= |x| |t|
    the two norms        ldx + 1   each squared norm is such a chain over positive terms, (ldx + 1) u relative; the root halves it
    the two roots        2
    their product        1
    the quotient         1
    the difference       2         one rounding of a value of at most 2
in units of u: 2 ldx + 8.  Two more units cover the second-order terms and the model's own error (np.longdouble, 64
significant bits: ldx 2^-64 for its dot product), so
    |d_dev - d_model| <= (2 ldx + 10) 2^-53                                     (a = 2, b = 10)
absolute.  The minimum over j and over calls is exact and adds nothing.  The same bound holds for scipy's cdist with the number
of columns d in place of ldx: it forms the same quantities in FP64.
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

TCAL_FIXTURES = ["tcal_synth150", "tcal_usps500", "tcal_synth60_retry"]
RBMAL_FIXTURES = ["rbmal_synth150", "rbmal_usps500", "rbmal_butterflies"]
MARGIN = 1e-9

_cache = {}


def load(name):
    """(npz, X) of a fixture, loaded once; the rows of some fixtures are those of an older one (`X_from`)."""
    if name not in _cache:
        z = np.load(os.path.join(GOLD, name + ".npz"))
        X = z["X"] if "X" in z.files else np.load(os.path.join(GOLD, str(z["X_from"]) + ".npz"))["X"]
        _cache[name] = (z, X)                  # shared among the tests: treat as read-only
    return _cache[name]


def rng_state(z, prefix):
    """The generator state that make_golden_competitors.state_arrays stored under `prefix`, as np.random.set_state takes it."""
    pos = z[prefix + "_pos"]
    return ("MT19937", z[prefix + "_key"], int(pos[0]), int(pos[1]), float(z[prefix + "_gauss"]))


def same_rng_state(z, prefix):
    st = np.random.get_state(legacy=True)
    want = rng_state(z, prefix)
    return st[0] == want[0] and np.array_equal(st[1], want[1]) and tuple(st[2:]) == tuple(want[2:])


# ------------------------------------------------------------------------------------------------ ital_cosine_min
def bound(ldx):
    return (2 * ldx + 10) * 2.0 ** -53


def pair_model(X, xnorm, T, tnorm):
    """d[i][j] of the DEFINITION in np.longdouble.  The norms are the FP64 inputs, as the kernel gets them.  A dot product
    below FP64's smallest subnormal is the zero the FP64 sum gives (it decides between inf and NaN over a zero norm)."""
    ld = np.longdouble
    dot = np.asarray(X, dtype=ld) @ np.asarray(T, dtype=ld).T
    dot = np.where(np.abs(dot) < ld(2.0) ** -1075, ld(0), dot)
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = dot / (np.sqrt(np.asarray(xnorm, dtype=ld))[:, None] * np.sqrt(np.asarray(tnorm, dtype=ld))[None, :])
        cos = np.where(np.abs(cos) > 1, np.copysign(ld(1), cos), cos)
    return 1 - cos


def model(X, xnorm, T, tnorm, prev=None):
    """out[i] of the DEFINITION (np.longdouble): the NaN-propagating minimum over j, and with `prev` (accumulate) over it."""
    d = pair_model(X, xnorm, T, tnorm).min(axis=1)          # np.min propagates NaN
    if prev is not None:
        d = np.minimum(np.asarray(prev, dtype=np.longdouble), d)     # so does np.minimum
    return d


def check(got, X, xnorm, T, tnorm, ncols, prev=None):
    """Raises AssertionError unless `got` has the model's NaN positions and lies within bound(ncols) of it elsewhere.
    Returns the largest ratio of an error to the bound."""
    got = np.asarray(got)
    want = model(X, xnorm, T, tnorm, prev)
    assert got.shape == want.shape, (got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "NaN positions differ: %s vs %s" % (np.flatnonzero(np.isnan(got)), np.flatnonzero(nan))
    if nan.all():
        return 0.0
    err = np.abs(got[~nan].astype(np.longdouble) - want[~nan])
    ratio = float(err.max() / bound(ncols))
    assert ratio <= 1.0, "error %g is %.3g times the bound %g" % (float(err.max()), ratio, bound(ncols))
    return ratio
