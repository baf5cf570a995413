"""The kernels of include/ital_prepare.h on the device against the extended-precision model and the checkers of
tests/_prepare_ref.py (where the bounds are derived), the equalities they hold in bits, and ital_amd/prepare.py end to end.
Run on the GPU box: python -m pytest tests -m gpu."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _prepare_ref as ref  # noqa: E402

from ital_amd import _lib  # noqa: E402

NS = (1, 2, 17, 127, 128, 129, 300)          # 129: one row more than one range of ital_col_stats
DS = (1, 5, 16, 17, 40, 129, 257)            # 129 / 257: ragged tiles, 3 / 6 lower-triangular tile pairs
KS = (1, 5, 16, 17, 129)
N_COV_RANGE = _lib.PREPARE_COV_UNIT + 1                                # one row more than one range of ital_col_cov
N_COV_CAP = _lib.PREPARE_COV_UNIT * _lib.PREPARE_COV_CAP + 1           # one row more than its 32 ranges of one unit
N_STATS_CAP = _lib.PREPARE_STATS_UNIT * _lib.PREPARE_STATS_CAP + 1     # and of ital_col_stats: 131 073 x 3 doubles = 3 MB
SHAPES = [(n, d) for n in NS for d in (5, 17)] + [(n, d) for n in (129, 300) for d in DS if d not in (5, 17)]
GUARD = 64
DTYPES = (torch.float64, torch.float32, torch.float16, torch.bfloat16)
CODES = {torch.float64: 0, torch.float32: 1, torch.float16: 2, torch.bfloat16: 3}
IDS = {torch.float64: "f64", torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _values(n, d, dtype, seed=0):
    """n x d float64 values that the element type holds exactly: columns of different scale and offset, duplicate rows and
    (from 3 columns on) a column of constants."""
    rng = np.random.default_rng(1000 * n + d + seed)
    X = rng.normal(size=(n, d)) * (1.0 + np.arange(d) % 4) + (np.arange(d) % 3 - 1.0)
    if d >= 3:
        X[:, 2] = 0.375
    if n > 11:
        X[7] = X[3]
        X[11] = X[3]
    return torch.from_numpy(X).to(dtype).to(torch.float64).numpy()


def _padded(vals, dtype, dev, extra=0):
    """The values as a padded device matrix of the element type; with `extra` the row stride is that much longer and the
    columns from d on hold 7, which nothing may read."""
    n, d = vals.shape
    M = torch.full((n, (d + 15) // 16 * 16 + extra), 7.0 if extra else 0.0, dtype=torch.float64, device=dev)
    M[:, :d] = torch.from_numpy(vals).to(dev)
    return M.to(dtype)


class Guarded(object):
    """A device buffer of `count` elements between guard elements."""

    def __init__(self, count, dtype, dev):
        self.count = count
        self.fill = 0x5A if dtype == torch.uint8 else -7.0
        self.t = torch.full((count + 2 * GUARD,), self.fill, dtype=dtype, device=dev)

    @property
    def data(self):
        return self.t[GUARD:GUARD + self.count]

    def ptr(self):
        return self.t[GUARD:].data_ptr()

    def check(self):
        assert (self.t[:GUARD] == self.fill).all() and (self.t[GUARD + self.count:] == self.fill).all()


def _host(t):
    return t.to(torch.float64).cpu().numpy()


def _vec(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _col_stats(X, n, d):
    lib = _lib.lib()
    out = [Guarded(d, torch.float64, X.device) for _ in range(3)]
    need = lib.ital_col_stats_workspace(n, d)
    work = Guarded(need, torch.uint8, X.device)
    _lib.check(lib.ital_col_stats(X.data_ptr(), CODES[X.dtype], n, d, X.shape[1], out[0].ptr(), out[1].ptr(), out[2].ptr(),
                                  work.ptr(), need, _stream()))
    for g in out + [work]:
        g.check()
    return [_host(g.data) for g in out]


def _scale(X, n, d, lo, span, ydtype, ldy=None):
    ldy = ldy or (d + 15) // 16 * 16
    Y = Guarded(n * ldy, ydtype, X.device)
    lo, span = _vec(lo, X.device), _vec(span, X.device)                 # held until the call is enqueued
    _lib.check(_lib.lib().ital_scale_rows(X.data_ptr(), CODES[X.dtype], n, d, X.shape[1], lo.data_ptr(), span.data_ptr(), Y.ptr(),
                                          CODES[ydtype], ldy, _stream()))
    Y.check()
    return _host(Y.data.view(n, ldy))


def _cov(X, n, d, mean, ldc=None, raw=False):
    lib = _lib.lib()
    ldc = ldc or d
    C = Guarded(d * ldc, torch.float64, X.device)
    need = lib.ital_col_cov_workspace(n, d)
    work = Guarded(need, torch.uint8, X.device)
    mean = _vec(mean, X.device)
    _lib.check(lib.ital_col_cov(X.data_ptr(), CODES[X.dtype], n, d, X.shape[1], mean.data_ptr(), C.ptr(), ldc, work.ptr(), need,
                                _stream()))
    C.check()
    work.check()
    full = C.data.view(d, ldc)
    assert (full[:, d:] == -7.0).all()                                  # the columns between d and ldc belong to the caller
    return full[:, :d].clone() if raw else _host(full[:, :d])


def _project(X, n, d, shift, W, ydtype, ldy=None):
    k = W.shape[1]
    ldy = ldy or (k + 15) // 16 * 16
    Y = Guarded(n * ldy, ydtype, X.device)
    shift, Wd = _vec(shift, X.device), _vec(W, X.device)
    _lib.check(_lib.lib().ital_project_rows(X.data_ptr(), CODES[X.dtype], n, d, X.shape[1], shift.data_ptr(), Wd.data_ptr(), k, k,
                                            Y.ptr(), CODES[ydtype], ldy, _stream()))
    Y.check()
    return _host(Y.data.view(n, ldy))


# ------------------------------------------------------------------------------------------------------ ital_col_stats
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_col_stats(dev, dtype):
    worst = 0.0
    for n, d in SHAPES + [(N_STATS_CAP, 3)]:
        vals = _values(n, d, dtype)
        extra = 16 if n == 300 else 0
        mn, mx, sm = _col_stats(_padded(vals, dtype, dev, extra), n, d)
        worst = max(worst, ref.check_stats(mn, mx, sm, vals))
    print("col_stats %s: worst sum error %.3g of its bound" % (IDS[dtype], worst))


def test_col_stats_nan_and_infinities(dev):
    vals = _values(300, 6, torch.float64)
    vals[150, 1] = np.nan
    vals[0, 3], vals[299, 3] = np.inf, 5.0
    vals[1, 4], vals[2, 4] = np.inf, -np.inf                            # no NaN in the column: only its sum is NaN
    mn, mx, sm = _col_stats(_padded(vals, torch.float64, dev), 300, 6)
    assert np.isnan([mn[1], mx[1], sm[1]]).all()
    assert mx[3] == np.inf and sm[3] == np.inf and mn[3] == vals[:, 3].min()
    assert mn[4] == -np.inf and mx[4] == np.inf and np.isnan(sm[4])
    keep = [0, 2, 5]
    ref.check_stats(mn[keep], mx[keep], sm[keep], vals[:, keep])


# ------------------------------------------------------------------------------------------------------ ital_scale_rows
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_scale_rows_has_numpys_bits(dev, dtype):
    for n, d in SHAPES:
        vals = _values(n, d, dtype)
        X = _padded(vals, dtype, dev, 16 if n == 300 else 0)
        lo, hi = vals.min(), vals.max()
        glob = (np.full(d, lo), np.full(d, hi - lo if hi > lo else 1.0))
        span = vals.max(axis=0) - vals.min(axis=0)
        span[span == 0] = 1.0
        for shift, sp in (glob, (vals.min(axis=0), span)):
            ref.check_scale(_scale(X, n, d, shift, sp, torch.float64), vals, shift, sp)
        for ydtype in DTYPES[1:]:
            ref.check_scale(_scale(X, n, d, glob[0], glob[1], ydtype, ldy=(d + 15) // 16 * 16 + 16), vals, glob[0], glob[1],
                            CODES[ydtype])


def test_scale_rows_narrowing_edges(dev):
    """Ties, the overflow threshold, subnormals, signed zeros, infinities and NaN through the one rounding."""
    edge = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -24,
                     65519.999, 65520.0, -65520.0, 65504.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -26, -0.0, 0.0,
                     np.inf, -np.inf, np.nan, 3.3895313892515355e38, 3.3961775292304601e38, 3.4028235677973366e38, 1e-40, 1e-320,
                     2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1 / 3.0])
    vals = np.tile(edge, (3, 1))
    d = vals.shape[1]
    X = _padded(vals, torch.float64, dev)
    lo, span = np.zeros(d), np.ones(d)
    for ydtype in DTYPES:
        got = _scale(X, 3, d, lo, span, ydtype)
        ref.check_scale(got, vals, lo, span, CODES[ydtype])
    f16 = _scale(X, 3, d, lo, span, torch.float16)[0]
    assert f16[5] == 65504.0 and f16[6] == np.inf and f16[7] == -np.inf and f16[9] == 2.0 ** -24 and f16[10] == 0.0
    assert np.signbit(f16[13]) and not np.signbit(f16[14]) and np.isnan(f16[17])


def test_scale_rows_reproduces_the_reference(dev, golden_dir):
    z = np.load(os.path.join(golden_dir, "prepare_minmax.npz"))
    lo, hi = z["X_train"].min(), z["X_train"].max()
    for name in ("X_train", "X_test"):
        vals = z[name]
        got = _scale(_padded(vals, torch.float64, dev), vals.shape[0], 5, np.full(5, lo), np.full(5, hi - lo), torch.float64)
        assert ref.same_bits(got[:, :5], z[name + "_norm"])


# ------------------------------------------------------------------------------------------------------ ital_col_cov
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_col_cov(dev, dtype):
    worst = 0.0
    for n, d in SHAPES + [(N_COV_RANGE, 5), (N_COV_CAP, 3)]:
        vals = _values(n, d, dtype)
        mean = vals.sum(axis=0) / n
        C = _cov(_padded(vals, dtype, dev, 16 if n == 300 else 0), n, d, mean, ldc=d + (3 if n == 129 else 0))
        worst = max(worst, ref.check_cov(C, vals, mean))
        if n == 1:
            assert not ref.bits(C).any()                                # exactly +0
    print("col_cov %s: worst error %.3g of its bound" % (IDS[dtype], worst))


def test_col_cov_masks_rows_after_centring(dev):
    """Large means: a masked row entering as 0 - mean, or a pad column as -mean, would be far outside the bound."""
    for n, d in ((17, 5), (N_COV_RANGE, 17), (300, 129)):
        vals = _values(n, d, torch.float64) + 1e3
        mean = vals.sum(axis=0) / n
        ref.check_cov(_cov(_padded(vals, torch.float64, dev), n, d, mean), vals, mean)


def test_col_cov_has_the_same_bits_on_any_stream(dev):
    n, d = 2 * _lib.PREPARE_COV_UNIT + 77, 129
    vals = _values(n, d, torch.float32)
    X = _padded(vals, torch.float32, dev)
    mean = vals.sum(axis=0) / n
    first = _cov(X, n, d, mean, raw=True)
    other = torch.cuda.Stream(device=dev)
    other.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(other):
        second = _cov(X, n, d, mean, raw=True)
    other.synchronize()
    torch.mm(torch.ones((64, 64), device=dev), torch.ones((64, 64), device=dev))    # an unrelated launch in between
    third = _cov(X, n, d, mean, ldc=d + 5, raw=True)
    assert torch.equal(first.view(torch.int64), second.view(torch.int64))
    assert torch.equal(first.view(torch.int64), third.view(torch.int64))
    assert ref.same_bits(_host(first), _host(_cov(_padded(vals, torch.float64, dev), n, d, mean, raw=True)))   # widening is exact


# ------------------------------------------------------------------------------------------------------ ital_project_rows
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_project_rows(dev, dtype):
    worst = 0.0
    rng = np.random.default_rng(5)
    cases = [(n, d, k) for n, d in SHAPES for k in ((1, 5) if d > 1 else (1,)) if k <= d]
    cases += [(300, 257, k) for k in KS] + [(129, 129, 129), (300, 40, 17), (127, 17, 16)]
    for n, d, k in cases:
        vals = _values(n, d, dtype)
        shift, W = vals.sum(axis=0) / n, rng.normal(size=(d, k))
        X = _padded(vals, dtype, dev, 16 if n == 300 else 0)
        worst = max(worst, ref.check_project(_project(X, n, d, shift, W, torch.float64), vals, shift, W))
        ydtype = DTYPES[1 + (n + d + k) % 3]
        ldy = (k + 15) // 16 * 16 + (16 if k % 2 else 0)
        ref.check_project(_project(X, n, d, shift, W, ydtype, ldy), vals, shift, W, CODES[ydtype])
    print("project_rows %s: worst error %.3g of its bound" % (IDS[dtype], worst))


def test_project_rows_does_not_depend_on_the_row_or_the_type(dev):
    vals = _values(300, 40, torch.float16)
    shift, W = vals.sum(axis=0) / 300, np.random.default_rng(6).normal(size=(40, 17))
    whole = _project(_padded(vals, torch.float16, dev), 300, 40, shift, W, torch.float64)
    part = _project(_padded(vals[131:], torch.float64, dev), 169, 40, shift, W, torch.float64)
    assert ref.same_bits(whole[131:], part)


# ------------------------------------------------------------------------------------------------------ ital_amd.prepare
@pytest.mark.parametrize("storage,dtype", [("f64", torch.float64), ("f32", torch.float32), ("f16", torch.float16),
                                           ("bf16", torch.bfloat16)])
def test_apply_fills_xnorm_by_the_stores_route(dev, storage, dtype):
    from ital_amd import PCA, DeviceData, MinMax
    vals = _values(300, 20, torch.float32)
    src = DeviceData(torch.from_numpy(vals).to(torch.float32), storage="source", device=dev)
    ptr, before = src.X.data_ptr(), src.X.clone()
    with pytest.raises(ValueError):
        MinMax.fit(src).then(MinMax.fit(DeviceData(vals[:, :3], device=dev)))
    T = MinMax.fit(src)
    T = T.then(PCA.fit(T.apply(src), 4))
    out = T.apply(src, storage=storage, chunk_bytes=1 << 14)                                      # several pieces
    assert out.shape == (300, 4) and out.X.dtype == dtype and out.ldx == 16 and out.epoch == 0
    assert src.X.data_ptr() == ptr and torch.equal(src.X, before) and src.epoch == 0
    again = DeviceData(out.X[:, :4].clone(), storage="source", device=dev)
    assert torch.equal(out.xnorm.view(torch.int64), again.xnorm.view(torch.int64))
    assert torch.equal(out.X, again.X) and not out.X[:, 4:].to(torch.float64).view(torch.int64).any()
    one = T.apply(src, storage=storage)                                                           # one piece: the same bits
    assert torch.equal(one.X, out.X)
    rows = T.apply(torch.from_numpy(vals).to(torch.float32), storage=storage, chunk_bytes=1 << 14)
    assert rows.shape == (300, 4) and rows.dtype == dtype and torch.equal(rows, out.X[:, :4])
    assert out.append(rows[:5]) == 5 and len(out) == 305


def test_min_max_end_to_end(dev, golden_dir):
    from ital_amd import ITAL, DeviceData, MinMax, column_stats, mvn_stream
    z = np.load(os.path.join(golden_dir, "prepare_minmax.npz"))
    store = DeviceData(z["X_train"], device=dev)
    T = MinMax.fit(store)
    assert ref.same_bits(T.apply(store).rows(), z["X_train_norm"])
    assert ref.same_bits(_host(T.apply(z["X_test"])), z["X_test_norm"])
    st = column_stats(store)
    assert np.array_equal(st.min, z["X_train"].min(axis=0)) and np.array_equal(st.max, z["X_train"].max(axis=0))
    per = MinMax.fit(store, per_column=True)
    assert per.span[4] == 1.0 and not per.apply(store).rows()[:, 4].any()
    with pytest.raises(ValueError):
        MinMax.fit(DeviceData(np.full((4, 3), 2.5), device=dev))

    raw = np.random.default_rng(8).normal(size=(120, 6)) * 3 + 1
    host = (raw - raw.min()) / (raw.max() - raw.min())
    ls = float(np.sqrt(6 / 12.0))
    runs = []
    for data in (MinMax.fit(DeviceData(raw, device=dev)).apply(DeviceData(raw, device=dev)), host):
        mvn_stream.GLOBAL.reset()
        L = ITAL(data, length_scale=ls, device=dev)
        L.update({5: 1})
        picks = []
        for _ in range(2):
            got = [int(i) for i in L.fetch_unlabelled(3)]
            picks.append(got)
            L.update({i: (1 if host[i, 0] > 0.5 else -1) for i in got})
        runs.append((picks, np.array(L.rel_mean)))
    assert runs[0][0] == runs[1][0] and ref.same_bits(runs[0][1], runs[1][1])


def test_pca_end_to_end(dev):
    """Rank-3 data plus 1e-6 noise in d = 20: the top-3 subspace within the Davis-Kahan angle of numpy's on the
    longdouble-centred data, sin Theta <= ||bound matrix||_F / gap with gap = lambda_3 - lambda_4 of numpy's matrix.  The
    bound matrix is that of C for the mean the device used (tests/_prepare_ref.py) plus n dm dm^T, dm = that mean minus the
    longdouble one: the rows centred by the exact mean sum to zero, so C(m + dm) = C(m) + n dm dm^T exactly -- the reference
    matrix is centred by another mean than the device's, and this is all the difference (about 1e-30 here)."""
    from ital_amd import PCA, DeviceData
    from ital_amd.prepare import scatter_matrix
    rng = np.random.default_rng(9)
    n, d, k = 400, 20, 3
    vals = rng.normal(size=(n, 3)) * np.array([5.0, 3.0, 2.0]) @ np.linalg.qr(rng.normal(size=(d, 3)))[0].T
    vals = vals + 1e-6 * rng.normal(size=(n, d)) + rng.normal(size=d)
    store = DeviceData(vals, device=dev)
    T = PCA.fit(store, k)
    mean_ld = vals.astype(ref.LD).sum(axis=0) / n
    Z = vals.astype(ref.LD) - mean_ld
    C_ld = np.asarray(Z.T @ Z / (n - 1), dtype=np.float64)
    lam, V = np.linalg.eigh(C_ld)
    lam, V = lam[::-1], V[:, ::-1]
    _, bound = ref.model_cov(vals, T.shift)
    dm = np.abs(T.shift.astype(ref.LD) - mean_ld)
    assert (dm <= ref.model_stats(vals)[3] / n + ref.U * np.abs(mean_ld)).all()
    E = np.asarray(bound + n * np.outer(dm, dm), dtype=np.float64) / (n - 1)
    allowed = np.linalg.norm(E, "fro") / (lam[k - 1] - lam[k])
    sine = ref.subspace_sine(V[:, :k], T.W)
    print("pca: sin Theta %.3g, allowed %.3g" % (sine, allowed))
    assert sine <= allowed
    np.testing.assert_allclose(T.eigenvalues, lam[:k], rtol=1e-12)
    back = type(T).from_state_dict(T.state_dict())
    assert np.array_equal(back.eigenvalues, T.eigenvalues) and np.array_equal(back.W, T.W) and T.then(T.__class__(
        [(0, np.zeros(k), np.ones(k))])).eigenvalues is None
    assert np.array_equal(scatter_matrix(store, T.shift), scatter_matrix(store, T.shift))
    out = T.apply(store)
    ref.check_project(_host(out.X), vals, T.shift, T.W)
    ref.check_project(_host(T.apply(store, storage="f16").X), vals, T.shift, T.W, 2)
    white = PCA.fit(store, k, whiten=True)
    np.testing.assert_allclose(white.apply(store).rows().var(axis=0, ddof=1), 1.0, rtol=1e-9)
    assert np.array_equal(white.eigenvalues, T.eigenvalues)
    flat = DeviceData(np.hstack([rng.normal(size=(30, 2)), np.full((30, 1), 2.5), np.full((30, 1), -1.0)]), device=dev)
    assert not (PCA.fit(flat, 4).eigenvalues[2:] > 0).any()         # two constant columns: exact zero rows of C, no variance
    with pytest.raises(ValueError, match="whiten"):
        PCA.fit(flat, 4, whiten=True)
    for bad in (0, 21, 2.5):
        with pytest.raises(ValueError):
            PCA.fit(store, bad)
    with pytest.raises(ValueError):
        PCA.fit(DeviceData(vals[:1], device=dev), 1)


def test_apply_never_holds_an_fp64_copy_of_the_input(dev):
    from ital_amd import PCA, DeviceData
    n, d, k = 20000, 64, 16
    vals = (torch.randn((n, d), generator=torch.Generator().manual_seed(3)) * 2).to(torch.float16)
    store = DeviceData(vals, storage="source", device=dev, chunk_bytes=1 << 20)
    T = PCA.fit(store, k)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = T.apply(store, storage="f16", chunk_bytes=1 << 20)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    out_bytes = out._X.numel() * 2 + out._xnorm.numel() * 8
    assert out.shape == (n, k) and peak < out_bytes + n * d * 8, (peak, out_bytes)
    print("apply 20000 x 64 f16 -> 16: peak %d B beyond the input, output %d B, an FP64 copy would be %d B"
          % (peak, out_bytes, n * d * 8))
