"""Feature rows kept in their source precision on the device (DeviceData(storage="source"), include/ital_rows.h).

The widening conversion f16 / bf16 / f32 -> f64 is exact, and the typed kernels form (double)element in registers and feed the
same operands in the same order to the same FP64 MFMA and FP64 arithmetic.  So nothing here has a tolerance: every result on
compact rows is compared BY ITS BITS (int64 views; NaN and the sign of zero included) with the result of the existing FP64
entry point, or of a learner on the FP64 store, on the exactly widened rows.  The host side is tests/test_compact_store_host.py.
Run: python -m pytest tests -m gpu."""
import ctypes
import gc
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden  # noqa: E402  (fixture table only)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


def _pad16(v):
    return (v + 15) // 16 * 16


NARROW = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CODES = {torch.float64: 0, torch.float32: 1, torch.float16: 2, torch.bfloat16: 3}
BITS = {torch.float64: torch.int64, torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
NS = (1, 15, 16, 17, 63, 64, 65, 257)
DS = (1, 3, 4, 5, 15, 16, 17, 64, 65, 130)        # pad edge, lane-vector edge (4), a partial trip of four 16-feature steps


def _values(n, d, dtype, seed):
    """n x d host values of `dtype`, among them -0.0, the type's smallest subnormal and its largest finite value (as
    tests/test_gpu_device_data.py draws them)."""
    g = torch.Generator().manual_seed(seed)
    v = (torch.randn((n, d), generator=g, dtype=torch.float64) * 3).to(dtype)
    flat = v.view(-1)
    info = torch.finfo(dtype)
    for at, s in enumerate([-0.0, 0.0, 1.0]):
        if at < flat.numel():
            flat[at] = s
    if flat.numel() > 5:
        flat[3] = torch.tensor(info.smallest_normal, dtype=dtype) * torch.tensor(info.eps, dtype=dtype)
        flat[4] = -info.max if dtype is not torch.float64 else -1e150
        assert flat[3] != 0
    return v


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(BITS[a.dtype]), b.view(BITS[b.dtype]))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rows(vals, dev, extra=0):
    """The values as compact padded rows (built with tensor operations, not by the kernel under test), their exact FP64
    expansion and its norms by ital_row_norms."""
    from ital_amd import _lib
    n, d = vals.shape
    ldx = _pad16(d)
    Xc = torch.zeros((n + extra, ldx), dtype=vals.dtype, device=dev)
    Xc[:n, :d] = vals.to(dev)
    Xf = Xc.to(torch.float64)
    xn = torch.zeros(n + extra, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().ital_row_norms(Xf.data_ptr(), n, ldx, xn.data_ptr(), _stream()))
    return Xc, Xf, xn, ldx


def _rand(shape, dev, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).to(dev)


def _selected(c, d, ldx, dev, seed):
    """c FP64 rows that are no data rows, zero padded, and their norms."""
    from ital_amd import _lib
    Xs = torch.zeros((16, ldx), dtype=torch.float64, device=dev)
    Xs[:, :d] = _rand((16, d), dev, seed, 3.0)
    sn = torch.zeros(16, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().ital_row_norms(Xs.data_ptr(), 16, ldx, sn.data_ptr(), _stream()))
    return Xs, sn


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("name", list(NARROW))
def test_the_whitening_sweep_on_typed_rows_has_the_bits_of_the_fp64_sweep(dev, name):
    """ital_whiten_append_t against ital_whiten_append on the widened rows: the appended rows of V, mu and s2."""
    from ital_amd import _lib
    lib, dtype = _lib.lib(), NARROW[name]
    live = 0
    for n in NS:
        for d in DS:
            Xc, Xf, xn, ldx = _rows(_values(n, d, dtype, 1000 * n + d), dev)
            ls = 3.0 * float(np.sqrt(2 * d))
            for c, m in ((5, 17), (16, 0)):
                ldw, ldv = 48, _pad16(n)
                Xs, sn = _selected(c, d, ldx, dev, n + d + c)
                Lblk = _rand((16, ldw), dev, 7 + c, 0.3)
                Lblk[:, m:m + 16] = torch.tril(Lblk[:, m:m + 16]) + 2.0 * torch.eye(16, dtype=torch.float64, device=dev)
                alpha = _rand((16,), dev, 11)
                V0, mu0, s20 = _rand((m + 16, ldv), dev, 13, 0.1), _rand((n,), dev, 17), _rand((n,), dev, 19)
                got = []
                for X, xtype in ((Xf, None), (Xc, CODES[dtype])):
                    V, mu, s2 = V0.clone(), mu0.clone(), s20.clone()
                    args = (X.data_ptr(), xn.data_ptr(), n, ldx, Xs.data_ptr(), sn.data_ptr(), c, Lblk.data_ptr(), ldw,
                            Lblk.data_ptr() + 8 * m, alpha.data_ptr(), V.data_ptr(), ldv, m, 1.0, ls, mu.data_ptr(), s2.data_ptr())
                    if xtype is None:
                        _lib.check(lib.ital_whiten_append(*args, _stream()))
                    else:
                        _lib.check(lib.ital_whiten_append_t(*args, xtype, _stream()))
                    got.append((V, mu, s2))
                (Va, mua, s2a), (Vb, mub, s2b) = got
                what = (name, n, d, c, m)
                assert _same_bits(Va, Vb) and _same_bits(mua, mub) and _same_bits(s2a, s2b), what
                assert _same_bits(Va[:m], V0[:m]) and not _same_bits(Va[m:m + c, :n], V0[m:m + c, :n]), what
                live += int((Va[m:m + c, :n].abs() > 1e-300).sum())
    assert live > 1000          # the comparison is not one of underflowed kernels


@pytest.mark.parametrize("name", list(NARROW))
def test_kernel_columns_on_typed_rows(dev, name):
    """ital_rbf_cols_t and ital_cross_cov_cols_t at c in {1, 5, 16}, m in {0, 1, 17}."""
    from ital_amd import _lib
    lib, dtype = _lib.lib(), NARROW[name]
    for n in (1, 17, 65, 257):
        for d in (1, 5, 17, 130):
            Xc, Xf, xn, ldx = _rows(_values(n, d, dtype, 77 * n + d), dev)
            ls, ldo = 3.0 * float(np.sqrt(2 * d)), _pad16(n)
            for c in (1, 5, 16):
                Xs, sn = _selected(c, d, ldx, dev, n + d + c)
                head = (xn.data_ptr(), n, ldx, Xs.data_ptr(), sn.data_ptr(), c)
                a, b = (torch.full((c, ldo), float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
                _lib.check(lib.ital_rbf_cols(Xf.data_ptr(), *head, 1.3, ls, a.data_ptr(), ldo, _stream()))
                _lib.check(lib.ital_rbf_cols_t(Xc.data_ptr(), *head, 1.3, ls, b.data_ptr(), ldo, CODES[dtype], _stream()))
                assert _same_bits(a, b) and bool(torch.isfinite(a[:, :n]).all()) and bool(torch.isnan(a[:, n:]).all()), (name, n, d, c)
                for m in (0, 1, 17):
                    W, V = _rand((16, 32), dev, m + 3, 0.2), _rand((max(m, 1), ldo), dev, m + 5, 0.2)
                    a, b = (torch.full((c, ldo), float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
                    tail = (W.data_ptr(), 32, V.data_ptr(), ldo, m, 1.3, ls)
                    _lib.check(lib.ital_cross_cov_cols(Xf.data_ptr(), *head, *tail, a.data_ptr(), ldo, _stream()))
                    _lib.check(lib.ital_cross_cov_cols_t(Xc.data_ptr(), *head, *tail, b.data_ptr(), ldo, CODES[dtype], _stream()))
                    assert _same_bits(a, b) and bool(torch.isfinite(a[:, :n]).all()), (name, n, d, c, m)


def _fitted_gp(vals, dev, m):
    """An FP64 model on the widened values with m labels: the labelled-set state the row sweeps are run against."""
    from ital_amd import GaussianProcess
    n, d = vals.shape
    gp = GaussianProcess(vals.to(torch.float64).numpy(), 3.0 * float(np.sqrt(2 * d)), device=dev, capacity=48)
    idx = np.random.default_rng(m).permutation(n)[:m]
    idx = idx[idx > 5][: m]                # not the rows that hold the extreme values
    gp.update(idx.tolist(), np.where(np.arange(len(idx)) % 3 == 0, 1.0, -1.0))
    torch.cuda.synchronize()
    return gp


@pytest.mark.parametrize("chunk", [0, 32])
@pytest.mark.parametrize("name", list(NARROW))
def test_whiten_rows_over_a_sub_range_reads_xnorm_and_leaves_it_alone(dev, name, chunk):
    from ital_amd import _lib
    lib, dtype = _lib.lib(), NARROW[name]
    n, d, r0, k = 257, 65, 16, 150
    vals = _values(n, d, dtype, 5)
    Xc, Xf, xn, ldx = _rows(vals, dev)
    gp = _fitted_gp(vals, dev, 40)
    m = gp.m
    assert m > 32
    ldv = _pad16(k)
    out = []
    for X, xtype in ((Xf, 0), (Xc, CODES[dtype])):
        V = torch.full((gp.cap, ldv), float("nan"), dtype=torch.float64, device=dev)
        mu, s2 = (torch.full((k,), float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
        # FP64: the call writes the norms (they start as NaN); typed: they are the store's, an input
        norms = torch.full((k,), float("nan"), dtype=torch.float64, device=dev) if xtype == 0 else xn[r0:r0 + k].clone()
        r = _lib.ItalRewhitenDesc()
        r.X, r.n_rows, r.ldx = X.data_ptr() + X.element_size() * r0 * ldx, k, ldx
        r.XT, r.XTn, r.L, r.ldl, r.alpha, r.m = gp.XT.data_ptr(), gp.XTn.data_ptr(), gp.L.data_ptr(), gp.cap, gp.alpha.data_ptr(), m
        r.var, r.length_scale = float(gp.var), float(gp.length_scale)
        r.xnorm, r.V, r.ldv, r.v_rows, r.mu, r.s2, r.chunk = norms.data_ptr(), V.data_ptr(), ldv, gp.cap, mu.data_ptr(), s2.data_ptr(), chunk
        if xtype == 0:
            _lib.check(lib.ital_whiten_rows(ctypes.byref(r), _stream()))
        else:
            _lib.check(lib.ital_whiten_rows_t(ctypes.byref(r), xtype, _stream()))
        out.append((V, mu, s2, norms))
    (Va, mua, s2a, na), (Vb, mub, s2b, nb) = out
    assert _same_bits(Va[:, :k], Vb[:, :k]) and _same_bits(mua, mub) and _same_bits(s2a, s2b)
    assert _same_bits(nb, xn[r0:r0 + k]) and _same_bits(na, nb)            # unchanged by the typed call; what the FP64 call wrote
    # and it is the model's own state on those rows: the sweep is DEFINED as the appends in blocks of 16 that built the model
    assert _same_bits(Va[:m, :k], gp.V[:m, r0:r0 + k]) and _same_bits(mua, gp.mu[r0:r0 + k])
    assert bool((Va[m:, :k].contiguous().view(torch.int64) == 0).all())


@pytest.mark.parametrize("name", list(NARROW))
def test_the_record_of_a_selection_carries_the_widened_row(dev, name):
    from ital_amd import _lib
    from ital_amd._batch import make_batch_buffers
    lib, dtype = _lib.lib(), NARROW[name]
    for n, d in ((17, 5), (65, 130)):
        Xc, Xf, xn, ldx = _rows(_values(n, d, dtype, 31 * n + d), dev)
        cap, m, ldv = 16, 3, _pad16(n)
        V, mu, s2, mi = _rand((cap, ldv), dev, 1), _rand((n,), dev, 2), _rand((n,), dev, 3).abs(), _rand((n,), dev, 4)
        mi[0] = 50.0                       # the winner: row 0 holds -0.0, the smallest subnormal and the largest magnitude
        cand = torch.arange(n, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        recs = []
        for X, xtype in ((Xf, None), (Xc, CODES[dtype])):
            b = make_batch_buffers(dev, 4, ldx, cap, ldv, 1)
            alive = torch.ones(n, dtype=torch.uint8, device=dev)
            head = (mi.data_ptr(), cand.data_ptr(), alive.data_ptr(), n, 0, None, 0, 0, 0, mu.data_ptr(), s2.data_ptr(), X.data_ptr(),
                    xn.data_ptr(), ldx, V.data_ptr(), ldv, m, cap, b["C"].data_ptr(), ldv, 0)
            tail = (0, b["batch"], status.data_ptr(), b["rec"].data_ptr(), b["ret"].data_ptr())
            if xtype is None:
                _lib.check(lib.ital_select_fused(*head, *tail, _stream()))
            else:
                _lib.check(lib.ital_select_fused_t(*head, *tail, xtype, _stream()))
            rec2 = torch.full_like(b["rec"], float("nan"))
            local = head[:-1] + (0, 4, status.data_ptr(), b["work"].data_ptr(), rec2.data_ptr())
            alive.fill_(1)
            if xtype is None:
                _lib.check(lib.ital_select_local(*local, _stream()))
            else:
                _lib.check(lib.ital_select_local_t(*local, xtype, _stream()))
            recs.append((b["rec"].clone(), b["XB"][0].clone(), int(b["ret"][0]), rec2))
        (ra, xa, wa, la), (rb, xb, wb, lb) = recs
        assert wa == wb == 0
        h = _lib.ITAL_REC_HEADER
        assert _same_bits(ra, rb) and _same_bits(xa, xb) and _same_bits(la, lb) and _same_bits(la, ra), (name, n, d)
        assert _same_bits(ra[h:h + ldx], Xf[0]) and _same_bits(xb, Xf[0])          # -0.0 keeps its sign in the record


@pytest.mark.parametrize("name", list(NARROW))
def test_gather_block_widens_while_it_copies(dev, name):
    from ital_amd import _lib
    lib, dtype = _lib.lib(), NARROW[name]
    for n, d in ((17, 5), (257, 130)):
        Xc, Xf, xn, ldx = _rows(_values(n, d, dtype, 13 * n + d), dev)
        m, ldv, row0 = 5, _pad16(n), 100
        V, mu, s2 = _rand((8, ldv), dev, 1), _rand((n,), dev, 2), _rand((n,), dev, 3)
        cand = torch.tensor([row0, row0 + n - 1, 3, row0 + n, row0 + n // 2, row0 + 1], dtype=torch.int64, device=dev)   # two are another rank's
        nc, ldc = len(cand), 16
        outs = []
        for X, xtype in ((Xf, None), (Xc, CODES[dtype])):
            Xg = torch.full((nc, ldx), float("nan"), dtype=torch.float64, device=dev)
            Vg = torch.full((m, ldc), float("nan"), dtype=torch.float64, device=dev)
            vec = torch.full((3, nc), float("nan"), dtype=torch.float64, device=dev)
            args = (cand.data_ptr(), nc, row0, n, X.data_ptr(), xn.data_ptr(), ldx, V.data_ptr(), ldv, m, mu.data_ptr(), s2.data_ptr(),
                    Xg.data_ptr(), Vg.data_ptr(), ldc, vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr())
            if xtype is None:
                _lib.check(lib.ital_gather_block(*args, _stream()))
            else:
                _lib.check(lib.ital_gather_block_t(*args, xtype, _stream()))
            outs.append((Xg, Vg[:, :nc], vec))
        for a, b in zip(*outs):
            assert _same_bits(a, b), (name, n, d)
        Xg, _, vec = outs[1]
        assert _same_bits(Xg[0], Xf[0]) and _same_bits(Xg[1], Xf[n - 1]) and bool((Xg[2].view(torch.int64) == 0).all())
        assert _same_bits(vec[0, :2], xn[[0, n - 1]]) and float(vec[0, 3]) == 0.0


# ------------------------------------------------------------------------------------------------ the ingest
def _source(layout, vals, dev):
    """The four source layouts of tests/test_gpu_device_data.py: (device view, element stride of its rows)."""
    n, d = vals.shape
    es = vals.element_size()
    if layout == "contiguous":
        return vals.to(dev), d
    if layout == "row_strided":
        buf = torch.zeros((n, d + 5), dtype=vals.dtype, device=dev)
        buf[:, :d] = vals.to(dev)
        return buf[:, :d], d + 5
    if layout == "offset_one":            # one element into an allocation: never on a 16-B boundary
        buf = torch.zeros(n * d + 1, dtype=vals.dtype, device=dev)
        t = buf[1:].view(n, d)
        t.copy_(vals.to(dev))
        assert t.data_ptr() % 16 != 0 and t.data_ptr() % es == 0
        return t, d
    ld = _pad16(d) + 16                   # aligned16: pointer and row stride multiples of 16 B
    buf = torch.zeros((n, ld), dtype=vals.dtype, device=dev)
    buf[:, :d] = vals.to(dev)
    assert buf.data_ptr() % 16 == 0 and (ld * es) % 16 == 0
    return buf[:, :d], ld


@pytest.mark.parametrize("layout", ["contiguous", "row_strided", "offset_one", "aligned16"])
@pytest.mark.parametrize("name", ["f64", "f32", "f16", "bf16"])
def test_compact_ingest_keeps_the_bits_pads_with_plus_zero_and_gives_the_fp64_norms(dev, name, layout):
    from ital_amd import _lib
    lib = _lib.lib()
    dtype = torch.float64 if name == "f64" else NARROW[name]
    nan = float("nan")
    scratch = torch.full((7, 144), nan, dtype=torch.float64, device=dev)            # 7 rows at a time: several blocks
    for n in (1, 63, 64, 65, 257):
        for d in (1, 3, 4, 5, 15, 16, 17, 130):
            vals = _values(n, d, dtype, 1000 * n + d)
            src, ld = _source(layout, vals, dev)
            ldx = _pad16(d)
            X = torch.full((n + 3, ldx), nan, dtype=dtype, device=dev)
            xnorm = torch.full((n + 3,), nan, dtype=torch.float64, device=dev)
            _lib.check(lib.ital_ingest_rows_t(src.data_ptr(), CODES[dtype], n, d, ld, X.data_ptr(), ldx, xnorm.data_ptr(),
                                              scratch.data_ptr(), 7, _stream()))
            what = (name, layout, n, d)
            assert _same_bits(X[:n, :d], vals.to(dev)), what                                   # also the sign of -0.0
            assert bool((X[:n, d:].contiguous().view(BITS[dtype]) == 0).all()), what           # pad columns: +0 by their bits
            assert bool(torch.isnan(X[n:]).all()) and bool(torch.isnan(xnorm[n:]).all()), what  # rows >= n: not touched
            Xf = X[:n].to(torch.float64)
            norms = torch.empty(n, dtype=torch.float64, device=dev)
            _lib.check(lib.ital_row_norms(Xf.data_ptr(), n, ldx, norms.data_ptr(), _stream()))
            assert _same_bits(xnorm[:n], norms) and bool(torch.isfinite(norms).all()), what


def test_device_data_source_storage(dev):
    from ital_amd import DeviceData
    A = np.random.default_rng(3).standard_normal((257, 140)).astype(np.float32)
    T = torch.from_numpy(A)
    for dt in (torch.float32, torch.float16, torch.bfloat16, torch.float64):
        t = T.to(dt)
        wide = DeviceData(t, device=dev)
        assert wide.storage is torch.float64 and DeviceData(t, device=dev, storage="f64").X.dtype is torch.float64
        for src in (t, t.to(dev), t.to(dev)[:, 3:131]):
            for chunk in (256 << 20, 3000):
                s = DeviceData(src, device=dev, storage="source", chunk_bytes=chunk)
                w = wide if src.shape[1] == 140 else DeviceData(src, device=dev)
                assert s.storage is dt and s.X.dtype is dt and s.X.shape == w.X.shape and s.X.is_contiguous() and s.xnorm.dtype is torch.float64
                assert _same_bits(s.X.to(torch.float64), w.X) and _same_bits(s.xnorm, w.xnorm)
                assert s.rows().dtype == np.float64 and np.array_equal(s.rows(), w.rows())
                assert np.array_equal(s.rows([5, 0, -1]), w.rows([5, 0, -1]))
    assert DeviceData(A, device=dev, storage="source").storage is torch.float32                 # numpy sources too
    assert DeviceData(A.astype(np.int32), device=dev, storage="source").storage is torch.float64
    # append: rows of the store's type, in place and by a device-to-device reallocation in that type
    h = T.to(torch.float16)
    c = DeviceData(h[:200], device=dev, storage="source", capacity=230)
    ptr = c.X.data_ptr()
    assert c.append(h[200:230].to(dev)) == 30 and c.X.data_ptr() == ptr
    before = (c.n, c.capacity, c.X.data_ptr(), c.X.clone(), c.xnorm.clone())
    for other in (T[230:], T[230:].to(torch.bfloat16), A[230:].astype(np.float64)):
        with pytest.raises(TypeError, match="float16"):
            c.append(other)
    with pytest.raises(ValueError):
        c.append(h[:3, :7])
    assert before[:3] == (c.n, c.capacity, c.X.data_ptr()) and _same_bits(before[3], c.X) and _same_bits(before[4], c.xnorm)
    assert c.append(A[230:].astype(np.float16)) == 27 and c.X.data_ptr() != ptr and c.capacity == 460 and c.X.dtype is torch.float16
    full = DeviceData(h, device=dev)
    assert _same_bits(c.X.to(torch.float64), full.X) and _same_bits(c.xnorm, full.xnorm)
    with pytest.raises(ValueError, match="storage"):
        DeviceData(h, device=dev, storage="f16")


def test_memory_of_a_compact_store(dev):
    from ital_amd import DeviceData
    n, d, ldx = 4096, 256, 256
    t = torch.from_numpy(np.random.default_rng(9).standard_normal((n, d)).astype(np.float16))
    own = n * ldx * 2 + n * 8
    chunk = 1 << 20
    for src in (t, t.to(dev)):
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        s = DeviceData(src, device=dev, storage="source", chunk_bytes=chunk)
        torch.cuda.synchronize()
        grown = torch.cuda.memory_allocated(dev) - before
        peak = torch.cuda.max_memory_allocated(dev) - before
        print("compact store: %d B (rows and norms: %d B), peak during construction %d B" % (grown, own, peak))
        assert 0 < grown <= own + (1 << 20), grown
        # the chunk is chunk_bytes of f16 rows on their way in; its FP64 expansion is four times that
        assert peak <= own + 4 * chunk + (2 << 20), peak
        assert peak < n * ldx * 8                      # the full FP64 matrix never existed
        del s


# ------------------------------------------------------------------------------------------------ learners
def _snap(L):
    gp = L.gp
    m = gp.m
    return dict(m=m, ind=list(gp.ind), y=None if gp.y is None else gp.y.copy(), mu=gp.mu.clone(), s2=gp.s2.clone(),
                V=gp.V[:m].clone(), L=gp.L[:m, :m].clone(), alpha=gp.alpha[:m].clone(), xnorm=gp.xnorm.clone())


def _same_snap(a, b, what):
    assert a["m"] == b["m"] and a["ind"] == b["ind"] and np.array_equal(a["y"], b["y"]), what
    for key in ("mu", "s2", "V", "L", "alpha", "xnorm"):
        assert _same_bits(a[key], b[key]), (what, key)


def _same_logs(a, b):
    assert len(a) == len(b)
    for at, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, dict):
            _same_snap(x, y, at)
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), at
        else:
            assert x == y, (at, x, y)


def _reset_streams(seed=0):
    from ital_amd import mvn_stream
    mvn_stream.GLOBAL.reset()
    np.random.seed(seed)


def _golden_log(name, z, data, dev):
    """The fixture's session on `data`: picks and the model's state after every round."""
    import ital_amd
    cls = getattr(ital_amd, make_golden.FIXTURES[name]["learner"])
    _reset_streams()
    L = cls(data, length_scale=float(z["length_scale"]), device=dev, **make_golden.FIXTURES[name]["kw"])
    L.update({int(z["query"]): 1})
    log = [_snap(L)]
    for r in range(int(z["rounds"])):
        ret = L.fetch_unlabelled(int(z["k"]))
        L.update({int(i): float(z["rel"][i]) for i in ret})
        log += [list(ret), _snap(L)]
    return L, log


@pytest.mark.parametrize("name", list(NARROW))
@pytest.mark.parametrize("fixture", ["usps500", "usps500_mcmi"])
def test_the_golden_sessions_on_a_compact_store(dev, golden_dir, fixture, name):
    from ital_amd import DeviceData
    z = np.load(os.path.join(golden_dir, fixture + ".npz"))
    t = torch.from_numpy(z["X"]).to(NARROW[name])           # the golden matrix rounded to the type first
    C, got = _golden_log(fixture, z, DeviceData(t, device=dev, storage="source"), dev)
    W, want = _golden_log(fixture, z, DeviceData(t, device=dev), dev)
    assert C.gp.Xd.dtype is NARROW[name] and C.gp.xtype == CODES[NARROW[name]] and W.gp.xtype == 0
    assert C.gp.Xd.data_ptr() == C.data.X.data_ptr()
    _same_logs(got, want)
    assert len(got) == 1 + 2 * int(z["rounds"]) and _same_bits(C.gp.Xd.to(torch.float64), W.gp.Xd)


def _truth(X, i):
    return 1 if X[i, 0] > 0.5 else -1


def _two_rounds(L, X, k, log, rounds=2):
    for r in range(rounds):
        _reset_streams(4 + r)
        got = L.fetch_unlabelled(k)
        L.update({int(i): _truth(X, int(i)) for i in got})
        log += [[int(i) for i in got], _snap(L)]


def _pair(t, dev, **kw):
    from ital_amd import DeviceData
    return (DeviceData(t, device=dev, storage="source", **kw), DeviceData(t, device=dev, **kw))


def _small(name, n=60, d=5, seed=17):
    X = np.random.default_rng(seed).random((n, d))
    t = torch.from_numpy(X).to(NARROW[name])
    return t, t.to(torch.float64).numpy()


def _make(kind, store, ls, dev):
    import ital_amd
    from ital_amd import baselines
    if kind == "noisy_user":
        return ital_amd.ITAL(store, length_scale=ls, device=dev, label_prob=0.8, mistake_prob=0.1)
    if kind == "top_candidates":
        return ital_amd.ITAL(store, length_scale=ls, device=dev, top_candidates=30)
    if kind == "steps":
        L = ital_amd.ITAL(store, length_scale=ls, device=dev)
        L.round_call = False
        return L
    if kind == "adapt":
        return ital_amd.AdaptAL(store, length_scale=ls, device=dev, subsample=40)
    if kind == "var_corr":
        return baselines.VarianceSampling(store, length_scale=ls, device=dev, use_correlations=True)
    return baselines.LEARNERS[kind](store, length_scale=ls, device=dev)


@pytest.mark.parametrize("name", list(NARROW))
@pytest.mark.parametrize("kind", ["noisy_user", "top_candidates", "steps", "adapt", "border_div", "var_corr", "entropy"])
def test_learners_on_a_compact_store_pick_and_hold_what_they_do_on_the_fp64_store(dev, kind, name):
    t, X = _small(name)
    ls = float(np.sqrt(5 / 12.0))
    logs = []
    for store in _pair(t, dev):
        L = _make(kind, store, ls, dev)
        L.update({3: 1, 11: -1, 40: 1, 50: -1})
        log = [_snap(L)]
        _two_rounds(L, X, 3, log)
        logs.append(log)
    _same_logs(*logs)
    assert len(set(logs[0][1])) == 3 and logs[0][2]["m"] == 7


@pytest.mark.parametrize("name", list(NARROW))
def test_a_live_session_on_a_compact_store(dev, name):
    """revoke / relabel, set_params, tune_params, clone, a state_dict round trip, predict_stored / top_results / predict."""
    import ital_amd
    t, X = _small(name, n=90)
    ls = float(np.sqrt(5 / 12.0))
    logs = []
    for store in _pair(t, dev):
        L = ital_amd.ITAL(store, length_scale=ls, device=dev)
        L.update({3: 1, 11: -1, 40: 1, 50: -1})
        log = [_snap(L)]
        _two_rounds(L, X, 4, log, rounds=1)
        L.revoke([log[-2][1]])
        log.append(_snap(L))
        L.relabel({11: 1})
        log.append(_snap(L))
        L.set_params(length_scale=1.3 * ls, noise=1e-4)
        log.append(_snap(L))
        best, score = L.tune_params(grid={"length_scale": [0.5 * ls, ls, 2 * ls]})
        log += [sorted(best.items()), float(score), _snap(L)]
        twin = L.clone()
        assert twin.gp.Xd.data_ptr() == L.gp.Xd.data_ptr() and twin.gp.xtype == L.gp.xtype
        log.append(_snap(twin))
        _two_rounds(twin, X, 4, log, rounds=1)
        _two_rounds(L, X, 4, log, rounds=1)
        mean, var = L.gp.predict_stored(cov_mode="diag")
        m2, cov = L.gp.predict_stored([0, 5, 17], cov_mode="full")
        log += [mean, var, m2, cov, L.top_results(5), L.top_results(), np.asarray(L.rel_mean), L.gp.rbf_cols([0, 7]).cpu().numpy()]
        log += list(L.gp.predict(X[:9] + 0.01, cov_mode="diag"))
        sd = L.state_dict()
        R = ital_amd.ITAL(store, length_scale=L.length_scale, var=L.var, noise=L.noise, device=dev).load_state_dict(sd)
        log.append(_snap(R))
        _two_rounds(R, X, 4, log, rounds=1)
        logs.append(log)
    _same_logs(*logs)


@pytest.mark.parametrize("spare", [0, 64], ids=["reallocates", "in_place"])
@pytest.mark.parametrize("name", list(NARROW))
@pytest.mark.parametrize("cls_name", ["ITAL", "MCMI_min"])
def test_growth_of_a_compact_store_reaches_the_learner_that_syncs(dev, cls_name, name, spare):
    import ital_amd
    cls = getattr(ital_amd, cls_name)
    kw = dict(subsample=60) if cls_name == "MCMI_min" else {}
    t, X = _small(name, n=120, d=6)
    ls = float(np.sqrt(6 / 12.0))
    logs = []
    for store in _pair(t[:90], dev, capacity=90 + spare):
        A, B = cls(store, length_scale=ls, device=dev, **kw), cls(store, length_scale=ls, device=dev, **kw)
        log = []
        for L in (A, B):
            L.update({3: 1, 11: -1, 40: 1, 77: -1})
            _two_rounds(L, X, 4, log, rounds=1)
        ptr = store.X.data_ptr()
        assert store.append(t[90:]) == 30 and (store.X.data_ptr() == ptr) == (spare > 0) and store.X.dtype is store.storage
        assert A.sync_data() == 30 and A.gp.n == 120 and A.gp.Xd.data_ptr() == store.X.data_ptr()
        log.append(_snap(A))
        # B has not synced: it stays on its prefix, also across the reallocation
        assert B.gp.n == 90 and B.gp.Xd.shape[0] == 90 and (B.gp.Xd.data_ptr() == store.X.data_ptr()) == (spare > 0)
        _two_rounds(A, X, 4, log, rounds=1)
        _two_rounds(B, X, 4, log, rounds=1)
        assert max(log[-2]) < 90 and A.add_data(t[:5].to(dev)) is A and A.gp.n == 125 and B.gp.n == 90
        log.append(_snap(A))
        logs.append(log)
    _same_logs(*logs)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_on_a_compact_store_name_it_and_change_nothing(dev):
    from ital_amd import ITAL, DeviceData, GaussianProcess, baselines
    t, X = _small("f16")
    store = DeviceData(t, device=dev, storage="source")
    rows, norms = store.X.clone(), store.xnorm.clone()
    E = baselines.EMOC(store, length_scale=0.6, device=dev)
    E.update({3: 1, 9: -1})
    before, rounds = _snap(E), E.rounds
    with pytest.raises(NotImplementedError, match="compact store"):
        E.fetch_unlabelled(3)
    _same_snap(_snap(E), before, "EMOC")
    assert E.rounds == rounds and E.get_unseen() == [i for i in range(60) if i not in (3, 9)]
    for make in (lambda: GaussianProcess(store, 0.6, device=dev, rank=0, world=2),
                 lambda: ITAL(store, length_scale=0.6, device=dev, rank=1, world=2)):
        with pytest.raises(NotImplementedError, match="compact store"):
            make()
    assert _same_bits(store.X, rows) and _same_bits(store.xnorm, norms) and len(store) == 60
    # the FP64 store still answers EMOC
    W = baselines.EMOC(DeviceData(t, device=dev), length_scale=0.6, device=dev)
    W.update({3: 1, 9: -1})
    assert len(W.fetch_unlabelled(3)) == 3
