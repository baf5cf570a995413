"""The dense tune kernels, one call each, against the extended-precision reference of tests/_dense_ref.py.

ital_gram_rows, ital_chol_batched, ital_chol_solve_batched and ital_kernel_matvec (include/ital_dense.h, csrc/dense.hip) are
called through ctypes on buffers built on the host.  Every byte a call must not read, and every byte it must not write, holds
NaN: the padding columns and rows past n, the strict upper triangle of every matrix handed to the factor and to the solves,
W's columns F .. ldw - 1, out's columns F .. ldo - 1, the rows past na / nb of the feature rows and their norms, the workspace
past ital_kernel_matvec_workspace (an index past n[b] of a Gram's idx points at a NaN row).  Afterwards everything outside the
documented write set is compared by its bits with what was uploaded, and every output is finite.  Leading dimensions are
strictly larger than n, not multiples of 16, and each matrix of a batch has its own.  The results are judged by the
componentwise bounds of _dense_ref.py (a-priori operation counts; nothing is fitted): largest residual / bound <= 1.  The host
side -- that a plain FP64 emulation passes the same bounds at the same shapes and that the checker rejects the mistakes these
kernels could make -- is tests/test_dense_ref_host.py.

The Grams are those of near-flat kernels over rows of the unit cube (`uniform`, noise 1e-3) and over rows every third of
which repeats its predecessor to 1e-6 (`neardup`, noise 1e-6): condition numbers up to 3e5 and 2e7 to 3e8 at n = 129 and 321,
three decades past the 1e5 that the evidence tests allow.  The factor runs on the device's own Gram and the solves on the
device's own factor, so the chain Gram -> factor -> solve runs unbroken, as the evidence prologue runs it, and each kernel is
still judged on its own input.

Largest residual / bound observed (MI355X / FP64 NumPy emulation on the host), printed again by every run with -s:

    quantity                      data      device    emulation
    ital_gram_rows                uniform   0.161     0.153
    ital_gram_rows                neardup   0.127     0.142
    ital_chol_batched             uniform   0.157     0.494
    ital_chol_batched             neardup   0.306     0.421
    ital_chol_batched             host      0.180     0.180
    ital_chol_solve_batched +-1   uniform   0.062     0.084
    ital_chol_solve_batched +-1   neardup   0.128     0.062
    ital_chol_solve_batched +-1   host      0.008     0.048
    ital_chol_solve_batched 1e+-3 uniform   0.159     0.097
    ital_chol_solve_batched 1e+-3 neardup   0.176     0.176
    ital_chol_solve_batched 1e+-3 host      0.126     0.126
    ital_kernel_matvec            small     0.072     0.042
    ital_kernel_matvec            loop      0.00027   0.00015
    ital_kernel_matvec vs emu     loop      0.00020   -

(The mixed batches, which have no emulation: Gram 0.119, factor 0.351.  The loop shapes sum 4224 and 8250 terms of mixed
signs; the bound grows with the number of terms, the error like its root.  `vs emu` is device against emulation at twice the
bound, over all of out.)  The device sits where the emulation does; the accuracy of the device exp in the Gram epilogue, which
nothing else in the repository measures, stays inside the 1 ulp that dK allows it (Gram ratio 0.16 at most).  No test failed
and dense.hip is unchanged.

The production loop of kernel_w_kernel: at (4000, 4224) and (4001, 8250) a workgroup walks 2 and 3 tiles of b
(_dense_ref.expected_split, a host copy of kw_split, asserted here), which no other kernel-level test reaches.

Read, not measured: chol_diag_kernel and chol_trsm_kernel stage only c <= r of a block, chol_syrk_kernel's clamped rows past n
re-read row n - 1 of the panel (inside the matrix), and kernel_w_kernel reads W only under j < jend && col < F: the NaN guards
confirm all of it.  A NaN at a strictly lower entry (r, c) is first seen by the pivot of row r (info == r + 1): column c's
own pivot does not depend on row r.  In that case row r carries NaN from column c on, also in columns before the failing block;
every other row is clean there.  Two remarks on the caller's side of the contract, not exercised here: with max_n <= 0
ital_chol_batched returns before it writes info, and a max_n smaller than some n[b] leaves that matrix factored only up to
max_n rounded up to 64 columns, with info[b] == 0 (tune.py, evidence.hip and adapt_al.py pass the true maximum).

Run: python -m pytest tests/test_gpu_dense_kernels.py -m gpu -s."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _dense_ref as ref  # noqa: E402

NAN = float("nan")
WORST = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (entry, kind, name), (d, e) in sorted(WORST.items()):
        print("%-20s %-8s %-7s largest residual/bound: device %.3g, emulation %.3g" % (entry, kind, name, d, e))


def _note(entry, kind, ratios, emulated=None):
    """Device ratios and, where the same inputs went through the FP64 emulation, its ratios beside them."""
    emulated = emulated or {}
    for name, r in ratios.items():
        key = (entry, kind, name)
        d, e = WORST.get(key, (0.0, 0.0))
        WORST[key] = (max(d, r), max(e, emulated.get(name, 0.0)))
    print(entry, kind, "device", {k: "%.3g" % v for k, v in ratios.items()},
          "emulation", {k: "%.3g" % v for k, v in emulated.items()})


def _lib():
    from ital_amd import _lib
    return _lib.lib(), _lib.check


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _down(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(before, after, written=None):
    """Everything outside the boolean mask `written` has the bits it was uploaded with."""
    keep = np.ones(before.shape, dtype=bool) if written is None else ~written
    return bool(np.array_equal(_bits(before)[keep], _bits(after)[keep]))


def _lower_mask(shape, n):
    w = np.zeros(shape, dtype=bool)
    w[:n, :n] = np.tri(n, dtype=bool)
    return w


def _ld(n, b=0):
    """A leading dimension strictly greater than n that is no multiple of 16; matrix b of a batch gets its own."""
    ld = n + 3 + 2 * b
    while ld % 16 == 0:
        ld += 1
    return ld


def _ptrs(tensors, dev):
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64, device=dev)


def _ints(values, dtype, dev):
    return torch.tensor(list(values), dtype=dtype, device=dev)


def _id(case):
    return "-".join(str(v) for v in case)


def _rows(dev, X, guard=2):
    """Feature rows followed by `guard` rows of NaN, and their squared norms by ital_row_norms (what the library hands to
    these kernels) with NaN behind.  Returns (host rows, device rows, device norms, host norms)."""
    lib, check = _lib()
    host = np.full((X.shape[0] + guard, X.shape[1]), NAN)
    host[:X.shape[0]] = X
    Xd = _up(host, dev)
    xn = torch.full((host.shape[0],), NAN, dtype=torch.float64, device=dev)
    check(lib.ital_row_norms(Xd.data_ptr(), X.shape[0], X.shape[1], xn.data_ptr(), _stream()))
    return host, Xd, xn, _down(xn)


# ------------------------------------------------------------------------------------------------ the three batched calls
def _gram_call(dev, s, idxs, ns, max_n, first_b=0):
    """One ital_gram_rows over the rows of case `s`: matrix b takes the first ns[b] entries of idxs[b].  Every index past
    ns[b] points at the first NaN row.  Returns the device matrices and their host copies after the call."""
    lib, check = _lib()
    X0, Xd, xn, xn0 = _rows(dev, s.X)
    poison = s.X.shape[0]
    idx0 = []
    for idx, n in zip(idxs, ns):
        full = np.full(len(idx) + 2, poison, dtype=np.int64)
        full[:n] = idx[:n]
        idx0.append(full)
    idxd = [_up(i, dev) for i in idx0]
    K0 = [np.full((n + 2, _ld(n, first_b + b)), NAN) for b, n in enumerate(ns)]
    Kd = [_up(k, dev) for k in K0]
    ip, kp = _ptrs(idxd, dev), _ptrs(Kd, dev)
    nd, ldd = _ints(ns, torch.int32, dev), _ints((k.shape[1] for k in K0), torch.int64, dev)
    check(lib.ital_gram_rows(Xd.data_ptr(), xn.data_ptr(), s.ldx, ip.data_ptr(), nd.data_ptr(), kp.data_ptr(), ldd.data_ptr(),
                             len(ns), max_n, float(s.var), float(s.ls), float(s.noise), _stream()))
    K1 = [_down(k) for k in Kd]
    for n, k0, k1 in zip(ns, K0, K1):
        assert _same(k0, k1, _lower_mask(k0.shape, n)), ("ital_gram_rows wrote outside the lower triangle", n)
        assert np.isfinite(k1[:n, :n][np.tril_indices(n)]).all(), n
    assert _same(X0, _down(Xd)) and _same(xn0, _down(xn))
    for i0, i1 in zip(idx0, idxd):
        assert np.array_equal(i0, _down(i1))
    return Kd, K1


def _chol_call(dev, Ad, ns, max_n, status0=0):
    """ital_chol_batched in place on the device matrices Ad.  Returns (host copies after, info, status); asserts that nothing
    outside the lower triangles changed, that info's guard entry did not, and that sizes and leading dimensions did not."""
    lib, check = _lib()
    A0 = [_down(a) for a in Ad]
    ap = _ptrs(Ad, dev)
    nd, ldd = _ints(ns, torch.int32, dev), _ints((a.shape[1] for a in Ad), torch.int64, dev)
    info = torch.full((len(ns) + 1,), -5, dtype=torch.int32, device=dev)
    status = torch.full((2,), status0, dtype=torch.int32, device=dev)
    check(lib.ital_chol_batched(ap.data_ptr(), nd.data_ptr(), ldd.data_ptr(), len(ns), max_n, info.data_ptr(),
                                status.data_ptr(), _stream()))
    A1 = [_down(a) for a in Ad]
    for n, a0, a1 in zip(ns, A0, A1):
        assert _same(a0, a1, _lower_mask(a0.shape, n)), ("ital_chol_batched wrote outside the lower triangle", n)
    info_h, status_h = _down(info), _down(status)
    assert info_h[-1] == -5 and status_h[1] == status0
    assert np.array_equal(_down(nd), np.asarray(ns, dtype=np.int32))
    return A1, info_h[:-1], int(status_h[0])


def _solve_call(dev, Ld, ns, ys, info):
    """ital_chol_solve_batched: ys[b] is the right-hand side of matrix b (n[b] entries, two NaN behind them on the device).
    info: an int32 array or None (NULL).  Returns the vectors after the call; asserts that the factors and the guards kept
    their bits."""
    lib, check = _lib()
    L0 = [_down(a) for a in Ld]
    y0 = []
    for n, y in zip(ns, ys):
        full = np.full(n + 2, NAN)
        full[:n] = y[:n]
        y0.append(full)
    yd = [_up(y, dev) for y in y0]
    lp, yp = _ptrs(Ld, dev), _ptrs(yd, dev)
    nd, ldd = _ints(ns, torch.int32, dev), _ints((a.shape[1] for a in Ld), torch.int64, dev)
    infod = None if info is None else _up(np.asarray(info, dtype=np.int32), dev)
    check(lib.ital_chol_solve_batched(lp.data_ptr(), nd.data_ptr(), ldd.data_ptr(), yp.data_ptr(), len(ns),
                                      None if infod is None else infod.data_ptr(), _stream()))
    y1 = [_down(y) for y in yd]
    for a0, a in zip(L0, Ld):
        assert _same(a0, _down(a)), "ital_chol_solve_batched wrote to a factor"
    for n, a, b in zip(ns, y0, y1):
        assert _same(a[n:], b[n:])
    if infod is not None:
        assert np.array_equal(_down(infod), np.asarray(info, dtype=np.int32))
    return y0, y1


def _guarded_dev(dev, A, b=0):
    n = A.shape[0]
    return _up(ref.guarded(ref.lower_nan(A), _ld(n, b)), dev)


def _solve_ratios(dev, Ld, L1, n, pair):
    out = {}
    for name, y in zip(("solve", "solve6"), pair):
        _, y1 = _solve_call(dev, [Ld], [n], [y], [0])
        assert np.isfinite(y1[0][:n]).all()
        out[name] = ref.check_solve(L1, y1[0], y, n)
    return out


# ------------------------------------------------------------------------------------------------ Gram -> factor -> solve
@pytest.mark.parametrize("case", ref.GRAM_CASES, ids=_id)
def test_the_chain_gram_factor_solve_against_the_extended_reference(dev, case):
    s = ref.gram_case(*case)
    n = s.n
    Kref, dK = ref.gram_ref(*case)
    Kd, K1 = _gram_call(dev, s, [s.idx], [n], n)
    ratios = dict(gram=ref.check_gram(K1[0], Kref, dK, s.noise))
    L1, info, status = _chol_call(dev, Kd, [n], n)
    assert info[0] == 0 and status == 0
    ratios["factor"] = ref.check_factor(L1[0], K1[0], n)
    ratios.update(_solve_ratios(dev, Kd[0], L1[0], n, (s.y, s.y_wide)))
    _note("chain", s.kind, ratios, ref.emu_chain(s, Kref, dK))
    assert max(ratios.values()) <= 1.0, (case, ratios)


@pytest.mark.parametrize("n", ref.SIZES)
def test_the_factor_and_the_solves_on_host_built_matrices(dev, n):
    A = ref.host_spd(n)
    Ad = _guarded_dev(dev, A)
    L1, info, status = _chol_call(dev, [Ad], [n], n)
    assert info[0] == 0 and status == 0
    ratios = dict(factor=ref.check_factor(L1[0], A, n))
    ratios.update(_solve_ratios(dev, Ad, L1[0], n, ref.rhs(n)))
    _note("chol+solve", "host", ratios, ref.emu_factor_solve(A, ref.rhs(n)))
    assert max(ratios.values()) <= 1.0, (n, ratios)


def _batch_idx(s):
    rng = np.random.default_rng(99)
    return [rng.permutation(s.X.shape[0]).astype(np.int64) for _ in ref.BATCH_SIZES]


def test_a_mixed_gram_batch_gives_each_matrix_the_bits_it_gets_alone(dev):
    """Sizes 65, 0, 129, 1, 64, 193 over one row set, max_n = 200 larger than all of them."""
    s = ref.gram_case("neardup", 16, 1.2, 193)
    ns, idxs = list(ref.BATCH_SIZES), _batch_idx(s)
    assert 0 in ns and ref.BATCH_MAX_N > max(ns) and ref.BATCH_MAX_N <= s.X.shape[0]
    _, batch = _gram_call(dev, s, idxs, ns, ref.BATCH_MAX_N)
    worst = 0.0
    for b, (n, idx) in enumerate(zip(ns, idxs)):
        _, alone = _gram_call(dev, s, [idx], [n], max(n, 1), first_b=b)
        assert _same(alone[0], batch[b]), ("matrix %d of the batch differs from the single call" % b, n)
        if n:
            R = s.X[idx[:n]]
            Kref, dK = ref.kernel_ref(R, R, s.var, s.ls)
            worst = max(worst, ref.check_gram(batch[b], Kref, dK, s.noise))
    _note("gram batch", s.kind, dict(gram=worst))
    assert worst <= 1.0


def test_a_mixed_cholesky_batch_equals_the_single_calls_bit_for_bit(dev):
    ns = list(ref.BATCH_SIZES)
    mats = [ref.host_spd(n, seed=b) if n else np.zeros((0, 0)) for b, n in enumerate(ns)]
    batch, info, status = _chol_call(dev, [_guarded_dev(dev, A, b) for b, A in enumerate(mats)], ns, ref.BATCH_MAX_N, status0=6)
    assert status == 6 and (info == 0).all()
    worst = 0.0
    for b, (n, A) in enumerate(zip(ns, mats)):
        if n:
            alone, info1, _ = _chol_call(dev, [_guarded_dev(dev, A, b)], [n], n)
            assert info1[0] == 0 and _same(alone[0], batch[b]), ("matrix %d of the batch differs from the single call" % b, n)
            worst = max(worst, ref.check_factor(batch[b], A, n))
    _note("chol batch", "host", dict(factor=worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ failure paths
FAIL_N = 200
FAIL_BATCH = (70, FAIL_N, 129, 0)            # the failed matrix is matrix 1, between two sound ones and an empty one


def _failure_batch(dev, bad):
    mats = [ref.host_spd(70, seed=1), bad, ref.host_spd(129, seed=2), np.zeros((0, 0))]
    Ad = [_guarded_dev(dev, A, b) for b, A in enumerate(mats)]
    A1, info, status = _chol_call(dev, Ad, list(FAIL_BATCH), FAIL_N, status0=6)
    for b in (0, 2):
        assert info[b] == 0
        assert ref.check_factor(A1[b], mats[b], FAIL_BATCH[b]) <= 1.0
    assert info[3] == 0 and status == 7
    return mats, Ad, A1, info


@pytest.mark.parametrize("j", [0, 63, 64, 65, 127, 128, 199])
def test_a_pivot_that_is_not_positive_is_reported_by_its_column(dev, j):
    bad = ref.host_spd(FAIL_N)
    bad[j, j] = -1.0
    mats, Ad, A1, info = _failure_batch(dev, bad)
    assert info[1] == j + 1
    k0 = j // 64 * 64
    got = A1[1]
    assert ref.check_factor(got, bad, FAIL_N, ncols=k0) <= 1.0          # the columns before the failing block: a leading factor
    assert not np.isnan(got[:FAIL_N, :k0][np.tril_indices(FAIL_N, 0, k0)]).any()
    # the solves skip the failed matrix, solve the sound ones and skip the empty one
    ys = [ref.rhs(n, seed=5)[1] for n in FAIL_BATCH]
    y0, y1 = _solve_call(dev, Ad, list(FAIL_BATCH), ys, info)
    assert _same(y0[1], y1[1]), "the right-hand side of the failed matrix changed"
    for b in (0, 2):
        assert ref.check_solve(A1[b], y1[b], ys[b], FAIL_BATCH[b]) <= 1.0


@pytest.mark.parametrize("r,c", [(64, 0), (70, 66), (130, 3), (199, 198)])
def test_a_nan_below_the_diagonal_is_reported_by_its_row(dev, r, c):
    bad = ref.host_spd(FAIL_N)
    bad[r, c] = NAN
    mats, Ad, A1, info = _failure_batch(dev, bad)
    assert info[1] == r + 1
    k0 = r // 64 * 64
    got, clean = A1[1].copy(), bad.copy()
    assert not np.isnan(np.delete(got[:FAIL_N, :k0], r, axis=0)[np.tril_indices(FAIL_N - 1, 0, k0)]).any()
    assert not np.isnan(got[r, :min(c, k0)]).any()
    got[r, :FAIL_N], clean[r, :FAIL_N] = 0.0, 0.0                       # row r is tainted from column c on: judged without it
    assert ref.check_factor(got, clean, FAIL_N, ncols=k0) <= 1.0


def test_the_solves_without_info_solve_every_matrix_and_skip_an_empty_one(dev):
    ns = [70, 0, 129]
    mats = [ref.host_spd(70, seed=1), np.zeros((0, 0)), ref.host_spd(129, seed=2)]
    Ad = [_guarded_dev(dev, A, b) for b, A in enumerate(mats)]
    A1, info, status = _chol_call(dev, Ad, ns, 129)
    assert (info == 0).all() and status == 0
    ys = [ref.rhs(n, seed=6)[1] for n in ns]
    y0, y1 = _solve_call(dev, Ad, ns, ys, None)
    assert _same(y0[1], y1[1])
    for b in (0, 2):
        assert ref.check_solve(A1[b], y1[b], ys[b], ns[b]) <= 1.0
    # and with an info that marks matrix 2 as failed, only matrix 0 is solved
    y0, y1 = _solve_call(dev, Ad, ns, ys, [0, 0, 3])
    assert _same(y0[2], y1[2]) and ref.check_solve(A1[0], y1[0], ys[0], 70) <= 1.0


# ------------------------------------------------------------------------------------------------ ital_kernel_matvec
def _matvec_call(dev, s, ldw=None, ldo=None, F=None, ldx=None, nb=None, short=0, refuse=None):
    """One ital_kernel_matvec on NaN-guarded buffers.  `refuse`: the call must return an error whose message holds this text
    and change nothing.  Returns out[na][F]."""
    from ital_amd import _lib
    lib = _lib.lib()
    F = s.F if F is None else F
    ldw = s.F + 3 if ldw is None else ldw
    ldo = s.F + 2 if ldo is None else ldo
    A0, Ad, an, an0 = _rows(dev, s.Xa)
    B0, Bd, bn, bn0 = _rows(dev, s.Xb)
    W0 = np.full((s.nb + 2, max(ldw, s.F + 3)), NAN)
    W0[:s.nb, :s.F] = s.W
    out0 = np.full((s.na + 2, max(ldo, s.F + 2)), NAN)
    wl = int(lib.ital_kernel_matvec_workspace(s.na, s.nb))
    assert wl == ref.expected_workspace(s.na, s.nb)
    work0 = np.full(wl + 64, NAN)
    Wd, outd, workd = _up(W0, dev), _up(out0, dev), _up(work0, dev)
    rc = lib.ital_kernel_matvec(Ad.data_ptr(), an.data_ptr(), s.na, Bd.data_ptr(), bn.data_ptr(), s.nb if nb is None else nb,
                                s.ldx if ldx is None else ldx, Wd.data_ptr(), ldw, F, float(s.var), float(s.ls),
                                outd.data_ptr(), ldo, workd.data_ptr(), wl - short, _stream())
    out1, work1 = _down(outd), _down(workd)
    assert _same(A0, _down(Ad)) and _same(B0, _down(Bd)) and _same(an0, _down(an)) and _same(bn0, _down(bn))
    assert _same(W0, _down(Wd))
    if refuse is not None:
        msg = lib.ital_last_error().decode()
        assert rc != 0 and "ital_kernel_matvec" in msg and refuse in msg, (rc, msg)
        assert _same(out0, out1) and _same(work0, work1)
        return None
    _lib.check(rc)
    written = np.zeros(out0.shape, dtype=bool)
    written[:s.na, :F] = True
    assert _same(out0, out1, written), "ital_kernel_matvec wrote outside out[na][F]"
    assert _same(work0[wl:], work1[wl:]), "ital_kernel_matvec wrote past its workspace"
    assert np.isfinite(out1[:s.na, :F]).all()
    return out1[:s.na, :F]


@pytest.mark.parametrize("case", ref.MATVEC_SMALL_CASES, ids=_id)
def test_kernel_matvec_against_the_extended_reference(dev, case):
    na, nb, ldx, F = case
    s = ref.matvec_case(*case)
    if (na, nb) in ref.MATVEC_SMALL_SPLITS:
        assert (s.nsplit, s.per) == ref.MATVEC_SMALL_SPLITS[(na, nb)]
    out = _matvec_call(dev, s)
    Kref, dK = ref.kernel_ref(s.Xa, s.Xb, s.var, s.ls)
    r = ref.check_matvec(out, Kref, dK, s.W, nb, s.nsplit)
    emu = ref.emu_matvec(s.Xa, ref.row_norms64(s.Xa), s.Xb, ref.row_norms64(s.Xb), s.W, s.var, s.ls)
    _note("ital_kernel_matvec", "small", dict(out=r), dict(out=ref.check_matvec(emu, Kref, dK, s.W, nb, s.nsplit)))
    assert r <= 1.0, (case, r)


@pytest.mark.parametrize("shape", ref.MATVEC_LOOP, ids=_id)
def test_kernel_matvec_in_the_production_loop(dev, shape):
    """More than one tile per workgroup: the loop over j0 re-points its row pointers, reuses the staging LDS and carries the
    accumulators across tiles."""
    na, nb, ldx, F, nsplit, per, last = shape
    s = ref.matvec_case(na, nb, ldx, F)
    assert ref.expected_split(na, nb) == (nsplit, per) and per > 1
    assert ref._cdiv(nb - (nsplit - 1) * per * ref.T, ref.T) == last
    out = _matvec_call(dev, s)
    rows = ref.loop_rows(na, nb)
    Kref, dK = ref.kernel_ref(s.Xa[rows], s.Xb, s.var, s.ls)
    emu = ref.emu_matvec(s.Xa, ref.row_norms64(s.Xa), s.Xb, ref.row_norms64(s.Xb), s.W, s.var, s.ls)
    ratios = dict(out=ref.check_matvec(out[rows], Kref, dK, s.W, nb, nsplit),
                  vs_emu=ref.check_matvec_against_emulation(out, emu, ref.matvec_bound64(s.Xa, s.Xb, s.W, s.var, s.ls, nsplit)))
    _note("ital_kernel_matvec", "loop", ratios, dict(out=ref.check_matvec(emu[rows], Kref, dK, s.W, nb, nsplit)))
    assert max(ratios.values()) <= 1.0, (shape, ratios)


def test_kernel_matvec_refusals_change_nothing_and_name_the_call(dev):
    s = ref.matvec_case(130, 129, 16, 5)
    assert s.nsplit > 1
    _matvec_call(dev, s, F=17, ldw=20, ldo=20, refuse="F must be")
    _matvec_call(dev, s, ldw=s.F - 1, refuse="ldw")
    _matvec_call(dev, s, ldo=s.F - 1, refuse="ldo")
    _matvec_call(dev, s, nb=0, refuse="nb")
    _matvec_call(dev, s, ldx=8, refuse="ldx")
    _matvec_call(dev, s, short=1, refuse="work")
