"""The GP update kernels, one step from known inputs, against the extended-precision reference of tests/_gp_update_ref.py.

ital_chol_append (chol_append_kernel), ital_whiten_append and ital_cross_cov_cols (kcols_body in its two modes), ital_predict,
ital_stage_labelled and ital_gp_append are called through ctypes on buffers built on the host: the state before the call is
solved in the extended type from the reference kernel values and rounded to FP64, so every residual is that of ONE call.  Every
byte a call must not read, and every byte it must not write, holds NaN; afterwards everything outside the documented write set is
compared by its bits with what was uploaded, and the write set is finite.  The results are judged by the componentwise residual
bounds of _gp_update_ref.py (a-priori operation counts; nothing is fitted): largest residual / bound <= 1.  The host side --
that a plain FP64 emulation passes the same bounds at the same shapes and that the checker rejects the mistakes these kernels can
make -- is tests/test_gp_update_ref_host.py.

Largest residual / bound observed (MI355X; FP64 NumPy emulation on the host beside it), printed again by every run with -s:

    entry point             data      factor        alpha         whitened rows  mu            s2           cross-cov
    ital_chol_append        uniform   0.072 / 0.079 0.088 / 0.064
    ital_chol_append        neardup   0.063 / 0.070 0.057 / 0.040
    ital_whiten_append      uniform                               0.109 / 0.089  0.474 / 0.474 0.327 / 0.324
    ital_whiten_append      free                                  0.085 / 0.080  0.123 / 0.111 0.234 / 0.284
    ital_cross_cov_cols     uniform                                                                         0.109 / 0.095
    ital_predict            uniform                               0.088 / 0.090  0.315 / 0.298 0.253 / 0.245
    ital_predict            halved L                              0.123          0.141         0.254
    ital_gp_append          uniform   0.056        0.017         0.062          0.304         0.248
    GaussianProcess.update  chain     0.028         0.076         0.053          0.012         0.010

(device / emulation; the last three rows have no emulation.)  The device sits where the emulation does, an order of magnitude inside
the factor, alpha and whitening bounds: the reciprocal-then-multiply of the substitution, the lane-strided sums and the MFMA
accumulation order cost nothing that shows.  mu and s2 come closest to 1 (0.47, at c = 1, where gamma(c + 2) counts three roundings and
the update makes two or three) on the device and in the emulation alike.  The chain's ratios are smaller because its bounds
carry the counts of up to 135 rows.  Of the strict upper triangle of L: ital_chol_append loads the part inside the 64 x 64
diagonal blocks and never uses it (the NaN there changes nothing); the head of ital_amd/csrc/chol.hip says so.  (The note is
not in include/ital_hip.h yet: the header is hashed into the source stamp of the committed profiles, tools/stamp.py, and the six
whose stamps still match -- general scorer, MCMI, C5 -- would lose the counters bench.py quotes from them.  It belongs in the
header when those profiles are next retaken.)

What a passing result does NOT tell: these are backward-error bounds, so an error in one entry that stays below the bound of the
residuals it moves is invisible.  For an entry of an appended row that is small against its row -- L[m][m // 2] of 1e-4 to
3e-3 at four of the thirty append shapes -- that admits a relative error of that one entry of 1e-11 (three shapes), at the
near-duplicate (65, 15) shape of up to 1e-6; in absolute terms it is the same few 1e-14 everywhere
(tests/test_gp_update_ref_host.py asserts where the line lies, from row m's bounds alone).  No correct FP64 append is held to
less.

Run: python -m pytest tests/test_gpu_gp_update.py -m gpu."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _gp_update_ref as ref  # noqa: E402

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
    for (entry, kind, name), r in sorted(WORST.items()):
        print("device  %-18s %-8s %-9s largest residual/bound = %.3g" % (entry, kind, name, r))


def _note(entry, kind, ratios):
    for name, r in ratios.items():
        key = (entry, kind, name)
        WORST[key] = max(WORST.get(key, 0.0), r)
    print(entry, kind, {k: "%.3g" % v for k, v in ratios.items()})


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _down(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _untouched(before, after, written=None):
    """Everything outside the boolean mask `written` has the bits it was uploaded with."""
    keep = np.ones(before.shape, dtype=bool) if written is None else ~written
    return bool(np.array_equal(_bits(before)[keep], _bits(after)[keep]))


def _mask(shape, *index):
    w = np.zeros(shape, dtype=bool)
    w[index] = True
    return w


def _ld(v):
    """A leading dimension strictly greater than v that is neither a multiple of 64 nor the padded size."""
    ld = v + 3
    while ld % 16 == 0:
        ld += 1
    return ld


def _lower(block, size):
    """The lower triangle of a size x size block; NaN above the diagonal."""
    return np.where(np.tri(size, dtype=bool), block[:size, :size], NAN)


def _norms(rows_t, count, ldx, dev):
    """Squared norms of the first `count` rows by ital_row_norms (what the library hands to these kernels); NaN behind."""
    from ital_amd import _lib
    out = torch.full((rows_t.shape[0],), NAN, dtype=torch.float64, device=dev)
    if count:
        _lib.check(_lib.lib().ital_row_norms(rows_t.data_ptr(), count, ldx, out.data_ptr(), _stream()))
    return out


def _guarded(rows, extra, dev):
    """The rows followed by `extra` rows of NaN, on the host and on the device."""
    host = np.full((rows.shape[0] + extra,) + rows.shape[1:], NAN)
    host[:rows.shape[0]] = rows
    return host, _up(host, dev)


# ------------------------------------------------------------------------------------------------ ital_chol_append
def _factor_buffers(s, dev):
    """L, alpha, XT, XTn of the state before the append: NaN in the strict upper triangle of L, in its rows >= m, in
    alpha[m:], in XT rows >= m + c."""
    m, M = s.m, s.m + s.c
    rows, ldl = M + 2, _ld(M)
    L0 = np.full((rows, ldl), NAN)
    L0[:m, :m] = _lower(s.L, m)
    a0 = np.full(rows, NAN)
    a0[:m] = s.alpha[:m]
    XT0, XTd = _guarded(s.XT[:M], 2, dev)
    return types.SimpleNamespace(rows=rows, ldl=ldl, L0=L0, a0=a0, XT0=XT0, L=_up(L0, dev), alpha=_up(a0, dev), XT=XTd,
                                 XTn=_norms(XTd, M, s.ldx, dev))


def _chol_append(dev, s, positive_definite=True):
    from ital_amd import _lib
    m, c, M = s.m, s.c, s.m + s.c
    b = _factor_buffers(s, dev)
    XTn0 = _down(b.XTn)
    y0 = np.full(16, NAN)
    y0[:c] = s.y[m:M]
    yd = _up(y0, dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().ital_chol_append(b.XT.data_ptr(), b.XTn.data_ptr(), s.ldx, b.L.data_ptr(), b.ldl, b.alpha.data_ptr(),
                                           yd.data_ptr(), m, c, float(s.var), float(s.ls), float(s.noise), status.data_ptr(),
                                           _stream()))
    L1, a1 = _down(b.L), _down(b.alpha)
    what = (s.kind, m, c, s.ldx)
    assert _untouched(b.L0, L1, _mask(L1.shape, slice(m, M), slice(0, M))), what
    assert _untouched(b.a0, a1, _mask(a1.shape, slice(m, M))), what
    assert _untouched(b.XT0, _down(b.XT)) and _untouched(XTn0, _down(b.XTn)) and _untouched(y0, _down(yd)), what
    if positive_definite:
        assert np.isfinite(L1[m:M, :M]).all() and np.isfinite(a1[m:M]).all(), what
    return L1[:M, :M], a1[:M], int(_down(status)[0])


def _id(case):
    return "-".join(str(v) for v in case)


@pytest.mark.parametrize("case", ref.CHOL_CASES, ids=_id)
def test_chol_append_against_the_extended_reference(dev, case):
    s = ref.state(*case)
    L, alpha, status = _chol_append(dev, s)
    assert status == 0
    assert not ref.check_structure(L, s.m, s.c), ref.check_structure(L, s.m, s.c)
    ratios = ref.judge_chol(s, L, alpha)
    _note("ital_chol_append", s.kind, ratios)
    assert max(ratios.values()) <= 1.0, (case, ratios)


@pytest.mark.parametrize("m", [0, 3])
def test_chol_append_reports_a_matrix_that_is_not_positive_definite(dev, m):
    """Two identical new rows with var = 1 and noise = -0.5: the Schur diagonal of the second is 0.5 - 2 = -1.5.  The old rows
    lie far from each other and from the new ones, so their own Gram matrix 0.5 I + (tiny) is positive definite."""
    s = types.SimpleNamespace(kind="not_pd", m=m, c=2, ldx=16, var=1.0, ls=0.5, noise=-0.5)
    M = m + 2
    s.XT = np.zeros((M, 16))
    for r in range(m):
        s.XT[r, r] = 10.0
    s.XT[m:, :5] = -0.25
    s.y = np.array([1.0, -1.0, 1.0, 1.0, -1.0])[:M]
    K, _ = ref.kernel_ref(s.XT, s.XT, s.var, s.ls)
    G = K + ref.xp(s.noise) * ref.xp(np.eye(M))
    s.L, s.alpha = np.zeros((M, M)), np.zeros(M)
    if m:
        Lx = ref.chol_x(G[:m, :m])
        s.L[:m, :m] = ref.rnd(Lx)
        s.alpha[:m] = ref.rnd(ref.solve_lower_x(Lx, ref.xp(s.y[:m])[:, None])[:, 0])
    L, alpha, status = _chol_append(dev, s, positive_definite=False)        # rows < m: compared by their bits in there
    assert status & 1
    assert L[m, m] == pytest.approx(np.sqrt(0.5), rel=1e-12) and not L[m + 1, m + 1] > 0


# ------------------------------------------------------------------------------------------------ ital_whiten_append
def _prior(s):
    """mu and s2 of the state's first m labelled rows (FP64; the checks start from whatever the call was given)."""
    m = s.m
    if s.kind == "free":
        return s.mu_in, s.s2_in
    return s.V[:m].T @ s.alpha[:m], s.var - (s.V[:m] ** 2).sum(axis=0)


def _sweep_buffers(s, dev):
    """The inputs of a sweep over the n data rows: NaN in the row behind X, in xnorm[n:], in the strict upper triangle of
    L22 and in the factor rows' columns >= m + c, in V rows >= m and columns >= n, in mu[n:] and s2[n:]."""
    n, m, c, M = s.n, s.m, s.c, s.m + s.c
    b = types.SimpleNamespace(ldw=_ld(M), ldv=_ld(n))
    b.X0, b.X = _guarded(s.X, 1, dev)
    b.xn = _norms(b.X, n, s.ldx, dev)
    b.Xs0, b.Xs = _guarded(s.XT[m:M], 1, dev)
    b.sn = _norms(b.Xs, c, s.ldx, dev)
    b.Lrows0 = np.full((c + 1, b.ldw), NAN)
    b.Lrows0[:c, :m] = s.L[m:M, :m]
    b.Lrows0[:c, m:M] = _lower(s.L[m:M, m:M], c)
    b.Lrows = _up(b.Lrows0, dev)
    b.V0 = np.full((M + 1, b.ldv), NAN)
    b.V0[:m, :n] = s.V[:m]
    b.V = _up(b.V0, dev)
    mu_in, s2_in = _prior(s)
    b.mu0, b.s20 = np.full(n + 2, NAN), np.full(n + 2, NAN)
    b.mu0[:n], b.s20[:n] = mu_in, s2_in
    b.mu, b.s2 = _up(b.mu0, dev), _up(b.s20, dev)
    b.an0, b.an = _guarded(s.alpha[m:M], 1, dev)
    return b


def _whiten_append(dev, s):
    from ital_amd import _lib
    n, m, c, M = s.n, s.m, s.c, s.m + s.c
    b = _sweep_buffers(s, dev)
    xn0, sn0 = _down(b.xn), _down(b.sn)
    _lib.check(_lib.lib().ital_whiten_append(b.X.data_ptr(), b.xn.data_ptr(), n, s.ldx, b.Xs.data_ptr(), b.sn.data_ptr(), c,
                                             b.Lrows.data_ptr(), b.ldw, b.Lrows.data_ptr() + 8 * m, b.an.data_ptr(),
                                             b.V.data_ptr(), b.ldv, m, float(s.var), float(s.ls), b.mu.data_ptr(),
                                             b.s2.data_ptr(), _stream()))
    V1, mu1, s21 = _down(b.V), _down(b.mu), _down(b.s2)
    what = (s.kind, n, m, c, s.ldx)
    assert _untouched(b.V0, V1, _mask(V1.shape, slice(m, M), slice(0, n))), what
    assert _untouched(b.mu0, mu1, _mask(mu1.shape, slice(0, n))) and _untouched(b.s20, s21, _mask(s21.shape, slice(0, n))), what
    assert _untouched(b.X0, _down(b.X)) and _untouched(xn0, _down(b.xn)) and _untouched(b.Xs0, _down(b.Xs)), what
    assert _untouched(sn0, _down(b.sn)) and _untouched(b.Lrows0, _down(b.Lrows)) and _untouched(b.an0, _down(b.an)), what
    assert np.isfinite(V1[m:M, :n]).all() and np.isfinite(mu1[:n]).all() and np.isfinite(s21[:n]).all(), what
    return ref.judge_whiten(s, V1[:M, :n], b.mu0[:n], mu1[:n], b.s20[:n], s21[:n])


@pytest.mark.parametrize("case", ref.WHITEN_CASES, ids=_id)
def test_whiten_append_against_the_extended_reference(dev, case):
    n, m, c, ldx = case
    ratios = _whiten_append(dev, ref.state("uniform", m, c, ldx, n))
    _note("ital_whiten_append", "uniform", ratios)
    assert max(ratios.values()) <= 1.0, (case, ratios)


def test_whiten_append_on_free_form_inputs(dev):
    """An arbitrary well-conditioned triangular L22, random L21, V, alpha, mu and s2: the residual form needs no consistent
    state."""
    ratios = _whiten_append(dev, ref.free_form_whiten())
    _note("ital_whiten_append", "free", ratios)
    assert max(ratios.values()) <= 1.0, ratios


# ------------------------------------------------------------------------------------------------ ital_cross_cov_cols
@pytest.mark.parametrize("case", ref.CROSS_CASES, ids=_id)
def test_cross_cov_cols_against_the_extended_reference(dev, case):
    from ital_amd import _lib
    n, m, c, ldx = case
    s = ref.state("uniform", m, c, ldx, n)
    b = _sweep_buffers(s, dev)
    W0 = np.full((c + 1, b.ldw), NAN)
    W0[:c, :m] = s.W
    V0 = np.full((m + 1, b.ldv), NAN)
    V0[:m, :n] = s.V[:m]
    out0 = np.full((c + 1, b.ldv), NAN)
    W, V, out = _up(W0, dev), _up(V0, dev), _up(out0, dev)
    _lib.check(_lib.lib().ital_cross_cov_cols(b.X.data_ptr(), b.xn.data_ptr(), n, ldx, b.Xs.data_ptr(), b.sn.data_ptr(), c,
                                              W.data_ptr(), b.ldw, V.data_ptr(), b.ldv, m, float(s.var), float(s.ls),
                                              out.data_ptr(), b.ldv, _stream()))
    out1 = _down(out)
    what = (n, m, c, ldx)
    assert _untouched(out0, out1, _mask(out1.shape, slice(0, c), slice(0, n))) and np.isfinite(out1[:c, :n]).all(), what
    assert _untouched(W0, _down(W)) and _untouched(V0, _down(V)) and _untouched(b.X0, _down(b.X)), what
    ratios = ref.judge_cross(s, out1[:c, :n])
    _note("ital_cross_cov_cols", "uniform", ratios)
    assert max(ratios.values()) <= 1.0, (what, ratios)


# ------------------------------------------------------------------------------------------------ ital_stage_labelled
def _label_batch(slots, y):
    from ital_amd import _lib
    lb = _lib.ItalLabelBatch()
    lb.c = len(slots)
    for j, (slot, label) in enumerate(zip(slots, y)):
        lb.slot[j], lb.y[j] = int(slot), float(label)
    return lb


@pytest.mark.parametrize("ldx", [16, 80, 144])
def test_stage_labelled_copies_rows_norms_and_labels_by_their_bits(dev, ldx):
    """Regression: the staging kernels used to sum the squares one feature per lane, ital_row_norms two per lane, so the staged
    norm of a row differed in its last bit from that row's entry in xnorm (seen at all three sizes).  They now share the order.
    ldx = 16: eight lanes hold a pair; 80: forty; 144: eight lanes make a second trip."""
    from ital_amd import _lib
    lib = _lib.lib()
    d = ldx - 9
    rng = np.random.default_rng(ldx)
    rows = ref.padded(3.0 * rng.standard_normal((6, d)), ldx)
    rows[2, 1] = -0.0
    rows[4, ldx - 1] = -0.0                 # a pad column keeps its bits too
    slots = [4, 0, 5, 2, 0]
    y = [1.0, -1.0, -0.0, 0.5, 1.0]
    c = len(slots)
    rows_t = _up(rows, dev)
    XT = torch.full((c + 1, ldx), NAN, dtype=torch.float64, device=dev)
    XTn = torch.full((c + 1,), NAN, dtype=torch.float64, device=dev)
    yd = torch.full((17,), NAN, dtype=torch.float64, device=dev)
    _lib.check(lib.ital_stage_labelled(rows_t.data_ptr(), ldx, _label_batch(slots, y), XT.data_ptr(), XTn.data_ptr(),
                                       yd.data_ptr(), _stream()))
    XT1, XTn1, y1 = _down(XT), _down(XTn), _down(yd)
    assert _untouched(rows[slots], XT1[:c]) and np.isnan(XT1[c]).all() and _untouched(rows, _down(rows_t))
    assert _untouched(np.array(y), y1[:c]) and np.isnan(y1[c:]).all()
    want = torch.full((c + 1,), NAN, dtype=torch.float64, device=dev)
    _lib.check(lib.ital_row_norms(XT.data_ptr(), c, ldx, want.data_ptr(), _stream()))
    want = _down(want)
    print("staged norms, ldx = %d: %s\nital_row_norms:       %s" % (ldx, XTn1[:c].tolist(), want[:c].tolist()))
    assert np.isfinite(XTn1[:c]).all() and np.isnan(XTn1[c])
    assert _untouched(want, XTn1)


# ------------------------------------------------------------------------------------------------ ital_gp_append
@pytest.mark.parametrize("m,c", [(0, 1), (63, 2), (65, 15)])
def test_gp_append_has_the_bits_of_the_three_separate_calls(dev, m, c):
    """Both paths are the same Cholesky kernel (with and without the staging in front) and the same sweep, so equality is the
    contract.  The slots are out of order; the one-call result is judged by the residual bounds as well."""
    from ital_amd import _lib
    lib = _lib.lib()
    s = ref.state("uniform", m, c, 16, 65)
    n, M, ldx = s.n, m + c, s.ldx
    rng = np.random.default_rng(m + c)
    slots = rng.permutation(c + 3)[:c]
    rows = ref.padded(rng.random((c + 3, s.d)), ldx)
    rows[slots] = s.XT[m:M]
    rows_t = _up(rows, dev)
    lb = _label_batch(slots, s.y[m:M])
    got = []
    for one_call in (False, True):
        f, b = _factor_buffers(s, dev), _sweep_buffers(s, dev)
        f.XT[m:] = NAN                       # the new rows are not there yet: the staging brings them
        f.XTn[m:] = NAN
        ybuf = torch.full((16,), NAN, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        XTm, XTnm = f.XT.data_ptr() + 8 * m * ldx, f.XTn.data_ptr() + 8 * m
        Lm = f.L.data_ptr() + 8 * m * f.ldl
        if one_call:
            a = _lib.ItalAppendDesc()
            a.rows, a.ldx, a.lb, a.X, a.xnorm, a.n = rows_t.data_ptr(), ldx, lb, b.X.data_ptr(), b.xn.data_ptr(), n
            a.XT, a.XTn, a.L, a.ldl, a.alpha, a.ybuf = f.XT.data_ptr(), f.XTn.data_ptr(), f.L.data_ptr(), f.ldl, \
                f.alpha.data_ptr(), ybuf.data_ptr()
            a.V, a.ldv, a.m, a.var, a.length_scale, a.noise = b.V.data_ptr(), b.ldv, m, float(s.var), float(s.ls), float(s.noise)
            a.mu, a.s2, a.status = b.mu.data_ptr(), b.s2.data_ptr(), status.data_ptr()
            _lib.check(lib.ital_gp_append(ctypes.byref(a), _stream()))
        else:
            _lib.check(lib.ital_stage_labelled(rows_t.data_ptr(), ldx, lb, XTm, XTnm, ybuf.data_ptr(), _stream()))
            _lib.check(lib.ital_chol_append(f.XT.data_ptr(), f.XTn.data_ptr(), ldx, f.L.data_ptr(), f.ldl, f.alpha.data_ptr(),
                                            ybuf.data_ptr(), m, c, float(s.var), float(s.ls), float(s.noise), status.data_ptr(),
                                            _stream()))
            _lib.check(lib.ital_whiten_append(b.X.data_ptr(), b.xn.data_ptr(), n, ldx, XTm, XTnm, c, Lm, f.ldl, Lm + 8 * m,
                                              f.alpha.data_ptr() + 8 * m, b.V.data_ptr(), b.ldv, m, float(s.var), float(s.ls),
                                              b.mu.data_ptr(), b.s2.data_ptr(), _stream()))
        got.append([_down(t) for t in (f.L, f.alpha, b.V, b.mu, b.s2, f.XT, f.XTn, ybuf)] + [int(_down(status)[0])])
    three, one = got
    assert three[-1] == 0 and one[-1] == 0
    for name, x, y in zip(("L", "alpha", "V", "mu", "s2", "XT", "XTn", "ybuf"), three, one):
        assert _untouched(x, y), (m, c, name)
    L, alpha, V, mu, s2, XT, XTn, _, _ = one
    assert _untouched(s.XT[:M], XT[:M]) and np.isnan(XT[M:]).all() and np.isfinite(XTn[m:M]).all() and np.isnan(XTn[M:]).all()
    assert not ref.check_structure(L[:M, :M], m, c)
    mu_in, s2_in = _prior(s)
    ratios = ref.judge_chol(s, L[:M, :M], alpha[:M])
    # the sweep read the factor rows and alpha_new the device had just written: it is judged against those
    t = types.SimpleNamespace(**vars(s))
    t.L, t.alpha = np.tril(L[:M, :M]), alpha[:M]
    t.L[:m], t.alpha[:m] = 0.0, 0.0
    ratios.update(ref.judge_whiten(t, V[:M, :n], mu_in, mu[:n], s2_in, s2[:n]))
    _note("ital_gp_append", "uniform", ratios)
    assert max(ratios.values()) <= 1.0, ratios


# ------------------------------------------------------------------------------------------------ ital_predict
def _predict(dev, s, clamp):
    """ital_predict of the state's m labelled rows at its n data rows.  Returns Vt, mean, pvar."""
    from ital_amd import _lib
    m, nt, ldx = s.m + s.c, s.n, s.ldx
    ldl, ldvt = _ld(m), _ld(nt)
    L0 = np.full((m + 1, ldl), NAN)
    L0[:m, :m] = _lower(s.L, m)
    a0, ad = _guarded(s.alpha, 1, dev)
    XT0, XT = _guarded(s.XT, 1, dev)
    XTn = _norms(XT, m, ldx, dev)
    Xt0, Xt = _guarded(s.X, 1, dev)
    Ld = _up(L0, dev)
    mean, pvar, xtn = (torch.full((nt + 2,), NAN, dtype=torch.float64, device=dev) for _ in range(3))
    Vt = torch.full((m + 1, ldvt), NAN, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().ital_predict(Xt.data_ptr(), nt, ldx, XT.data_ptr(), XTn.data_ptr(), m, Ld.data_ptr(), ldl, ad.data_ptr(),
                                       float(s.var), float(s.ls), mean.data_ptr(), pvar.data_ptr(), xtn.data_ptr(), Vt.data_ptr(),
                                       ldvt, clamp, _stream()))
    Vt1, mean1, pvar1, xtn1 = _down(Vt), _down(mean), _down(pvar), _down(xtn)
    what = (m, nt, clamp)
    assert _untouched(L0, _down(Ld)) and _untouched(a0, _down(ad)) and _untouched(XT0, _down(XT)) and _untouched(Xt0, _down(Xt)), what
    assert np.isnan(Vt1[m]).all() and np.isnan(Vt1[:, nt:]).all() and np.isfinite(Vt1[:m, :nt]).all(), what
    for v in (mean1, pvar1, xtn1):
        assert np.isnan(v[nt:]).all() and np.isfinite(v[:nt]).all(), what
    return Vt1[:m, :nt], mean1[:nt], pvar1[:nt]


@pytest.mark.parametrize("case", ref.PREDICT_CASES, ids=_id)
def test_predict_against_the_extended_reference(dev, case):
    m, nt = case
    s = ref.state("uniform", m, 0, 16, nt)
    ratios = ref.judge_predict(s, *_predict(dev, s, 0))
    _note("ital_predict", "uniform", ratios)
    assert max(ratios.values()) <= 1.0, (case, ratios)


@pytest.mark.parametrize("m,nt", [(1, 1), (17, 65), (65, 17), (65, 65)])
def test_predict_clamps_the_variance_at_labelled_points(dev, m, nt):
    """Test points equal to labelled points with noise = 1e-10, the case the learners meet.  The variance there is 1e-10 with a
    rounding error of some 1e-14, so it stays positive (on the device and in the FP64 emulation alike): this case shows that
    the clamp leaves such values alone.  That it clamps is test_predict_clamps_a_negative_variance_to_plus_zero."""
    s = ref.state("uniform", m, 0, 16, nt, 1e-10, True)
    _, _, raw = _predict(dev, s, 0)
    _, _, clamped = _predict(dev, s, 1)
    print("unclamped variances at labelled points: min %.3g max %.3g, %d of %d negative" % (raw.min(), raw.max(), (raw < 0).sum(), nt))
    assert (clamped >= 0).all()
    assert _untouched(np.where(raw > 0, raw, 0.0), clamped)


@pytest.mark.parametrize("m,nt", [(1, 1), (17, 65), (65, 17), (65, 65)])
def test_predict_clamps_a_negative_variance_to_plus_zero(dev, m, nt):
    """A consistent state keeps var - colsum(Vt^2) at +noise or above up to rounding, so a negative variance needs an
    inconsistent one: the factor is halved (exactly; Vt doubles and colsum(Vt^2) reaches 4 var at a labelled point, the variance
    -3 var), and every second test point is moved far from all labelled rows, where the variance stays +var.  The unclamped
    result is held to the residual bounds against the halved factor, so the negative numbers are the right ones; the clamped
    result equals max(0, unclamped) by bits, +0.0 where it was negative, and the mean and Vt do not depend on the clamp."""
    s = types.SimpleNamespace(**vars(ref.state("uniform", m, 0, 16, nt)))
    s.L = 0.5 * s.L
    s.X = s.X.copy()
    s.X[1::2, :s.d] += 5.0
    s.K_TX, s.dK_TX = ref.kernel_ref(s.XT, s.X, s.var, s.ls)
    Vt, mean, raw = _predict(dev, s, 0)
    Vc, mean_c, clamped = _predict(dev, s, 1)
    print("unclamped variances: min %.3g max %.3g, %d of %d negative" % (raw.min(), raw.max(), (raw < 0).sum(), nt))
    assert (raw < 0).any() and raw.min() < -1.0
    assert nt == 1 or (raw[1::2] > 1.0).all()
    ratios = ref.judge_predict(s, Vt, mean, raw)
    _note("ital_predict", "halved L", ratios)
    assert max(ratios.values()) <= 1.0, ratios
    assert _untouched(np.where(raw > 0, raw, 0.0), clamped) and (_bits(clamped[raw < 0]) == 0).all()
    assert _untouched(Vt, Vc) and _untouched(mean, mean_c)


# ------------------------------------------------------------------------------------------------ the Python path
def test_a_chain_of_updates_through_capacity_growth(dev):
    """GaussianProcess.update with c = 1, 4, 17, 3, 40, 70 from capacity 16: m crosses 16, 64 and 128 and ends at 135, the
    buffers are re-allocated on the way and the last five labelled rows repeat earlier ones (Schur diagonal = noise).  Every
    row of L, alpha and V was produced against the device's own earlier rows, so the rowwise bounds compose: row g is judged
    with the count m + c + 4 of the append (of at most 16 rows) that wrote it; mu and s2 from the prior with gamma(m + 8)."""
    from ital_amd import GaussianProcess
    n, d = 130, 40
    rng = np.random.default_rng(135)
    X = rng.random((n, d))
    gp = GaussianProcess(X, 0.8 * float(np.sqrt(d / 12.0)), device=dev, capacity=16)
    order = np.concatenate((rng.permutation(n), rng.permutation(n)[:5]))
    y = np.where(rng.random(len(order)) < 0.5, 1.0, -1.0)
    y[n:] = y[[int(np.nonzero(order[:n] == i)[0][0]) for i in order[n:]]]          # a repeated row keeps its label
    steps, at = {}, 0
    for size in (1, 4, 17, 3, 40, 70):
        gp.update(order[at:at + size].tolist(), y[at:at + size])
        for c0 in range(0, size, 16):
            c = min(16, size - c0)
            steps.update({g: at + c0 + c + 4 for g in range(at + c0, at + c0 + c)})
        at += size
    m = gp.m
    assert m == 135 == len(steps) and gp.cap >= m and int(_down(gp.status)[0]) == 0
    L, alpha, V = _down(gp.L)[:m, :m], _down(gp.alpha)[:m], _down(gp.V)[:m, :n]
    XT, Xd, mu, s2 = _down(gp.XT)[:m], _down(gp.Xd)[:n], _down(gp.mu)[:n], _down(gp.s2)[:n]
    assert _untouched(ref.padded(X[order], gp.ldx), XT) and _untouched(y, gp.y)
    assert (np.diag(L) > 0).all() and (_bits(np.triu(L, 1)) == 0).all()
    K_TT, dK_TT = ref.kernel_ref(XT, XT, gp.var, gp.length_scale)
    G = K_TT + ref.xp(gp.noise) * ref.xp(np.eye(m))
    K_TX, dK_TX = ref.kernel_ref(XT, Xd, gp.var, gp.length_scale)
    r_mu, r_s2 = ref.check_mu_s2(np.zeros(n), mu, np.full(n, float(gp.var)), s2, V, alpha, m + 8)
    ratios = dict(factor=ref.check_factor(L, range(m), G, dK_TT, steps), alpha=ref.check_alpha(L, alpha, y, range(m), steps),
                  whiten=ref.check_whiten(L, V, range(m), K_TX, dK_TX, steps), mu=r_mu, s2=r_s2)
    _note("GaussianProcess.update", "chain", ratios)
    assert max(ratios.values()) <= 1.0, ratios
