"""A live session in a library-owned context (include/ital_ctx_live.h, csrc/ctx_live.hip): the capacity grows, rows arrive
and leave, the hyper-parameters change and are scored -- through ctypes with host arrays only, against contexts built from
scratch on the result and against the Python learners' add_data / remove_data / set_params / tune_params.

"Equal" is np.array_equal on the float64 arrays throughout: either both sides run the same kernels on the same operands, or
the DEFINITION of ital_whiten_rows (include/ital_rewhiten.h) states the equality -- which is why the 21 labels are given as
one ital_ctx_update call of 16 and one of 5, the block partition that DEFINITION names."""
import ctypes
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ranks  # noqa: E402

N, D = 150, 8
LS = float(np.sqrt(8 / 12.0))
XALL = np.random.default_rng(17).random((192, D))
X = XALL[:N]
YALL = np.where(XALL[:, 0] > 0.5, 1.0, -1.0)


def _rel_first(ids):
    """The order in which a learner's update() hands a dict of these ids to its GP: relevant ones first."""
    return [i for i in ids if YALL[i] > 0] + [i for i in ids if YALL[i] < 0]


BLOCK_A = _rel_first([3, 7, 12, 20, 25, 31, 38, 44, 52, 59, 63, 70, 77, 81, 95, 101])      # 16 labels
BLOCK_B = _rel_first([110, 118, 123, 131, 140])                                            # 5 more
LABELLED = BLOCK_A + BLOCK_B
REMOVED = [0, 7, 88, 149]                                                                  # 7 is labelled


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ital_amd import _lib
    torch.cuda.init()
    return _lib.load()


def _i64(v):
    return np.ascontiguousarray(v, dtype=np.int64)


class Ctx:
    """One context through ctypes; every call returns the library's code (the caller asserts)."""

    def __init__(self, lib, X, ls=LS, var=1.0, noise=1e-6, capacity=64, rank=0, world=1, comm=None, n_total=None):
        self.lib = lib
        X = np.ascontiguousarray(X, dtype=np.float64)
        self.h = ctypes.c_void_p()
        rc = lib.ital_ctx_create(len(X) if n_total is None else n_total, X.shape[1], float(ls), float(var), float(noise), capacity,
                                 rank, world, comm, ctypes.byref(self.h))
        assert rc == 0, self.err()
        assert lib.ital_ctx_fit(self.h, X.ctypes.data, 0, None) == 0, self.err()

    def err(self):
        return self.lib.ital_last_error().decode()

    def close(self):
        assert self.lib.ital_ctx_destroy(self.h) == 0

    def try_update(self, idx, y=None):
        idx = _i64(idx)
        y = np.ascontiguousarray(YALL[idx] if y is None else y, dtype=np.float64)
        return self.lib.ital_ctx_update(self.h, idx.ctypes.data, y.ctypes.data, len(idx), None)

    def update(self, idx, y=None):
        assert self.try_update(idx, y) == 0, self.err()

    def label(self):
        """The 21 labels as one update of 16 and one of 5."""
        self.update(BLOCK_A)
        self.update(BLOCK_B)
        return self

    def revoke(self, idx):
        idx = _i64(idx)
        return self.lib.ital_ctx_revoke(self.h, idx.ctypes.data, len(idx), None)

    def fetch(self, k):
        p = np.zeros(max(k, 1), dtype=np.int64)
        rc = self.lib.ital_ctx_fetch(self.h, k, p.ctypes.data, None)
        return rc, p[: max(rc, 0)].tolist()

    def fetch_list(self, k, cand, subset=()):
        """k picks out of the candidate list `cand`, optionally with a change-estimation subset."""
        cand, subset = _i64(cand), _i64(subset)
        p = np.zeros(max(k, 1), dtype=np.int64)
        rc = self.lib.ital_ctx_fetch_list(self.h, k, cand.ctypes.data, len(cand), subset.ctypes.data if len(subset) else None,
                                          len(subset), p.ctypes.data, None)
        return rc, p[: max(rc, 0)].tolist()

    def mcmi_fetch(self, k, cand=None):
        p = np.zeros(max(k, 1), dtype=np.int64)
        cand = None if cand is None else _i64(cand)
        rc = self.lib.ital_ctx_mcmi_fetch(self.h, k, None if cand is None else cand.ctypes.data, 0 if cand is None else len(cand),
                                          p.ctypes.data, None)
        return rc, p[: max(rc, 0)].tolist()

    def predict_stored(self):
        n = self.lib.ital_ctx_local_rows(self.h, None)
        mean, var = np.empty(n), np.empty(n)
        assert self.lib.ital_ctx_predict_stored(self.h, mean.ctypes.data, var.ctypes.data, None) == 0, self.err()
        return mean, var

    def top_results(self, k):
        idx = np.zeros(max(k, 1), dtype=np.int64)
        rc = self.lib.ital_ctx_top_results(self.h, k, idx.ctypes.data, None)
        return rc, idx[:k].tolist()

    def predict(self, Xt):
        Xt = np.ascontiguousarray(Xt, dtype=np.float64)
        mean, var = np.empty(len(Xt)), np.empty(len(Xt))
        rc = self.lib.ital_ctx_predict(self.h, Xt.ctypes.data, len(Xt), mean.ctypes.data, var.ctypes.data, None)
        return rc, mean, var

    # ---- include/ital_ctx_live.h
    def reserve(self, capacity):
        return self.lib.ital_ctx_reserve(self.h, capacity, None)

    def add_rows(self, rows, k=None, on_device=0):
        if rows is None:
            return self.lib.ital_ctx_add_rows(self.h, None, 0 if k is None else k, on_device, None)
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        return self.lib.ital_ctx_add_rows(self.h, rows.ctypes.data, len(rows) if k is None else k, on_device, None)

    def remove_rows(self, idx, n_old=None):
        idx = _i64(idx)
        imap = None if n_old is None else np.full(n_old, -7, dtype=np.int64)
        rc = self.lib.ital_ctx_remove_rows(self.h, idx.ctypes.data, len(idx), None if imap is None else imap.ctypes.data, None)
        return rc if n_old is None else (rc, imap)

    def set_params(self, length_scale=np.nan, var=np.nan, noise=np.nan):
        return self.lib.ital_ctx_set_params(self.h, float(length_scale), float(var), float(noise), None)

    def evidence(self, params):
        params = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 3)
        scores = np.full((len(params), 3), 7.0)
        ok = np.full(len(params), -1, dtype=np.int32)
        rc = self.lib.ital_ctx_evidence(self.h, params.ctypes.data, len(params), scores.ctypes.data, ok.ctypes.data, None)
        return rc, scores, ok


def assert_same_state(a, b):
    """predict_stored in bits, top_results."""
    (ma, va), (mb, vb) = a.predict_stored(), b.predict_stored()
    assert ma.shape == mb.shape
    assert np.array_equal(ma, mb), np.abs(ma - mb).max()
    assert np.array_equal(va, vb), np.abs(va - vb).max()
    ra, rb = a.top_results(10), b.top_results(10)
    assert ra[0] == 0 and rb[0] == 0 and ra[1] == rb[1]


def assert_same_fetch(a, b, k=4):
    """Both contexts stand at the same position of mvndst's stream."""
    ra, rb = a.fetch(k), b.fetch(k)
    assert ra[0] == k and rb[0] == k, (a.err(), ra, rb)
    assert ra[1] == rb[1]
    return ra[1]


def _learner(data=X, **kw):
    from ital_amd import ITAL
    L = ITAL(data, length_scale=kw.pop("length_scale", LS), device="cuda:0", **kw)
    L.update({i: YALL[i] for i in BLOCK_A})
    L.update({i: YALL[i] for i in BLOCK_B})
    assert [int(i) for i in L.gp.ind] == LABELLED      # the context's insertion order
    return L


def _learner_fetch(L, k=4, reset=True):
    from ital_amd import mvn_stream
    if reset:
        mvn_stream.GLOBAL.reset()                      # where a fresh context's stream stands
    return [int(i) for i in L.fetch_unlabelled(k)]


# ------------------------------------------------------------------ rows arrive
def test_added_rows_equal_a_context_built_on_all_rows(lib):
    a, b = Ctx(lib, X).label(), Ctx(lib, XALL).label()
    try:
        assert a.top_results(10)[0] == 0 and a.mcmi_fetch(3)[0] == 3      # scratch sized by the 150 rows exists
        assert a.add_rows(XALL[150:187]) == 0, a.err()                    # ldv 160 -> 192
        assert lib.ital_ctx_local_rows(a.h, None) == 187
        assert a.add_rows(XALL[187:192]) == 0, a.err()                    # ldv stays 192
        assert a.add_rows(XALL[:0]) == 0 and a.add_rows(None, 0) == 0     # k == 0
        assert_same_state(a, b)
        assert b.mcmi_fetch(3)[0] == 3
        picks = assert_same_fetch(a, b)
        assert a.mcmi_fetch(3)[1] == b.mcmi_fetch(3)[1]
        # the picks and a new row can be labelled: by the next update the new rows are ordinary rows
        new = picks + [i for i in (190,) if i not in picks]
        a.update(new)
        b.update(new)
        assert_same_state(a, b)
    finally:
        a.close()
        b.close()
    L = _learner()
    L.add_data(XALL[150:187])
    L.add_data(XALL[187:192])
    assert _learner_fetch(L) == picks


def test_added_rows_from_device_memory(lib):
    a, b = Ctx(lib, X).label(), Ctx(lib, XALL[:170]).label()
    try:
        rows = torch.from_numpy(XALL[150:170].copy()).to("cuda:0")
        torch.cuda.synchronize()
        assert lib.ital_ctx_add_rows(a.h, rows.data_ptr(), 20, 1, None) == 0, a.err()
        assert_same_state(a, b)
    finally:
        a.close()
        b.close()


def test_rows_added_before_the_first_label(lib):
    a, b = Ctx(lib, X), Ctx(lib, XALL[:163])
    try:
        assert a.add_rows(XALL[150:163]) == 0, a.err()
        (ma, va), (mb, vb) = a.predict_stored(), b.predict_stored()
        assert np.array_equal(ma, mb) and np.array_equal(va, vb) and (va == 1.0).all()
        a.label()
        b.label()
        assert_same_state(a, b)
        assert_same_fetch(a, b)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ rows leave
def test_removed_unlabelled_rows_leave_the_survivors_bits(lib):
    a = Ctx(lib, X).label()
    try:
        mean, var = a.predict_stored()
        gone = [0, 88, 149]
        rc, imap = a.remove_rows(gone, N)
        assert rc == 0, a.err()
        m2, v2 = a.predict_stored()
        assert np.array_equal(m2, np.delete(mean, gone)) and np.array_equal(v2, np.delete(var, gone))
        want = np.full(N, -1, dtype=np.int64)
        want[np.delete(np.arange(N), gone)] = np.arange(N - 3)
        assert np.array_equal(imap, want)
        # ... and are what a context built on the surviving rows holds (labels renumbered)
        b = Ctx(lib, np.delete(X, gone, 0))
        try:
            b.update(imap[BLOCK_A], YALL[BLOCK_A])
            b.update(imap[BLOCK_B], YALL[BLOCK_B])
            assert_same_state(a, b)
            assert_same_fetch(a, b)
        finally:
            b.close()
    finally:
        a.close()


def test_removed_rows_with_a_labelled_one(lib):
    from ital_amd.device_data import removal_map
    a, r = Ctx(lib, X).label(), Ctx(lib, X).label()
    try:
        for c in (a, r):                                  # scratch sized by the 150 rows exists
            assert c.top_results(10)[0] == 0 and c.mcmi_fetch(3)[0] == 3 and c.predict(XALL[150:160])[0] == 0
        rc, imap = a.remove_rows(REMOVED, N)
        assert rc == 0, a.err()
        assert np.array_equal(imap, removal_map(N, REMOVED))
        assert np.array_equal(imap[np.delete(np.arange(N), REMOVED)], np.arange(N - 4)) and (imap[REMOVED] == -1).all()
        assert lib.ital_ctx_local_rows(a.h, None) == N - 4
        # the same as taking the label back first
        assert r.revoke([7]) == 0, r.err()
        assert r.remove_rows(REMOVED) == 0, r.err()
        assert_same_state(a, r)
        assert a.mcmi_fetch(3)[1] == r.mcmi_fetch(3)[1]
        # the removed sample's label is gone: 20 labelled samples are left, and they cannot be labelled again
        assert a.try_update([int(imap[3])]) == -22 and "Cannot change feedback" in a.err()
        L = _learner()
        assert np.array_equal(L.remove_data(REMOVED), imap)
        want = _learner_fetch(L)
        got = assert_same_fetch(a, r)
        assert got == want
        old = np.delete(np.arange(N), REMOVED)[got]       # the picks in the numbering before the removal
        assert np.array_equal(imap[old], got) and not set(old) & set(REMOVED)
        # rows arrive again: every scratch buffer that was sized by the old row count is rebuilt
        for c in (a, r):
            assert c.add_rows(XALL[150:163]) == 0, c.err()
        L.add_data(XALL[150:163])
        assert_same_state(a, r)
        assert a.top_results(10)[1] == [int(i) for i in L.top_results(10)]
        assert assert_same_fetch(a, r) == _learner_fetch(L, reset=False)
        assert a.mcmi_fetch(5)[1] == r.mcmi_fetch(5)[1]
        rc, pm, _ = a.predict(XALL[170:180])
        assert rc == 0, a.err()
        np.testing.assert_allclose(pm, L.gp.predict(XALL[170:180]), rtol=0, atol=2e-9)
    finally:
        a.close()
        r.close()


# ------------------------------------------------------------------ other hyper-parameters
NEW = dict(length_scale=LS * 1.5, var=0.7, noise=1e-4)


def _fresh_with(lib, order, data=X, **params):
    f = Ctx(lib, data, params["length_scale"], params["var"], params["noise"])
    f.update(order)                                       # one call: blocks of 16 from position 0
    return f


def test_set_params_equals_a_fresh_context(lib):
    a, n = Ctx(lib, X).label(), Ctx(lib, X).label()
    f = _fresh_with(lib, LABELLED, **NEW)
    try:
        assert a.set_params(**NEW) == 0, a.err()
        assert_same_state(a, f)
        # a NaN keeps the value
        assert n.set_params(length_scale=NEW["length_scale"]) == 0 and n.set_params(var=0.7, noise=1e-4) == 0, n.err()
        assert n.set_params() == 0
        assert_same_state(n, f)
        picks = assert_same_fetch(a, f)
        assert n.fetch(4)[1] == picks
        L = _learner()
        L.set_params(**NEW)
        assert _learner_fetch(L) == picks
    finally:
        a.close()
        n.close()
        f.close()


def test_set_params_after_a_revoke_follows_the_insertion_order(lib):
    a = Ctx(lib, X).label()
    order = [i for i in LABELLED if i != LABELLED[3]]
    f = _fresh_with(lib, order, **NEW)
    try:
        assert a.revoke([LABELLED[3]]) == 0, a.err()
        assert a.set_params(**NEW) == 0, a.err()
        assert_same_state(a, f)
        assert_same_fetch(a, f)
        # and back: the labels are remembered across the rebuild
        assert a.set_params(LS, 1.0, 1e-6) == 0, a.err()
        g = _fresh_with(lib, order, length_scale=LS, var=1.0, noise=1e-6)
        try:
            assert_same_state(a, g)
        finally:
            g.close()
    finally:
        a.close()
        f.close()


def test_set_params_before_the_first_label(lib):
    a = Ctx(lib, X)
    f = _fresh_with(lib, LABELLED, **NEW)
    try:
        assert a.set_params(**NEW) == 0, a.err()
        mean, var = a.predict_stored()
        assert (mean == 0).all() and (var == 0.7).all()
        a.update(LABELLED)
        assert_same_state(a, f)
    finally:
        a.close()
        f.close()


def _twins():
    """Ten labelled samples and their exact copies, also labelled: with noise = 0 the copies' pivots are rounding residue
    around zero, and the Gram is not positive definite -- for numpy's Cholesky and for ital_chol_append alike."""
    Xd = X.copy()
    Xd[100:110] = Xd[:10]
    ids = list(range(10)) + list(range(100, 110)) + [120]
    y = {i: float(YALL[i - 100 if 100 <= i < 110 else i]) for i in ids}          # twins agree
    ids = [i for i in ids if y[i] > 0] + [i for i in ids if y[i] < 0]
    return Xd, ids, np.array([y[i] for i in ids])


def test_twins_are_not_positive_definite_for_numpy():
    Xd, ids, _ = _twins()
    T = Xd[ids]
    K = np.exp(((T[:, None, :] - T[None, :, :]) ** 2).sum(-1) / (-2 * LS * LS))
    assert np.linalg.matrix_rank(K) <= len(ids) - 10
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(K - 1e-12 * np.eye(len(ids)))       # (the exact Gram is singular: any rounding decides)


def test_set_params_refuses_a_gram_that_is_not_positive_definite(lib):
    Xd, ids, y = _twins()
    a = Ctx(lib, Xd)
    try:
        a.update(ids[:16], y[:16])
        a.update(ids[16:], y[16:])
        mean, var = a.predict_stored()
        b = Ctx(lib, Xd)
        try:
            b.update(ids[:16], y[:16])
            b.update(ids[16:], y[16:])
            assert a.set_params(noise=0.0) == -33 and "not positive definite" in a.err()
            assert a.set_params(LS * 2, 0.5, 0.0) == -33
            m2, v2 = a.predict_stored()
            assert np.array_equal(mean, m2) and np.array_equal(var, v2)
            assert_same_state(a, b)
            assert_same_fetch(a, b)                       # (all twins are labelled: no two candidates are alike)
            # the old parameters are still the context's: a change of the variance alone keeps noise = 1e-6
            assert a.set_params(var=0.9) == 0 and b.set_params(LS, 0.9, 1e-6) == 0
            assert_same_state(a, b)
        finally:
            b.close()
    finally:
        a.close()


# ------------------------------------------------------------------ the capacity
def test_reserve_lifts_the_capacity(lib):
    a, b = Ctx(lib, X, capacity=16), Ctx(lib, X, capacity=48)
    first, more = LABELLED[:10], LABELLED[10:]
    try:
        a.update(first)
        b.update(first)
        assert a.top_results(10)[0] == 0 and a.mcmi_fetch(3)[0] == 3 and b.mcmi_fetch(3)[0] == 3
        assert a.predict(XALL[150:160])[0] == 0 and a.revoke([first[2]]) == 0 and a.try_update([first[2]]) == 0
        assert b.revoke([first[2]]) == 0 and b.try_update([first[2]]) == 0
        before = a.predict_stored()
        assert a.try_update(more) == -12 and "capacity" in a.err()
        after = a.predict_stored()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert a.reserve(16) == 0 and a.reserve(3) == 0 and a.reserve(-5) == 0       # not above the capacity: no-ops
        assert a.try_update(more) == -12
        assert a.reserve(48) == 0, a.err()
        assert_same_state(a, b)
        a.update(more)
        b.update(more)
        assert_same_state(a, b)
        assert_same_fetch(a, b)                           # k = 4: records of the new length
        ra, rb = a.mcmi_fetch(3), b.mcmi_fetch(3)
        assert ra[0] == 3 and ra == rb, a.err()
        ra, rb = a.predict(XALL[150:170]), b.predict(XALL[150:170])
        assert ra[0] == 0 and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
        assert a.revoke([more[0]]) == 0 and b.revoke([more[0]]) == 0                 # a workspace of the new capacity
        assert_same_state(a, b)
        # 48 is a capacity like any other: 49 labels do not fit, 37 is rounded up to 48
        assert a.reserve(37) == 0 and a.try_update(list(range(141, 150)) + list(range(111, 118)) + list(range(82, 95))) == -12
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ scratch that was in use when the shape changed
# 40 unlabelled candidates below row 150 that no case removes, and a change-estimation subset of 7: five of them, two others
_FREE = [i for i in range(1, 149) if i not in LABELLED and i != 88]
CAND = _FREE[::3][:40]
SUBSET = CAND[2::9][:5] + [i for i in _FREE if i not in CAND][5:7]
GONE = [0, 88, 149, 160, 186]                             # unlabelled, outside CAND and SUBSET
POINTS = XALL[187:192]                                    # rows of no context


def _session(c, num):
    """The calls that grow every lazily grown buffer of a context, `num` giving the context's number of every row of XALL:
    the candidate buffers, the scorers' workspace and the stream tables (lattice scorer, k = 4), the batch state at kmax = 9
    and the subset staging (general scorer), the MCMI block with its covariances and workspace (k = 5), the top-k and
    predict scratch, the workspace of ital_gp_remove.  The last label is taken back and given again, which keeps the
    insertion order.  Returns the index lists and the float64 arrays."""
    cand, subset, last = num[CAND], num[SUBSET], int(num[LABELLED[-1]])
    lists = [c.fetch_list(4, cand), c.fetch_list(2, cand, subset), c.mcmi_fetch(5, cand)]
    assert [r[0] for r in lists] == [4, 2, 5], (c.err(), lists)
    rc, top = c.top_results(10)
    assert rc == 0, c.err()
    rc, mean, var = c.predict(POINTS)
    assert rc == 0, c.err()
    assert c.revoke([last]) == 0, c.err()
    c.update([last], YALL[LABELLED[-1:]])
    return [r[1] for r in lists] + [top], [mean, var]


@pytest.mark.parametrize("case", ["reserve", "add_rows", "remove_rows", "remove_rows_labelled"])
def test_scratch_in_use_survives_a_change_of_shape(lib, case):
    """Context a has used every lazily grown buffer when its capacity or its rows change, and uses them all again; context b
    makes the same calls at the final shape from the start, so its scratch is never dropped.  Explicit candidate lists keep
    both at the same position of mvndst's stream, which advances by the length of the list.  A labelled row's removal does
    not equal a fresh factorisation in bits: there b takes the label back first (the equality stated above)."""
    from ital_amd.device_data import removal_map
    before_a = before_b = after = np.arange(len(XALL))    # the numbering of XALL's rows in a / b before the call, in both after
    if case == "reserve":
        a, b = Ctx(lib, X, capacity=32), Ctx(lib, X, capacity=64)
    elif case == "add_rows":
        a, b = Ctx(lib, X), Ctx(lib, XALL[:187])
    elif case == "remove_rows":
        after = before_b = removal_map(187, GONE)
        a, b = Ctx(lib, XALL[:187]), Ctx(lib, np.delete(XALL[:187], GONE, 0))
    else:
        after = removal_map(N, REMOVED)
        a, b = Ctx(lib, X), Ctx(lib, X)
    try:
        for c, num in ((a, before_a), (b, before_b)):
            c.update(num[BLOCK_A], YALL[BLOCK_A])
            c.update(num[BLOCK_B], YALL[BLOCK_B])
            _session(c, num)
        if case == "reserve":
            assert a.reserve(64) == 0, a.err()
        elif case == "add_rows":
            assert a.add_rows(XALL[150:187]) == 0, a.err()
        elif case == "remove_rows":
            assert a.remove_rows(GONE) == 0, a.err()
        else:
            assert a.remove_rows(REMOVED) == 0, a.err()
            assert b.revoke([7]) == 0 and b.remove_rows(REMOVED) == 0, b.err()
        (lists_a, arrays_a), (lists_b, arrays_b) = _session(a, after), _session(b, after)
        assert lists_a == lists_b
        for va, vb in zip(arrays_a, arrays_b):
            assert np.array_equal(va, vb), np.abs(va - vb).max()
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ scoring candidates
def _grid9(noise_of_last):
    ls = [0.2, 0.4, 0.6, 0.8, 1.0, 1.3, 1.7, 2.2, 0.8]
    p = np.array([[v, 1.0, 1e-6] for v in ls])
    p[2, 1], p[5, 2] = 0.6, 1e-3
    p[8, 2] = noise_of_last
    return p


def test_evidence_equals_the_python_learner(lib):
    from ital_amd import ITAL
    Xd, ids, y = _twins()
    L = ITAL(Xd, length_scale=LS, device="cuda:0")
    L.update({i: y[j] for j, i in enumerate(ids[:16])})
    L.update({i: y[16 + j] for j, i in enumerate(ids[16:])})
    order = [int(i) for i in L.gp.ind]
    a = Ctx(lib, Xd)
    try:
        a.update(order, np.asarray(L.gp.y, dtype=np.float64))
        params = _grid9(0.0)                              # the last candidate: twins without noise
        want = L.gp.evidence(params)
        state = a.predict_stored()
        rc, scores, ok = a.evidence(params)
        assert rc == 0, a.err()
        assert np.array_equal(ok, want["ok"].astype(np.int32))
        assert ok[:8].all() and ok[8] == 0
        assert scores[8, 0] == -np.inf and scores[8, 1] == -np.inf and scores[8, 2] == np.inf
        for j, name in enumerate(("lml", "loo_logp", "loo_mse")):
            assert np.array_equal(scores[:, j], want[name]), name
        assert np.isfinite(scores[:8]).all()
        # a candidate alone, or at another position, has the same bits; the context is as it was
        rc, one, ok1 = a.evidence(params[3])
        assert rc == 0 and ok1[0] == 1 and np.array_equal(one[0], scores[3])
        after = a.predict_stored()
        assert np.array_equal(state[0], after[0]) and np.array_equal(state[1], after[1])
        assert a.fetch(0)[0] == 0
    finally:
        a.close()


def test_grid_search_equals_tune_params(lib):
    grid = [0.2, 0.35, 0.5, 0.65, 0.8, 1.0, 1.25, 1.6, 2.0]
    L = _learner()
    best, score = L.tune_params(OrderedDict((("length_scale", grid),)), criterion="lml")
    a = Ctx(lib, X).label()
    try:
        rc, scores, ok = a.evidence([[v, 1.0, 1e-6] for v in grid])
        assert rc == 0 and ok.all(), a.err()
        g = int(np.argmax(scores[:, 0]))                  # (first maximum, the tie rule of the alternating search)
        assert grid[g] == best["length_scale"] and scores[g, 0] == score
        assert grid[g] != LS
        assert a.set_params(length_scale=grid[g]) == 0, a.err()
        mean, var = a.predict_stored()
        lm, lv = L.gp.predict_stored(cov_mode="diag")
        assert np.array_equal(mean, np.asarray(lm)) and np.array_equal(var, np.asarray(lv))
        rc, picks = a.fetch(4)
        assert rc == 4 and picks == _learner_fetch(L)
    finally:
        a.close()


# ------------------------------------------------------------------ refusals
def test_error_codes(lib):
    a = Ctx(lib, X)
    h = ctypes.c_void_p()
    assert lib.ital_ctx_create(N, D, LS, 1.0, 1e-6, 64, 0, 1, None, ctypes.byref(h)) == 0
    buf = np.zeros(32)
    try:
        # a context without ital_ctx_fit
        assert lib.ital_ctx_reserve(h, 128, None) == -22 and "ital_ctx_fit" in a.err()
        assert lib.ital_ctx_add_rows(h, buf.ctypes.data, 1, 0, None) == -22 and "ital_ctx_fit" in a.err()
        assert lib.ital_ctx_remove_rows(h, _i64([1]).ctypes.data, 1, None, None) == -22 and "ital_ctx_fit" in a.err()
        assert lib.ital_ctx_set_params(h, 1.0, 1.0, 0.1, None) == -22 and "ital_ctx_fit" in a.err()
        assert lib.ital_ctx_evidence(h, buf.ctypes.data, 1, buf.ctypes.data, buf.ctypes.data, None) == -22 and "ital_ctx_fit" in a.err()
        # before the first label
        assert a.evidence([[1.0, 1.0, 1e-6]])[0] == -22 and "fitted relevance model" in a.err()
        a.label()
        state = a.predict_stored()
        assert a.reserve((1 << 20) + 1) == -22 and "2^20" in a.err()
        assert a.add_rows(XALL[150:160], k=-1) == -22 and "negative count" in a.err()
        assert a.add_rows(None, 3) == -22 and "rows missing" in a.err()
        for bad, why in (([150], "outside the data"), ([-1], "outside the data"), ([4, 9, 4], "named twice"),
                         (list(range(N)), "no row would be left")):
            assert a.remove_rows(bad) == -22 and why in a.err(), bad
        assert lib.ital_ctx_remove_rows(a.h, None, 2, None, None) == -22 and "idx missing" in a.err()
        assert lib.ital_ctx_remove_rows(a.h, _i64([1]).ctypes.data, 0, None, None) == -22 and "fewer than one" in a.err()
        for bad in (dict(length_scale=0.0), dict(length_scale=-1.0), dict(var=0.0), dict(var=-2.0), dict(noise=-1e-9)):
            assert a.set_params(**bad) == -22 and "must be positive" in a.err(), bad
        assert lib.ital_ctx_evidence(a.h, buf.ctypes.data, 0, buf.ctypes.data, buf.ctypes.data, None) == -22
        assert "fewer than one candidate" in a.err()
        for args in ((None, 1, buf.ctypes.data, buf.ctypes.data), (buf.ctypes.data, 1, None, buf.ctypes.data),
                     (buf.ctypes.data, 1, buf.ctypes.data, None)):
            assert lib.ital_ctx_evidence(a.h, *args, None) == -22 and "NULL pointer" in a.err()
        after = a.predict_stored()
        assert np.array_equal(state[0], after[0]) and np.array_equal(state[1], after[1])
        assert lib.ital_ctx_local_rows(a.h, None) == N and a.fetch(4)[0] == 4
    finally:
        a.close()
        assert lib.ital_ctx_destroy(h) == 0
    # rows cannot arrive or leave on several ranks (rank 0 of 2; the communicator is never used by these calls)
    s = Ctx(lib, X[:75], rank=0, world=2, comm=ctypes.c_void_p(1), n_total=N)
    try:
        assert s.add_rows(XALL[150:160]) == -38 and "cannot grow" in s.err()
        assert s.remove_rows([3]) == -38 and "cannot shrink" in s.err()
        assert s.add_rows(XALL[:0]) == 0
    finally:
        s.close()


# ------------------------------------------------------------------ several ranks
def _rank_session(lib, rank, world, comm):
    from ital_amd import sharding
    row0, row1 = sharding.row_range(N, world, rank)
    ctx = Ctx(lib, X[row0:row1], capacity=16, rank=rank, world=world, comm=comm, n_total=N)
    try:
        ctx.update(LABELLED[:10])
        assert ctx.try_update(LABELLED[10:]) == -12
        assert ctx.reserve(48) == 0, ctx.err()
        ctx.update(LABELLED[10:])
        assert ctx.set_params(**NEW) == 0, ctx.err()
        rc, picks = ctx.fetch(4)
        assert rc == 4, ctx.err()
        return picks, ctx.add_rows(XALL[150:160])
    finally:
        ctx.close()


def _rank_worker(rank, world, port, mode, out):
    dev, group = _ranks.join(rank, world, port, mode)
    try:
        from ital_amd import _lib, sharding
        lib = _lib.load()
        comm = sharding.raw_comm(group, dev)
        if comm is None:
            out[rank] = ("no raw communicator", sharding.raw_comm_reason(group, dev))
            return
        res = _rank_session(lib, rank, world, comm)
        torch.cuda.synchronize()
        out[rank] = ("ok",) + res
    finally:
        _ranks.leave(group)


@pytest.mark.parametrize("world,mode", [(1, "rccl1"), (2, "rccl")])
def test_reserve_and_set_params_on_several_ranks(lib, world, mode):
    """Every rank makes the same calls; the picks are those of one rank without a communicator.  One rank with a
    communicator (the exchange path of every greedy step) runs wherever RCCL loads; two ranks need two devices."""
    picks, grow = _rank_session(lib, 0, 1, None)
    assert grow == 0
    res = _ranks.spawn(_rank_worker, world, mode)
    assert all(r[0] == "ok" for r in res), res
    assert all(r[1] == picks for r in res)
    assert all(r[2] == (0 if world == 1 else -38) for r in res)
