"""Host side of remove_data() (no device): the index arithmetic of ital_amd/device_data.py against np.delete, the C declarations
of include/ital_compact.h against their bindings, every refusal of the two entry points (decided before any HIP call), the
store's change log on a stub that records calls instead of launching, and the refusals of the learner that need no GPU.  The
GPU side is tests/test_gpu_remove_data.py."""
import ctypes
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

COMPACT = ["ital_compact_rows", "ital_compact_cols"]


# ------------------------------------------------------------------------------------------------ index arithmetic
def _np_delete_map(n, ids):
    """The map np.delete defines: tag every row with its old index, delete, read the new positions off."""
    left = np.delete(np.arange(n), ids, axis=0)
    out = np.full(n, -1, dtype=np.int64)
    out[left] = np.arange(len(left))
    return out


@pytest.mark.parametrize("n", [1, 2, 65])
def test_one_removal_equals_np_delete(n):
    from ital_amd.device_data import keep_indices, normalize_ids, removal_map
    rng = np.random.default_rng(n)
    cases = [[], [0], [n - 1], [-1], list(range(0, n, 2)), [0, 0, n - 1, -n], list(rng.permutation(n)[: n // 3])]
    for ids in cases:
        removed = normalize_ids(ids, n)
        assert removed == sorted(set(int(i) % n for i in ids))
        got = removal_map(n, removed)
        assert got.dtype == np.int64 and got.shape == (n,)
        assert np.array_equal(got, _np_delete_map(n, removed)), ids
        assert np.array_equal(keep_indices(n, removed), np.delete(np.arange(n), removed))
    assert np.array_equal(removal_map(n, []), np.arange(n))                 # the identity for an empty list
    for bad in ([n], [-n - 1], [0, n + 3]):
        with pytest.raises(IndexError):
            normalize_ids(bad, n)


@pytest.mark.parametrize("n", [1, 2, 65])
def test_three_composed_events_equal_np_delete_on_tagged_rows(n):
    from ital_amd.device_data import compose_maps, log_index_map, normalize_ids, removal_map
    rng = np.random.default_rng(100 + n)
    tags = np.arange(n)                                  # rows tagged with their first index; appended rows get -1
    first = normalize_ids(rng.permutation(n)[: n // 2], n)
    tags1 = np.delete(tags, first)
    k = 5
    tags2 = np.concatenate((tags1, np.full(k, -1)))
    second = normalize_ids(rng.permutation(len(tags2))[: len(tags2) // 2], len(tags2))
    tags3 = np.delete(tags2, second)
    events = [("remove", first, n), ("append", k), ("remove", second, len(tags2))]
    got, n_after = log_index_map(events, n)
    want = np.full(n, -1, dtype=np.int64)
    for new, old in enumerate(tags3):
        if old >= 0:
            want[old] = new
    assert n_after == len(tags3) and np.array_equal(got, want)
    assert np.array_equal(got, compose_maps(removal_map(n, first), removal_map(len(tags2), second)))
    ident, same = log_index_map([], n)
    assert same == n and np.array_equal(ident, np.arange(n))
    assert np.array_equal(log_index_map([("append", 3)], n)[0], np.arange(n))
    with pytest.raises(ValueError):
        log_index_map([("remove", [0], n + 1)], n)


@pytest.mark.parametrize("n", [1, 2, 65])
def test_id_sets_are_remapped_by_bisection(n):
    from ital_amd.device_data import normalize_ids, remap_ids, removal_map
    rng = np.random.default_rng(200 + n)
    removed = normalize_ids(rng.permutation(n)[: n // 3], n)
    ids = set(int(i) for i in rng.permutation(n)[: max(1, n // 2)]) | set(removed[:2])      # some of them removed
    m = removal_map(n, removed)
    got = remap_ids(ids, removed)
    assert isinstance(got, set) and got == set(int(m[i]) for i in ids if m[i] >= 0)
    assert remap_ids(ids, []) == ids and remap_ids([], removed) == set()
    assert remap_ids([n + 4], removed) == {n + 4 - len(removed)}            # a query row moves down by all of them
    if removed:
        assert remap_ids([removed[0]], removed) == set()


# ------------------------------------------------------------------------------------------------ the C ABI
def _ctype_of(decl):
    decl = decl.strip()
    if "*" in decl:
        return ctypes.c_void_p
    base = " ".join(w for w in decl.split()[:-1] if w != "const")
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "hipStream_t": ctypes.c_void_p}[base]


def test_compact_declarations_equal_bindings_and_are_exported():
    from ital_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "ital_compact.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", code)) == set(COMPACT) == set(_lib.COMPACT_SIGNATURES)
    for name in dir(_lib):
        if name.endswith("SIGNATURES") and name != "COMPACT_SIGNATURES":
            assert not set(COMPACT) & set(getattr(_lib, name)), name
    for name in COMPACT:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        res, args = _lib.COMPACT_SIGNATURES[name]
        assert res is ctypes.c_int and [_ctype_of(a) for a in m.group(1).split(",")] == args, name
    raw = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    for name in COMPACT:
        assert hasattr(raw, name), name
        assert list(getattr(lib, name).argtypes) == _lib.COMPACT_SIGNATURES[name][1]
    assert "compact.hip" in build.SOURCES
    for untouched in ("ital_hip.h", "ital_ctx.h", "ital_ingest.h", "ital_rows.h"):
        assert "ital_compact" not in open(os.path.join(ROOT, "include", untouched)).read()


# fake pointers that are never followed: every case below is decided before any HIP call
ROWS_OK = dict(X=1 << 20, xnorm=2 << 20, n=20, ldx=16, xtype=0, keep=3 << 20, n_keep=10, X_dst=4 << 20, xnorm_dst=5 << 20,
               status=None)
COLS_OK = dict(V=1 << 20, ldv=32, m=4, mu=2 << 20, s2=3 << 20, n=20, keep=4 << 20, n_keep=10, V_dst=5 << 20, ldv_dst=16,
               v_rows_dst=16, mu_dst=6 << 20, s2_dst=7 << 20, status=None)


def _rows(lib, **kw):
    a = dict(ROWS_OK)
    a.update(kw)
    return lib.ital_compact_rows(a["X"], a["xnorm"], a["n"], a["ldx"], a["xtype"], a["keep"], a["n_keep"], a["X_dst"],
                                 a["xnorm_dst"], a["status"], None)


def _cols(lib, **kw):
    a = dict(COLS_OK)
    a.update(kw)
    return lib.ital_compact_cols(a["V"], a["ldv"], a["m"], a["mu"], a["s2"], a["n"], a["keep"], a["n_keep"], a["V_dst"],
                                 a["ldv_dst"], a["v_rows_dst"], a["mu_dst"], a["s2_dst"], a["status"], None)


ROWS_REFUSED = {
    "null_X": dict(X=None), "null_xnorm": dict(xnorm=None), "null_keep": dict(keep=None), "null_X_dst": dict(X_dst=None),
    "null_xnorm_dst": dict(xnorm_dst=None), "negative_n": dict(n=-1, n_keep=0), "negative_n_keep": dict(n_keep=-1),
    "n_keep_above_n": dict(n_keep=21), "ldx_no_multiple_of_16": dict(ldx=24), "unknown_xtype_high": dict(xtype=4),
    "unknown_xtype_negative": dict(xtype=-1), "X_unaligned": dict(X=(1 << 20) + 8), "X_dst_unaligned": dict(X_dst=(4 << 20) + 8),
    # 20 rows of 16 doubles are 2560 B: the destination starts inside / the source starts inside the destination / the same
    "X_dst_inside_X": dict(X_dst=(1 << 20) + 1280), "X_inside_X_dst": dict(X_dst=(1 << 20) - 128), "X_in_place": dict(X_dst=1 << 20),
    "xnorm_dst_inside_xnorm": dict(xnorm_dst=(2 << 20) + 80), "xnorm_in_place": dict(xnorm_dst=2 << 20),
}

COLS_REFUSED = {
    "null_V": dict(V=None), "null_mu": dict(mu=None), "null_s2": dict(s2=None), "null_keep": dict(keep=None),
    "null_V_dst": dict(V_dst=None), "null_mu_dst": dict(mu_dst=None), "null_s2_dst": dict(s2_dst=None),
    "negative_n": dict(n=-1, n_keep=0), "negative_n_keep": dict(n_keep=-1), "n_keep_above_n": dict(n_keep=21),
    "ldv_dst_no_multiple_of_16": dict(ldv_dst=24), "ldv_dst_below_n_keep": dict(ldv_dst=0), "ldv_dst_below_n_keep_32": dict(
        n=40, ldv=48, n_keep=33, ldv_dst=32), "negative_m": dict(m=-1), "v_rows_dst_below_m": dict(v_rows_dst=3),
    "ldv_below_n": dict(ldv=16),
    # V holds (3 * 32 + 20) * 8 = 928 B, V_dst 16 * 16 * 8 = 2048 B
    "V_dst_inside_V": dict(V_dst=(1 << 20) + 920), "V_inside_V_dst": dict(V_dst=(1 << 20) - 2040), "V_in_place": dict(V_dst=1 << 20),
    "mu_dst_inside_mu": dict(mu_dst=(2 << 20) + 152), "mu_in_place": dict(mu_dst=2 << 20), "s2_in_place": dict(s2_dst=3 << 20),
    "s2_inside_s2_dst": dict(s2_dst=(3 << 20) - 72),
}


@pytest.mark.parametrize("case", sorted(ROWS_REFUSED))
def test_compact_rows_refuses_before_any_hip_call(case):
    from ital_amd import _lib
    lib = _lib.load()
    assert _rows(lib, **ROWS_REFUSED[case]) == -22, case
    assert "ital_compact_rows" in lib.ital_last_error().decode(), case


@pytest.mark.parametrize("case", sorted(COLS_REFUSED))
def test_compact_cols_refuses_before_any_hip_call(case):
    from ital_amd import _lib
    lib = _lib.load()
    assert _cols(lib, **COLS_REFUSED[case]) == -22, case
    assert "ital_compact_cols" in lib.ital_last_error().decode(), case


def test_nothing_to_do_returns_0_without_a_launch():
    from ital_amd import _lib
    lib = _lib.load()
    # no survivor: checked, then 0 without a launch -- also with no buffers behind it
    assert _rows(lib, n_keep=0) == 0
    assert _rows(lib, n=0, n_keep=0, X=None, xnorm=None, keep=None, X_dst=None, xnorm_dst=None) == 0
    assert _rows(lib, n_keep=0, ldx=24) == -22
    assert _cols(lib, n=0, n_keep=0, m=0, v_rows_dst=0, ldv_dst=0, V=None, mu=None, s2=None, keep=None, V_dst=None,
                 mu_dst=None, s2_dst=None) == 0
    # m == 0 needs no V
    assert _cols(lib, n_keep=0, m=0, v_rows_dst=0, V=None, V_dst=None) == 0


# ------------------------------------------------------------------------------------------------ the store's change log
def _stub_store(n, d=3):
    """A DeviceData without a device: the two methods that launch are replaced by ones that record their calls."""
    torch = pytest.importorskip("torch")
    from ital_amd.device_data import DeviceData
    s = object.__new__(DeviceData)
    s.n, s.d, s.ldx, s.capacity, s.storage, s.device = n, d, 16, 4 * n, torch.float64, "cpu"
    s.log, s.epoch, s.calls = [], 0, []

    def write(t):
        s.calls.append(("write", int(t.shape[0])))
        s.n += int(t.shape[0])

    def compact(keep):
        s.calls.append(("compact", keep.tolist()))
        s.n = len(keep)
    s._write, s._compact = write, compact
    return s


def test_the_store_logs_appends_and_removals_with_epochs():
    from ital_amd.device_data import log_index_map
    s = _stub_store(6)
    assert (s.epoch, s.log) == (0, [])
    m = s.remove([4, 1, 1, -1])
    assert m.tolist() == [0, -1, 1, 2, -1, -1] and m.dtype == np.int64
    assert (s.n, s.epoch, s.log) == (3, 1, [("remove", [1, 4, 5], 6)])
    assert s.calls == [("compact", [0, 2, 3])]
    assert s.append(np.zeros((2, 3))) == 2
    assert (s.n, s.epoch, s.log[-1]) == (5, 2, ("append", 2))
    assert s.remove([]).tolist() == [0, 1, 2, 3, 4] and s.append(np.zeros((0, 3))) == 0      # no-ops: no entry
    assert s.epoch == 2 and len(s.log) == 2
    s.remove(iter([0]))
    assert (s.n, s.epoch, s.log[-1]) == (4, 3, ("remove", [0], 5))
    assert [c[0] for c in s.calls] == ["compact", "write", "compact"]
    # the log is a few integers per event, and describes what happened to the first six rows
    got, n_after = log_index_map(s.log, 6)
    assert n_after == s.n and got.tolist() == [-1, -1, 0, 1, -1, -1]
    # refusals change nothing
    before = (s.n, s.epoch, list(s.log), list(s.calls))
    with pytest.raises(IndexError):
        s.remove([4])
    with pytest.raises(IndexError):
        s.remove([0, -5])
    with pytest.raises(ValueError):
        s.remove([0, 1, 2, 3])
    with pytest.raises(ValueError):
        s.append(np.zeros((2, 4)))
    assert (s.n, s.epoch, s.log, s.calls) == before


# ------------------------------------------------------------------------------------------------ the learners
def _bare_ital(**kw):
    """An ITAL instance without a device (only the option logic is exercised)."""
    from ital_amd.ital import ITAL
    L = object.__new__(ITAL)
    for k, v in kw.items():
        setattr(L, k, v)
    return L


def test_several_ranks_cannot_shrink():
    L = _bare_ital(world=2, data=np.zeros((5, 3)))
    with pytest.raises(NotImplementedError, match="cannot shrink"):
        L.remove_data([1])
    from ital_amd.gp import GaussianProcess
    g = object.__new__(GaussianProcess)
    g.world, g.store, g.X_host = 2, None, np.zeros((5, 3))
    with pytest.raises(NotImplementedError, match="cannot shrink"):
        g.drop_rows([1])


def test_every_learner_has_remove_data():
    import ital_amd
    from ital_amd import baselines
    from ital_amd.retrieval_base import ActiveRetrievalBase
    assert callable(ital_amd.GaussianProcess.drop_rows) and callable(ital_amd.DeviceData.remove)
    for cls in (ital_amd.ITAL, ital_amd.MCMI_min, ital_amd.AdaptAL, baselines.BorderlineSampling, baselines.EntropySampling):
        assert cls.remove_data is ActiveRetrievalBase.remove_data
        assert isinstance(cls.last_index_map, property)
