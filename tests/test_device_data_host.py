"""Host side of DeviceData and ital_ingest_rows (no device): the C declaration of include/ital_ingest.h against its binding,
the argument checks that come before any HIP call, the dtype mapping, what as_rows() makes of the input kinds, and the
refusals that need no GPU.  The GPU side is tests/test_gpu_device_data.py."""
import ctypes
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

INGEST = ["ital_ingest_rows"]


def test_ingest_declaration_equals_binding_and_is_exported():
    from ital_amd import _lib
    header = open(os.path.join(ROOT, "include", "ital_ingest.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", code))
    assert declared == set(INGEST) == set(_lib.INGEST_SIGNATURES), declared ^ set(_lib.INGEST_SIGNATURES)
    others = [getattr(_lib, name) for name in dir(_lib) if name.endswith("SIGNATURES") and name != "INGEST_SIGNATURES"]
    assert len(others) >= 7
    for other in others:
        assert not declared & set(other)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in INGEST:
        assert hasattr(raw, name), name
    lib = _lib.load()
    for name, (res, args) in _lib.INGEST_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert re.search(r"\bint\s+ital_ingest_rows\s*\(\s*const\s+void\s*\*\s*src,\s*int\s+dtype,\s*int64_t\s+n,\s*int\s+d,\s*"
                     r"int64_t\s+ld_src,\s*double\s*\*\s*X,\s*int\s+ldx,\s*double\s*\*\s*xnorm,\s*hipStream_t\s+stream\)\s*;", code)
    c = ctypes
    assert _lib.INGEST_SIGNATURES["ital_ingest_rows"] == (c.c_int, [c.c_void_p, c.c_int, c.c_int64, c.c_int, c.c_int64, c.c_void_p,
                                                                    c.c_int, c.c_void_p, c.c_void_p])
    for macro, value in (("ITAL_INGEST_F64", _lib.INGEST_F64), ("ITAL_INGEST_F32", _lib.INGEST_F32),
                         ("ITAL_INGEST_F16", _lib.INGEST_F16), ("ITAL_INGEST_BF16", _lib.INGEST_BF16)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), code), macro
    for untouched in ("ital_hip.h", "ital_ctx.h"):
        assert "ital_ingest" not in open(os.path.join(ROOT, "include", untouched)).read()
    from ital_amd import build
    assert "ingest.hip" in build.SOURCES
    import ital_amd
    assert "DeviceData" in ital_amd.__all__
    from ital_amd.device_data import DeviceData
    assert ital_amd.DeviceData is DeviceData


def _call(lib, **kw):
    # fake pointers that are never followed: every case below is decided before any HIP call
    a = dict(src=4096, dtype=1, n=20, d=10, ld_src=10, X=8192, ldx=16, xnorm=16384)
    a.update(kw)
    return lib.ital_ingest_rows(a["src"], a["dtype"], a["n"], a["d"], a["ld_src"], a["X"], a["ldx"], a["xnorm"], None)


def test_entry_point_refuses_bad_arguments_without_a_device():
    from ital_amd import _lib
    lib = _lib.load()
    for bad in (dict(src=None), dict(X=None), dict(xnorm=None), dict(n=-1), dict(d=0), dict(d=-3), dict(ldx=24), dict(ldx=8),
                dict(ldx=0), dict(d=17), dict(d=33, ldx=32, ld_src=40), dict(ld_src=9), dict(ld_src=0), dict(ld_src=-10),
                dict(dtype=-1), dict(dtype=4), dict(dtype=0, src=4100), dict(dtype=1, src=4098), dict(dtype=2, src=4097),
                dict(dtype=3, src=4097), dict(X=8200), dict(xnorm=16388)):
        assert _call(lib, **bad) == -22, bad
        assert "ital_ingest_rows" in lib.ital_last_error().decode(), bad
    # nothing to do: checked, then 0 without a launch -- also with no buffers behind it
    assert _call(lib, n=0) == 0
    assert _call(lib, n=0, src=None, X=None, xnorm=None) == 0
    assert _call(lib, n=0, ldx=24) == -22


def test_dtype_codes():
    torch = pytest.importorskip("torch")
    from ital_amd import _lib
    from ital_amd.device_data import DTYPE_CODES, dtype_code
    assert (_lib.INGEST_F64, _lib.INGEST_F32, _lib.INGEST_F16, _lib.INGEST_BF16) == (0, 1, 2, 3)
    assert DTYPE_CODES == {torch.float64: 0, torch.float32: 1, torch.float16: 2, torch.bfloat16: 3}
    assert [dtype_code(t) for t in (torch.float64, torch.float32, torch.float16, torch.bfloat16)] == [0, 1, 2, 3]
    assert [dtype_code(t) for t in (np.float64, np.float32, np.float16, "f8", np.dtype("<f4"))] == [0, 1, 2, 0, 1]
    for other in (torch.int32, torch.int64, torch.uint8, torch.bool, torch.complex64, np.int16, np.uint8, np.complex128, bool):
        assert dtype_code(other) is None, other


def test_as_rows_keeps_type_and_stride_and_converts_the_rest():
    torch = pytest.importorskip("torch")
    from ital_amd.device_data import as_rows
    T = torch.arange(40 * 140, dtype=torch.float32).reshape(40, 140)
    for dt in (torch.float64, torch.float32, torch.float16, torch.bfloat16):
        t = as_rows(T.to(dt))
        assert t.dtype is dt and t.shape == (40, 140) and t.stride() == (140, 1)
    v = as_rows(T[:, 3:131])                                   # a row-strided view is read as it is
    assert v.data_ptr() == T[:, 3:131].data_ptr() and v.stride() == (140, 1) and v.shape == (40, 128)
    s = as_rows(T[:, ::2])                                     # an inner stride: made contiguous first
    assert s.stride() == (70, 1) and torch.equal(s, T[:, ::2])
    tr = as_rows(T.t())
    assert tr.stride() == (40, 1) and torch.equal(tr, T.t())
    e = as_rows(T[:1].expand(5, 140))                          # row stride 0
    assert e.stride() == (140, 1) and e.shape == (5, 140)
    i = as_rows(torch.arange(12, dtype=torch.int32).reshape(3, 4))
    assert i.dtype is torch.float64 and i[2, 3] == 11.0
    A = np.arange(30 * 20, dtype=np.float32).reshape(30, 20)
    for dt in (np.float64, np.float32, np.float16):
        t = as_rows(A.astype(dt))
        assert t.dtype is torch.from_numpy(np.zeros(1, dtype=dt)).dtype and t.stride() == (20, 1)
    assert as_rows(A).data_ptr() == A.ctypes.data              # no host copy of what already has the form
    assert as_rows(A[:, 2:9]).stride() == (20, 1)
    assert as_rows(A[::-1]).stride() == (20, 1) and as_rows(A[::-1])[0, 0] == A[-1, 0]
    assert as_rows(A.astype(np.int16)).dtype is torch.float64 and as_rows([[1, 2], [3, 4]]).dtype is torch.float64
    assert as_rows(A.astype(">f4")).dtype is torch.float64     # a byte order torch does not read
    ro = A.copy()
    ro.setflags(write=False)
    assert torch.equal(as_rows(ro), torch.from_numpy(A))
    for bad in (np.zeros(5), np.zeros((2, 3, 4)), torch.zeros(7), torch.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            as_rows(bad)
    for bad in (np.zeros((3, 2), dtype=np.complex128), torch.zeros((3, 2), dtype=torch.complex64)):
        with pytest.raises(TypeError):
            as_rows(bad)


def test_device_data_without_a_device_raises_as_the_gp_does(monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # also where there is one
    import ital_amd
    X = np.zeros((4, 3))
    with pytest.raises(RuntimeError, match="needs a HIP device") as gp_err:
        ital_amd.GaussianProcess(X, 1.0)
    with pytest.raises(RuntimeError, match="needs a HIP device") as dd_err:
        ital_amd.DeviceData(X)
    assert type(gp_err.value) is type(dd_err.value) is RuntimeError
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        ital_amd.ITAL(torch.zeros((4, 3)), length_scale=1.0)


def test_learners_have_sync_data_and_clone_and_refuse_them_on_their_own_rows():
    import ital_amd
    from ital_amd import baselines
    from ital_amd.retrieval_base import ActiveRetrievalBase
    assert callable(ital_amd.GaussianProcess.sync_data) and callable(ital_amd.GaussianProcess.clone)
    for cls in (ital_amd.ITAL, ital_amd.MCMI_min, ital_amd.AdaptAL, baselines.BorderlineSampling, baselines.EntropySampling):
        assert cls.sync_data is ActiveRetrievalBase.sync_data and cls.clone is ActiveRetrievalBase.clone
    L = ActiveRetrievalBase.__new__(ActiveRetrievalBase)       # a learner needs a device to be constructed: this one is bare
    L.data, L.gp, L.world = np.zeros((5, 3)), None, 1
    with pytest.raises(ValueError, match="DeviceData"):
        L.clone()
    with pytest.raises(ValueError, match="DeviceData"):
        L.sync_data()
    assert L._num_samples() == 5
