"""Host side of whitening a row range against the whole labelled set (no device): the C declarations of
include/ital_rewhiten.h against their bindings, the descriptor's fields, the argument checks that come before any HIP call,
and the learner-level refusals of add_data() that need no GPU.  The GPU side is tests/test_gpu_rewhiten.py."""
import ctypes
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

REWHITEN = ["ital_whiten_rows", "ital_whiten_rows_chunk"]


def test_rewhiten_declarations_equal_bindings_and_are_exported():
    from ital_amd import _lib
    header = open(os.path.join(ROOT, "include", "ital_rewhiten.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", code))
    assert declared == set(REWHITEN) == set(_lib.REWHITEN_SIGNATURES), declared ^ set(_lib.REWHITEN_SIGNATURES)
    for other in (_lib.SIGNATURES, _lib.CTX_SIGNATURES, _lib.DENSE_SIGNATURES, _lib.ADAPT_SIGNATURES, _lib.REVOKE_SIGNATURES):
        assert not declared & set(other)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in REWHITEN:
        assert hasattr(raw, name), name
    lib = _lib.load()
    for name, (res, args) in _lib.REWHITEN_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert re.search(r"\bint\s+ital_whiten_rows\s*\(\s*const\s+ital_rewhiten_desc\s*\*\s*desc,\s*hipStream_t\s+stream\)\s*;", code)
    assert _lib.REWHITEN_SIGNATURES["ital_whiten_rows"] == (ctypes.c_int, [ctypes.POINTER(_lib.ItalRewhitenDesc), ctypes.c_void_p])
    # the two public headers the issue leaves untouched do not know the new entry point
    for untouched in ("ital_hip.h", "ital_ctx.h"):
        assert "ital_whiten_rows" not in open(os.path.join(ROOT, "include", untouched)).read()
    from ital_amd import build
    assert "rewhiten.hip" in build.SOURCES


def test_rewhiten_desc_fields_follow_the_header():
    """Same field names in the same order as the struct in the header, pointers as pointers, scalars by their C type."""
    from ital_amd import _lib
    header = open(os.path.join(ROOT, "include", "ital_rewhiten.h")).read()
    body = re.search(r"typedef struct ital_rewhiten_desc \{(.*?)\} ital_rewhiten_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.search(r"([A-Za-z_0-9]+)$", d).group(1) for d in fields]
    assert names == [f[0] for f in _lib.ItalRewhitenDesc._fields_]
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for d, (name, ctype) in zip(fields, _lib.ItalRewhitenDesc._fields_):
        assert ctype is (ctypes.c_void_p if "*" in d else kinds[d.split()[0]]), name


def _desc(**kw):
    from ital_amd import _lib
    d = _lib.ItalRewhitenDesc()
    base = dict(X=64, n_rows=20, ldx=16, XT=64, XTn=64, L=64, ldl=16, alpha=64, m=8, var=1.0, length_scale=0.5, xnorm=64,
                V=64, ldv=32, v_rows=16, mu=64, s2=64, chunk=0)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def test_entry_point_refuses_bad_arguments_without_a_device():
    """-22 before any HIP call: NULL pointers, ldx % 16 != 0, ldl < m, ldv < n_rows, negative sizes (and the other shapes
    the kernel relies on)."""
    from ital_amd import _lib
    lib = _lib.load()

    def refused(rc):
        assert rc == -22
        assert "ital_whiten_rows" in lib.ital_last_error().decode()

    assert lib.ital_whiten_rows_chunk() in (32, 64, 128)
    refused(lib.ital_whiten_rows(None, None))
    for bad in (dict(X=None), dict(xnorm=None), dict(V=None), dict(mu=None), dict(s2=None), dict(XT=None), dict(XTn=None),
                dict(L=None), dict(alpha=None), dict(ldx=0), dict(ldx=-16), dict(ldx=8), dict(ldx=24), dict(ldl=7),
                dict(ldv=19), dict(n_rows=-1), dict(m=-1), dict(v_rows=7), dict(v_rows=-1), dict(chunk=16), dict(chunk=48),
                dict(chunk=-64), dict(chunk=256)):
        refused(lib.ital_whiten_rows(ctypes.byref(_desc(**bad)), None))
    # nothing to do: checked, then a no-op without a HIP call (also with no labelled set behind it)
    assert lib.ital_whiten_rows(ctypes.byref(_desc(n_rows=0)), None) == 0
    assert lib.ital_whiten_rows(ctypes.byref(_desc(n_rows=0, m=0, XT=None, XTn=None, L=None, alpha=None, ldl=0)), None) == 0


def test_learners_have_add_data_and_set_params():
    import ital_amd
    from ital_amd import baselines
    from ital_amd.retrieval_base import ActiveRetrievalBase
    assert callable(ital_amd.GaussianProcess.extend) and callable(ital_amd.GaussianProcess.set_params)
    for cls in (ital_amd.ITAL, ital_amd.MCMI_min, ital_amd.AdaptAL, baselines.BorderlineSampling, baselines.EntropySampling):
        assert cls.add_data is ActiveRetrievalBase.add_data and cls.set_params is ActiveRetrievalBase.set_params


def test_add_data_refusals_at_the_learner_level():
    """What add_data() decides before it touches the GP: an empty array is a no-op, another column count a ValueError, a
    sharded collection a NotImplementedError that says why (a learner needs a device to be constructed: this one is bare)."""
    from ital_amd.retrieval_base import ActiveRetrievalBase
    L = ActiveRetrievalBase.__new__(ActiveRetrievalBase)
    L.data, L.gp, L.world = np.zeros((5, 3)), None, 2
    assert L.add_data(np.zeros((0, 3))) is L and L.add_data([]) is L
    with pytest.raises(ValueError):
        L.add_data(np.zeros((2, 4)))
    with pytest.raises(ValueError):
        L.add_data(np.zeros(3))
    with pytest.raises(NotImplementedError, match="row sharding cannot grow"):
        L.add_data(np.zeros((2, 3)))
    assert L.data.shape == (5, 3)
