"""Host side of taking feedback back (no device): the C declarations of include/ital_revoke.h and ital_ctx_revoke against
their bindings, the argument checks that come before any HIP call, and the `appends` bookkeeping of GaussianProcess.remove
as a pure function.  The GPU side is tests/test_gpu_revoke.py."""
import ctypes
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

REVOKE = ["ital_gp_remove", "ital_gp_remove_workspace"]


def test_revoke_declarations_equal_bindings_and_are_exported():
    from ital_amd import _lib
    header = open(os.path.join(ROOT, "include", "ital_revoke.h")).read()
    declared = set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", header))      # the regex of the ital_hip.h export test
    assert declared == set(REVOKE) == set(_lib.REVOKE_SIGNATURES), declared ^ set(_lib.REVOKE_SIGNATURES)
    for other in (_lib.SIGNATURES, _lib.CTX_SIGNATURES, _lib.DENSE_SIGNATURES, _lib.ADAPT_SIGNATURES):
        assert not declared & set(other)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in REVOKE + ["ital_ctx_revoke"]:
        assert hasattr(raw, name), name
    lib = _lib.load()
    for name, (res, args) in _lib.REVOKE_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    ctx_header = open(os.path.join(ROOT, "include", "ital_ctx.h")).read()
    assert re.search(r"\bint\s+ital_ctx_revoke\s*\(\s*ital_ctx\s*\*\s*ctx,\s*const\s+int64_t\s*\*\s*idx,\s*int\s+c,\s*hipStream_t\s+stream\)\s*;",
                     ctx_header)
    assert _lib.CTX_SIGNATURES["ital_ctx_revoke"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p])
    # the untouched public header does not know the new entry points
    assert "ital_gp_remove" not in open(os.path.join(ROOT, "include", "ital_hip.h")).read()


def test_remove_desc_fields_follow_the_header():
    """Same field names in the same order as the struct in the header, pointers as pointers."""
    from ital_amd import _lib
    header = open(os.path.join(ROOT, "include", "ital_revoke.h")).read()
    body = re.search(r"typedef struct ital_remove_desc \{(.*?)\} ital_remove_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.search(r"([A-Za-z_0-9]+)$", d).group(1) for d in fields]
    assert names == [f[0] for f in _lib.ItalRemoveDesc._fields_]
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    for d, (name, ctype) in zip(fields, _lib.ItalRemoveDesc._fields_):
        assert ctype is (ctypes.c_void_p if "*" in d else kinds[d.split()[0]]), name


def _desc(**kw):
    from ital_amd import _lib
    d = _lib.ItalRemoveDesc()
    ws = int(_lib.load().ital_gp_remove_workspace(8))
    base = dict(XT=64, XTn=64, ldx=16, L=64, ldl=16, alpha=64, V=64, ldv=32, n=20, mu=64, s2=64, m=8, p=3, work=64,
                work_doubles=ws, status=64)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def test_entry_points_refuse_bad_arguments_without_a_device():
    """-22 before any HIP call: NULL, m <= 0, p outside [0, m), ldl < m (and the other shapes the kernels rely on)."""
    from ital_amd import _lib
    lib = _lib.load()

    def refused(rc, name="ital_gp_remove"):
        assert rc == -22
        assert name in lib.ital_last_error().decode()

    assert lib.ital_gp_remove_workspace(0) == 0 and lib.ital_gp_remove_workspace(-4) == 0
    assert lib.ital_gp_remove_workspace(1) == 8 + 4 + 1
    assert lib.ital_gp_remove_workspace(256) == 8 + 4 * 256 + 256 * 256
    refused(lib.ital_gp_remove(None, None))
    for bad in (dict(m=0), dict(m=-1), dict(p=-1), dict(p=8), dict(ldl=7), dict(ldx=0), dict(ldv=19), dict(ldv=33), dict(n=-1),
                dict(XT=None), dict(XTn=None), dict(L=None), dict(alpha=None), dict(work=None), dict(status=None), dict(V=None),
                dict(mu=None), dict(s2=None), dict(work_doubles=8 + 4 * 8 + 8 * 8 - 1), dict(work=72)):
        refused(lib.ital_gp_remove(ctypes.byref(_desc(**bad)), None))
    idx = (ctypes.c_int64 * 2)(1, 2)
    refused(lib.ital_ctx_revoke(None, idx, 2, None), "ital_ctx_revoke")


def test_appends_bookkeeping():
    from ital_amd.gp import appends_after_remove as f
    a = [1, 16, 16, 5]
    assert f(a, 0) == [0, 16, 16, 5] and a == [1, 16, 16, 5]       # first group, to 0; the argument is left alone
    assert f(a, 1) == [1, 15, 16, 5] and f(a, 16) == [1, 15, 16, 5]
    assert f(a, 17) == [1, 16, 15, 5] and f(a, 32) == [1, 16, 15, 5]
    assert f(a, 33) == [1, 16, 16, 4] and f(a, 37) == [1, 16, 16, 4]
    assert f([0, 3, 0, 2], 3) == [0, 3, 0, 1]                      # groups that went to 0 earlier hold no position
    assert f([1, 1], 1) == [1, 0]
    assert f([-2, 4, 3], 2) == [-2, 3, 3] and f([-2, 4, 3], 6) == [-2, 4, 2]    # positions count through the queries
    with pytest.raises(ValueError):
        f([-2, 4, 3], 1)                                           # a query
    with pytest.raises(ValueError):
        f(a, 38)
    with pytest.raises(ValueError):
        f(a, -1)
    seq = list(range(9))                                           # a replay of the list appends exactly the survivors
    groups = [3, 4, 2]
    for p in (8, 3, 0, 2):
        groups = f(groups, p)
        del seq[p]
    at, replay = 0, []
    for c in groups:
        replay += seq[at:at + c]
        at += c
    assert replay == seq == [1, 2, 5, 6, 7] and groups == [2, 2, 1]


def test_learners_have_revoke_and_relabel():
    import ital_amd
    from ital_amd.retrieval_base import ActiveRetrievalBase
    assert callable(ActiveRetrievalBase.revoke) and callable(ActiveRetrievalBase.relabel)
    for name in ("ITAL", "MCMI_min", "AdaptAL"):
        assert getattr(ital_amd, name).revoke is ActiveRetrievalBase.revoke
    assert callable(ital_amd.GaussianProcess.remove)
