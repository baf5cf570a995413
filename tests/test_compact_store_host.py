"""Host side of the compact store (no device): the declarations of include/ital_rows.h against their bindings, the header
through a C compiler, the argument checks that come before any HIP call (-22: unknown element type, X not aligned to 16 B,
a NULL xnorm of ital_whiten_rows_t, the ingest's own), and the validation of DeviceData's `storage`.  The GPU side is
tests/test_gpu_compact_store.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

TYPED = ["ital_rbf_cols", "ital_cross_cov_cols", "ital_whiten_append", "ital_gp_append", "ital_score_step", "ital_fetch_round",
         "ital_select_local", "ital_select_fused", "ital_gather_block", "ital_whiten_rows"]
ROWS = [name + "_t" for name in TYPED] + ["ital_ingest_rows_t"]


def _code():
    header = open(os.path.join(ROOT, "include", "ital_rows.h")).read()
    return re.sub(r"/\*.*?\*/", "", header, flags=re.S)


def test_rows_declarations_equal_bindings_and_are_exported():
    from ital_amd import _lib
    code = _code()
    declared = set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", code))
    assert declared == set(ROWS) == set(_lib.ROWS_SIGNATURES), declared ^ set(_lib.ROWS_SIGNATURES)
    others = [getattr(_lib, name) for name in dir(_lib) if name.endswith("SIGNATURES") and name != "ROWS_SIGNATURES"]
    assert len(others) >= 8
    for other in others:
        assert not declared & set(other)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    for name, (res, args) in _lib.ROWS_SIGNATURES.items():
        assert hasattr(raw, name), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    # a typed entry point takes what its FP64 sibling takes, with `int xtype` in front of the stream -- in C and in ctypes
    sigs = dict(_lib.SIGNATURES)
    sigs.update(_lib.REWHITEN_SIGNATURES)
    for name in TYPED:
        res, args = sigs[name]
        assert _lib.ROWS_SIGNATURES[name + "_t"] == (res, args[:-1] + [ctypes.c_int, args[-1]]), name
        assert re.search(r"\bint\s+%s_t\s*\([^;]*,\s*int\s+xtype,\s*hipStream_t\s+stream\)\s*;" % name, code), name
    c = ctypes
    assert _lib.ROWS_SIGNATURES["ital_ingest_rows_t"] == (c.c_int, [c.c_void_p, c.c_int, c.c_int64, c.c_int, c.c_int64, c.c_void_p,
                                                                    c.c_int, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p])
    assert re.search(r"\bint\s+ital_ingest_rows_t\s*\(\s*const\s+void\s*\*\s*src,\s*int\s+dtype,\s*int64_t\s+n,\s*int\s+d,\s*"
                     r"int64_t\s+ld_src,\s*void\s*\*\s*X,\s*int\s+ldx,\s*double\s*\*\s*xnorm,\s*double\s*\*\s*scratch,\s*"
                     r"int64_t\s+scratch_rows,\s*hipStream_t\s+stream\)\s*;", code)
    # no existing public header knows the new entry points
    for untouched in ("ital_hip.h", "ital_ctx.h", "ital_ingest.h", "ital_rewhiten.h", "ital_dense.h"):
        text = open(os.path.join(ROOT, "include", untouched)).read()
        assert "ital_rows" not in text and not re.search(r"ital_[a-z_]+_t\s*\(", text), untouched
    from ital_amd import build
    assert "rows.hip" in build.SOURCES
    assert os.path.realpath(os.path.join(ROOT, "include", "ital_rows.h")) in [os.path.realpath(h) for h in build.headers()]
    assert os.path.realpath(os.path.join(ROOT, "ital_amd", "csrc", "rows_elem.h")) in [os.path.realpath(h) for h in build.headers()]


def test_the_header_parses_as_c_and_as_cxx(tmp_path):
    src = tmp_path / "use_rows.c"
    src.write_text('#include "ital_rows.h"\n'
                   "typedef int (*round_fn)(const ital_round_desc*, int, hipStream_t);\n"
                   "typedef int (*rows_fn)(const ital_rewhiten_desc*, int, hipStream_t);\n"
                   "round_fn use_round = ital_fetch_round_t;\n"
                   "rows_fn use_rows = ital_whiten_rows_t;\n"
                   "int main(void) { return (ITAL_INGEST_BF16 == 3 && sizeof(ital_append_desc) > 0) ? 0 : 1; }\n")
    inc = os.path.join(ROOT, "include")
    for cc, std, name in (("gcc", "-std=c99", "use_rows.c"), ("g++", "-std=c++11", "use_rows.cpp")):
        unit = tmp_path / name
        unit.write_text(src.read_text())
        r = subprocess.run([cc, std, "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(unit)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


# fake pointers that are never followed: every case below is decided before any HIP call
P = 4096          # aligned to 16 B
ODD = 4104        # aligned to 8 B only


def _refused(lib, rc, who):
    assert rc == -22, who
    assert who in lib.ital_last_error().decode(), (who, lib.ital_last_error().decode())


def _kcols_calls(lib, X, xtype):
    yield "ital_rbf_cols", lib.ital_rbf_cols_t(X, P, 20, 16, P, P, 1, 1.0, 0.5, P, 32, xtype, None)
    yield "ital_cross_cov_cols", lib.ital_cross_cov_cols_t(X, P, 20, 16, P, P, 1, P, 16, P, 32, 0, 1.0, 0.5, P, 32, xtype, None)
    yield "ital_whiten_append", lib.ital_whiten_append_t(X, P, 20, 16, P, P, 1, P, 16, P, P, P, 32, 0, 1.0, 0.5, P, P, xtype, None)
    yield "ital_gather_block", lib.ital_gather_block_t(P, 3, 0, 20, X, P, 16, P, 32, 0, P, P, P, P, 16, P, P, P, xtype, None)


def _select_calls(lib, X, xtype):
    from ital_amd import _lib
    b = _lib.ItalBatch(4, 16, 16, P, P, P, P, P, P, P, P)
    head = (P, P, P, 10, 0, None, 0, 0, 0, P, P, X, P, 16, P, 32, 0, 16, P, 32, 0)
    yield "ital_select_local", lib.ital_select_local_t(*head, 4, P, P, P, xtype, None)
    yield "ital_select_fused", lib.ital_select_fused_t(*head, 0, b, P, P, P, xtype, None)


def _desc_calls(lib, X, xtype):
    from ital_amd import _lib
    a = _lib.ItalAppendDesc()
    a.rows, a.ldx, a.X, a.xnorm, a.n, a.XT, a.XTn, a.L, a.ldl, a.alpha, a.ybuf = P, 16, X, P, 20, P, P, P, 16, P, P
    a.V, a.ldv, a.m, a.var, a.length_scale, a.noise, a.mu, a.s2, a.status = P, 32, 0, 1.0, 0.5, 1e-6, P, P, P
    a.lb.c = 1
    yield "ital_gp_append", lib.ital_gp_append_t(ctypes.byref(a), xtype, None)
    d = _lib.ItalScoreDesc()
    d.t, d.n_cand, d.sel_X = 1, 10, X
    yield "ital_score_step", lib.ital_score_step_t(ctypes.byref(d), xtype, None)
    r = _lib.ItalRoundDesc()
    r.k, r.step.sel_X = 1, X
    yield "ital_fetch_round", lib.ital_fetch_round_t(ctypes.byref(r), xtype, None)
    yield "ital_whiten_rows", lib.ital_whiten_rows_t(ctypes.byref(_rewhiten_desc(X=X)), xtype, None)


def _rewhiten_desc(**kw):
    from ital_amd import _lib
    d = _lib.ItalRewhitenDesc()
    base = dict(X=P, n_rows=20, ldx=16, XT=P, XTn=P, L=P, ldl=16, alpha=P, m=8, var=1.0, length_scale=0.5, xnorm=P,
                V=P, ldv=32, v_rows=16, mu=P, s2=P, chunk=0)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("calls", [_kcols_calls, _select_calls, _desc_calls])
def test_typed_entry_points_refuse_an_unknown_type_and_an_unaligned_matrix_without_a_device(calls):
    from ital_amd import _lib
    lib = _lib.load()
    for xtype in (-1, 4, 17):
        for who, rc in calls(lib, P, xtype):
            _refused(lib, rc, who)
            assert "type" in lib.ital_last_error().decode(), who
    for xtype in (0, 1, 2, 3):
        for who, rc in calls(lib, ODD, xtype):
            _refused(lib, rc, who)
            assert "16 B" in lib.ital_last_error().decode(), who


def test_whiten_rows_t_needs_xnorm_and_keeps_the_checks_of_its_sibling():
    from ital_amd import _lib
    lib = _lib.load()
    for xtype in (0, 1, 2, 3):
        _refused(lib, lib.ital_whiten_rows_t(ctypes.byref(_rewhiten_desc(xnorm=None)), xtype, None), "ital_whiten_rows")
        _refused(lib, lib.ital_whiten_rows_t(None, xtype, None), "ital_whiten_rows")
        for bad in (dict(X=None), dict(V=None), dict(ldx=24), dict(ldl=7), dict(ldv=19), dict(n_rows=-1), dict(chunk=48)):
            _refused(lib, lib.ital_whiten_rows_t(ctypes.byref(_rewhiten_desc(**bad)), xtype, None), "ital_whiten_rows")
        assert lib.ital_whiten_rows_t(ctypes.byref(_rewhiten_desc(n_rows=0)), xtype, None) == 0      # no launch


def _ingest(lib, **kw):
    a = dict(src=P, dtype=2, n=20, d=10, ld_src=10, X=2 * P, ldx=16, xnorm=3 * P, scratch=4 * P, scratch_rows=8)
    a.update(kw)
    return lib.ital_ingest_rows_t(a["src"], a["dtype"], a["n"], a["d"], a["ld_src"], a["X"], a["ldx"], a["xnorm"], a["scratch"],
                                  a["scratch_rows"], None)


def test_compact_ingest_refuses_bad_arguments_without_a_device():
    from ital_amd import _lib
    lib = _lib.load()
    for bad in (dict(src=None), dict(X=None), dict(xnorm=None), dict(n=-1), dict(d=0), dict(ldx=24), dict(ldx=8), dict(d=17),
                dict(ld_src=9), dict(dtype=-1), dict(dtype=4), dict(dtype=1, src=4098), dict(dtype=2, src=4097),
                dict(dtype=3, src=4097), dict(dtype=0, src=4100), dict(X=2 * P + 8), dict(xnorm=3 * P + 4), dict(scratch=None),
                dict(scratch_rows=0), dict(scratch_rows=-3), dict(scratch=4 * P + 8)):
        _refused(lib, _ingest(lib, **bad), "ital_ingest_rows_t")
    assert _ingest(lib, n=0) == 0
    assert _ingest(lib, n=0, src=None, X=None, xnorm=None, scratch=None, scratch_rows=0) == 0
    assert _ingest(lib, n=0, ldx=24) == -22


def test_rows_fn_picks_the_sibling():
    from ital_amd import _lib
    lib = _lib.lib()
    assert _lib.rows_fn("ital_rbf_cols", _lib.INGEST_F64) is lib.ital_rbf_cols
    typed = _lib.rows_fn("ital_rbf_cols", 7)                  # the type reaches the C side in front of the stream
    _refused(lib, typed(P, P, 20, 16, P, P, 1, 1.0, 0.5, P, 32, None), "ital_rbf_cols")


def test_storage_is_validated_before_anything_else(monkeypatch):
    torch = pytest.importorskip("torch")
    import inspect
    import ital_amd
    X = np.zeros((4, 3), dtype=np.float32)
    for bad in ("f32", "float16", "compact", None, 16, torch.float16):
        with pytest.raises(ValueError, match="storage"):
            ital_amd.DeviceData(X, storage=bad)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for ok in ("f64", "source"):
        with pytest.raises(RuntimeError, match="needs a HIP device"):
            ital_amd.DeviceData(X, storage=ok)
    p = inspect.signature(ital_amd.DeviceData.__init__).parameters["storage"]
    assert p.default == "f64" and p.kind is inspect.Parameter.KEYWORD_ONLY
