"""The context layer beyond the perfect user (include/ital_ctx.h): its declarations, their bindings and the layout of
ital_ctx_model -- checks that need no GPU.  The GPU side is tests/test_gpu_ctx_models*.py."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "ital_ctx.h")
CXX = os.environ.get("CXX", "g++")


def test_ctx_header_declarations_equal_the_bindings():
    from ital_amd import _lib
    header = open(HEADER).read()
    declared = set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", header))     # the regex of the ital_hip.h export test
    assert "ital_ctx_model" not in declared             # a struct name is never followed by "(" in the header
    assert declared == set(_lib.CTX_SIGNATURES), declared ^ set(_lib.CTX_SIGNATURES)
    assert not declared & set(_lib.SIGNATURES)           # ital_hip.h's table stays what ital_hip.h declares
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    loaded = _lib.load()
    for name, (res, args) in _lib.CTX_SIGNATURES.items():
        fn = getattr(loaded, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_ctx_model_layout_matches_the_header(tmp_path):
    from ital_amd import _lib
    if shutil.which(CXX) is None:
        pytest.skip("no C++ compiler on this box")
    src = tmp_path / "layout.cpp"
    fields = [f[0] for f in _lib.ItalCtxModel._fields_]
    body = "".join('    printf("%s %%zu\\n", offsetof(ital_ctx_model, %s));\n' % (f, f) for f in fields)
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "ital_ctx.h"\nint main() {\n'
                   '    printf("sizeof %zu\\n", sizeof(ital_ctx_model));\n' + body + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    build = subprocess.run([CXX, "-O1", "-std=c++17", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                            "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    out = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(_lib.ItalCtxModel)
    for f in fields:
        assert int(out[f]) == getattr(_lib.ItalCtxModel, f).offset, f


def test_ctx_entry_points_refuse_bad_arguments_without_a_device():
    """Argument checks come before any device work: a NULL context is -22 for every new entry point."""
    from ital_amd import _lib
    lib = _lib.load()
    model = _lib.ItalCtxModel(1.0, 0.0, 0, 0, 0, 0.0)
    picks = (ctypes.c_int64 * 4)()
    assert lib.ital_ctx_set_model(None, ctypes.byref(model)) == -22
    assert lib.ital_ctx_fetch_list(None, 2, None, 0, None, 0, picks, None) == -22
    assert lib.ital_ctx_mcmi_fetch(None, 2, None, 0, picks, None) == -22
    assert lib.ital_ctx_top_results(None, 2, picks, None) == -22
    assert lib.ital_ctx_predict(None, None, 0, None, None, None) == -22
