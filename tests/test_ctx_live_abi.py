"""A live session in a context (include/ital_ctx_live.h): its declarations, their bindings and the argument checks that come
before any device work -- checks that need no GPU.  The GPU side is tests/test_gpu_ctx_live.py."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "ital_ctx_live.h")

NAMES = {"ital_ctx_reserve", "ital_ctx_add_rows", "ital_ctx_remove_rows", "ital_ctx_set_params", "ital_ctx_evidence"}


def _tables(_lib):
    return {name: table for name, table in vars(_lib).items() if name.endswith("_SIGNATURES") and isinstance(table, dict)}


def test_live_header_declarations_equal_the_bindings():
    from ital_amd import _lib
    header = open(HEADER).read()
    declared = set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", header))     # the regex of the ital_hip.h export test
    assert declared == NAMES
    assert declared == set(_lib.CTX_LIVE_SIGNATURES), declared ^ set(_lib.CTX_LIVE_SIGNATURES)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    loaded = _lib.load()
    for name, (res, args) in _lib.CTX_LIVE_SIGNATURES.items():
        fn = getattr(loaded, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_live_names_are_in_no_other_table_and_no_other_header():
    from ital_amd import _lib
    tables = _tables(_lib)
    assert "CTX_LIVE_SIGNATURES" in tables and len(tables) > 5
    for name, table in tables.items():
        if name != "CTX_LIVE_SIGNATURES":
            assert not NAMES & set(table), name
    inc = os.path.join(ROOT, "include")
    for f in sorted(os.listdir(inc)):
        if f.endswith(".h") and f != "ital_ctx_live.h":
            declared = set(re.findall(r"\b(ital_[a-z_0-9]+)\s*\(", open(os.path.join(inc, f)).read()))
            assert not NAMES & declared, f


def test_live_argument_types_follow_the_header():
    """The C parameter lists, read out of the header, against the ctypes argument lists."""
    from ital_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for name, (res, args) in _lib.CTX_LIVE_SIGNATURES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        want = []
        for p in m.group(1).split(","):
            p = p.strip()
            if "*" in p or p.startswith("hipStream_t"):
                want.append(ctypes.c_void_p)
            else:
                want.append(kinds[p.split()[0]])
        assert res is ctypes.c_int and args == want, (name, args, want)


def test_live_entry_points_refuse_a_null_context_without_a_device():
    """Argument checks come before any HIP call: a NULL context is -22 for each of the five."""
    from ital_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 8)()
    idx = (ctypes.c_int64 * 4)()
    ok = (ctypes.c_int * 2)()
    nan = float("nan")
    for rc in (lib.ital_ctx_reserve(None, 64, None),
               lib.ital_ctx_add_rows(None, buf, 1, 0, None),
               lib.ital_ctx_remove_rows(None, idx, 1, None, None),
               lib.ital_ctx_set_params(None, nan, nan, nan, None),
               lib.ital_ctx_evidence(None, buf, 2, buf, ok, None)):
        assert rc == -22
        assert b"ital_ctx_" in lib.ital_last_error()
