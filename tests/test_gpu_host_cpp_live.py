"""A host that is not Python drives a live session: tests/host_gpu_live_driver.cpp (C++, include/ital_ctx_live.h, nothing of
ital_amd and no device buffer of its own) labels, takes rows in, scores a grid of hyper-parameters and applies the best,
deletes rows and fetches -- and must print what the same calls return through ctypes.  Built and run the way
tests/test_gpu_host_cpp.py builds host_gpu_driver.cpp."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CXX = os.environ.get("CXX", "g++")      # host-only code: any C++17 compiler (the HIP runtime API is plain C)
sys.path.insert(0, HERE)


def test_cpp_host_drives_a_live_session(tmp_path):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if shutil.which(CXX) is None:
        pytest.skip("no C++ compiler on this box")
    import test_gpu_ctx_live as live
    from ital_amd import _lib
    lib_path = os.path.join(ROOT, "ital_amd", "libital_hip.so")
    assert os.path.exists(lib_path), "build the library first (python -m ital_amd.build)"
    exe = str(tmp_path / "host_gpu_live_driver")
    build = subprocess.run([CXX, "-O1", "-std=c++17", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                            "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "host_gpu_live_driver.cpp"), "-o", exe,
                            lib_path, "-Wl,-rpath," + os.path.dirname(lib_path), "-L/opt/rocm/lib", "-lamdhip64",
                            "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    X, Xnew = live.X, live.XALL[150:187]
    grid = np.array([[v, var, 1e-6] for v in (0.3, 0.5, 0.8, 1.2, 1.8) for var in (0.7, 1.0)])
    labels, gone, k = live.LABELLED, live.REMOVED + [160], 4
    files = {}
    for name, arr in (("X", X), ("Xnew", Xnew), ("grid", grid)):
        files[name] = str(tmp_path / (name + ".f64"))
        np.ascontiguousarray(arr, dtype=np.float64).tofile(files[name])
    args = [exe, files["X"], str(len(X)), str(X.shape[1]), repr(live.LS), files["Xnew"], str(len(Xnew)), files["grid"],
            str(len(grid)), str(k), str(len(labels))]
    for i in labels:
        args += [str(i), repr(float(live.YALL[i]))]
    args += [str(len(gone))] + [str(i) for i in gone]
    run = subprocess.run(args, capture_output=True, text=True, timeout=600)
    print(run.stdout[:2000], run.stderr[-2000:])
    assert run.returncode == 0, (run.stdout[:2000], run.stderr[-2000:])
    out = {line.split(":")[0]: line.split(":")[1].split() for line in run.stdout.splitlines()}

    # the same calls through ctypes
    lib = _lib.load()
    c = live.Ctx(lib, X, capacity=16)
    try:
        assert c.reserve(len(labels) + k) == 0, c.err()
        c.update(labels)
        assert c.add_rows(Xnew) == 0, c.err()
        rc, scores, ok = c.evidence(grid)
        assert rc == 0 and ok.all(), c.err()
        best = int(np.argmax(scores[:, 0]))
        assert c.set_params(*grid[best]) == 0, c.err()
        rc, imap = c.remove_rows(gone, len(X) + len(Xnew))
        assert rc == 0, c.err()
        rc, picks = c.fetch(k)
        assert rc == k, c.err()
        mean, _ = c.predict_stored()
    finally:
        c.close()
    assert int(out["best"][0]) == best and float(out["best"][1]) == scores[best, 0]
    assert [int(v) for v in out["map"]] == imap.tolist()
    assert [int(v) for v in out["picks"]] == picks
    assert np.array_equal(np.array([float(v) for v in out["means"]]), mean)      # %.17g round-trips a double
