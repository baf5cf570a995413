"""A host that is not Python drives the context layer beyond the perfect user: tests/host_gpu_driver_models.cpp (C++,
include/ital_ctx.h + the HIP runtime, nothing of ital_amd) replays the golden sessions synth200_noisy (a noisy user, two
rounds) and usps500_mcmi (MCMI_min on the reference's subsample, two rounds) -- updates, fetches, top_results and predict --
from raw files written here, and must reproduce the reference's results (ital/ital.py:84-134, ital/mcmi.py:48-81)."""
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
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden  # noqa: E402  (fixture table only)

_LABEL_MODES = {"mean": 0, "optimistic": 1, "pessimistic": 2}


def _session_file(z, name, path):
    kw = make_golden.FIXTURES[name]["kw"]
    mcmi = make_golden.FIXTURES[name]["learner"] == "MCMI_min"
    num = lambda v: repr(float(v))          # noqa: E731
    out = [1 if mcmi else 0, len(z["X"]), z["X"].shape[1], num(z["length_scale"]), num(z["var"]), num(z["noise"]), int(z["k"]),
           int(z["rounds"]), num(kw.get("label_prob", 1.0)), num(kw.get("mistake_prob", 0.0)),
           _LABEL_MODES[kw.get("label_estimation", "mean")]]
    prev = 0
    for r in range(int(z["rounds"])):
        ind, y = z["r%d_ind" % r][prev:], z["r%d_y" % r][prev:]
        prev += len(ind)
        out += [len(ind)] + [int(i) for i in ind] + [num(v) for v in y]
        cand = z["r%d_s0_cand" % r] if mcmi else []
        out += [len(cand)] + [int(i) for i in cand] + [int(i) for i in z["r%d_ret" % r]]
    last = z["r%d_ret" % (int(z["rounds"]) - 1)]
    out += [len(last)] + [int(i) for i in last] + [num(z["rel"][i]) for i in last]
    out += [int(i) for i in z["top_results_10"]]
    out += [len(z["predict_X"])] + [num(v) for v in z["predict_X"].ravel()]
    out += [num(v) for v in z["predict_mean"]] + [num(v) for v in z["predict_var"]]
    with open(path, "w") as f:
        f.write(" ".join(str(v) for v in out) + "\n")


@pytest.mark.parametrize("name", ["synth200_noisy", "usps500_mcmi"])
def test_cpp_host_replays_the_golden_session(tmp_path, name):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if shutil.which(CXX) is None:
        pytest.skip("no C++ compiler on this box")
    lib = os.path.join(ROOT, "ital_amd", "libital_hip.so")
    assert os.path.exists(lib), "build the library first (python -m ital_amd.build)"
    exe = str(tmp_path / "host_gpu_driver_models")
    build = subprocess.run([CXX, "-O1", "-std=c++17", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                            "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "host_gpu_driver_models.cpp"), "-o", exe,
                            lib, "-Wl,-rpath," + os.path.dirname(lib), "-L/opt/rocm/lib", "-lamdhip64",
                            "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    z = np.load(os.path.join(HERE, "golden", name + ".npz"))
    xfile, sfile = str(tmp_path / "X.f64"), str(tmp_path / "session.txt")
    np.ascontiguousarray(z["X"], dtype=np.float64).tofile(xfile)
    _session_file(z, name, sfile)
    run = subprocess.run([exe, xfile, sfile], capture_output=True, text=True, timeout=600)
    print(run.stdout, run.stderr[-2000:])
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    assert "ok (the reference's session)" in run.stdout
