"""The context layer with a user model on several devices, one rank per device over RCCL (include/ital_ctx.h): the noisy
golden session of the reference with the rows sharded, and top_results / predict identical on every rank.  Skips on a box
with fewer GPUs than ranks, as tests/test_gpu_multidevice.py does.  Reference: ital/ital.py:124-130 (Pool.map + np.argmax ->
row shards + one record all-gather per greedy step), ital/retrieval_base.py:64-75, ital/gp.py:264-292."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import _ranks  # noqa: E402
import make_golden  # noqa: E402  (fixture table only)
from test_gpu_ctx_models import Ctx  # noqa: E402

NDEV = _ranks.device_count()
WORLDS = [pytest.param(w, marks=pytest.mark.skipif(NDEV < w, reason="%d GPUs visible, %d needed (one device per rank)" % (NDEV, w)))
          for w in (2, 4, 8)]


def _worker(rank, world, port, name, out):
    dev, group = _ranks.join(rank, world, port, "rccl")
    try:
        from ital_amd import _lib, sharding
        lib = _lib.load()
        comm = sharding.raw_comm(group, dev)
        if comm is None:
            out[rank] = ("no raw communicator", sharding.raw_comm_reason(group, dev))
            return
        z = np.load(os.path.join(HERE, "golden", name + ".npz"))
        n = len(z["X"])
        row0, row1 = sharding.row_range(n, world, rank)
        ctx = Ctx(lib, z["X"][row0:row1], z["length_scale"], z["var"], z["noise"], rank=rank, world=world, comm=comm,
                  n_total=n)
        try:
            assert ctx.set_model(**make_golden.FIXTURES[name]["kw"]) == 0, ctx.err()
            picks, prev, k = [], 0, int(z["k"])
            for r in range(int(z["rounds"])):
                ind, y = z["r%d_ind" % r], z["r%d_y" % r]
                ctx.update(ind[prev:], y[prev:])
                prev = len(ind)
                mean, var = ctx.predict_stored()
                np.testing.assert_allclose(mean, z["r%d_rel_mean" % r][row0:row1], rtol=0, atol=2e-9)
                np.testing.assert_allclose(var, z["r%d_var" % r][row0:row1], rtol=0, atol=2e-9)
                rc, got = ctx.fetch(k)
                assert rc == k, ctx.err()
                picks.append(got)
            ctx.update(picks[-1], z["rel"][picks[-1]])
            mean, _ = ctx.predict_stored()
            np.testing.assert_allclose(mean, z["final_rel_mean"][row0:row1], rtol=0, atol=1e-9)
            rc, top = ctx.top_results(10)
            assert rc == 0, ctx.err()
            rc, pm, pv = ctx.predict(z["predict_X"])
            assert rc == 0, ctx.err()
            assert ctx.mcmi_fetch(2)[0] == -38
            out[rank] = ("ok", picks, top, pm.tolist(), pv.tolist())
        finally:
            ctx.close()
    finally:
        _ranks.leave(group)


@pytest.mark.parametrize("world", WORLDS)
def test_noisy_golden_on_several_devices(world):
    name = "synth200_noisy"
    z = np.load(os.path.join(HERE, "golden", name + ".npz"))
    res = _ranks.spawn(_worker, world, name)
    assert all(r[0] == "ok" for r in res), res
    for r in range(int(z["rounds"])):
        assert all(res[w][1][r] == z["r%d_ret" % r].tolist() for w in range(world)), r
    assert all(res[w][2] == z["top_results_10"].tolist() for w in range(world))
    for w in range(world):
        assert res[w][3] == res[0][3] and res[w][4] == res[0][4]      # every rank computes the same prediction
    np.testing.assert_allclose(res[0][3], z["predict_mean"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(res[0][4], z["predict_var"], rtol=0, atol=1e-9)
