"""Inputs and upload helpers that tests/test_gpu_evidence.py and tests/test_gpu_evidence_grad.py share: the candidates, the
label generator, the upload of feature rows and parameters, and one call of ital_gp_evidence through its raw descriptor."""
import ctypes

import numpy as np
import torch

GUARD = -7.0             # what output buffers hold before a call: nothing outside the documented part may change

CANDS = {3: [(0.5, 1.0, 0.1), (0.8, 1.5, 0.3), (0.35, 0.7, 0.05)],
         40: [(1.2, 1.0, 1e-4), (1.8, 1.5, 1e-3), (0.9, 0.7, 1e-6)]}


def _labels(rng, m):
    return np.where(rng.random(m) < 0.4, 1.0, -1.0)


def _case(m, d, G):
    rng = np.random.default_rng(1000 * d + m)
    X = rng.random((m, d))
    return X, _labels(rng, m), CANDS[d][:G]


def _lib():
    from ital_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _upload(X, dev):
    """Feature rows zero padded to a multiple of 16 columns, and their squared norms (ital_row_norms)."""
    L, lib = _lib()
    m, d = X.shape
    ldx = (d + 15) // 16 * 16
    XT = torch.zeros((m, ldx), dtype=torch.float64, device=dev)
    XT[:, :d] = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
    XTn = torch.empty(m, dtype=torch.float64, device=dev)
    L.check(lib.ital_row_norms(XT.data_ptr(), m, ldx, XTn.data_ptr(), _stream()))
    return XT, XTn, ldx


def _params(cands, dev):
    return torch.tensor([[float(v) for v in c] for c in cands], dtype=torch.float64, device=dev)


def _evidence(X, y, cands, dev, pad=0):
    """ital_gp_evidence on G candidates; leading dimensions m + pad; K and the workspace (one guard element behind it) start
    as GUARD.  Returns the device tensors."""
    L, lib = _lib()
    XT, XTn, ldx = _upload(X, dev)
    m, G = len(X), len(cands)
    ld = ldm = m + pad
    yd = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).to(dev)
    prm = _params(cands, dev)
    K = torch.full((G, m, ld), GUARD, dtype=torch.float64, device=dev)
    need = int(lib.ital_gp_evidence_workspace(m, G))
    work = torch.full((need + 1,), GUARD, dtype=torch.float64, device=dev)
    scores = torch.full((G, 3), GUARD, dtype=torch.float64, device=dev)
    info = torch.full((G,), -1, dtype=torch.int32, device=dev)
    lm = torch.full((G, ldm), GUARD, dtype=torch.float64, device=dev)
    lv = torch.full((G, ldm), GUARD, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    d = L.ItalEvidenceDesc()
    d.XT, d.XTn, d.ldx, d.y, d.m, d.params, d.G = XT.data_ptr(), XTn.data_ptr(), ldx, yd.data_ptr(), m, prm.data_ptr(), G
    d.K, d.ld, d.scores, d.info, d.loo_mean, d.loo_var, d.ldm = K.data_ptr(), ld, scores.data_ptr(), info.data_ptr(), \
        lm.data_ptr(), lv.data_ptr(), ldm
    d.status, d.work, d.work_doubles, d.ev = status.data_ptr(), work.data_ptr(), need, None
    before = int(lib.ital_launch_count())
    L.check(lib.ital_gp_evidence(ctypes.byref(d), _stream()))
    launches = int(lib.ital_launch_count()) - before
    torch.cuda.synchronize()
    return dict(scores=scores, info=info, loo_mean=lm, loo_var=lv, status=int(status.item()), K=K, m=m, work=work, need=need,
                launches=launches)
