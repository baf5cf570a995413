"""USDM on the device: uncertainty sampling with diversity maximization (Yang et al., IJCV 2015), the reference's
ital/baseline_methods.py:575-658.

Per fetch the reference solves one dense non-symmetric system of the size of the unlabelled set (the harmonic label
propagation over a k-nearest-neighbour graph) and then 2 to 100 dense symmetric ones inside an augmented-Lagrangian loop.
Here, on the device (include/ital_usdm.h, include/ital_dense.h, include/ital_knn.h):

    ital_knn_rows            the graph, once per data set: kept on the store and shared by every learner on it
    ital_usdm_laplacian      M = D_uu - W_uu and W_ul y from the neighbour lists and the id sets
    ital_lu_factor / _solve  p = M^-1 W_ul y by an LU without pivoting (M is diagonally dominant by rows)   (FP64 MFMA)
    ital_gram_rows           K_uu, once per fetch                                                          (FP64 MFMA)
    per iteration            ital_usdm_shift (K_uu + mu 11^T + mu I into the buffer the Laplacian used), ital_chol_batched,
                             ital_chol_solve_batched, the vector updates in torch, ital_symv_lower for the objective, and
                             one scalar read for the reference's stop test

numpy's own partition order decides the returned list, as in the reference.

Limits.  The graph is the `knn` nearest rows by squared Euclidean distance, which is the reference's
argpartition(diag(diag K) - K) as long as the knn-th largest kernel value of every row is above zero and there is no tie at
the boundary.  The loop's systems are symmetric positive definite and are solved by Cholesky where the reference calls a
pivoted LU: should a pivot not be positive in floating point, the reference would go on and this learner raises LinAlgError.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check
from .device_data import _knn_args, neighbour_lists
from .gp import _pad16, _ptr, _stream
from .retrieval_base import ActiveRetrievalBase

EPS = 1e-6          # the weight of a pair that is no neighbour (baseline_methods.py:607)


def usdm_entropy_term(prob, r):
    """b of the reference (baseline_methods.py:621) from the clipped probabilities; numpy arrays or torch tensors."""
    log = torch.log if isinstance(prob, torch.Tensor) else np.log
    return (float(r) * (prob * log(prob) + (1.0 - prob) * log(1.0 - prob))) / float(np.log(0.5))


class USDM(ActiveRetrievalBase):
    """Uncertainty sampling with diversity maximization (reference ital/baseline_methods.py:575-658); constructor arguments
    as the reference's plus the keyword-only placement arguments.  `knn`: neighbours per row of the graph, 1..32.

    Not supported: row sharding (the graph is not built across the shards of several ranks); rows kept in their source
    precision (`DeviceData(storage="source")`: ital_gram_rows reads FP64 rows); and `queries`.  The reference accepts
    queries but gives every query row y = 0 in the label propagation -- its `i in self.relevant_ids` is never true for a
    query row -- which treats a query as an irrelevant sample; that is not copied here, queries are refused instead."""

    def __init__(self, data=None, queries=[], length_scale=0.1, var=1.0, noise=1e-6, knn=5, r=1.0, max_iter=100, tol=1e-6,
                 **placement):
        if int(placement.get("world", 1)) > 1:
            raise NotImplementedError("USDM needs neighbour lists over all rows: they are not built across row shards")
        _knn_args(knn, "sqeuclidean")
        self.knn = int(knn)
        self.r = r
        self.max_iter = max_iter
        self.tol = tol
        self._lists = {}              # a learner on plain numpy data keeps its neighbour lists itself
        ActiveRetrievalBase.__init__(self, data, queries, length_scale, var, noise, **placement)
        #: what the last fetch computed (numpy): candidates, prob, b, f; iterations and the objective of each
        self.last = None

    def fit(self, data, queries=[]):
        if len(queries) > 0:
            raise NotImplementedError("USDM does not take queries: the reference labels a query row y = 0 in its label "
                                      "propagation, as if it were irrelevant; give the query's feedback by update()")
        ActiveRetrievalBase.fit(self, data, queries)
        if self.gp is not None and self.gp.Xd.dtype != torch.float64:
            raise NotImplementedError("USDM needs FP64 rows on the device (ital_gram_rows): build the DeviceData with "
                                      "storage='f64'")

    def _start_afresh(self):
        """add_data() / remove_data() / sync_data() / set_params(): what the learner keeps is dropped."""
        ActiveRetrievalBase._start_afresh(self)
        self._lists = {}
        self.last = None

    def _graph(self):
        """The NeighbourLists of the samples this learner knows: the store's own (shared by every learner on it that sees
        the same rows), or the learner's for plain numpy data."""
        gp = self.gp
        cache = gp.store._knn if gp.store is not None else self._lists
        return neighbour_lists(cache, gp.Xd, gp.xnorm, gp.n, "sqeuclidean", self.knn, True)

    def fetch_unlabelled(self, k):
        """Fetches a batch of unlabelled samples (reference baseline_methods.py:611-626); list of python ints."""
        gp = self.gp
        if len(self.queries) > 0:
            raise NotImplementedError("USDM does not take queries")
        if len(self.relevant_ids) == 0 and len(self.irrelevant_ids) == 0:
            raise RuntimeError("fetch_unlabelled() needs labelled samples to propagate from: call update() first")
        self._last_batch = None
        self.last = None
        u = np.asarray(self._unseen_array(), dtype=np.int64)
        n, n_u = int(gp.n), len(u)
        np.argpartition(np.empty(n_u), k - 1)               # k > n_u: numpy's ValueError, before any device work
        lib, dev = _lib.lib(), gp.device
        ld = _pad16(n_u)
        work_len = int(lib.ital_symv_lower_workspace(n_u))
        need = 8 * (2 * n_u * ld + work_len + 16 * n_u) + 9 * n
        with torch.cuda.device(dev):
            free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
            if need > free:
                raise MemoryError("USDM: the two %d x %d matrices of a fetch take %d bytes, more than the %d free on %s"
                                  % (n_u, n_u, need, free, dev))
            st = _stream()
            pos = np.full(n, -1, dtype=np.int64)
            pos[u] = np.arange(n_u, dtype=np.int64)
            rel = np.zeros(n, dtype=np.uint8)
            rel[np.fromiter(self.relevant_ids, dtype=np.int64, count=len(self.relevant_ids))] = 1
            u_d, pos_d, rel_d = (torch.from_numpy(a).to(dev) for a in (u, pos, rel))
            idx = self._graph().idx
            M = torch.empty((n_u, ld), dtype=torch.float64, device=dev)
            Kuu = torch.empty((n_u, ld), dtype=torch.float64, device=dev)
            p = torch.empty(n_u, dtype=torch.float64, device=dev)
            flags = torch.zeros(4, dtype=torch.int32, device=dev)       # LU info, LU status, Cholesky info, Cholesky status
            # ---- the harmonic solve (baseline_methods.py:619-620)
            check(lib.ital_usdm_laplacian(_ptr(idx), self.knn, n, _ptr(u_d), n_u, _ptr(pos_d), _ptr(rel_d),
                                          len(self.relevant_ids), EPS, _ptr(M), ld, _ptr(p), st))
            check(lib.ital_lu_factor(_ptr(M), n_u, ld, _ptr(flags[0:]), _ptr(flags[1:]), st))
            check(lib.ital_lu_solve(_ptr(M), n_u, ld, _ptr(p), _ptr(flags[0:]), st))
            prob = torch.clamp(p, 1e-8, 1.0 - 1e-8)
            b = usdm_entropy_term(prob, self.r)
            # ---- K_uu, once (lower triangle)
            ptrs = torch.tensor([u_d.data_ptr(), Kuu.data_ptr(), M.data_ptr(), ld], dtype=torch.int64, device=dev)
            n_p = torch.tensor([n_u], dtype=torch.int32, device=dev)
            check(lib.ital_gram_rows(_ptr(gp.Xd), _ptr(gp.xnorm), gp.ldx, _ptr(ptrs[0:]), _ptr(n_p), _ptr(ptrs[1:]), _ptr(ptrs[3:]),
                                     1, n_u, float(self.var), float(self.length_scale), 0.0, st))
            pivot = int(flags[0].item())
            if pivot != 0:
                raise np.linalg.LinAlgError("USDM: the graph Laplacian of the unlabelled samples has no LU factorisation "
                                            "without pivoting (pivot %d)" % pivot)
            f, objectives = self._alm(lib, st, Kuu, M, ld, b, k, ptrs, n_p, flags, work_len)
            f_host = f.cpu().numpy()
            self.last = dict(candidates=u, prob=prob.cpu().numpy(), b=b.cpu().numpy(), f=f_host,
                             iterations=len(objectives), objectives=np.array(objectives, dtype=np.float64))
        return u[np.argpartition(-f_host, k - 1)[:k]].tolist()

    def _alm(self, lib, st, Kuu, B, ld, b, k, ptrs, n_p, flags, work_len):
        """The augmented-Lagrangian loop (baseline_methods.py:629-658): the device vector f and the list of objectives."""
        n_u, dev = b.shape[0], b.device
        mu, rho = 1e-6, 1.1
        f = torch.full((n_u,), 1.0, dtype=torch.float64, device=dev) / n_u
        v = f.clone()
        lambda1 = torch.zeros((), dtype=torch.float64, device=dev)
        lambda2 = torch.zeros(n_u, dtype=torch.float64, device=dev)
        Kf = torch.empty(n_u, dtype=torch.float64, device=dev)
        work = torch.empty(max(work_len, 1), dtype=torch.float64, device=dev)
        y_p = torch.tensor([f.data_ptr()], dtype=torch.int64, device=dev)
        obj, objectives = None, []
        for it in range(self.max_iter):
            check(lib.ital_usdm_shift(_ptr(Kuu), n_u, ld, mu, _ptr(B), ld, st))
            f.copy_(mu * (v + 1.0) - (lambda2 + lambda1) - b)
            check(lib.ital_chol_batched(_ptr(ptrs[2:]), _ptr(n_p), _ptr(ptrs[3:]), 1, n_u, _ptr(flags[2:]), _ptr(flags[3:]), st))
            check(lib.ital_chol_solve_batched(_ptr(ptrs[2:]), _ptr(n_p), _ptr(ptrs[3:]), _ptr(y_p), 1, _ptr(flags[2:]), st))
            v = f + lambda2 / mu
            v[v < 0] = 0
            lambda1 = lambda1 + mu * (f.sum() - k)
            lambda2 = lambda2 + mu * (f - v)
            mu_used, mu = mu, mu * rho
            check(lib.ital_symv_lower(_ptr(Kuu), n_u, ld, _ptr(f), _ptr(Kf), _ptr(work), work.shape[0], st))
            both = torch.stack((torch.dot(f, Kf) / 2 + torch.dot(f, b), flags[2].to(torch.float64))).cpu().numpy()
            if both[1] != 0:
                raise np.linalg.LinAlgError("USDM: K_uu + mu 11^T + mu I is not positive definite in floating point in "
                                            "iteration %d (mu = %g, pivot %d); the reference's pivoted LU would go on"
                                            % (it, mu_used, int(both[1])))
            obj_prev, obj = obj, float(both[0])
            objectives.append(obj)
            if (obj_prev is not None) and (abs(obj_prev - obj) < self.tol):
                break
        return f, objectives
