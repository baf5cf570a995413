"""Streaming Gaussian process on MI355X: host-side mirror of reference ital/gp.py `GaussianProcess`.

Same public surface for the hot path (fit / update / reset / predict_stored / predict, attributes
ind, y, X, length_scale, var, noise) but a different state: the reference stores the dense N x N kernel
`K_all` (gp.py:128) and an explicit inverse re-computed at every update (gp.py:194); this class keeps, per
GPU, the row shard of X and the Cholesky-whitened block

    L L^T = K[T,T] + noise*I + diag(label_noise),   V = L^-1 K[T,:]  (m x n, one contiguous n-vector per labelled point),
    mu = V^T alpha (alpha = L^-1 y),   s2 = var - colsum(V^2)          

so an update appends c rows (rank-c Cholesky append) and N never appears squared.  All arithmetic runs in
the HIP kernels of libital_hip.so; torch only owns the device buffers and the stream.
"""
import ctypes
import os
import time

import numpy as np
import torch

from . import _lib, sharding
from ._lib import check
from .device_data import DTYPE_CODES, DeviceData


def _pad16(v):
    return (int(v) + 15) // 16 * 16


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _candidate_params(model, params_list):
    """float64 [G, 3] (length_scale, var, noise) of hyper-parameter candidates: dicts with `length_scale`, `var`, `noise`;
    what one leaves out is `model`'s current value.  TypeError for any other key, ValueError for a non-positive length_scale
    or var.  evidence(), evidence_grad() and tune.session_scores read their candidates through this; an array it returned
    passes through (session_scores parses once, then hands evidence() the array)."""
    if isinstance(params_list, np.ndarray):
        if params_list.dtype != np.float64 or params_list.ndim != 2 or params_list.shape[1] != 3:
            raise TypeError("candidates as an array are float64 [G, 3]")
        if not (params_list[:, :2] > 0).all():
            raise ValueError("length_scale and var must be positive")
        return np.ascontiguousarray(params_list)
    rows = []
    for p in params_list:
        unknown = set(p) - {"length_scale", "var", "noise"}
        if unknown:
            raise TypeError("unexpected GP parameters: %s" % ", ".join(sorted(unknown)))
        row = (float(p.get("length_scale", model.length_scale)), float(p.get("var", model.var)),
               float(p.get("noise", model.noise)))
        if not (row[0] > 0 and row[1] > 0):
            raise ValueError("length_scale and var must be positive")
        rows.append(row)
    return np.array(rows, dtype=np.float64).reshape(len(rows), 3)


def appends_after_remove(appends, p):
    """`appends` (sizes of the calls that built the labelled set, in order; negative: a group of queries) once the sample at
    labelled position `p` has left: the group that held it shrinks by one -- possibly to 0, which load_state_dict skips --
    so that a replay of the list appends exactly the surviving sequence.  Query groups are never touched: a position
    inside one is a ValueError, like a position outside the labelled set."""
    out = list(appends)
    at = 0
    for g, c in enumerate(out):
        if at <= p < at + abs(c):
            if c < 0:
                raise ValueError("labelled position %d is a query" % p)
            out[g] = c - 1
            return out
        at += abs(c)
    raise ValueError("labelled position %d outside the %d labelled samples" % (p, at))


class GaussianProcess(object):
    """GP on a row shard of `data` (rows [row0, row1) on this rank).

    # Arguments (as reference ital/gp.py:103-120, plus keyword-only placement):
    - data: n-by-d array of all samples; or a `DeviceData` (rows that are on the device already, shared with every other
      learner built on it: nothing is uploaded), or a torch tensor (wrapped in a DeviceData of this model's own).
    - length_scale, var, noise: kernel hyper-parameters.
    - device: torch device of this rank.
    - rank / world / group: row sharding over `world` processes (torch.distributed group for the exchange).
    """

    def __init__(self, data, length_scale, var=1.0, noise=1e-6, pdist=None, *, device=None, rank=0, world=1,
                 group=None, capacity=None):
        if pdist is not None:
            raise NotImplementedError("pre-computed distances are a dense-kernel feature of the reference (gp.py:116-128)")
        if not torch.cuda.is_available():
            raise RuntimeError("ital_amd.GaussianProcess needs a HIP device (no CPU fallback)")
        self._lib = _lib.lib()
        self.device = torch.device(device if device is not None else "cuda:0")
        self.rank, self.world, self.group = int(rank), int(world), group
        # the exchange steps run whenever there is more than one rank -- or, with ITAL_FORCE_COLLECTIVES=1, also on a
        # one-rank process group (lets a single-GPU box drive the RCCL code path end to end)
        self.collective = self.world > 1 or (group is not None and os.environ.get("ITAL_FORCE_COLLECTIVES") == "1")
        local = None
        if isinstance(data, torch.Tensor):
            if self.world > 1:
                raise NotImplementedError("a tensor is kept as a DeviceData, which is not sharded: pass ShardedRows to several ranks")
            data = DeviceData(data, device=self.device)
        self.store = data if isinstance(data, DeviceData) else None
        #: the epoch of the store's change log this model has seen (sync_data), and what its last call found there
        self._epoch = self.store.epoch if self.store is not None else 0
        self.last_index_map, self.last_removals = None, []
        if self.store is not None:
            if self.world > 1 and self.store.storage != torch.float64:
                raise NotImplementedError("a compact store (DeviceData(storage='source'), %s rows) cannot be used by several "
                                          "ranks: row sharding reads FP64 rows" % self.store.storage)
            if self.world > 1:
                raise NotImplementedError("a DeviceData is not sharded: pass ShardedRows to several ranks")
            if self.store.device != self.device:
                raise ValueError("the DeviceData lives on %s, this model on %s" % (self.store.device, self.device))
        elif isinstance(data, sharding.ShardedRows):
            local = data
        else:
            data = np.asarray(data, dtype=np.float64)
        if data.ndim != 2:
            raise ValueError("data must be an n-by-d array")
        self.n_total, self.d = data.shape
        self.row0, self.row1 = sharding.row_range(self.n_total, self.world, self.rank)
        if local is not None and (local.row0, local.row1) != (self.row0, self.row1):
            raise ValueError("ShardedRows holds rows [%d, %d), this rank owns [%d, %d)"
                             % (local.row0, local.row1, self.row0, self.row1))
        self.n = self.row1 - self.row0
        self.ldx = _pad16(self.d)
        self.ldv = _pad16(max(self.n, 1))
        self.length_scale = length_scale
        self.length_scale_sq = length_scale * length_scale
        self.var = var
        self.noise = noise
        self.X_host = data if self.store is None else None  # the reference keeps a copy too (gp.py:122)
        with torch.cuda.device(self.device):
            if self.store is not None:
                # views of the shared rows up to THIS model's row count: no upload, no norms launch
                self.Xd, self.xnorm = self.store.X, self.store.xnorm
            else:
                Xp = torch.zeros((max(self.n, 1), self.ldx), dtype=torch.float64, device=self.device)
                if self.n:
                    rows = local.local if local is not None else data[self.row0:self.row1]
                    Xp[: self.n, : self.d] = torch.from_numpy(np.ascontiguousarray(rows)).to(self.device)
                self.Xd = Xp
                self.xnorm = torch.empty(max(self.n, 1), dtype=torch.float64, device=self.device)
                check(self._lib.ital_row_norms(_ptr(self.Xd), self.n, self.ldx, _ptr(self.xnorm), _stream()))
            # element type of Xd (the INGEST_* codes): FP64 unless the rows are views of a compact store, whose readers are
            # the typed entry points of include/ital_rows.h
            self.xtype = DTYPE_CODES[self.Xd.dtype]
            self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._gather_bufs = {}
            if capacity is None:
                # room for 256 labelled samples (a session of 60 rounds of 4) unless the whitened block V would take more
                # than 2 GiB up front; growing later costs a reallocation and a copy of V and of the batch buffers (13 ms
                # at 9298 rows: visible in a 3 ms round)
                capacity = int(min(256, max(64, (2 << 30) // (8 * self.ldv))))
            self._alloc(capacity)
        self.reset()

    # ------------------------------------------------------------------ storage
    def _alloc(self, cap):
        cap = _pad16(cap)
        dev = self.device
        old = getattr(self, "cap", 0)
        V = torch.zeros((cap, self.ldv), dtype=torch.float64, device=dev)
        # the kernels use the lower triangle only (ital_chol_append loads the strict upper triangle of the diagonal blocks
        # without using it, csrc/chol.hip); the zeros there serve the host side (_factor, state_dict)
        L = torch.zeros((cap, cap), dtype=torch.float64, device=dev)
        alpha = torch.zeros(cap, dtype=torch.float64, device=dev)
        XT = torch.zeros((cap, self.ldx), dtype=torch.float64, device=dev)
        XTn = torch.zeros(cap, dtype=torch.float64, device=dev)
        if old:
            V[:old] = self.V
            L[:old, :old] = self.L
            alpha[:old] = self.alpha
            XT[:old] = self.XT
            XTn[:old] = self.XTn
        self.V, self.L, self.alpha, self.XT, self.XTn, self.cap = V, L, alpha, XT, XTn, cap

    @property
    def X(self):
        return self.X_host if self.store is None else self.store.rows()[: self.n_total]

    @property
    def K_all(self):
        raise AttributeError("the dense N x N kernel matrix is never formed by ital_amd (reference gp.py:128 is "
                             "replaced by column streaming); use rbf_cols()")

    # attributes of the reference's GP that derive from the m x m Gram matrix of the labelled samples: reconstructed on
    # demand from the Cholesky factor kept on the device (K = L L^T includes the noise term, as gp.py:156)
    def _factor(self):
        return self.L[: self.m, : self.m].cpu().numpy()

    @property
    def K(self):
        if self.m == 0:
            return None
        f = self._factor()
        return f @ f.T

    @property
    def K_inv(self):
        if self.m == 0:
            return None
        fi = np.linalg.inv(self._factor())
        return fi.T @ fi

    @property
    def w(self):
        if self.m == 0:
            return None
        import scipy.linalg
        return scipy.linalg.solve_triangular(self._factor(), self.alpha[: self.m].cpu().numpy(), lower=True, trans="T")

    def kernel(self, a, b=None):
        """RBF kernel between the rows of `a` and of `b` (default: the labelled samples vs `a`, as reference
        gp.py:390-416), computed by ital_cov_block (FP64 MFMA) with an empty whitened part."""
        if b is None:
            if self.m == 0:
                raise RuntimeError("the GP has not been fitted")
            a, b = self.XT[: self.m, : self.d].cpu().numpy(), a
        a = np.atleast_2d(np.asarray(a, dtype=np.float64))
        b = np.atleast_2d(np.asarray(b, dtype=np.float64))
        dev = self.device
        A = torch.zeros((len(a), self.ldx), dtype=torch.float64, device=dev)
        B = torch.zeros((len(b), self.ldx), dtype=torch.float64, device=dev)
        A[:, : self.d] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        B[:, : self.d] = torch.from_numpy(np.ascontiguousarray(b)).to(dev)
        an = torch.empty(len(a), dtype=torch.float64, device=dev)
        bn = torch.empty(len(b), dtype=torch.float64, device=dev)
        out = torch.empty((len(a), _pad16(len(b))), dtype=torch.float64, device=dev)
        st = _stream()
        check(self._lib.ital_row_norms(_ptr(A), len(a), self.ldx, _ptr(an), st))
        check(self._lib.ital_row_norms(_ptr(B), len(b), self.ldx, _ptr(bn), st))
        check(self._lib.ital_cov_block(_ptr(A), _ptr(an), len(a), _ptr(B), _ptr(bn), len(b), self.ldx, 0, 0, 0, 0, 0,
                                       float(self.var), float(self.length_scale), _ptr(out), out.shape[1], st))
        return out[:, : len(b)].cpu().numpy()

    def reset(self):
        """Back to the state right after __init__ (reference gp.py:132-138)."""
        self.ind = []
        self.y = None
        self.m = 0
        self.appends = []          # sizes of the update() calls that built the labelled set (state_dict / replay)
        self.label_noise = np.zeros(0)       # extra noise variance of every labelled sample, aligned with ind (reweigh)
        self.mu = torch.zeros(max(self.n, 1), dtype=torch.float64, device=self.device)
        self.s2 = torch.full((max(self.n, 1),), float(self.var), dtype=torch.float64, device=self.device)
        self.mu_all = torch.zeros(self.n_total, dtype=torch.float64, device=self.device) if self.collective else self.mu[: self.n]
        self._mean_host = None
        self.status.zero_()

    # ------------------------------------------------------------------ fitting
    def fit(self, ind, y):
        """Fits to a subset of the data (reference gp.py:141-161)."""
        self.reset()
        return self.update(ind, y)

    def update(self, ind, y, row_cache=None):
        """Adds labelled samples (reference gp.py:164-200), as a rank-c Cholesky append.

        `row_cache`: optional (device matrix [k, ldx], {data index: row of that matrix}) holding feature rows that are
        already replicated on every rank -- the batch state of the last fetch_unlabelled: the winners' rows travelled in
        the selection records, so labelling them needs no further exchange between the ranks."""
        ind = [int(i) for i in ind]
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        if len(ind) != len(y):
            raise ValueError("ind and y differ in length")
        if len(ind) == 0:
            return self
        hc = getattr(self, "host_clock", None)       # bench.py: where the host's time between two rounds goes
        t0 = time.perf_counter() if hc is not None else 0.0
        if row_cache is not None and all(i in row_cache[1] for i in ind):
            if len(ind) <= 16:
                self._append_staged(row_cache[0], [row_cache[1][i] for i in ind], y)
            else:
                slots = torch.as_tensor([row_cache[1][i] for i in ind], dtype=torch.int64, device=self.device)
                self._append(row_cache[0].index_select(0, slots), y)
        else:
            self._append(self._gather_rows(ind), y)
        self.ind += ind
        self.y = y.copy() if self.y is None else np.concatenate((self.y, y))
        self.label_noise = np.concatenate((self.label_noise, np.zeros(len(ind))))
        self.appends.append(len(ind))
        t1 = time.perf_counter() if hc is not None else 0.0
        self._replicate_mean()
        if hc is not None:
            hc["append_s"] = hc.get("append_s", 0.0) + (t1 - t0)
            hc["means_s"] = hc.get("means_s", 0.0) + (time.perf_counter() - t1)
        return self

    def update_points(self, points, y, ind=None):
        """Adds labelled feature vectors that are not rows of the data matrix (the reference appends queries as
        extra rows, ital/retrieval_base.py:40,56-58)."""
        pts = np.atleast_2d(np.asarray(points, dtype=np.float64))
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        rows = torch.zeros((len(pts), self.ldx), dtype=torch.float64, device=self.device)
        rows[:, : self.d] = torch.from_numpy(np.ascontiguousarray(pts)).to(self.device)
        self._append(rows, y)
        self.ind += list(ind) if ind is not None else list(range(self.n_total + self.m - len(y), self.n_total + self.m))
        self.y = y.copy() if self.y is None else np.concatenate((self.y, y))
        self.label_noise = np.concatenate((self.label_noise, np.zeros(len(y))))
        self.appends.append(-len(y))          # negative: feature vectors that are not rows of the data (queries)
        self._replicate_mean()
        return self

    def _owned(self, ind):
        """Host-side ownership of global indices: (mask as a float64 device column, clamped local indices on the device).
        Worked out with numpy -- a device-side mask would cost a nonzero() and a host synchronisation per use."""
        idx = np.asarray([int(i) for i in ind], dtype=np.int64)
        own = (idx >= self.row0) & (idx < self.row1)
        loc = np.where(own, idx - self.row0, 0)
        return (torch.from_numpy(own.astype(np.float64)).to(self.device),
                torch.from_numpy(loc).to(self.device), bool(own.any()))

    def _gather_rows(self, ind):
        """Feature rows of global indices, replicated on every rank (owners contribute, the rest adds zeros)."""
        if not self.collective:
            idx = torch.as_tensor(ind, dtype=torch.int64, device=self.device)
            # every row is local: no ownership test, no host synchronisation (a compact store's rows are widened: exact)
            return self.Xd.index_select(0, idx).to(torch.float64)
        mask, loc, any_own = self._owned(ind)
        if any_own:
            rows = self.Xd.index_select(0, loc).to(torch.float64) * mask[:, None]
        else:
            rows = torch.zeros((len(ind), self.ldx), dtype=torch.float64, device=self.device)
        sharding.all_reduce_sum(rows, self.group)
        return rows

    def gather_columns(self, mat, ind):
        """mat[:, local column of each global index] replicated on every rank ([rows, len(ind)]); `mat` holds one column
        per local data row (V, or covariance columns)."""
        mask, loc, any_own = self._owned(ind)
        if any_own:
            out = mat.index_select(1, loc) * mask[None, :]
        else:
            out = torch.zeros((mat.shape[0], len(loc)), dtype=torch.float64, device=self.device)
        if self.collective:
            sharding.all_reduce_sum(out, self.group)
        return out

    def _append_staged(self, matrix, slots, y):
        """_append for up to 16 samples whose feature rows are rows `slots` of a replicated device matrix (the batch state
        of the last fetch): ONE call (ital_gp_append: staging + Cholesky append in one launch, then the whitening sweep)
        instead of gather, copies, norms, a label upload and three calls."""
        c = len(slots)
        if self.m + c > self.cap:
            self._alloc(max(2 * self.cap, self.m + c))
        if getattr(self, "_ybuf", None) is None:
            self._ybuf = torch.empty(16, dtype=torch.float64, device=self.device)
        d = getattr(self, "_append_desc", None)
        key = (self.V.data_ptr(), self.mu.data_ptr(), self.cap)
        if d is None or d[0] != key:          # the pointers only change when the labelled-set buffers are re-allocated
            a = _lib.ItalAppendDesc()
            a.ldx, a.X, a.xnorm, a.n = self.ldx, _ptr(self.Xd), _ptr(self.xnorm), self.n
            a.XT, a.XTn, a.L, a.ldl, a.alpha, a.ybuf = _ptr(self.XT), _ptr(self.XTn), _ptr(self.L), self.cap, _ptr(self.alpha), \
                _ptr(self._ybuf)
            a.V, a.ldv, a.mu, a.s2, a.status = _ptr(self.V), self.ldv, _ptr(self.mu), _ptr(self.s2), _ptr(self.status)
            self._append_desc = d = (key, a)
        a = d[1]
        a.rows, a.m = _ptr(matrix), self.m
        a.var, a.length_scale, a.noise = float(self.var), float(self.length_scale), float(self.noise)
        a.lb.c = c
        for j in range(c):
            a.lb.slot[j] = int(slots[j])
            a.lb.y[j] = float(y[j])
        check(_lib.rows_fn("ital_gp_append", self.xtype)(ctypes.byref(a), _stream()))
        self.m += c

    def _append(self, rows, y):
        lib, st = self._lib, _stream()
        whiten_append = _lib.rows_fn("ital_whiten_append", self.xtype)
        c_total = rows.shape[0]
        if self.m + c_total > self.cap:
            self._alloc(max(2 * self.cap, self.m + c_total))
        yd = torch.from_numpy(np.ascontiguousarray(y)).to(self.device)
        for c0 in range(0, c_total, 16):
            c = min(16, c_total - c0)
            m = self.m
            self.XT[m:m + c] = rows[c0:c0 + c]
            check(lib.ital_row_norms(_ptr(self.XT[m:m + c]), c, self.ldx, _ptr(self.XTn[m:m + c]), st))
            check(lib.ital_chol_append(_ptr(self.XT), _ptr(self.XTn), self.ldx, _ptr(self.L), self.cap, _ptr(self.alpha),
                                       _ptr(yd[c0:c0 + c]), m, c, float(self.var), float(self.length_scale),
                                       float(self.noise), _ptr(self.status), st))
            L21 = self.L[m:]
            check(whiten_append(_ptr(self.Xd), _ptr(self.xnorm), self.n, self.ldx, _ptr(self.XT[m:m + c]),
                                _ptr(self.XTn[m:m + c]), c, _ptr(L21), self.cap,
                                L21.data_ptr() + 8 * m, _ptr(self.alpha[m:m + c]), _ptr(self.V), self.ldv, m,
                                float(self.var), float(self.length_scale), _ptr(self.mu), _ptr(self.s2), st))
            self.m += c

    def remove(self, ind):
        """Takes labelled samples (data indices) out of the model again: afterwards the state is what fitting the surviving
        samples in their order gives (up to rounding).  The reference has no such call -- a label, once given, stays
        (retrieval_base.py:183-189), its way back is fit() on the survivors, gp.py:141-161; here each sample leaves by a row
        deletion of the Cholesky factor and one orthogonal sweep over the whitened block (ital_gp_remove), highest
        labelled position first: those sweeps are the shortest and shift nothing below them.  Every rank makes the same
        call (L, alpha, XT are replicated, V is column-sharded: no exchange beyond the replicated means).

        ValueError for an index that has no label, one named twice and for a query row (>= number of samples: queries are
        part of the learner's construction); nothing is changed then.  An empty list is a no-op."""
        ind = [int(i) for i in ind]
        if not ind:
            return self
        if len(set(ind)) != len(ind):
            raise ValueError("a sample is named twice")
        pos_of = {i: p for p, i in enumerate(self.ind)}
        for i in ind:
            if i >= self.n_total:
                raise ValueError("%d is a query row: queries cannot be removed" % i)
            if i not in pos_of:
                raise ValueError("sample %d has no label" % i)
        lib, st = self._lib, _stream()
        need = int(lib.ital_gp_remove_workspace(self.cap))
        work = getattr(self, "_remove_work", None)
        if work is None or work.numel() < need:
            self._remove_work = work = torch.empty(need, dtype=torch.float64, device=self.device)
        r = _lib.ItalRemoveDesc()
        r.XT, r.XTn, r.ldx, r.L, r.ldl, r.alpha = _ptr(self.XT), _ptr(self.XTn), self.ldx, _ptr(self.L), self.cap, _ptr(self.alpha)
        r.V, r.ldv, r.n, r.mu, r.s2 = _ptr(self.V), self.ldv, self.n, _ptr(self.mu), _ptr(self.s2)
        r.work, r.work_doubles, r.status = _ptr(work), work.numel(), _ptr(self.status)
        for p in sorted((pos_of[i] for i in ind), reverse=True):
            r.m, r.p = self.m, p
            check(lib.ital_gp_remove(ctypes.byref(r), st))
            self.appends = appends_after_remove(self.appends, p)
            del self.ind[p]
            self.y = np.delete(self.y, p)
            self.label_noise = np.delete(self.label_noise, p)
            self.m -= 1
        if self.m == 0:
            self.reset()              # nothing is left: the prior, exactly (the kernels left rows >= m of V, L, XT zero)
        self._replicate_mean()
        return self

    # ------------------------------------------------------------------ trusting a label less, without taking it back
    def _reweigh_call(self, L, alpha, status, pos, delta, factor_only=False):
        """One ital_gp_reweigh call over the factor (L, alpha) -- and, unless `factor_only`, this rank's V, mu, s2 -- for the
        labelled positions `pos` (strictly increasing) whose diagonal entry changes by `delta`; `status`: the word it may
        set.  The host arrays are read before the call returns."""
        lib, r = self._lib, len(pos)
        need = int(lib.ital_gp_reweigh_workspace(self.m, r))
        work = getattr(self, "_reweigh_work", None)
        if work is None or work.numel() < need:
            self._reweigh_work = work = torch.empty(need, dtype=torch.float64, device=self.device)
        d = _lib.ItalReweighDesc()
        d.L, d.ldl, d.alpha, d.m = _ptr(L), self.cap, _ptr(alpha), self.m
        if factor_only:
            d.V, d.ldv, d.n, d.mu, d.s2 = None, 0, 0, None, None
        else:
            d.V, d.ldv, d.n, d.mu, d.s2 = _ptr(self.V), self.ldv, self.n, _ptr(self.mu), _ptr(self.s2)
        d.work, d.work_doubles, d.status, d.r = _ptr(work), work.numel(), _ptr(status), r
        cpos = (ctypes.c_int * r)(*[int(p) for p in pos])
        cdelta = (ctypes.c_double * r)(*[float(v) for v in delta])
        d.pos, d.delta = ctypes.cast(cpos, ctypes.c_void_p), ctypes.cast(cdelta, ctypes.c_void_p)
        check(lib.ital_gp_reweigh(ctypes.byref(d), _stream()))

    def reweigh(self, ind, extra):
        """Sets the extra noise variance of labelled samples (data indices `ind`; `extra`: one value >= 0 for all of them or
        one per index): the model becomes the GP on K_TT + noise I + diag(label_noise), with labels, labelled order and
        `appends` as they are.  The value is absolute -- a call sets it, 0 is a label of full weight again, a large one
        approaches remove([i]).  The factor's trailing block goes through one rank-one update or downdate per changed
        label and V through ONE sweep for up to eight of them (ital_gp_reweigh); no feature row is read.  Every rank makes
        the same call.  The reference has nothing like it: its noise is one scalar (gp.py:156).

        ValueError (nothing is changed) for an index that has no label, one named twice, a query row, a negative or
        non-finite value.  An empty list, or values that all equal the present ones, is a no-op without a launch.
        LinAlgError when the device refused (a pivot of the downdate was not positive): the model is then as it was."""
        ind = [int(i) for i in ind]
        extra = np.asarray(extra, dtype=np.float64)
        if extra.ndim == 0:
            extra = np.full(len(ind), float(extra))
        extra = extra.reshape(-1)
        if len(extra) != len(ind):
            raise ValueError("ind and extra differ in length")
        if not np.all(np.isfinite(extra)) or np.any(extra < 0):
            raise ValueError("the extra noise of a label must be finite and >= 0")
        if len(set(ind)) != len(ind):
            raise ValueError("a sample is named twice")
        pos_of = {i: p for p, i in enumerate(self.ind)}
        for i in ind:
            if i >= self.n_total:
                raise ValueError("%d is a query row: queries keep their full weight" % i)
            if i not in pos_of:
                raise ValueError("sample %d has no label" % i)
        changes = sorted((pos_of[i], float(v)) for i, v in zip(ind, extra) if float(v) != self.label_noise[pos_of[i]])
        if not changes:
            return self
        pos = [p for p, _ in changes]
        delta = [v - float(self.label_noise[p]) for p, v in changes]
        with torch.cuda.device(self.device):
            status = torch.zeros(1, dtype=torch.int32, device=self.device)     # the call's own word: a refusal changes nothing
            self._reweigh_call(self.L, self.alpha, status, pos, delta)
            self.check_status(int(status.item()))
            for p, v in changes:
                self.label_noise[p] = v
            self._replicate_mean()
        return self

    def _no_label_noise(self, what):
        """ValueError while any label carries extra noise: `what` rebuilds Grams from XT with the scalar noise alone."""
        if np.any(self.label_noise != 0):
            raise ValueError("%s does not know the per-label noise of this session yet: clear it first with "
                             "set_label_noise / reweigh(ind, 0)" % what)

    # ------------------------------------------------------------------ what a removal would change, without making it
    def _influence_desc(self, mask=None):
        """ital_influence_desc over this rank's state with its output tables; the tensors it points to ride along."""
        lib = self._lib
        need = int(lib.ital_gp_influence_workspace(self.m, self.n))
        work = getattr(self, "_influence_work", None)
        if work is None or work.numel() < need:
            self._influence_work = work = torch.empty(need, dtype=torch.float64, device=self.device)
        keep = dict(work=work, coef=torch.empty((self.m, 2), dtype=torch.float64, device=self.device),
                    stats=torch.empty((self.m, 4), dtype=torch.float64, device=self.device),
                    # a word of its own: a broken factor shows as NaN rows here and leaves the session's status alone
                    status=torch.zeros(1, dtype=torch.int32, device=self.device), mask=mask)
        d = _lib.ItalInfluenceDesc()
        d.L, d.ldl, d.alpha, d.m = _ptr(self.L), self.cap, _ptr(self.alpha), self.m
        d.V, d.ldv, d.n, d.mu, d.s2 = _ptr(self.V), self.ldv, self.n, _ptr(self.mu), _ptr(self.s2)
        d.mask = _ptr(mask) if mask is not None else None
        d.coef, d.stats, d.work, d.work_doubles, d.status = _ptr(keep["coef"]), _ptr(keep["stats"]), _ptr(work), work.numel(), \
            _ptr(keep["status"])
        return d, keep

    def influence(self, mask=None):
        """What taking each labelled sample back would change, for all of them in one pass over the whitened block
        (ital_gp_influence: the product L^-1^T V on FP64 MFMA, nothing of size m x N stored, the state only read).  Returns a
        dict of arrays in labelled order (the order of `ind`): c = diag K^-1, w = K^-1 y, loo_mean = y - w / c and
        loo_var = 1 / c (R&W 5.12), and over the rows that `mask` (bool over all samples; None: all) counts: dmu_sq, the
        summed squared change of the predictive mean; dmu_max, its largest absolute change; flips, the rows whose mean
        changes sign; ds2, the total predictive variance the label removes.  A label whose c is not positive and finite (a
        factor that was broken before) has NaN everywhere.  Several ranks: every rank makes the call; sums add, maxima take
        the max."""
        if self.m == 0:
            raise RuntimeError("the GP has not been fitted: call fit()/update() first")
        dmask = None
        if mask is not None:
            mask = np.asarray(mask)
            if mask.shape != (self.n_total,):
                raise ValueError("mask must name every one of the %d samples" % self.n_total)
            dmask = torch.from_numpy(np.ascontiguousarray(mask[self.row0:self.row1] != 0).astype(np.uint8)).to(self.device)
            if dmask.numel() == 0:
                dmask = torch.zeros(1, dtype=torch.uint8, device=self.device)
        d, keep = self._influence_desc(dmask)
        check(self._lib.ital_gp_influence(ctypes.byref(d), _stream()))
        coef = keep["coef"].cpu().numpy()
        stats = keep["stats"]
        if self.collective:
            stats = sharding.all_gather_parts(stats.reshape(-1), [4 * self.m] * self.world, self.group)
            parts = stats.cpu().numpy().reshape(self.world, self.m, 4)
            stats = parts.sum(axis=0)
            stats[:, 1] = parts[:, :, 1].max(axis=0)
        else:
            stats = stats.cpu().numpy()
        c, w = coef[:, 0].copy(), coef[:, 1].copy()
        y = np.asarray(self.y, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return dict(c=c, w=w, loo_mean=y - w / c, loo_var=1.0 / c, dmu_sq=stats[:, 0].copy(), dmu_max=stats[:, 1].copy(),
                        flips=stats[:, 2].copy(), ds2=stats[:, 3].copy())

    def preview_remove(self, ind):
        """Predictive mean and variance of every sample as they would be after remove([i]), one row per listed labelled
        sample i (data indices; each row is a removal of that sample alone), with no change of state: (mean[r, N], var[r, N]),
        full length on every rank.  ValueError as remove() for an index without a label and for a query row."""
        ind = [int(i) for i in ind]
        pos_of = {i: p for p, i in enumerate(self.ind)}
        for i in ind:
            if i >= self.n_total:
                raise ValueError("%d is a query row: queries cannot be removed" % i)
            if i not in pos_of:
                raise ValueError("sample %d has no label" % i)
        r = len(ind)
        if r == 0:
            return np.zeros((0, self.n_total)), np.zeros((0, self.n_total))
        d, keep = self._influence_desc()
        mu_out = torch.zeros((r, self.ldv), dtype=torch.float64, device=self.device)
        s2_out = torch.zeros((r, self.ldv), dtype=torch.float64, device=self.device)
        sel = (ctypes.c_int * r)(*[pos_of[i] for i in ind])
        check(self._lib.ital_gp_preview_remove(ctypes.byref(d), sel, r, _ptr(mu_out), _ptr(s2_out), self.ldv, _stream()))
        mean = np.stack([self._full(mu_out[q]) for q in range(r)])
        var = np.stack([self._full(s2_out[q]) for q in range(r)])
        return mean, np.maximum(0, var)

    # ------------------------------------------------------------------ a live session: more rows, other hyper-parameters
    def _whiten_rows(self, row_start, n_rows, x_row_start=None):
        """xnorm, V[0:m], mu, s2 of the local rows [row_start, row_start + n_rows) against the whole current labelled set
        (ital_whiten_rows: the feature rows are read ceil(m / chunk) times, not ceil(m / 16) times); rows m .. cap of V zero.
        On a compact store xnorm is only read: the store wrote it with the rows.  x_row_start: where the feature rows and
        their norms stand in Xd / xnorm, if not at row_start (sync_data, while it walks a log)."""
        x0 = row_start if x_row_start is None else x_row_start
        r = _lib.ItalRewhitenDesc()
        r.X, r.n_rows, r.ldx = self.Xd.data_ptr() + self.Xd.element_size() * x0 * self.ldx, n_rows, self.ldx
        r.XT, r.XTn, r.L, r.ldl, r.alpha, r.m = _ptr(self.XT), _ptr(self.XTn), _ptr(self.L), self.cap, _ptr(self.alpha), self.m
        r.var, r.length_scale = float(self.var), float(self.length_scale)
        r.xnorm, r.V, r.ldv, r.v_rows = self.xnorm.data_ptr() + 8 * x0, self.V.data_ptr() + 8 * row_start, self.ldv, self.cap
        r.mu, r.s2, r.chunk = self.mu.data_ptr() + 8 * row_start, self.s2.data_ptr() + 8 * row_start, 0
        check(_lib.rows_fn("ital_whiten_rows", self.xtype)(ctypes.byref(r), _stream()))

    def extend(self, rows):
        """Appends samples to the data matrix of a live model: they get the indices n_total .. n_total + len(rows) - 1.  The
        buffers indexed by row (Xd, xnorm, V with its new leading dimension, mu, s2) grow by device-to-device copies -- no
        feature of an existing row is uploaded again, none of their whitened columns recomputed -- and the new range alone
        is whitened against the labelled set (ital_whiten_rows).  Queries are labelled rows numbered from n_total on: their
        entries of `ind` move up by len(rows).  The reference has no such call: its dense K_all (gp.py:128) is built once.

        An empty array is a no-op; ValueError (nothing changed) for another number of columns; NotImplementedError on
        several ranks: row sharding cannot grow yet.  On a DeviceData: store.append(rows), then sync_data()."""
        if self.store is not None:
            self.store.append(rows)
            self.sync_data()
            return self
        rows = np.asarray(rows, dtype=np.float64)
        if rows.size == 0:
            return self
        if rows.ndim != 2 or rows.shape[1] != self.d:
            raise ValueError("rows must be a k-by-%d array" % self.d)
        if self.world > 1 or not isinstance(self.X_host, np.ndarray):
            raise NotImplementedError("row sharding cannot grow yet: extend() needs all rows on one rank")
        k, n_old, m, dev = len(rows), self.n, self.m, self.device
        n_new = n_old + k
        ldv = _pad16(n_new)
        with torch.cuda.device(dev):
            Xd = torch.zeros((n_new, self.ldx), dtype=torch.float64, device=dev)
            Xd[:n_old] = self.Xd[:n_old]
            Xd[n_old:, : self.d] = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
            xnorm = torch.empty(n_new, dtype=torch.float64, device=dev)
            mu = torch.empty(n_new, dtype=torch.float64, device=dev)
            s2 = torch.empty(n_new, dtype=torch.float64, device=dev)
            V = torch.zeros((self.cap, ldv), dtype=torch.float64, device=dev)
            xnorm[:n_old], mu[:n_old], s2[:n_old] = self.xnorm[:n_old], self.mu[:n_old], self.s2[:n_old]
            if m and n_old:
                V[:m, :n_old] = self.V[:m, :n_old]
            self.Xd, self.xnorm, self.mu, self.s2, self.V = Xd, xnorm, mu, s2, V
            self.n, self.ldv = n_new, ldv
            self.ind = [i + k if i >= self.n_total else i for i in self.ind]
            self.n_total += k
            self.row1 = self.row0 + n_new
            self.X_host = np.concatenate((self.X_host, rows))
            self._append_desc = None          # it holds X, xnorm, n and ldv
            self._gather_bufs = {}
            self._whiten_rows(n_old, k)
            self._replicate_mean()
        return self

    # ------------------------------------------------------------------ a live session: rows leave
    def _compact_cols(self, keep):
        """V, mu, s2 <- their columns `keep` (ascending int64 numpy array of local rows) in new tensors with the leading
        dimension of len(keep) rows (ital_compact_cols: bits kept, V zero outside [0:m, 0:len(keep))); n, n_total, row1 and
        ldv follow.  Xd and xnorm are the caller's business.  The status word collects an index outside the rows."""
        n_new, dev = len(keep), self.device
        ldv = _pad16(max(n_new, 1))
        keep_d = torch.from_numpy(np.ascontiguousarray(keep, dtype=np.int64)).to(dev)
        V = torch.empty((self.cap, ldv), dtype=torch.float64, device=dev)
        mu = torch.zeros(max(n_new, 1), dtype=torch.float64, device=dev) if n_new == 0 else \
            torch.empty(n_new, dtype=torch.float64, device=dev)
        s2 = torch.full((1,), float(self.var), dtype=torch.float64, device=dev) if n_new == 0 else \
            torch.empty(n_new, dtype=torch.float64, device=dev)
        check(self._lib.ital_compact_cols(_ptr(self.V), self.ldv, self.m, _ptr(self.mu), _ptr(self.s2), self.n, _ptr(keep_d),
                                          n_new, _ptr(V), ldv, self.cap, _ptr(mu), _ptr(s2), _ptr(self.status), _stream()))
        self.V, self.mu, self.s2, self.ldv = V, mu, s2, ldv
        self.n_total -= self.n - n_new
        self.n = n_new
        self.row1 = self.row0 + n_new
        self._append_desc = None              # it holds X, xnorm, n and ldv
        self._gather_bufs = {}
        return keep_d

    def _renumber(self, removed):
        """`ind` after the data rows `removed` (ascending, none of them labelled any more) have left: data rows move down by
        the number of removed rows below them, query rows by all of them."""
        import bisect
        self.ind = [i - bisect.bisect_left(removed, i) for i in self.ind]

    def drop_rows(self, ids):
        """Deletes samples from the data matrix of a live model that owns its rows, like np.delete(X, ids, axis=0): the
        survivors keep their order and get the indices 0 .. n_total - r - 1.  The labelled ones among `ids` first leave the
        model through remove() (a Cholesky row deletion and one sweep each, in that method's order); what is left is a gather
        without arithmetic -- Xd, xnorm (ital_compact_rows) and V, mu, s2 (ital_compact_cols, into tensors with the new leading
        dimension) keep the bits of every survivor.  `ind` is renumbered: query rows move down by the number of removed rows.
        The reference has no such call: its dense K_all (gp.py:128) is built once.

        `ids`: any iterable of ints; duplicates are collapsed, negative ones count from the end.  An empty list is a no-op.
        ValueError (nothing changed) for a query row or any id >= n_total and for removing every row, IndexError for one
        below -n_total; NotImplementedError on several ranks: row sharding cannot shrink yet.  On a DeviceData:
        store.remove(ids), then sync_data()."""
        from .device_data import compact_rows, keep_indices
        if self.world > 1 or (self.store is None and not isinstance(self.X_host, np.ndarray)):
            raise NotImplementedError("row sharding cannot shrink yet: drop_rows() needs all rows on one rank")
        if self.store is not None:
            raise ValueError("this model views the rows of a DeviceData: store.remove(ids), then sync_data()")
        n = self.n_total
        removed = set()
        for i in ids:
            i = int(i)
            if i >= n:
                raise ValueError("%d is a query row or outside the %d samples: it cannot be removed" % (i, n))
            if i < -n:
                raise IndexError("row index %d outside the %d rows" % (i, n))
            removed.add(i + n if i < 0 else i)
        removed = sorted(removed)
        if not removed:
            return self
        if len(removed) == n:
            raise ValueError("drop_rows() would leave no row")
        labelled = set(self.ind)
        labelled = [i for i in removed if i in labelled]
        with torch.cuda.device(self.device):
            if labelled:
                self.remove(labelled)
            keep = keep_indices(n, removed)
            n_old, Xd_old, xnorm_old = self.n, self.Xd, self.xnorm
            keep_d = self._compact_cols(keep)
            self.Xd = torch.empty((len(keep), self.ldx), dtype=Xd_old.dtype, device=self.device)
            self.xnorm = torch.empty(len(keep), dtype=torch.float64, device=self.device)
            compact_rows(Xd_old, xnorm_old, n_old, keep_d, self.Xd, self.xnorm, self.status)
            self.X_host = np.delete(self.X_host, removed, 0)
            self._renumber(removed)
            self._replicate_mean()
            self.check_status()
        return self

    def _grow_to_store(self, x_row0, k):
        """What sync_data() does for k appended rows: V (new leading dimension), mu and s2 grow by device-to-device copies
        and the new columns n .. n + k - 1 alone are whitened against the labelled set (ital_whiten_rows) -- from the rows
        x_row0 .. x_row0 + k - 1 of the store as it is NOW, which is where rows appended earlier in the log have moved to
        when rows below them have left since (x_row0 == n when none did)."""
        n_old, n_new, m, dev = self.n, self.n + k, self.m, self.device
        ldv = _pad16(n_new)
        mu = torch.empty(n_new, dtype=torch.float64, device=dev)
        s2 = torch.empty(n_new, dtype=torch.float64, device=dev)
        V = torch.zeros((self.cap, ldv), dtype=torch.float64, device=dev)
        mu[:n_old], s2[:n_old] = self.mu[:n_old], self.s2[:n_old]
        if m and n_old:
            V[:m, :n_old] = self.V[:m, :n_old]
        self.Xd, self.xnorm, self.mu, self.s2, self.V = self.store.X, self.store.xnorm, mu, s2, V
        self.n, self.ldv = n_new, ldv
        self.ind = [i + k if i >= self.n_total else i for i in self.ind]
        self.n_total += k
        self.row1 = self.row0 + n_new
        self._append_desc = None          # it holds X, xnorm, n and ldv
        self._gather_bufs = {}
        self._whiten_rows(n_old, k, x_row0)       # writes the new rows' xnorm again: the bits the store already holds

    def sync_data(self):
        """Catches up with the DeviceData this model was built on: walks the store's change log from the epoch this model has
        seen and applies its events in order.

        - Appended rows: what extend() does, minus the growth of Xd and xnorm -- V (new leading dimension), mu and s2 grow by
          device-to-device copies, the new range alone is whitened against the labelled set (ital_whiten_rows), query rows
          move up in `ind`.  Appends that follow one another are taken in as one range.
        - Removed rows: the labelled ones among them leave through remove() (a Cholesky row deletion and a sweep each), then V,
          mu and s2 are gathered (ital_compact_cols: no arithmetic), `ind` is renumbered.
        A row that was appended AND removed within the walked part of the log never enters the model; one that was appended
        and stayed is whitened from where it stands in the store now.  At the end Xd and xnorm are views of the store's rows
        and the means are replicated.

        Returns the number of rows gained (0: nothing was appended, or nothing of it is left).  `last_index_map` is the
        composed index map of the removals this call applied (int64 array of the old length: new index, or -1), None if there
        were none; `last_removals` their ascending id lists, each in the numbering the model had when it was applied.  Until
        sync_data() is called the model goes on on its own n rows, also across a reallocation of the store (its views keep the
        old tensors alive).  ValueError without a DeviceData."""
        if self.store is None:
            raise ValueError("this model owns its rows: build it on a DeviceData to share and grow them")
        store = self.store
        events = store.log[self._epoch:store.epoch]
        self.last_index_map, self.last_removals = None, []
        if not events:
            return 0
        # first pass, on the host: which of the rows appended in these events are still there at the end (by serial number)
        n0 = self.n
        serial, born = np.zeros(0, dtype=np.int64), 0
        old = n0
        for ev in events:
            if ev[0] == "append":
                serial = np.concatenate((serial, np.arange(born, born + ev[1], dtype=np.int64)))
                born += ev[1]
            else:
                ids = np.asarray(ev[1], dtype=np.int64)
                if ev[2] != old + len(serial):
                    raise RuntimeError("the store's log and this model's row count disagree")
                serial = np.delete(serial, ids[ids >= old] - old)
                old -= int((ids < old).sum())
        survivors = serial                      # ascending; survivor t stands in row `old + t` of the store now
        if old + len(survivors) != store.n:
            raise RuntimeError("the store's log and its row count disagree")
        alive = None                            # original indices of this model's first rows that are still there
        gained, born, pending, a = 0, 0, 0, n0
        with torch.cuda.device(self.device):
            def take_in():
                nonlocal pending, gained
                # the rows born in [born - pending, born) that survive: a contiguous range of the store's tail
                lo, hi = np.searchsorted(survivors, (born - pending, born))
                if hi > lo:
                    self._grow_to_store(old + int(lo), int(hi - lo))
                    gained += int(hi - lo)
                pending = 0

            for ev in events:
                if ev[0] == "append":
                    born += ev[1]
                    pending += ev[1]
                    continue
                take_in()
                removed = [i for i in ev[1] if i < a]      # the rest never entered the model
                if not removed:
                    continue
                if alive is None:
                    alive = np.arange(n0, dtype=np.int64)
                labelled = set(self.ind)
                labelled = [i for i in removed if i in labelled]
                if labelled:
                    self.remove(labelled)
                # the model's rows: the a rows it had before the walk that are left, then the survivors taken in so far
                self._compact_cols(np.delete(np.arange(self.n, dtype=np.int64), np.asarray(removed, dtype=np.int64)))
                self._renumber(removed)
                alive = np.delete(alive, np.asarray(removed, dtype=np.int64))
                a -= len(removed)
                self.last_removals.append(removed)
            take_in()
            self.Xd, self.xnorm = store.X, store.xnorm
            self._epoch = store.epoch
            if alive is not None:
                self.last_index_map = np.full(n0, -1, dtype=np.int64)
                self.last_index_map[alive] = np.arange(len(alive), dtype=np.int64)
            if self.n != store.n:
                raise RuntimeError("the store's log and this model's row count disagree")
            self._replicate_mean()
            if alive is not None:
                self.check_status()
        return gained

    def clone(self):
        """A second model on the same DeviceData in this model's state: same row count (also when the store has grown since),
        same hyper-parameters; V[:m], L, alpha, XT, XTn, mu, s2 and the status word are copied device to device, the labelled
        set and `appends` on the host.  Work buffers are not carried over.  ValueError for a model that owns its rows."""
        if self.store is None:
            raise ValueError("clone() shares the rows between the two models: build the model on a DeviceData "
                             "(ital_amd.DeviceData(data)) instead of a numpy array")
        g = object.__new__(GaussianProcess)
        g.__dict__.update(self.__dict__)
        for name in ("_append_desc", "_ybuf", "_remove_work", "_reweigh_work", "_topk_work", "host_clock"):
            g.__dict__.pop(name, None)
        g.ind, g.appends = list(self.ind), list(self.appends)
        g.y = None if self.y is None else self.y.copy()
        g.label_noise = self.label_noise.copy()
        with torch.cuda.device(self.device):
            g.V = torch.zeros_like(self.V)
            if self.m:
                g.V[: self.m] = self.V[: self.m]
            g.L, g.alpha, g.XT, g.XTn = self.L.clone(), self.alpha.clone(), self.XT.clone(), self.XTn.clone()
            g.mu, g.s2, g.status = self.mu.clone(), self.s2.clone(), self.status.clone()
            g._gather_bufs = {}
            g._replicate_mean()
        return g

    def set_params(self, length_scale=None, var=None, noise=None):
        """Other kernel hyper-parameters for a live model (None: as it is), e.g. what ital_amd.tune found: the factor and alpha
        are built anew in fresh buffers (ital_chol_append over the stored XT, y in blocks of 16) and, once the status word
        says the Gram was positive definite, swapped in; every local row is then whitened again (ital_whiten_rows) and the
        means replicated -- every rank makes the same call.  The per-label noise of reweigh() stays: it goes onto the new
        factor by one factor-only ital_gp_reweigh call before the swap.  LinAlgError leaves the model exactly as it was.
        What the parent offered instead: set the attributes and fit(ind, y), i.e. ceil(m/16) sweeps over X and V."""
        ls = float(self.length_scale if length_scale is None else length_scale)
        var = float(self.var if var is None else var)
        noise = float(self.noise if noise is None else noise)
        if not (ls > 0 and var > 0):
            raise ValueError("length_scale and var must be positive")
        with torch.cuda.device(self.device):
            if self.m == 0:
                self.s2.fill_(var)
            else:
                lib, st, m = self._lib, _stream(), self.m
                L = torch.zeros((self.cap, self.cap), dtype=torch.float64, device=self.device)
                alpha = torch.zeros(self.cap, dtype=torch.float64, device=self.device)
                status = torch.zeros(1, dtype=torch.int32, device=self.device)
                yd = torch.from_numpy(np.ascontiguousarray(self.y, dtype=np.float64)).to(self.device)
                for c0 in range(0, m, 16):
                    c = min(16, m - c0)
                    check(lib.ital_chol_append(_ptr(self.XT), _ptr(self.XTn), self.ldx, _ptr(L), self.cap, _ptr(alpha),
                                               _ptr(yd[c0:c0 + c]), c0, c, var, ls, noise, _ptr(status), st))
                pos = [int(p) for p in np.flatnonzero(self.label_noise)]
                if pos:                       # the per-label noise on top, factor only: the rows are whitened below anyway
                    self._reweigh_call(L, alpha, status, pos, [float(self.label_noise[p]) for p in pos], factor_only=True)
                self.check_status(int(status.item()))
                self.L, self.alpha = L, alpha
                self._append_desc = None      # it holds L and alpha
            self.length_scale, self.length_scale_sq, self.var, self.noise = ls, ls * ls, var, noise
            if self.m:
                self._whiten_rows(0, self.n)
                self._replicate_mean()
        return self

    def _evidence_run(self, params_list, max_bytes, events, shapes, chunk_of, desc_cls, entry, workspace, n_events, outputs):
        """What evidence(), evidence_grad() and loo_grad() share: the candidates go through `entry` (descriptor `desc_cls`, workspace
        function `workspace`) in chunks of at most `chunk_of(max_bytes)`, with y, the parameters, the Grams, the workspace,
        info and a status word of the call's own on the device; `events` (`n_events` of them) reach the last chunk only.
        `shapes`: name -> shape of one candidate's entry of each returned float64 array; `ok` [G] bool is added.
        `outputs(d, chunk)` allocates the chunk's output buffers, names them in the descriptor and returns
        download(out, g0, c), which copies the first c candidates' results to out[...][g0:g0 + c]."""
        if self.m == 0:
            raise RuntimeError("the GP has not been fitted")
        self._no_label_noise("the evidence family (evidence, evidence_grad, loo_grad, tune_params, fit_params, session_scores)")
        prm = _candidate_params(self, params_list)
        G, m, dev = len(prm), self.m, self.device
        out = {k: np.empty((G,) + s) for k, s in shapes.items()}
        out["ok"] = np.zeros(G, dtype=bool)
        if G == 0:
            return out
        chunk = min(G, chunk_of(max_bytes))
        with torch.cuda.device(dev):
            yd = torch.from_numpy(np.ascontiguousarray(self.y, dtype=np.float64)).to(dev)
            pd = torch.from_numpy(prm).to(dev)
            K = torch.empty(chunk * m * m, dtype=torch.float64, device=dev)
            need = int(workspace(m, chunk))
            work = torch.empty(need, dtype=torch.float64, device=dev)
            info = torch.empty(chunk, dtype=torch.int32, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)      # the call's own word: the model's is not touched
            d = desc_cls()
            d.XT, d.XTn, d.ldx, d.y, d.m = _ptr(self.XT), _ptr(self.XTn), self.ldx, _ptr(yd), m
            d.K, d.ld, d.info, d.status, d.work, d.work_doubles = _ptr(K), m, _ptr(info), _ptr(status), _ptr(work), need
            download = outputs(d, chunk)
            for g0 in range(0, G, chunk):
                c = min(chunk, G - g0)
                d.params, d.G = pd.data_ptr() + 24 * g0, c
                ev = None
                if events is not None and g0 + c == G:
                    ev = (ctypes.c_void_p * n_events)(*[e.cuda_event for e in events])
                d.ev = ctypes.addressof(ev) if ev is not None else None
                check(entry(ctypes.byref(d), _stream()))
                download(out, g0, c)                  # synchronises: the chunk's buffers are free again
                out["ok"][g0:g0 + c] = info[:c].cpu().numpy() == 0
        return out

    def evidence_chunk(self, max_bytes=1 << 30):
        """Candidates evidence() sends to the device at once so that their Grams, workspace and outputs stay below
        `max_bytes` (at most 65535, the limit of one ital_gp_evidence call); MemoryError if one candidate alone exceeds it."""
        m = self.m
        per = 8 * (m * m + int(self._lib.ital_gp_evidence_workspace(m, 1)) + 2 * m + 4)
        if per > max_bytes:
            raise MemoryError("one candidate at m = %d takes %d bytes, more than max_bytes = %d" % (m, per, max_bytes))
        return int(min(max_bytes // per, 65535))

    def evidence(self, params_list, *, max_bytes=1 << 30, events=None):
        """Scores hyper-parameter candidates against the model's own labelled set (queries included), without touching the
        model: for each dict of `params_list` (`length_scale`, optional `var` / `noise`; default: the model's current value)
        the log marginal likelihood and the closed-form leave-one-out quantities of include/ital_evidence.h.  Returns a dict
        of numpy arrays: `lml`, `loo_logp`, `loo_mse` [G], `ok` [G] bool (the candidate's Gram was positive definite;
        otherwise -inf, -inf, +inf and NaN rows), `loo_mean`, `loo_var` [G, m].  `params_list` may also be the candidates as
        a float64 [G, 3] array of (length_scale, var, noise) rows.

        The candidates go to the device in chunks whose Grams and workspace stay below `max_bytes` (ital_gp_evidence: a
        number of launches that does not depend on the chunk); a candidate's values do not depend on the chunking.  Reads
        XT, XTn and y and writes buffers of its own: L, alpha, V, mu, s2, the status word and both random streams stay as
        they are.  Every rank computes the same thing locally: no collective.  RuntimeError for an unfitted model,
        ValueError for a non-positive length_scale / var, MemoryError if one candidate alone exceeds max_bytes.
        `events`: None, or six recorded torch events that bracket the five stages of the LAST chunk (tools/evidence_bench.py)."""
        m = self.m

        def outputs(d, chunk):
            scores = torch.empty((chunk, 3), dtype=torch.float64, device=self.device)
            lm = torch.empty((chunk, m), dtype=torch.float64, device=self.device)
            lv = torch.empty((chunk, m), dtype=torch.float64, device=self.device)
            d.scores, d.loo_mean, d.loo_var, d.ldm = _ptr(scores), _ptr(lm), _ptr(lv), m

            def download(out, g0, c):
                sc = scores[:c].cpu().numpy()
                out["lml"][g0:g0 + c], out["loo_logp"][g0:g0 + c], out["loo_mse"][g0:g0 + c] = sc[:, 0], sc[:, 1], sc[:, 2]
                out["loo_mean"][g0:g0 + c] = lm[:c].cpu().numpy()
                out["loo_var"][g0:g0 + c] = lv[:c].cpu().numpy()
            return download

        return self._evidence_run(params_list, max_bytes, events, dict(lml=(), loo_logp=(), loo_mse=(), loo_mean=(m,), loo_var=(m,)),
                                  self.evidence_chunk, _lib.ItalEvidenceDesc, self._lib.ital_gp_evidence,
                                  self._lib.ital_gp_evidence_workspace, 6, outputs)

    def evidence_grad_chunk(self, max_bytes=1 << 30):
        """Candidates evidence_grad() sends to the device at once so that their Grams, workspace and outputs stay below
        `max_bytes` (at most 65535, the limit of one ital_gp_evidence_grad call); MemoryError if one candidate alone exceeds
        it.  The squared distances are shared by the candidates of a chunk and counted once."""
        m = self.m
        one, two = (int(self._lib.ital_gp_evidence_grad_workspace(m, c)) for c in (1, 2))
        per = 8 * (m * m + (two - one) + 5)
        shared = 8 * (2 * one - two)
        if shared + per > max_bytes:
            raise MemoryError("one candidate at m = %d takes %d bytes, more than max_bytes = %d" % (m, shared + per, max_bytes))
        return int(min((max_bytes - shared) // per, 65535))

    def evidence_grad(self, params_list, *, max_bytes=1 << 30, events=None):
        """The log marginal likelihood of hyper-parameter candidates on the model's own labelled set (queries included) and
        its gradient in the LOGARITHMS of the parameters, without touching the model: for each dict of `params_list`
        (`length_scale`, optional `var` / `noise`; default: the model's current value) the quantities of
        include/ital_evidence_grad.h.  Returns a dict of numpy arrays: `lml` [G] (the bits evidence() returns), `grad`
        [G, 3] (d lml / d log length_scale, d log var, d log noise), `ok` [G] bool (the candidate's Gram was positive
        definite; otherwise -inf and a NaN row).

        Argument handling, chunking and errors are those of evidence(): chunks whose Grams and workspace stay below
        `max_bytes`, values that do not depend on the chunking; XT, XTn and y are read and only buffers of the call's own are
        written -- L, alpha, V, mu, s2, the status word and both random streams stay as they are.  Every rank computes the same
        thing locally: no collective.  RuntimeError for an unfitted model, ValueError for a non-positive length_scale / var,
        MemoryError if one candidate alone exceeds max_bytes.
        `events`: None, or eight recorded torch events that bracket the seven stages of the LAST chunk
        (tools/evidence_grad_bench.py)."""
        def outputs(d, chunk):
            values = torch.empty(chunk, dtype=torch.float64, device=self.device)
            grad = torch.empty((chunk, 3), dtype=torch.float64, device=self.device)
            d.values, d.grad = _ptr(values), _ptr(grad)

            def download(out, g0, c):
                out["lml"][g0:g0 + c] = values[:c].cpu().numpy()
                out["grad"][g0:g0 + c] = grad[:c].cpu().numpy()
            return download

        return self._evidence_run(params_list, max_bytes, events, dict(lml=(), grad=(3,)), self.evidence_grad_chunk,
                                  _lib.ItalEvidenceGradDesc, self._lib.ital_gp_evidence_grad,
                                  self._lib.ital_gp_evidence_grad_workspace, 8, outputs)

    def loo_grad_chunk(self, max_bytes=1 << 30):
        """Candidates loo_grad() sends to the device at once so that their Grams, workspace and outputs stay below `max_bytes`
        (at most 65535, the limit of one ital_gp_loo_grad call); MemoryError if one candidate alone exceeds it.  The squared
        distances are shared by the candidates of a chunk and counted once."""
        m = self.m
        one, two = (int(self._lib.ital_gp_loo_grad_workspace(m, c)) for c in (1, 2))
        per = 8 * (m * m + (two - one) + 9)
        shared = 8 * (2 * one - two)
        if shared + per > max_bytes:
            raise MemoryError("one candidate at m = %d takes %d bytes, more than max_bytes = %d" % (m, shared + per, max_bytes))
        return int(min((max_bytes - shared) // per, 65535))

    def loo_grad(self, params_list, *, max_bytes=1 << 30, events=None):
        """The closed-form leave-one-out scores of hyper-parameter candidates on the model's own labelled set (queries
        included) and their gradients in the LOGARITHMS of the parameters, without touching the model: for each dict of
        `params_list` (`length_scale`, optional `var` / `noise`; default: the model's current value) the quantities of
        include/ital_loo_grad.h.  Returns a dict of numpy arrays: `loo_logp`, `loo_mse` [G] (the bits evidence() returns),
        `grad_logp`, `grad_mse` [G, 3] (d / d log length_scale, d log var, d log noise), `ok` [G] bool (the candidate's Gram
        was positive definite; otherwise -inf, +inf and NaN rows).

        Argument handling, chunking and errors are those of evidence_grad(): chunks whose Grams and workspace stay below
        `max_bytes`, values that do not depend on the chunking; XT, XTn and y are read and only buffers of the call's own are
        written -- L, alpha, V, mu, s2, the status word and both random streams stay as they are.  Every rank computes the same
        thing locally: no collective.  RuntimeError for an unfitted model, ValueError for a non-positive length_scale / var,
        MemoryError if one candidate alone exceeds max_bytes.
        `events`: None, or nine recorded torch events that bracket the eight stages of the LAST chunk
        (tools/loo_grad_bench.py)."""
        def outputs(d, chunk):
            values = torch.empty((chunk, 2), dtype=torch.float64, device=self.device)
            grad = torch.empty((chunk, 2, 3), dtype=torch.float64, device=self.device)
            d.values, d.grad = _ptr(values), _ptr(grad)

            def download(out, g0, c):
                v, g = values[:c].cpu().numpy(), grad[:c].cpu().numpy()
                out["loo_logp"][g0:g0 + c], out["loo_mse"][g0:g0 + c] = v[:, 0], v[:, 1]
                out["grad_logp"][g0:g0 + c], out["grad_mse"][g0:g0 + c] = g[:, 0], g[:, 1]
            return download

        return self._evidence_run(params_list, max_bytes, events, dict(loo_logp=(), loo_mse=(), grad_logp=(3,), grad_mse=(3,)),
                                  self.loo_grad_chunk, _lib.ItalLooGradDesc, self._lib.ital_gp_loo_grad,
                                  self._lib.ital_gp_loo_grad_workspace, 9, outputs)

    def check_status(self, status=None):
        """Raises if a kernel flagged a numerical failure.  `status`: the word as already downloaded (e.g. the OR over all
        ranks that the selection step returns); otherwise this rank's word is read (synchronises).  Bit 1 comes from the
        replicated Cholesky append and is therefore the same on every rank."""
        s = int(self.status.item()) if status is None else int(status)
        if s & 1:
            raise np.linalg.LinAlgError("kernel matrix of the labelled samples is not positive definite "
                                        "(the reference would warn at gp.py:31)")
        if s & 2:
            raise np.linalg.LinAlgError("singular conditional covariance in the orthant integrator "
                                        "(duplicate samples in the batch?)")

    # ------------------------------------------------------------------ prediction
    def _full(self, t):
        """Local shard vector -> full-length numpy array (all ranks; a collective when the rows are sharded)."""
        return self._full_device(t).cpu().numpy()

    def _full_device(self, t, keep=None):
        """Local shard vector -> full-length device vector, replicated on every rank (one all-gather of equal-sized,
        padded shards when the rows are sharded).  `keep`: name under which the send / receive buffers are kept between
        calls (the means are replicated after every update: no allocation, and no copy at all when the shards are equal)."""
        loc = t[: self.n]
        if not self.collective:
            return loc
        pad = (self.n_total + self.world - 1) // self.world
        bufs = self._gather_bufs.get(keep) if keep else None
        if bufs is None:
            bufs = (torch.zeros(pad, dtype=loc.dtype, device=self.device),
                    torch.empty((self.world, pad), dtype=loc.dtype, device=self.device))
            if keep:
                self._gather_bufs[keep] = bufs
        send, recv = bufs
        if self.n == pad and loc.is_contiguous():
            send = loc                       # equal shards: the local vector is the send buffer, no staging copy
        else:
            send[: self.n] = loc
        sharding.gather_records(send, recv, self.group)
        if pad * self.world == self.n_total:
            return recv.view(-1)
        parts = []
        for r in range(self.world):
            a, b = sharding.row_range(self.n_total, self.world, r)
            parts.append(recv[r, : b - a])
        return torch.cat(parts)

    def _replicate_mean(self):
        """Called by every rank at the end of an update: the predictive means of ALL samples as a device vector on every
        rank (asynchronous, on the stream).  What reads them later -- `rel_mean`, top_results(), the candidate restriction
        of `top_candidates` -- is then a local operation: reading an attribute on one rank only cannot dead-lock the
        others (the reference refreshes `rel_mean` inside update() too, retrieval_base.py:58,120)."""
        self.mu_all = self._full_device(self.mu, keep="mu")
        self._mean_host = None

    def mean_host(self):
        """Predictive mean of every sample as a numpy array (downloaded on first use after an update; no collective)."""
        if self._mean_host is None:
            self._mean_host = self.mu_all.cpu().numpy()
        return self._mean_host

    def topk_mean(self, k):
        """Indices of the k samples of largest predictive mean, descending (NaN first, ties by descending index), selected
        on the device (ital_topk): nothing of size N is downloaded.  Local operation on the replicated means."""
        k = int(k)
        n = self.n_total
        if not (1 <= k <= min(_lib.ITAL_TOPK_MAX, n)):
            raise ValueError("k outside 1..min(%d, number of samples)" % _lib.ITAL_TOPK_MAX)
        if getattr(self, "_topk_work", None) is None:
            self._topk_work = torch.empty(int(self._lib.ital_topk_workspace()), dtype=torch.uint8, device=self.device)
        vals = torch.empty(k, dtype=torch.float64, device=self.device)
        idx = torch.empty(k, dtype=torch.int64, device=self.device)
        check(self._lib.ital_topk(_ptr(self.mu_all), n, 0, k, _ptr(vals), _ptr(idx), _ptr(self._topk_work), _stream()))
        return idx.cpu().numpy()

    def rank_mean(self, k=None):
        """The first k entries (None: all) of the complete ranking of the samples by predictive mean, in topk_mean's order,
        sorted on the device (ital_rank_desc; metrics.rank): only the k indices asked for are downloaded.  Local operation
        on the replicated means."""
        from . import metrics
        n = self.n_total
        if k is not None and not (0 <= int(k) <= n):
            raise ValueError("k outside 0..number of samples")
        with torch.cuda.device(self.device):
            order = metrics.rank(self.mu_all[:n])
        return (order if k is None else order[: int(k)]).cpu().numpy()

    def predict_stored(self, ind=None, cov_mode=None):
        """Predictive mean / variance / covariance of samples of the data matrix (reference gp.py:203-232)."""
        if self.m == 0:
            raise RuntimeError("the GP has not been fitted: call fit()/update() first "
                               "(the reference fails with an AttributeError at gp.py:222)")
        mean = self.mean_host()
        if ind is not None:
            ind = np.asarray(ind, dtype=np.int64)
            mean = mean[ind]
        if cov_mode is None:
            return mean
        if cov_mode == "diag":
            var = np.maximum(0, self._full(self.s2))
            return mean, (var if ind is None else var[ind])
        if cov_mode == "full":
            if ind is None:
                raise ValueError("full covariance of all samples is an N x N matrix; pass `ind`")
            return mean, self._cov_full(ind)
        raise ValueError("cov_mode must be None, 'diag' or 'full'")

    def _cov_full(self, ind):
        """K[S,S] - V[:,S]^T V[:,S] for a short index list S: feature rows and whitened columns of S are replicated (owners
        contribute), every rank then forms the |S| x |S| block itself (ital_cov_block, FP64 MFMA)."""
        ind = [int(i) for i in ind]
        ns = len(ind)
        rows = self._gather_rows(ind)
        norms = torch.empty(ns, dtype=torch.float64, device=self.device)
        check(self._lib.ital_row_norms(_ptr(rows), ns, self.ldx, _ptr(norms), _stream()))
        lds = _pad16(ns)
        Vs = torch.zeros((max(self.m, 1), lds), dtype=torch.float64, device=self.device)
        Vs[: self.m, :ns] = self.gather_columns(self.V[: max(self.m, 1)], ind)[: self.m]
        out = torch.empty((ns, lds), dtype=torch.float64, device=self.device)
        check(self._lib.ital_cov_block(_ptr(rows), _ptr(norms), ns, _ptr(rows), _ptr(norms), ns, self.ldx, _ptr(Vs), lds,
                                       _ptr(Vs), lds, self.m, float(self.var), float(self.length_scale), _ptr(out), lds,
                                       _stream()))
        return out[:, :ns].cpu().numpy()

    def updated_prediction(self, ind, y, pred_ind, cov_mode=None):
        """Prediction for `pred_ind` after a simulated update with (ind, y), without updating (reference gp.py:295-344).
        The scorers do this inside their kernels (closed form on the fed-back block); this API call, which the reference
        exposes to callers, applies the same closed form on the host to the posterior block the device computes:
        W = (Sigma_FF + noise I)^-1, mu' = mu_P + Sigma_PF W (y - mu_F), Sigma' = Sigma_PP - Sigma_PF W Sigma_FP."""
        ind = [int(i) for i in ind]
        pred = [int(i) for i in pred_ind]
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        mean, cov = self.predict_stored(pred + ind, cov_mode="full")
        n = len(pred)
        s_ff = cov[n:, n:] + self.noise * np.eye(len(ind))
        s_pf = cov[:n, n:]
        sol = np.linalg.solve(s_ff, np.column_stack((y - mean[n:], s_pf.T)))
        new_mean = mean[:n] + s_pf @ sol[:, 0]
        if cov_mode is None:
            return new_mean
        new_cov = cov[:n, :n] - s_pf @ sol[:, 1:]
        if cov_mode == "full":
            return new_mean, new_cov
        if cov_mode == "diag":
            return new_mean, np.maximum(0, np.diag(new_cov))
        raise ValueError("cov_mode must be None, 'diag' or 'full'")

    def rbf_cols(self, ind):
        """Kernel columns k(x_j, X) for a short index list (what replaces slicing K_all)."""
        rows = self._gather_rows([int(i) for i in ind])
        norms = torch.empty(len(ind), dtype=torch.float64, device=self.device)
        check(self._lib.ital_row_norms(_ptr(rows), len(ind), self.ldx, _ptr(norms), _stream()))
        out = torch.empty((len(ind), self.ldv), dtype=torch.float64, device=self.device)
        for c0 in range(0, len(ind), 16):
            c = min(16, len(ind) - c0)
            check(_lib.rows_fn("ital_rbf_cols", self.xtype)(_ptr(self.Xd), _ptr(self.xnorm), self.n, self.ldx,
                                                            _ptr(rows[c0:c0 + c]), _ptr(norms[c0:c0 + c]), c, float(self.var),
                                                            float(self.length_scale), _ptr(out[c0:c0 + c]), self.ldv, _stream()))
        return out[:, : self.n]

    def predict(self, X, cov_mode=None, on_device=False):
        """Predictive mean (and variance / full covariance) for external samples (reference gp.py:264-292).  Every rank
        computes it for all of X (the labelled-set state is replicated): no collective.  X: an array, or a torch tensor
        (f16 / bf16 / f32 / f64, host or device) that ital_ingest_rows converts on the device.  on_device (with cov_mode
        None): the means stay where they were computed and come back as a float64 device tensor."""
        if on_device and cov_mode is not None:
            raise ValueError("on_device returns the means alone: cov_mode must be None")
        if self.m == 0:
            raise RuntimeError("the GP has not been fitted")
        if cov_mode not in (None, "diag", "full"):
            raise ValueError("cov_mode must be None, 'diag' or 'full'")
        dev = self.device
        if isinstance(X, torch.Tensor):
            # f16 / bf16 / f32 / f64, host or device: converted and padded on the device (the same bits as the float64 array)
            Xt = DeviceData(X if X.ndim != 1 else X[None], device=dev)
            if Xt.d != self.d:
                raise ValueError("X must have %d columns" % self.d)
            nt, Xt = Xt.n, Xt.X
        else:
            X = np.atleast_2d(np.asarray(X, dtype=np.float64))
            nt = X.shape[0]
            Xt = torch.zeros((nt, self.ldx), dtype=torch.float64, device=dev)
            Xt[:, : self.d] = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
        ldvt = _pad16(nt)
        mean = torch.empty(nt, dtype=torch.float64, device=dev)
        pvar = torch.empty(nt, dtype=torch.float64, device=dev)
        xtn = torch.empty(nt, dtype=torch.float64, device=dev)
        Vt = torch.empty((self.m, ldvt), dtype=torch.float64, device=dev)
        check(self._lib.ital_predict(_ptr(Xt), nt, self.ldx, _ptr(self.XT), _ptr(self.XTn), self.m, _ptr(self.L), self.cap,
                                     _ptr(self.alpha), float(self.var), float(self.length_scale), _ptr(mean), _ptr(pvar),
                                     _ptr(xtn), _ptr(Vt), ldvt, 1, _stream()))
        if cov_mode == "diag":
            return mean.cpu().numpy(), pvar.cpu().numpy()
        if cov_mode == "full":
            cov = torch.empty((nt, ldvt), dtype=torch.float64, device=dev)
            check(self._lib.ital_cov_block(_ptr(Xt), _ptr(xtn), nt, _ptr(Xt), _ptr(xtn), nt, self.ldx, _ptr(Vt), ldvt,
                                           _ptr(Vt), ldvt, self.m, float(self.var), float(self.length_scale), _ptr(cov),
                                           ldvt, _stream()))
            return mean.cpu().numpy(), cov[:, :nt].cpu().numpy()
        return mean if on_device else mean.cpu().numpy()
