"""AdaptAL on MI355X: host-side mirror of reference ital/adapt_al.py `AdaptAL` (drop-in learner).

Li & Guo's adaptive active learner scores a candidate by entropy ** beta * information_density ** (1 - beta), collects the
top k for every beta and keeps the k of that short list with the smallest expected classification error (reference
adapt_al.py:79-112).  The information density is log(K_ii / sigma_i) / 2 with sigma_i = K_ii - k_i^T K_(-i)^-1 k_i over the
PRIOR Gram K of the candidates (+ noise); the reference gets sigma from one `reduced_inv` per candidate, here it is the
Schur complement identity sigma_i = 1 / (K^-1)_ii: one Cholesky, one triangular inverse.  On the device, per fetch:

    ital_gather_block     features, whitened columns, mean, variance of the candidate block       [replicated]
    ital_gram_rows        the candidates' prior Gram + noise I                  (FP64 MFMA)
    ital_chol_batched     its Cholesky factor
    ital_chol_inv_diag    (K^-1)_ii                                             (FP64 MFMA, include/ital_adapt.h)
    ital_adapt_scores     entropy, density          -> download of 2 nc doubles; the betas and argpartition on the host
    ital_cov_block        posterior covariance rows of the short list with the block
    ital_adapt_error      expected classification error of the short list -> download; argpartition on the host

numpy's own partition order decides the returned list, as in the reference.  With several ranks the candidate block is
gathered to every rank and every rank computes the whole (small) problem: all ranks return the same list.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check
from .gp import _pad16, _ptr, _stream
from .mcmi import MCMI_min
from .retrieval_base import ActiveRetrievalBase


class AdaptAL(ActiveRetrievalBase):
    """Constructor arguments as reference ital/adapt_al.py:49-76; `parallelized` is accepted and ignored."""

    #: refuse a candidate Gram whose buffers (the Gram and the triangular inverse's work space, three nc x nc matrices)
    #: exceed this many bytes (use `subsample`, as the reference's configs do: mirflickr.conf, imagenet.conf).  32 GiB: nc up
    #: to ~37 000 without subsample, a ninth of an MI355X's 288 GB next to the GP state and the gathered block (cap x nc)
    max_gram_bytes = 32 << 30

    def __init__(self, data=None, queries=[], length_scale=0.1, var=1.0, noise=1e-6, subsample=None, parallelized=True,
                 betas=[0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0], *, device=None, rank=0, world=1, group=None):
        ActiveRetrievalBase.__init__(self, data, queries, length_scale, var, noise, device=device, rank=rank,
                                     world=world, group=group)
        self.subsample = subsample
        self.parallelized = parallelized
        self.betas = betas
        self._block_bufs = None
        self._gram_bufs = None
        self._err_bufs = None
        #: what the last fetch computed (numpy): candidates, entropy, density, max_ind, error vector (None: early return)
        self.last = None

    def _start_afresh(self):
        """add_data() / set_params(): the block, Gram and error buffers start afresh."""
        ActiveRetrievalBase._start_afresh(self)
        self._block_bufs = self._gram_bufs = self._err_bufs = None
        self.last = None

    _gather_block = MCMI_min._gather_block      # the replicated candidate block, kept between fetches of one shape

    def _gram_buffers(self, nc, ldc, work_len):
        dev = self.gp.device
        if self._gram_bufs is None or self._gram_bufs[0] != nc:
            K = torch.empty((nc, ldc), dtype=torch.float64, device=dev)
            idx = torch.arange(nc, dtype=torch.int64, device=dev)
            self._gram_bufs = (nc, K, idx, torch.empty(work_len, dtype=torch.float64, device=dev),
                               torch.empty((3, nc), dtype=torch.float64, device=dev),
                               torch.tensor([idx.data_ptr()], dtype=torch.int64, device=dev),
                               torch.tensor([nc], dtype=torch.int32, device=dev),
                               torch.tensor([K.data_ptr()], dtype=torch.int64, device=dev),
                               torch.tensor([ldc], dtype=torch.int64, device=dev),
                               torch.zeros(2, dtype=torch.int32, device=dev))
        return self._gram_bufs[1:]

    def fetch_unlabelled(self, k):
        """Fetches a batch of unlabelled samples (reference ital/adapt_al.py:79-112); list of python ints."""
        gp = self.gp
        if gp.m == 0:
            raise RuntimeError("fetch_unlabelled() needs a fitted relevance model: call update() first or pass queries")
        cand = self._unseen_array()
        if self.subsample and (self.subsample < len(cand)):
            # same call on the global numpy RNG as the reference (adapt_al.py:92-93; an array draws as a list does)
            cand = np.random.choice(cand, self.subsample, replace=False)
        if len(cand) < k:
            k = len(cand)
        self._last_batch = None
        self.last = None
        if k <= 0:
            return []
        lib = _lib.lib()
        dev = gp.device
        cand = np.asarray(cand, dtype=np.int64)
        nc = len(cand)
        ldc = _pad16(nc)
        work_len = int(lib.ital_chol_inv_diag_workspace(nc))
        if 8 * (nc * ldc + work_len) > self.max_gram_bytes:
            raise MemoryError("AdaptAL: the %d x %d candidate Gram and its inverse take %d bytes, more than max_gram_bytes = "
                              "%d; pass subsample= (reference configs use 1000)"
                              % (nc, nc, 8 * (nc * ldc + work_len), self.max_gram_bytes))
        var, ls, noise = float(self.var), float(self.length_scale), float(self.noise)
        with torch.cuda.device(dev):
            st = _stream()
            Xc, Vc, ldc, xnc, muc, s2c = self._gather_block(cand)
            K, idx, work, vec, idx_p, n_p, K_p, ld_p, info = self._gram_buffers(nc, ldc, work_len)
            # the Gram over the gathered block with the identity index list: the rows may live on other ranks
            check(lib.ital_gram_rows(_ptr(Xc), _ptr(xnc), gp.ldx, _ptr(idx_p), _ptr(n_p), _ptr(K_p), _ptr(ld_p), 1, nc, var, ls,
                                     noise, st))
            info.zero_()
            check(lib.ital_chol_batched(_ptr(K_p), _ptr(n_p), _ptr(ld_p), 1, nc, _ptr(info[:1]), _ptr(info[1:]), st))
            check(lib.ital_chol_inv_diag(_ptr(K), nc, ldc, _ptr(vec[0]), _ptr(work), work_len, _ptr(info[:1]), st))
            check(lib.ital_adapt_scores(_ptr(muc), _ptr(s2c), _ptr(vec[0]), nc, var + noise, _ptr(vec[1]), _ptr(vec[2]), st))
            pivot = int(info[0].item())                  # synchronises; the vectors below are then ready
            if pivot != 0:
                raise np.linalg.LinAlgError("AdaptAL: the Gram of the candidates is not positive definite (pivot %d)" % pivot)
            host = vec[1:].cpu().numpy()
            entropy, density = host[0], host[1]
            # for every beta the k samples maximising the combination; their union (reference adapt_al.py:102-104)
            scores = np.stack([(entropy ** beta) * (density ** (1. - beta)) for beta in self.betas])
            max_ind = np.unique(np.argpartition(-scores, k - 1, axis=-1)[:, :k].ravel())
            self.last = dict(candidates=cand, entropy=entropy, density=density, max_ind=max_ind, err=None)
            if len(max_ind) <= k:
                return cand[max_ind].tolist()
            r = len(max_ind)
            sel = torch.from_numpy(max_ind.astype(np.int64)).to(dev)
            rows = sel.to(torch.int32)
            Xr, xnr = Xc.index_select(0, sel), xnc.index_select(0, sel)
            Vr = Vc.index_select(1, sel).contiguous()
            if self._err_bufs is None or self._err_bufs[0] != (r, ldc):
                self._err_bufs = ((r, ldc), torch.empty((r, ldc), dtype=torch.float64, device=dev),
                                  torch.empty(3 * r, dtype=torch.float64, device=dev))
            _, C, out = self._err_bufs
            check(lib.ital_cov_block(_ptr(Xr), _ptr(xnr), r, _ptr(Xc), _ptr(xnc), nc, gp.ldx, _ptr(Vr), r, _ptr(Vc), ldc, gp.m,
                                     var, ls, _ptr(C), ldc, st))
            check(lib.ital_adapt_error(_ptr(C), ldc, _ptr(rows), r, nc, _ptr(muc), _ptr(s2c), noise, _ptr(out[r:]), _ptr(out),
                                       st))
            err = out[:r].cpu().numpy()
        self.last["err"] = err
        # the k samples of the short list minimising the expected classification error (adapt_al.py:110-112)
        min_ind = np.argpartition(err, k - 1)[:k]
        return cand[max_ind[min_ind]].tolist()
