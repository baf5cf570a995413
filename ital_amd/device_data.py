"""Feature rows that live on the device and are shared: `DeviceData`.

Every kernel reads the data matrix as FP64 rows padded to a multiple of 16 columns, with their squared norms next to them
(`GaussianProcess.Xd`, `.xnorm`).  A learner built from a numpy array makes its own pair; a `DeviceData` is that pair as an
object of its own, so that

  - it can be built from whatever the caller has -- numpy or torch, host or device, f16 / bf16 / f32 / f64, row-strided --
    without a float64 copy on the host and without an n x d FP64 staging tensor on the device (ital_ingest_rows converts,
    pads and norms; host data travels in its own type, in pieces of at most `chunk_bytes`);
  - several learners over one database view the same rows (`GaussianProcess(data=store)` uploads nothing);
  - it grows in place (`append`), and each learner catches up when it chooses to (`sync_data`);
  - rows leave it (`remove`): the survivors are gathered into fresh tensors (ital_compact_rows), and a change log of a few
    integers per event tells each learner what happened since it last looked.

The index arithmetic of a removal -- the map old index -> new index, its composition over several events, the remapping of
id sets -- is in plain functions below, which need no device.

One host thread drives a store and its learners; everything runs on the current torch stream of the store's device.
"""
import bisect
import warnings

import numpy as np
import torch

from . import _lib
from ._lib import check


def _pad16(v):
    return (int(v) + 15) // 16 * 16


def _stream():
    return torch.cuda.current_stream().cuda_stream


#: torch dtype -> element type of ital_ingest_rows (every other real dtype goes through float64)
DTYPE_CODES = {torch.float64: _lib.INGEST_F64, torch.float32: _lib.INGEST_F32, torch.float16: _lib.INGEST_F16,
               torch.bfloat16: _lib.INGEST_BF16}
_NUMPY_CODES = {np.dtype(np.float64): _lib.INGEST_F64, np.dtype(np.float32): _lib.INGEST_F32,
                np.dtype(np.float16): _lib.INGEST_F16}


def dtype_code(dtype):
    """Element type of ital_ingest_rows for a torch or numpy dtype; None for one that has to be converted first."""
    if isinstance(dtype, torch.dtype):
        return DTYPE_CODES.get(dtype)
    try:
        return _NUMPY_CODES.get(np.dtype(dtype))
    except TypeError:
        return None


def as_rows(data):
    """`data` (numpy array, torch tensor or anything numpy converts) as a 2-D torch tensor of one of the four element types
    whose inner stride is 1 and whose row stride is at least its width -- on the side it came from, sharing its memory where
    it already has that form.  ValueError for anything but two dimensions, TypeError for a complex dtype."""
    if isinstance(data, torch.Tensor):
        t = data.detach()
        if t.is_complex():
            raise TypeError("complex feature rows")
        if t.ndim != 2:
            raise ValueError("data must be an n-by-d array")
        if t.dtype not in DTYPE_CODES:
            t = t.to(torch.float64)
    else:
        a = np.asarray(data)
        if np.iscomplexobj(a):
            raise TypeError("complex feature rows")
        if a.ndim != 2:
            raise ValueError("data must be an n-by-d array")
        if a.dtype not in _NUMPY_CODES:
            a = a.astype(np.float64)
        item = a.dtype.itemsize
        if a.shape[1] and (a.strides[1] != item or a.strides[0] % item or a.strides[0] < a.shape[1] * item):
            a = np.ascontiguousarray(a)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # a read-only array: it is only read
            t = torch.from_numpy(a)
    if t.shape[1] and (t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1])):
        t = t.contiguous()
    return t


def ingest_same(t, X, xnorm, scratch):
    """Rows of the DEVICE tensor `t` -> X[i, :] (padded rows of t's OWN element type, bits kept) and xnorm[i] (FP64, the bits
    ingest() gives), i < len(t), on the current stream (ital_ingest_rows_t).  scratch: [rows, ldx] float64 -- the FP64
    expansion exists one block of that many rows at a time, for the norms alone."""
    k, d = t.shape
    if k == 0:
        return
    ld = t.stride(0) if k > 1 else d
    check(_lib.lib().ital_ingest_rows_t(t.data_ptr(), DTYPE_CODES[t.dtype], k, d, ld, X.data_ptr(), X.shape[1], xnorm.data_ptr(),
                                        0 if scratch is None else scratch.data_ptr(), 0 if scratch is None else scratch.shape[0],
                                        _stream()))


def ingest(t, X, xnorm):
    """Rows of the DEVICE tensor `t` (as as_rows() leaves it) -> X[i, :] (padded FP64) and xnorm[i], i < len(t), on the
    current stream.  X: [>= len(t), ldx] float64, contiguous; xnorm: [>= len(t)] float64."""
    k, d = t.shape
    if k == 0:
        return
    ld = t.stride(0) if k > 1 else d
    check(_lib.lib().ital_ingest_rows(t.data_ptr(), DTYPE_CODES[t.dtype], k, d, ld, X.data_ptr(), X.shape[1], xnorm.data_ptr(),
                                      _stream()))


# ---------------------------------------------------------------------------------------------------- index arithmetic
def normalize_ids(ids, n):
    """`ids` (any iterable of ints; negative ones count from the end of the n rows) as an ascending list of distinct python
    ints in [0, n).  IndexError for an id outside the rows."""
    out = set()
    for i in ids:
        i = int(i)
        if not -n <= i < n:
            raise IndexError("row index %d outside the %d rows" % (i, n))
        out.add(i + n if i < 0 else i)
    return sorted(out)


def keep_indices(n, removed):
    """The survivors of removing the ascending, distinct ids `removed` from n rows: ascending int64 array."""
    return np.delete(np.arange(n, dtype=np.int64), np.asarray(removed, dtype=np.int64))


def removal_map(n, removed):
    """The index map of one removal: int64 array of length n with the new index of every row, -1 for a removed one."""
    out = np.full(n, -1, dtype=np.int64)
    keep = keep_indices(n, removed)
    out[keep] = np.arange(len(keep), dtype=np.int64)
    return out


def compose_maps(first, second):
    """The map of `first` followed by `second` (`second` may be longer than first's survivors: rows appended in between are
    not in the domain of the result)."""
    first, second = np.asarray(first, dtype=np.int64), np.asarray(second, dtype=np.int64)
    out = np.full(len(first), -1, dtype=np.int64)
    alive = first >= 0
    out[alive] = second[first[alive]]
    return out


def log_index_map(events, n):
    """The composed index map of the rows 0 .. n - 1 over `events` (the entries of DeviceData.log) and the row count after
    them: (int64 array of length n, n_after).  ValueError for a log that does not start at n rows."""
    out = np.arange(n, dtype=np.int64)
    for ev in events:
        if ev[0] == "append":
            n += int(ev[1])
        elif ev[0] == "remove":
            if ev[2] != n:
                raise ValueError("the log removes from %d rows where there are %d" % (ev[2], n))
            out = compose_maps(out, removal_map(n, ev[1]))
            n -= len(ev[1])
        else:
            raise ValueError("unknown event %r" % (ev[0],))
    return out, n


def remap_ids(ids, removed):
    """The ids of `ids` that survive the removal of the ascending list `removed`, under their new numbers, as a set: an id
    moves down by the number of removed ids below it (bisection: O(|ids| log |removed|), nothing N-sized)."""
    out = set()
    for i in ids:
        i = int(i)
        at = bisect.bisect_left(removed, i)
        if at < len(removed) and removed[at] == i:
            continue
        out.add(i - at)
    return out


def compact_rows(X, xnorm, n, keep, X_dst, xnorm_dst, status=None):
    """X_dst[j] <- X[keep[j]], xnorm_dst[j] <- xnorm[keep[j]] (bits kept) for the device index array `keep`, on the current
    stream (ital_compact_rows).  X, X_dst: padded rows of one of the four element types."""
    check(_lib.lib().ital_compact_rows(X.data_ptr(), xnorm.data_ptr(), n, X.shape[1], DTYPE_CODES[X.dtype], keep.data_ptr(),
                                       keep.shape[0], X_dst.data_ptr(), xnorm_dst.data_ptr(),
                                       0 if status is None else status.data_ptr(), _stream()))


# ---------------------------------------------------------------------------------------------------- neighbour lists
def _knn_args(k, metric):
    if metric not in _lib.KNN_METRICS:
        raise ValueError("metric must be one of %s, not %r" % (sorted(_lib.KNN_METRICS), metric))
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= _lib.KNN_MAX_K:
        raise ValueError("k must be an integer in 1..%d, not %r" % (_lib.KNN_MAX_K, k))
    return int(k), _lib.KNN_METRICS[metric]


def knn_rows(X, xnorm, n, q, c, metric, k, skip_self, idx, dist, rowsum=None, accumulate=False, splits=0):
    """The rows q = (q0, q1) of idx / dist (and rowsum) <- the k nearest of the query rows [q0, q1) among the rows
    c = (c0, c1) of the n padded device rows X with squared norms xnorm, on the current stream (ital_knn_rows).  idx: [n, k]
    int64, dist: [n, k] float64, rowsum: [n] float64 or None, all contiguous.  The workspace lives until the call returns; the
    caching allocator keeps it for the stream's work."""
    q0, q1 = q
    nq = q1 - q0
    if nq <= 0:
        return
    lib = _lib.lib()
    bytes_ = lib.ital_knn_workspace(nq, k, splits)
    work = torch.empty(max(bytes_, 8), dtype=torch.uint8, device=X.device)
    check(lib.ital_knn_rows(X.data_ptr(), DTYPE_CODES[X.dtype], xnorm.data_ptr(), n, X.shape[1], q0, q1, c[0], c[1],
                            _lib.KNN_METRICS[metric] if isinstance(metric, str) else metric, k, int(bool(skip_self)),
                            int(bool(accumulate)), splits, dist[q0:].data_ptr(), idx[q0:].data_ptr(),
                            0 if rowsum is None else rowsum[q0:].data_ptr(), work.data_ptr(), bytes_, _stream()))


class NeighbourLists(object):
    """The k nearest neighbours of the first n rows of one storage tensor, with the sums of their distances: what a store (or
    a learner on plain numpy data) keeps per (metric, k, skip_self).  `grow` takes in rows appended to the same storage by two
    accumulating calls -- old rows against the new data range, new rows against everything -- which by the definition of
    ital_knn_rows give the bits of a fresh computation."""

    def __init__(self, X, xnorm, n, metric, k, skip_self):
        self.metric, self.k, self.skip_self = metric, k, bool(skip_self)
        self.X, self.n = X, 0          # the storage is held: its address cannot come back under other rows
        self.idx = self.dist = self.rowsum = None
        self.density = None           # (sum - 1) / (k - 1): made on demand by neighbour_density
        self.grow(X, xnorm, n)

    def serves(self, X, n):
        return X.data_ptr() == self.X.data_ptr() and n == self.n

    def extends(self, X, n):
        return X.data_ptr() == self.X.data_ptr() and n > self.n

    def grow(self, X, xnorm, n):
        old = self.n
        with torch.cuda.device(X.device):
            idx = torch.empty((max(n, 1), self.k), dtype=torch.int64, device=X.device)
            dist = torch.empty((max(n, 1), self.k), dtype=torch.float64, device=X.device)
            rowsum = torch.empty(max(n, 1), dtype=torch.float64, device=X.device)
            if old:
                idx[:old], dist[:old] = self.idx[:old], self.dist[:old]
                knn_rows(X, xnorm, n, (0, old), (old, n), self.metric, self.k, self.skip_self, idx, dist, rowsum, accumulate=True)
            knn_rows(X, xnorm, n, (old, n), (0, n), self.metric, self.k, self.skip_self, idx, dist, rowsum)
        self.idx, self.dist, self.rowsum, self.n, self.density = idx, dist, rowsum, n, None

    def densities(self):
        """(rowsum - 1.0) / (k - 1) per row, the reference's expression (baseline_methods.py:469) with K = k - 1: one FP64
        subtraction and one FP64 division."""
        if self.density is None:
            self.density = (self.rowsum[: self.n] - 1.0) / float(self.k - 1)
        return self.density


def neighbour_lists(cache, X, xnorm, n, metric, k, skip_self):
    """The NeighbourLists of the first n rows of X from the dict `cache`: served when they were built for this storage and
    row count, grown when the same storage holds more rows now, built afresh otherwise (never a list that looks past n)."""
    key = (metric, k, bool(skip_self))
    kept = cache.get(key)
    if kept is not None and kept.serves(X, n):
        return kept
    if kept is not None and kept.extends(X, n):
        kept.grow(X, xnorm, n)
        return kept
    cache[key] = NeighbourLists(X, xnorm, n, metric, k, skip_self)
    return cache[key]


def check_density_k(K, n):
    if isinstance(K, bool) or int(K) != K or int(K) < 1:
        raise ValueError("K must be a positive integer, not %r" % (K,))
    if K + 1 > n:
        raise ValueError("K + 1 = %d neighbours (self included) of %d rows" % (K + 1, n))
    if K + 1 > _lib.KNN_MAX_K:
        raise ValueError("K + 1 = %d is above the %d neighbours ital_knn_rows keeps" % (K + 1, _lib.KNN_MAX_K))
    return int(K)


class DeviceData(object):
    """n x d feature rows on `device` as padded rows `X` [n, ldx] -- FP64, or the source's own element type -- and FP64
    squared norms `xnorm` [n].

    - data: 2-D numpy array or torch tensor, on the host or on a device; f16 / f32 / f64 (bf16 for tensors) travel and are
      converted in their own type, any other real dtype goes through float64.  A row-strided view (`T[:, 3:131]`) is read as
      it is.  The source is never aliased: afterwards the caller may free or overwrite it.
    - capacity: rows to make room for (at least n); `append` within it writes in place.
    - chunk_bytes: host data is uploaded in pieces of at most this size, each converted behind its upload.
    - storage: "f64" (the default): padded FP64 rows.  "source": the rows stay in the element type as_rows() leaves them in
      (f16, bf16, f32 or f64; nothing is ever narrowed) -- 2 or 4 bytes per feature instead of 8.  Every kernel that reads
      whole rows widens the elements in registers (include/ital_rows.h), so a learner on a compact store computes, bit for
      bit, what one on the FP64 store of the same values computes; `xnorm` holds the bits the FP64 store's has.  The FP64
      expansion exists only as a scratch block of at most chunk_bytes while rows are written (for the norms).  `append`
      takes rows of the store's element type.
    """

    def __init__(self, data, *, storage="f64", device=None, capacity=None, chunk_bytes=256 << 20):
        if storage not in ("f64", "source"):
            raise ValueError("storage must be 'f64' or 'source', not %r" % (storage,))
        if not torch.cuda.is_available():
            raise RuntimeError("ital_amd.DeviceData needs a HIP device (no CPU fallback)")
        t = as_rows(data)
        #: torch dtype of the stored rows
        self.storage = t.dtype if storage == "source" else torch.float64
        self.device = torch.device(device if device is not None else "cuda:0")
        self.chunk_bytes = int(chunk_bytes)
        self.n = 0
        self.d = int(t.shape[1])
        if self.d < 1:
            raise ValueError("data must have at least one column")
        self.ldx = _pad16(self.d)
        #: the change log: ("append", k) and ("remove", ascending removed ids, n before) in order; `epoch` == len(log).  A
        #: learner remembers the epoch it has seen and walks the log from there (GaussianProcess.sync_data).
        self.log, self.epoch = [], 0
        #: neighbour lists per (metric, k, skip_self) (NeighbourLists): shared by every learner on this store
        self._knn = {}
        self._alloc(max(int(t.shape[0]), int(capacity or 0), 1))
        self._write(t)

    # ------------------------------------------------------------------ storage
    def _alloc(self, capacity):
        with torch.cuda.device(self.device):
            X = torch.empty((capacity, self.ldx), dtype=self.storage, device=self.device)
            xnorm = torch.empty(capacity, dtype=torch.float64, device=self.device)
            if self.n:
                # the tensors left behind are not freed here: a learner that still views them keeps them, and its prefix
                X[: self.n] = self._X[: self.n]
                xnorm[: self.n] = self._xnorm[: self.n]
                for kept in self._knn.values():        # the same rows at a new address: the lists stay and can still grow
                    if kept.X.data_ptr() == self._X.data_ptr():
                        kept.X = X
        self._X, self._xnorm, self.capacity = X, xnorm, int(capacity)

    def _write(self, t):
        """Rows n .. n + len(t) - 1 <- t (there is room), then n grows."""
        k = int(t.shape[0])
        if k == 0:
            return
        with torch.cuda.device(self.device):
            X, xnorm = self._X[self.n:], self._xnorm[self.n:]
            write, scratch = ingest, None
            if self.storage != torch.float64:
                # the norms come from ital_ingest_rows on a bounded FP64 block (freed when this call returns)
                scratch = torch.empty((max(1, min(k, self.chunk_bytes // (8 * self.ldx))), self.ldx), dtype=torch.float64,
                                      device=self.device)

                def write(piece, X, xnorm):
                    ingest_same(piece, X, xnorm, scratch)
            if t.is_cuda:
                if t.device != self.device:
                    t = t.to(self.device)
                write(t, X, xnorm)
            else:
                step = max(1, self.chunk_bytes // (self.d * t.element_size()))
                for r0 in range(0, k, step):
                    piece = t[r0:r0 + step].contiguous().to(self.device)
                    write(piece, X[r0:], xnorm[r0:])
        self.n += k

    # ------------------------------------------------------------------ what a learner and its caller read
    @property
    def X(self):
        """[n, ldx] view of the rows in use."""
        return self._X[: self.n]

    @property
    def xnorm(self):
        """[n] view of their squared norms."""
        return self._xnorm[: self.n]

    @property
    def shape(self):
        return (self.n, self.d)

    ndim = 2

    def __len__(self):
        return self.n

    def rows(self, idx=None):
        """The rows (all, or those of the index list `idx`) as a float64 numpy array: downloaded on demand, not kept."""
        if idx is None:
            return self._X[: self.n, : self.d].cpu().to(torch.float64).numpy()
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        if len(idx) and (idx.min() < -self.n or idx.max() >= self.n):
            raise IndexError("row index outside the %d rows" % self.n)
        sel = torch.from_numpy(idx % max(self.n, 1)).to(self.device)
        return self._X[: self.n].index_select(0, sel)[:, : self.d].to(torch.float64).cpu().numpy()

    # ------------------------------------------------------------------ neighbour lists
    def _view(self, view):
        """(X, xnorm, n) of the store, or of a learner's own prefix `view` = (X, xnorm, n) of it."""
        return (self._X, self._xnorm, self.n) if view is None else view

    def knn(self, k, metric="cosine", skip_self=True, rows=None):
        """The k nearest rows of every row -- or of the rows `rows`, a range or a list of indices -- as device tensors
        (idx int64 [q, k], dist float64 [q, k]): ital_knn_rows (include/ital_knn.h, where distance and order are defined; slots
        beyond the available rows hold -1 / +inf).  metric: "cosine" or "sqeuclidean".  The lists of all rows are computed once
        per (metric, k, skip_self) and kept on the store; after append() the next request extends them, remove() drops them.
        The tensors returned without `rows` are the kept ones: do not write to them.  ValueError for k outside 1..32 or an
        unknown metric."""
        k, _ = _knn_args(k, metric)
        kept = neighbour_lists(self._knn, self._X, self._xnorm, self.n, metric, k, skip_self)
        if rows is None:
            return kept.idx[: self.n], kept.dist[: self.n]
        if isinstance(rows, range) and rows.step == 1 and 0 <= rows.start <= rows.stop <= self.n:
            return kept.idx[rows.start:rows.stop], kept.dist[rows.start:rows.stop]
        sel = np.asarray(list(rows), dtype=np.int64).reshape(-1)
        if len(sel) and (sel.min() < -self.n or sel.max() >= self.n):
            raise IndexError("row index outside the %d rows" % self.n)
        sel = torch.from_numpy(sel % max(self.n, 1)).to(self.device)
        return kept.idx.index_select(0, sel), kept.dist.index_select(0, sel)

    def neighbour_density(self, K, view=None):
        """The device vector (sum of the cosine distances to the K + 1 nearest rows, the row itself included, - 1.0) / K: the
        density of the reference's SUD (baseline_methods.py:469) with its `- 1.0`, which makes the density of a tight
        neighbourhood negative.  Kept on the store and shared by every learner on it; `view`: a learner's own (X, xnorm, n),
        for one that has not caught up with the store.  ValueError if K + 1 > n or K + 1 > 32."""
        X, xnorm, n = self._view(view)
        K = check_density_k(K, n)
        return neighbour_lists(self._knn, X, xnorm, n, "cosine", K + 1, False).densities()

    def append(self, rows):
        """Adds rows (the input kinds of the constructor) as rows n .. n + k - 1 and returns k.  ValueError, with nothing
        changed, for another number of columns.  Within the capacity the rows are written in place -- rows >= n are read by
        nobody: every learner reads up to its own row count; beyond it the store moves to max(2 * capacity, n + k) rows by a
        device-to-device copy, and learners that still view the old tensors go on with those."""
        t = as_rows(rows) if not (isinstance(rows, (list, tuple)) and len(rows) == 0) else None
        if t is None or t.shape[0] == 0:
            return 0
        if t.shape[1] != self.d:
            raise ValueError("rows must be a k-by-%d array" % self.d)
        if self.storage != torch.float64 and t.dtype != self.storage:
            raise TypeError("this store keeps %s rows: append rows of that type (nothing is narrowed), not %s"
                            % (self.storage, t.dtype))
        k = int(t.shape[0])
        if self.n + k > self.capacity:
            self._alloc(max(2 * self.capacity, self.n + k))
        self._write(t)
        self._record(("append", k))
        return k

    def _record(self, event):
        self.log.append(event)
        self.epoch += 1

    def _compact(self, keep):
        """The rows `keep` (ascending int64 numpy array) gathered into fresh tensors of the same capacity, which become the
        store's; the old ones are not freed here -- a learner that still views them keeps them, and its rows."""
        with torch.cuda.device(self.device):
            keep_d = torch.from_numpy(keep).to(self.device)
            X = torch.empty((self.capacity, self.ldx), dtype=self.storage, device=self.device)
            xnorm = torch.empty(self.capacity, dtype=torch.float64, device=self.device)
            compact_rows(self._X, self._xnorm, self.n, keep_d, X, xnorm)       # the ids were checked on the host
        self._X, self._xnorm, self.n = X, xnorm, len(keep)
        self._knn = {}                                  # the lists may name removed rows

    def remove(self, ids):
        """Deletes rows like np.delete(X, ids, axis=0): the survivors keep their order and get the indices 0 .. n - r - 1.
        Returns the index map: an int64 array of the old length with the new index of every row, -1 for a removed one.  `ids`:
        any iterable of ints; duplicates are collapsed, negative indices count from the end as in rows().  An empty list is a
        no-op that returns the identity.  IndexError for an id outside the rows, ValueError for removing every row; nothing is
        changed then.

        Never writes to tensors a learner may view: the survivors are gathered (ital_compact_rows, bits kept) into a fresh
        allocation of the same capacity that is swapped in, as when append() outgrows the capacity.  A learner that has not
        called sync_data() since goes on, consistently, on the rows it knows."""
        n = self.n
        removed = normalize_ids(ids, n)
        if not removed:
            return np.arange(n, dtype=np.int64)
        if len(removed) == n:
            raise ValueError("remove() would leave no row")
        self._compact(keep_indices(n, removed))
        self._record(("remove", removed, n))
        return removal_map(n, removed)
