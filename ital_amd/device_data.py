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
