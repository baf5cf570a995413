"""Preparing feature rows on the device: column statistics, min-max scaling and PCA of a `DeviceData` store.

The reference scales its rows to [0, 1] by the global minimum and maximum of the training set (datasets.py:107-112) and one
of its data sets is a PCA reduction; both happen on the host there.  Here a store that is already on the device -- f16 /
bf16 / f32 / f64, possibly far larger than an FP64 copy of it would fit -- is read in its own element type by the kernels
of include/ital_prepare.h:

    stats = column_stats(store)                       # min, max, sum, mean per column
    T = MinMax.fit(store)                             # the reference's rule; per_column=True for a span per column
    P = PCA.fit(store, 50)                            # scatter matrix on the FP64 MFMA, numpy.linalg.eigh of the d x d result
    small = T.then(P).apply(store, storage="f16")     # a NEW store; the source and the sessions on it are not touched
    rows = P.apply(tensor_of_test_rows)               # a device tensor for gp.predict / evaluate(X=...) / store.append

Public: column_stats, scatter_matrix (the d x d result of ital_col_cov as numpy), principal_axes, MinMax, PCA, Transform
(with Transform.reference, the same chain in numpy float64 on the host, for small checks), ColumnStats.

`apply` works in pieces of at most `chunk_bytes`, so no FP64 copy of a whole input ever exists.  A new store's `xnorm` is
filled by the store's own route (DeviceData._write): the bits ital_row_norms gives on the FP64 expansion of the stored values.
One host thread drives a store; everything runs on the current torch stream of the data's device.
"""
import collections

import numpy as np

from . import _lib

__all__ = ["ColumnStats", "column_stats", "scatter_matrix", "principal_axes", "Transform", "MinMax", "PCA"]

ColumnStats = collections.namedtuple("ColumnStats", "min max sum mean")

STORAGE = ("f64", "f32", "f16", "bf16")
_SCALE, _PROJECT = 0, 1


def principal_axes(C, k):
    """The k leading eigenpairs of the symmetric matrix C as (eigenvalues [k] descending, axes [d, k]) from
    numpy.linalg.eigh: every axis has its entry of largest magnitude positive, the first such entry deciding on ties.
    ValueError for a C that is not square or k outside 1..d."""
    C = np.asarray(C, dtype=np.float64)
    if C.ndim != 2 or C.shape[0] != C.shape[1]:
        raise ValueError("C must be a square matrix")
    d = C.shape[0]
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= d:
        raise ValueError("k must be an integer in 1..%d, not %r" % (d, k))
    lam, V = np.linalg.eigh(C)                        # ascending
    order = np.arange(d)[::-1][: int(k)]
    lam, W = lam[order], V[:, order].copy()
    lead = np.argmax(np.abs(W), axis=0)               # the first entry of largest magnitude
    W[:, W[lead, np.arange(W.shape[1])] < 0] *= -1.0
    return lam, np.ascontiguousarray(W)


def _torch():
    import torch
    return torch


def _storage_dtype(storage):
    torch = _torch()
    if storage not in STORAGE:
        raise ValueError("storage must be one of %s, not %r" % (", ".join(STORAGE), storage))
    return {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[storage]


def _is_store(data):
    from .device_data import DeviceData
    return isinstance(data, DeviceData)


def _need_store(store):
    if not _is_store(store):
        raise TypeError("a DeviceData store is needed, not %s" % type(store).__name__)
    return store._X[: store.n]


def _vector(a, device):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def column_stats(store):
    """ColumnStats(min, max, sum, mean) of the store's columns as float64 numpy arrays [d] (ital_col_stats; mean = sum / n on
    the host).  A column that holds a NaN gives NaN everywhere.  ValueError for a store without rows."""
    torch = _torch()
    from .device_data import DTYPE_CODES, _stream
    X = _need_store(store)
    n, d = store.n, store.d
    if n < 1:
        raise ValueError("column_stats of a store without rows")
    lib = _lib.lib()
    with torch.cuda.device(store.device):
        out = torch.empty((3, d), dtype=torch.float64, device=store.device)
        nbytes = lib.ital_col_stats_workspace(n, d)
        work = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=store.device)
        _lib.check(lib.ital_col_stats(X.data_ptr(), DTYPE_CODES[X.dtype], n, d, X.shape[1], out[0].data_ptr(), out[1].data_ptr(),
                                      out[2].data_ptr(), work.data_ptr(), nbytes, _stream()))
        host = out.cpu().numpy()
    return ColumnStats(host[0], host[1], host[2], host[2] / float(n))


def scatter_matrix(store, mean):
    """sum_i (x_i - mean)(x_i - mean)^T of the store's rows as a float64 numpy array [d, d] (ital_col_cov)."""
    torch = _torch()
    from .device_data import DTYPE_CODES, _stream
    X = _need_store(store)
    n, d = store.n, store.d
    mean = np.asarray(mean, dtype=np.float64).reshape(-1)
    if mean.shape[0] != d:
        raise ValueError("mean must have %d entries" % d)
    lib = _lib.lib()
    with torch.cuda.device(store.device):
        C = torch.empty((d, d), dtype=torch.float64, device=store.device)
        nbytes = lib.ital_col_cov_workspace(n, d)
        work = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=store.device)
        m = _vector(mean, store.device)
        _lib.check(lib.ital_col_cov(X.data_ptr(), DTYPE_CODES[X.dtype], n, d, X.shape[1], m.data_ptr(), C.data_ptr(), d,
                                    work.data_ptr(), nbytes, _stream()))
        return C.cpu().numpy()


class Transform(object):
    """A chain of steps over feature rows, each `(x - shift) / span` per column or `(x - shift) @ W`, with the numbers kept as
    float64 numpy arrays.  `steps`: tuples (kind, shift, span or W); `shift`, `span`, `W` name those of a single step (None
    where the step has none); d_in / d_out: columns read and written.  `eigenvalues`: float64 array [d_out] or None -- the
    eigenvalues of C / (n - 1) that belong to the axes of a transform from PCA.fit (before any whitening); kept by
    state_dict, None for every other transform, a composed one included."""

    def __init__(self, steps, eigenvalues=None):
        steps = tuple(steps)
        if not steps:
            raise ValueError("a transform needs at least one step")
        clean = []
        for kind, shift, other in steps:
            shift = np.ascontiguousarray(shift, dtype=np.float64).reshape(-1)
            other = np.ascontiguousarray(other, dtype=np.float64)
            if kind == _SCALE:
                if other.shape != shift.shape:
                    raise ValueError("shift and span must have one entry per column")
                width = len(shift)
            elif kind == _PROJECT:
                if other.ndim != 2 or other.shape[0] != len(shift) or not 1 <= other.shape[1] <= _lib.PREPARE_MAX_K:
                    raise ValueError("W must be d-by-k with k in 1..%d" % _lib.PREPARE_MAX_K)
                width = other.shape[1]
            else:
                raise ValueError("unknown step %r" % (kind,))
            if clean and len(shift) != clean[-1][3]:
                raise ValueError("a step of %d columns after one that writes %d" % (len(shift), clean[-1][3]))
            clean.append((kind, shift, other, width))
        self.steps = tuple((k, s, o) for k, s, o, _ in clean)
        self.d_in, self.d_out = len(clean[0][1]), clean[-1][3]
        if eigenvalues is not None:
            eigenvalues = np.ascontiguousarray(eigenvalues, dtype=np.float64).reshape(-1)
            if len(self.steps) != 1 or self.steps[0][0] != _PROJECT or len(eigenvalues) != self.d_out:
                raise ValueError("eigenvalues belong to a single projection, one per axis")
        self.eigenvalues = eigenvalues

    # ------------------------------------------------------------------ what a single step holds
    def _single(self):
        if len(self.steps) != 1:
            raise AttributeError("a composed transform: read its .steps")
        return self.steps[0]

    @property
    def shift(self):
        return self._single()[1]

    @property
    def span(self):
        kind, _, other = self._single()
        return other if kind == _SCALE else None

    @property
    def W(self):
        kind, _, other = self._single()
        return other if kind == _PROJECT else None

    def then(self, other):
        """This transform followed by `other`.  ValueError if other does not read d_out columns."""
        if other.d_in != self.d_out:
            raise ValueError("the second transform reads %d columns, the first writes %d" % (other.d_in, self.d_out))
        return Transform(self.steps + other.steps)

    def state_dict(self):
        out = {"kinds": np.array([k for k, _, _ in self.steps], dtype=np.int64)}
        for i, (_, shift, other) in enumerate(self.steps):
            out["shift%d" % i], out["other%d" % i] = shift.copy(), other.copy()
        if self.eigenvalues is not None:
            out["eigenvalues"] = self.eigenvalues.copy()
        return out

    @classmethod
    def from_state_dict(cls, state):
        kinds = np.asarray(state["kinds"]).reshape(-1)
        return cls([(int(k), np.asarray(state["shift%d" % i]), np.asarray(state["other%d" % i])) for i, k in enumerate(kinds)],
                   eigenvalues=state.get("eigenvalues"))

    def reference(self, rows):
        """The transform of host rows in numpy float64 (the definition, for small checks; no device)."""
        Y = np.asarray(rows, dtype=np.float64)
        for kind, shift, other in self.steps:
            Y = (Y - shift) / other if kind == _SCALE else (Y - shift) @ other
        return Y

    # ------------------------------------------------------------------ on the device
    def _run(self, X, rows, params, bufs, out, ytype):
        """The steps over the `rows` padded rows of the device tensor X; the last step writes `out` (element type code ytype),
        the steps before it the FP64 tensors `bufs`."""
        from .device_data import DTYPE_CODES, _stream
        lib = _lib.lib()
        for i, (kind, _, other) in enumerate(self.steps):
            last = i == len(self.steps) - 1
            Y, yt = (out, ytype) if last else (bufs[i], _lib.INGEST_F64)
            shift, par = params[i]
            if kind == _SCALE:
                _lib.check(lib.ital_scale_rows(X.data_ptr(), DTYPE_CODES[X.dtype], rows, len(other), X.shape[1], shift.data_ptr(),
                                               par.data_ptr(), Y.data_ptr(), yt, Y.shape[1], _stream()))
            else:
                _lib.check(lib.ital_project_rows(X.data_ptr(), DTYPE_CODES[X.dtype], rows, other.shape[0], X.shape[1],
                                                 shift.data_ptr(), par.data_ptr(), other.shape[1], other.shape[1], Y.data_ptr(),
                                                 yt, Y.shape[1], _stream()))
            X = Y

    def apply(self, data, storage="f64", chunk_bytes=256 << 20, device=None):
        """The transformed rows in the element type `storage` ("f64", "f32", "f16", "bf16": rounded once, to nearest even).

        - data a DeviceData: a NEW DeviceData of d_out columns on the same device; the source is only read.
        - data a tensor or an array of rows (the input kinds of DeviceData): a device tensor [n, d_out] (a view of padded rows)
          on `device` (a device tensor's own, else "cuda:0").

        Rows are taken in pieces whose FP64 intermediates stay below `chunk_bytes` in all."""
        torch = _torch()
        from . import device_data as dd
        dtype = _storage_dtype(storage)
        ytype = dd.DTYPE_CODES[dtype]
        store = data if _is_store(data) else None
        if store is not None:
            n, d, dev = store.n, store.d, store.device
        else:
            if not torch.cuda.is_available():
                raise RuntimeError("ital_amd.prepare needs a HIP device (no CPU fallback)")
            t = dd.as_rows(data)
            n, d = int(t.shape[0]), int(t.shape[1])
            dev = torch.device(device) if device is not None else (t.device if t.is_cuda else torch.device("cuda:0"))
        if d != self.d_in:
            raise ValueError("the transform reads %d columns, the data has %d" % (self.d_in, d))
        widths = [dd._pad16(len(s)) for _, s, _ in self.steps] + [dd._pad16(self.d_out)]    # input, intermediates, output
        per_row = 8 * sum(widths[1:]) + (8 * widths[0] if store is None else 0)
        step = max(1, min(max(n, 1), int(chunk_bytes) // per_row))
        with torch.cuda.device(dev):
            params = [(_vector(s, dev), _vector(o, dev)) for _, s, o in self.steps]
            bufs = [torch.empty((step, w), dtype=torch.float64, device=dev) for w in widths[1:-1]]
            if store is not None:
                new = dd.DeviceData(torch.empty((0, self.d_out), dtype=dtype), storage="source", device=dev, capacity=max(n, 1),
                                    chunk_bytes=store.chunk_bytes)
                piece = torch.empty((step, widths[-1]), dtype=dtype, device=dev)
                X = store._X
                for r0 in range(0, n, step):
                    rows = min(step, n - r0)
                    self._run(X[r0:r0 + rows], rows, params, bufs, piece, ytype)
                    new._write(piece[:rows, : self.d_out])
                return new
            out = torch.empty((max(n, 1), widths[-1]), dtype=dtype, device=dev)
            wide = torch.empty((step, widths[0]), dtype=torch.float64, device=dev)
            norms = torch.empty(step, dtype=torch.float64, device=dev)
            for r0 in range(0, n, step):
                rows = min(step, n - r0)
                part = t[r0:r0 + rows]
                if not part.is_cuda:
                    part = part.contiguous()
                part = part.to(dev)
                dd.ingest(part, wide, norms)
                self._run(wide, rows, params, bufs, out[r0:], ytype)
            return out[:n, : self.d_out]


class MinMax(object):
    """Min-max scaling, fitted on a store."""

    @staticmethod
    def fit(store, per_column=False):
        """per_column False (the reference's rule, datasets.py:110-112): every column is shifted by the global minimum and
        divided by (global maximum - global minimum); ValueError when the two are equal.  True: a column's own minimum and span,
        a constant column gets the span 1 and becomes 0."""
        st = column_stats(store)
        d = store.d
        if per_column:
            span = st.max - st.min
            span[span == 0] = 1.0
            return Transform([(_SCALE, st.min, span)])
        lo, hi = np.min(st.min), np.max(st.max)
        if hi == lo:
            raise ValueError("the rows hold one value only: nothing to scale by")
        return Transform([(_SCALE, np.full(d, lo), np.full(d, hi - lo))])


class PCA(object):
    """Principal component analysis, fitted on a store."""

    @staticmethod
    def fit(store, k, whiten=False):
        """The projection onto the k leading principal axes of the store's rows: centred by the column means of column_stats,
        axes from principal_axes(C / (n - 1), k) with C the scatter matrix of ital_col_cov; `whiten` divides an axis by the
        root of its eigenvalue.  The transform carries `eigenvalues` [k].  ValueError for n < 2, k outside 1..min(d, 512), or
        `whiten` with an eigenvalue among the k that is not positive (rank-deficient rows: ask for fewer axes)."""
        _need_store(store)
        n, d = store.n, store.d
        if n < 2:
            raise ValueError("PCA needs at least two rows")
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= min(d, _lib.PREPARE_MAX_K):
            raise ValueError("k must be an integer in 1..%d, not %r" % (min(d, _lib.PREPARE_MAX_K), k))
        mean = column_stats(store).mean
        lam, W = principal_axes(scatter_matrix(store, mean) / float(n - 1), int(k))
        if whiten:
            if not (lam > 0).all():
                raise ValueError("whiten: %d of the %d leading eigenvalues are not positive (smallest %g)"
                                 % (int((~(lam > 0)).sum()), int(k), float(np.min(lam))))
            W = W / np.sqrt(lam)
        return Transform([(_PROJECT, mean, W)], eigenvalues=lam)
