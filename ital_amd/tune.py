"""Cross-validated GP hyper-parameter search on the device: counterpart of the reference's `optimize_parameters.py`.

    from ital_amd import tune
    best, ap = tune.optimize_gp_params(dataset, relevance, tune.default_grids['ls_only'])
    python -m ital_amd.tune configs/iris.conf [--grid=ls_only --n_folds=10 ...]

Same names, signatures, defaults and return values as the reference (`optimize_parameters.py:16-170`), plus the keyword-only
`device=` and `max_bytes=`.  Folds, average precision and the alternating control flow run on the host exactly as there;
each fold's GP runs on the device (include/ital_dense.h): the fold's Gram from the feature rows
(ital_gram_rows), a batched Cholesky of all fold Grams that fit into `max_bytes` (ital_chol_batched), alpha = K^-1 y
(ital_chol_solve_batched), and every fold's held-out predictions in one kernel-times-matrix pass (ital_kernel_matvec).
Nothing of size N^2 is formed on the host or sent to the device.

Parity limit: the reference inverts each fold's Gram explicitly (dpotrf + dpotri), the device solves
with the Cholesky factor, so held-out scores agree to the conditioning of the fold's Gram.  A fold Gram that is not
positive definite in floating point makes the reference warn and go on with a meaningless inverse; here the warning is the
same and that grid value scores -inf, so it is never selected.
"""
import math
import sys
import warnings
from collections import OrderedDict

import numpy as np

default_grids = {'full': OrderedDict((
    ('length_scale', [0.001, 0.005, 0.01, 0.05, 0.1, 0.5, 1.0, 1.5, 2.0, 2.5, 3., 4., 5., 6., 7., 8., 9., 10., 15., 20., 25.]),
    ('var', [0.1, 0.5, 1.0, 1.5, 2.0, 2.5, 5.0, 10.0]),
    ('noise', [1e-8, 1e-6, 1e-4, 1e-3, 1e-2, 0.05, 0.1])
)), 'ls_only': OrderedDict((
    ('length_scale', [0.001, 0.005, 0.01, 0.05, 0.1, 0.5, 1.0, 1.5, 2.0, 2.5, 3., 4., 5., 6., 7., 8., 9., 10., 15., 20., 25.]),
))}

default_init = {'length_scale': 0.1, 'var': 1.0, 'noise': 1e-6}

#: device memory the fold Grams of one batch may take (bytes); a single fold above it raises MemoryError
DEFAULT_MAX_BYTES = 32 << 30
#: right-hand sides per ital_kernel_matvec call
_MAX_F = 16


# ----------------------------------------------------------------------------------------------------------- host side
def _features(dataset):
    X = getattr(dataset, 'X_train_norm', None)
    if X is None:
        X = dataset
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError('dataset must have X_train_norm or be an n-by-d array')
    return X


def _check_params(gp_params):
    if gp_params.get('pdist') is not None or 'pdist' in gp_params:
        raise NotImplementedError('pre-computed distances are a dense-kernel feature of the reference (gp.py:116-128); '
                                  'the device computes distances from the feature rows')
    unknown = set(gp_params) - {'length_scale', 'var', 'noise'}
    if unknown:
        raise TypeError('unexpected GP parameters: %s' % ', '.join(sorted(unknown)))
    if 'length_scale' not in gp_params:
        raise TypeError("missing GP parameter 'length_scale'")


def fold_split(X, relevance, n_folds=10):
    """(rows, targets, folds) as the reference builds them (optimize_parameters.py:48-57): `rows` are the samples whose
    relevance is not 0, `folds` the (train, test) position arrays into `rows` of StratifiedKFold(n_folds, shuffle=True,
    random_state=0) -- KFold for regression (relevance None)."""
    from sklearn.model_selection import KFold, StratifiedKFold
    rows = np.arange(len(X))
    if relevance is not None:
        relevance = np.asarray(relevance)
        rows = rows[relevance != 0]
        kfold = StratifiedKFold(n_folds, shuffle=True, random_state=0)
        folds = list(kfold.split(X[rows], relevance[rows]))
    else:
        kfold = KFold(n_folds, shuffle=True, random_state=0)
        folds = list(kfold.split(X[rows], None))
    return rows, folds


# --------------------------------------------------------------------------------------------------------- device side
class _DeviceRows(object):
    """The feature rows of a dataset on the device (zero padded to a multiple of 16 columns) and their squared norms."""

    def __init__(self, X, device):
        import torch
        from . import _lib
        if not torch.cuda.is_available():
            raise RuntimeError('ital_amd.tune needs a HIP device (no CPU fallback)')
        self.torch = torch
        self.lib = _lib.lib()
        self.check = _lib.check
        self.device = torch.device(device if device is not None else 'cuda:0')
        self.n, self.d = X.shape
        self.ldx = max(16, (self.d + 15) // 16 * 16)
        with torch.cuda.device(self.device):
            self.Xd = torch.zeros((max(self.n, 1), self.ldx), dtype=torch.float64, device=self.device)
            self.Xd[:self.n, :self.d] = torch.from_numpy(np.ascontiguousarray(X)).to(self.device)
            self.xnorm = torch.empty(max(self.n, 1), dtype=torch.float64, device=self.device)
            self.check(self.lib.ital_row_norms(self.Xd.data_ptr(), self.n, self.ldx, self.xnorm.data_ptr(), self.stream()))

    def stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def ptrs(self, values, dtype):
        return self.torch.tensor(values, dtype=dtype, device=self.device)


def _fold_predictions(dev, params_list, fits, max_bytes):
    """For every params p and fold f with fit rows fits[f] = (global row indices, targets): the fold GP's predictive mean
    at every row, out[p] = [n, n_folds] (numpy), and ok[p] = whether every fold Gram was positive definite."""
    torch = dev.torch
    n_folds = len(fits)
    jobs = [(p, f) for p in range(len(params_list)) for f in range(n_folds)]
    size = [len(fits[f][0]) for f in range(n_folds)]
    for f in range(n_folds):
        if 8 * size[f] * size[f] > max_bytes:
            raise MemoryError('a fold Gram of n_train = %d takes %d bytes, more than max_bytes = %d'
                              % (size[f], 8 * size[f] * size[f], max_bytes))
    alpha = [[None] * n_folds for _ in params_list]
    ok = [True] * len(params_list)
    idx_dev = [torch.from_numpy(np.ascontiguousarray(fits[f][0], dtype=np.int64)).to(dev.device) for f in range(n_folds)]
    y_dev = [torch.from_numpy(np.ascontiguousarray(fits[f][1], dtype=np.float64)).to(dev.device) for f in range(n_folds)]
    status = torch.zeros(1, dtype=torch.int32, device=dev.device)
    out = {}
    done = [0] * len(params_list)
    start = 0
    while start < len(jobs):
        stop, used = start, 0
        while stop < len(jobs) and used + 8 * size[jobs[stop][1]] ** 2 <= max_bytes:
            used += 8 * size[jobs[stop][1]] ** 2
            stop += 1
        batch = jobs[start:stop]
        offs = np.cumsum([0] + [size[f] ** 2 for _, f in batch])
        buf = torch.empty(int(offs[-1]), dtype=torch.float64, device=dev.device)
        ys = [y_dev[f].clone() for _, f in batch]
        st = dev.stream()
        mats = [buf.data_ptr() + 8 * int(offs[b]) for b in range(len(batch))]
        keep = []                       # pointer arrays stay referenced until the batch has synchronised (info.cpu())
        # the Gram: one call per grid value of the batch (var / length scale / noise are per call)
        for p in sorted(set(p for p, _ in batch)):
            sel = [b for b in range(len(batch)) if batch[b][0] == p]
            prm = params_list[p]
            fs = [batch[b][1] for b in sel]
            arrs = (dev.ptrs([idx_dev[f].data_ptr() for f in fs], torch.int64), dev.ptrs([size[f] for f in fs], torch.int32),
                    dev.ptrs([mats[b] for b in sel], torch.int64), dev.ptrs([size[f] for f in fs], torch.int64))
            keep.append(arrs)
            dev.check(dev.lib.ital_gram_rows(dev.Xd.data_ptr(), dev.xnorm.data_ptr(), dev.ldx, arrs[0].data_ptr(),
                                             arrs[1].data_ptr(), arrs[2].data_ptr(), arrs[3].data_ptr(), len(sel),
                                             max(size[f] for f in fs), float(prm.get('var', 1.0)),
                                             float(prm['length_scale']), float(prm.get('noise', 1e-6)), st))
        n_b = dev.ptrs([size[f] for _, f in batch], torch.int32)
        ld_b = dev.ptrs([size[f] for _, f in batch], torch.int64)
        a_b = dev.ptrs(mats, torch.int64)
        y_b = dev.ptrs([y.data_ptr() for y in ys], torch.int64)
        info = torch.zeros(len(batch), dtype=torch.int32, device=dev.device)
        dev.check(dev.lib.ital_chol_batched(a_b.data_ptr(), n_b.data_ptr(), ld_b.data_ptr(), len(batch),
                                            max(size[f] for _, f in batch), info.data_ptr(), status.data_ptr(), st))
        dev.check(dev.lib.ital_chol_solve_batched(a_b.data_ptr(), n_b.data_ptr(), ld_b.data_ptr(), y_b.data_ptr(),
                                                  len(batch), info.data_ptr(), st))
        info_h = info.cpu().numpy()
        for b, (p, f) in enumerate(batch):
            if info_h[b] != 0:
                ok[p] = False
            alpha[p][f] = ys[b]
            done[p] += 1
            if done[p] == n_folds:
                out[p] = _predict(dev, params_list[p], fits, idx_dev, alpha[p]) if ok[p] else None
                alpha[p] = None
        del buf
        start = stop
    return [out[p] for p in range(len(params_list))], ok


def _predict(dev, prm, fits, idx_dev, alphas):
    """out[i][f] = sum over fold f's fit rows j of k(x_i, x_j) alpha_f[j], every row i."""
    torch = dev.torch
    n_folds = len(fits)
    n = dev.n
    W = torch.zeros((n, n_folds), dtype=torch.float64, device=dev.device)
    for f in range(n_folds):
        W[idx_dev[f], f] = alphas[f]
    out = torch.empty((n, n_folds), dtype=torch.float64, device=dev.device)
    work_len = dev.lib.ital_kernel_matvec_workspace(n, n)
    work = torch.empty(max(int(work_len), 1), dtype=torch.float64, device=dev.device)
    for c0 in range(0, n_folds, _MAX_F):
        F = min(_MAX_F, n_folds - c0)
        dev.check(dev.lib.ital_kernel_matvec(dev.Xd.data_ptr(), dev.xnorm.data_ptr(), n, dev.Xd.data_ptr(),
                                             dev.xnorm.data_ptr(), n, dev.ldx, W.data_ptr() + 8 * c0, n_folds, F,
                                             float(prm.get('var', 1.0)), float(prm['length_scale']),
                                             out.data_ptr() + 8 * c0, n_folds, work.data_ptr(), int(work_len), dev.stream()))
    return out.cpu().numpy()


def _scores(dataset, relevance, params_list, n_folds, fewshot, device, max_bytes, dev=None):
    """The reference's cross_validate_gp / cross_validate_fewshot for several parameter sets at once."""
    from sklearn.metrics import average_precision_score, mean_squared_error
    for prm in params_list:
        _check_params(prm)
    X = _features(dataset)
    rows, folds = fold_split(X, relevance, n_folds)
    if relevance is not None:
        relevance = np.asarray(relevance)
        target = relevance
    else:
        target = np.asarray(dataset.y_train, dtype=np.float64)
    fits = []
    for train_ind, test_ind in folds:
        fit_ind = test_ind if fewshot else train_ind
        fits.append((rows[fit_ind], target[rows[fit_ind]] if relevance is not None else target[fit_ind]))
    if dev is None:
        dev = _DeviceRows(X, device)
    preds, ok = _fold_predictions(dev, params_list, fits, max_bytes)
    result = []
    for p in range(len(params_list)):
        if not ok[p]:
            warnings.warn('Matrix is not positive semi-definite.', stacklevel=3)
            result.append(-np.inf)
            continue
        out = preds[p]
        if fewshot:
            perf = []
            for f, (train_ind, test_ind) in enumerate(folds):
                scores = out[rows[train_ind], f]
                if relevance is not None:
                    perf.append(average_precision_score(relevance[rows[train_ind]], scores))
                else:
                    perf.append(-math.sqrt(mean_squared_error(target[train_ind], scores)))
            result.append(np.mean(perf))
        else:
            scores = np.ndarray((len(rows),), dtype=float)
            for f, (train_ind, test_ind) in enumerate(folds):
                scores[test_ind] = out[rows[test_ind], f]
            if relevance is not None:
                result.append(average_precision_score(relevance[rows], scores))
            else:
                result.append(-math.sqrt(mean_squared_error(target, scores)))
    return result


def held_out_scores(dataset, relevance, gp_params, n_folds=10, fewshot=False, *, device=None, max_bytes=DEFAULT_MAX_BYTES):
    """(rows, folds, out): the fold split and every fold GP's predictive mean at every sample (out[i][f]); None when a fold
    Gram is not positive definite.  The quantities cross_validate_gp scores."""
    _check_params(gp_params)
    X = _features(dataset)
    rows, folds = fold_split(X, relevance, n_folds)
    target = np.asarray(relevance) if relevance is not None else np.asarray(dataset.y_train, dtype=np.float64)
    fits = []
    for train_ind, test_ind in folds:
        fit_ind = test_ind if fewshot else train_ind
        fits.append((rows[fit_ind], target[rows[fit_ind]] if relevance is not None else target[fit_ind]))
    preds, ok = _fold_predictions(_DeviceRows(X, device), [gp_params], fits, max_bytes)
    return rows, folds, preds[0] if ok[0] else None


def cross_validate_gp(dataset, relevance, gp_params, n_folds=10, *, device=None, max_bytes=DEFAULT_MAX_BYTES):
    """Performs k-fold cross-validation (reference optimize_parameters.py:28-62).

    Returns the average precision of the held-out predictions for retrieval (relevance given; samples with relevance 0
    are left out), -RMSE against dataset.y_train for regression (relevance None), -inf (with the reference's warning)
    when a fold Gram is not positive definite."""
    return _scores(dataset, relevance, [gp_params], n_folds, False, device, max_bytes)[0]


def cross_validate_fewshot(dataset, relevance, gp_params, n_folds=10, *, device=None, max_bytes=DEFAULT_MAX_BYTES):
    """k-fold cross-validation trained on the smaller part of every split and evaluated on the larger one (reference
    optimize_parameters.py:65-101); the mean over the splits."""
    return _scores(dataset, relevance, [gp_params], n_folds, True, device, max_bytes)[0]


cross_validate_gp.device_sweep = True
cross_validate_fewshot.device_sweep = True


def _evaluate(dataset, relevance, params_list, n_folds, fewshot, device, max_bytes, cache):
    fn = cross_validate_fewshot if fewshot else cross_validate_gp
    if not getattr(fn, 'device_sweep', False):       # a replaced scorer (tests, a user's own): once per value, in order
        return [fn(dataset, relevance, prm, n_folds=n_folds) for prm in params_list]
    if 'dev' not in cache:
        cache['dev'] = _DeviceRows(_features(dataset), device)
    return _scores(dataset, relevance, params_list, n_folds, fewshot, device, max_bytes, dev=cache['dev'])


def optimize_gp_params(dataset, relevance, grid=default_grids['full'], init=default_init, n_folds=10, fewshot=False,
                       verbose=1, *, device=None, max_bytes=DEFAULT_MAX_BYTES):
    """Optimizes the hyper-parameters of a GP kernel for a certain dataset by alternating grid search (reference
    optimize_parameters.py:104-170): returns (dict of the best values, the performance obtained with them).

    All values of the parameter being swept are cross-validated in one device batch; the lines of `verbose` > 1 are
    printed in grid order."""
    cache = {}
    best_params, best_perf = _alternating_search(
        grid, init, lambda cv_list: _evaluate(dataset, relevance, cv_list, n_folds, fewshot, device, max_bytes, cache), verbose)
    return best_params, best_perf if relevance is not None else -best_perf


def _alternating_search(grid, init, evaluate, verbose):
    """The control flow of the reference's optimize_gp_params (optimize_parameters.py:121-170): one parameter of `grid` is
    swept at a time, the others held at their current values (at first `init`'s), until a sweep changes nothing or makes
    things worse.  `evaluate(list of dicts)` gives their performances, higher is better; ties go to the first best value in
    grid order.  Returns (dict of the best values, their performance)."""
    param_names = list(grid.keys())
    cur_params = [init[p] for p in param_names]
    changed = [True] * len(param_names)
    changing_param = 0
    perf = {}
    best_perf = -np.inf

    while any(changed):

        values = list(grid[param_names[changing_param]])
        cv_list = [{param_names[i]: val if i == changing_param else cur_params[i] for i in range(len(param_names))}
                   for val in values]
        results = evaluate(cv_list)
        cur_perfs = {}
        for val, res in zip(values, results):
            cur_perfs[val] = res
            if verbose > 1:
                print('    {} = {} : {:.4f}'.format(param_names[changing_param], val, cur_perfs[val]))
        best_val = max(cur_perfs.keys(), key=lambda v: cur_perfs[v])

        if cur_perfs[best_val] < best_perf:
            break
        best_perf = cur_perfs[best_val]

        if verbose > 0:
            print('{} : {:.4f}'.format(', '.join('{} = {}'.format(param_names[i], best_val if i == changing_param
                                                                  else cur_params[i]) for i in range(len(param_names))),
                                       best_perf))

        changed[changing_param] = (best_val != cur_params[changing_param])
        cur_params[changing_param] = best_val
        perf[tuple(cur_params)] = best_perf
        changing_param = (changing_param + 1) % len(param_names)

        if len(param_names) < 2:
            break

    best_params = max(perf.keys(), key=lambda p: perf[p])
    return dict(zip(param_names, best_params)), best_perf


# ------------------------------------------------------------------------------------- a live session's own labels
#: what session_scores can rank candidates by (all: higher is better)
SESSION_CRITERIA = ('lml', 'loo_logp', 'loo_mse', 'loo_ap')


def _session_gp(gp_or_learner):
    return getattr(gp_or_learner, 'gp', gp_or_learner)


def session_scores(gp_or_learner, params_list, criterion='lml'):
    """Scores hyper-parameter candidates (dicts with `length_scale`, `var`, `noise`; what is missing is the session's current
    value) against the labelled samples of a live session -- a GaussianProcess or a learner -- on the device
    (GaussianProcess.evidence, include/ital_evidence.h).  No ground truth is needed: the session's own m labels are all
    there is.  Returns a list of floats, higher is better:

    - 'lml': log marginal likelihood (Rasmussen & Williams 2.30);
    - 'loo_logp': leave-one-out log predictive probability (5.10);
    - 'loo_mse': minus the mean squared leave-one-out residual;
    - 'loo_ap': average precision of the leave-one-out means against the labels' signs, the reference's criterion
      (optimize_parameters.py:59) with leave-one-out as the folds; ValueError unless the labels hold both signs.

    A candidate whose Gram is not positive definite scores -inf, with the warning of cross_validate_gp."""
    if criterion not in SESSION_CRITERIA:
        raise ValueError('criterion must be one of %s' % ', '.join(SESSION_CRITERIA))
    from .gp import _candidate_params
    gp = _session_gp(gp_or_learner)
    # refuses an unknown key or a non-positive value before any device work
    prm = _candidate_params(gp, [dict(p) for p in params_list])
    if criterion == 'loo_ap':
        from sklearn.metrics import average_precision_score
        y = np.asarray(gp.y if gp.y is not None else [], dtype=np.float64)
        if not (np.any(y > 0) and np.any(y <= 0)):
            raise ValueError("criterion 'loo_ap' needs labels of both signs")
    ev = gp.evidence(prm)
    result = []
    for g in range(len(prm)):
        if not ev['ok'][g]:
            warnings.warn('Matrix is not positive semi-definite.', stacklevel=2)
            result.append(-np.inf)
        elif criterion == 'loo_ap':
            result.append(float(average_precision_score(y > 0, ev['loo_mean'][g])))
        elif criterion == 'loo_mse':
            result.append(-float(ev['loo_mse'][g]))
        else:
            result.append(float(ev[criterion][g]))
    return result


def optimize_session_params(gp_or_learner, grid=default_grids['ls_only'], init=None, criterion='lml', verbose=1):
    """optimize_gp_params for a live session: the same alternating grid search, tie rule and printed lines, scored by
    session_scores on the session's own labels instead of cross-validation against ground truth.  `init`: where the search
    starts (None: the session's current parameters); parameters that `grid` does not name stay at the session's values.
    Returns (dict of the best values, their score) -- what set_params() takes."""
    gp = _session_gp(gp_or_learner)
    if init is None:
        init = {'length_scale': gp.length_scale, 'var': gp.var, 'noise': gp.noise}
    return _alternating_search(grid, init, lambda cv_list: session_scores(gp_or_learner, cv_list, criterion), verbose)


# ------------------------------------------------------------------ a live session, continuously: evidence gradients
PARAM_NAMES = ('length_scale', 'var', 'noise')

#: the box fit_session_params searches by default: the span of default_grids['full'] in length scale and variance, and a
#: noise between the grid's floor, 1e-8 (strictly positive: the factor's pivots stay away from 0), and the variance's scale
DEFAULT_FIT_BOUNDS = {'length_scale': (1e-3, 25.0), 'var': (0.1, 10.0), 'noise': (1e-8, 1.0)}


#: L-BFGS-B's stopping rules in maximize_lml.  The objective is a SUM over restarts: scipy's default relative decrease
#: (ftol 2.2e-9) of the sum would stop the run while single restarts still climb, so both rules are set near machine precision
#: and `maxiter` is what ends a run that keeps creeping.
LBFGSB_OPTIONS = dict(maxcor=10, ftol=1e-15, gtol=1e-9, maxls=30)


class _Dropped(Exception):
    """An evaluation inside scipy's iteration came back with restarts that are not positive definite."""

    def __init__(self, bad):
        Exception.__init__(self)
        self.bad = bad


def _bounds_array(bounds):
    b = dict(DEFAULT_FIT_BOUNDS)
    b.update(bounds or {})
    unknown = set(b) - set(PARAM_NAMES)
    if unknown:
        raise TypeError('unexpected GP parameters: %s' % ', '.join(sorted(unknown)))
    arr = np.array([[float(b[k][0]), float(b[k][1])] for k in PARAM_NAMES])
    if not np.all((arr[:, 0] > 0) & (arr[:, 0] <= arr[:, 1])):
        raise ValueError('bounds must satisfy 0 < low <= high')
    return arr


def _free_columns(free):
    free = tuple(free)
    unknown = set(free) - set(PARAM_NAMES)
    if unknown:
        raise TypeError('unexpected GP parameters: %s' % ', '.join(sorted(unknown)))
    cols = [k for k, name in enumerate(PARAM_NAMES) if name in free]
    if not cols:
        raise ValueError('no parameter to fit')
    return cols


def maximize_lml(evaluate, starts, bounds=None, free=PARAM_NAMES, maxiter=100):
    """Maximises a log marginal likelihood over the logarithms of (length_scale, var, noise) from R starting points at once
    (host only: `evaluate` is all it knows of the model).

    `evaluate(theta[R', 3]) -> (lml[R'], grad[R', 3], ok[R'])`: values and gradients in (log length_scale, log var,
    log noise) of a batch of parameter triples -- GaussianProcess.evidence_grad behind fit_session_params.  `starts`: [R, 3]
    triples; `bounds`: dict name -> (low, high), defaults DEFAULT_FIT_BOUNDS (starts are clipped into them); `free`: the
    names that move.  The other columns keep their start values bit for bit, and their gradient components are ignored.

    One scipy.optimize.minimize(method='L-BFGS-B', jac=True) runs over the concatenated free log-parameters of all restarts
    with the objective -sum_r lml_r.  The sum is separable, so its gradient is the restarts' own gradients side by side and
    every restart climbs its own hill, while one call of `evaluate` serves all of them per iteration.  A restart whose
    evaluation comes back ok = False (its Gram is not positive definite there) is dropped, and the survivors resume from the
    last iterate, with what is left of `maxiter`.  Because the line search accepts a step on the SUM, a single restart may
    lose a little in a step that the others gain from: each restart therefore reports the best point at which it was
    evaluated, which is never below its start.

    Returns (best, lml, records): `best` a dict of all three parameters at the best restart (None and -inf if no restart is
    left), `records` one dict per start -- `start`, `params`, `lml` (its best evaluation), `dropped`, and the `iterations`
    and `evaluations` of the run it was part of."""
    from scipy.optimize import minimize
    cols = _free_columns(free)
    box = _bounds_array(bounds)
    starts = np.array(starts, dtype=np.float64).reshape(-1, 3)
    R, nf = len(starts), len(cols)
    start_theta = starts.copy()
    start_theta[:, cols] = np.clip(starts[:, cols], box[cols, 0], box[cols, 1])
    x_start = np.log(start_theta[:, cols])
    best_lml = np.full(R, -np.inf)
    best_theta = start_theta.copy()
    dropped = np.zeros(R, dtype=bool)
    alive = np.arange(R)
    x_cur = x_start.copy()                      # [R, nf]: the last iterate of every restart
    evaluations, iterations = 0, 0

    def theta_of(x, rows):
        theta = start_theta[rows].copy()
        exact = x == x_start[rows]             # a point that has not moved is its start, not exp(log(start))
        theta[:, cols] = np.where(exact, start_theta[rows][:, cols], np.exp(x))
        return theta

    while len(alive) and iterations < max(1, maxiter):
        rows = alive

        def objective(xflat):
            nonlocal evaluations
            x = xflat.reshape(len(rows), nf)
            theta = theta_of(x, rows)
            lml, grad, ok = evaluate(theta)
            evaluations += 1
            lml, grad = np.asarray(lml, dtype=np.float64), np.asarray(grad, dtype=np.float64).reshape(len(rows), 3)
            ok = np.asarray(ok, dtype=bool) & np.isfinite(lml) & np.all(np.isfinite(grad[:, cols]), axis=1)
            better = ok & (lml > best_lml[rows])
            best_lml[rows[better]] = lml[better]
            best_theta[rows[better]] = theta[better]
            if not ok.all():
                raise _Dropped(~ok)
            return -float(lml.sum()), -grad[:, cols].reshape(-1)

        def callback(xk):
            nonlocal iterations
            iterations += 1
            x_cur[rows] = xk.reshape(len(rows), nf)

        try:
            minimize(objective, x_cur[rows].reshape(-1), jac=True, method='L-BFGS-B',
                     bounds=[tuple(np.log(box[c])) for _ in rows for c in cols], callback=callback,
                     options=dict(LBFGSB_OPTIONS, maxiter=max(1, maxiter - iterations)))
            break
        except _Dropped as e:
            dropped[rows[e.bad]] = True
            alive = rows[~e.bad]

    records = [dict(start=dict(zip(PARAM_NAMES, (float(v) for v in starts[r]))),
                    params=dict(zip(PARAM_NAMES, (float(v) for v in best_theta[r]))) if np.isfinite(best_lml[r]) else None,
                    lml=float(best_lml[r]), dropped=bool(dropped[r]), iterations=iterations, evaluations=evaluations)
               for r in range(R)]
    best_lml = np.where(dropped, -np.inf, best_lml)          # the result comes from the survivors
    if not np.any(np.isfinite(best_lml)):
        return None, -np.inf, records
    r = int(np.argmax(best_lml))
    return records[r]['params'], float(best_lml[r]), records


def session_starts(init, restarts=8, bounds=None, free=PARAM_NAMES):
    """The starting points of fit_session_params, [R, 3] rows of (length_scale, var, noise), R <= restarts.  Row 0 is `init`.
    The others are a fixed design inside the box -- no random generator is involved: n_l length scales crossed with n_n
    noise levels, length scale varying fastest, of which the first restarts - 1 are taken; n_n = 2 when at least four
    points are wanted, else 1, and n_l = ceil((restarts - 1) / n_n).  Both sets are log-spaced and strictly inside their
    bounds, low (high / low)^(k / (n + 1)), k = 1 .. n.  `var` starts at init's value everywhere, and so does a parameter
    that is not in `free` (the design then collapses along it; duplicate rows are left out)."""
    cols = _free_columns(free)
    box = _bounds_array(bounds)
    init = np.array([float(init[k]) for k in PARAM_NAMES])
    rows = [init]
    want = max(0, int(restarts) - 1)
    if want:
        n_n = 2 if (want >= 4 and 2 in cols and 0 in cols) else 1
        n_l = -(-want // n_n)
        inside = lambda lo, hi, n: [lo * (hi / lo) ** (k / (n + 1.0)) for k in range(1, n + 1)]
        ls = inside(box[0, 0], box[0, 1], n_l) if 0 in cols else [init[0]]
        if 2 in cols:
            ns = inside(box[2, 0], box[2, 1], n_n if 0 in cols else want)
        else:
            ns = [init[2]]
        for noise in ns:
            for l in ls:
                row = np.array([l, init[1], noise])
                if len(rows) <= want and not any(np.array_equal(row, r) for r in rows):
                    rows.append(row)
    return np.array(rows)


#: the criteria fit_session_params can climb: those of session_scores that have a gradient on the device
FIT_CRITERIA = ('lml', 'loo_logp', 'loo_mse')


def fit_session_params(gp_or_learner, params=PARAM_NAMES, init=None, restarts=8, bounds=None, maxiter=100, verbose=0,
                       records=None, criterion='lml'):
    """Fits kernel hyper-parameters of a live session -- a GaussianProcess or a learner -- to its own labels by maximising the
    log marginal likelihood continuously, from its gradient on the device (GaussianProcess.evidence_grad,
    include/ital_evidence_grad.h): what GaussianProcessRegressor.fit does, and the other half of optimize_session_params,
    which can only find what lies on its grid.

    `params`: the names that are fitted; the others stay at `init`.  `init`: dict of starting values (None, or a missing
    name: the session's current value); it is restart 0.  The other restarts are the fixed design of session_starts inside
    `bounds` (dict name -> (low, high); what is missing comes from DEFAULT_FIT_BOUNDS, whose noise floor is 1e-8); all of
    them run in one L-BFGS-B iteration (maximize_lml), one device call per evaluation.  No random generator is touched.
    `verbose`: 1 prints the result, 2 every restart.  `records`: a list that receives maximize_lml's per-restart records.
    Returns (dict of the fitted values of `params`, their lml) -- what set_params() takes -- or (None, -inf) if no start has
    a positive definite Gram.

    `criterion`: 'lml', or one of the closed-form leave-one-out scores of session_scores, 'loo_logp' and 'loo_mse', climbed
    from GaussianProcess.loo_grad (include/ital_loo_grad.h) through the same maximize_lml; the score returned is then the
    criterion's value in session_scores' orientation (minus the mse).  'loo_ap' has no gradient: ValueError, as for any other
    name.  loo_mse does not change when var and noise are scaled together, so it fits at most one of them: ValueError."""
    if criterion not in FIT_CRITERIA:
        raise ValueError("criterion must be one of %s: %r has no gradient" % (', '.join(FIT_CRITERIA), criterion))
    gp = _session_gp(gp_or_learner)
    cols = _free_columns(params)
    if criterion == 'loo_mse' and 1 in cols and 2 in cols:
        raise ValueError('loo_mse does not change when var and noise are scaled together: fit at most one of var and noise')
    start = {'length_scale': gp.length_scale, 'var': gp.var, 'noise': gp.noise}
    unknown = set(init or {}) - set(PARAM_NAMES)
    if unknown:
        raise TypeError('unexpected GP parameters: %s' % ', '.join(sorted(unknown)))
    start.update(init or {})
    box = _bounds_array(bounds)
    # restart 0 is never clipped: the box grows to hold it (a fitted parameter that starts at 0 has no logarithm: ValueError)
    if any(not float(start[PARAM_NAMES[c]]) > 0 for c in cols):
        raise ValueError('a fitted parameter must start at a positive value')
    bounds = {name: (min(box[k, 0], float(start[name])), max(box[k, 1], float(start[name]))) if k in cols
              else tuple(box[k]) for k, name in enumerate(PARAM_NAMES)}
    starts = session_starts(start, restarts, bounds, params)

    def evaluate(theta):
        cands = [dict(zip(PARAM_NAMES, (float(v) for v in row))) for row in theta]
        if criterion == 'lml':
            ev = gp.evidence_grad(cands)
            return ev['lml'], ev['grad'], ev['ok']
        ev = gp.loo_grad(cands)
        if criterion == 'loo_mse':
            return -ev['loo_mse'], -ev['grad_mse'], ev['ok']
        return ev['loo_logp'], ev['grad_logp'], ev['ok']

    best, lml, recs = maximize_lml(evaluate, starts, bounds, params, maxiter)
    if records is not None:
        records.extend(recs)
    if verbose >= 2:
        for r, rec in enumerate(recs):
            print('restart {}: {} -> {} : {:.4f}{}'.format(r, rec['start'], rec['params'], rec['lml'],
                                                           ' (dropped)' if rec['dropped'] else ''))
    if best is None:
        return None, -np.inf
    best = {PARAM_NAMES[c]: best[PARAM_NAMES[c]] for c in cols}
    if verbose >= 1:
        print('{} : {:.4f}'.format(', '.join('{} = {}'.format(k, v) for k, v in best.items()), lml))
    return best, lml


# ------------------------------------------------------------------------------------------------------------------ CLI
USAGE = '''
Optimizes GP hyper-parameters for a given dataset using alternating optimization.

Usage: {} <experiment-config-file> [--<override-option>=<override-value> ...]

The [EXPERIMENT] section of the given config file may specify the following
configuration directives to control the optimization:

     - grid: either "full" to optimize length scale, variance, and noise of the
             kernel or "ls_only" to optimize the length scale only (default: full).
     - n_folds: number of folds for k-fold cross validation (default: 10).
     - few_shot: boolean specifying whether the GP should be trained on the
                 smaller fraction of the data and evaluated on the bigger
                 one instead of the normal k-fold cross-validation (default: False).
     - verbosity: verbosity level between 0 and 2 (default: 1).
     - query_classes: classes to optimize for (default: all).

All directives from the [EXPERIMENT] section may also be overriden on the
command line by passing --key=value arguments.
'''


def parse_args(argv):
    """(config file or None, overrides) as the reference parses sys.argv[1:] (optimize_parameters.py:175-190); raises
    SystemExit on an unexpected argument."""
    config_file = None
    overrides = {}
    for arg in argv:
        if arg.lower() == '--help':
            config_file = None
            break
        elif arg.startswith('--'):
            k, v = arg[2:].split('=', maxsplit=1)
            overrides[k] = v
        elif config_file is None:
            config_file = arg
        else:
            print('Unexpected argument: {}'.format(arg))
            raise SystemExit(1)
    return config_file, overrides


def main(argv=None, *, device=None):
    from . import harness
    argv = sys.argv[1:] if argv is None else argv
    config_file, overrides = parse_args(argv)
    if config_file is None:
        print(USAGE.format('python -m ital_amd.tune'))
        return None
    config = harness.read_config_file(config_file, 'EXPERIMENT', overrides)
    name = config['EXPERIMENT']['dataset']
    dataset = harness.load_dataset(name, **(config[name] if name in config else {}))
    grid = default_grids[config.get('EXPERIMENT', 'grid', fallback='full')]
    n_folds = config.getint('EXPERIMENT', 'n_folds', fallback=10)
    fewshot = config.getboolean('EXPERIMENT', 'few_shot', fallback=False)
    verbose = config.getint('EXPERIMENT', 'verbosity', fallback=1)

    query_classes = str(config.get('EXPERIMENT', 'query_classes', fallback='')).split()
    if len(query_classes) == 0:
        query_classes = list(dataset.class_relevance.keys())
    else:
        for i in range(len(query_classes)):
            try:
                query_classes[i] = int(query_classes[i])
            except ValueError:
                pass

    # Optimize GP parameters individually for each class
    best_params = {}
    best_perf = {}
    for di, ds in enumerate([dataset]):
        for lbl in query_classes:
            print('--- DATASET {}, CLASS {} ---'.format(di + 1, lbl))
            relevance, _ = ds.class_relevance[lbl]
            lbl_best, lbl_perf = optimize_gp_params(ds, relevance, grid, n_folds=n_folds, fewshot=fewshot, verbose=verbose,
                                                    device=device)
            best_params[(di, lbl)] = lbl_best
            best_perf[(di, lbl)] = lbl_perf
            print()

    for di, lbl in best_params.keys():
        print('Best parameters for dataset {}, class {} (AP: {:.2f}): {!r}'.format(di + 1, lbl, best_perf[(di, lbl)],
                                                                                  best_params[(di, lbl)]))
    return best_params, best_perf


if __name__ == '__main__':
    main()
