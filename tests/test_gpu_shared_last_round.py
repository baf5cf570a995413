"""The t = 4 lattice sum in which a wave takes four records (consecutive sign patterns of one candidate) and evaluates the
16 chains their full rounds leave over in one round for the four (csrc/qmc_share.h, qmc_main_kernel<4>): MI vectors against
the oracle at the tolerance of test_gpu_parity.py, on inputs that take every path of it -- asserted from the record meta
words the scorer leaves in its workspace:
  (a) groups of four consecutive sign patterns of one candidate in which some records are decided early and some are
      integrated (the lanes of the former run a dead copy in the shared round): candidates that nearly duplicate a labelled
      sample (|mean| / sd ~ 700 with noise 1e-6) have their own variable decided, so half of their patterns are empty before
      any lattice point; where such a sample is picked, the same holds for every candidate of the later steps,
  (b) dead candidates (the picks of the earlier steps) between live ones,
  (c) more than one slab of the workspace (`qmc_work_bytes` lowered),
  (d) label_estimation 'optimistic' / 'pessimistic' (sums flagged for the recomputation in the reference's order),
  (e) calls with negated variables (mixed limit types after the re-ordering).
Run on the GPU box: python -m pytest tests -m gpu."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = 4
NPAT = 1 << T
REC = T * (T - 1) // 2 + T + 1 + 5 * (T - 1)      # doubles per prepared call (score.hip Qmc<4>::REC)
R_META = T * (T - 1) // 2 + T
CAND_DOUBLES = NPAT * (REC + 1) + 3               # records, terms, generator state per candidate
META_EVAL = 1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


def _inputs(seed, n, d, ndup):
    """Random points; the last `ndup` odd rows nearly duplicate one of the five labelled samples each."""
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    ls = float(np.sqrt(d / 12.0))
    lab = [int(i) for i in rng.choice(n - 2 * ndup, 5, replace=False)]
    for j in range(ndup):
        X[n - 1 - 2 * j] = X[lab[j % 5]] + 1e-3 * ls * rng.standard_normal(d) / np.sqrt(d)
    labels = {i: (1 if X[i, 0] > 0.5 else -1) for i in lab}
    return X, ls, labels


@pytest.mark.parametrize("seed,n,d,ndup,mode,work_bytes", [
    (22, 330, 8, 6, "mean", 1 << 19),          # three slabs of 150 candidates
    (24, 150, 5, 5, "mean", None),
    (23, 120, 10, 4, "optimistic", None),
    (21, 96, 6, 4, "pessimistic", None),
    (26, 200, 6, 4, "pessimistic", 1 << 19),   # two slabs
    (27, 220, 10, 4, "optimistic", 1 << 19),   # two slabs
])
def test_shared_last_round_against_oracle(dev, seed, n, d, ndup, mode, work_bytes):
    from ital_amd import ITAL, mvn_stream
    from oracle import mvn as omvn
    from oracle.ital import OracleITAL
    X, ls, labels = _inputs(seed, n, d, ndup)
    omvn.rng_reset()
    B = OracleITAL(X, length_scale=ls, label_estimation=mode)
    B.update(labels)
    want = [int(i) for i in B.fetch_unlabelled(T)]
    cand0 = B.trace[0][0]
    pos = {c: i for i, c in enumerate(cand0)}
    n_cand = len(cand0)

    for round_call in (True, False):           # the round as one call, and step by step (whose workspace is read below)
        mvn_stream.GLOBAL.reset()
        A = ITAL(X, length_scale=ls, label_estimation=mode, device=dev)
        A.keep_scores = True
        A.round_call = round_call
        if work_bytes is not None:
            A.qmc_work_bytes = work_bytes
        A.update(labels)
        generic, fetch_generic = [], A._fetch_generic
        A._fetch_generic = lambda *a, **kw: (generic.append(1), fetch_generic(*a, **kw))[1]
        got = A.fetch_unlabelled(T)
        assert not generic, "the round fell back to the general scorer: these inputs do not reach qmc_main_kernel<4>"
        for t, (cand, vals, _) in enumerate(B.trace):
            mine = A.last_scores[t].cpu().numpy()[[pos[c] for c in cand]]
            err = np.abs(mine - vals) / (1e-10 + 1e-8 * np.abs(vals))
            print(f"{mode} seed {seed} round_call {round_call} step {t}: max error / tolerance {float(err.max()):.3g}")
            np.testing.assert_allclose(mine, vals, rtol=1e-8, atol=1e-10, err_msg=f"step {t}")
        assert got == want
        assert mvn_stream.GLOBAL.draws == omvn.rng_draws()

    # ---- the records of the last slab of the t = 4 step, as the scorer left them
    work = A._fetch_bufs["qmc_work"].cpu().numpy()
    slab = min(work.size // CAND_DOUBLES, n_cand)
    if work_bytes is not None:
        assert n_cand > slab, "the step was meant to run in several slabs"            # (c)
    lo = ((n_cand - 1) // slab) * slab
    dead = sorted(pos[c] for c in want[:T - 1])
    assert any(0 < p < n_cand - 1 for p in dead)                                      # (b)
    live = [p for p in range(lo, n_cand) if p not in dead]
    meta = work[:(n_cand - lo) * NPAT * REC].reshape(n_cand - lo, NPAT, REC)[:, :, R_META].copy().view(np.int64)
    meta = meta[[p - lo for p in live]]
    evaluated = (meta & META_EVAL) != 0
    per_group = evaluated.reshape(len(live), NPAT // 4, 4).sum(axis=2)
    n_mixed = int(((per_group > 0) & (per_group < 4)).sum())
    print(f"{mode} seed {seed}: {len(live)} live candidates in the last slab, {int(evaluated.sum())} records integrated, "
          f"{int((~evaluated).sum())} decided early, {n_mixed} groups of four with both kinds, {int((per_group == 0).sum())} with none")
    assert evaluated.any() and (~evaluated).any() and n_mixed > 0                     # (a)
    limit_types = (meta[evaluated] >> 8) & (NPAT - 1)
    assert ((limit_types != 0) & (limit_types != NPAT - 1)).any()                     # (e)
