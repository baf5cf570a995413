"""The lattice sums in which the chains of a lane share reciprocal seeds (csrc/device_math.h fast_div_group; score.hip
ITAL_QMC_BATCH_DIV: Phi and the central Phi^-1 in qmc_main_kernel<3>, the central Phi^-1 in qmc_main_kernel<4>): a round of
k = 4 -- greedy steps t = 1 .. 4, so both kernels -- against the oracle at the tolerance of test_gpu_parity.py, the picks
and the MVNUNI draw counts equal to the oracle's, as one call and step by step, for the three label estimations.

What can go wrong in a seed group is a chain whose denominator is special next to live ones, so the inputs are those of
test_gpu_shared_last_round.py (same generator, same seeds: their meta-word statistics are asserted there and again here):
  (a) rows that nearly duplicate a labelled sample: their variable is decided (|mean| / sd ~ 700), chains reach
      |z| > 37 -- Phi exactly 0 or 1, numerator 0 / -2^-600 over denominator 1 in mvn_phi_nd -- and interval widths of
      exactly 0 or 1 feed Phi^-1 the arguments 0 and 1 (tail arguments, whose central quotient is discarded) in the same
      group as live chains;
  (b) dead candidates (the picks of the earlier steps) between live ones;
  (c) records decided early next to integrated ones, and calls with negated variables (flip_width after the shared seed).
Run on the GPU box: python -m pytest tests -m gpu."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = 4
NPAT = 1 << T
REC = T * (T - 1) // 2 + T + 1 + 5 * (T - 1)      # doubles per prepared call (score.hip Qmc<4>::REC)
R_META = T * (T - 1) // 2 + T
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


@pytest.mark.parametrize("seed,n,d,ndup,mode", [
    (24, 150, 5, 5, "mean"),
    (23, 120, 10, 4, "optimistic"),
    (21, 96, 6, 4, "pessimistic"),
])
def test_round_with_shared_seeds_against_oracle(dev, seed, n, d, ndup, mode):
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
    assert len(B.trace) == T

    for round_call in (True, False):           # the round as one call, and step by step (whose workspace is read below)
        mvn_stream.GLOBAL.reset()
        A = ITAL(X, length_scale=ls, label_estimation=mode, device=dev)
        A.keep_scores = True
        A.round_call = round_call
        A.update(labels)
        generic, fetch_generic = [], A._fetch_generic
        A._fetch_generic = lambda *a, **kw: (generic.append(1), fetch_generic(*a, **kw))[1]
        got = A.fetch_unlabelled(T)
        assert not generic, "the round fell back to the general scorer: these inputs do not reach qmc_main_kernel<3> / <4>"
        for t, (cand, vals, _) in enumerate(B.trace):
            mine = A.last_scores[t].cpu().numpy()[[pos[c] for c in cand]]
            err = np.abs(mine - vals) / (1e-10 + 1e-8 * np.abs(vals))
            print(f"{mode} seed {seed} round_call {round_call} step {t}: max error / tolerance {float(err.max()):.3g}")
            np.testing.assert_allclose(mine, vals, rtol=1e-8, atol=1e-10, err_msg=f"step {t}")
        assert got == want
        assert mvn_stream.GLOBAL.draws == omvn.rng_draws()

    # ---- the records of the t = 4 step, as the scorer left them (one slab at these sizes)
    work = A._fetch_bufs["qmc_work"].cpu().numpy()
    dead = sorted(pos[c] for c in want[:T - 1])
    assert any(0 < p < n_cand - 1 for p in dead)                                      # (b)
    live = [p for p in range(n_cand) if p not in dead]
    meta = work[:n_cand * NPAT * REC].reshape(n_cand, NPAT, REC)[:, :, R_META].copy().view(np.int64)[live]
    evaluated = (meta & META_EVAL) != 0
    print(f"{mode} seed {seed}: {len(live)} live candidates, {int(evaluated.sum())} records integrated, "
          f"{int((~evaluated).sum())} decided early")
    assert evaluated.any() and (~evaluated).any()                                     # (a), (c)
    limit_types = (meta[evaluated] >> 8) & (NPAT - 1)
    assert ((limit_types != 0) & (limit_types != NPAT - 1)).any()                     # (c)
