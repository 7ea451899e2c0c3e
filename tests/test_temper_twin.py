"""The definitions of parallel tempering (tests/_temper_np.py, the float64 twin of csrc/mdbn_temper.hip) against ground truth
on the CPU: a planted two-mode layer whose exact visible marginals come from enumerating the hidden states -- tempered
ladders find them, a plain chain from the same start does not -- and the invariance of the swap move."""
import numpy as np
import pytest

import _temper_np as T

SEED, STREAM, STEP = 5, 3, 11
M, R, N_SWEEPS, BURN_IN = 64, 16, 1200, 300


def ladder_error(v_avg, exact):
    """``(max_i |mean over ladders - exact|, bound)`` with bound = max(4 SE, 0.01), SE the largest across-ladder standard error."""
    v_avg = np.asarray(v_avg, dtype=np.float64)
    err = np.abs(v_avg.mean(axis=0) - exact).max()
    se = (v_avg.std(axis=0, ddof=1) / np.sqrt(v_avg.shape[0])).max()
    return float(err), float(max(4.0 * se, 0.01))


@pytest.fixture(scope="module")
def two_mode():
    W, c, b, bA = T.two_mode_model(24, 12, 0)
    return W, c, b, bA, T.exact_visible_mean(W, c, b)


def test_two_mode_ground_truth(two_mode):
    """(a) 64 ladders of 16 temperatures from h = 0 reach the exact marginals of the two-mode layer."""
    W, c, b, bA, exact = two_mode
    r = T.pt_twin(W, c, b, bA, False, np.linspace(0, 1, R), np.zeros((M * R, 12)), N_SWEEPS, BURN_IN, SEED, STREAM, STEP)
    err, bound = ladder_error(r["v_avg"], exact)
    tries = M * N_SWEEPS / 2.0
    print("two-mode 24->12, %d ladders x %d temperatures, %d sweeps: error %.4f (bound %.4f), swap acceptance %.2f .. %.2f"
          % (M, R, N_SWEEPS, err, bound, r["accepted"].min() / tries, r["accepted"].max() / tries))
    assert err <= bound, (err, bound)
    assert sorted(r["rank"][0]) == list(range(R))


def test_plain_chain_is_stuck(two_mode):
    """(b) the same model and start with the swaps disabled: the beta = 1 chains never reach the heavy mode."""
    W, c, b, bA, exact = two_mode
    r = T.pt_twin(W, c, b, bA, False, np.linspace(0, 1, R), np.zeros((M * R, 12)), N_SWEEPS, BURN_IN, SEED, STREAM, STEP, swaps=False)
    err, _ = ladder_error(r["v_avg"], exact)
    print("two-mode 24->12 without swaps: error %.4f" % err)
    assert r["accepted"].sum() == 0
    assert err > 0.3, err


def test_swap_leaves_the_target_invariant():
    """(c) V = 3, H = 2, R = 2: the pair (v at beta_0, v at beta_1) must be distributed as the PRODUCT of the two exact
    marginals -- what a swap rule with a wrong acceptance ratio breaks.  512 ladders, each a time average over 600 sweeps after
    100; the across-ladder standard error per cell."""
    V, H, n, burn, Ml = 3, 2, 700, 100, 512
    rs = np.random.RandomState(2)
    W, c, b, bA = rs.normal(0, 1.0, (V, H)), rs.normal(0, 0.5, H), rs.normal(0, 0.5, V), rs.normal(0, 0.5, V)
    betas = np.array([0.3, 1.0], dtype=np.float32)
    r = T.pt_twin(W, c, b, bA, False, betas, np.zeros((Ml * 2, H)), n, burn, SEED, STREAM, STEP)
    states = ((np.arange(8)[:, None] >> np.arange(V)[None, :]) & 1).astype(np.float64)
    hid = ((np.arange(4)[:, None] >> np.arange(H)[None, :]) & 1).astype(np.float64)
    marg = []
    for beta in betas.astype(np.float64):
        logp = beta * (states @ W @ hid.T + (hid @ c)[None, :]) + (states @ (bA + beta * (b - bA)))[:, None]
        p = np.exp(logp - logp.max()).sum(axis=1)
        marg.append(p / p.sum())
    want = np.outer(marg[0], marg[1])
    # the rank a slot held when it drew v in sweep t: the map after sweep t - 1's swap
    before = np.concatenate([np.tile(np.arange(2), (1, Ml, 1)), r["trace_swaps"][:-1, :, 0, :]], axis=0)        # [n, M, 2]
    code = (r["trace_v"].reshape(n, Ml, 2, V) * (1 << np.arange(V))).sum(axis=3).astype(np.int64)               # [n, M, slot]
    slot0 = np.argmin(before, axis=2)                                                                         # slot of rank 0
    c0 = np.take_along_axis(code, slot0[:, :, None], axis=2)[:, :, 0]
    c1 = np.take_along_axis(code, 1 - slot0[:, :, None], axis=2)[:, :, 0]
    cell = (8 * c0 + c1)[burn:]                                                                               # [n - burn, M]
    freq = np.stack([(cell == k).mean(axis=0) for k in range(64)], axis=1)                                    # [M, 64]
    mean, se = freq.mean(axis=0), freq.std(axis=0, ddof=1) / np.sqrt(Ml)
    z = np.abs(mean - want.reshape(-1)) / np.maximum(se, 1e-12)
    tries = Ml * n / 2.0
    print("swap invariance 3->2, R = 2: acceptance %.2f, largest |error| / SE over the 64 cells %.2f" % (r["accepted"][0] / tries, z.max()))
    assert 0.05 < r["accepted"][0] / tries < 0.98
    assert z.max() <= 4.0, z.max()
