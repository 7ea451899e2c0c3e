"""The float64 numpy twin of the device's clamped Gibbs sampling (tests/_clamp_np.py) against exact posteriors and against
itself (no GPU): the reference restatement the GPU tests compare with must itself sit inside the bounds they use."""
import numpy as np
import pytest

import _ais_np as A
import _clamp_np as Cn

# chains, steps and burn-in of the ground-truth tests (here and in tests/test_gpu_clamp.py), chosen so that the twin's
# largest standard error stays under SE_CAP on every case: a 4-sigma test hides nothing only if sigma is small
M, N_STEPS, BURN_IN, SE_CAP = 128, 600, 100, 0.01


def ground_truth_case(V, H, s, gauss):
    """Parameters of a brute-force case of _ais_np.CASES, one row with about half its columns observed, and the exact
    E[v | v_obs], E[h | v_obs]."""
    W, c, b, _ = A.case_params(V, H, s, gauss)
    rs = np.random.RandomState(11)
    held = Cn.half_mask(V)[0] != 0
    row = (rs.normal(size=V).astype(np.float32) + b) if gauss else (rs.uniform(size=V) < 0.5).astype(np.float32)
    ev, eh = Cn.exact_posterior(W, c, b, gauss, row, held)
    return W, c, b, row, held, ev, eh


@pytest.mark.parametrize("V,H,s,gauss", A.CASES)
def test_twin_against_exact_posterior(V, H, s, gauss):
    """M = 128 chains of 600 steps (100 burn-in) from the model's base, Philox seed 1: the chain-averaged v_avg / h_avg within 4
    standard errors (std over chains / sqrt(M)) of the exact posterior means, and the largest standard error <= 0.01.  Gaussian
    visibles run the Gibbs sampler of the model (``sampler``: the hidden sample goes down, unit noise), as RBM.impute does.

    Measured (largest standard error; largest |error|; largest |error| / standard error):
      24 -> 12 RBM    v 0.00121  0.00179  2.47     h 0.00111  0.00176  2.32
      100 -> 16 RBM   v 0.00079  0.00100  2.28     h 0.00129  0.00126  1.38
      20 -> 10 GRBM   v 0.00253  0.00257  1.72     h 0.00092  0.00107  1.68
      40 -> 14 GRBM   v 0.00230  0.00348  1.59     h 0.00131  0.00181  1.66
    (The reference's GRBM chain, which feeds the hidden MEAN down, is a mean-field iteration and not a sampler of the posterior:
    test_reference_grbm_chain_is_not_a_posterior_sampler.)"""
    W, c, b, row, held, ev, eh = ground_truth_case(V, H, s, gauss)
    base = b.astype(np.float64) if gauss else Cn.sigmoid(b.astype(np.float64))
    start = np.repeat(np.where(held, row, base)[None], M, axis=0)
    r = Cn.clamp_twin(W, c, b, gauss, start, start, held[None], N_STEPS, BURN_IN, 1, 0, 0, sampler=gauss)
    worst_se, worst_z = 0.0, 0.0
    for name, est, exact in (("v", r["v_avg"][:, ~held], ev[~held]), ("h", r["h_avg"], eh)):
        m, se = est.mean(axis=0), est.std(axis=0) / np.sqrt(M)
        z = np.abs(m - exact) / np.maximum(se, 1e-12)
        print("twin %d->%d %s %s: largest standard error %.5f, largest |error| %.5f, largest |error| / standard error %.2f"
              % (V, H, "GRBM" if gauss else "RBM", name, se.max(), np.abs(m - exact).max(), z.max()))
        worst_se, worst_z = max(worst_se, se.max()), max(worst_z, z.max())
    np.testing.assert_array_equal(r["v_avg"][:, held], start[:, held])
    assert worst_se <= SE_CAP, worst_se
    assert worst_z <= 4.0, worst_z


def test_reference_grbm_chain_is_not_a_posterior_sampler():
    """Why RBM.impute does not run a GRBM's ``gibbs_vhv`` chain: with the hidden mean fed down the averages settle, with tiny
    standard errors, on values that are not the posterior means (measured on 40 -> 14: |error| 0.012 at a standard error of
    0.0012 with the visible noise on; without it the chain is deterministic).  Kept as a record of that fact, not as a bound."""
    V, H, s, gauss = A.CASES[3]
    W, c, b, row, held, ev, eh = ground_truth_case(V, H, s, gauss)
    start = np.repeat(np.where(held, row, b.astype(np.float64))[None], M, axis=0)
    r = Cn.clamp_twin(W, c, b, True, start, start, held[None], N_STEPS, BURN_IN, 1, 0, 0, add_noise=True)
    m, se = r["h_avg"].mean(axis=0), r["h_avg"].std(axis=0) / np.sqrt(M)
    assert (np.abs(m - eh) / se).max() > 8.0
    r = Cn.clamp_twin(W, c, b, True, start[:4], start[:4], held[None], 50, 10, 1, 0, 0)
    assert r["h_avg"].std(axis=0).max() < 1e-12


@pytest.mark.parametrize("gauss", [False, True])
def test_exact_posterior_against_full_enumeration(gauss):
    """The closed form over the missing visibles against a plain enumeration of (h, missing v) on a layer small enough for it
    (Bernoulli), and against the conditional-Gaussian algebra done the long way (Gaussian: numeric integration on a grid)."""
    V, H = 6, 3
    W, c, b, _ = A.case_params(V, H, 0.6, gauss, dtype=np.float64)
    held = np.array([True, False, True, False, False, True])
    row = np.array([1.0, 0, 0.0, 0, 0, 1.0]) if not gauss else np.array([0.3, 0, -1.2, 0, 0, 0.8])
    ev, eh = Cn.exact_posterior(W, c, b, gauss, row, held)
    miss = np.flatnonzero(~held)
    hs = ((np.arange(1 << H)[:, None] >> np.arange(H)) & 1).astype(np.float64)
    if gauss:
        g = np.linspace(-9, 9, 181)
        vs = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    else:
        vs = ((np.arange(1 << miss.size)[:, None] >> np.arange(miss.size)) & 1).astype(np.float64)
    num_v, num_h, den = np.zeros(miss.size), np.zeros(H), 0.0
    for h in hs:
        full = np.repeat(row[None], len(vs), axis=0)
        full[:, miss] = vs
        e = full @ W @ h + h @ c + (-0.5 * ((full - b) ** 2).sum(axis=1) if gauss else full @ b)
        w = np.exp(e - 40.0)
        den += w.sum()
        num_v += w @ vs
        num_h += w.sum() * h
    np.testing.assert_allclose(ev[miss], num_v / den, rtol=0, atol=1e-8)
    np.testing.assert_allclose(eh, num_h / den, rtol=0, atol=1e-8)
    np.testing.assert_array_equal(ev[held], row[held])


@pytest.mark.parametrize("gauss", [False, True])
def test_full_mask_is_one_propup(gauss):
    V, H, B = 24, 12, 10
    W, c, b, _ = A.case_params(V, H, 0.5, gauss, dtype=np.float64)
    rs = np.random.RandomState(0)
    obs, v0 = rs.uniform(size=(B, V)), rs.uniform(size=(B, V))
    r = Cn.clamp_twin(W, c, b, gauss, v0, obs, np.ones((1, V)), 5, 3, 1, 0, 0)         # (two accumulated steps: x + x and / 2 are exact)
    want = Cn.sigmoid(obs @ W + c)
    for k in ("v", "v_mean", "v_avg"):
        np.testing.assert_array_equal(r[k], obs)
    np.testing.assert_array_equal(r["h_mean"], want)
    np.testing.assert_array_equal(r["h_avg"], want)
    assert (r["trace_v"] == obs[None]).all()


def test_float32_twin_follows_the_float64_one():
    """The float32 restatement along the float64 twin's samples: no flip away from a tie, the same averages up to float32."""
    V, H, B, n, burn = 40, 14, 32, 8, 2
    W, c, b, _ = A.case_params(V, H, 0.2, True)
    rs = np.random.RandomState(2)
    v0, obs, mask = rs.normal(size=(B, V)).astype(np.float32), rs.normal(size=(B, V)).astype(np.float32), Cn.half_mask(V, rows=B)
    r64 = Cn.clamp_twin(W, c, b, True, v0, obs, mask, n, burn, 5, 3, 11, add_noise=True)
    forced = (r64["trace_h"].astype(np.float32), r64["trace_v"].astype(np.float32))
    f64 = Cn.clamp_twin(W, c, b, True, v0, obs, mask, n, burn, 5, 3, 11, add_noise=True, forced=forced)
    f32 = Cn.clamp_twin(W, c, b, True, v0, obs, mask, n, burn, 5, 3, 11, add_noise=True, forced=forced, dtype=np.float32)
    assert f64["flips_outside_mask"] == 0 and f32["flips_outside_mask"] == 0 and f64["max_v_diff"] <= 1e-6
    for k in ("v_avg", "h_avg", "h_mean", "v_mean"):
        assert np.abs(f32[k] - f64[k]).max() <= 1e-5, k


def test_near_tie_share_of_the_parity_inputs():
    """The GPU parity cases mask draws with |u - p| < 4e-6; on exactly those inputs the twin's own draws inside the mask are at
    most 1e-3 of all draws (for uniform u the expected share is 8e-6)."""
    from test_gpu_clamp import PARITY, _params, _inputs, SEED, STREAM, STEP, TIE_SHARE
    for V, H, gauss, noise, s, _ in PARITY:
        W, c, b = _params(V, H, s)
        for B in (64, 22):
            for per_row in (True, False):
                v0, obs, mask = _inputs(V, gauss, B, per_row)
                r = Cn.clamp_twin(W, c, b, gauss, v0, obs, mask, 8, 2, SEED, STREAM, STEP, add_noise=noise is True, sampler=noise == "gibbs")
                assert r["n_draws"] > 0 and r["n_ties"] <= TIE_SHARE * r["n_draws"], (V, H, r["n_ties"], r["n_draws"])
