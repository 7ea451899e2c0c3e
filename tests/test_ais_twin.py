"""The float64 numpy twin of the device's annealed importance sampling (tests/_ais_np.py) against exact partition functions
(no GPU): the reference restatement the GPU tests compare with must itself sit inside the bounds they use."""
import numpy as np
import pytest

import _ais_np as A


@pytest.mark.parametrize("V,H,s,gauss", A.CASES)
def test_twin_against_brute_force(V, H, s, gauss):
    """M = 512, K = 1000, uniform schedule, Philox seed 1: |log Z^ - log Z| <= 4 std_err and <= 0.05 nats."""
    W, c, b, bA = A.case_params(V, H, s, gauss)
    exact = A.brute_log_Z(W, c, b, gauss)
    r = A.ais_twin(W, c, b, bA, gauss, np.linspace(0, 1, 1001), 512, 1, 0, 0)
    log_Z, err = A.estimate(r["logw"], bA, H, gauss)
    print("twin %d->%d %s: log Z^ %.5f exact %.5f |err| %.5f std_err %.5f" % (V, H, "GRBM" if gauss else "RBM", log_Z, exact, abs(log_Z - exact), err))
    assert abs(log_Z - exact) <= 4 * err, (log_Z, exact, err)
    assert abs(log_Z - exact) <= 0.05, (log_Z, exact)


@pytest.mark.parametrize("gauss", [False, True])
def test_one_temperature_is_plain_importance_sampling(gauss):
    """K = 1: v ~ p_0, log w = log p*_1(v) - log p*_0(v), written out directly."""
    from oracle import philox_np
    V, H, M = 20, 10, 64
    W, c, b, bA = A.case_params(V, H, 0.25, gauss, dtype=np.float64)
    bA = bA + 0.1
    r = A.ais_twin(W, c, b, bA, gauss, [0.0, 1.0], M, 3, 2, 5)
    u = philox_np.uniform(M, V, 3, 2, 5, 0).astype(np.float64)
    if gauss:
        u2 = philox_np.uniform(M, V, 3, 2, 5, philox_np.NORMAL_BIT).astype(np.float64)
        v = bA + np.sqrt(-2 * np.log(u)) * np.cos(2 * np.pi * u2)
        want = np.logaddexp(0, v @ W + c).sum(1) - 0.5 * ((v - b) ** 2).sum(1) - (H * np.log(2) - 0.5 * ((v - bA) ** 2).sum(1))
    else:
        v = (u < 1 / (1 + np.exp(-bA))).astype(np.float64)
        want = np.logaddexp(0, v @ W + c).sum(1) + v @ b - (H * np.log(2) + v @ bA)
    np.testing.assert_array_equal(r["trace_v"][0], v)
    np.testing.assert_allclose(r["logw"], want, rtol=0, atol=1e-10)


@pytest.mark.parametrize("gauss", [False, True])
def test_no_coupling_is_exact(gauss):
    """W = 0, b_A = b: every chain has log w = sum softplus(c) - H log 2, hence the exact log Z with zero standard error."""
    V, H = 24, 12
    _, c, b, _ = A.case_params(V, H, 0.5, gauss, dtype=np.float64)
    W = np.zeros((V, H))
    r = A.ais_twin(W, c, b, b, gauss, np.linspace(0, 1, 41), 32, 1, 0, 0)
    np.testing.assert_allclose(r["logw"], np.logaddexp(0, c).sum() - H * np.log(2), rtol=0, atol=1e-9)
    log_Z, err = A.estimate(r["logw"], b, H, gauss)
    assert abs(log_Z - A.brute_log_Z(W, c, b, gauss)) <= 1e-9 and err <= 1e-9


def test_float32_twin_follows_the_float64_one():
    """The float32 restatement (the device's regrouping) along the float64 twin's samples: the same log w up to float32."""
    V, H, gauss = 40, 14, True
    W, c, b, bA = A.case_params(V, H, 0.2, gauss)
    bA = bA + np.float32(0.2)
    betas = np.linspace(0, 1, 9)
    r64 = A.ais_twin(W, c, b, bA, gauss, betas, 64, 5, 3, 11)
    forced = (r64["trace_h"].astype(np.float32), r64["trace_v"].astype(np.float32))
    f64 = A.ais_twin(W, c, b, bA, gauss, betas, 64, 5, 3, 11, forced=forced)
    f32 = A.ais_twin(W, c, b, bA, gauss, betas, 64, 5, 3, 11, dtype=np.float32, forced=forced)
    assert f64["flips_outside_mask"] == 0 and f32["flips_outside_mask"] == 0
    assert np.abs(f32["logw"] - f64["logw"]).max() <= 1e-3


@pytest.mark.parametrize("V,H,gauss,s", [(100, 24, False, 0.3), (400, 40, True, 0.05), (1024, 256, True, 0.02)])
def test_near_tie_share_of_the_parity_inputs(V, H, gauss, s):
    """The GPU parity cases mask draws with |u - p| < 4e-6; on exactly those inputs the twin's own draws inside the mask are
    at most 1e-3 of all draws (for uniform u the expected share is 8e-6)."""
    from test_gpu_ais import _params, SEED, STREAM, STEP, TIE_SHARE
    W, c, b, bA = _params(V, H, gauss, s)
    for M in (64, 22):
        r = A.ais_twin(W, c, b, bA, gauss, np.linspace(0, 1, 9), M, SEED, STREAM, STEP)
        assert r["n_draws"] > 0 and r["n_ties"] <= TIE_SHARE * r["n_draws"], (r["n_ties"], r["n_draws"])
