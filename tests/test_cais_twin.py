"""The float64 numpy twin of the device's clamped annealed importance sampling (tests/_cais_np.py) against exact conditional
partition functions (no GPU): the reference restatement the GPU tests compare with must itself sit inside the bounds they
use, and its two limits -- no held column, every column held -- must be what include/mdbn_hip.h says they are."""
import numpy as np
import pytest

import _ais_np as A
import _cais_np as CA

N_ROWS, CHAINS, K = 8, 256, 1000


@pytest.mark.parametrize("V,H,s,gauss", A.CASES)
def test_twin_against_brute_force(V, H, s, gauss):
    """8 rows with per-row block masks over half the columns, C = 256, K = 1000, uniform schedule, Philox seed 1: every row
    |log Z_r^ - log Z_r| <= 4 std_err and <= 0.05 nats."""
    W, c, b, bA = A.case_params(V, H, s, gauss)
    obs, mask = CA.observed(N_ROWS, V, gauss), CA.block_masks(N_ROWS, V)
    r = CA.cais_twin(W, c, b, bA, gauss, np.linspace(0, 1, K + 1), obs, mask, CHAINS, 1, 0, 0)
    log_Z, err = CA.estimate_rows(r["logw"], bA, mask, H, gauss)
    assert (r["trace_v"][-1][np.repeat(mask != 0, CHAINS, axis=0)] == np.repeat(obs, CHAINS, axis=0)[np.repeat(mask != 0, CHAINS, axis=0)]).all()
    for row in range(N_ROWS):
        exact = CA.exact_cond_log_Z(W, c, b, obs[row], mask[row], gauss)
        print("twin %d->%d %s row %d: log Z^ %.5f exact %.5f |err| %.5f std_err %.5f (%.2f std_err)"
              % (V, H, "GRBM" if gauss else "RBM", row, log_Z[row], exact, abs(log_Z[row] - exact), err[row], abs(log_Z[row] - exact) / err[row]))
        assert abs(log_Z[row] - exact) <= 4 * err[row], (row, log_Z[row], exact, err[row])
        assert abs(log_Z[row] - exact) <= 0.05, (row, log_Z[row], exact)


@pytest.mark.parametrize("V,H,s,gauss", A.CASES)
def test_every_column_held_is_the_closed_form(V, H, s, gauss):
    """A row with no free column: nothing is random, the increments telescope to sum_j softplus(a_j(obs)) - H log 2 (to
    1e-9), every chain alike; log Z_r is then sum_j softplus(a_j(obs)), the exact one, with no standard error.  The other row
    of the run keeps a mask of its own."""
    W, c, b, bA = A.case_params(V, H, s, gauss, dtype=np.float64)
    obs = CA.observed(2, V, gauss, seed=1)
    mask = np.stack([np.ones(V, dtype=np.float32), CA.block_masks(1, V, seed=1)[0]])
    r = CA.cais_twin(W, c, b, bA, gauss, np.linspace(0, 1, 41), obs, mask, 6, 1, 0, 0)
    want = np.logaddexp(0.0, obs[0].astype(np.float64) @ W + c).sum()
    np.testing.assert_allclose(r["logw"][0], want - H * np.log(2.0), rtol=0, atol=1e-9)
    assert (r["trace_v"][:, :6] == obs[0]).all()
    log_Z, err = CA.estimate_rows(r["logw"], bA, mask, H, gauss)
    assert abs(log_Z[0] - want) <= 1e-9 and err[0] <= 1e-12
    assert abs(CA.exact_cond_log_Z(W, c, b, obs[0], mask[0], gauss) - want) <= 1e-9
    assert err[1] > 0 and r["n_draws"] > 0


@pytest.mark.parametrize("C", [4, 3])
@pytest.mark.parametrize("V,H,s,gauss", A.CASES)
def test_no_held_column_is_the_unclamped_twin(V, H, s, gauss, C):
    """A zero mask: the float64 log weights, and the samples, of ais_twin with M = N C chains, exactly."""
    W, c, b, bA = A.case_params(V, H, s, gauss)
    bA = bA + np.float32(0.1)
    N, betas = 5, np.linspace(0, 1, 21)
    for mask in (np.zeros((1, V), dtype=np.float32), np.zeros((N, V), dtype=np.float32)):
        r = CA.cais_twin(W, c, b, bA, gauss, betas, CA.observed(N, V, gauss), mask, C, 5, 3, 11)
        want = A.ais_twin(W, c, b, bA, gauss, betas, N * C, 5, 3, 11)
        np.testing.assert_array_equal(r["logw"].reshape(-1), want["logw"])
        np.testing.assert_array_equal(r["trace_h"], want["trace_h"])
        np.testing.assert_array_equal(r["trace_v"], want["trace_v"])
        assert r["n_draws"] == want["n_draws"] and r["n_ties"] == want["n_ties"]


def test_float32_twin_follows_the_float64_one():
    """The float32 restatement (the device's regrouping: masked s1, d2 per mask row) along the float64 twin's samples: the same
    log w up to float32, no flip, and ties counted over the free columns only."""
    V, H, gauss, N, C = 40, 14, True, 7, 3
    W, c, b, bA = A.case_params(V, H, 0.2, gauss)
    bA = bA + np.float32(0.2)
    betas = np.linspace(0, 1, 9)
    obs, mask = CA.observed(N, V, gauss), CA.block_masks(N, V)
    r64 = CA.cais_twin(W, c, b, bA, gauss, betas, obs, mask, C, 5, 3, 11)
    forced = (r64["trace_h"].astype(np.float32), r64["trace_v"].astype(np.float32))
    f64 = CA.cais_twin(W, c, b, bA, gauss, betas, obs, mask, C, 5, 3, 11, forced=forced)
    f32 = CA.cais_twin(W, c, b, bA, gauss, betas, obs, mask, C, 5, 3, 11, dtype=np.float32, forced=forced)
    assert f64["flips_outside_mask"] == 0 and f32["flips_outside_mask"] == 0
    assert f64["n_draws"] == (len(betas) - 2) * N * C * H           # Gaussian visibles: only the hidden draws are Bernoulli
    assert np.abs(f32["logw"] - f64["logw"]).max() <= 1e-3
    assert np.abs(f32["logw"] - r64["logw"]).max() <= 1e-3


def test_host_finish_per_row():
    """estimate_rows: equal weights give log Z_A,r + log w exactly with the base model over the row's free columns."""
    bA = np.array([0.3, -1.0, 2.0])
    mask = np.array([[0, 0, 0], [1, 0, 1], [1, 1, 1]], dtype=np.float32)
    logw = np.array([[250.0] * 4, [700.0, 700.0 + np.log(3.0)] * 2, [5.0] * 4])
    lz, err = CA.estimate_rows(logw, bA, mask, 5, False)
    sp = np.logaddexp(0, bA)
    np.testing.assert_allclose(lz, [250.0 + 5 * np.log(2) + sp.sum(), 700.0 + np.log(2.0) + 5 * np.log(2) + sp[1], 5.0 + 5 * np.log(2)], rtol=0, atol=1e-12)
    np.testing.assert_allclose(err, [0.0, 0.5 / np.sqrt(4), 0.0], rtol=0, atol=1e-12)
    lz, _ = CA.estimate_rows(logw, bA, mask, 5, True)
    np.testing.assert_allclose(lz, np.array([250.0, 700.0 + np.log(2.0), 5.0]) + 5 * np.log(2) + 0.5 * np.log(2 * np.pi) * np.array([3, 1, 0]),
                               rtol=0, atol=1e-12)
