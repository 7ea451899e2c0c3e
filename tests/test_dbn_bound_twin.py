"""The definitions of the variational lower bound (tests/_dbn_bound_np.py, the float64 twin of mdbn_amd/bound.py) against
ground truth by enumeration; no GPU.  The device draws the uniforms the twin draws here (tests/test_gpu_dbn_bound.py)."""
import numpy as np
import pytest

import _dbn_bound_np as T

SCALES = (0.5, 1.5)
NAMES = ("bernoulli_8_6_4", "gauss_8_6_4", "deep_7_5_4_3", "forest")
S = 64


@pytest.fixture(scope="module")
def truth():
    """{(name, scale): (model, inputs, exact log p, exact bound, exact log Z)}, computed once."""
    out = {}
    for scale in SCALES:
        for name, (model, inputs) in T.stacks(scale).items():
            out[name, scale] = (model, inputs) + T.brute_force(model, inputs)
    return out


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", NAMES)
def test_exact_bound_is_below_exact_log_p(truth, name, scale):
    _, _, log_p, bound, _ = truth[name, scale]
    assert np.isfinite(log_p).all() and np.isfinite(bound).all()
    assert (bound <= log_p + 1e-12).all(), (bound - log_p).max()
    assert (log_p - bound).max() > 1e-3, "an untied stack whose bound is tight everywhere tests nothing"


@pytest.mark.parametrize("scale", SCALES)
def test_tied_transpose_stack_is_tight(truth, scale):
    """W_2 = W_1^T, b_2 = c_1, c_2 = b_1: q is the first RBM's exact posterior and B = log p_RBM1(x_0)."""
    model, inputs = truth["bernoulli_8_6_4", scale][:2]
    tied = T.tied(model)
    log_p, bound, _ = T.brute_force(tied, inputs)
    first = T.f64(tied["bottoms"][0][0])
    rbm1 = -T.free_energy(inputs[0], first) - T.exact_log_z(first)
    assert np.abs(bound - log_p).max() <= 1e-12
    assert np.abs(bound - rbm1).max() <= 1e-12


@pytest.mark.parametrize("gauss", (False, True))
def test_one_layer_is_the_rbm_log_likelihood(gauss):
    rs = np.random.RandomState(5)
    model = dict(bottoms=[T.make_net(rs, (8, 4), gauss, 1.0, 77)], joint=None)
    x = T.make_data(rs, 5, 8, gauss)
    log_p, bound, log_z = T.brute_force(model, [x])
    want = -T.free_energy(x, T.f64(model["bottoms"][0][0])) - log_z
    assert np.abs(bound - want).max() <= 1e-12 and np.abs(log_p - want).max() <= 1e-12
    est = T.estimate(model, [x], S, log_z)
    assert est["values"].shape == (5, 1) and est["stderr"] == 0.0 and not est["uniforms"][0]
    assert np.abs(est["rows"] - want).max() <= 1e-12


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", NAMES)
def test_sampled_estimate_meets_the_exact_bound(truth, name, scale):
    """|estimate - exact| <= 4 standard errors of the estimate (the factor of the AIS tests), with the exact log Z."""
    model, inputs, _, bound, log_z = truth[name, scale]
    est = T.estimate(model, inputs, S, log_z)
    assert est["stderr"] > 0
    assert abs(est["bound"] - bound.mean()) <= 4 * est["stderr"], (est["bound"], bound.mean(), est["stderr"])
    assert np.abs(est["modality_rows"].sum(axis=0) + est["joint_rows"] - est["rows"]).max() <= 1e-9
    # the device compares the same uniforms with float32 means: at most 0.1 % of the draws may lie within the tie mask
    assert T.tie_fraction(est) <= 1e-3


def test_teacher_forced_estimate_reproduces_the_free_run():
    model, inputs = T.stacks(0.5)["forest"]
    free = T.estimate(model, inputs, 8, 0.25)
    forced = T.estimate(model, inputs, 8, 0.25, samples=free["samples"])
    assert np.array_equal(free["rows"], forced["rows"]) and np.array_equal(free["values"], forced["values"])
