"""The float64 twin of the sparsity-target kernels (tests/_sparsity_np.py) against the definition (CPU): what the penalty
adds to the gradients is the derivative of the penalty's linearisation, the bias-only form leaves the weights alone, the
pipeline sparsity -> centring equals the penalty taken through the centred input, and the penalty does what it is for."""
import numpy as np
import pytest

import _center_np as cn
import _sparsity_np as sn
from oracle import rbm_np
from oracle.philox_np import PhiloxDraws

CASES = [(12, 7, 10, 10, False), (12, 7, 10, 10, True), (16, 8, 7, 10, False), (16, 8, 7, 10, True)]      # V, H, n, batch_size, gauss


def chain(V, H, n, gauss, seed=0):
    rs = np.random.RandomState(seed + V)
    v0 = rs.normal(size=(n, V)) if gauss else (rs.uniform(size=(n, V)) < 0.3).astype(np.float64)
    s = rbm_np.RBMState(V, H, numpy_rng=np.random.RandomState(seed + 1), gauss=gauss)
    s.hbias, s.vbias = rs.normal(scale=0.3, size=H), rs.normal(scale=0.3, size=V)
    ph, _, out = rbm_np.cd_chain(s, v0, PhiloxDraws(7, 1, seed, 0), 1)
    return s, v0, ph, out[1], out[4], rs


def gradients(s, v0, ph, nv, nh, batch_size, q=None, v_mean=None, target=0.3, cost=0.0, weights=True):
    S, s_h, s_v = rbm_np.cd_statistics(v0, ph, nv, nh)
    if cost:
        S, s_h, s_v = sn.stats(S, s_h, s_v, q, v_mean, target, cost * batch_size if weights else 0.0, cost * v0.shape[0])
    return rbm_np.rbm_grad(s, S, s_h, s_v, batch_size, v0.shape[0], 0.0)


@pytest.mark.parametrize("V,H,n,batch_size,gauss", CASES)
def test_the_additions_are_the_gradient_of_the_linearised_penalty(V, H, n, batch_size, gauss):
    """F(W, b) = sum_j c (p - q_j) mean_r (v0_r . W_j + b_j) with q held constant: dF/dW_ij = c (p - q_j) <v_i>,
    dF/db_j = c (p - q_j).  Central differences of a function linear in (W, b) are exact to rounding."""
    s, v0, ph, nv, nh, rs = chain(V, H, n, gauss)
    p, c = 0.3, 1.7
    q, v_mean = sn.activity(rs.uniform(size=H), v0, ph, 0.1)
    assert np.abs(v_mean - v0.mean(0)).max() < 1e-15
    plain = gradients(s, v0, ph, nv, nh, batch_size)
    sparse = gradients(s, v0, ph, nv, nh, batch_size, q, v_mean, p, c)

    def F(W, b):
        return float((c * (p - q) * (v0 @ W + b).mean(axis=0)).sum())

    eps = 1e-4
    dW, db = np.zeros((V, H)), np.zeros(H)
    for i in range(V):
        for j in range(H):
            e = np.zeros((V, H))
            e[i, j] = eps
            dW[i, j] = (F(s.W + e, s.hbias) - F(s.W - e, s.hbias)) / (2 * eps)
    for j in range(H):
        e = np.zeros(H)
        e[j] = eps
        db[j] = (F(s.W, s.hbias + e) - F(s.W, s.hbias - e)) / (2 * eps)
    assert np.abs((sparse[0] - plain[0]) - dW).max() < 1e-8
    assert np.abs((sparse[1] - plain[1]) - db).max() < 1e-8
    assert np.array_equal(sparse[2], plain[2])                   # the visible biases take no part
    # the bias-only form of Lee et al.: the same hidden-bias term, the weights' gradient untouched
    bias_only = gradients(s, v0, ph, nv, nh, batch_size, q, None, p, c, weights=False)
    assert np.array_equal(bias_only[0], plain[0]) and np.array_equal(bias_only[1], sparse[1])


def test_the_estimate_starts_at_the_batch_means_then_slides():
    s, v0, ph, nv, nh, rs = chain(12, 7, 10, False)
    q, v_mean = sn.activity(np.zeros(7), None, ph, 1.0)
    assert v_mean is None and np.allclose(q, ph.mean(0), atol=1e-15)
    q0 = rs.uniform(size=7)
    q, _ = sn.activity(q0, v0, ph, 1.0 - 0.9)
    assert np.allclose(q, 0.9 * q0 + 0.1 * ph.mean(0), atol=1e-15)
    # at the target nothing is added; a zero cost is the plain step
    S, s_h, s_v = rbm_np.cd_statistics(v0, ph, nv, nh)
    S2, sh2, sv2 = sn.stats(S, s_h, s_v, np.full(7, 0.3), v0.mean(0), 0.3, 10.0, 10.0)
    assert np.array_equal(S2, S) and np.array_equal(sh2, s_h) and sv2 is not None and np.array_equal(sv2, s_v)


@pytest.mark.parametrize("V,H,n,batch_size,gauss", CASES)
def test_sparsity_then_centring_is_the_penalty_through_the_centred_input(V, H, n, batch_size, gauss):
    s, v0, ph, nv, nh, rs = chain(V, H, n, gauss)
    p, c, rho = 0.2, 2.5, float(n) / batch_size
    mu, lam, q = rs.uniform(size=V), rs.uniform(size=H), rs.uniform(size=H)
    m_v, t = v0.mean(0), p - q
    S, s_h, s_v = rbm_np.cd_statistics(v0, ph, nv, nh)
    S1, sh1, sv1 = sn.stats(S, s_h, s_v, q, m_v, p, c * batch_size, c * n)
    S2, sh2, sv2 = cn.center_stats(S1, sh1, sv1, mu, lam, rho)
    direct = cn.centered_product(v0, ph, nv, nh, mu, lam) + c * batch_size * np.outer(m_v - rho * mu, t)
    assert np.abs(S2 - direct).max() < 1e-10
    # the bias sums pick up center_stats' reparameterisation terms of the corrected S as it stands
    assert np.abs(sh2 - (s_h + c * n * t - rho * (direct.T @ mu))).max() < 1e-10
    assert np.abs(sv2 - (s_v - rho * (direct @ lam))).max() < 1e-10


@pytest.mark.parametrize("case,sparsity,target,measured", sn.BEHAVIOUR_RUNS,
                         ids=["%s-%s" % (r[0], "plain" if not r[1] else "cost%g%s" % (r[1]["cost"], "" if r[1].get("weights", True) else "-bias-only"))
                              for r in sn.BEHAVIOUR_RUNS])
def test_the_penalty_moves_the_activities_to_the_target(case, sparsity, target, measured):
    """Measured on the float64 oracle with exactly these inputs (tests/_sparsity_np.py: 100 -> 24, 200 rows, B = 20,
    momentum 0.5 then 0.9 from step 100), per-unit mean activation over all rows after the run:

      Bernoulli (30 % ones, lr 0.1, weight cost 2e-4, 400 steps)
        plain CD                               0.008 .. 0.123    nearest unit 0.1775 from the target 0.3
        target 0.3, cost 1, decay 0.9          0.257 .. 0.316    farthest unit 0.0432 from it
        target 0.3, cost 3, bias only          0.043 .. 0.306    farthest unit 0.2568
        (target 0.3, cost 3 with weights       0.080 .. 0.341    farthest 0.2200: too strong for this lr, not asserted)
      Gaussian (N(0, 1) rows, lr 0.005, lambda_2 0.1, 600 steps)
        plain CD                               0.453 .. 0.532    nearest unit 0.2525 from the target 0.2
        target 0.2, cost 5, decay 0.9          0.209 .. 0.222    farthest unit 0.0224

    A sparse run must end within twice its figure, a plain run at least half its figure away."""
    act = sn.behaviour_on_the_oracle(case, **sparsity)
    figure, ok = sn.behaviour_holds(act, sparsity, target, measured)
    print("%s %r: activations %.4f .. %.4f, figure %.4f (measured %.4f)" % (case, sparsity, act.min(), act.max(), figure, measured))
    assert ok
