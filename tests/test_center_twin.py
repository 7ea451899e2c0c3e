"""The float64 twin of the centred-gradient kernels (tests/_center_np.py) against the definition (CPU): the corrected
statistics are the product of centred units, zero offsets change nothing, and a whole centred step with
batch_size != n_rows is the reference's gradient rule fed the centred means."""
import numpy as np
import pytest

import _center_np as cn
from oracle import rbm_np
from oracle.philox_np import PhiloxDraws

CASES = [(12, 7, 10, False), (12, 7, 10, True), (16, 8, 20, False), (16, 8, 20, True)]


def chain(V, H, B, gauss, k=1, seed=0):
    rs = np.random.RandomState(seed + V)
    v0 = rs.normal(size=(B, V)) if gauss else (rs.uniform(size=(B, V)) < 0.3).astype(np.float64)
    s = rbm_np.RBMState(V, H, numpy_rng=np.random.RandomState(seed + 1), gauss=gauss)
    s.hbias, s.vbias = rs.normal(scale=0.3, size=H), rs.normal(scale=0.3, size=V)
    ph, _, out = rbm_np.cd_chain(s, v0, PhiloxDraws(7, 1, seed, 0), k)
    return s, v0, ph, out[1], out[4], rs


@pytest.mark.parametrize("V,H,B,gauss", CASES)
def test_corrected_statistics_are_the_centred_product(V, H, B, gauss):
    s, v0, ph, nv, nh, rs = chain(V, H, B, gauss)
    mu, lam = rs.uniform(size=V), rs.uniform(size=H)
    S, s_h, s_v = rbm_np.cd_statistics(v0, ph, nv, nh)
    S2, sh2, sv2 = cn.center_stats(S, s_h, s_v, mu, lam, 1.0)
    assert np.abs(S2 - cn.centered_product(v0, ph, nv, nh, mu, lam)).max() < 1e-10
    # the bias sums: the centred gradient of Melchior et al. with n_rows == batch_size
    assert np.abs(sv2 - (s_v - S2 @ lam)).max() < 1e-10 and np.abs(sh2 - (s_h - S2.T @ mu)).max() < 1e-10


@pytest.mark.parametrize("V,H,B,gauss", CASES)
def test_zero_offsets_are_the_identity(V, H, B, gauss):
    s, v0, ph, nv, nh, _ = chain(V, H, B, gauss)
    S, s_h, s_v = rbm_np.cd_statistics(v0, ph, nv, nh)
    S2, sh2, sv2 = cn.center_stats(S, s_h, s_v, np.zeros(V), np.zeros(H), 0.625)
    assert np.array_equal(S2, S) and np.array_equal(sh2, s_h) and np.array_equal(sv2, s_v)


def test_offsets_slide_towards_the_batch_means():
    s, v0, ph, nv, nh, rs = chain(12, 7, 10, False)
    mu, lam = cn.center_offsets(np.zeros(12), np.zeros(7), v0, ph, 1.0)
    assert np.allclose(mu, v0.mean(0), atol=1e-15) and np.allclose(lam, ph.mean(0), atol=1e-15)
    mu0, lam0 = rs.uniform(size=12), rs.uniform(size=7)
    mu, lam = cn.center_offsets(mu0, lam0, v0, ph, 0.01)
    assert np.allclose(mu, 0.99 * mu0 + 0.01 * v0.mean(0), atol=1e-15)
    assert np.allclose(lam, 0.99 * lam0 + 0.01 * ph.mean(0), atol=1e-15)


@pytest.mark.parametrize("gauss", [False, True])
def test_a_whole_centred_step_is_the_gradient_rule_fed_the_centred_means(gauss):
    """batch_size != n_rows (a ragged last minibatch): W's gradient divides by batch_size, the bias gradients by n_rows
    (rbm.py:411-417), and the correction of the bias sums carries rho = n_rows / batch_size so that
    g_vb = <v0 - nv> - g_W lam and g_hb = <ph - nh> - g_W' mu exactly, weight cost aside."""
    V, H, n, batch_size = 16, 8, 7, 10
    s, v0, ph, nv, nh, rs = chain(V, H, n, gauss, k=2)
    s.W_speed, s.hbias_speed, s.vbias_speed = rs.normal(size=(V, H)), rs.normal(size=H), rs.normal(size=V)
    s.freeze_W0()
    mu0, lam0 = rs.uniform(size=V), rs.uniform(size=H)
    ref = s.copy()
    mu, lam = cn.centered_update(s, (mu0, lam0), v0, ph, nv, nh, 0.01, batch_size, 0.05, lambda_2=0.1 if gauss else 0.0,
                                 weightcost=0.0 if gauss else 2e-4, momentum=0.5)
    mu_r, lam_r = 0.99 * mu0 + 0.01 * v0.mean(0), 0.99 * lam0 + 0.01 * ph.mean(0)
    assert np.abs(mu - mu_r).max() < 1e-14 and np.abs(lam - lam_r).max() < 1e-14
    Sd = cn.centered_product(v0, ph, nv, nh, mu_r, lam_r)
    g_W = Sd / batch_size - (0.0 if gauss else 2e-4) * ref.W0
    g_vb = (v0 - nv).mean(0) - (Sd / batch_size) @ lam_r
    g_hb = (ph - nh).mean(0) - (Sd / batch_size).T @ mu_r
    rbm_np.apply_update(ref, g_W, g_hb, g_vb, 0.05, 0.0, 0.1 if gauss else 0.0, 0.5)
    for name in ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed"):
        assert np.abs(getattr(s, name) - getattr(ref, name)).max() < 1e-10, name
