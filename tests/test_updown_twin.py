"""The float64 twin of up-down fine-tuning (tests/_updown_np.py) against first principles: its delta-rule statistics are the
autograd gradients of the directed log-likelihoods, and the stacked operands of the issue's composition reproduce them through
the oracle's CD statistics.  No GPU."""
import numpy as np
import pytest
import torch

import _updown_np as ud
from oracle import rbm_np


def _layer(seed, V, H, gauss):
    rs = np.random.RandomState(seed)
    W = rs.normal(0, 0.7, (V, H))
    G = W + rs.normal(0, 0.2, (V, H))               # untied
    b, c = rs.normal(0, 0.5, H), rs.normal(0, 0.5, V)
    x_hi = (rs.uniform(size=(9, H)) < 0.5).astype(np.float64)
    x_lo = rs.normal(0, 1, (9, V)) if gauss else (rs.uniform(size=(9, V)) < 0.4).astype(np.float64)
    return W, G, b, c, x_lo, x_hi


@pytest.mark.parametrize("gauss", [False, True])
def test_generative_statistics_are_the_gradient_of_log_p(gauss):
    W, G, b, c, x_lo, x_hi = _layer(3 + gauss, 7, 5, gauss)
    Gt = torch.tensor(G, dtype=torch.float64, requires_grad=True)
    ct = torch.tensor(c, dtype=torch.float64, requires_grad=True)
    pre = torch.tensor(x_hi) @ Gt.T + ct
    xt = torch.tensor(x_lo)
    if gauss:
        log_p = (-0.5 * (xt - pre) ** 2).sum()       # unit-variance Gaussian, up to its constant
    else:
        log_p = (xt * pre - torch.nn.functional.softplus(pre)).sum()
    log_p.backward()
    S, s_v, cost = ud.delta_gen(x_lo, x_hi, G, c, gauss)
    assert np.abs(S - Gt.grad.numpy()).max() < 1e-10
    assert np.abs(s_v - ct.grad.numpy()).max() < 1e-10
    assert abs(cost + float(log_p.detach())) < 1e-10 * max(1.0, abs(cost))      # the cost is -log p


@pytest.mark.parametrize("gauss", [False, True])
def test_recognition_statistics_are_the_gradient_of_log_q(gauss):
    W, G, b, c, y_lo, y_hi = _layer(5 + gauss, 7, 5, gauss)        # (a Gaussian bottom: the dream y_lo is real-valued)
    Wt = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    pre = torch.tensor(y_lo) @ Wt + bt
    log_q = (torch.tensor(y_hi) * pre - torch.nn.functional.softplus(pre)).sum()
    log_q.backward()
    S, s_h, r = ud.delta_rec(y_lo, y_hi, W, b)
    assert np.abs(S - Wt.grad.numpy()).max() < 1e-10
    assert np.abs(s_h - bt.grad.numpy()).max() < 1e-10
    assert np.abs(r - torch.sigmoid(pre).detach().numpy()).max() < 1e-12


@pytest.mark.parametrize("gauss", [False, True])
def test_stacked_operands_reproduce_the_rules_through_cd_statistics(gauss):
    W, G, b, c, x_lo, x_hi = _layer(7 + gauss, 6, 4, gauss)
    S, s_v, _ = ud.delta_gen(x_lo, x_hi, G, c, gauss)
    g = ud.predict(x_hi, G, c, gauss)[1]
    S2, _, s_v2 = rbm_np.cd_statistics(*ud.stacked_gen(x_lo, x_hi, g))
    assert np.abs(S - S2).max() < 1e-12 and np.abs(s_v - s_v2).max() < 1e-12
    S, s_h, r = ud.delta_rec(x_lo, x_hi, W, b)        # (with a Gaussian bottom: on a real-valued y_lo)
    S2, s_h2, s_v2 = rbm_np.cd_statistics(*ud.stacked_rec(x_lo, x_hi, r))
    assert np.abs(S - S2).max() < 1e-12 and np.abs(s_h - s_h2).max() < 1e-12
    assert np.abs(s_v2).max() == 0.0                  # [y; y]: the visible half of the statistics vanishes


def test_update_is_the_oracles_rule():
    rs = np.random.RandomState(1)
    V, H = 5, 3
    s = rbm_np.RBMState(V, H, W=rs.normal(0, 1, (V, H)), hbias=rs.normal(0, 1, H), vbias=rs.normal(0, 1, V), dtype=np.float64)
    s.W_speed, s.hbias_speed, s.vbias_speed = rs.normal(0, 1, (V, H)), rs.normal(0, 1, H), rs.normal(0, 1, V)
    S, s_h, s_v = rs.normal(0, 3, (V, H)), rs.normal(0, 3, H), rs.normal(0, 3, V)
    hp = dict(lr=0.07, momentum=0.5, weightcost=0.002, lambda_1=0.01, lambda_2=0.03, batch_size=20)
    W1, Ws1 = ud.update(s.W, s.W_speed, S, hp, 20, True)
    b1, bs1 = ud.update(s.hbias, s.hbias_speed, s_h, hp, 17, False)
    g = rbm_np.rbm_grad(s, S, s_h, s_v, 20, 17, 0.002, strict_reference=False)
    rbm_np.apply_update(s, g[0], g[1], g[2], 0.07, 0.01, 0.03, 0.5)
    for mine, ref in ((W1, s.W), (Ws1, s.W_speed), (b1, s.hbias), (bs1, s.hbias_speed)):
        assert np.abs(mine - ref).max() < 1e-14
