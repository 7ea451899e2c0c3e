"""The float64 twin of up-down fine-tuning with categorical visible units (tests/_gupdown_np.py) against first principles: its
grouped generative statistics are the autograd gradient of sum_r log p(x_0 | x_1), its cost is minus the directed term of the
bound's twin, the stacked operands reproduce it through the oracle's CD statistics, and a layer without a table is the
Bernoulli twin's.  No GPU."""
import numpy as np
import torch

import _gbound_np as gb
import _gupdown_np as gud
import _softmax_np as sm
import _updown_np as ud
from oracle import rbm_np

BOUNDS, V, H, N = [0, 3, 6, 8], 10, 4, 7           # groups (3, 3, 2) and two Bernoulli columns


def mixed_layer(seed=5):
    rs = np.random.RandomState(seed)
    G, c = rs.normal(0, 1, (V, H)), rs.normal(0, 1, V)
    x_hi = (rs.uniform(size=(N, H)) < 0.5).astype(np.float64)
    x_lo = sm.one_hot_data(rs, N, V, BOUNDS, p=0.5).astype(np.float64)
    return G, c, x_lo, x_hi


def torch_log_p(x_lo, x_hi, G, c, bounds):
    pre = x_hi @ G.T + c
    cols = torch.from_numpy(sm.bernoulli_columns(bounds, pre.shape[1]))
    total = (x_lo[:, cols] * pre[:, cols] - torch.nn.functional.softplus(pre[:, cols])).sum()
    for lo, hi in sm.spans(bounds):
        total = total + (x_lo[:, lo:hi] * torch.log_softmax(pre[:, lo:hi], dim=1)).sum()
    return total


def test_delta_gen_is_the_autograd_gradient_of_the_log_likelihood():
    G, c, x_lo, x_hi = mixed_layer()
    S, s_v, cost = gud.delta_gen(x_lo, x_hi, G, c, BOUNDS)
    tG, tc = torch.tensor(G, requires_grad=True), torch.tensor(c, requires_grad=True)
    ll = torch_log_p(torch.from_numpy(x_lo), torch.from_numpy(x_hi), tG, tc, BOUNDS)
    ll.backward()
    assert np.abs(S - tG.grad.numpy()).max() < 1e-10
    assert np.abs(s_v - tc.grad.numpy()).max() < 1e-10
    assert abs(cost + float(ll.detach())) < 1e-10
    # the grouped means are a distribution inside every group
    g = gud.predict(x_hi, G, c, BOUNDS)[1]
    for lo, hi in sm.spans(BOUNDS):
        assert np.abs(g[:, lo:hi].sum(axis=1) - 1.0).max() < 1e-14
        assert np.abs(s_v[lo:hi].sum()) < 1e-12                  # ... so a group's bias statistics cancel on one-hot rows


def test_the_cost_is_minus_the_directed_term_of_the_bound():
    G, c, x_lo, x_hi = mixed_layer(6)
    want = -gb.row_loglik_grouped(x_hi, dict(W=G, c=c, gauss=False), x_lo, BOUNDS).sum()
    assert abs(gud.delta_gen(x_lo, x_hi, G, c, BOUNDS)[2] - want) < 1e-12 * max(1.0, abs(want))
    assert abs(sm.grouped_cost(x_hi @ G.T + c, x_lo, BOUNDS) - want) < 1e-12 * max(1.0, abs(want))      # the CD step's cost
    # finite where a probability underflows: pre-activations alternating +-80 inside a 64-column group
    Gs = np.zeros((66, 1))
    cs = np.concatenate([[0.5], 80.0 * (-1.0) ** np.arange(64), [-0.25]])
    x = np.zeros((2, 66))
    x[0, 1 + 1] = x[1, 1 + 2] = 1.0                                # a category at -80, one at +80
    got = gud.cost(np.zeros((2, 1)) @ Gs.T + cs, x, [1, 65])
    want = (80.0 + np.log(32.0) + 80.0) + np.log(32.0) + 2 * (ud.softplus(0.5) + ud.softplus(-0.25))
    assert np.isfinite(got) and abs(got - want) < 1e-9


def test_stacked_operands_reproduce_the_statistics_through_the_cd_statistics():
    G, c, x_lo, x_hi = mixed_layer(7)
    S, s_v, _ = gud.delta_gen(x_lo, x_hi, G, c, BOUNDS)
    g = gud.predict(x_hi, G, c, BOUNDS)[1]
    S2, s_h2, s_v2 = rbm_np.cd_statistics(*ud.stacked_gen(x_lo, x_hi, g))
    assert np.abs(S2 - S).max() < 1e-12 and np.abs(s_v2 - s_v).max() < 1e-12
    assert np.abs(s_h2).max() == 0.0                               # P2 = [x_hi; -x_hi]: the hidden half has nothing to learn


def test_gen_step_applies_the_update_rule_and_a_layer_without_a_table_is_the_bernoulli_twin():
    G, c, x_lo, x_hi = mixed_layer(8)
    hp = dict(lr=0.05, momentum=0.5, weightcost=0.001, lambda_1=0.002, lambda_2=0.01, batch_size=10)
    rs = np.random.RandomState(2)
    base = dict(W=G, G=G, c=c, b=np.zeros(H), Gs=rs.normal(size=G.shape), cs=rs.normal(size=V), gauss=False)
    l = ud.untie(dict(base, bounds=BOUNDS))
    S, s_v, cost = gud.delta_gen(x_lo, x_hi, G, c, BOUNDS)
    want_G = ud.update(l["G"], l["Gs"], S, hp, 10, True)
    want_c = ud.update(l["c"], l["cs"], s_v, hp, N, False)
    b0 = l["b"].copy()
    assert gud.gen_step(l, x_lo, x_hi, hp, N) == cost
    assert np.array_equal(l["G"], want_G[0]) and np.array_equal(l["Gs"], want_G[1])
    assert np.array_equal(l["c"], want_c[0]) and np.array_equal(l["cs"], want_c[1])
    assert np.array_equal(l["b"], b0) and np.array_equal(l["W"], G)          # the recognition half does not move
    plain, mine = ud.untie(base), ud.untie(base)
    assert gud.gen_step(mine, x_lo, x_hi, hp, N) == ud.gen_step(plain, x_lo, x_hi, hp, N)
    assert all(np.array_equal(mine[k], plain[k]) for k in ("G", "Gs", "c", "cs"))


def test_one_hot_states_enumerate_the_layer_and_exact_log_p_is_a_distribution():
    states = gud.one_hot_states(7, [1, 3, 6])                      # a Bernoulli column, groups of 2 and 3, a Bernoulli column
    assert states.shape == (2 * 2 * 3 * 2, 7) and len({tuple(s) for s in states}) == 24
    assert (states[:, 1:3].sum(axis=1) == 1).all() and (states[:, 3:6].sum(axis=1) == 1).all()
    rs = np.random.RandomState(4)
    net = [ud.untie(dict(W=rs.normal(size=(a, b)), b=rs.normal(size=b), c=rs.normal(size=a), gauss=False))
           for a, b in ((7, 4), (4, 3), (3, 2))]
    net[0]["bounds"] = [1, 3, 6]
    assert abs(np.logaddexp.reduce(gud.exact_log_p(net, states))) < 1e-12
