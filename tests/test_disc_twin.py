"""The float64 twin of the classification RBM (tests/_disc_np.py) against independent witnesses, on the CPU: the posterior
against brute-force free energies, the statistics against torch.autograd, the stacked-operand form (what the device runs)
against the direct form, and the toy learning problem the device test repeats."""
import numpy as np
import pytest

import _disc_np as dn
from _softmax_np import one_hot_data

# (V, H, N, boundaries of all groups, index of the label group): the label block first, last, and between another group and
# Bernoulli columns -- every other group counts as input
CASES = [(9, 5, 7, [0, 3], 0), (20, 6, 11, [2, 5, 18, 20], 1), (30, 4, 5, [4, 8, 11, 30], 1), (70, 8, 3, [1, 3, 6, 70], 2)]


def case(V, H, N, bounds, g, scale=1.0):
    rs = np.random.RandomState(V * 7 + H)
    v = one_hot_data(rs, N, V, bounds)
    W, hb, vb = scale * rs.normal(size=(V, H)), scale * rs.normal(size=H), scale * rs.normal(size=V)
    return v, W, hb, vb, bounds[g], bounds[g + 1] - bounds[g]


@pytest.mark.parametrize("V,H,N,bounds,g", CASES)
def test_posterior_is_the_softmax_of_the_free_energies(V, H, N, bounds, g):
    v, W, hb, vb, lo, K = case(V, H, N, bounds, g)
    got, want = dn.posterior(v, W, hb, vb, lo, K), dn.brute_posterior(v, W, hb, vb, lo, K)
    assert np.abs(got - want).max() <= 1e-12
    assert np.abs(np.exp(dn.logp(v, W, hb, vb, lo, K)) - want[np.arange(N), dn.labels(v, lo, K)]).max() <= 1e-12
    junk = v.copy()
    junk[:, lo:lo + K] = 0.5                    # what the block holds is ignored
    assert np.array_equal(dn.posterior(junk, W, hb, vb, lo, K), got)


@pytest.mark.parametrize("V,H,N,bounds,g", CASES)
def test_statistics_are_the_gradient_of_the_log_posterior(V, H, N, bounds, g):
    import torch
    v, W, hb, vb, lo, K = case(V, H, N, bounds, g)
    tW, thb, tvb = (torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in (W, hb, vb))
    x = torch.tensor(v, dtype=torch.float64)
    y = torch.tensor(dn.labels(v, lo, K))
    neg_F = []
    for c in range(K):                          # -F(row with category c), every term kept
        xc = x.clone()
        xc[:, lo:lo + K] = 0.0
        xc[:, lo + c] = 1.0
        neg_F.append(xc @ tvb + torch.nn.functional.softplus(xc @ tW + thb).sum(dim=1))
    total = torch.log_softmax(torch.stack(neg_F, dim=1), dim=1)[torch.arange(N), y].sum()
    total.backward()
    S, s_h, s_v, nll = dn.stats(v, W, hb, vb, lo, K)
    assert abs(nll + float(total.detach())) <= 1e-10
    for got, want in ((S, tW.grad), (s_h, thb.grad), (s_v, tvb.grad)):
        assert np.abs(got - want.numpy()).max() <= 1e-10


@pytest.mark.parametrize("V,H,N,bounds,g", CASES)
@pytest.mark.parametrize("gen,w", [(0.0, 1.0), (1.0, 0.5), (0.25, 2.0)])
def test_stacked_operands_give_the_direct_statistics(V, H, N, bounds, g, gen, w):
    v, W, hb, vb, lo, K = case(V, H, N, bounds, g)
    rs = np.random.RandomState(3)
    nv, ph, nh = rs.uniform(size=(N, V)), rs.uniform(size=(N, H)), rs.uniform(size=(N, H))
    got = dn.stacked_stats(v, W, hb, vb, lo, K, gen=gen, w=w, nv=nv, ph=ph, nh=nh)
    if gen > 0.0:
        want = dn.hybrid_stats(v, W, hb, vb, lo, K, gen, w, nv, ph, nh)
    else:
        want = tuple(w * t for t in dn.stats(v, W, hb, vb, lo, K)[:3])
    for a, b in zip(got, want):
        assert np.abs(a - b).max() <= 1e-10 * max(1.0, np.abs(b).max())


def test_saturated_scores_stay_finite():
    v, W, hb, vb, lo, K = case(20, 6, 11, [2, 5, 18, 20], 1, scale=60.0)
    S, s_h, s_v, nll = dn.stats(v, W, hb, vb, lo, K)
    assert np.abs(dn.scores(v, W, hb, vb, lo, K)[0]).max() > 200
    assert all(np.isfinite(t).all() for t in (S, s_h, s_v, dn.posterior(v, W, hb, vb, lo, K))) and np.isfinite(nll)


def test_discriminative_steps_learn_the_toy_problem():
    """Purely discriminative steps under the project's update rule: accuracy >= 0.9 on the training batch and the NLL halved
    within 300 steps (the device test runs the same problem through RBM.training).  Seed and rate are fixed so that the twin
    meets both with room: it ends at accuracy 1.0 with the NLL below a tenth of where it began."""
    rows, lo, K, W = dn.toy_problem()
    s, nll = dn.toy_train(rows, lo, K, W)
    final = -dn.logp(rows, s.W, s.hbias, s.vbias, lo, K).mean()
    acc = dn.accuracy(rows, s, lo, K)
    print("toy: NLL %.4f -> %.4f, accuracy %.3f" % (nll[0], final, acc))
    assert acc >= 0.9 and final <= 0.5 * nll[0]
