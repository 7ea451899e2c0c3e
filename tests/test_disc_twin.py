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


# ------------------------------------------------------------------------------------------------------------------ launch geometry
def test_the_geometry_mirror_at_256_compute_units():
    """The mirror of class_geom() written out at cu = 256 -- an edit of the mirror shows up here --, and what every case of
    ``geometry_cases`` is meant to reach there: (R, rows of the last batch, trips of workgroup 0)."""
    # (B, K, ldh, training mode) -> (R, G)
    table = {(1, 3, 40, False): (1, 1), (33, 3, 40, False): (1, 33), (256, 3, 40, False): (1, 256), (257, 3, 40, False): (2, 129),
             (512, 3, 40, True): (2, 256), (514, 3, 40, False): (3, 172), (769, 3, 40, False): (4, 193), (770, 64, 516, False): (4, 193),
             (771, 3, 40, False): (4, 193), (1024, 3, 40, False): (4, 256), (4096, 3, 40, True): (4, 1024), (4097, 3, 40, True): (4, 1024),
             (4119, 3, 40, True): (4, 1024), (4119, 3, 40, False): (4, 1030), (1 << 24, 3, 40, False): (4, 1 << 22),
             (4119, 2, 64, True): (4, 1024), (4119, 3, 64, True): (4, 1024),
             (4119, 2, 11008, True): (4, 1024), (4119, 3, 11008, True): (4, 1016), (4119, 64, 1024, True): (4, 512),
             (100, 64, 1 << 24, True): (1, 1)}
    for (B, K, ldh, train), want in table.items():
        assert dn.class_geom(256, B, K, ldh, train) == want, (B, K, ldh, train)
    assert dn.geometry_cases(256) == {"cu+1": (257, (2, 1, 1)), "2cu+2": (514, (3, 1, 1)), "3cu+1": (769, (4, 1, 1)),
                                      "3cu+2": (770, (4, 2, 1)), "3cu+3": (771, (4, 3, 1)), "4cu": (1024, (4, 4, 1)),
                                      "16cu+23": (4119, (4, 3, 2))}
    assert list(dn.geometry_cases(256)) == dn.GEOMETRY_KEYS
    # the busiest workgroup of the capped launch: 1030 batches on 1024 workgroups, workgroups 0 .. 5 take the second trip
    assert dn.class_reach(256, 4119, 3, 40, True) == (4, 3, 2) and dn.class_reach(256, 4119, 3, 40, False) == (4, 3, 1)
    # other CU counts reach the same (R, tail, trips), with B the formula's or a few rows more
    for cu in (8, 64, 255, 304):
        for key, (B, want) in dn.geometry_cases(cu).items():
            f = dict((k, f) for k, f, _ in dn.GEOMETRY)[key]
            assert 0 <= B - f(cu) <= dn.CLASS_R and dn.class_reach(cu, B, 3, 40, True) == want, (cu, key)


@pytest.mark.parametrize("name,V,H,B,bounds,g,scale", dn.MANY_ROW_POSTERIOR, ids=[c[0] for c in dn.MANY_ROW_POSTERIOR])
def test_the_twin_alone_on_the_many_row_posterior_cases(name, V, H, B, bounds, g, scale):
    B = dn.rows_of(256, B)
    distinct = name.startswith("between")
    rows, W, hb, vb, lo, K = dn.posterior_inputs(V, H, B, bounds, g, scale, distinct)
    p, lp = dn.posterior(rows, W, hb, vb, lo, K), dn.logp(rows, W, hb, vb, lo, K)
    assert p.shape == (B, K) and np.isfinite(p).all() and np.isfinite(lp).all() and -lp.sum() > 0
    assert np.abs(p.sum(axis=1) - 1.0).max() <= 1e-12
    if distinct:
        assert dn.distinct_inputs(rows, lo, K) == B
    else:
        assert dn.distinct_inputs(rows, lo, K) >= min(B, 12)        # (K = 64 of V = 70 leaves 12 different inputs)


@pytest.mark.parametrize("name,V,H,B,bounds,g,scale", dn.MANY_ROW_STATS, ids=[c[0] for c in dn.MANY_ROW_STATS])
def test_the_twin_alone_on_the_many_row_statistics_cases(name, V, H, B, bounds, g, scale):
    B = dn.rows_of(256, B)
    v0, nv, ph, nh, W, hb, vb, lo, K, _ = dn.stats_inputs(V, H, B, bounds, g, scale, name.startswith("odd_small"))
    if name.startswith("saturated"):
        assert np.abs(dn.scores(v0, W, hb, vb, lo, K)[0]).max() > 200
    S, s_h, s_v, nll = dn.stats(v0, W, hb, vb, lo, K)
    assert all(np.isfinite(t).all() for t in (S, s_h, s_v)) and np.isfinite(nll)
    assert nll > 0 and np.abs(s_v).max() > 0 and np.abs(S).max() > 0
    hS, hh, hv = dn.hybrid_stats(v0, W, hb, vb, lo, K, 1.0, 0.5, nv.astype(np.float64), ph.astype(np.float64), nh.astype(np.float64))
    assert all(np.isfinite(t).all() for t in (hS, hh, hv)) and np.abs(hv).max() > 0 and np.abs(hS).max() > 0
    # the stacked operands, what the device's one product is measured on, give the same sum
    gS = dn.stacked_stats(v0, W, hb, vb, lo, K, gen=1.0, w=0.5, nv=nv.astype(np.float64), ph=ph.astype(np.float64), nh=nh.astype(np.float64))[0]
    assert np.abs(gS - hS).max() <= 1e-10 * np.abs(hS).max()
