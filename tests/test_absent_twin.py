"""The float64 twin of the absent visible units (tests/_absent_np.py) against first principles: its free energy against the
enumeration of the hidden states, its statistics against torch.autograd's gradient of sum_rows log p_{O_r}(v_{r, O_r}) with
exact per-pattern model expectations, its step against the existing oracle's when nothing is missing, and the tie counts
of the kernel cases the GPU test shares."""
import itertools

import numpy as np
import pytest
import torch

import _absent_np as an
from _oracle_engine import OracleEngine
from mdbn_amd.engine import RngAddr
from oracle import rbm_np
from oracle.philox_np import PhiloxDraws


def tiny(gauss, seed=3):
    V, H = (4, 3) if gauss else (5, 3)
    rs = np.random.RandomState(seed)
    s = rbm_np.RBMState(V, H, W=rs.normal(scale=0.7, size=(V, H)), hbias=rs.normal(scale=0.5, size=H),
                        vbias=rs.normal(scale=0.5, size=V), dtype=np.float64, gauss=gauss)
    x = rs.normal(size=(6, V)) if gauss else (rs.uniform(size=(6, V)) < 0.5).astype(np.float64)
    mask = rs.uniform(size=(6, V)) < 0.6
    mask[0, :] = False              # a wholly-absent row
    mask[1, :] = True               # a wholly-observed row
    mask[2, :] = [True] + [False] * (V - 1)
    x[~mask] = np.nan
    return s, x


@pytest.mark.parametrize("gauss", [False, True], ids=["bernoulli", "gauss"])
def test_free_energy_is_minus_log_sum_over_hidden_states(gauss):
    s, x = tiny(gauss)
    assert np.abs(an.free_energy_absent(s, x) - an.brute_free_energy(s, x)).max() < 1e-12


def _torch_log_p(W, c, b, v, mask, gauss):
    """log p_O(v_O) of one row in torch float64: -F_O(v) - log Z_O, both by enumeration of the hidden states."""
    H = W.shape[1]
    m = torch.from_numpy(mask.astype(np.float64))
    hs = torch.tensor(list(itertools.product((0.0, 1.0), repeat=H)), dtype=torch.float64)        # [2^H, H]
    a = hs @ W.t()                                                                              # [2^H, V]
    vt = torch.from_numpy(np.where(mask, v, 0.0))
    if gauss:
        neg_E = -0.5 * (m * (vt - b) ** 2).sum() + a @ (m * vt) + hs @ c
        log_Z = torch.logsumexp(hs @ c + (m * (0.5 * np.log(2.0 * np.pi) + b * a + 0.5 * a * a)).sum(dim=1), dim=0)
    else:
        neg_E = (m * vt) @ b + a @ (m * vt) + hs @ c
        log_Z = torch.logsumexp(hs @ c + (m * torch.nn.functional.softplus(b + a)).sum(dim=1), dim=0)
    return torch.logsumexp(neg_E, dim=0) - log_Z


@pytest.mark.parametrize("gauss", [False, True], ids=["bernoulli", "gauss"])
def test_positive_statistics_minus_exact_expectations_are_the_gradient(gauss):
    s, x = tiny(gauss)
    W = torch.tensor(s.W, dtype=torch.float64, requires_grad=True)
    c = torch.tensor(s.hbias, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(s.vbias, dtype=torch.float64, requires_grad=True)
    mask = ~np.isnan(x)
    total = sum(_torch_log_p(W, c, b, x[r], mask[r], gauss) for r in range(x.shape[0]))
    total.backward()
    v0, m2, ph, _, _ = an.cd_chain(s, x, PhiloxDraws(5, 1, 0), 1)
    assert (m2 == mask).all()
    S, s_h, s_v = v0.T @ ph, ph.sum(axis=0), v0.sum(axis=0)
    for r in range(x.shape[0]):
        Evh, Eh, Ev = an.model_expectations(s, mask[r])
        S, s_h, s_v = S - Evh, s_h - Eh, s_v - Ev
    assert np.abs(S - W.grad.numpy()).max() < 1e-10
    assert np.abs(s_h - c.grad.numpy()).max() < 1e-10
    assert np.abs(s_v - b.grad.numpy()).max() < 1e-10


def test_a_row_that_observes_nothing_contributes_nothing():
    s, x = tiny(False)
    S, s_h, s_v, cost, (v0, mask, ph, nv, nh, _) = an.cd_step_absent(s, x, PhiloxDraws(5, 1, 0), 2)
    assert not mask[0].any() and (ph[0] == nh[0]).all() and (v0[0] == 0).all() and (nv[0] == 0).all()
    S1, h1, v1, cost1, _ = an.cd_step_absent(s, x[1:], PhiloxDraws(5, 1, 0, row_offset=1), 2)
    assert np.abs(S - S1).max() < 1e-13 and np.abs(s_h - h1).max() < 1e-13 and np.abs(s_v - v1).max() < 1e-13
    assert abs(cost - cost1) < 1e-12


@pytest.mark.parametrize("gauss", [False, True], ids=["bernoulli", "gauss"])
def test_with_nothing_missing_the_step_is_the_oracle_cd_step(gauss):
    rs = np.random.RandomState(11)
    V, H, B = 9, 6, 7
    W = torch.from_numpy(rs.normal(scale=0.3, size=(V, H)))
    hb, vb = torch.from_numpy(rs.normal(scale=0.2, size=H)), torch.from_numpy(rs.normal(scale=0.2, size=V))
    x = rs.normal(size=(B, V)) if gauss else (rs.uniform(size=(B, V)) < 0.4).astype(np.float64)
    rng = RngAddr(77, 2, 5, 0, 3)
    want, _ = OracleEngine().cd_step(x, None, W, hb, vb, gauss, 2, rng)
    got, _ = an.AbsentOracle().cd_step_absent(x, None, W, hb, vb, gauss, 2, rng)
    assert np.abs(want.numpy() - got.numpy()).max() < 1e-12


def test_split_words_and_counts():
    x = np.zeros((3, 70), dtype=np.float32)
    x[0, :] = np.nan
    x[1, [0, 31, 32, 69]] = np.nan
    x[2, 5] = np.inf                # a value, not a marker
    filled, mask, words, count = an.split(x)
    assert words.shape == (3, 3) and list(count) == [0, 66, 70]
    assert (words[0] == 0).all() and words[2, 2] == (1 << 6) - 1 and words[1, 0] == 0x7ffffffe and words[1, 1] == 0xfffffffe
    assert (an.mask_of(words, 70) == mask).all() and filled[2, 5] == np.inf and (filled[0] == 0).all()


@pytest.mark.parametrize("V,ldv,B", an.KERNEL_CASES)
def test_the_twin_alone_stays_within_the_tie_cap(V, ldv, B):
    x, pre, seed = an.case_inputs(V, B, False)
    U, _ = an.case_draws(V, B, seed)
    mask = ~np.isnan(x)
    mean, _ = an.visible(pre, mask, False, False, U)
    assert an.tie_draws(mean, mask, U) <= an.TIE_CAP
    # ... and with every bit set (the bit-equality case of the GPU test)
    full = np.ones_like(mask)
    assert an.tie_draws(an.visible(pre, full, False, False, U)[0], full, U) <= an.TIE_CAP


@pytest.mark.parametrize("seed", an.TOY_SEEDS)
def test_the_toy_problem_on_the_twin(seed):
    """The end-to-end problem of tests/test_gpu_absent.py with exact conditional means: the layer trained on all patients
    imputes the withheld block better than the one trained on the complete patients only, and better than the block's mean."""
    train, test, (lo, hi) = an.toy_problem(seed)
    complete = train[~np.isnan(train).any(axis=1)]
    e_all, e_complete, e_mean = an.toy_errors(an.toy_exact_impute(an.toy_train_twin(train, seed), test, lo, hi),
                                              an.toy_exact_impute(an.toy_train_twin(complete, seed), test, lo, hi), train, test, lo, hi)
    print("toy on the twin, seed %d: all patients %.4f, the %d complete ones %.4f, block mean %.4f" % (seed, e_all, len(complete), e_complete, e_mean))
    assert e_all < e_complete and e_all < e_mean
