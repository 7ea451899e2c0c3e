"""Clamped Gibbs sampling of a layer with categorical visible units on the CPU: the twin (tests/_gclamp_np.py) against exact
posteriors, the public classes on a checker engine that has ``gibbs_clamped_grouped``, a mask that splits a group, the
C-ABI name, and the tie counts of the GPU test's cases under the twin alone."""
import itertools
import os
import re

import numpy as np
import pytest

import _gclamp_np as Gc
import _softmax_np as sm
import mdbn_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V0, H0, BOUNDS0 = 12, 7, [2, 5, 8, 10]     # the (3, 3, 2) + 2 + 2 Bernoulli layer of tests/test_softmax_api.py


def _layer(eng, V, H, bounds, W=None, c=None, b=None, seed=11):
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(seed),
                       engine=eng, visible_groups=bounds)
    if W is not None:
        rbm.W.set_value(W); rbm.hbias.set_value(c); rbm.vbias.set_value(b)
    return rbm


def test_exact_posterior_is_the_sum_over_all_states():
    """``exact_posterior_grouped`` against the sum over every (free visible state, hidden state) of a tiny layer."""
    rs = np.random.RandomState(0)
    V, H, bounds = 10, 3, [2, 5, 8, 10]            # two Bernoulli columns, groups of 3, 3, 2
    W, c, b = rs.normal(0, 0.7, (V, H)), rs.normal(0, 0.5, H), rs.normal(0, 0.5, V)
    held = np.zeros(V, dtype=bool)
    held[1] = True
    held[5:8] = True
    row = np.zeros(V)
    row[1], row[6] = 0.3, 1.0                      # (a held Bernoulli column may hold any real value)
    num_v, num_h, Z = np.zeros(V), np.zeros(H), 0.0
    for b0 in (0.0, 1.0):
        for c0, c2 in itertools.product(range(3), range(2)):
            v = row.copy()
            v[0] = b0
            v[2 + c0] = 1.0
            v[8 + c2] = 1.0
            for h in itertools.product((0.0, 1.0), repeat=H):
                h = np.array(h)
                w = np.exp(v @ W @ h + v @ b + h @ c)
                num_v += w * v
                num_h += w * h
                Z += w
    ev, eh = Gc.exact_posterior_grouped(W, c, b, bounds, row, held)
    np.testing.assert_allclose(ev, num_v / Z, rtol=0, atol=1e-12)
    np.testing.assert_allclose(eh, num_h / Z, rtol=0, atol=1e-12)


def test_float32_twin_follows_the_float64_twin():
    """The float32 form along the float64 form's samples: the same draws away from ties, means within the ``prob`` tolerance."""
    V, H, s, bounds, _ = Gc.PARITY[1]
    W, c, b = Gc.parity_params(V, H, s)
    v0, obs, mask = Gc.inputs(V, bounds, 22, True)
    r64 = Gc.gclamp_twin(W, c, b, bounds, v0, obs, mask, Gc.N_STEPS, Gc.BURN_IN, Gc.SEED, Gc.STREAM, Gc.STEP)
    r32 = Gc.gclamp_twin(W, c, b, bounds, v0, obs, mask, Gc.N_STEPS, Gc.BURN_IN, Gc.SEED, Gc.STREAM, Gc.STEP, dtype=np.float32,
                         forced=(r64["trace_h"], r64["trace_v"]))
    held = Gc.group_held(mask, bounds, 22, V)
    assert (r64["trace_v"][:, held] == obs[held][None]).all()
    assert held[0].all() and not held[1].any()              # the mask set: a row with every unit held, a row with none
    for lo, hi in sm.spans(bounds):
        free = ~held[:, lo]
        assert (r64["trace_v"][:, free, lo:hi].sum(axis=2) == 1.0).all()
    mask_w = max(Gc.TIE, 4.0 * r32["c_gap"])
    assert r32["flips_outside_mask"] == 0 and r32["group_miss"] < mask_w
    assert np.abs(r32["v_mean"] - r64["v_mean"]).max() <= sm.MEAN_TOL and np.abs(r32["h_mean"] - r64["h_mean"]).max() <= 2e-6


def test_public_calls_on_a_checker_engine_with_the_grouped_call():
    eng = Gc.GclampOracle()
    rs = np.random.RandomState(1)
    W, c, b = (x.astype(np.float32) for x in (rs.normal(0, 0.4, (V0, H0)), rs.normal(0, 0.5, H0), rs.normal(0, 0.5, V0)))
    rbm = _layer(eng, V0, H0, BOUNDS0, W, c, b)
    data = sm.one_hot_data(rs, 6, V0, BOUNDS0, p=0.4)
    mask = Gc.unit_mask(V0, BOUNDS0, rows=6)
    held = mask != 0
    n = 9
    out = rbm.gibbs_vhv_clamped(data, mask, n, burn_in=2, trace=True)
    assert rbm._rng_step == 2 * n
    state, v_avg, tv = (np.asarray(out[i].get_value()) for i in (5, 6, 9))
    assert tv.shape == (n, 6, V0) and (tv[:, held] == data[held][None]).all()
    for lo, hi in sm.spans(BOUNDS0):
        free = ~held[:, lo]
        assert np.isin(tv[:, free, lo:hi], (0.0, 1.0)).all() and (tv[:, free, lo:hi].sum(axis=2) == 1.0).all()
        assert np.abs(v_avg[free, lo:hi].sum(axis=1) - 1.0).max() <= 1e-6
    np.testing.assert_array_equal(state, tv[-1])
    # ... and it is the twin's chain
    tw = Gc.gclamp_twin(W, c, b, BOUNDS0, data, data, mask, n, 2, rbm.theano_rng.seed, rbm.stream_id, 0)
    np.testing.assert_array_equal(tv, tw["trace_v"])
    np.testing.assert_allclose(v_avg, tw["v_avg"], rtol=0, atol=1e-6)
    # impute: free groups start at the softmax of vbias, v_hat sums to 1 over them, observed entries come back exactly
    v_hat, h_hat = rbm.impute(data, mask, n_steps=12, burn_in=3, n_chains=2)
    assert rbm._rng_step == 2 * n + 2 * 12
    np.testing.assert_array_equal(v_hat[held], data[held])
    for lo, hi in sm.spans(BOUNDS0):
        free = ~held[:, lo]
        assert np.abs(v_hat[free, lo:hi].sum(axis=1) - 1.0).max() <= 1e-6
    assert h_hat.shape == (6, H0) and (h_hat > 0).all() and (h_hat < 1).all()
    # a [V] mask for the whole batch
    out = rbm.gibbs_vhv_clamped(data, mask[2], 3)
    assert rbm._rng_step == 2 * n + 2 * 12 + 6 and np.asarray(out[5].get_value()).shape == (6, V0)


def test_a_mask_that_splits_a_group_is_refused_before_anything_is_drawn():
    rbm = _layer(Gc.GclampOracle(), V0, H0, BOUNDS0)
    data = sm.one_hot_data(np.random.RandomState(0), 4, V0, BOUNDS0)
    mask = Gc.unit_mask(V0, BOUNDS0, rows=4)
    mask[3, 5:8] = (1.0, 0.0, 1.0)
    for call in (lambda: rbm.gibbs_vhv_clamped(data, mask, 2), lambda: rbm.impute(data, mask, n_steps=2, burn_in=0),
                 lambda: rbm.impute(data, mask[3], n_steps=2, burn_in=0)):
        with pytest.raises(ValueError, match=r"columns 5 \.\. 7"):
            call()
    assert rbm._rng_step == 0


def test_other_engines_keep_the_refusal():
    plain = _layer(sm.GroupedOracle(), V0, H0, BOUNDS0)         # an engine without gibbs_clamped_grouped
    data = sm.one_hot_data(np.random.RandomState(0), 4, V0, BOUNDS0)
    for call in (lambda: plain.gibbs_vhv_clamped(data, np.zeros(V0), 2), lambda: plain.impute(data, np.zeros(V0), n_steps=2, burn_in=0)):
        with pytest.raises(NotImplementedError, match="visible_groups"):
            call()
    assert plain._rng_step == 0


def _ground_truth_twin(V, H, s, bounds, one_free):
    W, c, b, row, held, ev, eh = Gc.ground_truth_case(V, H, s, bounds, one_free)
    seed = (Gc.ONE_FREE_SEEDS if one_free else Gc.CASE_SEEDS)[V]
    start = np.repeat(Gc.base_start(b, bounds, row, held)[None], Gc.M, axis=0)
    r = Gc.gclamp_twin(W, c, b, bounds, start, np.repeat(row[None], Gc.M, axis=0), held[None].astype(np.float32), Gc.GT_STEPS,
                       Gc.GT_BURN, seed, Gc.STREAM, Gc.STEP, gaps=True)
    return r, held, ev, eh


@pytest.mark.parametrize("one_free", [False, True])
@pytest.mark.parametrize("V,H,s,bounds", Gc.CASES)
def test_twin_against_exact_posterior(V, H, s, bounds, one_free):
    """The float64 twin ALONE under the case's seed: v_avg / h_avg of M = 128 chains of 600 steps (100 burn-in) within 2.5
    standard errors of the exact posterior means, the largest standard error <= 0.01, and its near ties within the share the
    GPU test allows -- so that on the device only the kernel can break either."""
    r, held, ev, eh = _ground_truth_twin(V, H, s, bounds, one_free)
    se, z = Gc.z_statistic(r["v_avg"], r["h_avg"], held, ev, eh)
    mask, near, draws = Gc.near_ties(r)
    print("gclamp twin %d->%d%s: largest standard error %.5f, largest |error| / standard error %.2f; near ties %d of %d draws"
          % (V, H, " one group free" if one_free else "", se, z, near, draws))
    assert se <= Gc.SE_CAP and z <= Gc.GT_Z, (se, z)
    assert near <= Gc.TIE_SHARE * draws, (near, draws)


@pytest.mark.parametrize("per_row", [True, False])
@pytest.mark.parametrize("B", Gc.PARITY_B)
@pytest.mark.parametrize("V,H,s,bounds,paths", Gc.PARITY[:2])
def test_the_gpu_cases_stay_under_the_tie_share_with_the_twin_alone(V, H, s, bounds, paths, B, per_row):
    """tests/test_gpu_gclamp.py caps the near ties of a forced run at TIE_SHARE of its draws; the twin alone must stay under
    it on the same inputs and seed.  (The 1024 -> 256 case runs on the GPU only: its twin takes seconds.)"""
    W, c, b = Gc.parity_params(V, H, s)
    v0, obs, mask = Gc.inputs(V, bounds, B, per_row)
    r = Gc.gclamp_twin(W, c, b, bounds, v0, obs, mask, Gc.N_STEPS, Gc.BURN_IN, Gc.SEED, Gc.STREAM, Gc.STEP, gaps=True)
    _, near, draws = Gc.near_ties(r)
    assert near <= Gc.TIE_SHARE * draws, (near, draws)


def test_declared_exported_and_bound(built_lib):
    from mdbn_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mdbn_hip.h")).read()
    name = "mdbn_gibbs_clamped_grouped"
    assert re.search(r"^int\s+%s\(" % name, header, re.M) and name in _lib.SIGNATURES and hasattr(lib, name)
    decl = header[header.index(name + "("):]
    assert len(_lib.SIGNATURES[name]) == decl[:decl.index(");")].count(",") + 1
    plain = _lib.SIGNATURES["mdbn_gibbs_clamped"]
    assert _lib.SIGNATURES[name][:-3] == plain[:14] + plain[16:]          # mdbn_gibbs_clamped's without gauss, add_noise
    # the rules that need no device: a bad table, path 1 on a layer that is not LDS-resident
    host = np.array([0, 5, 10], dtype=np.int32)

    def run(V=100, H=24, path=0, table=host, dev=1, n_steps=4):
        t = None if table is None else table.ctypes.data
        return lib.mdbn_gibbs_clamped_grouped(None, None, None, None, None, 8, 8, V, None, V, H, H, None, None, n_steps, 0, None, None,
                                              None, None, None, None, None, path, 0, None, None, 0,
                                              table.ctypes.data if (dev and table is not None) else None, t,
                                              0 if table is None else table.size - 1)
    assert run(table=np.array([0, 10, 5], dtype=np.int32)) == -1 and "group" in _lib.last_error()
    assert run(table=np.array([0, 1], dtype=np.int32)) == -1 and "group" in _lib.last_error()
    assert run(table=np.array([0, 65], dtype=np.int32)) == -1 and "group" in _lib.last_error()
    assert run(table=np.array([90, 101], dtype=np.int32)) == -1 and "group" in _lib.last_error()
    assert run(dev=0) == -1 and "group_start" in _lib.last_error()
    assert run(n_steps=0) == -1 and "n_steps" in _lib.last_error()
    assert run(V=1024, H=256, path=1, table=np.arange(0, 1025, 4, dtype=np.int32)) == -1 and "LDS-resident" in _lib.last_error()
    assert run() == -1 and "workspace" in _lib.last_error()          # a good table: the next rule in line
    assert run(table=None) == -1 and "workspace" in _lib.last_error()        # n_groups = 0 reads no table
