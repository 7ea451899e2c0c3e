"""Clamped annealed importance sampling of a layer with categorical visible units on the CPU: the twin (tests/_gcais_np.py)
against exact conditional partition functions and its two limits, the public classes on a checker engine that has
``ais_conditional_grouped``, what is refused, and the tie counts of the GPU test's cases under the twin alone."""
import itertools

import numpy as np
import pytest

import _cais_np as CA
import _gais_np as G
import _gcais_np as X
import _gclamp_np as Gc
import _softmax_np as sm
import mdbn_amd

V0, H0, BOUNDS0 = 12, 7, [2, 5, 8, 10]     # the (3, 3, 2) + 2 + 2 Bernoulli layer of tests/test_softmax_api.py


def _layer(eng, W=None, c=None, b=None, seed=11):
    rbm = mdbn_amd.RBM(n_visible=V0, n_hidden=H0, numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(seed),
                       engine=eng, visible_groups=BOUNDS0)
    if W is not None:
        rbm.W.set_value(W); rbm.hbias.set_value(c); rbm.vbias.set_value(b)
    return rbm


def _small_params(seed=1):
    rs = np.random.RandomState(seed)
    return tuple(x.astype(np.float32) for x in (rs.normal(0, 0.4, (V0, H0)), rs.normal(0, 0.5, H0), rs.normal(0, 0.5, V0)))


def test_exact_values_are_the_sums_over_all_states():
    """``exact_cond_log_Z_grouped`` / ``exact_cond_log_p_grouped`` against the sum over every (free visible state, hidden state)
    of a tiny layer with a held Bernoulli column (a real value) and a held group."""
    rs = np.random.RandomState(0)
    V, H, bounds = 10, 3, [2, 5, 8, 10]            # two Bernoulli columns, groups of 3, 3, 2
    W, c, b = rs.normal(0, 0.7, (V, H)), rs.normal(0, 0.5, H), rs.normal(0, 0.5, V)
    held = np.zeros(V, dtype=bool)
    held[1] = True
    held[5:8] = True
    row = np.zeros(V)
    row[1], row[6] = 0.3, 1.0
    row[0], row[3], row[9] = 1.0, 1.0, 1.0         # the free block that is scored
    Z, p_row = 0.0, 0.0
    for b0 in (0.0, 1.0):
        for c0, c2 in itertools.product(range(3), range(2)):
            v = np.where(held, row, 0.0)
            v[0] = b0
            v[2 + c0] = 1.0
            v[8 + c2] = 1.0
            w = sum(np.exp(v @ W @ np.array(h) + v[~held] @ b[~held] + np.array(h) @ c) for h in itertools.product((0.0, 1.0), repeat=H))
            Z += w
            if (v == row).all():
                p_row = w
    assert abs(X.exact_cond_log_Z_grouped(W, c, b, bounds, row, held) - np.log(Z)) <= 1e-12
    assert abs(X.exact_cond_log_p_grouped(W, c, b, bounds, row, held) - np.log(p_row / Z)) <= 1e-12
    # no groups in the table: the plain conditional partition function
    assert abs(X.exact_cond_log_Z_grouped(W, c, b, [V], row, held) - CA.exact_cond_log_Z(W, c, b, row, held, False)) <= 1e-12


def test_the_two_limits_of_the_twin():
    """No groups in the table: ``cais_twin``; no held unit: ``_gais_np.ais_twin`` with M = N C -- the same samples, the same
    float64 log weights; float32 follows float64 along its samples."""
    V, H, s, bounds, _ = X.PARITY[1]
    W, c, b, bA = G.parity_params(V, H, s)
    N, C = X.SHAPES[1]
    betas = np.linspace(0, 1, 9)
    obs, mask = X.clamp_inputs(N, V, bounds, N)
    plain = CA.cais_twin(W, c, b, bA, False, betas, obs, mask, C, X.SEED, X.STREAM, X.STEP)
    got = X.gcais_twin(W, c, b, bA, [V], betas, obs, mask, C, X.SEED, X.STREAM, X.STEP)
    for k in ("trace_h", "trace_v"):
        np.testing.assert_array_equal(got[k], plain[k])
    np.testing.assert_allclose(got["logw"], plain["logw"], rtol=0, atol=1e-10)
    assert got["n_draws"] == plain["n_draws"] and got["group_draws"] == 0
    free_run = G.ais_twin(W, c, b, bA, bounds, betas, N * C, X.SEED, X.STREAM, X.STEP, gaps=False)
    got = X.gcais_twin(W, c, b, bA, bounds, betas, obs, np.zeros((1, V), dtype=np.float32), C, X.SEED, X.STREAM, X.STEP)
    for k in ("trace_h", "trace_v"):
        np.testing.assert_array_equal(got[k], free_run[k])
    np.testing.assert_allclose(got["logw"].reshape(-1), free_run["logw"], rtol=0, atol=1e-10)
    assert got["group_draws"] == free_run["group_draws"] and got["n_draws"] == free_run["n_draws"]
    # the clamp as the device reads it, and the float32 form along the float64 form's samples
    r64 = X.gcais_twin(W, c, b, bA, bounds, betas, obs, mask, C, X.SEED, X.STREAM, X.STEP)
    held = X.chain_held(mask, bounds, N, V, C)
    assert held[:C].all() and not held[C:2 * C].any()       # the mask set: a row with every unit held, a row with none
    assert (r64["trace_v"][:, held] == np.repeat(obs, C, axis=0)[held][None]).all()
    for lo, hi in sm.spans(bounds):
        free = ~held[:, lo]
        assert (r64["trace_v"][:, free, lo:hi].sum(axis=2) == 1.0).all() and np.isin(r64["trace_v"][:, free, lo:hi], (0.0, 1.0)).all()
    assert (r64["logw"][0] == r64["logw"][0, 0]).all()      # every unit held: nothing is random
    r32 = X.gcais_twin(W, c, b, bA, bounds, betas, obs, mask, C, X.SEED, X.STREAM, X.STEP, dtype=np.float32,
                       forced=(r64["trace_h"], r64["trace_v"]))
    width = max(X.TIE, 4.0 * r32["c_gap"])
    assert r32["flips_outside_mask"] == 0 and r32["group_miss"] < width
    assert np.abs(r32["logw"] - r64["logw"]).max() <= 1e-3


@pytest.mark.parametrize("V,H,s,bounds", X.CASES)
def test_the_twin_alone_meets_the_exact_values(V, H, s, bounds):
    """The float64 twin ALONE under the case's seed: 8 rows (row 0 holds every unit, row 1 none), C = 256, 1000 temperatures;
    every row's log Z_r^ and log p^ within 4 standard errors and 0.05 nats of the exact value -- so that on the device only
    the kernel can break it."""
    W, c, b, bA = G.case_params(V, H, s)
    v, mask = X.ground_truth_inputs(V, bounds)
    held = mask != 0
    assert held[0].all() and not held[1].any()
    Gc_held = Gc.group_held(mask, bounds, X.N_ROWS, V)
    np.testing.assert_array_equal(held, Gc_held)            # unit masks: constant on groups
    r = X.gcais_twin(W, c, b, bA, bounds, np.linspace(0, 1, X.N_BETAS + 1), np.where(held, v, np.float32(0)), mask, X.CHAINS,
                     X.CASE_SEEDS[V], X.STREAM, X.STEP, gaps=False)
    log_Z, err = X.estimate_rows(r["logw"], bA, mask, H, bounds)
    free = ~np.repeat(held, X.CHAINS, axis=0)
    for lo, hi in sm.spans(bounds):
        assert (r["trace_v"][:, free[:, lo], lo:hi].sum(axis=2) == 1.0).all()
    for row in range(X.N_ROWS):
        exact = X.exact_cond_log_Z_grouped(W, c, b, bounds, v[row], held[row])
        exact_p = X.exact_cond_log_p_grouped(W, c, b, bounds, v[row], held[row])
        log_p = exact_p + exact - log_Z[row]                # log p*_1(v_F) - log Z_r^
        print("GCAIS twin %d->%d row %d: log Z^ %.5f exact %.5f |err| %.2e = %.2f std_err (%.5f); log p^ %.5f exact %.5f"
              % (V, H, row, log_Z[row], exact, abs(log_Z[row] - exact), abs(log_Z[row] - exact) / err[row] if err[row] > 0 else 0.0, err[row],
                 log_p, exact_p))
        if held[row].all():                                 # (row 0, and whichever row the draw of the masks left no free unit)
            assert err[row] == 0.0 and abs(log_Z[row] - exact) <= 1e-9 and abs(exact_p) <= 1e-9
            continue
        assert err[row] > 0
        assert abs(log_Z[row] - exact) <= 4 * err[row] and abs(log_Z[row] - exact) <= 0.05, (row, log_Z[row], exact, err[row])
        assert abs(log_p - exact_p) <= 4 * err[row] and abs(log_p - exact_p) <= 0.05, (row, log_p, exact_p, err[row])


@pytest.mark.parametrize("V,H,s,bounds", X.CASES)
def test_one_group_free_twin_meets_the_group_posterior(V, H, s, bounds):
    """One row with only its first group free: the exact log p is the log of the exact group posterior, and the float64 twin
    alone under the case's seed meets it within 4 standard errors and 0.05 nats."""
    W, c, b, bA = G.case_params(V, H, s)
    row, mask = X.one_free_inputs(V, bounds)
    lo, hi = sm.spans(bounds)[0]
    W64, c64, b64 = (np.asarray(a, dtype=np.float64) for a in (W, c, b))
    neg_F = np.empty(hi - lo)
    for k in range(hi - lo):
        x = row[0].astype(np.float64)
        x[lo:hi] = 0.0
        x[lo + k] = 1.0
        neg_F[k] = x @ b64 + np.logaddexp(0.0, x @ W64 + c64).sum()
    want = float(neg_F[int(row[0, lo:hi].argmax())] - np.logaddexp.reduce(neg_F))
    exact_p = X.exact_cond_log_p_grouped(W, c, b, bounds, row[0], mask[0])
    assert abs(exact_p - want) <= 1e-10
    r = X.gcais_twin(W, c, b, bA, bounds, np.linspace(0, 1, X.N_BETAS + 1), np.where(mask != 0, row, np.float32(0)), mask, X.CHAINS,
                     X.ONE_FREE_SEEDS[V], X.STREAM, X.STEP, gaps=False)
    log_Z, err = X.estimate_rows(r["logw"], bA, mask, H, bounds)
    log_p = exact_p + X.exact_cond_log_Z_grouped(W, c, b, bounds, row[0], mask[0]) - log_Z[0]
    print("GCAIS twin %d->%d one group free: log p^ %.5f exact %.5f |err| %.2e std_err %.5f" % (V, H, log_p, want, abs(log_p - want), err[0]))
    assert abs(log_p - want) <= 4 * err[0] and abs(log_p - want) <= 0.05


def test_public_calls_on_a_checker_engine_with_the_grouped_call():
    eng = X.GcaisOracle()
    W, c, b = _small_params()
    rbm = _layer(eng, W, c, b)
    rs = np.random.RandomState(2)
    data = sm.one_hot_data(rs, 6, V0, BOUNDS0, p=0.4)
    mask = Gc.unit_mask(V0, BOUNDS0, rows=6)
    held = mask != 0
    K, Cn = 30, 16
    bA = rbm.base_rate_vbias(data)
    log_Z, err = rbm.conditional_log_partition(data, mask, n_chains=Cn, n_betas=K, base_vbias=bA)
    assert rbm._rng_step == 2 * K - 1 and log_Z.shape == err.shape == (6,)
    tw = X.gcais_twin(W, c, b, bA, BOUNDS0, np.linspace(0, 1, K + 1), np.where(held, data, np.float32(0)), mask, Cn,
                      rbm.theano_rng.seed, rbm.stream_id, 0, gaps=False)
    want_lz, want_err = X.estimate_rows(tw["logw"], bA, mask, H0, BOUNDS0)
    np.testing.assert_allclose(log_Z, want_lz, rtol=0, atol=1e-10)
    np.testing.assert_allclose(err, want_err, rtol=0, atol=1e-10)
    assert err[0] == 0.0 and (err[1:] > 0).all()
    for row in range(6):
        assert abs(log_Z[row] - X.exact_cond_log_Z_grouped(W, c, b, BOUNDS0, data[row], held[row])) < 1.0
    # conditional_log_likelihood is built from conditional_log_partition at the same RNG position; 2K - 1 steps each
    step = rbm._rng_step
    log_p, err_p = rbm.conditional_log_likelihood(data, mask, n_chains=Cn, n_betas=K, base_vbias=bA)
    assert rbm._rng_step == step + 2 * K - 1
    rbm._rng_step = step
    log_Z2, err2 = rbm.conditional_log_partition(data, mask, n_chains=Cn, n_betas=K, base_vbias=bA)
    neg_F = -np.asarray(rbm.free_energy(data).get_value(), dtype=np.float64)
    term = -(held * data.astype(np.float64) * b.astype(np.float64)[None, :]).sum(axis=1)
    want = neg_F + term - log_Z2
    np.testing.assert_array_equal(log_p[1:], want[1:])
    np.testing.assert_array_equal(err_p[1:], err2[1:])
    # a row with no free unit: (0, 0)
    assert log_p[0] == 0.0 and err_p[0] == 0.0 and abs(want[0]) < 1e-4
    for row in range(1, 6):
        assert abs(log_p[row] - X.exact_cond_log_p_grouped(W, c, b, BOUNDS0, data[row], held[row])) < 1.0
    # a held group (and a held Bernoulli column) takes real values: they enter through v W alone
    real = data.copy()
    g_held = next(i for i in range(2, 6) if held[i, 5] and not held[i].all())
    real[g_held, 5:8] = (0.2, 0.5, 0.9)
    rbm._rng_step = step
    lp, _ = rbm.conditional_log_likelihood(real, mask, n_chains=Cn, n_betas=K, base_vbias=bA)
    assert np.isfinite(lp).all() and lp[g_held] != log_p[g_held]
    assert abs(lp[g_held] - X.exact_cond_log_p_grouped(W, c, b, BOUNDS0, real[g_held], held[g_held])) < 1.0
    # a [V] mask for every row, the base rate from the data
    rbm._rng_step = step
    lp, e = rbm.conditional_log_likelihood(data, mask[2], n_chains=4, n_betas=5)
    assert lp.shape == (6,) and rbm._rng_step == step + 9


def test_what_is_refused_before_anything_is_drawn():
    rbm = _layer(X.GcaisOracle(), *_small_params())
    data = sm.one_hot_data(np.random.RandomState(0), 4, V0, BOUNDS0)
    mask = Gc.unit_mask(V0, BOUNDS0, rows=4)
    mask[2:, 5:8] = 0.0                              # the group [5, 8) of rows 2 and 3 is free
    split = mask.copy()
    split[3, 5:8] = (1.0, 0.0, 1.0)
    for call in (lambda: rbm.conditional_log_partition(data, split, n_chains=4, n_betas=4),
                 lambda: rbm.conditional_log_likelihood(data, split, n_chains=4, n_betas=4),
                 lambda: rbm.conditional_log_likelihood(data, split[3], n_chains=4, n_betas=4)):
        with pytest.raises(ValueError, match=r"columns 5 \.\. 7"):
            call()
    for values in ((0.0, 0.0, 0.0), (1.0, 1.0, 0.0)):    # a free group with no 1, with two
        bad = data.copy()
        bad[3, 5:8] = values
        with pytest.raises(ValueError, match="exactly one 1"):
            rbm.conditional_log_likelihood(bad, mask, n_chains=4, n_betas=4)
    half = data.copy()
    half[2, 5:8] = (0.5, 0.5, 0.0)
    with pytest.raises(ValueError):
        rbm.conditional_log_likelihood(half, mask, n_chains=4, n_betas=4)
    free_col = int(np.flatnonzero(mask[2, :2] == 0)[0]) if (mask[2, :2] == 0).any() else None
    if free_col is not None:                         # a free Bernoulli entry that is neither 0 nor 1
        frac = data.copy()
        frac[2, free_col] = 0.5
        with pytest.raises(ValueError, match="0 / 1"):
            rbm.conditional_log_likelihood(frac, mask, n_chains=4, n_betas=4)
    assert rbm._rng_step == 0
    # ... while a HELD group may hold anything, also under conditional_log_partition (which reads no free entry at all)
    anything = data.copy()
    anything[0, 5:8] = (1.0, 1.0, 0.3)               # (row 0 holds every unit)
    rbm.conditional_log_likelihood(anything, mask, n_chains=4, n_betas=4)
    bad = data.copy()
    bad[3, 5:8] = 0.0
    rbm.conditional_log_partition(bad, mask, n_chains=4, n_betas=4)
    assert rbm._rng_step == 2 * 7


def test_other_engines_keep_the_refusal():
    data = sm.one_hot_data(np.random.RandomState(0), 4, V0, BOUNDS0)
    for eng in (sm.GroupedOracle(), G.GaisOracle(), Gc.GclampOracle()):     # engines without ais_conditional_grouped
        assert not hasattr(eng, "ais_conditional_grouped")
        plain = _layer(eng)
        for call in (lambda: plain.conditional_log_partition(data, np.zeros(V0)), lambda: plain.conditional_log_likelihood(data, np.zeros(V0))):
            with pytest.raises(NotImplementedError, match="visible_groups"):
                call()
        assert plain._rng_step == 0
    sigma_free = _layer(X.GcaisOracle())
    for call in (lambda: sigma_free.tempered_chains(2), lambda: sigma_free.check_log_partition()):   # what stays refused
        with pytest.raises(NotImplementedError, match="visible_groups"):
            call()


@pytest.mark.parametrize("mask_rows", ["per row", 1])
@pytest.mark.parametrize("N,C", X.SHAPES)
@pytest.mark.parametrize("V,H,s,bounds,paths", X.PARITY[:2])
def test_the_gpu_cases_stay_under_the_tie_cap_with_the_twin_alone(V, H, s, bounds, paths, N, C, mask_rows):
    """tests/test_gpu_gcais.py caps the near ties of a forced run; under the case's seed the twin alone must stay under the
    same cap, so that only the kernel can break it.  (The 1024 -> 256 case runs on the GPU only: its twin takes seconds.)"""
    W, c, b, bA = G.parity_params(V, H, s)
    obs, mask = X.clamp_inputs(N, V, bounds, N if mask_rows == "per row" else 1)
    r = X.gcais_twin(W, c, b, bA, bounds, np.linspace(0, 1, 9), obs, mask, C, X.SEED, X.STREAM, X.STEP, gaps=True)
    width, near, cap = X.near_ties(r)
    print("GCAIS twin alone %d->%d N=%d C=%d: C_c gap %.3e, mask %.3e, near ties %d, cap %d" % (V, H, N, C, r["c_gap"], width, near, cap))
    assert near <= cap
