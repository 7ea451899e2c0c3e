"""Annealed importance sampling of a layer with categorical visible units on the CPU: the twin (tests/_gais_np.py) against
exact partition functions, the grouped base model, the public classes on the checker engine, what is refused, the C-ABI
name, and the tie counts of the GPU test's cases under the twin alone."""
import itertools
import os
import re

import numpy as np
import pytest

import _ais_np as A
import _gais_np as G
import _softmax_np as sm
import mdbn_amd
from mdbn_amd import temper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V0, H0, BOUNDS0 = 12, 7, [2, 5, 8, 10]     # the (3, 3, 2) + 2 + 2 Bernoulli layer of tests/test_softmax_api.py


def _layer(eng, V, H, bounds, W=None, c=None, b=None, seed=11):
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(seed),
                       engine=eng, visible_groups=bounds)
    if W is not None:
        rbm.W.set_value(W); rbm.hbias.set_value(c); rbm.vbias.set_value(b)
    return rbm


def test_brute_log_Z_is_the_sum_over_all_states():
    rs = np.random.RandomState(0)
    V, H, bounds = 10, 3, [2, 5, 8, 10]            # groups of 3, 3, 2 and two Bernoulli columns
    W, c, b = rs.normal(0, 0.7, (V, H)), rs.normal(0, 0.5, H), rs.normal(0, 0.5, V)
    rows = []
    for bern in itertools.product((0.0, 1.0), repeat=2):
        for cats in itertools.product(range(3), range(3), range(2)):
            v = np.zeros(V)
            v[:2] = bern
            for (lo, _), k in zip(sm.spans(bounds), cats):
                v[lo + k] = 1.0
            rows.append(v)
    v = np.array(rows)
    assert v.shape[0] == 4 * 18
    terms = []
    for h in itertools.product((0.0, 1.0), repeat=H):
        h = np.array(h)
        terms.append(v @ b + h @ c + v @ W @ h)
    t = np.concatenate(terms)
    exact = t.max() + np.log(np.exp(t - t.max()).sum())
    assert abs(G.brute_log_Z(W, c, b, bounds) - exact) <= 1e-10
    # ... and the free energy of the one-hot rows sums to the same number
    F = -(v @ b) - np.logaddexp(0.0, v @ W + c).sum(axis=1)
    assert abs(np.logaddexp.reduce(-F) - exact) <= 1e-10


@pytest.mark.parametrize("V,H,s,bounds", G.CASES)
def test_the_twin_alone_meets_the_exact_value(V, H, s, bounds):
    W, c, b, bA = G.case_params(V, H, s)
    exact = G.brute_log_Z(W, c, b, bounds)
    r = G.ais_twin(W, c, b, bA, bounds, np.linspace(0, 1, 1001), 512, G.CASE_SEEDS[V], G.STREAM, G.STEP, gaps=False)
    log_Z, err = G.estimate(r["logw"], bA, H, bounds)
    print("GAIS twin %d->%d: log Z^ %.5f exact %.5f |err| %.5f = %.2f std_err (%.5f)" % (V, H, log_Z, exact, abs(log_Z - exact),
                                                                                       abs(log_Z - exact) / err, err))
    for lo, hi in sm.spans(bounds):
        assert (r["trace_v"][:, :, lo:hi].sum(axis=2) == 1.0).all()
    assert abs(log_Z - exact) <= 4 * err and abs(log_Z - exact) <= 0.05, (log_Z, exact, err)


def test_pick_is_grouped_sample():
    rs = np.random.RandomState(3)
    bounds = [1, 3, 67, 70]
    pre = 2.0 * rs.normal(size=(33, 70))
    U = rs.uniform(size=(33, 70)).astype(np.float32)
    want = sm.grouped_sample(sm.grouped_softmax(pre, bounds)[0], bounds, U)
    np.testing.assert_array_equal(G.pick(G.running_sums(pre, bounds, np.float64), bounds, U), want)


def test_base_rate_and_the_grouped_base_model():
    eng = G.GaisOracle()
    rbm = _layer(eng, V0, H0, BOUNDS0)
    data = sm.one_hot_data(np.random.RandomState(0), 40, V0, BOUNDS0, p=0.4)
    data[:, 2:5] = 0.0
    data[:, 2] = 1.0                                # categories 3 and 4 of the first group are never seen
    bA = rbm.base_rate_vbias(data).astype(np.float64)
    assert np.isfinite(bA).all()
    for lo, hi in sm.spans(BOUNDS0):
        assert abs(np.logaddexp.reduce(bA[lo:hi])) < 1e-6
        n = data[:, lo:hi].sum(axis=0, dtype=np.float64)
        np.testing.assert_allclose(bA[lo:hi], np.log((n + 0.05) / (40 + 0.05 * (hi - lo))), rtol=1e-6, atol=1e-9)
    bern = sm.bernoulli_columns(BOUNDS0, V0)
    p = (data[:, bern].sum(axis=0, dtype=np.float64) + 0.05) / 40.1
    np.testing.assert_allclose(bA[bern], np.log(p) - np.log1p(-p), rtol=1e-5, atol=1e-6)
    want = H0 * np.log(2.0) + np.logaddexp(0.0, bA[bern]).sum() + sum(np.logaddexp.reduce(bA[lo:hi]) for lo, hi in sm.spans(BOUNDS0))
    assert abs(temper.base_log_partition(bA, H0, False, BOUNDS0) - want) < 1e-12
    assert abs(temper.base_log_partition(bA, H0, False, rbm.visible_groups) - G.log_Z_base(bA, H0, BOUNDS0)) < 1e-12
    assert temper.base_log_partition(bA, H0, False) == A.log_Z_base(bA, H0, False)        # no groups: unchanged
    lz, err = mdbn_amd.ais_estimate(np.zeros(8), bA, H0, False, groups=BOUNDS0)
    assert abs(lz - want) < 1e-12 and err == 0.0
    with pytest.raises(ValueError):
        temper.base_log_partition(bA, H0, True, BOUNDS0)


def test_public_calls_on_the_checker_engine():
    eng = G.GaisOracle()
    rs = np.random.RandomState(1)
    W, c, b = (x.astype(np.float32) for x in (rs.normal(0, 0.4, (V0, H0)), rs.normal(0, 0.5, H0), rs.normal(0, 0.5, V0)))
    rbm = _layer(eng, V0, H0, BOUNDS0, W, c, b)
    data = sm.one_hot_data(rs, 40, V0, BOUNDS0, p=0.4)
    K, M = 40, 32
    bA = rbm.base_rate_vbias(data)
    log_Z, err = rbm.log_partition(n_chains=M, n_betas=K, base_vbias=bA)
    assert rbm._rng_step == 2 * K - 1
    tw = G.ais_twin(rbm.W.get_value(), rbm.hbias.get_value(), rbm.vbias.get_value(), bA, BOUNDS0, np.linspace(0, 1, K + 1), M,
                    rbm.theano_rng.seed, rbm.stream_id, 0, gaps=False)
    assert (log_Z, err) == G.estimate(tw["logw"], bA, H0, BOUNDS0)
    exact = G.brute_log_Z(rbm.W.get_value(), rbm.hbias.get_value(), rbm.vbias.get_value(), BOUNDS0)
    assert abs(log_Z - exact) < 1.0
    ll, err2 = rbm.log_likelihood(data, n_chains=M, n_betas=K)
    assert rbm._rng_step == 2 * (2 * K - 1)
    rbm._rng_step = 2 * K - 1
    log_Z2, err3 = rbm.log_partition(n_chains=M, n_betas=K, data=data)
    assert ll == float(np.mean(-np.asarray(rbm.free_energy(data).get_value(), dtype=np.float64)) - log_Z2) and err2 == err3
    # a DBN whose input layer has groups
    mdbn_amd.DBN.verbose = False
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(9), n_ins=V0, gauss=False,
                       hidden_layers_sizes=[H0], n_outs=4, engine=eng, visible_groups=BOUNDS0)
    got = net.layer_log_likelihood(0, data, n_chains=8, n_betas=10)
    net.rbm_layers[0]._rng_step -= 19
    assert got == net.rbm_layers[0].log_likelihood(data, n_chains=8, n_betas=10) and np.isfinite(got[0])


def test_rows_that_are_not_one_hot_are_refused():
    eng = G.GaisOracle()
    rbm = _layer(eng, V0, H0, BOUNDS0)
    data = sm.one_hot_data(np.random.RandomState(0), 10, V0, BOUNDS0)
    for bad_value in (1.0, 0.0):
        bad = data.copy()
        bad[4, 5:8] = bad_value                     # two (three) 1s in a group; none
        with pytest.raises(ValueError, match="exactly one 1"):
            rbm.log_likelihood(bad, n_chains=4, n_betas=4)
    half = data.copy()
    half[2, 8:10] = 0.5
    with pytest.raises(ValueError, match="exactly one 1"):
        rbm.log_likelihood(half, n_chains=4, n_betas=4)
    assert rbm._rng_step == 0


def test_what_stays_refused():
    eng = G.GaisOracle()
    rbm = _layer(eng, V0, H0, BOUNDS0)
    data = sm.one_hot_data(np.random.RandomState(0), 10, V0, BOUNDS0)
    mask = np.zeros(V0)
    for call in (lambda: rbm.log_partition(n_chains=4, n_betas=4, method="tempering"),
                 lambda: rbm.log_likelihood(data, n_chains=4, n_betas=4, method="tempering"),
                 lambda: rbm.check_log_partition(), lambda: rbm.tempered_chains(2),
                 lambda: rbm.gibbs_vhv_clamped(data[:2], mask, 2), lambda: rbm.impute(data[:2], mask, n_steps=2, burn_in=0),
                 lambda: rbm.conditional_log_partition(data[:2], mask), lambda: rbm.conditional_log_likelihood(data[:2], mask)):
        with pytest.raises(NotImplementedError, match="visible_groups"):
            call()
    assert rbm._rng_step == 0                       # refused before anything was drawn
    plain = _layer(sm.GroupedOracle(), V0, H0, BOUNDS0)         # an engine without ais_grouped
    for call in (lambda: plain.log_partition(n_chains=4, n_betas=4), lambda: plain.log_likelihood(data, n_chains=4, n_betas=4)):
        with pytest.raises(NotImplementedError, match="visible_groups"):
            call()
    assert plain._rng_step == 0


def test_declared_exported_and_bound(built_lib):
    from mdbn_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mdbn_hip.h")).read()
    name = "mdbn_ais_run_grouped"
    assert re.search(r"^int\s+%s\(" % name, header, re.M) and name in _lib.SIGNATURES and hasattr(lib, name)
    decl = header[header.index(name + "("):]
    assert len(_lib.SIGNATURES[name]) == decl[:decl.index(");")].count(",") + 1
    assert _lib.SIGNATURES[name][:22] == _lib.SIGNATURES["mdbn_ais_run"]
    # the rules that need no device: a Gaussian layer, a bad table, path 1 on a layer that is not LDS-resident
    host = np.array([0, 5, 10], dtype=np.int32)

    def run(V=100, H=24, gauss=0, path=0, table=host, dev=1):
        t = None if table is None else table.ctypes.data
        return lib.mdbn_ais_run_grouped(None, None, None, V, H, H, None, None, None, gauss, None, 9, 64, V, None, None, None, None,
                                        path, None, None, 0, table.ctypes.data if (dev and table is not None) else None, t,
                                        0 if table is None else table.size - 1)
    assert run(gauss=1) == -1 and "Gaussian" in _lib.last_error()
    assert run(table=np.array([0, 10, 5], dtype=np.int32)) == -1 and "group" in _lib.last_error()
    assert run(table=np.array([0, 1], dtype=np.int32)) == -1 and "group" in _lib.last_error()
    assert run(table=np.array([0, 65], dtype=np.int32)) == -1 and "group" in _lib.last_error()
    assert run(table=np.array([90, 101], dtype=np.int32)) == -1 and "group" in _lib.last_error()
    assert run(dev=0) == -1 and "group_start" in _lib.last_error()
    assert run(V=1024, H=256, path=1, table=np.arange(0, 1025, 4, dtype=np.int32)) == -1 and "LDS-resident" in _lib.last_error()
    assert run() == -1 and "workspace" in _lib.last_error()          # a good table: the next rule in line


@pytest.mark.parametrize("M", G.PARITY_M)
@pytest.mark.parametrize("V,H,s,bounds,paths", G.PARITY)
def test_the_gpu_cases_stay_under_the_tie_cap_with_the_twin_alone(V, H, s, bounds, paths, M):
    """tests/test_gpu_gais.py caps the near ties of a forced run; under the case's seed the twin alone must stay under the
    same cap, so that only the kernel can break it."""
    W, c, b, bA = G.parity_params(V, H, s)
    r = G.ais_twin(W, c, b, bA, bounds, np.linspace(0, 1, 9), M, G.SEED, G.STREAM, G.STEP, gaps=True)
    mask = max(A.TIE, 4.0 * r["c_gap"])
    near, cap = r["n_ties"] + r["group_near"](mask), G.tie_cap(r, mask)
    print("GAIS twin alone %d->%d M=%d: C_c gap %.3e, mask %.3e, near ties %d, cap %d" % (V, H, M, r["c_gap"], mask, near, cap))
    assert near <= cap
