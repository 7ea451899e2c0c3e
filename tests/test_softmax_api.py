"""Categorical visible units through the public classes on the CPU checker engine: the model against an enumeration of its
energy function, the C-ABI names, the engine calls a grouped plan makes and their order, six steps against a hand-written
float64 loop (plain, centred, sparse, and centred + sparse through the weights or the biases only), what is refused, the trainers' keyword, the checkpoint round trip, one_hot_groups,
and the tie count of the GPU test's kernel cases under the twin alone."""
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import _softmax_np as sm
import mdbn_amd
from mdbn_amd import _lib, checkpoint, utils
from oracle import rbm_np
from oracle.philox_np import PhiloxDraws, uniform

V, H, N = 12, 7, 40
BOUNDS = [2, 5, 8, 10]          # two Bernoulli columns, groups of 3, 3 and 2, two Bernoulli columns
SIZES = (10, 10, 7, 10, 1, 10)  # a ragged and a one-row minibatch
NAMES = ("mdbn_group_softmax_workspace_bytes", "mdbn_group_softmax_sample", "mdbn_cd_step_grouped", "mdbn_center_hidden_rows")
PARAMS = ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed")
LOGGED = ("cd_step", "cd_step_grouped", "cd_forward", "cd_statistics", "cd_train_step", "apply_update", "center_offsets",
          "center_hidden_rows", "center_stats", "sparsity_activity", "sparsity_stats", "group_softmax", "propdown", "free_energy")


class Recorder(object):
    """Proxy of an engine: logs the name of every call in LOGGED, passes everything through."""

    def __init__(self, engine, log):
        self._engine, self._log = engine, log

    def __getattr__(self, name):
        target = getattr(self._engine, name)
        if name not in LOGGED:
            return target

        def call(*args, **kw):
            self._log.append(name)
            return target(*args, **kw)
        return call


class FakeGroup(object):
    world_size, rank = 2, 0

    def shard(self, n):
        return (0, n)


def problem():
    rs = np.random.RandomState(0)
    return sm.one_hot_data(rs, N, V, BOUNDS, p=0.4).astype(np.float64), [rs.permutation(N)[:n].astype(np.int64) for n in SIZES]


def layer(engine, groups=BOUNDS, n_visible=V):
    return mdbn_amd.RBM(n_visible=n_visible, n_hidden=H, numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(11),
                        engine=engine, visible_groups=groups)


def make(mode="plain", groups=BOUNDS, persistent=False, k=2):
    log = []
    inner = sm.GroupedOracle()
    eng = Recorder(inner, log)
    data, batches = problem()
    rbm = layer(eng, groups)
    chain = np.zeros((10, H), dtype=np.float32) if persistent else None
    _, up = rbm.get_cost_updates(lr=0.05, k=k, batch_size=10, persistent=chain, weightcost=2e-4, **sm.MODE_KEYWORDS[mode])
    fn = mdbn_amd.function(up, mdbn_amd.shared(data, engine=eng), data_parallel=None)
    del log[:]
    return fn, rbm, log, batches, inner, data


def take(log):
    out = list(log)
    del log[:]
    return out


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_the_names_are_in_the_header_and_in_the_signatures():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mdbn_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["mdbn_group_softmax_sample"]) == 17 and len(_lib.SIGNATURES["mdbn_cd_step_grouped"]) == 6
    assert len(_lib.SIGNATURES["mdbn_center_hidden_rows"]) == 21
    assert re.search(r"#define\s+MDBN_GROUP_MAX\s+(\d+)", header).group(1) == str(utils.GROUP_MAX) and utils.GROUP_MAX >= 64
    # the struct the driver takes keeps its layout: the table travels as extra arguments
    assert "group" not in " ".join(f[0] for f in _lib.CdArgs._fields_ + _lib.UpdateArgs._fields_)


# ------------------------------------------------------------------------------------------------------------------ the model
def test_the_twin_the_free_energy_and_group_posterior_are_the_enumerated_model():
    """Groups (3, 3, 2) plus two Bernoulli units, H = 3: every one of the 18 * 4 visible and 8 hidden states of
    E(v, h) = -v . vbias - h . hbias - v W h, against the twin's p(v | h), exp(-F(v)) and group_posterior."""
    rs = np.random.RandomState(3)
    bounds, Vs, Hs = [0, 3, 6, 8], 10, 3
    # (parameters that float32 holds exactly: a layer's arrays are float32 whatever the engine computes in)
    W, hb, vb = (rs.normal(size=n).astype(np.float32).astype(np.float64) for n in ((Vs, Hs), Hs, Vs))
    vis = []
    for a, b, c, d, e in itertools.product(range(3), range(3), range(2), range(2), range(2)):
        v = np.zeros(Vs)
        v[a], v[3 + b], v[6 + c], v[8], v[9] = 1, 1, 1, d, e
        vis.append(v)
    vis = np.array(vis)
    hid = np.array(list(itertools.product((0.0, 1.0), repeat=Hs)))
    assert vis.shape == (72, Vs) and hid.shape == (8, Hs)
    joint = np.exp(vis @ vb[:, None] + (hid @ hb)[None, :] + vis @ W @ hid.T)          # exp(-E) [72, 8]
    # p(v | h): the product of the grouped means over the units that are on (and 1 - mean over Bernoulli units that are off)
    mean = sm.grouped_softmax(hid @ W.T + vb, bounds)[0]                               # [8, V]
    p = np.ones((72, 8))
    for i, v in enumerate(vis):
        p[i] = np.prod(np.where(v[None, :8] == 1, mean[:, :8], 1.0), axis=1) * np.prod(np.where(v[None, 8:] == 1, mean[:, 8:],
                                                                                                1 - mean[:, 8:]), axis=1)
    assert np.abs(p - joint / joint.sum(axis=0, keepdims=True)).max() < 1e-12
    # exp(-F(v)) is the joint summed over h
    s = rbm_np.RBMState(Vs, Hs, W=W, hbias=hb, vbias=vb)
    marg = joint.sum(axis=1)
    assert np.abs(np.exp(-rbm_np.free_energy(s, vis)) / marg - 1.0).max() < 1e-12
    # group_posterior: p(category | the other visibles) from the marginal
    eng = sm.GroupedOracle()
    rbm = mdbn_amd.RBM(n_visible=Vs, n_hidden=Hs, W=W, hbias=hb, vbias=vb, engine=eng, visible_groups=bounds)
    for g, (lo, hi) in enumerate(sm.spans(bounds)):
        got = rbm.group_posterior(vis, g)
        rest = np.delete(vis, np.arange(lo, hi), axis=1)
        for i in range(72):
            same = (np.delete(vis, np.arange(lo, hi), axis=1) == rest[i]).all(axis=1)
            want = np.array([marg[same & (vis[:, lo + c] == 1)].sum() for c in range(hi - lo)])
            assert np.abs(got[i] - want / want.sum()).max() < 1e-12
    assert rbm._rng_step == 0
    assert np.abs(rbm.group_posterior(vis, -1) - rbm.group_posterior(vis, 2)).max() == 0.0
    with pytest.raises(IndexError):
        rbm.group_posterior(vis, 3)


def test_sampling_rule_first_boundary_above_u_and_the_last_category_fallback():
    mean = np.array([[0.25, 0.25, 0.5, 0.3], [0.25, 0.25, 0.5, 0.3], [0.25, 0.25, 0.5, 0.3], [0.2, 0.3, 0.4, 0.3]])
    U = np.array([[0.1, 0, 0, 0.2], [0.25, 0, 0, 0.3], [0.9999, 0, 0, 0.9], [0.95, 0, 0, 0.1]])
    s = sm.grouped_sample(mean, [0, 3], U)
    assert s.tolist() == [[1, 0, 0, 1], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 1, 1]]       # (row 3: the sum falls short of u)
    assert sm.tie_draws(mean, [0, 3], U) == 2                                          # row 1: u on C_0 and on the Bernoulli mean
    # the cross-entropy comes from the log-sum-exp: finite where the probability underflows
    pre = np.array([[0.0, -2000.0, 3.0]])
    assert np.isclose(sm.grouped_cost(pre, np.array([[0.0, 1.0, 1.0]]), [0, 2]), 2000.0 + np.log1p(np.exp(-3.0)))


def test_the_row_route_to_the_centred_hidden_statistic_is_the_route_through_S():
    rs = np.random.RandomState(4)
    B, rho = 9, 0.9
    v0, nv = sm.one_hot_data(rs, B, V, BOUNDS).astype(np.float64), sm.grouped_softmax(rs.normal(size=(B, V)), BOUNDS)[0]
    ph, nh, mu, lam = rs.uniform(size=(B, H)), rs.uniform(size=(B, H)), rs.uniform(size=V), rs.uniform(size=H)
    S, s_h, s_v = rbm_np.cd_statistics(v0, ph, nv, nh)
    import _center_np as cn
    want = cn.center_stats(S, s_h, s_v, mu, lam, rho)[1]
    assert np.abs(sm.center_hidden_rows(v0, nv, ph, nh, s_h, s_v, mu, lam, rho) - want).max() < 1e-12
    # after a sparsity transform of the packed statistics the rows no longer hold all of S and s_h: its share is added
    import _sparsity_np as sn
    q, vm = rs.uniform(size=H), v0.mean(axis=0)
    for w_scale, b_scale in ((0.05 * 10, 0.05 * B), (0.0, 0.05 * B)):
        S2, sh2, sv2 = sn.stats(S, s_h, s_v, q, vm if w_scale else None, 0.1, w_scale, b_scale)
        want = cn.center_stats(S2, sh2, sv2, mu, lam, rho)[1]
        got = sm.center_hidden_rows(v0, nv, ph, nh, sh2, sv2, mu, lam, rho, sparsity=(q, vm if w_scale else None, 0.1, w_scale, b_scale))
        assert np.abs(got - want).max() < 1e-12
        assert np.abs(sm.center_hidden_rows(v0, nv, ph, nh, sh2, sv2, mu, lam, rho) - want).max() > 1e-3   # (without it: wrong)


# ------------------------------------------------------------------------------------------------------------------ eager calls
def test_eager_sampling_goes_through_the_kernel_call_and_keeps_the_step_count():
    log = []
    inner = sm.GroupedOracle()
    rbm = layer(Recorder(inner, log))
    rs = np.random.RandomState(1)
    h = (rs.uniform(size=(6, H)) < 0.5).astype(np.float64)
    pre, mean = rbm.propdown(h)
    assert take(log) == ["propdown", "group_softmax"] and rbm._rng_step == 1
    want = sm.grouped_softmax(h @ rbm.W.get_value().astype(np.float64) .T + rbm.vbias.get_value(), BOUNDS)[0]
    assert np.abs(mean.tensor.numpy() - want).max() < 1e-12 and np.abs(pre.tensor.numpy() - (h @ rbm.W.tensor.numpy().T)).max() < 1e-12
    _, mean2, sample = rbm.sample_v_given_h(h)
    U = uniform(6, V, rbm.theano_rng.seed, rbm.stream_id, 1, 0, 0)
    assert np.array_equal(sample.tensor.numpy(), sm.grouped_sample(want, BOUNDS, U))
    for lo, hi in sm.spans(BOUNDS):
        assert (sample.tensor.numpy()[:, lo:hi].sum(axis=1) == 1).all()
    assert rbm._rng_step == 2
    # the chain call loops the eager calls: the same draws as n_steps eager gibbs_vhv calls
    v = sm.one_hot_data(rs, 6, V, BOUNDS).astype(np.float64)
    a, b = layer(inner), layer(inner)
    b.stream_id = a.stream_id
    out = a.gibbs_vhv_chain(v, 3)
    x = v
    for _ in range(3):
        eager = b.gibbs_vhv(x)
        x = eager[5]
    assert a._rng_step == b._rng_step == 6
    for got, want_t in zip(out, eager):
        assert np.array_equal(got.tensor.numpy(), want_t.tensor.numpy())
    # the reconstruction cost is the cross-entropy of the twin, mean over rows; free energies are untouched
    pre = rs.normal(size=(6, V))
    assert np.isclose(rbm.get_reconstruction_cost(pre, v), sm.grouped_cost(pre, v, BOUNDS) / 6.0, rtol=1e-12)
    plain = layer(inner, None)
    assert np.array_equal(plain.free_energy(v).tensor.numpy(), layer(inner).free_energy(v).tensor.numpy())


def test_a_dbn_takes_the_table_for_its_input_layer_and_down_pass_returns_grouped_means():
    mdbn_amd.DBN.verbose = False
    eng = sm.GroupedOracle()
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, gauss=False, hidden_layers_sizes=[H], n_outs=4, engine=eng,
                       visible_groups=BOUNDS)
    assert net.rbm_layers[0].visible_groups.host.tolist() == BOUNDS and net.rbm_layers[1].visible_groups is None
    x = net.down_pass(np.random.RandomState(2).uniform(size=(5, 4)))
    for lo, hi in sm.spans(BOUNDS):
        assert np.allclose(x[:, lo:hi].sum(axis=1), 1.0, atol=1e-6)
    assert not np.allclose(x[:, :2].sum(axis=1), 1.0)
    with pytest.raises(ValueError, match="gauss=False"):
        mdbn_amd.DBN(n_ins=V, hidden_layers_sizes=[H], n_outs=4, engine=eng, visible_groups=BOUNDS)
    k3 = mdbn_amd.DBN(n_ins=V, gauss=False, hidden_layers_sizes=[], n_outs=4, engine=eng, visible_groups=3)
    assert k3.rbm_layers[0].visible_groups.host.tolist() == [0, 3, 6, 9, 12]


# ------------------------------------------------------------------------------------------------------------------ calls
@pytest.mark.parametrize("mode,between", [("plain", []), ("centered", ["center_offsets", "center_hidden_rows", "center_stats"]),
                                          ("sparse", ["sparsity_activity", "sparsity_stats"]),
                                          ("both", ["sparsity_activity", "sparsity_stats", "center_offsets", "center_hidden_rows",
                                                    "center_stats"]),
                                          ("both_bias", ["sparsity_activity", "sparsity_stats", "center_offsets",
                                                         "center_hidden_rows", "center_stats"])])
def test_a_grouped_plan_makes_these_calls_in_this_order(mode, between):
    fn, rbm, log, batches, inner, _ = make(mode)
    for b in batches:
        fn(indexes=b, momentum=0.5)
        assert take(log) == ["cd_step_grouped"] + between + ["apply_update"]
    assert fn.plan.grouped is rbm.visible_groups
    assert rbm._n_updates == len(batches) and rbm._rng_step == len(batches)


def test_the_default_plan_is_unchanged():
    fn, rbm, log, batches, inner, _ = make("plain", groups=None)
    for b in batches:
        fn(indexes=b, momentum=0.5)
        assert take(log) == ["cd_train_step"]
    assert fn.plan.grouped is None and rbm.visible_groups is None
    fn, rbm, log, batches, inner, _ = make("centered", groups=None)
    fn(indexes=batches[0], momentum=0.5)
    assert take(log) == ["cd_step", "center_offsets", "center_stats", "apply_update"]
    fn, rbm, log, batches, inner, _ = make("plain", groups=None, persistent=True)
    fn(indexes=batches[0], momentum=0.5)
    assert take(log) == ["cd_step", "free_energy", "free_energy", "apply_update"] and rbm.bit_i_idx == 1


def test_pcd_reports_the_cross_entropy_and_keeps_its_chain():
    fn, rbm, log, batches, inner, data = make("plain", persistent=True, k=1)
    s = rbm_np.RBMState(V, H, W=rbm.W.tensor.numpy(), hbias=rbm.hbias.tensor.numpy(), vbias=rbm.vbias.tensor.numpy())
    chain0 = fn.plan.persistent.get_value().astype(np.float64)
    cost = float(fn(indexes=batches[0], momentum=0.5))
    assert take(log) == ["cd_step_grouped", "apply_update"] and rbm.bit_i_idx == 0     # no pseudo-likelihood pass
    v0 = data[batches[0]]
    _, _, out, _ = sm.cd_chain(s, v0, PhiloxDraws(rbm.theano_rng.seed, rbm.stream_id, 0, 0), 1, BOUNDS, persistent=chain0)
    assert np.isclose(cost, sm.grouped_cost(out[0], v0, BOUNDS) / 10.0, rtol=1e-12) and cost > 0.0
    assert np.array_equal(fn.plan.persistent.get_value(), out[5].astype(np.float32))
    with pytest.raises(ValueError):
        fn(indexes=batches[2], momentum=0.5)                    # 7 rows against a 10-row chain: as the plain PCD step


# ------------------------------------------------------------------------------------------------------------------ results
@pytest.mark.parametrize("mode", ["plain", "centered", "sparse", "both", "both_bias"])
def test_six_steps_equal_a_hand_written_float64_loop(mode):
    fn, rbm, log, batches, inner, data = make(mode)
    s = rbm_np.RBMState(V, H, W=rbm.W.tensor.numpy(), hbias=rbm.hbias.tensor.numpy(), vbias=rbm.vbias.tensor.numpy())
    s.freeze_W0()
    state, costs, want = None, [], []
    for t, b in enumerate(batches):
        momentum, lr = (0.5 if t < 3 else 0.9), (0.05 if t % 2 else 0.02)
        costs.append(float(fn(indexes=b, momentum=momentum, lr=lr)))
        v0 = data[b]
        ph, _, out, _ = sm.cd_chain(s, v0, PhiloxDraws(rbm.theano_rng.seed, rbm.stream_id, t, 0), 2, BOUNDS)
        for lo, hi in sm.spans(BOUNDS):
            assert (out[2][:, lo:hi].sum(axis=1) == 1).all()
        want.append(sm.grouped_cost(out[0], v0, BOUNDS) / len(b))
        state = sm.update(s, state, v0, ph, out[1], out[4], 10, lr, mode=mode, momentum=momentum, weightcost=2e-4)
    for name in PARAMS:
        assert np.abs(getattr(rbm, name).tensor.numpy() - getattr(s, name)).max() < 1e-12, name
    assert np.allclose(costs, want, rtol=1e-12)
    assert inner.keep_seen == [True] * len(batches)
    # ... and differ from the same layer without groups (the softmax is not a no-op)
    plain, prbm = make(mode, groups=None)[:2]
    for t, b in enumerate(batches):
        plain(indexes=b, momentum=0.5 if t < 3 else 0.9, lr=0.05 if t % 2 else 0.02)
    assert np.abs(prbm.W.tensor.numpy() - rbm.W.tensor.numpy()).max() > 1e-6


# ------------------------------------------------------------------------------------------------------------------ minibatch forms
def run_forms(mode, batches, hint=False):
    """Six steps of ``make(mode)`` on the index lists ``batches`` (any form), then the float64 loop on the same lists.
    -> (costs, parameters and speeds, the layer, the twin's state, the twin's costs)"""
    import torch
    fn, rbm, log, _, inner, data = make(mode)
    s = rbm_np.RBMState(V, H, W=rbm.W.tensor.numpy(), hbias=rbm.hbias.tensor.numpy(), vbias=rbm.vbias.tensor.numpy())
    s.freeze_W0()
    state, costs, want = None, [], []
    for t, b in enumerate(batches):
        momentum, lr = (0.5 if t < 3 else 0.9), (0.05 if t % 2 else 0.02)
        extra = dict(next_indexes=batches[t + 1]) if hint and t + 1 < len(batches) else {}
        costs.append(float(fn(indexes=b, momentum=momentum, lr=lr, **extra)))
        rows = np.asarray(b.cpu() if isinstance(b, torch.Tensor) else b)
        v0 = data[rows]
        ph, _, out, _ = sm.cd_chain(s, v0, PhiloxDraws(rbm.theano_rng.seed, rbm.stream_id, t, 0), 2, BOUNDS)
        want.append(sm.grouped_cost(out[0], v0, BOUNDS) / len(rows))
        state = sm.update(s, state, v0, ph, out[1], out[4], 10, lr, mode=mode, momentum=momentum, weightcost=2e-4)
    return costs, [getattr(rbm, name).tensor.numpy().copy() for name in PARAMS], rbm, s, want


@pytest.mark.parametrize("mode", ["plain", "both"])
def test_the_hint_of_the_next_minibatch_changes_nothing_on_a_ragged_schedule(mode):
    _, batches = problem()                                      # 10, 10, 7, 10, 1, 10 rows at batch_size 10
    plain, hinted = run_forms(mode, batches), run_forms(mode, batches, hint=True)
    assert plain[0] == hinted[0] and all(np.array_equal(a, b) for a, b in zip(plain[1], hinted[1]))
    for name, got in zip(PARAMS, hinted[1]):
        assert np.abs(got - getattr(hinted[3], name)).max() < 1e-12, name
    assert np.allclose(hinted[0], hinted[4], rtol=1e-12)


def test_index_forms_int32_int64_and_a_repeated_row():
    import torch
    _, batches = problem()
    forms = {"int64": [torch.from_numpy(b) for b in batches],
             "int32": [torch.from_numpy(b.astype(np.int32)) for b in batches],
             "list": [[int(i) for i in b[:-1]] + [int(b[0])] if len(b) > 1 else [int(b[0])] for b in batches]}
    res = {form: run_forms("plain", idx) for form, idx in forms.items()}
    for form, (costs, params, rbm, s, want) in res.items():
        assert np.allclose(costs, want, rtol=1e-12), form
        for name, got in zip(PARAMS, params):
            assert np.abs(got - getattr(s, name)).max() < 1e-12, (form, name)
    assert res["int32"][0] == res["int64"][0] and all(np.array_equal(a, b) for a, b in zip(res["int32"][1], res["int64"][1]))
    assert res["list"][0] != res["int64"][0]


# ------------------------------------------------------------------------------------------------------------------ refused
def test_every_refused_combination_raises():
    eng = sm.GroupedOracle()
    rbm = layer(eng)
    data, _ = problem()
    shared = mdbn_amd.shared(data, engine=eng)
    _, up = rbm.get_cost_updates(lr=0.05, batch_size=10)
    with pytest.raises(NotImplementedError, match="visible_groups"):
        mdbn_amd.function(up, shared, data_parallel=FakeGroup())
    with pytest.raises(NotImplementedError, match="visible_groups"):
        rbm.get_cost_updates(lr=0.05, batch_size=10, symbolic_grad=True)
    mask = np.zeros(V)
    for call in (lambda: rbm.log_partition(n_chains=4, n_betas=4), lambda: rbm.log_likelihood(data, n_chains=4, n_betas=4),
                 lambda: rbm.check_log_partition(), lambda: rbm.tempered_chains(2), lambda: rbm.sample_tempered(2, n_sweeps=2, burn_in=0),
                 lambda: rbm.gibbs_vhv_clamped(data[:2], mask, 2), lambda: rbm.impute(data[:2], mask, n_steps=2, burn_in=0),
                 lambda: rbm.conditional_log_partition(data[:2], mask), lambda: rbm.conditional_log_likelihood(data[:2], mask),
                 lambda: rbm.training(data, None, 1, batch_size=10, tempering=3)):
        with pytest.raises(NotImplementedError, match="visible_groups"):
            call()
    assert rbm._rng_step == 0                                                          # refused before anything was drawn
    mdbn_amd.DBN.verbose = False
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, gauss=False, hidden_layers_sizes=[H], n_outs=4, engine=eng,
                       visible_groups=BOUNDS)
    with pytest.raises(NotImplementedError, match="visible_groups"):
        net.log_likelihood_bound(data[:4], n_samples=2)
    with pytest.raises(NotImplementedError, match="visible_groups"):
        net.fine_tune(data, 1, batch_size=10, lr=0.01)
    # the Gaussian layer has no groups; bad tables are refused where they are given
    with pytest.raises(ValueError, match="GRBM"):
        mdbn_amd.GRBM(n_visible=V, n_hidden=H, engine=eng, visible_groups=3)
    with pytest.raises(ValueError, match="GRBM"):
        mdbn_amd.GRBM(n_visible=V, n_hidden=H, engine=eng).training(data, None, 1, visible_groups=3)
    for bad in (5, 1, 65, [0, 1, 4], [0, 3, 3], [4, 2], [0, 13], [-1, 3], [3], [0.0, 3.0], [0, 70], True):
        with pytest.raises(ValueError):
            layer(eng, bad)
    with pytest.raises(ValueError):
        layer(eng, 65, n_visible=130)
    assert layer(eng, 64, n_visible=128).visible_groups.n_groups == 2
    with pytest.raises(ValueError, match="visible_groups"):
        layer(eng, None).group_posterior(data, 0)
    # a layer without groups: none of this is refused, nothing is marked
    plain = layer(eng, None)
    _, plan = plain.get_cost_updates(lr=0.05, batch_size=10, symbolic_grad=True)
    assert plan.grouped is None and mdbn_amd.function(plan, shared, data_parallel=FakeGroup()).plan.grouped is None


# ------------------------------------------------------------------------------------------------------------------ trainers
def test_the_trainers_pass_the_keyword_down():
    mdbn_amd.DBN.verbose = False
    eng = sm.GroupedOracle()
    data, _ = problem()
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, gauss=False, hidden_layers_sizes=[H], n_outs=4, engine=eng)
    net.data_parallel = None
    net.shuffle_rng = np.random.RandomState(3)
    net.training(data, batch_size=10, k=1, pretraining_epochs=[2, 2], pretrain_lr=[0.05, 0.05], visible_groups=BOUNDS)
    assert net.rbm_layers[0].visible_groups.host.tolist() == BOUNDS and net.rbm_layers[1].visible_groups is None
    assert [f.plan.grouped is not None for f in net.training_functions(data, batch_size=10, k=1)[0]] == [True, False]
    for extra in (dict(persistent=False), dict(persistent=True), dict(persistent=False, centered=True)):
        r = layer(eng, None)
        hist = r.training(data, None, 1, batch_size=10, visible_groups=BOUNDS, **extra)
        assert r.visible_groups.host.tolist() == BOUNDS and hist[0][0] > 0.0           # a cross-entropy, under PCD too
    from mdbn_amd import MDBN
    for f, before in ((MDBN.train_bottom_layer, "graph_output"), (MDBN.train_top, "rng"), (mdbn_amd.RBM.training, "tempering"),
                      (mdbn_amd.GRBM.training, "graph_output"), (mdbn_amd.DBN.training, "on_step")):
        names = list(inspect.signature(f).parameters)
        assert names[names.index("visible_groups") - 1] == before, f.__qualname__
        assert inspect.signature(f).parameters["visible_groups"].default is None
    prev = mdbn_amd.set_engine(eng)
    try:
        net2, out, _ = MDBN.train_bottom_layer(data, None, batch_size=10, layers_sizes=[4], pretraining_epochs=[1], pretrain_lr=[0.05],
                                               rng=np.random.RandomState(2), visible_groups=BOUNDS)
        assert not net2.rbm_layers[0].gauss and net2.rbm_layers[0].visible_groups.host.tolist() == BOUNDS and out.shape == (N, 4)
        assert MDBN.build_bottom_layer(V, [4], np.random.RandomState(2)).rbm_layers[0].gauss
    finally:
        import mdbn_amd.engine as E
        E._default_engine = None


# ------------------------------------------------------------------------------------------------------------------ checkpoint
def test_checkpoint_round_trip_keeps_the_table(tmp_path):
    mdbn_amd.DBN.verbose = False
    eng = sm.GroupedOracle()
    data, _ = problem()
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, gauss=False, hidden_layers_sizes=[], n_outs=H, engine=eng,
                       visible_groups=BOUNDS)
    rbm = net.rbm_layers[0]
    _, up = rbm.get_cost_updates(0.05, k=1, batch_size=10)
    fn = mdbn_amd.function(up, mdbn_amd.shared(data, engine=eng), data_parallel=None)
    for t in range(2):
        fn(indexes=np.arange(10) + 10 * t, momentum=0.5)
    path = str(tmp_path / "grouped.npz")
    checkpoint.save_network(path, {'cn': net}, resume=True)
    assert np.load(path, allow_pickle=True)['cn_config'].tolist()['visible_groups'] == BOUNDS
    want = [float(fn(indexes=np.arange(10) + 10 * t, momentum=0.5)) for t in (2, 3)]
    r2 = checkpoint.load_network(path, engine=eng)['cn'].rbm_layers[0]
    assert r2.visible_groups.host.tolist() == BOUNDS and r2.visible_groups.tensor.tolist() == BOUNDS and not r2.gauss
    _, up2 = r2.get_cost_updates(0.05, k=1, batch_size=10)
    fn2 = mdbn_amd.function(up2, mdbn_amd.shared(data, engine=eng), data_parallel=None)
    got = [float(fn2(indexes=np.arange(10) + 10 * t, momentum=0.5)) for t in (2, 3)]
    np.testing.assert_allclose(got, want, rtol=1e-5)            # (float64 checker, float32 file: equal to rounding)
    # a file without a table loads as before
    plain = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, gauss=False, hidden_layers_sizes=[], n_outs=H, engine=eng)
    checkpoint.save_network(path, {'cn': plain}, resume=True)
    assert 'visible_groups' not in np.load(path, allow_pickle=True)['cn_config'].tolist()
    assert checkpoint.load_network(path, engine=eng)['cn'].rbm_layers[0].visible_groups is None


# ------------------------------------------------------------------------------------------------------------------ utils
def test_one_hot_groups():
    codes = np.array([[0, 4], [2, 1], [4, 4]])
    x = utils.one_hot_groups(codes, 5)
    assert x.dtype == np.float32 and x.shape == (3, 10)
    assert x.tolist() == [[1, 0, 0, 0, 0, 0, 0, 0, 0, 1], [0, 0, 1, 0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0, 0, 0, 1]]
    assert np.array_equal(x.reshape(3, 2, 5).argmax(axis=2), codes)
    assert utils.one_hot_groups(np.zeros((0, 3), dtype=np.int32), 4).shape == (0, 12)
    for bad, K in ((np.array([[0, 5]]), 5), (np.array([[-1, 0]]), 5), (np.array([[0.0, 1.0]]), 5), (np.array([0, 1]), 5), (codes, 1)):
        with pytest.raises(ValueError):
            utils.one_hot_groups(bad, K)
    assert utils.group_boundaries(5, 20).tolist() == [0, 5, 10, 15, 20] and utils.group_boundaries([1, 3, 67, 70], 70).dtype == np.int32


# ------------------------------------------------------------------------------------------------------------------ tie cap
@pytest.mark.parametrize("V_,ldv,bounds,B", sm.KERNEL_CASES, ids=["%dx%d" % (c[3], c[0]) for c in sm.KERNEL_CASES])
def test_the_tie_cap_holds_for_the_reference_alone(V_, ldv, bounds, B):
    """The kernel cases of tests/test_gpu_softmax.py, same host-made pre-activations and Philox address: the twin alone has
    at most TIE_CAP draws within the means' bound of a boundary, so more than that on the device is the kernel's doing."""
    pre, v0, U, seed = sm.case_inputs(V_, ldv, bounds, B)
    mean = sm.grouped_softmax(pre, bounds)[0]
    n = sm.tie_draws(mean, bounds, U)
    print("B = %d, V = %d, seed %d: %d draws near a boundary" % (B, V_, seed, n))
    assert n <= sm.TIE_CAP
    # (the inputs are what the docstring says: finite costs at +-80, valid targets)
    assert np.isfinite(sm.grouped_cost(pre, v0, bounds))
    for lo, hi in sm.spans(bounds):
        assert (v0[:, lo:hi].sum(axis=1) == 1).all()
