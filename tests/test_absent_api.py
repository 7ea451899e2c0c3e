"""Training on tables with missing entries, host logic on the checker engine (tests/_absent_np.AbsentOracle: the absent-unit
calls from the float64 twin): every refusal, the keyword through the trainers, ``get_output(missing=True)``,
``MDBN.train_joint``, and that a plan without ``missing`` is the plan of before."""
import numpy as np
import pytest

import mdbn_amd
from mdbn_amd import MDBN
import _absent_np as an
from _oracle_engine import OracleEngine
from oracle import rbm_np
from oracle.philox_np import PhiloxDraws

V, H, N = 12, 5, 40


def problem(seed=0, gauss=False, holes=True):
    rs = np.random.RandomState(seed)
    x = rs.normal(size=(N, V)).astype(np.float32) if gauss else (rs.uniform(size=(N, V)) < 0.4).astype(np.float32)
    if holes:
        x[rs.uniform(size=(N, V)) < 0.25] = np.nan
        x[3, :] = np.nan
    return x


def layer(eng, cls=mdbn_amd.RBM, **kw):
    return cls(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(11), engine=eng, **kw)


class FakeGroup(object):
    world_size, rank = 2, 0

    def shard(self, n):
        return 0, n // 2


def test_every_refusal_comes_before_anything_runs():
    eng = an.AbsentOracle()
    rbm, data = layer(eng), problem()
    kw = dict(lr=0.05, batch_size=10, missing=True)
    with pytest.raises(NotImplementedError, match="visible_groups"):
        layer(eng, visible_groups=[0, 3, 6]).get_cost_updates(**kw)
    sig = layer(eng, mdbn_amd.GRBM)
    sig.set_sigma(1.0)
    with pytest.raises(NotImplementedError, match="log_sigma"):
        sig.get_cost_updates(**kw)
    with pytest.raises(NotImplementedError, match="log_sigma"):
        layer(eng, mdbn_amd.GRBM).get_cost_updates(learn_sigma=0.01, **kw)
    with pytest.raises(NotImplementedError, match="centered"):
        rbm.get_cost_updates(centered=True, **kw)
    with pytest.raises(NotImplementedError, match="sparsity"):
        rbm.get_cost_updates(sparsity_target=0.1, sparsity_cost=0.05, **kw)
    with pytest.raises(NotImplementedError, match="discriminative"):
        rbm.get_cost_updates(discriminative=1.0, **kw)
    with pytest.raises(NotImplementedError, match="symbolic_grad"):
        rbm.get_cost_updates(symbolic_grad=True, **kw)
    with pytest.raises(NotImplementedError, match="persistent"):
        rbm.get_cost_updates(persistent=np.zeros((10, H), dtype=np.float32), **kw)
    with pytest.raises(NotImplementedError, match="persistent"):
        rbm.training(data, None, 1, batch_size=10, missing=True)                    # (persistent defaults to True)
    with pytest.raises(NotImplementedError, match="tempering"):
        rbm.training(data, None, 1, batch_size=10, missing=True, persistent=False, tempering=4)
    with pytest.raises(NotImplementedError, match="cd_step_absent"):
        layer(OracleEngine()).get_cost_updates(**kw)
    _, up = rbm.get_cost_updates(**kw)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        mdbn_amd.function(up, mdbn_amd.shared(data, engine=eng), data_parallel=FakeGroup())
    up.rbm = layer(OracleEngine())                                                  # (a plan handed to a layer of another engine)
    with pytest.raises(NotImplementedError, match="cd_step_absent"):
        mdbn_amd.function(up, mdbn_amd.shared(data, engine=OracleEngine()), data_parallel=None)
    for r in (rbm, sig):
        assert r._rng_step == 0 and r._n_updates == 0
    assert eng.calls == []
    # a sparsity target at cost 0 is no sparsity target
    rbm.get_cost_updates(sparsity_target=0.1, sparsity_cost=0.0, **kw)


def test_without_the_keyword_the_plan_and_the_calls_are_those_of_before():
    eng = an.AbsentOracle()
    data = problem(holes=False)
    a, b = layer(eng), layer(eng)
    _, plain = a.get_cost_updates(lr=0.05, batch_size=10, weightcost=2e-4)
    _, off = b.get_cost_updates(lr=0.05, batch_size=10, weightcost=2e-4, missing=False)
    assert plain.absent is False and off.absent is False
    skip = ("rbm", "W0")
    assert {k: v for k, v in vars(plain).items() if k not in skip} == {k: v for k, v in vars(off).items() if k not in skip}
    log = []
    for name in ("cd_step", "cd_train_step", "apply_update"):
        def wrap(*args, _f=getattr(eng, name), _n=name, **kw):
            log.append(_n)
            return _f(*args, **kw)
        setattr(eng, name, wrap)
    fa = mdbn_amd.function(plain, mdbn_amd.shared(data, engine=eng), data_parallel=None)
    fb = mdbn_amd.function(off, mdbn_amd.shared(data, engine=eng), data_parallel=None)
    for t in range(3):
        ca, cb = fa(indexes=np.arange(10) + 10 * t, momentum=0.5), fb(indexes=np.arange(10) + 10 * t, momentum=0.5)
        assert float(ca) == float(cb)
    for n in ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed"):
        assert np.array_equal(getattr(a, n).get_value(), getattr(b, n).get_value()), n
    # the single-device path: one train-step call per step (tests/test_step_function_paths.py), none of the new calls
    assert [n for n in log if n == "cd_train_step"] == ["cd_train_step"] * 6 and eng.calls == []
    # ... and a NaN in the table then runs straight through, as before
    bad = problem()
    fc = mdbn_amd.function(layer(eng).get_cost_updates(lr=0.05, batch_size=10)[1], mdbn_amd.shared(bad, engine=eng), data_parallel=None)
    assert np.isnan(float(fc(indexes=np.arange(10), momentum=0.0))) and eng.calls == []


@pytest.mark.parametrize("gauss", [False, True], ids=["bernoulli", "gauss"])
def test_a_step_applies_the_twins_statistics(gauss):
    eng = an.AbsentOracle()
    cls = mdbn_amd.GRBM if gauss else mdbn_amd.RBM
    rbm, data = layer(eng, cls), problem(gauss=gauss)
    s = rbm_np.RBMState(V, H, W=rbm.W.get_value(), hbias=rbm.hbias.get_value(), vbias=rbm.vbias.get_value(), gauss=gauss)
    _, up = rbm.get_cost_updates(lr=0.05, batch_size=10, k=2, missing=True)
    assert up.absent is True
    fn = mdbn_amd.function(up, mdbn_amd.shared(data, engine=eng), data_parallel=None)
    idx = np.arange(10)                       # (holds the wholly-absent row 3)
    for t in range(2):
        S, s_h, s_v, c, _ = an.cd_step_absent(s, data[idx].astype(np.float64),
                                              PhiloxDraws(rbm.theano_rng.seed, rbm.stream_id, t, 0), 2)
        cost = float(fn(indexes=idx, momentum=0.5))
        g = rbm_np.rbm_grad(s, S, s_h, s_v, 10, 10, 0.0)        # the divisors stay the batch size
        rbm_np.apply_update(s, g[0], g[1], g[2], 0.05, 0.0, 0.0, 0.5)
        scale = 1.0 / (10 * V) if gauss else 1.0 / 10
        assert abs(cost - c * scale) <= 1e-9 * max(1.0, abs(cost))
        for n in ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed"):
            assert np.abs(getattr(rbm, n).get_value() - getattr(s, n)).max() <= 1e-6, (n, t)
    assert eng.calls == ["cd_step_absent"] * 2 and rbm._rng_step == 2


def test_eager_calls():
    eng = an.AbsentOracle()
    rbm, data = layer(eng), problem()
    s = rbm_np.RBMState(V, H, W=rbm.W.get_value(), hbias=rbm.hbias.get_value(), vbias=rbm.vbias.get_value())
    F = rbm.free_energy(data, missing=True).get_value()
    assert np.abs(F - an.free_energy_absent(s, data.astype(np.float64))).max() <= 1e-5
    filled = np.where(np.isnan(data), 0.0, data)
    assert np.array_equal(rbm.propup(data, missing=True)[1].get_value(), rbm.propup(filled)[1].get_value())
    assert np.isnan(rbm.propup(data)[1].get_value()).any()
    step = rbm._rng_step
    a = rbm.sample_h_given_v(data, missing=True)[2].get_value()
    rbm._rng_step = step
    assert np.array_equal(a, rbm.sample_h_given_v(filled)[2].get_value())
    gap = rbm.free_energy_gap(data[:20], data[20:], missing=True)
    want = an.free_energy_absent(s, data[20:].astype(np.float64)).mean() - an.free_energy_absent(s, data[:20].astype(np.float64)).mean()
    assert abs(gap - want) <= 1e-5
    with pytest.raises(NotImplementedError, match="visible_groups"):
        layer(eng, visible_groups=[0, 3, 6]).free_energy(data, missing=True)


def _net(eng, gauss=False, n_ins=V):
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=n_ins, gauss=gauss, hidden_layers_sizes=[H], n_outs=4, engine=eng)
    net.data_parallel = None
    net.shuffle_rng = np.random.RandomState(3)
    return net


def test_get_output_marks_exactly_the_wholly_absent_rows():
    mdbn_amd.DBN.verbose = False
    eng = an.AbsentOracle()
    net, data = _net(eng), problem()
    data[7, :] = np.nan
    data[8, 0], data[8, 1:] = 1.0, np.nan                       # one observed entry: not an absent row
    for layer_i in (0, 1, -1):
        out = net.get_output(data, layer_i, missing=True)
        nan_rows = np.isnan(out).all(axis=1)
        assert np.flatnonzero(nan_rows).tolist() == [3, 7] and not np.isnan(out[~nan_rows]).any()
        seen = ~nan_rows
        assert np.array_equal(out[seen], net.get_output(np.where(np.isnan(data), 0.0, data)[seen], layer_i))
    assert np.isnan(net.get_output(data)).any(axis=1).sum() > 2           # (without the keyword: as before)


def test_the_trainers_pass_the_keyword_down():
    mdbn_amd.DBN.verbose = False
    eng = an.AbsentOracle()
    data = problem()
    r = layer(eng)
    hist = r.training(data, data[:8], 1, batch_size=10, persistent=False, missing=True)
    assert eng.calls.count("cd_step_absent") == N // 10 and eng.calls.count("free_energy_absent") == 2
    assert np.isfinite(hist[0][0]) and np.isfinite(hist[0][1])
    eng.calls = []
    g = layer(eng, mdbn_amd.GRBM)
    g.training(problem(gauss=True), None, 1, batch_size=10, missing=True)
    assert eng.calls == ["cd_step_absent"] * (N // 10)
    # DBN.training: every layer, the upper one on the activations of get_output(missing=True)
    for gauss in (False, True):
        eng.calls = []
        net = _net(eng, gauss)
        x = problem(gauss=gauss)
        plans = [f.plan for f in net.training_functions(x, batch_size=10, k=1, missing=True)[0]]
        assert [p.absent for p in plans] == [True, True]
        assert [f.plan.absent for f in net.training_functions(x, batch_size=10, k=1)[0]] == [False, False]
        eng.calls = []
        net.training(x, batch_size=10, k=1, pretraining_epochs=[2, 2], pretrain_lr=[0.01, 0.01], validation_set_x=x[:8], missing=True)
        # (the reference's early stopping compares the epoch budget with the iteration count: a layer ends after a few steps)
        steps = [r._n_updates for r in net.rbm_layers]
        assert min(steps) >= 1 and eng.calls.count("cd_step_absent") == sum(steps) and "absent_mark_rows" in eng.calls
        assert "cd_step" not in eng.calls and "free_energy_absent" in eng.calls
        assert all(np.isfinite(p.get_value()).all() for p in net.params)
        cached = net._lower_cache[1][2].numpy()
        assert np.flatnonzero(np.isnan(cached).all(axis=1)).tolist() == [3] and not np.isnan(np.delete(cached, 3, axis=0)).any()
    with pytest.raises(NotImplementedError, match="centered"):
        _net(eng).training(data, batch_size=10, k=1, pretraining_epochs=[1, 1], pretrain_lr=[0.01, 0.01], missing=True, centered=True)
    with pytest.raises(NotImplementedError, match="log_sigma"):
        _net(eng, True).training(data, batch_size=10, k=1, pretraining_epochs=[1, 1], pretrain_lr=[0.01, 0.01], missing=True,
                                 learn_sigma=0.01)


def test_train_joint_builds_the_nan_blocks_and_refuses_a_patient_with_nothing():
    mdbn_amd.DBN.verbose = False
    eng = an.AbsentOracle()
    mdbn_amd.set_engine(eng)
    saved = dict(MDBN.TOP_SHAPE), dict(MDBN.TOP_SCHEDULE)
    try:
        MDBN.TOP_SHAPE.update(hidden_layers_sizes=[H], n_outs=3)
        MDBN.TOP_SCHEDULE.update(pretraining_epochs=[1, 1], pretrain_lr=[0.05, 0.05])
        rs = np.random.RandomState(4)
        nets = [_net(eng, True, 6), _net(eng, True, 9), _net(eng, True, 5)]
        xs = [rs.normal(size=(N, n)).astype(np.float32) for n in (6, 9, 5)]
        xs[0][:5] = np.nan                      # patients 0-4 lack modality 0
        xs[1][5:9] = np.nan                     # patients 5-8 lack modality 1
        xs[1][20, 2:4] = np.nan                 # a hole inside a measured row: allowed
        table = MDBN.joint_table(nets, [xs[0], xs[1], None])
        assert table.shape == (N, 12) and table.dtype == np.float32
        nan = np.isnan(table)
        assert nan[:5, :4].all() and not nan[5:, :4].any()
        assert nan[5:9, 4:8].all() and not nan[:5, 4:8].any() and not nan[9:, 4:8].any()
        assert nan[:, 8:].all()
        full = xs[1].copy()
        full[20, 2:4] = 0.0
        assert np.array_equal(table[9:, 4:8], nets[1].get_output(full[9:]))
        eng.calls = []
        joint = MDBN.train_joint(nets, [xs[0], xs[1], xs[2]], 10, np.random.RandomState(2))
        steps = [r._n_updates for r in joint.rbm_layers]
        assert joint.n_ins == 12 and min(steps) >= 1 and eng.calls.count("cd_step_absent") == sum(steps)
        assert [type(r).__name__ for r in joint.rbm_layers] == ["RBM", "RBM"] and "cd_step" not in eng.calls
        assert all(np.isfinite(p.get_value()).all() for p in joint.params)
        xs[1][3:5] = np.nan                     # patients 3 and 4 now have nothing
        xs[2][3:5] = np.nan
        with pytest.raises(ValueError, match=r"2 patient\(s\) have no modality at all \(first: row 3\)"):
            MDBN.train_joint(nets, xs, 10, np.random.RandomState(2))
        with pytest.raises(ValueError, match="same number of rows"):
            MDBN.joint_table(nets, [xs[0][:10], xs[1], None])
    finally:
        MDBN.TOP_SHAPE.clear(); MDBN.TOP_SHAPE.update(saved[0])
        MDBN.TOP_SCHEDULE.clear(); MDBN.TOP_SCHEDULE.update(saved[1])
        import mdbn_amd.engine as E
        E._default_engine = None


def test_the_new_symbols_are_declared_and_bound():
    import os
    from mdbn_amd import _lib, build
    header = open(os.path.join(os.path.dirname(build.HERE), "include", "mdbn_hip.h")).read()
    for name in ("mdbn_absent_split", "mdbn_absent_visible_workspace_bytes", "mdbn_absent_visible", "mdbn_cd_step_absent_workspace_bytes",
                 "mdbn_cd_step_absent", "mdbn_absent_mark_rows", "mdbn_free_energy_absent_workspace_bytes", "mdbn_free_energy_absent"):
        assert name + "(" in header and name in _lib.SIGNATURES, name
    assert "mdbn_absent.hip" in build.SOURCES and "mdbn_drv_absent.hip" in build.SOURCES
