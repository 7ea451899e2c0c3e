"""The sparsity target through the public classes on the CPU checker engine: the C-ABI names, the engine calls a sparse plan
makes and their order (alone and with the centred gradient), the schedule of the rates and scales, six steps against a
hand-written float64 loop, what is refused, the trainers, the checkpoint round trip and RBM.hidden_activity.  Shapes of
tests/test_center_api.py: the smallest with a ragged and a one-row minibatch."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _center_np as cn
import _sparsity_np as sn
import mdbn_amd
from mdbn_amd import MDBN, _lib, checkpoint
from _oracle_engine import OracleEngine
from oracle import rbm_np
from oracle.philox_np import PhiloxDraws

V, H, N = 12, 7, 40
SIZES = (10, 10, 7, 10, 1, 10)
NAMES = ("mdbn_sparsity_activity", "mdbn_sparsity_stats")
LOGGED = ("cd_step", "cd_forward", "cd_statistics", "cd_train_step", "apply_update", "center_offsets", "center_stats",
          "sparsity_activity", "sparsity_stats")
KEYWORDS = ["sparsity_target", "sparsity_cost", "sparsity_decay", "sparsity_weights"]
SPARSE = [("cd_step", None), ("sparsity_activity", None), ("sparsity_stats", None), ("apply_update", 0)]
SPARSE_CENTRED = SPARSE[:3] + [("center_offsets", None), ("center_stats", None), ("apply_update", 0)]


class SparsityOracle(OracleEngine):
    """The checker engine with the calls of the sparse and of the centred step, from the twins."""

    def __init__(self):
        OracleEngine.__init__(self)
        self.keep_seen, self.rates, self.scales, self.with_v, self.nus = [], [], [], [], []

    def cd_step(self, data, indexes, *args, **kw):
        self.keep_seen.append(kw.pop("keep_f32", None))
        stats, sc = OracleEngine.cd_step(self, data, indexes, *args, **kw)
        data = self.as_matrix(data)
        sc.V2 = data if indexes is None else data[self.index_tensor(indexes)]
        sc.P2 = self._t(sc.ph_mean)
        return stats, sc

    def sparsity_activity(self, scratch, B, q, v_mean, rate):
        assert scratch.P2.shape[0] == B
        self.rates.append(rate)
        self.with_v.append(v_mean is not None)
        q2, m = sn.activity(q.numpy(), scratch.V2.numpy() if v_mean is not None else None, scratch.P2.numpy(), rate)
        q.copy_(self._t(q2))
        self.last_q = q
        if v_mean is not None:
            assert scratch.V2.shape[0] == B
            v_mean.copy_(self._t(m))

    def sparsity_stats(self, stats, V, H, ldv, ldh, q, v_mean, target, w_scale, b_scale):
        self.scales.append((w_scale, b_scale))
        st = stats.numpy()
        S, s_h, s_v = sn.stats(st[:V * H].reshape(V, H), st[V * H:V * H + H], st[V * H + H:V * H + H + V], q.numpy(),
                               None if v_mean is None else v_mean.numpy(), target, w_scale, b_scale)
        stats[:V * H + H + V] = self._t(np.concatenate([S.ravel(), s_h, s_v]))
        return stats

    def center_offsets(self, scratch, B, mu, lam, nu):
        self.nus.append(nu)
        m, l = cn.center_offsets(mu.numpy(), lam.numpy(), scratch.V2.numpy(), scratch.P2.numpy(), nu)
        mu.copy_(self._t(m))
        lam.copy_(self._t(l))

    def center_stats(self, stats, V, H, ldv, ldh, mu, lam, row_scale):
        st = stats.numpy()
        S, s_h, s_v = cn.center_stats(st[:V * H].reshape(V, H), st[V * H:V * H + H], st[V * H + H:V * H + H + V],
                                      mu.numpy(), lam.numpy(), row_scale)
        stats[:V * H + H + V] = self._t(np.concatenate([S.ravel(), s_h, s_v]))
        return stats


class Recorder(object):
    """Proxy of an engine: logs (name, phase) of every step-level call, passes everything else through."""

    def __init__(self, engine, log):
        self._engine, self._log = engine, log

    def __getattr__(self, name):
        target = getattr(self._engine, name)
        if name not in LOGGED:
            return target

        def call(*args, **kw):
            phase = kw.get("phase", args[16] if len(args) > 16 else 0) if name == "apply_update" else None
            self._log.append((name, phase))
            return target(*args, **kw)
        return call


class FakeGroup(object):
    world_size, rank = 2, 0

    def shard(self, n):
        return (0, n)


def problem(gauss):
    rs = np.random.RandomState(0)
    data = rs.normal(size=(N, V)) if gauss else (rs.uniform(size=(N, V)) < 0.4).astype(np.float64)
    return data, [rs.permutation(N)[:n].astype(np.int64) for n in SIZES]


def hyper(gauss):
    return dict(lambda_2=0.1) if gauss else dict(weightcost=2e-4)


def make(gauss=1, sparse=True, centered=False, persistent=False, **kw):
    """-> (fn, rbm, log, batches, inner engine, data)"""
    log = []
    inner = SparsityOracle()
    eng = Recorder(inner, log)
    data, batches = problem(gauss)
    cls = mdbn_amd.GRBM if gauss else mdbn_amd.RBM
    rbm = cls(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(11), engine=eng)
    chain = np.zeros((10, H), dtype=np.float32) if persistent else None
    extra = dict(dict(sparsity_target=0.2, sparsity_cost=1.5), **kw) if sparse else dict(kw)
    if centered:
        extra["centered"] = True
    _, up = rbm.get_cost_updates(lr=0.05, k=2, batch_size=10, persistent=chain, **dict(hyper(gauss), **extra))
    fn = mdbn_amd.function(up, mdbn_amd.shared(data, engine=eng), data_parallel=None)
    del log[:]
    return fn, rbm, log, batches, inner, data


def take(log):
    out = list(log)
    del log[:]
    return out


def lrs(t):
    return 0.05 if t % 2 else 0.02


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_the_two_names_are_in_the_header_and_in_the_signatures():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mdbn_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name]) == 12, name
    from mdbn_amd import build
    assert "mdbn_sparsity.hip" in build.SOURCES


# ------------------------------------------------------------------------------------------------------------------ calls
@pytest.mark.parametrize("gauss", [1, 0])
def test_a_sparse_plan_makes_these_calls_in_this_order(gauss):
    fn, rbm, log, batches, inner, _ = make(gauss, sparsity_decay=0.75)
    for t, b in enumerate(batches):
        fn(indexes=b, momentum=0.5, lr=lrs(t))
        assert take(log) == SPARSE
    assert inner.keep_seen == [True] * len(batches)             # the float32 copies of v0 / ph_mean, for that call only
    assert inner.rates == [1.0] + [1.0 - 0.75] * (len(batches) - 1)
    # w_scale = cost * batch_size whatever the minibatch holds, b_scale = cost * n_rows
    assert inner.scales == [(1.5 * 10.0, 1.5 * float(n)) for n in SIZES]
    assert inner.with_v == [True] * len(batches)
    assert rbm._n_updates == len(batches) and rbm._rng_step == len(batches)
    assert rbm.v_offset is None and rbm.h_offset is None and rbm.h_activity.shape == (H,)


def test_the_bias_only_form_passes_no_visible_means_and_a_zero_weight_scale():
    fn, rbm, log, batches, inner, _ = make(0, sparsity_weights=False)
    for b in batches:
        fn(indexes=b, momentum=0.5)
        assert take(log) == SPARSE
    assert inner.with_v == [False] * len(batches)
    assert inner.scales == [(0.0, 1.5 * float(n)) for n in SIZES]
    assert inner.rates == [1.0] + [1.0 - 0.9] * (len(batches) - 1)              # the default decay


@pytest.mark.parametrize("gauss", [1, 0])
def test_sparse_and_centred_runs_the_sparsity_transform_first(gauss):
    fn, rbm, log, batches, inner, _ = make(gauss, centered=True)
    for b in batches:
        fn(indexes=b, momentum=0.5)
        assert take(log) == SPARSE_CENTRED
    assert inner.nus == [1.0] + [0.01] * (len(batches) - 1)
    assert rbm.v_offset is not None and rbm.h_activity is not None and rbm.h_activity is not rbm.h_offset


def test_a_centred_only_plan_and_a_plain_plan_call_what_they_called_before():
    fn, rbm, log, batches, inner, _ = make(1, sparse=False, centered=True)
    for b in batches:
        fn(indexes=b, momentum=0.5)
        assert take(log) == [("cd_step", None), ("center_offsets", None), ("center_stats", None), ("apply_update", 0)]
    assert rbm.h_activity is None and inner.rates == []
    # a plain plan; a target at cost 0 and a cost without a target are plain plans too
    for kw in ({}, dict(sparsity_target=0.2), dict(sparsity_cost=2.0), dict(sparsity_target=0.2, sparsity_cost=0.0)):
        fn, rbm, log, batches, inner, _ = make(1, sparse=False, **kw)
        assert not fn.plan.sparse
        for b in batches:
            fn(indexes=b, momentum=0.5)
            assert take(log) == [("cd_train_step", None)]
        assert rbm.h_activity is None and inner.rates == [] and inner.scales == []


def test_pcd_keeps_its_monitor_and_its_chain():
    fn, rbm, log, batches, inner, data = make(0, persistent=True)
    full = [b for b in batches if len(b) == 10]
    chain0 = fn.plan.persistent.get_value().copy()
    cost = fn(indexes=full[0], momentum=0.5)
    assert take(log) == SPARSE
    assert rbm.bit_i_idx == 1 and float(cost) < 0.0             # the pseudo-likelihood, not the update's cost slot
    assert not np.array_equal(fn.plan.persistent.get_value(), chain0)
    with pytest.raises(ValueError):
        fn(indexes=batches[2], momentum=0.5)                    # 7 rows against a 10-row chain: as the plain PCD step


def test_first_step_sets_the_estimate_to_the_batch_means_then_it_slides():
    fn, rbm, log, batches, inner, data = make(0, sparsity_decay=0.75)
    assert rbm.h_activity is None
    fn(indexes=batches[0], momentum=0.5)
    assert np.allclose(rbm.h_activity.get_value(), inner.last.ph_mean.mean(0), atol=1e-7)
    q0 = rbm.h_activity.get_value().astype(np.float64)
    fn(indexes=batches[1], momentum=0.5)
    assert np.allclose(rbm.h_activity.get_value(), q0 + 0.25 * (inner.last.ph_mean.mean(0) - q0), atol=1e-6)
    p = fn.plan
    assert p.sparse and (p.sparsity_target, p.sparsity_cost, p.sparsity_decay, p.sparsity_weights) == (0.2, 1.5, 0.75, True)
    assert make(1)[0].plan.sparsity_decay == 0.9


# ------------------------------------------------------------------------------------------------------------------ results
@pytest.mark.parametrize("weights", [True, False])
@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("gauss", [1, 0])
def test_six_steps_equal_a_hand_written_float64_loop(gauss, centered, weights):
    fn, rbm, log, batches, inner, data = make(gauss, centered=centered, sparsity_weights=weights)
    s = rbm_np.RBMState(V, H, W=rbm.W.tensor.numpy(), hbias=rbm.hbias.tensor.numpy(), vbias=rbm.vbias.tensor.numpy(), gauss=bool(gauss))
    s.freeze_W0()
    q = mu = lam = None
    costs, want = [], []
    for t, b in enumerate(batches):
        momentum = 0.5 if t < 3 else 0.9
        costs.append(float(fn(indexes=b, momentum=momentum, lr=lrs(t))))
        v0 = data[b]
        n = len(b)
        ph, _, out = rbm_np.cd_chain(s, v0, PhiloxDraws(rbm.theano_rng.seed, rbm.stream_id, t, 0), 2)
        nv, nh = out[1], out[4]
        want.append(rbm_np.reconstruction_cost(s, out[0], v0))
        # the step written out: estimate, penalty, (offsets, correction,) the reference's gradient rule
        q = ph.mean(0) if q is None else q + (1.0 - 0.9) * (ph.mean(0) - q)
        S = v0.T @ ph - nv.T @ nh
        s_h, s_v = (ph - nh).sum(0) + 1.5 * n * (0.2 - q), (v0 - nv).sum(0)
        if weights:
            S = S + 1.5 * 10 * np.outer(v0.mean(0), 0.2 - q)
        if centered:
            mu = v0.mean(0) if mu is None else mu + 0.01 * (v0.mean(0) - mu)
            lam = ph.mean(0) if lam is None else lam + 0.01 * (ph.mean(0) - lam)
            S = S - np.outer(mu, s_h) - np.outer(s_v, lam)
            s_h, s_v = s_h - (n / 10.0) * (S.T @ mu), s_v - (n / 10.0) * (S @ lam)
        g_W = S / 10.0 - hyper(gauss).get("weightcost", 0.0) * s.W0
        rbm_np.apply_update(s, g_W, s_h / n, s_v / n, lrs(t), 0.0, hyper(gauss).get("lambda_2", 0.0), momentum)
    for name in ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed"):
        assert np.abs(getattr(rbm, name).tensor.numpy() - getattr(s, name)).max() < 1e-12, name
    assert np.abs(rbm.h_activity.tensor.numpy() - q).max() < 1e-12
    if centered:
        assert np.abs(rbm.v_offset.tensor.numpy() - mu).max() < 1e-12 and np.abs(rbm.h_offset.tensor.numpy() - lam).max() < 1e-12
    assert np.allclose(costs, want, rtol=1e-12)
    # ... and differ from the same plan without the penalty (it is not a no-op)
    other, orbm = make(gauss, sparse=False, centered=centered)[:2]
    for t, b in enumerate(batches):
        other(indexes=b, momentum=0.5 if t < 3 else 0.9, lr=lrs(t))
    assert np.abs(orbm.hbias.tensor.numpy() - rbm.hbias.tensor.numpy()).max() > 1e-6


def test_the_twin_loop_is_the_same_step():
    """tests/_sparsity_np.sparse_update, which the GPU tests compare against, is the hand-written loop above."""
    fn, rbm, log, batches, inner, data = make(1, centered=True)
    s = rbm_np.RBMState(V, H, W=rbm.W.tensor.numpy(), gauss=True)
    state = None
    for t, b in enumerate(batches):
        fn(indexes=b, momentum=0.5, lr=lrs(t))
        ph, _, out = rbm_np.cd_chain(s, data[b], PhiloxDraws(rbm.theano_rng.seed, rbm.stream_id, t, 0), 2)
        state = sn.sparse_update(s, state, data[b], ph, out[1], out[4], 10, lrs(t), 0.2, 1.5, centered=True, momentum=0.5, lambda_2=0.1)
    assert np.abs(rbm.W.tensor.numpy() - s.W).max() < 1e-12 and np.abs(rbm.h_activity.tensor.numpy() - state["q"]).max() < 1e-12
    assert np.abs(rbm.v_offset.tensor.numpy() - state["offsets"][0]).max() < 1e-12


# ------------------------------------------------------------------------------------------------------------------ refused
def test_what_is_refused():
    eng = SparsityOracle()
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(11), engine=eng)
    sparse = dict(sparsity_target=0.2, sparsity_cost=1.0)
    _, up = rbm.get_cost_updates(lr=0.05, batch_size=10, **sparse)
    data = mdbn_amd.shared(problem(0)[0], engine=eng)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        mdbn_amd.function(up, data, data_parallel=FakeGroup())
    with pytest.raises(NotImplementedError, match="symbolic_grad"):
        rbm.get_cost_updates(lr=0.05, batch_size=10, symbolic_grad=True, **sparse)
    for bad in (dict(sparsity_target=0.0), dict(sparsity_target=1.0), dict(sparsity_target=-0.1), dict(sparsity_target=float("nan")),
                dict(sparsity_cost=-1.0), dict(sparsity_cost=float("nan")), dict(sparsity_decay=1.0), dict(sparsity_decay=-0.1),
                dict(sparsity_decay=float("nan"))):
        with pytest.raises(ValueError):
            rbm.get_cost_updates(lr=0.05, batch_size=10, **dict(sparse, **bad))
    # the plain plan on a group, and a plain symbolic_grad plan: as before
    _, plain = rbm.get_cost_updates(lr=0.05, batch_size=10)
    assert mdbn_amd.function(plain, data, data_parallel=FakeGroup()).plan.sparse is False
    assert rbm.get_cost_updates(lr=0.05, batch_size=10, symbolic_grad=True)[1].sparse is False
    assert rbm.get_cost_updates(lr=0.05, batch_size=10, sparsity_decay=0.0, **sparse)[1].sparsity_decay == 0.0


# ------------------------------------------------------------------------------------------------------------------ trainers
def test_the_trainers_pass_the_keywords_down():
    mdbn_amd.DBN.verbose = False
    eng = SparsityOracle()
    rs = np.random.RandomState(2)
    x = rs.normal(size=(30, V))
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[H], n_outs=4, engine=eng)
    net.data_parallel = None
    kw = dict(sparsity_target=0.1, sparsity_cost=2.0, sparsity_decay=0.95, sparsity_weights=False)
    fns, _ = net.training_functions(x, batch_size=10, k=1, **kw)
    for f in fns:
        assert f.plan.sparse and not f.plan.centered
        assert (f.plan.sparsity_target, f.plan.sparsity_cost, f.plan.sparsity_decay, f.plan.sparsity_weights) == (0.1, 2.0, 0.95, False)
    assert [f.plan.sparse for f in net.training_functions(x, batch_size=10, k=1)[0]] == [False, False]
    net.shuffle_rng = np.random.RandomState(3)
    net.training(x, batch_size=10, k=1, pretraining_epochs=[2, 2], pretrain_lr=[0.005, 0.1], centered=True, **kw)
    assert all(r.h_activity is not None and r.v_offset is not None for r in net.rbm_layers)
    assert [r.h_activity.shape for r in net.rbm_layers] == [(H,), (4,)]
    assert eng.rates[0] == 1.0 and set(eng.rates[1:3]) == {1.0 - 0.95} and not any(eng.with_v)
    for cls, extra in ((mdbn_amd.RBM, dict(persistent=False)), (mdbn_amd.RBM, dict(persistent=True)), (mdbn_amd.GRBM, {})):
        r = cls(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(11), engine=eng)
        data = x if cls is mdbn_amd.GRBM else (x > 0).astype(np.float64)
        r.training(data, None, 1, batch_size=10, sparsity_target=0.2, sparsity_cost=1.0, **extra)
        assert r.h_activity is not None and r.h_activity.shape == (H,) and r.v_offset is None
    for f in (MDBN.train_bottom_layer, MDBN.train_top):
        names = list(inspect.signature(f).parameters)
        assert names[-6:] == KEYWORDS + ["centered", "offset_rate"], f.__name__
    for f in (mdbn_amd.RBM.get_cost_updates, mdbn_amd.RBM.training, mdbn_amd.GRBM.training, mdbn_amd.DBN.training_functions,
              mdbn_amd.DBN.training):
        names = list(inspect.signature(f).parameters)
        assert names[-4:] == KEYWORDS and names[-6:-4] == ["centered", "offset_rate"], f.__qualname__
        defaults = [inspect.signature(f).parameters[k].default for k in KEYWORDS]
        assert defaults == [None, 0.0, 0.9, True], f.__qualname__


def test_the_mdbn_trainers_hand_the_keywords_to_every_layer(monkeypatch):
    seen = []

    def fake_training(self, *args, **kw):
        seen.append({k: kw.get(k) for k in KEYWORDS + ["centered"]})

    monkeypatch.setattr(mdbn_amd.DBN, "training", fake_training)
    monkeypatch.setattr(mdbn_amd.DBN, "get_output", lambda self, x, layer=-1: None)
    monkeypatch.setattr(mdbn_amd.DBN, "verbose", False)
    monkeypatch.setattr(MDBN, "shared", lambda x, **kw: np.asarray(x))

    class CheckerDBN(mdbn_amd.DBN):
        def __init__(self, **kw):
            mdbn_amd.DBN.__init__(self, engine=SparsityOracle(), **kw)

    monkeypatch.setattr(MDBN, "DBN", CheckerDBN)
    x = np.random.RandomState(0).normal(size=(20, V))
    kw = dict(sparsity_target=0.1, sparsity_cost=2.0, sparsity_decay=0.95, sparsity_weights=False)
    MDBN.train_bottom_layer(x, None, batch_size=10, layers_sizes=[H, 4], rng=np.random.RandomState(1), **kw)
    MDBN.train_top(10, False, x, None, np.random.RandomState(1), **kw)
    MDBN.train_modalities([dict(train_set=x, layers_sizes=[H, 4], batch_size=10, **kw), dict(train_set=x, layers_sizes=[4])],
                          np.random.RandomState(1), group=None)
    assert seen[:2] == [dict(kw, centered=False)] * 2 and seen[2] == dict(kw, centered=None)      # (train_modalities has no centred form)
    assert seen[3] == dict.fromkeys(KEYWORDS + ["centered"])     # a modality that names none of them: the trainer's defaults


# ------------------------------------------------------------------------------------------------------------------ checkpoint
def test_checkpoint_round_trip_keeps_the_activity_estimate(tmp_path):
    mdbn_amd.DBN.verbose = False
    eng = SparsityOracle()
    rs = np.random.RandomState(0)
    x = rs.normal(size=(40, V))
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[], n_outs=H, engine=eng)
    rbm = net.rbm_layers[0]
    plan = dict(k=1, lambda_2=0.1, batch_size=10, centered=True, sparsity_target=0.2, sparsity_cost=1.0)
    _, up = rbm.get_cost_updates(0.005, **plan)
    fn = mdbn_amd.function(up, mdbn_amd.shared(x, engine=eng), data_parallel=None)
    for t in range(2):
        fn(indexes=np.arange(10) + 10 * t, momentum=0.5)
    path = str(tmp_path / "sparse.npz")
    checkpoint.save_network(path, {'ge': net}, resume=True)
    want = [float(fn(indexes=np.arange(10) + 10 * t, momentum=0.5)) for t in (2, 3)]
    r2 = checkpoint.load_network(path, engine=eng)['ge'].rbm_layers[0]
    saved = np.load(path, allow_pickle=True)['ge_resume'][0]
    assert saved['h_activity'].dtype == np.float32 and saved['h_activity'].shape == (H,)
    assert np.array_equal(r2.h_activity.get_value(), saved['h_activity']) and r2.h_activity.shape == (H,)
    assert r2.v_offset is not None
    n_first = len(eng.rates)
    _, up2 = r2.get_cost_updates(0.005, **plan)
    fn2 = mdbn_amd.function(up2, mdbn_amd.shared(x, engine=eng), data_parallel=None)
    got = [float(fn2(indexes=np.arange(10) + 10 * t, momentum=0.5)) for t in (2, 3)]
    assert eng.rates[n_first:] == [1.0 - 0.9] * 2               # a restored layer goes on sliding: no second initialisation
    # (the checker computes in float64 while a checkpoint holds float32: equal to rounding; exact on the HIP engine)
    np.testing.assert_allclose(got, want, rtol=1e-5)
    np.testing.assert_allclose(r2.W.get_value(), rbm.W.get_value(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(r2.h_activity.get_value(), rbm.h_activity.get_value(), rtol=1e-5, atol=1e-7)
    # a plain checkpoint holds no such key and loads as before
    plain = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[], n_outs=H, engine=eng)
    checkpoint.save_network(path, {'ge': plain}, resume=True)
    assert 'h_activity' not in np.load(path, allow_pickle=True)['ge_resume'][0]
    assert checkpoint.load_network(path, engine=eng)['ge'].rbm_layers[0].h_activity is None


# ------------------------------------------------------------------------------------------------------------------ hidden_activity
def test_hidden_activity_over_uneven_chunks_is_the_one_shot_mean():
    eng = SparsityOracle()
    rs = np.random.RandomState(4)
    x = rs.normal(size=(23, V))
    for cls in (mdbn_amd.RBM, mdbn_amd.GRBM):
        rbm = cls(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(11), engine=eng)
        rbm.hbias.set_value(rs.normal(size=H).astype(np.float32))
        step0 = rbm._rng_step
        del eng.rates[:]
        got = rbm.hidden_activity(x, chunk_rows=10)             # chunks of 10, 10 and 3 rows
        assert eng.rates == [1.0, 10.0 / 20.0, 3.0 / 23.0] and not any(eng.with_v)
        assert got.dtype == np.float32 and got.shape == (H,) and rbm._rng_step == step0
        want = rbm_np.sigmoid(x @ rbm.W.get_value().astype(np.float64) + rbm.hbias.get_value().astype(np.float64)).mean(0)
        # the accumulator of the checker engine is float64 (the result is handed back as float32): the running mean over
        # the chunks is the mean over all rows
        assert np.abs(eng.last_q.numpy() - want).max() < 1e-12
        assert np.array_equal(got, eng.last_q.numpy().astype(np.float32))
        with pytest.raises(ValueError):
            rbm.hidden_activity(np.zeros((0, V)))
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[H], n_outs=4, engine=eng)
    acts = net.hidden_activity(x)
    assert [a.shape for a in acts] == [(H,), (4,)]
    h1 = rbm_np.sigmoid(x @ net.rbm_layers[0].W.get_value().astype(np.float64) + net.rbm_layers[0].hbias.get_value())
    h2 = rbm_np.sigmoid(h1 @ net.rbm_layers[1].W.get_value().astype(np.float64) + net.rbm_layers[1].hbias.get_value())
    assert np.abs(acts[0] - h1.mean(0)).max() < 1e-7 and np.abs(acts[1] - h2.mean(0)).max() < 1e-7
