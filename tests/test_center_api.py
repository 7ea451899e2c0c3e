"""The centred step through the public classes on the CPU checker engine: the C-ABI names, the engine calls a centred plan
makes and their order, the offsets' schedule, six steps against a hand-written float64 loop, what is refused, and the
checkpoint round trip.  Shapes of tests/test_step_function_paths.py: the smallest with a ragged and a one-row minibatch."""
import os
import re

import numpy as np
import pytest
import torch

import _center_np as cn
import mdbn_amd
from mdbn_amd import _lib, checkpoint
from _oracle_engine import OracleEngine
from oracle import rbm_np
from oracle.philox_np import PhiloxDraws

V, H, N = 12, 7, 40
SIZES = (10, 10, 7, 10, 1, 10)
NAMES = ("mdbn_center_workspace_bytes", "mdbn_center_offsets", "mdbn_center_stats")
LOGGED = ("cd_step", "cd_forward", "cd_statistics", "cd_train_step", "apply_update", "center_offsets", "center_stats")


class CenterOracle(OracleEngine):
    """The checker engine with the two calls of the centred step, from the twin."""

    def __init__(self):
        OracleEngine.__init__(self)
        self.keep_seen, self.nus, self.rhos = [], [], []

    def cd_step(self, data, indexes, *args, **kw):
        self.keep_seen.append(kw.pop("keep_f32", None))
        stats, sc = OracleEngine.cd_step(self, data, indexes, *args, **kw)
        data = self.as_matrix(data)
        sc.v0 = (data if indexes is None else data[self.index_tensor(indexes)]).numpy()
        return stats, sc

    def center_offsets(self, scratch, B, mu, lam, nu):
        assert scratch.v0.shape[0] == B and scratch.ph_mean.shape[0] == B
        self.nus.append(nu)
        m, l = cn.center_offsets(mu.numpy(), lam.numpy(), scratch.v0, scratch.ph_mean, nu)
        mu.copy_(self._t(m))
        lam.copy_(self._t(l))

    def center_stats(self, stats, V, H, ldv, ldh, mu, lam, row_scale):
        self.rhos.append(row_scale)
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


def make(gauss=1, centered=True, persistent=False, **kw):
    """-> (fn, rbm, log, batches, inner engine, data)"""
    log = []
    inner = CenterOracle()
    eng = Recorder(inner, log)
    data, batches = problem(gauss)
    cls = mdbn_amd.GRBM if gauss else mdbn_amd.RBM
    rbm = cls(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(11), engine=eng)
    chain = np.zeros((10, H), dtype=np.float32) if persistent else None
    center = dict(centered=True, **kw) if centered else {}
    _, up = rbm.get_cost_updates(lr=0.05, k=2, batch_size=10, persistent=chain, **dict(hyper(gauss), **center))
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
def test_the_three_names_are_in_the_header_and_in_the_signatures():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mdbn_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["mdbn_center_offsets"]) == 12 and len(_lib.SIGNATURES["mdbn_center_stats"]) == 12
    assert len(_lib.SIGNATURES["mdbn_center_workspace_bytes"]) == 4


# ------------------------------------------------------------------------------------------------------------------ calls
@pytest.mark.parametrize("gauss", [1, 0])
def test_a_centred_plan_makes_these_calls_in_this_order(gauss):
    fn, rbm, log, batches, inner, _ = make(gauss)
    for t, b in enumerate(batches):
        fn(indexes=b, momentum=0.5, lr=lrs(t))
        assert take(log) == [("cd_step", None), ("center_offsets", None), ("center_stats", None), ("apply_update", 0)]
    assert inner.keep_seen == [True] * len(batches)             # the float32 copies of v0 / ph_mean, for that call only
    assert inner.rhos == [n / 10.0 for n in SIZES]              # rho = n_rows / batch_size
    assert rbm._n_updates == len(batches) and rbm._rng_step == len(batches)


def test_pcd_keeps_its_monitor_and_its_chain():
    fn, rbm, log, batches, inner, data = make(0, persistent=True)
    full = [b for b in batches if len(b) == 10]
    chain0 = fn.plan.persistent.get_value().copy()
    cost = fn(indexes=full[0], momentum=0.5)
    assert take(log) == [("cd_step", None), ("center_offsets", None), ("center_stats", None), ("apply_update", 0)]
    assert rbm.bit_i_idx == 1 and float(cost) < 0.0             # the pseudo-likelihood, not the update's cost slot
    assert not np.array_equal(fn.plan.persistent.get_value(), chain0)
    with pytest.raises(ValueError):
        fn(indexes=batches[2], momentum=0.5)                    # 7 rows against a 10-row chain: as the plain PCD step


def test_the_default_plan_still_logs_one_train_step_call():
    fn, rbm, log, batches, inner, _ = make(1, centered=False)
    for b in batches:
        fn(indexes=b, momentum=0.5)
        assert take(log) == [("cd_train_step", None)]
    assert rbm.v_offset is None and rbm.h_offset is None and inner.nus == []


# ------------------------------------------------------------------------------------------------------------------ offsets
def test_first_step_sets_the_offsets_to_the_batch_means_then_they_slide():
    fn, rbm, log, batches, inner, data = make(0, offset_rate=0.25)
    assert rbm.v_offset is None and rbm.h_offset is None
    fn(indexes=batches[0], momentum=0.5)
    assert np.allclose(rbm.v_offset.get_value(), data[batches[0]].mean(0), atol=1e-7)
    assert np.allclose(rbm.h_offset.get_value(), inner.last.ph_mean.mean(0), atol=1e-7)
    mu0, lam0 = rbm.v_offset.get_value().astype(np.float64), rbm.h_offset.get_value().astype(np.float64)
    fn(indexes=batches[1], momentum=0.5)
    assert np.allclose(rbm.v_offset.get_value(), mu0 + 0.25 * (data[batches[1]].mean(0) - mu0), atol=1e-6)
    assert np.allclose(rbm.h_offset.get_value(), lam0 + 0.25 * (inner.last.ph_mean.mean(0) - lam0), atol=1e-6)
    assert inner.nus == [1.0, 0.25]
    assert fn.plan.centered and fn.plan.offset_rate == 0.25
    assert make(1)[0].plan.offset_rate == 0.01                  # the default: Melchior et al.'s sliding factor


# ------------------------------------------------------------------------------------------------------------------ results
@pytest.mark.parametrize("gauss", [1, 0])
def test_six_steps_equal_a_hand_written_float64_loop(gauss):
    fn, rbm, log, batches, inner, data = make(gauss)
    s = rbm_np.RBMState(V, H, W=rbm.W.tensor.numpy(), hbias=rbm.hbias.tensor.numpy(), vbias=rbm.vbias.tensor.numpy(), gauss=bool(gauss))
    s.freeze_W0()
    offsets, costs, want = None, [], []
    for t, b in enumerate(batches):
        momentum = 0.5 if t < 3 else 0.9
        costs.append(float(fn(indexes=b, momentum=momentum, lr=lrs(t))))
        v0 = data[b]
        ph, _, out = rbm_np.cd_chain(s, v0, PhiloxDraws(rbm.theano_rng.seed, rbm.stream_id, t, 0), 2)
        c = rbm_np.reconstruction_cost(s, out[0], v0)
        offsets = cn.centered_update(s, offsets, v0, ph, out[1], out[4], 0.01, 10, lrs(t), momentum=momentum, **hyper(gauss))
        want.append(c)
    for name in ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed"):
        assert np.abs(getattr(rbm, name).tensor.numpy() - getattr(s, name)).max() < 1e-12, name
    assert np.abs(rbm.v_offset.tensor.numpy() - offsets[0]).max() < 1e-12
    assert np.abs(rbm.h_offset.tensor.numpy() - offsets[1]).max() < 1e-12
    assert np.allclose(costs, want, rtol=1e-12)
    # ... and differ from the plain rule's (the offsets are not a no-op)
    plain, prbm = make(gauss, centered=False)[:2]
    for t, b in enumerate(batches):
        plain(indexes=b, momentum=0.5 if t < 3 else 0.9, lr=lrs(t))
    assert np.abs(prbm.W.tensor.numpy() - rbm.W.tensor.numpy()).max() > 1e-6


# ------------------------------------------------------------------------------------------------------------------ refused
def test_a_data_parallel_group_and_symbolic_grad_are_refused():
    eng = CenterOracle()
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(11), engine=eng)
    _, up = rbm.get_cost_updates(lr=0.05, batch_size=10, centered=True)
    data = mdbn_amd.shared(problem(0)[0], engine=eng)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        mdbn_amd.function(up, data, data_parallel=FakeGroup())
    with pytest.raises(NotImplementedError, match="symbolic_grad"):
        rbm.get_cost_updates(lr=0.05, batch_size=10, centered=True, symbolic_grad=True)
    with pytest.raises(ValueError):
        rbm.get_cost_updates(lr=0.05, batch_size=10, centered=True, offset_rate=0.0)
    _, plain = rbm.get_cost_updates(lr=0.05, batch_size=10)
    assert mdbn_amd.function(plain, data, data_parallel=FakeGroup()).plan.centered is False     # the plain plan: as before


# ------------------------------------------------------------------------------------------------------------------ trainers
def test_the_trainers_pass_the_keywords_down():
    mdbn_amd.DBN.verbose = False
    eng = CenterOracle()
    rs = np.random.RandomState(2)
    x = rs.normal(size=(30, V))
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[H], n_outs=4, engine=eng)
    net.data_parallel = None
    fns, _ = net.training_functions(x, batch_size=10, k=1, centered=True, offset_rate=0.05)
    assert [f.plan.centered for f in fns] == [True, True] and [f.plan.offset_rate for f in fns] == [0.05, 0.05]
    assert [f.plan.centered for f in net.training_functions(x, batch_size=10, k=1)[0]] == [False, False]
    net.shuffle_rng = np.random.RandomState(3)
    net.training(x, batch_size=10, k=1, pretraining_epochs=[2, 2], pretrain_lr=[0.005, 0.1], centered=True)
    assert all(r.v_offset is not None and r.h_offset is not None for r in net.rbm_layers)
    assert eng.nus[0] == 1.0 and set(eng.nus[1:3]) == {0.01}
    for cls, extra in ((mdbn_amd.RBM, dict(persistent=False)), (mdbn_amd.RBM, dict(persistent=True)), (mdbn_amd.GRBM, {})):
        r = cls(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(11), engine=eng)
        data = x if cls is mdbn_amd.GRBM else (x > 0).astype(np.float64)
        r.training(data, None, 1, batch_size=10, centered=True, offset_rate=0.02, **extra)
        assert r.v_offset is not None and r.v_offset.shape == (V,) and r.h_offset.shape == (H,)
    import inspect
    from mdbn_amd import MDBN
    for f in (MDBN.train_bottom_layer, MDBN.train_top):
        names = list(inspect.signature(f).parameters)
        assert names[-2:] == ["centered", "offset_rate"], f.__name__


# ------------------------------------------------------------------------------------------------------------------ checkpoint
def test_checkpoint_round_trip_keeps_the_offsets(tmp_path):
    mdbn_amd.DBN.verbose = False
    eng = CenterOracle()
    rs = np.random.RandomState(0)
    x = rs.normal(size=(40, V))
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[], n_outs=H, engine=eng)
    rbm = net.rbm_layers[0]
    _, up = rbm.get_cost_updates(0.005, k=1, lambda_2=0.1, batch_size=10, centered=True)
    fn = mdbn_amd.function(up, mdbn_amd.shared(x, engine=eng), data_parallel=None)
    for t in range(2):
        fn(indexes=np.arange(10) + 10 * t, momentum=0.5)
    path = str(tmp_path / "centred.npz")
    checkpoint.save_network(path, {'ge': net}, resume=True)
    want = [float(fn(indexes=np.arange(10) + 10 * t, momentum=0.5)) for t in (2, 3)]
    r2 = checkpoint.load_network(path, engine=eng)['ge'].rbm_layers[0]
    saved = np.load(path, allow_pickle=True)['ge_resume'][0]
    assert np.array_equal(r2.v_offset.get_value(), saved['v_offset']) and np.array_equal(r2.h_offset.get_value(), saved['h_offset'])
    assert r2.v_offset.shape == (V,) and r2.h_offset.shape == (H,)
    n_first = len(eng.nus)
    _, up2 = r2.get_cost_updates(0.005, k=1, lambda_2=0.1, batch_size=10, centered=True)
    fn2 = mdbn_amd.function(up2, mdbn_amd.shared(x, engine=eng), data_parallel=None)
    got = [float(fn2(indexes=np.arange(10) + 10 * t, momentum=0.5)) for t in (2, 3)]
    assert eng.nus[n_first:] == [0.01, 0.01]                    # a restored layer goes on sliding: no second initialisation
    # (the checker computes in float64 while a checkpoint holds float32: equal to rounding; exact on the HIP engine)
    np.testing.assert_allclose(got, want, rtol=1e-5)
    np.testing.assert_allclose(r2.W.get_value(), rbm.W.get_value(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(r2.v_offset.get_value(), rbm.v_offset.get_value(), rtol=1e-5, atol=1e-7)
    # a file without offsets loads as before
    plain = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[], n_outs=H, engine=eng)
    checkpoint.save_network(path, {'ge': plain}, resume=True)
    assert 'v_offset' not in np.load(path, allow_pickle=True)['ge_resume'][0]
    r3 = checkpoint.load_network(path, engine=eng)['ge'].rbm_layers[0]
    assert r3.v_offset is None and r3.h_offset is None
