"""The learned per-column variance of a Gaussian layer on the CPU checker engine: the model (the twin's gradient against
central differences of the exact log-likelihood, the density's normalisation), the C-ABI names, the engine calls a plan with
``log_sigma`` makes and their order, six steps against a hand-written float64 loop (alone, centred, with a sparsity target), the
full-batch fixed point, the identities at sigma = 1, the eager surface in raw units, what is refused, the trainers' keyword, the
checkpoint round trip and the DBN's shared ``log_sigma``.  Shapes of tests/test_sparsity_api.py: the smallest with a ragged and
a one-row minibatch."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _center_np as cn
import _sigma_np as sg
import _sparsity_np as sn
import mdbn_amd
from mdbn_amd import MDBN, _lib, checkpoint
from _oracle_engine import OracleEngine
from oracle import rbm_np
from oracle.philox_np import PhiloxDraws

V, H, N = 12, 7, 40
SIZES = (10, 10, 7, 10, 1, 10)
ETA = 0.03
NAMES = {"mdbn_sigma_scale_rows": 13, "mdbn_sigma_update": 17, "mdbn_sigma_workspace_bytes": 4}
LOGGED = ("cd_step", "cd_forward", "cd_statistics", "cd_train_step", "apply_update", "center_offsets", "center_stats",
          "sparsity_activity", "sparsity_stats", "sigma_scale_rows", "sigma_update", "propdown")
SIGMA = [("sigma_scale_rows", None), ("cd_step", None), ("propdown", None), ("sigma_update", None)]
FROZEN = SIGMA[:2]
SPARSE = [("sparsity_activity", None), ("sparsity_stats", None)]
CENTRED = [("center_offsets", None), ("center_stats", None)]
UPDATE = [("apply_update", 0)]
TOL = 2e-6                      # the project's parameter tolerance, of max(1, max|ref|)


class SigmaOracle(OracleEngine):
    """The checker engine with the calls of a step in units (and of the sparse and the centred transforms), from the twins."""

    def __init__(self):
        OracleEngine.__init__(self)
        self.keep_seen, self.signs, self.updates = [], [], []

    def cd_step(self, data, indexes, *args, **kw):
        self.keep_seen.append(kw.pop("keep_f32", None))
        self.cd_indexes = indexes
        stats, sc = OracleEngine.cd_step(self, data, indexes, *args, **kw)
        data = self.as_matrix(data)
        sc.V2 = (data if indexes is None else data[self.index_tensor(indexes)]).clone()
        sc.P2 = self._t(sc.ph_mean)
        return stats, sc

    def propdown(self, h, W, vbias, gauss=False, add_noise=False, rng=None, v0=None, out=None):
        res = OracleEngine.propdown(self, h, W, vbias, gauss=gauss, add_noise=add_noise, rng=rng, v0=v0)
        if out is None:
            return res
        assert gauss and not add_noise and rng is None
        out.copy_(res[1])
        return out, out, out

    def sigma_scale_rows(self, src, indexes, log_sigma, sign, out=None):
        self.signs.append(sign)
        src = self.as_matrix(src)
        rows = self._t(sg.scale_rows(src.numpy(), None if indexes is None else self.index_tensor(indexes).numpy(), log_sigma.numpy(), sign))
        if out is None:
            return rows
        out.copy_(rows)
        return out

    def sigma_update(self, U, M, n_rows, lr, momentum, lo, hi, log_sigma, log_sigma_speed):
        assert U.shape == M.shape and U.shape[0] == n_rows
        self.updates.append((n_rows, lr, momentum, lo, hi))
        g, _ = sg.grad(U.numpy(), M.numpy(), n_rows)
        s, speed = sg.update(log_sigma.numpy(), log_sigma_speed.numpy(), g, lr, momentum, lo, hi)
        log_sigma.copy_(self._t(s))
        log_sigma_speed.copy_(self._t(speed))
        self.last_g = g

    def sparsity_activity(self, scratch, B, q, v_mean, rate):
        q2, m = sn.activity(q.numpy(), scratch.V2.numpy() if v_mean is not None else None, scratch.P2.numpy(), rate)
        q.copy_(self._t(q2))
        if v_mean is not None:
            v_mean.copy_(self._t(m))

    def sparsity_stats(self, stats, V, H, ldv, ldh, q, v_mean, target, w_scale, b_scale):
        st = stats.numpy()
        S, s_h, s_v = sn.stats(st[:V * H].reshape(V, H), st[V * H:V * H + H], st[V * H + H:V * H + H + V], q.numpy(),
                               None if v_mean is None else v_mean.numpy(), target, w_scale, b_scale)
        stats[:V * H + H + V] = self._t(np.concatenate([S.ravel(), s_h, s_v]))
        return stats

    def center_offsets(self, scratch, B, mu, lam, nu):
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


def problem():
    rs = np.random.RandomState(0)
    data = rs.normal(size=(N, V)) * np.exp(rs.uniform(-1.0, 1.0, size=V))[None, :]      # columns of unequal spread
    return data, [rs.permutation(N)[:n].astype(np.int64) for n in SIZES]


def layer(eng, cls=None):
    return (cls or mdbn_amd.GRBM)(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(11),
                                  engine=eng)


def make(learn=ETA, sigma=None, **kw):
    """-> (fn, rbm, log, batches, inner engine, data)"""
    log = []
    inner = SigmaOracle()
    eng = Recorder(inner, log)
    data, batches = problem()
    rbm = layer(eng)
    if sigma is not None:
        rbm.set_sigma(sigma)
    _, up = rbm.get_cost_updates(lr=0.05, k=2, batch_size=10, lambda_2=0.1, learn_sigma=learn, **kw)
    fn = mdbn_amd.function(up, mdbn_amd.shared(data, engine=eng), data_parallel=None)
    del log[:]
    del inner.signs[:]
    return fn, rbm, log, batches, inner, data


def take(log):
    out = list(log)
    del log[:]
    return out


def lrs(t):
    return 0.05 if t % 2 else 0.02


def close(got, want, tol=TOL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max())


# ------------------------------------------------------------------------------------------------------------------ the model
def test_the_twin_gradient_equals_central_differences_of_the_exact_log_likelihood():
    s = sg.state(3, 3, seed=1)
    rs = np.random.RandomState(2)
    log_sigma = rs.uniform(-0.7, 0.7, size=3)
    x = rs.normal(size=(50, 3)) * np.exp(log_sigma)[None, :] * 1.3
    U = sg.scale_rows(x, None, log_sigma, -1.0)
    g, _ = sg.grad(U, sg.cond_mean(s, U))
    h = 1e-5
    for i in range(3):
        e = np.zeros(3)
        e[i] = h
        fd = (sg.log_likelihood(s, x, log_sigma + e) - sg.log_likelihood(s, x, log_sigma - e)) / (2.0 * h)
        assert abs(fd - g[i]) < 1e-7, (i, fd, g[i])
    # ... and log Z does not depend on log_sigma: the exact model expectation of u dF_u/du is 1 in every column


def test_the_density_of_raw_rows_integrates_to_one():
    s = sg.state(2, 2, seed=3)
    log_sigma = np.array([-0.8, 0.6])
    x1, x2 = np.arange(-9.0, 9.0 + 1e-9, 0.02), np.arange(-30.0, 30.0 + 1e-9, 0.05)
    grid = np.stack(np.meshgrid(x1, x2, indexing="ij"), axis=-1).reshape(-1, 2)
    p = np.exp(-sg.free_energy(s, grid, log_sigma) - sg.log_z_unit(s)).reshape(len(x1), len(x2))
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    total = trapezoid(trapezoid(p, x2, axis=1), x1)
    assert abs(total - 1.0) < 1e-9, total
    assert p[0].max() < 1e-30 and p[-1].max() < 1e-30 and p[:, 0].max() < 1e-30 and p[:, -1].max() < 1e-30    # (the box holds the mass)


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_the_three_names_are_in_the_header_and_in_the_signatures():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mdbn_hip.h")).read()
    for name, n_args in NAMES.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == n_args, name
    from mdbn_amd import build
    assert "mdbn_sigma.hip" in build.SOURCES and "mdbn_drv_sigma.hip" in build.SOURCES
    assert hasattr(mdbn_amd.HipEngine, "sigma_scale_rows") and hasattr(mdbn_amd.HipEngine, "sigma_update")


# ------------------------------------------------------------------------------------------------------------------ calls
@pytest.mark.parametrize("extra,middle", [({}, []), (dict(centered=True), CENTRED),
                                          (dict(sparsity_target=0.2, sparsity_cost=1.5), SPARSE),
                                          (dict(centered=True, sparsity_target=0.2, sparsity_cost=1.5), SPARSE + CENTRED)])
def test_a_plan_with_learn_sigma_makes_these_calls_in_this_order(extra, middle):
    fn, rbm, log, batches, inner, _ = make(**extra)
    assert fn.plan.sigma and fn.plan.learn_sigma == ETA
    for t, b in enumerate(batches):
        fn(indexes=b, momentum=0.5 if t < 3 else 0.9, lr=lrs(t))
        assert take(log) == SIGMA + middle + UPDATE
        assert inner.cd_indexes is None                         # the unchanged step on an identity minibatch: the staging rows
    assert inner.keep_seen == [True] * len(batches) and inner.signs == [-1.0] * len(batches)
    lo, hi = mdbn_amd.GRBM.log_sigma_range
    assert inner.updates == [(n, ETA, 0.5 if t < 3 else 0.9, lo, hi) for t, n in enumerate(SIZES)]
    assert (lo, hi) == (-4.6, 4.6)
    assert rbm._n_updates == len(batches) and rbm._rng_step == len(batches)      # the extra propdown consumes no RNG step


def test_a_frozen_sigma_scales_the_rows_and_skips_the_rest_and_a_plain_layer_takes_none_of_it():
    fn, rbm, log, batches, inner, _ = make(learn=None, sigma=np.linspace(0.5, 2.0, V))
    s0 = rbm.log_sigma.tensor.numpy().copy()
    for b in batches:
        fn(indexes=b, momentum=0.5)
        assert take(log) == FROZEN + UPDATE
    assert np.array_equal(rbm.log_sigma.tensor.numpy(), s0) and not rbm.log_sigma_speed.tensor.numpy().any()
    assert fn.plan.sigma and fn.plan.learn_sigma is None and inner.updates == []
    fn, rbm, log, batches, inner, _ = make(learn=None)
    for b in batches:
        fn(indexes=b, momentum=0.5)
        assert take(log) == [("cd_train_step", None)]
    assert rbm.log_sigma is None and rbm.log_sigma_speed is None and not fn.plan.sigma and inner.signs == []


# ------------------------------------------------------------------------------------------------------------------ results
@pytest.mark.parametrize("variant", ["alone", "centered", "sparse"])
def test_six_steps_equal_a_hand_written_float64_loop(variant):
    extra = dict(alone={}, centered=dict(centered=True), sparse=dict(sparsity_target=0.2, sparsity_cost=1.5))[variant]
    fn, rbm, log, batches, inner, data = make(**extra)
    assert not rbm.log_sigma.tensor.numpy().any()               # learn_sigma on a fresh layer: the plain GRBM before the first step
    s = rbm_np.RBMState(V, H, W=rbm.W.tensor.numpy(), hbias=rbm.hbias.tensor.numpy(), vbias=rbm.vbias.tensor.numpy(), gauss=True)
    ls, ls_speed = np.zeros(V), np.zeros(V)
    lo, hi = mdbn_amd.GRBM.log_sigma_range
    q = mu = lam = None
    costs, want = [], []
    for t, b in enumerate(batches):
        momentum = 0.5 if t < 3 else 0.9
        costs.append(float(fn(indexes=b, momentum=momentum, lr=lrs(t))))
        n = len(b)
        u = data[b] * np.exp(-ls)[None, :]                      # the rows in units
        ph, _, out = rbm_np.cd_chain(s, u, PhiloxDraws(rbm.theano_rng.seed, rbm.stream_id, t, 0), 2)
        nv, nh = out[1], out[4]
        want.append(rbm_np.reconstruction_cost(s, out[0], u))   # the monitoring cost, in units
        # every gradient of the step at the old parameters: the exact one of log_sigma first
        m = ph @ s.W.T + s.vbias
        g = (u * (u - m)).mean(axis=0) - 1.0
        S = u.T @ ph - nv.T @ nh
        s_h, s_v = (ph - nh).sum(0), (u - nv).sum(0)
        if variant == "sparse":
            q = ph.mean(0) if q is None else q + (1.0 - 0.9) * (ph.mean(0) - q)
            s_h = s_h + 1.5 * n * (0.2 - q)
            S = S + 1.5 * 10 * np.outer(u.mean(0), 0.2 - q)
        if variant == "centered":
            mu = u.mean(0) if mu is None else mu + 0.01 * (u.mean(0) - mu)
            lam = ph.mean(0) if lam is None else lam + 0.01 * (ph.mean(0) - lam)
            S = S - np.outer(mu, s_h) - np.outer(s_v, lam)
            s_h, s_v = s_h - (n / 10.0) * (S.T @ mu), s_v - (n / 10.0) * (S @ lam)
        rbm_np.apply_update(s, S / 10.0, s_h / n, s_v / n, lrs(t), 0.0, 0.1, momentum)
        ls, ls_speed = np.clip(ls + ls_speed * ETA, lo, hi), g + (ls_speed - g) * momentum
    for name in ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed"):
        assert close(getattr(rbm, name).tensor.numpy(), getattr(s, name)), name
    assert close(rbm.log_sigma.tensor.numpy(), ls) and close(rbm.log_sigma_speed.tensor.numpy(), ls_speed)
    assert np.abs(ls).max() > 1e-2                              # (it moved: the columns have unequal spread)
    assert np.allclose(costs, want, rtol=1e-9)
    if variant == "centered":
        assert close(rbm.v_offset.tensor.numpy(), mu) and close(rbm.h_offset.tensor.numpy(), lam)
    if variant == "sparse":
        assert close(rbm.h_activity.tensor.numpy(), q)
    # ... and differ from the plain plan (it is not a no-op)
    other, orbm = make(learn=None, **extra)[:2]
    for t, b in enumerate(batches):
        other(indexes=b, momentum=0.5 if t < 3 else 0.9, lr=lrs(t))
    assert np.abs(orbm.W.tensor.numpy() - rbm.W.tensor.numpy()).max() > 1e-6


def test_the_full_batch_fixed_point():
    x, want = sg.fixed_point_problem()
    eng = SigmaOracle()
    rbm = mdbn_amd.GRBM(n_visible=64, n_hidden=8, W=np.zeros((64, 8), dtype=np.float32), numpy_rng=np.random.RandomState(5),
                        theano_rng=mdbn_amd.RandomStreams(11), engine=eng)
    _, up = rbm.get_cost_updates(lr=0.0, k=1, batch_size=32, learn_sigma=0.1)
    fn = mdbn_amd.function(up, mdbn_amd.shared(x, engine=eng), data_parallel=None)
    for _ in range(100):
        fn(momentum=0.0)
    assert not rbm.W.tensor.numpy().any() and not rbm.vbias.tensor.numpy().any()
    assert np.abs(rbm.log_sigma.tensor.numpy() - want).max() < 2e-6
    assert np.abs(want).max() > 1.0


# ------------------------------------------------------------------------------------------------------------------ minibatch forms
def follow(s, rbm, data, batches, chain=None):
    """The float64 loop of ``make()``'s plan without a transform, from the state ``s`` taken before the first step; ``chain``:
    PCD from that chain (the cost is then the pseudo-likelihood of the rows in units).  -> (log_sigma, speed, costs, chain)"""
    ls, speed, costs = np.zeros(V), np.zeros(V), []
    lo, hi = mdbn_amd.GRBM.log_sigma_range
    for t, b in enumerate(batches):
        b = np.asarray(b.cpu() if isinstance(b, torch.Tensor) else b)
        n, momentum = len(b), (0.5 if t < 3 else 0.9)
        u = data[b] * np.exp(-ls)[None, :]
        ph, _, out = rbm_np.cd_chain(s, u, PhiloxDraws(rbm.theano_rng.seed, rbm.stream_id, t, 0), 2, chain)
        if chain is not None:
            costs.append(rbm_np.pseudo_likelihood_cost(s, u))
            s.bit_i_idx = (s.bit_i_idx + 1) % V
            chain = out[5]
        else:
            costs.append(rbm_np.reconstruction_cost(s, out[0], u))
        g = (u * (u - (ph @ s.W.T + s.vbias))).mean(axis=0) - 1.0
        S, s_h, s_v = rbm_np.cd_statistics(u, ph, out[1], out[4])
        rbm_np.apply_update(s, S / 10.0, s_h / n, s_v / n, lrs(t), 0.0, 0.1, momentum)
        ls, speed = np.clip(ls + speed * ETA, lo, hi), g + (speed - g) * momentum
    return ls, speed, costs, chain


def state_of(rbm):
    return rbm_np.RBMState(V, H, W=rbm.W.tensor.numpy(), hbias=rbm.hbias.tensor.numpy(), vbias=rbm.vbias.tensor.numpy(), gauss=True)


def run(fn, batches, hint=False):
    return [float(fn(indexes=b, momentum=0.5 if t < 3 else 0.9, lr=lrs(t),
                     **(dict(next_indexes=batches[t + 1]) if hint and t + 1 < len(batches) else {}))) for t, b in enumerate(batches)]


def everything(rbm):
    return [getattr(rbm, n).tensor.numpy().copy() for n in ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed", "log_sigma",
                                                            "log_sigma_speed")]


def test_the_hint_of_the_next_minibatch_changes_nothing():
    res = []
    for hint in (False, True):
        fn, rbm, log, batches, inner, _ = make()
        res.append((run(fn, batches, hint), everything(rbm)))
        assert take(log) == (SIGMA + UPDATE) * len(batches)         # (the hint reaches no engine call)
    assert res[0][0] == res[1][0] and all(np.array_equal(a, b) for a, b in zip(res[0][1], res[1][1]))


def test_a_short_minibatch_has_staging_rows_of_its_own():
    """10, 10, 7, 10, 1, 10 rows at batch_size 10: rows 7 .. 9 (1 .. 9) of the ten-row staging matrices hold NaN while the short
    steps run, and the results are those of the float64 loop."""
    fn, rbm, log, batches, inner, data = make()
    s = state_of(rbm)
    costs = []
    for t, b in enumerate(batches):
        if len(b) < 10:
            for m in fn._sigma_rows[10]:
                m[len(b):] = float("nan")
        costs.append(float(fn(indexes=b, momentum=0.5 if t < 3 else 0.9, lr=lrs(t))))
    assert sorted(fn._sigma_rows) == [1, 7, 10] and all(np.isfinite(m.numpy()).all() for m in fn._sigma_rows[10])
    ls, speed, want, _ = follow(s, rbm, data, batches)
    assert np.isfinite(costs).all() and np.allclose(costs, want, rtol=1e-9)
    assert close(rbm.log_sigma.tensor.numpy(), ls) and close(rbm.log_sigma_speed.tensor.numpy(), speed)
    for name in ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed"):
        assert close(getattr(rbm, name).tensor.numpy(), getattr(s, name)), name


def test_pcd_with_learn_sigma_keeps_its_chain_and_monitors_the_rows_in_units():
    rs = np.random.RandomState(8)
    chain0 = (rs.uniform(size=(10, H)) < 0.5).astype(np.float32)
    fn, rbm, log, batches, inner, data = make(persistent=chain0.copy())
    batches = [b for b in batches if len(b) == 10]
    s = state_of(rbm)
    costs = run(fn, batches)
    assert take(log) == (SIGMA + [("apply_update", 0)]) * len(batches) and rbm.bit_i_idx == len(batches)
    ls, speed, want, chain = follow(s, rbm, data, batches, chain=chain0.astype(np.float64))
    assert np.array_equal(fn.plan.persistent.get_value(), chain.astype(np.float32))
    assert np.allclose(costs, want, rtol=1e-9)                  # the pseudo-likelihood of the rows IN UNITS ...
    s2 = state_of(rbm)
    s2.bit_i_idx = rbm.bit_i_idx - 1
    assert abs(rbm_np.pseudo_likelihood_cost(s2, data[batches[-1]]) - want[-1]) > 1e-3 * abs(want[-1])    # ... not of the raw rows
    assert close(rbm.log_sigma.tensor.numpy(), ls) and close(rbm.W.tensor.numpy(), s.W) and np.abs(ls).max() > 1e-2
    with pytest.raises(ValueError):
        fn(indexes=np.arange(7), momentum=0.5)                  # 7 rows against a 10-row chain: as the plain PCD step


def test_index_forms_int32_int64_and_a_repeated_row():
    _, batches = problem()
    forms = {"int64": [torch.from_numpy(b) for b in batches],
             "int32": [torch.from_numpy(b.astype(np.int32)) for b in batches],
             "list": [[int(i) for i in b[:-1]] + [int(b[0])] if len(b) > 1 else [int(b[0])] for b in batches]}
    res = {}
    for form, idx in forms.items():
        fn, rbm, log, _, inner, data = make()
        s = state_of(rbm)
        costs = run(fn, idx)
        ls, speed, want, _ = follow(s, rbm, data, idx)
        assert np.allclose(costs, want, rtol=1e-9), form
        assert close(rbm.log_sigma.tensor.numpy(), ls) and close(rbm.W.tensor.numpy(), s.W), form
        res[form] = (costs, everything(rbm))
    assert res["int32"][0] == res["int64"][0] and all(np.array_equal(a, b) for a, b in zip(res["int32"][1], res["int64"][1]))
    assert res["list"][0] != res["int64"][0]


def test_the_first_hidden_layer_of_a_pretrained_dbn_takes_raw_rows_to_units():
    mdbn_amd.DBN.verbose = False
    eng = SigmaOracle()
    x = problem()[0]
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[H], n_outs=4, engine=eng)
    net.data_parallel = None
    net.shuffle_rng = np.random.RandomState(3)
    net.training(x, batch_size=10, k=1, pretraining_epochs=[3, 2], pretrain_lr=[0.005, 0.1], learn_sigma=0.05)
    rbm, first = net.rbm_layers[0], net.sigmoid_layers[0]
    assert first.log_sigma is rbm.log_sigma and net.sigmoid_layers[1].log_sigma is None
    ls = rbm.log_sigma.tensor.numpy()
    want = rbm_np.sigmoid((x * np.exp(-ls)[None, :]) @ rbm.W.tensor.numpy() + rbm.hbias.tensor.numpy())
    got = first.forward(x).numpy()
    assert np.abs(got - want).max() < 1e-12 and np.abs(ls).max() > 1e-3
    assert np.abs(got - rbm_np.sigmoid(x @ rbm.W.tensor.numpy() + rbm.hbias.tensor.numpy())).max() > 1e-3


# ------------------------------------------------------------------------------------------------------------------ identities
def eager(rbm, x, h):
    """Every eager call of the surface, as host arrays (the RNG steps advance alike on both layers)."""
    out = []
    for res in (rbm.propup(x), rbm.sample_h_given_v(x), rbm.propdown(h), rbm.sample_v_given_h(h), rbm.gibbs_hvh(h), rbm.gibbs_vhv(x),
                rbm.gibbs_vhv_chain(x, 2), [rbm.free_energy(x)]):
        out += [np.asarray(r.tensor.numpy()) for r in res]
    out += list(rbm.free_energies(x[:5], x[5:])) + [np.float64(rbm.free_energy_gap(x[:5], x[5:])), rbm.base_rate_vbias(x),
                                                   rbm.hidden_activity(x, chunk_rows=4), np.float64(rbm.get_pseudo_likelihood_cost(x))]
    return out


@pytest.mark.parametrize("error_free", [True, False])
def test_sigma_one_is_the_plain_layer_bit_for_bit(error_free):
    rs = np.random.RandomState(3)
    x, h = rs.normal(size=(9, V)), (rs.uniform(size=(9, H)) < 0.5).astype(np.float64)
    res = []
    for sigma in (None, 1.0):
        eng = SigmaOracle()
        rbm = layer(eng)
        rbm.error_free = error_free
        rbm.vbias.set_value(np.linspace(-1, 1, V).astype(np.float32))
        if sigma is not None:
            rbm.set_sigma(sigma)
            assert not rbm.log_sigma.tensor.numpy().any() and not rbm.log_sigma_speed.tensor.numpy().any()
            assert rbm.log_sigma.shape == (V,) and np.array_equal(rbm.sigma, np.ones(V, dtype=np.float32))
        res.append((eager(rbm, x, h), rbm._rng_step))
    assert res[0][1] == res[1][1]
    assert len(res[0][0]) == len(res[1][0]) > 20
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b)
    # a frozen sigma = 1 trains as the plain layer does, bit for bit
    runs = []
    for sigma in (None, 1.0):
        fn, rbm, log, batches, inner, _ = make(learn=None, sigma=sigma)
        costs = [float(fn(indexes=b, momentum=0.5, lr=lrs(t))) for t, b in enumerate(batches)]
        runs.append((costs, rbm.W.tensor.numpy().copy(), rbm.vbias_speed.tensor.numpy().copy()))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])


def test_eager_calls_take_and_return_raw_units():
    rs = np.random.RandomState(4)
    sigma = np.exp(rs.uniform(-1.0, 1.0, size=V))
    x, h = rs.normal(size=(9, V)) * sigma[None, :], (rs.uniform(size=(9, H)) < 0.5).astype(np.float64)
    eng = SigmaOracle()
    plain, rbm = layer(eng), layer(eng)
    for r in (plain, rbm):
        r.vbias.set_value(np.linspace(-1, 1, V).astype(np.float32))
    rbm.set_sigma(sigma)
    s32 = rbm.log_sigma.tensor.numpy()                          # (float32 values, held in float64 on the checker)
    sig = np.exp(s32)
    assert np.allclose(rbm.sigma, sigma, rtol=1e-6) and rbm.sigma.dtype == np.float32
    u = x / sig[None, :]
    assert close(rbm.propup(x)[1].tensor.numpy(), plain.propup(u)[1].tensor.numpy(), 1e-12)
    assert close(rbm.sample_h_given_v(x)[1].tensor.numpy(), plain.propup(u)[1].tensor.numpy(), 1e-12)
    assert close(rbm.free_energy(x).tensor.numpy(), plain.free_energy(u).tensor.numpy() + s32.sum(), 1e-12)
    assert close(rbm.sample_v_given_h(h)[1].tensor.numpy(), plain.sample_v_given_h(h)[1].tensor.numpy() * sig[None, :], 1e-12)
    assert close(rbm.propdown(h)[0].tensor.numpy(), plain.propdown(h)[0].tensor.numpy() * sig[None, :], 1e-12)
    assert close(rbm.gibbs_vhv(x)[4].tensor.numpy(), plain.gibbs_vhv(u)[4].tensor.numpy() * sig[None, :], 1e-12)
    assert close(rbm.gibbs_vhv_chain(x, 3)[5].tensor.numpy(), plain.gibbs_vhv_chain(u, 3)[5].tensor.numpy() * sig[None, :], 1e-10)
    assert close(rbm.hidden_activity(x), plain.hidden_activity(u), 1e-6)
    assert close(rbm.base_rate_vbias(x), plain.base_rate_vbias(u), 1e-6)
    # the noise of a sample has the column's standard deviation
    rbm.error_free = plain.error_free = False
    rbm._rng_step = plain._rng_step = 50
    a, b = rbm.sample_v_given_h(h), plain.sample_v_given_h(h)
    assert close(a[2].tensor.numpy() - a[1].tensor.numpy(), (b[2].tensor.numpy() - b[1].tensor.numpy()) * sig[None, :], 1e-10)
    # the exact log-likelihood of the twin is mean(-F) - log Z of the unit model
    st = rbm_np.RBMState(V, H, W=rbm.W.tensor.numpy(), hbias=rbm.hbias.tensor.numpy(), vbias=rbm.vbias.tensor.numpy(), gauss=True)
    assert close(-rbm.free_energy(x).tensor.numpy().mean() - sg.log_z_unit(st), sg.log_likelihood(st, x, s32), 1e-12)
    rbm.set_sigma(None)
    assert rbm.log_sigma is None and rbm.log_sigma_speed is None and rbm.sigma is None


# ------------------------------------------------------------------------------------------------------------------ surface
def test_where_the_keyword_sits_and_its_default():
    for f in (mdbn_amd.RBM.get_cost_updates, mdbn_amd.DBN.training_functions):
        names = list(inspect.signature(f).parameters)
        assert names[names.index("centered") - 1] == "learn_sigma", f.__qualname__
    for f in (mdbn_amd.GRBM.training, mdbn_amd.DBN.training, MDBN.train_bottom_layer):
        names = list(inspect.signature(f).parameters)
        assert names[names.index("visible_groups") + 1] == "learn_sigma", f.__qualname__
    for f in (mdbn_amd.RBM.get_cost_updates, mdbn_amd.DBN.training_functions, mdbn_amd.GRBM.training, mdbn_amd.DBN.training,
              MDBN.train_bottom_layer):
        sig = inspect.signature(f)
        assert sig.parameters["learn_sigma"].default is None and list(sig.parameters)[-1] != "learn_sigma", f.__qualname__


def test_bad_values_are_refused_with_value_errors():
    eng = SigmaOracle()
    rbm = layer(eng)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            rbm.get_cost_updates(lr=0.05, batch_size=10, learn_sigma=bad)
    assert rbm.log_sigma is None
    with pytest.raises(ValueError):
        layer(eng, mdbn_amd.RBM).get_cost_updates(lr=0.05, batch_size=10, learn_sigma=0.1)
    for bad in (0.0, -1.0, float("nan"), np.ones(V - 1), np.r_[np.ones(V - 1), 0.0], float("inf")):
        with pytest.raises(ValueError):
            rbm.set_sigma(bad)
    assert rbm.log_sigma is None and not hasattr(mdbn_amd.RBM, "set_sigma")
    assert rbm.get_cost_updates(lr=0.05, batch_size=10)[1].sigma is False


def test_what_is_refused_names_log_sigma_and_draws_nothing():
    eng = SigmaOracle()
    rs = np.random.RandomState(1)
    x = rs.normal(size=(10, V))
    mask = np.r_[np.ones(V // 2), np.zeros(V - V // 2)]
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[H], n_outs=4, engine=eng)
    rbm = net.rbm_layers[0]
    rbm.set_sigma(0.5)
    refused = [
        lambda: rbm.get_cost_updates(lr=0.05, batch_size=10, symbolic_grad=True),
        lambda: rbm.get_cost_updates(lr=0.05, batch_size=10, symbolic_grad=True, learn_sigma=0.1),
        lambda: mdbn_amd.function(rbm.get_cost_updates(lr=0.05, batch_size=10)[1], mdbn_amd.shared(x, engine=eng), data_parallel=FakeGroup()),
        lambda: rbm.log_partition(method="tempering"),
        lambda: rbm.log_likelihood(x, method="tempering"),
        lambda: rbm.check_log_partition(data=x),
        lambda: rbm.tempered_chains(4),
        lambda: rbm.sample_tempered(4, n_sweeps=3, burn_in=1),
        lambda: mdbn_amd.RBM.training(rbm, x, None, 1, tempering=4),
        lambda: rbm.gibbs_vhv_clamped(x, mask, 3),
        lambda: rbm.impute(x, mask, n_steps=3, burn_in=1),
        lambda: rbm.conditional_log_partition(x, mask),
        lambda: rbm.conditional_log_likelihood(x, mask),
        lambda: net.log_likelihood_bound(x, n_samples=2),
        lambda: net.fine_tune(x, 1, batch_size=5, lr=0.01),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(NotImplementedError, match="log_sigma"):
            call()
        assert all(r._rng_step == 0 for r in net.rbm_layers), i
    # a fresh layer asked for learn_sigma with symbolic_grad is refused before log_sigma is made
    fresh = layer(eng)
    with pytest.raises(NotImplementedError, match="log_sigma"):
        fresh.get_cost_updates(lr=0.05, batch_size=10, symbolic_grad=True, learn_sigma=0.1)
    assert fresh.log_sigma is None
    # the plain layer on a group, as before
    assert mdbn_amd.function(fresh.get_cost_updates(lr=0.05, batch_size=10)[1], mdbn_amd.shared(x, engine=eng),
                             data_parallel=FakeGroup()).plan.sigma is False


# ------------------------------------------------------------------------------------------------------------------ the DBN
def test_the_dbn_shares_log_sigma_with_its_input_layer():
    mdbn_amd.DBN.verbose = False
    eng = SigmaOracle()
    rs = np.random.RandomState(2)
    sigma = np.exp(rs.uniform(-1.0, 1.0, size=V))
    x = rs.normal(size=(30, V)) * sigma[None, :]
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[H], n_outs=4, engine=eng)
    rbm = net.rbm_layers[0]
    plain_out = net.get_output(x, 0)
    assert net.sigmoid_layers[0].log_sigma is None and net.sigmoid_layers[1].log_sigma is None
    rbm.vbias.set_value(np.linspace(-1, 1, V).astype(np.float32))
    rbm.set_sigma(sigma)
    assert net.sigmoid_layers[0].log_sigma is rbm.log_sigma and net.sigmoid_layers[1].log_sigma is None
    got = net.get_output(x, 0)
    assert np.array_equal(got, eng.to_numpy(rbm.propup(x)[1].tensor)) and np.abs(got - plain_out).max() > 1e-3
    acts = net.hidden_activity(x)
    assert close(acts[0], got.mean(0), 1e-6) and close(acts[1], net.get_output(x).mean(0), 1e-6)
    # down_pass returns raw units: the bottom layer's mean times sigma
    h = (rs.uniform(size=(6, H)) < 0.5).astype(np.float64)
    sig = np.exp(rbm.log_sigma.tensor.numpy())
    want = (h @ rbm.W.tensor.numpy().T + rbm.vbias.tensor.numpy()) * sig[None, :]
    assert close(net.down_pass(h, 0), want, 1e-6)
    # the cached lower-layer activations of training follow a sigma that is given later
    table = mdbn_amd.shared(x, engine=eng)
    provider = net._layer_input_fn(1, table)
    first = provider()
    assert provider() is first
    rbm.set_sigma(2.0 * sigma)
    second = provider()
    assert second is not first and np.array_equal(eng.to_numpy(second), net.get_output(x, 0))
    # a Bernoulli input layer has no such link
    bern = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, gauss=False, hidden_layers_sizes=[H], n_outs=4, engine=eng)
    assert bern.sigmoid_layers[0].log_sigma is None


def test_the_trainers_pass_the_keyword_down(monkeypatch):
    mdbn_amd.DBN.verbose = False
    eng = SigmaOracle()
    x = problem()[0][:30]
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[H], n_outs=4, engine=eng)
    net.data_parallel = None
    fns, _ = net.training_functions(x, batch_size=10, k=1, learn_sigma=0.02)
    assert [f.plan.sigma for f in fns] == [True, False] and [f.plan.learn_sigma for f in fns] == [0.02, None]
    assert net.rbm_layers[1].log_sigma is None
    plain = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[H], n_outs=4, engine=eng)
    assert [f.plan.sigma for f in plain.training_functions(x, batch_size=10, k=1)[0]] == [False, False]
    with pytest.raises(ValueError):
        mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, gauss=False, hidden_layers_sizes=[H], n_outs=4,
                     engine=eng).training_functions(x, batch_size=10, k=1, learn_sigma=0.02)
    net.shuffle_rng = np.random.RandomState(3)
    net.training(x, batch_size=10, k=1, pretraining_epochs=[3, 2], pretrain_lr=[0.005, 0.1], learn_sigma=0.05, centered=True)
    assert np.abs(net.rbm_layers[0].log_sigma.tensor.numpy()).max() > 1e-3 and net.rbm_layers[1].log_sigma is None
    # the upper layer trained on what the input layer's propup sees
    assert np.array_equal(net.get_output(x, 0), eng.to_numpy(net.rbm_layers[0].propup(x)[1].tensor))
    r = layer(eng)
    r.training(x, None, 2, batch_size=10, learn_sigma=0.05)
    assert np.abs(r.log_sigma.tensor.numpy()).max() > 1e-3
    seen = []
    monkeypatch.setattr(mdbn_amd.DBN, "training", lambda self, *a, **kw: seen.append(kw.get("learn_sigma", "absent")))
    monkeypatch.setattr(mdbn_amd.DBN, "get_output", lambda self, x, layer=-1: None)
    monkeypatch.setattr(MDBN, "shared", lambda x, **kw: np.asarray(x))

    class CheckerDBN(mdbn_amd.DBN):
        def __init__(self, **kw):
            mdbn_amd.DBN.__init__(self, engine=SigmaOracle(), **kw)

    monkeypatch.setattr(MDBN, "DBN", CheckerDBN)
    MDBN.train_bottom_layer(x, None, batch_size=10, layers_sizes=[H, 4], rng=np.random.RandomState(1), learn_sigma=0.02)
    MDBN.train_bottom_layer(x, None, batch_size=10, layers_sizes=[H, 4], rng=np.random.RandomState(1))
    assert seen == [0.02, "absent"]


# ------------------------------------------------------------------------------------------------------------------ checkpoint
def test_checkpoint_round_trip_keeps_log_sigma_and_its_speed(tmp_path):
    mdbn_amd.DBN.verbose = False
    eng = SigmaOracle()
    x = problem()[0]
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[], n_outs=H, engine=eng)
    rbm = net.rbm_layers[0]
    plan = dict(k=1, lambda_2=0.1, batch_size=10, learn_sigma=0.05)
    _, up = rbm.get_cost_updates(0.005, **plan)
    fn = mdbn_amd.function(up, mdbn_amd.shared(x, engine=eng), data_parallel=None)
    for t in range(2):
        fn(indexes=np.arange(10) + 10 * t, momentum=0.5)
    path = str(tmp_path / "sigma.npz")
    checkpoint.save_network(path, {'ge': net}, resume=True)
    want = [float(fn(indexes=np.arange(10) + 10 * t, momentum=0.5)) for t in (2, 3)]
    r2 = checkpoint.load_network(path, engine=eng)['ge'].rbm_layers[0]
    saved = np.load(path, allow_pickle=True)['ge_resume'][0]
    for key in ("log_sigma", "log_sigma_speed"):
        assert saved[key].dtype == np.float32 and saved[key].shape == (V,) and np.abs(saved[key]).max() > 0
        assert np.array_equal(getattr(r2, key).get_value(), saved[key])
    _, up2 = r2.get_cost_updates(0.005, **plan)                 # (a restored log_sigma is kept: no second initialisation)
    fn2 = mdbn_amd.function(up2, mdbn_amd.shared(x, engine=eng), data_parallel=None)
    got = [float(fn2(indexes=np.arange(10) + 10 * t, momentum=0.5)) for t in (2, 3)]
    # (the checker computes in float64 while a checkpoint holds float32: equal to rounding; exact on the HIP engine)
    np.testing.assert_allclose(got, want, rtol=1e-5)
    np.testing.assert_allclose(r2.log_sigma.get_value(), rbm.log_sigma.get_value(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(r2.log_sigma_speed.get_value(), rbm.log_sigma_speed.get_value(), rtol=1e-5, atol=1e-7)
    # a plain checkpoint holds no such key and loads as before
    plain = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[], n_outs=H, engine=eng)
    checkpoint.save_network(path, {'ge': plain}, resume=True)
    assert 'log_sigma' not in np.load(path, allow_pickle=True)['ge_resume'][0]
    assert checkpoint.load_network(path, engine=eng)['ge'].rbm_layers[0].log_sigma is None
