"""Discriminative / hybrid training of a classification RBM, host logic on the checker engine (tests/_disc_np.DiscOracle: the
classification calls from the float64 twin): the read-only methods, every refusal, the keywords through the trainers, and
that a plan without ``discriminative`` is the plan of before."""
import numpy as np
import pytest

import mdbn_amd
from mdbn_amd import MDBN
import _disc_np as dn
import _softmax_np as sm

V, H, N = 20, 6, 40
BOUNDS = [2, 5, 16, 20]          # two Bernoulli columns, groups of 3 and 11, the label block of 4 last
LO, K = 16, 4


def problem(seed=0):
    return sm.one_hot_data(np.random.RandomState(seed), N, V, BOUNDS)


def layer(eng, groups=BOUNDS, cls=mdbn_amd.RBM):
    return cls(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(11), engine=eng,
               **({} if groups is None else dict(visible_groups=groups)))


class FakeGroup(object):
    world_size, rank = 2, 0

    def shard(self, n):
        return 0, n // 2


def test_read_only_methods_match_the_twin_and_consume_no_random_numbers():
    eng = dn.DiscOracle()
    rbm, data = layer(eng), problem()
    W, hb, vb = rbm.W.get_value(), rbm.hbias.get_value(), rbm.vbias.get_value()
    post = rbm.label_posterior(data)
    assert post.dtype == np.float64 and post.shape == (N, K)
    assert np.abs(post - dn.posterior(data, W, hb, vb, LO, K)).max() <= 1e-12
    assert np.abs(post - rbm.group_posterior(data, -1)).max() <= 1e-9           # the independent witness
    assert np.abs(rbm.label_posterior(data, 0) - rbm.group_posterior(data, 0)).max() <= 1e-9
    assert np.array_equal(rbm.predict(data), post.argmax(axis=1))
    assert np.abs(rbm.label_log_likelihood(data) - dn.logp(data, W, hb, vb, LO, K)).max() <= 1e-12
    assert rbm._rng_step == 0
    junk = data.copy()
    junk[:, LO:LO + K] = 0.25
    assert np.array_equal(rbm.label_posterior(junk), post)                      # what the block holds is ignored ...
    with pytest.raises(ValueError, match="exactly one 1"):
        rbm.label_log_likelihood(junk)                                          # ... unless its category is asked for
    for call in (rbm.label_posterior, rbm.predict, rbm.label_log_likelihood):
        with pytest.raises(ValueError, match="label group"):
            call(data, 3)
        with pytest.raises(ValueError, match="label group"):
            call(data, -4)
    plain = layer(eng, None)
    for call in (plain.label_posterior, plain.predict, plain.label_log_likelihood):
        with pytest.raises(ValueError, match="visible_groups"):
            call(data)
    with pytest.raises(NotImplementedError, match="class_posterior"):
        layer(sm.GroupedOracle()).label_posterior(data)


def test_every_refusal_comes_before_anything_runs():
    eng = dn.DiscOracle()
    rbm, data = layer(eng), problem()
    shared = mdbn_amd.shared(data, engine=eng)
    kw = dict(lr=0.05, batch_size=10, discriminative=1.0)
    with pytest.raises(ValueError, match="visible_groups"):
        layer(eng, None).get_cost_updates(**kw)
    for g in (3, -4, 7):
        with pytest.raises(ValueError, match="label group"):
            rbm.get_cost_updates(label_group=g, **kw)
    with pytest.raises(NotImplementedError, match="centered"):
        rbm.get_cost_updates(centered=True, **kw)
    with pytest.raises(NotImplementedError, match="symbolic_grad"):
        rbm.get_cost_updates(symbolic_grad=True, **kw)
    with pytest.raises(NotImplementedError, match="sparsity"):
        rbm.get_cost_updates(generative=0.0, sparsity_target=0.1, sparsity_cost=0.05, **kw)
    with pytest.raises(NotImplementedError, match="persistent"):
        rbm.get_cost_updates(generative=0.0, persistent=np.zeros((10, H), dtype=np.float32), **kw)
    with pytest.raises(NotImplementedError, match="class_stats"):
        layer(sm.GroupedOracle()).get_cost_updates(**kw)
    for bad in (dict(discriminative=0.0), dict(discriminative=-1.0), dict(discriminative=float("nan")), dict(generative=-0.5),
                dict(generative=float("inf"))):
        with pytest.raises(ValueError):
            rbm.get_cost_updates(**dict(kw, **bad))
    _, up = rbm.get_cost_updates(**kw)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        mdbn_amd.function(up, shared, data_parallel=FakeGroup())
    # the training table is checked once, when the step function is built: the label block must be one-hot
    bad = data.copy()
    bad[3, LO:LO + K] = 0.0
    with pytest.raises(ValueError, match="row 3"):
        mdbn_amd.function(up, mdbn_amd.shared(bad, engine=eng), data_parallel=None)
    assert rbm._rng_step == 0 and rbm._n_updates == 0 and eng.calls == []
    # what composes: a sparsity target and a persistent chain with generative > 0
    rbm.get_cost_updates(sparsity_target=0.1, sparsity_cost=0.05, **kw)
    rbm.get_cost_updates(persistent=np.zeros((10, H), dtype=np.float32), **kw)


def test_without_the_keyword_the_plan_is_the_plan_of_before():
    eng = dn.DiscOracle()
    data = problem()
    a, b = layer(eng), layer(eng)
    _, plain = a.get_cost_updates(lr=0.05, batch_size=10, weightcost=2e-4)
    _, none = b.get_cost_updates(lr=0.05, batch_size=10, weightcost=2e-4, discriminative=None, label_group=0, generative=0.0)
    assert plain.disc_weight is None and none.disc_weight is None and none.gen_weight == 1.0 and none.label_span is None
    skip = ("rbm", "W0", "grouped")
    assert {k: v for k, v in vars(plain).items() if k not in skip} == {k: v for k, v in vars(none).items() if k not in skip}
    fa = mdbn_amd.function(plain, mdbn_amd.shared(data, engine=eng), data_parallel=None)
    fb = mdbn_amd.function(none, mdbn_amd.shared(data, engine=eng), data_parallel=None)
    for t in range(3):
        ca, cb = fa(indexes=np.arange(10) + 10 * t, momentum=0.5), fb(indexes=np.arange(10) + 10 * t, momentum=0.5)
        assert float(ca) == float(cb)
    for n in ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed"):
        assert np.array_equal(getattr(a, n).get_value(), getattr(b, n).get_value()), n
    assert eng.calls == [] and fa.discriminative_cost is None


@pytest.mark.parametrize("gen,w", [(0.0, 1.0), (1.0, 0.5), (0.5, 2.0)])
def test_a_step_applies_the_weighted_sum_of_both_statistics(gen, w):
    """One step function call against the twin: gen x (CD statistics of the checker's own chain) + w x (discriminative
    statistics) through the project's update rule; discriminative_cost is the mean NLL at the parameters of before."""
    from oracle import rbm_np
    eng = dn.DiscOracle()
    rbm, data = layer(eng), problem()
    s = rbm_np.RBMState(V, H, W=rbm.W.get_value(), hbias=rbm.hbias.get_value(), vbias=rbm.vbias.get_value())
    _, up = rbm.get_cost_updates(lr=0.1, batch_size=10, discriminative=w, generative=gen)
    fn = mdbn_amd.function(up, mdbn_amd.shared(data, engine=eng), data_parallel=None)
    idx = np.arange(10) + 5
    for t in range(2):                      # (the parameter step uses the old speed: the second call moves the parameters)
        rows = data[idx].astype(np.float64)
        want_nll = -dn.logp(rows, s.W, s.hbias, s.vbias, LO, K).mean()
        cost = float(fn(indexes=idx, momentum=0.5))
        assert abs(fn.discriminative_cost - want_nll) <= 1e-12
        if gen > 0.0:
            sc = eng.last
            S, s_h, s_v = dn.hybrid_stats(rows, s.W, s.hbias, s.vbias, LO, K, gen, w, sc.nv_mean, sc.ph_mean, sc.nh_mean)
            assert cost > 0.0 and abs(cost - want_nll) > 1e-6               # the CD monitor, not the NLL
        else:
            S, s_h, s_v = (w * x for x in dn.stats(rows, s.W, s.hbias, s.vbias, LO, K)[:3])
            assert abs(cost - want_nll) <= 1e-12                            # no chain: the monitor is the NLL
        dn.update(s, S, s_h, s_v, 10, 10, 0.1, momentum=0.5)
        for n in ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed"):
            assert np.abs(getattr(rbm, n).get_value() - getattr(s, n)).max() <= 1e-6, (n, t)      # (float32 storage)
    assert eng.calls == [dict(lo=LO, K=K, gen=gen, w=w, pure=gen == 0.0, B=10)] * 2
    assert rbm._rng_step == 2


def test_the_trainers_pass_the_keywords_down():
    mdbn_amd.DBN.verbose = False
    eng = dn.DiscOracle()
    data = problem()
    # RBM.training: hybrid under CD and PCD, pure without a chain
    for extra, pure in ((dict(persistent=False), False), (dict(persistent=True), False), (dict(persistent=False, generative=0.0), True)):
        eng.calls = []
        r = layer(eng, None)
        hist = r.training(data, None, 1, batch_size=10, visible_groups=BOUNDS, discriminative=0.5, label_group=-1, **extra)
        assert len(eng.calls) == N // 10 and all(c["w"] == 0.5 and c["lo"] == LO and c["K"] == K and c["pure"] == pure for c in eng.calls)
        assert hist[0][0] > 0.0
    with pytest.raises(NotImplementedError, match="persistent"):
        layer(eng).training(data, None, 1, batch_size=10, discriminative=0.5, generative=0.0)       # (persistent defaults to True)
    # DBN.training: the input layer only
    eng.calls = []
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, gauss=False, hidden_layers_sizes=[H], n_outs=4, engine=eng,
                       visible_groups=BOUNDS)
    net.data_parallel = None
    net.shuffle_rng = np.random.RandomState(3)
    net.training(data, batch_size=10, k=1, pretraining_epochs=[2, 2], pretrain_lr=[0.05, 0.05], discriminative=2.0, label_group=0,
                 generative=0.5)
    assert len(eng.calls) >= 1 and all(c == dict(lo=2, K=3, gen=0.5, w=2.0, pure=False, B=10) for c in eng.calls)
    plans = [f.plan for f in net.training_functions(data, batch_size=10, k=1, discriminative=1.0)[0]]
    assert [p.disc_weight for p in plans] == [1.0, None] and plans[0].label_span == (LO, K) and plans[0].gen_weight == 1.0
    assert [f.plan.disc_weight for f in net.training_functions(data, batch_size=10, k=1)[0]] == [None, None]
    gauss = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, gauss=True, hidden_layers_sizes=[H], n_outs=4, engine=eng)
    with pytest.raises(ValueError, match="visible_groups"):
        gauss.training_functions(data, batch_size=10, k=1, discriminative=1.0)
    # MDBN.train_top: the joint layer
    eng.calls = []
    mdbn_amd.set_engine(eng)
    saved = dict(MDBN.TOP_SHAPE), dict(MDBN.TOP_SCHEDULE)
    try:
        MDBN.TOP_SHAPE.update(hidden_layers_sizes=[H], n_outs=3)
        MDBN.TOP_SCHEDULE.update(pretraining_epochs=[1, 1], pretrain_lr=[0.05, 0.05])
        top = MDBN.train_top(10, False, data, None, np.random.RandomState(2), visible_groups=BOUNDS, discriminative=1.5, generative=0.25)
        assert top.rbm_layers[0].visible_groups.host.tolist() == BOUNDS
        assert len(eng.calls) >= 1 and all(c == dict(lo=LO, K=K, gen=0.25, w=1.5, pure=False, B=10) for c in eng.calls)
    finally:
        MDBN.TOP_SHAPE.clear(); MDBN.TOP_SHAPE.update(saved[0])
        MDBN.TOP_SCHEDULE.clear(); MDBN.TOP_SCHEDULE.update(saved[1])
        import mdbn_amd.engine as E
        E._default_engine = None
