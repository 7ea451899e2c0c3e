"""Which engine calls a ``StepFunction`` makes on each of its paths, in which order, and that the paths agree bit for bit
(CPU, checker engine): single device, synchronous group, overlapped group with the deferred update as its own call or inside
the statistics half.  Only the public surface is touched, plus ``fn.overlap`` / ``fn.fuse_deferred`` / ``fn.comm_cus``.
Shapes of tests/test_dp_gloo.py: the smallest with a ragged and a one-row minibatch."""
import numpy as np
import pytest

import mdbn_amd
from _oracle_engine import OracleEngine

V, H, N = 12, 7, 40
SIZES = (10, 10, 7, 10, 1, 10)
LOGGED = ("cd_step", "cd_forward", "cd_statistics", "cd_train_step", "apply_update")


class SplitOracle(OracleEngine):
    """The checker engine with the two halves of a step: the statistics are computed at ``cd_forward`` time (from the
    parameters BEFORE the deferred update), the deferred update is applied in ``cd_statistics``."""

    def __init__(self):
        OracleEngine.__init__(self)
        self.comm_cus_seen, self.forward_hints = set(), []

    def cd_step(self, *args, **kw):
        self.comm_cus_seen.add(kw.pop("comm_cus", 0))
        return OracleEngine.cd_step(self, *args, **kw)

    def cd_forward(self, data, indexes, W, hbias, vbias, gauss, k, rng, add_noise=False, sample_stats=False, stats=None,
                   comm_cus=0, next_indexes=None):
        self.comm_cus_seen.add(comm_cus)
        self.forward_hints.append(next_indexes)
        return OracleEngine.cd_step(self, data, indexes, W, hbias, vbias, gauss, k, rng, add_noise=add_noise,
                                    sample_stats=sample_stats, stats=stats)

    def cd_statistics(self, token, deferred=None):
        stats, sc = token
        cost = None
        if deferred is not None:
            cost = OracleEngine.apply_update(self, *deferred[:16], phase=deferred[16], ldv=deferred[17])
        return stats, sc, cost


class Recorder(object):
    """Proxy of an engine: logs (name, phase) of every step-level call, passes everything else through."""

    def __init__(self, engine, log):
        self._engine, self._log = engine, log
        self.train_step_hints = []

    def __getattr__(self, name):
        target = getattr(self._engine, name)            # (AttributeError for what the engine lacks: the probes see through)
        if name not in LOGGED:
            return target

        def call(*args, **kw):
            phase = None
            if name == "apply_update":
                phase = kw.get("phase", args[16] if len(args) > 16 else 0)
            elif name == "cd_statistics":
                deferred = kw.get("deferred", args[1] if len(args) > 1 else None)
                phase = None if deferred is None else deferred[16]
            elif name == "cd_train_step":
                self.train_step_hints.append(kw.get("next_indexes"))
            self._log.append((name, phase))
            return target(*args, **kw)
        return call


class Work(object):
    def __init__(self, log):
        self._log = log

    def wait(self):
        self._log.append(("wait", None))


class FakeGroup(object):
    """One process standing in for rank 0 of two: it owns every row (or none: ``empty``), the sum over ranks is the identity."""
    world_size, rank = 2, 0

    def __init__(self, log, empty=False):
        self._log, self.empty, self.reduced_abs_sums = log, empty, []

    def shard(self, n):
        return (n, n) if self.empty else (0, n)

    def all_reduce_sum(self, tensor, engine=None):
        self.reduced_abs_sums.append(float(tensor.abs().sum()))
        self._log.append(("reduce", None))

    def all_reduce_sum_async(self, tensor, engine=None):
        self.reduced_abs_sums.append(float(tensor.abs().sum()))
        self._log.append(("reduce_async", None))
        return Work(self._log)


def problem(gauss):
    rs = np.random.RandomState(0)
    data = rs.normal(size=(N, V)) if gauss else (rs.uniform(size=(N, V)) < 0.4).astype(np.float64)
    return data, [rs.permutation(N)[:n].astype(np.int64) for n in SIZES]


def make(gauss=1, group="fake", overlap=True, split=True, empty=False):
    """-> (fn, rbm, log, batches, recorder, group)"""
    log = []
    inner = SplitOracle() if split else OracleEngine()
    eng = Recorder(inner, log)
    data, batches = problem(gauss)
    cls = mdbn_amd.GRBM if gauss else mdbn_amd.RBM
    rbm = cls(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(11), engine=eng)
    hp = dict(lambda_2=0.1) if gauss else dict(weightcost=2e-4)
    _, up = rbm.get_cost_updates(lr=0.05, k=2, batch_size=10, **hp)
    grp = FakeGroup(log, empty) if group == "fake" else None
    fn = mdbn_amd.function(up, mdbn_amd.shared(data, engine=eng), data_parallel=grp, overlap=overlap)
    assert fn.overlap == bool(overlap and grp is not None)
    del log[:]
    return fn, rbm, log, batches, eng, grp


def take(log):
    out = list(log)
    del log[:]
    return out


def lrs(t):
    return 0.05 if t % 2 else 0.02


# ------------------------------------------------------------------------------------------------------------------ call order
def test_single_device_is_one_train_step_call_per_step():
    fn, rbm, log, batches, eng, _ = make(group=None)
    for t, b in enumerate(batches):
        fn(indexes=b, momentum=0.5, lr=lrs(t))
        assert take(log) == [("cd_train_step", None)]
    assert fn._staging is None                          # feed contract: a device-resident table never builds a feed
    assert rbm._n_updates == len(batches) and rbm._rng_step == len(batches)


def test_synchronous_group_reduces_then_applies_the_whole_rule():
    fn, rbm, log, batches, _, _ = make(overlap=False)
    for b in batches:
        fn(indexes=b, momentum=0.5)
        assert take(log) == [("cd_step", None), ("reduce", None), ("apply_update", 0)]
    fn.flush()
    assert take(log) == [] and fn._staging is None


@pytest.mark.parametrize("split", [True, False])
def test_overlapped_group_with_the_update_as_its_own_call(split):
    fn, rbm, log, batches, _, _ = make(split=split)
    fn.fuse_deferred = 0 if split else 1                # (an engine without the two halves never fuses)
    for t, b in enumerate(batches):
        fn(indexes=b, momentum=0.5)
        if t == 0:
            assert take(log) == [("cd_step", None), ("reduce_async", None), ("apply_update", 2)]
        else:
            assert take(log) == [("cd_step", None), ("reduce_async", None), ("wait", None), ("apply_update", 3)]
    fn.flush()
    assert take(log) == [("wait", None), ("apply_update", 1)]
    fn.flush()
    assert take(log) == []


@pytest.mark.parametrize("comm_cus,fuse", [(0, 1), (0, 2), (8, 2)])
def test_overlapped_group_with_the_update_inside_the_statistics_half(comm_cus, fuse):
    fn, rbm, log, batches, eng, _ = make()
    fn.fuse_deferred, fn.comm_cus = fuse, comm_cus
    for t, b in enumerate(batches):
        fn(indexes=b, momentum=0.5)
        if t == 0:
            assert take(log) == [("cd_step", None), ("reduce_async", None), ("apply_update", 2)]
        else:
            assert take(log) == [("cd_forward", None), ("wait", None), ("cd_statistics", 3), ("reduce_async", None)]
    assert eng.comm_cus_seen == {comm_cus}
    fn.flush()
    assert take(log) == [("wait", None), ("apply_update", 1)]


def test_balanced_launches_fuse_only_at_two():
    fn, rbm, log, batches, eng, _ = make()
    fn.comm_cus = 8
    for t, b in enumerate(batches):
        fn.fuse_deferred = 1 if t < 4 else 2            # read at every call
        fn(indexes=b, momentum=0.5)
        names = [n for n, _ in take(log)]
        assert ("cd_forward" in names) == (t >= 4) and ("cd_step" in names) == (t < 4)
    assert eng.comm_cus_seen == {8}


def test_path_attributes_are_read_at_every_call():
    fn, rbm, log, batches, _, _ = make()
    fn(indexes=batches[0], momentum=0.5)
    fn(indexes=batches[1], momentum=0.5)
    assert ("cd_forward", None) in take(log)
    fn.fuse_deferred = 0
    fn(indexes=batches[2], momentum=0.5)
    assert take(log) == [("cd_step", None), ("reduce_async", None), ("wait", None), ("apply_update", 3)]
    fn.flush()
    take(log)
    fn.overlap = False
    fn(indexes=batches[3], momentum=0.5)
    assert take(log) == [("cd_step", None), ("reduce", None), ("apply_update", 0)]


# ------------------------------------------------------------------------------------------------------------------ the hint
def test_next_indexes_rules_of_the_two_paths():
    """Single device: the hint goes to ``cd_train_step`` whenever the step has an index list.  Forward half: only a hint as
    long as the minibatch, as the index tensor of this rank's rows."""
    fn, rbm, log, batches, eng, _ = make(group=None)
    fn(indexes=batches[0], momentum=0.5, next_indexes=batches[2])
    fn(indexes=None, momentum=0.5, next_indexes=batches[1])
    fn(indexes=batches[1], momentum=0.5)
    assert eng.train_step_hints[0] is batches[2] and eng.train_step_hints[1:] == [None, None]

    fn, rbm, log, batches, eng, _ = make()
    fn(indexes=batches[0], momentum=0.5, next_indexes=batches[1])
    fn(indexes=batches[1], momentum=0.5, next_indexes=batches[2])      # 7 rows after 10: not passed
    fn(indexes=batches[2], momentum=0.5)
    fn(indexes=batches[3], momentum=0.5, next_indexes=batches[5])
    hints = eng._engine.forward_hints
    assert hints[0] is None and hints[1] is None and np.array_equal(hints[2].numpy(), batches[5])


# ------------------------------------------------------------------------------------------------------------------ results
def _run(gauss, mode):
    fn, rbm, log, batches, _, _ = make(gauss=gauss, group=None if mode == "single" else "fake", overlap=mode in ("fused", "unfused"))
    fn.fuse_deferred = 1 if mode == "fused" else 0
    costs = [fn(indexes=b, momentum=0.5 if t < 3 else 0.9, lr=lrs(t)) for t, b in enumerate(batches)]
    n_before = len(log)
    mid = rbm.W_speed.get_value().copy()                # reading a speed flushes the pipeline
    flushed = log[n_before:]
    costs = [float(c) for c in costs]
    fn.flush()
    assert len(log) == n_before + len(flushed)          # nothing was left to complete
    out = dict(W=rbm.W.tensor.numpy().copy(), Ws=rbm.W_speed.tensor.numpy().copy(), hb=rbm.hbias.tensor.numpy().copy(),
               hbs=rbm.hbias_speed.tensor.numpy().copy(), vb=rbm.vbias.tensor.numpy().copy(),
               vbs=rbm.vbias_speed.tensor.numpy().copy(), mid=mid, costs=np.array(costs),
               n=np.array([rbm._n_updates, rbm._rng_step]))
    return out, flushed, [n for n, _ in log]


@pytest.fixture(scope="module")
def runs():
    return {(g, m): _run(g, m) for g in (1, 0) for m in ("sync", "unfused", "fused", "single")}


@pytest.mark.parametrize("gauss", [1, 0])
def test_every_path_gives_the_same_run_bit_for_bit(runs, gauss):
    sync = runs[(gauss, "sync")][0]
    for mode in ("unfused", "fused", "single"):        # (one rank owning every row under an identity sum IS the single device)
        other = runs[(gauss, mode)][0]
        for key in sync:
            assert np.array_equal(sync[key], other[key]), (mode, key)
    assert np.array_equal(sync["mid"], sync["Ws"].astype(np.float32))      # (get_value is float32) nothing was left undone
    assert "cd_forward" in runs[(gauss, "fused")][2] and "cd_forward" not in runs[(gauss, "unfused")][2]


@pytest.mark.parametrize("gauss", [1, 0])
def test_reading_a_speed_mid_run_flushes(runs, gauss):
    for mode in ("unfused", "fused"):
        assert runs[(gauss, mode)][1] == [("wait", None), ("apply_update", 1)], mode
    assert runs[(gauss, "sync")][1] == []


def test_float_of_the_last_cost_completes_its_step():
    ref = _run(1, "sync")[0]
    for fuse in (0, 1):
        fn, rbm, log, batches, _, _ = make()
        fn.fuse_deferred = fuse
        costs = [fn(indexes=b, momentum=0.5 if t < 3 else 0.9, lr=lrs(t)) for t, b in enumerate(batches)]
        take(log)
        assert float(costs[2]) == ref["costs"][2] and take(log) == []       # an earlier step's cost is there already
        assert float(costs[-1]) == ref["costs"][-1]
        assert take(log) == [("wait", None), ("apply_update", 1)]
        assert np.array_equal(rbm.W_speed.tensor.numpy(), ref["Ws"])
        fn.flush()
        assert take(log) == []


# ------------------------------------------------------------------------------------------------------------------ no rows
@pytest.mark.parametrize("overlap,fuse", [(False, 1), (True, 0), (True, 1)])
def test_a_rank_that_owns_no_row_still_reduces(overlap, fuse):
    fn, rbm, log, batches, _, grp = make(overlap=overlap, empty=True)
    fn.fuse_deferred = fuse
    for t, b in enumerate(batches):
        fn(indexes=b, momentum=0.5)
        got = take(log)
        assert not [n for n, _ in got if n.startswith("cd_")]
        if not overlap:
            assert got == [("reduce", None), ("apply_update", 0)]
        elif t == 0:
            assert got == [("reduce_async", None), ("apply_update", 2)]
        else:
            assert got == [("reduce_async", None), ("wait", None), ("apply_update", 3)]
    assert grp.reduced_abs_sums == [0.0] * len(batches)                     # zeroed statistics went into every collective
    fn.flush()
    assert rbm._n_updates == len(batches) and rbm._rng_step == len(batches)
