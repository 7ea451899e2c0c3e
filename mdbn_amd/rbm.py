"""RBM / GRBM with the class surface of the reference's src/rbm.py, executed eagerly on
MI355X through the HIP engine (no Theano graphs).

Where the reference returns symbolic expressions these methods return device arrays
(``SharedArray``; ``numpy.asarray`` / ``.get_value()`` bring them to the host).  The
compiled step function of the reference -- ``theano.function(..., updates=updates,
givens={input: train_set_x[indexes], momentum: m})`` (rbm.py:533-544, dbn.py:302-312) --
is ``mdbn_amd.function(updates, train_set_x)``, called as ``fn(indexes=, momentum=, lr=)``.

Randomness: Philox streams addressed by (seed, stream, step, draw, global row); every
sampling call and every step-function call consumes one ``step`` (see csrc/philox.h).
"""
from __future__ import print_function

import os
import timeit
from collections import deque, namedtuple

import numpy
import torch

from . import dist as _dist
from .engine import GroupTable, RngAddr, get_engine
from .rng import RandomStreams
from .shared import HostTable, SharedArray, as_tensor, shared, weight_ld
from .utils import get_minibatches_idx, group_boundaries


class Scalar(object):
    """A symbolic scalar input of a step function (``tensor.scalar('lr')``, dbn.py:272)."""

    def __init__(self, name):
        self.name = name


class CostHandle(object):
    """What ``get_cost_updates`` returns as the monitoring cost: the value itself is
    produced by each call of the step function (rbm.py:367-374)."""

    def __init__(self, kind):
        self.kind = kind      # 'reconstruction' | 'pseudo_likelihood'


class UpdatePlan(object):
    """The ``updates`` dictionary of rbm.py:353-371 in closed form: everything one
    CD-k / PCD-k step needs, bound when ``get_cost_updates`` is called."""

    def __init__(self, rbm, lr, k, lambda_1, lambda_2, weightcost, batch_size, persistent, W0,
                 symbolic_grad=False, centered=False, offset_rate=0.01, sparsity_target=None, sparsity_cost=0.0,
                 sparsity_decay=0.9, sparsity_weights=True, grouped=None, learn_sigma=None, disc_weight=None, gen_weight=1.0,
                 label_span=None, absent=False):
        self.rbm, self.lr, self.k = rbm, lr, int(k)
        self.lambda_1, self.lambda_2, self.weightcost = lambda_1, lambda_2, weightcost
        self.batch_size, self.persistent, self.W0 = batch_size, persistent, W0
        # compute_symbolic_grad (rbm.py:378-390): negative data = nv_samples[-1], no weight-cost
        # term, true means (the batch_size argument is not used)
        self.symbolic_grad = bool(symbolic_grad)
        # centred gradient (StepFunction._statistics_step): the statistics are referred to the layer's running offsets
        # rbm.v_offset / rbm.h_offset, which slide towards the batch means by offset_rate per step
        self.centered, self.offset_rate = bool(centered), float(offset_rate)
        # sparsity target (StepFunction._statistics_step): a penalty of sparsity_cost drives the layer's running estimate
        # rbm.h_activity of every hidden unit's mean activation towards sparsity_target; sparsity_weights=False: through the
        # hidden biases only
        self.sparse = sparsity_target is not None and float(sparsity_cost) > 0.0
        self.sparsity_target = None if sparsity_target is None else float(sparsity_target)
        self.sparsity_cost, self.sparsity_decay = float(sparsity_cost), float(sparsity_decay)
        self.sparsity_weights = bool(sparsity_weights)
        # categorical visible units (StepFunction._statistics_step): the layer's GroupTable when its visibles hold softmax
        # groups -- the step's statistics then come from engine.cd_step_grouped --, else None
        self.grouped = grouped
        # learned per-column variance (StepFunction._statistics_step): a layer with ``log_sigma`` trains on its rows in units
        # x exp(-log_sigma); ``learn_sigma``: the rate of log_sigma's own exact gradient step, None: sigma stays as it is
        self.sigma = rbm.log_sigma is not None
        self.learn_sigma = None if learn_sigma is None else float(learn_sigma)
        # classification RBM (StepFunction._statistics_step): ``disc_weight`` w > 0 adds w x the exact gradient of
        # sum_rows log p(label | rest) for the label block ``label_span`` = (first column, K) to ``gen_weight`` x the CD
        # statistics; gen_weight = 0: purely discriminative, no chain is run.  None: none of it
        self.disc_weight = None if disc_weight is None else float(disc_weight)
        self.gen_weight, self.label_span = float(gen_weight), label_span
        # absent visible units (StepFunction._statistics_step): NaN in the table means "this row did not observe this unit";
        # the step's statistics then come from engine.cd_step_absent (CD with a per-row mask).  False: none of it
        self.absent = bool(absent)


class LazyCost(object):
    """Monitoring cost of a data-parallel step whose all-reduce is still in flight: resolving
    it (``float(c)``) completes the deferred part of that step first."""

    def __init__(self, stepfn, token):
        self._stepfn, self._token, self._value = stepfn, token, None

    def _resolve(self):
        if self._value is None:
            self._stepfn._resolve_cost(self)
        return self._value

    def reshape(self, *shape):
        return self._resolve().reshape(*shape)

    def __float__(self):
        return float(self._resolve())

    def item(self):
        return float(self)


# What engine.sparsity_activity reads of a CD step's scratch, for hidden means that no CD step made (RBM.hidden_activity)
ActivityRows = namedtuple("ActivityRows", "P2")

# The rows one call trains on: the matrix and the index tensor of THIS rank's rows (None: all of ``data``), the size of the whole
# minibatch, the rank's rows [lo, hi) of it, and whether ``data`` is a buffer of a HostFeed (to be handed back).
Minibatch = namedtuple("Minibatch", "data idx n_global lo hi staged")
Hyper = namedtuple("Hyper", "lr momentum batch_size n_rows cost_scale ldv")     # of one step's update, beside the plan's constants
Pending = namedtuple("Pending", "work stats hyper lazy")    # deferred half of an overlapped step: all-reduce in flight, ..., LazyCost


class HostFeed(object):
    """Feed of a host-resident training table (shared.HostTable) into the steps of one step function, through a RowFeeder
    (engine.row_feeder, mdbn_feeder_*): CPU threads gather an ANNOUNCED minibatch's rows into pinned staging, one SDMA copy
    moves them, three slots deep -- no kernel runs beside the step (a PCIe gather kernel there costs it 60 us).  Unannounced
    minibatches are gathered on the spot by the PCIe gather kernel, in stream order.  ``shard(n)``: this rank's rows of an
    n-row minibatch."""

    def __init__(self, engine, shard):
        self.engine, self.shard = engine, shard
        self.feeder, self.queue = None, deque()     # RowFeeder; announced and submitted: (key, ticket, n_global, lo, hi, key version)
        self.held, self.now = None, None            # ticket of the fed buffer the current step reads; buffer of unannounced rows

    @staticmethod
    def _same_indexes(a, b):
        if a is b:
            return True
        if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor):
            # the prefetched view is kept alive, so its storage cannot have been reused: equal address, length and
            # type mean the same (never mutated) index list
            return a.data_ptr() == b.data_ptr() and a.numel() == b.numel() and a.dtype == b.dtype and a.device == b.device
        if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
            return False
        a, b = numpy.asarray(a), numpy.asarray(b)
        return a.shape == b.shape and bool((a == b).all())

    def announce(self, table, batches, host_indexes):
        """``batches`` (non-empty list) are the next calls' ``indexes``, ``host_indexes`` the same values on the host:
        whatever was announced before is void, their rows start moving now."""
        self.drop()
        shards = []
        for key, h in zip(batches, host_indexes):
            h = h if isinstance(h, torch.Tensor) else torch.from_numpy(numpy.ascontiguousarray(numpy.asarray(h), dtype=numpy.int64))
            h = h.to(torch.int64).reshape(-1)
            if len(h):      # as engine.index_tensor: numpy fancy indexing (negative values count from the end)
                lo_i, hi_i = int(h.min()), int(h.max())
                if lo_i < -len(table) or hi_i >= len(table):
                    raise IndexError("minibatch index out of range for %d rows: [%d, %d]" % (len(table), lo_i, hi_i))
                if lo_i < 0:
                    h = torch.where(h < 0, h + len(table), h)
            lo, hi = self.shard(len(h))
            shards.append((key, h[lo:hi].contiguous(), len(h), lo, hi))
        need = max(hi - lo for _, _, _, lo, hi in shards)
        fd = self.feeder
        if need > 0 and (fd is None or fd.max_rows < need or fd.host is not table.host):     # (set_value replaces .host)
            if fd is not None:
                fd.close()
            fd = self.feeder = self.engine.row_feeder(table.host, table.cols, need)
        for key, h, n_global, lo, hi in shards:
            ticket = fd.submit(h) if hi > lo else None
            # (the version counter of an announced index TENSOR: a buffer refilled in place afterwards is not the announced list)
            self.queue.append((key, ticket, n_global, lo, hi, getattr(key, "_version", None)))

    def drop(self):
        """Void every announcement (and hand back a buffer still held)."""
        self.consumed()
        if self.queue:
            self.queue.clear()
            if self.feeder is not None:
                self.feeder.cancel()

    def take(self, table, indexes):
        """The Minibatch of this step: this rank's rows in a device buffer -- the fed one if ``indexes`` is what was announced
        next, else gathered now by the PCIe kernel -- to be read with the identity index."""
        eng = self.engine
        self.consumed()                            # (a step that raised before handing its rows back)
        if self.queue:
            key, ticket, n_global, lo, hi, key_version = self.queue[0]
            if self._same_indexes(key, indexes) and key_version == getattr(indexes, "_version", None):
                self.queue.popleft()
                if ticket is None:
                    return Minibatch(eng.alloc_matrix(0, table.cols, table.host.stride(0)), None, n_global, lo, hi, True)
                buf = self.feeder.acquire(ticket, hi - lo)
                self.held = ticket
                return Minibatch(buf, None, n_global, lo, hi, True)
            self.drop()                            # not what was announced: the remaining announcements are void
        n_global = len(table) if indexes is None else len(indexes)
        lo, hi = self.shard(n_global)
        buf = self.now
        if buf is None or buf.shape[0] != hi - lo:
            buf = self.now = eng.alloc_matrix(hi - lo, table.cols, table.host.stride(0))
        if hi > lo:
            idx = torch.arange(lo, hi, dtype=torch.int64, device=eng.device) if indexes is None else \
                eng.index_tensor(indexes, len(table))[lo:hi]
            table.rows(idx, out=buf)               # same stream as the steps: the previous reader of `buf` is ahead of it
        return Minibatch(buf, None, n_global, lo, hi, True)

    def consumed(self):
        """The step that reads the fed rows has been enqueued: their slot may be refilled after it."""
        if self.held is not None:
            self.feeder.release(self.held)
            self.held = None


class StepFunction(object):
    """One compiled training step: ``fn(indexes=, momentum=, lr=)`` -> monitoring cost
    (0-d device tensor; ``float(cost)`` synchronises).

    Data-parallel: with an initialised ``torch.distributed`` group of N ranks
    each rank computes the statistics of its contiguous slice of the minibatch, the packed
    [S | s_h | s_v | cost] buffer is sum-all-reduced (RCCL over xGMI), and every rank applies
    the same update; ``batch_size`` is the global minibatch size (rbm.py:413).

    Overlap: the parameter step uses the OLD speed (rbm.py:364-365), so theta(t+1) does not
    depend on step t's gradient.  With ``overlap=True`` (default when eligible: lambda_1 == 0
    and weightcost == 0 or a frozen W0) the all-reduce of step t is started asynchronously,
    theta(t+1) is applied at once, and the speed update that needs the reduced statistics runs
    at the end of step t+1 -- the collective hides behind a whole step of compute while every
    value stays bit-identical to the synchronous order.  ``flush()`` completes the deferred
    part (called automatically when speeds or the cost are read)."""

    accepts_next_indexes = True         # fn(indexes=, momentum=, lr=, next_indexes=): the trainers pass the hint when they can

    def __init__(self, updates, train_set_x, input_fn=None, name=None, data_parallel="auto", overlap=True):
        self.plan = updates
        self.rbm = updates.rbm
        self.engine = self.rbm.engine
        self.train_set_x = train_set_x
        self.input_fn = input_fn            # maps the DBN's data matrix to this layer's input
        self.name = name
        self.group = _dist.default_group() if data_parallel == "auto" else data_parallel
        p = updates
        self.overlap = bool(overlap and self.group is not None and self.group.world_size > 1
                            and p.persistent is None and p.lambda_1 == 0.0
                            and (p.weightcost == 0.0 or p.W0 is not None))
        if p.centered and self.group is not None and self.group.world_size > 1:
            raise NotImplementedError("centered=True on a data-parallel group of %d ranks: the offsets need the means of the "
                                      "whole minibatch in the all-reduce, which is not built yet" % self.group.world_size)
        if p.sparse and self.group is not None and self.group.world_size > 1:
            raise NotImplementedError("a sparsity target on a data-parallel group of %d ranks: the activity estimate needs "
                                      "the means of the whole minibatch in the all-reduce, which is not built yet"
                                      % self.group.world_size)
        if p.grouped is not None and self.group is not None and self.group.world_size > 1:
            raise NotImplementedError("categorical visible units (visible_groups) on a data-parallel group of %d ranks: the "
                                      "grouped step is not sharded yet" % self.group.world_size)
        if p.sigma and self.group is not None and self.group.world_size > 1:
            raise NotImplementedError("a layer with log_sigma (learned per-column variance) on a data-parallel group of %d "
                                      "ranks: the step of log_sigma needs the rows of the whole minibatch, which is not "
                                      "built yet" % self.group.world_size)
        if p.absent:
            if self.group is not None and self.group.world_size > 1:
                raise NotImplementedError("missing=True on a data-parallel group of %d ranks: the absent-unit step is not "
                                          "sharded yet" % self.group.world_size)
            if not hasattr(self.rbm.engine, "cd_step_absent"):
                raise NotImplementedError("missing=True needs an engine with the absent-unit step (cd_step_absent); %s has none"
                                          % type(self.rbm.engine).__name__)
        self.discriminative_nll = None      # 0-d device tensor: -sum log p(label | rest) of the last minibatch (a discriminative plan)
        if p.disc_weight is not None:
            if self.group is not None and self.group.world_size > 1:
                raise NotImplementedError("discriminative= on a data-parallel group of %d ranks: the discriminative statistics "
                                          "are not sharded yet" % self.group.world_size)
            if not hasattr(self.rbm.engine, "class_stats"):
                raise NotImplementedError("discriminative= needs an engine with the classification calls (class_stats); %s has "
                                          "none" % type(self.rbm.engine).__name__)
            if input_fn is None and train_set_x is not None:
                # (once, on the host: a label block that is not one-hot has no category to train for)
                lo, K = p.label_span
                self.rbm._check_one_hot(train_set_x, spans=[(lo, lo + K)])
        self._pending = None                # Pending: the deferred half of the last overlapped step
        self._feed = None                   # HostFeed of a host-resident table, made by its first announcement or step
        self._n_calls = 0
        eng = self.engine                   # what the engine offers (the checker engine lacks most of it)
        self._has_feeder, self._has_cache = hasattr(eng, "row_feeder"), hasattr(eng, "cd_train_step_cached")
        self._has_forward, self._has_count = getattr(eng, "cd_forward", None) is not None, hasattr(eng, "count_nonfinite")
        # statistics buffers of the data-parallel path are OWNED by this step function: a deferred
        # update reads them a whole call later, so another step function of the same shape (two
        # equal-sized modalities, alternating layers) must not share them
        self._stats_slots = [None, None]
        self._v_mean = None                 # [V] means of v0 of the current minibatch (a sparse step with sparsity_weights)
        self._sigma_rows = {}               # n -> ([n, V] staging of the minibatch in units, [n, V] conditional means): a layer with log_sigma
        self._fast = []                     # warm: [engine.StepCache] of the previous single-device call (cd_train_step_cached)
        # nan_guard: check cost and parameters for NaN / Inf after every call (synchronises; what the
        # reference's commented-out NanGuardMode would do, rbm.py:542-543, dbn.py:311)
        self.nan_guard = bool(getattr(self.engine, "nan_guard", False))
        self.comm_cus = 0
        # Overlapped data-parallel order with the deferred update of step t-1 INSIDE the statistics GEMM of step t (one
        # launch and one queue packet fewer: 163 -> 146 us per step without a collective on one GPU), at the price of waiting
        # for the all-reduce of step t-1 before that GEMM instead of after it (~100 us of cover instead of ~150).  The
        # balanced launches (comm_cus > 0) can carry it too (a flat share of the arrays per workgroup), but gain only 3 us
        # from it and lose the longer cover (185.0 vs 187.8 us alone, 216 vs 203 beside a 120-us stand-in): only with
        # MDBN_DP_FUSED_UPDATE=2 / fn.fuse_deferred = 2.  0 restores the update launch after the step everywhere;
        # bench.py --gpus N measures all of them.
        self.fuse_deferred = int(os.environ.get("MDBN_DP_FUSED_UPDATE", "1"))       # 0 | 1 | 2 (2: balanced launches too)
        if self.group is not None and self.group.world_size > 1 and hasattr(eng, "set_option"):
            # The collective's kernels run beside the next step's GEMMs and take whole CUs (RCCL's gfx950 all-reduce
            # kernel: 248-256 VGPRs per wave, 37.6 KB LDS -- nothing of ours fits next to it), and a one-workgroup-per-
            # CU GEMM grid on fewer CUs needs a second round: measured 163 -> 219 us per step with EIGHT CUs taken.
            # So an overlapped data-parallel step CAN leave `comm_cus` CUs to the collective and launch its GEMMs
            # balanced on the rest (mdbn_planes.hip, "BALANCED launches"): MDBN_COMM_CUS /
            # fn.comm_cus, default 0 (dist.DEFAULT_COMM_CUS says why); bench.py --gpus N measures the choices.
            self.comm_cus = _dist.comm_cus() if self.overlap else 0      # handed to every cd_step call
            self.engine.set_option("gemm_cw", 1)        # exact-f32 fallback kernels: one MFMA wave per SIMD
        if self.overlap:
            for arr in self.rbm.params_speed:
                arr._sync_hook = self.flush

    # -- where the minibatch comes from
    def _data(self):
        if self.input_fn is not None:
            return self.input_fn()
        return self.engine.as_matrix(self.train_set_x)

    def _host_table(self):
        return self.train_set_x if (self.input_fn is None and isinstance(self.train_set_x, HostTable)) else None

    def _shard(self, n_global):
        return (0, n_global) if self.group is None else self.group.shard(n_global)

    def _host_feed(self):
        if self._feed is None:
            self._feed = HostFeed(self.engine, self._shard)
        return self._feed

    _staging = property(lambda self: None if self._feed is None else vars(self._feed))     # the feed's state as a mapping

    def announce(self, batches, host_indexes=None):
        """Tell the step function which minibatches come next, in order (the trainers know the epoch's order up front):
        with a host-resident table their rows start moving now, up to two minibatches ahead of the step that reads them.
        ``batches``: the index lists / tensors exactly as the following calls will pass them; ``host_indexes``: the same
        values as host arrays, when the caller has them (saves one device-to-host copy of the list).  A pure hint: a call
        whose ``indexes`` are not the announced ones drops the remaining announcements.  No-op for device-resident data."""
        table = self._host_table()
        if table is None or not torch.cuda.is_available() or not self._has_feeder:
            return
        batches = list(batches)
        if not batches:
            return
        if host_indexes is None:
            if any(isinstance(b, torch.Tensor) and b.device.type != "cpu" for b in batches):
                flat = torch.cat([torch.as_tensor(b).reshape(-1).to(torch.int64) for b in batches]).cpu()   # one copy for all
                host_indexes = list(torch.split(flat, [len(b) for b in batches]))
            else:
                host_indexes = batches
        self._host_feed().announce(table, batches, host_indexes)

    def prefetch(self, indexes):
        """``announce([indexes])``: the next minibatch only."""
        self.announce([indexes])

    def _minibatch(self, indexes):
        """The Minibatch of this call, from either source."""
        table = self._host_table()
        if table is not None and torch.cuda.is_available():
            # the shard's rows arrive in a device buffer (fed ahead of the step when announced), read with the identity index
            return self._host_feed().take(table, indexes)
        data = self._data()
        n_global = data.shape[0] if indexes is None else len(indexes)
        lo, hi = self._shard(n_global)      # data-parallel shard of the minibatch: contiguous rows [lo, hi) of `indexes`
        if indexes is None:
            idx = None if (lo == 0 and hi == data.shape[0]) else torch.arange(lo, hi, dtype=torch.int64, device=data.device)
        else:
            idx = self.engine.index_tensor(indexes, data.shape[0])
            if lo != 0 or hi != n_global:   # (a view of everything would be the same list: as much host time as the record costs)
                idx = idx[lo:hi]
        return Minibatch(data, idx, n_global, lo, hi, False)

    def _rows_consumed(self, mb, next_indexes):
        """The step reading ``mb`` has been enqueued: fed rows go back, and the next shard of a host table starts moving."""
        if mb.staged:
            self._feed.consumed()
            if next_indexes is not None and not self._feed.queue:
                self.announce([next_indexes])

    # -- the one statement of what every path passes to the engine
    def _params(self):
        """(W, W_speed, W0, hbias, hbias_speed, vbias, vbias_speed), as cd_train_step and apply_update take them."""
        rbm, W0 = self.rbm, self.plan.W0
        return (rbm.W.tensor, rbm.W_speed.tensor, W0.tensor if W0 is not None else None,
                rbm.hbias.tensor, rbm.hbias_speed.tensor, rbm.vbias.tensor, rbm.vbias_speed.tensor)

    def _update_args(self, stats, hp, phase):
        """The 18 arguments of ``apply_update`` (and of ``cd_statistics(deferred=)``)."""
        p = self.plan
        return self._params() + (stats, hp.lr, p.lambda_1, p.lambda_2, p.weightcost, hp.momentum, hp.batch_size, hp.n_rows,
                                 hp.cost_scale, phase, hp.ldv)

    def _rng_addr(self, step, lo):
        return RngAddr(self.rbm.theano_rng.seed, self.rbm.stream_id, step, 0, lo)

    def _cost_scale(self, n_global):
        # rbm.py:480 (sum over units, mean over rows) / rbm.py:697 (mean over everything)
        return 1.0 / (n_global * self.rbm.n_visible) if self.rbm.gauss else 1.0 / n_global

    # -- deferred half of an overlapped step: speeds (and cost) from the reduced statistics
    def _take_pending(self):                        # the pending step, its all-reduce awaited (on the stream)
        pend, self._pending = self._pending, None
        pend.work.wait()
        return pend

    def _deferred_args(self, pend, lr):
        """Speeds from the reduced statistics of step t-1, then theta(t+1) from those speeds: phases 1 and 2 touch the same
        arrays, so they run as ONE pass (phase 3; the speed half keeps step t-1's momentum and divisors, the other this lr)."""
        return self._update_args(pend.stats, pend.hyper._replace(lr=lr), 3)

    def flush(self):
        """Complete the deferred speed update of the last overlapped step (no-op otherwise)."""
        if self._pending is not None:
            pend = self._take_pending()
            pend.lazy._value = self.engine.apply_update(*self._update_args(pend.stats, pend.hyper, 1))

    def _resolve_cost(self, lazy):
        if self._pending is not None and self._pending.lazy is lazy:
            self.flush()
        if lazy._value is None:
            raise RuntimeError("cost of a step that was never completed")

    def __call__(self, indexes=None, momentum=0.0, lr=None, next_indexes=None):
        """``next_indexes``: the minibatch of the NEXT call, when the caller knows it (the trainers do: the epoch's order
        is drawn up front, dbn.py:446-458) -- a pure hint: the single-device plane path then gathers those rows inside
        this step's statistics kernel, a host-resident table starts moving them over PCIe; results never change."""
        p = self.plan
        if lr is None:
            lr = p.lr
        if isinstance(lr, Scalar):
            raise TypeError("step function needs lr= (learning rate is a symbolic input)")
        mb = self._minibatch(indexes)
        batch_size = p.batch_size if (p.batch_size is not None and not p.symbolic_grad) else mb.n_global
        step = self.rbm._take_step()
        distributed = self.group is not None and self.group.world_size > 1
        if p.centered or p.sparse or p.grouped is not None or p.sigma or p.absent:
            return self._statistics_step(mb, step, lr, momentum, batch_size, next_indexes)
        if not distributed and p.persistent is None and mb.hi > mb.lo:
            return self._single_device_step(mb, step, lr, momentum, batch_size, next_indexes)
        return self._group_step(mb, step, lr, momentum, batch_size, next_indexes, distributed)

    @property
    def discriminative_cost(self):
        """Mean -log p(label | rest) over the last minibatch, at the parameters before its update (a plan with
        ``discriminative=``; None before the first step).  Reading it synchronises."""
        if self.discriminative_nll is None:
            return None
        return float(self.discriminative_nll) / self._disc_rows

    def _single_device_step(self, mb, step, lr, momentum, batch_size, next_indexes):
        """The whole step function in one library call (mdbn_cd_train_step)."""
        p, rbm, eng = self.plan, self.rbm, self.engine
        params = self._params()
        if self._fast and mb.idx is not None and not mb.staged and not self.nan_guard:
            # the argument structs of the previous call (small layers are host-bound: engine.cd_train_step_cached)
            out = eng.cd_train_step_cached(self._fast, mb.data, mb.idx, params, batch_size, mb.n_global, step, lr, momentum, next_indexes)
            if out is not None:
                rbm._n_updates += 1
                return out
        extra = {"cache_out": self._fast} if self._has_cache else {}
        if next_indexes is not None and mb.idx is not None and not mb.staged:
            extra["next_indexes"] = next_indexes        # the train-step hint: as it came, whenever the step has an index list
        out = eng.cd_train_step(mb.data, mb.idx, *params, rbm.gauss, p.k, self._rng_addr(step, mb.lo), lr, p.lambda_1,
                                p.lambda_2, p.weightcost, momentum, batch_size, mb.n_global, self._cost_scale(mb.n_global),
                                sample_stats=p.symbolic_grad, **extra)
        rbm._n_updates += 1
        self._rows_consumed(mb, next_indexes)
        if self.nan_guard:
            self._check_finite(out)
        return out

    def _group_step(self, mb, step, lr, momentum, batch_size, next_indexes, distributed):
        """The step in pieces -- statistics of this rank's rows, (all-reduce,) update: data parallel, and PCD anywhere."""
        p, rbm, eng = self.plan, self.rbm, self.engine
        data = mb.data
        persistent = None
        if p.persistent is not None:
            persistent = p.persistent.tensor
            if persistent.shape[0] != mb.n_global:
                raise ValueError("persistent chain has %d rows but the minibatch has %d (the reference fails the same way, "
                                 "rbm.py:416)" % (persistent.shape[0], mb.n_global))
            if distributed:
                # PCD under data parallelism: chain row g belongs to the rank that owns minibatch row g
                # (rbm.py:308-311,369); a rank only ever reads and writes its own rows of the chain
                persistent = persistent[mb.lo:mb.hi]
        slot = self._n_calls & 1 if self.overlap else 0     # the other buffer may still be reducing
        self._n_calls += 1
        if self._stats_slots[slot] is None:
            self._stats_slots[slot] = eng.new_stats_buffer(rbm.n_visible, rbm.n_hidden, data.stride(0), rbm.W.tensor.stride(0))
        stats = self._stats_slots[slot]
        deferred_done = False
        if mb.hi > mb.lo:
            extra = {"comm_cus": self.comm_cus} if self.comm_cus else {}
            if self.overlap and self._pending is not None and self._has_forward and \
                    int(self.fuse_deferred) >= (2 if self.comm_cus else 1):
                self._forward_then_statistics(mb, step, lr, stats, next_indexes, extra)
                deferred_done = True
            else:
                eng.cd_step(data, mb.idx, rbm.W.tensor, rbm.hbias.tensor, rbm.vbias.tensor, rbm.gauss, p.k,
                            self._rng_addr(step, mb.lo), persistent=persistent, sample_stats=p.symbolic_grad, stats=stats, **extra)
        else:                                  # this rank holds no row of a short minibatch
            stats.zero_()
        cost, cost_scale = self._pcd_monitor(mb, stats, distributed) if p.persistent is not None else \
            (None, self._cost_scale(mb.n_global))
        self._rows_consumed(mb, next_indexes)        # host-resident table: the next shard starts moving now
        hp = Hyper(lr, momentum, batch_size, mb.n_global, cost_scale, data.stride(0))
        if self.overlap:
            return self._overlapped_tail(stats, hp, deferred_done)
        if distributed:
            self.group.all_reduce_sum(stats, eng)
        out = eng.apply_update(*self._update_args(stats, hp, 0))
        rbm._n_updates += 1
        if self.nan_guard:
            self._check_finite(cost if cost is not None else out)
        return cost if cost is not None else out

    def _statistics_step(self, mb, step, lr, momentum, batch_size, next_indexes):
        """The step in the order statistics, transforms, update -- CD or PCD on one device: the statistics are materialised
        (with the float32 copies of v0 / ph_mean in the scratch), transformed in place, and the unchanged update rule runs on
        them.

        Sparsity target (Hinton's guide, section 11): the layer's activity estimate q slides towards the means of ph_mean
        of this minibatch (the first sparse step of a layer sets it to those means), then with t = target - q,
        s_h += cost n_rows t and, unless sparsity_weights is off, S += cost batch_size <v0> t'.

        Centred gradient (Melchior et al. 2016, Algorithm 1), after the sparsity transform: the offsets slide towards the
        means of v0 and ph_mean of this minibatch (the first step of a layer sets them to those means), the statistics are
        corrected for the offsets -- S' = S - mu s_h' - s_v lam', s_v' = s_v - rho S' lam, s_h' = s_h - rho S'^T mu,
        rho = n_rows / batch_size.

        Categorical visible units (a layer with ``visible_groups``): the statistics come from ``cd_step_grouped`` -- inside a
        group p(v | h) is a softmax and the chain carries one-hot samples --, everything after that call is unchanged, so
        both transforms compose with it.  The monitoring cost is the cost slot of that call, the cross-entropy of the last
        Gibbs step against v0 (categorical inside the groups), under PCD too: the pseudo-likelihood flips one bit, and a
        one-hot group with one bit flipped is outside the model's support.

        Learned per-column variance (a GRBM with ``log_sigma`` s): the minibatch is gathered as u = x exp(-s), the rows in
        units (``sigma_scale_rows`` into a staging matrix this step function keeps), and the unchanged CD step runs on that
        staging matrix with the identity index -- statistics, offsets and activities all live in units, so both transforms
        compose without change, and the monitoring cost is the cost slot of that call, in units.  With ``learn_sigma`` the
        conditional means m = vbias + ph_mean W^T (one noise-free propdown of the scratch's ph_mean, no RNG step) and
        ``sigma_update`` follow: g = mean_r[u (u - m)] - 1, exact -- no chain state enters --, taken at the parameters of
        before ``apply_update``; log_sigma then takes the visible bias's rule at rate ``learn_sigma``, clamped to
        ``GRBM.log_sigma_range``.

        Classification RBM (a plan with ``disc_weight`` w; Larochelle & Bengio 2008): right after the grouped CD step, and
        before the sparsity transform, ``class_stats`` replaces the statistics by gen_weight x (those of the CD step) + w x
        (the exact gradient of sum_rows log p(label | rest)) -- one statistics GEMM on the stacked operands of both.  With
        gen_weight = 0 no chain is run: the rows are gathered and ``class_stats`` forms the discriminative statistics alone;
        the monitoring cost is then the mean -log p(label | rest), which ``discriminative_cost`` gives in both forms.

        Absent visible units (a plan with ``absent``: ``get_cost_updates(missing=True)``; Salakhutdinov, Mnih & Hinton 2007):
        the statistics come from ``cd_step_absent`` -- a NaN of the table is a unit the row's RBM does not have, v0 and nv are
        zero there --, everything after that call is unchanged.  The divisors stay the batch size: the step follows the mean
        log-likelihood per row.  The monitoring cost is summed over the observed entries only, so the costs of tables with
        different missingness do not compare."""
        p, rbm, eng = self.plan, self.rbm, self.engine
        data = mb.data
        fed = mb                                        # the rows as they arrived (a fed buffer goes back once they are read)
        if p.sigma:
            n = mb.n_global                             # (one device: this call holds the whole minibatch)
            if n not in self._sigma_rows:
                if len(self._sigma_rows) > 4:           # (a full and a ragged minibatch per epoch, as a rule)
                    self._sigma_rows.clear()
                self._sigma_rows[n] = (eng.alloc_matrix(n, rbm.n_visible, data.stride(0)),
                                       eng.alloc_matrix(n, rbm.n_visible, data.stride(0)) if p.learn_sigma is not None else None)
            data, cond_mean = self._sigma_rows[n]
            eng.sigma_scale_rows(mb.data, mb.idx, rbm.log_sigma.tensor, -1.0, out=data)
            mb = mb._replace(data=data, idx=None, staged=False)
        persistent = None
        if p.persistent is not None:
            persistent = p.persistent.tensor
            if persistent.shape[0] != mb.n_global:
                raise ValueError("persistent chain has %d rows but the minibatch has %d (the reference fails the same way, "
                                 "rbm.py:416)" % (persistent.shape[0], mb.n_global))
        V, H, ldv, ldh = rbm.n_visible, rbm.n_hidden, data.stride(0), rbm.W.tensor.stride(0)
        pure = p.disc_weight is not None and p.gen_weight == 0.0
        if pure:                                        # no chain: the gathered rows are all the statistics need
            v0 = eng.gather_rows(data, mb.idx) if mb.idx is not None else data
            ldv = v0.stride(0)
        if self._stats_slots[0] is None:
            self._stats_slots[0] = eng.new_stats_buffer(V, H, ldv, ldh)
        stats = self._stats_slots[0]
        self._n_calls += 1
        if pure:
            lo, K = p.label_span
            self._disc_rows = mb.n_global
            self.discriminative_nll = eng.class_stats(None, v0, mb.n_global, rbm.W.tensor, rbm.hbias.tensor, rbm.vbias.tensor, lo, K,
                                                      0.0, p.disc_weight, stats)
        elif p.absent:
            _, scratch = eng.cd_step_absent(data, mb.idx, rbm.W.tensor, rbm.hbias.tensor, rbm.vbias.tensor, rbm.gauss, p.k,
                                            self._rng_addr(step, mb.lo), add_noise=rbm.gauss and not getattr(rbm, "error_free", True),
                                            stats=stats)
        elif p.grouped is not None:
            _, scratch = eng.cd_step_grouped(data, mb.idx, rbm.W.tensor, rbm.hbias.tensor, rbm.vbias.tensor, p.k,
                                             self._rng_addr(step, mb.lo), p.grouped, persistent=persistent, stats=stats,
                                             keep_f32=True)
            if p.disc_weight is not None:
                lo, K = p.label_span
                self._disc_rows = mb.n_global
                self.discriminative_nll = eng.class_stats(scratch, None, mb.n_global, rbm.W.tensor, rbm.hbias.tensor,
                                                          rbm.vbias.tensor, lo, K, p.gen_weight, p.disc_weight, stats)
        else:
            _, scratch = eng.cd_step(data, mb.idx, rbm.W.tensor, rbm.hbias.tensor, rbm.vbias.tensor, rbm.gauss, p.k,
                                     self._rng_addr(step, mb.lo), persistent=persistent, stats=stats, keep_f32=True)
        if p.sigma and p.learn_sigma is not None:       # (all gradients of a step are taken at the old parameters)
            n = mb.n_global
            eng.propdown(scratch.P2[:n], rbm.W.tensor, rbm.vbias.tensor, gauss=True, out=cond_mean)
            lo, hi = rbm.log_sigma_range
            eng.sigma_update(scratch.V2[:n], cond_mean, n, p.learn_sigma, momentum, lo, hi, rbm.log_sigma.tensor,
                             rbm.log_sigma_speed.tensor)
        sparsity = None                                 # what sparsity_stats was given (the centred row route below needs it)
        if p.sparse:
            first = rbm.h_activity is None
            if first:
                rbm.h_activity = SharedArray(None, engine=eng, _tensor=eng.alloc_vector(H))
            v_mean = None
            if p.sparsity_weights:
                if self._v_mean is None:
                    self._v_mean = eng.alloc_vector(V)
                v_mean = self._v_mean
            eng.sparsity_activity(scratch, mb.n_global, rbm.h_activity.tensor, v_mean, 1.0 if first else 1.0 - p.sparsity_decay)
            sparsity = (rbm.h_activity.tensor, v_mean, p.sparsity_target,
                        p.sparsity_cost * float(batch_size) if p.sparsity_weights else 0.0, p.sparsity_cost * float(mb.n_global))
            eng.sparsity_stats(stats, V, H, ldv, ldh, *sparsity)
        if p.centered:
            first = rbm.v_offset is None
            if first:
                rbm.v_offset = SharedArray(None, engine=eng, _tensor=eng.alloc_vector(V))
                rbm.h_offset = SharedArray(None, engine=eng, _tensor=eng.alloc_vector(H))
            eng.center_offsets(scratch, mb.n_global, rbm.v_offset.tensor, rbm.h_offset.tensor, 1.0 if first else p.offset_rate)
            rho = float(mb.n_global) / float(batch_size)
            # a layer with groups: s_h' from the rows of the scratch, not from S (the same number; on one-hot rows the sum over
            # S cancels (mu . mu) s_h and multiplies the float32 error of S by sum(mu): engine.center_hidden_rows)
            # (with what the sparsity transform added to S and s_h, which the rows do not hold)
            s_h = eng.center_hidden_rows(scratch, mb.n_global, stats, V, H, ldv, ldh, rbm.v_offset.tensor, rbm.h_offset.tensor,
                                         rho, sparsity=sparsity) if p.grouped is not None else None
            eng.center_stats(stats, V, H, ldv, ldh, rbm.v_offset.tensor, rbm.h_offset.tensor, rho)
            if s_h is not None:
                eng.center_stats_store_hidden(stats, V, H, ldh, s_h)
        cost, cost_scale = self._pcd_monitor(mb, stats, False) if (p.persistent is not None and p.grouped is None) else \
            (None, self._cost_scale(mb.n_global))
        self._rows_consumed(fed, next_indexes)
        hp = Hyper(lr, momentum, batch_size, mb.n_global, cost_scale, ldv)
        out = eng.apply_update(*self._update_args(stats, hp, 0))
        rbm._n_updates += 1
        if self.nan_guard:
            self._check_finite(cost if cost is not None else out)
        return cost if cost is not None else out

    def _forward_then_statistics(self, mb, step, lr, stats, next_indexes, extra):
        """Overlapped order with the update INSIDE the statistics GEMM: the forward half of step t (everything that reads
        theta(t)), then wait for the all-reduce of step t-1, then the statistics half, whose kernel applies the deferred
        update of step t-1 (speeds from its reduced statistics, theta(t+1) from those speeds) beside its own main loop --
        bitwise what apply_update(phase=3) after cd_step does, one launch fewer."""
        p, rbm, eng = self.plan, self.rbm, self.engine
        forward_hint = None                         # the forward hint: this rank's rows of a hint as long as the minibatch
        if next_indexes is not None and mb.idx is not None and not mb.staged and len(next_indexes) == mb.n_global:
            forward_hint = eng.index_tensor(next_indexes, mb.data.shape[0])[mb.lo:mb.hi]
        token = eng.cd_forward(mb.data, mb.idx, rbm.W.tensor, rbm.hbias.tensor, rbm.vbias.tensor, rbm.gauss, p.k,
                               self._rng_addr(step, mb.lo), sample_stats=p.symbolic_grad, stats=stats,
                               next_indexes=forward_hint, **extra)
        pend = self._take_pending()
        _, _, pend.lazy._value = eng.cd_statistics(token, deferred=self._deferred_args(pend, lr))

    def _pcd_monitor(self, mb, stats, distributed):
        """PCD monitors the pseudo-likelihood (rbm.py:371) with pre-update parameters: -> (cost or None, cost_scale)."""
        rbm = self.rbm
        if mb.hi > mb.lo:
            cost = rbm._pseudo_likelihood_value(self.engine.gather_rows(mb.data, mb.idx) if mb.idx is not None else mb.data)
        else:
            cost = None
            rbm.bit_i_idx = (rbm.bit_i_idx + 1) % rbm.n_visible
        if not distributed:
            return cost, 0.0
        # a mean over rows: every rank contributes (its mean * its rows) through the cost slot of the
        # statistics buffer, the update kernel divides the all-reduced sum by the global row count
        ldh = rbm.W.tensor.stride(0)
        stats[rbm.n_visible * ldh + ldh + mb.data.stride(0)] = cost * float(mb.hi - mb.lo) if cost is not None else 0.0
        return None, 1.0 / mb.n_global

    def _overlapped_tail(self, stats, hp, deferred_done):
        """Start this step's all-reduce, apply what does not wait for it, leave the rest pending: -> LazyCost."""
        work = self.group.all_reduce_sum_async(stats, self.engine)
        if deferred_done:
            pass                                   # (step t-1's update went into this step's statistics GEMM)
        elif self._pending is not None:
            pend = self._take_pending()
            pend.lazy._value = self.engine.apply_update(*self._deferred_args(pend, hp.lr))
        else:
            self.engine.apply_update(*self._update_args(stats, hp, 2))     # theta(t+1)
        lazy = LazyCost(self, self._n_calls)
        self._pending = Pending(work, stats, hp, lazy)
        self.rbm._n_updates += 1
        return lazy

    def _check_finite(self, cost):
        rbm = self.rbm
        c = float(cost)
        sigma = () if rbm.log_sigma is None else (rbm.log_sigma.tensor, rbm.log_sigma_speed.tensor)
        bad = self.engine.count_nonfinite(rbm.W.tensor, rbm.W_speed.tensor, rbm.hbias.tensor, rbm.vbias.tensor, *sigma) \
            if self._has_count else 0
        if bad or not numpy.isfinite(c):
            raise FloatingPointError("step %d of %s: cost = %r, %d non-finite parameter / speed values (learning rate "
                                     "too large for this data?)" % (rbm._n_updates, self.name or "step function", c, bad))


def function(updates, train_set_x=None, input_fn=None, name=None, data_parallel="auto", overlap=True):
    """Stand-in for ``theano.function([indexes, momentum, lr], cost, updates=updates,
    givens={x: train_set_x[indexes], rbm.momentum: momentum})`` (dbn.py:302-312)."""
    return StepFunction(updates, train_set_x, input_fn=input_fn, name=name,
                        data_parallel=data_parallel, overlap=overlap)


def ais_estimate(logw, base_vbias, n_hidden, gauss, groups=None):
    """``(log_Z, std_err)`` from the per-chain log importance weights of an AIS run (float64 on the host):
    log Z_A + logsumexp(logw) - log M with log Z_A = H log 2 + sum softplus(b_A) (Bernoulli) | H log 2 + V/2 log 2 pi
    (unit-variance Gaussian visibles), and the delta-method standard error std(w) / (mean(w) sqrt(M)).  ``groups`` (a
    ``GroupTable`` or its boundaries): the weights of a run on a layer with softmax groups (``HipEngine.ais_grouped``) --
    a group contributes logsumexp_{c in g} b_A,c to log Z_A (``temper.base_log_partition``)."""
    from .temper import base_log_partition
    logw = numpy.asarray(logw, dtype=numpy.float64)
    log_ZA = base_log_partition(base_vbias, n_hidden, gauss, groups)
    top = logw.max()
    w = numpy.exp(logw - top)
    log_Z = log_ZA + top + numpy.log(w.mean())
    err = w.std() / (w.mean() * numpy.sqrt(w.size))
    return float(log_Z), float(err)


def ais_estimate_rows(logw, base_vbias, mask, n_hidden, gauss, groups=None):
    """``(log_Z [N], std_err [N])`` from the log importance weights ``logw`` [N, C] of a clamped AIS run (float64 on the host),
    per data row r: log Z_A,r + logsumexp_c(logw[r]) - log C, with the base-rate model over the row's free columns (``mask``
    [1 | N, V] zero) alone -- log Z_A,r = H log 2 + sum_free softplus(b_A) (Bernoulli) | H log 2 + |free| / 2 log 2 pi
    (Gaussian) -- and ``ais_estimate``'s delta-method standard error std(w) / (mean(w) sqrt(C)) of each row.  ``groups`` (a
    ``GroupTable`` or its boundaries; Bernoulli only): the weights of a run on a layer with softmax groups
    (``HipEngine.ais_conditional_grouped``) -- a group is free when the mask at its FIRST column is 0, and a free group
    contributes logsumexp_{c in g} b_A,c instead of its columns' softplus."""
    logw = numpy.asarray(logw, dtype=numpy.float64)
    free = numpy.broadcast_to(numpy.asarray(mask) == 0, (logw.shape[0], numpy.asarray(mask).shape[1]))
    bA = numpy.asarray(base_vbias, dtype=numpy.float64)
    per_col = numpy.full(bA.shape, 0.5 * numpy.log(2.0 * numpy.pi)) if gauss else numpy.logaddexp(0.0, bA)
    if groups is not None:
        if gauss:
            raise ValueError("groups: a Gaussian visible layer has no categorical units")
        b = numpy.asarray(getattr(groups, "host", groups), dtype=numpy.int64)
        free, per_col = free.copy(), per_col.copy()
        for lo, hi in zip(b[:-1], b[1:]):           # the group's term sits at its first column, under that column's mask
            per_col[lo] = numpy.logaddexp.reduce(bA[lo:hi])
            per_col[lo + 1:hi] = 0.0
            free[:, lo + 1:hi] = False
    log_ZA = n_hidden * numpy.log(2.0) + (free * per_col[None, :]).sum(axis=1)
    top = logw.max(axis=1)
    w = numpy.exp(logw - top[:, None])
    mean = w.mean(axis=1)
    return log_ZA + top + numpy.log(mean), w.std(axis=1) / (mean * numpy.sqrt(logw.shape[1]))


class RBM(object):
    """Restricted Boltzmann Machine (RBM) -- Bernoulli visible and hidden units."""

    gauss = False

    def __init__(self, input=None, n_visible=784, n_hidden=500, W=None, hbias=None,
                 vbias=None, numpy_rng=None, theano_rng=None, engine=None, visible_groups=None):
        """Same arguments as reference rbm.py:49-59.  ``W`` / ``hbias`` / ``vbias`` may be
        ``SharedArray`` objects shared with another network (a DBN's HiddenLayer),
        ndarrays, or None (initialised as rbm.py:100-131).  ``theano_rng`` is a
        ``mdbn_amd.RandomStreams``.

        ``visible_groups``: categorical visible units (Salakhutdinov, Mnih & Hinton 2007) -- an int K: all visibles in
        groups of K (``n_visible % K == 0``); or ascending column boundaries ``[g_0, ..., g_G]``: group g is columns
        g_g .. g_{g+1} - 1 (2 .. 64 columns each), the columns outside [g_0, g_G) stay Bernoulli units.  A data row holds
        exactly one 1 in every group (``utils.one_hot_groups``).  p(v | h) is a softmax inside a group; the free energy,
        ``propup`` and the CD statistics are those of the Bernoulli layer.  None: no groups, nothing changes."""
        self.engine = engine if engine is not None else get_engine()
        self.n_visible = n_visible
        self.n_hidden = n_hidden

        if numpy_rng is None:
            numpy_rng = numpy.random.RandomState(1234)             # rbm.py:87-89
        if theano_rng is None:
            theano_rng = RandomStreams(numpy_rng.randint(2 ** 30))  # rbm.py:91-92

        if W is None:
            bound = 4 * numpy.sqrt(6. / (n_hidden + n_visible))     # rbm.py:100-107
            initial_W = numpy.asarray(numpy_rng.uniform(low=-bound, high=bound,
                                                        size=(n_visible, n_hidden)),
                                      dtype=numpy.float32)
            W = shared(initial_W, name='W', engine=self.engine, ld=weight_ld(self.engine, n_visible, n_hidden))
        if hbias is None:
            hbias = shared(numpy.zeros(n_hidden, dtype=numpy.float32), name='hbias', engine=self.engine)
        if vbias is None:
            vbias = shared(numpy.zeros(n_visible, dtype=numpy.float32), name='vbias', engine=self.engine)

        self.input = input                     # None: the data rows themselves
        self.W = shared(W, name='W', engine=self.engine)
        self.hbias = shared(hbias, name='hbias', engine=self.engine)
        self.vbias = shared(vbias, name='vbias', engine=self.engine)
        if self.W.shape != (n_visible, n_hidden):
            raise ValueError("W has shape %r, expected %r" % (self.W.shape, (n_visible, n_hidden)))
        self.theano_rng = theano_rng
        self.stream_id = theano_rng.new_stream()
        self.params = [self.W, self.hbias, self.vbias]

        self.momentum = 0.0                    # rbm.py:151; supplied per step-function call

        z = numpy.zeros
        self.W_speed = shared(z((n_visible, n_hidden), numpy.float32), name='W_speed', engine=self.engine,
                              ld=self.W.tensor.stride(0))        # (same layout as W: the update walks both)
        self.hbias_speed = shared(z(n_hidden, numpy.float32), name='hbias_speed', engine=self.engine)
        self.vbias_speed = shared(z(n_visible, numpy.float32), name='vbias_speed', engine=self.engine)
        self.params_speed = [self.W_speed, self.hbias_speed, self.vbias_speed]

        # rbm.py:415 captures W.get_value() when the update graph is built: a frozen
        # snapshot.  strict_reference=False uses the live W instead.
        self.strict_reference = True
        self._W0_snapshot = None               # the frozen weight-cost constant of the last get_cost_updates
        self._resume_W0 = None                 # ... restored from a checkpoint, consumed by the next one
        self.v_offset = self.h_offset = None   # running means of the centred gradient (SharedArray [V] / [H]; optimiser state,
                                               # like the speeds: None until the first centred step)
        self.h_activity = None                 # running mean activation of the hidden units under a sparsity target
                                               # (SharedArray [H]; optimiser state: None until the first sparse step)
        self.W_gen = self.W_gen_speed = None   # generative (top-down) weights of a layer untied by up-down fine-tuning
                                               # (SharedArray [V, H] on W's leading dimension; None: tied, W serves both ways)
        self.log_sigma = self.log_sigma_speed = None   # learned per-column variance of a Gaussian layer (GRBM.set_sigma):
                                               # SharedArray [V] each, a parameter and its speed; None: unit variance
        self.bit_i_idx = 0                     # rbm.py:425
        self._rng_step = 0
        self._n_updates = 0
        self.visible_groups = None             # GroupTable of a layer with softmax visible units (device + host copy), or None
        self.set_visible_groups(visible_groups)

    def set_visible_groups(self, visible_groups):
        """Declare (or with None remove) the softmax groups of the visible layer: see ``__init__``.  Step functions built
        before keep the table they were built with."""
        if visible_groups is None:
            self.visible_groups = None
            return
        if self.gauss:
            raise ValueError("visible_groups: a Gaussian visible layer (GRBM) has no categorical units")
        self.visible_groups = GroupTable(self.engine, group_boundaries(visible_groups, self.n_visible))

    def _no_groups(self, what):
        if self.visible_groups is not None:
            raise NotImplementedError("%s on a layer with categorical visible units (visible_groups) is not built yet: it "
                                      "would sample the groups as independent sigmoid units" % what)

    def _check_one_hot(self, data, spans=None):
        """ValueError unless every group (``spans``: only these) of every row of ``data`` (host copy) holds exactly one 1 and
        zeros."""
        if isinstance(data, torch.Tensor):
            data = data.detach().cpu().numpy()
        x = numpy.asarray(getattr(data, "get_value", lambda: data)())
        for lo, hi in (self.visible_groups.spans() if spans is None else spans):
            g = x[:, lo:hi]
            bad = numpy.nonzero(~(((g == 0) | (g == 1)).all(axis=1) & (g.sum(axis=1) == 1)))[0]
            if bad.size:
                raise ValueError("row %d of the data does not hold exactly one 1 in the group of columns %d .. %d"
                                 % (int(bad[0]), lo, hi - 1))

    def _no_sigma(self, what):
        if self.log_sigma is not None:
            raise NotImplementedError("%s on a layer with log_sigma (learned per-column variance) is not built yet: it would "
                                      "run the unit-variance model on raw rows" % what)

    def _units(self, v):
        """``v`` (raw rows) as the unit-variance model sees them: v exp(-log_sigma), a device matrix; without ``log_sigma``
        ``v`` itself."""
        if self.log_sigma is None:
            return v
        return self.engine.sigma_scale_rows(as_tensor(v, self.engine), None, self.log_sigma.tensor, -1.0)

    def _raw(self, u):
        """The way back: ``u`` (a device matrix in units, or None) times exp(log_sigma); without ``log_sigma`` ``u`` itself."""
        if self.log_sigma is None or u is None:
            return u
        return self.engine.sigma_scale_rows(u, None, self.log_sigma.tensor, 1.0)

    @property
    def down_W(self):
        """The matrix a directed top-down pass through this layer uses: ``W_gen`` once ``updown`` has untied the layer, else W.
        The RBM's own methods (propdown, Gibbs chains, free energy, AIS) keep to W: they describe the recognition RBM."""
        return self.W.tensor if self.W_gen is None else self.W_gen.tensor

    @property
    def Wt(self):
        """rbm.py:139: a transposed view; the kernels read W transposed in place."""
        return self.W.tensor.t()

    # ------------------------------------------------------------------ helpers
    def _take_step(self):
        s = self._rng_step
        self._rng_step += 1
        return s

    def _rng(self, draw=0):
        return RngAddr(self.theano_rng.seed, self.stream_id, self._take_step(), draw, 0)

    def _wrap(self, t):
        return None if t is None else SharedArray(None, engine=self.engine, _tensor=t)

    # ------------------------------------------------------------------ energies
    def _zero_filled(self, v, what):
        """``v`` with 0 where it holds NaN (an absent unit), a device matrix (``engine.absent_split``)."""
        self._no_groups(what)
        self._no_sigma(what)
        return self.engine.absent_split(as_tensor(v, self.engine), want_count=False)[0]

    def free_energy(self, v_sample, missing=False):
        ''' Function to compute the free energy (rbm.py:166-171); with ``log_sigma`` s: of the raw rows,
        F(x) = F_u(x exp(-s)) + sum(s).  ``missing=True``: NaN marks a unit the row did not observe, and the free energy is
        F_O over the units it did (``engine.free_energy_absent``; likelihoods of such rows need a partition function per
        pattern and are not offered) '''
        if missing:
            self._no_groups("free_energy(missing=True)")
            self._no_sigma("free_energy(missing=True)")
            return self._wrap(self.engine.free_energy_absent(as_tensor(v_sample, self.engine), self.W.tensor, self.hbias.tensor,
                                                             self.vbias.tensor, self.gauss))
        if self.log_sigma is not None:
            F = self.engine.free_energy(self._units(v_sample), self.W.tensor, self.hbias.tensor, self.vbias.tensor, self.gauss)
            return self._wrap(F + self.log_sigma.tensor.sum())
        return self._wrap(self.engine.free_energy(as_tensor(v_sample, self.engine), self.W.tensor,
                                                  self.hbias.tensor, self.vbias.tensor, self.gauss))

    def free_energy_gap(self, train, test, missing=False):
        """mean F(test) - mean F(train) (rbm.py:173-180); returns a Python float.  ``missing=True``: over the observed units
        of every row (``free_energy``)."""
        kw = {"missing": True} if missing else {}
        ft, fs = self.free_energy(train, **kw).tensor, self.free_energy(test, **kw).tensor
        return float(fs.mean() - ft.mean())

    def free_energies(self, train, test, missing=False):
        """rbm.py:182-185, evaluated: two host vectors (as dbn.py:498-501 consumes them).  ``missing``: as ``free_energy``."""
        kw = {"missing": True} if missing else {}
        return self.free_energy(train, **kw).get_value(), self.free_energy(test, **kw).get_value()

    # ------------------------------------------------------------------ likelihood (annealed importance sampling)
    def base_rate_vbias(self, data):
        """Visible bias of the base-rate model of ``data`` (host matrix): Bernoulli: the logit of the smoothed column
        means (N mean + 0.05) / (N + 0.1) -- a constant column stays finite --; Gaussian: the column means.  On a softmax group
        of K columns (``visible_groups``) the log of the smoothed category shares, b_A,c = log((n_c + 0.05) / (N + 0.05 K)) with
        n_c the column's count: the group's logsumexp is 0 and a category never seen stays finite."""
        if isinstance(data, torch.Tensor):
            data = data.detach().cpu().numpy()
        x = numpy.asarray(getattr(data, "get_value", lambda: data)(), dtype=numpy.float64)
        if self.log_sigma is not None:          # the base-rate model of the unit-variance layer: the data in units
            x = x * numpy.exp(-numpy.asarray(self.log_sigma.get_value(), dtype=numpy.float64))[None, :]
        mean = x.mean(axis=0)
        if self.gauss:
            return mean.astype(numpy.float32)
        p = (x.shape[0] * mean + 0.05) / (x.shape[0] + 0.1)
        bA = numpy.log(p) - numpy.log1p(-p)
        if self.visible_groups is not None:
            n = x.sum(axis=0)
            for lo, hi in self.visible_groups.spans():
                bA[lo:hi] = numpy.log((n[lo:hi] + 0.05) / (x.shape[0] + 0.05 * (hi - lo)))
        return bA.astype(numpy.float32)

    def _ais_schedule(self, betas, n_betas, base_vbias, data):
        """``(betas float32, K, base_vbias float32)`` of an AIS run from the arguments of ``log_partition``: ``betas`` None:
        ``linspace(0, 1, n_betas + 1)`` (n_betas None: 1000); ``base_vbias`` None: from ``data``, with neither the layer's own
        visible bias."""
        if betas is None:
            betas = numpy.linspace(0.0, 1.0, int(1000 if n_betas is None else n_betas) + 1)
        betas = numpy.asarray(betas, dtype=numpy.float32)
        if base_vbias is None:
            base_vbias = self.base_rate_vbias(data) if data is not None else self.vbias.get_value()
        return betas, betas.size - 1, numpy.asarray(base_vbias, dtype=numpy.float32)

    def log_partition(self, n_chains=512, betas=None, n_betas=None, base_vbias=None, data=None, path=0, method="ais",
                      n_ladders=64, n_sweeps=1200, burn_in=300, estimator="mid"):
        """``(log_Z, std_err)`` of the layer by annealed importance sampling (Salakhutdinov & Murray 2008) on the device:
        ``n_chains`` chains through the inverse temperatures ``betas`` (None: ``linspace(0, 1, n_betas + 1)``, n_betas None:
        1000) from the base-rate model ``base_vbias`` (None: taken from ``data`` by ``base_rate_vbias``; with neither, the
        layer's own visible bias).  The logsumexp and the delta-method standard error std(w) / (mean(w) sqrt(M)) are float64
        numpy on the host.  Consumes 2K - 1 RNG steps.

        ``method="tempering"``: the estimate of ``TemperedChains.log_partition`` instead -- ``n_ladders`` parallel-tempering
        ladders of ``n_betas`` temperatures (None: 16; or ``betas``, from 0 to 1) from the same base-rate model run
        ``n_sweeps`` sweeps; the works of the swap attempts after ``burn_in`` bridge neighbouring temperatures
        (``estimator``: "mid" or "bar"); the error is the delete-one-ladder jackknife.  Consumes 3 n_sweeps RNG steps.  Where
        chains mix badly AIS under-estimates log Z without its error showing it; ``check_log_partition`` runs both.

        A layer with ``visible_groups``: the same run with a group's visible draw one category of its softmax
        (``HipEngine.ais_grouped``) and the base model's log Z_A with a logsumexp per group; ``method="tempering"`` runs the
        grouped ladder (``HipEngine.temper_grouped``) from the same base model."""
        if self.visible_groups is not None and not hasattr(self.engine, "temper_grouped" if method == "tempering" else "ais_grouped"):
            self._no_groups("log_partition(method=\"tempering\") on this engine" if method == "tempering" else "log_partition on this engine")
        if method == "tempering":
            self._no_sigma("log_partition(method=\"tempering\")")       # (AIS needs no change: log Z is the unit model's)
            r = self.tempered_chains(n_ladders, betas=betas, n_betas=16 if n_betas is None else n_betas, base_vbias=base_vbias,
                                     data=data).log_partition(n_sweeps, burn_in, path=path, method=estimator)
            return r.log_z, r.stderr
        if method != "ais":
            raise ValueError("method must be 'ais' or 'tempering', got %r" % (method,))
        betas, K, base_vbias = self._ais_schedule(betas, n_betas, base_vbias, data)
        step = self._rng_step
        rng = RngAddr(self.theano_rng.seed, self.stream_id, step, 0, 0)
        if self.visible_groups is not None:
            logw = self.engine.ais_grouped(self.W.tensor, self.hbias.tensor, self.vbias.tensor, base_vbias, betas, int(n_chains),
                                           rng, self.visible_groups, path=path)
        else:
            logw = self.engine.ais(self.W.tensor, self.hbias.tensor, self.vbias.tensor, base_vbias, self.gauss, betas,
                                   int(n_chains), rng, path=path)
        self._rng_step = step + 2 * K - 1
        return ais_estimate(logw, base_vbias, self.n_hidden, self.gauss, self.visible_groups)

    def check_log_partition(self, data=None, base_vbias=None, path=0, n_chains=512, n_betas=None, n_ladders=64,
                            n_ladder_betas=16, n_sweeps=1200, burn_in=300, estimator="mid"):
        """AIS and the tempering estimate of log Z from the SAME base-rate model (``base_vbias``; None: from ``data``; with
        neither, the layer's own visible bias), side by side: a dict with ``ais`` / ``ais_stderr``, ``tempering`` /
        ``tempering_stderr``, ``bracket`` = (log_z_fwd, log_z_rev) of the tempering run (biased low / high), ``z`` =
        |ais - tempering| / sqrt(se_ais^2 + se_tempering^2) and ``detail`` (the ``LogZ`` of the tempering run).  Asserts
        nothing: a large ``z``, or an AIS value below the bracket, says the AIS chains missed a mode (INTEGRATION)."""
        self._no_sigma("check_log_partition")
        if self.visible_groups is not None and not (hasattr(self.engine, "ais_grouped") and hasattr(self.engine, "temper_grouped")):
            self._no_groups("check_log_partition on this engine")
        if base_vbias is None:
            base_vbias = self.base_rate_vbias(data) if data is not None else self.vbias.get_value()
        ais, se_a = self.log_partition(n_chains=n_chains, n_betas=n_betas, base_vbias=base_vbias, path=path)
        r = self.tempered_chains(n_ladders, n_betas=n_ladder_betas, base_vbias=base_vbias).log_partition(
            n_sweeps, burn_in, path=path, method=estimator)
        scale = float(numpy.sqrt(se_a ** 2 + r.stderr ** 2))
        return dict(ais=ais, ais_stderr=se_a, tempering=r.log_z, tempering_stderr=r.stderr, bracket=(r.log_z_fwd, r.log_z_rev),
                    z=abs(ais - r.log_z) / scale if scale > 0 else float("inf") if ais != r.log_z else 0.0, detail=r)

    def log_likelihood(self, data, **ais):
        """``(mean log p(data), std_err)``: mean(-free_energy(data)) - log_Z with ``log_partition(**ais)``'s estimate (the
        standard error is that of log_Z; ``data`` also gives the base rate unless ``base_vbias`` / ``data`` is passed;
        ``method="tempering"`` and its keywords reach ``log_partition`` like any other).  With ``log_sigma`` s the free energy
        carries the sum(s) term of the change of variables and log_Z is the unit model's: nats per raw row.  With
        ``visible_groups`` every group of every row of ``data`` must hold exactly one 1 (checked on the host: ValueError)."""
        if self.visible_groups is not None:
            tempering = ais.get("method", "ais") == "tempering"
            if not hasattr(self.engine, "temper_grouped" if tempering else "ais_grouped"):
                self._no_groups("log_likelihood(method=\"tempering\") on this engine" if tempering else "log_likelihood on this engine")
            self._check_one_hot(data)
        if ais.get("method", "ais") == "tempering":
            self._no_sigma("log_likelihood(method=\"tempering\")")
        if "base_vbias" not in ais and "data" not in ais:
            ais = dict(ais, data=data)
        log_Z, err = self.log_partition(**ais)
        neg_F = -numpy.asarray(self.free_energy(data).get_value(), dtype=numpy.float64)
        return float(neg_F.mean() - log_Z), err

    # ------------------------------------------------------------------ propagation
    def propup(self, vis, missing=False):
        '''[pre_sigmoid_activation, sigmoid(pre)] (rbm.py:187-199); ``missing=True``: NaN entries go up as 0 (absent units)'''
        if missing:
            vis = self._zero_filled(vis, "propup(missing=True)")
        pre, mean, _ = self.engine.propup(as_tensor(self._units(vis), self.engine), self.W.tensor, self.hbias.tensor,
                                          want_sample=False)
        return [self._wrap(pre), self._wrap(mean)]

    def hidden_activity(self, data, chunk_rows=4096):
        """Mean of p(h = 1 | v) over all rows of ``data`` for every hidden unit: float32 [n_hidden], computed on the device
        -- what a sparsity target (``get_cost_updates``) steers.  ``data`` goes up ``chunk_rows`` rows at a time; each chunk's
        column means are folded into one accumulator at rate n_chunk / n_seen (``engine.sparsity_activity``), which is the
        exact running mean.  No random number is consumed."""
        eng = self.engine
        x = as_tensor(data, eng)
        if x.shape[0] < 1:
            raise ValueError("hidden_activity needs at least one row")
        q = eng.alloc_vector(self.n_hidden)
        seen, step = 0, max(1, int(chunk_rows))
        for lo in range(0, x.shape[0], step):
            rows = self._units(x[lo:lo + step])
            mean = eng.propup(rows, self.W.tensor, self.hbias.tensor, want_pre=False, want_sample=False)[1]
            seen += rows.shape[0]
            eng.sparsity_activity(ActivityRows(mean), rows.shape[0], q, None, float(rows.shape[0]) / float(seen))
        return numpy.asarray(eng.to_numpy(q), dtype=numpy.float32)

    def sample_h_given_v(self, v0_sample, missing=False):
        ''' [pre_sigmoid_h1, h1_mean, h1_sample] (rbm.py:201-213); ``missing=True``: NaN entries go up as 0 (absent units) '''
        if missing:
            v0_sample = self._zero_filled(v0_sample, "sample_h_given_v(missing=True)")
        pre, mean, sample = self.engine.propup(as_tensor(self._units(v0_sample), self.engine), self.W.tensor,
                                               self.hbias.tensor, rng=self._rng())
        return [self._wrap(pre), self._wrap(mean), self._wrap(sample)]

    def _grouped_down(self, hid, rng, W=None):
        """(pre, mean, sample) of p(v | h) on a layer with softmax groups: the linear pre-activations h W^T + vbias, then
        ``engine.group_softmax`` (sample None without ``rng``)."""
        pre = self.engine.propdown(as_tensor(hid, self.engine), self.W.tensor if W is None else W, self.vbias.tensor,
                                   gauss=True, add_noise=False, rng=None)[1]
        mean, sample = self.engine.group_softmax(pre, self.visible_groups, rng)
        return pre, mean, sample

    def propdown(self, hid):
        '''[pre_sigmoid_activation, sigmoid(pre)] (rbm.py:215-227); with ``visible_groups``: [pre, grouped means] -- softmax
        inside every group, sigmoid on the other columns; with ``log_sigma``: both entries times sigma, raw units as every
        visible-side result of such a layer (the first is then the conditional mean sigma (vbias + W h))'''
        if self.visible_groups is not None:
            self._take_step()                                  # (one step per call, as without groups)
            pre, mean, _ = self._grouped_down(hid, None)
            return [self._wrap(pre), self._wrap(mean)]
        pre, mean, _ = self.engine.propdown(as_tensor(hid, self.engine), self.W.tensor, self.vbias.tensor,
                                            gauss=False, rng=self._rng())
        return [self._wrap(self._raw(pre)), self._wrap(self._raw(mean))]

    def sample_v_given_h(self, h0_sample):
        ''' [pre_sigmoid_v1, v1_mean, v1_sample] (rbm.py:229-240); with ``visible_groups`` the sample holds exactly one 1 in
        every group (one uniform per group, at its first column) '''
        if self.visible_groups is not None:
            pre, mean, sample = self._grouped_down(h0_sample, self._rng())
            return [self._wrap(pre), self._wrap(mean), self._wrap(sample)]
        pre, mean, sample = self.engine.propdown(as_tensor(h0_sample, self.engine), self.W.tensor,
                                                 self.vbias.tensor, gauss=False, rng=self._rng())
        return [self._wrap(pre), self._wrap(mean), self._wrap(sample)]

    def group_posterior(self, v, group):
        """Exact p(category | all other visibles) of softmax group ``group`` for every row of ``v``: float64 [N, K],
        softmax_c(-F(v with the group set to category c)) -- K free energies on the device, the finish in float64 on the
        host.  What ``v`` holds inside the group is ignored.  With a label block in the joint layer this is the class
        prediction of a classification RBM (Larochelle & Bengio 2008).  No random number is consumed."""
        if self.visible_groups is None:
            raise ValueError("group_posterior needs a layer with visible_groups")
        lo, hi = self.visible_groups.spans()[range(self.visible_groups.n_groups)[int(group)]]
        x = self.engine.as_matrix(as_tensor(v, self.engine)).clone()
        neg_F = numpy.empty((x.shape[0], hi - lo), dtype=numpy.float64)
        for c in range(hi - lo):
            x[:, lo:hi] = 0.0
            x[:, lo + c] = 1.0
            neg_F[:, c] = -self.free_energy(x).tensor.detach().cpu().to(torch.float64).numpy()
        neg_F -= neg_F.max(axis=1, keepdims=True)
        p = numpy.exp(neg_F)
        return p / p.sum(axis=1, keepdims=True)

    def _label_span(self, group, what):
        """(first column, K) of softmax group ``group`` (negative: from the end), the label block of a classification RBM."""
        if self.visible_groups is None:
            raise ValueError("%s needs a layer with visible_groups: the label block is one of its groups" % what)
        n = self.visible_groups.n_groups
        if not -n <= int(group) < n:
            raise ValueError("%s: label group %r of a layer with %d groups" % (what, group, n))
        lo, hi = self.visible_groups.spans()[int(group) % n]
        return lo, hi - lo

    def _class_call(self, v, group, what, want_logp):
        lo, K = self._label_span(group, what)
        if not hasattr(self.engine, "class_posterior"):
            raise NotImplementedError("%s needs an engine with the classification calls (class_posterior); %s has none"
                                      % (what, type(self.engine).__name__))
        if want_logp:
            self._check_one_hot(v, spans=[(lo, lo + K)])
        return self.engine.class_posterior(as_tensor(v, self.engine), self.W.tensor, self.hbias.tensor, self.vbias.tensor, lo, K,
                                           want_logp=want_logp)

    def label_posterior(self, v, group=-1):
        """Exact p(category | all other visibles) of softmax group ``group`` (the label block of a classification RBM;
        default: the last group) for every row of ``v``: float64 [N, K].  The numbers of ``group_posterior`` from one device
        call -- one propup of the rows with the block set to zero, shared by all categories, and one kernel for the K scores
        and their softmax -- instead of K free-energy passes.  What ``v`` holds inside the group is ignored; no random number
        is consumed."""
        post, _ = self._class_call(v, group, "label_posterior", False)
        return post.detach().cpu().to(torch.float64).numpy()

    def predict(self, v, group=-1):
        """The most probable category of group ``group`` for every row of ``v`` (``label_posterior``): int64 [N]."""
        return self.label_posterior(v, group).argmax(axis=1)

    def label_log_likelihood(self, v, group=-1):
        """log p(y* | all other visibles) for every row of ``v``, y* the category its block of group ``group`` holds (exactly
        one 1, checked on the host): float64 [N].  No random number is consumed."""
        _, logp = self._class_call(v, group, "label_log_likelihood", True)
        return logp.detach().cpu().to(torch.float64).numpy()

    def gibbs_hvh(self, h0_sample):
        ''' One Gibbs step starting from the hidden state (rbm.py:242-248) '''
        pre_sigmoid_v1, v1_mean, v1_sample = self.sample_v_given_h(h0_sample)
        pre_sigmoid_h1, h1_mean, h1_sample = self.sample_h_given_v(v1_sample)
        return [pre_sigmoid_v1, v1_mean, v1_sample,
                pre_sigmoid_h1, h1_mean, h1_sample]

    def gibbs_vhv(self, v0_sample):
        ''' One Gibbs step starting from the visible state (rbm.py:250-256) '''
        pre_sigmoid_h1, h1_mean, h1_sample = self.sample_h_given_v(v0_sample)
        pre_sigmoid_v1, v1_mean, v1_sample = self.sample_v_given_h(h1_sample)
        return [pre_sigmoid_h1, h1_mean, h1_sample,
                pre_sigmoid_v1, v1_mean, v1_sample]

    def gibbs_vhv_chain(self, v0_sample, n_steps):
        """``n_steps`` of ``gibbs_vhv`` as ONE device call (the ``theano.scan`` over gibbs_vhv of rbm.py:822-838):
        the six outputs of the LAST step, identical bit for bit to calling ``gibbs_vhv`` ``n_steps`` times,
        without the per-step allocations and launches' host overhead.  Consumes 2 * n_steps RNG steps."""
        step = self._rng_step
        self._rng_step += 2 * int(n_steps)
        if not hasattr(self.engine, "gibbs_chain") or self.visible_groups is not None:
            # checker engine, or a layer with softmax groups (no chain call of its own): compose the eager steps
            self._rng_step = step
            out, v = None, v0_sample
            for _ in range(int(n_steps)):
                out = self.gibbs_vhv(v)
                v = out[5]
            return out
        out = self.engine.gibbs_chain(as_tensor(self._units(v0_sample), self.engine), self.W.tensor, self.hbias.tensor,
                                      self.vbias.tensor, self.gauss, int(n_steps),
                                      RngAddr(self.theano_rng.seed, self.stream_id, step, 0, 0),
                                      add_noise=self.gauss and not getattr(self, "error_free", True))
        if self.log_sigma is not None:          # the visible half back in raw units (pre_v and v_mean are one matrix)
            out = list(out)
            back = {}
            for i in (3, 4, 5):
                if out[i] is not None:
                    key = out[i].data_ptr()
                    if key not in back:
                        back[key] = self._raw(out[i])
                    out[i] = back[key]
        return [self._wrap(t) for t in out]

    # ------------------------------------------------------------------ clamped Gibbs sampling / imputation
    def _clamp_mask(self, observed_mask, B):
        m = numpy.asarray(getattr(observed_mask, "get_value", lambda: observed_mask)())
        if m.ndim == 1:
            m = m[None, :]
        if m.ndim != 2 or m.shape[1] != self.n_visible or m.shape[0] not in (1, B):
            raise ValueError("observed_mask must be [%d] or [1 | %d, %d], got %r" % (self.n_visible, B, self.n_visible, m.shape))
        return (m != 0).astype(numpy.float32)

    def _check_group_mask(self, mask):
        """ValueError unless every row of the 0 / 1 ``mask`` is constant over every group (a group is held or free as a whole)."""
        for lo, hi in self.visible_groups.spans():
            bad = numpy.nonzero((mask[:, lo:hi] != mask[:, lo:lo + 1]).any(axis=1))[0]
            if bad.size:
                raise ValueError("row %d of observed_mask splits the group of columns %d .. %d: a group is observed or missing "
                                 "as a whole" % (int(bad[0]), lo, hi - 1))

    def gibbs_vhv_clamped(self, v, observed_mask, n_steps, burn_in=0, trace=False, path=0, sampler=False):
        """``n_steps`` of ``gibbs_vhv`` with the visibles where ``observed_mask`` is nonzero held at their values in ``v``
        (the other entries of ``v`` start the chain), as ONE device call (mdbn_gibbs_clamped).  ``observed_mask``: [B, V]
        per element, or [V] / [1, V] for the whole batch.  Returns the six outputs of the LAST step as
        ``gibbs_vhv_chain`` does -- v_mean and the visible sample after the clamp; the two pre-activations are None on
        the device -- followed by ``v_avg`` and ``h_avg``, the means of v_mean / h_mean over the steps
        ``burn_in .. n_steps - 1`` (the estimate of E[v | v_obs], E[h | v_obs]), and with ``trace`` by the hidden samples
        [n_steps, B, H] and the clamped states [n_steps, B, V] of every step.  Consumes 2 * n_steps RNG steps.

        A Bernoulli layer's chain is a Gibbs sampler, so its averages estimate the posterior means.  The GRBM chain of the
        reference (``gibbs_vhv``: the hidden MEAN goes down, noise only if not ``error_free``) is a mean-field iteration, and
        its averages are not posterior means; ``sampler=True`` runs the Gibbs sampler of the same model instead (the hidden
        SAMPLE goes down, the visible draw always carries its N(0, 1) noise).  It changes nothing for a Bernoulli layer.

        A layer with ``visible_groups`` (on an engine with ``gibbs_clamped_grouped``; refused elsewhere): a free group's draw is
        one category of its softmax and its v_mean the softmax (mdbn_gibbs_clamped_grouped); a group is held or free as a whole,
        so a mask that is not constant over a group is a ValueError, raised before anything is drawn."""
        grouped = self.visible_groups is not None
        if grouped and not hasattr(self.engine, "gibbs_clamped_grouped"):
            self._no_groups("gibbs_vhv_clamped on this engine")
        self._no_sigma("gibbs_vhv_clamped")
        sampler = bool(sampler and self.gauss)
        n_steps, burn_in = int(n_steps), int(burn_in)
        if n_steps < 1 or not 0 <= burn_in < n_steps:
            raise ValueError("need n_steps >= 1 and 0 <= burn_in < n_steps, got %d, %d" % (n_steps, burn_in))
        x = as_tensor(v, self.engine)
        mask = self._clamp_mask(observed_mask, x.shape[0])
        step = self._rng_step
        if grouped:
            self._check_group_mask(mask)
            self._rng_step = step + 2 * n_steps
            res = self.engine.gibbs_clamped_grouped(x, x, mask, self.W.tensor, self.hbias.tensor, self.vbias.tensor, n_steps,
                                                    RngAddr(self.theano_rng.seed, self.stream_id, step, 0, 0), self.visible_groups,
                                                    burn_in=burn_in, path=path, trace=trace)
            state, h_mean, h_sample, v_mean, v_avg, h_avg = res[:6]
            return [self._wrap(t) for t in (None, h_mean, h_sample, None, v_mean, state, v_avg, h_avg) + tuple(res[6:])]
        if not hasattr(self.engine, "gibbs_clamped"):        # checker engine: compose the eager steps
            held = as_tensor(numpy.broadcast_to(mask, tuple(x.shape)).copy(), self.engine) != 0
            obs, state = x, x
            v_acc, h_acc, out, th, tv = 0.0, 0.0, None, [], []
            for t in range(n_steps):
                pre_h, h_mean, h_sample = self.sample_h_given_v(state)
                if sampler:
                    mean, _, new = self.engine.propdown(h_sample.tensor, self.W.tensor, self.vbias.tensor, gauss=True,
                                                        add_noise=True, rng=self._rng())
                    pre_v, v_mean, v_new = self._wrap(mean), self._wrap(mean), self._wrap(new)
                else:
                    pre_v, v_mean, v_new = self.sample_v_given_h(h_mean if self.gauss else h_sample)
                v_mean, state = torch.where(held, obs, v_mean.tensor), torch.where(held, obs, v_new.tensor)
                if t >= burn_in:
                    v_acc, h_acc = v_acc + v_mean, h_acc + h_mean.tensor
                th.append(h_sample.tensor)
                tv.append(state)
                out = [pre_h, h_mean, h_sample, pre_v, self._wrap(v_mean), self._wrap(state)]
            out += [self._wrap(v_acc / (n_steps - burn_in)), self._wrap(h_acc / (n_steps - burn_in))]
            assert self._rng_step == step + 2 * n_steps
            return out + ([self._wrap(torch.stack(th)), self._wrap(torch.stack(tv))] if trace else [])
        self._rng_step = step + 2 * n_steps
        res = self.engine.gibbs_clamped(x, x, mask, self.W.tensor, self.hbias.tensor, self.vbias.tensor, self.gauss, n_steps,
                                        RngAddr(self.theano_rng.seed, self.stream_id, step, 0, 0), burn_in=burn_in,
                                        add_noise=self.gauss and not sampler and not getattr(self, "error_free", True), path=path, trace=trace,
                                        sampler=sampler)
        state, h_mean, h_sample, v_mean, v_avg, h_avg = res[:6]
        return [self._wrap(t) for t in (None, h_mean, h_sample, None, v_mean, state, v_avg, h_avg) + tuple(res[6:])]

    def impute(self, v, observed_mask, n_steps=1000, burn_in=200, n_chains=1, path=0):
        """Posterior means of the unobserved visibles and of the hidden layer given the observed visibles:
        ``(v_hat [N, V], h_hat [N, H])`` as host arrays.  The unobserved entries of ``v`` (anything: they are ignored)
        start at the model's base (``sigmoid(vbias)``; GRBM: ``vbias``), every row runs ``n_chains`` independent clamped
        chains (consecutive Philox rows) of ``n_steps`` Gibbs steps (``sampler=True``: a GRBM runs the Gibbs sampler of its
        model, not the reference's mean-field chain), and v_mean / h_mean are averaged over the steps from
        ``burn_in`` on and over the chains.  Observed entries of ``v_hat`` are the observed values.  Consumes
        2 * n_steps RNG steps.

        A layer with ``visible_groups`` (on an engine with ``gibbs_clamped_grouped``; refused elsewhere): a free group starts
        at the softmax of its ``vbias``, and its ``v_hat`` sums to 1; ``observed_mask`` must be constant over every group."""
        if self.visible_groups is not None and not hasattr(self.engine, "gibbs_clamped_grouped"):
            self._no_groups("impute on this engine")
        self._no_sigma("impute")
        x = numpy.asarray(getattr(v, "get_value", lambda: v)(), dtype=numpy.float32)
        N, n_chains = x.shape[0], int(n_chains)
        mask = self._clamp_mask(observed_mask, N)
        b = numpy.asarray(self.vbias.get_value(), dtype=numpy.float64)
        base = b if self.gauss else 1.0 / (1.0 + numpy.exp(-b))
        if self.visible_groups is not None:
            self._check_group_mask(mask)
            for lo, hi in self.visible_groups.spans():
                e = numpy.exp(b[lo:hi] - b[lo:hi].max())
                base[lo:hi] = e / e.sum()
        base = base.astype(numpy.float32)
        held = numpy.broadcast_to(mask != 0, x.shape)
        start = numpy.where(held, x, base[None, :]).astype(numpy.float32)
        if n_chains > 1:
            start = numpy.repeat(start, n_chains, axis=0)
            if mask.shape[0] != 1:
                mask = numpy.repeat(mask, n_chains, axis=0)
        out = self.gibbs_vhv_clamped(start, mask, n_steps, burn_in=burn_in, path=path, sampler=True)
        v_hat, h_hat = (numpy.asarray(t.get_value(), dtype=numpy.float64) for t in out[6:8])
        if n_chains > 1:
            v_hat = v_hat.reshape(N, n_chains, -1).mean(axis=1)
            h_hat = h_hat.reshape(N, n_chains, -1).mean(axis=1)
        # (an observed entry is its observed value, not the float32 mean of n_steps copies of it)
        v_hat = numpy.where(held, x, v_hat)
        return v_hat.astype(numpy.float32), h_hat.astype(numpy.float32)

    # ------------------------------------------------------------------ conditional likelihood (clamped AIS)
    def conditional_log_partition(self, v, observed_mask, n_chains=64, betas=None, n_betas=None, base_vbias=None, data=None, path=0):
        """``(log_Z [N], std_err [N])``: for every row of ``v`` the log partition function of the layer with the visibles where
        ``observed_mask`` is nonzero held at their values in ``v`` -- an RBM over the row's free visibles with the hidden bias
        hbias + v_O W_O -- by annealed importance sampling on the device (mdbn_ais_cond_run), ``n_chains`` chains per row.
        ``observed_mask``: [N, V] per element, or [V] / [1, V] for every row; the free entries of ``v`` are ignored.
        ``betas`` / ``n_betas`` / ``base_vbias`` / ``data``: the schedule and the base-rate model, as ``log_partition`` (the
        base-rate model of a row is ``base_vbias`` on its free columns).  The logsumexp and the delta-method standard error of
        every row are float64 numpy on the host (``ais_estimate_rows``); a row with no free column has std_err 0.  Consumes
        2K - 1 RNG steps.

        A layer with ``visible_groups`` (on an engine with ``ais_conditional_grouped``; refused elsewhere): a free group's draw
        is one category of its softmax (mdbn_ais_cond_run_grouped) and the base model counts it as one logsumexp; a group is
        held or free as a whole, so a mask that is not constant over a group is a ValueError, raised before anything is drawn."""
        grouped = self.visible_groups is not None
        if grouped and not hasattr(self.engine, "ais_conditional_grouped"):
            self._no_groups("conditional_log_partition on this engine")
        self._no_sigma("conditional_log_partition")
        x = numpy.asarray(getattr(v, "get_value", lambda: v)(), dtype=numpy.float32)
        if x.ndim != 2 or x.shape[1] != self.n_visible or x.shape[0] < 1:
            raise ValueError("v must be [N >= 1, %d], got %r" % (self.n_visible, x.shape))
        mask = self._clamp_mask(observed_mask, x.shape[0])
        if grouped:
            self._check_group_mask(mask)
        betas, K, base_vbias = self._ais_schedule(betas, n_betas, base_vbias, data)
        step = self._rng_step
        obs = numpy.where(numpy.broadcast_to(mask != 0, x.shape), x, numpy.float32(0))
        rng = RngAddr(self.theano_rng.seed, self.stream_id, step, 0, 0)
        if grouped:
            logw = self.engine.ais_conditional_grouped(self.W.tensor, self.hbias.tensor, self.vbias.tensor, base_vbias, betas, obs,
                                                       mask, int(n_chains), rng, self.visible_groups, path=path)
        else:
            logw = self.engine.ais_conditional(self.W.tensor, self.hbias.tensor, self.vbias.tensor, base_vbias, self.gauss, betas,
                                               obs, mask, int(n_chains), rng, path=path)
        self._rng_step = step + 2 * K - 1
        return ais_estimate_rows(logw, base_vbias, mask, self.n_hidden, self.gauss, self.visible_groups)

    def conditional_log_likelihood(self, v, observed_mask, **ais):
        """``(log_p [N], std_err [N])``: log p(v_F | v_O) of every row of ``v`` -- its free block F (``observed_mask`` zero)
        given its observed block O, Srivastava & Salakhutdinov 2012 --
            -free_energy(v) - sum_{i in O} v_i b_i - log_Z_r                (Bernoulli visibles)
            -free_energy(v) + 1/2 sum_{i in O} (v_i - b_i)^2 - log_Z_r      (Gaussian visibles)
        with ``conditional_log_partition(v, observed_mask, **ais)``'s estimate of log_Z_r (the standard error is that
        estimate's); the free energy is the device's, the rest float64 on the host.  A row with no free column gets log_p = 0,
        std_err = 0.  A Bernoulli layer gives probability to 0 / 1 states only: free entries of ``v`` that are neither are
        refused (observed entries may hold any real value: they enter through v W alone).

        A layer with ``visible_groups`` (on an engine with ``ais_conditional_grouped``; refused elsewhere): ``observed_mask``
        must be constant over every group, and every FREE group of every row must hold exactly one 1 (ValueError otherwise,
        before anything is drawn; a held group may hold anything).  With one group free this is log p(category | everything
        else) of a classification RBM, the log of ``group_posterior``'s entry, with a standard error."""
        grouped = self.visible_groups is not None
        if grouped and not hasattr(self.engine, "ais_conditional_grouped"):
            self._no_groups("conditional_log_likelihood on this engine")
        self._no_sigma("conditional_log_likelihood")
        x = numpy.asarray(getattr(v, "get_value", lambda: v)(), dtype=numpy.float32)
        if x.ndim != 2 or x.shape[1] != self.n_visible or x.shape[0] < 1:
            raise ValueError("v must be [N >= 1, %d], got %r" % (self.n_visible, x.shape))
        mask = self._clamp_mask(observed_mask, x.shape[0])
        if grouped:
            self._check_group_mask(mask)
        held = numpy.broadcast_to(mask != 0, x.shape)
        if not self.gauss and not numpy.isin(x[~held], (0.0, 1.0)).all():
            raise ValueError("a Bernoulli layer scores 0 / 1 states: a free entry of v is neither")
        if grouped:
            for lo, hi in self.visible_groups.spans():
                bad = numpy.nonzero(~held[:, lo] & (x[:, lo:hi].sum(axis=1) != 1))[0]
                if bad.size:
                    raise ValueError("row %d of v does not hold exactly one 1 in the free group of columns %d .. %d"
                                     % (int(bad[0]), lo, hi - 1))
        log_Z, err = self.conditional_log_partition(x, observed_mask, **ais)
        neg_F = -numpy.asarray(self.free_energy(x).get_value(), dtype=numpy.float64)
        b = numpy.asarray(self.vbias.get_value(), dtype=numpy.float64)[None, :]
        x64 = x.astype(numpy.float64)
        held_term = 0.5 * (held * (x64 - b) ** 2).sum(axis=1) if self.gauss else -(held * x64 * b).sum(axis=1)
        log_p = neg_F + held_term - log_Z
        none_free = held.all(axis=1)
        return numpy.where(none_free, 0.0, log_p), numpy.where(none_free, 0.0, err)

    # ------------------------------------------------------------------ parallel tempering
    def tempered_chains(self, n_ladders, betas=None, n_betas=16, base_vbias=None, data=None, start_h=None):
        """``n_ladders`` parallel-tempering ladders of this layer (``mdbn_amd.temper.TemperedChains``): Gibbs chains at the
        inverse temperatures ``betas`` (None: ``linspace(0, 1, n_betas)``) of the tempered family of ``log_partition`` --
        base-rate visible bias ``base_vbias`` (None: taken from ``data`` by ``base_rate_vbias``; with neither, the layer's own
        visible bias) -- with swaps between neighbouring temperatures, so that the beta = 1 replica crosses between modes a
        plain chain never leaves.  ``start_h``: [n_ladders, H] (every temperature of a ladder starts there) or
        [n_ladders * R, H]; None: zeros.  A GRBM ladder runs the Gibbs sampler of its model (hidden sample down, unit noise),
        not the reference's mean-field chain.  Each sweep consumes 3 RNG steps.

        A layer with ``visible_groups`` (on an engine with ``temper_grouped``; refused elsewhere): a group's visible draw is one
        category of its softmax at the row's temperature, ``v_avg`` holds the softmax means, and the ladder's log Z starts
        from the grouped base model (a logsumexp per group)."""
        if self.visible_groups is not None and not hasattr(self.engine, "temper_grouped"):
            self._no_groups("tempered_chains on this engine")
        self._no_sigma("tempered_chains")
        from .temper import TemperedChains
        if betas is None:
            betas = numpy.linspace(0.0, 1.0, int(n_betas))
        if base_vbias is None:
            base_vbias = self.base_rate_vbias(data) if data is not None else self.vbias.get_value()
        return TemperedChains(self, n_ladders, betas, base_vbias, start_h=start_h)

    def sample_tempered(self, n_samples, n_sweeps=1000, burn_in=200, path=0, **ladder):
        """``n_samples`` ladders run for ``n_sweeps`` sweeps: host arrays ``(v, h, v_avg, h_avg, acceptance)`` -- the state of
        every ladder's beta = 1 replica after the last sweep, the means of its conditional expectations over the sweeps
        from ``burn_in`` on, and the accepted share of the swap attempts per neighbour pair.  ``ladder``: the arguments of
        ``tempered_chains``.  Consumes 3 * n_sweeps RNG steps."""
        chains = self.tempered_chains(int(n_samples), **ladder)
        v_avg, h_avg, acceptance = chains.run(n_sweeps, burn_in=burn_in, path=path)[:3]
        v, h = chains.samples()
        return tuple(numpy.asarray(t.get_value()) for t in (v, h, v_avg, h_avg, acceptance))

    def make_sample_fn(self, persistent_vis_chain, n_steps=500):
        """The ``sample_fn`` of rbm.py:844-853: each call runs ``n_steps`` Gibbs steps from the persistent visible
        chain, stores ``vis_samples[-1]`` back into it and returns ``(vis_mfs[-1], vis_samples[-1])`` as host arrays."""
        chain = shared(persistent_vis_chain, engine=self.engine)

        def sample_fn():
            out = self.gibbs_vhv_chain(chain, n_steps)
            chain.set_value(out[5])
            return out[4].get_value(), out[5].get_value()
        return sample_fn

    # ------------------------------------------------------------------ CD-k / PCD-k
    def _refuse_missing(self, persistent=None, symbolic_grad=False, discriminative=None, learn_sigma=None, centered=False,
                        sparse=False, tempering=None):
        """What ``missing=True`` does not compose with yet, each with its reason; raised before anything runs."""
        if self.visible_groups is not None:
            raise NotImplementedError("missing=True on a layer with visible_groups is not built: a group with some of its "
                                      "categories absent needs a softmax over the observed ones, which the grouped kernel lacks")
        if self.log_sigma is not None or learn_sigma is not None:
            raise NotImplementedError("missing=True on a layer with log_sigma / learn_sigma is not built: the variance "
                                      "statistic would have to count the rows that observed each column")
        if centered:
            raise NotImplementedError("missing=True with centered=True is not built: the offsets are batch means, which a "
                                      "column with absent entries does not have over the whole minibatch")
        if sparse:
            raise NotImplementedError("missing=True with a sparsity target is not built: the weight term of the penalty uses "
                                      "the batch means of the visible units, undefined for columns with absent entries")
        if discriminative is not None:
            raise NotImplementedError("missing=True with discriminative= is not built: the label posterior needs the grouped "
                                      "step, which has no mask")
        if symbolic_grad:
            raise NotImplementedError("missing=True with symbolic_grad=True is not supported: the absent-unit step takes its "
                                      "negative statistics from the means")
        if persistent is not None and persistent is not False:
            raise NotImplementedError("missing=True with a persistent chain is not built: a fantasy particle has no pattern "
                                      "of observed units of its own (pass persistent=None / False)")
        if tempering is not None:
            raise NotImplementedError("missing=True with tempering= is not built: the ladders are persistent chains")
        if not hasattr(self.engine, "cd_step_absent"):
            raise NotImplementedError("missing=True needs an engine with the absent-unit step (cd_step_absent); %s has none"
                                      % type(self.engine).__name__)

    def get_cost_updates(self, lr=0.1, k=1, lambda_1=0.0, lambda_2=0.0, weightcost=0.0,
                         batch_size=None, persistent=None, symbolic_grad=False, discriminative=None, label_group=-1,
                         generative=1.0, missing=False, learn_sigma=None, centered=False, offset_rate=0.01, sparsity_target=None,
                         sparsity_cost=0.0, sparsity_decay=0.9, sparsity_weights=True):
        """One step of CD-k or PCD-k (rbm.py:258-376).  Returns ``(cost, updates)``; pass
        ``updates`` to ``mdbn_amd.function`` to obtain the step function.

        ``lr`` may be a float or a ``Scalar`` (then the step function takes ``lr=``).
        ``persistent``: None for CD, a SharedArray [batch_size, n_hidden] for PCD.
        ``centered``: the centred gradient (Montavon & Mueller 2012; Melchior et al. 2016) -- visible and hidden units are
        referred to the running means ``self.v_offset`` / ``self.h_offset`` of the data and of ph_mean before the statistics
        are formed; the offsets slide by ``offset_rate`` per step (the first centred step sets them to its batch means).
        The model and its parameters (W, vbias, hbias) keep their meaning; the offsets are optimiser state.
        ``sparsity_target`` p in (0, 1) with ``sparsity_cost`` c > 0: a penalty that drives every hidden unit's mean
        activation towards p (Lee et al. 2008; Nair & Hinton 2009; Hinton's guide, section 11).  ``self.h_activity`` q is the
        running estimate of those means -- the first sparse step sets it to the means of ph_mean over its minibatch,
        afterwards q += (1 - ``sparsity_decay``) (mean - q) -- and the step adds c (p - q_j) to the hidden-bias gradient and,
        with ``sparsity_weights`` (False: the bias-only form of Lee et al.), c (p - q_j) <v_i> to the weight gradient.  q is
        optimiser state; without a target, or at cost 0, the step is the plain one.  Composes with ``centered``.
        A layer with ``visible_groups`` trains by the grouped step (``StepFunction._statistics_step``): softmax inside the
        groups, the same statistics and update; both options above compose with it, ``symbolic_grad`` does not.  Its
        monitoring cost is the cross-entropy of the reconstruction (categorical inside the groups) under PCD as well: the
        pseudo-likelihood flips one bit of a row, which takes a one-hot group out of the model's support.
        ``learn_sigma`` eta > 0 (a GRBM only): the layer learns a standard deviation per visible column (``GRBM.set_sigma``
        says what the model is) -- ``self.log_sigma`` is created as zeros on first use, so the layer starts as the plain
        GRBM, and every step moves it by its exact gradient at rate eta under the visible bias's momentum rule
        (``StepFunction._statistics_step``).  A layer whose ``log_sigma`` is set trains in units with or without it: None
        keeps sigma as it is.  The monitoring cost of such a layer is in units.  Composes with ``centered`` and the sparsity
        target, not with ``symbolic_grad``.
        ``discriminative`` w > 0 (a layer with ``visible_groups``; Larochelle & Bengio 2008): group ``label_group`` is a
        one-hot label block and the step follows the hybrid objective -- ``generative`` x (the CD statistics) + w x (the exact
        gradient of sum_rows log p(label | all other visibles), no sampling) through the unchanged update rule.
        ``generative=0`` trains the label's conditional alone and runs no chain (no ``persistent``, no sparsity target: both
        live on the chain's rows); the monitoring cost is then the mean -log p(label | rest), which the step function's
        ``discriminative_cost`` gives in either form.  A sparsity target composes with ``generative > 0``; ``centered`` and
        ``symbolic_grad`` do not compose.  None: nothing changes.
        ``missing=True``: the table may hold NaN, "this row did not observe this unit" (Salakhutdinov, Mnih & Hinton 2007: a
        missing unit is absent from that row's RBM, all rows share the weights) -- the step is CD with a per-row mask
        (``StepFunction._statistics_step``), the gradient of the MEAN log-likelihood per row over the units each row observed.
        The monitoring cost sums over observed entries only: costs of tables with different missingness do not compare.  It
        composes with nothing else yet (``_refuse_missing`` lists what is refused and why).  False: nothing changes, and a
        NaN in the table behaves as before."""
        if missing:
            self._refuse_missing(persistent=persistent, symbolic_grad=symbolic_grad, discriminative=discriminative,
                                 learn_sigma=learn_sigma, centered=centered,
                                 sparse=sparsity_target is not None and float(sparsity_cost) > 0.0)
        label_span = None
        if discriminative is not None:
            w, alpha = float(discriminative), float(generative)
            if not (w > 0.0 and numpy.isfinite(w)):
                raise ValueError("discriminative must be a positive weight, got %r" % (discriminative,))
            if not (alpha >= 0.0 and numpy.isfinite(alpha)):
                raise ValueError("generative must be a weight >= 0, got %r" % (generative,))
            label_span = self._label_span(label_group, "get_cost_updates(discriminative=)")
            if centered:
                raise NotImplementedError("discriminative= with centered=True is not built: the offsets are defined on the rows "
                                          "of the CD step, the discriminative statistics have none")
            if symbolic_grad:
                raise NotImplementedError("discriminative= with symbolic_grad=True is not supported")
            if alpha == 0.0 and persistent is not None:
                raise NotImplementedError("generative=0 runs no chain: a persistent chain would never move (pass persistent=None)")
            if alpha == 0.0 and sparsity_target is not None and float(sparsity_cost) > 0.0:
                raise NotImplementedError("generative=0 with a sparsity target: the activity estimate reads the hidden means of "
                                          "the CD step, which is not run")
            if not hasattr(self.engine, "class_stats"):
                raise NotImplementedError("discriminative= needs an engine with the classification calls (class_stats); %s has "
                                          "none" % type(self.engine).__name__)
        if learn_sigma is not None:
            if not self.gauss:
                raise ValueError("learn_sigma: a Bernoulli visible layer has no variance to learn (a GRBM has)")
            if not float(learn_sigma) > 0.0 or not numpy.isfinite(float(learn_sigma)):
                raise ValueError("learn_sigma must be a positive rate, got %r" % (learn_sigma,))
        if symbolic_grad and (learn_sigma is not None or self.log_sigma is not None):
            raise NotImplementedError("symbolic_grad=True on a layer with log_sigma (learned per-column variance) is not supported")
        if learn_sigma is not None and self.log_sigma is None:
            self.set_sigma(1.0)
        if self.visible_groups is not None and symbolic_grad:
            raise NotImplementedError("symbolic_grad=True on a layer with categorical visible units (visible_groups) is not supported")
        sparse = sparsity_target is not None and float(sparsity_cost) > 0.0
        if sparsity_target is not None and not 0.0 < float(sparsity_target) < 1.0:
            raise ValueError("sparsity_target must lie in (0, 1), got %r" % (sparsity_target,))
        if not float(sparsity_cost) >= 0.0:
            raise ValueError("sparsity_cost must not be negative, got %r" % (sparsity_cost,))
        if not 0.0 <= float(sparsity_decay) < 1.0:
            raise ValueError("sparsity_decay must lie in [0, 1), got %r" % (sparsity_decay,))
        if sparse and symbolic_grad:
            raise NotImplementedError("a sparsity target with symbolic_grad=True is not supported")
        if centered and symbolic_grad:
            raise NotImplementedError("centered=True with symbolic_grad=True is not supported")
        if centered and not 0.0 < float(offset_rate) <= 1.0:
            raise ValueError("offset_rate must lie in (0, 1], got %r" % (offset_rate,))
        if symbolic_grad and self.gauss and not getattr(self, "error_free", True):
            raise NotImplementedError("symbolic_grad with a noisy GRBM (error_free=False) is not supported")
        if symbolic_grad:
            weightcost = 0.0           # tensor.grad of the free-energy difference has no such term
        W0 = None
        if weightcost != 0.0 and self.strict_reference:
            # rbm.py:415; same padded layout as W (a plain clone() would drop the leading dimension)
            snap = self.engine.alloc_matrix(self.n_visible, self.n_hidden, self.W.tensor.stride(0))
            if self._resume_W0 is not None:
                # resumed run: the constant is the W of the ORIGINAL graph construction (checkpoint.py)
                snap.copy_(as_tensor(self._resume_W0, self.engine))
                self._resume_W0 = None
            else:
                snap.copy_(self.W.tensor)
            W0 = SharedArray(None, engine=self.engine, _tensor=snap)
            self._W0_snapshot = W0
        if persistent is not None:
            persistent = shared(persistent, engine=self.engine)
            if persistent.tensor.stride(0) != self.W.tensor.stride(0):
                t = self.engine.alloc_matrix(persistent.shape[0], persistent.shape[1], self.W.tensor.stride(0))
                t.copy_(persistent.tensor)
                persistent.tensor = t
        updates = UpdatePlan(self, lr, k, lambda_1, lambda_2, weightcost, batch_size, persistent, W0,
                             symbolic_grad=symbolic_grad, centered=centered, offset_rate=offset_rate,
                             sparsity_target=sparsity_target, sparsity_cost=sparsity_cost, sparsity_decay=sparsity_decay,
                             sparsity_weights=sparsity_weights, grouped=self.visible_groups, learn_sigma=learn_sigma,
                             disc_weight=discriminative, gen_weight=generative if discriminative is not None else 1.0,
                             label_span=label_span, absent=missing)
        cost = CostHandle('pseudo_likelihood' if (persistent is not None and self.visible_groups is None) else 'reconstruction')
        return cost, updates

    def _pseudo_likelihood_value(self, x):
        """rbm.py:421-447 on the current minibatch; advances bit_i_idx (rbm.py:445)."""
        eng = self.engine
        xi = eng.round_flip(x)                                        # tensor.round
        fe_xi = eng.free_energy(xi, self.W.tensor, self.hbias.tensor, self.vbias.tensor, self.gauss)
        xi_flip = eng.round_flip(x, self.bit_i_idx)                   # bit i flipped (rbm.py:436)
        fe_flip = eng.free_energy(xi_flip, self.W.tensor, self.hbias.tensor, self.vbias.tensor, self.gauss)
        cost = eng.pl_cost(fe_xi, fe_flip, self.n_visible)            # rbm.py:442
        self.bit_i_idx = (self.bit_i_idx + 1) % self.n_visible
        return cost

    def get_pseudo_likelihood_cost(self, v):
        """Stochastic approximation to the pseudo-likelihood (rbm.py:421-447) of rows ``v``."""
        return float(self._pseudo_likelihood_value(as_tensor(self._units(v), self.engine)))

    def get_reconstruction_cost(self, pre_sigmoid_nv, v0):
        """rbm.py:449-482 evaluated on given arrays (monitoring helper; the step function
        computes the same quantity fused into the last propdown).  With ``visible_groups``: the categorical cross-entropy
        of the groups, formed from the log-sum-exp, plus the Bernoulli cross-entropy of the other columns; mean over rows."""
        if self.visible_groups is not None:
            pre = as_tensor(pre_sigmoid_nv, self.engine)
            return float(self.engine.group_softmax(pre, self.visible_groups, None, v0=as_tensor(v0, self.engine))[2]) / pre.shape[0]
        return float(self.engine.recon_cost(as_tensor(pre_sigmoid_nv, self.engine), as_tensor(v0, self.engine),
                                            gauss=False))

    # ------------------------------------------------------------------ stand-alone trainer
    def training(self, train_set_x, validation_set_x, training_epochs, batch_size=10,
                 learning_rate=0.1, k=1, initial_momentum=0.0, final_momentum=0.0,
                 weightcost=0.0, lambda_2=0.0, persistent=True, display_fn=None, graph_output=False, tempering=None,
                 visible_groups=None, discriminative=None, label_group=-1, generative=1.0, missing=False, centered=False,
                 offset_rate=0.01, sparsity_target=None, sparsity_cost=0.0, sparsity_decay=0.9, sparsity_weights=True):
        """rbm.py:484-520 (note: like the reference, ``lambda_2`` is accepted but not used).

        ``tempering=R`` (with ``persistent``): PCD whose negative chains are the beta = 1 replicas of ``batch_size``
        parallel-tempering ladders of R temperatures (Desjardins et al. 2010) -- every step is ``chains.run(1)``,
        ``chains.to_persistent``, the unchanged PCD step, ``chains.from_persistent``; the ladders stay in ``self.tempered``.
        None: nothing changes.  On a layer with ``visible_groups`` the ladders are the grouped ones (``tempered_chains``) and
        the step the grouped PCD step.  ``centered`` / ``offset_rate``: the centred gradient, ``sparsity_*``: the sparsity target
        (``get_cost_updates``).  ``visible_groups`` (not None): ``set_visible_groups`` first -- the layer trains with
        categorical visible units.  ``discriminative`` / ``label_group`` / ``generative``: the hybrid or purely discriminative
        objective of a classification RBM (``get_cost_updates``); ``generative=0`` needs ``persistent=False``.
        ``missing=True`` (needs ``persistent=False``): the tables may hold NaN for entries that were not measured
        (``get_cost_updates``); the free-energy gap is then taken over the observed units of every row."""
        if visible_groups is not None:
            self.set_visible_groups(visible_groups)
        if missing:
            self._refuse_missing(persistent=persistent, discriminative=discriminative, centered=centered, tempering=tempering,
                                 sparse=sparsity_target is not None and float(sparsity_cost) > 0.0)
        disc = dict(discriminative=discriminative, label_group=label_group, generative=generative) if discriminative is not None else {}
        if tempering is not None:
            if self.visible_groups is not None and not hasattr(self.engine, "temper_grouped"):
                self._no_groups("training(tempering=) on this engine")
            self._no_sigma("training(tempering=)")
        if persistent:
            persistent_chain = shared(numpy.zeros((batch_size, self.n_hidden), dtype=numpy.float32),
                                      engine=self.engine)               # rbm.py:496-498
        else:
            persistent_chain = None
        cost, updates = self.get_cost_updates(lr=learning_rate, k=k, weightcost=weightcost,
                                              batch_size=batch_size, persistent=persistent_chain,
                                              centered=centered, offset_rate=offset_rate, sparsity_target=sparsity_target,
                                              sparsity_cost=sparsity_cost, sparsity_decay=sparsity_decay,
                                              sparsity_weights=sparsity_weights, missing=missing, **disc)
        step_hooks = None
        if tempering is not None:
            if not persistent:
                raise ValueError("tempering needs persistent=True: the ladders' beta = 1 replicas are the PCD chains")
            chains = self.tempered = self.tempered_chains(batch_size, n_betas=int(tempering))
            chain_buffer = updates.persistent              # (the buffer the step reads and writes: on W's leading dimension)

            def before_step():
                chains.run(1)
                chains.to_persistent(chain_buffer)
            step_hooks = (before_step, lambda: chains.from_persistent(chain_buffer))
        return self.learn_model(train_set_x=train_set_x, validation_set_x=validation_set_x,
                                training_epochs=training_epochs, batch_size=batch_size,
                                initial_momentum=initial_momentum, final_momentum=final_momentum,
                                cost=cost, updates=updates, display_fn=display_fn,
                                graph_output=graph_output, step_hooks=step_hooks, missing=missing)

    def learn_model(self, train_set_x, validation_set_x, training_epochs, batch_size,
                    initial_momentum, final_momentum, cost, updates, display_fn, graph_output,
                    verbose=True, shuffle_rng=None, step_hooks=None, missing=False):
        """Epoch loop of rbm.py:522-629.  ``display_fn`` / ``graph_output`` are accepted and
        ignored (plotting is outside the engine).  Returns the per-epoch (cost, gap) list.
        ``step_hooks``: ``(before, after)`` callables run around every step (``training(tempering=...)``)."""
        before_step, after_step = step_hooks if step_hooks is not None else (None, None)
        train_set_x = shared(train_set_x, engine=self.engine)
        validation_set_x = shared(validation_set_x, engine=self.engine) if validation_set_x is not None else None
        train_rbm = function(updates, train_set_x, name='train_rbm')
        n_train_data = train_set_x.shape[0]
        n_val = validation_set_x.shape[0] if validation_set_x is not None else 0
        history = []
        start_time = timeit.default_timer()
        momentum = initial_momentum
        for epoch in range(training_epochs):
            if epoch == 6:                                               # rbm.py:584-585
                momentum = final_momentum
            _, minibatches = get_minibatches_idx(n_train_data, batch_size, shuffle=True, rng=shuffle_rng)
            dev_idx = self.engine.index_tensor(numpy.concatenate(minibatches))
            # costs are 0-d device scalars (views into the engine's cost blocks): kept unread for the whole epoch -- no
            # synchronisation inside it -- and read back with one copy per block at its end; the mean is formed on the host
            # in float64, as the reference's numpy.mean over its per-minibatch floats (rbm.py:587-592)
            costs = []
            views = list(torch.split(dev_idx, [len(b) for b in minibatches]))
            train_rbm.announce(views, host_indexes=minibatches)      # the epoch's order (a host-resident table starts feeding)
            for b_i in range(len(minibatches)):
                # the next minibatch of the epoch as a hint (gathered inside this step's statistics kernel)
                nxt = views[b_i + 1] if b_i + 1 < len(minibatches) else None
                if before_step is not None:
                    before_step()
                costs.append(train_rbm(views[b_i], momentum, next_indexes=nxt))
                if after_step is not None:
                    after_step()
            train_rbm.flush()
            mean_cost = float(numpy.sum(numpy.asarray(self.engine.cost_values(costs), dtype=numpy.float64))) / len(minibatches)
            feg = None
            if n_val:
                # rbm.py:597: gap between the first n_val training rows and the validation set
                feg = self.free_energy_gap(train_set_x[numpy.arange(n_val)], validation_set_x, **({"missing": True} if missing else {}))
            if verbose:
                print('Training epoch %d, cost is ' % epoch, mean_cost)
                print('Free energy gap is ', feg)
            history.append((mean_cost, feg))
        end_time = timeit.default_timer()
        if verbose:
            print('Training took %f minutes' % ((end_time - start_time) / 60.))
        return history


class GRBM(RBM):
    """Gaussian-Bernoulli RBM, mean-field visibles (rbm.py:631-728): unit variance as the reference's, or with a standard
    deviation per visible column once ``set_sigma`` / ``get_cost_updates(learn_sigma=)`` has made ``log_sigma``."""

    gauss = True
    # Clamp of log_sigma in a training step: sigma between 0.01 and 100.  A guard that keeps exp(+-log_sigma) and the scaled
    # rows far from float32 overflow if a step goes wrong -- not a tuned value; z-scored data sits well inside it.
    log_sigma_range = (-4.6, 4.6)

    def __init__(self, input=None, n_visible=784, n_hidden=500, W=None, hbias=None, vbias=None,
                 numpy_rng=None, theano_rng=None, error_free=True, engine=None, visible_groups=None):
        if visible_groups is not None:
            raise ValueError("visible_groups: a Gaussian visible layer (GRBM) has no categorical units")
        super(GRBM, self).__init__(input, n_visible, n_hidden, W, hbias, vbias, numpy_rng,
                                   theano_rng, engine=engine)
        self.error_free = error_free

    @property
    def sigma(self):
        """Host copy of the standard deviations exp(log_sigma), float32 [n_visible]; None on a unit-variance layer."""
        return None if self.log_sigma is None else numpy.exp(self.log_sigma.get_value()).astype(numpy.float32)

    def set_sigma(self, values):
        """Give the layer a standard deviation per visible column: ``values`` a positive scalar or [n_visible] array (None:
        back to the unit-variance layer).  With s = log sigma and u = x exp(-s), the row in units, the model is
        p(x) = p_u(u) exp(-sum(s)), p_u the unit-variance GRBM of (W, hbias, vbias): p(h | x) = sigmoid(hbias + u W),
        x | h ~ N(sigma (vbias + W h), sigma^2), F(x) = F_u(u) + sum(s), and log Z is p_u's.  Makes ``log_sigma`` and a zero
        ``log_sigma_speed``; the eager methods then take and return raw rows, and step functions built from now on train in
        units (``get_cost_updates``).  ``set_sigma(1.0)`` is the plain GRBM bit for bit."""
        if values is None:
            self.log_sigma = self.log_sigma_speed = None
            return
        v = numpy.asarray(values, dtype=numpy.float64)
        if v.ndim == 0:
            v = numpy.full(self.n_visible, float(v))
        if v.shape != (self.n_visible,) or not numpy.all(numpy.isfinite(v)) or not numpy.all(v > 0.0):
            raise ValueError("set_sigma needs a positive scalar or %d positive values" % self.n_visible)
        self.log_sigma = shared(numpy.log(v).astype(numpy.float32), name='log_sigma', engine=self.engine)
        self.log_sigma_speed = shared(numpy.zeros(self.n_visible, dtype=numpy.float32), name='log_sigma_speed', engine=self.engine)

    def sample_v_given_h(self, h0_sample):
        ''' [v1_mean, v1_mean, v1_sample]; linear mean, optional N(0,1) noise (rbm.py:647-660); with ``log_sigma``: both
        scaled back to raw units, so the noise has the column's standard deviation '''
        pre, mean, sample = self.engine.propdown(as_tensor(h0_sample, self.engine), self.W.tensor,
                                                 self.vbias.tensor, gauss=True,
                                                 add_noise=not self.error_free, rng=self._rng())
        if self.log_sigma is not None:
            mean, sample = self._raw(mean), (self._raw(sample) if not self.error_free else None)
            sample = mean if sample is None else sample
        return [self._wrap(mean), self._wrap(mean), self._wrap(sample)]

    def gibbs_hvh(self, h0_sample):
        ''' Gibbs step from the hidden state; h1 from the visible MEAN (rbm.py:662-671) '''
        pre_sigmoid_v1, v1_mean, v1_sample = self.sample_v_given_h(h0_sample)
        pre_sigmoid_h1, h1_mean, h1_sample = self.sample_h_given_v(v1_mean)
        return [pre_sigmoid_v1, v1_mean, v1_sample,
                pre_sigmoid_h1, h1_mean, h1_sample]

    def gibbs_vhv(self, v0_sample):
        ''' Gibbs step from the visible state; v1 from the hidden MEAN (rbm.py:673-682) '''
        pre_sigmoid_h1, h1_mean, h1_sample = self.sample_h_given_v(v0_sample)
        pre_sigmoid_v1, v1_mean, v1_sample = self.sample_v_given_h(h1_mean)
        return [pre_sigmoid_h1, h1_mean, h1_sample,
                pre_sigmoid_v1, v1_mean, v1_sample]

    def get_reconstruction_cost(self, pre_sigmoid_nv, v0):
        """mean((sigmoid(v1_mean) - v0)^2) over samples and features (rbm.py:690-699)."""
        return float(self.engine.recon_cost(as_tensor(pre_sigmoid_nv, self.engine), as_tensor(v0, self.engine),
                                            gauss=True))

    def training(self, train_set_x, validation_set_x, training_epochs, batch_size=10,
                 learning_rate=0.01, k=1, initial_momentum=0.0, final_momentum=0.0,
                 weightcost=0.0, lambda_1=0.0, lambda_2=0.1, persistent=False,
                 display_fn=None, graph_output=False, visible_groups=None, learn_sigma=None, missing=False, centered=False,
                 offset_rate=0.01, sparsity_target=None, sparsity_cost=0.0, sparsity_decay=0.9, sparsity_weights=True):
        """rbm.py:701-728: always CD (``persistent`` is ignored, as in the reference).  ``centered`` / ``offset_rate``: the
        centred gradient, ``sparsity_*``: the sparsity target, ``learn_sigma``: the rate of the learned per-column variance
        (``get_cost_updates``).  ``visible_groups`` is refused.  ``missing=True``: the tables may hold NaN for entries that
        were not measured (``get_cost_updates``)."""
        if visible_groups is not None:
            raise ValueError("visible_groups: a Gaussian visible layer (GRBM) has no categorical units")
        cost, updates = self.get_cost_updates(lr=learning_rate, k=k, lambda_1=lambda_1,
                                              lambda_2=lambda_2, weightcost=weightcost,
                                              batch_size=batch_size, learn_sigma=learn_sigma, centered=centered,
                                              offset_rate=offset_rate,
                                              sparsity_target=sparsity_target, sparsity_cost=sparsity_cost,
                                              sparsity_decay=sparsity_decay, sparsity_weights=sparsity_weights, missing=missing)
        return self.learn_model(train_set_x=train_set_x, validation_set_x=validation_set_x,
                                training_epochs=training_epochs, batch_size=batch_size,
                                initial_momentum=initial_momentum, final_momentum=final_momentum,
                                cost=cost, updates=updates, display_fn=display_fn,
                                graph_output=graph_output, missing=missing)
