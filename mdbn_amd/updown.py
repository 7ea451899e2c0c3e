"""Up-down fine-tuning of a pre-trained DBN or multimodal stack (Hinton, Osindero & Teh 2006, "A fast learning algorithm for
deep belief nets", the contrastive wake-sleep of its appendix B): the host side of ``DBN.fine_tune`` and ``MDBN.fine_tune``.

Greedy pre-training leaves the recognition weights (upwards) and the generative weights (downwards) of every layer below the
top RBM as ONE matrix.  Fine-tuning unties them -- ``rbm.W_gen``, a copy of W on W's leading dimension, with a zero
``rbm.W_gen_speed`` -- and one step on a minibatch x_0 of n rows is, with pre-step parameters in every pass:

    wake    l = 0 .. L-2:  q_l = sigmoid(x_l W_l + hbias_l),  x_{l+1} ~ Bernoulli(q_l)              (RBM l's stream)
    top     the CD-k statistics of the top RBM on x_{L-1}; y_{L-1} = the visible sample of its last Gibbs step
    sleep   l = L-2 .. 0:  p_l = act(y_{l+1} G_l^T + vbias_l),  y_l ~ p_l,  r_l = sigmoid(y_l W_l + hbias_l)
    then    the top RBM's update, and for every directed layer
            generative   S = (x_l - g_l)^T x_{l+1},  s_v = sum_r (x_l - g_l),  g_l = act(x_{l+1} G_l^T + vbias_l)
                         -> G_l, W_gen_speed, vbias_l, vbias_speed                                   (hbias untouched)
            recognition  S = y_l^T (y_{l+1} - r_l),  s_h = sum_r (y_{l+1} - r_l)
                         -> W_l, W_speed, hbias_l, hbias_speed                                       (vbias untouched)

all by the engine's update rule (lr, momentum, weightcost, lambda_1, lambda_2; S over batch_size, bias sums over the rows
present).  At a Gaussian bottom layer y_0 is the linear mean, plus N(0, 1) noise exactly when that GRBM is ``error_free=False``.
At the input layer of a network with ``visible_groups`` act is the softmax inside every group and the sigmoid on the other
columns: y_0 holds one category per group, drawn by the engine's ``group_softmax`` from the linear pre-activations through
``down_W`` (one uniform per group, at its first column: the addressing of ``RBM.sample_v_given_h``), g_0 is the grouped mean
(``updown_gen_step_grouped``; the same S and s_v are the exact gradient of sum_r log p(x_0 | x_1)), and the recognition rule
sees y_0 as the 0 / 1 matrix it is.  The data rows must be one-hot in every group (ValueError); an engine without
``updown_gen_step_grouped`` and a JOINT network whose own input layer has groups -- its input is sampled, not one-hot data --
are refused (NotImplementedError) before anything is drawn.
Every draw advances ``_rng_step`` of the RBM whose conditional is sampled: two runs from the same seeds agree bit for bit.

A stack is ``(nets, joint)`` as ``bound.stack_bound`` walks it: every layer of every modality DBN and the joint DBN's lower
layers are directed, the joint's last RBM is the top; the wake pass concatenates the modality tops in the order given, the sleep
pass splits the dream back by column blocks.  ``joint`` None: the one DBN of ``nets`` alone, its last RBM the top."""
import collections

import numpy

from .engine import RngAddr
from .shared import HostTable, SharedArray, shared
from .utils import get_minibatches_idx

PATHS = {"auto": 0, "fused": 1, "composed": 2}

# lr .. lambda_2: the update rule's arguments for the directed layers; top_lr: the top RBM's learning rate; k: its CD steps;
# batch_size: the divisor of S (the batch_size ARGUMENT, as in the CD step); path: "auto" | "fused" | "composed"
Hyper = collections.namedtuple("Hyper", "lr top_lr k momentum weightcost lambda_1 lambda_2 batch_size path")
# what one step leaves for inspection: the wake states x / dream states y per network (bottoms first, the joint last; x[m][l] is
# the input of directed layer l of network m), the recognition means r of the dream, and the two costs (0-d engine scalars)
StepRecord = collections.namedtuple("StepRecord", "x y r gen_cost top_cost")


def _rng(r):
    return RngAddr(r.theano_rng.seed, r.stream_id, r._take_step(), 0, 0)


def untie(rbm):
    """Give ``rbm`` generative weights of its own: a copy of W on W's leading dimension, and a zero speed (no-op when untied)."""
    if rbm.W_gen is not None:
        return
    eng, W = rbm.engine, rbm.W.tensor
    G = eng.alloc_matrix(W.shape[0], W.shape[1], W.stride(0))
    G.copy_(W)
    rbm.W_gen = SharedArray(None, name='W_gen', engine=eng, _tensor=G)
    rbm.W_gen_speed = SharedArray(None, name='W_gen_speed', engine=eng, _tensor=eng.alloc_matrix(W.shape[0], W.shape[1], W.stride(0)))


def plan(nets, joint):
    """(directed layers per network -- the bottoms, then the joint if any --, the top RBM)."""
    if not nets or (joint is None and len(nets) != 1):
        raise ValueError("one DBN, or modality DBNs under a joint DBN")
    top_net = joint if joint is not None else nets[0]
    if joint is None and top_net.n_layers < 2:
        raise ValueError("up-down fine-tuning needs a directed layer below the top RBM: n_layers >= 2")
    if joint is not None and joint.n_ins != sum(net.stacked_layers_sizes[-1] for net in nets):
        raise ValueError("the joint network has %d inputs, the modalities' tops %d units"
                         % (joint.n_ins, sum(net.stacked_layers_sizes[-1] for net in nets)))
    directed = [list(net.rbm_layers) if joint is not None else list(net.rbm_layers[:-1]) for net in nets]
    if joint is not None:
        directed.append(list(joint.rbm_layers[:-1]))
    return directed, top_net.rbm_layers[-1]


def _single_device():
    from . import dist
    grp = dist.default_group()
    if grp is not None and grp.world_size > 1:
        raise NotImplementedError("up-down fine-tuning runs on one device (a process group of %d ranks is up)" % grp.world_size)


def _check_groups(nets, joint):
    """What a stack with categorical visible units needs, before anything is planned, drawn or called: an engine with the
    grouped generative rule, and groups at the input layers of the modality networks only."""
    for net in list(nets) + ([joint] if joint is not None else []):
        if not hasattr(net.engine, "updown_gen_step_grouped"):
            net.rbm_layers[0]._no_groups("fine_tune on this engine")
    if joint is not None and joint.rbm_layers[0].visible_groups is not None:
        raise NotImplementedError("fine_tune with categorical visible units (visible_groups) in the JOINT network's input layer is "
                                  "not built: its input is sampled, not one-hot data")


def _wake(eng, layers, x):
    xs = [x]
    for r in layers:
        xs.append(eng.propup(xs[-1], r.W.tensor, r.hbias.tensor, rng=_rng(r), want_pre=False, want_mean=False)[2])
    return xs


def _sleep(eng, layers, y_top):
    """The dream below ``y_top`` through ``layers`` (top-down) and its recognition means: (ys, rs), bottom first."""
    ys, rs = [y_top], []
    for r in reversed(layers):
        if r.visible_groups is not None:
            # one category per group from the linear pre-activations through the GENERATIVE weights (RBM._grouped_down reads W)
            pre = eng.propdown(ys[0], r.down_W, r.vbias.tensor, gauss=True, add_noise=False, rng=None)[1]
            y = eng.group_softmax(pre, r.visible_groups, _rng(r))[1]
        else:
            noisy = bool(r.gauss and not getattr(r, "error_free", True))
            y = eng.propdown(ys[0], r.down_W, r.vbias.tensor, gauss=r.gauss, add_noise=noisy, rng=_rng(r))[2]
        rs.insert(0, eng.propup(y, r.W.tensor, r.hbias.tensor, want_pre=False, want_sample=False)[1])
        ys.insert(0, y)
    return ys, rs


def step(nets, joint, rows, hp):
    """One up-down step on the minibatch ``rows`` (one device matrix per modality, the same n rows each).  Returns a
    ``StepRecord``."""
    import torch
    directed, top = plan(nets, joint)
    eng = top.engine
    for layers in directed:
        for r in layers:
            untie(r)
    n = int(rows[0].shape[0])
    # wake: recognition samples upwards
    xs = [_wake(eng, layers, eng.as_matrix(x)) for layers, x in zip(directed, rows)]
    if joint is not None:
        xs.append(_wake(eng, directed[-1], eng.as_matrix(torch.cat([x[-1] for x in xs], dim=1))))
    # top: the CD-k statistics of the top RBM on the wake state; the dream starts from its last visible sample
    stats, scratch = eng.cd_step(xs[-1][-1], None, top.W.tensor, top.hbias.tensor, top.vbias.tensor, top.gauss, hp.k,
                                 RngAddr(top.theano_rng.seed, top.stream_id, top._take_step(), 0, 0), keep_f32=True)
    y_top = eng.as_matrix(scratch.vs[:n]).clone()
    # sleep: the generative model dreams downwards, the recognition model looks at the dream
    ys, rs = [None] * len(directed), [None] * len(directed)
    if joint is not None:
        ys[-1], rs[-1] = _sleep(eng, directed[-1], y_top)
        lo = 0
        for m, net in enumerate(nets):
            w = net.stacked_layers_sizes[-1]
            ys[m], rs[m] = _sleep(eng, directed[m], eng.as_matrix(ys[-1][0][:, lo:lo + w].clone()))
            lo += w
    else:
        ys[0], rs[0] = _sleep(eng, directed[0], y_top)
    # updates, after every pass: the top RBM's, then the delta rules of every directed layer
    ldv = getattr(xs[-1][-1], "stride", lambda _: None)(0)
    top_cost = eng.apply_update(top.W.tensor, top.W_speed.tensor, None, top.hbias.tensor, top.hbias_speed.tensor,
                                top.vbias.tensor, top.vbias_speed.tensor, stats, hp.top_lr, hp.lambda_1, hp.lambda_2,
                                hp.weightcost, hp.momentum, hp.batch_size, n, 1.0 / n, 0, ldv)
    top._n_updates += 1
    rule = (hp.lr, hp.lambda_1, hp.lambda_2, hp.weightcost, hp.momentum, hp.batch_size, n)
    gen_cost = []
    for m, layers in enumerate(directed):
        for l, r in enumerate(layers):
            if r.visible_groups is not None:
                c = eng.updown_gen_step_grouped(xs[m][l], xs[m][l + 1], r.W_gen.tensor, r.W_gen_speed.tensor, r.vbias.tensor,
                                                r.vbias_speed.tensor, r.visible_groups, *rule, cost_scale=1.0 / n, path=hp.path)
            else:
                c = eng.updown_gen_step(xs[m][l], xs[m][l + 1], r.W_gen.tensor, r.W_gen_speed.tensor, r.vbias.tensor,
                                        r.vbias_speed.tensor, r.gauss, *rule, cost_scale=1.0 / n, path=hp.path)
            if l == 0 and (joint is None or m < len(nets)):
                gen_cost.append(c)                      # -log p(x_0 | x_1) of the data rows, per row
            eng.updown_rec_step(ys[m][l], ys[m][l + 1], rs[m][l], r.W.tensor, r.W_speed.tensor, r.hbias.tensor,
                                r.hbias_speed.tensor, *rule, path=hp.path)
            r._n_updates += 1
    return StepRecord(xs, ys, rs, gen_cost, top_cost)


def _minibatch(data, idx, eng):
    if isinstance(data, HostTable) and data._mirror is None:
        return data.rows(idx)
    return eng.gather_rows(data.tensor, idx)


def fine_tune(nets, joint, inputs, epochs, batch_size=20, lr=None, k=1, momentum=0.0, weightcost=0.0, lambda_1=0.0,
              lambda_2=0.0, top_lr=None, on_epoch=None, path="auto"):
    """``epochs`` epochs of up-down steps over the rows of ``inputs`` (one table per modality).  The epoch order comes from
    the ``shuffle_rng`` of the joint DBN (of the DBN itself without one), as in ``DBN.training``.  Returns the per-epoch
    record: ``[(mean generative cost of x_0 under the wake pass, the top RBM's mean monitoring cost), ...]``;
    ``on_epoch(epoch, record)`` is called after every epoch."""
    if lr is None:
        raise TypeError("fine_tune needs lr=")
    if path not in PATHS:
        raise ValueError("path must be one of %r, got %r" % (sorted(PATHS), path))
    for net in nets:
        net.rbm_layers[0]._no_sigma("fine_tune")
    _check_groups(nets, joint)
    directed, top = plan(nets, joint)
    _single_device()
    if len(inputs) != len(nets) or any(x is None for x in inputs):
        raise ValueError("one input per modality: every modality is given")
    eng = top.engine
    tables = [shared(x, engine=eng) for x in inputs]
    N = len(tables[0])
    if N < 1 or any(len(t) != N for t in tables):
        raise ValueError("all modalities need the same number (>= 1) of rows")
    for net, t in zip(nets, tables):
        if t.shape[1] != net.n_ins:
            raise ValueError("data has %d columns, the network %d inputs" % (t.shape[1], net.n_ins))
    for net, t in zip(nets, tables):
        if net.rbm_layers[0].visible_groups is not None:
            # g_0 is a softmax and the cost linear in the row only on one-hot groups (the host copy is checked, as the bound's)
            net.rbm_layers[0]._check_one_hot(t)
    hp = Hyper(float(lr), float(lr if top_lr is None else top_lr), int(k), float(momentum), float(weightcost), float(lambda_1),
               float(lambda_2), int(batch_size), path)
    owner = joint if joint is not None else nets[0]
    history = []
    for epoch in range(1, int(epochs) + 1):
        batches = get_minibatches_idx(N, batch_size, shuffle=True, rng=owner.shuffle_rng)[1]
        gen, topc = [], []
        for b in batches:
            idx = eng.index_tensor(numpy.asarray(b))
            rec = step(nets, joint, [_minibatch(t, idx, eng) for t in tables], hp)
            gen.append(rec.gen_cost)
            topc.append(rec.top_cost)
        flat = eng.cost_values([c for g in gen for c in g] + topc)
        per = len(gen[0]) if gen else 0
        g_vals = [sum(flat[i * per:(i + 1) * per]) for i in range(len(gen))]
        t_vals = flat[len(gen) * per:]
        history.append((float(numpy.mean(g_vals)), float(numpy.mean(t_vals))))
        if on_epoch is not None:
            on_epoch(epoch, history[-1])
    for net in list(nets) + ([joint] if joint is not None else []):
        net._lower_cache = {}                   # the recognition weights have moved: cached activations are stale
    return history
