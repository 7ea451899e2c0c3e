"""Multimodal glue: one DBN per modality, one joint DBN on top (the call surface of the reference's
src/MDBN.py:29-76, which its experiment drivers use: AMLsm2.py:38-92)."""
from __future__ import print_function

from .dbn import DBN
from .shared import shared

# the joint network of MDBN.py:31-42: Bernoulli 24 -> 3 on the concatenated modality outputs, CD-1
TOP_SHAPE = dict(gauss=False, hidden_layers_sizes=[24], n_outs=3)
TOP_SCHEDULE = dict(k=1, pretraining_epochs=[800, 800], pretrain_lr=[0.1, 0.1])
SPARSITY_KEYS = ("sparsity_target", "sparsity_cost", "sparsity_decay", "sparsity_weights")     # of RBM.get_cost_updates


def _fit(net, data, held_out, batch_size, graph_output, **schedule):
    net.training(data, batch_size, validation_set_x=held_out, graph_output=graph_output, **schedule)
    return net


def train_top(batch_size, graph_output, joint_train_set, joint_val_set, rng, visible_groups=None, discriminative=None,
              label_group=-1, generative=1.0, missing=False, sparsity_target=None, sparsity_cost=0.0, sparsity_decay=0.9,
              sparsity_weights=True, centered=False, offset_rate=0.01):
    """Joint DBN over the concatenated top-layer activations of the modalities (MDBN.py:31-42).  ``sparsity_*``: the sparsity
    target, ``centered`` / ``offset_rate``: the centred gradient (``RBM.get_cost_updates``).  ``visible_groups``: categorical
    units in the joint layer (``RBM.__init__``) -- a one-hot label block appended to the activations makes it a
    classification RBM, read out by ``RBM.label_posterior`` / ``RBM.predict``; ``discriminative`` / ``label_group`` /
    ``generative`` train the joint layer for that label (the hybrid objective of ``RBM.get_cost_updates``).  ``missing=True``:
    the joint table may hold NaN where a patient lacks a modality (``train_joint`` builds such a table) -- every layer trains
    by the absent-unit step (``DBN.training``)."""
    joint = shared(joint_train_set)
    net = DBN(numpy_rng=rng, n_ins=joint.shape[1], visible_groups=visible_groups, **TOP_SHAPE)
    return _fit(net, joint, joint_val_set, batch_size, graph_output, centered=centered, offset_rate=offset_rate,
                sparsity_target=sparsity_target, sparsity_cost=sparsity_cost, sparsity_decay=sparsity_decay,
                sparsity_weights=sparsity_weights, **TOP_SCHEDULE, **({"missing": True} if missing else {}),
                **(dict(discriminative=discriminative, label_group=label_group, generative=generative) if discriminative is not None else {}))


def build_bottom_layer(n_visible, layers_sizes, rng, visible_groups=None):
    """The (untrained) DBN of one modality: Gaussian first layer, ``layers_sizes[-1]`` output nodes (MDBN.py:58-62).
    Constructing it is the only thing that draws from ``rng`` (dbn.py:110-114,155-159).  ``visible_groups``: a categorical
    modality (copy-number calls, mutation classes: ``utils.one_hot_groups``) -- a Bernoulli first layer with those softmax
    groups instead."""
    return DBN(numpy_rng=rng, n_ins=n_visible, hidden_layers_sizes=layers_sizes[:-1], n_outs=layers_sizes[-1],
               gauss=visible_groups is None, visible_groups=visible_groups)


def train_modalities(modalities, rng, group="auto", shuffle_seed=None, graph_output=False):
    """One DBN per modality, as successive ``train_bottom_layer`` calls with one ``rng`` threaded through them
    (AMLsm2.py:38-62) -- placed MODALITY-PARALLEL when a process group of N > 1 ranks is up (the c5
    alternative to row-sharding tiny layers): the modalities are independent until the joint layer, so modality i
    is trained on rank i % N alone, with single-process step functions and no collective per step, and its
    parameters are broadcast once when it is done.

    ``modalities``: ordered list of dicts with ``train_set``, optional ``validation_set``, and the keyword
    arguments of ``train_bottom_layer`` (batch_size, k, layers_sizes, pretraining_epochs, pretrain_lr, lambda_1,
    lambda_2, sparsity_target, sparsity_cost, sparsity_decay, sparsity_weights).  Returns ``[(net, out_train, out_val), ...]`` in the same order, identical on every rank.

    Every rank CONSTRUCTS all networks in order -- construction is all that consumes ``rng``, so the initial weights
    and the state ``rng`` is left in (for ``train_top``) are those of the sequential reference on every rank.  The
    minibatch shuffles cannot come from numpy's global state as in the reference (utils.py:62: its sequence would
    depend on how long the previous modality trained): modality i shuffles with ``RandomState(shuffle_seed + i)``
    (``shuffle_seed`` defaults to 0 under a process group; None in a single process keeps the reference's global
    state).  With the same ``shuffle_seed`` the placement does not change any result."""
    import numpy
    from . import dist
    grp = dist.default_group() if group == "auto" else group
    world, rank = (grp.world_size, grp.rank) if grp is not None else (1, 0)
    if world > 1 and shuffle_seed is None:
        shuffle_seed = 0
    nets = []
    for i, m in enumerate(modalities):
        rows = shared(m["train_set"])
        net = build_bottom_layer(rows.shape[1], m.get("layers_sizes", [40]), rng)
        if shuffle_seed is not None:
            net.shuffle_rng = numpy.random.RandomState(shuffle_seed + i)
        if world > 1:
            net.data_parallel = None                 # trained by its owner alone
        nets.append((net, rows, None if m.get("validation_set") is None else shared(m["validation_set"])))
    for i, (m, (net, rows, held_out)) in enumerate(zip(modalities, nets)):
        if i % world == rank:
            _fit(net, rows, held_out, m.get("batch_size", 20), graph_output, k=m.get("k", 1),
                 pretraining_epochs=m.get("pretraining_epochs", [800]), pretrain_lr=m.get("pretrain_lr", [0.005]),
                 lambda_1=m.get("lambda_1", 0.0), lambda_2=m.get("lambda_2", 0.1),
                 **{key: m[key] for key in SPARSITY_KEYS if key in m})
    if world > 1:
        import torch.distributed as td
        for i, (net, _, _) in enumerate(nets):       # one broadcast per array, once per modality
            for r in net.rbm_layers:
                for arr in (r.W, r.hbias, r.vbias, r.W_speed, r.hbias_speed, r.vbias_speed):
                    t = arr.tensor
                    base = t._base if getattr(t, "_base", None) is not None else t     # the padded storage of a matrix
                    td.broadcast(base, src=i % world, group=grp.pg)
                    arr.version += 1                 # caches keyed on the array (lower-layer activations) are stale
            # the host-side counters of the owner's layers (Philox step, update count, pseudo-likelihood bit): replicas stay
            # interchangeable for whatever follows (sampling, further training, checkpoints)
            state = [[(r._rng_step, r._n_updates, r.bit_i_idx) for r in net.rbm_layers]]
            td.broadcast_object_list(state, src=i % world, group=grp.pg)
            for r, (step, n_upd, bit) in zip(net.rbm_layers, state[0]):
                r._rng_step, r._n_updates, r.bit_i_idx = step, max(n_upd, r._n_updates + 1), bit
    return [(net, net.get_output(rows), net.get_output(held_out)) for net, rows, held_out in nets]


def train_bottom_layer(train_set, validation_set, batch_size=20, k=1, layers_sizes=[40],
                       pretraining_epochs=[800], pretrain_lr=[0.005], lambda_1=0.0, lambda_2=0.1,
                       rng=None, graph_output=False, visible_groups=None, learn_sigma=None, missing=False, sparsity_target=None,
                       sparsity_cost=0.0, sparsity_decay=0.9, sparsity_weights=True, centered=False, offset_rate=0.01):
    """DBN of one modality, Gaussian first layer (MDBN.py:45-76).  Returns the network and its
    outputs for the training and the validation rows (None without validation rows).  ``sparsity_*``: the sparsity target,
    ``centered`` / ``offset_rate``: the centred gradient (``RBM.get_cost_updates``).  ``visible_groups``: a categorical
    modality, on a Bernoulli first layer with those softmax groups (``build_bottom_layer``).  ``learn_sigma``: the Gaussian
    first layer learns a standard deviation per column at that rate (``DBN.training``).  ``missing=True``: the tables may hold
    NaN for entries that were not measured (a sparse mutation or methylation table with holes; a row of NaN: a patient without
    this modality) -- every layer trains by the absent-unit step, and the outputs are those of ``get_output(missing=True)``."""
    rows = shared(train_set)
    held_out = None if validation_set is None else shared(validation_set)
    n_visible, n_top = rows.shape[1], layers_sizes[-1]
    if DBN.verbose:
        print('Visible nodes: %i' % n_visible)
        print('Output nodes: %i' % n_top)
    net = _fit(build_bottom_layer(n_visible, layers_sizes, rng, visible_groups),
               rows, held_out, batch_size, graph_output, k=k, pretraining_epochs=pretraining_epochs,
               pretrain_lr=pretrain_lr, lambda_1=lambda_1, lambda_2=lambda_2, centered=centered, offset_rate=offset_rate,
               sparsity_target=sparsity_target, sparsity_cost=sparsity_cost, sparsity_decay=sparsity_decay,
               sparsity_weights=sparsity_weights, **({} if learn_sigma is None else dict(learn_sigma=learn_sigma)),
               **({"missing": True} if missing else {}))
    if missing:
        return net, net.get_output(rows, missing=True), net.get_output(held_out, missing=True)
    return net, net.get_output(rows), net.get_output(held_out)


def joint_table(nets, inputs):
    """The joint layer's table for patients who may lack modalities: ``inputs[i]`` is the data matrix of modality i, or None
    when nobody has it, with the NaN-row convention of ``impute_modalities`` -- a row of NaN: this patient lacks modality i.
    Every modality goes up by ``get_output(missing=True)`` (a row that is only partly NaN is allowed: the modality network
    takes it zero-filled), and a patient without the modality gets a block of NaN.  A patient with no modality at all is
    refused (ValueError).  Returns a float32 host array [N, sum of the modality tops]."""
    import numpy
    widths = [net.stacked_layers_sizes[-1] for net in nets]
    if len(inputs) != len(nets):
        raise ValueError("one input (or None) per modality")
    rows = [len(x) for x in inputs if x is not None]
    if not rows or len(set(rows)) != 1:
        raise ValueError("at least one modality must be given, and all given ones need the same number of rows")
    table = numpy.full((rows[0], sum(widths)), numpy.nan, dtype=numpy.float32)
    lo = 0
    for net, x, w in zip(nets, inputs, widths):
        if x is not None:
            x = numpy.asarray(getattr(x, "get_value", lambda: x)(), dtype=numpy.float32)
            table[:, lo:lo + w] = net.get_output(x, missing=True)       # (rows of NaN come out as rows of NaN)
        lo += w
    nobody = numpy.flatnonzero(numpy.isnan(table).all(axis=1))
    if nobody.size:
        raise ValueError("%d patient(s) have no modality at all (first: row %d): nothing to train on" % (nobody.size, nobody[0]))
    return table


def train_joint(nets, inputs, batch_size, rng, graph_output=False, validation_inputs=None, **top):
    """The joint DBN trained on ALL patients, whichever modalities each one has -- what replaces keeping only the patients
    present in every table (data/AML/common_pat_id.sh).  ``nets``: the trained modality DBNs in the joint layer's column
    order; ``inputs``: as ``joint_table``; ``validation_inputs``: the same for held-out patients, or None.  The joint table
    holds a block of NaN where a patient lacks a modality, and ``train_top(..., missing=True)`` trains on it: such a block is
    absent from that patient's RBM (Salakhutdinov, Mnih & Hinton 2007).  ``top``: further keywords of ``train_top`` (what
    ``missing=True`` does not compose with is refused there).  Returns the joint DBN."""
    table = joint_table(nets, inputs)
    held_out = None if validation_inputs is None else joint_table(nets, validation_inputs)
    return train_top(batch_size, graph_output, table, held_out, rng, missing=True, **top)


def impute_modalities(nets, joint, inputs, n_steps=1000, burn_in=200, n_chains=8):
    """Answer for rows of which some modality was never measured (the patients data/AML/common_pat_id.sh drops).

    ``nets``: the modality DBNs in the joint layer's column order; ``joint``: the joint DBN (``train_top``);
    ``inputs[i]``: the data matrix of modality i, or None when it is missing for every row.  A row of NaNs inside a given
    matrix marks that modality as missing for that row alone, so rows may differ in what they lack (a row that is only partly
    NaN is refused).  Observed modalities go up
    (``get_output``), the joint layer's first RBM runs ``RBM.impute`` with the column-block mask -- clamped Gibbs sampling on
    the device, ``n_chains`` chains per row -- and the result is ``(joint_visible [N, sum of tops], joint_top =
    joint.get_output(joint_visible), {i: nets[i].down_pass(block_i)})`` for every modality i that is missing somewhere
    (rows where it was observed reproduce the mean-field reconstruction of their own block)."""
    import numpy
    widths = [net.stacked_layers_sizes[-1] for net in nets]
    if len(inputs) != len(nets):
        raise ValueError("one input (or None) per modality")
    rows = [len(x) for x in inputs if x is not None]
    if not rows or len(set(rows)) != 1:
        raise ValueError("at least one modality must be given, and all given ones need the same number of rows")
    N = rows[0]
    visible = numpy.zeros((N, sum(widths)), dtype=numpy.float32)
    mask = numpy.zeros((N, sum(widths)), dtype=numpy.float32)
    missing, lo = [], 0
    for i, (net, x, w) in enumerate(zip(nets, inputs, widths)):
        seen = numpy.zeros(N, dtype=bool)
        if x is not None:
            x = numpy.asarray(getattr(x, "get_value", lambda: x)(), dtype=numpy.float32)
            nan = numpy.isnan(x)
            seen = ~nan.all(axis=1)
            if (nan.any(axis=1) & seen).any():
                raise ValueError("modality %d: a row is partly NaN; a missing modality is a row of NaN only" % i)
            if seen.any():
                visible[seen, lo:lo + w] = net.get_output(x[seen])
        mask[seen, lo:lo + w] = 1.0
        if not seen.all():
            missing.append((i, lo, w))
        lo += w
    if not mask.any(axis=1).all():
        raise ValueError("a row with no observed modality cannot be imputed")
    joint_visible, _ = joint.rbm_layers[0].impute(visible, mask, n_steps=n_steps, burn_in=burn_in, n_chains=n_chains)
    return joint_visible, joint.get_output(joint_visible), {i: nets[i].down_pass(joint_visible[:, lo:lo + w])
                                                           for i, lo, w in missing}


def log_likelihood_bound(nets, joint, inputs, n_samples=64, **kw):
    """Variational lower bound on log p of the raw data of every modality under the whole multimodal model, in nats per row
    (``DBN.log_likelihood_bound`` for the forest of networks; ``bound.stack_bound``).

    ``nets`` / ``joint`` as ``impute_modalities``; ``inputs``: one data matrix per modality, a list in the order of ``nets`` or
    a dict {modality index: matrix} with exactly the keys 0 .. len(nets) - 1.  Every modality DBN is sampled up through ALL
    its layers -- each contributes a directed term log p(x_{l-1} | x_l) and the entropy of its recognition distribution --,
    the sampled tops are concatenated in the column order of the joint layer (the order ``train_top`` is given the outputs
    in), and the joint DBN continues up to its top RBM, whose free energy and log Z close the bound.  Keywords: ``log_z``,
    ``chunk_rows``, ``trace`` and those of ``RBM.log_partition``.  Returns a ``bound.StackBound``: the fields of ``bound.Bound``
    plus ``modality_rows`` [M, N] (the terms each modality's layers add) and ``joint_rows`` [N]; ``rows`` is their sum.  Every
    sampled layer consumes one RNG step of its own RBM."""
    from .bound import stack_bound
    if isinstance(inputs, dict):
        if set(inputs) != set(range(len(nets))):
            raise ValueError("inputs must have exactly the keys 0 .. %d, got %r" % (len(nets) - 1, sorted(inputs, key=repr)))
        inputs = [inputs[i] for i in range(len(nets))]
    if len(inputs) != len(nets) or any(x is None for x in inputs):
        raise ValueError("one input per modality: every modality is given")
    return stack_bound(list(zip(nets, inputs)), joint, n_samples=n_samples, **kw)


def fine_tune(nets, joint, inputs, epochs, batch_size=20, *, lr, k=1, momentum=0.0, weightcost=0.0, lambda_1=0.0, lambda_2=0.0,
              top_lr=None, on_epoch=None, path="auto"):
    """Up-down fine-tuning of the whole multimodal model (``DBN.fine_tune`` over the structure ``log_likelihood_bound`` walks;
    ``updown.py``): every layer of every modality DBN and the joint DBN's lower layers are directed and get generative weights
    of their own, the joint DBN's last RBM is the top.  The wake pass concatenates the sampled modality tops in the order of
    ``nets``, the sleep pass splits the dream back by the same column blocks.  ``inputs``: one data matrix per modality, a list
    or a dict {modality index: matrix}.  A modality network whose input layer has ``visible_groups`` dreams one category per group
    and is trained against the grouped means (its data rows must be one-hot per group: ValueError); groups in the JOINT network's
    own input layer and an engine without ``updown_gen_step_grouped`` are refused (NotImplementedError) before anything is drawn.
    The epoch order comes from ``joint.shuffle_rng``.  Returns the per-epoch record
    ``[(sum over the modalities of the mean -log p(x_0 | x_1) per row, the top RBM's mean monitoring cost), ...]``."""
    from . import updown
    if isinstance(inputs, dict):
        if set(inputs) != set(range(len(nets))):
            raise ValueError("inputs must have exactly the keys 0 .. %d, got %r" % (len(nets) - 1, sorted(inputs, key=repr)))
        inputs = [inputs[i] for i in range(len(nets))]
    return updown.fine_tune(list(nets), joint, list(inputs), epochs, batch_size, lr=lr, k=k, momentum=momentum,
                            weightcost=weightcost, lambda_1=lambda_1, lambda_2=lambda_2, top_lr=top_lr, on_epoch=on_epoch,
                            path=path)


def modality_log_likelihood(nets, joint, inputs, target, n_chains=64, n_betas=1000, path=0, base_data=None):
    """How well the joint layer predicts modality ``target`` from the others, in nats per row (Srivastava & Salakhutdinov
    2012): log p(block_target | the other blocks) under the joint DBN's first RBM.

    ``nets`` / ``joint`` as ``impute_modalities``; ``inputs[i]``: the data matrix of modality i -- every modality is given.
    All modalities go up (``get_output``); the target block is scored as the 0 / 1 state ``activation >= 0.5`` (a Bernoulli
    joint layer gives probability to 0 / 1 states only), the other blocks are held at their activations, and
    ``RBM.conditional_log_likelihood`` -- clamped AIS on the device, ``n_chains`` chains per row through ``n_betas``
    temperatures from the base-rate model -- scores it.  ``base_data``: the stacked training activations the base rates are
    taken from (``RBM.base_rate_vbias``; None: the rows' own activations).  Returns a dict: ``log_p [N]``, ``std_err [N]``
    (that of the AIS estimate of each row's partition function), ``baseline [N]`` (the same 0 / 1 block under independent
    Bernoulli units at the block's base rate, float64 on the host), ``gain`` = mean(log_p - baseline) and ``gain_std_err`` =
    sqrt(sum std_err^2) / N.  Consumes 2 n_betas - 1 RNG steps of the joint layer's first RBM.

    The blocks are the modality tops.  A one-hot label block of a joint layer with ``visible_groups`` is not one of ``nets`` and
    is not scored here: call ``joint.rbm_layers[0].conditional_log_likelihood(v, unit_mask)`` with a mask that frees the label
    block (a group is observed or missing as a whole)."""
    import numpy
    widths = [net.stacked_layers_sizes[-1] for net in nets]
    if len(inputs) != len(nets) or any(x is None for x in inputs):
        raise ValueError("one input per modality: every modality is given")
    if not 0 <= int(target) < len(nets):
        raise ValueError("target %r is not one of the %d modalities" % (target, len(nets)))
    rbm = joint.rbm_layers[0]
    if rbm.gauss:
        raise ValueError("the joint layer has Gaussian visibles: a block of it is not a 0 / 1 state")
    blocks = [numpy.asarray(net.get_output(numpy.asarray(getattr(x, "get_value", lambda: x)(), dtype=numpy.float32)), dtype=numpy.float32)
              for net, x in zip(nets, inputs)]
    if len(set(len(b) for b in blocks)) != 1:
        raise ValueError("all modalities need the same number of rows")
    stacked = numpy.concatenate(blocks, axis=1)
    lo = sum(widths[:int(target)])
    hi = lo + widths[int(target)]
    visible = stacked.copy()
    visible[:, lo:hi] = (stacked[:, lo:hi] >= 0.5).astype(numpy.float32)
    mask = numpy.ones((1, stacked.shape[1]), dtype=numpy.float32)
    mask[:, lo:hi] = 0.0
    base_vbias = rbm.base_rate_vbias(stacked if base_data is None else base_data)
    log_p, err = rbm.conditional_log_likelihood(visible, mask, n_chains=n_chains, n_betas=n_betas, base_vbias=base_vbias, path=path)
    bA = numpy.asarray(base_vbias, dtype=numpy.float64)[lo:hi]
    baseline = visible[:, lo:hi].astype(numpy.float64) @ bA - numpy.logaddexp(0.0, bA).sum()
    return dict(log_p=log_p, std_err=err, baseline=baseline, gain=float(numpy.mean(log_p - baseline)),
                gain_std_err=float(numpy.sqrt((err ** 2).sum()) / len(err)))
