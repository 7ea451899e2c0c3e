"""Variational lower bound on log p(data) of a DBN, and of a multimodal stack of DBNs (Salakhutdinov & Murray 2008, "On the
quantitative analysis of deep belief networks", section 4.2): the host estimator behind ``DBN.log_likelihood_bound`` and
``MDBN.log_likelihood_bound``.

With the recognition model q(x_l | x_{l-1}) = Bernoulli(sigmoid(x_{l-1} W_l + b_l)) of the layers below the top RBM L,

    B(x_0) = E_q[ sum_{l < L} ( log p(x_{l-1} | x_l) + H[q(. | x_{l-1})] ) - F_L(x_{L-1}) ] - log Z_L   <=   log p(x_0)

The expectation is a mean over ``n_samples`` sampled configurations per data row (replica row n S + s belongs to data row n);
the entropies are analytic.  An input layer with ``visible_groups`` (K-ary softmax units) changes one term: its log p(x_0 | x_1)
is a log-softmax per group (``HipEngine.propdown_row_loglik_grouped``); q, the entropies and the layers above are those of
the Bernoulli layer, and a single such RBM takes log Z from its grouped AIS run.  The device forms every per-replica term
(``HipEngine.sample_replicas``, ``HipEngine.propdown_row_loglik``, ``free_energy``); sums over layers, means over replicas and everything after them are float64
numpy on the host, the rule of the AIS estimators."""
import collections

import numpy

from .engine import RngAddr
from .shared import HostTable, shared

# bound: mean of ``rows``; stderr: sampling error of that mean, sqrt(sum row_var / S) / N (the error of log_z is NOT in it);
# log_z / log_z_stderr: of the top RBM (stderr 0.0 for a given log_z); rows [N] float64: the bound of every data row;
# row_stderr [N]; trace: None, or what the run sampled (see ``stack_bound``)
Bound = collections.namedtuple("Bound", "bound stderr log_z log_z_stderr rows row_stderr trace")
# ... of a multimodal stack: modality_rows [M, N] the directed + entropy terms of each modality's layers, joint_rows [N] those
# of the joint network with -F_L - log Z_L; rows = modality_rows.sum(0) + joint_rows
StackBound = collections.namedtuple("StackBound", Bound._fields + ("modality_rows", "joint_rows"))


def bound_chunks(n_rows, n_samples, chunk_rows):
    """[(lo, hi), ...]: the data rows of every chunk, so that rows x n_samples <= chunk_rows (at least one row)."""
    n_rows, n_samples, chunk_rows = int(n_rows), int(n_samples), int(chunk_rows)
    if n_samples < 1:
        raise ValueError("n_samples must be >= 1, got %r" % (n_samples,))
    if chunk_rows < 1:
        raise ValueError("chunk_rows must be >= 1, got %r" % (chunk_rows,))
    per = max(1, chunk_rows // n_samples)
    return [(lo, min(n_rows, lo + per)) for lo in range(0, n_rows, per)]


def _rows(data, lo, hi):
    if isinstance(data, HostTable) and data._mirror is None:
        return data.rows(slice(lo, hi))             # streamed: the table is never uploaded whole (DBN._forward)
    return data.tensor[lo:hi]


def _host64(t):
    return t.detach().cpu().numpy().astype(numpy.float64)


def _climb(net, x, n_sampled, div, row_offset, steps, keep, data_layer=True):
    """Sample ``x`` up through ``rbm_layers[:n_sampled]`` of ``net``: ``div`` replicas of every row at the first of them (1: the
    rows are replica rows already), one sample per replica row above.  Returns the top samples and the per-replica sum of
    log p(x_{l-1} | x_l) + H[q(. | x_{l-1})] over these layers (float64 numpy); ``keep`` (a dict of lists, or None) receives
    the samples and terms.  ``data_layer``: ``x`` is data, so a first layer with ``visible_groups`` scores it with a log-softmax
    per group (``propdown_row_loglik_grouped``); the joint network's input is sampled units and keeps the sigmoid term."""
    eng = net.engine
    total = None
    for l in range(n_sampled):
        r = net.rbm_layers[l]
        mean = eng.propup(x, r.W.tensor, r.hbias.tensor, want_pre=False, want_sample=False)[1]
        sample, entropy = eng.sample_replicas(mean, div, RngAddr(r.theano_rng.seed, r.stream_id, steps[id(r)], 0, row_offset))
        # (the directed term is the generative model's: the generative weights of a layer untied by fine-tuning)
        if l == 0 and data_layer and r.visible_groups is not None:
            directed = eng.propdown_row_loglik_grouped(sample, r.down_W, r.vbias.tensor, x, r.visible_groups, target_div=div)
        else:
            directed = eng.propdown_row_loglik(sample, r.down_W, r.vbias.tensor, x, r.gauss, target_div=div)
        directed = _host64(directed)
        entropy = _host64(entropy)
        term = directed + numpy.repeat(entropy, div)
        total = term if total is None else total + term
        if keep is not None:
            keep["samples"][l].append(eng.to_numpy(sample))
            keep["directed"][l].append(directed)
            keep["entropy"][l].append(entropy)
        x, div = sample, 1
    return x, total


def stack_bound(bottoms, joint, n_samples=64, log_z=None, chunk_rows=16384, trace=False, **ais):
    """The bound for ``bottoms`` = [(DBN, data), ...] under the joint DBN ``joint``, or for the one DBN of ``bottoms`` alone
    (``joint`` None).  Under a joint network every layer of a bottom network is sampled and contributes a directed term, the
    sampled tops are concatenated in the order of ``bottoms`` and the joint network continues; the last RBM of the joint
    network (of the DBN itself without one) is the undirected top.  ``trace``: the record's ``trace`` is a dict with ``nets`` (per
    network, bottoms first: ``samples`` / ``directed`` / ``entropy``, one array per sampled layer), ``free_energy`` [N S] and
    ``values`` [N, S] (the per-replica sums)."""
    import torch
    S = int(n_samples)
    if S < 1:
        raise ValueError("n_samples must be >= 1, got %r" % (n_samples,))
    if not bottoms or (joint is None and len(bottoms) != 1):
        raise ValueError("one DBN, or modality DBNs under a joint DBN")
    nets = [net for net, _ in bottoms]
    for net in nets:
        net.rbm_layers[0]._no_sigma("log_likelihood_bound")
        # (a single RBM with groups has no directed term: its log_partition refuses where the engine lacks the grouped AIS)
        if (joint is not None or net.n_layers > 1) and not hasattr(net.engine, "propdown_row_loglik_grouped"):
            net.rbm_layers[0]._no_groups("log_likelihood_bound on this engine")
    datas =[shared(d, engine=net.engine) for net, d in bottoms]
    N = len(datas[0])
    if N < 1:
        raise ValueError("no data rows")
    if any(len(d) != N for d in datas):
        raise ValueError("all modalities need the same number of rows")
    for net, d in zip(nets, datas):
        if d.shape[1] != net.n_ins:
            raise ValueError("data has %d columns, the network %d inputs" % (d.shape[1], net.n_ins))
    for net, d in zip(nets, datas):
        if net.rbm_layers[0].visible_groups is not None:
            # categorical input units: the directed term is linear in the data row, which must be one-hot in every group
            # (checked on the host copy; a HostTable through its host rows, without an upload)
            net.rbm_layers[0]._check_one_hot(d)
    top_net = joint if joint is not None else nets[0]
    top = top_net.rbm_layers[-1]
    eng = top_net.engine
    n_up = [net.n_layers if joint is not None else net.n_layers - 1 for net in nets]
    n_joint = joint.n_layers - 1 if joint is not None else 0
    if joint is not None and joint.n_ins != sum(net.stacked_layers_sizes[-1] for net in nets):
        raise ValueError("the joint network has %d inputs, the modalities' tops %d units"
                         % (joint.n_ins, sum(net.stacked_layers_sizes[-1] for net in nets)))
    sampled = [r for net, n in zip(nets, n_up) for r in net.rbm_layers[:n]] + (joint.rbm_layers[:n_joint] if joint is not None else [])
    if not sampled:
        S = 1                                       # a single RBM: B = -F - log Z exactly, no sample is drawn
    chunks = bound_chunks(N, S, chunk_rows)

    if log_z is None:
        if "base_vbias" not in ais and "data" not in ais:
            # the base rate of the top layer's AIS run: the data seen through the layers below it (DBN.layer_log_likelihood)
            if joint is None:
                below = datas[0].get_value() if top_net.n_layers == 1 else top_net.get_output(datas[0], top_net.n_layers - 2)
            else:
                below = numpy.concatenate([net.get_output(d) for net, d in zip(nets, datas)], axis=1)
                if joint.n_layers > 1:
                    below = joint.get_output(below, joint.n_layers - 2)
            ais = dict(ais, data=below)
        log_z, log_z_err = top.log_partition(**ais)
    else:
        log_z, log_z_err = float(log_z), 0.0

    # every sampled layer draws from its own RBM's stream at its current step, whatever the chunking; the counters move once
    steps = {id(r): r._rng_step for r in sampled}
    keeps = None
    if trace:
        keeps = [dict(samples=[[] for _ in range(n)], directed=[[] for _ in range(n)], entropy=[[] for _ in range(n)])
                 for n in n_up + ([n_joint] if joint is not None else [])]
    rows, row_var = numpy.zeros(N), numpy.zeros(N)
    modality_rows, joint_rows = numpy.zeros((len(nets), N)), numpy.zeros(N)
    fe_all, values_all = [], []
    for lo, hi in chunks:
        offset, tops = lo * S, []
        value = numpy.zeros((hi - lo) * S)          # per replica: the sum of every term but log Z
        for m, (net, d) in enumerate(zip(nets, datas)):
            x, term = _climb(net, eng.as_matrix(_rows(d, lo, hi)), n_up[m], S, offset, steps, keeps[m] if trace else None)
            if term is not None:
                modality_rows[m, lo:hi] = term.reshape(hi - lo, S).mean(axis=1)
                value += term
            tops.append(x)
        if joint is not None:
            xj = eng.as_matrix(torch.cat(tops, dim=1))
            xj, jterm = _climb(joint, xj, n_joint, 1, offset, steps, keeps[-1] if trace else None, data_layer=False)
        else:
            xj, jterm = tops[0], None
        fe = _host64(eng.free_energy(xj, top.W.tensor, top.hbias.tensor, top.vbias.tensor, top.gauss))
        jvalue = -fe if jterm is None else jterm - fe
        value += jvalue
        joint_rows[lo:hi] = jvalue.reshape(hi - lo, S).mean(axis=1) - log_z
        value = value.reshape(hi - lo, S)
        rows[lo:hi] = value.mean(axis=1) - log_z
        if S > 1:
            row_var[lo:hi] = value.var(axis=1, ddof=1)
        if trace:
            fe_all.append(fe)
            values_all.append(value)
    for r in sampled:
        r._rng_step = steps[id(r)] + 1
    record = None
    if trace:
        record = dict(nets=[{k: [numpy.concatenate(c, axis=0) for c in v] for k, v in keep.items()} for keep in keeps],
                      free_energy=numpy.concatenate(fe_all), values=numpy.concatenate(values_all, axis=0))
    out = Bound(float(rows.mean()), float(numpy.sqrt(row_var.sum() / S) / N), float(log_z), float(log_z_err), rows,
                numpy.sqrt(row_var / S), record)
    if joint is None:
        return out
    return StackBound(*(out + (modality_rows, joint_rows)))
