"""float64 numpy twin of up-down fine-tuning (mdbn_amd/updown.py, csrc/mdbn_updown.hip; TEST-ONLY, no GPU needed).

A layer is a dict: ``W`` [V, H] recognition weights, ``b`` [H] hidden bias, ``c`` [V] visible (generative) bias, ``G`` [V, H]
generative weights (a directed layer; made from W by ``untie``), the speeds ``Ws`` / ``bs`` / ``cs`` / ``Gs``, ``gauss``, ``noisy`` (a
Gaussian layer that adds N(0, 1) to its dream) and ``seed`` / ``stream`` / ``step`` of its Philox stream.  A MODEL is
``dict(bottoms=[net, ...], joint=net | None)`` as in ``_dbn_bound_np``: without a joint net the one bottom net's last layer is the
undirected top, under a joint net every bottom layer is directed and the joint net's last layer is the top.

``delta_gen`` / ``delta_rec`` are the two delta rules' statistics; ``stacked_gen`` / ``stacked_rec`` the operands that make the
statistics of a CD step (oracle ``cd_statistics``) reproduce them; ``update`` the engine's update rule (rbm.py:347-365);
``step`` one whole up-down step, on its own Philox draws or teacher-forced along recorded samples; ``exact_log_p`` the exact
log p(x_0) of an enumerable stack under its GENERATIVE parameters."""
import numpy as np

from oracle import philox_np, rbm_np

EPS = rbm_np.EPSILON


def sigmoid(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def f64(a):
    return np.array(a, dtype=np.float64)


def untie(layer):
    """float64 copies of a layer's arrays, with generative weights and zero speeds where they are missing."""
    l = dict(layer)
    for k in ("W", "b", "c"):
        l[k] = f64(layer[k])
    l["G"] = f64(layer["G"]) if layer.get("G") is not None else l["W"].copy()
    for k, like in (("Ws", "W"), ("Gs", "W"), ("bs", "b"), ("cs", "c")):
        l[k] = f64(layer[k]) if layer.get(k) is not None else np.zeros_like(l[like])
    l.setdefault("noisy", False)
    return l


# ------------------------------------------------------------------ the delta rules
def predict(x_hi, G, c, gauss):
    """(pre, g): the generative prediction of the layer below from the state above."""
    pre = f64(x_hi) @ G.T + c
    return pre, (pre if gauss else sigmoid(pre))


def delta_gen(x_lo, x_hi, G, c, gauss):
    """(S, s_v, cost): S = (x_lo - g)^T x_hi, s_v = sum_r (x_lo - g), cost = sum_r -log p(x_lo | x_hi) (Gaussian: without the
    constant V / 2 log 2 pi)."""
    x_lo, x_hi = f64(x_lo), f64(x_hi)
    pre, g = predict(x_hi, G, c, gauss)
    err = x_lo - g
    cost = 0.5 * (err ** 2).sum() if gauss else (x_lo * softplus(-pre) + (1.0 - x_lo) * softplus(pre)).sum()
    return err.T @ x_hi, err.sum(axis=0), float(cost)


def delta_rec(y_lo, y_hi, W, b):
    """(S, s_h, r): S = y_lo^T (y_hi - r), s_h = sum_r (y_hi - r), r = sigmoid(y_lo W + b)."""
    y_lo, y_hi = f64(y_lo), f64(y_hi)
    r = sigmoid(y_lo @ W + b)
    return y_lo.T @ (y_hi - r), (y_hi - r).sum(axis=0), r


def stacked_gen(x_lo, x_hi, g):
    """(v0, ph, nv, nh) whose CD statistics are the generative rule's: V2 = [x_lo; g], P2 = [x_hi; -x_hi]."""
    return f64(x_lo), f64(x_hi), f64(g), f64(x_hi)


def stacked_rec(y_lo, y_hi, r):
    """... the recognition rule's: V2 = [y_lo; y_lo], P2 = [y_hi; -r]."""
    return f64(y_lo), f64(y_hi), f64(y_lo), f64(r)


def update(theta, speed, S, hp, divisor, weights):
    """The update rule (rbm.py:347-365) on one array: (new theta, new speed).  ``weights``: the lambda shrink and the weight
    cost apply (on the live matrix); biases have multiplier 1."""
    g = S / divisor
    m = 1.0
    if weights:
        g = g - hp["weightcost"] * theta
        shrink = 1.0 + 2.0 * hp["lr"] * hp["lambda_1"] / (np.abs(theta) + EPS)
        g = g / shrink
        m = (1.0 - 2.0 * hp["lr"] * hp["lambda_2"]) / shrink
    return theta * m + speed * hp["lr"], g + (speed - g) * hp["momentum"]


def gen_step(l, x_lo, x_hi, hp, n_rows):
    """The generative half on layer ``l`` IN PLACE; returns the cost sum."""
    S, s_v, cost = delta_gen(x_lo, x_hi, l["G"], l["c"], l["gauss"])
    l["G"], l["Gs"] = update(l["G"], l["Gs"], S, hp, hp["batch_size"], True)
    l["c"], l["cs"] = update(l["c"], l["cs"], s_v, hp, n_rows, False)
    return cost


def rec_step(l, y_lo, y_hi, hp, n_rows, r=None):
    S, s_h, own = delta_rec(y_lo, y_hi, l["W"], l["b"])
    if r is not None:                                 # the statistics from a GIVEN r (kernel tests feed the device's own)
        S, s_h = f64(y_lo).T @ (f64(y_hi) - f64(r)), (f64(y_hi) - f64(r)).sum(axis=0)
    l["W"], l["Ws"] = update(l["W"], l["Ws"], S, hp, hp["batch_size"], True)
    l["b"], l["bs"] = update(l["b"], l["bs"], s_h, hp, n_rows, False)
    return own


# ------------------------------------------------------------------ one whole step
class Draws(object):
    """The samples of a step: the layers' own Philox draws (u < mean), or with ``recorded`` = the device's samples in call order
    teacher-forced along them (checked against the own draw away from ties)."""

    def __init__(self, recorded=None, tie=1e-6):
        self.recorded = list(recorded) if recorded is not None else None
        self.tie, self.flips, self.taken = tie, 0, []

    def bernoulli(self, l, mean, what):
        u = philox_np.uniform(mean.shape[0], mean.shape[1], l["seed"], l["stream"], l["step"], 0).astype(np.float64)
        l["step"] += 1
        s = (u < mean).astype(np.float64)
        if self.recorded is not None:
            s, n = rbm_np._follow(s, self.recorded.pop(0), u, mean, self.tie, what)
            self.flips += n
        self.taken.append(s)
        return s

    def gaussian(self, l, mean, what):
        step = l["step"]
        l["step"] += 1                                # (a noise-free Gaussian layer takes its step as well: GRBM.sample_v_given_h)
        if self.recorded is not None:
            y = f64(self.recorded.pop(0))
        elif l.get("noisy"):
            y = mean + philox_np.normal(mean.shape[0], mean.shape[1], l["seed"], l["stream"], step, 0).astype(np.float64)
        else:
            y = mean
        self.taken.append(y)
        return y


def plan(model):
    bottoms, joint = model["bottoms"], model.get("joint")
    if joint is None:
        assert len(bottoms) == 1 and len(bottoms[0]) >= 2
        return [bottoms[0][:-1]], bottoms[0][-1]
    return [list(net) for net in bottoms] + [joint[:-1]], joint[-1]


def top_cd(top, v0, k, forced=None, tie=1e-6):
    """The top RBM's CD-k statistics on ``v0`` and the visible sample of its last Gibbs step.  ``forced``: (trace_h, trace_v) of the
    device's chain."""
    s = rbm_np.RBMState(top["W"].shape[0], top["W"].shape[1], W=top["W"], hbias=top["b"], vbias=top["c"], dtype=np.float64,
                        gauss=False)
    draws = philox_np.PhiloxDraws(top["seed"], top["stream"], top["step"], 0)
    top["step"] += 1
    if forced is None:
        ph_mean, _, out = rbm_np.cd_chain(s, v0, draws, k)
    else:
        ph_mean, _, out, _ = rbm_np.cd_chain_forced(s, v0, draws, k, forced[0], forced[1], tie=tie)
    pre_nv, nv_mean, nv_sample, _, nh_mean, _ = out
    S, s_h, s_v = rbm_np.cd_statistics(v0, ph_mean, nv_mean, nh_mean)
    cost = float((v0 * softplus(-pre_nv) + (1.0 - v0) * softplus(pre_nv)).sum())
    return (S, s_h, s_v, cost), nv_sample


def step(model, rows, hp, draws=None, forced_top=None):
    """One up-down step IN PLACE on ``model`` (layers as ``untie`` returns them).  ``hp``: lr, top_lr, k, momentum, weightcost,
    lambda_1, lambda_2, batch_size.  Returns a dict: ``x`` / ``y`` / ``r`` per network, ``gen_cost`` (per row, summed over the
    bottoms) and ``top_cost`` (per row)."""
    draws = draws if draws is not None else Draws()
    directed, top = plan(model)
    joint = model.get("joint")
    n = len(rows[0])

    def wake(layers, x):
        xs = [f64(x)]
        for l in layers:
            xs.append(draws.bernoulli(l, sigmoid(xs[-1] @ l["W"] + l["b"]), "wake"))
        return xs

    def sleep(layers, y_top):
        ys, rs = [f64(y_top)], []
        for l in reversed(layers):
            pre, p = predict(ys[0], l["G"], l["c"], l["gauss"])
            y = draws.gaussian(l, p, "dream") if l["gauss"] else draws.bernoulli(l, p, "dream")
            rs.insert(0, sigmoid(y @ l["W"] + l["b"]))
            ys.insert(0, y)
        return ys, rs

    n_bottom = len(model["bottoms"])
    xs = [wake(layers, x) for layers, x in zip(directed[:n_bottom], rows)]
    if joint is not None:
        xs.append(wake(directed[-1], np.concatenate([x[-1] for x in xs], axis=1)))
    (S, s_h, s_v, cost), y_top = top_cd(top, xs[-1][-1], hp["k"], forced_top, draws.tie)
    ys, rs = [None] * len(directed), [None] * len(directed)
    if joint is not None:
        ys[-1], rs[-1] = sleep(directed[-1], y_top)
        lo = 0
        for m, net in enumerate(model["bottoms"]):
            w = net[-1]["W"].shape[1]
            ys[m], rs[m] = sleep(directed[m], ys[-1][0][:, lo:lo + w])
            lo += w
    else:
        ys[0], rs[0] = sleep(directed[0], y_top)
    thp = dict(hp, lr=hp["top_lr"])
    top["W"], top["Ws"] = update(top["W"], top["Ws"], S, thp, hp["batch_size"], True)
    top["b"], top["bs"] = update(top["b"], top["bs"], s_h, thp, n, False)
    top["c"], top["cs"] = update(top["c"], top["cs"], s_v, thp, n, False)
    gen_cost = 0.0
    for m, layers in enumerate(directed):
        for k, l in enumerate(layers):
            c = gen_step(l, xs[m][k], xs[m][k + 1], hp, n)
            if k == 0 and m < n_bottom:
                gen_cost += c / n
            rec_step(l, ys[m][k], ys[m][k + 1], hp, n)
    return dict(x=xs, y=ys, r=rs, gen_cost=gen_cost, top_cost=cost / n)


# ------------------------------------------------------------------ exact likelihood of an enumerable stack
def bits(n):
    return ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.float64)


def exact_log_p(net, x0):
    """Exact log p(x_0) [N] of a single Bernoulli DBN (a list of layers, the last one the top RBM) under its generative
    parameters G / c and the top RBM, by enumeration."""
    top = net[-1]
    v = bits(top["W"].shape[0])
    log_top = softplus(v @ top["W"] + top["b"]).sum(axis=1) + v @ top["c"]
    log_top = log_top - np.logaddexp.reduce(log_top)          # log p(x_{L-1}) of every configuration
    states, log_prior = v, log_top
    for l in reversed(net[:-1]):                               # marginal of the layer below every directed layer
        assert not l["gauss"]
        lower = bits(l["G"].shape[0])
        pre = states @ l["G"].T + l["c"]                       # [configs above, V]
        cond = lower @ pre.T - softplus(pre).sum(axis=1)[None, :]      # log p(lower | above)
        log_prior = np.logaddexp.reduce(cond + log_prior[None, :], axis=1)
        states = lower
    x0 = f64(x0)
    index = (x0 @ (1 << np.arange(x0.shape[1]))).astype(int)
    return log_prior[index]
