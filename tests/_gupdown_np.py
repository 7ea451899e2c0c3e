"""float64 numpy twin of up-down fine-tuning for stacks whose INPUT layer holds softmax groups (mdbn_amd/updown.py,
csrc/mdbn_updown.hip: mdbn_updown_gen_step_grouped; TEST-ONLY, no GPU needed).

Layers and models are those of tests/_updown_np.py; the first layer of a bottom net may carry ``bounds``, the int boundaries
``[g_0, ..., g_G]`` of tests/_softmax_np.py.  One conditional changes, at such a layer:

    g_0 = p(x_0 | x_1) = softmax inside every group, sigmoid on the Bernoulli columns, of pre = x_1 G_0^T + c_0

so the dream's y_0 is one category per group (the first c with u < C_c, the uniform of the group's first column), the generative
rule keeps S = (x_0 - g_0)^T x_1 and s_v = sum_r (x_0 - g_0) with the grouped g_0, and its cost is
sum_r sum_g (m_g + log sum_c exp(pre_c - m_g) - sum_c x_c pre_c) plus the Bernoulli cross-entropy outside the span.  Wake, top,
the recognition rule and the update rule are _updown_np's, used by import.  ``GupdownOracle`` is the checker engine with the
calls ``updown.step`` makes on such a stack."""
import numpy as np
import torch

import _gbound_np as gb
import _softmax_np as sm
import _updown_np as ud
from _oracle_engine import OracleEngine
from oracle import philox_np, rbm_np
from oracle.philox_np import PhiloxDraws

f64 = ud.f64


# ------------------------------------------------------------------ the generative rule of a layer with groups
def predict(x_hi, G, c, bounds):
    """(pre, g): the linear pre-activations and the grouped means."""
    pre = f64(x_hi) @ G.T + c
    return pre, sm.grouped_softmax(pre, bounds)[0]


def cost(pre, x_lo, bounds):
    """sum_r -log p(x_lo | x_hi): per group m + log sum_c exp(pre_c - m) - sum_c x_c pre_c, per Bernoulli column the
    cross-entropy x softplus(-pre) + (1 - x) softplus(pre)."""
    pre, x = f64(pre), f64(x_lo)
    cols = sm.bernoulli_columns(bounds, pre.shape[1])
    total = (x[:, cols] * ud.softplus(-pre[:, cols]) + (1.0 - x[:, cols]) * ud.softplus(pre[:, cols])).sum()
    for lo, hi in sm.spans(bounds):
        p = pre[:, lo:hi]
        m = p.max(axis=1)
        total += (m + np.log(np.exp(p - m[:, None]).sum(axis=1)) - (x[:, lo:hi] * p).sum(axis=1)).sum()
    return float(total)


def delta_gen(x_lo, x_hi, G, c, bounds):
    """(S, s_v, cost) of the grouped generative rule."""
    x_lo, x_hi = f64(x_lo), f64(x_hi)
    pre, g = predict(x_hi, G, c, bounds)
    err = x_lo - g
    return err.T @ x_hi, err.sum(axis=0), cost(pre, x_lo, bounds)


def gen_step(l, x_lo, x_hi, hp, n_rows):
    """_updown_np.gen_step on layer ``l`` IN PLACE, grouped where the layer carries ``bounds``; returns the cost sum."""
    if l.get("bounds") is None:
        return ud.gen_step(l, x_lo, x_hi, hp, n_rows)
    S, s_v, c = delta_gen(x_lo, x_hi, l["G"], l["c"], l["bounds"])
    l["G"], l["Gs"] = ud.update(l["G"], l["Gs"], S, hp, hp["batch_size"], True)
    l["c"], l["cs"] = ud.update(l["c"], l["cs"], s_v, hp, n_rows, False)
    return c


# ------------------------------------------------------------------ one whole step
class Draws(ud.Draws):
    """_updown_np.Draws with the categorical dream of a grouped layer.  ``ties``: the draws the twin's own float64 means leave
    within _softmax_np's tie width; ``dreams``: every grouped sample taken."""

    def __init__(self, recorded=None, tie=1e-6):
        ud.Draws.__init__(self, recorded, tie)
        self.ties, self.dreams = 0, []

    def categorical(self, l, mean, what):
        u = philox_np.uniform(mean.shape[0], mean.shape[1], l["seed"], l["stream"], l["step"], 0).astype(np.float64)
        l["step"] += 1
        s = sm.grouped_sample(mean, l["bounds"], u)
        self.ties += sm.tie_draws(mean, l["bounds"], u)
        if self.recorded is not None:
            s, n = sm.follow(s, self.recorded.pop(0), mean, l["bounds"], u, what=what)
            self.flips += n
        self.taken.append(s)
        self.dreams.append(s)
        return s


def step(model, rows, hp, draws=None, forced_top=None):
    """_updown_np.step for a model whose bottom nets' first layers may carry ``bounds``: the same dict."""
    draws = draws if draws is not None else Draws()
    directed, top = ud.plan(model)
    joint = model.get("joint")
    n = len(rows[0])

    def wake(layers, x):
        xs = [f64(x)]
        for l in layers:
            xs.append(draws.bernoulli(l, ud.sigmoid(xs[-1] @ l["W"] + l["b"]), "wake"))
        return xs

    def sleep(layers, y_top):
        ys, rs = [f64(y_top)], []
        for l in reversed(layers):
            if l.get("bounds") is not None:
                y = draws.categorical(l, predict(ys[0], l["G"], l["c"], l["bounds"])[1], "dream")
            else:
                p = ud.predict(ys[0], l["G"], l["c"], l["gauss"])[1]
                y = draws.gaussian(l, p, "dream") if l["gauss"] else draws.bernoulli(l, p, "dream")
            rs.insert(0, ud.sigmoid(y @ l["W"] + l["b"]))
            ys.insert(0, y)
        return ys, rs

    n_bottom = len(model["bottoms"])
    xs = [wake(layers, x) for layers, x in zip(directed[:n_bottom], rows)]
    if joint is not None:
        xs.append(wake(directed[-1], np.concatenate([x[-1] for x in xs], axis=1)))
    (S, s_h, s_v, top_cost), y_top = ud.top_cd(top, xs[-1][-1], hp["k"], forced_top, draws.tie)
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
    top["W"], top["Ws"] = ud.update(top["W"], top["Ws"], S, thp, hp["batch_size"], True)
    top["b"], top["bs"] = ud.update(top["b"], top["bs"], s_h, thp, n, False)
    top["c"], top["cs"] = ud.update(top["c"], top["cs"], s_v, thp, n, False)
    gen_cost = 0.0
    for m, layers in enumerate(directed):
        for k, l in enumerate(layers):
            c = gen_step(l, xs[m][k], xs[m][k + 1], hp, n)
            if k == 0 and m < n_bottom:
                gen_cost += c / n
            ud.rec_step(l, ys[m][k], ys[m][k + 1], hp, n)
    return dict(x=xs, y=ys, r=rs, gen_cost=gen_cost, top_cost=top_cost / n)


# ------------------------------------------------------------------ exact likelihood of an enumerable stack
def one_hot_states(V, bounds):
    """Every state of a layer with groups: one 1 per group, all 0 / 1 patterns on the Bernoulli columns.  [states, V]."""
    cols = sm.bernoulli_columns(bounds, V)
    out = np.zeros((1, V))
    for c in cols:
        out = np.concatenate([out, out + np.eye(V)[c]], axis=0)
    for lo, hi in sm.spans(bounds):
        out = np.concatenate([out + np.eye(V)[c] for c in range(lo, hi)], axis=0)
    return out


def exact_log_p(net, x0):
    """_updown_np.exact_log_p for a net whose first layer carries ``bounds``: exact log p(x_0) [N] under the generative
    parameters, the states of the layers above enumerated."""
    top = net[-1]
    v = ud.bits(top["W"].shape[0])
    log_top = ud.softplus(v @ top["W"] + top["b"]).sum(axis=1) + v @ top["c"]
    states, log_prior = v, log_top - np.logaddexp.reduce(log_top)
    for l in reversed(net[1:-1]):
        lower = ud.bits(l["G"].shape[0])
        pre = states @ l["G"].T + l["c"]
        cond = lower @ pre.T - ud.softplus(pre).sum(axis=1)[None, :]
        log_prior = np.logaddexp.reduce(cond + log_prior[None, :], axis=1)
        states = lower
    l = net[0]
    layer = dict(W=l["G"], c=l["c"], gauss=False)
    x0 = f64(x0)
    out = np.empty(len(x0))
    for r in range(len(x0)):
        cond = gb.row_loglik_grouped(states, layer, np.repeat(x0[r:r + 1], len(states), axis=0), l["bounds"])
        out[r] = np.logaddexp.reduce(cond + log_prior)
    return out


# ------------------------------------------------------------------ checker engine
class GupdownOracle(gb.GboundOracle):
    """The checker engine of a layer with groups plus the calls of an up-down step, COMPOSED as the library composes them:
    stacked operands, the oracle's CD statistics, the unchanged update rule with a throw-away vector for the bias half that
    must not move; the grouped generative rule takes the grouped means of the twin in place of the sigmoid.  ``log``: the
    step-level calls; ``paths``: the path every generative call was given."""

    def __init__(self):
        gb.GboundOracle.__init__(self)
        self.log, self.paths = [], []

    def propup(self, v, W, hbias, rng=None, **kw):
        self.log.append(("propup", id(W), rng.step if rng is not None else None))
        return OracleEngine.propup(self, v, W, hbias, rng=rng, **kw)

    def propdown(self, h, W, vbias, **kw):
        self.log.append(("propdown", id(W), kw["rng"].step if kw.get("rng") is not None else None))
        return OracleEngine.propdown(self, h, W, vbias, **kw)

    def group_softmax(self, pre, groups, rng, v0=None):
        self.log.append(("group_softmax", rng.step if rng is not None else None))
        return gb.GboundOracle.group_softmax(self, pre, groups, rng, v0=v0)

    def cd_step(self, data, indexes, W, hbias, vbias, gauss, k, rng, **kw):
        self.log.append(("cd_step", id(W), rng.step, kw.pop("keep_f32", None)))
        stats, sc = OracleEngine.cd_step(self, data, indexes, W, hbias, vbias, gauss, k, rng, **kw)
        v0 = self.as_matrix(data).numpy()
        out = rbm_np.cd_chain(self._state(W, hbias, vbias, gauss), v0, PhiloxDraws(rng.seed, rng.stream_id, rng.step, rng.row_offset), k)[2]
        sc.vs = self._t(out[2])
        return stats, sc

    def apply_update(self, W, *a, **kw):
        self.log.append(("apply_update", id(W)))
        return OracleEngine.apply_update(self, W, *a, **kw)

    def _rule(self, W, W_speed, hb, hbs, vb, vbs, S, s_h, s_v, rule):
        lr, l1, l2, wc, mu, batch_size, n_rows = rule
        stats = self._t(np.concatenate([S.ravel(), s_h, s_v, np.zeros(4)]))
        OracleEngine.apply_update(self, W, W_speed, None, hb, hbs, vb, vbs, stats, lr, l1, l2, wc, mu, batch_size, n_rows, 1.0)

    def _gen(self, x_lo, x_hi, G, G_speed, vbias, vbias_speed, g, rule):
        S, s_h, s_v = rbm_np.cd_statistics(*ud.stacked_gen(x_lo, x_hi, g))
        junk = torch.zeros(G.shape[1], dtype=self.t_dtype)
        self._rule(G, G_speed, junk, junk.clone(), vbias, vbias_speed, S, s_h, s_v, rule)

    def updown_gen_step(self, x_lo, x_hi, G, G_speed, vbias, vbias_speed, gauss, lr, lambda_1, lambda_2, weightcost, momentum,
                        batch_size, n_rows, cost_scale=1.0, path="auto"):
        self.log.append(("gen", id(G)))
        self.paths.append(path)
        x_lo, x_hi = self.as_matrix(x_lo).numpy(), self.as_matrix(x_hi).numpy()
        pre, g = ud.predict(x_hi, G.numpy(), vbias.numpy(), gauss)
        self._gen(x_lo, x_hi, G, G_speed, vbias, vbias_speed, g, (lr, lambda_1, lambda_2, weightcost, momentum, batch_size, n_rows))
        c = 0.5 * ((x_lo - g) ** 2).sum() if gauss else (x_lo * ud.softplus(-pre) + (1 - x_lo) * ud.softplus(pre)).sum()
        return torch.tensor(c * cost_scale, dtype=self.t_dtype)

    def updown_gen_step_grouped(self, x_lo, x_hi, G, G_speed, vbias, vbias_speed, groups, lr, lambda_1, lambda_2, weightcost,
                                momentum, batch_size, n_rows, cost_scale=1.0, path="auto"):
        self.log.append(("gen_grouped", id(G)))
        self.paths.append(path)
        x_lo, x_hi = self.as_matrix(x_lo).numpy(), self.as_matrix(x_hi).numpy()
        pre, g = predict(x_hi, G.numpy(), vbias.numpy(), groups.host)
        self._gen(x_lo, x_hi, G, G_speed, vbias, vbias_speed, g, (lr, lambda_1, lambda_2, weightcost, momentum, batch_size, n_rows))
        return torch.tensor(cost(pre, x_lo, groups.host) * cost_scale, dtype=self.t_dtype)

    def updown_rec_step(self, y_lo, y_hi, r, W, W_speed, hbias, hbias_speed, lr, lambda_1, lambda_2, weightcost, momentum,
                        batch_size, n_rows, path="auto"):
        self.log.append(("rec", id(W)))
        y_lo, y_hi, r = (self.as_matrix(t).numpy() for t in (y_lo, y_hi, r))
        S, s_h, s_v = rbm_np.cd_statistics(*ud.stacked_rec(y_lo, y_hi, r))
        junk = torch.zeros(W.shape[0], dtype=self.t_dtype)
        self._rule(W, W_speed, hbias, hbias_speed, junk, junk.clone(), S, s_h, s_v,
                   (lr, lambda_1, lambda_2, weightcost, momentum, batch_size, n_rows))


class NoGroupedRule(GupdownOracle):
    """... without the grouped generative rule: what ``fine_tune`` must refuse.  ``updown_gen_step_grouped`` is not an attribute."""

    def __getattribute__(self, name):
        if name == "updown_gen_step_grouped":
            raise AttributeError(name)
        return GupdownOracle.__getattribute__(self, name)


# ------------------------------------------------------------------ the stacks of the tests
def twin_net(dbn):
    """The twin's layers from a DBN on the checker engine (float64 tensors read directly), the table of its input layer kept."""
    net = []
    for r in dbn.rbm_layers:
        t = lambda a: None if a is None else a.tensor.numpy().copy()
        l = ud.untie(dict(W=t(r.W), b=t(r.hbias), c=t(r.vbias), G=t(r.W_gen), Ws=t(r.W_speed), bs=t(r.hbias_speed),
                          cs=t(r.vbias_speed), Gs=t(r.W_gen_speed), gauss=r.gauss, noisy=bool(r.gauss and not r.error_free),
                          seed=r.theano_rng.seed, stream=r.stream_id, step=r._rng_step))
        if r.visible_groups is not None:
            l["bounds"] = [int(b) for b in r.visible_groups.host]
        net.append(l)
    return net
