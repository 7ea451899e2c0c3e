"""float64 numpy twin of the variational lower bound for stacks whose INPUT layer holds softmax groups (mdbn_amd/bound.py,
csrc/mdbn_bound.hip: mdbn_propdown_rowll_grouped; TEST-ONLY, no GPU needed).

Models are those of tests/_dbn_bound_np.py; the first layer of a bottom net may carry ``bounds``, the int boundaries
``[g_0, ..., g_G]`` of tests/_softmax_np.py (group g is columns g_g .. g_{g+1} - 1, columns outside [g_0, g_G) are Bernoulli
units).  Only the directed term of such a layer differs from the Bernoulli stack's:

    log p(x_0 | x_1) = sum_g ( sum_{c in g} t_c pre_c - logsumexp_{c in g} pre_c ) + sum_{Bernoulli i} ( t_i pre_i - softplus(pre_i) )

q(x_1 | x_0), its entropy, the layers above and the top RBM are unchanged.  ``estimate`` / ``brute_force`` follow the functions
of the same names in _dbn_bound_np.py with that one term replaced; ``GboundOracle`` is the checker engine with the calls
``bound.stack_bound`` makes."""
import numpy as np
import torch

import _dbn_bound_np as T
import _gais_np as G
import _softmax_np as sm
from oracle import philox_np


def row_loglik_grouped(h, layer, target, bounds):
    """log p(target | h) of every row of a layer with groups: per group sum_c t_c (pre_c - m) - log sum_c exp(pre_c - m) with
    m the group's largest pre-activation, per Bernoulli column t pre - softplus(pre)."""
    pre = np.asarray(h, dtype=np.float64) @ np.asarray(layer["W"], dtype=np.float64).T + np.asarray(layer["c"], dtype=np.float64)
    t = np.asarray(target, dtype=np.float64)
    cols = sm.bernoulli_columns(bounds, pre.shape[1])
    out = (t[:, cols] * pre[:, cols] - T.softplus(pre[:, cols])).sum(axis=1)
    for lo, hi in sm.spans(bounds):
        x = pre[:, lo:hi]
        m = x.max(axis=1, keepdims=True)
        out = out + (t[:, lo:hi] * (x - m)).sum(axis=1) - np.log(np.exp(x - m).sum(axis=1))
    return out


def row_loglik(h, layer, target):
    if layer.get("bounds") is not None:
        assert not layer["gauss"]
        return row_loglik_grouped(h, layer, target, layer["bounds"])
    return T.row_loglik(h, layer, target)


def estimate(model, inputs, S, log_z, samples=None):
    """_dbn_bound_np.estimate with the directed term of a grouped input layer: same arguments, same dict."""
    ups, joint, top = T.plan(model)
    N = len(inputs[0])
    if not any(ups) and not joint:
        S = 1
    out = dict(samples=[], means=[], uniforms=[])

    def climb(layers, x, div, given):
        total, got, means, unis = np.zeros(len(x) * div), [], [], []
        for k, l in enumerate(layers):
            x = np.asarray(x, dtype=np.float64)
            mean = T.sigmoid(x @ l["W"] + l["b"])
            rep = np.repeat(mean, div, axis=0)
            if given is None:
                u = philox_np.uniform(len(rep), rep.shape[1], l["seed"], l["stream"], l["step"], 0).astype(np.float64)
                s = (u < rep).astype(np.float64)
                unis.append(u)
            else:
                s = np.asarray(given[k], dtype=np.float64)
            total = total + row_loglik(s, l, np.repeat(x, div, axis=0)) + np.repeat(T.entropy(mean), div)
            got.append(s)
            means.append(rep)
            x, div = s, 1
        if not layers:
            x = np.repeat(np.asarray(x, dtype=np.float64), div, axis=0)
        out["samples"].append(got); out["means"].append(means); out["uniforms"].append(unis)
        return x, total

    tops, value, modality_rows = [], np.zeros(N * S), []
    for m, (layers, x0) in enumerate(zip(ups, inputs)):
        x, term = climb(layers, x0, S, None if samples is None else samples[m])
        tops.append(x)
        value = value + term
        modality_rows.append(term.reshape(N, S).mean(axis=1))
    if model.get("joint") is not None:
        x, jterm = climb(joint, np.concatenate(tops, axis=1), 1, None if samples is None else samples[len(ups)])
    else:
        x, jterm = tops[0], 0.0
    jvalue = jterm - T.free_energy(x, top)
    value = (value + jvalue).reshape(N, S)
    var = value.var(axis=1, ddof=1) if S > 1 else np.zeros(N)
    out.update(rows=value.mean(axis=1) - log_z, row_stderr=np.sqrt(var / S), values=value,
               modality_rows=np.asarray(modality_rows), joint_rows=jvalue.reshape(N, S).mean(axis=1) - log_z)
    out.update(bound=float(out["rows"].mean()), stderr=float(np.sqrt(var.sum() / S) / N))
    return out


def brute_force(model, inputs):
    """(exact log p(x_0) [N], exact bound [N], exact log Z of the top layer): every configuration of every sampled layer is
    enumerated -- log p(x_0) = log sum_config p(x_0 | x_1) ... p_top(x_{L-1}) with the grouped p(x_0 | x_1) -- as
    _dbn_bound_np.brute_force."""
    ups, joint, top = T.plan(model)
    log_z = T.exact_log_z(top)
    sizes = [l["W"].shape[1] for layers in ups for l in layers] + [l["W"].shape[1] for l in joint]
    conf = T.bits(sum(sizes))
    C = len(conf)
    N = len(inputs[0])
    log_p, bound = np.zeros(N), np.zeros(N)
    for n in range(N):
        at, log_q, log_j, tops = 0, np.zeros(C), np.zeros(C), []

        def walk(layers, x, at, log_q, log_j):
            for l in layers:
                H = l["W"].shape[1]
                s = conf[:, at:at + H]
                at += H
                pre = x @ l["W"] + l["b"]
                log_q = log_q + (s * pre - T.softplus(pre)).sum(axis=1)
                log_j = log_j + row_loglik(s, l, x)
                x = s
            return x, at, log_q, log_j

        for layers, x0 in zip(ups, inputs):
            x = np.repeat(np.asarray(x0[n:n + 1], dtype=np.float64), C, axis=0)
            x, at, log_q, log_j = walk(layers, x, at, log_q, log_j)
            tops.append(x)
        x = np.concatenate(tops, axis=1) if model.get("joint") is not None else tops[0]
        x, at, log_q, log_j = walk(joint, x, at, log_q, log_j)
        log_j = log_j - T.free_energy(x, top) - log_z
        log_p[n] = np.logaddexp.reduce(log_j) if C > 1 else log_j[0]
        bound[n] = (np.exp(log_q) * (log_j - log_q)).sum()
    return log_p, bound, log_z


# ------------------------------------------------------------------ the stacks of the tests
def make_net(rs, sizes, scale, seed, bounds=None, gauss=False, first_stream=0):
    """_dbn_bound_np.make_net; ``bounds``: the table of the first layer."""
    net = T.make_net(rs, sizes, gauss, scale, seed, first_stream)
    if bounds is not None:
        net[0]["bounds"] = [int(b) for b in bounds]
    return net


def stacks(scale):
    """{name: (model, inputs)}: 10 -> 6 -> 4 with groups (3, 3, 2) and two Bernoulli columns; 9 -> 5 -> 4 -> 3 with K = 3; a
    forest of a grouped 9 -> 3 modality and a Gaussian 4 -> 2 modality under a joint 5 -> 4 -> 3."""
    out = {}
    for name, sizes, bounds, seed in (("mixed_10_6_4", (10, 6, 4), [0, 3, 6, 8], 31), ("k3_9_5_4_3", (9, 5, 4, 3), [0, 3, 6, 9], 32)):
        rs = np.random.RandomState(seed + int(10 * scale))
        net = make_net(rs, sizes, scale, 3000 + seed, bounds)
        out[name] = (dict(bottoms=[net], joint=None), [sm.one_hot_data(rs, 6, sizes[0], bounds, p=0.5)])
    rs = np.random.RandomState(33 + int(10 * scale))
    a = make_net(rs, (9, 3), scale, 4001, [0, 3, 6, 9])
    b = make_net(rs, (4, 2), scale, 4002, gauss=True)
    out["forest"] = (dict(bottoms=[a, b], joint=make_net(rs, (5, 4, 3), scale, 4003)),
                     [sm.one_hot_data(rs, 6, 9, [0, 3, 6, 9]), T.make_data(rs, 6, 4, True)])
    return out


# ------------------------------------------------------------------ the kernel cases (tests/test_gpu_gbound.py)
# (V, H, R, target_div, boundaries): see the table in the GPU test
KERNEL_CASES = [
    (7, 5, 5, 1, [1, 4, 7]),
    (70, 40, 15, 3, [1, 3, 67, 70]),
    (300, 200, 70, 7, [2, 66, 130, 194, 258, 300]),
    (500, 24, 129, 64, list(range(0, 501, 5))),
    (794, 24, 33, 1, [784, 794]),
    (260, 33, 130, 2, [100, 103, 167, 170]),
]


def kernel_case(V, H, R, div, bounds, seed=0):
    """(h, W, vbias, target) float32 of a kernel case: 0 / 1 samples, W ~ N(0, 1) / sqrt(H), vbias ~ N(0, 0.5), one-hot targets."""
    rs = np.random.RandomState(seed + V + 7 * H + 13 * R)
    h = (rs.uniform(size=(R, H)) < 0.5).astype(np.float32)
    W = (rs.normal(0, 1, (V, H)) / np.sqrt(H)).astype(np.float32)
    vb = rs.normal(0, 0.5, V).astype(np.float32)
    target = sm.one_hot_data(rs, (R + div - 1) // div, V, bounds, p=0.5)
    return h, W, vb, target


def kernel_reference(h, W, vb, target, div, bounds):
    layer = dict(W=W.astype(np.float64), c=vb.astype(np.float64), gauss=False)
    return row_loglik_grouped(h, layer, np.repeat(target.astype(np.float64), div, axis=0)[:len(h)], bounds)


# ------------------------------------------------------------------ checker engine
class GboundOracle(G.GaisOracle):
    """The checker engine of a layer with groups (sm.GroupedOracle, with the grouped AIS of _gais_np.py for a one-layer
    network) plus the three calls of the bound: ``sample_replicas``, ``propdown_row_loglik`` and
    ``propdown_row_loglik_grouped``, from the twin.  ``calls`` logs their names."""

    def __init__(self):
        G.GaisOracle.__init__(self)
        self.calls = []

    def sample_replicas(self, mean, n_samples, rng):
        self.calls.append("sample_replicas")
        m = self.as_matrix(mean).numpy()
        rep = np.repeat(m, int(n_samples), axis=0)
        u = self._u(rng, rep.shape[0], rep.shape[1]).astype(np.float64)
        return self._t((u < rep).astype(np.float64)), self._t(T.entropy(m))

    def _layer(self, W, vbias, gauss):
        return dict(W=W.numpy().astype(np.float64), c=vbias.numpy().astype(np.float64), gauss=bool(gauss))

    def propdown_row_loglik(self, h, W, vbias, target, gauss, target_div=1):
        self.calls.append("propdown_row_loglik")
        h, t = self.as_matrix(h).numpy(), self.as_matrix(target).numpy()
        return self._t(T.row_loglik(h, self._layer(W, vbias, gauss), np.repeat(t, int(target_div), axis=0)[:len(h)]))

    def propdown_row_loglik_grouped(self, h, W, vbias, target, groups, target_div=1):
        self.calls.append("propdown_row_loglik_grouped")
        h, t = self.as_matrix(h).numpy(), self.as_matrix(target).numpy()
        return self._t(row_loglik_grouped(h, self._layer(W, vbias, False), np.repeat(t, int(target_div), axis=0)[:len(h)], groups.host))
