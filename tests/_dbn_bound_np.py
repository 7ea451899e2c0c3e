"""float64 numpy twin of the variational lower bound of a DBN / a multimodal stack (mdbn_amd/bound.py, csrc/mdbn_bound.hip;
TEST-ONLY, no GPU needed).

A MODEL is ``dict(bottoms=[net, ...], joint=net | None)``; a net is a list of layers ``dict(W [V, H], b [H] hidden bias,
c [V] visible bias, gauss)``, each with ``seed`` / ``stream`` / ``step`` of its Philox stream where it is sampled.  Without a joint
net the one bottom net is the whole DBN: its layers but the last are sampled and the last is the undirected top; under a joint
net every layer of a bottom net is sampled, the tops are concatenated, and the joint net's last layer is the top.

``estimate`` is the estimator on the device's own uniforms (oracle/philox_np.py; or along given samples: teacher-forced);
``brute_force`` enumerates every hidden configuration: the exact log p(x_0) and the exact bound of each row."""
import numpy as np

from oracle import philox_np


def sigmoid(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def f64(layer):
    return dict(layer, W=np.asarray(layer["W"], dtype=np.float64), b=np.asarray(layer["b"], dtype=np.float64),
                c=np.asarray(layer["c"], dtype=np.float64))


def row_loglik(h, layer, target):
    """log p(target | h) of every row: sum_i t_i pre_i - softplus(pre_i) | -1/2 sum_i (t_i - pre_i)^2 - V / 2 log 2 pi."""
    pre = np.asarray(h, dtype=np.float64) @ layer["W"].T + layer["c"]
    t = np.asarray(target, dtype=np.float64)
    if layer["gauss"]:
        return -0.5 * ((t - pre) ** 2).sum(axis=1) - 0.5 * pre.shape[1] * np.log(2.0 * np.pi)
    return (t * pre - softplus(pre)).sum(axis=1)


def entropy(mean):
    m = np.asarray(mean, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(m > 0, m * np.log(m), 0.0) + np.where(m < 1, (1.0 - m) * np.log1p(-m), 0.0)
    return -t.sum(axis=1)


def free_energy(x, layer):
    x = np.asarray(x, dtype=np.float64)
    hidden = softplus(x @ layer["W"] + layer["b"]).sum(axis=1)
    if layer["gauss"]:
        return -hidden + 0.5 * ((x - layer["c"]) ** 2).sum(axis=1)
    return -hidden - x @ layer["c"]


def bits(n):
    """[2^n, n]: every 0 / 1 configuration of n units."""
    return ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.float64)


def exact_log_z(layer):
    """log Z of one RBM / unit-variance GRBM by enumerating its hidden layer."""
    W, b, c = layer["W"], layer["b"], layer["c"]
    h = bits(W.shape[1])
    act = h @ W.T                                   # [2^H, V]
    if layer["gauss"]:
        terms = h @ b + act @ c + 0.5 * (act ** 2).sum(axis=1) + 0.5 * W.shape[0] * np.log(2.0 * np.pi)
    else:
        terms = h @ b + softplus(act + c).sum(axis=1)
    return float(np.logaddexp.reduce(terms))


def plan(model):
    """(sampled layers of every bottom net, sampled layers of the joint net, the top layer), float64."""
    bottoms = [[f64(l) for l in net] for net in model["bottoms"]]
    if model.get("joint") is None:
        assert len(bottoms) == 1
        return [bottoms[0][:-1]], [], bottoms[0][-1]
    joint = [f64(l) for l in model["joint"]]
    return bottoms, joint[:-1], joint[-1]


def estimate(model, inputs, S, log_z, samples=None):
    """The estimator of mdbn_amd/bound.py in float64.  ``inputs``: one [N, V] matrix per bottom net.  ``samples``: None = draw
    (u < mean with the Philox uniforms of every sampled layer, replica row n S + s of data row n), or the samples to walk
    along, per net (bottoms first, then the joint net) a list of [N S, H] arrays.  Returns a dict: ``rows`` / ``row_stderr`` [N],
    ``bound``, ``stderr``, ``values`` [N, S], ``modality_rows`` [M, N], ``joint_rows`` [N], ``samples`` (as the argument), and
    ``means`` / ``uniforms`` of every sampled layer (per net) for the tie masks."""
    ups, joint, top = plan(model)
    N = len(inputs[0])
    if not any(ups) and not joint:
        S = 1
    out = dict(samples=[], means=[], uniforms=[])

    def climb(layers, x, div, given):
        total, got, means, unis = np.zeros(len(x) * div), [], [], []
        for k, l in enumerate(layers):
            mean = sigmoid(np.asarray(x, dtype=np.float64) @ l["W"] + l["b"])
            rep = np.repeat(mean, div, axis=0)
            if given is None:
                u = philox_np.uniform(len(rep), rep.shape[1], l["seed"], l["stream"], l["step"], 0).astype(np.float64)
                s = (u < rep).astype(np.float64)
                unis.append(u)
            else:
                s = np.asarray(given[k], dtype=np.float64)
            total = total + row_loglik(s, l, np.repeat(np.asarray(x, dtype=np.float64), div, axis=0)) + np.repeat(entropy(mean), div)
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
    jvalue = jterm - free_energy(x, top)
    value = (value + jvalue).reshape(N, S)
    var = value.var(axis=1, ddof=1) if S > 1 else np.zeros(N)
    out.update(rows=value.mean(axis=1) - log_z, row_stderr=np.sqrt(var / S), values=value,
               modality_rows=np.asarray(modality_rows), joint_rows=jvalue.reshape(N, S).mean(axis=1) - log_z)
    out.update(bound=float(out["rows"].mean()), stderr=float(np.sqrt(var.sum() / S) / N))
    return out


def brute_force(model, inputs):
    """(exact log p(x_0) [N], exact bound [N], exact log Z of the top layer) by enumerating every configuration of every
    sampled layer: log p = logsumexp_config log p(x_0, config), bound = sum_config q(config | x_0) (log p(x_0, config) -
    log q(config | x_0)) -- the expectation the estimator samples, entropies included."""
    ups, joint, top = plan(model)
    log_z = exact_log_z(top)
    sizes = [l["W"].shape[1] for layers in ups for l in layers] + [l["W"].shape[1] for l in joint]
    conf = bits(sum(sizes))
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
                log_q = log_q + (s * pre - softplus(pre)).sum(axis=1)       # log Bernoulli(s; sigmoid(pre))
                log_j = log_j + row_loglik(s, l, x)
                x = s
            return x, at, log_q, log_j

        for layers, x0 in zip(ups, inputs):
            x = np.repeat(np.asarray(x0[n:n + 1], dtype=np.float64), C, axis=0)
            x, at, log_q, log_j = walk(layers, x, at, log_q, log_j)
            tops.append(x)
        x = np.concatenate(tops, axis=1) if model.get("joint") is not None else tops[0]
        x, at, log_q, log_j = walk(joint, x, at, log_q, log_j)
        log_j = log_j - free_energy(x, top) - log_z
        log_p[n] = np.logaddexp.reduce(log_j) if C > 1 else log_j[0]
        bound[n] = (np.exp(log_q) * (log_j - log_q)).sum()
    return log_p, bound, log_z


def tie_fraction(est, tie=4e-6):
    """Fraction of the draws of ``estimate`` whose uniform lies within ``tie`` of its mean (such a draw may fall the other way
    on the device, whose mean is a float32)."""
    n = total = 0
    for means, unis in zip(est["means"], est["uniforms"]):
        for m, u in zip(means, unis):
            n += int((np.abs(u - m) < tie).sum())
            total += u.size
    return n / max(total, 1)


# ------------------------------------------------------------------ the stacks of the tests
def make_net(rs, sizes, gauss, scale, seed, first_stream=0):
    """Layers sizes[0] -> sizes[1] -> ...: W = scale N(0, 1) / sqrt(fan-in), biases N(0, 0.5), float32 values; layer k draws
    from stream first_stream + k (the order a DBN hands streams to its RBMs), step 0."""
    net = []
    for k in range(len(sizes) - 1):
        V, H = sizes[k], sizes[k + 1]
        net.append(dict(W=(scale * rs.normal(0, 1, (V, H)) / np.sqrt(V)).astype(np.float32),
                        b=rs.normal(0, 0.5, H).astype(np.float32), c=rs.normal(0, 0.5, V).astype(np.float32),
                        gauss=bool(gauss and k == 0), seed=seed, stream=first_stream + k, step=0))
    return net


def make_data(rs, n, V, gauss):
    return rs.normal(0, 1, (n, V)).astype(np.float32) if gauss else (rs.uniform(size=(n, V)) < 0.5).astype(np.float32)


def stacks(scale):
    """{name: (model, inputs)} of the twin and GPU tests at one weight scale."""
    out = {}
    for name, sizes, gauss, seed in (("bernoulli_8_6_4", (8, 6, 4), False, 11), ("gauss_8_6_4", (8, 6, 4), True, 12),
                                     ("deep_7_5_4_3", (7, 5, 4, 3), False, 13)):
        rs = np.random.RandomState(seed + int(10 * scale))
        out[name] = (dict(bottoms=[make_net(rs, sizes, gauss, scale, 1000 + seed)], joint=None), [make_data(rs, 6, sizes[0], gauss)])
    rs = np.random.RandomState(14 + int(10 * scale))
    a, b = make_net(rs, (5, 3), True, scale, 2001), make_net(rs, (4, 2), True, scale, 2002)
    out["forest"] = (dict(bottoms=[a, b], joint=make_net(rs, (5, 4, 3), False, scale, 2003)),
                     [make_data(rs, 6, 5, True), make_data(rs, 6, 4, True)])
    return out


def tied(model):
    """The two-layer stack whose second layer is the transpose of the first: W_2 = W_1^T, b_2 = c_1, c_2 = b_1."""
    first = model["bottoms"][0][0]
    second = dict(first, W=np.ascontiguousarray(first["W"].T), b=first["c"].copy(), c=first["b"].copy(), gauss=False,
                  stream=first["stream"] + 1)
    return dict(bottoms=[[first, second]], joint=None)
