"""Float64 twin of the classification RBM (TEST-ONLY): the exact posterior of a one-hot label block and the exact gradient of
sum_rows log p(y* | x) (Larochelle & Bengio 2008), in the notation of csrc/mdbn_class.h.

The block is columns lo .. lo + K - 1; everything outside it counts as input.  x~ = the row with the block set to zero,
A = hbias + x~ W, U = W[lo:lo+K], d = vbias[lo:lo+K]:
    o[y, j] = A[j] + U[y, j],   a[y] = d[y] + sum_j softplus(o[y, j]),   p(y | x) = softmax_y a[y]
    r_pos = sigmoid(o[y*, .]),  r_bar = sum_y p(y | x) sigmoid(o[y, .])
"""
import numpy as np
import torch

from oracle import rbm_np
from _softmax_np import GroupedOracle


def softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def masked(v, lo, K):
    x = np.array(v, dtype=np.float64)
    x[:, lo:lo + K] = 0.0
    return x


def scores(v, W, hbias, vbias, lo, K):
    """o [N, K, H] and a [N, K]."""
    W, hbias, vbias = (np.asarray(t, dtype=np.float64) for t in (W, hbias, vbias))
    A = masked(v, lo, K) @ W + hbias
    o = A[:, None, :] + W[lo:lo + K][None, :, :]
    return o, vbias[lo:lo + K][None, :] + softplus(o).sum(axis=2)


def posterior(v, W, hbias, vbias, lo, K):
    """p(y | x) [N, K], float64."""
    a = scores(v, W, hbias, vbias, lo, K)[1]
    e = np.exp(a - a.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def labels(v, lo, K):
    return np.asarray(v)[:, lo:lo + K].argmax(axis=1)


def logp(v, W, hbias, vbias, lo, K):
    """log p(y* | x) [N] for the category the block of every row holds."""
    a = scores(v, W, hbias, vbias, lo, K)[1]
    m = a.max(axis=1)
    return a[np.arange(len(a)), labels(v, lo, K)] - m - np.log(np.exp(a - m[:, None]).sum(axis=1))


def brute_posterior(v, W, hbias, vbias, lo, K):
    """softmax_c(-F(v with category c)) by K free energies."""
    s = rbm_np.RBMState(W.shape[0], W.shape[1], W=W, hbias=hbias, vbias=vbias)
    neg_F = np.empty((len(v), K))
    for c in range(K):
        x = masked(v, lo, K)
        x[:, lo + c] = 1.0
        neg_F[:, c] = -rbm_np.free_energy(s, x)
    e = np.exp(neg_F - neg_F.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def pieces(v, W, hbias, vbias, lo, K):
    """(x~, p [N, K], onehot [N, K], sig [N, K, H], r_pos [N, H], r_bar [N, H])."""
    o, _ = scores(v, W, hbias, vbias, lo, K)
    p = posterior(v, W, hbias, vbias, lo, K)
    hot = np.zeros_like(p)
    hot[np.arange(len(p)), labels(v, lo, K)] = 1.0
    sig = sigmoid(o)
    return masked(v, lo, K), p, hot, sig, (hot[:, :, None] * sig).sum(axis=1), (p[:, :, None] * sig).sum(axis=1)


def stats(v, W, hbias, vbias, lo, K):
    """The discriminative statistics (S [V, H], s_h [H], s_v [V]) and -sum log p(y* | x): the gradient of
    sum_rows log p(y* | x) with respect to W, hbias, vbias, ascent direction."""
    xt, p, hot, sig, r_pos, r_bar = pieces(v, W, hbias, vbias, lo, K)
    S = xt.T @ (r_pos - r_bar)
    S[lo:lo + K] = ((hot - p)[:, :, None] * sig).sum(axis=0)
    s_v = np.zeros(W.shape[0])
    s_v[lo:lo + K] = (hot - p).sum(axis=0)
    return S, (r_pos - r_bar).sum(axis=0), s_v, -logp(v, W, hbias, vbias, lo, K).sum()


def stacked_stats(v0, W, hbias, vbias, lo, K, gen=0.0, w=1.0, nv=None, ph=None, nh=None):
    """gen (CD statistics of v0, ph, nv, nh) + w (discriminative statistics) the way the device forms them: ONE product of the
    stacked operands V2' = [v0; v0 | nv; x~], P2' = [gen ph; w r_pos | -gen nh; -w r_bar] (gen = 0: the chain's halves are
    absent), s_h the column sum of P2', then the patch -- the block's rows of S minus w T, s_v rebuilt whole."""
    v0 = np.asarray(v0, dtype=np.float64)
    xt, p, hot, sig, r_pos, r_bar = pieces(v0, W, hbias, vbias, lo, K)
    if gen > 0.0:
        V2 = np.concatenate([v0, v0, nv, xt])
        P2 = np.concatenate([gen * ph, w * r_pos, -gen * nh, -w * r_bar])
    else:
        V2 = np.concatenate([v0, xt])
        P2 = np.concatenate([w * r_pos, -w * r_bar])
    S, s_h = V2.T @ P2, P2.sum(axis=0)
    T = (p[:, :, None] * sig).sum(axis=0)
    S[lo:lo + K] -= w * T
    s_v = gen * (v0 - nv).sum(axis=0) if gen > 0.0 else np.zeros(W.shape[0])
    s_v[lo:lo + K] += w * (hot - p).sum(axis=0)
    return S, s_h, s_v


def hybrid_stats(v0, W, hbias, vbias, lo, K, gen, w, nv, ph, nh):
    """The same sum formed directly: gen * rbm_np.cd_statistics + w * stats."""
    S, s_h, s_v = rbm_np.cd_statistics(np.asarray(v0, dtype=np.float64), ph, nv, nh)
    dS, dh, dv, _ = stats(v0, W, hbias, vbias, lo, K)
    return gen * S + w * dS, gen * s_h + w * dh, gen * s_v + w * dv


def update(s, S, s_h, s_v, batch_size, n_rows, lr, momentum=0.0, weightcost=0.0):
    """The project's update rule (oracle.rbm_np) on given statistics."""
    g = rbm_np.rbm_grad(s, S, s_h, s_v, batch_size, n_rows, weightcost)
    rbm_np.apply_update(s, g[0], g[1], g[2], lr, 0.0, 0.0, momentum)


# ------------------------------------------------------------------------------------------------------------------ the toy problem
TOY = dict(classes=3, inputs=12, H=8, B=32, flips=0.10, std=0.3, steps=300, lr=0.5, seed=4)


def toy_problem(seed=TOY["seed"]):
    """3 classes, 12 Bernoulli inputs made from class prototypes with 10 % flips, the one-hot label block behind them:
    (rows [B, 15] float32, lo, K, W [15, 8] float32 of std 0.3)."""
    rs = np.random.RandomState(seed)
    C, D, H, B = TOY["classes"], TOY["inputs"], TOY["H"], TOY["B"]
    proto = (rs.uniform(size=(C, D)) < 0.5).astype(np.float32)
    y = rs.randint(C, size=B)
    x = proto[y]
    flip = rs.uniform(size=x.shape) < TOY["flips"]
    x = np.where(flip, 1.0 - x, x).astype(np.float32)
    hot = np.zeros((B, C), dtype=np.float32)
    hot[np.arange(B), y] = 1.0
    W = (TOY["std"] * rs.normal(size=(D + C, H))).astype(np.float32)
    return np.concatenate([x, hot], axis=1), D, C, W


def toy_train(rows, lo, K, W, steps=TOY["steps"], lr=TOY["lr"]):
    """Purely discriminative steps of the twin under the project's update rule: -> (state, [mean NLL before every step])."""
    s = rbm_np.RBMState(W.shape[0], W.shape[1], W=W)
    B, nll = len(rows), []
    for _ in range(steps):
        S, s_h, s_v, n = stats(rows, s.W, s.hbias, s.vbias, lo, K)
        nll.append(n / B)
        update(s, S, s_h, s_v, B, B, lr)
    return s, nll


def accuracy(rows, s, lo, K):
    return float((posterior(rows, s.W, s.hbias, s.vbias, lo, K).argmax(axis=1) == labels(rows, lo, K)).mean())


# ------------------------------------------------------------------------------------------------------------------ checker engine
class DiscOracle(GroupedOracle):
    """The checker engine with the two classification calls, from the twin; ``calls`` records what the step functions asked for."""

    def __init__(self):
        GroupedOracle.__init__(self)
        self.calls = []

    def class_posterior(self, v, W, hbias, vbias, lo, K, want_logp=False):
        v = self.as_matrix(v).numpy()
        args = (v, W.numpy(), hbias.numpy(), vbias.numpy(), lo, K)
        return self._t(posterior(*args)), (self._t(logp(*args)) if want_logp else None)

    def class_stats(self, scratch, v0, B, W, hbias, vbias, lo, K, gen_weight, disc_weight, packed):
        self.calls.append(dict(lo=lo, K=K, gen=gen_weight, w=disc_weight, pure=scratch is None, B=B))
        V, H = W.shape
        rows = scratch.v0 if scratch is not None else self.as_matrix(v0).numpy()
        S, s_h, s_v, nll = stats(rows, W.numpy(), hbias.numpy(), vbias.numpy(), lo, K)
        n = V * H + H + V
        disc = disc_weight * np.concatenate([S.ravel(), s_h, s_v])
        if scratch is not None:
            packed[:n] = self._t(gen_weight * packed.numpy()[:n] + disc)
        else:
            packed[:n] = self._t(disc)
            packed[n] = nll
        return torch.tensor(nll, dtype=self.t_dtype)
