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


def score_sums(v, W, hbias, vbias, lo, K, rows=128):
    """a [N, K] alone, ``rows`` rows at a time: o [N, K, H] of a many-row case with K = 64 would take gigabytes."""
    v = np.asarray(v)
    return np.concatenate([scores(v[i:i + rows], W, hbias, vbias, lo, K)[1] for i in range(0, len(v), rows)])


def posterior(v, W, hbias, vbias, lo, K):
    """p(y | x) [N, K], float64."""
    a = score_sums(v, W, hbias, vbias, lo, K)
    e = np.exp(a - a.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def labels(v, lo, K):
    return np.asarray(v)[:, lo:lo + K].argmax(axis=1)


def logp(v, W, hbias, vbias, lo, K):
    """log p(y* | x) [N] for the category the block of every row holds."""
    a = score_sums(v, W, hbias, vbias, lo, K)
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


def stacked_operands(v0, W, hbias, vbias, lo, K, gen=0.0, w=1.0, nv=None, ph=None, nh=None):
    """(V2', P2') of ``stacked_stats``, float64: what the device hands its one statistics product."""
    v0 = np.asarray(v0, dtype=np.float64)
    xt, _, _, _, r_pos, r_bar = pieces(v0, W, hbias, vbias, lo, K)
    if gen > 0.0:
        return np.concatenate([v0, v0, nv, xt]), np.concatenate([gen * ph, w * r_pos, -gen * nh, -w * r_bar])
    return np.concatenate([v0, xt]), np.concatenate([w * r_pos, -w * r_bar])


def stacked_stats(v0, W, hbias, vbias, lo, K, gen=0.0, w=1.0, nv=None, ph=None, nh=None):
    """gen (CD statistics of v0, ph, nv, nh) + w (discriminative statistics) the way the device forms them: ONE product of the
    stacked operands V2' = [v0; v0 | nv; x~], P2' = [gen ph; w r_pos | -gen nh; -w r_bar] (gen = 0: the chain's halves are
    absent), s_h the column sum of P2', then the patch -- the block's rows of S minus w T, s_v rebuilt whole."""
    v0 = np.asarray(v0, dtype=np.float64)
    xt, p, hot, sig, r_pos, r_bar = pieces(v0, W, hbias, vbias, lo, K)
    V2, P2 = stacked_operands(v0, W, hbias, vbias, lo, K, gen, w, nv, ph, nh)
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


# ------------------------------------------------------------------------------------------------------------------ launch geometry
# A plain mirror of class_geom() in csrc/mdbn_drv_class.hip: a workgroup of class_forward owns R rows at a time (batch b of
# workgroup g is rows (g + b G) R ..), R = min(4, ceil(B / CUs)), G = ceil(B / R) workgroups; training mode keeps one [K][ldh]
# partial of T per workgroup, so there G is capped at min(4 CUs, 32 Mi floats / (K ldh)) and a workgroup takes several trips.
CLASS_R = 4
CLASS_PARTIAL_FLOATS = 32 << 20


def class_geom(cu, B, K, ldh, train):
    """-> (R, G) of a class_forward launch on a device of ``cu`` compute units."""
    cu = max(int(cu), 1)
    R = min(CLASS_R, max(1, -(-B // cu)))
    G = -(-B // R)
    if train:
        G = min(G, 4 * cu, max(1, CLASS_PARTIAL_FLOATS // (K * ldh)))
    return R, G


def class_reach(cu, B, K, ldh, train):
    """-> (R, rows of the last batch, trips of the busiest workgroup -- workgroup 0) of that launch."""
    R, G = class_geom(cu, B, K, ldh, train)
    batches = -(-B // R)
    return R, B - (batches - 1) * R, -(-batches // G)


# key -> (B as a function of the CU count, (R, rows of the last batch, trips of workgroup 0) the case is meant to reach, in
# posterior and in training mode alike except for the trips).  The layer is 21 x 37 with K = 3 (ldh = 40) unless a test says
# otherwise; neither cap of training mode depends on it as long as K ldh <= 8192.
GEOMETRY = [
    ("cu+1", lambda cu: cu + 1, (2, 1, 1)),
    ("2cu+2", lambda cu: 2 * cu + 2, (3, 1, 1)),
    ("3cu+1", lambda cu: 3 * cu + 1, (4, 1, 1)),
    ("3cu+2", lambda cu: 3 * cu + 2, (4, 2, 1)),
    ("3cu+3", lambda cu: 3 * cu + 3, (4, 3, 1)),
    ("4cu", lambda cu: 4 * cu, (4, 4, 1)),
    ("16cu+23", lambda cu: 16 * cu + 23, (4, 3, 2)),         # training mode: 4 cu + 6 batches on 4 cu workgroups
]
GEOMETRY_KEYS = [k for k, _, _ in GEOMETRY]


def geometry_cases(cu, K=3, ldh=40):
    """{key: (B, (R, rows of the last batch, trips))} on a device of ``cu`` compute units.  B is the key's formula; where the
    CU count's remainder keeps that B from the tail the case is meant for (cu + 1 is even on an odd count), B grows by the few
    rows that restore it -- on 256 units every B is the formula's.  The trips are those of training mode (posterior mode caps
    nothing: one trip)."""
    out = {}
    for key, f, want in GEOMETRY:
        B = f(cu)
        for _ in range(2 * CLASS_R + 1):
            if class_reach(cu, B, K, ldh, True) == want:
                break
            B += 1
        assert class_reach(cu, B, K, ldh, True) == want, "%s: %d compute units cannot reach %r" % (key, cu, want)
        assert want[2] > 1 or class_reach(cu, B, K, ldh, False) == want
        out[key] = (B, want)
    return out


def layer_params(V, H, scale, seed):
    """(W, hbias, vbias) float32 of a device test's layer."""
    rs = np.random.RandomState(seed)
    return tuple((scale * rs.normal(size=n)).astype(np.float32) for n in ((V, H), H, V))


# The cases of tests/test_gpu_disc.py beyond one row per workgroup; tests/test_disc_twin.py runs the twin alone on each.  B: a
# key of GEOMETRY or a number.  id, V, H, B, boundaries of the groups the rows are made with, label group, scale.
BETWEEN = (21, 37, [2, 5, 8], 1)
WIDE = (1030, 37, [0, 1022, 1027, 1030], 1)     # ldv = 1032: the block, columns 1022 .. 1026, lies across column 1024 and begins mid-quad
MANY_ROW_POSTERIOR = [("between_K3_H37_" + k,) + BETWEEN[:2] + (k,) + BETWEEN[2:] + (0.5,) for k in ("cu+1", "2cu+2", "3cu+1", "3cu+3", "4cu")]
MANY_ROW_POSTERIOR += [("last_K64_H513_3cu+2", 70, 513, "3cu+2", [1, 3, 6, 70], 2, 0.2),
                       ("wide_K5_H37_B33",) + WIDE[:2] + (33,) + WIDE[2:] + (0.5,)]
MANY_ROW_STATS = [("odd_small_" + k,) + BETWEEN[:2] + (k,) + BETWEEN[2:] + (0.3,) for k in ("cu+1", "3cu+1", "16cu+23")]
MANY_ROW_STATS += [("saturated_odd_small",) + BETWEEN[:2] + (33,) + BETWEEN[2:] + (30.0,),
                   ("wide_K5_H37_B33",) + WIDE[:2] + (33,) + WIDE[2:] + (0.3,)]


def rows_of(cu, B):
    return geometry_cases(cu)[B][0] if isinstance(B, str) else B


def posterior_inputs(V, H, B, bounds, g, scale, distinct=False):
    """(rows [B, V] float32, W, hbias, vbias, lo, K) of a posterior case on the device."""
    from _softmax_np import one_hot_data
    lo, K = bounds[g], bounds[g + 1] - bounds[g]
    rs = np.random.RandomState(B)
    rows = distinct_rows(rs, B, V, bounds, lo, K) if distinct else one_hot_data(rs, B, V, bounds)
    return (rows,) + layer_params(V, H, scale, V + H + B) + (lo, K)


def stats_inputs(V, H, B, bounds, g, scale, distinct=False):
    """(v0, nv [B, V], ph, nh [B, H] float32, W, hbias, vbias, lo, K, the generator they came from) of a statistics case on the
    device: the rows and the means a chain could have left."""
    from _softmax_np import grouped_softmax, one_hot_data
    lo, K = bounds[g], bounds[g + 1] - bounds[g]
    rs = np.random.RandomState(H)
    v0 = distinct_rows(rs, B, V, bounds, lo, K) if distinct else one_hot_data(rs, B, V, bounds)
    nv = grouped_softmax(rs.normal(size=(B, V)), bounds)[0].astype(np.float32)
    ph, nh = rs.uniform(size=(B, H)).astype(np.float32), rs.uniform(size=(B, H)).astype(np.float32)
    return (v0, nv, ph, nh) + layer_params(V, H, scale, V + B) + (lo, K, rs)


def distinct_rows(rs, B, V, bounds, lo, K, p=0.5):
    """``one_hot_data`` rows [B, V] that differ pairwise OUTSIDE the label block: p(y | x) sees nothing else of a row, so a row
    handed to another wave's slot of the workgroup shows up as another posterior."""
    from _softmax_np import one_hot_data
    seen, rows = set(), []
    for _ in range(64):
        if len(rows) == B:
            break
        for r in one_hot_data(rs, B, V, bounds, p):
            key = masked(r[None], lo, K).tobytes()
            if key not in seen and len(rows) < B:
                seen.add(key)
                rows.append(r)
    assert len(rows) == B, "%d columns outside the block hold fewer than %d different rows" % (V - K, B)
    return np.stack(rows)


def distinct_inputs(v, lo, K):
    """The number of different rows of ``v`` outside the label block."""
    return len({r.tobytes() for r in masked(v, lo, K)})


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
