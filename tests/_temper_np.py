"""numpy twin of the device's parallel tempering (csrc/mdbn_temper.hip, include/mdbn_hip.h: mdbn_pt_run; TEST-ONLY).

``pt_twin`` restates the sweep -- row m R + s = slot s of ladder m, ``rank[m][s]`` the temperature index the slot holds --
with the device's draw addressing (oracle/philox_np.py): sweep t draws v at ``step + 3t`` (row-indexed, global replica row),
the swap uniforms at ``step + 3t + 1`` (row = ladder, column = lower rank) and h at ``step + 3t + 2``; draw index 0.

    joint at beta:  log p_beta(v, h) = beta (v W h + c h) + { b_beta . v | -|v - b_beta|^2 / 2 },  b_beta = b_A + beta (b - b_A)
    1. v ~ sigmoid(b_beta + beta h W^T) | b_beta + beta h W^T + N(0, 1)
    2. a = v W + c;  l(beta') = sum_j softplus(beta' a_j) + { v . b_beta' | -|v - b_beta'|^2 / 2 }
    3. pairs (rho, rho + 1), rho = sweep0 + t (mod 2): accept iff log u < l_i(beta_j) + l_j(beta_i) - l_i(beta_i) - l_j(beta_j)
    4. h ~ sigmoid(beta a) at the rank after the swap

Float64 by default: the acceptance difference is then the DEFINITION, four evaluations of l.  With ``dtype=numpy.float32``
products, activations, row sums and the running sums are float32 and the difference is formed as the device forms it (the
regrouping of DESIGN 3.4: float32 row sums of softplus differences and of s1, combined in double): the gap between the two on
the same states is the float32 share of the device's error (tests/test_gpu_temper.py takes its tolerances from it).

With ``forced=(trace_v, trace_h, trace_swaps)`` the twin follows the device's recorded states and rank maps: at every draw it
still makes its OWN draw / decision from the recorded state and reports where it differs from the record and how close to a
tie that was."""
import numpy as np

from oracle import philox_np

TIE = 4e-6          # near-tie mask of the drift tests (tests/test_gpu_surface.py): |u - p| below it may fall either way


def sigmoid(x):
    # exp(-x) may overflow to +inf on a saturated layer (float32: from x = -88.7 down): 1 / (1 + inf) = 0 is the right limit
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def pt_twin(W, c, b, bA, gauss, betas, h0, n, burn_in, seed, stream, step, rank0=None, sweep0=0, dtype=np.float64,
            forced=None, swaps=True):
    """Returns dict(v, h, rank, accepted [R-1], v_avg [M, V], h_avg [M, H], trace_v, trace_h, trace_swaps [n, M, 2, R],
    logu, delta, decided (one entry per swap attempt, in (sweep, pair, ladder) order: log u, the twin's acceptance
    difference, the decision followed), n_draws, n_ties, flips_outside_mask, max_v_diff)."""
    W, c, b, bA = (np.asarray(x, dtype=dtype) for x in (W, c, b, bA))
    betas32 = np.asarray(betas, dtype=np.float32)
    betas = betas32.astype(dtype)
    R = betas.size
    h = np.asarray(h0, dtype=dtype).copy()
    MR, H = h.shape
    M, V = MR // R, W.shape[0]
    assert M * R == MR and n >= 1 and 0 <= burn_in < n
    rank = np.tile(np.arange(R), (M, 1)) if rank0 is None else np.asarray(rank0, dtype=np.int64).copy()
    db = (b - bA).astype(dtype)
    lad = np.arange(M)
    stat = dict(n_draws=0, n_ties=0, flips_outside_mask=0, max_v_diff=0.0)
    fv, fh, fs = (None, None, None) if forced is None else forced

    def bernoulli(p, uu, record):
        own = (uu < p).astype(dtype)
        tie = np.abs(uu.astype(np.float64) - p.astype(np.float64)) < TIE
        stat["n_draws"] += p.size
        stat["n_ties"] += int(tie.sum())
        if record is None:
            return own
        flip = record != own
        stat["flips_outside_mask"] += int((flip & ~tie).sum())
        return record.astype(dtype)

    def ell(v, a, bb):
        """l(beta') of every row at the betas ``bb`` [M R] (the definition)."""
        bias = bA[None, :] + bb[:, None] * db[None, :]
        vis = -0.5 * ((v - bias) ** 2).sum(axis=1) if gauss else (v * bias).sum(axis=1)
        return softplus(bb[:, None] * a).sum(axis=1) + vis

    v_sum, h_sum = np.zeros((M, V), dtype=dtype), np.zeros((M, H), dtype=dtype)
    accepted = np.zeros(R - 1, dtype=np.int64)
    tv, th, ts = np.zeros((n, MR, V), dtype=dtype), np.zeros((n, MR, H), dtype=dtype), np.zeros((n, M, 2, R), dtype=np.int32)
    logus, deltas, decided = [], [], []
    v = None
    for t in range(n):
        g = sweep0 + t
        flat = rank.reshape(-1)
        beta = betas[flat]
        top = flat == R - 1
        # 1. the visible draw
        m = (h @ W.T).astype(dtype)
        pre = (bA[None, :] + beta[:, None] * db[None, :] + beta[:, None] * m).astype(dtype)
        u1 = philox_np.uniform(MR, V, seed, stream, step + 3 * t, 0)
        if gauss:
            u2 = philox_np.uniform(MR, V, seed, stream, step + 3 * t, philox_np.NORMAL_BIT)
            z = np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(2.0 * np.pi * u2.astype(np.float64))
            v = (pre + z.astype(dtype)).astype(dtype)
            mean1 = pre
            if fv is not None:
                stat["max_v_diff"] = max(stat["max_v_diff"], float(np.abs(fv[t] - v).max()))
                v = fv[t].astype(dtype)
        else:
            mean1 = sigmoid(pre).astype(dtype)
            v = bernoulli(mean1, u1, None if fv is None else fv[t])
        tv[t] = v
        # 2. the pre-activations
        a = (v @ W + c).astype(dtype)
        # 3. the swaps
        inv = np.argsort(rank, axis=1)
        us = philox_np.uniform(M, R - 1, seed, stream, step + 3 * t + 1, 0)
        logu = np.log(us.astype(np.float64))
        dec = np.full((M, R), -1, dtype=np.int32)
        new_rank = rank.copy()
        for rho in range(g % 2, R - 1, 2):
            i, j = lad * R + inv[:, rho], lad * R + inv[:, rho + 1]
            b_lo, b_hi = betas[rho], betas[rho + 1]
            if dtype == np.float64:
                lo, hi = np.full(M, b_lo), np.full(M, b_hi)
                delta = (ell(v[i], a[i], hi) + ell(v[j], a[j], lo) - ell(v[i], a[i], lo) - ell(v[j], a[j], hi))
            else:
                hs_i = (softplus(b_hi * a[i]) - softplus(b_lo * a[i])).astype(dtype).sum(axis=1, dtype=dtype)
                hs_j = (softplus(b_lo * a[j]) - softplus(b_hi * a[j])).astype(dtype).sum(axis=1, dtype=dtype)
                s1_i = (((v[i] - bA[None, :]) if gauss else v[i]) * db[None, :]).astype(dtype).sum(axis=1, dtype=dtype)
                s1_j = (((v[j] - bA[None, :]) if gauss else v[j]) * db[None, :]).astype(dtype).sum(axis=1, dtype=dtype)
                delta = (hs_i.astype(np.float64) + hs_j.astype(np.float64)
                         + (np.float64(b_hi) - np.float64(b_lo)) * (s1_i.astype(np.float64) - s1_j.astype(np.float64)))
            own = (logu[:, rho] < delta) & bool(swaps)
            follow = own if fs is None else fs[t][:, 1, rho] == 1
            logus.append(logu[:, rho]); deltas.append(np.asarray(delta, dtype=np.float64)); decided.append(follow.copy())
            dec[:, rho] = follow
            accepted[rho] += int(follow.sum())
            si, sj = inv[follow, rho], inv[follow, rho + 1]
            new_rank[lad[follow], si] = rho + 1
            new_rank[lad[follow], sj] = rho
        rank = new_rank
        ts[t, :, 0, :] = rank
        ts[t, :, 1, :] = dec
        # 4. the hidden draw at the rank after the swap
        flat = rank.reshape(-1)
        p = sigmoid((betas[flat][:, None] * a).astype(dtype)).astype(dtype)
        h = bernoulli(p, philox_np.uniform(MR, H, seed, stream, step + 3 * t + 2, 0), None if fh is None else fh[t])
        th[t] = h
        if t >= burn_in:
            v_sum = (v_sum + mean1[top]).astype(dtype)
            h_sum = (h_sum + p[flat == R - 1]).astype(dtype)
    k = np.dtype(dtype).type(n - burn_in)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0)
    return dict(v=v, h=h, rank=rank, accepted=accepted, v_avg=(v_sum / k).astype(dtype), h_avg=(h_sum / k).astype(dtype),
                trace_v=tv, trace_h=th, trace_swaps=ts, logu=cat(logus), delta=cat(deltas), decided=cat(decided).astype(bool),
                **stat)


def exact_visible_mean(W, c, b, gauss=False):
    """Exact ``E[v]`` [V] of the layer by enumerating the 2^H hidden states (float64): p(h) is proportional to exp(c . h) times
    prod_i (1 + exp(b_i + W_i h)) (Bernoulli) | exp((b_i + W_i h)^2 / 2) (unit-variance Gaussian)."""
    W, c, b = (np.asarray(x, dtype=np.float64) for x in (W, c, b))
    H = W.shape[1]
    assert H <= 20
    k = np.arange(1 << H)
    h = ((k[:, None] >> np.arange(H)[None, :]) & 1).astype(np.float64)
    act = b[None, :] + h @ W.T
    logp = h @ c + ((0.5 * act ** 2).sum(axis=1) if gauss else np.logaddexp(0.0, act).sum(axis=1))
    p = np.exp(logp - logp.max())
    p /= p.sum()
    return p @ (act if gauss else sigmoid(act))


def two_mode_model(V=24, H=12, seed=0, gauss=False):
    """The planted two-mode layer of the ground-truth tests: ``(W, c, b, b_A)`` float64."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 2, V) * 2 - 1
    q = rng.integers(0, 2, H) * 2 - 1
    W = 0.5 * np.outer(p, q) + 0.05 * rng.standard_normal((V, H))
    b = -W.sum(1) / 2 + 0.15 * p
    c = -W.sum(0) / 2
    return W, c, b, np.zeros(V)
