"""numpy twin of the device's clamped Gibbs sampling (csrc/mdbn_clamp.hip; TEST-ONLY).

``clamp_twin`` restates mdbn_gibbs_clamped -- gibbs_vhv with the visibles where ``mask`` is nonzero held at ``obs``, and the
running means of v_mean / h_mean from ``burn_in`` on -- with the device's draw addressing (oracle/philox_np.py: hidden draw of
step t at ``step + 2t``, visible draw at ``step + 2t + 1``, draw index 0).  Float64 by default; with ``dtype=numpy.float32``
products, activations, the accumulators (in step order) and the final division are float32: the gap between the two on the
same samples is the float32 share of the device's error (tests/test_gpu_clamp.py takes its tolerance from it).

With ``forced=(trace_h, trace_v)`` the twin follows the device's recorded samples: at every step it still makes its OWN
draw from the recorded state, and reports where that draw differs from the record and how close to a tie it was.

``exact_posterior`` enumerates the 2^H hidden states: p(h | v_obs) is proportional to exp(h . (c + W_obs^T v_obs)) times
prod over the missing i of (1 + exp(b_i + W_i h)) (Bernoulli) | exp(b_i W_i h + (W_i h)^2 / 2) (unit-variance Gaussian)."""
import numpy as np

from oracle import philox_np

TIE = 4e-6          # near-tie mask of the drift tests (tests/test_gpu_surface.py): |u - p| below it may fall either way


def sigmoid(x):
    # exp(-x) may overflow to +inf on a saturated layer (float32: from x = -88.7 down): 1 / (1 + inf) = 0 is the right limit
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def clamp_twin(W, c, b, gauss, v0, obs, mask, n_steps, burn_in, seed, stream, step, add_noise=False, dtype=np.float64,
               forced=None, row_offset=0, sampler=False):
    """Returns dict(v, h_mean, h_sample, v_mean, v_avg, h_avg, trace_h [n_steps, B, H], trace_v [n_steps, B, V], n_draws,
    n_ties, n_flips, flips_outside_mask, max_v_diff).  ``sampler`` (Gaussian visibles, the library's gauss = 2): the hidden
    SAMPLE goes down and the visible draw always carries its N(0, 1) noise -- a Gibbs sampler of the model, where the
    reference's chain (hidden mean down) is a mean-field iteration."""
    sampler = bool(sampler and gauss)
    add_noise = bool(add_noise or sampler)
    W, c, b = (np.asarray(a, dtype=dtype) for a in (W, c, b))
    v0, obs = np.asarray(v0, dtype=dtype), np.asarray(obs, dtype=dtype)
    B, V = v0.shape
    H = W.shape[1]
    held = np.broadcast_to(np.asarray(mask) != 0, (B, V))
    assert n_steps >= 1 and 0 <= burn_in < n_steps
    stat = dict(n_draws=0, n_ties=0, n_flips=0, flips_outside_mask=0, max_v_diff=0.0)

    def u(st, cols, normal_bit=False):
        return philox_np.uniform(B, cols, seed, stream, st, philox_np.NORMAL_BIT if normal_bit else 0, row_offset)

    def bernoulli(p, uu, record, count=None):
        own = (uu < p).astype(dtype)
        if count is None:
            count = np.ones(p.shape, dtype=bool)
        tie = (np.abs(uu.astype(np.float64) - p.astype(np.float64)) < TIE) & count
        stat["n_draws"] += int(count.sum())
        stat["n_ties"] += int(tie.sum())
        if record is None:
            return own
        flip = (record != own) & count
        stat["n_flips"] += int(flip.sum())
        stat["flips_outside_mask"] += int((flip & ~tie).sum())
        return record.astype(dtype)

    th, tv = (None, None) if forced is None else forced
    v = np.where(held, obs, v0).astype(dtype)
    v_acc, h_acc = np.zeros((B, V), dtype=dtype), np.zeros((B, H), dtype=dtype)
    trace_h, trace_v = np.zeros((n_steps, B, H), dtype=dtype), np.zeros((n_steps, B, V), dtype=dtype)
    h_mean = h_sample = v_mean = None
    for t in range(n_steps):
        h_mean = sigmoid((v @ W + c).astype(dtype)).astype(dtype)
        h_sample = bernoulli(h_mean, u(step + 2 * t, H), None if th is None else th[t])
        trace_h[t] = h_sample
        pre = ((h_mean if gauss and not sampler else h_sample) @ W.T + b).astype(dtype)
        if gauss:
            v_mean, v_new = pre, pre
            if add_noise:
                u1, u2 = u(step + 2 * t + 1, V).astype(np.float64), u(step + 2 * t + 1, V, True).astype(np.float64)
                v_new = (pre + (np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)).astype(dtype)).astype(dtype)
            v_new = np.where(held, obs, v_new)
            if tv is not None:
                stat["max_v_diff"] = max(stat["max_v_diff"], float(np.abs(tv[t] - v_new).max()))
                v_new = tv[t].astype(dtype)
        else:
            v_mean = sigmoid(pre).astype(dtype)
            # (held entries are not draws: the record holds the observed value there)
            v_new = bernoulli(v_mean, u(step + 2 * t + 1, V), None if tv is None else tv[t], count=~held)
            v_new = np.where(held, obs, v_new)
        v_mean = np.where(held, obs, v_mean).astype(dtype)
        v = v_new.astype(dtype)
        trace_v[t] = v
        if t >= burn_in:
            v_acc = (v_acc + v_mean).astype(dtype)
            h_acc = (h_acc + h_mean).astype(dtype)
    n = np.dtype(dtype).type(n_steps - burn_in)
    return dict(v=v, h_mean=h_mean, h_sample=h_sample, v_mean=v_mean, v_avg=(v_acc / n).astype(dtype),
                h_avg=(h_acc / n).astype(dtype), trace_h=trace_h, trace_v=trace_v, **stat)


def exact_posterior(W, c, b, gauss, v_obs, held):
    """Exact ``(E[v | v_obs] [V], E[h | v_obs] [H])`` of ONE row (``held`` [V] bool, ``v_obs`` [V]: read where held), float64."""
    W, c, b, v_obs = (np.asarray(a, dtype=np.float64) for a in (W, c, b, v_obs))
    held = np.asarray(held, dtype=bool)
    V, H = W.shape
    assert H <= 20
    n = np.arange(1 << H)
    h = ((n[:, None] >> np.arange(H)[None, :]) & 1).astype(np.float64)
    act = b[None, ~held] + h @ W[~held].T                       # [2^H, missing]
    logp = h @ (c + W[held].T @ v_obs[held])
    if gauss:
        logp = logp + (0.5 * act ** 2).sum(axis=1)              # (b_i + W_i h)^2 / 2 = b_i W_i h + (W_i h)^2 / 2 + const
        cond = act
    else:
        logp = logp + np.logaddexp(0.0, act).sum(axis=1)
        cond = sigmoid(act)
    p = np.exp(logp - logp.max())
    p /= p.sum()
    ev = v_obs.copy()
    ev[~held] = p @ cond
    return ev, p @ h


def half_mask(V, seed=0, rows=None):
    """About half the columns observed: one row [1, V], or ``rows`` independent rows [rows, V] (float32 0 / 1)."""
    rs = np.random.RandomState(100 + seed)
    return (rs.uniform(size=(1 if rows is None else rows, V)) < 0.5).astype(np.float32)
