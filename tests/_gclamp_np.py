"""numpy twin of clamped Gibbs sampling on a layer with categorical visible units (mdbn_gibbs_clamped_grouped; TEST-ONLY):
``clamp_twin`` of tests/_clamp_np.py with a boundary list, and the running sums and ``pick`` of tests/_gais_np.py for the
visible draw of a group -- one category of the softmax over the group's pre-activations h W^T + b, from ONE uniform at the
group's first column.  A group is held or free as a whole: by the mask entry at its FIRST column (what the device does for
any mask; the masks of ``unit_mask`` are constant on groups).

float64 by default; ``dtype=numpy.float32``: products, activations, the exponentials, Z, the running sum C_c, the
accumulators (in step order) and the final division in float32 in the device's order.  With ``forced=(trace_h, trace_v)``
the twin follows the device's recorded samples, makes its OWN draw from the recorded state at every step and reports where
the two differ.  A group draw has K - 1 boundaries C_0 .. C_{K-2}; ``c_gap`` is the largest |C_c(float32) - C_c(float64)| the
run met on its own inputs (free groups only), ``group_miss`` the largest distance of a uniform from a boundary that separates
a recorded category from the twin's own, and ``group_near(mask)`` the number of free group draws with a boundary within
``mask`` of the uniform: the near-tie mask of a group draw is max(TIE, 4 c_gap), as in tests/test_gpu_gais.py.

``exact_posterior_grouped`` enumerates the 2^H hidden states: p(h | v_obs) is proportional to exp(h . (c + W_obs^T v_obs))
times prod over the free Bernoulli i of (1 + exp(b_i + W_i h)) times prod over the free groups g of sum_{c in g}
exp(b_c + W_c h).  ``GclampOracle`` is the CPU checker engine with ``gibbs_clamped_grouped``, composed from the checker's
propup, linear propdown and group_softmax, so the public classes run without a GPU."""
import numpy as np
import torch

import _clamp_np as Cn
import _gais_np as G
import _softmax_np as sm
from oracle import philox_np

TIE = Cn.TIE
TIE_SHARE = 1e-3        # tests/test_gpu_clamp.py: at most this share of the draws inside the near-tie mask


def group_held(mask, bounds, B, V):
    """[B, V] bool: the clamp as the device reads it -- a group's columns all follow the mask entry at its first column."""
    held = np.broadcast_to(np.asarray(mask) != 0, (B, V)).copy()
    for lo, hi in sm.spans(bounds):
        held[:, lo:hi] = held[:, lo:lo + 1]
    return held


def means_and_sums(pre, bounds, dtype):
    """(mean [B, V], C [B, V]) in ``dtype`` and the device's order: inside a group max, e = exp(x - max), Z = the ascending
    sum, mean = e / Z, C = the ascending sum of the means; elsewhere mean = C = sigmoid(pre)."""
    pre = np.asarray(pre, dtype=dtype)
    mean = Cn.sigmoid(pre).astype(dtype)
    C = mean.copy()
    for lo, hi in sm.spans(bounds):
        x = pre[:, lo:hi]
        e = np.exp(x - x.max(axis=1, keepdims=True)).astype(dtype)
        Z = np.cumsum(e, axis=1, dtype=dtype)[:, -1:]
        mean[:, lo:hi] = (e / Z).astype(dtype)
        C[:, lo:hi] = np.cumsum(mean[:, lo:hi], axis=1, dtype=dtype)
    return mean, C


def gclamp_twin(W, c, b, bounds, v0, obs, mask, n_steps, burn_in, seed, stream, step, dtype=np.float64, forced=None,
                row_offset=0, gaps=None):
    """Returns dict(v, h_mean, h_sample, v_mean, v_avg, h_avg, trace_h [n_steps, B, H], trace_v [n_steps, B, V]; n_draws,
    n_ties, n_flips, flips_outside_mask (hidden and free Bernoulli draws, mask ``TIE``); group_draws, group_boundaries,
    group_flips, group_miss, c_gap, group_near(mask) for the free group draws).  ``gaps``: measure ``c_gap`` and keep what
    ``group_near`` needs (default: only when forced)."""
    W, c, b = (np.asarray(a, dtype=dtype) for a in (W, c, b))
    v0, obs = np.asarray(v0, dtype=dtype), np.asarray(obs, dtype=dtype)
    B, V = v0.shape
    H = W.shape[1]
    groups, bern = sm.spans(bounds), sm.bernoulli_columns(bounds, V)
    held = group_held(mask, bounds, B, V)
    assert n_steps >= 1 and 0 <= burn_in < n_steps
    gaps = forced is not None if gaps is None else gaps
    stat = dict(n_draws=0, n_ties=0, n_flips=0, flips_outside_mask=0, group_draws=0, group_boundaries=0, group_flips=0,
                group_miss=0.0, c_gap=0.0)
    nearest = []                                         # per visible draw: [B, G] distance of u to the nearest boundary (inf: held)

    def u(st, cols):
        return philox_np.uniform(B, cols, seed, stream, st, 0, row_offset)

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

    def draw_v(pre, st, record):
        """-> (v_mean, v_new) before the clamp"""
        U = u(st, V)
        if dtype == np.float32:
            mean, C = means_and_sums(pre, bounds, np.float32)
            own = G.pick(C, bounds, U)
        else:
            mean = sm.grouped_softmax(pre, bounds)[0]
            own = sm.grouped_sample(mean, bounds, U)
            C = G.running_sums(pre, bounds, np.float64) if (gaps or record is not None) else None
        v = own.astype(dtype)
        if bern.size:
            rec_b = None if record is None else record[:, bern]
            v[:, bern] = bernoulli(mean[:, bern], U[:, bern], rec_b, count=~held[:, bern])
        free = np.stack([~held[:, lo] for lo, _ in groups], axis=1) if groups else np.zeros((B, 0), dtype=bool)
        stat["group_draws"] += int(free.sum())
        stat["group_boundaries"] += int(sum(free[:, g].sum() * (hi - lo - 1) for g, (lo, hi) in enumerate(groups)))
        if gaps and groups:
            C64 = G.running_sums(pre.astype(np.float64), bounds, np.float64)
            C32 = G.running_sums(pre.astype(np.float32), bounds, np.float32)
            near = np.full((B, len(groups)), np.inf)
            for g, (lo, hi) in enumerate(groups):
                f = free[:, g]
                if not f.any():
                    continue
                stat["c_gap"] = max(stat["c_gap"], float(np.abs(C32[f, lo:hi - 1].astype(np.float64) - C64[f, lo:hi - 1]).max()))
                near[f, g] = np.abs(U[f, lo:lo + 1].astype(np.float64) - C64[f, lo:hi - 1]).min(axis=1)
            nearest.append(near)
        if record is not None:
            rec = np.asarray(record, dtype=np.float64)
            for g, (lo, hi) in enumerate(groups):
                f = free[:, g]
                assert np.isin(rec[f, lo:hi], (0.0, 1.0)).all() and (rec[f, lo:hi].sum(axis=1) == 1.0).all(), \
                    "free group [%d, %d) does not hold exactly one 1" % (lo, hi)
                mine, theirs = own[:, lo:hi].argmax(axis=1), rec[:, lo:hi].argmax(axis=1)
                for r in np.nonzero((mine != theirs) & f)[0]:
                    stat["group_flips"] += 1
                    between = slice(lo + min(mine[r], theirs[r]), lo + max(mine[r], theirs[r]))
                    stat["group_miss"] = max(stat["group_miss"], float(np.abs(np.float64(U[r, lo]) - C[r, between]).max()))
                v[f, lo:hi] = rec[f, lo:hi]
        return mean.astype(dtype), v

    th, tv = (None, None) if forced is None else forced
    v = np.where(held, obs, v0).astype(dtype)
    v_acc, h_acc = np.zeros((B, V), dtype=dtype), np.zeros((B, H), dtype=dtype)
    trace_h, trace_v = np.zeros((n_steps, B, H), dtype=dtype), np.zeros((n_steps, B, V), dtype=dtype)
    h_mean = h_sample = v_mean = None
    for t in range(n_steps):
        h_mean = Cn.sigmoid((v @ W + c).astype(dtype)).astype(dtype)
        h_sample = bernoulli(h_mean, u(step + 2 * t, H), None if th is None else th[t])
        trace_h[t] = h_sample
        pre = (h_sample @ W.T + b).astype(dtype)
        v_mean, v_new = draw_v(pre, step + 2 * t + 1, None if tv is None else tv[t])
        v_mean = np.where(held, obs, v_mean).astype(dtype)
        v = np.where(held, obs, v_new).astype(dtype)
        trace_v[t] = v
        if t >= burn_in:
            v_acc = (v_acc + v_mean).astype(dtype)
            h_acc = (h_acc + h_mean).astype(dtype)
    n = np.dtype(dtype).type(n_steps - burn_in)

    def group_near(mask_width):
        return int(sum((x < mask_width).sum() for x in nearest))
    return dict(v=v, h_mean=h_mean, h_sample=h_sample, v_mean=v_mean, v_avg=(v_acc / n).astype(dtype),
                h_avg=(h_acc / n).astype(dtype), trace_h=trace_h, trace_v=trace_v, group_near=group_near, **stat)


def near_ties(r):
    """(mask, near ties, draws) of a run ``r`` measured with ``gaps``: hidden and Bernoulli draws within TIE, group draws with a
    boundary within mask = max(TIE, 4 c_gap) of the uniform."""
    mask = max(TIE, 4.0 * r["c_gap"])
    return mask, r["n_ties"] + r["group_near"](mask), r["n_draws"] + r["group_draws"]


def exact_posterior_grouped(W, c, b, bounds, v_obs, held):
    """Exact ``(E[v | v_obs] [V], E[h | v_obs] [H])`` of ONE row (``held`` [V] bool, constant on groups; ``v_obs`` [V]: read
    where held), float64, by enumerating the 2^H hidden states with a logsumexp per free group."""
    W, c, b, v_obs = (np.asarray(a, dtype=np.float64) for a in (W, c, b, v_obs))
    held = np.asarray(held, dtype=bool)
    V, H = W.shape
    assert H <= 16
    groups = [(lo, hi) for lo, hi in sm.spans(bounds) if not held[lo]]
    for lo, hi in sm.spans(bounds):
        assert (held[lo:hi] == held[lo]).all(), "the mask splits the group [%d, %d)" % (lo, hi)
    bern = np.array([i for i in sm.bernoulli_columns(bounds, V) if not held[i]], dtype=np.int64)
    n = np.arange(1 << H)
    h = ((n[:, None] >> np.arange(H)[None, :]) & 1).astype(np.float64)
    act = b[None, :] + h @ W.T                                  # [2^H, V]
    logp = h @ (c + W[held].T @ v_obs[held]) + np.logaddexp(0.0, act[:, bern]).sum(axis=1)
    for lo, hi in groups:
        logp = logp + np.logaddexp.reduce(act[:, lo:hi], axis=1)
    p = np.exp(logp - logp.max())
    p /= p.sum()
    ev = v_obs.copy()
    ev[bern] = p @ Cn.sigmoid(act[:, bern])
    for lo, hi in groups:
        x = act[:, lo:hi]
        e = np.exp(x - x.max(axis=1, keepdims=True))
        ev[lo:hi] = p @ (e / e.sum(axis=1, keepdims=True))
    return ev, p @ h


# ------------------------------------------------------------------------------------------------------------------ masks
def units(bounds, V):
    """[(first column, end column), ...] of the units of a row: the Bernoulli columns and the groups, in column order."""
    sp = sm.spans(bounds)
    lo0, hi0 = (sp[0][0], sp[-1][1]) if sp else (V, V)
    return [(i, i + 1) for i in range(lo0)] + sp + [(i, i + 1) for i in range(hi0, V)]


def unit_mask(V, bounds, seed=0, rows=None, p=0.5):
    """About half the UNITS observed (a group as a whole): one row [1, V], or ``rows`` independent rows [rows, V] (float32
    0 / 1).  With ``rows`` >= 2 the first row holds every unit and the second none."""
    rs = np.random.RandomState(100 + seed)
    un = units(bounds, V)
    R = 1 if rows is None else rows
    pick = rs.uniform(size=(R, len(un))) < p
    if rows is not None and rows >= 2:
        pick[0], pick[1] = True, False
    m = np.zeros((R, V), dtype=np.float32)
    for k, (lo, hi) in enumerate(un):
        m[:, lo:hi] = pick[:, k:k + 1]
    return m


def inputs(V, bounds, B, per_row, seed=9):
    """Start state (0 / 1, one-hot groups), observed values (one-hot groups; probabilities in (0, 1) on the Bernoulli columns,
    what a joint layer sees) and the mask."""
    rs = np.random.RandomState(seed)
    v0 = sm.one_hot_data(rs, B, V, bounds, p=0.5)
    obs = rs.uniform(size=(B, V)).astype(np.float32)
    hot = sm.one_hot_data(rs, B, V, bounds)
    for lo, hi in sm.spans(bounds):
        obs[:, lo:hi] = hot[:, lo:hi]
    return v0, obs, unit_mask(V, bounds, rows=B if per_row else None)


# ------------------------------------------------------------------------------------------------------------------ cases
# forced parity (tests/test_gpu_gclamp.py): V, H, scale of W, boundaries, paths
PARITY = [
    (100, 24, 0.3, list(range(0, 101, 5)), (1, 2)),
    (70, 24, 0.3, [1, 3, 67, 70], (1, 2)),
    (1024, 256, 0.02, list(range(0, 1025, 4)), (2,)),
]
PARITY_B = (64, 22)
N_STEPS, BURN_IN = 8, 2
SEED, STREAM, STEP = 5, 3, 11


def parity_params(V, H, s, seed=3):
    rs = np.random.RandomState(seed)
    W = rs.normal(0, s, (V, H)).astype(np.float32)
    return W, rs.normal(0, 0.5, H).astype(np.float32), rs.normal(0, 0.5, V).astype(np.float32)


# ground truth: the four brute-force cases of tests/_gais_np.py (V, H, scale of W, boundaries); M chains of GT_STEPS steps for
# one row with about half its units observed; the chain-averaged v_avg / h_avg within GT_Z standard errors (std over chains /
# sqrt(M)) of the exact posterior means, the largest standard error <= SE_CAP
CASES = G.CASES
M, GT_STEPS, GT_BURN, SE_CAP, GT_Z = 128, 600, 100, 0.01, 2.5
# Philox seed of a case's run (stream 3, step 11), and of its run with ONE group free: seeds under which the float64 twin ALONE
# meets the bound (tests/test_gclamp_twin.py asserts it), so that on the device only the kernel can break it
CASE_SEEDS = {24: 4, 100: 5, 70: 1, 40: 2}
ONE_FREE_SEEDS = {24: 1, 100: 4, 70: 1, 40: 1}


def ground_truth_case(V, H, s, bounds, one_free=False):
    """Parameters of a brute-force case, one 0 / 1 row with one-hot groups and about half its units observed (``one_free``:
    every unit but the first group), and the exact E[v | v_obs], E[h | v_obs].  -> W, c, b, row, held, ev, eh"""
    W, c, b, _ = G.case_params(V, H, s)
    rs = np.random.RandomState(11)
    row = sm.one_hot_data(rs, 1, V, bounds, p=0.5)[0]
    if one_free:
        held = np.ones(V, dtype=bool)
        lo, hi = sm.spans(bounds)[0]
        held[lo:hi] = False
    else:
        held = unit_mask(V, bounds)[0] != 0
    ev, eh = exact_posterior_grouped(W, c, b, bounds, row, held)
    return W, c, b, row, held, ev, eh


def base_start(b, bounds, row, held):
    """The start of ``RBM.impute``: observed entries, elsewhere sigmoid(vbias), a free group at the softmax of its vbias."""
    b = np.asarray(b, dtype=np.float64)
    base = 1.0 / (1.0 + np.exp(-b))
    for lo, hi in sm.spans(bounds):
        e = np.exp(b[lo:hi] - b[lo:hi].max())
        base[lo:hi] = e / e.sum()
    return np.where(held, row, base.astype(np.float32)).astype(np.float32)


def z_statistic(v_hat, h_hat, held, ev, eh):
    """(largest standard error, largest |error| / standard error) of the statistic of tests/test_gpu_clamp.py::test_ground_truth:
    per free visible column and per hidden unit, the mean over the M chains against the exact value, se = std / sqrt(M)."""
    worst_se, worst_z = 0.0, 0.0
    for est, exact in ((np.asarray(v_hat)[:, ~held], ev[~held]), (np.asarray(h_hat), eh)):
        est = est.astype(np.float64)
        m, se = est.mean(axis=0), est.std(axis=0) / np.sqrt(est.shape[0])
        worst_se = max(worst_se, float(se.max()))
        worst_z = max(worst_z, float((np.abs(m - exact) / np.maximum(se, 1e-12)).max()))
    return worst_se, worst_z


# ------------------------------------------------------------------------------------------------------------------ checker engine
class GclampOracle(sm.GroupedOracle):
    """The checker engine of a layer with groups plus ``gibbs_clamped_grouped``, composed from its own propup, linear
    propdown and group_softmax (float64)."""

    def gibbs_clamped_grouped(self, v, obs, mask, W, hbias, vbias, n_steps, rng, groups, burn_in=0, path=0, steps_per_launch=0,
                              trace=False):
        from mdbn_amd import RngAddr
        v, obs = self.as_matrix(v), self.as_matrix(obs)
        B, V = v.shape
        held = torch.from_numpy(group_held(np.asarray(getattr(mask, "numpy", lambda: mask)()), groups.host, B, V))
        state = torch.where(held, obs, v)
        v_acc, h_acc, th, tv = 0.0, 0.0, [], []
        h_mean = h_sample = v_mean = None
        for t in range(int(n_steps)):
            _, h_mean, h_sample = self.propup(state, W, hbias, rng=RngAddr(rng.seed, rng.stream_id, rng.step + 2 * t, 0, rng.row_offset))
            pre = self.propdown(h_sample, W, vbias, gauss=True, add_noise=False, rng=None)[1]
            mean, new = self.group_softmax(pre, groups, RngAddr(rng.seed, rng.stream_id, rng.step + 2 * t + 1, 0, rng.row_offset))
            v_mean, state = torch.where(held, obs, mean), torch.where(held, obs, new)
            if t >= burn_in:
                v_acc, h_acc = v_acc + v_mean, h_acc + h_mean
            th.append(h_sample)
            tv.append(state)
        n = int(n_steps) - int(burn_in)
        out = (state, h_mean, h_sample, v_mean, v_acc / n, h_acc / n)
        return out + ((torch.stack(th), torch.stack(tv)) if trace else ())
