"""float64 twin of the categorical visible units (mdbn_group_softmax_sample / mdbn_cd_step_grouped; TEST-ONLY): the grouped
softmax, the first-``u < C_c`` sampling rule with its last-category fall-back, the cross-entropy from the log-sum-exp, the
CD chain of a layer with groups written out on oracle/rbm_np.py (free or teacher-forced along a recorded chain), a checker
engine with the two engine calls, and the kernel cases the CPU and the GPU test share.

A table is the int boundaries ``[g_0, ..., g_G]``: group g is columns g_g .. g_{g+1} - 1; columns outside [g_0, g_G) are
Bernoulli units.  Uniforms are column-addressed matrices [B, V] (oracle.philox_np): a group uses the entry of its FIRST
column, a Bernoulli column its own."""
import numpy as np
import torch

import _center_np as cn
import _sparsity_np as sn
from _oracle_engine import OracleEngine, _Scratch
from oracle import rbm_np
from oracle.philox_np import PhiloxDraws, uniform

MEAN_TOL = 2e-6         # _margins.SURVEY["prob"]: a softmax entry is a probability like a sigmoid's


def spans(bounds):
    b = np.asarray(bounds, dtype=np.int64)
    return [(int(lo), int(hi)) for lo, hi in zip(b[:-1], b[1:])]


def bernoulli_columns(bounds, V):
    b = np.asarray(bounds, dtype=np.int64)
    if b.size < 2:
        return np.arange(V)
    return np.concatenate([np.arange(0, b[0]), np.arange(b[-1], V)])


def grouped_softmax(pre, bounds):
    """-> (mean [B, V], log Z [B, G], max [B, G]): softmax inside every group, sigmoid elsewhere."""
    pre = np.asarray(pre, dtype=np.float64)
    mean = rbm_np.sigmoid(pre)
    sp = spans(bounds)
    logZ, mx = np.zeros((pre.shape[0], len(sp))), np.zeros((pre.shape[0], len(sp)))
    for g, (lo, hi) in enumerate(sp):
        x = pre[:, lo:hi]
        m = x.max(axis=1, keepdims=True)
        e = np.exp(x - m)
        Z = e.sum(axis=1, keepdims=True)
        mean[:, lo:hi] = e / Z
        logZ[:, g], mx[:, g] = np.log(Z[:, 0]), m[:, 0]
    return mean, logZ, mx


def grouped_sample(mean, bounds, U):
    """The sample of ``mean`` under the uniforms ``U``: a group's category is the first c with u < C_c (C: the running sum
    of its means), the last one when none qualifies; a Bernoulli column is u < mean."""
    mean, U = np.asarray(mean, dtype=np.float64), np.asarray(U, dtype=np.float64)
    sample = (U < mean).astype(np.float64)
    for lo, hi in spans(bounds):
        C = np.cumsum(mean[:, lo:hi], axis=1)
        below = U[:, lo:lo + 1] < C
        cat = np.where(below.any(axis=1), below.argmax(axis=1), hi - lo - 1)
        sample[:, lo:hi] = 0.0
        sample[np.arange(mean.shape[0]), lo + cat] = 1.0
    return sample


def grouped_cost(pre, v0, bounds):
    """Sum over all rows: sum_c v0_c (log Z - (x_c - m)) inside the groups, v0 softplus(-x) + (1 - v0) softplus(x) elsewhere."""
    pre, v0 = np.asarray(pre, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    cols = bernoulli_columns(bounds, pre.shape[1])
    x, t = pre[:, cols], v0[:, cols]
    total = (t * rbm_np.softplus(-x) + (1.0 - t) * rbm_np.softplus(x)).sum()
    _, logZ, mx = grouped_softmax(pre, bounds)
    for g, (lo, hi) in enumerate(spans(bounds)):
        total += (v0[:, lo:hi] * (logZ[:, g:g + 1] - (pre[:, lo:hi] - mx[:, g:g + 1]))).sum()
    return float(total)


def tie_draws(mean, bounds, U, tol=MEAN_TOL):
    """Number of draws that float32 rounding of the means could decide either way: a Bernoulli column with |u - mean| < tol,
    a group with |u - C_c| < tol (c + 1) for a boundary c = 0 .. K - 2 between two categories (the means' own bound summed
    over the c + 1 terms of C_c)."""
    mean, U = np.asarray(mean, dtype=np.float64), np.asarray(U, dtype=np.float64)
    cols = bernoulli_columns(bounds, mean.shape[1])
    n = int((np.abs(U[:, cols] - mean[:, cols]) < tol).sum())
    for lo, hi in spans(bounds):
        C = np.cumsum(mean[:, lo:hi], axis=1)[:, :-1]
        width = tol * np.arange(1, hi - lo)[None, :]
        n += int((np.abs(U[:, lo:lo + 1] - C) < width).any(axis=1).sum())
    return n


def follow(own, recorded, mean, bounds, U, tol=MEAN_TOL, what="v"):
    """Teacher forcing on a grouped visible sample: ``recorded`` (the device's) must be a valid sample -- 0 / 1, one 1 per
    group -- and equal the twin's ``own`` except at ties: a Bernoulli column with |u - mean| < tol; a group where u lies
    within tol (c + 1) of EVERY boundary C_c that separates the two categories.  -> (recorded as float64, differing draws)."""
    own, rec = np.asarray(own, dtype=np.float64), np.asarray(recorded, dtype=np.float64)
    mean, U = np.asarray(mean, dtype=np.float64), np.asarray(U, dtype=np.float64)
    assert np.isin(rec, (0.0, 1.0)).all(), "%s: a sample that is neither 0 nor 1" % what
    cols = bernoulli_columns(bounds, mean.shape[1])
    differ = own[:, cols] != rec[:, cols]
    n = int(differ.sum())
    if n:
        gap = np.abs(U[:, cols] - mean[:, cols])[differ].max()
        assert gap < tol, "%s: a Bernoulli sample differs from the twin's away from a tie (|u - p| = %g)" % (what, gap)
    for lo, hi in spans(bounds):
        assert (rec[:, lo:hi].sum(axis=1) == 1.0).all(), "%s: group [%d, %d) does not hold exactly one 1" % (what, lo, hi)
        a, b = own[:, lo:hi].argmax(axis=1), rec[:, lo:hi].argmax(axis=1)
        C = np.cumsum(mean[:, lo:hi], axis=1)
        for r in np.nonzero(a != b)[0]:
            n += 1
            for c in range(min(a[r], b[r]), max(a[r], b[r])):
                gap = abs(U[r, lo] - C[r, c])
                assert gap < tol * (c + 1), "%s: row %d of group [%d, %d): category %d against the twin's %d, %g from boundary %d" % (
                    what, r, lo, hi, b[r], a[r], gap, c)
    return rec, n


# ------------------------------------------------------------------------------------------------------------------ the CD chain
def sample_v_given_h(s, h, bounds, U):
    pre = h @ s.W.T + s.vbias
    mean = grouped_softmax(pre, bounds)[0]
    return pre, mean, grouped_sample(mean, bounds, U)


def cd_chain(s, v0, draws, k, bounds, persistent=None, trace_h=None, trace_v=None, tie=1e-6):
    """rbm_np.cd_chain / cd_chain_forced for a layer with groups (draws: 0 = U_h0, 2t - 1 = the visible draw of step t, 2t = its
    hidden draw).  With ``trace_h`` / ``trace_v`` every sample the chain feeds onward is the recorded one, checked against
    the twin's own outside ties.  -> (ph_mean, ph_sample, [pre_v, v_mean, v_sample, pre_h, h_mean, h_sample], differing draws)."""
    B, forced, flips = v0.shape[0], trace_h is not None, 0
    U0 = draws.u(0, B, s.n_hidden)
    _, ph_mean, ph_sample = rbm_np.sample_h_given_v(s, v0, U0)
    if forced:
        ph_sample, n = rbm_np._follow(ph_sample, trace_h[0], U0, ph_mean, tie, "h0")
        flips += n
    chain = ph_sample if persistent is None else persistent
    out = None
    for t in range(1, k + 1):
        Uv = draws.u(2 * t - 1, B, s.n_visible)
        pre_v, v_mean, v_sample = sample_v_given_h(s, chain, bounds, Uv)
        if forced:
            v_sample, n = follow(v_sample, trace_v[t - 1], v_mean, bounds, Uv, what="v%d" % t)
            flips += n
        Uh = draws.u(2 * t, B, s.n_hidden)
        pre_h, h_mean, h_sample = rbm_np.sample_h_given_v(s, v_sample, Uh)
        if forced and (t < k or persistent is not None):
            h_sample, n = rbm_np._follow(h_sample, trace_h[t], Uh, h_mean, tie, "h%d" % t)
            flips += n
        out = [pre_v, v_mean, v_sample, pre_h, h_mean, h_sample]
        chain = h_sample
    return ph_mean, ph_sample, out, flips


def update(s, state, v0, ph, nv, nh, batch_size, lr, mode="plain", momentum=0.0, **hyper):
    """One update of ``s`` from the means of a chain: ``mode`` "plain", "centered" (offset rate 0.05) or "sparse" (target 0.1,
    cost 0.05).  ``state``: what the previous call returned (None first).  -> the new state."""
    if mode == "centered":
        return cn.centered_update(s, state, v0, ph, nv, nh, 0.05, batch_size, lr, momentum=momentum, **hyper)
    if mode == "sparse":
        return sn.sparse_update(s, state, v0, ph, nv, nh, batch_size, lr, 0.1, 0.05, momentum=momentum, **hyper)
    if mode in ("both", "both_bias"):           # sparsity target, then centring; "both_bias": through the hidden biases only
        return sn.sparse_update(s, state, v0, ph, nv, nh, batch_size, lr, 0.1, 0.05, weights=mode == "both", centered=True, nu=0.05,
                                momentum=momentum, **hyper)
    S, s_h, s_v = rbm_np.cd_statistics(v0, ph, nv, nh)
    g = rbm_np.rbm_grad(s, S, s_h, s_v, batch_size, v0.shape[0], hyper.get("weightcost", 0.0))
    rbm_np.apply_update(s, g[0], g[1], g[2], lr, hyper.get("lambda_1", 0.0), hyper.get("lambda_2", 0.0), momentum)
    return None


def transformed_stats(mode, state, v0, ph, nv, nh, batch_size):
    """(S, s_h, s_v, offsets or None) as the packed buffer holds them when the update of ``mode`` reads it: the statistics of
    the chain after the sparsity and the centring transform.  ``state``: what ``update`` returned for this step."""
    n = v0.shape[0]
    S, s_h, s_v = rbm_np.cd_statistics(v0, ph, nv, nh)
    offsets = None
    if mode in ("sparse", "both", "both_bias"):
        weights = mode != "both_bias"
        S, s_h, s_v = sn.stats(S, s_h, s_v, state["q"], v0.mean(axis=0) if weights else None, 0.1,
                               0.05 * batch_size if weights else 0.0, 0.05 * n)
        offsets = state.get("offsets")
    if mode == "centered":
        offsets = state
    if offsets is not None:
        S, s_h, s_v = cn.center_stats(S, s_h, s_v, offsets[0], offsets[1], float(n) / float(batch_size))
    return S, s_h, s_v, offsets


def center_hidden_rows(v0, nv, ph, nh, s_h, s_v, mu, lam, rho, sparsity=None):
    """s_h' = s_h - rho S'^T mu of _center_np.center_stats formed from the rows: d_r = mu . (x_r - mu),
    S'^T mu = sum_r (d_r ph_r - d_{B+r} nh_r) - (s_v . mu) lam.  ``s_h`` is the statistic as the packed buffer holds it;
    ``sparsity`` = (q, v_mean, target, w_scale, b_scale) of a sparsity transform that ran on the buffer before: its share
    (w_scale (v_mean . mu) - b_scale (mu . mu)) (target - q) of S'^T mu is added."""
    v0, nv, ph, nh, s_h, s_v, mu, lam = (np.asarray(x, dtype=np.float64) for x in (v0, nv, ph, nh, s_h, s_v, mu, lam))
    d0, d1 = (v0 - mu) @ mu, (nv - mu) @ mu
    t = d0 @ ph - d1 @ nh - (s_v @ mu) * lam
    if sparsity is not None:
        q, v_mean, target, w_scale, b_scale = sparsity
        vm_mu = 0.0 if (v_mean is None or w_scale == 0.0) else float(np.asarray(v_mean, dtype=np.float64) @ mu)
        t = t + (w_scale * vm_mu - b_scale * float(mu @ mu)) * (target - np.asarray(q, dtype=np.float64))
    return s_h - rho * t


MODE_KEYWORDS = {"plain": {}, "centered": dict(centered=True, offset_rate=0.05),
                 "sparse": dict(sparsity_target=0.1, sparsity_cost=0.05),
                 "both": dict(centered=True, offset_rate=0.05, sparsity_target=0.1, sparsity_cost=0.05),
                 "both_bias": dict(centered=True, offset_rate=0.05, sparsity_target=0.1, sparsity_cost=0.05, sparsity_weights=False)}


def one_hot_data(rs, N, V, bounds, p=0.3):
    """[N, V] float32: one 1 per group, Bernoulli(p) elsewhere."""
    x = (rs.uniform(size=(N, V)) < p).astype(np.float32)
    for lo, hi in spans(bounds):
        x[:, lo:hi] = 0.0
        x[np.arange(N), lo + rs.randint(hi - lo, size=N)] = 1.0
    return x


# ------------------------------------------------------------------------------------------------------------------ checker engine
class GroupedOracle(OracleEngine):
    """The checker engine with the two calls of a layer with groups, from the twin."""

    def __init__(self):
        OracleEngine.__init__(self)
        self.keep_seen = []

    def group_softmax(self, pre, groups, rng, v0=None):
        pre = self.as_matrix(pre).numpy()
        mean = grouped_softmax(pre, groups.host)[0]
        sample = None
        if rng is not None:
            sample = self._t(grouped_sample(mean, groups.host, self._u(rng, pre.shape[0], pre.shape[1])))
        if v0 is None:
            return self._t(mean), sample
        return self._t(mean), sample, torch.tensor(grouped_cost(pre, self.as_matrix(v0).numpy(), groups.host), dtype=self.t_dtype)

    def cd_step(self, data, indexes, *args, **kw):
        self.keep_seen.append(kw.pop("keep_f32", None))
        stats, sc = OracleEngine.cd_step(self, data, indexes, *args, **kw)
        data = self.as_matrix(data)
        sc.v0 = (data if indexes is None else data[self.index_tensor(indexes)]).numpy()
        return stats, sc

    def cd_step_grouped(self, data, indexes, W, hbias, vbias, k, rng, groups, persistent=None, stats_slot=0, stats=None,
                        keep_f32=None):
        self.keep_seen.append(keep_f32)
        data = self.as_matrix(data)
        v0 = (data if indexes is None else data[self.index_tensor(indexes)]).numpy()
        s = self._state(W, hbias, vbias, False)
        draws = PhiloxDraws(rng.seed, rng.stream_id, rng.step, rng.row_offset)
        chain0 = persistent.numpy().copy() if persistent is not None else None
        ph_mean, ph_sample, out, _ = cd_chain(s, v0, draws, k, groups.host, chain0)
        S, s_h, s_v = rbm_np.cd_statistics(v0, ph_mean, out[1], out[4])
        cost = grouped_cost(out[0], v0, groups.host)
        if persistent is not None:
            persistent.copy_(self._t(out[5]))
        if stats is None:
            stats = self.stats_buffer(W.shape[0], W.shape[1], stats_slot)
        stats.copy_(self._t(np.concatenate([S.ravel(), s_h, s_v, [cost, 0, 0, 0]])))
        sc = _Scratch()
        sc.v0, sc.ph_mean, sc.nv_mean, sc.nh_mean, sc.ph_sample = v0, ph_mean, out[1], out[4], ph_sample
        self.last = sc
        return stats, sc

    # the transforms that compose with the grouped step (tests/test_center_api.py, tests/test_sparsity_api.py keep their own)
    def center_offsets(self, scratch, B, mu, lam, nu):
        m, l = cn.center_offsets(mu.numpy(), lam.numpy(), scratch.v0, scratch.ph_mean, nu)
        mu.copy_(self._t(m))
        lam.copy_(self._t(l))

    def center_stats(self, stats, V, H, ldv, ldh, mu, lam, row_scale):
        st = stats.numpy()
        S, s_h, s_v = cn.center_stats(st[:V * H].reshape(V, H), st[V * H:V * H + H], st[V * H + H:V * H + H + V],
                                      mu.numpy(), lam.numpy(), row_scale)
        stats[:V * H + H + V] = self._t(np.concatenate([S.ravel(), s_h, s_v]))
        return stats

    def center_hidden_rows(self, scratch, B, stats, V, H, ldv, ldh, mu, lam, row_scale, sparsity=None):
        st = stats.numpy()
        if sparsity is not None:
            sparsity = tuple(x.numpy() if isinstance(x, torch.Tensor) else x for x in sparsity)
        return self._t(center_hidden_rows(scratch.v0, scratch.nv_mean, scratch.ph_mean, scratch.nh_mean, st[V * H:V * H + H],
                                          st[V * H + H:V * H + H + V], mu.numpy(), lam.numpy(), row_scale, sparsity))

    @staticmethod
    def center_stats_store_hidden(stats, V, H, ldh, s_h):
        stats[V * H:V * H + H] = s_h

    def sparsity_activity(self, scratch, B, q, v_mean, rate):
        new_q, vm = sn.activity(q.numpy(), scratch.v0 if v_mean is not None else None, scratch.ph_mean, rate)
        q.copy_(self._t(new_q))
        if v_mean is not None:
            v_mean.copy_(self._t(vm))

    def sparsity_stats(self, stats, V, H, ldv, ldh, q, v_mean, target, w_scale, b_scale):
        st = stats.numpy()
        S, s_h, s_v = sn.stats(st[:V * H].reshape(V, H), st[V * H:V * H + H], st[V * H + H:V * H + H + V], q.numpy(),
                               None if v_mean is None else v_mean.numpy(), target, w_scale, b_scale)
        stats[:V * H + H + V] = self._t(np.concatenate([S.ravel(), s_h, s_v]))
        return stats


# ------------------------------------------------------------------------------------------------------------------ kernel cases
# (V, ldv, boundaries): the smallest mixed layer; the largest and the smallest K, groups straddling 16-byte boundaries, a
# Bernoulli prefix column; the copy-number shape (40 groups of 5); the label block behind 784 Bernoulli units
KERNEL_SHAPES = [
    (7, 8, [0, 3, 5]),
    (70, 72, [1, 3, 67, 70]),
    (200, 200, list(range(0, 201, 5))),
    (794, 796, [784, 794]),
]
KERNEL_ROWS = [1, 5, 33]
ROW_OFFSET = 6              # not a multiple of 4: the 4-row Philox blocks straddle
KERNEL_CASES = [(V, ldv, b, B) for V, ldv, b in KERNEL_SHAPES for B in KERNEL_ROWS]
# Philox seed of a case: the first of 100 + shape index, + 1000, ... under which the twin alone has at most TIE_CAP draws
# near a boundary (tests/test_softmax_api.py asserts it), so that the GPU test's cap can only be broken by the kernel
CASE_SEEDS = {}
TIE_CAP = 4
STREAM, STEP, DRAW = 3, 11, 5


def case_seed(V, B):
    return CASE_SEEDS.get((V, B), 100 + V + 7 * B)


def case_inputs(V, ldv, bounds, B, seed=None):
    """-> (pre float32 [B, V], v0 float32 [B, V], U float32 [B, V], seed): N(0, 2^2) pre-activations made on the host; from
    five rows on, row 1 is all-equal, row 2 has one entry per unit block at +80 relative to the rest, row 3 at -80."""
    seed = case_seed(V, B) if seed is None else seed
    rs = np.random.RandomState(1000 * V + B)
    pre = (2.0 * rs.normal(size=(B, V))).astype(np.float32)
    if B >= 5:
        pre[1, :] = np.float32(0.375)
        for row, shift in ((2, 80.0), (3, -80.0)):
            pre[row, :] = np.float32(-1.5)
            for lo, hi in spans(bounds):
                pre[row, lo + rs.randint(hi - lo)] += np.float32(shift)
            for c in bernoulli_columns(bounds, V)[::3]:
                pre[row, c] += np.float32(shift)
    v0 = one_hot_data(rs, B, V, bounds)
    U = uniform(B, V, seed, STREAM, STEP, DRAW, ROW_OFFSET)
    return pre, v0, U, seed
