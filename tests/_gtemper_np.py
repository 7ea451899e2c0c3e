"""numpy twin of parallel tempering on a layer with categorical visible units (csrc/mdbn_temper.hip, include/mdbn_hip.h:
mdbn_pt_run_grouped; TEST-ONLY): ``pt_twin`` of tests/_temper_np.py with a boundary list.  On one-hot rows log p*_beta(v) =
sum_j softplus(beta a_j) + v . b_beta is the Bernoulli expression, so the swap decision, the hidden draw, the rank map and the
works (tests/_ptz_np.py ``works_from_trace``, unchanged) are the plain run's.  Two things change: the visible draw of a group
-- one category of the softmax over the group's tempered pre-activations at the beta of the row's rank, from ONE uniform at
the group's first column (``running_sums`` / ``pick`` of tests/_gais_np.py) -- and the beta = 1 visible mean that ``v_avg``
accumulates: the group's softmax mean.

float64 by default; ``dtype=numpy.float32``: the device's arithmetic and order (tests/_temper_np.py, tests/_gais_np.py).  With
``forced=(trace_v, trace_h, trace_swaps)`` the twin follows the device's record, makes its OWN draw / decision from the recorded
state and reports where the two differ; the group-draw bookkeeping (``group_flips``, ``group_miss``, ``c_gap``,
``group_near``, ``group_boundaries``) is that of ``_gais_np.ais_twin``.  With no groups every returned array equals
``_temper_np.pt_twin``'s exactly.

``exact_by_hidden`` / ``exact_by_rows`` give the exact visible marginals and log Z by enumeration (over the hidden states; over
the one-hot visible rows), ``planted`` the two-mode grouped layer of the ground-truth tests, ``GtemperOracle`` the CPU checker
engine with ``temper_grouped`` (and ``ais_grouped``), so the public classes run without a GPU."""
import itertools

import numpy as np

import _gais_np as G
import _softmax_np as sm
import _temper_np as T
from oracle import philox_np

TIE = T.TIE


def pt_twin(W, c, b, bA, bounds, betas, h0, n, burn_in, seed, stream, step, rank0=None, sweep0=0, dtype=np.float64,
            forced=None, swaps=True, row_offset=0):
    """``_temper_np.pt_twin`` (Bernoulli) for the boundary list ``bounds``: its dict, plus group_draws, group_boundaries,
    group_flips, group_miss, c_gap and group_near(mask)."""
    f32 = dtype == np.float32
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
    groups, bern = sm.spans(bounds), sm.bernoulli_columns(bounds, V)
    stat = dict(n_draws=0, n_ties=0, flips_outside_mask=0, max_v_diff=0.0, group_draws=0, group_boundaries=0, group_flips=0,
                group_miss=0.0, c_gap=0.0)
    nearest = []
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
        bias = bA[None, :] + bb[:, None] * db[None, :]
        return T.softplus(bb[:, None] * a).sum(axis=1) + (v * bias).sum(axis=1)

    def draw_v(pre, U, record):
        """-> (v, the beta-of-the-row mean: softmax inside a group, sigmoid elsewhere)."""
        mean = T.sigmoid(pre).astype(dtype)
        v = np.zeros_like(pre)
        v[:, bern] = bernoulli(mean[:, bern], U[:, bern], None if record is None else record[:, bern])
        if not groups:
            return v, mean
        if f32:
            C = G.running_sums(pre, bounds, np.float32)
            own = G.pick(C, bounds, U)
            for lo, hi in groups:
                x = pre[:, lo:hi]
                e = np.exp(x - x.max(axis=1, keepdims=True)).astype(np.float32)
                mean[:, lo:hi] = (e / np.cumsum(e, axis=1, dtype=np.float32)[:, -1:]).astype(np.float32)
        else:
            m64 = sm.grouped_softmax(pre, bounds)[0]
            own = sm.grouped_sample(m64, bounds, U)
            for lo, hi in groups:
                mean[:, lo:hi] = m64[:, lo:hi]
            C = G.running_sums(pre, bounds, np.float64) if record is not None else None
        stat["group_draws"] += pre.shape[0] * len(groups)
        stat["group_boundaries"] += pre.shape[0] * sum(hi - lo - 1 for lo, hi in groups)
        if record is not None:
            C64 = G.running_sums(pre.astype(np.float64), bounds, np.float64)
            C32 = G.running_sums(pre.astype(np.float32), bounds, np.float32)
            near = np.empty((pre.shape[0], len(groups)))
            for g, (lo, hi) in enumerate(groups):
                stat["c_gap"] = max(stat["c_gap"], float(np.abs(C32[:, lo:hi - 1].astype(np.float64) - C64[:, lo:hi - 1]).max()))
                near[:, g] = np.abs(U[:, lo:lo + 1].astype(np.float64) - C64[:, lo:hi - 1]).min(axis=1)
            nearest.append(near)
            rec = np.asarray(record, dtype=np.float64)
            assert np.isin(rec, (0.0, 1.0)).all(), "a visible sample that is neither 0 nor 1"
            for lo, hi in groups:
                assert (rec[:, lo:hi].sum(axis=1) == 1.0).all(), "group [%d, %d) does not hold exactly one 1" % (lo, hi)
                mine, theirs = own[:, lo:hi].argmax(axis=1), rec[:, lo:hi].argmax(axis=1)
                for r in np.nonzero(mine != theirs)[0]:
                    stat["group_flips"] += 1
                    between = slice(lo + min(mine[r], theirs[r]), lo + max(mine[r], theirs[r]))
                    stat["group_miss"] = max(stat["group_miss"], float(np.abs(np.float64(U[r, lo]) - C[r, between]).max()))
                v[:, lo:hi] = rec[:, lo:hi]
        else:
            for lo, hi in groups:
                v[:, lo:hi] = own[:, lo:hi]
        return v, mean

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
        u1 = philox_np.uniform(MR, V, seed, stream, step + 3 * t, 0, row_offset)
        v, mean1 = draw_v(pre, u1, None if fv is None else fv[t])
        tv[t] = v
        # 2. the pre-activations
        a = (v @ W + c).astype(dtype)
        # 3. the swaps
        inv = np.argsort(rank, axis=1)
        us = philox_np.uniform(M, R - 1, seed, stream, step + 3 * t + 1, 0, row_offset // R)
        logu = np.log(us.astype(np.float64))
        dec = np.full((M, R), -1, dtype=np.int32)
        new_rank = rank.copy()
        for rho in range(g % 2, R - 1, 2):
            i, j = lad * R + inv[:, rho], lad * R + inv[:, rho + 1]
            b_lo, b_hi = betas[rho], betas[rho + 1]
            if not f32:
                lo_, hi_ = np.full(M, b_lo), np.full(M, b_hi)
                delta = (ell(v[i], a[i], hi_) + ell(v[j], a[j], lo_) - ell(v[i], a[i], lo_) - ell(v[j], a[j], hi_))
            else:
                hs_i = (T.softplus(b_hi * a[i]) - T.softplus(b_lo * a[i])).astype(dtype).sum(axis=1, dtype=dtype)
                hs_j = (T.softplus(b_lo * a[j]) - T.softplus(b_hi * a[j])).astype(dtype).sum(axis=1, dtype=dtype)
                s1_i = (v[i] * db[None, :]).astype(dtype).sum(axis=1, dtype=dtype)
                s1_j = (v[j] * db[None, :]).astype(dtype).sum(axis=1, dtype=dtype)
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
        p = T.sigmoid((betas[flat][:, None] * a).astype(dtype)).astype(dtype)
        h = bernoulli(p, philox_np.uniform(MR, H, seed, stream, step + 3 * t + 2, 0, row_offset), None if fh is None else fh[t])
        th[t] = h
        if t >= burn_in:
            v_sum = (v_sum + mean1[top]).astype(dtype)
            h_sum = (h_sum + p[flat == R - 1]).astype(dtype)
    k = np.dtype(dtype).type(n - burn_in)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0)

    def group_near(mask):
        return int(sum((x < mask).sum() for x in nearest))
    return dict(v=v, h=h, rank=rank, accepted=accepted, v_avg=(v_sum / k).astype(dtype), h_avg=(h_sum / k).astype(dtype),
                trace_v=tv, trace_h=th, trace_swaps=ts, logu=cat(logus), delta=cat(deltas), decided=cat(decided).astype(bool),
                group_near=group_near, **stat)


def tie_cap(r, mask):
    """``_gais_np.tie_cap`` for a run of this twin."""
    return G.tie_cap(r, mask)


# ---------------------------------------------------------------------------------- exact values
def exact_by_hidden(W, c, b, bounds):
    """``(E[v] [V], log Z)`` by enumerating the 2^H hidden states, float64: p(h) is proportional to exp(c . h) times
    prod_Bernoulli (1 + exp(act_i)) prod_g sum_{c in g} exp(act_c), act = b + W h."""
    W, c, b = (np.asarray(x, dtype=np.float64) for x in (W, c, b))
    V, H = W.shape
    assert H <= 20
    bern, groups = sm.bernoulli_columns(bounds, V), sm.spans(bounds)
    k = np.arange(1 << H)
    h = ((k[:, None] >> np.arange(H)[None, :]) & 1).astype(np.float64)
    act = b[None, :] + h @ W.T
    logp = h @ c + np.logaddexp(0.0, act[:, bern]).sum(axis=1)
    for lo, hi in groups:
        logp += np.logaddexp.reduce(act[:, lo:hi], axis=1)
    top = logp.max()
    p = np.exp(logp - top)
    log_z = float(top + np.log(p.sum()))
    p /= p.sum()
    return p @ sm.grouped_softmax(act, bounds)[0], log_z


def exact_by_rows(W, c, b, bounds):
    """The same by enumerating the visible rows that hold one 1 per group (and any 0 / 1 in a Bernoulli column): log p*(v) =
    v . b + sum_j softplus(c_j + (v W)_j).  For layers with at most 2^20 such rows."""
    W, c, b = (np.asarray(x, dtype=np.float64) for x in (W, c, b))
    V, H = W.shape
    bern, groups = sm.bernoulli_columns(bounds, V), sm.spans(bounds)
    count = (1 << bern.size) * int(np.prod([hi - lo for lo, hi in groups], dtype=np.int64))
    assert count <= 1 << 20, count
    rows = np.zeros((count, V))
    choices = [[(), (int(col),)] for col in bern]                       # a Bernoulli column: off or on
    choices += [[(col,) for col in range(lo, hi)] for lo, hi in groups]
    for r, combo in enumerate(itertools.product(*choices)):
        on = [col for part in combo for col in part]
        rows[r, on] = 1.0
    logp = rows @ b + T.softplus(rows @ W + c).sum(axis=1)
    top = logp.max()
    p = np.exp(logp - top)
    log_z = float(top + np.log(p.sum()))
    return (p / p.sum()) @ rows, log_z


def planted(V=24, H=12, K=3, seed=0, strength=0.6, tilt=0.6, pull=1.0):
    """The planted two-mode layer with groups of K = 3: ``(W, c, b, b_A, bounds)`` float64.  Every group has one category of the
    heavy mode (p = +1), one of the light mode (p = -1) and a neutral one; W = strength p q^T + noise with q = +-1 per hidden
    unit.  The hidden bias c = pull q makes the mode (v on the +1 categories, h on the q = +1 units) the heavy one, the visible
    bias b = -tilt p leans the other way: from h = 0 the first visible draw falls towards the light mode, and a plain chain
    stays there."""
    assert V % K == 0 and K == 3
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.permutation([1.0, -1.0, 0.0]) for _ in range(V // K)])
    q = np.where(np.arange(H) % 2 == 0, 1.0, -1.0)[rng.permutation(H)]
    W = strength * np.outer(p, q) + 0.05 * rng.standard_normal((V, H))
    return W, pull * q, -tilt * p, np.zeros(V), list(range(0, V + 1, K))


# ---------------------------------------------------------------------------------- the cases the CPU and the GPU tests share
SEED, STREAM, STEP = 5, 3, 11
GT_M, GT_R, GT_SWEEPS, GT_BURN = 64, 16, 1200, 300
PARITY_M, PARITY_R, PARITY_N, PARITY_BURN = 5, 8, 40, 10
PARITY = [  # tag, V, H, scale of W, boundaries, saturated biases, paths
    ("groups of 5", 100, 24, 0.3, list(range(0, 101, 5)), False, (1, 2)),
    ("K = 2 and K = 64", 70, 24, 0.3, [1, 3, 67, 70], False, (1, 2)),
    ("saturated", 100, 24, 0.3, list(range(0, 101, 5)), True, (1, 2)),
]
LARGE = ("1024 -> 256", 1024, 256, 0.02, list(range(0, 1025, 4)), False, (2,))       # M = 4, 10 sweeps
RAGGED_R = 6


def parity_params(V, H, s, saturated=False):
    """W, c, b, b_A float32 of a forced-parity case (``_gais_np.parity_params``; ``saturated``: c and b on the ladder of
    tests/_saturated.py, as tests/test_gpu_gais.py places them)."""
    W, c, b, bA = G.parity_params(V, H, s)
    if saturated:
        import _saturated as S
        c, b = S.sampler_biases(V, H, False, b, 3)
        bA = (b + np.random.RandomState(4).normal(0, 0.3, V)).astype(np.float32)
    return W, c, b, bA


def start(M, R, H, seed=9):
    return (np.random.RandomState(seed).uniform(size=(M * R, H)) < 0.5).astype(np.float32)


def ground_truth_cases():
    """``[(tag, W, c, b, b_A, bounds)]``: the planted layer and 40 -> 14 with groups of 4 between Bernoulli columns."""
    W, c, b, bA, bounds = planted()
    V, H, s, bounds2 = G.CASES[3]
    W2, c2, b2, _ = G.case_params(V, H, s, np.float64)
    return [("planted 24->12 K=3", W, c, b, bA, bounds), ("40->14 K=4 between Bernoulli columns", W2, c2, b2, np.zeros(V), bounds2)]


class GtemperOracle(G.GaisOracle):
    """The checker engine of a layer with groups plus ``temper_grouped`` from the float64 twin (it records its calls)."""

    def __init__(self):
        super().__init__()
        self.temper_calls = []

    def temper_grouped(self, W, hbias, vbias, base_vbias, betas, v, h, rank, n_sweeps, rng, groups, burn_in=0, sweep0=0, path=0,
                       steps_per_launch=0, trace=False, zacc=None, trace_work=False):
        import torch
        import _ptz_np as Z
        bA = np.asarray(base_vbias.numpy() if hasattr(base_vbias, "numpy") else base_vbias, dtype=np.float64)
        self.temper_calls.append(dict(bounds=[int(x) for x in groups.host], base_vbias=bA.copy(), n=int(n_sweeps), burn_in=int(burn_in),
                                      sweep0=int(sweep0), step=int(rng.step), path=int(path), zacc=zacc is not None))
        Wn, cn, bn = W.numpy(), hbias.numpy(), vbias.numpy()
        rank0 = rank.numpy().astype(np.int64)
        r = pt_twin(Wn, cn, bn, bA, groups.host, betas, h.numpy(), int(n_sweeps), int(burn_in), rng.seed, rng.stream_id, rng.step,
                    rank0=rank0, sweep0=int(sweep0), row_offset=rng.row_offset)
        v.copy_(torch.from_numpy(r["v"]).to(v.dtype)); h.copy_(torch.from_numpy(r["h"]).to(h.dtype))
        rank.copy_(torch.from_numpy(r["rank"].astype(np.int32)))
        out = (torch.from_numpy(r["accepted"].astype(np.int32)), torch.from_numpy(r["v_avg"]).to(v.dtype),
               torch.from_numpy(r["h_avg"]).to(h.dtype))
        if trace:
            out += (torch.from_numpy(r["trace_v"]), torch.from_numpy(r["trace_h"]), torch.from_numpy(r["trace_swaps"]))
        if zacc is not None or trace_work:
            works = Z.works_from_trace(Wn, cn, bn, bA, False, betas, r["trace_v"], r["trace_swaps"], rank0=rank0, sweep0=int(sweep0))
            if zacc is not None:
                zacc.copy_(torch.from_numpy(Z.accumulate(works[int(burn_in):], zacc.numpy())))
            if trace_work:
                out += (torch.from_numpy(works),)
        return out


# ---------------------------------------------------------------------------------- what the CPU and the GPU tests share
EXCUSED_SHARE = 0.01        # tests/test_gpu_temper.py


def run_ladder(W, c, b, bA, bounds, betas, M, n, burn_in, seed=SEED, stream=STREAM, step=STEP, chunk=100, dtype=np.float64):
    """``pt_twin`` from h = 0 in chunks of ``chunk`` sweeps (the traces are dropped chunk by chunk): ``(v_avg [M, V] over the
    sweeps from burn_in on, works [n - burn_in, M, R - 1, 2] float64, accepted [R - 1])``."""
    import _ptz_np as Z
    R, (V, H) = len(betas), np.asarray(W).shape
    h, rank, acc, out, v_sum = np.zeros((M * R, H)), None, np.zeros(R - 1, dtype=np.int64), [], np.zeros((M, V))
    for t0 in range(0, n, chunk):
        k = min(chunk, n - t0)
        skip = min(max(burn_in - t0, 0), k)
        r = pt_twin(W, c, b, bA, bounds, betas, h, k, min(skip, k - 1), seed, stream, step + 3 * t0, rank0=rank, sweep0=t0, dtype=dtype)
        w = Z.works_from_trace(W, c, b, bA, False, betas, r["trace_v"], r["trace_swaps"], rank0=rank, sweep0=t0)
        out.append(w[skip:])
        if skip < k:
            v_sum += np.asarray(r["v_avg"], dtype=np.float64) * (k - skip)
        h, rank, acc = r["h"], r["rank"], acc + r["accepted"]
    return v_sum / (n - burn_in), np.concatenate(out), acc


def forced_pair(W, c, b, bA, bounds, betas, h0, n, burn_in, d, sweep0=0):
    """The float64 and the float32 twin along the record ``d`` (trace_v, trace_h, trace_swaps)."""
    kw = dict(forced=(d["trace_v"], d["trace_h"], d["trace_swaps"]), sweep0=sweep0)
    r64 = pt_twin(W, c, b, bA, bounds, betas, h0, n, burn_in, SEED, STREAM, STEP, **kw)
    r32 = pt_twin(W, c, b, bA, bounds, betas, h0, n, burn_in, SEED, STREAM, STEP, dtype=np.float32, **kw)
    return r64, r32


def check_forced(tag, d, r64, r32, bounds, check):
    """The forced-parity criteria of a record ``d`` (the ``_check_forced`` story of tests/test_gpu_temper.py plus the group
    draws' of tests/test_gpu_gais.py).  ``check``: ``_margins.check``."""
    gap_d = float(np.abs(r32["delta"] - r64["delta"]).max())
    gap_v = float(np.abs(r32["v_avg"].astype(np.float64) - r64["v_avg"]).max())
    gap_h = float(np.abs(r32["h_avg"].astype(np.float64) - r64["h_avg"]).max())
    dev_v, dev_h = float(np.abs(d["v_avg"] - r64["v_avg"]).max()), float(np.abs(d["h_avg"] - r64["h_avg"]).max())
    own = r64["logu"] < r64["delta"]
    differ = own != r64["decided"]
    band = np.abs(r64["logu"] - r64["delta"]) < 4 * gap_d
    n_att = r64["decided"].size
    mask = max(TIE, 4.0 * r64["c_gap"])
    near, cap = r64["n_ties"] + r64["group_near"](mask), tie_cap(r64, mask)
    print("%s: float32-vs-float64 gap of the twin delta %.3e v_avg %.3e h_avg %.3e; device v_avg %.3e h_avg %.3e; swap attempts %d, "
          "accepted %d, inside the band %d, excused decisions %d, decisions off outside the band %d; draws %d + %d group draws, C_c "
          "gap %.3e, mask %.3e, worst boundary miss %.3e, near ties %d (cap %d), flips outside the mask %d, group flips %d"
          % (tag, gap_d, gap_v, gap_h, dev_v, dev_h, n_att, int(r64["decided"].sum()), int(band.sum()), int((differ & band).sum()),
             int((differ & ~band).sum()), r64["n_draws"], r64["group_draws"], r64["c_gap"], mask, r64["group_miss"], near, cap,
             r64["flips_outside_mask"], r64["group_flips"]))
    tv = np.asarray(d["trace_v"])
    for lo, hi in sm.spans(bounds):
        assert (tv[:, :, lo:hi].sum(axis=2) == 1.0).all() and np.isin(tv[:, :, lo:hi], (0.0, 1.0)).all(), (tag, lo, hi)
    assert r64["flips_outside_mask"] == 0, "%s: %d samples differ from the twin's own draw away from a tie" % (tag, r64["flips_outside_mask"])
    assert r64["group_miss"] < mask, "%s: a category differs from the twin's %.3e from a boundary (mask %.3e)" % (tag, r64["group_miss"], mask)
    assert near <= cap, (tag, near, cap)
    assert not (differ & ~band).any(), "%s: %d swap decisions differ from the twin's away from a tie" % (tag, (differ & ~band).sum())
    assert (differ & band).sum() <= EXCUSED_SHARE * n_att, (tag, int((differ & band).sum()), n_att)
    # the trace, the state and the counts tell one story
    np.testing.assert_array_equal(d["v"], d["trace_v"][-1])
    np.testing.assert_array_equal(d["h"], d["trace_h"][-1])
    np.testing.assert_array_equal(d["rank"], d["trace_swaps"][-1, :, 0, :])
    np.testing.assert_array_equal(d["accepted"], (d["trace_swaps"][:, :, 1, :-1] == 1).sum(axis=(0, 1)))
    np.testing.assert_array_equal(d["trace_swaps"], r64["trace_swaps"])
    assert (np.sort(d["rank"], axis=1) == np.arange(d["rank"].shape[1])[None]).all(), "the rank map is no permutation"
    check(tag + ": v_avg", dev_v, 4 * gap_v, "pt_v_avg")
    check(tag + ": h_avg", dev_h, 4 * gap_h, "pt_h_avg")
