"""numpy twin of clamped annealed importance sampling on a layer with categorical visible units (mdbn_ais_cond_run_grouped;
TEST-ONLY): ``cais_twin`` of tests/_cais_np.py with a boundary list and the group draw of tests/_gais_np.py -- N data rows, C
chains each (chain m belongs to row m // C); the visible draw of a FREE group is one category of the softmax over its tempered
pre-activations, from ONE uniform at the group's first column; a group is held or free as a whole, by the mask entry at its
FIRST column (``_gclamp_np.group_held``: what the device does for any mask), and a held unit takes ``obs`` after every visible
draw and leaves the bias term of the weight update alone.  A held unit's uniform is drawn and not used.

float64 by default (the weight update is the textbook difference log p*_{beta_k}(v_F) - log p*_{beta_{k-1}}(v_F) of the
conditional family, which on one-hot rows is the Bernoulli expression); ``dtype=numpy.float32``: products, softplus, row sums,
the exponentials, Z and the running sums C_c in float32 in the device's order, the per-chain accumulator a double.  With
``forced=(trace_h, trace_v)`` the twin follows the recorded samples, makes its OWN draw from the recorded state at every
temperature and reports where the two differ -- over the free units only.  ``c_gap``, ``group_miss`` and ``group_near`` are
those of tests/_gclamp_np.py.

``exact_cond_log_Z_grouped`` enumerates the 2^H hidden states; ``GcaisOracle`` is the CPU checker engine with
``ais_conditional_grouped``, so the public classes run without a GPU."""
import numpy as np

import _ais_np as A
import _cais_np as CA
import _gais_np as G
import _gclamp_np as Gc
import _softmax_np as sm
from oracle import philox_np

TIE = A.TIE
TIE_SHARE = Gc.TIE_SHARE


def chain_held(mask, bounds, N, V, C):
    """[N C, V] bool: the clamp of every chain as the device reads it."""
    mask = np.asarray(mask)
    if mask.ndim == 1:
        mask = mask[None, :]
    assert mask.shape in ((1, V), (N, V)), mask.shape
    return np.repeat(Gc.group_held(mask, bounds, N, V), C, axis=0)


def gcais_twin(W, c, b, bA, bounds, betas, obs, mask, C, seed, stream, step, dtype=np.float64, forced=None, gaps=None):
    """Returns dict(logw [N, C] float64, trace_h [K-1, N C, H], trace_v [K, N C, V]; n_draws, n_ties, n_flips,
    flips_outside_mask (hidden and free Bernoulli draws, mask ``TIE``); group_draws, group_boundaries, group_flips, group_miss,
    c_gap, group_near(mask) for the free group draws).  ``gaps``: measure ``c_gap`` and keep what ``group_near`` needs
    (default: only when forced)."""
    f = np.dtype(dtype).type
    f32 = dtype == np.float32
    W, c, b, bA = (np.asarray(a, dtype=dtype) for a in (W, c, b, bA))
    betas = np.asarray(betas, dtype=np.float32)          # the device reads a float32 schedule
    V, H = W.shape
    K = betas.size - 1
    obs = np.asarray(obs, dtype=np.float32)              # ... and float32 observed values
    N = obs.shape[0]
    M = N * C
    groups, bern = sm.spans(bounds), sm.bernoulli_columns(bounds, V)
    held = chain_held(mask, bounds, N, V, C)
    free = ~held
    free_g = np.stack([free[:, lo] for lo, _ in groups], axis=1) if groups else np.zeros((M, 0), dtype=bool)
    obs_m = np.repeat(obs, C, axis=0).astype(dtype)
    db = b - bA
    gaps = forced is not None if gaps is None else gaps
    stat = dict(n_draws=0, n_ties=0, n_flips=0, flips_outside_mask=0, group_draws=0, group_boundaries=0, group_flips=0,
                group_miss=0.0, c_gap=0.0)
    nearest = []                                         # per visible draw: [M, G] distance of u to the nearest boundary (inf: held)

    def u(st, cols):
        return philox_np.uniform(M, cols, seed, stream, st, 0, 0)

    def bernoulli(p, uu, record, counted):
        own = (uu < p).astype(dtype)
        tie = (np.abs(uu.astype(np.float64) - p.astype(np.float64)) < TIE) & counted
        stat["n_draws"] += int(counted.sum())
        stat["n_ties"] += int(tie.sum())
        if record is None:
            return own
        flip = (record != own) & counted
        stat["n_flips"] += int(flip.sum())
        stat["flips_outside_mask"] += int((flip & ~tie).sum())
        return record.astype(dtype)

    def draw_v(beta, m, st, record):
        pre = ((bA + f(beta) * db) + f(beta) * m).astype(dtype)
        U = u(st, V)
        if f32:
            Cs = G.running_sums(pre, bounds, np.float32)
            own = G.pick(Cs, bounds, U)
        else:
            own = sm.grouped_sample(sm.grouped_softmax(pre, bounds)[0], bounds, U)
            Cs = G.running_sums(pre, bounds, np.float64) if (gaps or record is not None) else None
        v = own.astype(dtype)
        if bern.size:
            rec_b = None if record is None else record[:, bern]
            v[:, bern] = bernoulli(A.sigmoid(pre[:, bern]), U[:, bern], rec_b, free[:, bern])
        stat["group_draws"] += int(free_g.sum())
        stat["group_boundaries"] += int(sum(free_g[:, g].sum() * (hi - lo - 1) for g, (lo, hi) in enumerate(groups)))
        if gaps and groups:
            C64 = G.running_sums(pre.astype(np.float64), bounds, np.float64)
            C32 = G.running_sums(pre.astype(np.float32), bounds, np.float32)
            near = np.full((M, len(groups)), np.inf)
            for g, (lo, hi) in enumerate(groups):
                fr = free_g[:, g]
                if not fr.any():
                    continue
                stat["c_gap"] = max(stat["c_gap"], float(np.abs(C32[fr, lo:hi - 1].astype(np.float64) - C64[fr, lo:hi - 1]).max()))
                near[fr, g] = np.abs(U[fr, lo:lo + 1].astype(np.float64) - C64[fr, lo:hi - 1]).min(axis=1)
            nearest.append(near)
        if record is not None:
            rec = np.asarray(record, dtype=np.float64)
            for g, (lo, hi) in enumerate(groups):
                fr = free_g[:, g]
                assert np.isin(rec[fr, lo:hi], (0.0, 1.0)).all() and (rec[fr, lo:hi].sum(axis=1) == 1.0).all(), \
                    "free group [%d, %d) does not hold exactly one 1" % (lo, hi)
                mine, theirs = own[:, lo:hi].argmax(axis=1), rec[:, lo:hi].argmax(axis=1)
                for r in np.nonzero((mine != theirs) & fr)[0]:
                    stat["group_flips"] += 1
                    between = slice(lo + min(mine[r], theirs[r]), lo + max(mine[r], theirs[r]))
                    stat["group_miss"] = max(stat["group_miss"], float(np.abs(np.float64(U[r, lo]) - Cs[r, between]).max()))
                v[fr, lo:hi] = rec[fr, lo:hi]
        return np.where(held, obs_m, v)

    th, tv = (None, None) if forced is None else forced
    all_h = np.ones((M, H), dtype=bool)
    logw = np.zeros(M, dtype=np.float64)
    trace_h = np.zeros((max(K - 1, 0), M, H), dtype=dtype)
    trace_v = np.zeros((K, M, V), dtype=dtype)
    v = draw_v(0.0, np.zeros((M, V), dtype=dtype), step, None if tv is None else tv[0])
    for k in range(1, K + 1):
        trace_v[k - 1] = v
        b1, b0 = betas[k], betas[k - 1]
        a = (v @ W + c).astype(dtype)
        B1, B0 = float(b1), float(b0)
        if f32:         # the device's regrouping: hidden share + (b1 - b0) s1 over the free units, float32 sums
            hsum = (A.softplus(f(b1) * a) - A.softplus(f(b0) * a)).sum(axis=1, dtype=np.float32)
            s1 = np.where(free, v * db, f(0)).sum(axis=1, dtype=np.float32)
            logw += hsum.astype(np.float64) + (B1 - B0) * s1.astype(np.float64)
        else:
            logw += (CA.log_pstar_free(v, free, W, c, bA + B1 * db, B1, False)
                     - CA.log_pstar_free(v, free, W, c, bA + B0 * db, B0, False))
        if k == K:
            break
        h = bernoulli(A.sigmoid(f(b1) * a), u(step + 2 * k - 1, H), None if th is None else th[k - 1], all_h)
        trace_h[k - 1] = h
        v = draw_v(b1, (h @ W.T).astype(dtype), step + 2 * k, None if tv is None else tv[k])

    def group_near(width):
        return int(sum((x < width).sum() for x in nearest))
    return dict(logw=logw.reshape(N, C), trace_h=trace_h, trace_v=trace_v, group_near=group_near, **stat)


def near_ties(r):
    """(mask, near ties, cap) of a run ``r`` measured with ``gaps``: the mask max(4e-6, 4 c_gap) of a group boundary, the
    hidden and Bernoulli draws within TIE plus the free group draws with a boundary within the mask, and ``_gais_np.tie_cap``."""
    mask = max(TIE, 4.0 * r["c_gap"])
    return mask, r["n_ties"] + r["group_near"](mask), G.tie_cap(r, mask)


def exact_cond_log_Z_grouped(W, c, b, bounds, obs_row, held_row):
    """Exact log Z_r of the layer with the units where ``held_row`` (constant on groups) is set held at ``obs_row``, float64:
    log sum_h exp(h . c + h . (W_O^T v_O) + sum_{free Bernoulli i} softplus(b_i + W_i h) + sum_{free groups g}
    logsumexp_{c in g} (b_c + W_c h)) over the 2^H hidden states."""
    W, c, b, obs_row = (np.asarray(a, dtype=np.float64) for a in (W, c, b, obs_row))
    held = np.asarray(held_row) != 0
    V, H = W.shape
    assert H <= 20
    for lo, hi in sm.spans(bounds):
        assert (held[lo:hi] == held[lo]).all(), "the mask splits the group [%d, %d)" % (lo, hi)
    groups = [(lo, hi) for lo, hi in sm.spans(bounds) if not held[lo]]
    bern = np.array([i for i in sm.bernoulli_columns(bounds, V) if not held[i]], dtype=np.int64)
    c_r = c + np.where(held, obs_row, 0.0) @ W
    terms = []
    for start in range(0, 1 << H, 1 << 12):
        n = np.arange(start, min(1 << H, start + (1 << 12)))
        h = ((n[:, None] >> np.arange(H)[None, :]) & 1).astype(np.float64)
        act = b[None, :] + h @ W.T
        t = h @ c_r + np.logaddexp(0.0, act[:, bern]).sum(axis=1)
        for lo, hi in groups:
            t += np.logaddexp.reduce(act[:, lo:hi], axis=1)
        terms.append(t)
    t = np.concatenate(terms)
    return float(t.max() + np.log(np.exp(t - t.max()).sum()))


def exact_cond_log_p_grouped(W, c, b, bounds, v_row, held_row):
    """Exact log p(v_F | v_O) of one row (one-hot in its free groups, 0 / 1 in its free Bernoulli columns), float64:
    log p*_1(v_F) - log Z_r."""
    W, c, b, v = (np.asarray(a, dtype=np.float64) for a in (W, c, b, v_row))
    free = (np.asarray(held_row) == 0)[None, :]
    return float(CA.log_pstar_free(v[None, :], free, W, c, b, 1.0, False)[0]) - exact_cond_log_Z_grouped(W, c, b, bounds, v_row, held_row)


def log_Z_base_rows(bA, H, bounds, mask, N):
    """log Z_A,r [N] = H log 2 + sum_{free Bernoulli i} softplus(b_A,i) + sum_{free groups g} logsumexp_{c in g} b_A,c, float64;
    a group is free when the mask at its first column is 0."""
    bA = np.asarray(bA, dtype=np.float64)
    V = bA.size
    free = ~chain_held(mask, bounds, N, V, 1)
    bern = sm.bernoulli_columns(bounds, V)
    out = H * np.log(2.0) + np.where(free[:, bern], np.logaddexp(0.0, bA[bern])[None, :], 0.0).sum(axis=1)
    for lo, hi in sm.spans(bounds):
        out = out + np.where(free[:, lo], np.logaddexp.reduce(bA[lo:hi]), 0.0)
    return out


def estimate_rows(logw, bA, mask, H, bounds):
    """(log Z_r [N], delta-method standard error [N]) from the log weights [N, C], float64."""
    logw = np.asarray(logw, dtype=np.float64)
    N, C = logw.shape
    top = logw.max(axis=1)
    w = np.exp(logw - top[:, None])
    return log_Z_base_rows(bA, H, bounds, mask, N) + top + np.log(w.mean(axis=1)), w.std(axis=1) / (w.mean(axis=1) * np.sqrt(C))


# ------------------------------------------------------------------------------------------------------------------ cases
# ground truth: the four brute-force cases of tests/_gais_np.py, N_ROWS rows with the masks of _gclamp_np.inputs (row 0 holds
# every unit, row 1 none), CHAINS chains per row, N_BETAS temperatures
CASES = G.CASES
N_ROWS, CHAINS, N_BETAS = 8, 256, 1000
STREAM, STEP = G.STREAM, G.STEP
# Philox seed of a case's run (stream 3, step 11), and of its run with ONE group free: seeds under which the float64 twin ALONE
# meets every row's exact value within 4 standard errors and 0.05 nats (tests/test_gcais_twin.py asserts it), so that on the
# device only the kernel can break it
CASE_SEEDS = {24: 1, 100: 1, 70: 1, 40: 1}
ONE_FREE_SEEDS = {24: 1, 100: 1, 70: 1, 40: 1}
# forced parity (tests/test_gpu_gcais.py): the cases of _gclamp_np.PARITY, (data rows N, chains per row C)
PARITY = Gc.PARITY
SHAPES = [(16, 4), (7, 3)]
SEED = G.SEED


def ground_truth_inputs(V, bounds):
    """(v [N_ROWS, V], mask [N_ROWS, V]) of a ground-truth case, from ``_gclamp_np.inputs(V, bounds, N_ROWS, True)``: its
    masks; a free unit holds the 0 / 1 start state (one-hot groups), a held one the observed values (one-hot groups,
    probabilities in (0, 1) on the Bernoulli columns)."""
    v0, obs, mask = Gc.inputs(V, bounds, N_ROWS, True)
    return np.where(mask != 0, obs, v0).astype(np.float32), mask


def one_free_inputs(V, bounds, group=0):
    """One 0 / 1 row with one-hot groups and a [1, V] mask that frees group ``group`` alone."""
    row = sm.one_hot_data(np.random.RandomState(11), 1, V, bounds, p=0.5).astype(np.float32)
    mask = np.ones((1, V), dtype=np.float32)
    lo, hi = sm.spans(bounds)[group]
    mask[:, lo:hi] = 0.0
    return row, mask


def layer(eng, V, H, bounds, W, c, b, seed, stream=STREAM, step=STEP):
    """An ``RBM`` with ``visible_groups`` on ``eng`` whose next draw is the twin's (seed, stream, step)."""
    import mdbn_amd
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(seed), engine=eng,
                       visible_groups=bounds)
    rbm.W.set_value(W); rbm.hbias.set_value(c); rbm.vbias.set_value(b)
    rbm.stream_id, rbm._rng_step = stream, step
    return rbm


def clamp_inputs(N, V, bounds, mask_rows, seed=11):
    """Observed rows of a parity case (real values everywhere: a held unit need not be 0 / 1) and unit masks, about half the
    units held: one row per data row (the first holds every unit, the second none) or one row for all."""
    obs = np.random.RandomState(seed).uniform(size=(N, V)).astype(np.float32)
    return obs, Gc.unit_mask(V, bounds, rows=N if mask_rows != 1 else None)


# ------------------------------------------------------------------------------------------------------------------ checker engine
class GcaisOracle(Gc.GclampOracle):
    """The checker engine of a layer with groups and clamped Gibbs sampling plus ``ais_conditional_grouped`` from the float64
    twin."""

    def ais_conditional_grouped(self, W, hbias, vbias, base_vbias, betas, obs, mask, n_chains, rng, groups, path=0, trace=False,
                                state=False):
        obs, mask = (np.asarray(getattr(x, "numpy", lambda x=x: x)()) for x in (obs, mask))
        r = gcais_twin(W.numpy(), hbias.numpy(), vbias.numpy(), np.asarray(base_vbias, dtype=np.float64), groups.host, betas, obs,
                       mask, int(n_chains), rng.seed, rng.stream_id, rng.step, gaps=False)
        out = (r["logw"],)
        if trace:
            out += (r["trace_h"], r["trace_v"])
        if state:
            out += (r["trace_v"][-1],)
        return out if len(out) > 1 else out[0]
