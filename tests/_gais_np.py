"""numpy twin of annealed importance sampling on a layer with categorical visible units (mdbn_ais_run_grouped; TEST-ONLY):
``ais_twin`` of tests/_ais_np.py with a boundary list.  The run is the Bernoulli run -- on one-hot rows log p*_beta(v) =
sum_j softplus(beta a_j(v)) + v . b_beta -- except for the visible draw of a group: one category of the softmax over the
group's tempered pre-activations, from ONE uniform at the group's first column (``grouped_softmax`` / ``grouped_sample`` of
tests/_softmax_np.py).  ``brute_log_Z`` enumerates the hidden states; ``GaisOracle`` is the CPU checker engine with
``ais_grouped``, so the public classes run without a GPU.

float64 by default; ``dtype=numpy.float32``: products, softplus, row sums, the exponentials, Z and the running sum C_c in
float32 in the device's order, the per-chain accumulator a double.  With ``forced=(trace_h, trace_v)`` the twin follows the
recorded samples, makes its OWN draw from the recorded state at every temperature and reports where the two differ.  A
group draw has K - 1 boundaries C_0 .. C_{K-2}; ``c_gap`` is the largest |C_c(float32) - C_c(float64)| the run met on its own
inputs, and ``group_miss`` the largest distance of a uniform from a boundary that separates a recorded category from the
twin's own."""
import numpy as np

import _ais_np as A
import _softmax_np as sm
from oracle import philox_np

TIE = A.TIE


def log_Z_base(bA, H, bounds):
    """log Z_A = H log 2 + sum_{Bernoulli i} softplus(b_A,i) + sum_g logsumexp_{c in g} b_A,c, float64."""
    bA = np.asarray(bA, dtype=np.float64)
    out = H * np.log(2.0) + np.logaddexp(0.0, bA[sm.bernoulli_columns(bounds, bA.size)]).sum()
    for lo, hi in sm.spans(bounds):
        out += np.logaddexp.reduce(bA[lo:hi])
    return float(out)


def estimate(logw, bA, H, bounds):
    """(log Z, delta-method standard error) from per-chain log weights, float64."""
    logw = np.asarray(logw, dtype=np.float64)
    top = logw.max()
    w = np.exp(logw - top)
    return float(log_Z_base(bA, H, bounds) + top + np.log(w.mean())), float(w.std() / (w.mean() * np.sqrt(w.size)))


def running_sums(pre, bounds, dtype):
    """C [B, V]: inside a group the running sum of its softmax means in ascending c, in ``dtype`` and the device's order
    (max, e = exp(x - max), Z = the ascending sum, mean = e / Z, C = the ascending sum); elsewhere sigmoid(pre)."""
    pre = np.asarray(pre, dtype=dtype)
    C = A.sigmoid(pre).astype(dtype)
    for lo, hi in sm.spans(bounds):
        x = pre[:, lo:hi]
        e = np.exp(x - x.max(axis=1, keepdims=True)).astype(dtype)
        Z = np.cumsum(e, axis=1, dtype=dtype)[:, -1:]
        C[:, lo:hi] = np.cumsum((e / Z).astype(dtype), axis=1, dtype=dtype)
    return C


def pick(C, bounds, U):
    """The sample under the uniforms U from the running sums C: the first c of a group with u < C_c, the last when none
    qualifies (u: the group's first column); a Bernoulli column is u < C."""
    sample = (U < C).astype(np.float64)
    for lo, hi in sm.spans(bounds):
        below = U[:, lo:lo + 1] < C[:, lo:hi]
        cat = np.where(below.any(axis=1), below.argmax(axis=1), hi - lo - 1)
        sample[:, lo:hi] = 0.0
        sample[np.arange(C.shape[0]), lo + cat] = 1.0
    return sample


def ais_twin(W, c, b, bA, bounds, betas, M, seed, stream, step, dtype=np.float64, forced=None, row_offset=0, gaps=None):
    """Returns dict(logw [M] float64, trace_h [K-1, M, H], trace_v [K, M, V], n_draws, n_ties, n_flips, flips_outside_mask
    (hidden and Bernoulli draws, mask ``TIE``), and for the group draws: group_draws, group_boundaries (K - 1 per draw),
    group_flips, group_miss, c_gap, group_near(mask) -> the number of group draws with a boundary within ``mask`` of the
    uniform).  ``gaps``: measure ``c_gap`` and keep what ``group_near`` needs (default: only when forced)."""
    f = np.dtype(dtype).type
    f32 = dtype == np.float32
    W, c, b, bA = (np.asarray(a, dtype=dtype) for a in (W, c, b, bA))
    betas = np.asarray(betas, dtype=np.float32)          # the device reads a float32 schedule
    V, H = W.shape
    K = betas.size - 1
    db = b - bA
    groups, bern = sm.spans(bounds), sm.bernoulli_columns(bounds, V)
    gaps = forced is not None if gaps is None else gaps
    stat = dict(n_draws=0, n_ties=0, n_flips=0, flips_outside_mask=0, group_draws=0, group_boundaries=0, group_flips=0,
                group_miss=0.0, c_gap=0.0)
    nearest = []                                         # per visible draw: [M, G] distance of u to the nearest boundary

    def u(st, cols):
        return philox_np.uniform(M, cols, seed, stream, st, 0, row_offset)

    def bernoulli(p, uu, record):
        own = (uu < p).astype(dtype)
        tie = np.abs(uu.astype(np.float64) - p.astype(np.float64)) < TIE
        stat["n_draws"] += own.size
        stat["n_ties"] += int(tie.sum())
        if record is None:
            return own
        flip = record != own
        stat["n_flips"] += int(flip.sum())
        stat["flips_outside_mask"] += int((flip & ~tie).sum())
        return record.astype(dtype)

    def draw_v(beta, m, st, record):
        pre = ((bA + f(beta) * db) + f(beta) * m).astype(dtype)
        U = u(st, V)
        if f32:
            C = running_sums(pre, bounds, np.float32)
            own = pick(C, bounds, U)
        else:
            own = sm.grouped_sample(sm.grouped_softmax(pre, bounds)[0], bounds, U)
            C = running_sums(pre, bounds, np.float64) if (gaps or record is not None) else None
        v = own.astype(dtype)
        if bern.size:
            rec_b = None if record is None else record[:, bern]
            v[:, bern] = bernoulli(A.sigmoid(pre[:, bern]), U[:, bern], rec_b)
        stat["group_draws"] += M * len(groups)
        stat["group_boundaries"] += M * sum(hi - lo - 1 for lo, hi in groups)
        if gaps and groups:
            C64 = running_sums(pre.astype(np.float64), bounds, np.float64)
            C32 = running_sums(pre.astype(np.float32), bounds, np.float32)
            near = np.empty((M, len(groups)))
            for g, (lo, hi) in enumerate(groups):
                stat["c_gap"] = max(stat["c_gap"], float(np.abs(C32[:, lo:hi - 1].astype(np.float64) - C64[:, lo:hi - 1]).max()))
                near[:, g] = np.abs(U[:, lo:lo + 1].astype(np.float64) - C64[:, lo:hi - 1]).min(axis=1)
            nearest.append(near)
        if record is not None:
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
        return v

    th, tv = (None, None) if forced is None else forced
    logw = np.zeros(M, dtype=np.float64)
    trace_h = np.zeros((max(K - 1, 0), M, H), dtype=dtype)
    trace_v = np.zeros((K, M, V), dtype=dtype)
    v = draw_v(0.0, np.zeros((M, V), dtype=dtype), step, None if tv is None else tv[0])
    for k in range(1, K + 1):
        trace_v[k - 1] = v
        b1, b0 = betas[k], betas[k - 1]
        a = (v @ W + c).astype(dtype)
        B1, B0 = float(b1), float(b0)
        if f32:         # the device's regrouping: hidden share + (b1 - b0) s1, float32 sums
            hsum = (A.softplus(f(b1) * a) - A.softplus(f(b0) * a)).sum(axis=1, dtype=np.float32)
            s1 = (v * db).sum(axis=1, dtype=np.float32)
            logw += hsum.astype(np.float64) + (B1 - B0) * s1.astype(np.float64)
        else:
            logw += A.log_pstar(v, W, c, bA + B1 * db, B1, False) - A.log_pstar(v, W, c, bA + B0 * db, B0, False)
        if k == K:
            break
        h = bernoulli(A.sigmoid(f(b1) * a), u(step + 2 * k - 1, H), None if th is None else th[k - 1])
        trace_h[k - 1] = h
        v = draw_v(b1, (h @ W.T).astype(dtype), step + 2 * k, None if tv is None else tv[k])

    def group_near(mask):
        return int(sum((n < mask).sum() for n in nearest))
    return dict(logw=logw, trace_h=trace_h, trace_v=trace_v, group_near=group_near, **stat)


def tie_cap(r, mask):
    """3 + E + 4 sqrt(E) (the rule of tests/_step_forms.py ``draw_cap``): E = the expected number of draws of the run ``r``
    within a mask of a boundary -- 2 TIE per hidden or Bernoulli draw, 2 ``mask`` per boundary of a group draw."""
    E = 2.0 * TIE * r["n_draws"] + 2.0 * mask * r["group_boundaries"]
    return int(3 + E + 4.0 * np.sqrt(E))


def brute_log_Z(W, c, b, bounds):
    """Exact log Z by enumerating the 2^H hidden states: h . c + sum_Bern logaddexp(0, act) + sum_g logsumexp(act_g), float64."""
    W, c, b = (np.asarray(a, dtype=np.float64) for a in (W, c, b))
    V, H = W.shape
    assert H <= 20
    bern, groups = sm.bernoulli_columns(bounds, V), sm.spans(bounds)
    terms = []
    for lo in range(0, 1 << H, 1 << 12):
        n = np.arange(lo, min(1 << H, lo + (1 << 12)))
        h = ((n[:, None] >> np.arange(H)[None, :]) & 1).astype(np.float64)
        act = b[None, :] + h @ W.T
        t = h @ c + np.logaddexp(0.0, act[:, bern]).sum(axis=1)
        for g0, g1 in groups:
            t += np.logaddexp.reduce(act[:, g0:g1], axis=1)
        terms.append(t)
    t = np.concatenate(terms)
    return float(t.max() + np.log(np.exp(t - t.max()).sum()))


CASES = [   # V, H, scale of W, boundaries  (the four ground-truth cases)
    (24, 12, 0.5, list(range(0, 25, 3))),
    (100, 16, 0.3, list(range(0, 101, 5))),
    (70, 12, 0.3, [1, 3, 67, 70]),
    (40, 14, 0.4, list(range(4, 37, 4))),
]
# Philox seed of the twin's run of a case (stream 3, step 11): one under which the float64 twin alone meets the exact value
# within 4 standard errors and 0.05 nats (tests/test_gais_twin.py asserts it)
CASE_SEEDS = {24: 5, 100: 5, 70: 5, 40: 5}


def case_params(V, H, s, dtype=np.float32):
    rs = np.random.RandomState(7)
    W = rs.normal(0, s, (V, H))
    c, b = rs.normal(0, 0.5, H), rs.normal(0, 0.5, V)
    bA = rs.normal(0, 0.3, V)
    return tuple(np.asarray(a, dtype=dtype) for a in (W, c, b, bA))


# the forced-parity cases of tests/test_gpu_gais.py: V, H, scale of W, boundaries, paths; seed of the run (a case keeps its
# seed only while the twin alone stays under the tie cap: tests/test_gais_twin.py)
PARITY = [
    (100, 24, 0.3, list(range(0, 101, 5)), (1, 2)),
    (70, 24, 0.3, [1, 3, 67, 70], (1, 2)),
    (1024, 256, 0.02, list(range(0, 1025, 4)), (2,)),
]
PARITY_M = (64, 22)
SEED, STREAM, STEP = 5, 3, 11


def parity_params(V, H, s, seed=3):
    rs = np.random.RandomState(seed)
    W = rs.normal(0, s, (V, H)).astype(np.float32)
    c, b = rs.normal(0, 0.5, H).astype(np.float32), rs.normal(0, 0.5, V).astype(np.float32)
    bA = (b + rs.normal(0, 0.3, V)).astype(np.float32)
    return W, c, b, bA


class GaisOracle(sm.GroupedOracle):
    """The checker engine of a layer with groups plus ``ais_grouped`` from the float64 twin."""

    def ais_grouped(self, W, hbias, vbias, base_vbias, betas, n_chains, rng, groups, path=0, trace=False):
        r = ais_twin(W.numpy(), hbias.numpy(), vbias.numpy(), np.asarray(base_vbias, dtype=np.float64), groups.host, betas,
                     int(n_chains), rng.seed, rng.stream_id, rng.step, row_offset=rng.row_offset, gaps=False)
        return (r["logw"], r["trace_h"], r["trace_v"]) if trace else r["logw"]
