"""numpy twin of the device's annealed importance sampling (csrc/mdbn_ais.hip; TEST-ONLY).

``ais_twin`` restates the run of mdbn_ais_run -- Salakhutdinov & Murray 2008 with a base-rate model, unit-variance Gaussian
or Bernoulli visibles -- with the device's draw addressing (oracle/philox_np.py: v_1 at step s, hidden draw of temperature k
at s + 2k - 1, visible draw at s + 2k, draw index 0).  In float64 (the default) the weight update is the textbook difference
log p*_{beta_k}(v_k) - log p*_{beta_{k-1}}(v_k); with ``dtype=numpy.float32`` products, softplus and row sums are float32 in
the device's regrouping and only the per-chain accumulator is a double: the gap between the two on the same samples is the
float32 share of the device's error (tests/test_gpu_ais.py takes its tolerance from it).

With ``forced=(trace_h, trace_v)`` the twin follows the device's recorded samples: at every temperature it still makes its
OWN draw from the recorded state, and reports where that draw differs from the record and how close to a tie it was."""
import numpy as np

from oracle import philox_np

TIE = 4e-6          # near-tie mask of the drift tests (tests/test_gpu_surface.py): |u - p| below it may fall either way


def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    # exp(-x) may overflow to +inf on a saturated layer (float32: from x = -88.7 down): 1 / (1 + inf) = 0 is the right limit
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def log_pstar(v, W, c, b_beta, beta, gauss):
    """log p*_beta(v) (include/mdbn_hip.h), float64."""
    bias = -0.5 * ((v - b_beta) ** 2).sum(axis=1) if gauss else v @ b_beta
    return softplus(beta * (v @ W + c)).sum(axis=1) + bias


def log_Z_base(bA, H, gauss):
    bA = np.asarray(bA, dtype=np.float64)
    return H * np.log(2.0) + (0.5 * bA.size * np.log(2.0 * np.pi) if gauss else np.logaddexp(0.0, bA).sum())


def estimate(logw, bA, H, gauss):
    """(log Z, delta-method standard error) from per-chain log weights, float64."""
    logw = np.asarray(logw, dtype=np.float64)
    top = logw.max()
    w = np.exp(logw - top)
    return float(log_Z_base(bA, H, gauss) + top + np.log(w.mean())), float(w.std() / (w.mean() * np.sqrt(w.size)))


def ais_twin(W, c, b, bA, gauss, betas, M, seed, stream, step, dtype=np.float64, forced=None, row_offset=0):
    """Returns dict(logw [M] float64, trace_h [K-1, M, H], trace_v [K, M, V], n_draws, n_ties, n_flips,
    flips_outside_mask, max_v_diff)."""
    f = np.dtype(dtype).type
    f32 = dtype == np.float32
    W, c, b, bA = (np.asarray(a, dtype=dtype) for a in (W, c, b, bA))
    betas = np.asarray(betas, dtype=np.float32)          # the device reads a float32 schedule
    V, H = W.shape
    K = betas.size - 1
    db = b - bA
    d2 = (db * db).sum(dtype=dtype)
    stat = dict(n_draws=0, n_ties=0, n_flips=0, flips_outside_mask=0, max_v_diff=0.0)

    def u(st, cols, normal_bit=False):
        return philox_np.uniform(M, cols, seed, stream, st, philox_np.NORMAL_BIT if normal_bit else 0, row_offset)

    def draw_v(beta, m, st, record):
        pre = (bA + f(beta) * db) + f(beta) * m
        if gauss:
            u1, u2 = u(st, V).astype(np.float64), u(st, V, True).astype(np.float64)
            z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
            v = (pre + z.astype(dtype)).astype(dtype)
            if record is not None:
                stat["max_v_diff"] = max(stat["max_v_diff"], float(np.abs(record - v).max()))
                v = record.astype(dtype)
            return v
        return bernoulli(sigmoid(pre), u(st, V), record)

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

    th, tv = (None, None) if forced is None else forced
    logw = np.zeros(M, dtype=np.float64)
    trace_h = np.zeros((max(K - 1, 0), M, H), dtype=dtype)
    trace_v = np.zeros((K, M, V), dtype=dtype)
    v = draw_v(0.0, np.zeros((M, V), dtype=dtype), step, None if tv is None else tv[0])
    for k in range(1, K + 1):
        trace_v[k - 1] = v
        b1, b0 = betas[k], betas[k - 1]
        a = (v @ W + c).astype(dtype)
        if f32:         # the device's regrouping: hidden share + (b1 - b0) s1 - (b1^2 - b0^2) / 2 * d2, float32 sums
            hsum = (softplus(f(b1) * a) - softplus(f(b0) * a)).sum(axis=1, dtype=np.float32)
            s1 = (((v - bA) if gauss else v) * db).sum(axis=1, dtype=np.float32)
            B1, B0 = float(b1), float(b0)
            logw += hsum.astype(np.float64) + (B1 - B0) * s1.astype(np.float64)
            if gauss:
                logw -= 0.5 * (B1 * B1 - B0 * B0) * float(d2)
        else:
            B1, B0 = float(b1), float(b0)
            logw += log_pstar(v, W, c, bA + B1 * db, B1, gauss) - log_pstar(v, W, c, bA + B0 * db, B0, gauss)
        if k == K:
            break
        h = bernoulli(sigmoid(f(b1) * a), u(step + 2 * k - 1, H), None if th is None else th[k - 1])
        trace_h[k - 1] = h
        v = draw_v(b1, (h @ W.T).astype(dtype), step + 2 * k, None if tv is None else tv[k])
    return dict(logw=logw, trace_h=trace_h, trace_v=trace_v, **stat)


def brute_log_Z(W, c, b, gauss):
    """Exact log Z by enumerating the 2^H hidden states (Gaussian visibles integrate in closed form), float64."""
    W, c, b = (np.asarray(a, dtype=np.float64) for a in (W, c, b))
    V, H = W.shape
    assert H <= 20
    terms = []
    for lo in range(0, 1 << H, 1 << 12):
        n = np.arange(lo, min(1 << H, lo + (1 << 12)))
        h = ((n[:, None] >> np.arange(H)[None, :]) & 1).astype(np.float64)
        act = b[None, :] + h @ W.T
        if gauss:
            t = h @ c + 0.5 * (act ** 2).sum(axis=1) - 0.5 * (b ** 2).sum() + 0.5 * V * np.log(2.0 * np.pi)
        else:
            t = h @ c + np.logaddexp(0.0, act).sum(axis=1)
        terms.append(t)
    t = np.concatenate(terms)
    return float(t.max() + np.log(np.exp(t - t.max()).sum()))


CASES = [   # V, H, scale of W, gauss  (the issue's four ground-truth cases)
    (24, 12, 0.5, False), (100, 16, 0.3, False), (20, 10, 0.25, True), (40, 14, 0.2, True)]


def case_params(V, H, s, gauss, dtype=np.float32):
    rs = np.random.RandomState(7)
    W = rs.normal(0, s, (V, H))
    c, b = rs.normal(0, 0.5, H), rs.normal(0, 0.5, V)
    bA = b.copy() if gauss else rs.normal(0, 0.3, V)
    return tuple(np.asarray(a, dtype=dtype) for a in (W, c, b, bA))
