"""numpy twin of the device's clamped annealed importance sampling (csrc/mdbn_ais.hip under a clamp; TEST-ONLY).

``cais_twin`` restates the run of mdbn_ais_cond_run with the conventions of ``_ais_np.ais_twin``: N data rows, C chains each
(chain m belongs to row m // C), the visibles where ``mask`` is 1 held at ``obs`` after every visible draw, the bias term of
the weight update over the free columns only.  The Philox addressing is ais_twin's (oracle/philox_np.py, the global chain
row): a held column's uniform is drawn and not used.  In float64 (the default) the weight update is the textbook difference
log p*_{beta_k}(v_F) - log p*_{beta_{k-1}}(v_F) of the conditional family; with ``dtype=numpy.float32`` products, softplus
and row sums are float32 in the device's regrouping (s1 over the free columns, d2 per mask row).  With
``forced=(trace_h, trace_v)`` the twin follows the device's recorded samples; ties, flips and the Gaussian draw's distance
are counted over the FREE columns only (a held column is no draw).  With a zero mask every operation is ais_twin's own on
the same numbers, so the float64 log weights are equal to ais_twin's exactly."""
import numpy as np

import _ais_np as A
from oracle import philox_np


def _held(mask, N, V, C):
    mask = np.asarray(mask)
    if mask.ndim == 1:
        mask = mask[None, :]
    assert mask.shape in ((1, V), (N, V)), mask.shape
    return np.repeat(np.broadcast_to(mask != 0, (N, V)), C, axis=0)


def log_pstar_free(v, free, W, c, b_beta, beta, gauss):
    """log p*_beta(v_F) of the conditional family (include/mdbn_hip.h), float64: ``_ais_np.log_pstar`` with the bias term
    over the free columns -- a(v) = v W + c is taken over the whole row."""
    bias = -0.5 * np.where(free, (v - b_beta) ** 2, 0.0).sum(axis=1) if gauss else np.where(free, v, 0.0) @ b_beta
    return A.softplus(beta * (v @ W + c)).sum(axis=1) + bias


def cais_twin(W, c, b, bA, gauss, betas, obs, mask, C, seed, stream, step, dtype=np.float64, forced=None):
    """Returns dict(logw [N, C] float64, trace_h [K-1, N C, H], trace_v [K, N C, V], n_draws, n_ties, n_flips,
    flips_outside_mask, max_v_diff)."""
    f = np.dtype(dtype).type
    f32 = dtype == np.float32
    W, c, b, bA = (np.asarray(a, dtype=dtype) for a in (W, c, b, bA))
    betas = np.asarray(betas, dtype=np.float32)          # the device reads a float32 schedule
    V, H = W.shape
    K = betas.size - 1
    obs = np.asarray(obs, dtype=np.float32)              # ... and float32 observed values
    N = obs.shape[0]
    M = N * C
    held = _held(mask, N, V, C)
    free = ~held
    obs_m = np.repeat(obs, C, axis=0).astype(dtype)
    db = b - bA
    d2 = np.where(free, db * db, f(0)).sum(axis=1, dtype=dtype)            # [M]: per chain, its mask row's
    stat = dict(n_draws=0, n_ties=0, n_flips=0, flips_outside_mask=0, max_v_diff=0.0)

    def u(st, cols, normal_bit=False):
        return philox_np.uniform(M, cols, seed, stream, st, philox_np.NORMAL_BIT if normal_bit else 0, 0)

    def bernoulli(p, uu, record, counted):
        own = (uu < p).astype(dtype)
        tie = np.abs(uu.astype(np.float64) - p.astype(np.float64)) < A.TIE
        stat["n_draws"] += int(counted.sum())
        stat["n_ties"] += int((tie & counted).sum())
        if record is None:
            return own
        flip = (record != own) & counted
        stat["n_flips"] += int(flip.sum())
        stat["flips_outside_mask"] += int((flip & ~tie).sum())
        return record.astype(dtype)

    def draw_v(beta, m, st, record):
        pre = (bA + f(beta) * db) + f(beta) * m
        if gauss:
            u1, u2 = u(st, V).astype(np.float64), u(st, V, True).astype(np.float64)
            z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
            v = (pre + z.astype(dtype)).astype(dtype)
            if record is not None:
                if free.any():
                    stat["max_v_diff"] = max(stat["max_v_diff"], float(np.abs(record - v)[free].max()))
                v = record.astype(dtype)
        else:
            v = bernoulli(A.sigmoid(pre), u(st, V), record, free)
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
        if f32:         # the device's regrouping: hidden share + (b1 - b0) s1 - (b1^2 - b0^2) / 2 * d2, float32 sums
            hsum = (A.softplus(f(b1) * a) - A.softplus(f(b0) * a)).sum(axis=1, dtype=np.float32)
            s1 = np.where(free, ((v - bA) if gauss else v) * db, f(0)).sum(axis=1, dtype=np.float32)
            logw += hsum.astype(np.float64) + (B1 - B0) * s1.astype(np.float64)
            if gauss:
                logw -= 0.5 * (B1 * B1 - B0 * B0) * d2.astype(np.float64)
        else:
            logw += log_pstar_free(v, free, W, c, bA + B1 * db, B1, gauss) - log_pstar_free(v, free, W, c, bA + B0 * db, B0, gauss)
        if k == K:
            break
        h = bernoulli(A.sigmoid(f(b1) * a), u(step + 2 * k - 1, H), None if th is None else th[k - 1], all_h)
        trace_h[k - 1] = h
        v = draw_v(b1, (h @ W.T).astype(dtype), step + 2 * k, None if tv is None else tv[k])
    return dict(logw=logw.reshape(N, C), trace_h=trace_h, trace_v=trace_v, **stat)


def exact_cond_log_Z(W, c, b, obs_row, mask_row, gauss):
    """Exact log Z_r of the layer with the columns where ``mask_row`` is 1 held at ``obs_row``: the RBM over the free columns
    with hidden bias c + v_O W_O, by enumeration (``_ais_np.brute_log_Z``), float64."""
    W, c, b, obs_row = (np.asarray(a, dtype=np.float64) for a in (W, c, b, obs_row))
    held = np.asarray(mask_row) != 0
    return A.brute_log_Z(W[~held], c + np.where(held, obs_row, 0.0) @ W, b[~held], gauss)


def exact_cond_log_p(W, c, b, v_row, mask_row, gauss):
    """Exact log p(v_F | v_O) of one row, float64: log p*_1(v_F) - log Z_r."""
    W, c, b, v = (np.asarray(a, dtype=np.float64) for a in (W, c, b, v_row))
    free = (np.asarray(mask_row) == 0)[None, :]
    return float(log_pstar_free(v[None, :], free, W, c, b, 1.0, gauss)[0]) - exact_cond_log_Z(W, c, b, v_row, mask_row, gauss)


def estimate_rows(logw, bA, mask, H, gauss):
    """(log Z_r [N], delta-method standard error [N]) from the log weights [N, C], float64: the host finish per data row,
    with the base-rate model over the row's free columns."""
    logw = np.asarray(logw, dtype=np.float64)
    N, C = logw.shape
    bA = np.asarray(bA, dtype=np.float64)
    free = ~_held(mask, N, bA.size, 1)
    per_col = np.full(bA.size, 0.5 * np.log(2.0 * np.pi)) if gauss else np.logaddexp(0.0, bA)
    log_ZA = H * np.log(2.0) + np.where(free, per_col[None, :], 0.0).sum(axis=1)
    top = logw.max(axis=1)
    w = np.exp(logw - top[:, None])
    return log_ZA + top + np.log(w.mean(axis=1)), w.std(axis=1) / (w.mean(axis=1) * np.sqrt(C))


def block_masks(N, V, seed=0):
    """Per-row block masks over half the columns: row r holds the V // 2 columns (cyclically) from a start of its own."""
    rs = np.random.RandomState(seed)
    mask = np.zeros((N, V), dtype=np.float32)
    for r in range(N):
        mask[r, (rs.randint(V) + np.arange(V // 2)) % V] = 1.0
    return mask


def observed(N, V, gauss, seed=0):
    """Observed rows of the ground-truth cases: 0 / 1 (Bernoulli) or N(0, 1) (Gaussian) entries."""
    rs = np.random.RandomState(100 + seed)
    return rs.normal(size=(N, V)).astype(np.float32) if gauss else (rs.uniform(size=(N, V)) < 0.5).astype(np.float32)
