"""numpy twin of log Z from the tempering ladder (csrc/mdbn_temper.hip, include/mdbn_hip.h: mdbn_pt_run_z; TEST-ONLY).

The sweep itself is tests/_temper_np.py's ``pt_twin`` (imported, not restated).  This module restates what mdbn_pt_run_z adds:

    the works of the attempted pair (rho, rho + 1), held by the slots i / j when the sweep draws v:
        d_fwd = l_i(beta_{rho+1}) - l_i(beta_rho)        d_rev = l_j(beta_rho) - l_j(beta_{rho+1})
    ``works_from_trace`` in float64: the DEFINITION, four evaluations of l; with ``dtype=numpy.float32``: the device's
    regrouping (float32 row sums hsum and s1, g = |b - b_A|^2 in double from the float32 differences, combined in double):
        d_fwd = hsum_i + db s1_i - [Gaussian] (beta_hi^2 - beta_lo^2) g / 2,    d_rev = hsum_j - db s1_j + [Gaussian] ...
    the accumulator ``accumulate``: m' = max(m, d), s = s exp(m - m') + exp(d - m') (s double, the exponentials float32)
    the host finish ``ratios`` / ``estimate``: per pair log mean exp d_fwd, -log mean exp d_rev, their mean ("mid"), Bennett's
    acceptance ratio ("bar", bisection) and the delete-one-ladder jackknife -- all from the works themselves, float64.

Brute-force log Z and log Z of beta = 0 are tests/_ais_np.py's."""
import numpy as np

import _temper_np as T
from _ais_np import brute_log_Z, log_Z_base, softplus          # noqa: F401  (re-exported for the tests)


def works_from_trace(W, c, b, bA, gauss, betas, trace_v, trace_swaps, rank0=None, sweep0=0, dtype=np.float64):
    """``[n, M, R - 1, 2]`` float64: (d_fwd, d_rev) of every attempted pair of the recorded sweeps, NaN elsewhere.
    ``trace_v`` [n, M R, V] is the visible draw of a sweep, ``trace_swaps`` [n, M, 2, R] the rank map AFTER its swap."""
    f32 = dtype == np.float32
    W, c, b, bA = (np.asarray(x, dtype=dtype) for x in (W, c, b, bA))
    betas = np.asarray(betas, dtype=np.float32).astype(dtype)
    n, MR, V = trace_v.shape
    R = betas.size
    M = MR // R
    db = (b - bA).astype(dtype)
    g = float((db.astype(np.float64) ** 2).sum())
    lad = np.arange(M)
    rank = np.tile(np.arange(R), (M, 1)) if rank0 is None else np.asarray(rank0, dtype=np.int64)
    out = np.full((n, M, R - 1, 2), np.nan)

    def ell(v, a, beta):
        bias = bA + beta * db
        vis = -0.5 * ((v - bias[None, :]) ** 2).sum(axis=1) if gauss else v @ bias
        return softplus(beta * a).sum(axis=1) + vis

    for t in range(n):
        v = np.asarray(trace_v[t], dtype=dtype)
        a = (v @ W + c).astype(dtype)
        inv = np.argsort(rank, axis=1)
        for rho in range((sweep0 + t) % 2, R - 1, 2):
            i, j = lad * R + inv[:, rho], lad * R + inv[:, rho + 1]
            b_lo, b_hi = betas[rho], betas[rho + 1]
            if not f32:
                out[t, :, rho, 0] = ell(v[i], a[i], b_hi) - ell(v[i], a[i], b_lo)
                out[t, :, rho, 1] = ell(v[j], a[j], b_lo) - ell(v[j], a[j], b_hi)
                continue
            hs_i = (softplus(b_hi * a[i]) - softplus(b_lo * a[i])).astype(dtype).sum(axis=1, dtype=dtype).astype(np.float64)
            hs_j = (softplus(b_lo * a[j]) - softplus(b_hi * a[j])).astype(dtype).sum(axis=1, dtype=dtype).astype(np.float64)
            s1_i = (((v[i] - bA[None, :]) if gauss else v[i]) * db[None, :]).astype(dtype).sum(axis=1, dtype=dtype).astype(np.float64)
            s1_j = (((v[j] - bA[None, :]) if gauss else v[j]) * db[None, :]).astype(dtype).sum(axis=1, dtype=dtype).astype(np.float64)
            B_lo, B_hi = np.float64(b_lo), np.float64(b_hi)
            gq = 0.5 * (B_hi * B_hi - B_lo * B_lo) * g if gauss else 0.0
            out[t, :, rho, 0] = hs_i + (B_hi - B_lo) * s1_i - gq
            out[t, :, rho, 1] = hs_j - (B_hi - B_lo) * s1_j + gq
        rank = np.asarray(trace_swaps[t][:, 0, :], dtype=np.int64)
    return out


def new_zacc(M, R):
    z = np.zeros((M, R - 1, 4))
    z[:, :, 0::2] = -np.inf
    return z


def accumulate(works, zacc=None):
    """The device's recurrence over ``works`` [n, M, R - 1, 2] in sweep order: zacc [M, R - 1, 4] = {m_f, s_f, m_r, s_r}."""
    n, M, P, _ = works.shape
    z = new_zacc(M, P + 1) if zacc is None else np.array(zacc, dtype=np.float64)
    e32 = lambda x: np.exp(x.astype(np.float32)).astype(np.float64)
    for t in range(n):
        for k in (0, 1):
            d = works[t, :, :, k]
            on = ~np.isnan(d)
            m0, s0 = z[:, :, 2 * k], z[:, :, 2 * k + 1]
            dd = np.where(on, d, 0.0)
            m1 = np.maximum(m0, dd)
            with np.errstate(invalid="ignore"):
                s1 = s0 * e32(m0 - m1) + e32(dd - m1)
            z[:, :, 2 * k] = np.where(on, m1, m0)
            z[:, :, 2 * k + 1] = np.where(on, s1, s0)
    return z


def _lse(x, axis):
    top = x.max(axis=axis, keepdims=True)
    return np.squeeze(top, axis=axis) + np.log(np.exp(x - top).sum(axis=axis))


def zacc_log_sums(zacc):
    """log sum exp d per (ladder, pair, direction) [M, R - 1, 2] from the accumulators."""
    with np.errstate(divide="ignore"):
        return np.stack([zacc[:, :, 0] + np.log(zacc[:, :, 1]), zacc[:, :, 2] + np.log(zacc[:, :, 3])], axis=2)


def direct_log_sums(works):
    """The same from the works themselves: a float64 logsumexp over the sweeps."""
    n, M, P, _ = works.shape
    out = np.empty((M, P, 2))
    for p in range(P):
        w = works[~np.isnan(works[:, 0, p, 0]), :, p, :]            # [n_p, M, 2]
        out[:, p, :] = _lse(w, 0)
    return out


def bar_root(df, dr, iters=60):
    """Bennett's log ratio r from equally many forward and reverse works: sum_R f(-d_rev - r) = sum_F f(r - d_fwd),
    f(x) = 1 / (1 + exp x); the difference rises in r: bisection between the extremes of d_fwd and -d_rev."""
    lo, hi = min(df.min(), (-dr).min()), max(df.max(), (-dr).max())
    for _ in range(iters):
        r = 0.5 * (lo + hi)
        with np.errstate(over="ignore"):
            gap = (1.0 / (1.0 + np.exp(-dr - r))).sum() - (1.0 / (1.0 + np.exp(r - df))).sum()
        if gap > 0:
            hi = r
        else:
            lo = r
    return 0.5 * (lo + hi)


def ratios(works, method, ladders=None):
    """Per pair [R - 1]: the estimate of log Z_{rho+1} / Z_rho by ``method`` in ("fwd", "rev", "mid", "bar") from the works of
    the ladders ``ladders`` (None: all), pooled over sweeps and ladders."""
    P = works.shape[2]
    out = np.empty(P)
    for p in range(P):
        w = works[~np.isnan(works[:, 0, p, 0]), :, p, :]
        if ladders is not None:
            w = w[:, ladders, :]
        df, dr = w[:, :, 0].ravel(), w[:, :, 1].ravel()
        fwd = _lse(df, 0) - np.log(df.size)
        rev = -(_lse(dr, 0) - np.log(dr.size))
        out[p] = dict(fwd=fwd, rev=rev, mid=0.5 * (fwd + rev)).get(method) if method != "bar" else bar_root(df, dr, 40)
    return out


def estimate(works, log_z0, method="mid", jackknife=True):
    """``(log Z, delete-one-ladder jackknife standard error)`` by ``method`` from the works [n, M, R - 1, 2], float64."""
    M = works.shape[1]
    est = log_z0 + ratios(works, method).sum()
    if not jackknife:
        return float(est), float("nan")
    left = np.array([ratios(works, method, np.delete(np.arange(M), m)).sum() for m in range(M)])
    return float(est), float(np.sqrt((M - 1.0) / M * ((left - left.mean()) ** 2).sum()))


def run_works(W, c, b, bA, gauss, betas, M, n, burn_in, seed, stream=3, step=11, chunk=100, dtype=np.float64):
    """``pt_twin`` from h = 0 in chunks of ``chunk`` sweeps (its traces are dropped chunk by chunk) and the float64 works of the
    sweeps from ``burn_in`` on: ``(works [n - burn_in, M, R - 1, 2], accepted [R - 1])``."""
    R, H = len(betas), np.asarray(W).shape[1]
    h, rank, acc, out = np.zeros((M * R, H)), None, np.zeros(R - 1, dtype=np.int64), []
    for t0 in range(0, n, chunk):
        k = min(chunk, n - t0)
        r = T.pt_twin(W, c, b, bA, gauss, betas, h, k, 0, seed, stream, step + 3 * t0, rank0=rank, sweep0=t0, dtype=dtype)
        w = works_from_trace(W, c, b, bA, gauss, betas, r["trace_v"], r["trace_swaps"], rank0=rank, sweep0=t0)
        out.append(w[max(burn_in - t0, 0):])
        h, rank, acc = r["h"], r["rank"], acc + r["accepted"]
    return np.concatenate(out), acc
