"""float64 twin of the learned per-column variance of a Gaussian layer (mdbn_sigma_scale_rows / mdbn_sigma_update; TEST-ONLY)
and the model behind it written out on oracle/rbm_np.py: with s = log sigma and u = x exp(-s), p(x) = p_u(u) exp(-sum s), where
p_u is the unit-variance GRBM of (W, hbias, vbias) -- so F(x) = F_u(u) + sum(s), log Z is p_u's, and the gradient of the mean
log-likelihood with respect to s_i is mean_r[u_ri (u_ri - m_ri)] - 1, m = vbias + p(h = 1 | u) W^T."""
import itertools

import numpy as np

from oracle import rbm_np

LOG_SIGMA_RANGE = (-4.6, 4.6)


def scale_rows(src, idx, log_sigma, sign):
    """-> src[idx] * exp(sign * log_sigma) (idx None: every row)."""
    src = np.asarray(src, dtype=np.float64)
    rows = src if idx is None else src[np.asarray(idx)]
    return rows * np.exp(sign * np.asarray(log_sigma, dtype=np.float64))[None, :]


def cond_mean(s, U):
    """m = vbias + p(h = 1 | u) W^T for the rows ``U`` in units; ``s``: an rbm_np.RBMState."""
    return rbm_np.propup(s, U)[1] @ s.W.T + s.vbias


def grad(U, M, n_rows=None):
    """-> (g, scale): g_i = mean_r[U_ri (U_ri - M_ri)] - 1 over the first n_rows rows, and mean_r |U (U - M)| per column (what
    the statistics tolerance is relative to)."""
    U, M = np.asarray(U, dtype=np.float64), np.asarray(M, dtype=np.float64)
    n = U.shape[0] if n_rows is None else int(n_rows)
    t = U[:n] * (U[:n] - M[:n])
    return t.sum(axis=0) / n - 1.0, np.abs(t).mean(axis=0)


def update(log_sigma, speed, g, lr, momentum, lo=LOG_SIGMA_RANGE[0], hi=LOG_SIGMA_RANGE[1]):
    """The visible bias's rule (oracle/rbm_np.py:271-285) on log_sigma, clamped: -> (log_sigma', speed')."""
    log_sigma, speed = np.asarray(log_sigma, dtype=np.float64), np.asarray(speed, dtype=np.float64)
    return np.clip(log_sigma + speed * lr, lo, hi), g + (speed - g) * momentum


def free_energy(s, x, log_sigma):
    """F(x) = F_u(x exp(-log_sigma)) + sum(log_sigma) of the raw rows ``x``."""
    log_sigma = np.asarray(log_sigma, dtype=np.float64)
    return rbm_np.free_energy(s, scale_rows(x, None, log_sigma, -1.0)) + log_sigma.sum()


def log_z_unit(s):
    """Exact log Z of the unit-variance GRBM, by enumeration of the hidden states:
    log sum_h exp(c.h + b.Wh + |Wh|^2 / 2) + (V / 2) log 2 pi."""
    V, H = s.W.shape
    terms = []
    for bits in itertools.product((0.0, 1.0), repeat=H):
        h = np.asarray(bits)
        wh = s.W @ h
        terms.append(s.hbias @ h + s.vbias @ wh + 0.5 * wh @ wh)
    terms = np.asarray(terms)
    return float(terms.max() + np.log(np.exp(terms - terms.max()).sum()) + 0.5 * V * np.log(2.0 * np.pi))


def log_likelihood(s, x, log_sigma):
    """Exact mean log p(x) over the rows."""
    return float(np.mean(-free_energy(s, x, log_sigma)) - log_z_unit(s))


def state(V, H, seed, scale=0.5):
    """A small Gaussian layer with all three parameters away from zero."""
    rs = np.random.RandomState(seed)
    return rbm_np.RBMState(V, H, W=rs.normal(size=(V, H)) * scale, hbias=rs.normal(size=H) * scale, vbias=rs.normal(size=V) * scale,
                           gauss=True)


def fixed_point_problem():
    """The full-batch fixed point: 32 rows of 64 columns drawn as N(0, e^{2t}), t ~ U(-1.5, 1.5) per column.  With W = 0,
    lr = 0, vbias = 0 the conditional mean is 0 and g_i = exp(-2 s_i) mean_r x_ri^2 - 1 vanishes at s_i = log(mean x_i^2) / 2.
    -> (x, the fixed point)"""
    rs = np.random.RandomState(64)
    t = rs.uniform(-1.5, 1.5, size=64)
    x = rs.normal(size=(32, 64)) * np.exp(t)[None, :]
    x = x.astype(np.float32).astype(np.float64)
    return x, 0.5 * np.log((x ** 2).mean(axis=0))
