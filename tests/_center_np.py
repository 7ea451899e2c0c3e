"""float64 twin of the centred-gradient kernels (mdbn_center_offsets / mdbn_center_stats; TEST-ONLY) and the centred CD
step written out on oracle/rbm_np.py (Melchior, Fischer & Wiskott 2016, Algorithm 1, for a layer kept in its ordinary
parameters)."""
import numpy as np

from oracle import rbm_np


def center_offsets(mu, lam, v0, ph, nu):
    """-> (mu', lam'): the offsets slid towards the column means of v0 / ph by nu (nu = 1: the means themselves)."""
    v0, ph = np.asarray(v0, dtype=np.float64), np.asarray(ph, dtype=np.float64)
    mu, lam = np.asarray(mu, dtype=np.float64), np.asarray(lam, dtype=np.float64)
    return mu + nu * (v0.mean(axis=0) - mu), lam + nu * (ph.mean(axis=0) - lam)


def center_stats(S, s_h, s_v, mu, lam, rho):
    """-> (S', s_h', s_v'): S' = S - mu s_h' - s_v lam', s_h' = s_h - rho S'^T mu, s_v' = s_v - rho S' lam."""
    S, s_h, s_v, mu, lam = (np.asarray(x, dtype=np.float64) for x in (S, s_h, s_v, mu, lam))
    S2 = S - np.outer(mu, s_h) - np.outer(s_v, lam)
    return S2, s_h - rho * (S2.T @ mu), s_v - rho * (S2 @ lam)


def centered_product(v0, ph, nv, nh, mu, lam):
    """The statistics matrix formed from centred units directly: sum_r (v0 - mu)(ph - lam)' - (nv - mu)(nh - lam)'."""
    return (v0 - mu).T @ (ph - lam) - (nv - mu).T @ (nh - lam)


def unpack(stats, V, H, ldv, ldh):
    """(S [V, H], s_h [H], s_v [V], cost [4]) views' copies of a packed [V ldh | ldh | ldv | 4] buffer (float64)."""
    st = np.asarray(stats, dtype=np.float64)
    return (st[:V * ldh].reshape(V, ldh)[:, :H].copy(), st[V * ldh:V * ldh + H].copy(),
            st[V * ldh + ldh:V * ldh + ldh + V].copy(), st[V * ldh + ldh + ldv:V * ldh + ldh + ldv + 4].copy())


def centered_update(s, offsets, v0, ph, nv, nh, nu, batch_size, lr, lambda_1=0.0, lambda_2=0.0, weightcost=0.0, momentum=0.0,
                    strict_reference=True):
    """One centred update of the state ``s`` from the means of a CD chain; ``offsets``: (mu, lam) or None (the first
    centred step: the batch means).  -> the new (mu, lam)."""
    n = v0.shape[0]
    if offsets is None:
        mu, lam = center_offsets(np.zeros(v0.shape[1]), np.zeros(ph.shape[1]), v0, ph, 1.0)
    else:
        mu, lam = center_offsets(offsets[0], offsets[1], v0, ph, nu)
    S, s_h, s_v = rbm_np.cd_statistics(v0, ph, nv, nh)
    S, s_h, s_v = center_stats(S, s_h, s_v, mu, lam, float(n) / float(batch_size))
    g = rbm_np.rbm_grad(s, S, s_h, s_v, batch_size, n, weightcost, strict_reference=strict_reference)
    rbm_np.apply_update(s, g[0], g[1], g[2], lr, lambda_1, lambda_2, momentum)
    return mu, lam
