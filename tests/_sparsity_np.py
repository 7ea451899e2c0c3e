"""float64 twin of the sparsity-target kernels (mdbn_sparsity_activity / mdbn_sparsity_stats; TEST-ONLY) and the sparse CD
step written out on oracle/rbm_np.py (Hinton's practical guide, section 11; Nair & Hinton 2009; Lee, Ekanadham & Ng 2008),
with an optional centred stage after it (tests/_center_np.py)."""
import numpy as np

import _center_np as cn
from oracle import rbm_np


def activity(q, v0, ph, rate):
    """-> (q', v_mean): the estimate slid towards the column means of ph by rate (rate = 1: the means themselves), and the
    column means of v0 (None without v0)."""
    ph, q = np.asarray(ph, dtype=np.float64), np.asarray(q, dtype=np.float64)
    return q + rate * (ph.mean(axis=0) - q), None if v0 is None else np.asarray(v0, dtype=np.float64).mean(axis=0)


def stats(S, s_h, s_v, q, v_mean, target, w_scale, b_scale):
    """-> (S', s_h', s_v): with t = target - q, S' = S + w_scale v_mean t', s_h' = s_h + b_scale t (w_scale = 0: S as it is)."""
    S, s_h, s_v, q = (np.asarray(x, dtype=np.float64) for x in (S, s_h, s_v, q))
    t = target - q
    if w_scale != 0.0:
        S = S + np.outer(w_scale * np.asarray(v_mean, dtype=np.float64), t)
    return S, s_h + b_scale * t, s_v


def sparse_update(s, state, v0, ph, nv, nh, batch_size, lr, target, cost, decay=0.9, weights=True, centered=False, nu=0.01,
                  lambda_1=0.0, lambda_2=0.0, weightcost=0.0, momentum=0.0, strict_reference=True):
    """One sparse (and, with ``centered``, centred) update of the state ``s`` from the means of a CD chain.  ``state``: the
    dict {"q": ..., "offsets": (mu, lam)} the previous step returned, or None (the layer's first such step: q and the offsets
    start at the batch means).  -> the new dict."""
    n = v0.shape[0]
    state = dict(state or {})
    first = state.get("q") is None
    q, v_mean = activity(np.zeros(ph.shape[1]) if first else state["q"], v0 if weights else None, ph, 1.0 if first else 1.0 - decay)
    S, s_h, s_v = rbm_np.cd_statistics(v0, ph, nv, nh)
    S, s_h, s_v = stats(S, s_h, s_v, q, v_mean, target, cost * batch_size if weights else 0.0, cost * n)
    state["q"] = q
    if centered:
        if state.get("offsets") is None:
            mu, lam = cn.center_offsets(np.zeros(v0.shape[1]), np.zeros(ph.shape[1]), v0, ph, 1.0)
        else:
            mu, lam = cn.center_offsets(state["offsets"][0], state["offsets"][1], v0, ph, nu)
        S, s_h, s_v = cn.center_stats(S, s_h, s_v, mu, lam, float(n) / float(batch_size))
        state["offsets"] = (mu, lam)
    g = rbm_np.rbm_grad(s, S, s_h, s_v, batch_size, n, weightcost, strict_reference=strict_reference)
    rbm_np.apply_update(s, g[0], g[1], g[2], lr, lambda_1, lambda_2, momentum)
    return state


# ---------------------------------------------------------------------------------------------- the behaviour cases
# What the penalty is for, on a layer small enough for the float64 oracle: (gauss, steps, hyper-parameters of the update).
# 200 rows, minibatches of 20 taken in order, momentum 0.5 then 0.9 from step 100.  tests/test_sparsity_twin.py runs them on
# the oracle, tests/test_gpu_sparsity.py on the device through the public classes, both against the same bounds.
BEHAVIOUR_V, BEHAVIOUR_H, BEHAVIOUR_ROWS, BEHAVIOUR_B = 100, 24, 200, 20
BEHAVIOUR = {
    "bernoulli": dict(gauss=False, steps=400, lr=0.1, hyper=dict(weightcost=2e-4)),
    "gaussian": dict(gauss=True, steps=600, lr=0.005, hyper=dict(lambda_2=0.1)),
}


def behaviour_data(gauss):
    rs = np.random.RandomState(2008)
    shape = (BEHAVIOUR_ROWS, BEHAVIOUR_V)
    return rs.normal(size=shape) if gauss else (rs.uniform(size=shape) < 0.3).astype(np.float64)


def behaviour_batch(t):
    per_epoch = BEHAVIOUR_ROWS // BEHAVIOUR_B
    return np.arange(BEHAVIOUR_B) + BEHAVIOUR_B * (t % per_epoch)


def behaviour_momentum(t):
    return 0.5 if t < 100 else 0.9


def behaviour_on_the_oracle(case, seed=7, stream=1, **sparsity):
    """-> per-unit mean activation over all rows after the run; ``sparsity``: target=, cost=, decay=, weights= (none: plain CD)."""
    from oracle.philox_np import PhiloxDraws
    c = BEHAVIOUR[case]
    data = behaviour_data(c["gauss"])
    s = rbm_np.RBMState(BEHAVIOUR_V, BEHAVIOUR_H, numpy_rng=np.random.RandomState(123), gauss=c["gauss"])
    if c["hyper"].get("weightcost"):
        s.freeze_W0()
    state = None
    for t in range(c["steps"]):
        v0 = data[behaviour_batch(t)]
        if sparsity:
            ph, _, out = rbm_np.cd_chain(s, v0, PhiloxDraws(seed, stream, t, 0), 1)
            state = sparse_update(s, state, v0, ph, out[1], out[4], BEHAVIOUR_B, c["lr"], momentum=behaviour_momentum(t),
                                  **dict(c["hyper"], **sparsity))
        else:
            rbm_np.cd_step(s, v0, PhiloxDraws(seed, stream, t, 0), lr=c["lr"], k=1, batch_size=BEHAVIOUR_B,
                           momentum=behaviour_momentum(t), **c["hyper"])
    return rbm_np.propup(s, data)[1].mean(axis=0)


# (case, keywords of the penalty; {}: plain CD) -> what the float64 oracle measured with exactly these inputs: the largest
# |activation - target| over the units of a sparse run, the SMALLEST over the units of a plain run.  The tests assert a sparse
# run within twice its figure and a plain run at least half its figure away, on the oracle and on the device alike.
BEHAVIOUR_RUNS = [
    ("bernoulli", {}, 0.3, 0.1775),                                           # plain CD: activations 0.008 .. 0.123
    ("bernoulli", dict(target=0.3, cost=1.0, decay=0.9), 0.3, 0.0432),        # 0.257 .. 0.316
    ("bernoulli", dict(target=0.3, cost=3.0, decay=0.9, weights=False), 0.3, 0.2568),     # bias only: 0.043 .. 0.306
    ("gaussian", {}, 0.2, 0.2525),                                            # plain CD: 0.453 .. 0.532
    ("gaussian", dict(target=0.2, cost=5.0, decay=0.9), 0.2, 0.0224),         # 0.209 .. 0.222
]


def behaviour_holds(activations, sparsity, target, measured):
    """-> (figure, ok): the figure of BEHAVIOUR_RUNS for these activations and whether it meets the bound."""
    dev = np.abs(np.asarray(activations, dtype=np.float64) - target)
    return (dev.max(), dev.max() <= 2.0 * measured) if sparsity else (dev.min(), dev.min() >= 0.5 * measured)
