"""The two whole-step loops of the newest step variants (TEST-ONLY): a GRBM whose step learns a per-column variance
(``learn_sigma``) and a Bernoulli RBM with categorical visible units (``visible_groups``), each run through the public classes
on the device and followed by its float64 twin teacher-forced along the device's recorded chain (tests/_sigma_np.py,
tests/_softmax_np.py, tests/_center_np.py, tests/_sparsity_np.py on oracle/rbm_np.py).

``run_sigma`` / ``run_grouped`` take the form of the run as keywords -- the engine (with its options set), chain taps on or
off, the ``next_indexes`` hint, a persistent chain, a ragged schedule of row counts, the residency of the table and the form of
the index lists -- and return a ``Run``: the layer, the twin's state, the worst deviations, and the bits of everything a
second run is compared with.  With the taps off there is no recorded chain to follow: the run returns the device's results
only.  tests/test_gpu_sigma.py and tests/test_gpu_softmax.py call them with the arguments their own loops had."""
import types

import numpy as np

import _center_np as cn
import _sigma_np as sg
import _softmax_np as sm
import _sparsity_np as sn
from _margins import check
from oracle import rbm_np
from oracle.philox_np import PhiloxDraws

STEPS = 4
MOMENTA = (0.5, 0.5, 0.9, 0.9)
PARAMS = ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed")
SIGMA_NAMES = PARAMS + ("log_sigma", "log_sigma_speed")
TILED_F32 = dict(stream_x6=0, skinny_gemm=0, gemm_bf16x6=0, small_fused=0, thin_fused=0)      # (tests/test_gpu_center.py's)
RAGGED = (33, 33, 13, 33)       # rows of the four steps of a ragged run at batch_size = 33

# sigma
ETA, SIGMA_LR, SIGMA_L2 = 0.05, 0.002, 0.1
SPARSITY = dict(sparsity_target=0.2, sparsity_cost=1.0, sparsity_decay=0.9)
SIGMA_KEYWORDS = dict(alone={}, centered=dict(centered=True, offset_rate=0.05), sparse=SPARSITY,
                      both=dict(SPARSITY, centered=True, offset_rate=0.05))
# grouped
GROUPED_HP = dict(lr=0.1, weightcost=2e-4)


class Run(types.SimpleNamespace):
    pass


def set_options(eng, opts):
    for key, value in (opts or {}).items():
        if key == "planes_min_work":
            eng.set_planes_min_work(value)
        else:
            eng.set_option(key, value)
    return eng


def index_lists(eng, rs, N, sizes, form):
    """One index list per entry of ``sizes`` (and one more, for the hint of the last step), drawn from ``rs``: ``form`` None
    -- what ``engine.index_tensor`` makes of a permutation --, "int32" / "int64" -- a device tensor of that type --, "list" --
    a Python list whose last entry repeats its first.  -> (what the step function is given, the same values as host arrays)"""
    import torch
    given, host = [], []
    for n in list(sizes) + [sizes[-1]]:
        rows = rs.permutation(N)[:n]
        if form == "list":
            rows = rows.copy()
            rows[-1] = rows[0]
            given.append([int(r) for r in rows])
        elif form in ("int32", "int64"):
            t = torch.from_numpy(rows.astype(np.int32 if form == "int32" else np.int64)).to(eng.device)
            assert t.dtype == (torch.int32 if form == "int32" else torch.int64)
            given.append(t)
        else:
            assert form is None, form
            given.append(eng.index_tensor(rows, N))
        host.append(np.asarray(rows, dtype=np.int64))
    return given, host


def draw_cap(B, V, H, k, bounds=None, persistent=False):
    """Cap on the draws of one step that may differ from the twin's: every one must be a tie, and a draw is a tie with
    probability 2 tol per boundary -- tol = 1e-6 for a hidden unit (``rbm_np.cd_chain_forced``), ``sm.MEAN_TOL`` for a
    Bernoulli visible unit and for each of the K - 1 boundaries of a group (``sm.follow``).  E = the expected count over the
    draws the twin follows; the cap is 3 + E + 4 sqrt(E) (three as the small shapes have it, plus four standard deviations of
    a Poisson count).  Derived from the shape alone."""
    hidden = B * H * (k if not persistent else k + 1)         # h0 .. h_{k-1}, and h_k when the chain is kept
    E = 2.0 * 1e-6 * hidden
    if bounds is not None:
        groups = sm.spans(bounds)
        boundaries = sum(hi - lo - 1 for lo, hi in groups) + len(sm.bernoulli_columns(bounds, V))
        E += 2.0 * sm.MEAN_TOL * B * boundaries * k
    return int(3 + E + 4.0 * np.sqrt(E))


# ------------------------------------------------------------------------------------------------------------------ sigma
def sigma_engine(tapped=True, opts=None):
    """The HIP engine riding the statistics step of a layer with log_sigma: what every cd_step saw and left in its scratch
    (and, with the chain taps on, recorded), and the gradient of every sigma_update (read off a copy: momentum 0 makes the new
    speed g).  Product defaults but for ``opts``."""
    import mdbn_amd

    class SigmaTap(mdbn_amd.HipEngine):
        cd_forward = None           # (as tests/_shadow.py: every CD step goes through cd_step)

        def __init__(self):
            mdbn_amd.HipEngine.__init__(self)
            self.trace_chain = bool(tapped)
            self.rides, self.grads = [], []

        def cd_step(self, data, indexes, W, hbias, vbias, gauss, k, rng, persistent=None, add_noise=False, stats_slot=0,
                    sample_stats=False, stats=None, comm_cus=0, keep_f32=None):
            assert indexes is None and keep_f32 is True
            stats, sc = mdbn_amd.HipEngine.cd_step(self, data, None, W, hbias, vbias, gauss, k, rng, persistent=persistent,
                                                   add_noise=add_noise, stats=stats, keep_f32=keep_f32)
            B, V, H = data.shape[0], W.shape[0], W.shape[1]
            V2, P2 = sc.V2.cpu().numpy().copy(), sc.P2.cpu().numpy().copy()        # [v0 | nv_mean], [ph_mean | -nh_mean]
            assert V2.shape == (2 * B, V) and P2.shape == (2 * B, H)
            self.rides.append(dict(step=rng.step, u=V2[:B], ph=P2[:B], V2=V2, P2=P2,
                                   trace_h=sc.trace_h.cpu().numpy()[:, :, :H].copy() if self.trace_chain else None,
                                   stats=stats.cpu().numpy().copy(), ldv=sc.V2.stride(0), ldh=sc.P2.stride(0),
                                   planes=sc.planes is not None, fed=data.data_ptr()))
            return stats, sc

        def sigma_update(self, U, M, n_rows, lr, momentum, lo, hi, log_sigma, log_sigma_speed):
            s, speed = log_sigma.clone(), log_sigma_speed.clone()
            mdbn_amd.HipEngine.sigma_update(self, U, M, n_rows, 0.0, 0.0, lo, hi, s, speed)
            self.grads.append(speed.cpu().numpy().copy())
            return mdbn_amd.HipEngine.sigma_update(self, U, M, n_rows, lr, momentum, lo, hi, log_sigma, log_sigma_speed)

    return set_options(SigmaTap(), opts)


def sigma_twin_update(st, state, variant, u, ph, nv, nh, B, momentum):
    """One update of the float64 state from the means of a chain, by the transforms' twins (the sparsity target first)."""
    n = u.shape[0]
    S, s_h, s_v = rbm_np.cd_statistics(u, ph, nv, nh)
    if variant in ("sparse", "both"):
        first = state.get("q") is None
        q, v_mean = sn.activity(np.zeros(ph.shape[1]) if first else state["q"], u, ph, 1.0 if first else 1.0 - SPARSITY["sparsity_decay"])
        S, s_h, s_v = sn.stats(S, s_h, s_v, q, v_mean, SPARSITY["sparsity_target"], SPARSITY["sparsity_cost"] * B,
                               SPARSITY["sparsity_cost"] * n)
        state["q"] = q
    if variant in ("centered", "both"):
        first = state.get("offsets") is None
        mu, lam = cn.center_offsets(*((np.zeros(u.shape[1]), np.zeros(ph.shape[1])) if first else state["offsets"]), u, ph,
                                    1.0 if first else 0.05)
        S, s_h, s_v = cn.center_stats(S, s_h, s_v, mu, lam, float(n) / float(B))
        state["offsets"] = (mu, lam)
    g = rbm_np.rbm_grad(st, S, s_h, s_v, B, n, 0.0)
    rbm_np.apply_update(st, g[0], g[1], g[2], SIGMA_LR, 0.0, SIGMA_L2, momentum)


def sigma_table(V, N, seed=31):
    """-> (RandomState after the draw, [N, V] float32 rows N(0, 1) exp(U(-1, 1)) per column)"""
    rs = np.random.RandomState(seed)
    spread = np.exp(rs.uniform(-1.0, 1.0, size=V))
    return rs, (rs.normal(size=(N, V)) * spread[None, :]).astype(np.float32)


def run_sigma(eng, V, H, B, k, error_free, variant, hint=False, persistent=False, schedule=None, resident="device",
              index_form=None, poison_idle_rows=False, timing=False, seed=7):
    """Four steps of a GRBM with ``learn_sigma`` on ``eng`` (a ``sigma_engine``).  ``hint``: every call names the next
    minibatch; ``persistent``: PCD; ``schedule``: rows of each step (default: ``B`` every time); ``resident``: "device" |
    "host"; ``index_form``: see ``index_lists``; ``poison_idle_rows``: before a short step the rows it does not use of the
    full-size staging matrices are set to NaN; ``timing``: record the launch kinds, per step."""
    import mdbn_amd
    sizes = list(schedule) if schedule is not None else [B] * STEPS
    tapped = eng.trace_chain
    N = 2 * B + 7
    rs, data = sigma_table(V, N)
    rbm = mdbn_amd.GRBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(123), theano_rng=mdbn_amd.RandomStreams(seed),
                        error_free=error_free, engine=eng)
    st = rbm_np.RBMState(V, H, W=rbm.W.get_value(), gauss=True)
    chain = None
    if persistent:
        chain = (np.random.RandomState(5).uniform(size=(B, H)) < 0.5).astype(np.float32)
    _, updates = rbm.get_cost_updates(lr=SIGMA_LR, k=k, batch_size=B, lambda_2=SIGMA_L2, learn_sigma=ETA, persistent=chain,
                                      **SIGMA_KEYWORDS[variant])
    table = mdbn_amd.shared(data, engine=eng, resident=resident) if resident != "device" else mdbn_amd.shared(data, engine=eng)
    fn = mdbn_amd.function(updates, table, data_parallel=None)
    given, host = index_lists(eng, rs, N, sizes, index_form)
    ls, ls_speed, state = np.zeros(V), np.zeros(V), {}
    worst = dict(units=0.0, prob=0.0, stat=0.0, g=0.0, cost=0.0)
    r = Run(rbm=rbm, fn=fn, st=st, data=data, worst=worst, state=state, costs=[], scratch=[], kinds=[], flips=[], sizes=sizes,
            plan=updates, tapped=tapped)
    if timing:
        eng.kernel_timing(True)
    try:
        for t, n in enumerate(sizes):
            mom = MOMENTA[t]
            if poison_idle_rows and n < B:
                for m in fn._sigma_rows[B]:
                    m[n:].fill_(float("nan"))
            chain0 = updates.persistent.get_value().astype(np.float64) if persistent else None
            extra = dict(next_indexes=given[t + 1]) if hint else {}
            c = float(fn(indexes=given[t], momentum=mom, **extra))
            r.costs.append(c)
            ride, g_dev = eng.rides[t], eng.grads[t]
            assert ride["step"] == t and len(eng.rides) == t + 1 and len(eng.grads) == t + 1
            assert ride["u"].shape == (n, V) and ride["fed"] == fn._sigma_rows[n][0].data_ptr()
            r.scratch.append((ride["V2"], ride["P2"]))
            if timing:
                seen = [kd for _, _, _, kd in eng.kernel_timing_detail()]
                r.kinds.append(seen[sum(len(s) for s in r.kinds):])
            if not tapped:
                continue
            x = data[host[t]].astype(np.float64)
            u = x * np.exp(-ls)[None, :]                # the twin's rows in units, from the twin's own log_sigma
            worst["units"] = max(worst["units"], float((np.abs(ride["u"] - u) / np.maximum(np.abs(u), 1e-30)).max()))
            ph, _, out, flips = rbm_np.cd_chain_forced(st, u, PhiloxDraws(seed, rbm.stream_id, t), k, ride["trace_h"], None,
                                                       persistent=chain0, tie=1e-6)
            r.flips.append(flips)
            worst["prob"] = max(worst["prob"], float(np.abs(ride["ph"] - ph).max()))
            S, s_h, s_v, _ = cn.unpack(ride["stats"], V, H, ride["ldv"], ride["ldh"])
            for got, want in zip((S, s_h, s_v), rbm_np.cd_statistics(u, ph, out[1], out[4])):
                worst["stat"] = max(worst["stat"], float(np.abs(got - want).max() / max(1.0, np.abs(want).max())))
            if persistent:                              # the pseudo-likelihood of the rows IN UNITS, at the old parameters
                want_cost = rbm_np.pseudo_likelihood_cost(st, u)
                st.bit_i_idx = (st.bit_i_idx + 1) % V
                assert np.array_equal(updates.persistent.get_value(), ride["trace_h"][k]), "chain != recorded nh_sample"
            else:
                want_cost = rbm_np.reconstruction_cost(st, out[0], u)       # the monitoring cost, in units
            worst["cost"] = max(worst["cost"], abs(c - want_cost) / abs(want_cost))
            g, scale = sg.grad(u, ph @ st.W.T + st.vbias)               # at the parameters of before the update
            worst["g"] = max(worst["g"], float((np.abs(g_dev - g) / np.maximum(1.0, scale)).max()))
            sigma_twin_update(st, state, variant, u, ph, out[1], out[4], B, mom)
            ls, ls_speed = sg.update(ls, ls_speed, g, ETA, mom)
        eng.synchronize()
    finally:
        if timing:
            eng.kernel_timing(False)
    r.ls, r.ls_speed = ls, ls_speed
    r.params = {n: getattr(rbm, n).get_value() for n in SIGMA_NAMES}
    for n in ("v_offset", "h_offset", "h_activity"):
        if getattr(rbm, n, None) is not None:
            r.params[n] = getattr(rbm, n).get_value()
    if tapped:
        want = dict({n: getattr(st, n) for n in PARAMS}, log_sigma=ls, log_sigma_speed=ls_speed)
        r.errs = [(n, float(np.abs(r.params[n] - want[n]).max() / max(1.0, np.abs(want[n]).max()))) for n in SIGMA_NAMES]
    return r


def check_sigma(name, r, rel, pcd=False):
    """The bounds of tests/test_gpu_sigma.py on a tapped ``run_sigma``: every figure printed before the first assertion."""
    rbm, st, worst = r.rbm, r.st, r.worst
    held = r.data[:64]
    F_dev = rbm.free_energy(held).get_value().astype(np.float64)
    F_twin = sg.free_energy(st, held.astype(np.float64), r.ls)
    fe = float((np.abs(F_dev - F_twin) / np.maximum(1.0, np.abs(F_twin))).max())
    print("%s: %s; %s; free energy %.3e; draws that differ %s" % (name, ", ".join("%s %.3e" % e for e in r.errs),
                                                               ", ".join("%s %.3e" % kv for kv in sorted(worst.items())), fe, r.flips))
    assert max(r.flips) <= 3
    assert np.abs(r.ls).max() > 1e-3                # (log_sigma moved)
    # one product rounding and expf on top of a log_sigma that may sit 2e-6 from the twin's
    check("sigma step %s: rows in units rel" % name, worst["units"], rel + 2e-6)
    check("sigma step %s: ph_mean in P2" % name, worst["prob"], 2e-6, "prob")
    check("sigma step %s: S, s_h, s_v / max" % name, worst["stat"], 1e-5, "stats")
    check("sigma step %s: g / max(1, mean|u (u - m)|)" % name, worst["g"], 1e-5, "stats")
    if pcd:
        check("sigma step %s (PCD): cost rel" % name, worst["cost"], 1e-4)
    else:
        check("sigma step %s: cost rel" % name, worst["cost"], 1e-5)
    for pname, err in r.errs:
        check("sigma step %s: %s after %d steps / max" % (name, pname, STEPS), err, 2e-6, "update")
    check("sigma step %s: free energy rel" % name, fe, 1e-4, "free_energy")
    if "offsets" in r.state:
        check("sigma step %s: v_offset" % name, np.abs(rbm.v_offset.get_value() - r.state["offsets"][0]).max(), 2e-6)
        check("sigma step %s: h_offset" % name, np.abs(rbm.h_offset.get_value() - r.state["offsets"][1]).max(), 2e-6)
    if "q" in r.state:
        check("sigma step %s: h_activity" % name, np.abs(rbm.h_activity.get_value() - r.state["q"]).max(), 2e-6)


# ------------------------------------------------------------------------------------------------------------------ grouped
def run_grouped(eng, V, H, B, k, groups, persistent, mode, steps=STEPS, hint=True, schedule=None, resident="device",
                index_form=None, tapped=True, timing=False, cap=3, seed=7):
    """``steps`` steps of a Bernoulli RBM with ``visible_groups`` on ``eng``: with the taps on every step is checked against
    the twin at the bounds of tests/test_gpu_center.py as it is made.  ``cap``: draws of one step that may differ from the
    twin's (all of them ties)."""
    import mdbn_amd
    from mdbn_amd.utils import group_boundaries
    sizes = list(schedule) if schedule is not None else [B] * steps
    bounds = group_boundaries(groups, V).tolist()
    N = 3 * B + 7
    rs = np.random.RandomState(31)
    data = sm.one_hot_data(rs, N, V, bounds)
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(123), theano_rng=mdbn_amd.RandomStreams(seed), engine=eng,
                       visible_groups=groups)
    st = rbm_np.RBMState(V, H, W=rbm.W.get_value())
    st.freeze_W0()
    chain = (rs.uniform(size=(B, H)) < 0.5).astype(np.float32) if persistent else None
    _, updates = rbm.get_cost_updates(k=k, batch_size=B, persistent=chain, **dict(GROUPED_HP, **sm.MODE_KEYWORDS[mode]))
    table = mdbn_amd.shared(data, engine=eng, resident=resident) if resident != "device" else mdbn_amd.shared(data, engine=eng)
    fn = mdbn_amd.function(updates, table, data_parallel=None)
    given, host = index_lists(eng, rs, N, sizes, index_form)
    eng.trace_chain = bool(tapped)
    if timing:
        eng.kernel_timing(True)
    state, flips = None, 0
    r = Run(rbm=rbm, fn=fn, st=st, data=data, bounds=bounds, costs=[], scratch=[], kinds=[], sizes=sizes, plan=updates, twin_ties=[])
    try:
        for t, n in enumerate(sizes):
            mom = MOMENTA[t] if steps == STEPS else (0.5 if t < 2 else 0.9)
            chain0 = updates.persistent.get_value().astype(np.float64) if persistent else None
            extra = dict(next_indexes=given[t + 1]) if hint else {}
            c = fn(indexes=given[t], momentum=mom, **extra)
            sc = eng.last_scratch
            V2, P2 = sc.V2.cpu().numpy(), sc.P2.cpu().numpy()
            assert V2.shape[0] == 2 * n
            r.costs.append(float(c))
            r.scratch.append((V2.copy(), P2.copy()))
            if not tapped:
                continue
            v0 = data[host[t]].astype(np.float64)
            ph, _, out, n_differ = sm.cd_chain(st, v0, PhiloxDraws(seed, rbm.stream_id, t), k, bounds, persistent=chain0,
                                               trace_h=sc.trace_h.cpu().numpy()[:, :, :H], trace_v=sc.trace_v.cpu().numpy()[:, :, :V])
            flips += n_differ
            # (the twin alone: visible draws of the last Gibbs step within the means' bound of a boundary -- a seed is kept
            #  only while this count stays under the cap, so that more differing draws than the cap are the device's doing)
            r.twin_ties.append(sm.tie_draws(out[1], bounds, PhiloxDraws(seed, rbm.stream_id, t).u(2 * k - 1, n, V)))
            assert n_differ <= cap, "%d draws of step %d differ from the twin's (cap %d)" % (n_differ, t, cap)
            assert np.array_equal(V2[:n], v0.astype(np.float32)), "rows 0..B-1 of V2 are not v0"
            check("grouped step: ph_mean in P2", np.abs(P2[:n] - ph).max(), 2e-6, "prob")
            check("grouped step: nv_mean in V2", np.abs(V2[n:] - out[1]).max(), 2e-6, "nv_mean")
            check("grouped step: -nh_mean in P2", np.abs(P2[n:] + out[4]).max(), 2e-6, "prob")
            assert np.array_equal(sc.vs.cpu().numpy(), sc.trace_v.cpu().numpy()[k - 1, :, :V])
            if persistent:
                assert np.array_equal(updates.persistent.get_value(), sc.trace_h.cpu().numpy()[k, :, :H]), "chain != recorded nh_sample"
            want = sm.grouped_cost(out[0], v0, bounds) / n
            check("grouped step: cost rel", abs(float(c) - want) / abs(want), 1e-5)
            state = sm.update(st, state, v0, ph, out[1], out[4], B, GROUPED_HP["lr"], mode=mode, momentum=mom,
                              weightcost=GROUPED_HP["weightcost"])
            # the packed [S | s_h | s_v] the update read, after the transforms of the mode, and the offsets: the scales of
            # tests/test_gpu_center.py (a centred bias statistic is a sum over S': rho max sum |mu S'| and rho max sum |S' lam|)
            S, s_h, s_v, offsets = sm.transformed_stats(mode, state, v0, ph, out[1], out[4], B)
            ldv, ldh = sc.V2.stride(0), rbm.W.tensor.stride(0)
            gS, gsh, gsv, _ = cn.unpack(fn._stats_slots[0].cpu().numpy(), V, H, ldv, ldh)
            sh_scale, sv_scale = np.abs(s_h).max(), np.abs(s_v).max()
            if offsets is not None:
                sh_scale = max(sh_scale, np.abs(offsets[0][:, None] * S).sum(axis=0).max())
                sv_scale = max(sv_scale, np.abs(S * offsets[1][None, :]).sum(axis=1).max())
                check("grouped step: v_offset", np.abs(rbm.v_offset.get_value() - offsets[0]).max(), 2e-6)
                check("grouped step: h_offset", np.abs(rbm.h_offset.get_value() - offsets[1]).max(), 2e-6)
            check("grouped step %s: S / max|S|" % mode, np.abs(gS - S).max() / np.abs(S).max(), 1e-5, "stats")
            check("grouped step %s: s_h / scale" % mode, np.abs(gsh - s_h).max() / sh_scale, 1e-5, "stats")
            check("grouped step %s: s_v / scale" % mode, np.abs(gsv - s_v).max() / sv_scale, 1e-5, "stats")
        eng.synchronize()
        if timing:
            r.kinds = [kd for _, _, _, kd in eng.kernel_timing_detail()]
    finally:
        if timing:
            eng.kernel_timing(False)
        eng.trace_chain = False
    r.flips = flips
    r.params = {n: getattr(rbm, n).get_value() for n in PARAMS}
    for n in ("v_offset", "h_offset", "h_activity"):
        if getattr(rbm, n, None) is not None:
            r.params[n] = getattr(rbm, n).get_value()
    if tapped:
        r.errs = [(p, np.abs(r.params[p] - getattr(st, p)).max() / max(1.0, np.abs(getattr(st, p)).max())) for p in PARAMS]
    return r


def check_grouped(name, r):
    print("%s: %s, %d draws differ (near a boundary under the twin alone: %s)"       # every figure before the first assertion
          % (name, ", ".join("%s %.3e" % e for e in r.errs), r.flips, r.twin_ties))
    for p, err in r.errs:
        check("grouped step %s: %s after %d steps / max" % (name, p, len(r.sizes)), err, 2e-6, "update")


def same_bits(a, b, what):
    """Two runs left the same bits: parameters (and log_sigma, offsets, activities), costs, V2 and P2 of every step."""
    assert sorted(a.params) == sorted(b.params), what
    for n in a.params:
        np.testing.assert_array_equal(a.params[n].view(np.int32), b.params[n].view(np.int32), err_msg="%s: %s" % (what, n))
    np.testing.assert_array_equal(np.array(a.costs), np.array(b.costs), err_msg="%s: costs" % what)
    assert len(a.scratch) == len(b.scratch)
    for t, ((V2a, P2a), (V2b, P2b)) in enumerate(zip(a.scratch, b.scratch)):
        np.testing.assert_array_equal(V2a.view(np.int32), V2b.view(np.int32), err_msg="%s: V2 of step %d" % (what, t))
        np.testing.assert_array_equal(P2a.view(np.int32), P2b.view(np.int32), err_msg="%s: P2 of step %d" % (what, t))
