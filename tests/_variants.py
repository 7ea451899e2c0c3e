"""Helpers of tests/test_gpu_step_variants.py (TEST-ONLY): the three CD-step variants no fast path serves -- PCD
(mdbn_cd_args.persistent), sample statistics (sample_stats, the reference's compute_symbolic_grad) and the noisy GRBM inside
the step (gauss + add_noise) -- run through the generic body of cd_step_impl with the chain tapped, and the float64 oracle
teacher-forced along the device's taps (oracle.rbm_np.cd_chain_forced).

GEMM launch kinds (kernel_timing_detail): family = kind // 1000 (1: register streaming, 2+: planes), pipe = kind // 100 % 10
(0 exact f32, 1 bf16 pipe with six piece products, 2 with three), fused = kind // 10 % 10, layout = kind % 10 (0 propdown,
1 propup, 3 statistics)."""
import contextlib

import numpy as np

from oracle import rbm_np
from oracle.philox_np import PhiloxDraws
from _knobs import KNOBS
from _margins import check

PARAMS = ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed")
RNG = (5, 3, 11)                # seed, stream, step of every single-step case

# the knobs that keep a step off the one-launch, thin and plane paths: the baseline of a comparison with a plain CD step
NO_FAST_PATH = dict(small_fused=0, thin_fused=0, gemm_planes=0)

# name -> (gauss, k, keyword arguments of `cd`); `chain`: how the caller's persistent chain starts
VARIANTS = {
    "pcd_frac": (False, 2, dict(chain="frac")),         # U(0, 1): not representable in one bf16 piece
    "pcd_bin": (False, 1, dict(chain="bin")),           # 0/1 at p = 0.5; k = 1: the only hidden sample is the one written back
    "stats_rbm": (False, 2, dict(sample_stats=True)),
    "stats_grbm": (True, 2, dict(sample_stats=True)),
    "noise_grbm": (True, 2, dict(add_noise=True)),
}


def family(kind):
    return kind // 1000


def pipe(kind):
    return kind // 100 % 10


def fused(kind):
    return kind // 10 % 10


def forward(kinds):
    """The propup / propdown launches of a step (everything but the statistics GEMM)."""
    return [kd for kd in kinds if kd % 10 in (0, 1)]


@contextlib.contextmanager
def options(eng, **opts):
    """Set knobs for the block; every one is back at its default afterwards, whatever happens inside."""
    try:
        for name, value in opts.items():
            if name == "planes_min_work":
                eng.set_planes_min_work(value)
            else:
                eng.set_option(name, value)
        yield
    finally:
        for name in opts:
            if name == "planes_min_work":
                eng.set_planes_min_work(KNOBS[name]["default"])
            else:
                eng.set_option(name, KNOBS[name]["default"])


def split_planes(eng, x):
    """mdbn_split_planes of a device matrix: its [3, rows, ld] bf16 planes."""
    import ctypes as C
    import torch
    from mdbn_amd import _lib
    rows, ld = x.shape[0], x.stride(0)
    P = torch.empty((3, rows, ld), dtype=torch.int16, device=eng.device)
    base = x._base if x._base is not None else x
    _lib.check(eng.lib.mdbn_split_planes(eng.ctx, eng._stream(), C.c_void_p(base.data_ptr()), rows, ld,
                                         C.c_void_p(P.data_ptr())), "mdbn_split_planes")
    return P


def w_planes_in_step(eng, W):
    """The engine's planes of W are marked valid and hold the split of the CURRENT W bit for bit."""
    import torch
    wp, valid = eng.w_planes(W)
    assert wp is not None and valid, "the engine holds no valid planes of W"
    eng.synchronize()
    return bool(torch.equal(wp, split_planes(eng, W)))


def cd(eng, V, H, B, k, gauss, opts, chain=None, sample_stats=False, add_noise=False, seed=5, params=None):
    """One eng.cd_step with keep_f32 and the chain taps on under `opts`: inputs, statistics, V2, P2, taps, the caller's chain
    before and after the call, the GEMM launch kinds, and what the scratch / the engine hold of bf16 planes.  `params`: the
    layer's (W, hbias, vbias) in place of init_W and N(0, 0.2) biases (the data and the index list stay those of `seed`)."""
    from mdbn_amd import RngAddr
    rs = np.random.RandomState(seed)
    W = rbm_np.init_W(rs, V, H, np.float32)
    hb, vb = rs.normal(0, 0.2, H).astype(np.float32), rs.normal(0, 0.2, V).astype(np.float32)
    if params is not None:
        W, hb, vb = [np.ascontiguousarray(a, dtype=np.float32) for a in params]
        assert W.shape == (V, H) and hb.shape == (H,) and vb.shape == (V,), (W.shape, hb.shape, vb.shape)
    N = B + 13
    data = rs.normal(size=(N, V)).astype(np.float32) if gauss else (rs.uniform(size=(N, V)) < 0.3).astype(np.float32)
    idx = rs.permutation(N)[:B].astype(np.int64)
    chain0 = None
    if chain == "frac":
        chain0 = rs.uniform(size=(B, H)).astype(np.float32)
    elif chain == "bin":
        chain0 = (rs.uniform(size=(B, H)) < 0.5).astype(np.float32)
    dW, dhb, dvb, dx = [eng.to_device(a) for a in (W, hb, vb, data)]
    keep = (eng.keep_f32, eng.trace_chain)
    eng.keep_f32, eng.trace_chain = True, True
    eng.kernel_timing(True)
    try:
        with options(eng, **opts):
            eng._scratch.clear()                # fresh taps: a row no pass of this call writes stays zero
            pers = None
            if chain0 is not None:
                pers = eng.alloc_matrix(B, H, dW.stride(0))
                pers.copy_(eng.to_device(chain0))
            eligible = eng.plane_shape(B, V, H, dx.stride(0), dW.stride(0))
            stats, sc = eng.cd_step(dx, idx, dW, dhb, dvb, gauss, k, RngAddr(RNG[0], RNG[1], RNG[2], 0, 0), persistent=pers,
                                    add_noise=add_noise, sample_stats=sample_stats)
            eng.synchronize()
            kinds = [kd for _, _, _, kd in eng.kernel_timing_detail()]
            wp, _ = eng.w_planes(dW)
            planes_ok = None if wp is None else w_planes_in_step(eng, dW)
            outputs = dict(stats=stats, P2=sc.P2, V2=sc.V2, trace_h=sc.trace_h)
            if not gauss:
                outputs["trace_v"] = sc.trace_v
            nonfinite = {name: eng.count_nonfinite(t) for name, t in outputs.items()}   # pad columns included
    finally:
        eng.kernel_timing(False)
        eng.keep_f32, eng.trace_chain = keep
    n_h = k + 1 if pers is not None else k      # the last hidden sample exists only when it is written back to the chain
    return dict(V=V, H=H, B=B, k=k, gauss=gauss, opts=opts, sample_stats=sample_stats, add_noise=add_noise, W=W, hb=hb, vb=vb,
                x=data[idx], chain0=chain0, stats=stats.cpu().numpy(), ldh=sc.P2.stride(0), ldv=sc.V2.stride(0),
                P2=sc.P2.cpu().numpy(), V2=sc.V2.cpu().numpy(), th=sc.trace_h.cpu().numpy()[:n_h, :, :H],
                tv=None if gauss else sc.trace_v.cpu().numpy()[:, :, :V],
                chain1=None if pers is None else pers.cpu().numpy(), kinds=kinds, eligible=eligible,
                scratch_planes=sc.planes is not None, planes_ok=planes_ok, nonfinite=nonfinite)


def run_variant(eng, name, V, H, B, opts, **kw):
    gauss, k, args = VARIANTS[name]
    return cd(eng, V, H, B, k, gauss, opts, **dict(args, **kw))


def variant_statistics(v0, ph_mean, out, gauss, sample_stats):
    """S, s_h, s_v of a step from the outputs of its chain (`out` of cd_chain / cd_chain_forced).  Sample statistics of a
    Bernoulli RBM (rbm.py:339-342,378-390): the negative visible data is the last visible SAMPLE out[2], and out[4] is its
    propup already, because the chain feeds the sample upward (rbm.py:246).  A GRBM's sample is its mean (error_free), so its
    sample statistics are the plain ones."""
    nv = out[2] if (sample_stats and not gauss) else out[1]
    return rbm_np.cd_statistics(v0, ph_mean, nv, out[4])


def oracle(tag, r):
    """The step of `cd` against the float64 oracle teacher-forced along its own taps: DESIGN.md section 4's tolerances."""
    V, H, B, k, gauss = r["V"], r["H"], r["B"], r["k"], r["gauss"]
    msg = "%d->%d B=%d k=%d %r" % (V, H, B, k, r["opts"])
    st = rbm_np.RBMState(V, H, W=r["W"], hbias=r["hb"], vbias=r["vb"], gauss=gauss)
    v0 = r["x"].astype(np.float64)
    chain0 = None if r["chain0"] is None else r["chain0"].astype(np.float64)
    ph, _, out, flips = rbm_np.cd_chain_forced(st, v0, PhiloxDraws(RNG[0], RNG[1], RNG[2], 0), k, r["th"], r["tv"],
                                               persistent=chain0, tie=1e-6)
    S_o, s_h_o, s_v_o = variant_statistics(v0, ph, out, gauss, r["sample_stats"])
    ldh, ldv = r["ldh"], r["ldv"]
    d = r["stats"]
    S, s_h, s_v = d[:V * ldh].reshape(V, ldh), d[V * ldh:V * ldh + H], d[V * ldh + ldh:V * ldh + ldh + V]
    cost = d[V * ldh + ldh + ldv]
    assert not S[:, H:].any(), "%s: pad columns of S must stay zero (%s)" % (tag, msg)
    check(tag + ": S / max|S|", np.abs(S[:, :H] - S_o).max() / max(1.0, np.abs(S_o).max()), 1e-5, "stats", msg)
    check(tag + ": s_h / max", np.abs(s_h - s_h_o).max() / max(1.0, np.abs(s_h_o).max()), 1e-5, "stats", msg)
    check(tag + ": s_v / max", np.abs(s_v - s_v_o).max() / max(1.0, np.abs(s_v_o).max()), 1e-5, "stats", msg)
    check(tag + ": ph_mean", np.abs(r["P2"][:B, :H] - ph).max(), 2e-6, "prob", msg)
    check(tag + ": nh_mean", np.abs(-r["P2"][B:2 * B, :H] - out[4]).max(), 4e-6, "prob", msg)
    nv = r["V2"][B:2 * B, :V]
    if r["sample_stats"] and not gauss:
        # rows B..2B of V2 hold the SAMPLE (what the statistics GEMM and the last propup read), not the mean
        assert np.array_equal(nv, r["tv"][k - 1]), "%s: V2[B:2B] is not the recorded last visible sample (%s)" % (tag, msg)
        assert np.isin(nv, (0.0, 1.0)).all(), "%s: V2[B:2B] holds something else than 0/1 (%s)" % (tag, msg)
    else:
        check(tag + ": nv_mean / max|nv|", np.abs(nv - out[1]).max() / max(1.0, np.abs(out[1]).max()), 2e-6, "nv_mean", msg)
    pre = out[0]
    if gauss:
        want = ((rbm_np.sigmoid(pre) - v0) ** 2).sum()
    else:
        want = (v0 * rbm_np.softplus(-pre) + (1 - v0) * rbm_np.softplus(pre)).sum()
    check(tag + ": cost sum rel", abs(cost - want) / abs(want), 2e-6, msg=msg)
    if chain0 is not None:
        # rbm.py:369: the chain is replaced by the last hidden sample (checked against the oracle's own draw by _follow)
        assert np.array_equal(r["chain1"], r["th"][k]), "%s: persistent != recorded nh_sample (%s)" % (tag, msg)
        assert np.isin(r["chain1"], (0.0, 1.0)).all(), (tag, msg)
    assert flips <= 3, (tag, msg, flips)


def same(a, b, what):
    for key in ("stats", "P2", "V2", "th", "chain1"):
        if a[key] is None and b[key] is None:
            continue
        np.testing.assert_array_equal(a[key], b[key], err_msg="%s: %s" % (what, key))


def verdict(shadow, name, rbms=(), cost_tol=None, param_tol=None, stat_tol=None):
    """Record a ShadowEngine's worst deviations under their tolerances (as tests/test_gpu_surface.py does)."""
    if cost_tol is not None:
        check(name + ": step cost rel", shadow.cost_err, cost_tol)
    if stat_tol is not None:
        check(name + ": S / s_h / s_v rel-to-max", shadow.stat_err, stat_tol, "stats")
    for r in rbms:
        check(name + ": parameters vs shadow, rel-to-max", shadow.param_err(r), param_tol)
    check(name + ": |u - p| of a flipped draw", rbm_np.FLIP_GAP["max"], shadow.tie, "tie")
