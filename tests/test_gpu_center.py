"""Centred CD on the device: (a) the kernels of csrc/mdbn_center.hip alone against the float64 twin (tests/_center_np.py)
fed the device's own inputs, with poisoned pad columns, determinism and every MDBN_EINVAL case; (b) whole centred steps
through the public classes on every dispatch path of the CD step, against the twin loop teacher-forced along the device's
recorded chain; (c) with mu = 0 the centred update differs from the plain one by exactly what the twin says."""
import ctypes as C
import types

import numpy as np
import pytest

import _center_np as cn
from oracle import rbm_np
from oracle.philox_np import PhiloxDraws
from _margins import check

pytestmark = pytest.mark.gpu

# (V, H, ldh): small, ragged and the layer shapes of the presets -- 19937 rows: more row blocks than CUs, 32 rows per block -- then one with whole 16-byte
# groups of pad columns, 16 rows per block, and two / four 16-byte groups of a row per thread (H > 1024 / > 2048)
SHAPES = [(12, 7, 8), (100, 24, 24), (255, 200, 200), (784, 500, 500), (19937, 400, 400),
          (128, 400, 512), (8200, 36, 36), (40, 1100, 1100), (16, 2500, 2500)]
RHOS = [1.0, 20.0 / 32.0]
POISON = float("nan")


def packed(V, H, ldh, seed):
    """-> (stats float32 [V ldh + ldh + ldv + 4] with NaN in every pad column, ldv, mask of the pad entries, mu, lam)"""
    ldv = (V + 3) & ~3
    rs = np.random.RandomState(seed)
    st = rs.normal(size=V * ldh + ldh + ldv + 4).astype(np.float32)
    pad = np.zeros(st.size, dtype=bool)
    pad[:V * ldh].reshape(V, ldh)[:, H:] = True
    pad[V * ldh + H:V * ldh + ldh] = True
    pad[V * ldh + ldh + V:V * ldh + ldh + ldv] = True
    st[pad] = POISON
    return st, ldv, pad, rs.uniform(size=V).astype(np.float32), rs.uniform(-1, 1, size=H).astype(np.float32)


def bits(t):
    return t.detach().cpu().numpy().view(np.int32).copy()


def dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


# ------------------------------------------------------------------------------------------------------------------ (a) kernels
@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("V,H,ldh", SHAPES)
def test_center_stats_against_the_twin(hip_engine, V, H, ldh, rho):
    eng = hip_engine
    st, ldv, pad, mu, lam = packed(V, H, ldh, seed=V + H)
    d, dmu, dlam = dev(eng, st), dev(eng, mu), dev(eng, lam)
    eng.center_stats(d, V, H, ldv, ldh, dmu, dlam, rho)
    out = d.cpu().numpy()
    S, s_h, s_v, cost = cn.unpack(st, V, H, ldv, ldh)
    S2, sh2, sv2 = cn.center_stats(S, s_h, s_v, mu, lam, rho)
    gS, gsh, gsv, gcost = cn.unpack(out, V, H, ldv, ldh)
    tag = "center_stats %dx%d" % (V, H)
    check(tag + ": S' / max|S'|", np.abs(gS - S2).max() / np.abs(S2).max(), 1e-5, "stats")
    check(tag + ": s_v' / (rho max_i sum_j |S' lam|)", np.abs(gsv - sv2).max() / (rho * np.abs(S2 * lam[None, :]).sum(1).max()), 1e-5)
    check(tag + ": s_h' / (rho max_j sum_i |mu S'|)", np.abs(gsh - sh2).max() / (rho * np.abs(mu[:, None] * S2).sum(0).max()), 1e-5)
    # pad columns and the cost floats: bit-unchanged
    assert np.array_equal(out.view(np.int32)[pad], st.view(np.int32)[pad]), "a pad column was written"
    assert np.isfinite(out[~pad]).all(), "a pad column was read"
    assert np.array_equal(out[-4:].view(np.int32), st[-4:].view(np.int32)), "the cost floats were touched"
    assert np.array_equal(dmu.cpu().numpy(), mu) and np.array_equal(dlam.cpu().numpy(), lam)
    # a second run on the same inputs: bit-identical
    d2 = dev(eng, st)
    eng.center_stats(d2, V, H, ldv, ldh, dmu, dlam, rho)
    assert np.array_equal(bits(d2), out.view(np.int32)), "two runs differ"


@pytest.mark.parametrize("V,H,ldh", SHAPES)
def test_zero_offsets_return_the_buffer_bit_for_bit(hip_engine, V, H, ldh):
    eng = hip_engine
    st, ldv, pad, _, _ = packed(V, H, ldh, seed=3)
    d = dev(eng, st)
    eng.center_stats(d, V, H, ldv, ldh, dev(eng, np.zeros(V, np.float32)), dev(eng, np.zeros(H, np.float32)), 0.625)
    assert np.array_equal(bits(d), st.view(np.int32))


@pytest.mark.parametrize("B", [1, 20, 33, 512])
@pytest.mark.parametrize("V,H,ldh", [(12, 7, 8), (255, 200, 200), (4096, 1024, 1024)])
def test_center_offsets_against_the_twin(hip_engine, V, H, ldh, B):
    eng = hip_engine
    rs = np.random.RandomState(B + V)
    ldv = (V + 3) & ~3
    V2 = np.full((2 * B, ldv), POISON, dtype=np.float32)
    P2 = np.full((2 * B, ldh), POISON, dtype=np.float32)
    V2[:B, :V] = rs.normal(size=(B, V)) if V == 255 else (rs.uniform(size=(B, V)) < 0.3)
    P2[:B, :H] = rs.uniform(size=(B, H))
    sc = types.SimpleNamespace(V2=dev(eng, V2)[:, :V], P2=dev(eng, P2)[:, :H])
    mu0, lam0 = rs.uniform(size=V).astype(np.float32), rs.uniform(size=H).astype(np.float32)
    for nu in (1.0, 0.01):
        dmu, dlam = dev(eng, mu0), dev(eng, lam0)
        eng.center_offsets(sc, B, dmu, dlam, nu)
        mu, lam = cn.center_offsets(mu0, lam0, V2[:B, :V], P2[:B, :H], nu)
        check("center_offsets: mu", np.abs(dmu.cpu().numpy() - mu).max(), 2e-6)
        check("center_offsets: lam", np.abs(dlam.cpu().numpy() - lam).max(), 2e-6)
        again_mu, again_lam = dev(eng, mu0), dev(eng, lam0)
        eng.center_offsets(sc, B, again_mu, again_lam, nu)
        assert np.array_equal(bits(again_mu), bits(dmu)) and np.array_equal(bits(again_lam), bits(dlam)), "two runs differ"
    if B == 1:          # nu = 1 on one row: the offsets ARE that row
        dmu, dlam = dev(eng, mu0), dev(eng, lam0)
        eng.center_offsets(sc, 1, dmu, dlam, 1.0)
        assert np.array_equal(dmu.cpu().numpy(), V2[0, :V]) and np.array_equal(dlam.cpu().numpy(), P2[0, :H])


def test_every_einval_case_returns_without_touching_its_outputs(hip_engine):
    import torch
    from mdbn_amd import _lib
    eng, lib = hip_engine, hip_engine.lib
    V, H, ldh, B = 100, 24, 24, 20
    st, ldv, _, mu, lam = packed(V, H, ldh, seed=1)
    room = dev(eng, np.concatenate([st, np.zeros(8, np.float32)]))       # (room for a misaligned view of the same size)
    d, dmu, dlam = room[:st.size], dev(eng, mu), dev(eng, lam)
    need = C.c_int64()
    _lib.check(lib.mdbn_center_workspace_bytes(eng.ctx, V, H, C.byref(need)), "mdbn_center_workspace_bytes")
    assert need.value >= ((V + 31) // 32) * ((H + 3) & ~3) * 4
    ws = torch.zeros(need.value // 4 + 8, dtype=torch.float32, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    nan = float("nan")

    def stats_call(stats=d, V=V, H=H, ldv=ldv, ldh=ldh, mu=dmu, lam=dlam, rho=1.0, ws=ws, ws_bytes=None, ctx=eng.ctx):
        return lib.mdbn_center_stats(ctx, eng._stream(), p(stats), V, H, ldv, ldh, p(mu), p(lam), rho, p(ws),
                                     need.value if ws_bytes is None else ws_bytes)

    before = (bits(room), bits(dmu), bits(dlam), bits(ws))
    bad = [dict(V=0), dict(H=0), dict(V=-3), dict(stats=None), dict(mu=None), dict(lam=None), dict(ws=None), dict(ctx=None),
           dict(stats=room[1:1 + st.size]), dict(ws=ws[1:]), dict(mu=dmu.view(torch.uint8)[1:]), dict(lam=dlam.view(torch.uint8)[2:]),
           dict(ldh=H - 4), dict(ldh=H + 2), dict(ldv=V - 4), dict(ldv=V + 2), dict(rho=0.0), dict(rho=-1.0), dict(rho=nan),
           dict(rho=float("inf")), dict(ws_bytes=need.value - 4), dict(ws_bytes=0), dict(H=4097, ldh=4100)]
    for kw in bad:
        assert stats_call(**kw) == -1, kw
        assert _lib.last_error(), kw
    eng.synchronize()
    after = (bits(room), bits(dmu), bits(dlam), bits(ws))
    assert all(np.array_equal(a, b) for a, b in zip(before, after)), "a refused call wrote something"
    for args in ((0, H), (V, 0), (V, 4097)):
        assert lib.mdbn_center_workspace_bytes(eng.ctx, args[0], args[1], C.byref(need)) == -1
    assert lib.mdbn_center_workspace_bytes(eng.ctx, V, H, None) == -1

    v0 = torch.rand((B + 1, ldv), dtype=torch.float32, device=eng.device)
    ph = torch.rand((B + 1, ldh), dtype=torch.float32, device=eng.device)

    def off_call(v0=v0, ldv=ldv, ph=ph, ldh=ldh, B=B, V=V, H=H, nu=0.5, mu=dmu, lam=dlam, ctx=eng.ctx):
        return lib.mdbn_center_offsets(ctx, eng._stream(), p(v0), ldv, p(ph), ldh, B, V, H, nu, p(mu), p(lam))

    bad = [dict(B=0), dict(V=0), dict(H=0), dict(B=-1), dict(v0=None), dict(ph=None), dict(mu=None), dict(lam=None), dict(ctx=None),
           dict(nu=0.0), dict(nu=-0.5), dict(nu=1.5), dict(nu=nan), dict(v0=v0.reshape(-1)[1:]), dict(ph=ph.reshape(-1)[1:]),
           dict(ldv=V - 4), dict(ldh=H - 4), dict(ldv=V + 2), dict(ldh=H + 2)]
    for kw in bad:
        assert off_call(**kw) == -1, kw
    eng.synchronize()
    assert np.array_equal(bits(dmu), before[1]) and np.array_equal(bits(dlam), before[2]), "a refused call wrote something"
    assert off_call() == 0 and stats_call() == 0                         # ... and the good calls go through
    eng.synchronize()
    assert not np.array_equal(bits(dmu), before[1])


# ------------------------------------------------------------------------------------------------------------------ (b) whole steps
TILED_F32 = dict(stream_x6=0, skinny_gemm=0, gemm_bf16x6=0, small_fused=0, thin_fused=0)
CASES = [  # id, V, H, B, k, gauss, persistent, hyper-parameters, engine options, path of the run
    ("small_one_launch", 100, 24, 512, 1, False, False, dict(lr=0.1, weightcost=2e-4), {}, "small"),
    ("thin_batch20", 784, 500, 20, 1, False, False, dict(lr=0.1, weightcost=2e-4), {}, "thin"),
    ("stream_small_layer", 256, 200, 512, 2, True, False, dict(lr=0.002, lambda_2=0.1), {}, "stream"),
    ("planes_headline", 4096, 1024, 512, 1, True, False, dict(lr=0.001, lambda_2=0.1), {}, "planes"),
    ("tiled_f32_ragged", 250, 130, 99, 1, False, False, dict(lr=0.1, weightcost=2e-4), TILED_F32, "tiled_f32"),
    ("pcd_batch20", 784, 500, 20, 1, False, True, dict(lr=0.1, weightcost=2e-4), {}, "f32_operands"),
]
STEPS = 4
NAMES = ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed")


def _run(eng, V, H, B, k, gauss, persistent, hp, tapped):
    import mdbn_amd
    N = 3 * B + 7
    rs = np.random.RandomState(31)
    data = rs.normal(size=(N, V)).astype(np.float32) if gauss else (rs.uniform(size=(N, V)) < 0.3).astype(np.float32)
    cls = mdbn_amd.GRBM if gauss else mdbn_amd.RBM
    rbm = cls(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(123), theano_rng=mdbn_amd.RandomStreams(7), engine=eng)
    st = rbm_np.RBMState(V, H, W=rbm.W.get_value(), gauss=gauss)
    if hp.get("weightcost"):
        st.freeze_W0()
    chain = (rs.uniform(size=(B, H)) < 0.5).astype(np.float32) if persistent else None
    _, updates = rbm.get_cost_updates(k=k, batch_size=B, persistent=chain, centered=True, offset_rate=0.05, **hp)
    fn = mdbn_amd.function(updates, mdbn_amd.shared(data, engine=eng), data_parallel=None)
    order = [eng.index_tensor(rs.permutation(N)[:B], N) for _ in range(STEPS + 1)]
    eng.trace_chain = tapped
    eng.kernel_timing(True)
    costs, offsets, scratch = [], None, []
    twin_hp = {key: v for key, v in hp.items() if key != "lr"}
    try:
        for t in range(STEPS):
            mom = 0.5 if t < 2 else 0.9
            chain0 = updates.persistent.get_value().astype(np.float64) if persistent else None
            c = fn(indexes=order[t], momentum=mom, next_indexes=order[t + 1])
            sc = eng.last_scratch
            V2, P2 = sc.V2.cpu().numpy()[:B], sc.P2.cpu().numpy()[:B]
            scratch.append((V2, P2))
            if tapped:
                v0 = data[order[t].cpu().numpy()].astype(np.float64)
                forced = (sc.trace_h.cpu().numpy()[:, :, :H], None if gauss else sc.trace_v.cpu().numpy()[:, :, :V])
                ph, _, out, flips = rbm_np.cd_chain_forced(st, v0, PhiloxDraws(7, rbm.stream_id, t), k, forced[0], forced[1],
                                                           persistent=chain0, tie=1e-6)
                assert flips <= 3
                # what center_offsets reads: the float32 copies of v0 and ph_mean, on every path
                assert np.array_equal(V2, v0.astype(np.float32)), "rows 0..B-1 of V2 are not v0"
                check("centred step: ph_mean in P2", np.abs(P2 - ph).max(), 2e-6, "prob")
                if persistent:
                    want = rbm_np.pseudo_likelihood_cost(st, v0)
                    st.bit_i_idx = (st.bit_i_idx + 1) % V
                    check("centred step (PCD): cost rel", abs(float(c) - want) / abs(want), 1e-4)
                    assert np.array_equal(updates.persistent.get_value(), forced[0][k]), "chain != recorded nh_sample"
                else:
                    want = rbm_np.reconstruction_cost(st, out[0], v0)
                    check("centred step: cost rel", abs(float(c) - want) / abs(want), 1e-5)
                offsets = cn.centered_update(st, offsets, v0, ph, out[1], out[4], 0.05, B, hp["lr"], momentum=mom, **twin_hp)
            costs.append(float(c))
        eng.synchronize()
        kinds = [kd for _, _, _, kd in eng.kernel_timing_detail()]
    finally:
        eng.kernel_timing(False)
        eng.trace_chain = False
    params = {n: getattr(rbm, n).get_value() for n in NAMES}
    params["v_offset"], params["h_offset"] = rbm.v_offset.get_value(), rbm.h_offset.get_value()
    return params, np.array(costs), kinds, scratch, st, offsets


@pytest.mark.parametrize("name,V,H,B,k,gauss,persistent,hp,opts,path", CASES, ids=[c[0] for c in CASES])
def test_centred_steps_on_every_dispatch_path(built_lib, name, V, H, B, k, gauss, persistent, hp, opts, path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mdbn_amd
    eng = mdbn_amd.HipEngine()                     # product defaults but for `opts`; keep_f32 stays off
    for key, value in opts.items():
        eng.set_option(key, value)
    assert not eng.keep_f32
    tapped, tcosts, _, tscratch, st, offsets = _run(eng, V, H, B, k, gauss, persistent, hp, tapped=True)
    errs = [(pname, np.abs(tapped[pname] - getattr(st, pname)).max() / max(1.0, np.abs(getattr(st, pname)).max())) for pname in NAMES]
    errs += [("v_offset", np.abs(tapped["v_offset"] - offsets[0]).max()), ("h_offset", np.abs(tapped["h_offset"] - offsets[1]).max())]
    print("%s: %s" % (name, ", ".join("%s %.3e" % e for e in errs)))         # every figure before the first assertion
    for pname, err in errs[:len(NAMES)]:
        check("centred step %s: %s after %d steps / max" % (name, pname, STEPS), err, 2e-6, "update")
    for pname, err in errs[len(NAMES):]:
        check("centred step %s: %s" % (name, pname), err, 2e-6)
    # the same run without chain taps: the path it takes, and the same bits (keep_f32 of the call alone gives v0 / ph_mean)
    plain, pcosts, kinds, pscratch, _, _ = _run(eng, V, H, B, k, gauss, persistent, hp, tapped=False)
    assert not eng.keep_f32
    if path in ("small", "thin"):
        assert kinds == [], kinds
    elif path == "stream":
        assert kinds and all(1100 <= kd < 2000 for kd in kinds), kinds
    elif path == "planes":
        assert kinds and all(kd >= 2000 for kd in kinds), kinds
    elif path == "tiled_f32":
        assert len(kinds) == STEPS * (2 * k + 2) and all(kd < 100 for kd in kinds), kinds
    else:                                           # (PCD: + the two free-energy passes of the pseudo-likelihood monitor)
        assert len(kinds) == STEPS * (2 * k + 2 + 2) and all(kd < 2000 for kd in kinds), kinds
    for pname in plain:
        np.testing.assert_array_equal(plain[pname], tapped[pname], err_msg="%s: %s" % (name, pname))
    np.testing.assert_array_equal(pcosts, tcosts)
    for (V2a, P2a), (V2b, P2b) in zip(pscratch, tscratch):
        np.testing.assert_array_equal(V2a, V2b)
        np.testing.assert_array_equal(P2a, P2b)


def test_a_resumed_centred_run_continues_bit_for_bit(hip_engine, tmp_path):
    import mdbn_amd
    from mdbn_amd import checkpoint
    mdbn_amd.DBN.verbose = False
    eng = hip_engine
    rs = np.random.RandomState(0)
    V, H = 96, 40
    x = rs.normal(size=(40, V)).astype(np.float32)
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[], n_outs=H, engine=eng)
    rbm = net.rbm_layers[0]
    _, up = rbm.get_cost_updates(0.005, k=1, lambda_2=0.1, batch_size=10, centered=True)
    fn = mdbn_amd.function(up, mdbn_amd.shared(x, engine=eng), data_parallel=None)
    for t in range(2):
        fn(indexes=np.arange(10) + 10 * t, momentum=0.5)
    path = str(tmp_path / "centred.npz")
    checkpoint.save_network(path, {'ge': net}, resume=True)
    want = [float(fn(indexes=np.arange(10) + 10 * t, momentum=0.5)) for t in (2, 3)]
    r2 = checkpoint.load_network(path, engine=eng)['ge'].rbm_layers[0]
    _, up2 = r2.get_cost_updates(0.005, k=1, lambda_2=0.1, batch_size=10, centered=True)
    fn2 = mdbn_amd.function(up2, mdbn_amd.shared(x, engine=eng), data_parallel=None)
    got = [float(fn2(indexes=np.arange(10) + 10 * t, momentum=0.5)) for t in (2, 3)]
    assert got == want
    for n in NAMES + ("v_offset", "h_offset"):
        assert np.array_equal(getattr(r2, n).get_value(), getattr(rbm, n).get_value()), n


# ------------------------------------------------------------------------------------------------------------------ (c) invariance
@pytest.mark.parametrize("V,H,B,gauss", [(255, 200, 33, False), (784, 500, 20, True)])
def test_zero_visible_offset_changes_the_update_by_what_the_twin_says(hip_engine, V, H, B, gauss):
    """mu = 0, lam = anything: S' = S - s_v lam', s_h' = s_h (bit for bit), s_v' = s_v - rho S' lam.  So after the
    unchanged update rule the hidden-bias speed is the plain step's bit for bit, and the weight speed differs from it by
    -(1 - momentum) s_v lam' / batch_size."""
    import mdbn_amd
    from mdbn_amd import RngAddr
    eng = hip_engine
    rs = np.random.RandomState(V)
    data = rs.normal(size=(B, V)).astype(np.float32) if gauss else (rs.uniform(size=(B, V)) < 0.3).astype(np.float32)
    mom, batch_size, lr = 0.5, 32, 0.05
    rbms = [(mdbn_amd.GRBM if gauss else mdbn_amd.RBM)(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(3),
                                                       theano_rng=mdbn_amd.RandomStreams(7), engine=eng) for _ in range(2)]
    stats, _ = eng.cd_step(eng.to_device(data), None, rbms[0].W.tensor, rbms[0].hbias.tensor, rbms[0].vbias.tensor, gauss, 1,
                           RngAddr(7, 1, 0, 0, 0), stats=eng.new_stats_buffer(V, H))
    ldv, ldh = (V + 3) & ~3, rbms[0].W.tensor.stride(0)
    centred = stats.clone()
    lam = rs.uniform(size=H).astype(np.float32)
    eng.center_stats(centred, V, H, ldv, ldh, dev(eng, np.zeros(V, np.float32)), dev(eng, lam), float(B) / batch_size)
    S, s_h, s_v, _ = cn.unpack(stats.cpu().numpy(), V, H, ldv, ldh)
    for r, st in zip(rbms, (stats, centred)):
        eng.apply_update(r.W.tensor, r.W_speed.tensor, None, r.hbias.tensor, r.hbias_speed.tensor, r.vbias.tensor,
                         r.vbias_speed.tensor, st, lr, 0.0, 0.0, 0.0, mom, batch_size, B, 1.0, 0, ldv)
    plain, cent = rbms
    assert np.array_equal(cent.hbias_speed.get_value(), plain.hbias_speed.get_value())
    S2, _, sv2 = cn.center_stats(S, s_h, s_v, np.zeros(V), lam, float(B) / batch_size)
    dW = cent.W_speed.get_value().astype(np.float64) - plain.W_speed.get_value()
    want = -(1.0 - mom) * np.outer(s_v, lam) / batch_size
    scale = (1.0 - mom) * np.abs(S2).max() / batch_size
    check("centred vs plain: W_speed difference / ((1 - m) max|S'| / batch_size)", np.abs(dW - want).max() / scale, 1e-5, "stats")
    dv = cent.vbias_speed.get_value().astype(np.float64) - plain.vbias_speed.get_value()
    want_v = (1.0 - mom) * (sv2 - s_v) / B
    check("centred vs plain: vbias_speed difference", np.abs(dv - want_v).max() / ((1.0 - mom) * np.abs(S2 * lam[None, :]).sum(1).max() / batch_size),
          1e-5)
