"""Every tuning knob of mdbn_set_option (tests/_knobs.py) that no other test sets, against the float64 oracle.

include/mdbn_hip.h promises that no knob changes results beyond fp32 summation order, and MDBN_OPTIONS hands any knob to every
engine of a process.  Each case below forces the code path that reads the knob (the GEMM launch kinds of kernel_timing_detail
prove which kernel ran: 1000 = register streaming, 100 * pipe, 10 * fused, 2000+ = planes), runs a CD step or training steps
with the chain tapped, and checks the result against the teacher-forced oracle (rbm.py:258-376 step by step) with the
tolerances of the path's own tests; where the code computes the same sums in the same order, the result must also equal the
default setting's bit for bit.  One engine of this module's own; every knob set is reset to its default in `finally`."""
import contextlib

import numpy as np
import pytest

from oracle import rbm_np
from oracle.philox_np import PhiloxDraws
from _knobs import KNOBS
from _margins import check

pytestmark = pytest.mark.gpu

PARAMS = ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed")


@pytest.fixture(scope="module")
def eng(built_lib):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mdbn_amd
    return mdbn_amd.HipEngine()


def _reset(eng, name):
    if name == "planes_min_work":
        eng.set_planes_min_work(KNOBS[name]["default"])
    else:
        eng.set_option(name, KNOBS[name]["default"])


@contextlib.contextmanager
def _options(eng, **opts):
    try:
        for name, value in opts.items():
            if name == "planes_min_work":
                eng.set_planes_min_work(value)
            else:
                eng.set_option(name, value)
        yield
    finally:
        for name in opts:
            _reset(eng, name)


def _cd(eng, V, H, B, k, gauss, opts, seed=5):
    """One mdbn_cd_step with the chain tapped under `opts`: inputs, statistics, scratch, taps and GEMM launch kinds."""
    from mdbn_amd import RngAddr
    rs = np.random.RandomState(seed)
    W = rbm_np.init_W(rs, V, H, np.float32)
    hb, vb = rs.normal(0, 0.2, H).astype(np.float32), rs.normal(0, 0.2, V).astype(np.float32)
    N = B + 13
    data = rs.normal(size=(N, V)).astype(np.float32) if gauss else (rs.uniform(size=(N, V)) < 0.3).astype(np.float32)
    idx = rs.permutation(N)[:B].astype(np.int64)
    dW, dhb, dvb, dx = [eng.to_device(a) for a in (W, hb, vb, data)]
    eng.keep_f32, eng.trace_chain = True, True
    eng.kernel_timing(True)
    try:
        with _options(eng, **opts):
            stats, sc = eng.cd_step(dx, idx, dW, dhb, dvb, gauss, k, RngAddr(5, 3, 11, 0, 0))
            eng.synchronize()
            kinds = [kd for _, _, _, kd in eng.kernel_timing_detail()]
    finally:
        eng.kernel_timing(False)
        eng.keep_f32, eng.trace_chain = False, False
    return dict(V=V, H=H, B=B, k=k, gauss=gauss, opts=opts, W=W, hb=hb, vb=vb, x=data[idx], stats=stats.cpu().numpy(),
                ldh=sc.P2.stride(0), ldv=sc.V2.stride(0), P2=sc.P2.cpu().numpy(), V2=sc.V2.cpu().numpy(), th=sc.trace_h.cpu().numpy()[:, :, :H],
                tv=None if gauss else sc.trace_v.cpu().numpy()[:, :, :V], kinds=kinds)


def _oracle(tag, r):
    """The step of `_cd` against the float64 oracle teacher-forced along its own chain (tolerances of test_gpu_stream.py)."""
    V, H, B, k, gauss = r["V"], r["H"], r["B"], r["k"], r["gauss"]
    msg = "%d->%d B=%d CD-%d %r" % (V, H, B, k, r["opts"])
    st = rbm_np.RBMState(V, H, W=r["W"], hbias=r["hb"], vbias=r["vb"], gauss=gauss)
    v0 = r["x"].astype(np.float64)
    ph, _, out, flips = rbm_np.cd_chain_forced(st, v0, PhiloxDraws(5, 3, 11, 0), k, r["th"], r["tv"])
    S_o, s_h_o, s_v_o = rbm_np.cd_statistics(v0, ph, out[1], out[4])
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
    check(tag + ": nv_mean / max|nv|", np.abs(r["V2"][B:2 * B, :V] - out[1]).max() / max(1.0, np.abs(out[1]).max()),
          2e-6, "nv_mean", msg)
    pre = out[0]
    if gauss:
        want = ((rbm_np.sigmoid(pre) - v0) ** 2).sum()
    else:
        want = (v0 * rbm_np.softplus(-pre) + (1 - v0) * rbm_np.softplus(pre)).sum()
    check(tag + ": cost sum rel", abs(cost - want) / abs(want), 2e-6, msg=msg)
    assert flips <= 3, (tag, msg)


def _same(a, b, what):
    for key in ("stats", "P2", "V2", "th"):
        np.testing.assert_array_equal(a[key], b[key], err_msg="%s: %s" % (what, key))


def _train(eng, V, H, B, k, gauss, hp, opts, tapped=True, steps=3, resident="device", hints=False, seed=31):
    """`steps` calls of the compiled step function (rbm.py:258-376) under `opts`; with the chain tapped every step is checked
    against the oracle and the parameters / speeds after the steps too.  Returns parameters, costs, kinds, the number of
    steps whose minibatch the previous step gathered ahead, and the layer's W tensor."""
    import mdbn_amd
    N = 3 * B + 7
    rs = np.random.RandomState(seed)
    data = rs.normal(size=(N, V)).astype(np.float32) if gauss else (rs.uniform(size=(N, V)) < 0.3).astype(np.float32)
    cls = mdbn_amd.GRBM if gauss else mdbn_amd.RBM
    costs, prepared = [], 0
    with _options(eng, **opts):
        rbm = cls(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(123), theano_rng=mdbn_amd.RandomStreams(7),
                  engine=eng)
        st = rbm_np.RBMState(V, H, W=rbm.W.get_value(), gauss=gauss)
        if hp.get("weightcost"):
            st.freeze_W0()
        _, updates = rbm.get_cost_updates(k=k, batch_size=B, **hp)
        fn = mdbn_amd.function(updates, mdbn_amd.shared(data, engine=eng, resident=resident), data_parallel=None)
        order = [rs.permutation(N)[:B] for _ in range(steps + 1)]
        if hints:
            order = [eng.index_tensor(o, N) for o in order]
        eng.trace_chain = tapped
        eng.kernel_timing(True)
        try:
            for t in range(steps):
                mom = 0.5 if t < 2 else 0.9
                kw = dict(next_indexes=order[t + 1]) if hints else {}
                c = float(fn(indexes=order[t], momentum=mom, **kw))
                prepared += int(eng.last_scratch.ahead is not None)
                if tapped:
                    sc = eng.last_scratch
                    forced = (sc.trace_h.cpu().numpy()[:, :, :H], None if gauss else sc.trace_v.cpu().numpy()[:, :, :V])
                    idx = order[t].cpu().numpy() if hints else order[t]
                    want = rbm_np.cd_step(st, data[idx], PhiloxDraws(7, rbm.stream_id, t), k=k, batch_size=B,
                                          momentum=mom, forced=forced, **hp)
                    check("knobs training: cost rel", abs(c - want) / abs(want), 1e-5)
                costs.append(c)
            eng.synchronize()
            kinds = [kd for _, _, _, kd in eng.kernel_timing_detail()]
        finally:
            eng.kernel_timing(False)
            eng.trace_chain = False
    params = {n: getattr(rbm, n).get_value() for n in PARAMS}
    if tapped:
        for n in PARAMS:
            ref = getattr(st, n)
            check("knobs training: %s after the steps / max" % n, np.abs(params[n] - ref).max() / max(1.0, np.abs(ref).max()),
                  2e-6, "update")
    return params, np.array(costs), kinds, prepared, rbm.W.tensor


def _same_run(a, b, what):
    for n in PARAMS:
        np.testing.assert_array_equal(a[0][n], b[0][n], err_msg="%s: %s" % (what, n))
    np.testing.assert_array_equal(a[1], b[1], err_msg="%s: costs" % what)


# ------------------------------------------------------------------ tiled GEMM plan


@pytest.mark.parametrize("V,H,B,gauss", [(1024, 512, 256, True), (1000, 300, 200, False)], ids=["grbm_1024_512", "rbm_1000_300"])
@pytest.mark.parametrize("x6", [3, 0])
def test_tiled_gemm_plan_knobs_against_forced_oracle(eng, V, H, B, gauss, x6):
    """gemm_bk / gemm_cw / gemm_min_splitk are read by plan_gemm, which serves every pass that is neither streamed
    (stream_x6 = 0) nor on planes (gemm_planes = 0): the slice depth, the MFMA waves per SIMD of the exact-f32 kernel (the
    data-parallel fallback runs gemm_cw = 1, rbm.py) and the split-K plan.  With gemm_bf16x6 = 3 the 1024 -> 512 passes run
    the bf16x6 kernel over that plan's split (kinds 1xx), with 0 the exact kernel only.

    gemm_min_splitk above the default 128 lengthens the f32 chains of the exact kernel (too few jobs for bf16x6 then).  At
    the Gaussian 1024 -> 512 layer that measured ph_mean 2.65e-6 at 512 (two 512-long
    chains summed) and 2.03e-6 at 4096 (one 1024-long chain) against the float64 oracle: past the 2e-6 probability contract
    the default plans keep (chains of at most 128 per split).  Summation order, not a wrong sum -- so that layer is checked at
    32 only, and the Bernoulli 1000 -> 300 layer (measured within the contract) at 32, 512 and 4096."""
    base = dict(stream_x6=0, gemm_planes=0, gemm_bf16x6=x6)
    splitk = (32,) if gauss else (32, 512, 4096)
    for knob, values in (("gemm_bk", (0, 32, 64)), ("gemm_cw", (1, 2)), ("gemm_min_splitk", splitk)):
        for value in values:
            r = _cd(eng, V, H, B, 1, gauss, dict(base, **{knob: value}))
            _oracle("knobs tiled GEMM plan", r)
            assert r["kinds"] and all(kd < 1100 for kd in r["kinds"]), (knob, value, r["kinds"])
            if x6 == 0:
                assert all(kd < 100 or 1000 <= kd < 1100 for kd in r["kinds"]), (knob, value, r["kinds"])
            elif V == 1024:
                assert any(100 <= kd < 200 for kd in r["kinds"]), (knob, value, r["kinds"])


def test_bf16x6_job_floor_and_producer_waves(eng):
    """x6_min_jobs decides whether the tiled plans of 1024 -> 512 at B = 256 (8 - 64 tile jobs per pass) move to the bf16x6
    kernel; x6_producer_waves is read by every bf16x6 launch."""
    base = dict(stream_x6=0, gemm_planes=0)
    r = _cd(eng, 1024, 512, 256, 1, True, dict(base, x6_min_jobs=0))
    _oracle("knobs bf16x6 job floor", r)
    assert r["kinds"] and all(100 <= kd < 300 for kd in r["kinds"]), r["kinds"]       # (200: 0/1 row operand, three products)
    r = _cd(eng, 1024, 512, 256, 1, True, dict(base, x6_min_jobs=1 << 20))
    _oracle("knobs bf16x6 job floor", r)
    assert r["kinds"] and all(kd < 100 for kd in r["kinds"]), r["kinds"]
    for pw in (2, 4):
        r = _cd(eng, 1024, 512, 256, 1, True, dict(base, x6_min_jobs=0, x6_producer_waves=pw))
        _oracle("knobs bf16x6 producer waves", r)
        assert all(100 <= kd < 300 for kd in r["kinds"]), r["kinds"]


# ------------------------------------------------------------------ activation epilogue


@pytest.mark.parametrize("V,H,B", [(100, 260, 37), (784, 500, 20), (200, 1024, 512), (130, 2050, 1030)])
def test_epilogue_geometry_is_bitwise_the_auto_choice(eng, V, H, B):
    """epilogue_cw / epilogue_threads shape the activation epilogue launch, which every forward pass runs when the GEMM does
    not fuse it (fused_epilogue = 0; stream_x6 = 0 and skinny_gemm = 0 keep the passes on the tiled kernel).  Each output
    element is the same slab sum in the same order whatever the geometry: pre-activations, means and samples equal the auto
    choice bit for bit, the cost (one partial per block) to summation order; pre-activations against float64."""
    from mdbn_amd.engine import RngAddr
    rs = np.random.RandomState(V + H + B)
    Wn = (0.05 * rs.randn(V, H)).astype(np.float32)
    hbn, vbn = (0.1 * rs.randn(H)).astype(np.float32), (0.1 * rs.randn(V)).astype(np.float32)
    vn = rs.randn(B, V).astype(np.float32)
    hn = (rs.rand(B, H) < 0.5).astype(np.float32)
    W, hb, vb, v, hsrc = [eng.to_device(a) for a in (Wn, hbn, vbn, vn, hn)]

    def run(cw, threads):
        with _options(eng, fused_epilogue=0, stream_x6=0, skinny_gemm=0, epilogue_cw=cw, epilogue_threads=threads):
            up = eng.propup(v, W, hb, rng=RngAddr(7, 1, 3, 0))
            dn = eng.propdown(hsrc, W, vb, gauss=False, rng=RngAddr(7, 1, 3, 1), v0=(v > 0).float())
            dg = eng.propdown(hsrc, W, vb, gauss=True, add_noise=True, rng=RngAddr(7, 1, 3, 1), v0=v)
            return [t.cpu().numpy() for t in up] + [t.cpu().numpy() for t in dn] + [t.cpu().numpy() for t in dg[1:]]

    names = ["up.pre", "up.mean", "up.sample", "dn.pre", "dn.mean", "dn.sample", "dn.cost", "dg.mean", "dg.sample", "dg.cost"]
    auto = run(0, 0)
    pre_up = vn.astype(np.float64) @ Wn.astype(np.float64) + hbn
    pre_dn = hn.astype(np.float64) @ Wn.astype(np.float64).T + vbn
    check("knobs epilogue geometry: propup pre / max", np.abs(auto[0] - pre_up).max() / max(1.0, np.abs(pre_up).max()), 1e-5)
    check("knobs epilogue geometry: propdown pre / max", np.abs(auto[3] - pre_dn).max() / max(1.0, np.abs(pre_dn).max()), 1e-5)
    for cw in (1, 2, 4):
        for threads in (0, 64, 128, 256):
            got = run(cw, threads)
            for name, a, b in zip(names, got, auto):
                if name.endswith("cost"):
                    assert abs(float(a) - float(b)) <= 2e-6 * abs(float(b)) + 1e-6, (cw, threads, name)
                else:
                    assert np.array_equal(a, b), (cw, threads, name)
    for threads in (64, 128, 256):
        got = run(0, threads)
        for name, a, b in zip(names, got, auto):
            if not name.endswith("cost"):
                assert np.array_equal(a, b), (threads, name)


# ------------------------------------------------------------------ register-streaming limits


@pytest.mark.parametrize("V,H,B,opts", [(784, 500, 20, dict(thin_fused=0)), (16384, 400, 20, dict(thin_fused=0)),
                                        (100, 128, 300, dict(small_fused=0)), (256, 200, 129, dict(small_fused=0))],
                         ids=["thin_784_500", "thin_16384_400", "small_100_128", "small_256_200"])
def test_skinny_limits_against_forced_oracle(eng, V, H, B, opts):
    """skinny_fused_max_k (the K one streaming block takes alone: larger K splits, and above 64 rows leaves the streaming
    kernel) and skinny_max_macs (the size limit above 64 rows) are read by every pass of these layers once the thin /
    one-launch steps are off; stream_x6 = 0 keeps the passes on the exact-f32 streaming kernel so the kinds show the choice."""
    base = dict(opts, stream_x6=0)
    for knob, value in (("skinny_fused_max_k", 0), ("skinny_fused_max_k", 64), ("skinny_fused_max_k", 1024),
                        ("skinny_fused_max_k", 1 << 20), ("skinny_max_macs", 0), ("skinny_max_macs", 32 << 20),
                        ("skinny_max_macs", 1 << 40)):
        r = _cd(eng, V, H, B, 1, False, dict(base, **{knob: value}))
        _oracle("knobs skinny limits", r)
        kinds = r["kinds"]
        assert kinds and all(kd < 1100 for kd in kinds), (knob, value, kinds)
        if B > 64 and (value == 0 or (knob == "skinny_fused_max_k" and value < min(V, H))):
            assert not any(kd >= 1000 for kd in kinds), (knob, value, kinds)
        if B > 64 and knob == "skinny_max_macs" and value == 1 << 40:
            assert all(1000 <= kd < 1100 for kd in kinds[:-1]), (knob, value, kinds)      # (the forward passes)
        if B <= 64:
            assert any(1000 <= kd < 1100 for kd in kinds), (knob, value, kinds)


# ------------------------------------------------------------------ streaming kernel


STREAM_SHAPES = [(1024, 256, 512, 1, False), (2048, 400, 512, 2, True), (530, 77, 97, 1, True)]


@pytest.mark.parametrize("V,H,B,k,gauss", STREAM_SHAPES, ids=["c4_1024_256", "ge_2048_400_cd2", "ragged_530_77"])
def test_every_stream_tile_shape_against_forced_oracle(eng, V, H, B, k, gauss):
    """All nine (stream_mi, stream_ni) settings.  1024 -> 256 at B = 512 has fewer than 384 32 x 32 tiles (auto mi = 1):
    stream_ni = 2 must take 64-row tiles (launch_stream_gemm has no 32 x 64 tile), not fail every pass.  (Oracle only: the
    waves of a tile split K by the tile's shape, so the summation grouping follows the setting.)"""
    for mi in (0, 1, 2):
        for ni in (0, 1, 2):
            r = _cd(eng, V, H, B, k, gauss, dict(small_fused=0, stream_x6=2, stream_mi=mi, stream_ni=ni))
            _oracle("knobs stream tiles", r)
            assert len(r["kinds"]) == 2 * k + 2 and all(1100 <= kd < 2000 for kd in r["kinds"]), ((mi, ni), r["kinds"])


@pytest.mark.parametrize("V,H,B,k,gauss", STREAM_SHAPES, ids=["c4_1024_256", "ge_2048_400_cd2", "ragged_530_77"])
def test_stream_size_limit_zero_keeps_every_pass_off_the_streaming_kernel(eng, V, H, B, k, gauss):
    r = _cd(eng, V, H, B, k, gauss, dict(small_fused=0, stream_max_macs=0))
    _oracle("knobs stream size limit", r)
    assert r["kinds"] and not any(1100 <= kd < 2000 for kd in r["kinds"]), r["kinds"]


# ------------------------------------------------------------------ one-launch step


@pytest.mark.parametrize("V,H,B,gauss", [(100, 24, 4, False), (100, 24, 20, False), (100, 24, 512, False),
                                         (512, 40, 512, True)], ids=["b4", "b20", "b512", "grbm_512_40"])
def test_small_finish_lanes_against_forced_oracle(eng, V, H, B, gauss):
    """small_fin_lanes: threads of the one-launch step's finish kernel that share one sum of the per-workgroup partials (B = 4:
    one partial; 512: 128).  Every setting against the oracle, and each bit for bit from run to run."""
    for lanes in (0, 1, 2, 4, 8, 16):
        a = _cd(eng, V, H, B, 1, gauss, dict(small_fin_lanes=lanes))
        assert a["kinds"] == [], ("not the one-launch step", lanes, a["kinds"])
        _oracle("knobs small finish lanes", a)
        b = _cd(eng, V, H, B, 1, gauss, dict(small_fin_lanes=lanes))
        _same(a, b, "small_fin_lanes=%d repeat" % lanes)


# ------------------------------------------------------------------ training step


TRAIN_SHAPES = [(1024, 512, 256, True, dict(lr=0.002, lambda_2=0.1), dict(stream_x6=0)),
                (1024, 256, 512, False, dict(lr=0.1, weightcost=2e-4), {})]


@pytest.mark.parametrize("V,H,B,gauss,hp,opts", TRAIN_SHAPES, ids=["tiled_1024_512", "stream_1024_256"])
def test_fused_finalize_and_update_are_bitwise_the_separate_kernels(eng, V, H, B, gauss, hp, opts):
    """fused_update applies the update inside the statistics GEMM (or lets the update kernel sum the split-K slabs in
    sum_slabs order), fused_finalize runs the bias statistics / cost finalize there too: the same per-element arithmetic in
    the same order as the separate launches, so every combination equals (1, 1) bit for bit."""
    ref = _train(eng, V, H, B, 1, gauss, hp, dict(opts, fused_finalize=1, fused_update=1))
    for ff, fu in ((1, 0), (0, 1), (0, 0)):
        got = _train(eng, V, H, B, 1, gauss, hp, dict(opts, fused_finalize=ff, fused_update=fu))
        _same_run(got, ref, "fused_finalize=%d fused_update=%d" % (ff, fu))


@pytest.mark.parametrize("V,H,B,gauss,hp,opts", TRAIN_SHAPES, ids=["tiled_1024_512", "stream_1024_256"])
def test_update_overlap_is_bitwise_the_serial_update(eng, V, H, B, gauss, hp, opts):
    """update_overlap runs the finalize and the parameter half of the update on a side stream under the statistics GEMM:
    the parameter half uses the OLD speed (rbm.py:364-365), so the parameters, speeds and costs equal the serial step's."""
    ref = _train(eng, V, H, B, 1, gauss, hp, dict(opts, update_overlap=0))
    got = _train(eng, V, H, B, 1, gauss, hp, dict(opts, update_overlap=1))
    _same_run(got, ref, "update_overlap")


def test_update_overlap_on_a_plane_shape_keeps_w_planes_valid(eng):
    """On a shape the plane path serves, update_overlap takes the training step off the planes (the plane step has no side
    stream); its update must still rewrite W's bf16 planes, which must then hold the exact split of the new W."""
    import torch
    out = _train(eng, 1024, 512, 512, 1, True, dict(lr=0.002, lambda_2=0.1), dict(planes_min_work=0, update_overlap=1))
    assert out[2] and all(kd < 2000 for kd in out[2]), out[2]
    wp, valid = eng.w_planes(out[4])
    assert valid, "W's planes were not kept in step by the overlapped update"
    W = out[4].cpu().numpy().astype(np.float64)
    bits = wp.cpu().view(torch.int16).numpy().astype(np.uint32) & 0xFFFF
    pieces = (bits << 16).view(np.float32).astype(np.float64)
    rows, cols = W.shape
    np.testing.assert_array_equal(pieces[:, :rows, :cols].sum(axis=0), W)


def test_update_overlap_is_refused_with_l1_and_follows_the_oracle(eng):
    """lambda_1 != 0 needs the new speed before the parameters: the step ignores update_overlap (serial rule) -- same bits."""
    hp = dict(lr=0.002, lambda_1=0.01, lambda_2=0.05)
    ref = _train(eng, 1024, 256, 512, 1, True, hp, dict(update_overlap=0))
    got = _train(eng, 1024, 256, 512, 1, True, hp, dict(update_overlap=1))
    _same_run(got, ref, "update_overlap with lambda_1")


@pytest.mark.parametrize("V,H,B,gauss,hp", [(784, 500, 20, False, dict(lr=0.1, weightcost=2e-4)),
                                            (4096, 1024, 512, True, dict(lr=0.001, lambda_2=0.1))],
                         ids=["thin_784_500", "planes_4096_1024"])
def test_gather_ahead_off_is_bitwise_the_same_run(eng, V, H, B, gauss, hp):
    """gather_ahead = 0: every step gathers its own minibatch instead of taking the rows the previous step's kernel gathered
    from next_indexes -- the same rows, so the same bits; the ahead path is taken at 1 only.  (The product run with the
    hints against the oracle: test_gpu_product_defaults.py.)"""
    on = _train(eng, V, H, B, 1, gauss, hp, {}, tapped=False, hints=True)
    off = _train(eng, V, H, B, 1, gauss, hp, dict(gather_ahead=0), tapped=False, hints=True)
    assert on[3] == 3 and off[3] == 0, (on[3], off[3])
    _same_run(off, on, "gather_ahead")
    if V == 784:
        tapped = _train(eng, V, H, B, 1, gauss, hp, {}, tapped=True, hints=True)
        _same_run(on, tapped, "gather_ahead vs the oracle-checked run")


def test_host_feed_copy_streams_are_bitwise_the_device_table(eng):
    """feed_copy_streams: a host-resident table's row feeder (created after the option is set) moves each minibatch as 1 or 2
    copies; the rows, and so the run, are those of a device-resident table."""
    hp = dict(lr=0.1, weightcost=2e-4)
    ref = _train(eng, 784, 500, 20, 1, False, hp, {}, tapped=True)
    for n in (1, 2):
        got = _train(eng, 784, 500, 20, 1, False, hp, dict(feed_copy_streams=n), tapped=False, resident="host")
        _same_run(got, ref, "feed_copy_streams=%d" % n)


# ------------------------------------------------------------------ balanced plane launches


def test_balanced_workgroup_count_against_forced_oracle(eng):
    """bal_blocks: the plane GEMMs launched balanced on exactly that many workgroups (tiles x stages shared evenly, whole
    tiles + shared rests at 7 and 13 workgroups); against the oracle, and bit for bit from run to run."""
    for P in (7, 13, 256):
        a = _cd(eng, 1024, 512, 512, 1, False, dict(planes_min_work=0, bal_blocks=P))
        assert a["kinds"] and all(kd >= 2000 for kd in a["kinds"]), (P, a["kinds"])
        _oracle("knobs balanced workgroups", a)
        b = _cd(eng, 1024, 512, 512, 1, False, dict(planes_min_work=0, bal_blocks=P))
        _same(a, b, "bal_blocks=%d repeat" % P)


# ------------------------------------------------------------------ refusals


def test_refused_values_keep_the_previous_setting(eng):
    """Every invalid value of tests/_knobs.py raises MdbnError and leaves the setting before it in force: a step after the
    refusals equals the step before them bit for bit (same kernels, same bits)."""
    from mdbn_amd import _lib
    for name, e in sorted(KNOBS.items()):
        if not e["invalid"]:
            continue
        probe = next(v for v in e["valid"] if v != e["default"])
        with _options(eng, **{name: probe}):
            before = _cd(eng, 1000, 300, 200, 1, False, {})
            for bad in e["invalid"]:
                with pytest.raises(_lib.MdbnError):
                    eng.set_option(name, bad)
            after = _cd(eng, 1000, 300, 200, 1, False, {})
        assert after["kinds"] == before["kinds"], (name, before["kinds"], after["kinds"])
        _same(after, before, "%s after refusals" % name)
