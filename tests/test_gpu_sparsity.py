"""The sparsity target on the device: (a) the kernels of csrc/mdbn_sparsity.hip alone against the float64 twin
(tests/_sparsity_np.py) fed the device's own inputs, with poisoned pad columns, determinism and every MDBN_EINVAL case;
(b) whole sparse steps through the public classes on every dispatch path of the CD step, alone and with the centred gradient,
against the twin loop teacher-forced along the device's recorded chain; (c) the behaviour cases of tests/test_sparsity_twin.py
on the device, read through RBM.hidden_activity; (d) RBM.hidden_activity itself and a resumed run."""
import ctypes as C
import types

import numpy as np
import pytest

import _center_np as cn
import _sparsity_np as sn
from oracle import rbm_np
from oracle.philox_np import PhiloxDraws
from _margins import check

pytestmark = pytest.mark.gpu

# (V, H, ldh): small and ragged (H % 4 != 0), the smallest behaviour layer, an odd number of rows, whole 16-byte groups of pad
# columns, the widest preset (19937 rows: more row blocks than CUs, 32 rows per block), and rows wider than one pass of a
# workgroup (H > 1024: a thread walks several 16-byte groups of a row)
SHAPES = [(12, 7, 8), (100, 24, 24), (255, 200, 200), (128, 400, 512), (19937, 400, 400), (16, 2500, 2500)]
COST = 1.5
SCALES = [(10 * COST, 10 * COST), (32 * COST, 20 * COST), (0.0, 20 * COST)]
TARGET = 0.3
POISON = float("nan")


def packed(V, H, ldh, seed):
    """-> (stats float32 [V ldh + ldh + ldv + 4] with NaN in every pad column, ldv, mask of the pad entries, q, v_mean)"""
    ldv = (V + 3) & ~3
    rs = np.random.RandomState(seed)
    st = rs.normal(size=V * ldh + ldh + ldv + 4).astype(np.float32)
    pad = np.zeros(st.size, dtype=bool)
    pad[:V * ldh].reshape(V, ldh)[:, H:] = True
    pad[V * ldh + H:V * ldh + ldh] = True
    pad[V * ldh + ldh + V:V * ldh + ldh + ldv] = True
    st[pad] = POISON
    return st, ldv, pad, rs.uniform(size=H).astype(np.float32), rs.uniform(-1, 1, size=V).astype(np.float32)


def bits(t):
    return t.detach().cpu().numpy().view(np.int32).copy()


def dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


# ------------------------------------------------------------------------------------------------------------------ (a) kernels
@pytest.mark.parametrize("w_scale,b_scale", SCALES)
@pytest.mark.parametrize("V,H,ldh", SHAPES)
def test_sparsity_stats_against_the_twin(hip_engine, V, H, ldh, w_scale, b_scale):
    eng = hip_engine
    st, ldv, pad, q, v_mean = packed(V, H, ldh, seed=V + H)
    d, dq, dv = dev(eng, st), dev(eng, q), dev(eng, v_mean)
    eng.sparsity_stats(d, V, H, ldv, ldh, dq, dv if w_scale else None, TARGET, w_scale, b_scale)
    out = d.cpu().numpy()
    S, s_h, s_v, cost = cn.unpack(st, V, H, ldv, ldh)
    S2, sh2, _ = sn.stats(S, s_h, s_v, q, v_mean, TARGET, w_scale, b_scale)
    gS, gsh, gsv, gcost = cn.unpack(out, V, H, ldv, ldh)
    tag = "sparsity_stats %dx%d" % (V, H)
    check(tag + ": S' / max|S'|", np.abs(gS - S2).max() / np.abs(S2).max(), 1e-5, "stats")
    check(tag + ": s_h' / max|s_h'|", np.abs(gsh - sh2).max() / np.abs(sh2).max(), 1e-5, "stats")
    # pad columns, s_v and the cost floats: bit-unchanged; q and v_mean are inputs only
    assert np.array_equal(out.view(np.int32)[pad], st.view(np.int32)[pad]), "a pad column was written"
    assert np.isfinite(out[~pad]).all(), "a pad column was read"
    lo = V * ldh + ldh
    assert np.array_equal(out[lo:].view(np.int32), st[lo:].view(np.int32)), "s_v or the cost floats were touched"
    assert np.array_equal(dq.cpu().numpy(), q) and np.array_equal(dv.cpu().numpy(), v_mean)
    if w_scale == 0.0:
        assert np.array_equal(out[:V * ldh].view(np.int32), st[:V * ldh].view(np.int32)), "w_scale = 0 touched S"
        assert not np.array_equal(gsh, s_h)
    # a second run on the same inputs: bit-identical
    d2 = dev(eng, st)
    eng.sparsity_stats(d2, V, H, ldv, ldh, dq, dv if w_scale else None, TARGET, w_scale, b_scale)
    assert np.array_equal(bits(d2), out.view(np.int32)), "two runs differ"


@pytest.mark.parametrize("V,H,ldh", SHAPES)
def test_zero_scales_return_the_buffer_bit_for_bit(hip_engine, V, H, ldh):
    eng = hip_engine
    st, ldv, pad, q, v_mean = packed(V, H, ldh, seed=3)
    d = dev(eng, st)
    eng.sparsity_stats(d, V, H, ldv, ldh, dev(eng, q), dev(eng, v_mean), TARGET, 0.0, 0.0)
    assert np.array_equal(bits(d), st.view(np.int32))
    # ... and a unit at the target adds an exact zero
    eng.sparsity_stats(d, V, H, ldv, ldh, dev(eng, np.full(H, TARGET, np.float32)), dev(eng, v_mean), TARGET, 15.0, 30.0)
    out = d.cpu().numpy()
    assert np.array_equal(out[~pad], st[~pad]) and np.array_equal(out.view(np.int32)[pad], st.view(np.int32)[pad])


@pytest.mark.parametrize("B", [1, 20, 33, 512])
@pytest.mark.parametrize("V,H,ldh", [(12, 7, 8), (255, 200, 200), (4096, 1024, 1024)])
def test_sparsity_activity_against_the_twin(hip_engine, V, H, ldh, B):
    eng = hip_engine
    rs = np.random.RandomState(B + V)
    ldv = (V + 3) & ~3
    V2 = np.full((2 * B, ldv), POISON, dtype=np.float32)
    P2 = np.full((2 * B, ldh), POISON, dtype=np.float32)
    V2[:B, :V] = rs.normal(size=(B, V)) if V == 255 else (rs.uniform(size=(B, V)) < 0.3)
    P2[:B, :H] = rs.uniform(size=(B, H))
    sc = types.SimpleNamespace(V2=dev(eng, V2)[:, :V], P2=dev(eng, P2)[:, :H])
    q0, m0 = rs.uniform(size=H).astype(np.float32), rs.uniform(size=V).astype(np.float32)
    for rate in (1.0, 0.1):
        dq, dm = dev(eng, q0), dev(eng, m0)
        eng.sparsity_activity(sc, B, dq, dm, rate)
        q, m = sn.activity(q0, V2[:B, :V], P2[:B, :H], rate)
        check("sparsity_activity: q", np.abs(dq.cpu().numpy() - q).max(), 2e-6)
        check("sparsity_activity: v_mean", np.abs(dm.cpu().numpy() - m).max(), 2e-6)
        again_q, again_m = dev(eng, q0), dev(eng, m0)
        eng.sparsity_activity(sc, B, again_q, again_m, rate)
        assert np.array_equal(bits(again_q), bits(dq)) and np.array_equal(bits(again_m), bits(dm)), "two runs differ"
        # the hidden-only form: the same bits of q, and scratch.V2 is not looked at
        only_q = dev(eng, q0)
        eng.sparsity_activity(types.SimpleNamespace(P2=sc.P2), B, only_q, None, rate)
        assert np.array_equal(bits(only_q), bits(dq)), "the hidden-only form gives another q"
    if B == 1:          # rate = 1 on one row: the means ARE that row
        dq, dm = dev(eng, q0), dev(eng, m0)
        eng.sparsity_activity(sc, 1, dq, dm, 1.0)
        assert np.array_equal(dq.cpu().numpy(), P2[0, :H]) and np.array_equal(dm.cpu().numpy(), V2[0, :V])


def test_every_einval_case_returns_without_touching_its_outputs(hip_engine):
    import torch
    from mdbn_amd import _lib
    eng, lib = hip_engine, hip_engine.lib
    V, H, ldh, B = 100, 24, 24, 20
    st, ldv, _, q, v_mean = packed(V, H, ldh, seed=1)
    room = dev(eng, np.concatenate([st, np.zeros(8, np.float32)]))       # (room for a misaligned view of the same size)
    d, dq, dm = room[:st.size], dev(eng, q), dev(eng, v_mean)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    nan, inf = float("nan"), float("inf")

    def stats_call(stats=d, V=V, H=H, ldv=ldv, ldh=ldh, q=dq, v_mean=dm, target=0.3, w=15.0, b=30.0, ctx=eng.ctx):
        return lib.mdbn_sparsity_stats(ctx, eng._stream(), p(stats), V, H, ldv, ldh, p(q), p(v_mean), target, w, b)

    before = (bits(room), bits(dq), bits(dm))
    bad = [dict(V=0), dict(H=0), dict(V=-3), dict(H=-1), dict(stats=None), dict(q=None), dict(v_mean=None), dict(ctx=None),
           dict(stats=room[1:1 + st.size]), dict(q=dq.view(torch.uint8)[1:]), dict(v_mean=dm.view(torch.uint8)[2:]),
           dict(ldh=H - 4), dict(ldh=H + 2), dict(ldv=V - 4), dict(ldv=V + 2),
           dict(target=0.0), dict(target=1.0), dict(target=-0.2), dict(target=1.5), dict(target=nan),
           dict(w=-1.0), dict(w=nan), dict(w=inf), dict(b=-1.0), dict(b=nan), dict(b=inf)]
    for kw in bad:
        assert stats_call(**kw) == -1, kw
        assert _lib.last_error(), kw
    eng.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(before, (bits(room), bits(dq), bits(dm)))), "a refused call wrote something"
    assert stats_call(w=0.0, b=0.0) == 0 and stats_call(w=0.0, b=0.0, v_mean=None) == 0     # nothing to do: no launch
    eng.synchronize()
    assert np.array_equal(bits(room), before[0])

    v0 = torch.rand((B + 1, ldv), dtype=torch.float32, device=eng.device)
    ph = torch.rand((B + 1, ldh), dtype=torch.float32, device=eng.device)

    def act_call(ph=ph, ldh=ldh, v0=v0, ldv=ldv, B=B, V=V, H=H, rate=0.5, q=dq, v_mean=dm, ctx=eng.ctx):
        return lib.mdbn_sparsity_activity(ctx, eng._stream(), p(ph), ldh, p(v0), ldv, B, V, H, rate, p(q), p(v_mean))

    bad = [dict(B=0), dict(V=0), dict(H=0), dict(B=-1), dict(ph=None), dict(q=None), dict(ctx=None), dict(v0=None), dict(v_mean=None),
           dict(rate=0.0), dict(rate=-0.5), dict(rate=1.5), dict(rate=nan), dict(v0=v0.reshape(-1)[1:]), dict(ph=ph.reshape(-1)[1:]),
           dict(q=dq.view(torch.uint8)[1:]), dict(v_mean=dm.view(torch.uint8)[2:]),
           dict(ldv=V - 4), dict(ldh=H - 4), dict(ldv=V + 2), dict(ldh=H + 2)]
    for kw in bad:
        assert act_call(**kw) == -1, kw
        assert _lib.last_error(), kw
    eng.synchronize()
    assert np.array_equal(bits(dq), before[1]) and np.array_equal(bits(dm), before[2]), "a refused call wrote something"
    # ... and the good calls go through; without v0 / v_mean the visible size and its leading dimension are ignored
    assert act_call() == 0 and stats_call() == 0
    assert act_call(v0=None, v_mean=None, V=0, ldv=0) == 0 and stats_call(w=0.0, v_mean=None) == 0
    eng.synchronize()
    assert not np.array_equal(bits(dq), before[1]) and not np.array_equal(bits(dm), before[2])
    assert not np.array_equal(bits(room), before[0])


# ------------------------------------------------------------------------------------------------------------------ (b) whole steps
TILED_F32 = dict(stream_x6=0, skinny_gemm=0, gemm_bf16x6=0, small_fused=0, thin_fused=0)
SMALL_PLANES = dict(planes_min_work=0)              # the plane path at every whole-tile shape, as the hip_engine fixture
CASES = [  # id, V, H, B, k, gauss, persistent, centred, hyper-parameters, engine options, path of the run
    ("small_one_launch", 100, 24, 512, 1, False, False, False, dict(lr=0.1, weightcost=2e-4), {}, "small"),
    ("small_one_launch_centred", 100, 24, 512, 1, False, False, True, dict(lr=0.1, weightcost=2e-4), {}, "small"),
    ("thin_batch20", 784, 500, 20, 1, False, False, False, dict(lr=0.1, weightcost=2e-4), {}, "thin"),
    ("stream_small_layer", 256, 200, 512, 2, True, False, False, dict(lr=0.002, lambda_2=0.1), {}, "stream"),
    ("stream_small_layer_centred", 256, 200, 512, 2, True, False, True, dict(lr=0.002, lambda_2=0.1), {}, "stream"),
    ("tiled_f32_ragged", 250, 130, 99, 1, False, False, False, dict(lr=0.1, weightcost=2e-4), TILED_F32, "tiled_f32"),
    ("pcd_batch20", 784, 500, 20, 1, False, True, False, dict(lr=0.1, weightcost=2e-4), {}, "f32_operands"),
    ("planes_small", 1024, 512, 256, 1, True, False, False, dict(lr=0.001, lambda_2=0.1), SMALL_PLANES, "planes"),
]
STEPS = 4
NAMES = ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed")
SPARSITY = dict(sparsity_target=0.2, sparsity_cost=1.0, sparsity_decay=0.9)


def _run(eng, V, H, B, k, gauss, persistent, centered, hp, tapped):
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
    center = dict(centered=True, offset_rate=0.05) if centered else {}
    _, updates = rbm.get_cost_updates(k=k, batch_size=B, persistent=chain, **dict(hp, **dict(SPARSITY, **center)))
    fn = mdbn_amd.function(updates, mdbn_amd.shared(data, engine=eng), data_parallel=None)
    order = [eng.index_tensor(rs.permutation(N)[:B], N) for _ in range(STEPS + 1)]
    eng.trace_chain = tapped
    eng.kernel_timing(True)
    costs, state, scratch = [], None, []
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
                # what sparsity_activity reads: the float32 copies of v0 and ph_mean, on every path
                assert np.array_equal(V2, v0.astype(np.float32)), "rows 0..B-1 of V2 are not v0"
                check("sparse step: ph_mean in P2", np.abs(P2 - ph).max(), 2e-6, "prob")
                if persistent:
                    want = rbm_np.pseudo_likelihood_cost(st, v0)
                    st.bit_i_idx = (st.bit_i_idx + 1) % V
                    check("sparse step (PCD): cost rel", abs(float(c) - want) / abs(want), 1e-4)
                    assert np.array_equal(updates.persistent.get_value(), forced[0][k]), "chain != recorded nh_sample"
                else:
                    want = rbm_np.reconstruction_cost(st, out[0], v0)
                    check("sparse step: cost rel", abs(float(c) - want) / abs(want), 1e-5)
                state = sn.sparse_update(st, state, v0, ph, out[1], out[4], B, hp["lr"], SPARSITY["sparsity_target"],
                                         SPARSITY["sparsity_cost"], decay=SPARSITY["sparsity_decay"], centered=centered, nu=0.05,
                                         momentum=mom, **twin_hp)
            costs.append(float(c))
        eng.synchronize()
        kinds = [kd for _, _, _, kd in eng.kernel_timing_detail()]
    finally:
        eng.kernel_timing(False)
        eng.trace_chain = False
    params = {n: getattr(rbm, n).get_value() for n in NAMES}
    params["h_activity"] = rbm.h_activity.get_value()
    if centered:
        params["v_offset"], params["h_offset"] = rbm.v_offset.get_value(), rbm.h_offset.get_value()
    return params, np.array(costs), kinds, scratch, st, state


@pytest.mark.parametrize("name,V,H,B,k,gauss,persistent,centered,hp,opts,path", CASES, ids=[c[0] for c in CASES])
def test_sparse_steps_on_every_dispatch_path(built_lib, name, V, H, B, k, gauss, persistent, centered, hp, opts, path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mdbn_amd
    eng = mdbn_amd.HipEngine()                     # product defaults but for `opts`; keep_f32 stays off
    for key, value in opts.items():
        if key == "planes_min_work":
            eng.set_planes_min_work(value)
        else:
            eng.set_option(key, value)
    assert not eng.keep_f32
    tapped, tcosts, _, tscratch, st, state = _run(eng, V, H, B, k, gauss, persistent, centered, hp, tapped=True)
    errs = [(pname, np.abs(tapped[pname] - getattr(st, pname)).max() / max(1.0, np.abs(getattr(st, pname)).max())) for pname in NAMES]
    errs += [("h_activity", np.abs(tapped["h_activity"] - state["q"]).max())]
    if centered:
        errs += [("v_offset", np.abs(tapped["v_offset"] - state["offsets"][0]).max()),
                 ("h_offset", np.abs(tapped["h_offset"] - state["offsets"][1]).max())]
    print("%s: %s" % (name, ", ".join("%s %.3e" % e for e in errs)))         # every figure before the first assertion
    for pname, err in errs[:len(NAMES)]:
        check("sparse step %s: %s after %d steps / max" % (name, pname, STEPS), err, 2e-6, "update")
    for pname, err in errs[len(NAMES):]:
        check("sparse step %s: %s" % (name, pname), err, 2e-6)
    # the same run without chain taps: the path it takes, and the same bits (keep_f32 of the call alone gives v0 / ph_mean)
    plain, pcosts, kinds, pscratch, _, _ = _run(eng, V, H, B, k, gauss, persistent, centered, hp, tapped=False)
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


# ------------------------------------------------------------------------------------------------------------------ (c) behaviour
@pytest.mark.parametrize("case,sparsity,target,measured", sn.BEHAVIOUR_RUNS,
                         ids=["%s-%s" % (r[0], "plain" if not r[1] else "cost%g%s" % (r[1]["cost"], "" if r[1].get("weights", True) else "-bias-only"))
                              for r in sn.BEHAVIOUR_RUNS])
def test_the_penalty_moves_the_activities_to_the_target_on_the_device(hip_engine, case, sparsity, target, measured):
    """The runs of tests/test_sparsity_twin.py through the public classes: the same data, minibatches, schedule and bounds.
    The device's chain leaves the oracle's after the first tie, so the figures differ from the twin's; the bounds hold."""
    import mdbn_amd
    eng = hip_engine
    c = sn.BEHAVIOUR[case]
    data = sn.behaviour_data(c["gauss"]).astype(np.float32)
    cls = mdbn_amd.GRBM if c["gauss"] else mdbn_amd.RBM
    rbm = cls(n_visible=sn.BEHAVIOUR_V, n_hidden=sn.BEHAVIOUR_H, numpy_rng=np.random.RandomState(123),
              theano_rng=mdbn_amd.RandomStreams(7), engine=eng)
    kw = {"sparsity_" + key: value for key, value in sparsity.items()}
    _, updates = rbm.get_cost_updates(lr=c["lr"], k=1, batch_size=sn.BEHAVIOUR_B, **dict(c["hyper"], **kw))
    fn = mdbn_amd.function(updates, mdbn_amd.shared(data, engine=eng), data_parallel=None)
    batches = [eng.index_tensor(sn.behaviour_batch(t), len(data)) for t in range(sn.BEHAVIOUR_ROWS // sn.BEHAVIOUR_B)]
    for t in range(c["steps"]):
        fn(indexes=batches[t % len(batches)], momentum=sn.behaviour_momentum(t))
    act = rbm.hidden_activity(data)
    assert (rbm.h_activity is not None) == bool(sparsity)
    figure, ok = sn.behaviour_holds(act, sparsity, target, measured)
    print("%s %r: activations %.4f .. %.4f, figure %.4f (the twin's %.4f)" % (case, sparsity, act.min(), act.max(), figure, measured))
    tag = "sparsity behaviour %s %s" % (case, ", ".join("%s %g" % kv for kv in sorted(sparsity.items())) or "plain")
    if sparsity:
        check(tag + ": farthest unit from the target", figure, 2.0 * measured)
    else:
        check(tag + ": half the twin's distance / nearest unit's distance", 0.5 * measured / figure, 1.0)
    assert ok


# ------------------------------------------------------------------------------------------------------------------ (d)
def test_hidden_activity_against_the_float64_formula(hip_engine):
    import mdbn_amd
    eng = hip_engine
    V, H, N = 784, 500, 1000
    rs = np.random.RandomState(9)
    data = (rs.uniform(size=(N, V)) < 0.3).astype(np.float32)
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(123), theano_rng=mdbn_amd.RandomStreams(7), engine=eng)
    rbm.hbias.set_value(rs.normal(scale=0.5, size=H).astype(np.float32))
    step0 = rbm._rng_step
    chunked = rbm.hidden_activity(data, chunk_rows=384)          # 384 + 384 + 232 rows
    whole = rbm.hidden_activity(data)
    assert chunked.dtype == np.float32 and chunked.shape == (H,) and rbm._rng_step == step0
    want = rbm_np.sigmoid(data.astype(np.float64) @ rbm.W.get_value().astype(np.float64) + rbm.hbias.get_value().astype(np.float64)).mean(0)
    # 2e-6 for the probabilities plus 2e-6 for the mean of them
    check("hidden_activity 784x500, 1000 rows in chunks of 384", np.abs(chunked - want).max(), 4e-6, "prob")
    check("hidden_activity 784x500, 1000 rows at once", np.abs(whole - want).max(), 4e-6, "prob")
    check("hidden_activity: chunked against unchunked", np.abs(chunked.astype(np.float64) - whole).max(), 1e-6)
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[64], n_outs=16, gauss=False, engine=eng)
    acts = net.hidden_activity(data)
    h1 = rbm_np.sigmoid(data.astype(np.float64) @ net.rbm_layers[0].W.get_value().astype(np.float64) + net.rbm_layers[0].hbias.get_value())
    h2 = rbm_np.sigmoid(h1 @ net.rbm_layers[1].W.get_value().astype(np.float64) + net.rbm_layers[1].hbias.get_value())
    check("DBN.hidden_activity: layer 0", np.abs(acts[0] - h1.mean(0)).max(), 4e-6, "prob")
    check("DBN.hidden_activity: layer 1", np.abs(acts[1] - h2.mean(0)).max(), 4e-6, "prob")


def test_a_resumed_sparse_and_centred_run_continues_bit_for_bit(hip_engine, tmp_path):
    import mdbn_amd
    from mdbn_amd import checkpoint
    mdbn_amd.DBN.verbose = False
    eng = hip_engine
    rs = np.random.RandomState(0)
    V, H = 96, 40
    x = rs.normal(size=(40, V)).astype(np.float32)
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[], n_outs=H, engine=eng)
    rbm = net.rbm_layers[0]
    plan = dict(k=1, lambda_2=0.1, batch_size=10, centered=True, sparsity_target=0.2, sparsity_cost=2.0)
    _, up = rbm.get_cost_updates(0.005, **plan)
    fn = mdbn_amd.function(up, mdbn_amd.shared(x, engine=eng), data_parallel=None)
    for t in range(2):
        fn(indexes=np.arange(10) + 10 * t, momentum=0.5)
    path = str(tmp_path / "sparse.npz")
    checkpoint.save_network(path, {'ge': net}, resume=True)
    want = [float(fn(indexes=np.arange(10) + 10 * t, momentum=0.5)) for t in (2, 3)]
    r2 = checkpoint.load_network(path, engine=eng)['ge'].rbm_layers[0]
    assert r2.h_activity is not None and r2.v_offset is not None
    _, up2 = r2.get_cost_updates(0.005, **plan)
    fn2 = mdbn_amd.function(up2, mdbn_amd.shared(x, engine=eng), data_parallel=None)
    got = [float(fn2(indexes=np.arange(10) + 10 * t, momentum=0.5)) for t in (2, 3)]
    assert got == want
    for n in NAMES + ("v_offset", "h_offset", "h_activity"):
        assert np.array_equal(getattr(r2, n).get_value(), getattr(rbm, n).get_value()), n
