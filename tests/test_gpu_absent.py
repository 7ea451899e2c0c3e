"""The absent visible units on the device against the float64 twin (tests/_absent_np.py): (a) the row kernels on the shared
kernel cases, (b) mdbn_cd_step_absent teacher-forced along its own traces on the GEMM families of tests/test_gpu_disc.py, on
a workspace of exactly its sizer's bytes, and against mdbn_cd_step_grouped / mdbn_cd_step with nothing missing, (c) refused
calls, (d) mdbn_free_energy_absent, (e) the public path."""
import ctypes as C
import types

import numpy as np
import pytest

import _absent_np as an
import _step_forms as sf
from _center_np import unpack
from _margins import SURVEY, check
from oracle import rbm_np
from oracle.philox_np import PhiloxDraws

pytestmark = pytest.mark.gpu

POISON = float("nan")
PARAMS = ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed")
TILED_X6 = dict(stream_x6=0, skinny_gemm=0, small_fused=0, thin_fused=0, x6_min_jobs=0, gemm_bf16x6=3)
GUARD = 1024


def bits(t):
    return t.detach().cpu().numpy().view(np.int32).copy()


def padded(eng, a, ld, fill=POISON):
    import torch
    a = np.atleast_2d(np.asarray(a, dtype=np.float32))
    full = np.full((a.shape[0], ld), fill, dtype=np.float32)
    full[:, :a.shape[1]] = a
    return torch.from_numpy(full).to(eng.device)


def guard_scratch(eng):
    """Every workspace the engine's absent calls ask for becomes exactly the sizer's bytes with a guard behind it (the engine
    tells the library the sizer's figure).  -> check(): every guard is untouched."""
    import torch
    made = []

    def sized(attr, need):
        ws = torch.full((need // 4 + GUARD,), POISON, dtype=torch.float32, device=eng.device)
        ws[need // 4:] = 12345.0
        made.append((ws, need // 4))
        return ws
    eng._sized_scratch = sized
    return lambda: bool(made) and all((ws[n:] == 12345.0).all().item() for ws, n in made)


# ------------------------------------------------------------------------------------------------------------------ (a) kernels
@pytest.mark.parametrize("V,ldv,B", an.KERNEL_CASES)
def test_split_is_exact(hip_engine, V, ldv, B):
    import torch
    eng = hip_engine
    x, _, _ = an.case_inputs(V, B, True)
    if B > 1:
        x[B - 1, V - 1] = np.inf                                    # a value, not a marker
    late = early = None
    if V > an.COUNT_TRIP:
        # the count kernel's lanes come round again from column 2048 on: a row observed only there (dropped words would count
        # it 0, and absent_mark_rows would then make it a row of NaN), one observed only before, and row 0, wholly absent
        late, early = 1, 2
        x[late, :an.COUNT_TRIP], x[late, an.COUNT_TRIP:] = np.nan, 1.5
        x[early, :an.COUNT_TRIP] = np.nan_to_num(x[early, :an.COUNT_TRIP], nan=0.5)
        x[early, an.COUNT_TRIP:] = np.nan
    filled_w, mask, words, count = an.split(x)
    if late is not None:
        assert count[0] == 0 and count[late] == V - an.COUNT_TRIP and count[early] > 0 and not mask[early, an.COUNT_TRIP:].any()
    src = padded(eng, x, ldv)
    out = padded(eng, np.full((B, V), 7.0), ldv)
    obs = torch.full((B, words.shape[1]), -1, dtype=torch.int32, device=eng.device)
    cnt = torch.full((B,), -1, dtype=torch.int32, device=eng.device)
    rc = eng.lib.mdbn_absent_split(eng.ctx, eng._stream(), C.c_void_p(src.data_ptr()), B, ldv, V, C.c_void_p(out.data_ptr()), ldv,
                                   C.c_void_p(obs.data_ptr()), C.c_void_p(cnt.data_ptr()))
    assert rc == 0
    eng.synchronize()
    assert np.array_equal(obs.cpu().numpy().view(np.uint32), words) and np.array_equal(cnt.cpu().numpy(), count)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :V].view(np.int32)[mask], x.view(np.int32)[mask]) and (got[:, :V][~mask] == 0).all()
    assert np.isnan(got[:, V:]).all() and np.array_equal(bits(src), bits(padded(eng, x, ldv)))
    # in place, without the count
    obs2 = torch.zeros_like(obs)
    assert eng.lib.mdbn_absent_split(eng.ctx, eng._stream(), C.c_void_p(src.data_ptr()), B, ldv, V, C.c_void_p(src.data_ptr()), ldv,
                                     C.c_void_p(obs2.data_ptr()), None) == 0
    eng.synchronize()
    assert np.array_equal(bits(src), bits(out)) and np.array_equal(bits(obs2), bits(obs))
    # rows nobody observed become NaN
    y = padded(eng, np.ones((B, V)), ldv, fill=3.0)
    eng.absent_mark_rows(y[:, :V], cnt)
    eng.synchronize()
    got = y.cpu().numpy()
    assert np.array_equal(np.isnan(got[:, :V]).all(axis=1), count == 0) and (got[count > 0][:, :V] == 1).all() and (got[:, V:] == 3).all()
    if late is not None:
        dev = cnt.cpu().numpy()
        assert dev[late] == count[late] and dev[early] == count[early] and dev[0] == 0
        assert (got[late, :V] == 1).all() and (got[early, :V] == 1).all() and np.isnan(got[0, :V]).all(), "a row observed late became NaN"


@pytest.mark.parametrize("variant,gauss,noise", an.VARIANTS, ids=[v[0] for v in an.VARIANTS])
@pytest.mark.parametrize("V,ldv,B", an.KERNEL_CASES)
def test_visible_against_the_twin(hip_engine, V, ldv, B, variant, gauss, noise):
    import torch
    from mdbn_amd.engine import RngAddr
    eng = hip_engine
    x, pre, seed = an.case_inputs(V, B, gauss)
    U, Z = an.case_draws(V, B, seed)
    v0, mask, words, _ = an.split(x)
    want_mean, want_sample = an.visible(pre, mask, gauss, noise, U, Z)
    want_cost = an.cost(pre, v0, mask, gauss)
    rng = RngAddr(seed, an.STREAM, an.STEP, an.DRAW, an.ROW_OFFSET).c()
    obs = torch.from_numpy(words.view(np.int32).copy()).to(eng.device)
    n = C.c_int64()
    assert eng.lib.mdbn_absent_visible_workspace_bytes(eng.ctx, B, V, C.byref(n)) == 0 and n.value > 0

    def run(in_place):
        d_pre = padded(eng, pre, ldv)
        mean = d_pre if in_place else padded(eng, np.full((B, V), 5.0), ldv)
        sample, tap = padded(eng, np.full((B, V), 5.0), ldv), padded(eng, np.full((B, V), 5.0), ldv)
        d_v0 = padded(eng, v0, ldv)
        cost = torch.full((4,), POISON, dtype=torch.float32, device=eng.device)
        ws = torch.full((n.value // 4 + GUARD,), 12345.0, dtype=torch.float32, device=eng.device)
        rc = eng.lib.mdbn_absent_visible(eng.ctx, eng._stream(), C.c_void_p(d_pre.data_ptr()), B, ldv, V, C.c_void_p(obs.data_ptr()),
                                         int(gauss), int(noise), C.c_void_p(mean.data_ptr()), C.c_void_p(sample.data_ptr()),
                                         C.c_void_p(tap.data_ptr()), C.byref(rng), C.c_void_p(d_v0.data_ptr()), C.c_void_p(cost.data_ptr()),
                                         C.c_void_p(ws.data_ptr()), n.value)
        assert rc == 0
        eng.synchronize()
        assert (ws[n.value // 4:] == 12345.0).all().item(), "the guard behind the workspace was written"
        return mean, sample, tap, cost
    mean, sample, tap, cost = run(False)
    gm, gs, gt = mean.cpu().numpy(), sample.cpu().numpy(), tap.cpu().numpy()
    for g in (gm, gs, gt):
        assert np.isnan(g[:, V:]).all(), "a pad column was written"
        assert (g[:, :V][~mask] == 0).all(), "an absent entry is not 0"
    assert np.array_equal(gs.view(np.int32), gt.view(np.int32))
    mean_err = np.abs(gm[:, :V] - want_mean).max()
    cost_err = abs(float(cost[0]) - want_cost) / max(abs(want_cost), 1e-30) if mask.any() else abs(float(cost[0]))
    tag = "absent_visible %s V=%d B=%d" % (variant, V, B)
    if gauss:
        sample_err = np.abs(gs[:, :V] - want_sample).max()
        print("%s: mean %.3e, sample %.3e, cost rel %.3e" % (tag, mean_err, sample_err, cost_err))
        check(tag + ": sample", sample_err, 1e-4)
    else:
        differ = gs[:, :V] != want_sample
        gap = np.abs(U.astype(np.float64) - want_mean)[differ].max() if differ.any() else 0.0
        print("%s: mean %.3e, %d draws differ (largest |u - mean| %.3e), cost rel %.3e" % (tag, mean_err, differ.sum(), gap, cost_err))
        assert np.isin(gs[:, :V], (0.0, 1.0)).all() and gap < an.MEAN_TOL and differ.sum() <= an.TIE_CAP
    check(tag + ": mean", mean_err, SURVEY["prob"], "prob")
    check(tag + ": cost rel", cost_err, 1e-5)
    again = run(False)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(again, (mean, sample, tap, cost))), "two runs differ"
    inplace = run(True)
    assert np.array_equal(bits(inplace[0]), bits(mean)) and np.array_equal(bits(inplace[1]), bits(sample))


@pytest.mark.parametrize("V,ldv,B", an.KERNEL_CASES)
def test_with_every_bit_set_the_bernoulli_output_is_propdowns(hip_engine, V, ldv, B):
    from mdbn_amd.engine import RngAddr
    eng = hip_engine
    rs = np.random.RandomState(V + B)
    H = 16
    W = eng.to_device((0.5 * rs.normal(size=(V, H))).astype(np.float32))
    vb = eng.to_device((0.5 * rs.normal(size=V)).astype(np.float32))
    h = eng.to_device((rs.uniform(size=(B, H)) < 0.5).astype(np.float32))
    rng = RngAddr(an.case_seed(V, B), an.STREAM, an.STEP, an.DRAW, an.ROW_OFFSET)
    pre, mean, sample = eng.propdown(h, W, vb, gauss=False, rng=rng)
    _, obs, count = eng.absent_split(eng.alloc_matrix(B, V))
    got_mean, got_sample = eng.absent_visible(pre, obs, rng=rng)
    eng.synchronize()
    assert (count.cpu().numpy() == V).all()
    assert np.array_equal(bits(got_mean), bits(mean)) and np.array_equal(bits(got_sample), bits(sample))


# ------------------------------------------------------------------------------------------------------------------ (b) the step
# id, V, H, B, k, gauss, noise, engine options: the shapes of tests/test_gpu_disc.py's statistics cases
STEP_CASES = [
    ("odd_small", 21, 37, 33, 2, False, False, {}),
    ("skinny_thin", 794, 500, 20, 1, False, False, {}),
    ("stream_gauss", 256, 200, 512, 1, True, False, {}),
    ("tiled_f32_noise", 250, 130, 99, 3, True, True, sf.TILED_F32),
    ("tiled_x6", 250, 130, 99, 3, False, False, TILED_X6),
    ("whole_tile", 128, 128, 32, 1, False, False, {}),
]


def step_table(V, B, gauss, seed, holes=True):
    rs = np.random.RandomState(seed)
    N = B + 5
    x = rs.normal(size=(N, V)).astype(np.float32) if gauss else (rs.uniform(size=(N, V)) < 0.35).astype(np.float32)
    idx = rs.permutation(N)[:B]
    if holes:
        x[rs.uniform(size=(N, V)) < 0.3] = np.nan
        x[idx[0], :] = np.nan                                       # a wholly-absent row
        x[idx[-1], :] = np.nan_to_num(x[idx[-1], :], nan=1.0)       # a wholly-observed row
    return x, idx


@pytest.mark.parametrize("name,V,H,B,k,gauss,noise,opts", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_step_against_the_teacher_forced_twin(built_lib, name, V, H, B, k, gauss, noise, opts):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mdbn_amd
    from mdbn_amd.engine import RngAddr
    eng = sf.set_options(mdbn_amd.HipEngine(), opts)
    guards_ok = guard_scratch(eng)
    rs = np.random.RandomState(V + H)
    # (the ``update`` bound is absolute: it presumes gradient entries S / B of order 1, as a layer in training has them.  A
    #  Gaussian layer's linear means grow with the weights -- at scale 0.3 and H = 130 the noisy k = 3 chain reaches |S| / B
    #  of 30 and more --, so the Gaussian cases take weights of scale 0.1; max |S| / B is printed with the other figures)
    scale = 0.1 if gauss else 0.3
    W = (scale * rs.normal(size=(V, H))).astype(np.float32)
    hb, vb = (scale * rs.normal(size=H)).astype(np.float32), (scale * rs.normal(size=V)).astype(np.float32)
    dW, dhb, dvb = eng.to_device(W), eng.to_device(hb), eng.to_device(vb)
    x, idx = step_table(V, B, gauss, seed=B)
    data = eng.to_device(x)
    ldv, ldh = data.stride(0), dW.stride(0)
    rng = RngAddr(1234, 5, 7, 0, 2)
    eng.trace_chain = True
    stats, sc = eng.cd_step_absent(data, idx, dW, dhb, dvb, gauss, k, rng, add_noise=noise, stats=eng.new_stats_buffer(V, H, ldv, ldh))
    eng.synchronize()
    assert guards_ok(), "the guard behind the exact-size workspace was written"
    s = rbm_np.RBMState(V, H, W=W, hbias=hb, vbias=vb, gauss=gauss)
    s.error_free = not noise
    S, s_h, s_v, cost, (v0, mask, ph, nv, nh, flips) = an.cd_step_absent(
        s, x[idx].astype(np.float64), PhiloxDraws(1234, 5, 7, 2), k, trace_h=sc.trace_h.cpu().numpy()[:, :, :H],
        trace_v=sc.trace_v.cpu().numpy()[:, :, :V])
    E = 2e-6 * B * (H * k + (0 if gauss else V * k))
    assert flips <= int(3 + E + 4 * np.sqrt(E))
    gS, gsh, gsv, gcost = unpack(stats.cpu().numpy(), V, H, ldv, ldh)
    V2, P2 = sc.V2.cpu().numpy(), sc.P2.cpu().numpy()
    tag = "absent step %s" % name
    figures = [("S / max|S|", np.abs(gS - S).max() / np.abs(S).max()), ("s_h / max|s_h|", np.abs(gsh - s_h).max() / np.abs(s_h).max()),
               ("s_v / max|s_v|", np.abs(gsv - s_v).max() / np.abs(s_v).max()), ("cost rel", abs(gcost[0] - cost) / abs(cost))]
    print(tag + ": " + ", ".join("%s %.3e" % f for f in figures) + ", %d draws differ, max|S| / B %.3g" % (flips, np.abs(S).max() / B))
    for what, value in figures[:3]:
        check("%s: %s" % (tag, what), value, 1e-5, "stats")
    check(tag + ": cost rel", figures[3][1], 1e-5)
    assert (V2[:B][~mask] == 0).all() and (V2[B:][~mask] == 0).all() and (sc.vs.cpu().numpy()[~mask] == 0).all()
    assert not mask[0].any() and np.array_equal(P2[0].view(np.int32), (-P2[B]).view(np.int32)), "a wholly-absent row: ph != nh"
    # the unchanged update rule on these statistics
    speeds = [0.01 * rs.normal(size=t.shape).astype(np.float32) for t in (W, hb, vb)]
    s.W_speed, s.hbias_speed, s.vbias_speed = (t.astype(np.float64) for t in speeds)
    dev = [dW, eng.to_device(speeds[0]), None, dhb, eng.to_device(speeds[1]), dvb, eng.to_device(speeds[2])]
    eng.apply_update(*dev, stats, 0.1, 0.0, 0.0, 0.0, 0.5, float(B), float(B), 1.0 / B, ldv=ldv)
    g = rbm_np.rbm_grad(s, S, s_h, s_v, B, B, 0.0)
    rbm_np.apply_update(s, g[0], g[1], g[2], 0.1, 0.0, 0.0, 0.5)
    eng.synchronize()
    for n, t in zip(PARAMS, (dev[0], dev[3], dev[5], dev[1], dev[4], dev[6])):
        check("%s: %s after the update" % (tag, n), np.abs(t.cpu().numpy() - getattr(s, n)).max(), 1e-6, "update")


@pytest.mark.parametrize("name,V,H,B,k,gauss,noise,opts", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_with_nothing_missing_the_step_is_the_step_of_before(built_lib, name, V, H, B, k, gauss, noise, opts):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mdbn_amd
    from mdbn_amd.engine import RngAddr
    eng = sf.set_options(mdbn_amd.HipEngine(), opts)
    rs = np.random.RandomState(V + H)
    dW = eng.to_device((0.3 * rs.normal(size=(V, H))).astype(np.float32))
    dhb, dvb = eng.to_device((0.3 * rs.normal(size=H)).astype(np.float32)), eng.to_device((0.3 * rs.normal(size=V)).astype(np.float32))
    x, idx = step_table(V, B, gauss, seed=B, holes=False)
    data = eng.to_device(x)
    ldv, ldh = data.stride(0), dW.stride(0)
    rng = RngAddr(1234, 5, 7, 0, 2)
    stats, sc = eng.cd_step_absent(data, idx, dW, dhb, dvb, gauss, k, rng, add_noise=noise, stats=eng.new_stats_buffer(V, H, ldv, ldh))
    eng.synchronize()
    mine = [bits(t) for t in (sc.V2, sc.P2, sc.hs, sc.vs, stats)]
    if not gauss:
        none = types.SimpleNamespace(tensor=None, host=np.zeros(1, dtype=np.int32), n_groups=0)
        ref, sc2 = eng.cd_step_grouped(data, idx, dW, dhb, dvb, k, rng, none, stats=eng.new_stats_buffer(V, H, ldv, ldh))
        eng.synchronize()
        theirs = [bits(t) for t in (sc2.V2, sc2.P2, sc2.hs, sc2.vs, ref)]
        n = V * ldh + ldh + ldv
        for what, a, b in zip(("V2", "P2", "hs", "vs"), mine, theirs):
            assert np.array_equal(a, b), what
        assert np.array_equal(mine[4][:n], theirs[4][:n]), "S / s_h / s_v"
        c0, c1 = float(stats[n]), float(ref[n])
        check("absent step %s: cost against the grouped step's, rel" % name, abs(c0 - c1) / abs(c1), 1e-6)
    else:
        ref, _ = eng.cd_step(data, idx, dW, dhb, dvb, True, k, rng, add_noise=noise, stats=eng.new_stats_buffer(V, H, ldv, ldh),
                             keep_f32=True)
        eng.synchronize()
        a, b = unpack(stats.cpu().numpy(), V, H, ldv, ldh), unpack(ref.cpu().numpy(), V, H, ldv, ldh)
        for what, p, q in zip(("S", "s_h", "s_v"), a, b):
            check("absent step %s: %s against mdbn_cd_step / max" % (name, what), np.abs(p - q).max() / np.abs(q).max(), 1e-5, "stats")


# ------------------------------------------------------------------------------------------------------------------ (c) refusals
def test_every_refused_step_leaves_its_outputs_untouched(hip_engine):
    import torch
    from mdbn_amd import _lib
    from mdbn_amd.engine import RngAddr
    eng = hip_engine
    V, H, B = 21, 37, 5
    rs = np.random.RandomState(1)
    dW, dhb, dvb = eng.to_device(rs.normal(size=(V, H))), eng.to_device(rs.normal(size=H)), eng.to_device(rs.normal(size=V))
    data = eng.to_device(step_table(V, B, False, 3)[0])
    call = eng._cd_args(data, None, dW, dhb, dvb, False, 1, RngAddr(1, 2, 3), None, False, 0, keep_f32=True)
    a, sc = call.args, call.scratch
    a.B = B
    n = C.c_int64()
    assert eng.lib.mdbn_cd_step_absent_workspace_bytes(eng.ctx, B, V, H, a.ldv, a.ldh, C.byref(n)) == 0
    ws = torch.full((n.value // 4,), 9.0, dtype=torch.float32, device=eng.device)
    chain = eng.alloc_matrix(B, H, a.ldh)
    outs = [sc.V2, sc.P2, sc.hs, sc.vs, call.stats, ws, chain]
    for t in outs:
        t.fill_(4.0)
    before = [bits(t) for t in outs]
    good = dict(workspace=ws.data_ptr(), workspace_bytes=n.value)
    bad = [dict(persistent=chain.data_ptr()), dict(sample_stats=1), dict(B=0), dict(V=0), dict(H=0), dict(k=0), dict(ldv=V - 1),
           dict(ldh=a.ldh + 2), dict(W=None), dict(V2=None), dict(P2=None), dict(hs=None), dict(vs=None), dict(hbias=None), dict(stats=None),
           dict(workspace=None), dict(workspace=ws.data_ptr() + 4), dict(struct_size=8)]
    for kw in bad + [dict(workspace_bytes=n.value - 4)]:
        saved = {k: getattr(a, k) for k in list(good) + list(kw)}
        for k, v in dict(good, **kw).items():
            setattr(a, k, v)
        rc = eng.lib.mdbn_cd_step_absent(eng.ctx, eng._stream(), C.byref(a))
        assert rc == (-3 if "workspace_bytes" in kw else -1) and _lib.last_error(), kw
        for k, v in saved.items():
            setattr(a, k, v)
    eng.synchronize()
    assert all(np.array_equal(x, bits(t)) for x, t in zip(before, outs)), "a refused call wrote something"
    for k, v in good.items():
        setattr(a, k, v)
    assert eng.lib.mdbn_cd_step_absent(eng.ctx, eng._stream(), C.byref(a)) == 0, _lib.last_error()
    eng.synchronize()
    assert not np.array_equal(bits(call.stats), before[4])


# ------------------------------------------------------------------------------------------------------------------ (d) free energy
@pytest.mark.parametrize("gauss", [False, True], ids=["bernoulli", "gauss"])
@pytest.mark.parametrize("V", [33, 794, 4133])
def test_free_energy_against_the_twin(built_lib, V, gauss):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mdbn_amd
    eng = mdbn_amd.HipEngine()
    guards_ok = guard_scratch(eng)
    H, N = 50, 21
    rs = np.random.RandomState(V)
    W, hb, vb = (0.2 * rs.normal(size=(V, H))).astype(np.float32), (0.3 * rs.normal(size=H)).astype(np.float32), rs.normal(size=V).astype(np.float32)
    x, _, _ = an.case_inputs(V, N, gauss)
    got = eng.free_energy_absent(eng.to_device(x), eng.to_device(W), eng.to_device(hb), eng.to_device(vb), gauss).cpu().numpy()
    assert guards_ok(), "the guard behind the exact-size workspace was written"
    want = an.free_energy_absent(rbm_np.RBMState(V, H, W=W, hbias=hb, vbias=vb, gauss=gauss), x.astype(np.float64))
    err = (np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()
    print("free_energy_absent V=%d %s: %.3e" % (V, "gauss" if gauss else "bernoulli", err))
    check("free_energy_absent V=%d gauss=%d: rel" % (V, gauss), err, 1e-4, "free_energy")


# ------------------------------------------------------------------------------------------------------------------ (e) public path
@pytest.mark.parametrize("gauss", [False, True], ids=["bernoulli", "gauss"])
def test_training_steps_are_the_hand_composed_sequence_and_resume(hip_engine, tmp_path, gauss):
    import mdbn_amd
    from mdbn_amd import checkpoint
    from mdbn_amd.engine import RngAddr
    mdbn_amd.DBN.verbose = False
    eng = hip_engine
    V, H, B = 60, 24, 10
    x = step_table(V, 35, gauss, 9)[0]

    def net():
        return mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, gauss=gauss, hidden_layers_sizes=[], n_outs=H, engine=eng)

    def fresh(n):
        _, up = n.rbm_layers[0].get_cost_updates(0.05, k=1, batch_size=B, missing=True)
        return mdbn_amd.function(up, mdbn_amd.shared(x, engine=eng), data_parallel=None)
    a, b = net(), net()
    fn = fresh(a)
    costs = [float(fn(indexes=np.arange(B) + B * t, momentum=0.5)) for t in range(3)]
    assert np.isfinite(costs).all()
    r = b.rbm_layers[0]
    data = eng.as_matrix(mdbn_amd.shared(x, engine=eng))
    for t in range(3):
        stats, _ = eng.cd_step_absent(data, np.arange(B) + B * t, r.W.tensor, r.hbias.tensor, r.vbias.tensor, gauss, 1,
                                      RngAddr(r.theano_rng.seed, r.stream_id, t, 0, 0))
        c = eng.apply_update(r.W.tensor, r.W_speed.tensor, None, r.hbias.tensor, r.hbias_speed.tensor, r.vbias.tensor, r.vbias_speed.tensor,
                             stats, 0.05, 0.0, 0.0, 0.0, 0.5, B, B, 1.0 / (B * V) if gauss else 1.0 / B, 0, data.stride(0))
        assert float(c) == costs[t]
    for n in PARAMS:
        assert np.array_equal(getattr(a.rbm_layers[0], n).get_value(), getattr(r, n).get_value()), n
    # a resumed run continues bit for bit
    path = str(tmp_path / "absent.npz")
    checkpoint.save_network(path, {'cn': a}, resume=True)
    want = [float(fn(indexes=np.arange(B) + 5 * t, momentum=0.5)) for t in (1, 2)]
    a2 = checkpoint.load_network(path, engine=eng)['cn']
    fn2 = fresh(a2)
    assert [float(fn2(indexes=np.arange(B) + 5 * t, momentum=0.5)) for t in (1, 2)] == want
    for n in PARAMS:
        assert np.array_equal(getattr(a2.rbm_layers[0], n).get_value(), getattr(a.rbm_layers[0], n).get_value()), n


@pytest.mark.parametrize("seed", an.TOY_SEEDS)
def test_training_on_all_patients_imputes_better_than_on_the_complete_ones(hip_engine, seed):
    """The toy of tests/_absent_np.py through the public path: get_cost_updates(missing=True) on every patient against the
    same layer trained on the complete patients only, both imputing the withheld block of held-out patients by ``RBM.impute``.
    Asserted: strictly better than that, and than the block's training mean.  (The float64 twin with exact conditional means:
    tests/test_absent_twin.py.)"""
    import mdbn_amd
    eng = hip_engine
    T = an.TOY
    train, test, (lo, hi) = an.toy_problem(seed)
    complete = train[~np.isnan(train).any(axis=1)]
    V = train.shape[1]
    mask = np.ones((1, V), dtype=np.float32)
    mask[:, lo:hi] = 0.0

    def fit(rows):
        rbm = mdbn_amd.RBM(n_visible=V, n_hidden=T["H"], W=an.toy_init(seed, V), theano_rng=mdbn_amd.RandomStreams(seed), engine=eng)
        _, up = rbm.get_cost_updates(lr=T["lr"], k=T["k"], batch_size=T["B"], missing=True)
        fn = mdbn_amd.function(up, mdbn_amd.shared(rows, engine=eng), data_parallel=None)
        for idx in an.toy_batches(len(rows), seed):
            fn(indexes=idx, momentum=T["momentum"])
        return rbm.impute(test, mask, n_steps=600, burn_in=100, n_chains=4)[0][:, lo:hi].astype(np.float64)
    e_all, e_complete, e_mean = an.toy_errors(fit(train), fit(complete), train, test, lo, hi)
    print("toy on the device, seed %d: all patients %.4f, the %d complete ones %.4f, block mean %.4f" % (seed, e_all, len(complete), e_complete, e_mean))
    assert e_all < e_complete and e_all < e_mean
