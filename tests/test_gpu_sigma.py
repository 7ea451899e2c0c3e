"""The learned per-column variance of a Gaussian layer on the device: (a) the two kernels of csrc/mdbn_sigma.hip alone against
the float64 twin (tests/_sigma_np.py) fed the device's own inputs, with poisoned pad columns, determinism and every MDBN_EINVAL
case; (b) whole steps through the public classes, alone, centred and with a sparsity target, against the twin loop
teacher-forced along the device's recorded chain; (c) a frozen sigma = 1 against the plain statistics step issued by hand, the
full-batch fixed point, the log-likelihood against the exact value, and a resumed run."""
import ctypes as C

import numpy as np
import pytest

import _sigma_np as sg
import _step_forms as sf
from oracle import rbm_np
from _margins import check

pytestmark = pytest.mark.gpu

POISON = float("nan")
LO, HI = sg.LOG_SIGMA_RANGE
REL = 2.0 ** -22                # one product rounding (2^-24) plus expf's documented error (1 ulp = 2^-23)
NAMES = ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed", "log_sigma", "log_sigma_speed")


def bits(t):
    return t.detach().cpu().numpy().view(np.int32).copy()


def dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def padded(eng, a, ld, rows=None, fill=POISON):
    """-> (device view [rows, cols] of a [rows, ld] matrix whose pad columns, and rows past ``a``, hold ``fill``, the matrix)"""
    rows = a.shape[0] if rows is None else rows
    full = np.full((rows, ld), fill, dtype=np.float32)
    full[:a.shape[0], :a.shape[1]] = a
    d = dev(eng, full)
    return d[:, :a.shape[1]], d


# ------------------------------------------------------------------------------------------------------------------ (a) kernels
@pytest.mark.parametrize("B,V,ld", [(1, 7, 8), (5, 70, 72), (33, 200, 200), (20, 794, 796)])
def test_sigma_scale_rows_against_the_twin(hip_engine, B, V, ld):
    import torch
    eng = hip_engine
    rs = np.random.RandomState(B + V)
    N = B + 9
    table = (rs.normal(size=(N, V)) * 3.0).astype(np.float32)
    src, _ = padded(eng, table, ld)
    picks = rs.randint(-N, N, size=B)                           # negative values count from the end
    index_modes = [("none", src[:B], None, np.arange(B)), ("int32", src, picks.astype(np.int32), picks),
                   ("int64", src, picks.astype(np.int64), picks), ("offset6", src[6:6 + B], None, np.arange(B) + 6)]
    sigmas = [("normal", rs.normal(size=V)), ("bounds", np.where(np.arange(V) % 2, LO, HI))]
    worst = 0.0
    for sname, s in sigmas:
        s = s.astype(np.float32)
        ds = dev(eng, s)
        for iname, view, idx, rows in index_modes:
            for sign in (-1.0, 1.0):
                dst, full = padded(eng, np.zeros((B, V), np.float32), ld)       # (every entry NaN: what is not written shows)
                full.fill_(POISON)
                out = eng.sigma_scale_rows(view, None if idx is None else torch.from_numpy(idx).to(eng.device), ds, sign, out=dst)
                assert out is dst
                got = full.cpu().numpy()
                want = sg.scale_rows(table, rows, s, sign)
                assert np.isfinite(got[:, :V]).all(), "a pad column of src was read"
                worst = max(worst, float((np.abs(got[:, :V] - want) / np.abs(want)).max()))
                assert not got[:, V:].any() and not np.signbit(got[:, V:]).any(), "pad columns of dst are not zero"
                again, full2 = padded(eng, np.zeros((B, V), np.float32), ld)
                eng.sigma_scale_rows(view, None if idx is None else torch.from_numpy(idx).to(eng.device), ds, sign, out=again)
                assert np.array_equal(bits(full2), got.view(np.int32)), "two runs differ"
    print("sigma_scale_rows %dx%d: worst relative error %.3e (2^-22 = %.3e)" % (B, V, worst, REL))
    check("sigma_scale_rows: relative error", worst, REL)
    # log_sigma = 0: the plain gather, bit for bit (and the engine's default output, on src's leading dimension)
    zero = dev(eng, np.zeros(V, np.float32))
    for sign in (-1.0, 1.0):
        got = eng.sigma_scale_rows(src, picks.astype(np.int64), zero, sign)
        assert got.stride(0) == ld and np.array_equal(bits(got), bits(eng.gather_rows(src, picks.astype(np.int64))))
        assert np.array_equal(got.cpu().numpy(), table[picks])


def update_inputs(eng, B, V, n_rows, seed):
    rs = np.random.RandomState(seed)
    ld = (V + 3) & ~3
    U = rs.normal(size=(B, V)).astype(np.float32)
    M = (0.3 * rs.normal(size=(B, V))).astype(np.float32)
    U[n_rows:], M[n_rows:] = POISON, POISON                     # rows past n_rows are not read
    s = rs.uniform(-1.0, 1.0, size=V).astype(np.float32)
    speed = (0.5 * rs.normal(size=V)).astype(np.float32)
    return U, M, padded(eng, U, ld)[0], padded(eng, M, ld + 4)[0], s, speed


@pytest.mark.parametrize("momentum", [0.0, 0.5])
@pytest.mark.parametrize("B,V", [(1, 7), (33, 70), (20, 794), (64, 70), (65, 70), (512, 1024)])   # 64 | 65: one stage | two
def test_sigma_update_against_the_twin(hip_engine, B, V, momentum):
    eng = hip_engine
    lr = 0.07
    other = eng.stats_buffer(V, 8)
    other.copy_(dev(eng, np.arange(other.numel(), dtype=np.float32)))
    for n_rows in sorted({B, max(1, B - 3)}):
        U, M, dU, dM, s, speed = update_inputs(eng, B, V, n_rows, seed=B + V + n_rows)
        g, scale = sg.grad(U, M, n_rows)
        # (a) against the twin
        ds, dsp = dev(eng, s), dev(eng, speed)
        eng.sigma_update(dU, dM, n_rows, lr, momentum, LO, HI, ds, dsp)
        want_s, want_speed = sg.update(s, speed, g, lr, momentum, LO, HI)
        got_s, got_speed = ds.cpu().numpy(), dsp.cpu().numpy()
        assert np.isfinite(got_s).all() and np.isfinite(got_speed).all(), "a pad column or a dead row was read"
        tag = "sigma_update %dx%d" % (B, V)
        check(tag + ": log_sigma / max", np.abs(got_s - want_s).max() / max(1.0, np.abs(want_s).max()), 2e-6, "update")
        check(tag + ": speed / max", np.abs(got_speed - want_speed).max() / max(1.0, np.abs(want_speed).max()), 2e-6, "update")
        if momentum == 0.0:                                     # the new speed IS the gradient
            check(tag + ": g / max(1, mean|u (u - m)|)", (np.abs(got_speed - g) / np.maximum(1.0, scale)).max(), 1e-5, "stats")
        # two runs are bit-identical
        ds2, dsp2 = dev(eng, s), dev(eng, speed)
        eng.sigma_update(dU, dM, n_rows, lr, momentum, LO, HI, ds2, dsp2)
        assert np.array_equal(bits(ds2), bits(ds)) and np.array_equal(bits(dsp2), bits(dsp)), "two runs differ"
        # lr = 0 leaves log_sigma bit-unchanged and still moves the speed to the same bits
        ds3, dsp3 = dev(eng, s), dev(eng, speed)
        eng.sigma_update(dU, dM, n_rows, 0.0, momentum, LO, HI, ds3, dsp3)
        assert np.array_equal(bits(ds3), s.view(np.int32)) and np.array_equal(bits(dsp3), bits(dsp))
        # the clamp, at both ends
        s_edge = np.where(np.arange(V) % 2, HI - 0.01, LO + 0.01).astype(np.float32)
        sp_edge = np.where(np.arange(V) % 2, 1.0, -1.0).astype(np.float32)
        ds4, dsp4 = dev(eng, s_edge), dev(eng, sp_edge)
        eng.sigma_update(dU, dM, n_rows, 1.0, momentum, LO, HI, ds4, dsp4)
        assert np.array_equal(ds4.cpu().numpy(), np.where(np.arange(V) % 2, np.float32(HI), np.float32(LO)))
    assert np.array_equal(other.cpu().numpy(), np.arange(other.numel(), dtype=np.float32)), "a statistics buffer was touched"


def test_every_einval_case_returns_without_touching_its_outputs(hip_engine):
    import torch
    from mdbn_amd import _lib
    eng, lib = hip_engine, hip_engine.lib
    B, V, ld = 70, 30, 32                                        # (two stages: the workspace is needed)
    U, M, dU, dM, s, speed = update_inputs(eng, B, V, B, seed=1)
    room = torch.zeros(V + 8, dtype=torch.float32, device=eng.device)
    ds, dsp = dev(eng, s), dev(eng, speed)
    n = C.c_int64()
    assert lib.mdbn_sigma_workspace_bytes(eng.ctx, B, V, C.byref(n)) == 0 and n.value == 5 * 32 * 4
    assert lib.mdbn_sigma_workspace_bytes(eng.ctx, 64, V, C.byref(n)) == 0 and n.value == 0
    for kw in (dict(B=0), dict(V=0), dict(B=(1 << 19) + 1), dict(ctx=None), dict(out=None)):
        a = dict(dict(ctx=eng.ctx, B=B, V=V, out=C.byref(n)), **kw)
        assert lib.mdbn_sigma_workspace_bytes(a["ctx"], a["B"], a["V"], a["out"]) == -1, kw
    ws = torch.zeros(5 * 32 + 8, dtype=torch.float32, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    nan, inf = float("nan"), float("inf")

    def update_call(U=dU, ldu=dU.stride(0), M=dM, ldm=dM.stride(0), B=B, V=V, n_rows=B, lr=0.1, momentum=0.5, lo=LO, hi=HI, s=ds,
                    speed=dsp, ws=ws, ws_bytes=5 * 32 * 4, ctx=eng.ctx):
        return lib.mdbn_sigma_update(ctx, eng._stream(), p(U), ldu, p(M), ldm, B, V, n_rows, lr, momentum, lo, hi, p(s), p(speed),
                                     p(ws), ws_bytes)

    before = (bits(ds), bits(dsp))
    bad = [dict(B=0), dict(V=0), dict(B=-1), dict(n_rows=0), dict(n_rows=B + 1), dict(n_rows=-2), dict(U=None), dict(M=None),
           dict(s=None), dict(speed=None), dict(ctx=None), dict(ws=None), dict(ws_bytes=5 * 32 * 4 - 4), dict(ws=ws[1:]),
           dict(U=dU.reshape(-1)[1:]), dict(M=dM.reshape(-1)[1:]), dict(s=ds.view(torch.uint8)[1:]), dict(speed=dsp.view(torch.uint8)[2:]),
           dict(ldu=V - 2), dict(ldu=V + 1), dict(ldm=V - 2), dict(ldm=V + 1), dict(lr=-0.1), dict(lr=nan), dict(lr=inf),
           dict(momentum=-0.1), dict(momentum=1.5), dict(momentum=nan), dict(lo=1.0, hi=-1.0), dict(lo=nan), dict(hi=nan),
           dict(lo=-inf), dict(hi=inf), dict(B=(1 << 19) + 1)]
    for kw in bad:
        assert update_call(**kw) == -1, kw
        assert _lib.last_error(), kw
    eng.synchronize()
    assert np.array_equal(bits(ds), before[0]) and np.array_equal(bits(dsp), before[1]), "a refused call wrote something"

    table, _ = padded(eng, np.random.RandomState(2).normal(size=(B, V)).astype(np.float32), ld)
    dst, dst_full = padded(eng, np.zeros((B, V), np.float32), ld, fill=7.0)
    idx = torch.arange(B, dtype=torch.int64, device=eng.device)

    def scale_call(src=table, n_src=B, ld_src=ld, idx=idx, is64=1, B=B, V=V, s=ds, sign=-1.0, dst=dst, ld_dst=ld, ctx=eng.ctx):
        return lib.mdbn_sigma_scale_rows(ctx, eng._stream(), p(src), n_src, ld_src, p(idx), is64, B, V, p(s), sign, p(dst), ld_dst)

    kept = bits(dst_full)
    bad = [dict(B=0), dict(V=0), dict(n_src=0), dict(B=-1), dict(src=None), dict(dst=None), dict(s=None), dict(ctx=None),
           dict(idx=None, B=B + 1), dict(idx=idx.view(torch.uint8)[4:], B=B - 1), dict(src=table.reshape(-1)[1:]),
           dict(dst=dst_full.reshape(-1)[1:]), dict(s=ds.view(torch.uint8)[1:]), dict(ld_src=V - 2), dict(ld_src=V + 1),
           dict(ld_dst=V - 2), dict(ld_dst=V + 1), dict(sign=0.0), dict(sign=2.0), dict(sign=nan), dict(sign=-0.5)]
    for kw in bad:
        assert scale_call(**kw) == -1, kw
        assert _lib.last_error(), kw
    eng.synchronize()
    assert np.array_equal(bits(dst_full), kept), "a refused call wrote something"
    # ... and the good calls go through
    assert scale_call() == 0 and scale_call(idx=None) == 0 and update_call() == 0 and update_call(n_rows=B - 1) == 0
    assert update_call(B=64, n_rows=64, ws=None, ws_bytes=0) == 0           # one stage: no workspace
    eng.synchronize()
    assert not np.array_equal(bits(ds), before[0]) and not np.array_equal(bits(dst_full), kept)


# ------------------------------------------------------------------------------------------------------------------ (b) whole steps
shadow_engine = sf.sigma_engine         # (the riding engine and the whole-step loop live in tests/_step_forms.py)

CASES = [  # id, V, H, B, k, error_free, variant
    ("ragged_60x24", 60, 24, 33, 1, True, "alone"),
    ("thin_794x64_cd2_noisy", 794, 64, 20, 2, False, "alone"),
    ("tall_1024x256", 1024, 256, 512, 1, True, "alone"),
    ("tall_1024x256_centred", 1024, 256, 512, 1, True, "centered"),
    ("tall_1024x256_sparse", 1024, 256, 512, 1, True, "sparse"),
]
STEPS, ETA, LR, L2 = sf.STEPS, sf.ETA, sf.SIGMA_LR, sf.SIGMA_L2
SPARSITY = sf.SPARSITY
assert (STEPS, ETA, LR, L2) == (4, 0.05, 0.002, 0.1) and SPARSITY == dict(sparsity_target=0.2, sparsity_cost=1.0, sparsity_decay=0.9)


@pytest.mark.parametrize("name,V,H,B,k,error_free,variant", CASES, ids=[c[0] for c in CASES])
def test_sigma_steps_teacher_forced_along_the_device_chain(built_lib, name, V, H, B, k, error_free, variant):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    eng = shadow_engine()                           # product defaults; keep_f32 stays off but for the call that asks
    assert not eng.keep_f32
    r = sf.run_sigma(eng, V, H, B, k, error_free, variant)
    assert not eng.keep_f32 and [n for n, _ in r.errs] == list(NAMES)
    sf.check_sigma(name, r, REL)                    # (every figure printed, then the bounds as they were)
    assert ("offsets" in r.state) == (variant == "centered") and ("q" in r.state) == (variant == "sparse")


# ------------------------------------------------------------------------------------------------------------------ (c)
def test_a_frozen_sigma_of_one_is_the_plain_statistics_step_bit_for_bit(hip_engine):
    import mdbn_amd
    from mdbn_amd.engine import RngAddr
    eng = hip_engine
    V, H, B, N, k = 200, 48, 33, 80, 1
    rs = np.random.RandomState(5)
    data = rs.normal(size=(N, V)).astype(np.float32)
    shared = mdbn_amd.shared(data, engine=eng)
    layers = [mdbn_amd.GRBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(123), theano_rng=mdbn_amd.RandomStreams(7), engine=eng)
              for _ in range(2)]
    a, b = layers
    assert a.stream_id == b.stream_id
    a.set_sigma(1.0)
    _, up = a.get_cost_updates(lr=0.005, k=k, batch_size=B, lambda_2=0.1)
    assert up.sigma and up.learn_sigma is None
    fn = mdbn_amd.function(up, shared, data_parallel=None)
    stats = eng.new_stats_buffer(V, H, shared.tensor.stride(0), b.W.tensor.stride(0))
    for t in range(3):
        idx = eng.index_tensor(rs.permutation(N)[:B], N)
        got = float(fn(indexes=idx, momentum=0.5))
        eng.cd_step(shared.tensor, idx, b.W.tensor, b.hbias.tensor, b.vbias.tensor, True, k, RngAddr(7, b.stream_id, t, 0, 0), stats=stats,
                    keep_f32=True)
        want = float(eng.apply_update(b.W.tensor, b.W_speed.tensor, None, b.hbias.tensor, b.hbias_speed.tensor, b.vbias.tensor,
                                      b.vbias_speed.tensor, stats, 0.005, 0.0, 0.1, 0.0, 0.5, B, B, 1.0 / (B * V), 0, shared.tensor.stride(0)))
        assert got == want, t
        for n in NAMES[:6]:
            assert np.array_equal(getattr(a, n).get_value(), getattr(b, n).get_value()), (t, n)
    assert not a.log_sigma.get_value().any() and not a.log_sigma_speed.get_value().any()


def test_the_full_batch_fixed_point_on_the_device(hip_engine):
    import mdbn_amd
    eng = hip_engine
    x, want = sg.fixed_point_problem()
    rbm = mdbn_amd.GRBM(n_visible=64, n_hidden=8, W=np.zeros((64, 8), dtype=np.float32), numpy_rng=np.random.RandomState(5),
                        theano_rng=mdbn_amd.RandomStreams(11), engine=eng)
    _, up = rbm.get_cost_updates(lr=0.0, k=1, batch_size=32, learn_sigma=0.1)
    fn = mdbn_amd.function(up, mdbn_amd.shared(x.astype(np.float32), engine=eng), data_parallel=None)
    for _ in range(100):
        fn(momentum=0.0)
    assert not rbm.W.get_value().any() and not rbm.vbias.get_value().any()
    check("sigma fixed point: |log_sigma - log(mean x^2) / 2| after 100 steps", np.abs(rbm.log_sigma.get_value() - want).max(), 2e-6)


def test_log_likelihood_against_the_exact_value(hip_engine):
    import mdbn_amd
    eng = hip_engine
    st = sg.state(8, 4, seed=6, scale=0.4)
    rs = np.random.RandomState(7)
    sigma = np.exp(rs.uniform(-1.0, 1.0, size=8)).astype(np.float32)
    x = (rs.normal(size=(50, 8)) * sigma[None, :]).astype(np.float32)
    rbm = mdbn_amd.GRBM(n_visible=8, n_hidden=4, numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(1), engine=eng)
    rbm.W.set_value(st.W.astype(np.float32)); rbm.hbias.set_value(st.hbias.astype(np.float32)); rbm.vbias.set_value(st.vbias.astype(np.float32))
    rbm.set_sigma(sigma)
    st32 = rbm_np.RBMState(8, 4, W=rbm.W.get_value(), hbias=rbm.hbias.get_value(), vbias=rbm.vbias.get_value(), gauss=True)
    exact = sg.log_likelihood(st32, x.astype(np.float64), rbm.log_sigma.get_value().astype(np.float64))
    ll, err = rbm.log_likelihood(x, n_chains=512, n_betas=1000)
    plain = sg.log_likelihood(st32, x.astype(np.float64), np.zeros(8))
    print("sigma log-likelihood 8->4: %.5f exact %.5f |err| %.5f std_err %.5f (scored at unit variance: %.5f)" % (ll, exact, abs(ll - exact), err, plain))
    assert abs(ll - exact) <= 4 * err, (ll, exact, err)
    assert abs(ll - exact) <= 0.05, (ll, exact)
    assert abs(plain - exact) > 0.5                 # (the sum(s) term and the scaling are not a detail)


def test_a_resumed_run_with_a_learned_sigma_continues_bit_for_bit(hip_engine, tmp_path):
    import mdbn_amd
    from mdbn_amd import checkpoint
    mdbn_amd.DBN.verbose = False
    eng = hip_engine
    rs = np.random.RandomState(0)
    V, H = 96, 40
    x = (rs.normal(size=(40, V)) * np.exp(rs.uniform(-1, 1, size=V))[None, :]).astype(np.float32)
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[], n_outs=H, engine=eng)
    rbm = net.rbm_layers[0]
    plan = dict(k=1, lambda_2=0.1, batch_size=10, centered=True, learn_sigma=0.05)
    _, up = rbm.get_cost_updates(0.005, **plan)
    fn = mdbn_amd.function(up, mdbn_amd.shared(x, engine=eng), data_parallel=None)
    for t in range(2):
        fn(indexes=np.arange(10) + 10 * t, momentum=0.5)
    path = str(tmp_path / "sigma.npz")
    checkpoint.save_network(path, {'ge': net}, resume=True)
    want = [float(fn(indexes=np.arange(10) + 10 * t, momentum=0.5)) for t in (2, 3)]
    net2 = checkpoint.load_network(path, engine=eng)['ge']
    r2 = net2.rbm_layers[0]
    assert r2.log_sigma is not None and r2.log_sigma_speed.get_value().any() and net2.sigmoid_layers[0].log_sigma is r2.log_sigma
    _, up2 = r2.get_cost_updates(0.005, **plan)
    fn2 = mdbn_amd.function(up2, mdbn_amd.shared(x, engine=eng), data_parallel=None)
    got = [float(fn2(indexes=np.arange(10) + 10 * t, momentum=0.5)) for t in (2, 3)]
    assert got == want
    for n in NAMES + ("v_offset", "h_offset"):
        assert np.array_equal(getattr(r2, n).get_value(), getattr(rbm, n).get_value()), n
    assert np.array_equal(net2.get_output(x), net.get_output(x))
