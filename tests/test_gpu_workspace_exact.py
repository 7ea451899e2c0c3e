"""Every entry point on a workspace of EXACTLY its sizer's bytes, between guards (tests/_guarded.py).

The product engine hides any disagreement between a sizer and the kernels behind it: HipEngine.workspace never takes less
than 8 MiB and every allocation carries a pad.  A C caller allocates the sizer's figure.  Here every library call runs as
that caller would run it, between guards that are compared bit for bit after the call.  What each group asserts besides:

  C1  the CD step on every dispatch path (the path itself from the GEMM launch kinds), the step variants, the grouped step:
      the float64 oracle along the device's taps AND bit for bit the same call on the plain engine; the split step: bit
      for bit the plain engine's; the train step: the oracle and the plain engine's parameters; mdbn_cd_stats: float64 and
      the plain engine's bits.  Four bytes fewer declared: MDBN_ENOSPC with every output untouched, on four of the paths.
  C2  the CD step on leading dimensions wider than the policy's: on mdbn_workspace_bytes' figure (which does not cover
      them: the column-sum regions lie on the caller's strides) refused untouched, or right; on mdbn_workspace_bytes_ld's
      the oracle;
  C3  the propagate-only calls at the core sizer's bytes and at MDBN_MIN_WORKSPACE_BYTES: the oracle, and the run at the
      minimum against the run at the core sizer's bytes within twice the oracle tolerance (samples equal off ties); the
      rows are shown to be cut (more GEMM launches than passes) where slabs are needed -- with the activation as a launch of
      its own, and for the free energy --; under default options propup / propdown / the chain fuse the activation, need
      no slabs, and their run at the minimum is an uncut run.  Four bytes fewer: MDBN_ENOSPC, outputs untouched;
  C4  the feature sizers (centred step, sigma, up-down, grouped softmax, row log-likelihood, the samplers): bit for bit the
      plain engine's result; four bytes fewer: the family's error with every tensor the call could have written -- its
      outputs, the engine's copies of its operands, the test's in-place operands -- bit-unchanged (GuardedEngine.watching).

Every tolerance is the one the project applies to that call elsewhere (tests/_margins.py), or twice it
where two device runs are compared that are each within it of the oracle."""
import ctypes as C

import numpy as np
import pytest

from oracle import philox_np, rbm_np
from _margins import check
from _variants import NO_FAST_PATH, VARIANTS, cd, forward, options, oracle, run_variant, same

pytestmark = pytest.mark.gpu

ENOSPC = -3


@pytest.fixture(scope="module")
def guarded(built_lib):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from _guarded import GuardedEngine
    eng = GuardedEngine()
    eng.set_planes_min_work(0)          # as the shared fixture: every whole-tile shape on planes
    return eng


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _pair(hip_engine, guarded, fn):
    """fn(engine) on the shared engine, then on a fresh arena of the guarded one; the guards are checked after the call."""
    try:
        plain = fn(hip_engine)
        guarded.reset()
        got = fn(guarded)
        handed = guarded.check_guards()
    finally:
        for eng in (hip_engine, guarded):
            eng.set_planes_min_work(0)  # (_variants.options puts the library default back, the fixtures run on 0)
    return plain, got, handed


def _exact(guarded, handed, B, V, H, ldv=None, ldh=None):
    """The step's workspace was the sizer's figure to the byte."""
    n = C.c_int64()
    if ldv is None:
        assert guarded.lib.mdbn_workspace_bytes_ctx(guarded.ctx, B, V, H, C.byref(n)) == 0
    else:
        assert guarded.lib.mdbn_workspace_bytes_ld_ctx(guarded.ctx, B, V, H, ldv, ldh, C.byref(n)) == 0
    sizes = [b for what, b in handed if what == "workspace"]
    assert sizes and all(b == n.value for b in sizes), (sizes, n.value)
    print("workspace %d x %d -> %d: %d bytes, guards intact" % (B, V, H, n.value))
    return n.value


# ---------------------------------------------------------------------------------- C1: the CD step on every path
def _no_gemm(kinds):
    return kinds == []


def _forward_gemms(kinds):
    return bool(forward(kinds))


def _planes(kinds):
    return bool(kinds) and all(kd >= 2000 for kd in kinds)


def _gchain(kinds):
    return bool(kinds) and all(kd % 10 == 3 for kd in kinds)


GCHAIN = dict(small_fused=0, gchain=1, planes_min_work=1 << 30)
STEP_CASES = [  # id, V, H, B, k, gauss, options, the path by its GEMM launch kinds
    ("one_launch", 100, 24, 64, 1, False, {}, _no_gemm),
    ("thin", 784, 500, 20, 1, False, {}, _no_gemm),
    # 256 -> 128 at B = 128 is made of whole tiles, but its forward plans are not the plane path's (plane_plan: the bf16x6
    # plan of whole 32-deep slices): with planes_min_work = 0 the streaming kernels serve it.  1024 -> 512 at B = 256 is
    # the smallest shape the other modules run on planes.
    ("whole_tiles_256x128", 256, 128, 128, 1, True, dict(planes_min_work=0), _forward_gemms),
    ("planes", 1024, 512, 256, 1, True, dict(planes_min_work=0), _planes),
    ("gchain", 300, 130, 40, 3, False, GCHAIN, _gchain),
] + [("dense-%s-k%d-%s" % (name, k, "grbm" if gauss else "rbm"), 300, 40, 200, k, gauss, opts, served)
     for name, opts, served in (("nofast", NO_FAST_PATH, _forward_gemms), ("defaults", {}, _no_gemm))      # defaults: the one-launch step
     for k in (1, 3) for gauss in (False, True)]


@pytest.mark.parametrize("name,V,H,B,k,gauss,opts,served", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_cd_step_on_the_sizers_bytes(hip_engine, guarded, name, V, H, B, k, gauss, opts, served):
    plain, got, handed = _pair(hip_engine, guarded, lambda eng: cd(eng, V, H, B, k, gauss, opts))
    assert served(got["kinds"]), (name, got["kinds"])
    assert got["kinds"] == plain["kinds"], (name, got["kinds"], plain["kinds"])
    _exact(guarded, handed, B, V, H)
    oracle("exact workspace, " + name, got)
    same(got, plain, "exact workspace against the engine's, " + name)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_step_variants_on_the_sizers_bytes(hip_engine, guarded, variant):
    V, H, B = 300, 40, 200
    plain, got, handed = _pair(hip_engine, guarded, lambda eng: run_variant(eng, variant, V, H, B, {}))
    assert _forward_gemms(got["kinds"]) and got["kinds"] == plain["kinds"], (variant, got["kinds"], plain["kinds"])
    _exact(guarded, handed, B, V, H)
    oracle("exact workspace, " + variant, got)
    same(got, plain, "exact workspace against the engine's, " + variant)


def _fresh_pair(knobs):
    """A plain and a guarded engine of their own under the same knobs (test_gpu_deferred's helpers take an engine)."""
    import mdbn_amd
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from _guarded import GuardedEngine
    engines = mdbn_amd.HipEngine(), GuardedEngine()
    for eng in engines:
        for name, value in knobs.items():
            eng.set_option(name, value)
    return engines


SPLIT_CASES = [("dense", (300, 40, 200), NO_FAST_PATH, _forward_gemms), ("whole_tiles_256x128", (256, 128, 128), {"planes_min_work": 0}, _forward_gemms),
               ("planes", (1024, 512, 256), {"planes_min_work": 0}, _planes)]


@pytest.mark.parametrize("gauss", [True, False], ids=["grbm", "rbm_w0"])
@pytest.mark.parametrize("name,shape,knobs,served", SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_split_step_with_a_deferred_update_on_the_sizers_bytes(built_lib, name, shape, knobs, served, gauss):
    """mdbn_cd_forward + mdbn_cd_statistics(deferred = the previous step's phase-3 update): every output bit for bit the
    plain engine's (tests/test_gpu_deferred.py anchors that one to the rule in float64), guards intact."""
    import test_gpu_deferred as D
    plain, guarded = _fresh_pair(knobs)
    prob = D._Problem(shape, gauss)
    a, _, ka, _ = D._one_step(plain, prob, "B")
    guarded.reset()
    b, _, kb, _ = D._one_step(guarded, prob, "B")
    handed = guarded.check_guards()
    assert served(kb) and ka == kb, (name, ka, kb)
    V, H, B = shape
    _exact(guarded, handed, B, V, H)
    D._same(a, b, ("exact workspace", name, gauss))


def _shadowed():
    """cd_train_step through a ShadowEngine, plain and guarded: the float64 oracle rides along (tests/_shadow.py)."""
    from _guarded import GuardedEngine
    from _shadow import ShadowEngine

    class GuardedShadow(GuardedEngine, ShadowEngine):
        pass
    return ShadowEngine, GuardedShadow


@pytest.mark.parametrize("fused_update", [0, 1])
@pytest.mark.parametrize("name,shape", [("one_launch", (100, 24, 64)), ("dense", (300, 40, 200))])
def test_train_step_on_the_sizers_bytes(built_lib, name, shape, fused_update):
    """mdbn_cd_train_step, the update inside the statistics kernel and as a launch of its own: the oracle along the device's
    taps (cost 1e-5, parameters 2e-6 of their maximum: tests/test_gpu_product_defaults.py's bounds for this call), bit for bit
    the plain engine's parameters, guards intact."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_gpu_deferred as D
    Plain, Guarded = _shadowed()
    V, H, B = shape
    out = []
    for cls in (Plain, Guarded):
        eng = cls()
        eng.set_option("fused_update", fused_update)
        for gauss in (True, False):
            p = D._Problem(shape, gauss, seed=3)
            st = p.device(eng)
            if isinstance(eng, Guarded):
                eng.reset()
            cost = eng.cd_train_step(st.x, st.idx[0], st.W, st.W_speed, st.W0, st.hb, st.hbs, st.vb, st.vbs, gauss, 1, D._rng(0),
                                     p.lr, 0.0, p.l2, p.wc, D.MOMENTUM, p.batch_size, p.batch_size,
                                     1.0 / (B * V) if gauss else 1.0 / B)       # (the oracle's step: n_rows = the batch)
            snap = st.snapshot()
            snap["cost"] = np.array([float(cost)], np.float32)
            if isinstance(eng, Guarded):
                _exact(eng, eng.check_guards(), B, V, H)
            ref = eng.shadow[st.W.data_ptr()]
            tag = "exact workspace, train step %s fused_update=%d" % (name, fused_update)
            for mine, theirs in (("W", "W"), ("W_speed", "W_speed"), ("hb", "hbias"), ("hbs", "hbias_speed"), ("vb", "vbias"),
                                 ("vbs", "vbias_speed")):
                want = getattr(ref, theirs)
                g = snap[mine][:, :H] if want.ndim == 2 else snap[mine][:want.size]
                check(tag + ": %s / max" % theirs, np.abs(g - want).max() / max(1.0, np.abs(want).max()), 2e-6, "update")
            st.check_invariants(tag)
            out.append(snap)
        check("exact workspace, train step: cost rel", eng.cost_err, 1e-5)
        assert eng.steps == 2
    for a, b in zip(out[:2], out[2:]):
        D._same(a, b, ("exact workspace, train step", name, fused_update))


# ---------------------------------------------------------------------------------- C2: wide leading dimensions
def _cd_wide(eng, V, H, B, k, gauss, opts, ldv, ldh, policy_sizer, seed=5, fewer=0):
    """`_variants.cd` (the same inputs from the same seed, the same record) with the data, V2 and vs on `ldv` and W, P2 and hs
    on `ldh`.  policy_sizer: the workspace of mdbn_workspace_bytes (what a caller who read only that sizer allocates) instead
    of mdbn_workspace_bytes_ld's; fewer: bytes of it the library is not told about.  A refused call comes back as
    {"rc": ...} with the pre-filled outputs.

    Pad columns: zeros everywhere, because on a CD step no pad is 'neither read nor written'.  W's are read (the GEMMs run over
    the stored width and rely on exact zeros there: mdbn_hip.h, plane path note; csrc GemmArgs.Nst); the data's travel into
    V2 with the gather (the step gathers whole rows of ldv floats, dense_forward); V2's, P2's, hs' and vs' are written as
    exact zeros by every activation epilogue (Nst columns stored) and read by the statistics GEMM and the column sums.  A
    NaN in any of them is a NaN in S or s_h / s_v by the documented contract, not a finding."""
    import torch
    from mdbn_amd import RngAddr, _lib
    from _variants import RNG
    rs = np.random.RandomState(seed)
    W = rbm_np.init_W(rs, V, H, np.float32)
    hb, vb = rs.normal(0, 0.2, H).astype(np.float32), rs.normal(0, 0.2, V).astype(np.float32)
    N = B + 13
    data = rs.normal(size=(N, V)).astype(np.float32) if gauss else (rs.uniform(size=(N, V)) < 0.3).astype(np.float32)
    idx = rs.permutation(N)[:B].astype(np.int64)
    dW, dx = eng.alloc_matrix(V, H, ldh), eng.alloc_matrix(N, V, ldv)
    dW.copy_(torch.from_numpy(W))
    dx.copy_(torch.from_numpy(data))
    dhb, dvb = eng.to_device(hb), eng.to_device(vb)
    keep = (eng.keep_f32, eng.trace_chain)
    eng.keep_f32, eng.trace_chain = True, True
    eng.kernel_timing(True)
    try:
        with options(eng, **opts):
            eng.reset()
            sc = eng.cd_scratch(B, V, H, not gauss, ldv, ldh)
            stats = eng.new_stats_buffer(V, H, ldv, ldh)
            # every live entry of the outputs holds a pattern (the pad columns keep the zeros a step expects there)
            live = [sc.V2, sc.P2, stats[:V * ldh].view(V, ldh)[:, :H], stats[V * ldh:V * ldh + H],
                    stats[V * ldh + ldh:V * ldh + ldh + V], stats[V * ldh + ldh + ldv:]]
            for t in live:
                t.fill_(FILL)
            ws = eng.workspace(B, V, H) if policy_sizer else eng.workspace(B, V, H, ldv, ldh)
            call = eng._cd_args(dx, idx, dW, dhb, dvb, gauss, k, RngAddr(RNG[0], RNG[1], RNG[2], 0, 0), None, False, 0, stats=stats)
            assert call.scratch is sc
            call.args.workspace, call.args.workspace_bytes = ws.data_ptr(), ws.numel() * 4 - fewer
            rc = eng.lib.mdbn_cd_step(eng.ctx, eng._stream(), C.byref(call.args))
            handed = eng.check_guards()
            kinds = [kd for _, _, _, kd in eng.kernel_timing_detail()]
            if rc != 0:
                untouched = all(bool((t == FILL).all()) for t in live)
                return dict(rc=rc, untouched=untouched, kinds=kinds, error=_lib.last_error(), bytes=ws.numel() * 4, handed=handed)
    finally:
        eng.kernel_timing(False)
        eng.keep_f32, eng.trace_chain = keep
        eng.set_planes_min_work(0)
    return dict(rc=0, V=V, H=H, B=B, k=k, gauss=gauss, opts=opts, sample_stats=False, add_noise=False, W=W, hb=hb, vb=vb,
                x=data[idx], chain0=None, stats=stats.cpu().numpy(), ldh=ldh, ldv=ldv, P2=sc.P2.cpu().numpy(), V2=sc.V2.cpu().numpy(),
                th=sc.trace_h.cpu().numpy()[:k, :, :H], tv=None if gauss else sc.trace_v.cpu().numpy()[:, :, :V], chain1=None,
                kinds=kinds, bytes=ws.numel() * 4, handed=handed)


WIDE_CASES = [("one_launch", 100, 24, 64, 1, False, {}), ("dense-k1-rbm", 300, 40, 200, 1, False, NO_FAST_PATH),
              ("dense-k3-grbm", 300, 40, 200, 3, True, NO_FAST_PATH), ("dense-defaults-k1-grbm", 300, 40, 200, 1, True, {})]


@pytest.mark.parametrize("name,V,H,B,k,gauss,opts", WIDE_CASES, ids=[c[0] for c in WIDE_CASES])
def test_cd_step_on_wide_leading_dimensions(guarded, name, V, H, B, k, gauss, opts):
    """ldv = padded_ld(V) + 64, ldh = round_up(H, 128) + 128: the column sums of ceil(B / 4) row groups on these strides do not
    fit the regions mdbn_workspace_bytes sizes -- colPneg would start inside colPpos (a wrong s_h under a right-looking S)
    and the last row groups of colV would land behind the workspace.  On that sizer's bytes the call is either refused
    before any launch with its outputs untouched, or right; on mdbn_workspace_bytes_ld's it is right.  Guards intact both
    ways."""
    ldv, ldh = (V + 3) // 4 * 4 + 64, (H + 127) // 128 * 128 + 128
    r = _cd_wide(guarded, V, H, B, k, gauss, opts, ldv, ldh, policy_sizer=True)
    if r["rc"] != 0:
        assert r["untouched"] and r["kinds"] == [], (name, r)
        assert r["rc"] == ENOSPC and "mdbn_workspace_bytes_ld" in r["error"], (name, r["rc"], r["error"])
        print("%s on ldv %d ldh %d: %d bytes of mdbn_workspace_bytes refused before any launch" % (name, ldv, ldh, r["bytes"]))
    else:
        oracle("wide ld on mdbn_workspace_bytes, " + name, r)
    r = _cd_wide(guarded, V, H, B, k, gauss, opts, ldv, ldh, policy_sizer=False)
    assert r["rc"] == 0, (name, r)
    _exact(guarded, r["handed"], B, V, H, ldv, ldh)
    oracle("wide ld on mdbn_workspace_bytes_ld, " + name, r)


SHORT_CASES = [c for c in STEP_CASES if c[0] in ("one_launch", "thin", "planes", "dense-nofast-k1-rbm")]


@pytest.mark.parametrize("name,V,H,B,k,gauss,opts,served", SHORT_CASES, ids=[c[0] for c in SHORT_CASES])
def test_cd_step_refuses_four_bytes_fewer(guarded, name, V, H, B, k, gauss, opts, served):
    """The sizer's figure less four bytes, the buffer itself whole: MDBN_ENOSPC before any launch, V2 / P2 / the statistics
    still hold their pattern, guards intact."""
    r = _cd_wide(guarded, V, H, B, k, gauss, opts, (V + 3) // 4 * 4, (H + 3) // 4 * 4, policy_sizer=True, fewer=4)
    assert r["rc"] == ENOSPC and r["untouched"] and r["kinds"] == [], (name, r)


def _grouped_step(eng):
    """mdbn_cd_step_grouped (70 -> 24 in groups of 2, 64 and single columns, 33 rows, CD-2) with the chain tapped."""
    from mdbn_amd import RngAddr
    from mdbn_amd.engine import GroupTable
    V, H, B, bounds = 70, 24, 33, [1, 3, 67, 70]
    rs = np.random.RandomState(8)
    W = eng.to_device(rbm_np.init_W(rs, V, H, np.float32))
    hb, vb = eng.to_device(rs.normal(0, 0.2, H).astype(np.float32)), eng.to_device(rs.normal(0, 0.2, V).astype(np.float32))
    x = (rs.uniform(size=(B + 5, V)) < 0.3).astype(np.float32)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        x[:, lo:hi] = 0.0
        x[np.arange(B + 5), lo + rs.randint(0, hi - lo, B + 5)] = 1.0
    idx = rs.permutation(B + 5)[:B].astype(np.int64)
    eng._scratch.clear()
    stats, sc = eng.cd_step_grouped(eng.to_device(x), idx, W, hb, vb, 2, RngAddr(5, 3, 11, 0, 0), GroupTable(eng, np.asarray(bounds, np.int32)))
    eng.synchronize()
    return dict(stats=stats, V2=sc.V2, P2=sc.P2), (B, V, H)


def test_grouped_step_on_the_sizers_bytes(hip_engine, guarded):
    """mdbn_cd_step_grouped sizes with mdbn_workspace_bytes and runs its passes on the propagate-only carve-up of it: bit for
    bit the plain engine's step (tests/test_gpu_softmax.py checks that one against the twin), guards intact."""
    plain, _ = _grouped_step(hip_engine)
    guarded.reset()
    got, (B, V, H) = _grouped_step(guarded)
    _exact(guarded, guarded.check_guards(), B, V, H)
    _bit_equal(got, plain, "grouped step")


@pytest.mark.parametrize("V,H,B", [(300, 40, 200), (1024, 512, 256), (100, 24, 64)])
def test_cd_stats_on_the_sizers_bytes(hip_engine, guarded, V, H, B):
    """mdbn_cd_stats alone: S = V2^T P2, s_h and s_v against float64 (1e-5 of the maximum, the step's bound for them), bit for
    bit the plain engine's, guards intact; four bytes fewer: MDBN_ENOSPC, the statistics untouched."""
    import torch
    rs = np.random.RandomState(V + B)
    V2, P2 = rs.normal(size=(2 * B, V)).astype(np.float32), rs.uniform(-1, 1, size=(2 * B, H)).astype(np.float32)
    out = []
    for eng in (hip_engine, guarded):
        dV, dP = eng.to_device(V2), eng.to_device(P2)
        ldv, ldh = dV.stride(0), dP.stride(0)
        for fewer in ((0, 4) if eng is guarded else (0,)):
            stats = torch.full((V * ldh + ldh + ldv + 4,), FILL, dtype=torch.float32, device=eng.device)
            if eng is guarded:
                eng.reset()
            ws = eng.workspace(B, V, H)
            rc = eng.lib.mdbn_cd_stats(eng.ctx, eng._stream(), _p(dV), _p(dP), B, V, H, ldv, ldh, _p(stats), _p(ws), ws.numel() * 4 - fewer)
            eng.synchronize()
            if eng is guarded:
                _exact(eng, eng.check_guards(), B, V, H)
            if fewer:
                assert rc == ENOSPC and bool((stats == FILL).all()), (rc, "a refused mdbn_cd_stats wrote")
            else:
                assert rc == 0, rc
                out.append(stats.cpu().numpy())
    d = out[1]
    S, s_h, s_v = d[:V * ldh].reshape(V, ldh)[:, :H], d[V * ldh:V * ldh + H], d[V * ldh + ldh:V * ldh + ldh + V]
    a, b = V2.astype(np.float64), P2.astype(np.float64)
    S_o, s_h_o, s_v_o = a.T @ b, b[:B].sum(0) + b[B:].sum(0), a[:B].sum(0) - a[B:].sum(0)
    tag = "exact workspace, cd_stats %dx%d B=%d" % (V, H, B)
    check(tag + ": S / max|S|", np.abs(S - S_o).max() / max(1.0, np.abs(S_o).max()), 1e-5, "stats")
    check(tag + ": s_h / max", np.abs(s_h - s_h_o).max() / max(1.0, np.abs(s_h_o).max()), 1e-5, "stats")
    check(tag + ": s_v / max", np.abs(s_v - s_v_o).max() / max(1.0, np.abs(s_v_o).max()), 1e-5, "stats")
    live = np.ones(d.size, bool)
    live[-3:] = False               # (the cost slot is written, the three floats behind it are not the call's)
    assert np.array_equal(out[0][live].view(np.int32), d[live].view(np.int32)), tag + ": differs from the plain engine's"


# ---------------------------------------------------------------------------------- C3: propagation calls, rows cut to fit
PV, PH = 520, 40
ROWS = (300, 301, 7)
SEEDS = {300: 300, 301: 316, 7: 7}      # tests/test_workspace_sizers.py: with these no draw lies within 4e-6 of its mean
ADDR = (77, 1, 5, 0, 8)                 # seed base, stream, step, draw, row offset (the seed itself: + SEEDS[rows])
TIE, TIE_CAP = 1e-6, 2                  # test_gpu_parity's near-tie mask and its cap on masked entries
FILL = 7.0


def _layer(rows, gauss):
    rs = np.random.RandomState(SEEDS[rows] + (1000 if gauss else 0))
    W = rbm_np.init_W(rs, PV, PH, np.float32)
    hb, vb = rs.normal(0, 0.2, PH).astype(np.float32), rs.normal(0, 0.2, PV).astype(np.float32)
    x = rs.normal(size=(rows, PV)).astype(np.float32) if gauss else (rs.uniform(size=(rows, PV)) < 0.3).astype(np.float32)
    h = (rs.uniform(size=(rows, PH)) < 0.5).astype(np.float32)
    return W, hb, vb, x, h


def _state(W, hb, vb, gauss, noisy=False):
    s = rbm_np.RBMState(PV, PH, W=W, hbias=hb, vbias=vb, dtype=np.float64, gauss=gauss)
    s.error_free = not noisy
    return s


def _uniform(rows, cols, seed, step=ADDR[2], draw=ADDR[3]):
    return philox_np.uniform(rows, cols, seed, ADDR[1], step, draw, ADDR[4]).astype(np.float64)


def _oracle(call, rows):
    """name -> float64 result of the call, and name -> (uniforms, mean) of its Bernoulli outputs."""
    gauss = call in ("propup", "propdown_grbm", "propdown_noisy", "free_energy_grbm")
    W, hb, vb, x, h = _layer(rows, gauss)
    seed = ADDR[0] + SEEDS[rows]
    x64, h64 = x.astype(np.float64), h.astype(np.float64)
    if call == "propup":
        s = _state(W, hb, vb, True)
        pre, mean = rbm_np.propup(s, x64)
        u = _uniform(rows, PH, seed)
        return dict(pre=pre, mean=mean, sample=(u < mean).astype(np.float32)), dict(sample=(u, mean))
    if call == "propdown_rbm":
        s = _state(W, hb, vb, False)
        u = _uniform(rows, PV, seed)
        pre, mean, sample = rbm_np.sample_v_given_h(s, h64, u)
        cost = (x64 * rbm_np.softplus(-pre) + (1 - x64) * rbm_np.softplus(pre)).sum()
        return dict(pre=pre, mean=mean, sample=sample, cost=cost), dict(sample=(u, mean))
    if call in ("propdown_grbm", "propdown_noisy"):
        noisy = call == "propdown_noisy"
        s = _state(W, hb, vb, True, noisy)
        z = philox_np.normal(rows, PV, seed, ADDR[1], ADDR[2], ADDR[3], ADDR[4])
        _, mean, sample = rbm_np.sample_v_given_h(s, h64, z)
        return dict(mean=mean, sample=sample), {}
    if call == "gibbs":
        s = _state(W, hb, vb, False)
        v, ties = x64, {}
        for t in range(3):
            u_h, u_v = _uniform(rows, PH, seed, ADDR[2] + 2 * t, 0), _uniform(rows, PV, seed, ADDR[2] + 2 * t + 1, 0)
            out = rbm_np.gibbs_vhv(s, v, u_h, u_v)
            ties["h%d" % t], ties["v%d" % t] = (u_h, out[1]), (u_v, out[4])
            v = out[5]
        return dict(pre_h=out[0], h_mean=out[1], h_sample=out[2], pre_v=out[3], v_mean=out[4], v=out[5]), \
            dict(ties, h_sample=(u_h, out[1]), v=(u_v, out[4]))
    s = _state(W, hb, vb, gauss)
    F = rbm_np.free_energy(s, x64)
    hid = rbm_np.softplus(x64 @ s.W + s.hbias).sum(axis=1)
    return dict(F=F, scale=np.maximum(hid + np.abs(F + hid), 1.0)), {}


CALLS = ("propup", "propdown_rbm", "propdown_grbm", "propdown_noisy", "gibbs", "free_energy_rbm", "free_energy_grbm")


def _device(eng, call, rows, nbytes, declare=None, opts=None):
    """One propagate-only call through ctypes on a guarded workspace of `nbytes` bytes (declare: the bytes the library is
    told).  Returns (rc, outputs as numpy, the GEMM launch kinds)."""
    import torch
    from mdbn_amd import RngAddr
    gauss = call in ("propup", "propdown_grbm", "propdown_noisy", "free_energy_grbm")
    W, hb, vb, x, h = _layer(rows, gauss)
    dW, dhb, dvb, dx, dh = [eng.to_device(a) for a in (W, hb, vb, x, h)]
    ldv, ldh = dx.stride(0), dW.stride(0)
    assert (ldv, ldh) == (PV, PH)

    def out(cols, ld):
        t = eng.alloc_matrix(rows, cols, ld)
        t._base.fill_(FILL)
        return t
    rng = RngAddr(ADDR[0] + SEEDS[rows], *ADDR[1:]).c()
    eng.reset()
    ws = eng._alloc_scratch(nbytes, "%s, %d rows" % (call, rows))
    declare = nbytes if declare is None else declare
    lib, ctx, s = eng.lib, eng.ctx, eng._stream()
    eng.kernel_timing(True)
    try:
        with options(eng, **(opts or {})):
            if call == "propup":
                o = dict(pre=out(PH, ldh), mean=out(PH, ldh), sample=out(PH, ldh))
                rc = lib.mdbn_propup_sample(ctx, s, _p(dx), rows, ldv, _p(dW), PV, PH, ldh, _p(dhb), _p(o["pre"]), _p(o["mean"]), 1.0,
                                            _p(o["sample"]), C.byref(rng), _p(ws), declare)
            elif call.startswith("propdown"):
                o = dict(mean=out(PV, ldv), sample=out(PV, ldv))
                cost = None
                if call == "propdown_rbm":
                    o["pre"] = out(PV, ldv)
                    cost = o["cost"] = torch.full((4,), FILL, dtype=torch.float32, device=eng.device)
                rc = lib.mdbn_propdown_sample(ctx, s, _p(dh), rows, ldh, _p(dW), PV, PH, ldv, _p(dvb), int(gauss),
                                              int(call == "propdown_noisy"), _p(o.get("pre")), _p(o["mean"]), _p(o["sample"]),
                                              C.byref(rng), _p(dx) if cost is not None else None, _p(cost), _p(ws), declare)
            elif call == "gibbs":
                o = dict(pre_h=out(PH, ldh), h_mean=out(PH, ldh), h_sample=out(PH, ldh), pre_v=out(PV, ldv), v_mean=out(PV, ldv))
                v = eng.alloc_matrix(rows, PV, ldv)
                v.copy_(dx)
                o["v"] = v
                rc = lib.mdbn_gibbs_chain(ctx, s, _p(v), rows, ldv, _p(dW), PV, PH, ldh, _p(dhb), _p(dvb), 0, 0, 3, _p(o["pre_h"]),
                                          _p(o["h_mean"]), _p(o["h_sample"]), _p(o["pre_v"]), _p(o["v_mean"]), C.byref(rng), _p(ws),
                                          declare)
            else:
                o = dict(F=torch.full((rows,), FILL, dtype=torch.float32, device=eng.device))
                rc = lib.mdbn_free_energy(ctx, s, _p(dx), rows, ldv, _p(dW), PV, PH, ldh, _p(dhb), _p(dvb), int(gauss), _p(o["F"]),
                                          _p(ws), declare)
            eng.check_guards()
            kinds = [kd for _, _, _, kd in eng.kernel_timing_detail()]
    finally:
        eng.kernel_timing(False)
    res = {k: t.cpu().numpy() for k, t in o.items()}
    if call == "gibbs" and rc != 0:
        assert np.array_equal(res.pop("v"), x), "a refused chain moved its state"
    return rc, res, kinds


def _off_ties(tag, got, want, u, mean):
    bad = got != want
    assert np.all(np.abs(u - mean)[bad] < TIE), tag + ": sample mismatch outside the near-tie mask"
    assert bad.sum() <= TIE_CAP, (tag, int(bad.sum()))
    assert set(np.unique(got)) <= {0.0, 1.0}, tag


def _against_oracle(tag, call, rows, got):
    want, ties = _oracle(call, rows)
    if call == "propup":
        check(tag + ": p", np.abs(got["mean"] - want["mean"]).max(), 2e-6, "prob")
        check(tag + ": pre / max|pre|", np.abs(got["pre"] - want["pre"]).max() / max(1.0, np.abs(want["pre"]).max()), 2e-6)
        _off_ties(tag, got["sample"], want["sample"], *ties["sample"])
    elif call == "propdown_rbm":
        check(tag + ": p", np.abs(got["mean"] - want["mean"]).max(), 2e-6, "prob")
        _off_ties(tag, got["sample"], want["sample"], *ties["sample"])
        check(tag + ": recon cost rel", abs(got["cost"][0] - want["cost"]) / (abs(want["cost"]) + 0.05), 2e-6)
    elif call.startswith("propdown"):
        check(tag + ": nv_mean / max|nv|", np.abs(got["mean"] - want["mean"]).max() / max(1.0, np.abs(want["mean"]).max()), 2e-6,
              "nv_mean")
        if call == "propdown_noisy":
            check(tag + ": noisy sample", np.abs(got["sample"] - want["sample"]).max(), 1e-5)
        else:
            assert np.array_equal(got["sample"], got["mean"]), tag + ": the noise-free sample is the mean"
    elif call == "gibbs":
        check(tag + ": h_mean", np.abs(got["h_mean"] - want["h_mean"]).max(), 2e-6, "prob")
        check(tag + ": v_mean", np.abs(got["v_mean"] - want["v_mean"]).max(), 2e-6, "prob")
        _off_ties(tag + " h", got["h_sample"], want["h_sample"], *ties["h_sample"])
        _off_ties(tag + " v", got["v"], want["v"], *ties["v"])
    else:
        rel = np.abs(got["F"] - want["F"]) / np.maximum(np.abs(want["F"]), 1.0)
        check(tag + ": free energy rel", rel.max(), 1e-4, "free_energy")
        check(tag + ": free energy / term magnitude", (np.abs(got["F"] - want["F"]) / want["scale"]).max(), 5e-7)


def _against_unchunked(tag, call, rows, got, ref):
    """Two device runs, each within the oracle tolerance of the same float64 result: twice that between them."""
    _, ties = _oracle(call, rows)
    for name in got:
        a, b = got[name], ref[name]
        if name in ("sample", "h_sample", "v") and name in ties:
            u, mean = ties[name]
            assert np.all(np.abs(u - mean)[a != b] < TIE), "%s: %s differs from the uncut run outside the near-tie mask" % (tag, name)
        elif name == "cost":
            check(tag + ": recon cost, cut against uncut, rel", abs(a[0] - b[0]) / (abs(b[0]) + 0.05), 2e-6)
        elif name == "F":
            check(tag + ": free energy, cut against uncut, rel", (np.abs(a - b) / np.maximum(np.abs(b), 1.0)).max(), 2e-4, "free_energy")
        elif name == "sample" and call == "propdown_noisy":
            check(tag + ": noisy sample, cut against uncut", np.abs(a - b).max(), 2e-5)
        else:
            check(tag + ": %s, cut against uncut / max" % name, np.abs(a - b).max() / max(1.0, np.abs(b).max()), 4e-6)


def _sizes(eng, rows):
    n, m = C.c_int64(), C.c_int64()
    assert eng.lib.mdbn_workspace_bytes_ctx(eng.ctx, rows, PV, PH, C.byref(n)) == 0
    assert eng.lib.mdbn_min_workspace_bytes(C.byref(m)) == 0
    return n.value, m.value


def _gemms(kinds, call):
    """GEMM launches of the call's first pass direction (kind % 10: 1 = propup layout, 0 = propdown)."""
    want = 0 if call.startswith("propdown") else 1
    return sum(1 for kd in kinds if kd % 10 == want)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("call", CALLS)
def test_propagation_calls_cut_their_rows_to_the_workspace(guarded, call, rows):
    """(i) the core sizer's bytes; (ii) the smallest workspace the calls accept, under defaults and with the activation as a
    launch of its own (fused_epilogue = 0: split-K slabs for every pass), where 4096 floats of slabs cut 300 and 301 rows into
    chunks of at most 100 (propup side, ld 40) or 4 (propdown side, ld 520); (iii) four bytes fewer declared: MDBN_ENOSPC,
    nothing written.  A chunk must not change which uniform a row sees: 301 rows end in a ragged chunk, 7 rows are one.
    Under default options propup, propdown and the chain fuse the activation into the GEMM and need no slabs: their run at
    the minimum is an UNCUT run (one launch per pass, printed); the cut is proven for them under fused_epilogue = 0, and
    for the free energy (always slabs) under both."""
    eng = guarded
    core, least = _sizes(eng, rows)
    tag = "%s, %d rows" % (call, rows)
    rc, ref, kinds = _device(eng, call, rows, core)
    assert rc == 0, (tag, rc)
    _against_oracle(tag + " on mdbn_workspace_bytes", call, rows, ref)
    print("%s: mdbn_workspace_bytes %d, %d GEMM launches; minimum %d" % (tag, core, _gemms(kinds, call), least))
    for opts in ({}, dict(fused_epilogue=0)):
        rc, got, kinds = _device(eng, call, rows, least, opts=opts)
        assert rc == 0, (tag, opts, rc)
        n = _gemms(kinds, call)
        print("%s at %d bytes %r: %d GEMM launches" % (tag, least, opts, n))
        passes = 3 if call == "gibbs" else 1
        if rows >= 300 and (opts or call.startswith("free_energy")):
            assert n > passes, "%s %r: %d GEMM launches for %d passes -- the rows were not cut, the case tests nothing" % (tag, opts, n, passes)
        _against_oracle("%s at the minimum %r" % (tag, opts), call, rows, got)
        _against_unchunked("%s %r" % (tag, opts), call, rows, got, ref)
    rc, got, kinds = _device(eng, call, rows, least, declare=least - 4)
    assert rc == ENOSPC and kinds == [], (tag, rc, kinds)
    for name, a in got.items():
        assert (a == FILL).all(), "%s: %s written by a refused call" % (tag, name)


# ---------------------------------------------------------------------------------- C4: the feature sizers
# One small case per family, run by that family's own test helpers: bit for bit the plain engine's result (which the family's
# module checks against its twin), guards intact, and with four bytes fewer declared the family's refusal (every one of
# these entry points reports a short workspace as MDBN_EINVAL, before any launch) with nothing written.
EINVAL = -1


def _host(x):
    """Every array of a helper's result, as host arrays keyed by position / name (device tensors, tuples, dicts, numbers)."""
    import torch
    if isinstance(x, dict):
        return {k: _host(v) for k, v in x.items() if k not in ("state", "zacc_t")}
    if isinstance(x, (tuple, list)):
        return {i: _host(v) for i, v in enumerate(x)}
    if isinstance(x, torch.Tensor):
        return np.atleast_1d(np.ascontiguousarray((x if x._base is None else x._base).detach().cpu().numpy()))
    return None if x is None else np.atleast_1d(np.ascontiguousarray(x))


def _flat(d, prefix=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(_flat(v, "%s%s." % (prefix, k)))
        elif v is not None:
            out[prefix + str(k)] = v
    return out


def _bit_equal(a, b, what):
    a, b = _flat(_host(a)), _flat(_host(b))
    assert sorted(a) == sorted(b) and a, (what, sorted(a), sorted(b))
    for k in sorted(a):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k)
        assert np.array_equal(a[k].view(np.uint8) if a[k].dtype.kind == "f" else a[k], b[k].view(np.uint8) if b[k].dtype.kind == "f" else b[k]), \
            "%s: %s differs from the plain engine's" % (what, k)


def _own(eng, L):
    """The test's own device operands of a layer (tests/test_gpu_updown.py: layer): under watch on a watching engine."""
    import torch
    for t in L.values():
        if isinstance(t, torch.Tensor) and hasattr(eng, "_watch"):
            eng._watch(t)
    return L


def _updown_gen(eng, path, bounds=None):
    """test_gpu_updown.gen_once / test_gpu_gupdown.gen_once, with the layer in this test's hands."""
    if bounds is None:
        import test_gpu_updown as U
        rule = U.RULES[1]
        n, gauss, hp = rule[0], rule[1], U.hp_of(rule)
        L = _own(eng, U.layer(eng, 300, 512, 512, n, gauss, 5, poison=(path == "fused")))
        args = (hp["lr"], hp["lambda_1"], hp["lambda_2"], hp["weightcost"], hp["momentum"], hp["batch_size"], n)
        cost = eng.updown_gen_step(L["x_lo"], L["x_hi"], L["G"], L["Gs"], L["c"], L["cs"], gauss, *args, cost_scale=1.0 / n, path=path)
    else:
        import test_gpu_gupdown as U
        rule = U.RULES[1]
        n, hp = rule[0], U.hp_of(rule)
        L = _own(eng, U.layer(eng, 300, 510, 512, bounds, n, 5, poison=(path == "fused")))
        args = (hp["lr"], hp["lambda_1"], hp["lambda_2"], hp["weightcost"], hp["momentum"], hp["batch_size"], n)
        cost = eng.updown_gen_step_grouped(L["x_lo"], L["x_hi"], L["G"], L["Gs"], L["c"], L["cs"], U.table(eng, bounds), *args,
                                           cost_scale=1.0 / n, path=path)
    return dict(G=L["G"], Gs=L["Gs"], c=L["c"], cs=L["cs"], cost=float(cost))


def _updown_rec(eng, path):
    """test_gpu_updown.rec_once, with the layer in this test's hands."""
    import test_gpu_updown as U
    rule = U.RULES[1]
    n, hp = rule[0], U.hp_of(rule)
    L = _own(eng, U.layer(eng, 300, 512, 512, n, False, 6, poison=False))
    r = eng.propup(L["x_lo"], L["G"], L["b"], want_pre=False, want_sample=False)[1]
    eng.updown_rec_step(L["x_lo"], L["x_hi"], r, L["G"], L["Gs"], L["b"], L["bs"], hp["lr"], hp["lambda_1"], hp["lambda_2"],
                        hp["weightcost"], hp["momentum"], hp["batch_size"], n, path=path)
    return dict(G=L["G"], Gs=L["Gs"], b=L["b"], bs=L["bs"], r=r)


def _center(eng):
    import test_gpu_center as Ce
    V, H, ldh = 255, 200, 200
    st, ldv, _, mu, lam = Ce.packed(V, H, ldh, seed=V + H)
    st = np.nan_to_num(st, nan=0.0)
    d, dmu, dlam = Ce.dev(eng, st), Ce.dev(eng, mu), Ce.dev(eng, lam)
    _own(eng, dict(stats=d, mu=dmu, lam=dlam))
    try:
        eng.center_stats(d, V, H, ldv, ldh, dmu, dlam, 20.0 / 32.0)
    except Exception:
        assert np.array_equal(d.cpu().numpy(), st), "a refused mdbn_center_stats wrote its statistics"
        raise
    return dict(stats=d)


def _center_rows(eng):
    """mdbn_center_hidden_rows on the scratch of a real step (33 rows of 100 -> 24)."""
    from mdbn_amd import RngAddr
    V, H, B = 100, 24, 33
    rs = np.random.RandomState(2)
    W = eng.to_device(rbm_np.init_W(rs, V, H, np.float32))
    hb, vb = eng.to_device(rs.normal(0, 0.2, H).astype(np.float32)), eng.to_device(rs.normal(0, 0.2, V).astype(np.float32))
    x = eng.to_device((rs.uniform(size=(B, V)) < 0.3).astype(np.float32))
    mu, lam = eng.to_device(rs.uniform(size=V).astype(np.float32)), eng.to_device(rs.uniform(size=H).astype(np.float32))
    stats, sc = eng.cd_step(x, None, W, hb, vb, False, 1, RngAddr(5, 3, 11, 0, 0), keep_f32=True)
    out = eng.center_hidden_rows(sc, B, stats, V, H, sc.V2.stride(0), sc.P2.stride(0), mu, lam, 1.0)
    return dict(s_h=out)


def _sigma(eng):
    import test_gpu_sigma as Sg
    B, V = 70, 30                       # two stages
    U, M, dU, dM, s, speed = Sg.update_inputs(eng, B, V, B, seed=B + V)
    ds, dsp = Sg.dev(eng, s), Sg.dev(eng, speed)
    _own(eng, dict(U=dU, M=dM, log_sigma=ds, speed=dsp))
    try:
        eng.sigma_update(dU, dM, B, 0.07, 0.5, Sg.LO, Sg.HI, ds, dsp)
    except Exception:
        assert np.array_equal(ds.cpu().numpy(), s) and np.array_equal(dsp.cpu().numpy(), speed), "a refused mdbn_sigma_update wrote"
        raise
    return dict(log_sigma=ds, speed=dsp)


def _group_softmax(eng):
    import _softmax_np as sm
    from mdbn_amd import RngAddr
    from mdbn_amd.engine import GroupTable
    V, ldv, bounds, B = sm.KERNEL_CASES[0]
    pre, v0, _, seed = sm.case_inputs(V, ldv, bounds, B)
    out = eng.group_softmax(eng.to_device(pre), GroupTable(eng, bounds), RngAddr(seed, sm.STREAM, sm.STEP, sm.DRAW, sm.ROW_OFFSET),
                            v0=eng.to_device(v0))
    return dict(enumerate(out))


def _rowll(eng, grouped):
    from mdbn_amd.engine import GroupTable
    V, H, R = 100, 24, 37
    rs = np.random.RandomState(4)
    W, vb = eng.to_device(rs.normal(0, 0.3, (V, H)).astype(np.float32)), eng.to_device(rs.normal(0, 0.5, V).astype(np.float32))
    h = eng.to_device((rs.uniform(size=(R, H)) < 0.5).astype(np.float32))
    if grouped:
        t = np.zeros((R, V), np.float32)
        for lo in range(0, V, 5):
            t[np.arange(R), lo + rs.randint(0, 5, R)] = 1.0
        return dict(ll=eng.propdown_row_loglik_grouped(h, W, vb, eng.to_device(t), GroupTable(eng, np.arange(0, V + 1, 5, dtype=np.int32))))
    return dict(ll=eng.propdown_row_loglik(h, W, vb, eng.to_device((rs.uniform(size=(R, V)) < 0.5).astype(np.float32)), False))


def _ais(eng, path):
    import test_gpu_ais as A
    V, H, gauss, s, _ = A.PARITY[0]
    W, c, b, bA = A._params(V, H, gauss, s)
    return A._device(eng, W, c, b, bA, gauss, np.linspace(0, 1, 9), 22, path)


def _gais(eng, path):
    import _gais_np as G
    import test_gpu_gais as A
    V, H, s, bounds, _ = G.PARITY[0]
    W, c, b, bA = G.parity_params(V, H, s)
    return A._device(eng, W, c, b, bA, bounds, np.linspace(0, 1, 9), 22, path)


def _cais(eng, path):
    import test_gpu_ais as A
    import test_gpu_cais as CA
    V, H, gauss, s, _ = A.PARITY[0]
    W, c, b, bA = A._params(V, H, gauss, s)
    N, Cn = CA.SHAPES[1]
    obs, mask = CA._clamp_inputs(N, V, gauss, N)
    return CA._device(eng, W, c, b, bA, gauss, np.linspace(0, 1, 9), obs, mask, Cn, path)


def _gcais(eng, path):
    import _gais_np as G
    import _gcais_np as X
    import test_gpu_gcais as CA
    V, H, s, bounds, _ = X.PARITY[0]
    W, c, b, bA = G.parity_params(V, H, s)
    N, Cn = X.SHAPES[1]
    obs, mask = X.clamp_inputs(N, V, bounds, N)
    return CA._device(eng, W, c, b, bA, bounds, np.linspace(0, 1, 9), obs, mask, Cn, path)


def _clamp(eng, path):
    import test_gpu_clamp as Cl
    V, H, gauss, _, s, _ = Cl.PARITY[0]
    W, c, b = Cl._params(V, H, s)
    v0, obs, mask = Cl._inputs(V, gauss, 22, True)
    return Cl._device(eng, W, c, b, gauss, v0, obs, mask, 6, 2, path)


def _gclamp(eng, path):
    import _gclamp_np as Gc
    import test_gpu_gclamp as Cl
    V, H, s, bounds, _ = Gc.PARITY[0]
    W, c, b = Gc.parity_params(V, H, s)
    v0, obs, mask = Gc.inputs(V, bounds, 22, True)
    return Cl._device(eng, W, c, b, bounds, v0, obs, mask, Gc.N_STEPS, Gc.BURN_IN, path)


def _temper(eng, path):
    import test_gpu_temper as Te
    V, H, gauss, s, M, R, _, _ = Te.PARITY[0]
    W, c, b, bA = Te._params(V, H, s)
    return Te._device(eng, W, c, b, bA, gauss, np.linspace(0, 1, R).astype(np.float32), Te._start(M, R, H), 12, 3, path)


def _gtemper(eng, path):
    import _gtemper_np as GT
    import test_gpu_gtemper as Te
    _, V, H, s, bounds, sat, _ = GT.PARITY[0]
    W, c, b, bA = GT.parity_params(V, H, s, sat)
    M, R = GT.PARITY_M, GT.PARITY_R
    return Te._device(eng, W, c, b, bA, bounds, np.linspace(0, 1, R).astype(np.float32), GT.start(M, R, H), 12, 3, path)


def _ptz(eng, path):
    """The ladder-Z run: mdbn_pt_run_z with the work accumulators."""
    import test_gpu_ptz as Pz
    import test_gpu_temper as Te
    V, H, gauss, s, M, R, _, _ = Pz.TRACE[0]
    W, c, b, bA = Te._params(V, H, s)
    return Pz._run(eng, W, c, b, bA, gauss, np.linspace(0, 1, R).astype(np.float32), Te._start(M, R, H), 12, 3, path, trace=True)


GROUPS_300 = list(range(0, 301, 5))
FEATURES = [("center_stats", _center), ("center_hidden_rows", _center_rows), ("sigma_update", _sigma),
            ("group_softmax", _group_softmax), ("rowll", lambda e: _rowll(e, False)), ("rowll_grouped", lambda e: _rowll(e, True)),
            ("updown_gen_composed", lambda e: _updown_gen(e, "composed")), ("updown_gen_fused", lambda e: _updown_gen(e, "fused")),
            ("updown_rec_composed", lambda e: _updown_rec(e, "composed")), ("updown_rec_fused", lambda e: _updown_rec(e, "fused")),
            ("updown_gen_grouped_composed", lambda e: _updown_gen(e, "composed", GROUPS_300)),
            ("updown_gen_grouped_fused", lambda e: _updown_gen(e, "fused", GROUPS_300))] + \
           [("%s_path%d" % (name, path), (lambda f, p: lambda e: f(e, p))(fn, path))
            for name, fn in (("ais", _ais), ("ais_grouped", _gais), ("ais_conditional", _cais), ("ais_conditional_grouped", _gcais),
                             ("gibbs_clamped", _clamp), ("gibbs_clamped_grouped", _gclamp), ("temper", _temper),
                             ("temper_grouped", _gtemper), ("ladder_z", _ptz)) for path in (1, 2)]
# the allocations a case may make besides the one under test (a propup or a step of its set-up, on the shared workspace)
SETUP_ONLY = ("workspace",)


@pytest.mark.parametrize("name,fn", FEATURES, ids=[f[0] for f in FEATURES])
def test_feature_sizers_bytes_are_enough_and_four_fewer_are_refused(hip_engine, guarded, name, fn):
    import torch
    from mdbn_amd import MdbnError
    plain = fn(hip_engine)
    guarded.reset()
    got = fn(guarded)
    handed = guarded.check_guards()
    own = [(what, b) for what, b in handed if what not in SETUP_ONLY]
    assert own, (name, "the call took no workspace of its own from the engine", handed)
    print("%s: %s, guards intact" % (name, ", ".join("%s = %d bytes" % wb for wb in own)))
    _bit_equal(got, plain, name)
    # four bytes fewer declared, the real buffer whole
    # Under watch: every tensor the engine allocates during the case (the call's outputs, its copies of the operands, the
    # set-up step's scratch and statistics) and the case's own in-place operands are snapshotted before the library call
    # and compared bit for bit after it has refused.
    guarded.reset()
    guarded.declare_fewer = 1
    try:
        with guarded.watching():
            with pytest.raises(MdbnError, match=r"failed \(%d\)" % EINVAL):
                fn(guarded)
            n_watched = len(guarded._watched)
    finally:
        guarded.declare_fewer = 0
    assert [rc for _, rc in guarded.refusals] == [EINVAL], (name, guarded.refusals)
    assert n_watched > 0, (name, "nothing was under watch")
    assert guarded.written_by_refused == [], "%s: the refused %s wrote %r" % (name, guarded.refusals[0][0], guarded.written_by_refused)
    handed = guarded.check_guards()
    last = guarded.arenas[-1]
    assert last.what not in SETUP_ONLY, (name, handed)
    assert bool(torch.isnan(last.view).all()), "%s: the refused call wrote into its workspace" % name
    print("%s: %s refused (%d), %d tensors under watch unchanged" % (name, guarded.refusals[0][0], EINVAL, n_watched))
