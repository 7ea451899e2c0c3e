"""Clamped Gibbs sampling of a layer with categorical visible units on the device (csrc/mdbn_clamp.hip:
mdbn_gibbs_clamped_grouped, HipEngine.gibbs_clamped_grouped, RBM.gibbs_vhv_clamped / impute with ``visible_groups``) against
the numpy twin (tests/_gclamp_np.py) teacher-forced along the device's own samples, against exact posteriors, against the
plain mdbn_gibbs_clamped (n_groups = 0), against the composed eager step, and the one-launch path beside the general path.

Tolerances (tests/test_gpu_clamp.py's and tests/test_gpu_gais.py's): a hidden or Bernoulli sample equals the twin's own draw
outside the near-tie mask 4e-6; a group's category differs from the twin's only where every boundary C_c between the two lies
within max(4e-6, 4 c_gap) of the uniform, c_gap the twin's float32-versus-float64 gap of C_c on the same inputs; near ties at
most 1e-3 of the draws; h_mean and v_mean (sigmoid or softmax entry) within the ``prob`` tolerance 2e-6; v_avg / h_avg within
4x the gap between the float32 and the float64 twin along the device's recorded samples."""
import numpy as np
import pytest

import _gclamp_np as Gc
import _saturated as S
import _softmax_np as sm
from _margins import check

pytestmark = pytest.mark.gpu

SEED, STREAM, STEP = Gc.SEED, Gc.STREAM, Gc.STEP
PROB = 2e-6
NAMES = ("v", "h_mean", "h_sample", "v_mean", "v_avg", "h_avg", "trace_h", "trace_v")


def _device(eng, W, c, b, bounds, v0, obs, mask, n_steps, burn_in, path, trace=True, spl=0, step=STEP, seed=SEED):
    from mdbn_amd import RngAddr
    from mdbn_amd.engine import GroupTable
    dW, dc, db = eng.to_device(W), eng.to_device(c), eng.to_device(b)
    table = GroupTable(eng, bounds)
    eng.kernel_timing(True)
    try:
        out = eng.gibbs_clamped_grouped(v0, obs, mask, dW, dc, db, n_steps, RngAddr(seed, STREAM, step, 0, 0), table, burn_in=burn_in,
                                        path=path, steps_per_launch=spl, trace=trace)
        eng.synchronize()
        n_gemm = len(eng.kernel_timing_detail())
    finally:
        eng.kernel_timing(False)
    if path == 1:
        assert n_gemm == 0, "path 1 went through %d GEMM launches: not the one-launch kernel" % n_gemm
    if path == 2:
        assert n_gemm >= 2 * n_steps, "path 2 made %d GEMM launches for %d steps" % (n_gemm, n_steps)
    return {k: t.cpu().numpy() for k, t in zip(NAMES, out)}


def _forced(W, c, b, bounds, v0, obs, mask, n_steps, burn_in, d, step=STEP, seed=SEED):
    kw = dict(forced=(d["trace_h"], d["trace_v"]))
    r64 = Gc.gclamp_twin(W, c, b, bounds, v0, obs, mask, n_steps, burn_in, seed, STREAM, step, **kw)
    r32 = Gc.gclamp_twin(W, c, b, bounds, v0, obs, mask, n_steps, burn_in, seed, STREAM, step, dtype=np.float32, **kw)
    return r64, r32


def _check_traces(tag, d, bounds, obs, mask):
    B, V = obs.shape
    held = Gc.group_held(mask, bounds, B, V)
    assert all(np.isfinite(d[k]).all() for k in NAMES), tag
    assert (d["trace_v"][:, held] == obs[held][None]).all(), "%s: an observed entry moved" % tag
    for lo, hi in sm.spans(bounds):
        free = ~held[:, lo]
        g = d["trace_v"][:, free, lo:hi]
        assert np.isin(g, (0.0, 1.0)).all() and (g.sum(axis=2) == 1.0).all(), "%s: a free group [%d, %d) is not one-hot" % (tag, lo, hi)
    return held


def _check_forced(tag, d, r64, r32):
    gap_v = float(np.abs(r32["v_avg"].astype(np.float64) - r64["v_avg"]).max())
    gap_h = float(np.abs(r32["h_avg"].astype(np.float64) - r64["h_avg"]).max())
    dev_v, dev_h = float(np.abs(d["v_avg"] - r64["v_avg"]).max()), float(np.abs(d["h_avg"] - r64["h_avg"]).max())
    mask_w, near, draws = Gc.near_ties(r64)
    print("%s: float32-vs-float64 gap of the twin v_avg %.3e h_avg %.3e; device v_avg %.3e h_avg %.3e; h_mean %.3e v_mean %.3e; "
          "C_c gap %.3e, mask %.3e, worst boundary miss %.3e; draws %d + %d group draws, near ties %d, flips %d + %d"
          % (tag, gap_v, gap_h, dev_v, dev_h, np.abs(d["h_mean"] - r64["h_mean"]).max(), np.abs(d["v_mean"] - r64["v_mean"]).max(),
             r64["c_gap"], mask_w, r64["group_miss"], r64["n_draws"], r64["group_draws"], near, r64["n_flips"], r64["group_flips"]))
    assert r64["flips_outside_mask"] == 0, "%s: %d samples differ from the twin's own draw away from a tie" % (tag, r64["flips_outside_mask"])
    assert r64["group_miss"] < mask_w, "%s: a category differs from the twin's %.3e from a boundary (mask %.3e)" % (tag, r64["group_miss"], mask_w)
    assert near <= Gc.TIE_SHARE * draws, (tag, near, draws)
    np.testing.assert_array_equal(d["v"], d["trace_v"][-1])
    np.testing.assert_array_equal(d["h_sample"], d["trace_h"][-1])
    check(tag + ": h_mean", np.abs(d["h_mean"] - r64["h_mean"]).max(), PROB, "prob")
    check(tag + ": v_mean", np.abs(d["v_mean"] - r64["v_mean"]).max(), sm.MEAN_TOL, "prob")
    check(tag + ": v_avg", dev_v, 4 * gap_v, "clamp_v_avg")
    check(tag + ": h_avg", dev_h, 4 * gap_h, "clamp_h_avg")


@pytest.mark.parametrize("per_row", [True, False])
@pytest.mark.parametrize("B", Gc.PARITY_B)
@pytest.mark.parametrize("V,H,s,bounds,paths", Gc.PARITY)
def test_forced_parity(hip_engine, V, H, s, bounds, paths, B, per_row):
    W, c, b = Gc.parity_params(V, H, s)
    v0, obs, mask = Gc.inputs(V, bounds, B, per_row)
    for path in paths:
        d = _device(hip_engine, W, c, b, bounds, v0, obs, mask, Gc.N_STEPS, Gc.BURN_IN, path)
        assert d["trace_h"].shape == (Gc.N_STEPS, B, H) and d["trace_v"].shape == (Gc.N_STEPS, B, V)
        tag = "gclamp forced %d->%d B=%d %s mask path %d" % (V, H, B, "row" if per_row else "shared", path)
        _check_traces(tag, d, bounds, obs, mask)
        r64, r32 = _forced(W, c, b, bounds, v0, obs, mask, Gc.N_STEPS, Gc.BURN_IN, d)
        _check_forced(tag, d, r64, r32)


def test_forced_parity_on_a_saturated_layer(hip_engine):
    """100 -> 24 in groups of 5 at B = 64 with per-row masks, the biases on the ladder of tests/_saturated.py (pre-activations
    to +-120): the same rules, and the last h_mean held to the exactness rules of a saturated sigmoid."""
    V, H, s, bounds, paths = Gc.PARITY[0]
    B = 64
    W, c, b = Gc.parity_params(V, H, s)
    c, b = S.sampler_biases(V, H, False, b)
    v0, obs, mask = Gc.inputs(V, bounds, B, True)
    for path in paths:
        d = _device(hip_engine, W, c, b, bounds, v0, obs, mask, Gc.N_STEPS, Gc.BURN_IN, path)
        tag = "gclamp forced saturated %d->%d B=%d path %d" % (V, H, B, path)
        _check_traces(tag, d, bounds, obs, mask)
        r64, r32 = _forced(W, c, b, bounds, v0, obs, mask, Gc.N_STEPS, Gc.BURN_IN, d)
        _check_forced(tag, d, r64, r32)
        pre_h = d["trace_v"][-2].astype(np.float64) @ W + c
        S.check_saturation(tag + " h_mean", pre_h, d["h_mean"], d["h_sample"])
        assert d["v_mean"].min() >= 0.0 and d["v_mean"].max() <= 1.0


@pytest.mark.parametrize("path", [1, 2])
def test_no_groups_is_the_plain_call_bit_for_bit(hip_engine, path):
    """n_groups = 0 reads no table and reproduces mdbn_gibbs_clamped(gauss = 0): every output, both paths."""
    from mdbn_amd import RngAddr
    V, H, B, n, burn = 100, 24, 22, 12, 3
    W, c, b = Gc.parity_params(V, H, 0.3)
    rs = np.random.RandomState(9)
    v0 = (rs.uniform(size=(B, V)) < 0.5).astype(np.float32)
    obs = rs.uniform(size=(B, V)).astype(np.float32)
    mask = (rs.uniform(size=(B, V)) < 0.5).astype(np.float32)
    d = _device(hip_engine, W, c, b, [V], v0, obs, mask, n, burn, path)
    eng = hip_engine
    ref = eng.gibbs_clamped(v0, obs, mask, eng.to_device(W), eng.to_device(c), eng.to_device(b), False, n, RngAddr(SEED, STREAM, STEP, 0, 0),
                            burn_in=burn, path=path, trace=True)
    for k, t in zip(NAMES, ref):
        np.testing.assert_array_equal(d[k], t.cpu().numpy(), err_msg=k)


def test_full_mask_never_moves(hip_engine):
    V, H, s, bounds, _ = Gc.PARITY[0]
    B = 22
    W, c, b = Gc.parity_params(V, H, s)
    v0, obs, _ = Gc.inputs(V, bounds, B, False)
    for path in (1, 2):
        d = _device(hip_engine, W, c, b, bounds, v0, obs, np.ones((1, V), np.float32), 5, 3, path)     # (two accumulated steps: x + x and / 2 are exact)
        for k in ("v", "v_mean", "v_avg"):
            np.testing.assert_array_equal(d[k], obs, err_msg=k)
        assert (d["trace_v"] == obs[None]).all()
        np.testing.assert_array_equal(d["h_avg"], d["h_mean"])


def test_no_mask_general_path_is_the_composed_step_bit_for_bit(hip_engine):
    """100 -> 24 at 64 rows, all-zero mask, path 2: the states of mdbn_propup_sample + the linear propdown +
    mdbn_group_softmax_sample composed with the same uniforms.  Both run the exact-f32 pass kernels at this shape (the 0/1
    operand hint only matters to the bf16 three-product kernels); should the hint pick another kernel, the forced twin's
    conditions hold instead and the comparison is printed."""
    from mdbn_amd import RngAddr
    from mdbn_amd.engine import GroupTable
    V, H, s, bounds, _ = Gc.PARITY[0]
    B, n = 64, 6
    W, c, b = Gc.parity_params(V, H, s)
    v0, obs, _ = Gc.inputs(V, bounds, B, False)
    mask = np.zeros((1, V), np.float32)
    d = _device(hip_engine, W, c, b, bounds, v0, obs, mask, n, 0, 2)
    eng = hip_engine
    dW, dc, db, table = eng.to_device(W), eng.to_device(c), eng.to_device(b), GroupTable(eng, bounds)
    state, th, tv = eng.to_device(v0), [], []
    for t in range(n):
        _, h_mean, h_sample = eng.propup(state, dW, dc, rng=RngAddr(SEED, STREAM, STEP + 2 * t, 0, 0))
        pre = eng.propdown(h_sample, dW, db, gauss=True, add_noise=False, rng=None)[1]
        v_mean, state = eng.group_softmax(pre, table, RngAddr(SEED, STREAM, STEP + 2 * t + 1, 0, 0))
        th.append(h_sample.cpu().numpy()[:, :H].copy())
        tv.append(state.cpu().numpy()[:, :V].copy())
    same = (d["trace_h"] == np.stack(th)).all() and (d["trace_v"] == np.stack(tv)).all()
    print("gclamp no mask 100->24 B=64 path 2 against the composed step: states %s; h_mean differs by %.3e, v_mean by %.3e"
          % ("equal" if same else "DIFFER", np.abs(d["h_mean"] - h_mean.cpu().numpy()[:, :H]).max(),
             np.abs(d["v_mean"] - v_mean.cpu().numpy()[:, :V]).max()))
    if not same:
        r64, r32 = _forced(W, c, b, bounds, v0, obs, mask, n, 0, d)
        _check_forced("gclamp no mask 100->24 B=64 path 2", d, r64, r32)
        return
    np.testing.assert_array_equal(d["h_mean"], h_mean.cpu().numpy()[:, :H])
    np.testing.assert_array_equal(d["v_mean"], v_mean.cpu().numpy()[:, :V])


def test_paths_agree(hip_engine):
    """Path 1 and path 2 meet the same uniforms: identical traces except where a chain met a masked near-tie (the allowance of
    tests/test_gpu_clamp.py::test_paths_agree: at most 2 of the 64 chains; the forced twin vouches for each)."""
    V, H, s, bounds, _ = Gc.PARITY[0]
    B, n, burn = 64, 50, 10
    W, c, b = Gc.parity_params(V, H, s)
    v0, obs, mask = Gc.inputs(V, bounds, B, True)
    out, gaps = {}, {}
    for p in (1, 2):
        out[p] = _device(hip_engine, W, c, b, bounds, v0, obs, mask, n, burn, p)
        r64, r32 = _forced(W, c, b, bounds, v0, obs, mask, n, burn, out[p])
        _check_forced("gclamp paths 100->24 n=50 path %d" % p, out[p], r64, r32)
        gaps[p] = max(np.abs(r32[k].astype(np.float64) - r64[k]).max() for k in ("v_avg", "h_avg"))
    same = (out[1]["trace_h"] == out[2]["trace_h"]).all(axis=(0, 2)) & (out[1]["trace_v"] == out[2]["trace_v"]).all(axis=(0, 2))
    assert same.sum() >= B - 2, "%d of %d chains differ between the paths" % (B - same.sum(), B)
    for k in ("v_avg", "h_avg"):
        check("gclamp paths 100->24 n=50: %s path 1 vs 2" % k, np.abs(out[1][k] - out[2][k])[same].max(), 4 * max(gaps.values()), "clamp_" + k)


@pytest.mark.parametrize("case", [0, 1])
def test_cut_is_bit_invisible(hip_engine, case):
    V, H, s, bounds, _ = Gc.PARITY[case]
    B, n, burn = 22, 20, 5
    W, c, b = Gc.parity_params(V, H, s)
    v0, obs, mask = Gc.inputs(V, bounds, B, True)
    whole = _device(hip_engine, W, c, b, bounds, v0, obs, mask, n, burn, 1)
    for spl in (7, 1):
        cut = _device(hip_engine, W, c, b, bounds, v0, obs, mask, n, burn, 1, spl=spl)
        for k in NAMES:
            np.testing.assert_array_equal(cut[k], whole[k], err_msg="%s with %d steps per launch" % (k, spl))


@pytest.mark.parametrize("path", [1, 2])
def test_deterministic(hip_engine, path):
    V, H, s, bounds, _ = Gc.PARITY[1]
    W, c, b = Gc.parity_params(V, H, s)
    v0, obs, mask = Gc.inputs(V, bounds, 64, True)
    a = _device(hip_engine, W, c, b, bounds, v0, obs, mask, 20, 4, path)
    z = _device(hip_engine, W, c, b, bounds, v0, obs, mask, 20, 4, path)
    for k in NAMES:
        np.testing.assert_array_equal(a[k], z[k], err_msg=k)


def test_path_1_refused_where_it_does_not_fit_and_path_0_goes_by_shape(hip_engine):
    import mdbn_amd
    from mdbn_amd import RngAddr
    from mdbn_amd.engine import GroupTable
    V, H, s, bounds, _ = Gc.PARITY[2]
    W, c, b = Gc.parity_params(V, H, s)
    v0, obs, mask = Gc.inputs(V, bounds, 8, False)
    with pytest.raises(mdbn_amd.MdbnError, match="LDS-resident"):
        _device(hip_engine, W, c, b, bounds, v0, obs, mask, 2, 0, 1)
    eng = hip_engine
    for (V, H, s, bounds, _), one_launch in ((Gc.PARITY[0], True), (Gc.PARITY[2], False)):
        W, c, b = Gc.parity_params(V, H, s)
        v0, obs, mask = Gc.inputs(V, bounds, 22, True)
        n = 4
        eng.kernel_timing(True)
        try:
            out = eng.gibbs_clamped_grouped(v0, obs, mask, eng.to_device(W), eng.to_device(c), eng.to_device(b), n,
                                            RngAddr(SEED, STREAM, STEP, 0, 0), GroupTable(eng, bounds), burn_in=1, path=0)
            eng.synchronize()
            n_gemm = len(eng.kernel_timing_detail())
        finally:
            eng.kernel_timing(False)
        assert (n_gemm == 0) if one_launch else (n_gemm >= 2 * n), n_gemm
        want = _device(eng, W, c, b, bounds, v0, obs, mask, n, 1, 1 if one_launch else 2, trace=False)
        for k, t in zip(NAMES[:6], out):
            np.testing.assert_array_equal(t.cpu().numpy(), want[k], err_msg=k)


def _layer(eng, V, H, bounds, W, c, b, seed=1):
    import mdbn_amd
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(seed), engine=eng,
                       visible_groups=bounds)
    rbm.W.set_value(W); rbm.hbias.set_value(c); rbm.vbias.set_value(b)
    return rbm


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("one_free", [False, True])
@pytest.mark.parametrize("V,H,s,bounds", Gc.CASES)
def test_ground_truth(hip_engine, V, H, s, bounds, one_free, path):
    """The cases, chain lengths, seeds and bound of tests/test_gclamp_twin.py::test_twin_against_exact_posterior: 128 chains of
    600 steps (100 burn-in) from the base of RBM.impute for one row with about half its units observed (``one_free``: with one
    group free); |mean over chains - exact| <= 2.5 standard errors, the largest standard error <= 0.01.  With one group free
    the group's v_avg also meets RBM.group_posterior within the same bound."""
    W, c, b, row, held, ev, eh = Gc.ground_truth_case(V, H, s, bounds, one_free)
    seed = (Gc.ONE_FREE_SEEDS if one_free else Gc.CASE_SEEDS)[V]
    start = np.repeat(Gc.base_start(b, bounds, row, held)[None], Gc.M, axis=0)
    d = _device(hip_engine, W, c, b, bounds, start, np.repeat(row[None], Gc.M, axis=0), held[None].astype(np.float32), Gc.GT_STEPS,
                Gc.GT_BURN, path, trace=False, seed=seed)
    se, z = Gc.z_statistic(d["v_avg"], d["h_avg"], held, ev, eh)
    print("gclamp %d->%d%s path %d: largest standard error %.5f, largest |error| / standard error %.2f"
          % (V, H, " one group free" if one_free else "", path, se, z))
    np.testing.assert_array_equal(d["v_avg"][:, held], np.repeat(row[None, held], Gc.M, axis=0))
    assert se <= Gc.SE_CAP, se
    assert z <= Gc.GT_Z, z
    if one_free:
        lo, hi = sm.spans(bounds)[0]
        post = _layer(hip_engine, V, H, bounds, W, c, b).group_posterior(row[None], 0)[0]
        est = d["v_avg"][:, lo:hi].astype(np.float64)
        m, se_g = est.mean(axis=0), est.std(axis=0) / np.sqrt(Gc.M)
        z_g = float((np.abs(m - post) / np.maximum(se_g, 1e-12)).max())
        print("gclamp %d->%d one group free path %d against group_posterior: |error| / standard error %.2f; exact differs by %.3e"
              % (V, H, path, z_g, np.abs(post - ev[lo:hi]).max()))
        assert z_g <= Gc.GT_Z, z_g


def test_impute_takes_the_device_path_by_default(hip_engine):
    """RBM.impute on a grouped layer: one mdbn_gibbs_clamped_grouped call (no GEMM launch at an LDS-resident shape), free
    groups of v_hat sum to 1 within 1e-6, observed entries come back exactly, 2 n_steps RNG steps."""
    V, H, s, bounds = Gc.CASES[3]                       # 40 -> 14: groups of 4 between Bernoulli columns
    W, c, b, _ = Gc.G.case_params(V, H, s)
    rbm = _layer(hip_engine, V, H, bounds, W, c, b)
    N = 22
    data = sm.one_hot_data(np.random.RandomState(2), N, V, bounds, p=0.5)
    mask = Gc.unit_mask(V, bounds, rows=N)
    held = mask != 0
    eng = hip_engine
    eng.kernel_timing(True)
    try:
        v_hat, h_hat = rbm.impute(data, mask, n_steps=24, burn_in=4, n_chains=2)
        eng.synchronize()
        n_gemm = len(eng.kernel_timing_detail())
    finally:
        eng.kernel_timing(False)
    assert n_gemm == 0, "impute went through %d GEMM launches: not the one-launch kernel" % n_gemm
    assert rbm._rng_step == 48
    np.testing.assert_array_equal(v_hat[held], data[held])
    for lo, hi in sm.spans(bounds):
        free = ~held[:, lo]
        assert np.abs(v_hat[free, lo:hi].astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6
    assert np.isfinite(h_hat).all() and (v_hat >= 0).all() and (v_hat <= 1).all()
    with pytest.raises(ValueError, match="columns"):
        bad = mask.copy()
        lo, hi = sm.spans(bounds)[0]
        bad[3, lo] = 1.0 - bad[3, lo]
        rbm.impute(data, bad, n_steps=4, burn_in=0)
    assert rbm._rng_step == 48
