"""Clamped Gibbs sampling on the device (csrc/mdbn_clamp.hip: mdbn_gibbs_clamped, RBM.gibbs_vhv_clamped / impute) against the
float64 numpy twin (tests/_clamp_np.py) teacher-forced along the device's own samples, against exact posteriors, against
mdbn_gibbs_chain, and the one-launch path beside the general path.

Tolerances: samples equal the twin's own draw outside the project's near-tie mask (4e-6), at most 1e-3 of the draws inside
it; h_mean and Bernoulli v_mean within the ``prob`` tolerance (2e-6, tests/_margins.py); Gaussian visible means / samples
within V_ATOL = 1e-4 (test_gpu_ais.py's derivation: float32 sums of <= 1024 products plus a few ulp of Box-Muller).  The
averages v_avg / h_avg have NO fixed number: the twin is run twice along the device's recorded samples, in float64 and in
float32 (products, activations, accumulators in step order); the worst gap between the two is the float32 share of the
error on exactly these inputs, and the device gets 4x that (the rule of test_gpu_ais.py)."""
import numpy as np
import pytest

import _ais_np as A
import _clamp_np as Cn
import _saturated as S
from _margins import check

pytestmark = pytest.mark.gpu

SEED, STREAM, STEP = 5, 3, 11
V_ATOL = 1e-4
PROB = 2e-6
TIE_SHARE = 1e-3

PARITY = [  # V, H, gauss, add_noise (or "gibbs": the Gaussian Gibbs sampler, gauss = 2 of the library), scale of W, paths
    (100, 24, False, False, 0.3, (1, 2)),
    (400, 40, True, True, 0.05, (1, 2)),
    (400, 40, True, False, 0.05, (1, 2)),
    (400, 40, True, "gibbs", 0.05, (1, 2)),
    (1024, 256, True, False, 0.02, (2,)),
    (1024, 256, True, "gibbs", 0.02, (2,)),
    (784, 500, False, False, 0.05, (2,)),
]


def _params(V, H, s, seed=3):
    rs = np.random.RandomState(seed)
    W = rs.normal(0, s, (V, H)).astype(np.float32)
    return W, rs.normal(0, 0.5, H).astype(np.float32), rs.normal(0, 0.5, V).astype(np.float32)


def _inputs(V, gauss, B, per_row, binary_obs=False, seed=9):
    """Start state, observed values (Bernoulli layers: probabilities in (0, 1), what a joint layer sees) and the mask."""
    rs = np.random.RandomState(seed)
    if gauss:
        v0, obs = rs.normal(size=(B, V)).astype(np.float32), rs.normal(size=(B, V)).astype(np.float32)
    else:
        v0 = (rs.uniform(size=(B, V)) < 0.5).astype(np.float32)
        obs = (rs.uniform(size=(B, V)) < 0.5).astype(np.float32) if binary_obs else rs.uniform(size=(B, V)).astype(np.float32)
    return v0, obs, Cn.half_mask(V, rows=B if per_row else None)


NAMES = ("v", "h_mean", "h_sample", "v_mean", "v_avg", "h_avg", "trace_h", "trace_v")


def _device(eng, W, c, b, gauss, v0, obs, mask, n_steps, burn_in, path, add_noise=False, trace=True, spl=0, step=STEP):
    from mdbn_amd import RngAddr
    dW, dc, db = eng.to_device(W), eng.to_device(c), eng.to_device(b)
    eng.kernel_timing(True)
    try:
        out = eng.gibbs_clamped(v0, obs, mask, dW, dc, db, gauss, n_steps, RngAddr(SEED, STREAM, step, 0, 0), burn_in=burn_in,
                                add_noise=add_noise is True, path=path, steps_per_launch=spl, trace=trace, sampler=add_noise == "gibbs")
        eng.synchronize()
        n_gemm = len(eng.kernel_timing_detail())
    finally:
        eng.kernel_timing(False)
    if path == 1:
        assert n_gemm == 0, "path 1 went through %d GEMM launches: not the one-launch kernel" % n_gemm
    if path == 2:
        assert n_gemm >= 2 * n_steps, "path 2 made %d GEMM launches for %d steps" % (n_gemm, n_steps)
    return {k: t.cpu().numpy() for k, t in zip(NAMES, out)}


def _forced(W, c, b, gauss, v0, obs, mask, n_steps, burn_in, add_noise, d, step=STEP):
    kw = dict(add_noise=add_noise is True, sampler=add_noise == "gibbs", forced=(d["trace_h"], d["trace_v"]))
    r64 = Cn.clamp_twin(W, c, b, gauss, v0, obs, mask, n_steps, burn_in, SEED, STREAM, step, **kw)
    r32 = Cn.clamp_twin(W, c, b, gauss, v0, obs, mask, n_steps, burn_in, SEED, STREAM, step, dtype=np.float32, **kw)
    return r64, r32


def _check_forced(tag, d, r64, r32, gauss):
    gap_v = float(np.abs(r32["v_avg"].astype(np.float64) - r64["v_avg"]).max())
    gap_h = float(np.abs(r32["h_avg"].astype(np.float64) - r64["h_avg"]).max())
    dev_v, dev_h = float(np.abs(d["v_avg"] - r64["v_avg"]).max()), float(np.abs(d["h_avg"] - r64["h_avg"]).max())
    print("%s: float32-vs-float64 gap of the twin v_avg %.3e h_avg %.3e; device v_avg %.3e h_avg %.3e; h_mean %.3e v_mean %.3e; "
          "draws %d, near ties %d, flips %d, Gaussian sample diff %.3e"
          % (tag, gap_v, gap_h, dev_v, dev_h, np.abs(d["h_mean"] - r64["h_mean"]).max(), np.abs(d["v_mean"] - r64["v_mean"]).max(),
             r64["n_draws"], r64["n_ties"], r64["n_flips"], r64["max_v_diff"]))
    assert r64["flips_outside_mask"] == 0, "%s: %d samples differ from the twin's own draw away from a tie" % (tag, r64["flips_outside_mask"])
    assert r64["n_ties"] <= TIE_SHARE * r64["n_draws"], (tag, r64["n_ties"], r64["n_draws"])
    assert r64["max_v_diff"] <= V_ATOL, "%s: Gaussian visible sample off by %.3e" % (tag, r64["max_v_diff"])
    np.testing.assert_array_equal(d["v"], d["trace_v"][-1])
    np.testing.assert_array_equal(d["h_sample"], d["trace_h"][-1])
    check(tag + ": h_mean", np.abs(d["h_mean"] - r64["h_mean"]).max(), PROB, "prob")
    if gauss:
        check(tag + ": v_mean (Gaussian)", np.abs(d["v_mean"] - r64["v_mean"]).max(), V_ATOL, "clamp_v_gauss")
    else:
        check(tag + ": v_mean", np.abs(d["v_mean"] - r64["v_mean"]).max(), PROB, "prob")
    check(tag + ": v_avg", dev_v, 4 * gap_v, "clamp_v_avg")
    check(tag + ": h_avg", dev_h, 4 * gap_h, "clamp_h_avg")


@pytest.mark.parametrize("per_row", [True, False])
@pytest.mark.parametrize("B", [64, 22])
@pytest.mark.parametrize("V,H,gauss,noise,s,paths", PARITY)
def test_forced_parity(hip_engine, V, H, gauss, noise, s, paths, B, per_row):
    W, c, b = _params(V, H, s)
    v0, obs, mask = _inputs(V, gauss, B, per_row)
    n_steps, burn_in = 8, 2
    for path in paths:
        d = _device(hip_engine, W, c, b, gauss, v0, obs, mask, n_steps, burn_in, path, add_noise=noise)
        assert d["trace_h"].shape == (n_steps, B, H) and d["trace_v"].shape == (n_steps, B, V)
        assert all(np.isfinite(d[k]).all() for k in NAMES)
        held = np.broadcast_to(mask != 0, (B, V))
        assert (d["trace_v"][:, held] == obs[held][None]).all(), "an observed entry moved"
        r64, r32 = _forced(W, c, b, gauss, v0, obs, mask, n_steps, burn_in, noise, d)
        _check_forced("clamp forced %d->%d %s%s B=%d %s mask path %d" % (V, H, "GRBM" if gauss else "RBM", "+" + str(noise) if noise else "", B,
                                                                        "row" if per_row else "shared", path), d, r64, r32, gauss)


@pytest.mark.parametrize("V,H,gauss,noise,s,paths", [PARITY[0], PARITY[2]])
def test_forced_parity_on_a_saturated_layer(hip_engine, V, H, gauss, noise, s, paths):
    """B = 64 with per-row masks (the first case of test_forced_parity) on 100 -> 24 RBM and 400 -> 40 GRBM with the biases
    on the ladder of tests/_saturated.py (pre-activations to +-120): the same tolerances and bound rule, and the final means
    held to the exactness rules of a saturated sigmoid."""
    B, n_steps, burn_in = 64, 8, 2
    W, c, b = _params(V, H, s)
    c, b = S.sampler_biases(V, H, gauss, b)
    v0, obs, mask = _inputs(V, gauss, B, True)
    for path in paths:
        d = _device(hip_engine, W, c, b, gauss, v0, obs, mask, n_steps, burn_in, path, add_noise=noise)
        assert all(np.isfinite(d[k]).all() for k in NAMES)
        held = np.broadcast_to(mask != 0, (B, V))
        assert (d["trace_v"][:, held] == obs[held][None]).all(), "an observed entry moved"
        r64, r32 = _forced(W, c, b, gauss, v0, obs, mask, n_steps, burn_in, noise, d)
        tag = "clamp forced saturated %d->%d %s B=%d path %d" % (V, H, "GRBM" if gauss else "RBM", B, path)
        _check_forced(tag, d, r64, r32, gauss)
        # the last step: h_mean from the visible state before it, a Bernoulli v_mean from its hidden sample (where not held)
        pre_h = d["trace_v"][-2].astype(np.float64) @ W + c
        S.assert_bands(tag, [pre_h], S.REGIMES)
        S.check_saturation(tag + " h_mean", pre_h, d["h_mean"], d["h_sample"])
        if not gauss:
            pre_v = d["trace_h"][-1].astype(np.float64) @ W.T + b
            S.assert_bands(tag, [pre_v[~held]])
            S.check_saturation(tag + " v_mean", pre_v[~held], d["v_mean"][~held], d["v"][~held])


def test_path_1_refused_where_it_does_not_fit(hip_engine):
    import mdbn_amd
    W, c, b = _params(1024, 256, 0.02)
    v0, obs, mask = _inputs(1024, True, 8, False)
    with pytest.raises(mdbn_amd.MdbnError, match="LDS-resident"):
        _device(hip_engine, W, c, b, True, v0, obs, mask, 2, 0, 1)


@pytest.mark.parametrize("gauss,noise", [(False, False), (True, False), (True, True)])
def test_no_mask_general_path_is_gibbs_chain_bit_for_bit(hip_engine, gauss, noise):
    """100 -> 24 at 64 rows: both calls run the same exact-f32 pass kernels (the 0/1 operand hint of mdbn_gibbs_chain, which the
    clamped call may not give for a visible state, only matters to the bf16 three-product kernels: these shapes are not theirs)."""
    from mdbn_amd import RngAddr
    V, H, B, n = 100, 24, 64, 6
    W, c, b = _params(V, H, 0.3)
    v0, obs, _ = _inputs(V, gauss, B, False)
    d = _device(hip_engine, W, c, b, gauss, v0, obs, np.zeros((1, V), np.float32), n, 0, 2, add_noise=noise, trace=False)
    eng = hip_engine
    ref = eng.gibbs_chain(v0, eng.to_device(W), eng.to_device(c), eng.to_device(b), gauss, n, RngAddr(SEED, STREAM, STEP, 0, 0),
                          add_noise=noise)
    for name, t in (("h_mean", ref[1]), ("h_sample", ref[2]), ("v_mean", ref[4]), ("v", ref[5])):
        np.testing.assert_array_equal(d[name], t.cpu().numpy(), err_msg=name)


def test_no_mask_where_the_operand_hint_picks_another_kernel(hip_engine):
    """784 -> 500 at 128 rows (the bf16 three-product kernels serve it): without the 0/1 hint on the visible operand the clamped
    call may differ from mdbn_gibbs_chain in the last bits, so the assertion is the forced twin's: samples equal outside the
    near-tie mask, means within ``prob``.  How many rows end in mdbn_gibbs_chain's very state is printed."""
    from mdbn_amd import RngAddr
    V, H, B, n = 784, 500, 128, 6
    W, c, b = _params(V, H, 0.05)
    v0, obs, _ = _inputs(V, False, B, False)
    mask = np.zeros((1, V), np.float32)
    d = _device(hip_engine, W, c, b, False, v0, obs, mask, n, 0, 2)
    r64, r32 = _forced(W, c, b, False, v0, obs, mask, n, 0, False, d)
    _check_forced("clamp no mask 784->500 B=128 path 2", d, r64, r32, False)
    eng = hip_engine
    ref = eng.gibbs_chain(v0, eng.to_device(W), eng.to_device(c), eng.to_device(b), False, n, RngAddr(SEED, STREAM, STEP, 0, 0))
    same = (d["v"] == ref[5].cpu().numpy()).all(axis=1)
    print("clamp no mask 784->500 B=128: %d of %d rows end in mdbn_gibbs_chain's state; h_mean differs by %.3e"
          % (same.sum(), B, np.abs(d["h_mean"] - ref[1].cpu().numpy())[same].max() if same.any() else float("nan")))


def test_full_mask_never_moves(hip_engine):
    V, H, B = 100, 24, 22
    W, c, b = _params(V, H, 0.3)
    v0, obs, _ = _inputs(V, False, B, False)
    want = Cn.sigmoid(obs.astype(np.float64) @ W.astype(np.float64) + c)
    for path in (1, 2):
        d = _device(hip_engine, W, c, b, False, v0, obs, np.ones((1, V), np.float32), 5, 3, path)      # (two accumulated steps: x + x and / 2 are exact)
        for k in ("v", "v_mean", "v_avg"):
            np.testing.assert_array_equal(d[k], obs)
        assert (d["trace_v"] == obs[None]).all()
        np.testing.assert_array_equal(d["h_avg"], d["h_mean"])
        check("clamp full mask path %d: h_mean" % path, np.abs(d["h_mean"] - want).max(), PROB, "prob")


def test_paths_agree(hip_engine):
    """Path 1 and path 2 meet the same uniforms: identical traces except where a chain met a masked near-tie (such a chain is
    then a different, equally valid chain: the forced twin vouches for each)."""
    V, H, B, n, burn = 100, 24, 64, 50, 10
    W, c, b = _params(V, H, 0.3)
    v0, obs, mask = _inputs(V, False, B, True)
    out, gaps = {}, {}
    for p in (1, 2):
        out[p] = _device(hip_engine, W, c, b, False, v0, obs, mask, n, burn, p)
        r64, r32 = _forced(W, c, b, False, v0, obs, mask, n, burn, False, out[p])
        _check_forced("clamp paths 100->24 n=50 path %d" % p, out[p], r64, r32, False)
        gaps[p] = max(np.abs(r32[k].astype(np.float64) - r64[k]).max() for k in ("v_avg", "h_avg"))
    same = (out[1]["trace_h"] == out[2]["trace_h"]).all(axis=(0, 2)) & (out[1]["trace_v"] == out[2]["trace_v"]).all(axis=(0, 2))
    assert same.sum() >= B - 2, "%d of %d chains differ between the paths" % (B - same.sum(), B)
    for k in ("v_avg", "h_avg"):
        check("clamp paths 100->24 n=50: %s path 1 vs 2" % k, np.abs(out[1][k] - out[2][k])[same].max(), 4 * max(gaps.values()), "clamp_" + k)


@pytest.mark.parametrize("gauss,noise", [(False, False), (True, True), (True, "gibbs")])
def test_cut_is_bit_invisible(hip_engine, gauss, noise):
    V, H, B, n, burn = (400, 40, 22, 20, 5) if gauss else (100, 24, 64, 20, 5)
    W, c, b = _params(V, H, 0.05 if gauss else 0.3)
    v0, obs, mask = _inputs(V, gauss, B, True)
    whole = _device(hip_engine, W, c, b, gauss, v0, obs, mask, n, burn, 1, add_noise=noise)
    for spl in (7, 1):
        cut = _device(hip_engine, W, c, b, gauss, v0, obs, mask, n, burn, 1, add_noise=noise, spl=spl)
        for k in NAMES:
            np.testing.assert_array_equal(cut[k], whole[k], err_msg="%s with %d steps per launch" % (k, spl))


@pytest.mark.parametrize("path", [1, 2])
def test_deterministic(hip_engine, path):
    W, c, b = _params(100, 24, 0.3)
    v0, obs, mask = _inputs(100, False, 64, True)
    a = _device(hip_engine, W, c, b, False, v0, obs, mask, 20, 4, path, trace=False)
    z = _device(hip_engine, W, c, b, False, v0, obs, mask, 20, 4, path, trace=False)
    for k in NAMES[:6]:
        np.testing.assert_array_equal(a[k], z[k], err_msg=k)


def _layer(eng, V, H, gauss, W, c, b, seed=1):
    import mdbn_amd
    kw = dict(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(seed), engine=eng)
    rbm = mdbn_amd.GRBM(error_free=False, **kw) if gauss else mdbn_amd.RBM(**kw)
    rbm.W.set_value(W); rbm.hbias.set_value(c); rbm.vbias.set_value(b)
    return rbm


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("V,H,s,gauss", A.CASES)
def test_ground_truth(hip_engine, V, H, s, gauss, path):
    """The cases, chain lengths and bounds of tests/test_clamp_twin.py::test_twin_against_exact_posterior through RBM.impute:
    128 chains of 600 steps (100 burn-in) for one half-observed row; |estimate - exact| <= 4 standard errors of the device's
    own chains, and the largest standard error <= 0.01.  (RBM.impute runs a GRBM as the Gibbs sampler of its model.)"""
    from test_clamp_twin import M, N_STEPS, BURN_IN, SE_CAP, ground_truth_case
    W, c, b, row, held, ev, eh = ground_truth_case(V, H, s, gauss)
    rbm = _layer(hip_engine, V, H, gauss, W, c, b)
    v_hat, h_hat = rbm.impute(np.repeat(row[None], M, axis=0), held[None].astype(np.float32), n_steps=N_STEPS, burn_in=BURN_IN,
                              n_chains=1, path=path)
    assert rbm._rng_step == 2 * N_STEPS
    worst_se, worst_z = 0.0, 0.0
    for est, exact in ((v_hat[:, ~held], ev[~held]), (h_hat, eh)):
        m, se = est.astype(np.float64).mean(axis=0), est.astype(np.float64).std(axis=0) / np.sqrt(M)
        worst_se = max(worst_se, se.max())
        worst_z = max(worst_z, (np.abs(m - exact) / np.maximum(se, 1e-12)).max())
    print("clamp %d->%d %s path %d: largest standard error %.5f, largest |error| / standard error %.2f"
          % (V, H, "GRBM" if gauss else "RBM", path, worst_se, worst_z))
    np.testing.assert_array_equal(v_hat[:, held], np.repeat(row[None, held], M, axis=0))
    assert worst_se <= SE_CAP, worst_se
    assert worst_z <= 4.0, worst_z


@pytest.mark.parametrize("V,H,gauss,one_launch", [(100, 24, False, True), (400, 40, True, True), (1024, 256, True, False)])
def test_path_0_goes_by_shape(hip_engine, V, H, gauss, one_launch):
    """path = 0: LDS-resident layers take the one-launch kernel (no GEMM launch), the others the general path."""
    from mdbn_amd import RngAddr
    eng, n = hip_engine, 6
    W, c, b = _params(V, H, 0.05)
    v0, obs, mask = _inputs(V, gauss, 22, True)
    eng.kernel_timing(True)
    try:
        out = eng.gibbs_clamped(v0, obs, mask, eng.to_device(W), eng.to_device(c), eng.to_device(b), gauss, n, RngAddr(SEED, STREAM, STEP, 0, 0),
                                burn_in=1, path=0)
        eng.synchronize()
        n_gemm = len(eng.kernel_timing_detail())
    finally:
        eng.kernel_timing(False)
    assert (n_gemm == 0) if one_launch else (n_gemm >= 2 * n), n_gemm
    want = _device(eng, W, c, b, gauss, v0, obs, mask, n, 1, 1 if one_launch else 2, trace=False)
    for k, t in zip(NAMES[:6], out):
        np.testing.assert_array_equal(t.cpu().numpy(), want[k], err_msg=k)


def test_impute_default_path_on_the_device(hip_engine):
    """RBM.impute with its default path on a Bernoulli brute-force case: the bound of test_ground_truth."""
    from test_clamp_twin import M, N_STEPS, BURN_IN, SE_CAP, ground_truth_case
    V, H, s, gauss = A.CASES[1]
    W, c, b, row, held, ev, eh = ground_truth_case(V, H, s, gauss)
    rbm = _layer(hip_engine, V, H, gauss, W, c, b)
    v_hat, h_hat = rbm.impute(np.repeat(row[None], M, axis=0), held[None].astype(np.float32), n_steps=N_STEPS, burn_in=BURN_IN)
    m, se = h_hat.astype(np.float64).mean(axis=0), h_hat.astype(np.float64).std(axis=0) / np.sqrt(M)
    assert se.max() <= SE_CAP and (np.abs(m - eh) / np.maximum(se, 1e-12)).max() <= 4.0


def test_end_to_end_imputation_beats_the_training_mean(hip_engine):
    """tests/_clamp_e2e.py on the device, the run of tests/test_clamp_api.py::test_end_to_end_imputation_beats_the_training_mean
    (which passes on the CPU checker engine with the same seeds: 0.0970 against 0.1956): the imputed joint block of the withheld
    miRNA modality is strictly closer to the truth than the block's training mean.  Both errors are printed (measured on MI355X: 0.0948 against 0.1956)."""
    import _clamp_e2e
    mse_imputed, mse_mean = _clamp_e2e.run()
    print("end to end (device): imputed block MSE %.5f, training-mean MSE %.5f" % (mse_imputed, mse_mean))
    assert mse_imputed < mse_mean, (mse_imputed, mse_mean)
