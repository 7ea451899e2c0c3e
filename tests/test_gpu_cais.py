"""Clamped annealed importance sampling on the device (csrc/mdbn_ais.hip: mdbn_ais_cond_run, RBM.conditional_log_partition /
conditional_log_likelihood, MDBN.modality_log_likelihood) against the float64 numpy twin (tests/_cais_np.py) teacher-forced
along the device's own samples, against mdbn_ais_run (no held column: bit for bit), against the closed form (every column
held), against brute-force conditional partition functions, and the one-launch path beside the general path.

Tolerance of the per-chain log weights: the rule of tests/test_gpu_ais.py -- the twin runs twice along the device's recorded
samples, in float64 and with float32 products / softplus / row sums (the device's regrouping); the device gets 4x the worst
gap between the two for its own summation order.  Bound, measured value and margin go through tests/_margins.py as
``cais_logw``."""
import numpy as np
import pytest

import _ais_np as A
import _cais_np as CA
from _margins import check
from test_gpu_ais import PARITY, SATURATED, SEED, STEP, STREAM, TIE_SHARE, V_ATOL, _layer, _params, _saturated_params

pytestmark = pytest.mark.gpu

SHAPES = [(16, 4), (7, 3)]      # (data rows N, chains per row C): N C = 64 in whole slabs | 21 chains, slabs across two rows


def _clamp_inputs(N, V, gauss, mask_rows, seed=11):
    """Observed rows (real values: a Bernoulli layer's held columns need not be 0 / 1) and a random mask, about half held."""
    rs = np.random.RandomState(seed)
    obs = rs.normal(size=(N, V)).astype(np.float32) if gauss else rs.uniform(size=(N, V)).astype(np.float32)
    mask = (rs.uniform(size=(mask_rows, V)) < 0.5).astype(np.float32)
    return obs, mask


def _device(eng, W, c, b, bA, gauss, betas, obs, mask, C, path, trace=True, step=STEP, state=False):
    from mdbn_amd import RngAddr
    dW, dc, db = eng.to_device(W), eng.to_device(c), eng.to_device(b)
    eng.kernel_timing(True)
    try:
        out = eng.ais_conditional(dW, dc, db, bA, gauss, betas, obs, mask, C, RngAddr(SEED, STREAM, step, 0, 0), path=path,
                                  trace=trace, state=state)
        eng.synchronize()
        n_gemm = len(eng.kernel_timing_detail())
    finally:
        eng.kernel_timing(False)
    K = len(betas) - 1
    if path == 1:
        assert n_gemm == 0, "path 1 went through %d GEMM launches: not the one-launch kernel" % n_gemm
    if path == 2:
        assert n_gemm >= 2 * K - 1, "path 2 made %d GEMM launches for %d temperatures" % (n_gemm, K)
    return out


def _forced(W, c, b, bA, gauss, betas, obs, mask, C, th, tv, step=STEP):
    r64 = CA.cais_twin(W, c, b, bA, gauss, betas, obs, mask, C, SEED, STREAM, step, forced=(th, tv))
    r32 = CA.cais_twin(W, c, b, bA, gauss, betas, obs, mask, C, SEED, STREAM, step, dtype=np.float32, forced=(th, tv))
    return r64, float(np.abs(r32["logw"] - r64["logw"]).max())


def _check_forced(tag, logw, r64, gap, obs, mask, C, tv):
    print("%s: float32-vs-float64 gap of the twin %.3e, bound %.3e, device %.3e; draws %d, near ties %d, flips %d"
          % (tag, gap, 4 * gap, np.abs(logw - r64["logw"]).max(), r64["n_draws"], r64["n_ties"], r64["n_flips"]))
    assert r64["flips_outside_mask"] == 0, "%s: %d samples differ from the twin's own draw away from a tie" % (tag, r64["flips_outside_mask"])
    assert r64["n_ties"] <= TIE_SHARE * r64["n_draws"], (tag, r64["n_ties"], r64["n_draws"])
    assert r64["max_v_diff"] <= V_ATOL, "%s: Gaussian visible sample off by %.3e" % (tag, r64["max_v_diff"])
    held = np.repeat(np.broadcast_to(mask != 0, obs.shape), C, axis=0)
    want = np.repeat(obs, C, axis=0)
    assert (tv[:, held] == want[held][None, :]).all(), "%s: a held column of trace_v is not its observed value" % tag
    check(tag + ": log w per chain", np.abs(logw - r64["logw"]).max(), 4 * gap, "cais_logw")


@pytest.mark.parametrize("N,C", SHAPES)
@pytest.mark.parametrize("V,H,gauss,s,paths", PARITY)
def test_forced_parity(hip_engine, V, H, gauss, s, paths, N, C):
    W, c, b, bA = _params(V, H, gauss, s)
    betas = np.linspace(0, 1, 9)
    for path in paths:
        for mask_rows in (N, 1) if (N, C) == SHAPES[1] else (N,):        # per-row masks, and once one row for all
            obs, mask = _clamp_inputs(N, V, gauss, mask_rows)
            logw, th, tv = _device(hip_engine, W, c, b, bA, gauss, betas, obs, mask, C, path)
            assert logw.shape == (N, C) and th.shape == (7, N * C, H) and tv.shape == (8, N * C, V) and np.isfinite(logw).all()
            r64, gap = _forced(W, c, b, bA, gauss, betas, obs, mask, C, th, tv)
            _check_forced("CAIS forced %d->%d %s N=%d C=%d mask rows %d path %d" % (V, H, "GRBM" if gauss else "RBM", N, C, mask_rows, path),
                          logw, r64, gap, obs, mask, C, tv)


@pytest.mark.parametrize("V,H,gauss,s,paths", SATURATED)
def test_forced_parity_on_a_saturated_layer(hip_engine, V, H, gauss, s, paths):
    """The first (N, C) of test_forced_parity with the biases on the ladder of tests/_saturated.py (pre-activations to +-120):
    the same bound rule, tie share and flip count."""
    N, C = SHAPES[0]
    W, c, b, bA = _saturated_params(V, H, gauss, s)
    betas = np.linspace(0, 1, 9)
    obs, mask = _clamp_inputs(N, V, gauss, N)
    for path in paths:
        logw, th, tv = _device(hip_engine, W, c, b, bA, gauss, betas, obs, mask, C, path)
        assert logw.shape == (N, C) and th.shape == (7, N * C, H) and tv.shape == (8, N * C, V) and np.isfinite(logw).all()
        r64, gap = _forced(W, c, b, bA, gauss, betas, obs, mask, C, th, tv)
        _check_forced("CAIS forced saturated %d->%d %s N=%d C=%d path %d" % (V, H, "GRBM" if gauss else "RBM", N, C, path),
                      logw, r64, gap, obs, mask, C, tv)


@pytest.mark.parametrize("V,H,gauss,s,path", [(100, 24, False, 0.3, 1), (100, 24, False, 0.3, 2), (400, 40, True, 0.05, 1)])
def test_no_held_column_is_ais_run(hip_engine, V, H, gauss, s, path):
    """A zero mask: mdbn_ais_run with M = N C chains, bit for bit -- log w, the final state and both traces."""
    from mdbn_amd import RngAddr
    N, C = 11, 2
    W, c, b, bA = _params(V, H, gauss, s)
    betas = np.linspace(0, 1, 21)
    for mask_rows in (N, 1):
        obs, _ = _clamp_inputs(N, V, gauss, mask_rows)
        logw, th, tv, state = _device(hip_engine, W, c, b, bA, gauss, betas, obs, np.zeros((mask_rows, V), dtype=np.float32), C, path, state=True)
        want, wh, wv = hip_engine.ais(hip_engine.to_device(W), hip_engine.to_device(c), hip_engine.to_device(b), bA, gauss, betas, N * C,
                                      RngAddr(SEED, STREAM, STEP, 0, 0), path=path, trace=True)
        np.testing.assert_array_equal(logw.reshape(-1), want)
        np.testing.assert_array_equal(th, wh)
        np.testing.assert_array_equal(tv, wv)
        np.testing.assert_array_equal(state, wv[-1])                 # v_state on return is v_K, the last visible sample


@pytest.mark.parametrize("N,C", SHAPES)
@pytest.mark.parametrize("V,H,gauss,s,paths", PARITY)
def test_every_column_held(hip_engine, V, H, gauss, s, paths, N, C):
    """A mask of ones: nothing is random.  log w against sum_j softplus(a_j(obs)) - H log 2 (float64) within the forced-parity
    bound of the case (4x the twin's float32-vs-float64 gap on it), the state is obs, the chains of a row are bit-equal."""
    W, c, b, bA = _params(V, H, gauss, s)
    betas = np.linspace(0, 1, 9)
    obs, _ = _clamp_inputs(N, V, gauss, N)
    mask = np.ones((1, V), dtype=np.float32)
    want = np.logaddexp(0.0, obs.astype(np.float64) @ W.astype(np.float64) + c.astype(np.float64)).sum(axis=1) - H * np.log(2.0)
    r64 = CA.cais_twin(W, c, b, bA, gauss, betas, obs, mask, C, SEED, STREAM, STEP)
    r32 = CA.cais_twin(W, c, b, bA, gauss, betas, obs, mask, C, SEED, STREAM, STEP, dtype=np.float32)
    gap = float(np.abs(r32["logw"] - r64["logw"]).max())
    assert np.abs(r64["logw"] - want[:, None]).max() <= 1e-9
    for path in paths:
        logw, th, tv, state = _device(hip_engine, W, c, b, bA, gauss, betas, obs, mask, C, path, state=True)
        tag = "CAIS all held %d->%d %s N=%d C=%d path %d" % (V, H, "GRBM" if gauss else "RBM", N, C, path)
        print("%s: float32-vs-float64 gap of the twin %.3e, bound %.3e, device %.3e" % (tag, gap, 4 * gap, np.abs(logw - want[:, None]).max()))
        np.testing.assert_array_equal(state, np.repeat(obs, C, axis=0))
        assert (tv == np.repeat(obs, C, axis=0)[None]).all()
        assert (logw == logw[:, :1]).all(), "%s: the chains of a row differ" % tag
        check(tag + ": log w per chain", np.abs(logw - want[:, None]).max(), 4 * gap, "cais_logw")


N_ROWS, CHAINS = 8, 256


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("V,H,s,gauss", A.CASES)
def test_ground_truth(hip_engine, V, H, s, gauss, path):
    """8 rows with per-row block masks over half the columns, C = 256, 1000 temperatures: every row's log Z_r^ and log p^ within
    4 std_err and 0.05 nats of the brute-force conditional partition function / the float64 log p built from it."""
    W, c, b, bA = A.case_params(V, H, s, gauss)
    v, mask = CA.observed(N_ROWS, V, gauss), CA.block_masks(N_ROWS, V)
    rbm = _layer(hip_engine, V, H, gauss, W, c, b, seed=1)
    log_Z, err = rbm.conditional_log_partition(v, mask, n_chains=CHAINS, n_betas=1000, base_vbias=bA, path=path)
    log_p, err_p = rbm.conditional_log_likelihood(v, mask, n_chains=CHAINS, n_betas=1000, base_vbias=bA, path=path)
    assert log_Z.shape == err.shape == log_p.shape == err_p.shape == (N_ROWS,) and (err > 0).all() and (err_p > 0).all()
    for row in range(N_ROWS):
        exact = CA.exact_cond_log_Z(W, c, b, v[row], mask[row], gauss)
        exact_p = CA.exact_cond_log_p(W, c, b, v[row], mask[row], gauss)
        print("CAIS %d->%d %s path %d row %d: log Z^ %.5f exact %.5f |err| %.5f std_err %.5f; log p^ %.5f exact %.5f |err| %.5f std_err %.5f"
              % (V, H, "GRBM" if gauss else "RBM", path, row, log_Z[row], exact, abs(log_Z[row] - exact), err[row],
                 log_p[row], exact_p, abs(log_p[row] - exact_p), err_p[row]))
        assert abs(log_Z[row] - exact) <= 4 * err[row], (row, log_Z[row], exact, err[row])
        assert abs(log_Z[row] - exact) <= 0.05, (row, log_Z[row], exact)
        assert abs(log_p[row] - exact_p) <= 4 * err_p[row], (row, log_p[row], exact_p, err_p[row])
        assert abs(log_p[row] - exact_p) <= 0.05, (row, log_p[row], exact_p)


def test_paths_agree(hip_engine):
    """Path 1 and path 2 meet the same uniforms: identical traces except where a chain met a masked near-tie (the forced twin
    vouches for each), log w within the forced-parity bound."""
    V, H, gauss, (N, C) = 100, 24, False, SHAPES[0]
    W, c, b, bA = _params(V, H, gauss, 0.3)
    betas = np.linspace(0, 1, 51)
    obs, mask = _clamp_inputs(N, V, gauss, N)
    out = {p: _device(hip_engine, W, c, b, bA, gauss, betas, obs, mask, C, p) for p in (1, 2)}
    gaps = {}
    for p, (logw, th, tv) in out.items():
        r64, gaps[p] = _forced(W, c, b, bA, gauss, betas, obs, mask, C, th, tv)
        _check_forced("CAIS paths 100->24 K=50 path %d" % p, logw, r64, gaps[p], obs, mask, C, tv)
    same = (out[1][1] == out[2][1]).all(axis=(0, 2)) & (out[1][2] == out[2][2]).all(axis=(0, 2))
    assert same.sum() >= N * C - 2, "%d of %d chains differ between the paths" % (N * C - same.sum(), N * C)
    check("CAIS paths 100->24 K=50: log w path 1 vs 2", np.abs(out[1][0] - out[2][0]).reshape(-1)[same].max(), 4 * max(gaps.values()), "cais_logw")


def test_cut_is_invisible(hip_engine):
    """A schedule longer than one launch's share (AIS_CUT = 4096 temperatures, csrc/mdbn_ais.h) on path 1: every row's
    log Z_r^ against the uncut twin's, within 4 of the larger standard error (the chains need not be the twin's: near ties)."""
    V, H, gauss, (N, C), K = 100, 24, False, SHAPES[0], 4096 + 3
    W, c, b, bA = _params(V, H, gauss, 0.3)
    betas = np.linspace(0, 1, K + 1)
    obs, mask = _clamp_inputs(N, V, gauss, N)
    logw = _device(hip_engine, W, c, b, bA, gauss, betas, obs, mask, C, 1, trace=False)
    tw = CA.cais_twin(W, c, b, bA, gauss, betas, obs, mask, C, SEED, STREAM, STEP)
    (lz_d, err_d), (lz_t, err_t) = CA.estimate_rows(logw, bA, mask, H, gauss), CA.estimate_rows(tw["logw"], bA, mask, H, gauss)
    print("CAIS cut 100->24 K=%d: worst |device - twin| %.5f, chains equal to the twin's: %d of %d"
          % (K, np.abs(lz_d - lz_t).max(), int((np.abs(logw - tw["logw"]) < 1e-3).sum()), N * C))
    assert (np.abs(lz_d - lz_t) <= 4 * np.maximum(err_d, err_t)).all(), (lz_d, lz_t, err_d, err_t)


@pytest.mark.parametrize("path", [1, 2])
def test_deterministic(hip_engine, path):
    W, c, b, bA = _params(100, 24, False, 0.3)
    betas = np.linspace(0, 1, 21)
    obs, mask = _clamp_inputs(7, 100, False, 7)
    a = _device(hip_engine, W, c, b, bA, False, betas, obs, mask, 3, path, trace=False)
    z = _device(hip_engine, W, c, b, bA, False, betas, obs, mask, 3, path, trace=False)
    np.testing.assert_array_equal(a, z)


@pytest.mark.parametrize("gauss", [False, True])
def test_rng_bookkeeping(hip_engine, gauss):
    V, H, K = 40, 14, 6
    W, c, b, bA = A.case_params(V, H, 0.2, gauss)
    data, mask = CA.observed(32, V, gauss), CA.block_masks(32, V)
    one, two = _layer(hip_engine, V, H, gauss, W, c, b), _layer(hip_engine, V, H, gauss, W, c, b)
    assert one.stream_id == two.stream_id
    one.conditional_log_partition(data, mask, n_chains=3, n_betas=K, base_vbias=bA)
    assert one._rng_step == 2 * K - 1
    for t in range(2 * K - 1):                       # the eager steps the run stands for
        two.sample_h_given_v(data) if t % 2 == 0 else two.sample_v_given_h(data[:, :H])
    assert two._rng_step == 2 * K - 1
    got, want = one.gibbs_vhv(data), two.gibbs_vhv(data)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.get_value(), w.get_value())
    # conditional_log_likelihood is built from conditional_log_partition at the same RNG position
    step = one._rng_step
    log_p, err = one.conditional_log_likelihood(data, mask[:1], n_chains=5, n_betas=50)
    assert one._rng_step == step + 2 * 50 - 1
    one._rng_step = step
    log_Z, err2 = one.conditional_log_partition(data, mask[:1], n_chains=5, n_betas=50)
    held = np.broadcast_to(mask[:1] != 0, data.shape)
    bb = b.astype(np.float64)[None, :]
    term = 0.5 * (held * (data - bb) ** 2).sum(axis=1) if gauss else -(held * data * bb).sum(axis=1)
    np.testing.assert_array_equal(log_p, -np.asarray(one.free_energy(data).get_value(), dtype=np.float64) + term - log_Z)
    np.testing.assert_array_equal(err, err2)


def test_likelihood_edge_rules(hip_engine):
    """A row with no free column gets log_p = 0, std_err = 0; a Bernoulli layer refuses a free entry that is not 0 / 1 and takes
    any real value in a held one."""
    V, H = 24, 12
    W, c, b, bA = A.case_params(V, H, 0.5, False)
    rbm = _layer(hip_engine, V, H, False, W, c, b)
    v, mask = CA.observed(3, V, False), CA.block_masks(3, V)
    mask[1] = 1.0
    v[2, mask[2] != 0] = 0.37
    log_p, err = rbm.conditional_log_likelihood(v, mask, n_chains=8, n_betas=20, base_vbias=bA)
    assert log_p[1] == 0.0 and err[1] == 0.0 and np.isfinite(log_p).all() and err[0] > 0 and err[2] > 0
    v[0, np.flatnonzero(mask[0] == 0)[0]] = 0.5
    with pytest.raises(ValueError):
        rbm.conditional_log_likelihood(v, mask, n_chains=8, n_betas=20, base_vbias=bA)


def test_modality_log_likelihood(hip_engine):
    """Two tiny modality DBNs (tops 6 and 5) under a joint DBN 11 -> 8, random weights: log_p is conditional_log_likelihood of
    the joint layer's first RBM at the same RNG position on the binarised target block, baseline the closed form."""
    import mdbn_amd
    rs = np.random.RandomState(3)
    N, widths = 12, (6, 5)
    nets = [mdbn_amd.DBN(numpy_rng=np.random.RandomState(5 + i), theano_rng=mdbn_amd.RandomStreams(9 + i), n_ins=n_in,
                         hidden_layers_sizes=[7], n_outs=w, gauss=True, engine=hip_engine) for i, (n_in, w) in enumerate(zip((10, 9), widths))]
    joint = mdbn_amd.DBN(numpy_rng=np.random.RandomState(8), theano_rng=mdbn_amd.RandomStreams(4), n_ins=sum(widths),
                         hidden_layers_sizes=[8], n_outs=2, gauss=False, engine=hip_engine)
    inputs = [rs.normal(size=(N, 10)).astype(np.float32), rs.normal(size=(N, 9)).astype(np.float32)]
    rbm = joint.rbm_layers[0]
    blocks = [np.asarray(net.get_output(x), dtype=np.float32) for net, x in zip(nets, inputs)]
    stacked = np.concatenate(blocks, axis=1)
    for target, (lo, hi) in enumerate(((0, 6), (6, 11))):
        frac = (stacked[:, lo:hi] != 0) & (stacked[:, lo:hi] != 1)
        assert frac.any(), "the fixture's target block holds no fractional activation"
        step = rbm._rng_step
        out = mdbn_amd.modality_log_likelihood(nets, joint, inputs, target, n_chains=64, n_betas=200)
        assert rbm._rng_step == step + 2 * 200 - 1
        visible = stacked.copy()
        visible[:, lo:hi] = (stacked[:, lo:hi] >= 0.5).astype(np.float32)
        mask = np.ones((1, 11), dtype=np.float32)
        mask[:, lo:hi] = 0.0
        bA = rbm.base_rate_vbias(stacked)
        rbm._rng_step = step
        log_p, err = rbm.conditional_log_likelihood(visible, mask, n_chains=64, n_betas=200, base_vbias=bA)
        np.testing.assert_array_equal(out["log_p"], log_p)
        np.testing.assert_array_equal(out["std_err"], err)
        p = 1.0 / (1.0 + np.exp(-bA.astype(np.float64)[lo:hi]))
        t = visible[:, lo:hi].astype(np.float64)
        np.testing.assert_allclose(out["baseline"], (t * np.log(p) + (1 - t) * np.log1p(-p)).sum(axis=1), rtol=0, atol=1e-9)
        assert out["log_p"].shape == (N,) and np.isfinite(out["log_p"]).all() and (out["log_p"] < 0).all()
        assert np.isfinite(out["std_err"]).all() and (out["std_err"] >= 0).all()
        assert out["gain"] == float(np.mean(out["log_p"] - out["baseline"]))
        assert abs(out["gain_std_err"] - np.sqrt((err ** 2).sum()) / N) <= 1e-15
    other = mdbn_amd.modality_log_likelihood(nets, joint, inputs, 0, n_chains=64, n_betas=200, base_data=stacked[:5])
    assert np.isfinite(other["gain"])
    with pytest.raises(ValueError):
        mdbn_amd.modality_log_likelihood(nets, joint, [inputs[0], None], 0)
