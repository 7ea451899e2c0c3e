"""Annealed importance sampling on the device (csrc/mdbn_ais.hip: mdbn_ais_run, RBM.log_partition / log_likelihood) against
the float64 numpy twin (tests/_ais_np.py) teacher-forced along the device's own samples, against brute-force partition
functions, and the one-launch path beside the general path.

Tolerance of the per-chain log weights: NOT a fixed number.  For every case the twin is run twice along the device's recorded
samples, in float64 and with float32 products / softplus / row sums (the device's regrouping); the worst gap between the two
is the float32 share of the error on exactly these inputs, and the device gets 4x that for its own summation order (the
margin the nh_mean tolerance has over SURVEY 8d).  Bound, measured value and margin go through tests/_margins.py."""
import numpy as np
import pytest

import _ais_np as A
import _saturated as S
from _margins import check

pytestmark = pytest.mark.gpu

SEED, STREAM, STEP = 5, 3, 11
# Gaussian visible samples are real numbers, compared with the twin's own draw: float32 sums of <= 256 products of
# magnitude <= 1 (256 * 2^-24 * ~1 = 1.5e-5) plus a few ulp of a Box-Muller normal |z| <= 6 between ocml and libm (~3e-6)
V_ATOL = 1e-4
TIE_SHARE = 1e-3

PARITY = [  # V, H, gauss, scale of W, paths
    (100, 24, False, 0.3, (1, 2)),
    (400, 40, True, 0.05, (1, 2)),
    (1024, 256, True, 0.02, (2,)),
]


def _params(V, H, gauss, s, seed=3):
    rs = np.random.RandomState(seed)
    W = rs.normal(0, s, (V, H)).astype(np.float32)
    c, b = rs.normal(0, 0.5, H).astype(np.float32), rs.normal(0, 0.5, V).astype(np.float32)
    bA = (b + rs.normal(0, 0.3, V)).astype(np.float32)
    return W, c, b, bA


# the layers of the first two PARITY rows with their biases on the ladder of tests/_saturated.py
SATURATED = [row for row in PARITY if row[:2] in ((100, 24), (400, 40))]


def _saturated_params(V, H, gauss, s, seed=3):
    """`_params` with c and (Bernoulli) b from tests/_saturated.py: pre-activations from -120 to 120; bA = b + N(0, 0.3)."""
    W, _, b, _ = _params(V, H, gauss, s, seed)
    c, b = S.sampler_biases(V, H, gauss, b, seed)
    bA = (b + np.random.RandomState(seed + 1).normal(0, 0.3, V)).astype(np.float32)
    return W, c, b, bA


def _device(eng, W, c, b, bA, gauss, betas, M, path, trace=True, step=STEP):
    from mdbn_amd import RngAddr
    dW, dc, db = eng.to_device(W), eng.to_device(c), eng.to_device(b)
    eng.kernel_timing(True)
    try:
        out = eng.ais(dW, dc, db, bA, gauss, betas, M, RngAddr(SEED, STREAM, step, 0, 0), path=path, trace=trace)
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


def _forced(W, c, b, bA, gauss, betas, M, th, tv, step=STEP):
    r64 = A.ais_twin(W, c, b, bA, gauss, betas, M, SEED, STREAM, step, forced=(th, tv))
    r32 = A.ais_twin(W, c, b, bA, gauss, betas, M, SEED, STREAM, step, dtype=np.float32, forced=(th, tv))
    gap = float(np.abs(r32["logw"] - r64["logw"]).max())
    return r64, gap


def _check_forced(tag, logw, r64, gap):
    print("%s: float32-vs-float64 gap of the twin %.3e, bound %.3e, device %.3e; draws %d, near ties %d, flips %d"
          % (tag, gap, 4 * gap, np.abs(logw - r64["logw"]).max(), r64["n_draws"], r64["n_ties"], r64["n_flips"]))
    assert r64["flips_outside_mask"] == 0, "%s: %d samples differ from the twin's own draw away from a tie" % (tag, r64["flips_outside_mask"])
    assert r64["n_ties"] <= TIE_SHARE * r64["n_draws"], (tag, r64["n_ties"], r64["n_draws"])
    assert r64["max_v_diff"] <= V_ATOL, "%s: Gaussian visible sample off by %.3e" % (tag, r64["max_v_diff"])
    check(tag + ": log w per chain", np.abs(logw - r64["logw"]).max(), 4 * gap, "ais_logw")


@pytest.mark.parametrize("M", [64, 22])
@pytest.mark.parametrize("V,H,gauss,s,paths", PARITY)
def test_forced_parity(hip_engine, V, H, gauss, s, paths, M):
    W, c, b, bA = _params(V, H, gauss, s)
    betas = np.linspace(0, 1, 9)
    for path in paths:
        logw, th, tv = _device(hip_engine, W, c, b, bA, gauss, betas, M, path)
        assert th.shape == (7, M, H) and tv.shape == (8, M, V) and np.isfinite(logw).all()
        r64, gap = _forced(W, c, b, bA, gauss, betas, M, th, tv)
        _check_forced("AIS forced %d->%d %s M=%d path %d" % (V, H, "GRBM" if gauss else "RBM", M, path), logw, r64, gap)


@pytest.mark.parametrize("V,H,gauss,s,paths", SATURATED)
def test_forced_parity_on_a_saturated_layer(hip_engine, V, H, gauss, s, paths):
    """The first M of test_forced_parity on a layer whose hidden (and Bernoulli visible) pre-activations reach +-120: the
    same bound rule, tie share and flip count."""
    M = 64
    W, c, b, bA = _saturated_params(V, H, gauss, s)
    betas = np.linspace(0, 1, 9)
    for path in paths:
        logw, th, tv = _device(hip_engine, W, c, b, bA, gauss, betas, M, path)
        assert th.shape == (7, M, H) and tv.shape == (8, M, V) and np.isfinite(logw).all()
        S.assert_bands("AIS saturated hidden", [tv[-1].astype(np.float64) @ W + c], S.REGIMES)
        r64, gap = _forced(W, c, b, bA, gauss, betas, M, th, tv)
        _check_forced("AIS forced saturated %d->%d %s M=%d path %d" % (V, H, "GRBM" if gauss else "RBM", M, path), logw, r64, gap)


def _layer(eng, V, H, gauss, W, c, b, seed=7):
    import mdbn_amd
    cls = mdbn_amd.GRBM if gauss else mdbn_amd.RBM
    rbm = cls(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(seed), engine=eng)
    rbm.W.set_value(W); rbm.hbias.set_value(c); rbm.vbias.set_value(b)
    return rbm


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("V,H,s,gauss", A.CASES)
def test_ground_truth(hip_engine, V, H, s, gauss, path):
    """|log Z^ - log Z| <= 4 std_err and <= 0.05 nats against the brute-force partition function."""
    W, c, b, bA = A.case_params(V, H, s, gauss)
    exact = A.brute_log_Z(W, c, b, gauss)
    rbm = _layer(hip_engine, V, H, gauss, W, c, b, seed=1)
    log_Z, err = rbm.log_partition(n_chains=512, n_betas=1000, base_vbias=bA, path=path)
    print("AIS %d->%d %s path %d: log Z^ %.5f exact %.5f |err| %.5f std_err %.5f" % (V, H, "GRBM" if gauss else "RBM", path, log_Z, exact, abs(log_Z - exact), err))
    assert abs(log_Z - exact) <= 4 * err, (log_Z, exact, err)
    assert abs(log_Z - exact) <= 0.05, (log_Z, exact)


def test_paths_agree(hip_engine):
    """Path 1 and path 2 meet the same uniforms: identical traces except where a chain met a masked near-tie (such a chain
    is then a different, equally valid chain: the forced twin vouches for each), log w within the forced-parity bound."""
    V, H, gauss, M = 100, 24, False, 64
    W, c, b, bA = _params(V, H, gauss, 0.3)
    betas = np.linspace(0, 1, 51)
    out = {p: _device(hip_engine, W, c, b, bA, gauss, betas, M, p) for p in (1, 2)}
    gaps = {}
    for p, (logw, th, tv) in out.items():
        r64, gaps[p] = _forced(W, c, b, bA, gauss, betas, M, th, tv)
        _check_forced("AIS paths 100->24 K=50 path %d" % p, logw, r64, gaps[p])
    same = (out[1][1] == out[2][1]).all(axis=(0, 2)) & (out[1][2] == out[2][2]).all(axis=(0, 2))
    assert same.sum() >= M - 2, "%d of %d chains differ between the paths" % (M - same.sum(), M)
    check("AIS paths 100->24 K=50: log w path 1 vs 2", np.abs(out[1][0] - out[2][0])[same].max(), 4 * max(gaps.values()), "ais_logw")


def test_cut_is_invisible(hip_engine):
    """A schedule longer than one launch's share (AIS_CUT = 4096 temperatures, csrc/mdbn_ais.h): log Z^ against the
    uncut twin's, within 4 of the larger standard error (the chains need not be the twin's: near ties)."""
    V, H, gauss, M, K = 100, 24, False, 64, 4096 + 3
    W, c, b, bA = _params(V, H, gauss, 0.3)
    betas = np.linspace(0, 1, K + 1)
    logw = _device(hip_engine, W, c, b, bA, gauss, betas, M, 1, trace=False)
    tw = A.ais_twin(W, c, b, bA, gauss, betas, M, SEED, STREAM, STEP)
    (lz_d, err_d), (lz_t, err_t) = A.estimate(logw, bA, H, gauss), A.estimate(tw["logw"], bA, H, gauss)
    print("AIS cut 100->24 K=%d: device %.5f +- %.5f, twin %.5f +- %.5f, chains equal to the twin's: %d of %d"
          % (K, lz_d, err_d, lz_t, err_t, int((np.abs(logw - tw["logw"]) < 1e-3).sum()), M))
    assert abs(lz_d - lz_t) <= 4 * max(err_d, err_t), (lz_d, lz_t, err_d, err_t)


@pytest.mark.parametrize("path", [1, 2])
def test_deterministic(hip_engine, path):
    W, c, b, bA = _params(100, 24, False, 0.3)
    betas = np.linspace(0, 1, 21)
    a = _device(hip_engine, W, c, b, bA, False, betas, 64, path, trace=False)
    z = _device(hip_engine, W, c, b, bA, False, betas, 64, path, trace=False)
    np.testing.assert_array_equal(a, z)


@pytest.mark.parametrize("gauss", [False, True])
def test_rng_bookkeeping_and_log_likelihood(hip_engine, gauss):
    V, H, K = 40, 14, 6
    W, c, b, bA = A.case_params(V, H, 0.2, gauss)
    rs = np.random.RandomState(2)
    data = rs.normal(size=(32, V)).astype(np.float32) if gauss else (rs.uniform(size=(32, V)) < 0.4).astype(np.float32)
    one, two = _layer(hip_engine, V, H, gauss, W, c, b), _layer(hip_engine, V, H, gauss, W, c, b)
    assert one.stream_id == two.stream_id
    one.log_partition(n_chains=16, n_betas=K, base_vbias=bA)
    assert one._rng_step == 2 * K - 1
    for t in range(2 * K - 1):                       # the eager steps the run stands for
        two.sample_h_given_v(data) if t % 2 == 0 else two.sample_v_given_h(data[:, :H])
    assert two._rng_step == 2 * K - 1
    got, want = one.gibbs_vhv(data), two.gibbs_vhv(data)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.get_value(), w.get_value())
    # log_likelihood = mean(-free_energy) - log_Z of the two public calls at the same RNG position
    step = one._rng_step
    ll, err = one.log_likelihood(data, n_chains=64, n_betas=50)
    assert one._rng_step == step + 2 * 50 - 1
    one._rng_step = step
    log_Z, err2 = one.log_partition(n_chains=64, n_betas=50, data=data)
    assert ll == float(np.mean(-np.asarray(one.free_energy(data).get_value(), dtype=np.float64)) - log_Z) and err == err2


def test_dbn_layer_log_likelihood(hip_engine):
    import mdbn_amd
    rs = np.random.RandomState(4)
    data = rs.normal(size=(64, 30)).astype(np.float32)
    dbn = mdbn_amd.DBN(numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(9), n_ins=30,
                       hidden_layers_sizes=[12, 6], n_outs=2, gauss=True, engine=hip_engine)
    ll, err = dbn.layer_log_likelihood(1, data, n_chains=64, n_betas=100)
    rbm = dbn.rbm_layers[1]
    below = dbn.get_output(data, 0)
    rbm._rng_step -= 2 * 100 - 1
    want, err2 = rbm.log_likelihood(below, n_chains=64, n_betas=100)
    assert np.isfinite(ll) and ll == want and err == err2
