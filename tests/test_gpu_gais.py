"""Annealed importance sampling of a layer with categorical visible units on the device (csrc/mdbn_ais.hip:
mdbn_ais_run_grouped, HipEngine.ais_grouped, RBM.log_partition / log_likelihood with ``visible_groups``) against the numpy
twin (tests/_gais_np.py) teacher-forced along the device's own samples, against brute-force partition functions, against
mdbn_ais_run where there are no groups, and the one-launch path beside the general path.

Tolerance of the per-chain log weights: the rule of tests/test_gpu_ais.py -- 4x the twin's own float32-versus-float64 gap on
the recorded samples, through tests/_margins.py.  A draw that differs from the twin's own must be a near tie: |u - p| <
_ais_np.TIE for a hidden or Bernoulli draw; for a group every boundary C_c between the two categories within
max(TIE, 4 c_gap) of the uniform, c_gap the twin's float32-versus-float64 gap of C_c on the same inputs.  Near ties are capped
by 3 + E + 4 sqrt(E), E the expected count from the shape (_gais_np.tie_cap)."""
import ctypes as C

import numpy as np
import pytest

import _ais_np as A
import _gais_np as G
import _saturated as S
import _softmax_np as sm
from _margins import check

pytestmark = pytest.mark.gpu

SEED, STREAM, STEP = G.SEED, G.STREAM, G.STEP


def _table(eng, bounds):
    from mdbn_amd.engine import GroupTable
    return GroupTable(eng, np.asarray(bounds, dtype=np.int32))


def _device(eng, W, c, b, bA, bounds, betas, M, path, trace=True, step=STEP):
    from mdbn_amd import RngAddr
    dW, dc, db = eng.to_device(W), eng.to_device(c), eng.to_device(b)
    eng.kernel_timing(True)
    try:
        out = eng.ais_grouped(dW, dc, db, bA, betas, M, RngAddr(SEED, STREAM, step, 0, 0), _table(eng, bounds), path=path, trace=trace)
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


def _forced(W, c, b, bA, bounds, betas, M, th, tv, step=STEP):
    r64 = G.ais_twin(W, c, b, bA, bounds, betas, M, SEED, STREAM, step, forced=(th, tv))
    r32 = G.ais_twin(W, c, b, bA, bounds, betas, M, SEED, STREAM, step, dtype=np.float32, forced=(th, tv))
    return r64, float(np.abs(r32["logw"] - r64["logw"]).max())


def _check_forced(tag, logw, tv, bounds, r64, gap):
    mask = max(A.TIE, 4.0 * r64["c_gap"])
    near, cap = r64["n_ties"] + r64["group_near"](mask), G.tie_cap(r64, mask)
    print("%s: float32-vs-float64 gap of the twin %.3e, bound %.3e, device %.3e; C_c gap %.3e, mask %.3e, worst boundary miss %.3e; "
          "draws %d + %d group draws, near ties %d (cap %d), flips %d + %d"
          % (tag, gap, 4 * gap, np.abs(logw - r64["logw"]).max(), r64["c_gap"], mask, r64["group_miss"], r64["n_draws"],
             r64["group_draws"], near, cap, r64["n_flips"], r64["group_flips"]))
    for lo, hi in sm.spans(bounds):
        assert (tv[:, :, lo:hi].sum(axis=2) == 1.0).all() and np.isin(tv[:, :, lo:hi], (0.0, 1.0)).all(), (tag, lo, hi)
    assert r64["flips_outside_mask"] == 0, "%s: %d samples differ from the twin's own draw away from a tie" % (tag, r64["flips_outside_mask"])
    assert r64["group_miss"] < mask, "%s: a category differs from the twin's %.3e from a boundary (mask %.3e)" % (tag, r64["group_miss"], mask)
    assert near <= cap, (tag, near, cap)
    check(tag + ": log w per chain", np.abs(logw - r64["logw"]).max(), 4 * gap, "ais_logw")


@pytest.mark.parametrize("M", G.PARITY_M)
@pytest.mark.parametrize("V,H,s,bounds,paths", G.PARITY)
def test_forced_parity(hip_engine, V, H, s, bounds, paths, M):
    W, c, b, bA = G.parity_params(V, H, s)
    betas = np.linspace(0, 1, 9)
    for path in paths:
        logw, th, tv = _device(hip_engine, W, c, b, bA, bounds, betas, M, path)
        assert th.shape == (7, M, H) and tv.shape == (8, M, V) and np.isfinite(logw).all()
        r64, gap = _forced(W, c, b, bA, bounds, betas, M, th, tv)
        _check_forced("GAIS forced %d->%d M=%d path %d" % (V, H, M, path), logw, tv, bounds, r64, gap)


def test_forced_parity_on_a_saturated_layer(hip_engine):
    """100 -> 24 in groups of 5 with the biases on the ladder of tests/_saturated.py: the same bound rule, masks and cap."""
    V, H, s, bounds, paths = G.PARITY[0]
    M = 64
    W, _, b, _ = G.parity_params(V, H, s)
    c, b = S.sampler_biases(V, H, False, b, 3)
    bA = (b + np.random.RandomState(4).normal(0, 0.3, V)).astype(np.float32)
    betas = np.linspace(0, 1, 9)
    for path in paths:
        logw, th, tv = _device(hip_engine, W, c, b, bA, bounds, betas, M, path)
        assert np.isfinite(logw).all()
        r64, gap = _forced(W, c, b, bA, bounds, betas, M, th, tv)
        _check_forced("GAIS forced saturated %d->%d path %d" % (V, H, path), logw, tv, bounds, r64, gap)


@pytest.mark.parametrize("path", [1, 2])
def test_no_groups_is_the_plain_run_bit_for_bit(hip_engine, path):
    from mdbn_amd import RngAddr
    eng = hip_engine
    V, H, M = 100, 24, 22
    W, c, b, bA = G.parity_params(V, H, 0.3)
    betas = np.linspace(0, 1, 9)
    dW, dc, db = eng.to_device(W), eng.to_device(c), eng.to_device(b)
    rng = RngAddr(SEED, STREAM, STEP, 0, 0)
    empty = _table(eng, [V])
    assert empty.n_groups == 0
    plain = eng._ais(dW, dc, db, bA, False, betas, M, rng, path, True)
    grouped = eng._ais(dW, dc, db, bA, False, betas, M, rng, path, True, groups=empty)
    for p, g in zip(plain[:3], grouped[:3]):
        np.testing.assert_array_equal(p, g)
    np.testing.assert_array_equal(plain[3].cpu().numpy(), grouped[3].cpu().numpy())


def test_paths_agree(hip_engine):
    """Path 1 and path 2 meet the same uniforms over 50 temperatures: at most 2 of 64 chains part at a near tie, log w of the
    rest within the forced bound."""
    V, H, s, bounds, _ = G.PARITY[0]
    M = 64
    W, c, b, bA = G.parity_params(V, H, s)
    betas = np.linspace(0, 1, 51)
    out = {p: _device(hip_engine, W, c, b, bA, bounds, betas, M, p) for p in (1, 2)}
    gaps = {}
    for p, (logw, th, tv) in out.items():
        r64, gaps[p] = _forced(W, c, b, bA, bounds, betas, M, th, tv)
        _check_forced("GAIS paths 100->24 K=50 path %d" % p, logw, tv, bounds, r64, gaps[p])
    same = (out[1][1] == out[2][1]).all(axis=(0, 2)) & (out[1][2] == out[2][2]).all(axis=(0, 2))
    assert same.sum() >= M - 2, "%d of %d chains differ between the paths" % (M - same.sum(), M)
    check("GAIS paths 100->24 K=50: log w path 1 vs 2", np.abs(out[1][0] - out[2][0])[same].max(), 4 * max(gaps.values()), "ais_logw")


def test_cut_is_invisible(hip_engine):
    """4099 temperatures on path 1 (AIS_CUT = 4096): log Z^ against the uncut twin's within 4 of the larger standard error."""
    V, H, s, bounds, _ = G.PARITY[0]
    M, K = 64, 4096 + 3
    W, c, b, bA = G.parity_params(V, H, s)
    betas = np.linspace(0, 1, K + 1)
    logw = _device(hip_engine, W, c, b, bA, bounds, betas, M, 1, trace=False)
    tw = G.ais_twin(W, c, b, bA, bounds, betas, M, SEED, STREAM, STEP, gaps=False)
    (lz_d, err_d), (lz_t, err_t) = G.estimate(logw, bA, H, bounds), G.estimate(tw["logw"], bA, H, bounds)
    print("GAIS cut 100->24 K=%d: device %.5f +- %.5f, twin %.5f +- %.5f, chains equal to the twin's: %d of %d"
          % (K, lz_d, err_d, lz_t, err_t, int((np.abs(logw - tw["logw"]) < 1e-3).sum()), M))
    assert abs(lz_d - lz_t) <= 4 * max(err_d, err_t), (lz_d, lz_t, err_d, err_t)


@pytest.mark.parametrize("path", [1, 2])
def test_deterministic(hip_engine, path):
    V, H, s, bounds, _ = G.PARITY[0]
    W, c, b, bA = G.parity_params(V, H, s)
    betas = np.linspace(0, 1, 21)
    a = _device(hip_engine, W, c, b, bA, bounds, betas, 64, path, trace=False)
    z = _device(hip_engine, W, c, b, bA, bounds, betas, 64, path, trace=False)
    np.testing.assert_array_equal(a, z)


def _layer(eng, V, H, bounds, W, c, b, seed=7):
    import mdbn_amd
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(seed),
                       engine=eng, visible_groups=bounds)
    rbm.W.set_value(W); rbm.hbias.set_value(c); rbm.vbias.set_value(b)
    return rbm


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("V,H,s,bounds", G.CASES)
def test_ground_truth(hip_engine, V, H, s, bounds, path):
    """|log Z^ - log Z| <= 4 std_err and <= 0.05 nats against the brute-force partition function."""
    W, c, b, bA = G.case_params(V, H, s)
    exact = G.brute_log_Z(W, c, b, bounds)
    rbm = _layer(hip_engine, V, H, bounds, W, c, b, seed=1)
    log_Z, err = rbm.log_partition(n_chains=512, n_betas=1000, base_vbias=bA, path=path)
    print("GAIS %d->%d path %d: log Z^ %.5f exact %.5f |err| %.5f std_err %.5f" % (V, H, path, log_Z, exact, abs(log_Z - exact), err))
    assert abs(log_Z - exact) <= 4 * err, (log_Z, exact, err)
    assert abs(log_Z - exact) <= 0.05, (log_Z, exact)


def test_rng_bookkeeping_and_log_likelihood(hip_engine):
    V, H, s, bounds = G.CASES[3]
    K = 50
    W, c, b, bA = G.case_params(V, H, s)
    data = sm.one_hot_data(np.random.RandomState(2), 32, V, bounds)
    one = _layer(hip_engine, V, H, bounds, W, c, b)
    ll, err = one.log_likelihood(data, n_chains=64, n_betas=K)
    assert one._rng_step == 2 * K - 1
    one._rng_step = 0
    log_Z, err2 = one.log_partition(n_chains=64, n_betas=K, data=data)
    assert one._rng_step == 2 * K - 1
    assert ll == float(np.mean(-np.asarray(one.free_energy(data).get_value(), dtype=np.float64)) - log_Z) and err == err2
    bad = data.copy()
    bad[3, bounds[0]:bounds[1]] = 1.0
    with pytest.raises(ValueError, match="exactly one 1"):
        one.log_likelihood(bad, n_chains=64, n_betas=K)


def test_dbn_layer_log_likelihood(hip_engine):
    import mdbn_amd
    mdbn_amd.DBN.verbose = False
    bounds = list(range(0, 31, 5))
    data = sm.one_hot_data(np.random.RandomState(4), 64, 30, bounds)
    dbn = mdbn_amd.DBN(numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(9), n_ins=30,
                       hidden_layers_sizes=[12, 6], n_outs=2, gauss=False, engine=hip_engine, visible_groups=bounds)
    ll, err = dbn.layer_log_likelihood(0, data, n_chains=64, n_betas=100)
    rbm = dbn.rbm_layers[0]
    rbm._rng_step -= 2 * 100 - 1
    want, err2 = rbm.log_likelihood(data, n_chains=64, n_betas=100)
    assert np.isfinite(ll) and ll == want and err == err2


def test_refused_calls_leave_the_outputs_untouched(hip_engine):
    """Every MDBN_EINVAL case of mdbn_ais_run_grouped: a message, no launch, logw and v_state as they were."""
    import torch
    from mdbn_amd import RngAddr, _lib
    from mdbn_amd.engine import padded_ld
    eng = hip_engine

    def call(V, H, bounds, gauss=0, path=0, host=True, M=16):
        W, c, b, bA = G.parity_params(V, H, 0.05)
        dW, dc, db, dbA = (eng.to_device(x) for x in (W, c, b, bA))
        ldh, ldv = dW.stride(0), padded_ld(V)
        betas = torch.from_numpy(np.linspace(0, 1, 5).astype(np.float32)).to(eng.device)
        n = C.c_int64()
        _lib.check(eng.lib.mdbn_ais_workspace_bytes(eng.ctx, M, V, H, 5, 2, C.byref(n)), "mdbn_ais_workspace_bytes")
        ws = torch.empty(n.value // 4 + 64, dtype=torch.float32, device=eng.device)
        logw = torch.full((M,), 7.0, dtype=torch.float64, device=eng.device)
        v_state = torch.full((M, ldv), 7.0, dtype=torch.float32, device=eng.device)
        host_t = np.ascontiguousarray(bounds, dtype=np.int32)
        dev_t = torch.from_numpy(host_t.copy()).to(eng.device)
        r = RngAddr(SEED, STREAM, STEP, 0, 0).c()
        rc = eng.lib.mdbn_ais_run_grouped(
            eng.ctx, eng._stream(), eng._p(dW), V, H, ldh, eng._p(dc), eng._p(db), eng._p(dbA), gauss, eng._p(betas), 5, M, ldv,
            eng._p(v_state), eng._p(logw), None, None, path, C.byref(r), eng._p(ws), ws.numel() * 4, eng._p(dev_t),
            C.c_void_p(host_t.ctypes.data) if host else None, host_t.size - 1)
        eng.synchronize()
        return rc, _lib.last_error(), bool((logw == 7.0).all()) and bool((v_state == 7.0).all())

    good = list(range(0, 101, 5))
    rc, _, untouched = call(100, 24, good)
    assert rc == 0 and not untouched
    for what, kw in (("gauss", dict(V=100, H=24, bounds=good, gauss=1)),
                     ("a descending table", dict(V=100, H=24, bounds=[0, 10, 5, 20])),
                     ("a group of 1", dict(V=100, H=24, bounds=[0, 5, 6, 10])),
                     ("a group of 65", dict(V=100, H=24, bounds=[0, 65])),
                     ("a missing host copy", dict(V=100, H=24, bounds=good, host=False)),
                     ("path 1 at 1024 -> 256", dict(V=1024, H=256, bounds=list(range(0, 1025, 4)), path=1))):
        rc, msg, untouched = call(**kw)
        assert rc == -1 and msg and untouched, (what, rc, msg, untouched)
