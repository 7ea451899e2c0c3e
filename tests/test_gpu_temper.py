"""Parallel tempering on the device (csrc/mdbn_temper.hip: mdbn_pt_run, RBM.tempered_chains) against the float64 numpy twin
(tests/_temper_np.py) followed along the device's own trace, against exact marginals of a planted two-mode layer, and the
one-launch path beside the general path.

Tolerances: samples equal the twin's own draw outside the project's near-tie mask (4e-6); Gaussian visible samples within
V_ATOL = 1e-4 (test_gpu_ais.py's derivation).  Swap decisions and the running means have NO fixed number: the twin is run twice
along the device's recorded states, in float64 (the acceptance difference as DEFINED: four evaluations of l) and in float32
(the device's regrouped arithmetic); the worst gap between the two is the float32 share of the error on exactly these inputs.
A decision may differ from the float64 twin's only where |log u - delta| < 4x that gap (at most 1 % of the attempts), and the
means get 4x their own gap (the rule of test_gpu_ais.py / test_gpu_clamp.py).
Measured on MI355X: see DESIGN 3.6."""
import numpy as np
import pytest

import _saturated as S
import _temper_np as T
from _margins import check
from test_temper_twin import M as GT_M, R as GT_R, N_SWEEPS, BURN_IN, ladder_error

pytestmark = pytest.mark.gpu

SEED, STREAM, STEP = 5, 3, 11
V_ATOL = 1e-4
EXCUSED_SHARE = 0.01

PARITY = [  # V, H, gauss, scale of W, M, R, sweeps, paths
    (100, 24, False, 0.3, 5, 8, 40, (1, 2)),
    (40, 14, True, 0.1, 5, 8, 40, (1, 2)),
    (784, 500, False, 0.05, 4, 8, 10, (2,)),
]
NAMES = ("accepted", "v_avg", "h_avg", "trace_v", "trace_h", "trace_swaps")


def _params(V, H, s, seed=3):
    rs = np.random.RandomState(seed)
    W = rs.normal(0, s, (V, H)).astype(np.float32)
    return W, rs.normal(0, 0.5, H).astype(np.float32), rs.normal(0, 0.5, V).astype(np.float32), rs.normal(0, 0.3, V).astype(np.float32)


def _start(M, R, H, seed=9):
    return (np.random.RandomState(seed).uniform(size=(M * R, H)) < 0.5).astype(np.float32)


def _device(eng, W, c, b, bA, gauss, betas, h0, n, burn_in, path, spl=0, trace=True, sweep0=0):
    import torch
    from mdbn_amd import RngAddr
    from mdbn_amd.engine import padded_ld
    V, H = W.shape
    R = len(betas)
    M = h0.shape[0] // R
    dW, dc, db, dA = eng.to_device(W), eng.to_device(c), eng.to_device(b), eng.to_device(bA)
    v, h = eng.alloc_matrix(M * R, V, padded_ld(V)), eng.alloc_matrix(M * R, H, dW.stride(0))
    h.copy_(torch.from_numpy(h0))
    rank = torch.arange(R, dtype=torch.int32).repeat(M, 1).to(eng.device).contiguous()
    eng.kernel_timing(True)
    try:
        out = eng.temper(dW, dc, db, dA, gauss, betas, v, h, rank, n, RngAddr(SEED, STREAM, STEP, 0, 0), burn_in=burn_in,
                         sweep0=sweep0, path=path, steps_per_launch=spl, trace=trace)
        eng.synchronize()
        n_gemm = len(eng.kernel_timing_detail())
    finally:
        eng.kernel_timing(False)
    if path == 1:
        assert n_gemm == 0, "path 1 went through %d GEMM launches: not the one-launch kernel" % n_gemm
    if path == 2:
        assert n_gemm >= 2 * n, "path 2 made %d GEMM launches for %d sweeps" % (n_gemm, n)
    d = {k: t.cpu().numpy() for k, t in zip(NAMES, out)}
    d.update(v=v.cpu().numpy(), h=h.cpu().numpy(), rank=rank.cpu().numpy())
    return d


def _forced(W, c, b, bA, gauss, betas, h0, n, burn_in, d, sweep0=0):
    kw = dict(forced=(d["trace_v"], d["trace_h"], d["trace_swaps"]), sweep0=sweep0)
    r64 = T.pt_twin(W, c, b, bA, gauss, betas, h0, n, burn_in, SEED, STREAM, STEP, **kw)
    r32 = T.pt_twin(W, c, b, bA, gauss, betas, h0, n, burn_in, SEED, STREAM, STEP, dtype=np.float32, **kw)
    return r64, r32


def _check_forced(tag, d, r64, r32):
    gap_d = float(np.abs(r32["delta"] - r64["delta"]).max())
    gap_v = float(np.abs(r32["v_avg"].astype(np.float64) - r64["v_avg"]).max())
    gap_h = float(np.abs(r32["h_avg"].astype(np.float64) - r64["h_avg"]).max())
    dev_v, dev_h = float(np.abs(d["v_avg"] - r64["v_avg"]).max()), float(np.abs(d["h_avg"] - r64["h_avg"]).max())
    own = r64["logu"] < r64["delta"]
    differ = own != r64["decided"]
    band = np.abs(r64["logu"] - r64["delta"]) < 4 * gap_d
    n_att = r64["decided"].size
    print("%s: float32-vs-float64 gap of the twin delta %.3e v_avg %.3e h_avg %.3e; device v_avg %.3e h_avg %.3e; swap attempts %d, "
          "accepted %d, inside the band %d, excused decisions %d, decisions off outside the band %d; draws %d, near ties %d, "
          "flips outside the mask %d, Gaussian sample diff %.3e"
          % (tag, gap_d, gap_v, gap_h, dev_v, dev_h, n_att, int(r64["decided"].sum()), int(band.sum()), int((differ & band).sum()),
             int((differ & ~band).sum()), r64["n_draws"], r64["n_ties"], r64["flips_outside_mask"], r64["max_v_diff"]))
    assert r64["flips_outside_mask"] == 0, "%s: %d samples differ from the twin's own draw away from a tie" % (tag, r64["flips_outside_mask"])
    assert r64["max_v_diff"] <= V_ATOL, "%s: Gaussian visible sample off by %.3e" % (tag, r64["max_v_diff"])
    assert not (differ & ~band).any(), "%s: %d swap decisions differ from the twin's away from a tie" % (tag, (differ & ~band).sum())
    assert (differ & band).sum() <= EXCUSED_SHARE * n_att, (tag, int((differ & band).sum()), n_att)
    # the trace, the state and the counts tell one story
    np.testing.assert_array_equal(d["v"], d["trace_v"][-1])
    np.testing.assert_array_equal(d["h"], d["trace_h"][-1])
    np.testing.assert_array_equal(d["rank"], d["trace_swaps"][-1, :, 0, :])
    np.testing.assert_array_equal(d["accepted"], (d["trace_swaps"][:, :, 1, :-1] == 1).sum(axis=(0, 1)))
    np.testing.assert_array_equal(d["trace_swaps"], r64["trace_swaps"])
    assert (np.sort(d["rank"], axis=1) == np.arange(d["rank"].shape[1])[None]).all(), "the rank map is no permutation"
    check(tag + ": v_avg", dev_v, 4 * gap_v, "pt_v_avg")
    check(tag + ": h_avg", dev_h, 4 * gap_h, "pt_h_avg")


@pytest.mark.parametrize("V,H,gauss,s,M,R,n,paths", PARITY)
def test_device_against_twin(hip_engine, V, H, gauss, s, M, R, n, paths):
    W, c, b, bA = _params(V, H, s)
    betas = np.linspace(0, 1, R).astype(np.float32)
    h0 = _start(M, R, H)
    burn = n // 4
    for path in paths:
        d = _device(hip_engine, W, c, b, bA, gauss, betas, h0, n, burn, path)
        assert d["trace_v"].shape == (n, M * R, V) and d["trace_h"].shape == (n, M * R, H) and d["trace_swaps"].shape == (n, M, 2, R)
        assert all(np.isfinite(d[k]).all() for k in ("v_avg", "h_avg", "trace_v", "trace_h"))
        tries = (d["trace_swaps"][:, :, 1, :] >= 0).sum()
        assert tries == sum(M * len(range(t % 2, R - 1, 2)) for t in range(n)) and d["accepted"].sum() > 0
        r64, r32 = _forced(W, c, b, bA, gauss, betas, h0, n, burn, d)
        _check_forced("pt forced %d->%d %s M=%d R=%d path %d" % (V, H, "GRBM" if gauss else "RBM", M, R, path), d, r64, r32)


# 100 -> 24 RBM on both paths and 400 -> 40 GRBM (the general path) at the M, R and sweeps of the first PARITY row
SATURATED = [(100, 24, False, 0.3, (1, 2)), (400, 40, True, 0.05, (2,))]


def _saturated_params(V, H, gauss, s):
    """`_params` with c and (Bernoulli) b on the ladder of tests/_saturated.py: pre-activations from -120 to 120 at beta = 1."""
    W, _, b, bA = _params(V, H, s)
    c, b = S.sampler_biases(V, H, gauss, b)
    return W, c, b, bA


@pytest.mark.parametrize("V,H,gauss,s,paths", SATURATED)
def test_device_against_twin_on_a_saturated_layer(hip_engine, V, H, gauss, s, paths):
    M, R, n = PARITY[0][4:7]
    W, c, b, bA = _saturated_params(V, H, gauss, s)
    betas = np.linspace(0, 1, R).astype(np.float32)
    h0 = _start(M, R, H)
    burn = n // 4
    for path in paths:
        d = _device(hip_engine, W, c, b, bA, gauss, betas, h0, n, burn, path)
        assert all(np.isfinite(d[k]).all() for k in ("v_avg", "h_avg", "trace_v", "trace_h"))
        r64, r32 = _forced(W, c, b, bA, gauss, betas, h0, n, burn, d)
        _check_forced("pt forced saturated %d->%d %s M=%d R=%d path %d" % (V, H, "GRBM" if gauss else "RBM", M, R, path), d, r64, r32)


def test_path_1_refused_where_it_does_not_fit(hip_engine):
    import mdbn_amd
    W, c, b, bA = _params(784, 500, 0.05)
    with pytest.raises(mdbn_amd.MdbnError, match="LDS-resident"):
        _device(hip_engine, W, c, b, bA, False, np.linspace(0, 1, 8), _start(2, 8, 500), 2, 0, 1)
    W, c, b, bA = _params(100, 24, 0.3)
    with pytest.raises(mdbn_amd.MdbnError, match="multiple of 4"):
        _device(hip_engine, W, c, b, bA, False, np.linspace(0, 1, 6), _start(2, 6, 24), 2, 0, 1)


def test_ragged_ladder_on_the_general_path(hip_engine):
    """R = 6 (no multiple of the four-row Philox block: a ladder's rows straddle blocks) goes by shape to the general path."""
    V, H, M, R, n = 100, 24, 5, 6, 12
    W, c, b, bA = _params(V, H, 0.3)
    betas = np.linspace(0, 1, R).astype(np.float32)
    h0 = _start(M, R, H)
    d = _device(hip_engine, W, c, b, bA, False, betas, h0, n, 3, 0)
    r64, r32 = _forced(W, c, b, bA, False, betas, h0, n, 3, d)
    _check_forced("pt forced 100->24 RBM M=5 R=6 path 0", d, r64, r32)


@pytest.mark.parametrize("V,H,gauss,M,one_launch", [(100, 24, False, 512, True), (100, 24, False, 8, False), (400, 40, True, 512, False)])
def test_path_0_follows_the_measurement(hip_engine, V, H, gauss, M, one_launch):
    """path = 0 takes the one-launch kernel where it was measured to win (two workgroups per CU and >= 512 ladders: DESIGN 3.6)
    and the general path elsewhere -- also at 400->40, which fits but does not win."""
    R, n = 8, 4
    W, c, b, bA = _params(V, H, 0.1)
    betas = np.linspace(0, 1, R).astype(np.float32)
    h0 = _start(M, R, H)
    got = _device(hip_engine, W, c, b, bA, gauss, betas, h0, n, 1, 0, trace=False)
    want = _device(hip_engine, W, c, b, bA, gauss, betas, h0, n, 1, 1 if one_launch else 2, trace=False)
    for k in ("v", "h", "rank", "accepted", "v_avg", "h_avg"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_paths_agree(hip_engine):
    """Path 1 and path 2 meet the same uniforms: identical traces except where a ladder met a near tie (such a ladder is then a
    different, equally valid one: the twin vouches for each path).  The allowance of test_gpu_clamp.py::test_paths_agree."""
    V, H, M, R, n, burn = 100, 24, 64, 8, 50, 10
    W, c, b, bA = _params(V, H, 0.3)
    betas = np.linspace(0, 1, R).astype(np.float32)
    h0 = _start(M, R, H)
    out, gaps = {}, {}
    for p in (1, 2):
        out[p] = _device(hip_engine, W, c, b, bA, False, betas, h0, n, burn, p)
        r64, r32 = _forced(W, c, b, bA, False, betas, h0, n, burn, out[p])
        _check_forced("pt paths 100->24 n=50 path %d" % p, out[p], r64, r32)
        gaps[p] = max(np.abs(r32[k].astype(np.float64) - r64[k]).max() for k in ("v_avg", "h_avg"))
    same = np.ones(M, dtype=bool)
    for k, width in (("trace_v", V), ("trace_h", H)):
        same &= (out[1][k] == out[2][k]).reshape(n, M, R * width).all(axis=(0, 2))
    same &= (out[1]["trace_swaps"] == out[2]["trace_swaps"]).all(axis=(0, 2, 3))
    assert same.sum() >= M - 2, "%d of %d ladders differ between the paths" % (M - same.sum(), M)
    for k in ("v_avg", "h_avg"):
        check("pt paths 100->24 n=50: %s path 1 vs 2" % k, np.abs(out[1][k] - out[2][k])[same].max(), 4 * max(gaps.values()), "pt_" + k)


@pytest.mark.parametrize("gauss", [False, True])
def test_cut_is_bit_invisible(hip_engine, gauss):
    V, H, s = (40, 14, 0.1) if gauss else (100, 24, 0.3)
    M, R, n, burn = 6, 8, 20, 5
    W, c, b, bA = _params(V, H, s)
    betas = np.linspace(0, 1, R).astype(np.float32)
    h0 = _start(M, R, H)
    whole = _device(hip_engine, W, c, b, bA, gauss, betas, h0, n, burn, 1)
    assert whole["accepted"].sum() > 0
    for spl in (7, 1):
        cut = _device(hip_engine, W, c, b, bA, gauss, betas, h0, n, burn, 1, spl=spl)
        for k in NAMES + ("v", "h", "rank"):
            np.testing.assert_array_equal(cut[k], whole[k], err_msg="%s with %d sweeps per launch" % (k, spl))


@pytest.mark.parametrize("path", [1, 2])
def test_two_runs_continue_one(hip_engine, path):
    """run(12) then run(8) with sweep0 = 12 and the RNG step moved on is run(20): state, rank map and counts (the sums restart)."""
    import torch
    from mdbn_amd import RngAddr
    from mdbn_amd.engine import padded_ld
    eng = hip_engine
    V, H, M, R = 100, 24, 6, 8
    W, c, b, bA = _params(V, H, 0.3)
    betas = np.linspace(0, 1, R).astype(np.float32)
    h0 = _start(M, R, H)
    whole = _device(eng, W, c, b, bA, False, betas, h0, 20, 0, path, trace=False)
    dW, dc, db, dA = eng.to_device(W), eng.to_device(c), eng.to_device(b), eng.to_device(bA)
    v, h = eng.alloc_matrix(M * R, V, padded_ld(V)), eng.alloc_matrix(M * R, H, dW.stride(0))
    h.copy_(torch.from_numpy(h0))
    rank = torch.arange(R, dtype=torch.int32).repeat(M, 1).to(eng.device).contiguous()
    a1 = eng.temper(dW, dc, db, dA, False, betas, v, h, rank, 12, RngAddr(SEED, STREAM, STEP, 0, 0), path=path)[0].cpu().numpy()
    a2 = eng.temper(dW, dc, db, dA, False, betas, v, h, rank, 8, RngAddr(SEED, STREAM, STEP + 36, 0, 0), sweep0=12, path=path)[0].cpu().numpy()
    np.testing.assert_array_equal(v.cpu().numpy(), whole["v"])
    np.testing.assert_array_equal(h.cpu().numpy(), whole["h"])
    np.testing.assert_array_equal(rank.cpu().numpy(), whole["rank"])
    np.testing.assert_array_equal(a1 + a2, whole["accepted"])


def _layer(eng, V, H, gauss, W, c, b, seed=1):
    import mdbn_amd
    kw = dict(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(seed), engine=eng)
    rbm = mdbn_amd.GRBM(**kw) if gauss else mdbn_amd.RBM(**kw)
    rbm.W.set_value(np.asarray(W, dtype=np.float32)); rbm.hbias.set_value(np.asarray(c, dtype=np.float32))
    rbm.vbias.set_value(np.asarray(b, dtype=np.float32))
    return rbm


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("V,H,gauss", [(24, 12, False), (20, 10, True)])
def test_ground_truth(hip_engine, V, H, gauss, path):
    """Case (a) of tests/test_temper_twin.py on the device, and a Gaussian two-mode layer built the same way: 64 ladders of 16
    temperatures from h = 0, 1200 sweeps (300 burn-in); max_i |mean over ladders of v_avg - exact| <= max(4 SE, 0.01)."""
    W, c, b, bA = T.two_mode_model(V, H, 0, gauss)
    exact = T.exact_visible_mean(W, c, b, gauss)
    rbm = _layer(hip_engine, V, H, gauss, W, c, b)
    chains = rbm.tempered_chains(GT_M, n_betas=GT_R, base_vbias=bA)
    v_avg, h_avg, acceptance = chains.run(N_SWEEPS, burn_in=BURN_IN, path=path)
    assert rbm._rng_step == 3 * N_SWEEPS and chains.n_done == N_SWEEPS
    err, bound = ladder_error(v_avg.get_value(), exact)
    acc = np.asarray(acceptance.get_value())
    print("pt two-mode %d->%d %s path %d: error %.4f (bound %.4f), swap acceptance %.2f .. %.2f"
          % (V, H, "GRBM" if gauss else "RBM", path, err, bound, acc.min(), acc.max()))
    assert err <= bound, (err, bound)
    v, h = chains.samples()
    assert v.get_value().shape == (GT_M, V) and h.get_value().shape == (GT_M, H)


def test_plain_chain_is_stuck_on_the_device(hip_engine):
    """gibbs_vhv_chain from the same start (h = 0) never reaches the heavy mode of the two-mode layer: it misses by more than 0.3."""
    W, c, b, bA = T.two_mode_model(24, 12, 0)
    exact = T.exact_visible_mean(W, c, b)
    rbm = _layer(hip_engine, 24, 12, False, W, c, b)
    v0 = rbm.sample_v_given_h(np.zeros((GT_M, 12), dtype=np.float32))[2]
    out = rbm.gibbs_vhv_chain(v0, N_SWEEPS)
    err = np.abs(np.asarray(out[4].get_value(), dtype=np.float64).mean(axis=0) - exact).max()
    print("plain chain on the two-mode layer: error %.4f" % err)
    assert err > 0.3, err


def test_sample_tempered(hip_engine):
    W, c, b, bA = T.two_mode_model(24, 12, 0)
    rbm = _layer(hip_engine, 24, 12, False, W, c, b)
    v, h, v_avg, h_avg, acceptance = rbm.sample_tempered(32, n_sweeps=60, burn_in=20, n_betas=8, base_vbias=bA)
    assert v.shape == (32, 24) and h.shape == (32, 12) and v_avg.shape == (32, 24) and h_avg.shape == (32, 12) and acceptance.shape == (7,)
    assert set(np.unique(v)) <= {0.0, 1.0} and ((acceptance > 0) & (acceptance <= 1)).all() and rbm._rng_step == 180


def test_persistent_round_trip_and_tempered_pcd(hip_engine):
    """to_persistent / from_persistent copy the beta = 1 hidden rows exactly, and three steps of RBM.training(persistent=True,
    tempering=8) equal the hand-composed sequence run(1), to_persistent, PCD step, from_persistent bit for bit."""
    import torch
    import mdbn_amd
    eng = hip_engine
    V, H, B, R = 24, 12, 16, 8
    W, c, b, bA = T.two_mode_model(V, H, 0)
    data = (np.random.RandomState(4).uniform(size=(3 * B, V)) < 0.5).astype(np.float32)

    # the copies
    rbm = _layer(eng, V, H, False, 0.2 * W, c, b)
    chains = rbm.tempered_chains(B, n_betas=R, start_h=_start(B, R, H))
    chains.run(5)
    rank = chains.rank.cpu().numpy()
    top = np.arange(B) * R + np.argmax(rank == R - 1, axis=1)
    buf = mdbn_amd.shared(np.zeros((B, H), dtype=np.float32), engine=eng)
    chains.to_persistent(buf)
    np.testing.assert_array_equal(buf.get_value(), chains.h.cpu().numpy()[top])
    new = _start(B, 1, H, seed=12)
    before = chains.h.cpu().numpy().copy()
    chains.from_persistent(mdbn_amd.shared(new, engine=eng))
    after = chains.h.cpu().numpy()
    np.testing.assert_array_equal(after[top], new)
    rest = np.setdiff1d(np.arange(B * R), top)
    np.testing.assert_array_equal(after[rest], before[rest])

    # PT-PCD: the trainer against the sequence composed by hand
    one, two = _layer(eng, V, H, False, 0.2 * W, c, b), _layer(eng, V, H, False, 0.2 * W, c, b)
    np.random.seed(7)
    one.training(data, None, training_epochs=1, batch_size=B, learning_rate=0.05, k=1, persistent=True, tempering=R)
    np.random.seed(7)
    _, batches = mdbn_amd.get_minibatches_idx(3 * B, B, shuffle=True)
    persistent = mdbn_amd.shared(np.zeros((B, H), dtype=np.float32), engine=eng)
    cost, updates = two.get_cost_updates(lr=0.05, k=1, batch_size=B, persistent=persistent)
    ladders = two.tempered_chains(B, n_betas=R)
    step = mdbn_amd.function(updates, mdbn_amd.shared(data, engine=eng))
    for idx in batches:
        ladders.run(1)
        ladders.to_persistent(updates.persistent)
        step(eng.index_tensor(idx), 0.0)
        ladders.from_persistent(updates.persistent)
    step.flush()
    assert one._rng_step == two._rng_step and one.tempered.n_done == 3
    for name in ("W", "hbias", "vbias"):
        np.testing.assert_array_equal(getattr(one, name).get_value(), getattr(two, name).get_value(), err_msg=name)
    np.testing.assert_array_equal(one.tempered.h.cpu().numpy(), ladders.h.cpu().numpy())
    np.testing.assert_array_equal(one.tempered.rank.cpu().numpy(), ladders.rank.cpu().numpy())
    # and tempering=None is the PCD trainer as it was
    three, four = _layer(eng, V, H, False, 0.2 * W, c, b), _layer(eng, V, H, False, 0.2 * W, c, b)
    np.random.seed(7)
    three.training(data, None, training_epochs=1, batch_size=B, learning_rate=0.05, k=1, persistent=True)
    np.random.seed(7)
    four.training(data, None, training_epochs=1, batch_size=B, learning_rate=0.05, k=1, persistent=True, tempering=None)
    np.testing.assert_array_equal(three.W.get_value(), four.W.get_value())
    assert not np.array_equal(three.W.get_value(), one.W.get_value())
