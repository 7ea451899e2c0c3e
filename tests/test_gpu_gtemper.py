"""Parallel tempering of a layer with categorical visible units on the device (csrc/mdbn_temper.hip: mdbn_pt_run_grouped,
HipEngine.temper_grouped, RBM.tempered_chains / log_partition(method="tempering") / check_log_partition / training(tempering=)
with ``visible_groups``) against the numpy twin (tests/_gtemper_np.py) followed along the device's own trace, against
mdbn_pt_run / mdbn_pt_run_z where there are no groups, against exact marginals and log Z by enumeration, and the one-launch
path beside the general path.

Tolerances (tests/_gtemper_np.py ``check_forced``): the story of tests/test_gpu_temper.py -- a hidden or Bernoulli sample
equals the twin's own draw outside the near-tie mask (4e-6); a swap decision may differ from the float64 twin's only where
|log u - delta| < 4x the twin's float32-versus-float64 gap of delta, for at most 1 % of the attempts; v_avg / h_avg get 4x
their own float32-versus-float64 gap -- plus the group draws' of tests/test_gpu_gais.py: every recorded row one-hot per
group, a category that differs from the twin's own only with every boundary between the two within max(4e-6, 4 c_gap) of the
uniform, near ties capped by ``tie_cap``.  The cases, seeds and sizes are those tests/test_gtemper_twin.py passes with the
reference alone.  Measured on MI355X: DESIGN 3.18."""
import numpy as np
import pytest

import _gais_np as G
import _gtemper_np as GT
import _ptz_np as Z
import _softmax_np as sm
from _margins import check
from test_temper_twin import ladder_error

pytestmark = pytest.mark.gpu

SEED, STREAM, STEP = GT.SEED, GT.STREAM, GT.STEP
NAMES = ("accepted", "v_avg", "h_avg", "trace_v", "trace_h", "trace_swaps")


def _table(eng, bounds):
    from mdbn_amd.engine import GroupTable
    return GroupTable(eng, np.asarray(bounds, dtype=np.int32))


def _device(eng, W, c, b, bA, bounds, betas, h0, n, burn_in, path, spl=0, trace=True, sweep0=0, step=STEP, works=False,
            trace_work=False, zacc0=None, plain=False, state=None):
    """One call of temper_grouped (``plain``: of temper, ``bounds`` unused) -> dict of host arrays.  ``works``: with a fresh
    zacc (or ``zacc0``); ``state``: (v, h, rank) device tensors of an earlier call to continue."""
    import torch
    from mdbn_amd import RngAddr
    from mdbn_amd.engine import padded_ld
    from mdbn_amd.temper import new_works
    V, H = W.shape
    R = len(betas)
    M = h0.shape[0] // R
    dW, dc, db, dA = eng.to_device(W), eng.to_device(c), eng.to_device(b), eng.to_device(bA)
    if state is None:
        v, h = eng.alloc_matrix(M * R, V, padded_ld(V)), eng.alloc_matrix(M * R, H, dW.stride(0))
        h.copy_(torch.from_numpy(h0))
        rank = torch.arange(R, dtype=torch.int32).repeat(M, 1).to(eng.device).contiguous()
    else:
        v, h, rank = state
    zacc = None
    if works:
        zacc = torch.from_numpy(new_works(M, R) if zacc0 is None else zacc0).to(eng.device)
    kw = dict(burn_in=burn_in, sweep0=sweep0, path=path, steps_per_launch=spl, trace=trace)
    if works or trace_work:
        kw.update(zacc=zacc, trace_work=trace_work)
    rng = RngAddr(SEED, STREAM, step, 0, 0)
    eng.kernel_timing(True)
    try:
        if plain:
            out = eng.temper(dW, dc, db, dA, False, betas, v, h, rank, n, rng, **kw)
        else:
            out = eng.temper_grouped(dW, dc, db, dA, betas, v, h, rank, n, rng, _table(eng, bounds), **kw)
        eng.synchronize()
        n_gemm = len(eng.kernel_timing_detail())
    finally:
        eng.kernel_timing(False)
    if path == 1:
        assert n_gemm == 0, "path 1 went through %d GEMM launches: not the one-launch kernel" % n_gemm
    if path == 2:
        assert n_gemm >= 2 * n, "path 2 made %d GEMM launches for %d sweeps" % (n_gemm, n)
    names = NAMES[:3] + (NAMES[3:] if trace else ()) + (("trace_work",) if trace_work else ())
    d = {k: t.cpu().numpy() for k, t in zip(names, out)}
    d.update(v=v.cpu().numpy(), h=h.cpu().numpy(), rank=rank.cpu().numpy(), state=(v, h, rank))
    if zacc is not None:
        d["zacc"] = zacc.cpu().numpy()
    return d


def _same(a, b, keys, what):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (what, k))


def _parity(eng, tag, V, H, s, bounds, sat, M, R, n, paths):
    W, c, b, bA = GT.parity_params(V, H, s, sat)
    betas = np.linspace(0, 1, R).astype(np.float32)
    h0 = GT.start(M, R, H)
    burn = n // 4
    for path in paths:
        d = _device(eng, W, c, b, bA, bounds, betas, h0, n, burn, path)
        assert d["trace_v"].shape == (n, M * R, V) and d["trace_h"].shape == (n, M * R, H) and d["trace_swaps"].shape == (n, M, 2, R)
        assert all(np.isfinite(d[k]).all() for k in ("v_avg", "h_avg", "trace_v", "trace_h")) and d["accepted"].sum() > 0
        r64, r32 = GT.forced_pair(W, c, b, bA, bounds, betas, h0, n, burn, d)
        GT.check_forced("gpt forced %s %d->%d M=%d R=%d path %d" % (tag, V, H, M, R, path), d, r64, r32, bounds, check)


@pytest.mark.parametrize("tag,V,H,s,bounds,sat,paths", GT.PARITY)
def test_forced_parity(hip_engine, tag, V, H, s, bounds, sat, paths):
    _parity(hip_engine, tag, V, H, s, bounds, sat, GT.PARITY_M, GT.PARITY_R, GT.PARITY_N, paths)


def test_forced_parity_on_a_large_layer(hip_engine):
    tag, V, H, s, bounds, sat, paths = GT.LARGE
    _parity(hip_engine, tag, V, H, s, bounds, sat, 4, GT.PARITY_R, 10, paths)


def test_forced_parity_of_a_ragged_ladder(hip_engine):
    """R = 6 (a ladder's rows straddle the four-row Philox blocks) goes by shape to the general path."""
    tag, V, H, s, bounds, sat, _ = GT.PARITY[0]
    _parity(hip_engine, "ragged", V, H, s, bounds, sat, GT.PARITY_M, GT.RAGGED_R, 12, (0,))


# ---------------------------------------------------------------------------------- identities, bit for bit
CASE = GT.PARITY[0]
KEYS = NAMES + ("v", "h", "rank")


def _case(M=6, R=8):
    tag, V, H, s, bounds, sat, _ = CASE
    W, c, b, bA = GT.parity_params(V, H, s, sat)
    return W, c, b, bA, bounds, np.linspace(0, 1, R).astype(np.float32), GT.start(M, R, H)


@pytest.mark.parametrize("path", [1, 2])
def test_no_groups_is_the_plain_run_bit_for_bit(hip_engine, path):
    W, c, b, bA, _, betas, h0 = _case()
    V = W.shape[0]
    for works in (False, True):
        plain = _device(hip_engine, W, c, b, bA, None, betas, h0, 20, 5, path, plain=True, works=works, trace_work=works)
        empty = _device(hip_engine, W, c, b, bA, [V], betas, h0, 20, 5, path, works=works, trace_work=works)
        _same(plain, empty, KEYS + (("zacc", "trace_work") if works else ()), "n_groups = 0, path %d, works %s" % (path, works))
        assert plain["accepted"].sum() > 0


@pytest.mark.parametrize("path", [1, 2])
def test_recording_the_works_changes_no_other_output(hip_engine, path):
    W, c, b, bA, bounds, betas, h0 = _case()
    base = _device(hip_engine, W, c, b, bA, bounds, betas, h0, 20, 5, path)
    for works, tap in ((True, False), (False, True), (True, True)):
        got = _device(hip_engine, W, c, b, bA, bounds, betas, h0, 20, 5, path, works=works, trace_work=tap)
        _same(base, got, KEYS, "works %s, tap %s, path %d" % (works, tap, path))


def test_cut_is_bit_invisible(hip_engine):
    W, c, b, bA, bounds, betas, h0 = _case()
    whole = _device(hip_engine, W, c, b, bA, bounds, betas, h0, 20, 5, 1, works=True, trace_work=True)
    assert whole["accepted"].sum() > 0
    for spl in (7, 1):
        cut = _device(hip_engine, W, c, b, bA, bounds, betas, h0, 20, 5, 1, spl=spl, works=True, trace_work=True)
        _same(whole, cut, KEYS + ("zacc", "trace_work"), "%d sweeps per launch" % spl)


@pytest.mark.parametrize("path", [1, 2])
def test_two_runs_continue_one(hip_engine, path):
    """run(12) then run(8) with sweep0 = 12 and the RNG step moved on is run(20): state, rank map, counts and zacc."""
    W, c, b, bA, bounds, betas, h0 = _case()
    whole = _device(hip_engine, W, c, b, bA, bounds, betas, h0, 20, 0, path, trace=False, works=True)
    one = _device(hip_engine, W, c, b, bA, bounds, betas, h0, 12, 0, path, trace=False, works=True)
    two = _device(hip_engine, W, c, b, bA, bounds, betas, h0, 8, 0, path, trace=False, works=True, sweep0=12, step=STEP + 36,
                  zacc0=one["zacc"], state=one["state"])
    _same(whole, two, ("v", "h", "rank", "zacc"), "12 + 8 sweeps, path %d" % path)
    np.testing.assert_array_equal(one["accepted"] + two["accepted"], whole["accepted"])


def test_paths_agree_on_every_decision(hip_engine):
    """Path 1 and path 2 meet the same uniforms over 50 sweeps: every draw and every swap decision the same."""
    W, c, b, bA, bounds, betas, h0 = _case(M=8)
    n, burn = 50, 10
    out, gaps = {}, {}
    for p in (1, 2):
        out[p] = _device(hip_engine, W, c, b, bA, bounds, betas, h0, n, burn, p)
        r64, r32 = GT.forced_pair(W, c, b, bA, bounds, betas, h0, n, burn, out[p])
        GT.check_forced("gpt paths 100->24 n=50 path %d" % p, out[p], r64, r32, bounds, check)
        gaps[p] = max(np.abs(r32[k].astype(np.float64) - r64[k]).max() for k in ("v_avg", "h_avg"))
    _same(out[1], out[2], ("trace_swaps", "trace_v", "trace_h", "accepted", "rank"), "path 1 against path 2")
    for k in ("v_avg", "h_avg"):
        check("gpt paths 100->24 n=50: %s path 1 vs 2" % k, np.abs(out[1][k] - out[2][k]).max(), 4 * max(gaps.values()), "pt_" + k)


@pytest.mark.parametrize("path", [1, 2])
def test_deterministic(hip_engine, path):
    W, c, b, bA, bounds, betas, h0 = _case()
    a = _device(hip_engine, W, c, b, bA, bounds, betas, h0, 20, 5, path, works=True, trace_work=True)
    b2 = _device(hip_engine, W, c, b, bA, bounds, betas, h0, 20, 5, path, works=True, trace_work=True)
    _same(a, b2, KEYS + ("zacc", "trace_work"), "two runs, path %d" % path)


@pytest.mark.parametrize("path", [1, 2])
def test_the_tapped_works_are_the_works_of_the_trace(hip_engine, path):
    W, c, b, bA, bounds, betas, h0 = _case()
    n, burn = 20, 5
    d = _device(hip_engine, W, c, b, bA, bounds, betas, h0, n, burn, path, works=True, trace_work=True)
    w = d["trace_work"]
    tried = d["trace_swaps"][:, :, 1, :-1] >= 0
    np.testing.assert_array_equal(~np.isnan(w[..., 0]), tried)
    np.testing.assert_array_equal(~np.isnan(w[..., 1]), tried)
    w64 = Z.works_from_trace(W, c, b, bA, False, betas, d["trace_v"], d["trace_swaps"])
    w32 = Z.works_from_trace(W, c, b, bA, False, betas, d["trace_v"], d["trace_swaps"], dtype=np.float32)
    gap, worst = float(np.nanmax(np.abs(w32 - w64))), float(np.nanmax(np.abs(w - w64)))
    print("gpt works path %d: float32-vs-float64 gap of the twin's works %.3e (bound %.3e); device works off by %.3e at most"
          % (path, gap, 4 * gap, worst))
    check("gpt works path %d" % path, worst, 4 * gap, "ptz_work")
    # ... and zacc is the recurrence over the device's own works
    want = Z.accumulate(w[burn:])
    np.testing.assert_array_equal(d["zacc"][..., 0::2], want[..., 0::2])
    np.testing.assert_allclose(d["zacc"][..., 1::2], want[..., 1::2], rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------------- ground truth
def _layer(eng, W, c, b, bounds, seed=1):
    import mdbn_amd
    V, H = W.shape
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(seed),
                       engine=eng, visible_groups=bounds)
    rbm.W.set_value(np.asarray(W, dtype=np.float32)); rbm.hbias.set_value(np.asarray(c, dtype=np.float32))
    rbm.vbias.set_value(np.asarray(b, dtype=np.float32))
    return rbm


@pytest.fixture(scope="module")
def exact():
    """{case: (exact E[v], exact log Z)} of the float32 parameters the device holds, once."""
    out = {}
    for i, (tag, W, c, b, bA, bounds) in enumerate(GT.ground_truth_cases()):
        f = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
        out[i] = GT.exact_by_hidden(f(W), f(c), f(b), bounds)
    return out


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("case", [0, 1])
def test_ground_truth(hip_engine, exact, case, path):
    """64 ladders of 16 temperatures from h = 0, 1200 sweeps (300 burn-in): v_avg within max(4 SE, 0.01) of the exact marginals,
    the ladder's log Z within 4 standard errors and 0.05 nats of brute force."""
    tag, W, c, b, bA, bounds = GT.ground_truth_cases()[case]
    ev, lz = exact[case]
    rbm = _layer(hip_engine, W, c, b, bounds)
    chains = rbm.tempered_chains(GT.GT_M, n_betas=GT.GT_R, base_vbias=bA)
    v_avg, h_avg, acceptance = chains.run(GT.GT_SWEEPS, burn_in=GT.GT_BURN, path=path)
    assert rbm._rng_step == 3 * GT.GT_SWEEPS and chains.n_done == GT.GT_SWEEPS
    err, bound = ladder_error(v_avg.get_value(), ev)
    acc = np.asarray(acceptance.get_value())
    print("gpt %s path %d: v_avg error %.4f (bound %.4f), swap acceptance %.2f .. %.2f" % (tag, path, err, bound, acc.min(), acc.max()))
    assert err <= bound, (err, bound)
    v, _ = chains.samples()
    assert all((v.get_value()[:, lo:hi].sum(axis=1) == 1).all() for lo, hi in sm.spans(bounds))
    rbm2 = _layer(hip_engine, W, c, b, bounds)
    log_z, se = rbm2.log_partition(method="tempering", n_ladders=GT.GT_M, n_betas=GT.GT_R, n_sweeps=GT.GT_SWEEPS, burn_in=GT.GT_BURN,
                                   base_vbias=bA, path=path)
    r = _layer(hip_engine, W, c, b, bounds).tempered_chains(GT.GT_M, n_betas=GT.GT_R, base_vbias=bA).log_partition(
        GT.GT_SWEEPS, GT.GT_BURN, path=path)
    assert r.log_z == log_z and r.stderr == se            # (the same seed, the same run)
    print("gpt %s path %d: ladder log Z^ %.4f +- %.4f (bracket %.4f .. %.4f), exact %.4f" % (tag, path, log_z, se, r.log_z_fwd, r.log_z_rev, lz))
    assert se > 0 and abs(log_z - lz) <= 4 * se and abs(log_z - lz) <= 0.05, (log_z, se, lz)


def test_plain_chain_is_stuck_on_the_device(hip_engine, exact):
    """gibbs_vhv_chain from the same start (h = 0) stays in the light mode of the planted layer: it misses by more than 0.3."""
    tag, W, c, b, bA, bounds = GT.ground_truth_cases()[0]
    ev, _ = exact[0]
    rbm = _layer(hip_engine, W, c, b, bounds)
    v0 = rbm.sample_v_given_h(np.zeros((GT.GT_M, W.shape[1]), dtype=np.float32))[2]
    out = rbm.gibbs_vhv_chain(v0, GT.GT_SWEEPS)
    err = np.abs(np.asarray(out[4].get_value(), dtype=np.float64).mean(axis=0) - ev).max()
    print("plain grouped chain on the planted layer: error %.4f" % err)
    assert err > 0.3, err


def test_check_log_partition(hip_engine, exact):
    tag, W, c, b, bA, bounds = GT.ground_truth_cases()[1]
    _, lz = exact[1]
    rbm = _layer(hip_engine, W, c, b, bounds)
    out = rbm.check_log_partition(base_vbias=bA, n_chains=256, n_betas=500, n_ladders=32, n_ladder_betas=GT.GT_R, n_sweeps=400, burn_in=100)
    print("gpt check_log_partition %s: AIS %.4f +- %.4f, tempering %.4f +- %.4f, bracket (%.4f, %.4f), z %.2f, exact %.4f"
          % (tag, out["ais"], out["ais_stderr"], out["tempering"], out["tempering_stderr"], out["bracket"][0], out["bracket"][1],
             out["z"], lz))
    assert np.isfinite(out["ais"]) and np.isfinite(out["tempering"]) and np.isfinite(out["z"])
    assert out["bracket"] == (out["detail"].log_z_fwd, out["detail"].log_z_rev)


def test_tempered_pcd_is_the_hand_composed_sequence(hip_engine):
    """Three steps of training(persistent=True, tempering=8) on a 24 -> 12 grouped layer at batch 16 equal run(1),
    to_persistent, the grouped PCD step, from_persistent composed by hand, bit for bit."""
    import mdbn_amd
    eng = hip_engine
    B, R = 16, 8
    W, c, b, bA, bounds = GT.planted()
    V, H = W.shape
    data = sm.one_hot_data(np.random.RandomState(4), 3 * B, V, bounds)
    one, two = _layer(eng, 0.2 * W, c, b, bounds), _layer(eng, 0.2 * W, c, b, bounds)
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
    np.testing.assert_array_equal(one.tempered.v.cpu().numpy(), ladders.v.cpu().numpy())
    np.testing.assert_array_equal(one.tempered.rank.cpu().numpy(), ladders.rank.cpu().numpy())
    assert all((ladders.v.cpu().numpy()[:, lo:hi].sum(axis=1) == 1).all() for lo, hi in sm.spans(bounds))
    three = _layer(eng, 0.2 * W, c, b, bounds)
    np.random.seed(7)
    three.training(data, None, training_epochs=1, batch_size=B, learning_rate=0.05, k=1, persistent=True)
    assert not np.array_equal(three.W.get_value(), one.W.get_value())
