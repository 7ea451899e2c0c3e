"""log Z from the tempering ladder on the device (csrc/mdbn_temper.hip: mdbn_pt_run_z, TemperedChains.log_partition) against
the numpy twin (tests/_ptz_np.py) along the device's own trace, against mdbn_pt_run (recording the works moves nothing),
across the cuts of a run, and against exact partition functions.

Tolerances: a tapped work gets 4x the twin's own float32-versus-float64 gap on the same recorded states (the rule of
test_gpu_temper.py for the acceptance difference, which is d_fwd + d_rev); the accumulators get 1e-5 nats against the twin's
recurrence over the device's own tapped works (tests/test_ptz_twin.py derives it); the ground truth takes the AIS test's
criterion as it stands: |log Z^ - log Z| <= 4 standard errors and <= 0.05 nats.
Measured on MI355X: see DESIGN 3.7."""
import numpy as np
import pytest

import _ais_np as A
import _ptz_np as Z
import _temper_np as T
from _margins import check
from test_gpu_temper import SATURATED, _params, _saturated_params, _start, _layer, SEED, STREAM, STEP

pytestmark = pytest.mark.gpu

# The ladders of the ground truth: the tempering tests' own setting.  Smaller ones were tried on the CPU with the float64 twin
# (three seeds per layer): 32 x 16 x 600 and smaller meet the criterion on every seed too, but their jackknife
# standard error on the two-mode layer is 0.018 .. 0.042, so the fixed 0.05 nats would be a bound of 1.2 .. 2.8 sigma: a test
# that fails by chance.  At this setting it is 0.010 .. 0.012: 0.05 nats is beyond 4 sigma on every layer.
GT_M, GT_R, GT_SWEEPS, GT_BURN = 64, 16, 1200, 300

TRACE = [  # V, H, gauss, scale of W, M, R, sweeps, paths
    (100, 24, False, 0.3, 5, 8, 40, (1, 2)),
    (40, 14, True, 0.1, 5, 8, 40, (1, 2)),
    (784, 500, False, 0.05, 4, 8, 10, (2,)),
    (100, 24, False, 0.3, 5, 6, 12, (2,)),
]
STATE = ("v", "h", "rank", "accepted", "v_avg", "h_avg")


def _run(eng, W, c, b, bA, gauss, betas, h0, n, burn_in, path, spl=0, works=True, trace=False, state=None, zacc=None, sweep0=0, step=STEP,
         tap=True):
    """One engine call from ``h0`` (or the state ``state`` of an earlier call): dict of host arrays.  ``works``: through
    mdbn_pt_run_z with the accumulators and (``tap``) the tap of every work; otherwise mdbn_pt_run."""
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
    kw = {}
    if works:
        zacc = torch.from_numpy(new_works(M, R)).to(eng.device) if zacc is None else zacc
        kw = dict(zacc=zacc, trace_work=tap)
    out = eng.temper(dW, dc, db, dA, gauss, betas, v, h, rank, n, RngAddr(SEED, STREAM, step, 0, 0), burn_in=burn_in, sweep0=sweep0,
                     path=path, steps_per_launch=spl, trace=trace, **kw)
    eng.synchronize()
    names = ("accepted", "v_avg", "h_avg") + (("trace_v", "trace_h", "trace_swaps") if trace else ()) + (("works",) if works and tap else ())
    assert len(out) == len(names)
    d = {k: t.cpu().numpy() for k, t in zip(names, out)}
    d.update(v=v.cpu().numpy(), h=h.cpu().numpy(), rank=rank.cpu().numpy(), state=(v, h, rank))
    if works:
        d.update(zacc=zacc.cpu().numpy(), zacc_t=zacc)
    return d


@pytest.mark.parametrize("V,H,gauss,s,paths", SATURATED)
def test_works_along_the_device_trace_on_a_saturated_layer(hip_engine, V, H, gauss, s, paths):
    """M, R and sweeps of the first TRACE row with the biases on the ladder of tests/_saturated.py (test_gpu_temper.py)."""
    M, R, n = TRACE[0][4:7]
    _works_along_the_trace(hip_engine, "saturated ", _saturated_params(V, H, gauss, s), V, H, gauss, M, R, n, paths)


@pytest.mark.parametrize("V,H,gauss,s,M,R,n,paths", TRACE)
def test_works_along_the_device_trace(hip_engine, V, H, gauss, s, M, R, n, paths):
    _works_along_the_trace(hip_engine, "", _params(V, H, s), V, H, gauss, M, R, n, paths)


def _works_along_the_trace(hip_engine, what, params, V, H, gauss, M, R, n, paths):
    W, c, b, bA = params
    betas = np.linspace(0, 1, R).astype(np.float32)
    h0 = _start(M, R, H)
    burn = n // 4
    for path in paths:
        tag = "ptz %s%d->%d %s M=%d R=%d path %d" % (what, V, H, "GRBM" if gauss else "RBM", M, R, path)
        d = _run(hip_engine, W, c, b, bA, gauss, betas, h0, n, burn, path, trace=True)
        w = d["works"]
        assert w.shape == (n, M, R - 1, 2) and w.dtype == np.float64
        # NaN exactly where the pair was not tried
        tried = d["trace_swaps"][:, :, 1, :-1] >= 0
        np.testing.assert_array_equal(~np.isnan(w[..., 0]), tried)
        np.testing.assert_array_equal(~np.isnan(w[..., 1]), tried)
        assert tried.sum() == sum(M * len(range(t % 2, R - 1, 2)) for t in range(n))
        # every tapped work against the definition, along the device's recorded states
        w64 = Z.works_from_trace(W, c, b, bA, gauss, betas, d["trace_v"], d["trace_swaps"])
        w32 = Z.works_from_trace(W, c, b, bA, gauss, betas, d["trace_v"], d["trace_swaps"], dtype=np.float32)
        gap = float(np.nanmax(np.abs(w32 - w64)))
        worst = float(np.nanmax(np.abs(w - w64)))
        print("%s: float32-vs-float64 gap of the twin's works %.3e (bound %.3e); device works off by %.3e at most; |work| up to %.2f"
              % (tag, gap, 4 * gap, worst, np.nanmax(np.abs(w64))))
        check(tag + ": works", worst, 4 * gap, "ptz_work")
        # d_fwd + d_rev is the acceptance difference: a decision away from it would be a different swap rule
        logu = np.log(np.stack([A_uniform(M, R - 1, STEP + 3 * t + 1) for t in range(n)]).astype(np.float64))
        delta = w[..., 0] + w[..., 1]
        dec = d["trace_swaps"][:, :, 1, :-1]
        clear = tried & (np.abs(logu - np.where(tried, delta, 0.0)) > 8 * gap + 1e-5)
        np.testing.assert_array_equal((logu < delta)[clear], dec[clear] == 1)
        # the accumulators against the twin's recurrence over the device's own works
        want = Z.zacc_log_sums(Z.accumulate(w[burn:]))
        got = Z.zacc_log_sums(d["zacc"])
        off = float(np.abs(got - want).max())
        print("%s: accumulators against the recurrence over the tapped works: worst %.3e nats" % (tag, off))
        assert np.isfinite(got).all()
        check(tag + ": zacc", off, 1e-5, "ptz_zacc")
        np.testing.assert_array_equal(d["zacc"][..., 0::2], Z.accumulate(w[burn:])[..., 0::2])      # (the running maxima are works)


def A_uniform(rows, cols, step):
    from oracle import philox_np
    return philox_np.uniform(rows, cols, SEED, STREAM, step, 0)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("gauss", [False, True])
def test_outputs_are_those_of_pt_run(hip_engine, gauss, path):
    """With the same RNG address mdbn_pt_run_z returns v, h, rank, accepted, v_avg and h_avg bit-equal to mdbn_pt_run."""
    V, H, s = (40, 14, 0.1) if gauss else (100, 24, 0.3)
    M, R, n, burn = 6, 8, 20, 5
    W, c, b, bA = _params(V, H, s)
    betas = np.linspace(0, 1, R).astype(np.float32)
    h0 = _start(M, R, H)
    plain = _run(hip_engine, W, c, b, bA, gauss, betas, h0, n, burn, path, works=False)
    z = _run(hip_engine, W, c, b, bA, gauss, betas, h0, n, burn, path)
    assert plain["accepted"].sum() > 0 and np.isfinite(z["zacc"]).all() and (z["zacc"][..., 1::2] >= 1).all()
    bare = _run(hip_engine, W, c, b, bA, gauss, betas, h0, n, burn, path, tap=False)       # (on path 1 a kernel variant of its own)
    for k in STATE:
        np.testing.assert_array_equal(z[k], plain[k], err_msg=k)
        np.testing.assert_array_equal(bare[k], plain[k], err_msg=k + " without the tap")
    np.testing.assert_array_equal(bare["zacc"], z["zacc"])


@pytest.mark.parametrize("gauss", [False, True])
def test_cut_is_bit_invisible(hip_engine, gauss):
    """zacc (and the tap) at 7 and 1 sweeps per launch and at the default; run(12) + run(8) against run(20) on both paths."""
    V, H, s = (40, 14, 0.1) if gauss else (100, 24, 0.3)
    M, R, n, burn = 6, 8, 20, 5
    W, c, b, bA = _params(V, H, s)
    betas = np.linspace(0, 1, R).astype(np.float32)
    h0 = _start(M, R, H)
    whole = {p: _run(hip_engine, W, c, b, bA, gauss, betas, h0, n, burn, p) for p in (1, 2)}
    for spl in (7, 1):
        cut = _run(hip_engine, W, c, b, bA, gauss, betas, h0, n, burn, 1, spl=spl)
        for k in STATE + ("zacc", "works"):
            np.testing.assert_array_equal(cut[k], whole[1][k], err_msg="%s with %d sweeps per launch" % (k, spl))
    for path in (1, 2):
        one = _run(hip_engine, W, c, b, bA, gauss, betas, h0, 12, burn, path)
        two = _run(hip_engine, W, c, b, bA, gauss, betas, h0, 8, 0, path, state=one["state"], zacc=one["zacc_t"], sweep0=12, step=STEP + 36)
        np.testing.assert_array_equal(two["zacc"], whole[path]["zacc"], err_msg="path %d" % path)
        np.testing.assert_array_equal(np.concatenate([one["works"], two["works"]]), whole[path]["works"])
        for k in ("v", "h", "rank"):
            np.testing.assert_array_equal(two[k], whole[path][k], err_msg=k)


def _ground_truth_layer(name):
    if name == "two-mode":
        W, c, b, bA = T.two_mode_model(24, 12, 0)
        return W, c, b, bA, False
    V, H, s, gauss = dict(rbm=(24, 12, 0.5, False), grbm=(20, 10, 0.25, True))[name]
    return A.case_params(V, H, s, gauss) + (gauss,)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("name", ["rbm", "grbm", "two-mode"])
def test_ground_truth(hip_engine, name, path):
    """The 24->12 Bernoulli and 20->10 Gaussian layers of the AIS tests and the planted two-mode 24->12 layer of the tempering
    tests: 64 ladders of 16 temperatures from h = 0, 1200 sweeps (300 burn-in): |log Z^ - log Z| <= 4 SE and <= 0.05 nats.
    The bracket is printed, not asserted: fwd <= exact <= rev holds in expectation only."""
    W, c, b, bA, gauss = _ground_truth_layer(name)
    V, H = W.shape
    exact = A.brute_log_Z(W, c, b, gauss)
    rbm = _layer(hip_engine, V, H, gauss, W, c, b)
    chains = rbm.tempered_chains(GT_M, n_betas=GT_R, base_vbias=bA)
    r = chains.log_partition(GT_SWEEPS, GT_BURN, path=path)
    assert rbm._rng_step == 3 * GT_SWEEPS and chains.n_done == GT_SWEEPS
    print("ptz %s %d->%d path %d: log Z^ %.5f exact %.5f |err| %.5f SE %.5f; bracket fwd %+.5f rev %+.5f (against exact); "
          "swap acceptance %.2f .. %.2f" % (name, V, H, path, r.log_z, exact, abs(r.log_z - exact), r.stderr, r.log_z_fwd - exact,
                                            r.log_z_rev - exact, r.acceptance.min(), r.acceptance.max()))
    assert abs(r.log_z - exact) <= 4 * r.stderr, (r.log_z, exact, r.stderr)
    assert abs(r.log_z - exact) <= 0.05, (r.log_z, exact)


def test_ground_truth_bar_and_the_layer_methods(hip_engine):
    """Bennett's acceptance ratio from the device's tap on the two-mode layer (the same criterion), and RBM.log_partition /
    check_log_partition on the device: AIS and the tempering estimate side by side."""
    W, c, b, bA, gauss = _ground_truth_layer("two-mode")
    exact = A.brute_log_Z(W, c, b, gauss)
    rbm = _layer(hip_engine, 24, 12, gauss, W, c, b)
    r = rbm.tempered_chains(GT_M, n_betas=GT_R, base_vbias=bA).log_partition(GT_SWEEPS, GT_BURN, method="bar")
    print("ptz two-mode BAR: log Z^ %.5f exact %.5f |err| %.5f SE %.5f" % (r.log_z, exact, abs(r.log_z - exact), r.stderr))
    assert abs(r.log_z - exact) <= 4 * r.stderr and abs(r.log_z - exact) <= 0.05
    lz, se = rbm.log_partition(method="tempering", base_vbias=bA)
    assert abs(lz - exact) <= 4 * se and abs(lz - exact) <= 0.05
    both = rbm.check_log_partition(base_vbias=bA)
    print("two-mode 24->12: AIS %.5f +- %.5f, tempering %.5f +- %.5f, bracket (%.5f, %.5f), z = %.2f, exact %.5f"
          % (both["ais"], both["ais_stderr"], both["tempering"], both["tempering_stderr"], both["bracket"][0], both["bracket"][1],
             both["z"], exact))
    assert np.isfinite(both["z"]) and both["bracket"][0] != both["bracket"][1]
