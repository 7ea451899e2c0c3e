"""Clamped annealed importance sampling of a layer with categorical visible units on the device (csrc/mdbn_ais.hip:
mdbn_ais_cond_run_grouped, HipEngine.ais_conditional_grouped, RBM.conditional_log_partition / conditional_log_likelihood with
``visible_groups``) against the numpy twin (tests/_gcais_np.py) teacher-forced along the device's own samples, against
mdbn_ais_cond_run (no groups) and mdbn_ais_run_grouped (no held unit) bit for bit, against the closed form (every unit held),
against brute-force conditional partition functions and the exact group posterior, and the one-launch path beside the general
path.

Tolerance of the per-chain log weights: the rule of tests/test_gpu_ais.py -- 4x the twin's own float32-versus-float64 gap on
the recorded samples, through tests/_margins.py as ``cais_logw``.  A draw of a free unit that differs from the twin's own must
be a near tie: |u - p| < _ais_np.TIE for a hidden or Bernoulli draw; for a group every boundary C_c between the two
categories within max(TIE, 4 c_gap) of the uniform, c_gap the twin's float32-versus-float64 gap of C_c on the same inputs.
Near ties are capped by 3 + E + 4 sqrt(E), E the expected count from the shape (_gais_np.tie_cap)."""
import ctypes as C

import numpy as np
import pytest

import _gais_np as G
import _gcais_np as X
import _softmax_np as sm
from _margins import check

pytestmark = pytest.mark.gpu

SEED, STREAM, STEP = X.SEED, X.STREAM, X.STEP


def _table(eng, bounds):
    from mdbn_amd.engine import GroupTable
    return GroupTable(eng, np.asarray(bounds, dtype=np.int32))


def _timed(eng, K, path, call):
    """``call()`` with the GEMM launches counted: none on the one-launch path, at least 2K - 1 on the general path."""
    eng.kernel_timing(True)
    try:
        out = call()
        eng.synchronize()
        n_gemm = len(eng.kernel_timing_detail())
    finally:
        eng.kernel_timing(False)
    if path == 1:
        assert n_gemm == 0, "path 1 went through %d GEMM launches: not the one-launch kernel" % n_gemm
    if path == 2:
        assert n_gemm >= 2 * K - 1, "path 2 made %d GEMM launches for %d temperatures" % (n_gemm, K)
    return out


def _device(eng, W, c, b, bA, bounds, betas, obs, mask, Cn, path, trace=True, step=STEP, state=False, expect=None):
    from mdbn_amd import RngAddr
    dW, dc, db = eng.to_device(W), eng.to_device(c), eng.to_device(b)
    return _timed(eng, len(betas) - 1, path if expect is None else expect,
                  lambda: eng.ais_conditional_grouped(dW, dc, db, bA, betas, obs, mask, Cn, RngAddr(SEED, STREAM, step, 0, 0),
                                                      _table(eng, bounds), path=path, trace=trace, state=state))


def _forced(W, c, b, bA, bounds, betas, obs, mask, Cn, th, tv, step=STEP):
    r64 = X.gcais_twin(W, c, b, bA, bounds, betas, obs, mask, Cn, SEED, STREAM, step, forced=(th, tv))
    r32 = X.gcais_twin(W, c, b, bA, bounds, betas, obs, mask, Cn, SEED, STREAM, step, dtype=np.float32, forced=(th, tv))
    return r64, float(np.abs(r32["logw"] - r64["logw"]).max())


def _all_held_bound(W, c, b, bA, bounds, betas, rows):
    """For rows with every unit held (nothing is random, log w = log Z_r - log Z_A,r): the float64 twin's log w [R] and 4x its
    float32-versus-float64 gap, the device's allowance for its own summation order.  The gap of ONE row is one draw of the
    rounding error of a K-term float32 sum (it came out anywhere from 1e-8 to 7e-7 over the rows of one case), so the bound is
    the largest gap over ALL the rows handed in, as tests/test_gpu_cais.py::test_every_column_held takes it over its N rows --
    pass every row of the case, not only the ones that are checked."""
    mask = np.ones((1, rows.shape[1]), dtype=np.float32)
    r64 = X.gcais_twin(W, c, b, bA, bounds, betas, rows, mask, 1, SEED, STREAM, STEP, gaps=False)
    r32 = X.gcais_twin(W, c, b, bA, bounds, betas, rows, mask, 1, SEED, STREAM, STEP, dtype=np.float32, gaps=False)
    return r64["logw"][:, 0], 4.0 * float(np.abs(r32["logw"] - r64["logw"]).max())


def _check_forced(tag, logw, r64, gap, obs, mask, bounds, Cn, tv):
    width, near, cap = X.near_ties(r64)
    print("%s: float32-vs-float64 gap of the twin %.3e, bound %.3e, device %.3e; C_c gap %.3e, mask %.3e, worst boundary miss %.3e; "
          "draws %d + %d group draws, near ties %d (cap %d), flips %d + %d"
          % (tag, gap, 4 * gap, np.abs(logw - r64["logw"]).max(), r64["c_gap"], width, r64["group_miss"], r64["n_draws"],
             r64["group_draws"], near, cap, r64["n_flips"], r64["group_flips"]))
    N, V = obs.shape
    held = X.chain_held(mask, bounds, N, V, Cn)
    want = np.repeat(obs, Cn, axis=0)
    assert (tv[:, held] == want[held][None, :]).all(), "%s: a held entry of trace_v is not its observed value" % tag
    for lo, hi in sm.spans(bounds):
        free = ~held[:, lo]
        assert (tv[:, free, lo:hi].sum(axis=2) == 1.0).all() and np.isin(tv[:, free, lo:hi], (0.0, 1.0)).all(), (tag, lo, hi)
    assert r64["flips_outside_mask"] == 0, "%s: %d samples differ from the twin's own draw away from a tie" % (tag, r64["flips_outside_mask"])
    assert r64["group_miss"] < width, "%s: a category differs from the twin's %.3e from a boundary (mask %.3e)" % (tag, r64["group_miss"], width)
    assert near <= cap, (tag, near, cap)
    check(tag + ": log w per chain", np.abs(logw - r64["logw"]).max(), 4 * gap, "cais_logw")


@pytest.mark.parametrize("N,Cn", X.SHAPES)
@pytest.mark.parametrize("V,H,s,bounds,paths", X.PARITY)
def test_forced_parity(hip_engine, V, H, s, bounds, paths, N, Cn):
    W, c, b, bA = G.parity_params(V, H, s)
    betas = np.linspace(0, 1, 9)
    for path in paths:
        for mask_rows in (N, 1) if (N, Cn) == X.SHAPES[1] else (N,):     # per-row unit masks, and once one row for all
            obs, mask = X.clamp_inputs(N, V, bounds, mask_rows)
            assert mask.shape == (mask_rows, V)
            logw, th, tv = _device(hip_engine, W, c, b, bA, bounds, betas, obs, mask, Cn, path)
            assert logw.shape == (N, Cn) and th.shape == (7, N * Cn, H) and tv.shape == (8, N * Cn, V) and np.isfinite(logw).all()
            r64, gap = _forced(W, c, b, bA, bounds, betas, obs, mask, Cn, th, tv)
            _check_forced("GCAIS forced %d->%d N=%d C=%d mask rows %d path %d" % (V, H, N, Cn, mask_rows, path), logw, r64, gap,
                          obs, mask, bounds, Cn, tv)


def test_forced_parity_on_a_saturated_layer(hip_engine):
    """100 -> 24 in groups of 5 with the biases on the ladder of tests/_saturated.py (tests/test_gpu_ais.py's
    ``_saturated_params``): the same bound rule, masks and cap."""
    from test_gpu_ais import _saturated_params
    V, H, s, bounds, paths = X.PARITY[0]
    N, Cn = X.SHAPES[0]
    W, c, b, bA = _saturated_params(V, H, False, s)
    betas = np.linspace(0, 1, 9)
    obs, mask = X.clamp_inputs(N, V, bounds, N)
    for path in paths:
        logw, th, tv = _device(hip_engine, W, c, b, bA, bounds, betas, obs, mask, Cn, path)
        assert np.isfinite(logw).all()
        r64, gap = _forced(W, c, b, bA, bounds, betas, obs, mask, Cn, th, tv)
        _check_forced("GCAIS forced saturated %d->%d path %d" % (V, H, path), logw, r64, gap, obs, mask, bounds, Cn, tv)


@pytest.mark.parametrize("path", [1, 2])
def test_no_groups_is_the_plain_clamped_run_bit_for_bit(hip_engine, path):
    """n_groups = 0: mdbn_ais_cond_run(gauss = 0) -- log w, the final state and both traces."""
    from mdbn_amd import RngAddr
    eng = hip_engine
    V, H = 100, 24
    W, c, b, bA = G.parity_params(V, H, 0.3)
    betas = np.linspace(0, 1, 21)
    for (N, Cn), mask_rows in ((X.SHAPES[1], 7), (X.SHAPES[1], 1), ((11, 2), 11)):
        rs = np.random.RandomState(11)
        obs, mask = rs.uniform(size=(N, V)).astype(np.float32), (rs.uniform(size=(mask_rows, V)) < 0.5).astype(np.float32)
        got = _device(eng, W, c, b, bA, [V], betas, obs, mask, Cn, path, state=True)
        want = eng.ais_conditional(eng.to_device(W), eng.to_device(c), eng.to_device(b), bA, False, betas, obs, mask, Cn,
                                   RngAddr(SEED, STREAM, STEP, 0, 0), path=path, trace=True, state=True)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("V,H,s,bounds", [X.PARITY[0][:4], X.PARITY[1][:4]])
def test_no_held_unit_is_the_free_grouped_run_bit_for_bit(hip_engine, V, H, s, bounds, path):
    """A mask of zeros: mdbn_ais_run_grouped with M = N C chains -- log w, the final state and both traces."""
    from mdbn_amd import RngAddr
    eng = hip_engine
    W, c, b, bA = G.parity_params(V, H, s)
    betas = np.linspace(0, 1, 21)
    N, Cn = 11, 2
    for mask_rows in (N, 1):
        obs, _ = X.clamp_inputs(N, V, bounds, N)
        logw, th, tv, state = _device(eng, W, c, b, bA, bounds, betas, obs, np.zeros((mask_rows, V), dtype=np.float32), Cn, path, state=True)
        want, wh, wv = eng.ais_grouped(eng.to_device(W), eng.to_device(c), eng.to_device(b), bA, betas, N * Cn,
                                       RngAddr(SEED, STREAM, STEP, 0, 0), _table(eng, bounds), path=path, trace=True)
        np.testing.assert_array_equal(logw.reshape(-1), want)
        np.testing.assert_array_equal(th, wh)
        np.testing.assert_array_equal(tv, wv)
        np.testing.assert_array_equal(state, wv[-1])                 # v_state on return is v_K, the last visible sample


@pytest.mark.parametrize("N,Cn", X.SHAPES)
@pytest.mark.parametrize("V,H,s,bounds,paths", X.PARITY)
def test_every_unit_held(hip_engine, V, H, s, bounds, paths, N, Cn):
    """A mask of ones: nothing is random.  log w against sum_j softplus(a_j(obs)) - H log 2 (float64) within the forced-parity
    bound of the case (4x the twin's float32-vs-float64 gap on it), the state is obs, the chains of a row are bit-equal."""
    W, c, b, bA = G.parity_params(V, H, s)
    betas = np.linspace(0, 1, 9)
    obs, _ = X.clamp_inputs(N, V, bounds, N)
    mask = np.ones((1, V), dtype=np.float32)
    want = np.logaddexp(0.0, obs.astype(np.float64) @ W.astype(np.float64) + c.astype(np.float64)).sum(axis=1) - H * np.log(2.0)
    r64 = X.gcais_twin(W, c, b, bA, bounds, betas, obs, mask, Cn, SEED, STREAM, STEP, gaps=False)
    r32 = X.gcais_twin(W, c, b, bA, bounds, betas, obs, mask, Cn, SEED, STREAM, STEP, dtype=np.float32, gaps=False)
    gap = float(np.abs(r32["logw"] - r64["logw"]).max())
    assert np.abs(r64["logw"] - want[:, None]).max() <= 1e-9
    for path in paths:
        logw, th, tv, state = _device(hip_engine, W, c, b, bA, bounds, betas, obs, mask, Cn, path, state=True)
        tag = "GCAIS all held %d->%d N=%d C=%d path %d" % (V, H, N, Cn, path)
        print("%s: float32-vs-float64 gap of the twin %.3e, bound %.3e, device %.3e" % (tag, gap, 4 * gap, np.abs(logw - want[:, None]).max()))
        np.testing.assert_array_equal(state, np.repeat(obs, Cn, axis=0))
        assert (tv == np.repeat(obs, Cn, axis=0)[None]).all()
        assert (logw == logw[:, :1]).all(), "%s: the chains of a row differ" % tag
        check(tag + ": log w per chain", np.abs(logw - want[:, None]).max(), 4 * gap, "cais_logw")


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("V,H,s,bounds", [X.PARITY[0][:4], X.PARITY[1][:4]])
def test_a_group_follows_the_mask_at_its_first_column(hip_engine, V, H, s, bounds, path):
    """The engine itself (no RBM check in the way): a mask with 1 at a group's first column only gives exactly the outputs of
    the whole group held, one with 0 there and 1 on the rest of the group exactly those of the whole group free."""
    W, c, b, bA = G.parity_params(V, H, s)
    betas = np.linspace(0, 1, 9)
    N, Cn = X.SHAPES[1]
    obs, base = X.clamp_inputs(N, V, bounds, N)
    spans = sm.spans(bounds)
    picks = [spans[0], spans[len(spans) // 2], spans[-1]]
    for first_value in (1.0, 0.0):
        whole, ragged = base.copy(), base.copy()
        for r in range(N):
            lo, hi = picks[r % len(picks)]
            whole[r, lo:hi] = first_value
            ragged[r, lo] = first_value
            ragged[r, lo + 1:hi] = 1.0 - first_value
        assert (whole != ragged).any()
        want = _device(hip_engine, W, c, b, bA, bounds, betas, obs, whole, Cn, path, state=True)
        got = _device(hip_engine, W, c, b, bA, bounds, betas, obs, ragged, Cn, path, state=True)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
    held_all, free_all = base.copy(), base.copy()
    lo, hi = spans[0]
    held_all[:, lo:hi], free_all[:, lo:hi] = 1.0, 0.0
    a = _device(hip_engine, W, c, b, bA, bounds, betas, obs, held_all, Cn, path, trace=False)
    z = _device(hip_engine, W, c, b, bA, bounds, betas, obs, free_all, Cn, path, trace=False)
    assert (a != z).any()                                # (the two masks do give different runs)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("V,H,s,bounds", X.CASES)
def test_ground_truth(hip_engine, V, H, s, bounds, path):
    """The cases, masks, C, K and seeds of tests/test_gcais_twin.py::test_the_twin_alone_meets_the_exact_values through
    RBM.conditional_log_partition / conditional_log_likelihood: every row's log Z_r^ and log p^ within 4 std_err and 0.05 nats
    of the brute-force conditional partition function / the float64 log p built from it."""
    W, c, b, bA = G.case_params(V, H, s)
    v, mask = X.ground_truth_inputs(V, bounds)
    held = mask != 0
    rbm = X.layer(hip_engine, V, H, bounds, W, c, b, X.CASE_SEEDS[V])
    log_Z, err = rbm.conditional_log_partition(v, mask, n_chains=X.CHAINS, n_betas=X.N_BETAS, base_vbias=bA, path=path)
    assert rbm._rng_step == STEP + 2 * X.N_BETAS - 1
    rbm._rng_step = STEP
    log_p, err_p = rbm.conditional_log_likelihood(v, mask, n_chains=X.CHAINS, n_betas=X.N_BETAS, base_vbias=bA, path=path)
    assert log_Z.shape == err.shape == log_p.shape == err_p.shape == (X.N_ROWS,)
    none_free = held.all(axis=1)
    _, held_bound = _all_held_bound(W, c, b, bA, bounds, np.linspace(0, 1, X.N_BETAS + 1), v)
    for row in range(X.N_ROWS):
        exact = X.exact_cond_log_Z_grouped(W, c, b, bounds, v[row], held[row])
        exact_p = X.exact_cond_log_p_grouped(W, c, b, bounds, v[row], held[row])
        print("GCAIS %d->%d path %d row %d: log Z^ %.5f exact %.5f |err| %.5f std_err %.5f; log p^ %.5f exact %.5f |err| %.5f std_err %.5f"
              % (V, H, path, row, log_Z[row], exact, abs(log_Z[row] - exact), err[row],
                 log_p[row], exact_p, abs(log_p[row] - exact_p), err_p[row]))
        if none_free[row]:       # no free unit: nothing is random -- std_err 0, log Z_r within the float32 allowance, (0, 0) by rule
            assert err[row] == 0.0 and log_p[row] == 0.0 and err_p[row] == 0.0 and abs(exact_p) <= 1e-9
            check("GCAIS %d->%d path %d row %d (every unit held): log Z_r" % (V, H, path, row), abs(log_Z[row] - exact), held_bound,
                  "cais_logw")
            continue
        assert err[row] > 0 and err_p[row] > 0
        assert abs(log_Z[row] - exact) <= 4 * err[row], (row, log_Z[row], exact, err[row])
        assert abs(log_Z[row] - exact) <= 0.05, (row, log_Z[row], exact)
        assert abs(log_p[row] - exact_p) <= 4 * err_p[row], (row, log_p[row], exact_p, err_p[row])
        assert abs(log_p[row] - exact_p) <= 0.05, (row, log_p[row], exact_p)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("V,H,s,bounds", X.CASES)
def test_one_group_free_is_the_group_posterior(hip_engine, V, H, s, bounds, path):
    """The classification reading: one row with only its first group free; conditional_log_likelihood within 4 std_err and 0.05
    nats of log RBM.group_posterior(v, 0)[category]."""
    W, c, b, bA = G.case_params(V, H, s)
    row, mask = X.one_free_inputs(V, bounds)
    lo, hi = sm.spans(bounds)[0]
    rbm = X.layer(hip_engine, V, H, bounds, W, c, b, X.ONE_FREE_SEEDS[V])
    want = float(np.log(rbm.group_posterior(row, 0)[0, int(row[0, lo:hi].argmax())]))
    assert rbm._rng_step == STEP                         # (group_posterior draws nothing)
    log_p, err = rbm.conditional_log_likelihood(row, mask, n_chains=X.CHAINS, n_betas=X.N_BETAS, base_vbias=bA, path=path)
    print("GCAIS %d->%d path %d one group free: log p^ %.5f log posterior %.5f |err| %.5f std_err %.5f"
          % (V, H, path, log_p[0], want, abs(log_p[0] - want), err[0]))
    assert err[0] > 0
    assert abs(log_p[0] - want) <= 4 * err[0], (log_p[0], want, err[0])
    assert abs(log_p[0] - want) <= 0.05, (log_p[0], want)


def test_paths_agree(hip_engine):
    """Path 1 and path 2 meet the same uniforms over 50 temperatures: at most 2 of the 64 chains part at a masked near tie (the
    forced twin vouches for each), log w of the rest within the forced bound."""
    V, H, s, bounds, _ = X.PARITY[0]
    N, Cn = X.SHAPES[0]
    W, c, b, bA = G.parity_params(V, H, s)
    betas = np.linspace(0, 1, 51)
    obs, mask = X.clamp_inputs(N, V, bounds, N)
    out = {p: _device(hip_engine, W, c, b, bA, bounds, betas, obs, mask, Cn, p) for p in (1, 2)}
    gaps = {}
    for p, (logw, th, tv) in out.items():
        r64, gaps[p] = _forced(W, c, b, bA, bounds, betas, obs, mask, Cn, th, tv)
        _check_forced("GCAIS paths 100->24 K=50 path %d" % p, logw, r64, gaps[p], obs, mask, bounds, Cn, tv)
    same = (out[1][1] == out[2][1]).all(axis=(0, 2)) & (out[1][2] == out[2][2]).all(axis=(0, 2))
    assert same.sum() >= N * Cn - 2, "%d of %d chains differ between the paths" % (N * Cn - same.sum(), N * Cn)
    check("GCAIS paths 100->24 K=50: log w path 1 vs 2", np.abs(out[1][0] - out[2][0]).reshape(-1)[same].max(), 4 * max(gaps.values()),
          "cais_logw")


def test_cut_is_invisible(hip_engine):
    """4099 temperatures on path 1 (AIS_CUT = 4096) under one mask row for every data row (about half the units held): every
    row's log Z_r^ against the uncut twin's within 4 of the larger standard error (the chains need not be the twin's: near
    ties)."""
    V, H, s, bounds, _ = X.PARITY[0]
    (N, Cn), K = X.SHAPES[0], 4096 + 3
    W, c, b, bA = G.parity_params(V, H, s)
    betas = np.linspace(0, 1, K + 1)
    obs, mask = X.clamp_inputs(N, V, bounds, 1)
    held = X.chain_held(mask, bounds, 1, V, 1)[0]
    assert held.any() and not held.all()
    logw = _device(hip_engine, W, c, b, bA, bounds, betas, obs, mask, Cn, 1, trace=False)
    tw = X.gcais_twin(W, c, b, bA, bounds, betas, obs, mask, Cn, SEED, STREAM, STEP, gaps=False)
    (lz_d, err_d), (lz_t, err_t) = X.estimate_rows(logw, bA, mask, H, bounds), X.estimate_rows(tw["logw"], bA, mask, H, bounds)
    print("GCAIS cut 100->24 K=%d: worst |device - twin| %.5f, chains equal to the twin's: %d of %d"
          % (K, np.abs(lz_d - lz_t).max(), int((np.abs(logw - tw["logw"]) < 1e-3).sum()), N * Cn))
    assert (np.abs(lz_d - lz_t) <= 4 * np.maximum(err_d, err_t)).all(), (lz_d, lz_t, err_d, err_t)


@pytest.mark.parametrize("path", [1, 2])
def test_deterministic(hip_engine, path):
    V, H, s, bounds, _ = X.PARITY[0]
    W, c, b, bA = G.parity_params(V, H, s)
    betas = np.linspace(0, 1, 21)
    obs, mask = X.clamp_inputs(7, V, bounds, 7)
    a = _device(hip_engine, W, c, b, bA, bounds, betas, obs, mask, 3, path, trace=False)
    z = _device(hip_engine, W, c, b, bA, bounds, betas, obs, mask, 3, path, trace=False)
    np.testing.assert_array_equal(a, z)


def test_path_by_shape(hip_engine):
    """path = 0: the one-launch kernel where the layer is LDS-resident (no GEMM launch), the general path elsewhere; path = 1 at
    1024 -> 256 is MDBN_EINVAL "LDS-resident"."""
    from mdbn_amd import _lib
    betas = np.linspace(0, 1, 5)
    for (V, H, s, bounds, _), expect in ((X.PARITY[0], 1), (X.PARITY[2], 2)):
        W, c, b, bA = G.parity_params(V, H, s)
        obs, mask = X.clamp_inputs(7, V, bounds, 7)
        by_shape = _device(hip_engine, W, c, b, bA, bounds, betas, obs, mask, 3, 0, trace=False, expect=expect)
        np.testing.assert_array_equal(by_shape, _device(hip_engine, W, c, b, bA, bounds, betas, obs, mask, 3, expect, trace=False))
    with pytest.raises(_lib.MdbnError, match="LDS-resident"):
        _device(hip_engine, W, c, b, bA, bounds, betas, obs, mask, 3, 1, trace=False, expect=0)


def test_rng_bookkeeping_and_refusals(hip_engine):
    """2K - 1 steps per call; conditional_log_likelihood is conditional_log_partition at the same RNG position; a split mask
    and a free group that is not one-hot are refused before anything is drawn."""
    V, H, s, bounds = X.CASES[3]
    K = 50
    W, c, b, bA = G.case_params(V, H, s)
    data = sm.one_hot_data(np.random.RandomState(2), 12, V, bounds)
    from _gclamp_np import unit_mask
    mask = unit_mask(V, bounds, rows=12)
    held = mask != 0
    one = X.layer(hip_engine, V, H, bounds, W, c, b, 7, step=0)
    log_p, err = one.conditional_log_likelihood(data, mask, n_chains=5, n_betas=K)
    assert one._rng_step == 2 * K - 1
    one._rng_step = 0
    log_Z, err2 = one.conditional_log_partition(data, mask, n_chains=5, n_betas=K)
    assert one._rng_step == 2 * K - 1
    term = -(held * data.astype(np.float64) * b.astype(np.float64)[None, :]).sum(axis=1)
    want = -np.asarray(one.free_energy(data).get_value(), dtype=np.float64) + term - log_Z
    free_rows = ~held.all(axis=1)
    np.testing.assert_array_equal(log_p[free_rows], want[free_rows])
    np.testing.assert_array_equal(err[free_rows], err2[free_rows])
    assert log_p[0] == 0.0 and err[0] == 0.0             # (unit_mask: row 0 holds every unit)
    lo, hi = sm.spans(bounds)[1]
    split = mask.copy()
    split[1, lo:hi] = 0.0
    split[1, lo] = 1.0
    with pytest.raises(ValueError, match=r"columns %d \.\. %d" % (lo, hi - 1)):
        one.conditional_log_partition(data, split, n_chains=5, n_betas=K)
    bad = data.copy()
    bad[1, lo:hi] = 1.0                                  # (unit_mask: row 1 holds nothing)
    with pytest.raises(ValueError, match="exactly one 1"):
        one.conditional_log_likelihood(bad, mask, n_chains=5, n_betas=K)
    assert one._rng_step == 2 * K - 1


def test_refused_calls_leave_the_outputs_untouched(hip_engine):
    """Every MDBN_EINVAL case of mdbn_ais_cond_run_grouped: a message, no launch, logw and v_state as they were."""
    import torch
    from mdbn_amd import RngAddr, _lib
    from mdbn_amd.engine import padded_ld
    eng = hip_engine

    def call(V, H, bounds, path=0, host=True, N=4, Cn=4, mask_rows=None, n_betas=5, short=0):
        W, c, b, bA = G.parity_params(V, H, 0.05)
        dW, dc, db, dbA = (eng.to_device(x) for x in (W, c, b, bA))
        ldh, ldv = dW.stride(0), padded_ld(V)
        betas = torch.from_numpy(np.linspace(0, 1, 5).astype(np.float32)).to(eng.device)
        n = C.c_int64()
        _lib.check(eng.lib.mdbn_ais_cond_workspace_bytes(eng.ctx, N, Cn, V, H, 5, 2, C.byref(n)), "mdbn_ais_cond_workspace_bytes")
        ws = torch.empty(n.value // 4 + 64, dtype=torch.float32, device=eng.device)
        logw = torch.full((N * Cn,), 7.0, dtype=torch.float64, device=eng.device)
        v_state = torch.full((N * Cn, ldv), 7.0, dtype=torch.float32, device=eng.device)
        obs = torch.zeros((N, ldv), dtype=torch.float32, device=eng.device)
        mask = torch.zeros((N, ldv), dtype=torch.float32, device=eng.device)
        host_t = np.ascontiguousarray(bounds, dtype=np.int32)
        dev_t = torch.from_numpy(host_t.copy()).to(eng.device)
        r = RngAddr(SEED, STREAM, STEP, 0, 0).c()
        rc = eng.lib.mdbn_ais_cond_run_grouped(
            eng.ctx, eng._stream(), eng._p(dW), V, H, ldh, eng._p(dc), eng._p(db), eng._p(dbA), eng._p(betas), n_betas, eng._p(obs),
            eng._p(mask), N if mask_rows is None else mask_rows, N, Cn, ldv, eng._p(v_state), eng._p(logw), None, None, path,
            C.byref(r), eng._p(ws), 64 if short else ws.numel() * 4, eng._p(dev_t), C.c_void_p(host_t.ctypes.data) if host else None,
            host_t.size - 1)
        eng.synchronize()
        return rc, _lib.last_error(), bool((logw == 7.0).all()) and bool((v_state == 7.0).all())

    good = list(range(0, 101, 5))
    rc, _, untouched = call(100, 24, good)
    assert rc == 0 and not untouched
    for what, kw in (("a descending table", dict(V=100, H=24, bounds=[0, 10, 5, 20])),
                     ("a group of 1", dict(V=100, H=24, bounds=[0, 5, 6, 10])),
                     ("a group of 65", dict(V=100, H=24, bounds=[0, 65])),
                     ("a boundary beyond V", dict(V=100, H=24, bounds=[90, 101])),
                     ("a missing host copy", dict(V=100, H=24, bounds=good, host=False)),
                     ("mask_rows", dict(V=100, H=24, bounds=good, mask_rows=2)),
                     ("n_betas < 2", dict(V=100, H=24, bounds=good, n_betas=1)),
                     ("a short workspace", dict(V=100, H=24, bounds=good, short=1)),
                     ("path 1 at 1024 -> 256", dict(V=1024, H=256, bounds=list(range(0, 1025, 4)), path=1))):
        rc, msg, untouched = call(**kw)
        assert rc == -1 and msg and untouched, (what, rc, msg, untouched)
