"""The twin of parallel tempering on a layer with categorical visible units (tests/_gtemper_np.py) on the CPU: with no groups
it is tests/_temper_np.py's twin to the bit; against exact marginals and log Z by enumeration under the criteria, seeds and
sizes of tests/test_gpu_gtemper.py -- so that the reference alone passes what the device is asked to pass --; and the
float32 twin along its own record inside the caps of the forced-parity cases."""
import numpy as np
import pytest

import _gtemper_np as GT
import _ptz_np as Z
import _softmax_np as sm
import _temper_np as T
from _margins import check
from test_temper_twin import ladder_error


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_no_groups_is_the_plain_twin_exactly(dtype):
    V, H, M, R, n = 30, 12, 3, 4, 9
    rs = np.random.RandomState(3)
    W, c, b, bA = rs.normal(0, 0.3, (V, H)), rs.normal(0, 0.5, H), rs.normal(0, 0.5, V), rs.normal(0, 0.3, V)
    h0 = GT.start(M, R, H)
    betas = np.linspace(0, 1, R)
    want = T.pt_twin(W, c, b, bA, False, betas, h0, n, 2, GT.SEED, GT.STREAM, GT.STEP, dtype=dtype)
    got = GT.pt_twin(W, c, b, bA, [V], betas, h0, n, 2, GT.SEED, GT.STREAM, GT.STEP, dtype=dtype)
    for k, x in want.items():
        np.testing.assert_array_equal(np.asarray(got[k]), np.asarray(x), err_msg=k)
    assert got["group_draws"] == 0
    # ... and forced along that record it finds nothing to report
    f = GT.pt_twin(W, c, b, bA, [V], betas, h0, n, 2, GT.SEED, GT.STREAM, GT.STEP, dtype=dtype,
                   forced=(want["trace_v"], want["trace_h"], want["trace_swaps"]))
    assert f["flips_outside_mask"] == 0 and (f["decided"] == (f["logu"] < f["delta"])).all()


def test_a_group_row_holds_one_1_from_one_uniform():
    """Every recorded row is one-hot per group, and a group's category is the one its first column's uniform picks."""
    from oracle import philox_np
    V, H, M, R = 12, 5, 2, 4
    bounds = [1, 4, 9]
    rs = np.random.RandomState(5)
    W, c, b, bA = rs.normal(0, 0.5, (V, H)), rs.normal(0, 0.5, H), rs.normal(0, 0.5, V), rs.normal(0, 0.3, V)
    betas = np.linspace(0, 1, R)
    r = GT.pt_twin(W, c, b, bA, bounds, betas, np.zeros((M * R, H)), 3, 0, GT.SEED, GT.STREAM, GT.STEP)
    for lo, hi in sm.spans(bounds):
        assert (r["trace_v"][:, :, lo:hi].sum(axis=2) == 1).all()
    # sweep 0 from h = 0 with the identity rank map: x = b_A + beta (b - b_A)
    beta = np.tile(betas.astype(np.float32).astype(np.float64), M)
    pre = bA[None, :] + beta[:, None] * (b - bA)[None, :]
    U = philox_np.uniform(M * R, V, GT.SEED, GT.STREAM, GT.STEP, 0)
    np.testing.assert_array_equal(r["trace_v"][0], sm.grouped_sample(sm.grouped_softmax(pre, bounds)[0], bounds, U))


def test_the_two_enumerations_agree():
    W, c, b, bA, bounds = GT.planted()
    (ev_h, lz_h), (ev_r, lz_r) = GT.exact_by_hidden(W, c, b, bounds), GT.exact_by_rows(W, c, b, bounds)
    assert abs(lz_h - lz_r) <= 1e-10 and np.abs(ev_h - ev_r).max() <= 1e-12
    for lo, hi in sm.spans(bounds):
        assert abs(ev_h[lo:hi].sum() - 1.0) <= 1e-12
    import _gais_np as G
    assert abs(lz_h - G.brute_log_Z(W, c, b, bounds)) <= 1e-10
    # a layer with Bernoulli columns around the groups
    rs = np.random.RandomState(2)
    V, H, bounds = 9, 4, [2, 4, 7]
    W, c, b = rs.normal(0, 0.6, (V, H)), rs.normal(0, 0.5, H), rs.normal(0, 0.5, V)
    (ev_h, lz_h), (ev_r, lz_r) = GT.exact_by_hidden(W, c, b, bounds), GT.exact_by_rows(W, c, b, bounds)
    assert abs(lz_h - lz_r) <= 1e-10 and np.abs(ev_h - ev_r).max() <= 1e-12


@pytest.fixture(scope="module")
def ladders():
    """The float64 twin's ground-truth runs, once: {tag: (exact E[v], exact log Z, v_avg, works, log Z_A, W, c, b, bounds)}."""
    out = {}
    betas = np.linspace(0, 1, GT.GT_R)
    for tag, W, c, b, bA, bounds in GT.ground_truth_cases():
        ev, lz = GT.exact_by_hidden(W, c, b, bounds)
        v_avg, works, acc = GT.run_ladder(W, c, b, bA, bounds, betas, GT.GT_M, GT.GT_SWEEPS, GT.GT_BURN)
        import _gais_np as G
        out[tag] = (ev, lz, v_avg, works, G.log_Z_base(bA, W.shape[1], bounds), W, c, b, bounds)
    return out


@pytest.mark.parametrize("case", [0, 1])
def test_the_twin_meets_the_exact_values_under_the_gpu_criteria(ladders, case):
    tag = GT.ground_truth_cases()[case][0]
    ev, lz, v_avg, works, lz0 = ladders[tag][:5]
    err, bound = ladder_error(v_avg, ev)
    est, se = Z.estimate(works, lz0, "mid")
    fwd, rev = lz0 + Z.ratios(works, "fwd").sum(), lz0 + Z.ratios(works, "rev").sum()
    print("gtemper twin %s: v_avg error %.4f (bound %.4f); ladder log Z^ %.4f +- %.4f (bracket %.4f .. %.4f), exact %.4f"
          % (tag, err, bound, est, se, fwd, rev, lz))
    assert err <= bound, (err, bound)
    assert se > 0 and abs(est - lz) <= 4 * se and abs(est - lz) <= 0.05, (est, se, lz)


def test_a_plain_grouped_chain_stays_in_the_light_mode():
    """Grouped Gibbs sampling from h = 0 on the planted layer (the twin without swaps): the beta = 1 chains miss the exact
    marginals by more than 0.3."""
    W, c, b, bA, bounds = GT.planted()
    ev, _ = GT.exact_by_hidden(W, c, b, bounds)
    r = GT.pt_twin(W, c, b, bA, bounds, np.linspace(0, 1, GT.GT_R), np.zeros((GT.GT_M * GT.GT_R, W.shape[1])), 300, 75, GT.SEED,
                   GT.STREAM, GT.STEP, swaps=False)
    err, _ = ladder_error(r["v_avg"], ev)
    print("planted layer without swaps: error %.4f" % err)
    assert r["accepted"].sum() == 0 and err > 0.3, err


def _cases():
    out = [(tag, V, H, s, bounds, sat, GT.PARITY_M, GT.PARITY_R, GT.PARITY_N) for tag, V, H, s, bounds, sat, _ in GT.PARITY]
    tag, V, H, s, bounds, sat, _ = GT.LARGE
    out.append((tag, V, H, s, bounds, sat, 4, GT.PARITY_R, 10))
    tag, V, H, s, bounds, sat, _ = GT.PARITY[0]
    out.append(("ragged R = 6", V, H, s, bounds, sat, GT.PARITY_M, GT.RAGGED_R, 12))
    return out


@pytest.mark.parametrize("tag,V,H,s,bounds,sat,M,R,n", _cases())
def test_the_float32_twin_stays_inside_the_caps(tag, V, H, s, bounds, sat, M, R, n):
    """The float32 twin's own run as the record: the forced-parity criteria of tests/test_gpu_gtemper.py hold for the reference
    alone on every case, with its seeds and sizes."""
    W, c, b, bA = GT.parity_params(V, H, s, sat)
    betas = np.linspace(0, 1, R).astype(np.float32)
    h0 = GT.start(M, R, H)
    burn = n // 4
    d = GT.pt_twin(W, c, b, bA, bounds, betas, h0, n, burn, GT.SEED, GT.STREAM, GT.STEP, dtype=np.float32)
    assert d["accepted"].sum() > 0
    r64, r32 = GT.forced_pair(W, c, b, bA, bounds, betas, h0, n, burn, d)
    GT.check_forced("gtemper twin " + tag, d, r64, r32, bounds, check)
