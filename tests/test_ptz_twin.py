"""log Z from the tempering ladder, on the CPU: the float64 twin (tests/_ptz_np.py on tests/_temper_np.py's sweep) against
exact partition functions of the four ground-truth layers of the AIS tests, Bennett's acceptance ratio beside the bridged
mean, and the device's accumulator recurrence beside a direct float64 logsumexp of the same works."""
import numpy as np
import pytest

import _ais_np as A
import _ptz_np as Z

# The setting the float64 twin meets the criterion with on three seeds per layer: the ladders of the GPU tests
M, R, N_SWEEPS, BURN_IN = 32, 16, 600, 150
SEED = 1


@pytest.fixture(scope="module")
def runs():
    """One twin run per ground-truth layer, shared by the tests below: (works, accepted, exact log Z, log Z_0)."""
    out = {}
    for V, H, s, gauss in A.CASES:
        W, c, b, bA = A.case_params(V, H, s, gauss)
        works, acc = Z.run_works(W, c, b, bA, gauss, np.linspace(0, 1, R), M, N_SWEEPS, BURN_IN, SEED)
        out[(V, H)] = works, acc, A.brute_log_Z(W, c, b, gauss), A.log_Z_base(bA, H, gauss)
    return out


@pytest.mark.parametrize("V,H,s,gauss", A.CASES)
def test_twin_against_brute_force(runs, V, H, s, gauss):
    """|log Z^ - log Z| <= 4 standard errors and <= 0.05 nats (the AIS twin's criterion) for the bridged mean; the one-sided
    estimates and BAR are printed beside it."""
    works, acc, exact, z0 = runs[(V, H)]
    assert works.shape == (N_SWEEPS - BURN_IN, M, R - 1, 2) and acc.min() > 0
    mid, se = Z.estimate(works, z0, "mid")
    fwd, rev, bar = (Z.estimate(works, z0, m, jackknife=False)[0] for m in ("fwd", "rev", "bar"))
    print("ptz twin %d->%d %s: exact %.5f; error of fwd %+.5f rev %+.5f mid %+.5f bar %+.5f; jackknife SE of mid %.5f"
          % (V, H, "GRBM" if gauss else "RBM", exact, fwd - exact, rev - exact, mid - exact, bar - exact, se))
    assert abs(mid - exact) <= 4 * se, (mid, exact, se)
    assert abs(mid - exact) <= 0.05, (mid, exact)
    assert abs(0.5 * (fwd + rev) - mid) <= 1e-12


@pytest.mark.parametrize("V,H", [(24, 12), (20, 10)])
def test_bar_and_mid_agree(runs, V, H):
    """Bennett's acceptance ratio from the tapped works and the bridged mean agree within their joint jackknife error."""
    works, acc, exact, z0 = runs[(V, H)]
    mid, se_mid = Z.estimate(works, z0, "mid")
    bar, se_bar = Z.estimate(works, z0, "bar")
    print("ptz twin %d->%d: mid %.5f +- %.5f, bar %.5f +- %.5f, exact %.5f" % (V, H, mid, se_mid, bar, se_bar, exact))
    assert abs(bar - mid) <= 4 * np.hypot(se_mid, se_bar), (bar, mid, se_mid, se_bar)
    assert abs(bar - exact) <= 4 * se_bar and abs(bar - exact) <= 0.05


@pytest.mark.parametrize("V,H,s,gauss", A.CASES)
def test_recurrence_equals_direct_logsumexp(runs, V, H, s, gauss):
    """The accumulator (running maximum, float32 exponentials, double sum) against a float64 logsumexp of the same works: 1e-5
    nats -- at most 3 ulp of float32 per exponential (relative 4e-7 on every term, hence on the sum) plus one float32 rounding
    of the exponent per rescale (6e-8 relative on an O(10) exponent: 6e-7 absolute, a few dozen rescales at the very most)."""
    works = runs[(V, H)][0]
    z = Z.accumulate(works)
    worst = np.abs(Z.zacc_log_sums(z) - Z.direct_log_sums(works)).max()
    print("ptz twin %d->%d: recurrence vs direct logsumexp, worst %.3e nats" % (V, H, worst))
    assert worst <= 1e-5, worst
    # two halves accumulate what the whole does, bit for bit
    half = Z.accumulate(works[120:], Z.accumulate(works[:120]))
    np.testing.assert_array_equal(half, z)


def test_package_finish_equals_the_twin(runs):
    """mdbn_amd.temper.estimate_log_z (the host finish of the package) from the accumulators / the tap against the twin's
    estimate from the works themselves."""
    from mdbn_amd.temper import attempts, estimate_log_z
    works, acc, exact, z0 = runs[(20, 10)]
    tries = attempts(M, R, BURN_IN, N_SWEEPS - BURN_IN)
    z = Z.accumulate(works)
    for method in ("mid", "bar"):
        got = estimate_log_z(z, tries, z0, method, works)
        want, se = Z.estimate(works, z0, method)
        assert abs(got.log_z - want) <= 2e-5 and abs(got.stderr - se) <= 1e-5 + 1e-3 * se, (method, got, want, se)
        assert abs(got.log_z_fwd - Z.estimate(works, z0, "fwd", jackknife=False)[0]) <= 2e-4
        assert abs(got.log_z_rev - Z.estimate(works, z0, "rev", jackknife=False)[0]) <= 2e-4
        assert got.ratios_fwd.shape == (R - 1,) and (got.attempts == tries).all()


def test_float32_works_follow_the_definition():
    """The device's regrouping in float32 along the float64 twin's states: the same works up to float32 row sums."""
    import _temper_np as T
    V, H, s, gauss = 40, 14, 0.2, True
    W, c, b, bA = A.case_params(V, H, s, gauss)
    bA = bA + np.float32(0.2)                    # (b_A = b would make s1 and g vanish)
    betas = np.linspace(0, 1, 8)
    r = T.pt_twin(W, c, b, bA, gauss, betas, np.zeros((5 * 8, H)), 20, 0, 5, 3, 11)
    tv = r["trace_v"].astype(np.float32)
    w64 = Z.works_from_trace(W, c, b, bA, gauss, betas, tv, r["trace_swaps"])
    w32 = Z.works_from_trace(W, c, b, bA, gauss, betas, tv, r["trace_swaps"], dtype=np.float32)
    np.testing.assert_array_equal(np.isnan(w64), np.isnan(w32))
    np.testing.assert_array_equal(np.isnan(w64[:, :, :, 0]), r["trace_swaps"][:, :, 1, :-1] < 0)
    assert np.nanmax(np.abs(w32 - w64)) <= 1e-4
    # d_fwd + d_rev is the acceptance difference of the swap
    w = Z.works_from_trace(W, c, b, bA, gauss, betas, r["trace_v"], r["trace_swaps"])
    np.testing.assert_allclose(w[~np.isnan(w[..., 0])].sum(axis=1), _delta_in_trace_order(r, w), rtol=0, atol=1e-9)


def _delta_in_trace_order(r, w):
    """pt_twin's ``delta`` (one entry per attempt in (sweep, pair, ladder) order) reordered to w's (sweep, ladder, pair)."""
    n, M, P, _ = w.shape
    out = np.full((n, M, P), np.nan)
    at = 0
    for t in range(n):
        for rho in range(t % 2, P, 2):
            out[t, :, rho] = r["delta"][at:at + M]
            at += M
    return out[~np.isnan(w[..., 0])].ravel()
