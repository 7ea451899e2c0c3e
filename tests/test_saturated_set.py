"""The saturated parameter set of the GPU parity tests (tests/_saturated.py) does what it claims, checked on the float64
oracle alone (no GPU): at 100 -> 24, B = 64, CD-2, free-running, every one of the 13 bands of pre-activation holds values,
and no recorded draw lies within 1e-6 of its mean -- so the cap on tie flips of tests/_variants.py is met by the reference
itself.  Also: the float32 runs of the samplers' numpy twins evaluate their sigmoid on such values without overflow."""
import warnings

import numpy as np
import pytest

import _saturated as S
from _variants import RNG


def _free_run(V, H, B, gauss, k=2, seed=5):
    """The inputs _variants.cd draws for `seed` with the saturated parameters, and the oracle's own chain as taps."""
    rs = np.random.RandomState(seed)
    W, hb, vb = S.params(rs, V, H, gauss)
    N = B + 13
    data = rs.normal(size=(N, V)).astype(np.float32) if gauss else (rs.uniform(size=(N, V)) < 0.3).astype(np.float32)
    x = data[rs.permutation(N)[:B]]
    th, tv = S.free_run_taps(W, hb, vb, gauss, x, k, RNG)
    return S.replay(W, hb, vb, gauss, x, k, th, tv, RNG)


def test_params_are_init_W_and_ladder_biases():
    from oracle import rbm_np
    for gauss in (False, True):
        W, hb, vb = S.params(np.random.RandomState(5), 100, 24, gauss)
        assert np.array_equal(W, rbm_np.init_W(np.random.RandomState(5), 100, 24, np.float32))
        assert W.dtype == hb.dtype == vb.dtype == np.float32
        assert np.abs(hb - np.asarray(S.LADDER)[np.arange(24) % 21]).max() < 1.0
        if gauss:
            assert np.abs(vb).max() < 1.0
        else:
            assert np.abs(vb - np.asarray(S.LADDER)[(5 * np.arange(100) + 3) % 21]).max() < 1.0
            assert len(set((5 * np.arange(21) + 3) % 21)) == 21     # a stride that visits every rung


@pytest.mark.parametrize("gauss", [False, True], ids=["rbm", "grbm"])
def test_every_band_is_filled_and_no_oracle_draw_is_a_tie(gauss):
    passes = _free_run(100, 24, 64, gauss)
    assert [p["name"] for p in passes] == ["h0", "v1", "h1", "v2", "h2"]
    S.assert_bands("hidden passes", [p["pre"] for p in passes if p["layer"] == "h"])
    if gauss:
        # a GRBM's visible pass is linear and stays near zero: its sigmoid is saturated by the cost tests instead
        assert max(np.abs(p["pre"]).max() for p in passes if p["layer"] == "v") < 30
    else:
        for p in passes:                                            # a Bernoulli RBM: every single pass
            S.assert_bands(p["name"], [p["pre"]])
    ties, draws = S.oracle_ties(passes)
    assert draws == (64 * (2 * 24 + 2 * 100) if not gauss else 64 * 2 * 24) and ties == 0, (ties, draws)


def test_exactness_rules_hold_for_a_float32_sigmoid_and_catch_a_clamp():
    """check_saturation on the device's formula 1 / (1 + exp(-x)) evaluated in float32 on the ladder, and on wrong ones."""
    import _ais_np
    from oracle import rbm_np
    pre = np.asarray(S.LADDER, dtype=np.float64)[None, :] + np.linspace(-0.2, 0.2, 7)[:, None]
    mean = _ais_np.sigmoid(pre.astype(np.float32))
    assert mean.dtype == np.float32
    u = np.full(pre.shape, 0.5)
    assert S.check_saturation("exact", pre, mean, (u < mean).astype(np.float32)) > 0
    with pytest.raises(AssertionError):
        S.check_saturation("clamped", pre, rbm_np.sigmoid(np.clip(pre, -30, 30)).astype(np.float32))
    with pytest.raises(AssertionError):
        S.check_saturation("above one", pre, np.where(pre > 17.5, np.float32(1) + np.float32(2.0 ** -23), mean))
    with pytest.raises(AssertionError):
        S.check_saturation("nan", pre, np.where(pre < -88.8, np.float32("nan"), mean))


@pytest.mark.parametrize("module", ["_ais_np", "_clamp_np", "_temper_np"])
def test_twin_sigmoid_is_quiet_and_right_in_float32(module):
    twin = __import__(module)
    from oracle import rbm_np
    x = np.asarray(S.LADDER, dtype=np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = twin.sigmoid(x)
        got64 = twin.sigmoid(x.astype(np.float64))
    assert got.dtype == np.float32 and np.isfinite(got).all()
    np.testing.assert_allclose(got64, rbm_np.sigmoid(x.astype(np.float64)), rtol=1e-14, atol=0)
    np.testing.assert_allclose(got, rbm_np.sigmoid(x.astype(np.float64)), rtol=3e-7, atol=1.2e-38)    # (below the smallest normal: 0 will do)
