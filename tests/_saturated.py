"""A saturated (trained-like) layer for the parity tests (TEST-ONLY, no GPU needed to import).

Every other parity test keeps its pre-activations within a few units of zero (W = init_W, biases N(0, 0.2), data N(0, 1) or
0/1).  `params` keeps W and the data -- the GEMM operands, so the conditioning of the products does not change -- and moves the
BIASES onto a ladder that visits every place where the float32 sigmoid / softplus of csrc/mdbn_device.h changes behaviour:

    |x| = 24 ln 2 = 16.64    1 + exp(-x) rounds to 1: the sigmoid is exactly 1, the softplus drops its log term
    |x| = 126 ln 2 = 87.34   sigmoid(-x) falls below the smallest normal float32
    |x| = 128 ln 2 = 88.72   exp(x) overflows to +inf in float32
    |x| = 150 ln 2 = 103.97  sigmoid(-x) falls below the smallest subnormal

BANDS are the edges between these regimes (with a transition band on either side of 16.64 .. 17.33 = 25 ln 2); `band_counts`
histograms pre-activations over them, and every step test asserts on the ORACLE's pre-activations that the bands it claims are
populated.  `replay` restates a tapped CD-k step pass by pass in float64 along the device's recorded samples, and
`check_saturation` holds the device to what follows from the table above:

    oracle pre >= 17.5           the mean is exactly 1.0f, the sample is 1       (margin 0.17 over 25 ln 2)
    oracle pre <= -89            the mean is exactly 0 (either sign), the sample is 0       (margin 0.27 over 128 ln 2)
    -89 < oracle pre <= -87.34   the mean is <= 1.2e-38 (flushed or subnormal), the sample is 0

A uniform of oracle/philox_np.py lies in [2^-25, 1 - 2^-25], so in these regions `u < mean` leaves no tie: a sample that
differs is a failure."""
import numpy as np

from oracle import rbm_np
from oracle.philox_np import PhiloxDraws

LADDER = (-120, -104, -89, -88, -87, -40, -17.5, -16.5, -9, -3, 0, 3, 9, 16.5, 17.5, 40, 87, 88, 89, 104, 120)
BANDS = (-200, -103.98, -88.73, -87.34, -17.33, -16.64, -5, 5, 16.64, 17.33, 87.34, 88.73, 103.98, 200)

# the eleven bands other than the two 0.69 wide ones between 24 ln 2 and 25 ln 2, which a pass over two dozen units may miss
REGIMES = tuple(i for i in range(13) if i not in (4, 8))

UP_EXACT, LOW_EXACT, LOW_TINY, TINY = 17.5, -89.0, -87.34, 1.2e-38


def ladder_bias(rs, n, start=0, stride=1):
    """bias[i] = LADDER[(stride i + start) % 21] + N(0, 0.2), float32."""
    rungs = np.asarray(LADDER, dtype=np.float64)[(stride * np.arange(n) + start) % len(LADDER)]
    return (rungs + rs.normal(0, 0.2, n)).astype(np.float32)


def params(rs, V, H, gauss):
    """(W, hbias, vbias) float32: W = init_W unchanged, hbias on the ladder; vbias on the ladder (stride 5, so that a visible
    row of few units still meets every rung) for a Bernoulli RBM, N(0, 0.2) for a GRBM, whose visible mean IS its
    pre-activation and would carry the ladder into the next propup's operand."""
    W = rbm_np.init_W(rs, V, H, np.float32)
    hb = ladder_bias(rs, H)
    vb = rs.normal(0, 0.2, V).astype(np.float32) if gauss else ladder_bias(rs, V, start=3, stride=5)
    return W, hb, vb


def sampler_biases(V, H, gauss, b, seed=3):
    """(c, b) of a sampler test on the saturated layer: the hidden bias of `params`, and its visible bias for a Bernoulli
    layer; a GRBM keeps the test's own `b` (the test keeps its own W as well)."""
    _, c, b_sat = params(np.random.RandomState(seed), V, H, gauss)
    return c, (np.asarray(b, dtype=np.float32) if gauss else b_sat)


def band_counts(*pre):
    """Number of values in each of the 13 bands between consecutive BANDS edges (nothing may lie outside +-200)."""
    x = np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in pre])
    assert x.min() > BANDS[0] and x.max() < BANDS[-1], (x.min(), x.max())
    return np.histogram(x, bins=np.asarray(BANDS))[0]


def assert_bands(tag, pre, bands=range(13)):
    counts = band_counts(*pre)
    empty = [(BANDS[i], BANDS[i + 1]) for i in bands if counts[i] == 0]
    assert not empty, "%s: no oracle pre-activation in the bands %r (counts %r)" % (tag, empty, counts.tolist())
    return counts


def replay(W, hb, vb, gauss, v0, k, th, tv, rng):
    """The passes of a tapped CD-k step in float64 along the recorded samples th [>= k, B, H] / tv [k, B, V] (None for a
    GRBM): a list of dict(name, layer 'h' / 'v', pre, mean, u, sample), `sample` the device's recorded one or None where the
    step records none (the last hidden pass; a GRBM's visible pass, which is linear: u and sample None, mean = pre)."""
    st = rbm_np.RBMState(W.shape[0], W.shape[1], W=W, hbias=hb, vbias=vb, gauss=gauss)
    draws = PhiloxDraws(*rng)
    v0 = np.asarray(v0, dtype=np.float64)
    B, (V, H) = v0.shape[0], W.shape
    pre, mean = rbm_np.propup(st, v0)
    passes = [dict(name="h0", layer="h", pre=pre, mean=mean, u=draws.u(0, B, H), sample=np.asarray(th[0], dtype=np.float64))]
    chain = passes[0]["sample"]
    for t in range(1, k + 1):
        if gauss:
            pre = chain @ st.W.T + st.vbias
            passes.append(dict(name="v%d" % t, layer="v", pre=pre, mean=pre, u=None, sample=None))
            v_in = pre
        else:
            pre, mean = rbm_np.propdown(st, chain)
            v_in = np.asarray(tv[t - 1], dtype=np.float64)
            passes.append(dict(name="v%d" % t, layer="v", pre=pre, mean=mean, u=draws.u(2 * t - 1, B, V), sample=v_in))
        pre, mean = rbm_np.propup(st, v_in)
        rec = np.asarray(th[t], dtype=np.float64) if t < len(th) else None
        passes.append(dict(name="h%d" % t, layer="h", pre=pre, mean=mean, u=draws.u(2 * t, B, H), sample=rec))
        chain = rec
    return passes


def check_saturation(tag, pre, mean=None, sample=None):
    """The exactness rules of the module docstring for one sigmoid pass: `pre` the oracle's (float64), `mean` / `sample` the
    device's (either may be None).  Returns the number of elements in the three exact regions."""
    up, low, tiny = pre >= UP_EXACT, pre <= LOW_EXACT, (pre > LOW_EXACT) & (pre <= LOW_TINY)
    if mean is not None:
        mean = np.asarray(mean)
        assert np.isfinite(mean).all(), "%s: non-finite probability" % tag
        assert mean.min() >= 0.0 and mean.max() <= 1.0, "%s: probability outside [0, 1]: [%r, %r]" % (tag, mean.min(), mean.max())
        assert (mean[up] == 1.0).all(), "%s: pre >= %g but the mean is not exactly 1 (least %r, %d of %d)" % (
            tag, UP_EXACT, mean[up].min(), int((mean[up] != 1.0).sum()), int(up.sum()))
        assert (mean[low] == 0.0).all(), "%s: pre <= %g but the mean is not exactly 0 (largest %r, %d of %d)" % (
            tag, LOW_EXACT, mean[low].max(), int((mean[low] != 0.0).sum()), int(low.sum()))
        assert (mean[tiny] <= TINY).all(), "%s: %g < pre <= %g but the mean is %r" % (tag, LOW_EXACT, LOW_TINY, mean[tiny].max())
    if sample is not None:
        sample = np.asarray(sample)
        assert np.isin(sample, (0.0, 1.0)).all(), "%s: a sample that is neither 0 nor 1" % tag
        assert (sample[up] == 1.0).all(), "%s: %d samples are 0 where pre >= %g" % (tag, int((sample[up] != 1.0).sum()), UP_EXACT)
        assert (sample[low | tiny] == 0.0).all(), "%s: %d samples are 1 where pre <= %g" % (
            tag, int((sample[low | tiny] != 0.0).sum()), LOW_TINY)
    return int(up.sum() + low.sum() + tiny.sum())


def oracle_ties(passes, tie=1e-6):
    """(draws within `tie` of their mean, all draws) over the passes of `replay` whose sample the step records.  A mean below
    2^-25 or above 1 - 2^-25 (|pre| > 25 ln 2 = 17.33) is out of reach of every uniform, the smallest and the largest included:
    such a draw is decided whatever u is and is no tie, however close to 0 or 1 both lie."""
    n = total = 0
    for p in passes:
        if p["u"] is not None and p["sample"] is not None:
            open_ = (p["mean"] >= 2.0 ** -25) & (p["mean"] <= 1.0 - 2.0 ** -25)
            n += int(((np.abs(p["u"].astype(np.float64) - p["mean"]) < tie) & open_).sum())
            total += p["u"].size
    return n, total


def free_run_taps(W, hb, vb, gauss, v0, k, rng):
    """The float64 oracle's own chain as taps (th [k, B, H], tv [k, B, V] or None): what a device without rounding records."""
    st = rbm_np.RBMState(W.shape[0], W.shape[1], W=W, hbias=hb, vbias=vb, gauss=gauss)
    draws = PhiloxDraws(*rng)
    v0 = np.asarray(v0, dtype=np.float64)
    B = v0.shape[0]
    _, _, h = rbm_np.sample_h_given_v(st, v0, draws.u(0, B, st.n_hidden))
    th, tv = [h], []
    for t in range(1, k + 1):
        dv = None if gauss else draws.u(2 * t - 1, B, st.n_visible)
        out = rbm_np.gibbs_hvh(st, th[-1], dv, draws.u(2 * t, B, st.n_hidden))
        tv.append(out[2])
        th.append(out[5])
    return np.stack(th[:k]), None if gauss else np.stack(tv)
