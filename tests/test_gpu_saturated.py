"""Every activation epilogue on a saturated (trained-like) layer: tests/_saturated.py puts the biases on a ladder of
pre-activations from -120 to 120, so that sigmoidf_ / softplusf_ of csrc/mdbn_device.h are evaluated where float32 changes
behaviour (|x| = 16.64: 1 + exp(-x) rounds to 1; 87.34: below the smallest normal; 88.72: exp overflows; 103.97: below the
smallest subnormal) in each place that restates the activation, cost and column-sum lines.

Part 1: the CD-2 step of an RBM and a GRBM on every GEMM family of the generic step (the rows of FAMILIES in
tests/test_gpu_step_variants.py, with their launch-kind witnesses), on the streaming kernel's wider tiles and on the four fast
paths, taken: against the float64 oracle teacher-forced along the device's taps with DESIGN.md section 4's tolerances
unchanged (the GEMM operands are those of the other tests; one more bias add costs ulp(|pre|) / 2, below 1e-8 after the factor
p (1 - p)), plus the exactness rules of tests/_saturated.py.  Part 2: the eager Gibbs steps and the monitoring kernels.

Free energies are differences of sums in the thousands: their bound is not a fixed number but that of tests/test_gpu_ais.py
-- the quantity restated in numpy on the same float32 inputs in float64 and with float32 products and softplus, the device
gets 4x the gap -- or today's relative 1e-4 where that is the tighter one."""
import numpy as np
import pytest

import _saturated as S
from oracle import philox_np, rbm_np
from _margins import check
from _variants import NO_FAST_PATH, RNG, cd, oracle
from test_gpu_step_variants import FAMILIES, _check_kinds

pytestmark = pytest.mark.gpu

K = 2


@pytest.fixture(scope="module")
def eng(built_lib):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mdbn_amd
    return mdbn_amd.HipEngine()


# ------------------------------------------------------------------ 1. the CD step on every path

def _step(eng, V, H, B, gauss, opts):
    return cd(eng, V, H, B, K, gauss, opts, params=S.params(np.random.RandomState(5), V, H, gauss))


def _check_step(tag, r):
    """`oracle` (section 4's tolerances; the Bernoulli cost, half of whose terms are wrong-side saturated and of order 100,
    within 2e-6) and what only a saturated layer can show: finite outputs, probabilities in [0, 1], exact saturation."""
    V, H, B, gauss = r["V"], r["H"], r["B"], r["gauss"]
    oracle(tag, r)
    passes = S.replay(r["W"], r["hb"], r["vb"], gauss, r["x"], K, r["th"], r["tv"], RNG)
    S.assert_bands(tag + " hidden", [p["pre"] for p in passes if p["layer"] == "h"])
    if not gauss:
        S.assert_bands(tag + " visible", [p["pre"] for p in passes if p["layer"] == "v"])
    assert all(n == 0 for n in r["nonfinite"].values()), "%s: count_nonfinite %r" % (tag, r["nonfinite"])
    for name in ("stats", "P2", "V2", "th", "tv"):
        assert r[name] is None or np.isfinite(r[name]).all(), "%s: %s is not finite" % (tag, name)
    ldh, ldv = r["ldh"], r["ldv"]
    assert not r["stats"][:V * ldh].reshape(V, ldh)[:, H:].any(), "%s: pad columns of S" % tag
    assert np.isfinite(r["stats"][V * ldh + ldh + ldv]), "%s: cost" % tag
    # the device's means: ph_mean, -nh_mean of the last hidden pass, nv_mean of the last visible pass (a GRBM's is linear)
    means = {"h0": r["P2"][:B, :H], "h%d" % K: -r["P2"][B:2 * B, :H]}
    if not gauss:
        means["v%d" % K] = r["V2"][B:2 * B, :V]
    exact = 0
    for p in passes:
        if p["layer"] == "v" and gauss:
            continue
        exact += S.check_saturation("%s %s" % (tag, p["name"]), p["pre"], means.get(p["name"]), p["sample"])
    assert exact > 0
    return passes


@pytest.mark.parametrize("gauss", [False, True], ids=["rbm", "grbm"])
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_saturated_step_on_every_gemm_family(eng, fam, gauss):
    V, H, B, opts = FAMILIES[fam][:4]
    r = _step(eng, V, H, B, gauss, dict(opts, **NO_FAST_PATH))       # (a plain CD step would take a fast path where it can)
    _check_kinds("cd", fam, r)
    _check_step("saturated %s %s" % (fam, "GRBM" if gauss else "RBM"), r)


@pytest.mark.parametrize("gauss", [False, True], ids=["rbm", "grbm"])
@pytest.mark.parametrize("knob", ["stream_mi", "stream_ni"])
def test_saturated_step_on_wider_stream_tiles(eng, knob, gauss):
    V, H, B = FAMILIES["stream"][:3]
    r = _step(eng, V, H, B, gauss, dict(NO_FAST_PATH, **{knob: 2}))
    _check_kinds("cd", "stream", r)
    _check_step("saturated stream %s=2 %s" % (knob, "GRBM" if gauss else "RBM"), r)


def _one_launch(r):
    return r["kinds"] == []


def _planes(r):
    return r["eligible"] and r["scratch_planes"] and bool(r["kinds"]) and all(kd >= 2000 for kd in r["kinds"])


def _group_chain(r):
    # only the statistics GEMM (layout 3) is launched as a GEMM: no forward pass was
    return bool(r["kinds"]) and all(kd % 10 == 3 for kd in r["kinds"])


# path -> (V, H, B, knobs, witness that the path was TAKEN): the smallest shapes of each path's own tests
FAST = {
    "one_launch": (100, 24, 512, {}, _one_launch),
    "thin": (784, 500, 20, dict(small_fused=0), _one_launch),           # (no GEMM launch either)
    "planes": (1024, 512, 256, dict(planes_min_work=0), _planes),
    "group_chain": (256, 200, 512, dict(gchain=1, small_fused=0), _group_chain),
}


@pytest.mark.parametrize("gauss", [False, True], ids=["rbm", "grbm"])
@pytest.mark.parametrize("path", list(FAST))
def test_saturated_step_on_the_fast_paths(eng, path, gauss):
    V, H, B, opts, taken = FAST[path]
    r = _step(eng, V, H, B, gauss, opts)
    assert taken(r), "not on the %s path: kinds %r" % (path, r["kinds"])
    _check_step("saturated %s %s" % (path, "GRBM" if gauss else "RBM"), r)


# ------------------------------------------------------------------ 2. eager Gibbs steps and monitoring kernels

SHAPE = (130, 70, 37)           # the shape of test_monitoring_costs_on_device


def _layer(eng, gauss, seed=5, stream=31):
    import mdbn_amd
    V, H, _ = SHAPE
    W, hb, vb = S.params(np.random.RandomState(seed), V, H, gauss)
    cls = mdbn_amd.GRBM if gauss else mdbn_amd.RBM
    rbm = cls(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(stream), engine=eng)
    rbm.W.set_value(W); rbm.hbias.set_value(hb); rbm.vbias.set_value(vb)
    return rbm, rbm_np.RBMState(V, H, W=W, hbias=hb, vbias=vb, gauss=gauss)


def _data(rs, gauss):
    V, _, B = SHAPE
    return rs.normal(size=(B, V)).astype(np.float32) if gauss else (rs.uniform(size=(B, V)) < 0.3).astype(np.float32)


@pytest.mark.parametrize("gauss", [False, True], ids=["rbm", "grbm"])
def test_eager_gibbs_steps_on_a_saturated_layer(hip_engine, gauss):
    """gibbs_hvh / gibbs_vhv: the six outputs each, with the tolerances of test_eager_gibbs_steps_and_rng_accounting (the
    pre-activations relative to max|pre|), and the exactness rules."""
    V, H, B = SHAPE
    rbm, st = _layer(hip_engine, gauss)
    rs = np.random.RandomState(1)
    tol_h, tol_v = 2e-6, 4e-6                                   # (V, H <= 1024)

    def u(step, cols):
        return philox_np.uniform(B, cols, rbm.theano_rng.seed, rbm.stream_id, step, 0, 0)

    def sigmoid_pass(tag, got_pre, got_mean, got_sample, o_pre, o_mean, uu, tol, tol_pre):
        assert all(np.isfinite(a).all() for a in (got_pre, got_mean, got_sample)), tag
        check("saturated eager %s mean" % tag, np.abs(got_mean - o_mean).max(), tol, "prob")
        check("saturated eager %s pre / max|pre|" % tag, np.abs(got_pre - o_pre).max() / max(1.0, np.abs(o_pre).max()), tol_pre)
        bad = got_sample != (uu < o_mean)
        assert np.all(np.abs(uu - o_mean)[bad] < 1e-6), tag
        S.check_saturation("eager " + tag, o_pre, got_mean, got_sample)

    # --- gibbs_hvh from a binary hidden state
    h0 = (rs.uniform(size=(B, H)) < 0.5).astype(np.float32)
    s0 = rbm._rng_step
    pre_v, v_mean, v_sample, pre_h, h_mean, h_sample = [a.get_value() for a in rbm.gibbs_hvh(h0)]
    o_pre_v, o_v_mean, _ = rbm_np.sample_v_given_h(st, h0.astype(np.float64), u(s0, V))
    if gauss:
        scale = max(1.0, np.abs(o_v_mean).max())
        assert np.abs(v_mean - o_v_mean).max() <= tol_v * scale and np.abs(pre_v - o_pre_v).max() <= 2 * tol_v * scale
        assert np.array_equal(v_sample, v_mean)                 # error_free: the sample IS the mean
        v_in = v_mean
    else:
        sigmoid_pass("hvh v", pre_v, v_mean, v_sample, o_pre_v, o_v_mean, u(s0, V), tol_v, 2 * tol_v)
        S.assert_bands("eager hvh v", [o_pre_v])
        v_in = v_sample
    o_pre_h, o_h_mean = rbm_np.propup(st, v_in.astype(np.float64))
    sigmoid_pass("hvh h", pre_h, h_mean, h_sample, o_pre_h, o_h_mean, u(s0 + 1, H), tol_h, 1e-5)
    hidden = [o_pre_h]

    # --- gibbs_vhv from data
    v0 = _data(rs, gauss)
    s1 = rbm._rng_step
    pre_h, h_mean, h_sample, pre_v, v_mean, v_sample = [a.get_value() for a in rbm.gibbs_vhv(v0)]
    o_pre_h, o_h_mean = rbm_np.propup(st, v0.astype(np.float64))
    sigmoid_pass("vhv h", pre_h, h_mean, h_sample, o_pre_h, o_h_mean, u(s1, H), tol_h, 1e-5)
    hidden.append(o_pre_h)
    h_in = h_mean if gauss else h_sample
    o_pre_v, o_v_mean, _ = rbm_np.sample_v_given_h(st, h_in.astype(np.float64), u(s1 + 1, V))
    if gauss:
        scale = max(1.0, np.abs(o_v_mean).max())
        assert np.abs(v_mean - o_v_mean).max() <= tol_v * scale and np.abs(pre_v - o_pre_v).max() <= 2 * tol_v * scale
    else:
        sigmoid_pass("vhv v", pre_v, v_mean, v_sample, o_pre_v, o_v_mean, u(s1 + 1, V), tol_v, 2 * tol_v)
        S.assert_bands("eager vhv v", [o_pre_v])
    S.assert_bands("eager hidden passes", hidden)


def _ladder_matrix(rs, rows, cols):
    """Every rung of the ladder +- U(0, 1), rung by rung along the rows (float32)."""
    rungs = np.asarray(S.LADDER)[np.arange(rows * cols) % len(S.LADDER)].reshape(rows, cols)
    return (rungs + rs.uniform(-1, 1, (rows, cols))).astype(np.float32)


@pytest.mark.parametrize("gauss", [False, True], ids=["rbm", "grbm"])
def test_reconstruction_cost_of_saturated_pre_activations(hip_engine, gauss):
    """get_reconstruction_cost on pre = ladder +- U(0, 1) with the target on either side of every element: for a Bernoulli
    layer t and 1 - t (each element is once right-side and once wrong-side saturated, a BCE term of up to 121), for a GRBM
    sigmoid(pre) -+ U(0.1, 1).  Relative 2e-6 as in test_monitoring_costs_on_device."""
    V, _, B = SHAPE
    rbm, st = _layer(hip_engine, gauss)
    rs = np.random.RandomState(5)
    pre = _ladder_matrix(rs, B, V)
    S.assert_bands("recon cost", [pre])
    if gauss:
        d = rs.uniform(0.1, 1, (B, V))
        targets = [(rbm_np.sigmoid(pre.astype(np.float64)) + s * d).astype(np.float32) for s in (-1, 1)]
    else:
        t = (rs.uniform(size=(B, V)) < 0.5).astype(np.float32)
        targets = [t, 1 - t]
    for side, v0 in enumerate(targets):
        got = rbm.get_reconstruction_cost(pre, v0)
        want = rbm_np.reconstruction_cost(st, pre.astype(np.float64), v0.astype(np.float64))
        assert np.isfinite(got)
        check("saturated recon cost %s side %d: rel" % ("GRBM" if gauss else "RBM", side), abs(got - want) / abs(want), 2e-6)


def _softplus32(x):
    x = x.astype(np.float32)
    return np.maximum(x, np.float32(0)) + np.log1p(np.exp(-np.abs(x)))


def _free_energy_twin(st, x, f32):
    """rbm.py:166-171 / :684-688 on float32 inputs: float64 throughout, or (f32) as csrc/mdbn_kernels.hip groups it: float32
    products and softplus, the row sums in float64, the result rounded to float32."""
    W, hb, vb = [np.asarray(a, dtype=np.float32) for a in (st.W, st.hbias, st.vbias)]
    if not f32:
        return rbm_np.free_energy(st, x.astype(np.float64))
    a = (x.astype(np.float32) @ W + hb).astype(np.float32)
    F = -_softplus32(a).sum(axis=1, dtype=np.float64)
    if st.gauss:
        F += 0.5 * ((x - vb).astype(np.float32).astype(np.float64) ** 2).sum(axis=1)
    else:
        F -= (x.astype(np.float64) * vb.astype(np.float64)).sum(axis=1)
    return F.astype(np.float32).astype(np.float64)


def _bound(gap, today):
    """4x the float32 share measured by the two restatements, or today's bound where that is the tighter one."""
    return min(4.0 * gap, today)


@pytest.mark.parametrize("gauss", [False, True], ids=["rbm", "grbm"])
def test_free_energy_of_a_saturated_layer(hip_engine, gauss):
    rbm, st = _layer(hip_engine, gauss)
    x = _data(np.random.RandomState(7), gauss)
    S.assert_bands("free energy", [x.astype(np.float64) @ st.W + st.hbias])
    F = rbm.free_energy(x).get_value().astype(np.float64)
    F64, F32 = _free_energy_twin(st, x, False), _free_energy_twin(st, x, True)
    gap = float(np.abs(F32 - F64).max())
    bound = _bound(gap, 1e-4 * np.abs(F64).max())
    print("free energy %s: max|F| %.1f, float32-vs-float64 gap of the restatement %.3e, bound %.3e, device %.3e"
          % ("GRBM" if gauss else "RBM", np.abs(F64).max(), gap, bound, np.abs(F - F64).max()))
    assert np.isfinite(F).all()
    check("saturated free energy %s: abs" % ("GRBM" if gauss else "RBM"), np.abs(F - F64).max(), bound, "free_energy")


def _pl_twin(fe, fe_flip, V, f32):
    """-mean(V softplus(fe - fe_flip)) (rbm.py:442) of float32 vectors: in float64, or with a float32 difference, softplus
    and sum."""
    if f32:
        tot = _softplus32(fe.astype(np.float32) - fe_flip.astype(np.float32)).sum(dtype=np.float32)
        return float(-(np.float32(V) * tot) / np.float32(fe.size))
    return float(-np.mean(V * rbm_np.softplus(fe.astype(np.float64) - fe_flip.astype(np.float64))))


def test_pl_cost_of_differences_on_the_ladder(hip_engine):
    """engine.pl_cost with fe - fe_flip = ladder +- U(0, 1) on free energies in the thousands."""
    V = SHAPE[0]
    rs = np.random.RandomState(3)
    n = 4 * len(S.LADDER) + 5
    fe = rs.normal(0, 2000, n).astype(np.float32)
    fe_flip = (fe - _ladder_matrix(rs, 1, n)[0]).astype(np.float32)
    S.assert_bands("pl_cost", [fe.astype(np.float64) - fe_flip])
    got = float(hip_engine.pl_cost(hip_engine.to_device(fe), hip_engine.to_device(fe_flip), V))
    want, w32 = _pl_twin(fe, fe_flip, V, False), _pl_twin(fe, fe_flip, V, True)
    gap = abs(w32 - want)
    bound = _bound(gap, 1e-4 * abs(want) + 1e-6)
    print("pl_cost: %.6f, float64 %.6f, gap of the restatement %.3e, bound %.3e, device %.3e" % (got, want, gap, bound, abs(got - want)))
    assert np.isfinite(got)
    check("saturated pl_cost: abs", abs(got - want), bound)


@pytest.mark.parametrize("gauss", [False, True], ids=["rbm", "grbm"])
def test_pseudo_likelihood_cost_of_a_saturated_layer(hip_engine, gauss):
    """get_pseudo_likelihood_cost over three bit positions; for the RBM the flipped bits' visible biases sit on the rungs
    -88, -9 and 16.5, so that softplus(F(x) - F(x_flip)) is saturated on either side."""
    V, H, B = SHAPE
    rbm, st = _layer(hip_engine, gauss)
    rs = np.random.RandomState(5)
    x = (rs.randint(0, 7, (B, V)) / 4.0 - 0.5).astype(np.float32)        # quarters, as test_monitoring_costs_on_device
    for step in range(3):
        i = rbm.bit_i_idx
        st.bit_i_idx = i
        got = rbm.get_pseudo_likelihood_cost(x)
        want = rbm_np.pseudo_likelihood_cost(st, x.astype(np.float64))
        xi = (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.float32)
        flip = xi.copy()
        flip[:, i] = 1 - xi[:, i]
        w32 = _pl_twin(_free_energy_twin(st, xi, True), _free_energy_twin(st, flip, True), V, True)
        gap = abs(w32 - want)
        bound = _bound(gap, 1e-4 * abs(want) + 1e-6)
        print("PL %s bit %d: %.6f, float64 %.6f, gap of the restatement %.3e, bound %.3e, device %.3e"
              % ("GRBM" if gauss else "RBM", i, got, want, gap, bound, abs(got - want)))
        assert np.isfinite(got)
        check("saturated pseudo-likelihood %s: abs" % ("GRBM" if gauss else "RBM"), abs(got - want), bound)
    assert rbm.bit_i_idx == 3
