"""The CD-step variants no fast path serves, on every GEMM family of the generic step, against the float64 oracle.

small_eligible / thin_eligible / planes_eligible and the group-chain test of csrc/mdbn_capi.hip refuse a step with a
persistent chain (PCD -- the default of RBM.training), with sample statistics (symbolic_grad=True) or with a noisy GRBM
(gauss + add_noise): it runs the generic body of cd_step_impl, whose run_affine picks a kernel family by shape.  Each variant
adds code that exists only there: the first propdown reads the caller's chain as a general f32 operand (six bf16 piece
products, not the three of a 0/1 operand), the last propup writes its sample into `persistent`; the last propdown of a
sample-statistics step writes the SAMPLE into rows B..2B of V2, feeds it upward and sums target - sample (colsum_kind 2).

Part 1 runs every variant on every family (the launch kinds prove which kernel ran), part 2 on shapes the one-launch, thin and
plane steps would otherwise take (the variant must fall back, bit for bit as with the fast path's knob off, and W's bf16 planes
must stay in step with W), part 3 trains through the Python surface.  Tolerances: DESIGN.md section 4 (tests/_margins.py).
One engine of this module's own; every knob set is reset to its default in `finally` (tests/_variants.py)."""
import contextlib
import io

import numpy as np
import pytest

from oracle import rbm_np
from oracle.philox_np import PhiloxDraws
from _margins import check
from _variants import (NO_FAST_PATH, PARAMS, VARIANTS, cd, family, forward, fused, options, oracle, pipe, run_variant, same,
                       verdict, w_planes_in_step)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(built_lib):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mdbn_amd
    return mdbn_amd.HipEngine()


@pytest.fixture()
def shadow(built_lib):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mdbn_amd
    import mdbn_amd.engine as E
    from _shadow import ShadowEngine
    prev = E._default_engine
    s = mdbn_amd.set_engine(ShadowEngine())
    rbm_np.FLIP_GAP["max"] = 0.0
    yield s
    E._default_engine = prev


# ------------------------------------------------------------------ 1. variant x kernel family

TILED_F32 = dict(stream_x6=0, skinny_gemm=0, gemm_bf16x6=0)
TILED_X6 = dict(stream_x6=0, skinny_gemm=0, x6_min_jobs=0, gemm_planes=0)


def _skinny_fused(kinds):
    return all(family(kd) == 1 and pipe(kd) == 0 and fused(kd) == 1 for kd in forward(kinds))


def _skinny_split(kinds):
    return all(family(kd) == 1 and pipe(kd) == 0 for kd in forward(kinds)) and any(fused(kd) == 0 for kd in forward(kinds))


def _stream(kinds):
    return all(family(kd) == 1 and pipe(kd) in (1, 2) for kd in forward(kinds))


def _tiled_f32_fused(kinds):
    return all(family(kd) == 0 and pipe(kd) == 0 and fused(kd) == 1 for kd in forward(kinds))


def _tiled_f32_slabs(kinds):
    return all(family(kd) == 0 and pipe(kd) == 0 and fused(kd) == 0 for kd in forward(kinds))


def _tiled_x6(kinds):
    return all(family(kd) == 0 and pipe(kd) in (1, 2) for kd in forward(kinds))


# family -> (V, H, B, knobs, what the forward launch kinds must show, runs on the bf16 pipe).  Every shape but 256 -> 128 is
# ragged (V, H no multiples of 4 or 32, B no multiple of 4 where the family allows: B = 100 is the issue's streaming shape).
# 250 -> 130: the LDS-tiled plan splits K from 256 on (gemm_min_splitk = 128), and only an unsplit pass fuses its epilogue.
FAMILIES = {
    "skinny_fused": (130, 70, 37, {}, _skinny_fused, False),
    "skinny_splitk": (2050, 70, 33, {}, _skinny_split, False),          # propup K = 2050 > skinny_fused_max_k
    "stream": (300, 130, 100, {}, _stream, True),
    "tiled_f32_fused": (250, 130, 99, TILED_F32, _tiled_f32_fused, False),
    "tiled_f32_slabs": (300, 130, 100, dict(TILED_F32, fused_epilogue=0), _tiled_f32_slabs, False),
    "tiled_x6": (256, 128, 128, TILED_X6, _tiled_x6, True),
    "tiled_x6_ragged": (250, 130, 99, TILED_X6, _tiled_x6, True),
}


def _check_kinds(name, fam, r):
    V, H, B, _, shows, bf16 = FAMILIES[fam]
    k, kinds = r["k"], r["kinds"]
    assert len(kinds) == 2 * k + 2 and [kd % 10 for kd in kinds] == [1] + [0, 1] * k + [3], (name, fam, kinds)
    assert all(kd < 2000 for kd in kinds) and shows(kinds), (name, fam, kinds)
    if bf16 and name == "pcd_frac":
        # the caller's chain may hold anything: six products; every later pass of the Bernoulli chain reads 0/1 samples
        assert pipe(kinds[1]) == 1, ("first propdown of a fractional chain", fam, kinds)
        assert all(pipe(kd) == 2 for kd in kinds[2:-1]), ("later passes of a Bernoulli chain", fam, kinds)
    if bf16 and name == "pcd_bin":
        assert pipe(kinds[1]) == 1, ("a caller's chain is never taken for 0/1", fam, kinds)


@pytest.mark.parametrize("fam", list(FAMILIES))
@pytest.mark.parametrize("name", list(VARIANTS))
def test_variant_on_every_gemm_family_against_forced_oracle(eng, name, fam):
    V, H, B, opts = FAMILIES[fam][:4]
    r = run_variant(eng, name, V, H, B, opts)
    _check_kinds(name, fam, r)
    oracle("variants %s" % fam, r)
    if name == "noise_grbm":
        # the noisy sample never feeds the chain (rbm.py:669): the same bits as the noiseless step on the same kernels
        gauss, k, _ = VARIANTS[name]
        plain = cd(eng, V, H, B, k, gauss, dict(opts, **NO_FAST_PATH))
        assert plain["kinds"] == r["kinds"], (fam, plain["kinds"], r["kinds"])
        same(r, plain, "add_noise vs the noiseless step (%s)" % fam)


@pytest.mark.parametrize("knob", ["stream_mi", "stream_ni"])
def test_fractional_chain_on_wider_stream_tiles(eng, knob):
    """64-row / 64 x 64 tiles of the streaming kernel split their fragments elsewhere: the six-product first propdown again."""
    V, H, B = FAMILIES["stream"][:3]
    r = run_variant(eng, "pcd_frac", V, H, B, {knob: 2})
    _check_kinds("pcd_frac", "stream", r)
    oracle("variants stream %s=2" % knob, r)


# ------------------------------------------------------------------ 2. fallback from the fast paths

# shape -> (V, H, B, knobs of the run, the fast path's knob).  The plane shape is the smallest whole-tile one whose three GEMMs
# all stay off the register-streaming kernels under the default limits (256 -> 128 at B = 128 plans skinny and is refused by
# mdbn_planes_eligible_ctx): about 70 us of GPU time per step, 134 M multiply-adds per pass for the float64 oracle.
FAST = {
    "one_launch": (100, 24, 512, {}, "small_fused"),
    "thin": (784, 500, 20, {}, "thin_fused"),
    "planes": (1024, 512, 256, dict(planes_min_work=0), "gemm_planes"),
}


@pytest.mark.parametrize("shape", list(FAST))
@pytest.mark.parametrize("name", list(VARIANTS))
def test_variant_falls_back_from_the_fast_path(eng, name, shape):
    V, H, B, opts, knob = FAST[shape]
    gauss, k, _ = VARIANTS[name]
    plain = cd(eng, V, H, B, k, gauss, opts)
    if shape == "planes":
        assert plain["eligible"] and plain["scratch_planes"], "not a plane shape: %r" % ((V, H, B),)
        assert plain["kinds"] and all(kd >= 2000 for kd in plain["kinds"]), plain["kinds"]
    else:
        assert plain["kinds"] == [], ("plain CD is not on the %s step" % shape, plain["kinds"])
    r = run_variant(eng, name, V, H, B, opts)
    assert len(r["kinds"]) == 2 * k + 2 and all(kd < 2000 for kd in r["kinds"]), (name, shape, r["kinds"])
    off = run_variant(eng, name, V, H, B, dict(opts, **{knob: 0}))
    assert off["kinds"] == r["kinds"], (name, shape, r["kinds"], off["kinds"])
    same(r, off, "%s with %s=0" % (name, knob))
    oracle("variants fallback %s" % shape, r)
    if shape == "planes":
        # the engine hands W's planes in (stale: a fresh W); the step re-splits them on entry whichever path it takes
        assert r["eligible"] and r["scratch_planes"], "the variant ran without plane buffers"
        assert r["planes_ok"] is True, "W's planes do not hold the split of W after the fallback step"
        assert off["planes_ok"] is None and not off["scratch_planes"]


# ------------------------------------------------------------------ 3. training through the Python surface

STREAM_KNOBS = {}
TILED_KNOBS = dict(stream_x6=0, skinny_gemm=0)


def _family_of_run(opts, kinds):
    fwd = forward(kinds)
    if opts:
        assert fwd and all(family(kd) == 0 for kd in fwd), kinds
    else:
        assert fwd and all(family(kd) == 1 and pipe(kd) in (1, 2) for kd in fwd), kinds


def _params_close(tag, rbm, st):
    for n in PARAMS:
        ref = getattr(st, n)
        check("variants %s: %s after a step / max" % (tag, n),
              np.abs(getattr(rbm, n).get_value() - ref).max() / max(1.0, np.abs(ref).max()), 2e-6, "update")


def _taps(eng, gauss, k, V, H, pcd):
    sc = eng.last_scratch
    th = sc.trace_h.cpu().numpy()[:k + 1 if pcd else k, :, :H]
    return th, None if gauss else sc.trace_v.cpu().numpy()[:, :, :V]


def _timed_step(eng, fn, k, **kw):
    """One call of a step function with the GEMM launches recorded: (cost, kinds of the CD step).  A PCD step is followed by
    the two free-energy GEMMs of its pseudo-likelihood monitor, which are not the step's."""
    eng.kernel_timing(True)
    try:
        c = float(fn(**kw))
        eng.synchronize()
        kinds = [kd for _, _, _, kd in eng.kernel_timing_detail()]
    finally:
        eng.kernel_timing(False)
    return c, kinds[:2 * k + 2]


@pytest.mark.parametrize("opts", [STREAM_KNOBS, TILED_KNOBS], ids=["stream", "tiled"])
def test_pcd_training_from_a_fractional_chain(eng, opts):
    """PCD-2 at 300 -> 130, B = 100 through get_cost_updates(persistent=chain): cd_step + apply_update, weight cost, momentum
    0.5 -> 0.9; every step replayed by the oracle along the device's taps, the chain after every step the oracle's."""
    import mdbn_amd
    V, H, B, N, k = 300, 130, 100, 300, 2
    rs = np.random.RandomState(17)
    data = (rs.uniform(size=(N, V)) < 0.3).astype(np.float32)
    chain0 = rs.uniform(size=(B, H)).astype(np.float32)
    hp = dict(lr=0.1, weightcost=2e-4)
    with options(eng, **opts):
        rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(123), theano_rng=mdbn_amd.RandomStreams(9),
                           engine=eng)
        st = rbm_np.RBMState(V, H, W=rbm.W.get_value())
        st.freeze_W0()
        st.persistent = chain0.astype(np.float64)
        chain = mdbn_amd.shared(chain0, engine=eng)
        _, up = rbm.get_cost_updates(k=k, batch_size=B, persistent=chain, **hp)
        fn = mdbn_amd.function(up, mdbn_amd.shared(data, engine=eng), data_parallel=None)
        eng.trace_chain = True
        try:
            for t in range(4):
                mom = 0.5 if t < 2 else 0.9
                idx = rs.permutation(N)[:B]
                c, kinds = _timed_step(eng, fn, k, indexes=idx, momentum=mom)
                _family_of_run(opts, kinds)
                if not opts and t == 0:
                    assert pipe(kinds[1]) == 1, ("first propdown of a fractional chain", kinds)
                want = rbm_np.cd_step(st, data[idx], PhiloxDraws(9, rbm.stream_id, t), k=k, batch_size=B, momentum=mom,
                                      persistent=True, forced=_taps(eng, False, k, V, H, True), **hp)
                np.testing.assert_allclose(c, want, rtol=2e-4, err_msg="pseudo-likelihood cost of step %d" % t)
                assert np.array_equal(up.persistent.get_value(), st.persistent), "chain diverged at step %d" % t
                _params_close("PCD training", rbm, st)
        finally:
            eng.trace_chain = False
    assert rbm.bit_i_idx == st.bit_i_idx == 4


@pytest.mark.parametrize("opts", [STREAM_KNOBS, TILED_KNOBS], ids=["stream", "tiled"])
@pytest.mark.parametrize("gauss", [False, True], ids=["rbm", "grbm"])
def test_symbolic_grad_training_teacher_forced(eng, gauss, opts):
    """symbolic_grad=True at 300 -> 130, B = 100, 3 steps of CD-2: teacher-forced, so the parameters hold the 2e-6 of every
    other training test (test_symbolic_grad_on_device follows its own chain and allows 2e-5)."""
    import mdbn_amd
    V, H, B, N, k = 300, 130, 100, 300, 2
    rs = np.random.RandomState(23)
    data = rs.normal(size=(N, V)).astype(np.float32) if gauss else (rs.uniform(size=(N, V)) < 0.4).astype(np.float32)
    cls = mdbn_amd.GRBM if gauss else mdbn_amd.RBM
    lr = 0.005 if gauss else 0.01
    with options(eng, **opts):
        rbm = cls(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(21), engine=eng)
        st = rbm_np.RBMState(V, H, W=rbm.W.get_value(), gauss=gauss)
        _, up = rbm.get_cost_updates(lr=lr, k=k, batch_size=B, symbolic_grad=True)
        fn = mdbn_amd.function(up, mdbn_amd.shared(data, engine=eng), data_parallel=None)
        eng.trace_chain = True
        try:
            for t in range(3):
                idx = rs.permutation(N)[:B]
                c, kinds = _timed_step(eng, fn, k, indexes=idx, momentum=0.5)
                _family_of_run(opts, kinds)
                want = rbm_np.cd_step(st, data[idx], PhiloxDraws(21, rbm.stream_id, t), lr=lr, k=k, momentum=0.5,
                                      symbolic_grad=True, forced=_taps(eng, gauss, k, V, H, False))
                check("variants symbolic-grad training: cost rel", abs(c - want) / abs(want), 1e-5)
        finally:
            eng.trace_chain = False
    _params_close("symbolic-grad training", rbm, st)


def test_w_planes_stay_in_step_through_pcd_steps_on_a_plane_shape(eng):
    """1024 -> 512 at B = 256 with planes_min_work = 0: two PCD steps (cd_step off the planes + apply_update) and then two
    plain CD steps of a second step function on the same RBM, which the plane path serves from the planes the PCD steps left:
    a stale plane set would put them far outside the oracle's 2e-6."""
    import mdbn_amd
    V, H, B, N, k = 1024, 512, 256, 600, 1
    rs = np.random.RandomState(29)
    data = (rs.uniform(size=(N, V)) < 0.3).astype(np.float32)
    chain0 = rs.uniform(size=(B, H)).astype(np.float32)
    with options(eng, planes_min_work=0):
        assert eng.plane_shape(B, V, H, V, H), "not a plane shape"
        rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(123), theano_rng=mdbn_amd.RandomStreams(13),
                           engine=eng)
        st = rbm_np.RBMState(V, H, W=rbm.W.get_value())
        st.persistent = chain0.astype(np.float64)
        x = mdbn_amd.shared(data, engine=eng)
        _, up_pcd = rbm.get_cost_updates(lr=0.05, k=k, batch_size=B, persistent=mdbn_amd.shared(chain0, engine=eng))
        _, up_cd = rbm.get_cost_updates(lr=0.05, k=k, batch_size=B)
        fn_pcd = mdbn_amd.function(up_pcd, x, data_parallel=None)
        fn_cd = mdbn_amd.function(up_cd, x, data_parallel=None)
        eng.trace_chain = True
        try:
            for t in range(4):
                pcd = t < 2
                idx = rs.permutation(N)[:B]
                c, kinds = _timed_step(eng, fn_pcd if pcd else fn_cd, k, indexes=idx, momentum=0.5)
                assert eng.last_scratch.planes is not None, "the step ran without plane buffers"
                if pcd:
                    assert kinds and all(kd < 2000 for kd in kinds), (t, kinds)
                else:
                    assert kinds and all(kd >= 2000 for kd in kinds), (t, kinds)
                want = rbm_np.cd_step(st, data[idx], PhiloxDraws(13, rbm.stream_id, t), lr=0.05, k=k, batch_size=B, momentum=0.5,
                                      persistent=pcd, forced=_taps(eng, False, k, V, H, pcd))
                if pcd:
                    np.testing.assert_allclose(c, want, rtol=2e-4, err_msg="pseudo-likelihood cost of step %d" % t)
                    assert np.array_equal(up_pcd.persistent.get_value(), st.persistent), "chain diverged at step %d" % t
                else:
                    check("variants plane shape: cost rel", abs(c - want) / abs(want), 1e-5)
                _params_close("plane shape", rbm, st)
                assert w_planes_in_step(eng, rbm.W.tensor), "W's planes are not the split of W after step %d" % t
        finally:
            eng.trace_chain = False


def test_rbm_training_default_is_pcd_on_the_streaming_kernel(shadow):
    """RBM.training with its default persistent=True at B = 100 on 300 -> 130: two epochs, every step replayed by the shadow."""
    import mdbn_amd
    V, H, N, B, k = 300, 130, 300, 100, 2
    rs = np.random.RandomState(0)
    data = (rs.uniform(size=(N, V)) < 0.3).astype(np.float32)
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(123), theano_rng=mdbn_amd.RandomStreams(5),
                       engine=shadow)
    np.random.seed(4)                                        # the reference shuffles with the global state (utils.py:62)
    shadow.kernel_timing(True)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            history = rbm.training(data, data[:30], training_epochs=2, batch_size=B, learning_rate=0.1, k=k,
                                   initial_momentum=0.6, final_momentum=0.9, weightcost=2e-4)
        shadow.synchronize()
        kinds = [kd for _, _, _, kd in shadow.kernel_timing_detail()]
    finally:
        shadow.kernel_timing(False)
    steps = 2 * (N // B)
    assert len(history) == 2 and shadow.steps == steps and len(shadow.pl_costs) == steps
    # (besides the steps' launches: the exact-f32 GEMMs of the free energies behind the monitor and the gap, kind 1)
    assert not any(kd >= 2000 for kd in kinds), kinds
    assert sum(family(kd) == 1 and pipe(kd) in (1, 2) for kd in forward(kinds)) == steps * (2 * k + 1), kinds
    per_epoch = np.array(shadow.pl_costs).reshape(2, N // B).mean(axis=1)
    np.testing.assert_allclose([c for c, _ in history], per_epoch, rtol=2e-4)
    assert rbm.bit_i_idx == steps % V
    verdict(shadow, "RBM.training default PCD-2 (300->130, B = 100)", [rbm], stat_tol=1e-5, param_tol=5e-6)
