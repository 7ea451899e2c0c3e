"""Option "slab_tail" (csrc/mdbn_planes.hip, gemm_planes_slabtail_kernel): the split-K propup on planes walks its last
stages quarter-major and stores each quarter's partials while the other quarters' MFMAs run.  Every accumulator still sums
the same stage sums in the same order, so everything downstream must be BIT FOR BIT what option 0 gives.

The propup on planes is reached through the CD step (run_affine_planes serves nothing else): a CD-1 step of a GRBM runs it
twice from f32 operands (three planes: v0, then the reconstruction's mean), a CD-1 step of a Bernoulli RBM once from three
planes and once from the 0/1 sample plane (one plane).  Shapes: one output tile or two (B = 128; H = 128, 256), and V with
"gemm_min_splitk" chosen so that plan_forward (mdbn_capi.hip: try_bf16x6) gives the stages per workgroup wanted below --
kchunk = round_up(ceil(V / sk), 32) with sk = min(256 / tiles, V / gemm_min_splitk); at the library's own 128 no workgroup
has fewer than four stages, so the knob is part of the case:

    stages  gemm_min_splitk  V      slabs   why
    1       32               1024   32      fewer stages than the tail (T = 2): a one-stage tail at stage 0
    2       64               1024   16      the whole workgroup is the tail (a T = 3 build: fewer stages than the tail)
    3       96               768    8       the tail begins at stage 1: hand-over behind an odd body (T = 3: at stage 0)
    4       128              1024   8       the tail begins at stage 2: hand-over behind an even body (T = 3: an odd one)
    5       160              1280   8       a real body in front of the tail, odd length
    16      512              2048   4       the headline workgroup's stage count, even body length

A timing record carries the kind of the launch and its M N K, not its split: kinds 2101 / 2201 are the plane propup with
fused == 0 from three planes / one plane, i.e. the slab kernel + epilogue launch, which run_affine_planes only issues for a
split plan; the split itself (slabs, stages) is asserted on _propup_plan below, the arithmetic of plan_forward, fed with the
very dict of plan knobs that _plan_knobs sets on the engine.  Under option 1 such a launch on the 16x16x32 shape IS
gemm_planes_slabtail_kernel: the library refuses the launch (an error from the step) where that kernel cannot take it, and
has no path back to the other one."""
import contextlib

import numpy as np
import pytest
import torch

from _knobs import KNOBS
from oracle import rbm_np

pytestmark = pytest.mark.gpu

B = 128
CASES = [(1, 32, 1024, 32), (2, 64, 1024, 16), (3, 96, 768, 8), (4, 128, 1024, 8), (5, 160, 1280, 8), (16, 512, 2048, 4)]
_DEFAULTS = {name: KNOBS[name]["default"] for name in ("gemm_min_splitk", "x6_min_jobs", "skinny_gemm")}      # the library's own


def _propup_plan(rows, He, V, knobs):
    """(slabs, stages per workgroup) of plan_forward(rows, He, V) on the bf16x6 tiling under the plan knobs `knobs`."""
    tiles = (rows // 128) * (He // 128)
    sk = min(max(1, 256 // tiles), max(1, V // knobs["gemm_min_splitk"]))
    assert tiles * sk >= knobs["x6_min_jobs"], "too few jobs for the bf16x6 plan"
    kchunk = (-(-V // sk) + 31) // 32 * 32
    sk = -(-V // kchunk)
    assert kchunk * sk == V
    return sk, kchunk // 32


@contextlib.contextmanager
def _plan_knobs(eng, **knobs):
    """Every knob plan_forward reads set to ONE dict for the length of a test -- the dict _propup_plan gets too -- and back to
    the library's defaults afterwards, so no test runs under what another one left."""
    knobs = dict(_DEFAULTS, **knobs)
    try:
        for name, value in knobs.items():
            eng.set_option(name, value)
        yield knobs
    finally:
        for name, value in _DEFAULTS.items():
            eng.set_option(name, value)
        eng.set_option("slab_tail", 1)


def _step(eng, gauss, V, H, tail, W, hb, vb, x):
    """One CD-1 step with the float32 copies and the chain taps on; everything the two propups (and what follows them) wrote."""
    from mdbn_amd import RngAddr
    eng.set_option("slab_tail", tail)
    assert eng.plane_shape(B, V, H, V, H), "not on the plane path: %r" % ((B, V, H),)
    dW, dhb, dvb, dx = [eng.to_device(a) for a in (W, hb, vb, x)]
    keep, eng.keep_f32, eng.trace_chain = eng.keep_f32, True, True
    eng.kernel_timing(True)
    try:
        stats, sc = eng.cd_step(dx, None, dW, dhb, dvb, gauss, 1, RngAddr(11, 1, 2, 0, 0))
        eng.synchronize()
        records = [(kind, alg) for _, alg, _, kind in eng.kernel_timing_detail()]
        assert sc.planes is not None
        # the plane scratch is [X2 planes: 6 B V | P2 planes: 6 B H | h sample plane: B H | v sample plane: B V]; a GRBM step
        # never writes the last block (its chain runs on the means), and the buffer is not initialised
        written = 6 * B * V + 7 * B * H + (0 if gauss else B * V)
        out = dict(stats=stats, P2=sc.P2, V2=sc.V2, hs=sc.hs, planes=sc.planes[:written], trace_h=sc.trace_h)
        if not gauss:
            out["trace_v"] = sc.trace_v
        out = {k: v.detach().clone().cpu().numpy() for k, v in out.items()}
    finally:
        eng.kernel_timing(False)
        eng.keep_f32, eng.trace_chain = keep, False
    return out, records


@pytest.mark.parametrize("gauss", [True, False], ids=["grbm", "rbm"])
@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("stages,min_splitk,V,slabs", CASES, ids=["nt%d" % c[0] for c in CASES])
def test_propup_with_slab_tail_is_bitwise_option_0_and_meets_the_oracle(hip_engine, stages, min_splitk, V, slabs, H, gauss):
    with _plan_knobs(hip_engine, gemm_min_splitk=min_splitk, x6_min_jobs=0, skinny_gemm=0) as knobs:
        assert _propup_plan(B, H, V, knobs) == (slabs, stages)
        _propup_case(hip_engine, V, H, gauss)


def _propup_case(eng, V, H, gauss):
    rs = np.random.RandomState(7)
    W = rbm_np.init_W(rs, V, H, np.float32)
    hb, vb = rs.normal(0, 0.2, H).astype(np.float32), rs.normal(0, 0.2, V).astype(np.float32)
    x = rs.normal(size=(B, V)).astype(np.float32) if gauss else (rs.uniform(size=(B, V)) < 0.3).astype(np.float32)
    ref, rec0 = _step(eng, gauss, V, H, 0, W, hb, vb, x)
    got, rec1 = _step(eng, gauss, V, H, 1, W, hb, vb, x)
    # the split-K plane propup ran, on this shape: twice from three planes (GRBM), once from three and once from one (RBM)
    flop = 2.0 * B * H * V
    for rec in (rec0, rec1):
        kinds = [kind for kind, _ in rec]
        assert kinds.count(2101) == (2 if gauss else 1) and kinds.count(2201) == (0 if gauss else 1), kinds
        assert all(alg == flop for kind, alg in rec if kind in (2101, 2201)), rec
        assert all(kind >= 2000 for kind in kinds), kinds                       # plane GEMMs only
    # means, samples, planes and bias partials (s_h in the statistics), and all that was computed from them
    for key in ref:
        assert np.array_equal(ref[key].view(np.uint32) if ref[key].dtype == np.float32 else ref[key],
                              got[key].view(np.uint32) if got[key].dtype == np.float32 else got[key]), key
    # float64 oracle on the operands the device used (tolerance of test_plane_step_against_oracle_teacher_forced)
    st = rbm_np.RBMState(V, H, W=W, hbias=hb, vbias=vb, gauss=gauss)
    _, ph = rbm_np.propup(st, x.astype(np.float64))
    assert np.abs(got["P2"][:B, :H] - ph).max() <= 2e-6
    v_in = got["V2"][B:2 * B, :V] if gauss else got["trace_v"].reshape(-1, B, got["trace_v"].shape[-1])[0][:, :V]
    _, nh = rbm_np.propup(st, v_in.astype(np.float64))
    assert np.abs(-got["P2"][B:2 * B, :H] - nh).max() <= 2e-6
    if not gauss:
        assert set(np.unique(v_in)) <= {0.0, 1.0}


@pytest.mark.parametrize("gauss", [True, False], ids=["grbm", "rbm"])
def test_three_cd1_steps_with_slab_tail_are_bitwise_option_0(hip_engine, gauss):
    """Three full CD-1 training steps at the smallest step shape of the plane tests (1024 -> 512, B = 256) under the library's
    own plan knobs, set here: propup split eight ways, four stages per workgroup.  Parameters, speeds and costs."""
    from test_gpu_planes import _run_steps
    V, H, Bs = 1024, 512, 256
    runs = {}
    with _plan_knobs(hip_engine) as knobs:
        assert _propup_plan(Bs, H, V, knobs) == (8, 4)
        for tail in (0, 1):
            hip_engine.set_option("slab_tail", tail)
            hip_engine.kernel_timing(True)
            try:
                runs[tail] = _run_steps(hip_engine, gauss, True, V, H, Bs, 1, steps=3)[0]
                hip_engine.synchronize()
                records = [(kind, alg) for _, alg, _, kind in hip_engine.kernel_timing_detail()]
            finally:
                hip_engine.kernel_timing(False)
            kinds = [kind for kind, _ in records]
            assert kinds.count(2101) == (6 if gauss else 3) and kinds.count(2201) == (0 if gauss else 3), kinds
            assert all(alg == 2.0 * Bs * H * V for kind, alg in records if kind in (2101, 2201)), records
    for key in runs[0]:
        assert np.array_equal(runs[0][key].view(np.uint32), runs[1][key].view(np.uint32)), key
