"""The 64-deep form of the narrow one-plane propdown kernel (csrc/mdbn_planes.hip, gemm_planes_kernel<..., BN = 64, KD = 64>;
LDS image: csrc/mdbn_planes_image.h, tests/test_narrow_deep_image.py).  Every accumulator sums the same products in the same
order as under 32-deep stages, so everything a step computes must be BIT FOR BIT what the 32-deep form gives.

The form has no option name: a context reads MDBN_NARROW_DEEP from the process environment ONCE, when it is created.  Two
engines live side by side here, one created with the variable at 1 and one with it at 0; what a context sent to the deep
form is counted by the library (mdbn_narrow_deep_launches), so a quiet return to the other form fails the test.

Shapes: batch 512 and V = 4096 keep propdown's 128 x 128 plan at 128 tiles and two splits, which is what sends it to
128 x 64 tiles; the reduction runs over H = 256, 512, 1024: 4, 8 and 16 deep stages (the three-slot ring wraps at 4).
H = 384 (6 deep stages, a whole number of turns of the ring) is NOT a plane shape at this batch and V, under any value of
"gemm_min_splitk": its propup has 12 tiles, plan_forward (mdbn_capi.hip: try_bf16x6) asks for min(21, 4096 / min_splitk)
slices, and propdown's two-way split needs min_splitk <= 192, i.e. 21 slices of 224 -- which do not add up to 4096, so
plane_plan refuses the layer (test_h384_at_the_headline_batch_is_not_a_plane_shape keeps that in view).  Six deep stages are
reached at B = 384, V = 3072, H = 384 under "gemm_min_splitk" = 192 instead: propup 9 tiles x 16 slices of 192, propdown 72
tiles x 2 slices of 192 (144 narrow tiles), statistics 72 tiles x 3 slices of 256.
H = 128 under "gemm_min_splitk" = 64 still takes narrow tiles but is below the 256 the deep form asks for: it must stay on
32-deep stages in both engines.  The plane path is forced on these small layers by "planes_min_work" = 0."""
import contextlib
import os

import numpy as np
import pytest

from oracle import rbm_np
from oracle.philox_np import PhiloxDraws

pytestmark = pytest.mark.gpu

# (B, V, H, "gemm_min_splitk"): 4, 8, 16 and 6 deep stages
CASES = [(512, 4096, 256, 128), (512, 4096, 512, 128), (512, 4096, 1024, 128), (384, 3072, 384, 192)]
IDS = ["H%d" % c[2] for c in CASES]
ENV = "MDBN_NARROW_DEEP"


@pytest.fixture(scope="module")
def engines(built_lib):
    """(engine created with the deep form on, engine created with it off)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mdbn_amd
    before = os.environ.get(ENV)
    made = []
    try:
        for flag in ("1", "0"):
            os.environ[ENV] = flag
            eng = mdbn_amd.HipEngine()
            eng.keep_f32 = True
            eng.set_planes_min_work(0)
            made.append(eng)
    finally:
        if before is None:
            del os.environ[ENV]
        else:
            os.environ[ENV] = before
    return tuple(made)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@contextlib.contextmanager
def _min_splitk(engs, value):
    try:
        for eng in engs:
            eng.set_option("gemm_min_splitk", value)
        yield
    finally:
        for eng in engs:
            eng.set_option("gemm_min_splitk", 128)          # the library's own


def _operands(B, V, H, gauss, seed=7):
    rs = np.random.RandomState(seed)
    W = rbm_np.init_W(rs, V, H, np.float32)
    hb, vb = rs.normal(0, 0.2, H).astype(np.float32), rs.normal(0, 0.2, V).astype(np.float32)
    x = rs.normal(size=(B, V)).astype(np.float32) if gauss else (rs.uniform(size=(B, V)) < 0.3).astype(np.float32)
    return W, hb, vb, x


def _step(eng, gauss, k, W, hb, vb, x):
    """One CD-k step with the float32 copies and the chain taps on -> (everything it wrote, timing records, launches the
    step sent to the deep form)."""
    from mdbn_amd import RngAddr
    (B, V), H = x.shape, W.shape[1]
    assert eng.plane_shape(B, V, H, V, H), "not on the plane path: %r" % ((B, V, H),)
    dW, dhb, dvb, dx = [eng.to_device(a) for a in (W, hb, vb, x)]
    eng.trace_chain = True
    eng.kernel_timing(True)
    deep0 = eng.narrow_deep_launches()
    try:
        stats, sc = eng.cd_step(dx, None, dW, dhb, dvb, gauss, k, RngAddr(11, 1, 2, 0, 0))
        eng.synchronize()
        records = [(kind, alg) for _, alg, _, kind in eng.kernel_timing_detail()]
        assert sc.planes is not None
        # plane scratch: [X2 planes: 6 B V | P2 planes: 6 B H | h sample plane: B H | v sample plane: B V]; a GRBM step never
        # writes the last block
        written = 6 * B * V + 7 * B * H + (0 if gauss else B * V)
        out = dict(stats=stats, P2=sc.P2, V2=sc.V2, hs=sc.hs, planes=sc.planes[:written], trace_h=sc.trace_h)
        if not gauss:
            out["trace_v"] = sc.trace_v
        out = {key: v.detach().clone().cpu().numpy() for key, v in out.items()}
    finally:
        eng.kernel_timing(False)
        eng.trace_chain = False
    return out, records, eng.narrow_deep_launches() - deep0


def _assert_propdown_ran(records, deep_count, flop, k, deep):
    kinds = [kind for kind, _ in records]
    assert kinds.count(2210) == k, kinds                          # 2210: the fused propdown on 128 x 64 tiles, one plane of A
    assert all(alg == flop for kind, alg in records if kind == 2210), records
    assert deep_count == (k if deep else 0), (deep_count, deep)


@pytest.mark.parametrize("gauss", [True, False], ids=["grbm", "rbm"])
@pytest.mark.parametrize("B,V,H,min_splitk", CASES, ids=IDS)
def test_one_propdown_is_bitwise_the_32_deep_form(engines, B, V, H, min_splitk, gauss):
    """A CD-1 step has one propdown, from the 0/1 hidden sample plane.  Its outputs -- the reconstruction's mean (float32 copy
    in V2 and the three planes in the X2 block of the plane scratch), the cost total and the column sums s_v in the packed
    statistics -- and everything computed from them are the same bits in both engines."""
    deep, flat = engines
    ops = _operands(B, V, H, gauss)
    with _min_splitk(engines, min_splitk):
        got, rec1, n1 = _step(deep, gauss, 1, *ops)
        ref, rec0, n0 = _step(flat, gauss, 1, *ops)
    _assert_propdown_ran(rec1, n1, 2.0 * B * V * H, 1, True)
    _assert_propdown_ran(rec0, n0, 2.0 * B * V * H, 1, False)
    for key in ref:
        assert np.array_equal(_bits(ref[key]), _bits(got[key])), key
    if not gauss:       # the probabilities against float64 on the hidden samples the device drew
        W, hb, vb, x = ops
        st = rbm_np.RBMState(V, H, W=W, hbias=hb, vbias=vb, gauss=False)
        h0 = got["trace_h"].reshape(-1, B, got["trace_h"].shape[-1])[0][:, :H]
        assert set(np.unique(h0)) <= {0.0, 1.0}
        _, nv = rbm_np.propdown(st, h0.astype(np.float64))
        assert np.abs(got["V2"][B:2 * B, :V] - nv).max() <= 2e-6


@pytest.mark.parametrize("gauss", [True, False], ids=["grbm", "rbm"])
def test_a_reduction_below_256_keeps_the_32_deep_form(engines, gauss):
    """H = 128 split two ways (gemm_min_splitk = 64) takes narrow tiles with K = 128: kind 2210 runs, in neither engine on
    64-deep stages, and the two engines agree."""
    B, V, H = 512, 4096, 128
    ops = _operands(B, V, H, gauss)
    outs = []
    with _min_splitk(engines, 64):
        for eng in engines:
            out, rec, n = _step(eng, gauss, 1, *ops)
            _assert_propdown_ran(rec, n, 2.0 * B * V * H, 1, False)
            outs.append(out)
    for key in outs[0]:
        assert np.array_equal(_bits(outs[0][key]), _bits(outs[1][key])), key


def test_h384_at_the_headline_batch_is_not_a_plane_shape(engines):
    """(See the module docstring: every "gemm_min_splitk" that lets propdown split two ways.)  Should the planner come to
    accept it, it belongs in CASES."""
    for min_splitk in (64, 128, 192):
        with _min_splitk(engines, min_splitk):
            assert not engines[0].plane_shape(512, 4096, 384, 4096, 384), min_splitk


@pytest.mark.parametrize("gauss", [True, False], ids=["grbm", "rbm"])
@pytest.mark.parametrize("B,V,H,min_splitk", CASES, ids=IDS)
def test_three_cd1_steps_are_bitwise_the_32_deep_form(engines, B, V, H, min_splitk, gauss):
    """Three CD-1 training steps: parameters, speeds and costs."""
    from test_gpu_planes import _run_steps
    runs = []
    for eng, is_deep in zip(engines, (True, False)):
        eng.kernel_timing(True)
        deep0 = eng.narrow_deep_launches()
        try:
            with _min_splitk([eng], min_splitk):
                runs.append(_run_steps(eng, gauss, True, V, H, B, 1, steps=3)[0])
            eng.synchronize()
            records = [(kind, alg) for _, alg, _, kind in eng.kernel_timing_detail()]
        finally:
            eng.kernel_timing(False)
        _assert_propdown_ran(records, eng.narrow_deep_launches() - deep0, 2.0 * B * V * H, 3, is_deep)
    for key in runs[0]:
        assert np.array_equal(_bits(runs[0][key]), _bits(runs[1][key])), key


@pytest.mark.parametrize("B,V,H,min_splitk", CASES, ids=IDS)
def test_deep_step_against_oracle_teacher_forced(engines, B, V, H, min_splitk):
    """One CD-2 step of a Bernoulli RBM in the deep engine with the chain taps on, the float64 oracle following the device:
    the tolerances of test_gpu_planes.py::test_plane_step_against_oracle_teacher_forced."""
    eng, k = engines[0], 2
    W, hb, vb, x = _operands(B, V, H, False, seed=3)
    with _min_splitk([eng], min_splitk):
        out, records, n = _step(eng, False, k, W, hb, vb, x)
    _assert_propdown_ran(records, n, 2.0 * B * V * H, k, True)
    st = rbm_np.RBMState(V, H, W=W, hbias=hb, vbias=vb, gauss=False)
    v0 = x.astype(np.float64)
    ph, _, chain, flips = rbm_np.cd_chain_forced(st, v0, PhiloxDraws(11, 1, 2, 0), k, out["trace_h"], out["trace_v"])
    S_o, s_h_o, s_v_o = rbm_np.cd_statistics(v0, ph, chain[1], chain[4])
    d = out["stats"]
    S, s_h, s_v = d[:V * H].reshape(V, H), d[V * H:V * H + H], d[V * H + H:V * H + H + V]
    assert np.abs(S - S_o).max() <= 1e-5 * np.abs(S_o).max()
    assert np.abs(s_h - s_h_o).max() <= 1e-5 * max(1.0, np.abs(s_h_o).max())
    assert np.abs(s_v - s_v_o).max() <= 1e-5 * max(1.0, np.abs(s_v_o).max())
    assert np.abs(out["P2"][:B] - ph).max() <= 2e-6
    assert np.abs(out["V2"][B:2 * B] - chain[1]).max() <= 2e-6        # the reconstruction's mean: the last propdown
    assert flips <= 3
