"""Option "slab_tail" on the statistics launch (csrc/mdbn_planes.hip, gemm_planes_statstail_kernel): the fused-update
statistics GEMM of the single-device step, where its loader waves apply the parameter half early, walks its last two stages
quarter-major, hands the finished tile to the loader waves in two halves and stores the first half's new speed while the
second half's MFMAs run.  Every accumulator sums the same products in the same order and the speed is formed by the same
functions on the same operands, so three training steps must be BIT FOR BIT what option 0 gives -- and what the separate
update kernel gives ("fused_update" 0: the independent reference).

Three CD-1 steps through the Python step function, momentum 0.5 (the old speed matters), the plane path forced as
test_gpu_planes._run_steps forces it, "gemm_min_splitk" 4096 so that the statistics GEMM of these small layers is one
unsplit launch (with "x6_min_jobs" 0 and "skinny_gemm" 0, without which so few tile jobs leave the plane path).  Cases:

    B = 256   16 stages, two W chunks per stage in the loader's chunk phase
    B = 384   24 stages, one chunk per stage
    B = 128   8 stages: the early parameter half is off, the launch stays on gemm_planes_kernel
    1024 -> 512 and 512 -> 1024: both branches of the tile order (tiles_m > tiles_n and the reverse)
    2048 -> 1024: 128 workgroups, few enough rows of the next minibatch per workgroup for the gather-ahead to run
    GRBM (lambda_2 decay) and Bernoulli RBM (weight cost on the frozen snapshot W0: the es.w0 operand)
    each with and without next_indexes

Preconditions, on both option arms: every step has exactly one statistics record and it is the fused-update kind (2123, what
the headline shape gives); the gather-ahead ran exactly where the library's rule (mdbn_capi.hip, planes_statistics:
set_gather_ahead) allows it for a named next minibatch.  That rule needs the early parameter half (B >= 192), at most four
(row, 256-octet pass) units per workgroup and enough stages; it excludes 1024 -> 512 and 512 -> 1024 at these batch sizes
(32 workgroups, 8 or 12 rows each), which is why the 2048 -> 1024 layer is here: there the hint must have been taken."""
import numpy as np
import pytest
import torch

from _knobs import KNOBS

pytestmark = pytest.mark.gpu

STEPS = 3
STATS_FUSED, STATS_UNFUSED = 2123, 2103      # 2000 + 100 (three planes) + 10 * fused + 2 * LAY_MN + LAY_MN
LAYERS = [(1024, 512), (512, 1024), (2048, 1024)]
# plan knobs of the test: forward passes and statistics GEMM unsplit (one to 128 tile jobs each), still on the bf16x6 tiling the
# plane path follows ("x6_min_jobs" 0, "skinny_gemm" 0: as test_gpu_slab_tail sets them for its small layers)
PLAN = dict(gemm_min_splitk=4096, x6_min_jobs=0, skinny_gemm=0)


def _ahead_expected(V, H, B):
    """planes_statistics' rule for the gather-ahead of a named next minibatch (fused update, early parameter half)."""
    nt, nwg = 2 * B // 32, (V // 128) * (H // 128)
    if nt < 12:
        return False
    rpw, passes = -(-B // nwg), -(-(V // 8) // 256)
    return rpw * passes <= 4 and 16 // (1 if nt >= 20 else 2) + 4 + 1 <= nt - 3


def _run(eng, gauss, V, H, B, hint):
    """STEPS training steps; (everything the steps wrote, statistics kinds per step, gather-ahead taken per step)."""
    import mdbn_amd
    assert eng.plane_shape(B, V, H, V, H), "test shape is not on the plane path: %r" % ((B, V, H),)
    rs = np.random.RandomState(3)
    N = 4 * B
    data = rs.normal(size=(N, V)).astype(np.float32) if gauss else (rs.uniform(size=(N, V)) < 0.3).astype(np.float32)
    cls = mdbn_amd.GRBM if gauss else mdbn_amd.RBM
    rbm = cls(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(123), theano_rng=mdbn_amd.RandomStreams(5), engine=eng)
    hp = dict(lr=0.001, lambda_2=0.1) if gauss else dict(lr=0.05, weightcost=2e-4)
    _, up = rbm.get_cost_updates(k=1, batch_size=B, **hp)
    assert gauss or up.W0 is not None, "the Bernoulli case is meant to carry a frozen W0"
    fn = mdbn_amd.function(up, mdbn_amd.shared(data, engine=eng), data_parallel=None)
    batches = [eng.index_tensor(rs.permutation(N)[:B]) for _ in range(STEPS + 1)]
    costs, kinds, ahead = [], [], []
    for t in range(STEPS):
        eng.kernel_timing(True)
        try:
            costs.append(float(fn(indexes=batches[t], momentum=0.5, next_indexes=batches[t + 1] if hint else None)))
            eng.synchronize()
            kinds.append([kind for _, _, _, kind in eng.kernel_timing_detail() if kind % 10 == 3 and kind >= 2000])
        finally:
            eng.kernel_timing(False)
        ahead.append(eng.last_scratch.ahead is not None)
    wp, valid = eng.w_planes(rbm.W.tensor)
    assert wp is not None and valid
    out = dict(costs=np.array(costs, dtype=np.float32), W=rbm.W.get_value(), Ws=rbm.W_speed.get_value(),
               hb=rbm.hbias.get_value(), hbs=rbm.hbias_speed.get_value(), vb=rbm.vbias.get_value(),
               vbs=rbm.vbias_speed.get_value(), planes=wp.detach().clone().cpu().numpy())
    return out, kinds, ahead


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("hint", [False, True], ids=["nohint", "hint"])
@pytest.mark.parametrize("gauss", [True, False], ids=["grbm", "rbm"])
@pytest.mark.parametrize("B", [256, 384, 128])
@pytest.mark.parametrize("V,H", LAYERS, ids=["%dx%d" % l for l in LAYERS])
def test_three_steps_with_the_statistics_tail_are_bitwise_option_0_and_the_separate_update(hip_engine, V, H, B, gauss, hint):
    eng = hip_engine
    keep = eng.keep_f32
    runs = {}
    try:
        eng.keep_f32 = False                # the product default: the gather-ahead needs it
        eng.set_option("gemm_planes", 1)
        eng.set_option("planes_mfma", 16)
        eng.set_option("stream_x6", 0)
        for name, value in PLAN.items():
            eng.set_option(name, value)
        for arm, (tail, fused) in dict(opt0=(0, 1), opt1=(1, 1), separate=(1, 0)).items():
            eng.set_option("slab_tail", tail)
            eng.set_option("fused_update", fused)
            runs[arm], kinds, ahead = _run(eng, gauss, V, H, B, hint)
            want = STATS_FUSED if fused else STATS_UNFUSED
            assert kinds == [[want]] * STEPS, (arm, kinds)
            if fused:
                assert ahead == [hint and _ahead_expected(V, H, B)] * STEPS, (arm, ahead)
    finally:
        eng.set_option("slab_tail", 1)
        eng.set_option("fused_update", 1)
        for name in PLAN:
            eng.set_option(name, KNOBS[name]["default"])
        eng.set_option("stream_x6", 2)
        eng.keep_f32 = keep
    for arm in ("opt1", "separate"):
        for key in runs["opt0"]:
            assert np.array_equal(_bits(runs["opt0"][key]), _bits(runs[arm][key])), (arm, key)


def test_the_gather_ahead_cases_are_real():
    """The rule as this file mirrors it: on at 2048 -> 1024 for B = 256 and 384, off for the two small layers and at B = 128."""
    assert _ahead_expected(2048, 1024, 256) and _ahead_expected(2048, 1024, 384)
    assert not any(_ahead_expected(V, H, B) for V, H in LAYERS[:2] for B in (128, 256, 384))
    assert not _ahead_expected(2048, 1024, 128)
