"""The learned-variance step and the grouped step on every dispatch path of the CD step: four steps through the public
classes (momentum 0.5, 0.5, 0.9, 0.9) against the float64 twin teacher-forced along the device's recorded chain
(tests/_step_forms.py), then the same run with the chain taps off -- the same bits, and the kernel kinds of its launches
(``kernel_timing_detail``) in the family the case names: plane kinds >= 2000, streaming kinds 1100 - 1999, tiled kinds < 100
(exact f32) or 100 - 299 (bf16x6), no recorded kind on the one-launch and the thin path.  Bounds: those of
tests/test_gpu_sigma.py and tests/test_gpu_softmax.py, through ``_margins.check``.

A step with ``learn_sigma`` adds one launch of its own to every step, whatever path the CD step takes: the noise-free
propdown of ph_mean that gives the conditional means (``mdbn_propdown`` on the f32 operands).  It is the last recorded launch
of a step and is asserted to be a propdown; the family is asserted on the launches before it.

The grouped step is composed of ``run_affine`` passes on f32 operands (csrc/mdbn_drv_groups.hip): it reaches the streaming,
the skinny and both tiled families, and neither the planes nor the one-launch and thin steps under any option (DESIGN.md
section 3.13) -- there is no grouped case on those."""
import pytest

import _step_forms as sf
from _variants import family, forward, pipe

pytestmark = pytest.mark.gpu

REL = 2.0 ** -22                # tests/test_gpu_sigma.py: one product rounding plus expf's documented error
PLANES = dict(planes_min_work=0)
# the tiled bf16x6 plans: at 250 -> 130 a pass has two to four 128 x 128 tile jobs, fewer than "x6_min_jobs" (48) keeps on the
# exact-f32 tiles, so the case sets it to 0 as tests/test_gpu_step_variants.py's TILED_X6 does
TILED_X6 = dict(stream_x6=0, skinny_gemm=0, small_fused=0, thin_fused=0, x6_min_jobs=0)
LABEL = [784, 794]
MIXED = [2, 5, 69, 131, 195, 250]       # groups of 3, 64 (MDBN_GROUP_MAX), 62, 64, 55 behind two Bernoulli columns; V % 4 = 2

SIGMA_CASES = [  # id, V, H, B, k, variant, options, family
    ("small", 100, 24, 512, 1, "alone", {}, "one_launch"),
    ("thin", 784, 500, 20, 1, "alone", {}, "thin"),
    ("stream", 256, 200, 512, 2, "alone", {}, "stream"),
    ("planes", 1024, 512, 256, 1, "alone", PLANES, "planes"),
    ("planes_ragged_H", 1024, 449, 256, 1, "alone", PLANES, "planes"),
    ("planes_centred_sparse", 1024, 512, 256, 1, "both", PLANES, "planes"),
    ("tiled_f32", 250, 130, 99, 1, "alone", sf.TILED_F32, "tiled_f32"),
    ("tiled_x6_stats", 250, 130, 99, 1, "alone", dict(TILED_X6, gemm_bf16x6=1), "tiled_x6"),
    ("tiled_x6_forward", 250, 130, 99, 1, "alone", dict(TILED_X6, gemm_bf16x6=2), "tiled_x6"),
    ("tiled_x6_both", 250, 130, 99, 1, "alone", dict(TILED_X6, gemm_bf16x6=3), "tiled_x6"),
]
GROUPED_CASES = [  # id, V, H, B, k, groups, persistent, mode, options, family
    ("thin_label", 794, 500, 20, 2, LABEL, False, "plain", {}, "skinny"),
    ("stream", 256, 200, 512, 1, 4, False, "plain", {}, "stream"),
    ("pcd_stream", 256, 200, 512, 1, 4, True, "plain", {}, "stream"),
    ("tiled_f32", 250, 130, 99, 1, MIXED, False, "plain", sf.TILED_F32, "tiled_f32"),
    ("tiled_f32_centred_sparse", 250, 130, 99, 1, MIXED, False, "both", sf.TILED_F32, "tiled_f32"),
    ("tiled_x6_stats", 250, 130, 99, 1, MIXED, False, "plain", dict(TILED_X6, gemm_bf16x6=1), "tiled_x6"),
    ("tiled_x6_forward", 250, 130, 99, 1, MIXED, False, "plain", dict(TILED_X6, gemm_bf16x6=2), "tiled_x6"),
    ("tiled_x6_both", 250, 130, 99, 1, MIXED, False, "plain", dict(TILED_X6, gemm_bf16x6=3), "tiled_x6"),
    # the shape and the option that put the plain and the sigma step on the planes: the composed step stays on f32 operands
    ("planes_shape", 1024, 512, 256, 1, 4, False, "plain", PLANES, "f32_operands"),
    ("planes_shape_centred_sparse", 1024, 512, 256, 1, 4, False, "both", PLANES, "f32_operands"),
    ("planes_shape_pcd", 1024, 512, 256, 1, 4, True, "plain", PLANES, "f32_operands"),
]


# Philox seed of a grouped case: 7 unless the twin alone has more draws near a boundary under it than the case's cap (the test
# asserts it; then the case gets the next seed here, as tests/_softmax_np.py's CASE_SEEDS does for the kernel cases)
CASE_SEEDS = {}


def assert_family(name, path, kinds, k, opts, steps=sf.STEPS):
    """``kinds``: the launches of the CD steps of a run, in order."""
    if path in ("one_launch", "thin"):
        assert kinds == [], (name, kinds)
        return
    assert kinds, name
    if path == "planes":
        assert all(kd >= 2000 for kd in kinds), (name, kinds)
    elif path == "stream":
        assert all(1100 <= kd < 2000 for kd in kinds), (name, kinds)
    elif path == "f32_operands":
        assert len(kinds) == steps * (2 * k + 2) and all(kd < 2000 for kd in kinds), (name, kinds)
    elif path == "skinny":                          # B <= 64: the register-streaming kernels, exact f32 or on the bf16 pipe
        assert all(family(kd) == 1 for kd in forward(kinds)) and all(kd < 2000 for kd in kinds), (name, kinds)
    elif path == "tiled_f32":
        assert len(kinds) == steps * (2 * k + 2) and all(kd < 100 for kd in kinds), (name, kinds)
    else:
        assert path == "tiled_x6"
        assert len(kinds) == steps * (2 * k + 2) and all(family(kd) == 0 for kd in kinds), (name, kinds)
        fwd, stats = forward(kinds), [kd for kd in kinds if kd % 10 == 3]
        assert len(stats) == steps
        assert all((pipe(kd) in (1, 2)) == bool(opts["gemm_bf16x6"] & 2) for kd in fwd), (name, kinds)
        assert all((pipe(kd) == 1) == bool(opts["gemm_bf16x6"] & 1) for kd in stats), (name, kinds)


@pytest.fixture
def have_gpu(built_lib):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("name,V,H,B,k,variant,opts,path", SIGMA_CASES, ids=[c[0] for c in SIGMA_CASES])
def test_sigma_steps_on_every_dispatch_path(have_gpu, name, V, H, B, k, variant, opts, path):
    def engine(tapped):
        eng = sf.sigma_engine(tapped=tapped, opts=opts)         # product defaults but for `opts`; keep_f32 stays off
        if name == "planes_ragged_H":
            eng.weight_ld_min_elems = 0         # (a layer this small keeps dense rows by default: pad W's rows to 512 here)
        assert not eng.keep_f32
        return eng
    tapped = sf.run_sigma(engine(True), V, H, B, k, True, variant)
    sf.check_sigma("path %s" % name, tapped, REL)
    plain = sf.run_sigma(engine(False), V, H, B, k, True, variant, timing=True)
    # every step: the launches of the CD step, then the propdown of the conditional means
    cd = []
    for kinds in plain.kinds:
        assert kinds and kinds[-1] % 10 == 0 and kinds[-1] < 2000, (name, plain.kinds)
        cd += kinds[:-1]
    print("path %s: kinds %s" % (name, plain.kinds[0]))
    assert_family(name, path, cd, k, opts)
    if path == "planes":
        assert tapped.rbm.W.tensor.stride(0) == 512
    sf.same_bits(plain, tapped, "sigma %s: taps off against taps on" % name)


@pytest.mark.parametrize("name,V,H,B,k,groups,persistent,mode,opts,path", GROUPED_CASES, ids=[c[0] for c in GROUPED_CASES])
def test_grouped_steps_on_every_dispatch_path(have_gpu, name, V, H, B, k, groups, persistent, mode, opts, path):
    import mdbn_amd
    from mdbn_amd.utils import group_boundaries
    eng = sf.set_options(mdbn_amd.HipEngine(), opts)
    assert not eng.keep_f32
    cap = sf.draw_cap(B, V, H, k, group_boundaries(groups, V).tolist(), persistent)
    assert 3 <= cap <= 12, cap
    seed = CASE_SEEDS.get(name, 7)
    tapped = sf.run_grouped(eng, V, H, B, k, groups, persistent, mode, cap=cap, seed=seed)
    sf.check_grouped("path %s" % name, tapped)
    assert max(tapped.twin_ties) <= cap, "the twin alone has %s draws near a boundary under seed %d: give the case the next seed" % (
        tapped.twin_ties, seed)
    plain = sf.run_grouped(eng, V, H, B, k, groups, persistent, mode, tapped=False, timing=True, seed=seed)
    print("path %s: kinds %s, cap %d" % (name, plain.kinds[:2 * k + 2], cap))
    assert_family(name, path, plain.kinds, k, opts)
    if persistent:
        # a caller's chain may hold anything: the first propdown of a step takes six piece products where it runs on the bf16
        # pipe; every other pass of the chain reads the step's own 0/1 samples and takes three
        per = 2 * k + 2
        firsts, later = plain.kinds[1::per], [kd for t in range(sf.STEPS) for kd in plain.kinds[t * per + 2:t * per + per - 1]]
        assert all(pipe(kd) in (0, 1) for kd in firsts) and all(pipe(kd) in (0, 2) for kd in later), (name, plain.kinds)
    sf.same_bits(plain, tapped, "grouped %s: taps off against taps on" % name)
