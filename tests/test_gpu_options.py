"""Library options and timing records belong to their context (include/mdbn_hip.h, "Tuning knobs, PER CONTEXT"): two engines
of one process -- modality-parallel placement in-process, a test toggling a knob -- never see each other's settings."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _kinds(eng, V, H, B, gauss=False):
    from mdbn_amd import RngAddr
    rs = np.random.RandomState(0)
    W = (rs.uniform(-0.1, 0.1, size=(V, H))).astype(np.float32)
    data = rs.normal(size=(B, V)).astype(np.float32) if gauss else (rs.uniform(size=(B, V)) < 0.3).astype(np.float32)
    dW, dhb, dvb, dx = [eng.to_device(a) for a in (W, np.zeros(H, np.float32), np.zeros(V, np.float32), data)]
    eng.kernel_timing(True)
    try:
        eng.cd_step(dx, None, dW, dhb, dvb, gauss, 1, RngAddr(1, 0, 0, 0, 0))
        eng.synchronize()
        return [k for _, _, _, k in eng.kernel_timing_detail()]
    finally:
        eng.kernel_timing(False)


def test_two_contexts_keep_their_own_options(built_lib):
    import mdbn_amd
    a, b = mdbn_amd.HipEngine(), mdbn_amd.HipEngine()
    # knob 1: the one-launch step of LDS-resident layers off on `a` only
    a.set_option("small_fused", 0)
    ka, kb = _kinds(a, 100, 24, 512), _kinds(b, 100, 24, 512)
    assert len(ka) > 0 and any(k >= 1000 for k in ka), ka          # the multi-launch path: register-streaming GEMMs (family 1)
    assert kb == [], kb                                            # b: the one-launch path records no GEMM launch
    # knob 2: the plane path for a small whole-tile shape on `b` only (the default rule keeps it off planes)
    b.set_planes_min_work(0)
    ka, kb = _kinds(a, 1024, 512, 256, gauss=True), _kinds(b, 1024, 512, 256, gauss=True)
    assert ka and all(k < 2000 for k in ka), ka                    # a: f32-operand kernels (families 0 / 1)
    assert kb and all(k >= 2000 for k in kb), kb                   # b: bf16 plane kernels (family 2)
    # ... and the sizing calls answer per context
    assert b.plane_shape(256, 1024, 512, 1024, 512) and not a.plane_shape(256, 1024, 512, 1024, 512)
    # the timing records are per context too: enabling on one does not record the other's launches
    a.kernel_timing(True)
    try:
        _ = _kinds(b, 1024, 512, 256, gauss=True)
        a.synchronize()
        assert a.kernel_timing_detail() == []
    finally:
        a.kernel_timing(False)


@pytest.mark.parametrize("shape", [(100, 24, 512), (784, 500, 20), (300, 130, 100)], ids=["one_launch", "thin", "streaming"])
def test_a_whole_step_between_forward_and_statistics_ends_the_hand_over(hip_engine, shape):
    """mdbn_cd_forward leaves partials in the workspace all shapes share; a whole step in between overwrites them, so the
    statistics half must then be refused (MDBN_EINVAL) on every path instead of summing foreign partials."""
    from mdbn_amd import RngAddr, _lib
    eng = hip_engine
    V, H, B = shape
    rs = np.random.RandomState(1)
    W = rs.uniform(-0.1, 0.1, size=(V, H)).astype(np.float32)
    data = (rs.uniform(size=(B, V)) < 0.3).astype(np.float32)
    dW, dhb, dvb, dx = [eng.to_device(a) for a in (W, np.zeros(H, np.float32), np.zeros(V, np.float32), data)]
    token = eng.cd_forward(dx, None, dW, dhb, dvb, False, 1, RngAddr(1, 0, 0, 0, 0))
    eng.cd_step(dx, None, dW, dhb, dvb, False, 1, RngAddr(1, 0, 1, 0, 0), stats_slot=1)        # a whole step in between
    with pytest.raises(_lib.MdbnError, match="must follow mdbn_cd_forward"):
        eng.cd_statistics(token)
    # the regular order still works afterwards
    token = eng.cd_forward(dx, None, dW, dhb, dvb, False, 1, RngAddr(1, 0, 2, 0, 0))
    eng.cd_statistics(token)
    eng.synchronize()


def test_environment_knobs_reach_every_new_context(built_lib, monkeypatch):
    """MDBN_OPTIONS="name=value,..." (A/B runs of the bench scripts): applied by every HipEngine created afterwards, to its own
    context only; an unknown name fails as mdbn_set_option does."""
    import mdbn_amd
    from mdbn_amd import _lib
    plain = mdbn_amd.HipEngine()
    monkeypatch.setenv("MDBN_OPTIONS", "stream_x6=0, small_fused=0")
    tuned = mdbn_amd.HipEngine()
    monkeypatch.delenv("MDBN_OPTIONS")
    ka, kb = _kinds(plain, 1000, 300, 200), _kinds(tuned, 1000, 300, 200)
    assert ka and all(1100 <= k < 2000 for k in ka), ka            # the default: the streaming bf16x6 kernel
    assert kb and not any(1100 <= k < 2000 for k in kb), kb        # stream_x6 = 0 on this context: LDS-tiled / exact kernels
    monkeypatch.setenv("MDBN_OPTIONS", "no_such_knob=1")
    with pytest.raises(_lib.MdbnError):
        mdbn_amd.HipEngine()


# (V, H, B), W's leading dimension (None: the default), the knobs the path needs, what the timing record of the whole step
# must show.  The paths of csrc/mdbn_capi.hip: one-launch (mdbn_small.hip), thin (mdbn_thin.hip), dense on the streaming /
# register-streaming / LDS-tiled GEMMs, planes (mdbn_planes.hip; also with a ragged hidden width on a padded leading
# dimension) and group-chain (mdbn_gchain.hip, whose statistics half is the dense one).
_HALVES = {
    "one_launch": ((100, 24, 512), None, {}, lambda ks: ks == []),
    "thin": ((784, 500, 20), None, {}, lambda ks: ks == []),
    "streaming": ((300, 130, 100), None, {}, lambda ks: ks and all(1100 <= k < 2000 for k in ks)),
    "tiled_f32": ((1000, 300, 200), None, {"stream_x6": 0, "small_fused": 0},
                  lambda ks: ks and not any(1100 <= k < 2000 for k in ks)),
    "default_1024": ((1024, 512, 256), None, {}, lambda ks: ks and all(k < 2000 for k in ks)),
    # (default options serve the shape above on the streaming kernel, kinds 11xx / 12xx; with that kernel off it runs on the
    #  LDS-tiled kernels of the bf16 pipe, kinds 100..999)
    "tiled_x6": ((1024, 512, 256), None, {"stream_x6": 0}, lambda ks: ks and all(100 <= k < 1000 for k in ks)),
    "planes": ((1024, 512, 256), None, {"planes_min_work": 0}, lambda ks: ks and all(k >= 2000 for k in ks)),
    "planes_ragged": ((1024, 500, 256), 512, {"planes_min_work": 0}, lambda ks: ks and all(k >= 2000 for k in ks)),
    # (one launch for the positive phase and the chain: the statistics GEMM is the only record)
    "gchain": ((256, 200, 512), None, {"gchain": 1}, lambda ks: len(ks) == 1 and ks[0] < 2000),
}


@pytest.mark.parametrize("gauss,k", [(False, 1), (True, 1), (False, 2)], ids=["rbm_k1", "grbm_k1", "rbm_k2"])
@pytest.mark.parametrize("path", list(_HALVES))
def test_the_two_halves_are_the_whole_step_bit_for_bit_on_every_path(built_lib, path, gauss, k):
    """mdbn_cd_forward + mdbn_cd_statistics enqueue what mdbn_cd_step enqueues: on identical inputs and RNG address the packed
    statistics [S | s_h | s_v | cost] and every scratch output are the same bits, on every step path; and a whole step between
    the halves ends the hand-over on every one of them."""
    import mdbn_amd
    from mdbn_amd import RngAddr, _lib
    (V, H, B), ldh, knobs, served = _HALVES[path]
    eng = mdbn_amd.HipEngine()                      # a fresh context: no knob leaks into the shared fixture
    for name, value in knobs.items():
        eng.set_option(name, value)
    rs = np.random.RandomState(2)
    W = rs.uniform(-0.1, 0.1, size=(V, H)).astype(np.float32)
    data = rs.normal(size=(B, V)).astype(np.float32) if gauss else (rs.uniform(size=(B, V)) < 0.3).astype(np.float32)
    dW = eng.alloc_matrix(V, H, ldh)                # (pad columns of a ragged width: exact zeros)
    dW.copy_(eng.to_device(W))
    dhb, dvb, dx = [eng.to_device(a) for a in (rs.normal(size=H).astype(np.float32) * 0.1, rs.normal(size=V).astype(np.float32) * 0.1, data)]
    ldv, ldh = dx.stride(0), dW.stride(0)
    rng = lambda step: RngAddr(1, 0, step, 0, 0)

    def outputs(stats, sc):
        eng.synchronize()
        bufs = [("stats", stats), ("V2", sc.V2), ("P2", sc.P2), ("hs", sc.hs), ("vs", sc.vs), ("planes", sc.planes)]
        return [(name, (t if t._base is None else t._base).detach().cpu().numpy().copy()) for name, t in bufs if t is not None]

    def clear(sc):                                  # what a path does not write compares as zeros, never as the other run's bits
        for t in (sc.V2, sc.P2, sc.hs, sc.vs, sc.planes):
            if t is not None:
                (t._base if t._base is not None else t).zero_()

    sc = eng.cd_scratch(B, V, H, not gauss, ldv, ldh)
    clear(sc)
    eng.kernel_timing(True)
    try:
        stats, sc1 = eng.cd_step(dx, None, dW, dhb, dvb, gauss, k, rng(0))
        whole = outputs(stats, sc1)
        kinds = [kind for _, _, _, kind in eng.kernel_timing_detail()]
    finally:
        eng.kernel_timing(False)
    assert sc1 is sc
    assert served(kinds), (path, kinds)
    assert (sc.planes is not None) == path.startswith("planes")
    clear(sc)
    token = eng.cd_forward(dx, None, dW, dhb, dvb, gauss, k, rng(0), stats=eng.stats_buffer(V, H, 1, ldv, ldh))
    stats2, sc2, _ = eng.cd_statistics(token)
    halves = outputs(stats2, sc2)
    assert sc2 is sc and stats2.data_ptr() != stats.data_ptr()
    assert [n for n, _ in whole] == [n for n, _ in halves]
    assert np.abs(whole[0][1]).max() > 0            # (the statistics were written at all)
    for (name, a), (_, b) in zip(whole, halves):
        assert np.array_equal(a, b), (path, name, int((a != b).sum()))
    # the hand-over, as test_a_whole_step_between_forward_and_statistics_ends_the_hand_over has it, on this path
    token = eng.cd_forward(dx, None, dW, dhb, dvb, gauss, k, rng(1))
    eng.cd_step(dx, None, dW, dhb, dvb, gauss, k, rng(2), stats_slot=1)
    with pytest.raises(_lib.MdbnError, match="must follow mdbn_cd_forward"):
        eng.cd_statistics(token)
    token = eng.cd_forward(dx, None, dW, dhb, dvb, gauss, k, rng(3))
    eng.cd_statistics(token)
    eng.synchronize()
