"""The deferred update of mdbn_cd_statistics (include/mdbn_hip.h), on every step path, in ONE process.

``cd_statistics(token, deferred=...)`` finishes step t and applies the phase-3 update of step t - 1.  On the plane path the
update runs INSIDE the statistics GEMM when it qualifies (csrc/mdbn_planes.hip: pl_loader's ``early == 2`` branch, its
flat-share twin in pl_loader_bal for balanced launches, deferred_bias_update on the MFMA waves); everywhere else the
library launches the update itself ahead of the statistics half (csrc/mdbn_capi.hip: cd_step_impl, planes_statistics).

Every case compares two orders from identical state, bit for bit:
  order A (the definition): cd_forward, apply_update(..., prev, phase), cd_statistics(token)
  order B                 : cd_forward, cd_statistics(token, deferred=(..., prev, ..., phase, ldv))
and one test anchors order B to the phase-3 rule restated in float64, so that order A is not its own witness.

That the inside route ran is witnessed by the gather-ahead: with an announced next minibatch on an unbalanced launch the
loader waves gather its rows only beside a deferred update they apply themselves (``CDScratch.ahead``)."""
import numpy as np
import pytest
import torch

import _margins
from test_gpu_options import _HALVES

pytestmark = pytest.mark.gpu

MOMENTUM = 0.6
# plane shapes: (V, H, B), W's leading dimension (None: the default), knobs.  nt = 2 B / 32 stages of the statistics GEMM; one
# workgroup per 128 x 128 tile.  The gather-ahead that witnesses the inside route needs ceil(B / tiles) rows per workgroup
# times ceil(V / 2048) passes <= 4 (planes_statistics), so the witnessed shapes have >= B / 4 tiles.  Statistics plan
# unsplit by default from 129 tiles on (below that the knobs of _UNSPLIT keep them in one piece), and a shape is a plane
# shape only if the split factors of both forward passes divide their reduction lengths into whole 32-deep slices.
_UNSPLIT = {"planes_min_work": 0, "gemm_min_splitk": 4096, "x6_min_jobs": 0}
_PLANE = {
    "D24": ((2048, 1280, 384), None, {"planes_min_work": 0}),     # 160 tiles, unsplit by default; nt = 24: the fewest stages of a
                                                                  # whole-tile batch, 16 items + 5 gather stages = nt - 3
    "D40": ((1792, 1536, 640), None, {"planes_min_work": 0}),     # 168 tiles, nt = 40, four gather units
    "P24": ((2560, 1280, 384), None, {"planes_min_work": 0}),     # 200 tiles, two rows x two passes, the second pass partial
    "K24": ((2048, 768, 384), None, _UNSPLIT),                    # 96 tiles, four rows per workgroup: every unit slot live
    "K24r": ((2048, 700, 384), 768, _UNSPLIT),                    # ragged hidden width on a padded leading dimension
    "K32w": ((2048, 1024, 512), None, _UNSPLIT),                  # 128 tiles, nt = 32
    "N24": ((1024, 512, 384), None, _UNSPLIT),                    # 32 tiles: inside by the rule, but 12 rows per workgroup do
    "N24r": ((1024, 500, 384), 512, _UNSPLIT),                    # not fit the four unit slots -- no gather-ahead, no witness
    "K32": ((1024, 512, 512), None, _UNSPLIT),                    # the base of the balanced cases
    "K16": ((2048, 768, 256), None, _UNSPLIT),                    # K24's layer at nt = 16 < 20: the launch
    "S2": ((1280, 1280, 384), None, {"planes_min_work": 0}),      # 100 tiles, nt = 24, statistics split two ways: the launch
}
_served_planes = lambda ks: bool(ks) and all(k >= 2000 for k in ks)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _engine(knobs):
    import mdbn_amd
    eng = mdbn_amd.HipEngine()                      # a fresh context: no knob leaks into the shared fixture
    for name, value in knobs.items():
        eng.set_option(name, value)
    return eng


class _Problem(object):
    """Host-side state of one case: every operand of the update rule is live (momentum, a non-zero initial speed,
    lambda_2; the Bernoulli RBM also weight cost on a frozen W0 != W; batch_size != n_rows)."""

    def __init__(self, shape, gauss, ldh=None, idx64=True, seed=0, lists=3):
        V, H, B = shape
        self.V, self.H, self.B, self.gauss, self.ldh = V, H, B, gauss, ldh
        rs = np.random.RandomState(seed)
        f = lambda *size: rs.normal(size=size).astype(np.float32)
        self.W = rs.uniform(-0.1, 0.1, size=(V, H)).astype(np.float32)
        self.W_speed = 0.01 * f(V, H)
        self.hb, self.vb, self.hbs, self.vbs = 0.1 * f(H), 0.1 * f(V), 0.01 * f(H), 0.01 * f(V)
        N = 2 * B
        self.data = f(N, V) if gauss else (rs.uniform(size=(N, V)) < 0.3).astype(np.float32)
        self.W0 = None if gauss else (self.W + 0.05 * f(V, H)).astype(np.float32)
        self.idx = [rs.permutation(N)[:B].astype(np.int64 if idx64 else np.int32) for _ in range(lists)]
        self.lr, self.l2, self.wc = (0.002, 0.1, 0.0) if gauss else (0.05, 0.01, 2e-4)
        self.batch_size, self.n_rows = float(B), float(2 * B)
        self.cost_scale = 1.0 / (self.n_rows * V) if gauss else 1.0 / self.n_rows

    def device(self, eng):
        return _State(eng, self)


class _State(object):
    """Device copy of a _Problem.  The bias vectors sit in front of a guard of sevens (a kernel that takes the padded width
    for the live one writes there); W and W_speed keep exact zeros in their pad columns."""
    GUARD = 16

    def __init__(self, eng, p):
        self.eng, self.p = eng, p

        def matrix(a):
            t = eng.alloc_matrix(p.V, p.H, p.ldh)
            t.copy_(torch.from_numpy(a))
            return t

        def vector(a):
            buf = torch.full((a.size + self.GUARD,), 7.0, dtype=torch.float32, device=eng.device)
            buf[:a.size].copy_(torch.from_numpy(a))
            return buf[:a.size]

        self.W, self.W_speed = matrix(p.W), matrix(p.W_speed)
        self.W0 = matrix(p.W0) if p.W0 is not None else None
        self.hb, self.hbs, self.vb, self.vbs = vector(p.hb), vector(p.hbs), vector(p.vb), vector(p.vbs)
        self.x = eng.to_device(p.data)
        self.idx = [torch.from_numpy(i).to(eng.device) for i in p.idx]
        self.ldv, self.ldh = self.x.stride(0), self.W.stride(0)

    def stats_buffer(self):
        return self.eng.new_stats_buffer(self.p.V, self.p.H, self.ldv, self.ldh)

    def update(self, stats, phase, lambda_1=0.0, momentum=MOMENTUM):
        """The ``deferred=`` tuple; its first 16 entries are apply_update's positional arguments."""
        p = self.p
        return (self.W, self.W_speed, self.W0, self.hb, self.hbs, self.vb, self.vbs, stats, p.lr, lambda_1, p.l2, p.wc,
                momentum, p.batch_size, p.n_rows, p.cost_scale, phase, self.ldv)

    def apply(self, upd):
        return self.eng.apply_update(*upd[:16], phase=upd[16], ldv=upd[17])

    def planes(self):
        ent = getattr(self.W, "_mdbn_planes", None)
        return None if ent is None else ent[0]

    def snapshot(self):
        self.eng.synchronize()
        whole = lambda t: (t if t._base is None else t._base).detach().cpu().numpy().copy()
        out = {name: whole(getattr(self, name)) for name in ("W", "W_speed", "hb", "hbs", "vb", "vbs")}
        if self.planes() is not None:
            out["W_planes"] = self.planes().cpu().numpy().copy()
        return out

    def check_invariants(self, label):
        """Pad columns of W and W_speed: exact zeros; the guards behind the biases: untouched; W's planes: the split of W."""
        p = self.p
        for name in ("W", "W_speed"):
            base = getattr(self, name)._base
            assert base.shape == (p.V, self.ldh)
            assert int(torch.count_nonzero(base[:, p.H:])) == 0, (label, name, "pad columns")
        for name in ("hb", "hbs", "vb", "vbs"):
            t = getattr(self, name)
            assert bool((t._base[t.numel():] == 7.0).all()), (label, name, "written past its end")
        if self.planes() is not None:
            p1, p2, p3 = [((self.planes()[i].to(torch.int32) & 0xffff) << 16).view(torch.float32) for i in range(3)]
            assert torch.equal(((p3 + p2) + p1).view(torch.int32), self.W._base.view(torch.int32)), (label, "(p3 + p2) + p1 != W")


def _rng(step):
    from mdbn_amd import RngAddr
    return RngAddr(11, 0, step, 0, 0)


def _one_step(eng, prob, order, k=1, comm_cus=0, phase=3, lambda_1=0.0, same_buffer=False, follow=False, announce=True,
              keep_inputs=False):
    """An earlier real step on another minibatch fills ``prev``; then the step under test in order A or B.  Returns every
    output as host arrays, the witness and the launch kinds of the two halves."""
    p, st = prob, prob.device(eng)
    prev = st.stats_buffer()
    eng.cd_step(st.x, st.idx[0], st.W, st.hb, st.vb, p.gauss, k, _rng(0), stats=prev, comm_cus=comm_cus)
    own = prev if same_buffer else st.stats_buffer()
    before = st.snapshot()
    inputs = dict(before, prev=prev.cpu().numpy().copy()) if keep_inputs else None
    eng.kernel_timing(True)
    try:
        token = eng.cd_forward(st.x, st.idx[1], st.W, st.hb, st.vb, p.gauss, k, _rng(1), stats=own, comm_cus=comm_cus,
                               next_indexes=st.idx[2] if announce else None)
        upd = st.update(prev, phase, lambda_1)
        if order == "A":
            cost = st.apply(upd)
            stats, sc, none = eng.cd_statistics(token)
            assert none is None
        else:
            stats, sc, cost = eng.cd_statistics(token, deferred=upd)
        assert stats is own
        eng.synchronize()
        kinds = [kind for _, _, _, kind in eng.kernel_timing_detail()]
    finally:
        eng.kernel_timing(False)
    witness = sc.ahead is not None
    out = st.snapshot()
    label = (order, p.gauss, (p.V, p.H, p.B))
    assert not np.array_equal(out["W"], before["W"]) and not np.array_equal(out["W_speed"], before["W_speed"]), label
    for name in ("hb", "hbs", "vb", "vbs"):
        assert not np.array_equal(out[name], before[name]), (label, name, "unchanged")
    st.check_invariants(label)
    out["cost"] = np.array([float(cost)], np.float32)
    out["stats"] = own.cpu().numpy().copy()
    assert np.abs(out["stats"]).max() > 0 and out["cost"][0] != 0
    if follow:
        # the NEXT step on the announced list: on rows gathered beside the deferred update where the witness is set
        nxt, xb = st.stats_buffer(), sc.x_buffer
        eng.cd_step(st.x, st.idx[2], st.W, st.hb, st.vb, p.gauss, k, _rng(2), stats=nxt, comm_cus=comm_cus)
        eng.synchronize()
        assert (sc.x_buffer != xb) == witness, (label, "the next step reads the X2 buffer that was gathered ahead, and only then")
        out["next_stats"] = nxt.cpu().numpy().copy()
    return out, witness, kinds, inputs


def _same(a, b, label):
    assert sorted(a) == sorted(b), (label, sorted(a), sorted(b))
    for name in sorted(a):
        assert a[name].shape == b[name].shape and np.array_equal(_bits(a[name]), _bits(b[name])), \
            (label, name, int((_bits(a[name]) != _bits(b[name])).sum()))


def _plane_engine(name, extra=None):
    (V, H, B), ldh, knobs = _PLANE[name]
    eng = _engine(dict(knobs, **(extra or {})))
    return eng, (V, H, B), ldh


def _both_orders(eng, prob, served, label, expect_witness, **kw):
    a, wa, ka, _ = _one_step(eng, prob, "A", **kw)
    b, wb, kb, inputs = _one_step(eng, prob, "B", **kw)
    assert served(ka) and served(kb), (label, ka, kb)
    assert ka == kb, (label, ka, kb)                # the same GEMMs either way: the update is no GEMM launch
    assert not wa, (label, "order A gathers nothing ahead")
    assert wb == expect_witness, (label, "inside route" if expect_witness else "launch", wb)
    _same(a, b, label)
    return a, b, inputs


# ---------------------------------------------------------------------------------- the plane path
@pytest.mark.parametrize("gauss", [True, False], ids=["grbm", "rbm_w0"])
@pytest.mark.parametrize("name,idx64", [("D24", True), ("D24", False), ("D40", True), ("P24", True), ("K24", True),
                                        ("K24", False), ("K24r", True), ("K32w", True), ("N24", True), ("N24r", True)],
                         ids=["D24-i64", "D24-i32", "D40", "P24", "K24-i64", "K24-i32", "K24r", "K32w", "N24", "N24r"])
def test_inside_the_statistics_gemm_is_the_launched_update_bit_for_bit(built_lib, name, idx64, gauss):
    """The loader waves' update (four asm loads per item behind counted waits; the fourth, from W0, live on the RBM) and the
    MFMA waves' bias / cost half equal apply_update(phase 3) ahead of the statistics half, in every bit of W, its planes,
    the speeds, the biases, the cost and this step's statistics -- at nt = 24, where the gather-ahead units leave no stage
    spare, 32 and 40, on a ragged width, with int32 and int64 index lists.  The witness proves the route; the next step on
    the rows gathered beside the update equals a step that gathered for itself.  (N24 / N24r, 1024 -> 512 | 500 at B = 384:
    the rule sends them inside as well, with too many rows per workgroup for the gather-ahead -- bit equality alone.)"""
    eng, shape, ldh = _plane_engine(name)
    prob = _Problem(shape, gauss, ldh, idx64)
    V, H, B = shape
    assert eng.plane_shape(B, V, H, V, ldh or H), (name, "not a plane shape under its knobs")
    _both_orders(eng, prob, _served_planes, (name, gauss, idx64), not name.startswith("N"), follow=True)


@pytest.mark.parametrize("gauss", [True, False], ids=["grbm", "rbm_w0"])
@pytest.mark.parametrize("name", ["K16", "S2"])
def test_too_few_stages_or_split_statistics_launch_the_update(built_lib, name, gauss):
    """nt = 16 < 20 and a split-K statistics plan: the library launches the update ahead of the GEMM(s); nothing is
    gathered ahead."""
    eng, shape, ldh = _plane_engine(name)
    V, H, B = shape
    assert eng.plane_shape(B, V, H, V, ldh or H), name
    _both_orders(eng, _Problem(shape, gauss, ldh), _served_planes, (name, gauss), False, follow=True)


_FALLBACKS = {
    "early_w=0": ({"early_w": 0}, {}),
    "planes_mfma=32": ({"planes_mfma": 32}, {}),
    "phase0": ({}, {"phase": 0}),
    "phase0_lambda1": ({}, {"phase": 0, "lambda_1": 0.01}),
    # order A is the definition: the update reads the buffer before the GEMM writes it
    "same_buffer": ({}, {"same_buffer": True}),
}


@pytest.mark.parametrize("gauss", [True, False], ids=["grbm", "rbm_w0"])
@pytest.mark.parametrize("case", list(_FALLBACKS))
def test_every_fallback_of_the_inside_route_is_the_launch(built_lib, case, gauss):
    """K24 takes the inside route (test above); each of these conditions must send the same shape to the launch, bitwise
    order A, the witness off."""
    knobs, kw = _FALLBACKS[case]
    eng, shape, ldh = _plane_engine("K24", knobs)
    V, H, B = shape
    assert eng.plane_shape(B, V, H, V, H)
    _both_orders(eng, _Problem(shape, gauss, ldh), _served_planes, (case, gauss), False, **kw)


@pytest.mark.parametrize("gauss", [True, False], ids=["grbm", "rbm_w0"])
@pytest.mark.parametrize("P", [15, 16, 17, 51, 52])
def test_balanced_launches_share_the_update_flat(built_lib, P, gauss):
    """K32 under ``bal_blocks = P`` (comm_cus in the call): 131072 float4 pieces, 32 tiles x 32 stages.  P = 15: a flat share
    of 9216 > 16 x 512 pieces, the launch; 16: exactly 8192; 17: workgroup 16's share is empty; 51: 3072 pieces, workgroup
    42 partial, 43..50 empty, 1024 / 51 = 20 stages; 52: 19 stages, the launch.  Bitwise order A under the same P, and the
    same bits when repeated.  (A balanced launch gathers nothing ahead: no witness either way.)"""
    eng, shape, ldh = _plane_engine("K32", {"bal_blocks": P})
    prob = _Problem(shape, gauss, ldh)
    balanced = lambda ks: _served_planes(ks) and ks[-1] >= 3000       # the statistics GEMM itself ran balanced
    a, b, _ = _both_orders(eng, prob, balanced, (P, gauss), False, comm_cus=1)
    again, w, _, _ = _one_step(eng, prob, "B", comm_cus=1)
    assert not w
    _same(b, again, (P, gauss, "repeated"))


# ---------------------------------------------------------------------------------- the float64 anchor
@pytest.mark.parametrize("name", ["N24r", "K24r"])
def test_order_b_is_the_phase_3_rule_in_float64(built_lib, name):
    """Order B on 1024 -> 500 (ldh 512) and, witnessed, on 2048 -> 700 (ldh 768), with weight cost and W0, against the rule restated in float64 on the same float32
    inputs: g = S / batch_size - wc W0, speed' = g + (speed - g) mu, W' = W (1 - 2 lr l2) + speed' lr; the biases with
    s / n_rows and decay 1; cost = cost_sum cost_scale.  Relative to each array's maximum, within the update rule's 1e-6
    (DESIGN.md section 4)."""
    eng, shape, ldh = _plane_engine(name)
    prob = _Problem(shape, False, ldh)
    V, H, B = shape
    out, witness, kinds, inp = _one_step(eng, prob, "B", keep_inputs=True)
    assert witness == (name == "K24r") and _served_planes(kinds)
    f8 = lambda x: np.asarray(x, np.float64)
    f4 = lambda x: float(np.float32(x))              # the scalars travel as float32
    lr, l2, wc, mu = f4(prob.lr), f4(prob.l2), f4(prob.wc), f4(MOMENTUM)
    prev = inp["prev"]
    S, s_h, s_v = prev[:V * ldh].reshape(V, ldh), prev[V * ldh:][:ldh], prev[V * ldh + ldh:][:V]
    cost_sum = prev[V * ldh + ldh + V]
    W0 = np.zeros((V, ldh), np.float32)
    W0[:, :H] = prob.W0
    g = f8(S) / prob.batch_size - wc * f8(W0)
    speed = g + (f8(inp["W_speed"]) - g) * mu
    want = {"W_speed": speed, "W": f8(inp["W"]) * (1.0 - 2.0 * lr * l2) + speed * lr}
    for b, bs, s, n in (("hb", "hbs", s_h, H), ("vb", "vbs", s_v, V)):
        gb = f8(s[:n]) / prob.n_rows
        want[bs] = gb + (f8(inp[bs][:n]) - gb) * mu
        want[b] = f8(inp[b][:n]) + want[bs] * lr
    want["cost"] = np.array([f8(cost_sum) * f4(prob.cost_scale)])
    for arr, ref in sorted(want.items()):
        got = f8(out[arr]).reshape(-1)[:ref.size] if ref.ndim == 1 else f8(out[arr])
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print("deferred anchor %d->%d %s: %.3e" % (V, H, arr, err))
        _margins.check("deferred anchor (%d->%d, B = %d, inside the statistics GEMM): %s / max" % (V, H, B, arr), err, 1e-6, "update")


# ---------------------------------------------------------------------------------- every other path
@pytest.mark.parametrize("gauss,k", [(True, 1), (False, 2)], ids=["grbm_k1", "rbm_w0_k2"])
@pytest.mark.parametrize("path", ["one_launch", "thin", "streaming", "tiled_f32", "tiled_x6", "gchain"])
def test_every_other_path_launches_the_update_ahead_of_its_statistics_half(built_lib, path, gauss, k):
    """Off the plane path the rule is one launch of the whole update ahead of the statistics half (cd_step_impl): order B
    equals order A bit for bit on the one-launch, thin, streaming, LDS-tiled and group-chain steps."""
    shape, ldh, knobs, served = _HALVES[path]
    eng = _engine(knobs)
    _both_orders(eng, _Problem(shape, gauss, ldh), served, (path, gauss, k), False, k=k)


# ---------------------------------------------------------------------------------- four steps in the product's order
_PIPELINE = {"D24": (_PLANE["D24"], _served_planes), "K24r": (_PLANE["K24r"], _served_planes),
             "thin": (_HALVES["thin"][:3], _HALVES["thin"][3])}


@pytest.mark.parametrize("gauss", [True, False], ids=["grbm", "rbm_w0"])
@pytest.mark.parametrize("name", list(_PIPELINE))
def test_four_overlapped_steps_equal_four_plain_ones(built_lib, name, gauss):
    """StepFunction.__call__'s overlapped order: cd_step + apply_update(phase 2); three times cd_forward(next_indexes) +
    cd_statistics(deferred = the previous statistics, phase 3) on two alternating buffers; apply_update(phase 1).  Against
    the same schedule with cd_step + apply_update(phase 3): every parameter, speed, cost and plane, bit for bit -- W and
    its planes as the loader waves wrote them feed the next forward half."""
    (shape, ldh, knobs), served = _PIPELINE[name]
    eng = _engine(knobs)
    prob = _Problem(shape, gauss, ldh, lists=5)
    mus = [0.5, 0.6, 0.7, 0.8]

    def run(overlapped):
        st = prob.device(eng)
        bufs = [st.stats_buffer(), st.stats_buffer()]
        costs, witnesses, kinds = [], [], []
        eng.cd_step(st.x, st.idx[0], st.W, st.hb, st.vb, gauss, 1, _rng(0), stats=bufs[0])
        st.apply(st.update(bufs[0], 2, momentum=mus[0]))
        for t in (1, 2, 3):
            upd = st.update(bufs[(t - 1) & 1], 3, momentum=mus[t - 1])
            if overlapped:
                eng.kernel_timing(True)
                try:
                    token = eng.cd_forward(st.x, st.idx[t], st.W, st.hb, st.vb, gauss, 1, _rng(t), stats=bufs[t & 1],
                                           next_indexes=st.idx[t + 1])
                    _, sc, cost = eng.cd_statistics(token, deferred=upd)
                    eng.synchronize()
                    kinds.append([kind for _, _, _, kind in eng.kernel_timing_detail()])
                finally:
                    eng.kernel_timing(False)
                witnesses.append(sc.ahead is not None)
            else:
                eng.cd_step(st.x, st.idx[t], st.W, st.hb, st.vb, gauss, 1, _rng(t), stats=bufs[t & 1])
                cost = st.apply(upd)
            costs.append(cost)
        costs.append(st.apply(st.update(bufs[3 & 1], 1, momentum=mus[3])))
        out = st.snapshot()
        st.check_invariants((name, gauss, overlapped))
        out["costs"] = np.array([float(c) for c in costs], np.float32)
        out["stats"] = np.stack([b.cpu().numpy() for b in bufs])
        return out, witnesses, kinds

    plain, _, _ = run(False)
    over, witnesses, kinds = run(True)
    assert all(served(ks) for ks in kinds), (name, kinds)
    assert witnesses == [name != "thin"] * 3, (name, witnesses)          # the plane shapes took the inside route every time
    assert np.all(over["costs"] != 0)
    _same(plain, over, (name, gauss))


# ---------------------------------------------------------------------------------- the protocol
@pytest.mark.parametrize("name", ["K24", "streaming"])
def test_a_refused_deferred_update_touches_nothing_and_ends_the_hand_over(built_lib, name):
    """A deferred update of phase 1 or 2, or one for another W / another leading dimension, is refused and launches
    nothing.  The mismatch is found after the hand-over check, so the call consumed the hand-over: a second, valid
    statistics call with the same token is refused, a fresh pair of halves succeeds."""
    from mdbn_amd import _lib
    shape, ldh, knobs = _PLANE[name] if name in _PLANE else _HALVES[name][:3]
    eng = _engine(knobs)
    prob = _Problem(shape, name in _PLANE, ldh)
    gauss = prob.gauss
    st = prob.device(eng)
    prev, own = st.stats_buffer(), st.stats_buffer()
    eng.cd_step(st.x, st.idx[0], st.W, st.hb, st.vb, gauss, 1, _rng(0), stats=prev)
    before = st.snapshot()
    forward = lambda step: eng.cd_forward(st.x, st.idx[1], st.W, st.hb, st.vb, gauss, 1, _rng(step), stats=own)
    # the argument checks of the update itself
    for phase in (1, 2):
        token = forward(1)
        with pytest.raises(_lib.MdbnError, match="a deferred update is phase 3"):
            eng.cd_statistics(token, deferred=st.update(prev, phase))
        _same(before, st.snapshot(), (name, "phase", phase))
    for other_ld in (None, st.ldh + 128):
        W2, W2s = eng.alloc_matrix(prob.V, prob.H, other_ld or st.ldh), eng.alloc_matrix(prob.V, prob.H, other_ld or st.ldh)
        W2.copy_(st.W)
        bad = (W2, W2s) + st.update(prev, 3)[2:]
        token = forward(2)
        with pytest.raises(_lib.MdbnError, match="deferred update does not match"):
            eng.cd_statistics(token, deferred=bad)
        eng.synchronize()
        _same(before, st.snapshot(), (name, "mismatch", other_ld))
        assert int(torch.count_nonzero(W2s._base)) == 0 and torch.equal(W2, st.W), (name, "the refused update ran")
        with pytest.raises(_lib.MdbnError, match="must follow mdbn_cd_forward"):
            eng.cd_statistics(token, deferred=st.update(prev, 3))
        _same(before, st.snapshot(), (name, "second call", other_ld))
    token = forward(3)
    _, _, cost = eng.cd_statistics(token, deferred=st.update(prev, 3))
    eng.synchronize()
    assert float(cost) != 0 and not np.array_equal(before["W"], st.snapshot()["W"])
