"""The classification RBM on the device against the float64 twin (tests/_disc_np.py): (a) mdbn_class_posterior, (b)
mdbn_class_stats, pure and hybrid, on every GEMM family mdbn_cd_stats dispatches to, (c) every refused call, (d) workspaces of
exactly the sizer's bytes, (e) the public surface -- label_posterior against group_posterior, the step function against the
twin teacher-forced along the device's recorded chain, the toy problem of tests/test_disc_twin.py, a resumed run."""
import ctypes as C

import numpy as np
import pytest

import _disc_np as dn
import _softmax_np as sm
import _step_forms as sf
from _center_np import unpack
from _margins import SURVEY, check
from oracle import rbm_np
from oracle.philox_np import PhiloxDraws

pytestmark = pytest.mark.gpu

POISON = float("nan")
PARAMS = ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed")
MIXED = [2, 5, 69, 131, 195, 250]
TILED_X6 = dict(stream_x6=0, skinny_gemm=0, small_fused=0, thin_fused=0, x6_min_jobs=0, gemm_bf16x6=3)


def ru4(n):
    return (n + 3) & ~3


def ru64(n):
    return (n + 63) & ~63


def bits(t):
    return t.detach().cpu().numpy().view(np.int32).copy()


def padded(eng, a, ld, fill=POISON):
    """Device matrix over storage [rows, ld] whose pad columns hold ``fill``."""
    import torch
    a = np.atleast_2d(np.asarray(a, dtype=np.float32))
    full = np.full((a.shape[0], ld), fill, dtype=np.float32)
    full[:, :a.shape[1]] = a
    return torch.from_numpy(full).to(eng.device)


def p_(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def sizer(eng, B, V, H, ldv, ldh, K, mode):
    n = C.c_int64()
    assert eng.lib.mdbn_class_workspace_bytes(eng.ctx, B, V, H, ldv, ldh, K, mode, C.byref(n)) == 0 and n.value > 0 and n.value % 4 == 0
    return n.value


GUARD = 1024


def guarded_ws(eng, nbytes):
    """A workspace of exactly ``nbytes`` followed by a poisoned guard region: (tensor, check())."""
    import torch
    ws = torch.full((nbytes // 4 + GUARD,), POISON, dtype=torch.float32, device=eng.device)
    ws[nbytes // 4:] = 12345.0
    want = bits(ws[nbytes // 4:])

    def unchanged():
        return np.array_equal(bits(ws[nbytes // 4:]), want)
    return ws, unchanged


class Layer(object):
    """Host parameters of a case and their device copies with NaN-poisoned pad columns."""

    def __init__(self, eng, V, H, scale, seed):
        rs = np.random.RandomState(seed)
        self.V, self.H, self.ldv, self.ldh = V, H, ru4(V) + (4 if V % 4 == 0 else 0), ru4(H) + (4 if H % 4 == 0 else 0)
        self.W = (scale * rs.normal(size=(V, H))).astype(np.float32)
        self.hb = (scale * rs.normal(size=H)).astype(np.float32)
        self.vb = (scale * rs.normal(size=V)).astype(np.float32)
        self.dW, self.dhb, self.dvb = padded(eng, self.W, self.ldh), eng.to_device(self.hb), eng.to_device(self.vb)


def posterior_call(eng, L, v, lo, K, post, logp, ws, ws_bytes=None, over=None):
    a = dict(ctx=eng.ctx, v=v, B=v.shape[0], ldv=L.ldv, W=L.dW, V=L.V, H=L.H, ldh=L.ldh, hb=L.dhb, vb=L.dvb, lo=lo, K=K, post=post,
             ldk=post.shape[1] if post is not None else K, logp=logp, ws=ws)
    a.update(over or {})             # (a refused call's one wrong argument)
    return eng.lib.mdbn_class_posterior(a["ctx"], eng._stream(), p_(a["v"]), a["B"], a["ldv"], p_(a["W"]), a["V"], a["H"], a["ldh"], p_(a["hb"]),
                                        p_(a["vb"]), a["lo"], a["K"], p_(a["post"]), a["ldk"], p_(a["logp"]), p_(a["ws"]),
                                        (a["ws"].numel() * 4 if a["ws"] is not None else 0) if ws_bytes is None else ws_bytes)


def stats_call(eng, L, V2, P2, B, lo, K, gen, w, stats, nll, ws, ws_bytes=None, over=None):
    a = dict(ctx=eng.ctx, V2=V2, P2=P2, B=B, W=L.dW, V=L.V, H=L.H, ldv=L.ldv, ldh=L.ldh, hb=L.dhb, vb=L.dvb, lo=lo, K=K, gen=gen, w=w,
             stats=stats, nll=nll, ws=ws)
    a.update(over or {})             # (a refused call's one wrong argument)
    return eng.lib.mdbn_class_stats(a["ctx"], eng._stream(), p_(a["V2"]), p_(a["P2"]), a["B"], p_(a["W"]), a["V"], a["H"], a["ldv"], a["ldh"],
                                    p_(a["hb"]), p_(a["vb"]), a["lo"], a["K"], a["gen"], a["w"], p_(a["stats"]), p_(a["nll"]), p_(a["ws"]),
                                    (a["ws"].numel() * 4 if a["ws"] is not None else 0) if ws_bytes is None else ws_bytes)


# ------------------------------------------------------------------------------------------------------------------ (a) posterior
# id, V, H, B, boundaries, label group, scale: H = 37 (ldh 40), 513 (more columns than threads), 64; K = 2, 3, 64; the block
# first, last, and between another group and Bernoulli columns; B = 1, 20, 33; "saturated": |z| up to 200
POSTERIOR_CASES = [
    ("first_K2_H37_B1", 21, 37, 1, [0, 2, 7], 0, 0.5),
    ("between_K3_H37_B20", 21, 37, 20, [2, 5, 8], 1, 0.5),
    ("last_K64_H64_B33", 70, 64, 33, [1, 3, 6, 70], 2, 0.3),
    ("last_K3_H513_B33", 30, 513, 33, [4, 8, 27, 30], 2, 0.2),
    ("first_K2_H513_B20", 30, 513, 20, [0, 2, 10], 0, 0.2),
    ("last_K64_H513_B1", 70, 513, 1, [1, 3, 6, 70], 2, 0.2),
    ("between_K3_H64_B33", 21, 64, 33, [2, 5, 8], 1, 0.5),
    ("saturated_K3_H37_B20", 21, 37, 20, [2, 5, 8], 1, 30.0),
]


def compute_units(eng):
    import torch
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


@pytest.mark.parametrize("name,V,H,B,bounds,g,scale", POSTERIOR_CASES, ids=[c[0] for c in POSTERIOR_CASES])
def test_posterior_against_the_twin(hip_engine, name, V, H, B, bounds, g, scale):
    """The new posterior may err at most twice what group_posterior (f32 free energies, float64 finish) errs against the same
    twin on the same case -- same float32 sums over H, different grouping --, the floor being the ``prob`` entry of
    tests/_margins.py.  Both figures are printed and recorded through ``_margins.check``."""
    posterior_case(hip_engine, name, V, H, B, bounds, g, scale)


@pytest.mark.parametrize("name,V,H,B,bounds,g,scale", dn.MANY_ROW_POSTERIOR, ids=[c[0] for c in dn.MANY_ROW_POSTERIOR])
def test_posterior_with_several_rows_per_workgroup(hip_engine, name, V, H, B, bounds, g, scale):
    """The same checks at the same bound where class_forward runs R = 2, 3, 4 rows per workgroup (B from the device's CU
    count: tests/_disc_np.py's ``geometry_cases``), the last batch short or full: waves 1 .. 3 take the softmax of their own
    rows.  The ``between`` rows differ pairwise outside the block, so a row in another wave's slot is an error of order 0.1.
    ``wide``: two column blocks of class_prep (ldv = 1032), the label block across column 1024."""
    eng = hip_engine
    cu = compute_units(eng)
    if isinstance(B, str):
        B, want = dn.geometry_cases(cu)[B]
        assert dn.class_reach(cu, B, bounds[g + 1] - bounds[g], ru4(H) + (4 if H % 4 == 0 else 0), False) == want
    R, G = dn.class_geom(cu, B, bounds[g + 1] - bounds[g], ru4(H) + (4 if H % 4 == 0 else 0), False)
    print("class_posterior %s: %d compute units, B = %d, R = %d, %d workgroups, last batch %d rows" % (name, cu, B, R, G, B - (G - 1) * R))
    posterior_case(eng, name, V, H, B, bounds, g, scale, distinct=name.startswith("between"))


def posterior_case(eng, name, V, H, B, bounds, g, scale, distinct=False):
    import torch
    import mdbn_amd
    L = Layer(eng, V, H, scale, seed=V + H + B)
    rows, W, _, _, lo, K = dn.posterior_inputs(V, H, B, bounds, g, scale, distinct)
    assert np.array_equal(W, L.W)
    if distinct:
        assert dn.distinct_inputs(rows, lo, K) == B
    want, want_lp = dn.posterior(rows, L.W, L.hb, L.vb, lo, K), dn.logp(rows, L.W, L.hb, L.vb, lo, K)
    if name.startswith("saturated"):
        assert np.abs(dn.scores(rows, L.W, L.hb, L.vb, lo, K)[0]).max() > 200
    # the independent witness on the same parameters (a layer of the label group alone where the rows' other groups are no
    # legal softmax groups: group_posterior only looks at the one it is asked for)
    legal = max(np.diff(bounds)) <= 64
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, W=L.W, hbias=L.hb, vbias=L.vb, engine=eng, visible_groups=bounds if legal else [lo, lo + K])
    witness = np.abs(rbm.group_posterior(rows, g if legal else 0) - want).max()
    ldk = K + 3
    need = sizer(eng, B, V, H, L.ldv, L.ldh, K, 0)

    def run():
        v = padded(eng, rows, L.ldv)
        post = torch.full((B, ldk), POISON, dtype=torch.float32, device=eng.device)
        logp = torch.full((B,), POISON, dtype=torch.float32, device=eng.device)
        ws, unchanged = guarded_ws(eng, need)
        assert posterior_call(eng, L, v, lo, K, post, logp, ws, ws_bytes=need) == 0
        eng.synchronize()
        assert unchanged(), "the guard behind the workspace was written"
        assert np.array_equal(bits(v), bits(padded(eng, rows, L.ldv))), "the rows were written"
        return post, logp
    post, logp = run()
    got, got_lp = post.cpu().numpy(), logp.cpu().numpy()
    assert np.isfinite(got[:, :K]).all() and np.isfinite(got_lp).all(), "a pad column was read, or a score overflowed"
    assert np.isnan(got[:, K:]).all(), "columns K.. of post were written"
    err = np.abs(got[:, :K] - want).max()
    lp_scale = max(1.0, np.abs(dn.score_sums(rows, L.W, L.hb, L.vb, lo, K)).max())
    print("class_posterior %s: posterior %.3e (group_posterior %.3e), logp / max|a| %.3e" % (
        name, err, witness, np.abs(got_lp - want_lp).max() / lp_scale))
    check("class_posterior %s: witness group_posterior" % name, witness, 1.0)
    check("class_posterior %s: posterior" % name, err, max(2.0 * witness, SURVEY["prob"]), "prob")
    # (a float32 score is a sum of H softplus terms: SURVEY's free-energy bound, relative to its size)
    check("class_posterior %s: logp / max|a|" % name, np.abs(got_lp - want_lp).max() / lp_scale, 1e-4, "free_energy")
    assert np.abs(got[:, :K].astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6
    best = np.sort(want, axis=1)
    clear = best[:, -1] - best[:, -2] > 1e-4                       # rows whose most probable class is not a near tie
    assert np.array_equal(got[:, :K].argmax(axis=1)[clear], want.argmax(axis=1)[clear]), "another class is the most probable"
    again = run()
    assert np.array_equal(bits(again[0]), bits(post)) and np.array_equal(bits(again[1]), bits(logp)), "two runs differ"
    # without logp what the block holds is ignored
    junk = rows.copy()
    junk[:, lo:lo + K] = 0.25
    post2 = torch.full((B, ldk), POISON, dtype=torch.float32, device=eng.device)
    ws = torch.zeros(need // 4, dtype=torch.float32, device=eng.device)
    assert posterior_call(eng, L, padded(eng, junk, L.ldv), lo, K, post2, None, ws) == 0
    eng.synchronize()
    assert np.array_equal(bits(post2), bits(post))


def test_the_sizer_tells_the_workgroups_of_training_mode(hip_engine):
    """With ldh a multiple of 64 only the partials of T, ru64(G K ldh) floats, make the workspace of modes 1 and 2 depend on K:
    bytes(K = 3) - bytes(K = 2) = 4 G ldh, G the workgroups of ``dn.class_geom`` -- this is how a test knows that the library
    caps them where the mirror does.  No launch.  Last: a layer so wide that 32 Mi floats / (3 ldh) is the smaller cap, for
    K = 3 alone; there G differs between the two K, and with it the [G][64] partials of n."""
    eng = hip_engine
    cu = compute_units(eng)
    V, H, ldv, ldh = 21, 60, 24, 64
    for key, (B, (R, nr, trips)) in dn.geometry_cases(cu).items():
        G = dn.class_geom(cu, B, 3, ldh, True)[1]
        assert dn.class_geom(cu, B, 2, ldh, True) == (R, G) and (G == 4 * cu) == (trips > 1)
        for mode in (1, 2):
            assert sizer(eng, B, V, H, ldv, ldh, 3, mode) - sizer(eng, B, V, H, ldv, ldh, 2, mode) == 4 * G * ldh, (key, mode)
    B = dn.geometry_cases(cu)["16cu+23"][0]
    wide = ru64(dn.CLASS_PARTIAL_FLOATS // (12 * cu) + 64)
    (R, G3), (_, G2) = dn.class_geom(cu, B, 3, wide, True), dn.class_geom(cu, B, 2, wide, True)
    assert G3 == dn.CLASS_PARTIAL_FLOATS // (3 * wide) < 4 * cu == G2

    def partials(G, K):                                 # T, n and nll of G workgroups, every piece a multiple of 64 floats
        return ru64(G * K * wide) + ru64(G * 64) + ru64(G)
    for mode in (1, 2):
        assert sizer(eng, B, V, wide - 4, ldv, wide, 3, mode) - sizer(eng, B, V, wide - 4, ldv, wide, 2, mode) == 4 * (partials(G3, 3) - partials(G2, 2))


# ------------------------------------------------------------------------------------------------------------------ (b) statistics
# id, V, H, B, boundaries (int: groups of K), label group, engine options: the families mdbn_cd_stats dispatches to at the smallest
# shapes of tests/test_gpu_feature_paths.py, a thin batch (B = 20), a whole-tile stack (4 B = 128 rows) and an odd small layer
STATS_CASES = [
    ("skinny_thin_label", 794, 500, 20, [784, 794], 0, {}),
    ("stream", 256, 200, 512, 4, -1, {}),
    ("tiled_f32", 250, 130, 99, MIXED, -1, sf.TILED_F32),
    ("tiled_x6", 250, 130, 99, MIXED, 1, TILED_X6),
    ("whole_tile", 128, 128, 32, [60, 64, 128], 0, {}),
    ("odd_small", 21, 37, 33, [2, 5, 8], 1, {}),
]


@pytest.mark.parametrize("gen,w", [(0.0, 1.0), (1.0, 0.5)], ids=["pure", "hybrid"])
@pytest.mark.parametrize("name,V,H,B,groups,g,opts", STATS_CASES, ids=[c[0] for c in STATS_CASES])
def test_statistics_against_the_twin(built_lib, name, V, H, B, groups, g, opts, gen, w):
    """Host-made operands (the rows, and for the hybrid form the means of a chain) through mdbn_class_stats against the twin at
    the project's bounds: ``stats`` 1e-5 of max |S|, then ``update`` 1e-6 after mdbn_apply_update; the block's rows of S and s_v,
    which the patch kernel makes, on their own."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mdbn_amd
    from mdbn_amd.utils import group_boundaries
    eng = sf.set_options(mdbn_amd.HipEngine(), opts)
    bounds = group_boundaries(groups, V).tolist()
    statistics_case(eng, name, V, H, B, bounds, g % (len(bounds) - 1), 0.3, gen, w)


@pytest.mark.parametrize("gen,w", [(0.0, 1.0), (1.0, 0.5)], ids=["pure", "hybrid"])
@pytest.mark.parametrize("name,V,H,B,bounds,g,scale", dn.MANY_ROW_STATS, ids=[c[0] for c in dn.MANY_ROW_STATS])
def test_statistics_with_several_rows_per_workgroup(built_lib, name, V, H, B, bounds, g, scale, gen, w):
    """The same figures where class_forward runs R = 2 and R = 4 rows per workgroup with a short last batch, and at
    B = 16 cu + 23: 4 cu + 6 batches on the 4 cu workgroups training mode is capped at, so workgroups 0 .. 5 take a second trip
    -- T accumulated in place, n and nll carried, red / p / ystar reused -- and class_patch sums 4 cu partials.  ``saturated``:
    |z| > 200 through the second pass's __expf and exactly one-hot posterior weights.  ``wide``: two column blocks of class_prep,
    the label block across column 1024 (hybrid: the second block's share of s_v).

    The bound: SURVEY's ``stats`` 1e-5 was only ever exercised up to B = 512, so the unchanged mdbn_cd_stats is measured on the
    twin's own stacked operands rounded to float32, against their float64 product, and max(1e-5, 2 x that) is allowed: the class
    path adds two float32 operand roundings and one sum of partials to that product."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mdbn_amd
    eng = mdbn_amd.HipEngine()
    cu = compute_units(eng)
    K, ldh = bounds[g + 1] - bounds[g], ru4(H) + (4 if H % 4 == 0 else 0)
    if isinstance(B, str):
        B, want = dn.geometry_cases(cu)[B]
        assert dn.class_reach(cu, B, K, ldh, True) == want
    R, G = dn.class_geom(cu, B, K, ldh, True)
    print("class_stats %s: %d compute units, B = %d, R = %d, %d workgroups for %d batches" % (name, cu, B, R, G, -(-B // R)))
    statistics_case(eng, name, V, H, B, bounds, g, scale, gen, w, distinct=name.startswith("odd_small"), witnessed=True)


def gemm_witness(eng, L, V2, P2):
    """max |S - float64 product| / max |S| of the unchanged mdbn_cd_stats on float32 operands [2 n, V], [2 n, H]."""
    import torch
    n = V2.shape[0] // 2
    need = C.c_int64()
    assert eng.lib.mdbn_workspace_bytes_ld_ctx(eng.ctx, n, L.V, L.H, L.ldv, L.ldh, C.byref(need)) == 0
    ws = torch.zeros((need.value + 3) // 4, dtype=torch.float32, device=eng.device)
    stats = torch.zeros(L.V * L.ldh + L.ldh + L.ldv + 4, dtype=torch.float32, device=eng.device)
    dV, dP = padded(eng, V2, L.ldv, fill=0.0), padded(eng, P2, L.ldh, fill=0.0)
    assert eng.lib.mdbn_cd_stats(eng.ctx, eng._stream(), p_(dV), p_(dP), n, L.V, L.H, L.ldv, L.ldh, p_(stats), p_(ws), ws.numel() * 4) == 0
    eng.synchronize()
    S = V2.astype(np.float64).T @ P2.astype(np.float64)
    return np.abs(unpack(stats.cpu().numpy(), L.V, L.H, L.ldv, L.ldh)[0] - S).max() / np.abs(S).max()


def statistics_case(eng, name, V, H, B, bounds, g, scale, gen, w, distinct=False, witnessed=False):
    import torch
    import mdbn_amd
    v0, nv, ph, nh, W, _, _, lo, K, rs = dn.stats_inputs(V, H, B, bounds, g, scale, distinct)
    L = Layer(eng, V, H, scale, seed=V + B)
    assert np.array_equal(W, L.W)
    hybrid = gen > 0.0
    ldv, ldh = L.ldv, L.ldh
    n_stats = V * ldh + ldh + ldv + 4
    need = sizer(eng, B, V, H, ldv, ldh, K, 2 if hybrid else 1)
    tag = "class_stats %s %s" % (name, "hybrid" if hybrid else "pure")
    if name.startswith("saturated"):
        assert np.abs(dn.scores(v0, L.W, L.hb, L.vb, lo, K)[0]).max() > 200
    bound = 1e-5
    if witnessed:
        ops = dn.stacked_operands(v0, L.W, L.hb, L.vb, lo, K, gen, w, nv.astype(np.float64), ph.astype(np.float64), nh.astype(np.float64))
        witness = gemm_witness(eng, L, ops[0].astype(np.float32), ops[1].astype(np.float32))
        check(tag + ": witness mdbn_cd_stats on the twin's operands, S / max|S|", witness, 1.0)
        bound = max(1e-5, 2.0 * witness)

    def run():
        V2 = padded(eng, np.concatenate([v0, nv]) if hybrid else v0, ldv)
        P2 = padded(eng, np.concatenate([ph, -nh]), ldh) if hybrid else None
        stats = torch.zeros(n_stats, dtype=torch.float32, device=eng.device)
        stats[V * ldh + ldh + ldv] = 77.0                                       # the CD cost a finished step left
        nll = torch.full((1,), POISON, dtype=torch.float32, device=eng.device)
        ws, unchanged = guarded_ws(eng, need)
        assert stats_call(eng, L, V2, P2, B, lo, K, gen, w, stats, nll, ws, ws_bytes=need) == 0, mdbn_amd._lib.last_error()
        eng.synchronize()
        assert unchanged(), "the guard behind the workspace was written"
        return stats, nll
    stats, nll = run()
    if hybrid:
        S, s_h, s_v = dn.hybrid_stats(v0, L.W, L.hb, L.vb, lo, K, gen, w, nv.astype(np.float64), ph.astype(np.float64), nh.astype(np.float64))
    else:
        S, s_h, s_v = (w * t for t in dn.stats(v0, L.W, L.hb, L.vb, lo, K)[:3])
    want_nll = -dn.logp(v0, L.W, L.hb, L.vb, lo, K).sum()
    gS, gsh, gsv, cost = unpack(stats.cpu().numpy(), V, H, ldv, ldh)
    assert np.isfinite(gS).all() and np.isfinite(gsh).all() and np.isfinite(gsv).all(), "a pad column was read"
    assert np.isfinite(float(nll[0])) and np.isfinite(cost).all()
    top = np.abs(S).max()
    figures = [("S / max|S|", np.abs(gS - S).max() / top), ("label rows of S / max|S|", np.abs(gS[lo:lo + K] - S[lo:lo + K]).max() / top),
               ("s_h / max|s_h|", np.abs(gsh - s_h).max() / np.abs(s_h).max()), ("s_v / max|s_v|", np.abs(gsv - s_v).max() / np.abs(s_v).max()),
               ("label s_v / max|s_v|", np.abs(gsv[lo:lo + K] - s_v[lo:lo + K]).max() / np.abs(s_v).max()),
               ("nll rel", abs(float(nll[0]) - want_nll) / want_nll)]
    if ldv > 1024:                                                              # the second column block of class_prep
        figures.append(("s_v from column 1024 / max|s_v|", np.abs(gsv[1024:] - s_v[1024:]).max() / np.abs(s_v).max()))
    print(tag + ": " + ", ".join("%s %.3e" % f for f in figures) + (", bound %.3e" % bound if witnessed else ""))
    for what, value in figures:
        check("%s: %s" % (tag, what), value, bound, "stats")
    if hybrid:
        assert cost[0] == 77.0, "the CD cost slot was written"
    else:
        assert cost[0] == np.float32(float(nll[0])) and np.array_equal(gsv[:lo], np.zeros(lo)) and np.array_equal(gsv[lo + K:], np.zeros(V - lo - K))
    again = run()
    assert np.array_equal(bits(again[0]), bits(stats)) and np.array_equal(bits(again[1]), bits(nll)), "two runs differ"
    if witnessed:               # (the update rule sees nothing of the launch geometry, and its absolute bound presumes |W| of order 1)
        return
    # the unchanged update rule on these statistics
    s = rbm_np.RBMState(V, H, W=L.W, hbias=L.hb, vbias=L.vb)
    s.W_speed, s.hbias_speed, s.vbias_speed = (0.01 * rs.normal(size=t.shape) for t in (s.W, s.hbias, s.vbias))
    W, Ws = eng.alloc_matrix(V, H, ldh), eng.alloc_matrix(V, H, ldh)
    W.copy_(torch.from_numpy(L.W)); Ws.copy_(torch.from_numpy(s.W_speed.astype(np.float32)))
    dev = [W, Ws, None, eng.to_device(L.hb), eng.to_device(s.hbias_speed.astype(np.float32)), eng.to_device(L.vb),
           eng.to_device(s.vbias_speed.astype(np.float32))]
    s.W_speed, s.hbias_speed, s.vbias_speed = (t.cpu().numpy().astype(np.float64) for t in (dev[1], dev[4], dev[6]))
    eng.apply_update(*dev, stats, 0.1, 0.0, 0.0, 0.0, 0.5, float(B), float(B), 1.0 / B, ldv=ldv)
    dn.update(s, S, s_h, s_v, B, B, 0.1, momentum=0.5)
    eng.synchronize()
    for n, t in zip(PARAMS, (dev[0], dev[3], dev[5], dev[1], dev[4], dev[6])):
        check("%s: %s after the update" % (tag, n), np.abs(t.cpu().numpy() - getattr(s, n)).max(), 1e-6, "update")


# ------------------------------------------------------------------------------------------------------------------ (c) refusals
def test_every_refused_call_leaves_its_outputs_untouched(hip_engine):
    import torch
    from mdbn_amd import _lib
    eng = hip_engine
    V, H, B, lo, K = 21, 37, 5, 5, 3
    L = Layer(eng, V, H, 0.5, seed=1)
    rows = sm.one_hot_data(np.random.RandomState(2), B, V, [2, 5, 8])
    v = padded(eng, rows, L.ldv, fill=0.0)
    V2 = padded(eng, np.concatenate([rows, rows]), L.ldv, fill=0.0)
    P2 = padded(eng, np.random.RandomState(3).uniform(size=(2 * B, H)), L.ldh, fill=0.0)
    post = torch.full((B, K), 3.0, dtype=torch.float32, device=eng.device)
    logp = torch.full((B,), 3.0, dtype=torch.float32, device=eng.device)
    stats = torch.full((V * L.ldh + L.ldh + L.ldv + 4,), 5.0, dtype=torch.float32, device=eng.device)
    nll = torch.full((1,), 7.0, dtype=torch.float32, device=eng.device)
    ws = torch.full((max(sizer(eng, B, V, H, L.ldv, L.ldh, K, m) for m in (0, 1, 2)) // 4,), 9.0, dtype=torch.float32, device=eng.device)
    outs = [post, logp, stats, nll, ws]
    before = [bits(t) for t in outs]
    common = [dict(ctx=None), dict(B=0), dict(B=(1 << 24) + 1), dict(V=0), dict(H=0), dict(H=(1 << 24) + 4), dict(ldv=V - 1), dict(ldv=L.ldv + 2),
              dict(ldh=H - 1), dict(ldh=L.ldh + 2), dict(W=None), dict(W=L.dW.reshape(-1)[1:]), dict(hb=None), dict(vb=None),
              dict(K=1), dict(K=65), dict(lo=-1), dict(lo=V - K + 1), dict(ws=None), dict(ws=ws[1:])]
    for kw in common + [dict(v=None), dict(v=v.reshape(-1)[1:]), dict(post=None), dict(ldk=K - 1)]:
        assert posterior_call(eng, L, v, lo, K, post, logp, ws, over=kw) == -1, kw
        assert _lib.last_error(), kw
    for kw in common + [dict(V2=None), dict(V2=V2.reshape(-1)[1:]), dict(P2=None), dict(P2=P2.reshape(-1)[1:]), dict(stats=None),
                        dict(stats=stats[1:]), dict(gen=-1.0), dict(w=-0.5), dict(gen=0.0, w=0.0), dict(gen=float("nan")), dict(w=float("inf"))]:
        assert stats_call(eng, L, V2, P2, B, lo, K, 1.0, 0.5, stats, nll, ws, over=kw) == -1, kw
        assert _lib.last_error(), kw
    # a short workspace: MDBN_ENOSPC, likewise before any launch
    assert posterior_call(eng, L, v, lo, K, post, logp, ws, ws_bytes=sizer(eng, B, V, H, L.ldv, L.ldh, K, 0) - 4) == -3
    for gen, mode in ((0.0, 1), (1.0, 2)):
        assert stats_call(eng, L, V2, P2, B, lo, K, gen, 0.5, stats, nll, ws, ws_bytes=sizer(eng, B, V, H, L.ldv, L.ldh, K, mode) - 4) == -3
    n = C.c_int64(-5)
    for bad in (dict(B=0), dict(K=1), dict(K=65), dict(mode=3), dict(ldh=H - 1), dict(K=V + 1)):
        a = dict(B=B, V=V, H=H, ldv=L.ldv, ldh=L.ldh, K=K, mode=0)
        a.update(bad)
        assert eng.lib.mdbn_class_workspace_bytes(eng.ctx, a["B"], a["V"], a["H"], a["ldv"], a["ldh"], a["K"], a["mode"], C.byref(n)) == -1, bad
    assert n.value == -5
    eng.synchronize()
    assert all(np.array_equal(a, bits(t)) for a, t in zip(before, outs)), "a refused call wrote something"
    # ... and the good calls go through (P2 is not needed without a chain)
    assert posterior_call(eng, L, v, lo, K, post, logp, ws) == 0
    assert stats_call(eng, L, V2, P2, B, lo, K, 1.0, 0.5, stats, nll, ws) == 0
    assert stats_call(eng, L, V2, None, B, lo, K, 0.0, 0.5, stats, nll, ws) == 0
    eng.synchronize()
    assert not np.array_equal(bits(post), before[0]) and not np.array_equal(bits(stats), before[2])


# ------------------------------------------------------------------------------------------------------------------ (e) public surface
def test_label_posterior_agrees_with_group_posterior(hip_engine):
    label_posterior_case(hip_engine, 40, "")


def test_label_posterior_of_more_rows_than_three_per_compute_unit(hip_engine):
    """label_posterior, predict and label_log_likelihood hand all their rows to ONE mdbn_class_posterior call: N = 3 cu + 1 rows
    run R = 4 rows per workgroup with a last batch of one.  The bounds of the 40-row test."""
    label_posterior_case(hip_engine, dn.geometry_cases(compute_units(hip_engine))["3cu+1"][0], " N=3cu+1")


def label_posterior_case(eng, N, suffix):
    import mdbn_amd
    V, H, bounds = 794, 64, [784, 794]
    rs = np.random.RandomState(5)
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, W=(0.1 * rs.normal(size=(V, H))).astype(np.float32),
                       hbias=(0.1 * rs.normal(size=H)).astype(np.float32), vbias=(0.1 * rs.normal(size=V)).astype(np.float32),
                       engine=eng, visible_groups=bounds)
    rows = sm.one_hot_data(rs, N, V, bounds)
    step = rbm._rng_step
    got, witness = rbm.label_posterior(rows), rbm.group_posterior(rows, 0)
    want = dn.posterior(rows, rbm.W.get_value(), rbm.hbias.get_value(), rbm.vbias.get_value(), 784, 10)
    w_err, err = np.abs(witness - want).max(), np.abs(got - want).max()
    print("label_posterior 794x64" + suffix + ": %.3e against the twin (group_posterior %.3e), %.3e against group_posterior" % (
        err, w_err, np.abs(got - witness).max()))
    check("label_posterior%s: against the twin" % suffix, err, max(2.0 * w_err, SURVEY["prob"]), "prob")
    check("label_posterior%s: against group_posterior" % suffix, np.abs(got - witness).max(), max(3.0 * w_err, SURVEY["prob"]), "prob")
    assert got.dtype == np.float64 and got.shape == (N, 10) and rbm._rng_step == step
    assert np.array_equal(rbm.predict(rows), got.argmax(axis=1))
    lp = rbm.label_log_likelihood(rows)
    a_max = np.abs(dn.score_sums(rows, rbm.W.get_value(), rbm.hbias.get_value(), rbm.vbias.get_value(), 784, 10)).max()
    check("label_log_likelihood%s: / max|a|" % suffix, np.abs(lp - np.log(want[np.arange(N), rows[:, 784:].argmax(axis=1)])).max() / a_max, 1e-4,
          "free_energy")


@pytest.mark.parametrize("name,V,H,B,k,groups,g,gen,w", [("hybrid_label_block", 794, 64, 20, 2, [784, 794], 0, 1.0, 0.5),
                                                        ("hybrid_60x24", 60, 24, 33, 1, 5, 3, 0.5, 2.0),
                                                        ("pure_60x24", 60, 24, 33, 1, 5, -1, 0.0, 1.0),
                                                        ("pure_60x24_cu+1", 60, 24, "cu+1", 1, 5, -1, 0.0, 1.0)],
                         ids=["hybrid_label_block", "hybrid_60x24", "pure_60x24", "pure_60x24_cu+1"])
def test_steps_against_the_teacher_forced_twin(built_lib, name, V, H, B, k, groups, g, gen, w):
    """Steps through the public classes against the float64 loop that follows the device's recorded chain: the packed
    statistics the update read, ``discriminative_cost``, then parameters and speeds.  ``cu+1``: a minibatch of one row more
    than the device has compute units, R = 2 rows per workgroup of class_forward with a last batch of one."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mdbn_amd
    from mdbn_amd.utils import group_boundaries
    eng = mdbn_amd.HipEngine()
    if isinstance(B, str):
        B = dn.geometry_cases(compute_units(eng))[B][0]
    bounds = group_boundaries(groups, V).tolist()
    n_groups = len(bounds) - 1
    lo, K = bounds[g % n_groups], bounds[g % n_groups + 1] - bounds[g % n_groups]
    rs = np.random.RandomState(31)
    N, seed = 3 * B + 7, 7
    data = sm.one_hot_data(rs, N, V, bounds)
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(123), theano_rng=mdbn_amd.RandomStreams(seed), engine=eng,
                       visible_groups=groups)
    st = rbm_np.RBMState(V, H, W=rbm.W.get_value())
    st.freeze_W0()
    _, up = rbm.get_cost_updates(k=k, batch_size=B, discriminative=w, label_group=g, generative=gen, **sf.GROUPED_HP)
    fn = mdbn_amd.function(up, mdbn_amd.shared(data, engine=eng), data_parallel=None)
    eng.trace_chain = True
    try:
        for t, mom in enumerate(sf.MOMENTA):
            idx = rs.permutation(N)[:B]
            v0 = data[idx].astype(np.float64)
            want_nll = -dn.logp(v0, st.W, st.hbias, st.vbias, lo, K).mean()
            c = float(fn(indexes=idx, momentum=mom))
            if gen > 0.0:
                sc = eng.last_scratch
                ph, _, out, differ = sm.cd_chain(st, v0, PhiloxDraws(seed, rbm.stream_id, t), k, bounds,
                                                 trace_h=sc.trace_h.cpu().numpy()[:, :, :H], trace_v=sc.trace_v.cpu().numpy()[:, :, :V])
                assert differ <= sf.draw_cap(B, V, H, k, bounds, False)
                S, s_h, s_v = dn.hybrid_stats(v0, st.W, st.hbias, st.vbias, lo, K, gen, w, out[1], ph, out[4])
                want_cost = sm.grouped_cost(out[0], v0, bounds) / B
            else:
                S, s_h, s_v = (w * x for x in dn.stats(v0, st.W, st.hbias, st.vbias, lo, K)[:3])
                want_cost = want_nll
            check("disc step %s: cost rel" % name, abs(c - want_cost) / abs(want_cost), 1e-5)
            check("disc step %s: discriminative_cost rel" % name, abs(fn.discriminative_cost - want_nll) / want_nll, 1e-5)
            gS, gsh, gsv, _ = unpack(fn._stats_slots[0].cpu().numpy(), V, H, ru4(V), rbm.W.tensor.stride(0))
            check("disc step %s: S / max|S|" % name, np.abs(gS - S).max() / np.abs(S).max(), 1e-5, "stats")
            check("disc step %s: s_h / max|s_h|" % name, np.abs(gsh - s_h).max() / np.abs(s_h).max(), 1e-5, "stats")
            check("disc step %s: s_v / max|s_v|" % name, np.abs(gsv - s_v).max() / np.abs(s_v).max(), 1e-5, "stats")
            dn.update(st, S, s_h, s_v, B, B, sf.GROUPED_HP["lr"], momentum=mom, weightcost=sf.GROUPED_HP["weightcost"])
    finally:
        eng.trace_chain = False
    for n in PARAMS:
        err = np.abs(getattr(rbm, n).get_value() - getattr(st, n)).max()
        print("disc step %s: %s %.3e" % (name, n, err))
        check("disc step %s: %s after %d steps" % (name, n, len(sf.MOMENTA)), err, 2e-6, "update")
    assert rbm._rng_step == len(sf.MOMENTA)


def test_discriminative_training_learns_the_toy_problem(hip_engine):
    """tests/test_disc_twin.py's problem through RBM.training(discriminative=1.0, generative=0.0): the same caps."""
    import mdbn_amd
    eng = hip_engine
    rows, lo, K, W = dn.toy_problem()
    T = dn.TOY
    rbm = mdbn_amd.RBM(n_visible=rows.shape[1], n_hidden=T["H"], W=W, engine=eng, visible_groups=[lo, lo + K])
    before = -rbm.label_log_likelihood(rows).mean()
    hist = rbm.training(rows, None, T["steps"], batch_size=T["B"], learning_rate=T["lr"], persistent=False, discriminative=1.0,
                        generative=0.0)
    after = -rbm.label_log_likelihood(rows).mean()
    acc = float((rbm.predict(rows) == rows[:, lo:].argmax(axis=1)).mean())
    print("toy on the device: NLL %.4f -> %.4f, accuracy %.3f" % (before, after, acc))
    assert len(hist) == T["steps"] and abs(hist[0][0] - before) <= 1e-4 * before      # the monitor of a pure step is the NLL
    assert acc >= 0.9 and after <= 0.5 * before


def test_a_resumed_discriminative_run_continues_bit_for_bit(hip_engine, tmp_path):
    import mdbn_amd
    from mdbn_amd import checkpoint
    mdbn_amd.DBN.verbose = False
    eng = hip_engine
    V, H, K = 60, 24, 5
    x = sm.one_hot_data(np.random.RandomState(0), 40, V, list(range(0, V + 1, K)))
    kw = dict(k=1, weightcost=2e-4, batch_size=10, discriminative=0.5, generative=1.0)

    def fresh(net):
        _, up = net.rbm_layers[0].get_cost_updates(0.05, **kw)
        return mdbn_amd.function(up, mdbn_amd.shared(x, engine=eng), data_parallel=None)
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, gauss=False, hidden_layers_sizes=[], n_outs=H, engine=eng,
                       visible_groups=K)
    fn = fresh(net)
    for t in range(2):
        fn(indexes=np.arange(10) + 10 * t, momentum=0.5)
    path = str(tmp_path / "disc.npz")
    checkpoint.save_network(path, {'cn': net}, resume=True)
    want = [(float(fn(indexes=np.arange(10) + 10 * t, momentum=0.5)), fn.discriminative_cost) for t in (2, 3)]
    net2 = checkpoint.load_network(path, engine=eng)['cn']
    fn2 = fresh(net2)
    got = [(float(fn2(indexes=np.arange(10) + 10 * t, momentum=0.5)), fn2.discriminative_cost) for t in (2, 3)]
    assert got == want
    for n in PARAMS:
        assert np.array_equal(getattr(net2.rbm_layers[0], n).get_value(), getattr(net.rbm_layers[0], n).get_value()), n
