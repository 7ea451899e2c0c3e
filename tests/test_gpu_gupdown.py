"""Up-down fine-tuning of stacks with categorical visible units on the device: (a) the grouped generative rule alone
(csrc/mdbn_updown.hip: updown_gen_grouped_kernel, and the composed path, through mdbn_updown_gen_step_grouped) against the float64
twin (tests/_gupdown_np.py) fed the device's own inputs, with poisoned pad columns, determinism, the plain kernel's bits outside
the span, a saturated group, the shapes that fall back, the bound's directed term, and every MDBN_EINVAL case; (b) four whole
steps of a DBN 60 -> 24 -> 12 with K = 5 and of a forest (grouped 40 -> 16 with K = 4, Gaussian 30 -> 12, joint 28 -> 16 -> 8)
against the twin loop teacher-forced along the device's recorded samples, on both paths, and the checkpoint round trip.

  (V, H, ldh)       groups                                           what it reaches
  (12, 7, 8)        bounds 1, 4, 7, 9 behind one Bernoulli column,   a pad column, every kind of row in one workgroup
                    three after
  (70, 66, 68)      2, 64, 3 behind a Bernoulli column               4 rows per workgroup: a 64-row group over sixteen nominal
                                                                     ranges, empty workgroups, one ragged 16-byte group per lane
  (300, 510, 512)   60 x K = 5                                       two 16-byte groups per lane, ragged H
  (794, 500, 500)   the label block [784, 794)                       a span in the last workgroups only
  (8200, 36, 36)    1640 x K = 5                                     33 rows per workgroup on 256 CUs: groups across nominal edges

Bounds, the project's own (tests/test_gpu_updown.py): parameters and speeds 2e-6 of max(1, max |reference|), probabilities 2e-6,
cost 1e-5 relative; the directed term of the bound 1e-4 relative (_margins: free_energy)."""
import ctypes as C

import numpy as np
import pytest

import _gupdown_np as gud
import _softmax_np as sm
import _updown_np as ud
from _margins import check

pytestmark = pytest.mark.gpu

NAN = float("nan")
SHAPES = [((12, 7, 8), [1, 4, 7, 9]), ((70, 66, 68), [1, 3, 67, 70]), ((300, 510, 512), list(range(0, 301, 5))),
          ((794, 500, 500), [784, 794]), ((8200, 36, 36), list(range(0, 8201, 5)))]
SHAPE_IDS = ["12x7", "70x66", "300x510", "794x500", "8200x36"]
# (n, momentum, weightcost, lambda_1, batch_size): the rules of tests/test_gpu_updown.py without the Gaussian flag
RULES = [(1, 0.0, 0.0, 0.0, 1), (20, 0.5, 2e-4, 0.0, 32), (32, 0.5, 0.0, 0.01, 20)]
RULE_IDS = ["n1", "n20_ragged", "n32_all_terms"]


def dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def bits(t):
    return t.detach().cpu().numpy().view(np.int32).copy()


def matrix(eng, rows, cols, ld, values, poison):
    full = np.full((rows, ld), NAN if poison else 0.0, dtype=np.float32)
    full[:, :cols] = values
    return dev(eng, full)[:, :cols], full


def layer(eng, V, H, ldh, bounds, n, seed, poison, saturate=None):
    """The buffers of a generative call and their host values; ``saturate`` = (lo, hi): the pre-activations of those rows of G
    alternate +-80 (column 0 of x_hi is all ones and carries them)."""
    rs = np.random.RandomState(seed)
    ldv = (V + 3) & ~3
    out = {}
    G = rs.normal(0, 1.0 / np.sqrt(H), (V, H))
    x_hi = (rs.uniform(size=(n, H)) < 0.4).astype(np.float64)
    if saturate is not None:
        lo, hi = saturate
        G[lo:hi, :] *= 1e-3
        G[lo:hi, 0] = 80.0 * (-1.0) ** np.arange(hi - lo)
        x_hi[:, 0] = 1.0
    out["G"], out["G0"] = matrix(eng, V, H, ldh, G, poison)
    out["Gs"], out["Gs0"] = matrix(eng, V, H, ldh, rs.normal(0, 0.01, (V, H)), poison)
    out["x_hi"], out["x_hi0"] = matrix(eng, n, H, ldh, x_hi, poison)
    out["x_lo"], out["x_lo0"] = matrix(eng, n, V, ldv, sm.one_hot_data(rs, n, V, bounds), poison)
    for name, size in (("c", V), ("cs", V), ("b", H), ("bs", H)):
        out[name + "0"] = rs.normal(0, 0.3 if len(name) == 1 else 0.01, size).astype(np.float32)
        out[name] = dev(eng, out[name + "0"])
    return out


def scaled(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


def hp_of(rule):
    n, mom, wc, l1, bs = rule
    return dict(lr=0.05, momentum=mom, weightcost=wc, lambda_1=l1, lambda_2=0.01, batch_size=bs)


def table(eng, bounds):
    from mdbn_amd.engine import GroupTable
    return GroupTable(eng, np.asarray(bounds, dtype=np.int32))


def gen_once(eng, V, H, ldh, bounds, rule, path, seed=5, plain=False, saturate=None):
    n, hp = rule[0], hp_of(rule)
    L = layer(eng, V, H, ldh, bounds, n, seed, poison=(path == "fused"), saturate=saturate)
    args = (hp["lr"], hp["lambda_1"], hp["lambda_2"], hp["weightcost"], hp["momentum"], hp["batch_size"], n)
    if plain:
        cost = eng.updown_gen_step(L["x_lo"], L["x_hi"], L["G"], L["Gs"], L["c"], L["cs"], False, *args, cost_scale=1.0 / n, path=path)
    else:
        cost = eng.updown_gen_step_grouped(L["x_lo"], L["x_hi"], L["G"], L["Gs"], L["c"], L["cs"], table(eng, bounds), *args,
                                           cost_scale=1.0 / n, path=path)
    return L, float(cost), hp


def gen_check(eng, V, H, ldh, bounds, rule, path, saturate=None):
    n = rule[0]
    L, cost, hp = gen_once(eng, V, H, ldh, bounds, rule, path, saturate=saturate)
    tw = ud.untie(dict(W=L["G0"][:, :H], G=L["G0"][:, :H], Gs=L["Gs0"][:, :H], b=L["b0"], c=L["c0"], cs=L["cs0"], gauss=False,
                       bounds=bounds))
    want = gud.gen_step(tw, L["x_lo0"][:, :V], L["x_hi0"][:, :H], hp, n) / n
    tag = "gupdown gen %s %dx%d n=%d%s" % (path, V, H, n, " saturated" if saturate else "")
    figs = [("G", scaled(L["G"].cpu().numpy(), tw["G"])), ("G_speed", scaled(L["Gs"].cpu().numpy(), tw["Gs"])),
            ("vbias", scaled(L["c"].cpu().numpy(), tw["c"])), ("vbias_speed", scaled(L["cs"].cpu().numpy(), tw["cs"]))]
    print("%s: %s, cost rel %.3e" % (tag, ", ".join("%s %.3e" % f for f in figs), abs(cost - want) / abs(want)))
    for name, err in figs:
        check("gupdown gen (%s): %s / max(1, max|ref|)" % (path, name), err, 2e-6, "update")
    check("gupdown gen (%s): cost rel" % path, abs(cost - want) / abs(want), 1e-5)
    assert np.isfinite(cost) and all(np.isfinite(L[k].cpu().numpy()).all() for k in ("G", "Gs", "c", "cs"))
    if path == "fused":                               # pad columns: neither read nor written
        for name in ("G", "Gs"):
            full = L[name]._base.cpu().numpy()
            assert np.array_equal(full[:, H:].view(np.int32), L[name + "0"][:, H:].view(np.int32)), "a pad column of %s was written" % name
    assert np.array_equal(L["x_lo"].cpu().numpy(), L["x_lo0"][:, :V]) and np.array_equal(L["x_hi"].cpu().numpy(), L["x_hi0"][:, :H])
    assert np.array_equal(L["b"].cpu().numpy(), L["b0"]) and np.array_equal(L["bs"].cpu().numpy(), L["bs0"])     # the hidden half
    again, cost2, _ = gen_once(eng, V, H, ldh, bounds, rule, path, saturate=saturate)
    for name in ("G", "Gs", "c", "cs"):
        assert np.array_equal(bits(again[name]), bits(L[name])), "two runs differ in %s" % name
    assert cost2 == cost
    return L, cost


# ------------------------------------------------------------------------------------------------------------------ (a) kernels
@pytest.mark.parametrize("path", ["fused", "composed"])
@pytest.mark.parametrize("rule", RULES, ids=RULE_IDS)
@pytest.mark.parametrize("shape,bounds", SHAPES, ids=SHAPE_IDS)
def test_grouped_generative_rule_against_the_twin(hip_engine, shape, bounds, rule, path):
    eng, (V, H, ldh), n = hip_engine, shape, rule[0]
    L, cost = gen_check(eng, V, H, ldh, bounds, rule, path)
    # the cost is minus the directed term of the bound on the same (x_hi, G, vbias, x_lo), pre-step parameters
    fresh = layer(eng, V, H, ldh, bounds, n, 5, poison=False)
    ll = eng.propdown_row_loglik_grouped(fresh["x_hi"], fresh["G"], fresh["c"], fresh["x_lo"], table(eng, bounds)).cpu().numpy()
    check("gupdown gen (%s): cost n against -sum propdown_row_loglik_grouped, rel" % path,
          abs(cost * n + float(ll.astype(np.float64).sum())) / abs(cost * n), 1e-4, "free_energy")
    if path == "fused":
        # rows outside the span: the plain one-pass kernel's bits on the same inputs
        P, _, _ = gen_once(eng, V, H, ldh, bounds, rule, "fused", plain=True)
        out = sm.bernoulli_columns(bounds, V)
        for name in ("G", "Gs"):
            assert np.array_equal(bits(L[name])[out], bits(P[name])[out]), "a row of %s outside the span differs from the plain kernel's" % name
        for name in ("c", "cs"):
            assert np.array_equal(bits(L[name])[out], bits(P[name])[out]), name


@pytest.mark.parametrize("n", [5, 13, 29])
def test_grouped_generative_rule_at_the_other_padded_batch_widths(hip_engine, n):
    (V, H, ldh), bounds = SHAPES[2]
    gen_check(hip_engine, V, H, ldh, bounds, (n, 0.5, 2e-4, 0.0, 20), "fused")


@pytest.mark.parametrize("path", ["fused", "composed"])
def test_a_saturated_group_of_64_rows_stays_finite(hip_engine, path):
    """Pre-activations alternating +-80 inside the 64-row group: exp(-160) underflows, the cost comes from the log-sum-exp."""
    (V, H, ldh), bounds = SHAPES[1]
    gen_check(hip_engine, V, H, ldh, bounds, RULES[1], path, saturate=(3, 67))


@pytest.mark.parametrize("V,H,ldh,n,bounds", [(300, 40, 40, 33, list(range(0, 301, 5))), (64, 516, 516, 20, [2, 10, 64])])
def test_shapes_outside_the_one_pass_regime_take_the_composed_path(hip_engine, V, H, ldh, n, bounds):
    from mdbn_amd import MdbnError
    eng = hip_engine
    rule = (n, 0.5, 2e-4, 0.0, 20)
    auto, cost_a, _ = gen_once(eng, V, H, ldh, bounds, rule, "auto")
    comp, cost_c, _ = gen_once(eng, V, H, ldh, bounds, rule, "composed")
    for name in ("G", "Gs", "c", "cs"):
        assert np.array_equal(bits(auto[name]), bits(comp[name])), name
    assert cost_a == cost_c
    with pytest.raises(MdbnError):
        gen_once(eng, V, H, ldh, bounds, rule, "fused")


def test_every_einval_case_returns_without_touching_its_outputs(hip_engine):
    import torch
    from mdbn_amd import _lib
    eng, lib = hip_engine, hip_engine.lib
    V, H, ldh, n = 100, 24, 24, 20
    ldv = V
    bounds = [10, 13, 77, 80]
    L = layer(eng, V, H, ldh, bounds, n, 2, poison=False)
    cost = torch.zeros(4, dtype=torch.float32, device=eng.device)
    need = C.c_int64()
    _lib.check(lib.mdbn_updown_gen_grouped_workspace_bytes(eng.ctx, n, V, H, ldv, ldh, 2, C.byref(need)), "gen sizer")
    ws = torch.zeros(need.value // 4 + 8, dtype=torch.float32, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    good = table(eng, bounds)

    def upd(**kw):
        u = _lib.UpdateArgs()
        u.W, u.W_speed = L["G"].data_ptr(), L["Gs"].data_ptr()
        u.vbias, u.vbias_speed = L["c"].data_ptr(), L["cs"].data_ptr()
        u.V, u.H, u.ldv, u.ldh = V, H, ldv, ldh
        u.lr, u.momentum, u.batch_size, u.n_rows, u.cost_scale = 0.05, 0.5, 20.0, float(n), 1.0
        for k, v in kw.items():
            setattr(u, k, v)
        return u

    def gen(u=None, x_lo=L["x_lo"], x_hi=L["x_hi"], n=n, path=0, ws=ws, ws_bytes=None, ctx=eng.ctx, cost=cost, tab=good, host=None,
            n_groups=None, no_dev=False, no_host=False):
        u = upd() if u is None else u
        host = tab.host if host is None else np.ascontiguousarray(host, dtype=np.int32)
        return lib.mdbn_updown_gen_step_grouped(
            ctx, eng._stream(), p(x_lo), p(x_hi), n, C.byref(u) if u is not False else None, p(cost), path, p(ws),
            need.value if ws_bytes is None else ws_bytes, None if no_dev else p(tab.tensor),
            None if no_host else C.c_void_p(host.ctypes.data), len(host) - 1 if n_groups is None else n_groups)

    watched = [L[k]._base if L[k]._base is not None else L[k] for k in ("G", "Gs", "c", "cs", "b", "bs")] + [cost, ws]
    before = [bits(t) for t in watched]
    misaligned = L["x_lo"]._base.reshape(-1)[1:1 + n * ldv]
    bad = [dict(n_groups=0), dict(n_groups=-1), dict(n_groups=51),                     # the plain call exists; more than V / 2
           dict(host=[10, 13, 12, 80]), dict(host=[10, 11, 77, 80]), dict(host=[10, 13, 78, 80]),     # descending; K = 1; K = 65
           dict(host=[10, 13, 77, 101]), dict(host=[-1, 13, 77, 80]), dict(no_dev=True), dict(no_host=True),
           # ... and whatever mdbn_updown_gen_step refuses
           dict(n=0), dict(n=-1), dict(x_lo=None), dict(x_hi=None), dict(ws=None), dict(ctx=None), dict(u=False),
           dict(x_lo=misaligned), dict(ws=ws[1:]), dict(path=3), dict(path=-1), dict(ws_bytes=need.value - 4, path=2),
           dict(ws_bytes=0), dict(cost=cost.view(torch.uint8)[1:]),
           dict(u=upd(V=0)), dict(u=upd(H=0)), dict(u=upd(ldh=H - 4)), dict(u=upd(ldh=H + 2)), dict(u=upd(ldv=V + 2)),
           dict(u=upd(W=None)), dict(u=upd(W_speed=None)), dict(u=upd(vbias=None)), dict(u=upd(vbias_speed=None)),
           dict(u=upd(hbias=L["b"].data_ptr())), dict(u=upd(batch_size=0.0)), dict(u=upd(n_rows=-1.0)), dict(u=upd(phase=1)),
           dict(u=upd(struct_size=8)), dict(u=upd(W=L["G"].data_ptr() + 4)),
           dict(n=33, path=1), dict(u=upd(H=516, ldh=516), path=1)]
    for kw in bad:
        assert gen(**kw) == -1, kw
        assert _lib.last_error(), kw
    bytes_out = C.c_int64(-7)
    assert lib.mdbn_updown_gen_grouped_workspace_bytes(eng.ctx, 33, V, H, ldv, ldh, 1, C.byref(bytes_out)) == -1 and bytes_out.value == -7
    assert lib.mdbn_updown_gen_grouped_workspace_bytes(eng.ctx, n, V, 516, ldv, 516, 1, C.byref(bytes_out)) == -1 and bytes_out.value == -7
    assert lib.mdbn_updown_gen_grouped_workspace_bytes(eng.ctx, n, V, H, ldv, ldh, 0, None) == -1
    eng.synchronize()
    assert all(np.array_equal(a, bits(t)) for a, t in zip(before, watched)), "a refused call wrote something"
    assert gen() == 0 and gen(path=2) == 0               # ... and the same arguments without the fault are accepted
    eng.synchronize()


# ------------------------------------------------------------------------------------------------------------------ (b) whole steps
STEPS = 4
HP = dict(lr=0.05, top_lr=0.03, k=1, momentum=0.5, weightcost=2e-4, lambda_1=0.0, lambda_2=0.01, batch_size=20)
NAMES = (("W", "W"), ("hbias", "b"), ("vbias", "c"), ("W_speed", "Ws"), ("hbias_speed", "bs"), ("vbias_speed", "cs"),
         ("W_gen", "G"), ("W_gen_speed", "Gs"))
K5, K4 = list(range(0, 61, 5)), list(range(0, 41, 4))


def make_dbn(eng, sizes, gauss, seed, bounds=None):
    import mdbn_amd
    mdbn_amd.DBN.verbose = False
    rs = np.random.RandomState(seed)
    Ws = [(rs.normal(0, 1, (a, b)) / np.sqrt(a)).astype(np.float32) for a, b in zip(sizes[:-1], sizes[1:])]
    bs = [rs.normal(0, 0.3, b).astype(np.float32) for b in sizes[1:]]
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(seed), theano_rng=mdbn_amd.RandomStreams(50 + seed), n_ins=sizes[0],
                       gauss=gauss, hidden_layers_sizes=list(sizes[1:-1]), n_outs=sizes[-1], W_list=Ws, b_list=bs, engine=eng,
                       visible_groups=bounds)
    for r in net.rbm_layers:
        r.vbias.set_value(rs.normal(0, 0.3, r.n_visible).astype(np.float32))
    return net


def twin_net(net):
    out = []
    for r in net.rbm_layers:
        l = ud.untie(dict(W=r.W.get_value(), b=r.hbias.get_value(), c=r.vbias.get_value(), gauss=r.gauss, noisy=False,
                          seed=r.theano_rng.seed, stream=r.stream_id, step=r._rng_step))
        if r.visible_groups is not None:
            l["bounds"] = [int(b) for b in r.visible_groups.host]
        out.append(l)
    return out


def run_steps(eng, nets, joint, tables, path):
    """STEPS up-down steps on the device, each followed by the twin's teacher-forced along the samples the device drew."""
    from mdbn_amd import updown
    model = dict(bottoms=[twin_net(n) for n in nets], joint=twin_net(joint) if joint is not None else None)
    top = (joint if joint is not None else nets[0]).rbm_layers[-1]
    hp = updown.Hyper(HP["lr"], HP["top_lr"], HP["k"], HP["momentum"], HP["weightcost"], HP["lambda_1"], HP["lambda_2"],
                      HP["batch_size"], path)
    rs = np.random.RandomState(3)
    n_rows = [20, 20, 13, 1]                            # the preset's batch, a ragged one, a single row
    flips = ties = dreams = 0
    eng.trace_chain = True
    try:
        for t in range(STEPS):
            idx = rs.permutation(len(tables[0]))[:n_rows[t]]
            rec = updown.step(nets, joint, [eng.to_device(x[idx]) for x in tables], hp)
            sc = eng.last_scratch
            Vt, Ht = top.n_visible, top.n_hidden
            forced = (sc.trace_h.cpu().numpy()[:, :n_rows[t], :Ht], sc.trace_v.cpu().numpy()[:, :n_rows[t], :Vt])
            assert np.array_equal(rec.y[-1][-1].cpu().numpy(), forced[1][-1])
            nb = len(nets)
            recorded = [s.cpu().numpy() for m in range(nb) for s in rec.x[m][1:]]
            if joint is not None:
                recorded += [s.cpu().numpy() for s in rec.x[nb][1:]]
                recorded += [s.cpu().numpy() for s in reversed(rec.y[nb][:-1])]
                recorded += [s.cpu().numpy() for m in range(nb) for s in reversed(rec.y[m][:-1])]
            else:
                recorded += [s.cpu().numpy() for s in reversed(rec.y[0][:-1])]
            # every y_0 row of a grouped layer is one-hot per group
            for m, net in enumerate(nets):
                g = net.rbm_layers[0].visible_groups
                if g is not None:
                    y0 = rec.y[m][0].cpu().numpy()
                    assert np.isin(y0, (0.0, 1.0)).all() and all((y0[:, lo:hi].sum(axis=1) == 1).all() for lo, hi in g.spans())
            draws = gud.Draws(recorded, tie=1e-6)
            want = gud.step(model, [x[idx] for x in tables], HP, draws, forced_top=forced)
            assert not draws.recorded, "the twin drew fewer samples than the device"
            flips, ties, dreams = flips + draws.flips, ties + draws.ties, dreams + len(draws.dreams)
            for m in range(len(rec.r)):
                for got, ref in zip(rec.r[m], want["r"][m]):
                    check("gupdown step (%s): r of the dream" % path, np.abs(got.cpu().numpy() - ref).max(), 2e-6, "prob")
            gen = sum(float(c) for c in rec.gen_cost)
            check("gupdown step (%s): generative cost rel" % path, abs(gen - want["gen_cost"]) / abs(want["gen_cost"]), 1e-5)
            check("gupdown step (%s): top cost rel" % path, abs(float(rec.top_cost) - want["top_cost"]) / abs(want["top_cost"]), 1e-5)
    finally:
        eng.trace_chain = False
    # no draw differs from the twin's beyond _softmax_np's tie cap (sm.follow asserts every difference IS a tie), and the twin
    # alone stays within that cap
    assert dreams == STEPS and flips <= sm.TIE_CAP and ties <= sm.TIE_CAP, (dreams, flips, ties)
    figs = []
    for net, tw in zip(list(nets) + ([joint] if joint is not None else []), model["bottoms"] + ([model["joint"]] if joint is not None else [])):
        for r, l in zip(net.rbm_layers, tw):
            assert r._rng_step == l["step"]
            for attr, key in NAMES:
                if getattr(r, attr) is not None:
                    figs.append(("%s[%dx%d]" % (attr, r.n_visible, r.n_hidden), scaled(getattr(r, attr).get_value(), l[key])))
    print("gupdown steps (%s): %s" % (path, ", ".join("%s %.3e" % f for f in figs)))
    for name, err in figs:
        check("gupdown %d steps (%s): %s / max(1, max|ref|)" % (STEPS, path, name.split("[")[0]), err, 2e-6, "update")
    return {(i, j, attr): getattr(r, attr).get_value() for i, net in enumerate(list(nets) + ([joint] if joint is not None else []))
            for j, r in enumerate(net.rbm_layers) for attr, _ in NAMES if getattr(r, attr) is not None}


@pytest.mark.parametrize("path", ["fused", "composed"])
def test_four_steps_of_a_dbn_with_groups(hip_engine, path, tmp_path):
    from mdbn_amd import checkpoint
    eng = hip_engine
    data = sm.one_hot_data(np.random.RandomState(4), 64, 60, K5)
    net = make_dbn(eng, (60, 24, 12), False, 11, K5)
    first = run_steps(eng, [net], None, [data], path)
    again = run_steps(eng, [make_dbn(eng, (60, 24, 12), False, 11, K5)], None, [data], path)
    for key in first:
        assert np.array_equal(first[key], again[key]), "two runs differ in %r" % (key,)
    # the checkpoint keeps the generative weights of the grouped layer
    file = str(tmp_path / "untied.npz")
    checkpoint.save_network(file, {"net": net}, resume=True)
    back = checkpoint.load_network(file, engine=eng)["net"]
    r, q = net.rbm_layers[0], back.rbm_layers[0]
    assert q.visible_groups is not None and np.array_equal(q.visible_groups.host, r.visible_groups.host)
    assert np.array_equal(r.W_gen.get_value(), q.W_gen.get_value()) and np.array_equal(r.W_gen_speed.get_value(), q.W_gen_speed.get_value())
    assert np.abs(r.W_gen.get_value() - r.W.get_value()).max() > 1e-4 and back.rbm_layers[-1].W_gen is None


@pytest.mark.parametrize("path", ["fused", "composed"])
def test_four_steps_of_a_forest_with_a_grouped_modality(hip_engine, path):
    eng = hip_engine
    rs = np.random.RandomState(5)
    tables = [sm.one_hot_data(rs, 48, 40, K4), rs.normal(0, 1, (48, 30)).astype(np.float32)]

    def stack():
        return [make_dbn(eng, (40, 16), False, 21, K4), make_dbn(eng, (30, 12), True, 22)], make_dbn(eng, (28, 16, 8), False, 23)
    nets, joint = stack()
    first = run_steps(eng, nets, joint, tables, path)
    nets, joint = stack()
    again = run_steps(eng, nets, joint, tables, path)
    for key in first:
        assert np.array_equal(first[key], again[key]), "two runs differ in %r" % (key,)
