"""Up-down fine-tuning on the device: (a) the two delta-rule calls alone (csrc/mdbn_updown.hip through mdbn_updown_gen_step /
mdbn_updown_rec_step) against the float64 twin (tests/_updown_np.py) fed the device's own inputs, on the one-pass and the
composed path, with poisoned pad columns, determinism, the shapes that fall back, and every MDBN_EINVAL case; (b) four whole
steps of a 3-layer DBN and of a two-modality stack against the twin loop teacher-forced along the device's recorded samples,
on both paths; (c) no bf16 plane of a weight matrix is stale after a step.

Pad columns are poisoned with NaN on the one-pass generative path only: that kernel neither reads nor writes them.  The composed
path and the recognition half walk the pad columns through the CD step's own GEMMs and update kernels, as every CD step does
(they hold zeros there), so those runs keep zero pads and make no claim about them.

Bounds: those of the whole-step tests of tests/test_gpu_center.py -- parameters and speeds 2e-6 of max(1, max |reference|),
probabilities 2e-6, cost 1e-5 relative."""
import ctypes as C

import numpy as np
import pytest

import _updown_np as ud
from _margins import check

pytestmark = pytest.mark.gpu

NAN = float("nan")
# (V, H, ldh): tiny with a pad column; the widest row the one-pass kernel takes; the preset's 784 -> 500; more workgroups than
# CUs on a narrow row; the 19 937-gene layer
SHAPES = [(12, 7, 8), (300, 512, 512), (784, 500, 500), (8200, 36, 36)]
# (n, gauss, momentum, weightcost, lambda_1, batch_size): one row; the preset's batch, Gaussian, ragged against batch_size;
# a full tile of 32 rows with every term of the rule on
RULES = [(1, False, 0.0, 0.0, 0.0, 1), (20, True, 0.5, 2e-4, 0.0, 32), (32, False, 0.5, 0.0, 0.01, 20)]


def dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def bits(t):
    return t.detach().cpu().numpy().view(np.int32).copy()


def matrix(eng, rs, rows, cols, ld, values, poison):
    """A device matrix [rows, cols] on leading dimension ld (pad columns NaN or zero) and its host values."""
    full = np.full((rows, ld), NAN if poison else 0.0, dtype=np.float32)
    full[:, :cols] = values
    return dev(eng, full)[:, :cols], full


def layer(eng, V, H, ldh, n, gauss, seed, poison):
    rs = np.random.RandomState(seed)
    ldv = (V + 3) & ~3
    out = {}
    out["G"], out["G0"] = matrix(eng, rs, V, H, ldh, rs.normal(0, 1.0 / np.sqrt(H), (V, H)), poison)
    out["Gs"], out["Gs0"] = matrix(eng, rs, V, H, ldh, rs.normal(0, 0.01, (V, H)), poison)
    out["x_hi"], out["x_hi0"] = matrix(eng, rs, n, H, ldh, rs.uniform(size=(n, H)) < 0.4, poison)
    lo = rs.normal(0, 1, (n, V)) if gauss else (rs.uniform(size=(n, V)) < 0.3)
    out["x_lo"], out["x_lo0"] = matrix(eng, rs, n, V, ldv, lo, poison)
    for name, size in (("c", V), ("cs", V), ("b", H), ("bs", H)):
        out[name + "0"] = rs.normal(0, 0.3 if len(name) == 1 else 0.01, size).astype(np.float32)
        out[name] = dev(eng, out[name + "0"])
    return out


def scaled(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


def hp_of(rule):
    n, gauss, mom, wc, l1, bs = rule
    return dict(lr=0.05, momentum=mom, weightcost=wc, lambda_1=l1, lambda_2=0.01, batch_size=bs)


def gen_once(eng, V, H, ldh, rule, path, seed=5):
    n, gauss = rule[0], rule[1]
    hp = hp_of(rule)
    L = layer(eng, V, H, ldh, n, gauss, seed, poison=(path == "fused"))
    cost = eng.updown_gen_step(L["x_lo"], L["x_hi"], L["G"], L["Gs"], L["c"], L["cs"], gauss, hp["lr"], hp["lambda_1"],
                               hp["lambda_2"], hp["weightcost"], hp["momentum"], hp["batch_size"], n, cost_scale=1.0 / n, path=path)
    return L, float(cost), hp


def gen_check(eng, V, H, ldh, rule, path):
    n, gauss = rule[0], rule[1]
    L, cost, hp = gen_once(eng, V, H, ldh, rule, path)
    tw = ud.untie(dict(W=L["G0"][:, :H], G=L["G0"][:, :H], Gs=L["Gs0"][:, :H], b=L["b0"], c=L["c0"], cs=L["cs0"], gauss=gauss))
    want = ud.gen_step(tw, L["x_lo0"][:, :V], L["x_hi0"][:, :H], hp, n) / n
    tag = "updown gen %s %dx%d n=%d" % (path, V, H, n)
    figs = [("G", scaled(L["G"].cpu().numpy(), tw["G"])), ("G_speed", scaled(L["Gs"].cpu().numpy(), tw["Gs"])),
            ("vbias", scaled(L["c"].cpu().numpy(), tw["c"])), ("vbias_speed", scaled(L["cs"].cpu().numpy(), tw["cs"]))]
    print("%s: %s, cost rel %.3e" % (tag, ", ".join("%s %.3e" % f for f in figs), abs(cost - want) / abs(want)))
    for name, err in figs:
        check("%s: %s / max(1, max|ref|)" % (tag, name), err, 2e-6, "update")
    check(tag + ": cost rel", abs(cost - want) / abs(want), 1e-5)
    if path == "fused":                               # pad columns: neither read nor written
        for name in ("G", "Gs"):
            full = L[name]._base.cpu().numpy()
            assert np.array_equal(full[:, H:].view(np.int32), L[name + "0"][:, H:].view(np.int32)), "a pad column of %s was written" % name
            assert np.isfinite(full[:, :H]).all(), "a pad column reached %s" % name
        assert np.isfinite(cost) and np.isfinite(L["c"].cpu().numpy()).all() and np.isfinite(L["cs"].cpu().numpy()).all()
    assert np.array_equal(L["x_lo"].cpu().numpy(), L["x_lo0"][:, :V]) and np.array_equal(L["x_hi"].cpu().numpy(), L["x_hi0"][:, :H])
    assert np.array_equal(L["b"].cpu().numpy(), L["b0"]) and np.array_equal(L["bs"].cpu().numpy(), L["bs0"])     # the hidden half
    again, cost2, _ = gen_once(eng, V, H, ldh, rule, path)
    for name in ("G", "Gs", "c", "cs"):
        assert np.array_equal(bits(again[name]), bits(L[name])), "two runs differ in %s" % name
    assert cost2 == cost


# ------------------------------------------------------------------------------------------------------------------ (a) kernels
@pytest.mark.parametrize("path", ["fused", "composed"])
@pytest.mark.parametrize("rule", RULES, ids=["n1", "n20_gauss_ragged", "n32_all_terms"])
@pytest.mark.parametrize("V,H,ldh", SHAPES)
def test_generative_rule_against_the_twin(hip_engine, V, H, ldh, rule, path):
    gen_check(hip_engine, V, H, ldh, rule, path)


@pytest.mark.parametrize("n", [5, 9, 13, 21, 25, 29])
def test_generative_rule_at_every_padded_batch_width(hip_engine, n):
    """The one-pass kernel is instantiated per minibatch rows rounded up to 4: the widths the rules above do not reach, on the
    widest row (two 16-byte groups per lane) with a ragged H."""
    gen_check(hip_engine, 300, 510, 512, (n, n % 2 == 1 and n > 20, 0.5, 2e-4, 0.0, 20), "fused")


@pytest.mark.parametrize("path", ["fused", "composed"])
def test_generative_rule_on_the_gene_layer(hip_engine, path):
    gen_check(hip_engine, 19937, 400, 400, RULES[1], path)


def rec_once(eng, V, H, ldh, rule, path, seed=6):
    n = rule[0]
    hp = hp_of(rule)
    L = layer(eng, V, H, ldh, n, False, seed, poison=False)
    r = eng.propup(L["x_lo"], L["G"], L["b"], want_pre=False, want_sample=False)[1]
    eng.updown_rec_step(L["x_lo"], L["x_hi"], r, L["G"], L["Gs"], L["b"], L["bs"], hp["lr"], hp["lambda_1"], hp["lambda_2"],
                        hp["weightcost"], hp["momentum"], hp["batch_size"], n, path=path)
    return L, r, hp


REC_CASES = [(s, r) for s in SHAPES for r in RULES] + [((19937, 400, 400), RULES[1])]     # (the gene layer: the preset's batch)


@pytest.mark.parametrize("path", ["fused", "composed"])
@pytest.mark.parametrize("shape,rule", REC_CASES, ids=["%dx%d_n%d" % (s[0], s[1], r[0]) for s, r in REC_CASES])
def test_recognition_rule_against_the_twin(hip_engine, shape, rule, path):
    (V, H, ldh), eng, n = shape, hip_engine, rule[0]
    L, r, hp = rec_once(eng, V, H, ldh, rule, path)
    tw = ud.untie(dict(W=L["G0"][:, :H], Ws=L["Gs0"][:, :H], b=L["b0"], bs=L["bs0"], c=L["c0"], gauss=False))
    own = ud.rec_step(tw, L["x_lo0"][:, :V], L["x_hi0"][:, :H], hp, n, r=r.cpu().numpy())
    tag = "updown rec %s %dx%d n=%d" % (path, V, H, n)
    check(tag + ": r (propup)", np.abs(r.cpu().numpy() - own).max(), 2e-6, "prob")
    figs = [("W", scaled(L["G"].cpu().numpy(), tw["W"])), ("W_speed", scaled(L["Gs"].cpu().numpy(), tw["Ws"])),
            ("hbias", scaled(L["b"].cpu().numpy(), tw["b"])), ("hbias_speed", scaled(L["bs"].cpu().numpy(), tw["bs"]))]
    print("%s: %s" % (tag, ", ".join("%s %.3e" % f for f in figs)))
    for name, err in figs:
        check("%s: %s / max(1, max|ref|)" % (tag, name), err, 2e-6, "update")
    assert np.array_equal(L["c"].cpu().numpy(), L["c0"]) and np.array_equal(L["cs"].cpu().numpy(), L["cs0"])     # the visible half
    again, _, _ = rec_once(eng, V, H, ldh, rule, path)
    for name in ("G", "Gs", "b", "bs"):
        assert np.array_equal(bits(again[name]), bits(L[name])), "two runs differ in %s" % name


@pytest.mark.parametrize("V,H,ldh,n", [(300, 40, 40, 33), (64, 516, 516, 20)])
def test_shapes_outside_the_one_pass_regime_take_the_composed_path(hip_engine, V, H, ldh, n):
    from mdbn_amd import MdbnError
    eng = hip_engine
    rule = (n, False, 0.5, 2e-4, 0.0, 20)
    auto, cost_a, _ = gen_once(eng, V, H, ldh, rule, "auto")
    comp, cost_c, _ = gen_once(eng, V, H, ldh, rule, "composed")
    for name in ("G", "Gs", "c", "cs"):
        assert np.array_equal(bits(auto[name]), bits(comp[name])), name
    assert cost_a == cost_c
    with pytest.raises(MdbnError):
        gen_once(eng, V, H, ldh, rule, "fused")
    ra, _, _ = rec_once(eng, V, H, ldh, rule, "auto")
    rc, _, _ = rec_once(eng, V, H, ldh, rule, "composed")
    for name in ("G", "Gs", "b", "bs"):
        assert np.array_equal(bits(ra[name]), bits(rc[name])), name
    with pytest.raises(MdbnError):
        rec_once(eng, V, H, ldh, rule, "fused")


def test_every_einval_case_returns_without_touching_its_outputs(hip_engine):
    import torch
    from mdbn_amd import _lib
    eng, lib = hip_engine, hip_engine.lib
    V, H, ldh, n = 100, 24, 24, 20
    ldv = V
    L = layer(eng, V, H, ldh, n, False, 2, poison=False)
    r = eng.propup(L["x_lo"], L["G"], L["b"], want_pre=False, want_sample=False)[1]
    cost = torch.zeros(4, dtype=torch.float32, device=eng.device)
    need = C.c_int64()
    _lib.check(lib.mdbn_updown_gen_workspace_bytes(eng.ctx, n, V, H, ldv, ldh, 2, C.byref(need)), "gen sizer")
    ws = torch.zeros(need.value // 4 + 8, dtype=torch.float32, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def upd(kind, **kw):
        u = _lib.UpdateArgs()
        u.W, u.W_speed = L["G"].data_ptr(), L["Gs"].data_ptr()
        if kind == "gen":
            u.vbias, u.vbias_speed = L["c"].data_ptr(), L["cs"].data_ptr()
        else:
            u.hbias, u.hbias_speed = L["b"].data_ptr(), L["bs"].data_ptr()
        u.V, u.H, u.ldv, u.ldh = V, H, ldv, ldh
        u.lr, u.momentum, u.batch_size, u.n_rows, u.cost_scale = 0.05, 0.5, 20.0, float(n), 1.0
        for k, v in kw.items():
            setattr(u, k, v)
        return u

    def gen(u=None, x_lo=L["x_lo"], x_hi=L["x_hi"], n=n, gauss=0, path=0, ws=ws, ws_bytes=None, ctx=eng.ctx, cost=cost):
        u = upd("gen") if u is None else u
        return lib.mdbn_updown_gen_step(ctx, eng._stream(), p(x_lo), p(x_hi), n, gauss, C.byref(u) if u is not False else None,
                                        p(cost), path, p(ws), need.value if ws_bytes is None else ws_bytes)

    def rec(u=None, y_lo=L["x_lo"], y_hi=L["x_hi"], r=r, n=n, path=0, ws=ws, ws_bytes=None, ctx=eng.ctx):
        u = upd("rec") if u is None else u
        return lib.mdbn_updown_rec_step(ctx, eng._stream(), p(y_lo), p(y_hi), p(r), n, C.byref(u) if u is not False else None,
                                        path, p(ws), need.value if ws_bytes is None else ws_bytes)

    watched = [L[k]._base if L[k]._base is not None else L[k] for k in ("G", "Gs", "c", "cs", "b", "bs")] + [cost, ws]
    before = [bits(t) for t in watched]
    misaligned = L["x_lo"]._base.reshape(-1)[1:1 + n * ldv]
    bad_gen = [dict(n=0), dict(n=-1), dict(x_lo=None), dict(x_hi=None), dict(ws=None), dict(ctx=None), dict(u=False),
               dict(x_lo=misaligned), dict(ws=ws[1:]), dict(gauss=2), dict(path=3), dict(path=-1), dict(ws_bytes=need.value - 4, path=2),
               dict(ws_bytes=0), dict(cost=cost.view(torch.uint8)[1:]),
               dict(u=upd("gen", V=0)), dict(u=upd("gen", H=0)), dict(u=upd("gen", ldh=H - 4)), dict(u=upd("gen", ldh=H + 2)),
               dict(u=upd("gen", ldv=V + 2)), dict(u=upd("gen", W=None)), dict(u=upd("gen", W_speed=None)),
               dict(u=upd("gen", vbias=None)), dict(u=upd("gen", vbias_speed=None)), dict(u=upd("gen", hbias=L["b"].data_ptr())),
               dict(u=upd("gen", batch_size=0.0)), dict(u=upd("gen", n_rows=-1.0)), dict(u=upd("gen", phase=1)),
               dict(u=upd("gen", struct_size=8)), dict(u=upd("gen", W=L["G"].data_ptr() + 4)),
               dict(n=33, path=1), dict(u=upd("gen", H=516, ldh=516), path=1)]
    for kw in bad_gen:
        assert gen(**kw) == -1, kw
        assert _lib.last_error(), kw
    bad_rec = [dict(n=0), dict(y_lo=None), dict(y_hi=None), dict(r=None), dict(ws=None), dict(ctx=None), dict(u=False),
               dict(y_lo=misaligned), dict(path=3), dict(ws_bytes=0), dict(u=upd("rec", hbias=None)),
               dict(u=upd("rec", vbias=L["c"].data_ptr())), dict(u=upd("rec", phase=2)), dict(u=upd("rec", ldh=H + 2)),
               dict(u=upd("rec", batch_size=-1.0)), dict(n=33, path=1)]
    for kw in bad_rec:
        assert rec(**kw) == -1, kw
        assert _lib.last_error(), kw
    bytes_out = C.c_int64(-7)
    assert lib.mdbn_updown_gen_workspace_bytes(eng.ctx, 33, V, H, ldv, ldh, 1, C.byref(bytes_out)) == -1 and bytes_out.value == -7
    assert lib.mdbn_updown_rec_workspace_bytes(eng.ctx, n, V, 516, ldv, 516, 1, C.byref(bytes_out)) == -1 and bytes_out.value == -7
    assert lib.mdbn_updown_gen_workspace_bytes(eng.ctx, n, V, H, ldv, ldh, 0, None) == -1
    eng.synchronize()
    assert all(np.array_equal(a, bits(t)) for a, t in zip(before, watched)), "a refused call wrote something"
    assert gen() == 0 and rec() == 0                     # ... and the same arguments without the fault are accepted
    eng.synchronize()


# ------------------------------------------------------------------------------------------------------------------ (b) whole steps
STEPS = 4
HP = dict(lr=0.05, top_lr=0.03, k=1, momentum=0.5, weightcost=2e-4, lambda_1=0.0, lambda_2=0.01, batch_size=20)
NAMES = (("W", "W"), ("hbias", "b"), ("vbias", "c"), ("W_speed", "Ws"), ("hbias_speed", "bs"), ("vbias_speed", "cs"),
         ("W_gen", "G"), ("W_gen_speed", "Gs"))


def make_dbn(eng, sizes, gauss, seed):
    import mdbn_amd
    mdbn_amd.DBN.verbose = False
    rs = np.random.RandomState(seed)
    Ws = [(rs.normal(0, 1, (a, b)) / np.sqrt(a)).astype(np.float32) for a, b in zip(sizes[:-1], sizes[1:])]
    bs = [rs.normal(0, 0.3, b).astype(np.float32) for b in sizes[1:]]
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(seed), theano_rng=mdbn_amd.RandomStreams(50 + seed), n_ins=sizes[0],
                       gauss=gauss, hidden_layers_sizes=list(sizes[1:-1]), n_outs=sizes[-1], W_list=Ws, b_list=bs, engine=eng)
    for r in net.rbm_layers:
        r.vbias.set_value(rs.normal(0, 0.3, r.n_visible).astype(np.float32))
    return net


def twin_net(net):
    out = []
    for r in net.rbm_layers:
        out.append(ud.untie(dict(W=r.W.get_value(), b=r.hbias.get_value(), c=r.vbias.get_value(), gauss=r.gauss, noisy=False,
                                 seed=r.theano_rng.seed, stream=r.stream_id, step=r._rng_step)))
    return out


def check_dream_noise(net, layer0, y, n):
    """A noisy Gaussian bottom (error_free=False): y_0 minus the twin's noise-free mean (pre-step parameters) is the N(0, 1)
    matrix of the layer's stream at its dream step (the wake pass took the step before it).  Bound 1e-4: float32 Box-Muller
    on values up to 5.5 rounds at some 1e-6 (log, the cosine of an argument up to 2 pi, the subtraction of the mean), a wrong
    stream or step is off by O(1)."""
    from oracle import philox_np
    mean = ud.predict(y[1].cpu().numpy(), layer0["G"], layer0["c"], True)[1]
    noise = y[0].cpu().numpy().astype(np.float64) - mean
    ref = philox_np.normal(n, mean.shape[1], layer0["seed"], layer0["stream"], layer0["step"] + 1, 0).astype(np.float64)
    check("updown step: N(0, 1) noise of a Gaussian dream", np.abs(noise - ref).max(), 1e-4)
    if noise.size >= 1000:                          # (std of 6020 draws: 1 +- 0.009)
        assert 0.9 < noise.std() < 1.1


def run_steps(eng, nets, joint, tables, path):
    """STEPS up-down steps on the device, each followed by the twin's teacher-forced along the samples the device drew."""
    from mdbn_amd import updown
    model = dict(bottoms=[twin_net(n) for n in nets], joint=twin_net(joint) if joint is not None else None)
    top = (joint if joint is not None else nets[0]).rbm_layers[-1]
    hp = updown.Hyper(HP["lr"], HP["top_lr"], HP["k"], HP["momentum"], HP["weightcost"], HP["lambda_1"], HP["lambda_2"],
                      HP["batch_size"], path)
    rs = np.random.RandomState(3)
    n_rows = [20, 20, 13, 1]                            # the preset's batch, a ragged one, a single row
    flips = 0
    eng.trace_chain = True
    try:
        for t in range(STEPS):
            idx = rs.permutation(len(tables[0]))[:n_rows[t]]
            rec = updown.step(nets, joint, [eng.to_device(x[idx]) for x in tables], hp)
            sc = eng.last_scratch
            Vt, Ht = top.n_visible, top.n_hidden
            forced = (sc.trace_h.cpu().numpy()[:, :n_rows[t], :Ht], sc.trace_v.cpu().numpy()[:, :n_rows[t], :Vt])
            # the dream starts from the visible sample of the top chain's last step
            assert np.array_equal(rec.y[-1][-1].cpu().numpy(), forced[1][-1])
            nb = len(nets)
            recorded = [s.cpu().numpy() for m in range(nb) for s in rec.x[m][1:]]
            if joint is not None:
                recorded += [s.cpu().numpy() for s in rec.x[nb][1:]]
                recorded += [s.cpu().numpy() for s in reversed(rec.y[nb][:-1])]
                recorded += [s.cpu().numpy() for m in range(nb) for s in reversed(rec.y[m][:-1])]
            else:
                recorded += [s.cpu().numpy() for s in reversed(rec.y[0][:-1])]
            for m, net in enumerate(nets):
                if net.rbm_layers[0].gauss and not net.rbm_layers[0].error_free:
                    check_dream_noise(net, model["bottoms"][m][0], rec.y[m], n_rows[t])
            draws = ud.Draws(recorded, tie=1e-6)
            want = ud.step(model, [x[idx] for x in tables], HP, draws, forced_top=forced)
            assert not draws.recorded, "the twin drew fewer samples than the device"
            flips += draws.flips
            for m in range(len(rec.r)):
                for got, ref in zip(rec.r[m], want["r"][m]):
                    check("updown step (%s): r of the dream" % path, np.abs(got.cpu().numpy() - ref).max(), 2e-6, "prob")
            gen = sum(float(c) for c in rec.gen_cost)
            check("updown step (%s): generative cost rel" % path, abs(gen - want["gen_cost"]) / abs(want["gen_cost"]), 1e-5)
            check("updown step (%s): top cost rel" % path, abs(float(rec.top_cost) - want["top_cost"]) / abs(want["top_cost"]), 1e-5)
    finally:
        eng.trace_chain = False
    assert flips <= 3
    figs = []
    for net, tw in zip(list(nets) + ([joint] if joint is not None else []), model["bottoms"] + ([model["joint"]] if joint is not None else [])):
        for r, l in zip(net.rbm_layers, tw):
            assert r._rng_step == l["step"]
            for attr, key in NAMES:
                if getattr(r, attr) is not None:
                    figs.append(("%s[%dx%d]" % (attr, r.n_visible, r.n_hidden), scaled(getattr(r, attr).get_value(), l[key])))
    print("updown steps (%s): %s" % (path, ", ".join("%s %.3e" % f for f in figs)))
    for name, err in figs:
        check("updown %d steps (%s): %s / max(1, max|ref|)" % (STEPS, path, name.split("[")[0]), err, 2e-6, "update")
    return {(i, j, attr): getattr(r, attr).get_value() for i, net in enumerate(list(nets) + ([joint] if joint is not None else []))
            for j, r in enumerate(net.rbm_layers) for attr, _ in NAMES if getattr(r, attr) is not None}


@pytest.mark.parametrize("gauss", [0, 1, 2], ids=["bernoulli", "gaussian_bottom", "noisy_gaussian_bottom"])
@pytest.mark.parametrize("path", ["fused", "composed"])
def test_four_steps_of_a_three_layer_dbn(hip_engine, path, gauss):
    eng = hip_engine
    rs = np.random.RandomState(4)
    data = rs.normal(0, 1, (64, 301)).astype(np.float32) if gauss else (rs.uniform(size=(64, 301)) < 0.3).astype(np.float32)

    def net():
        dbn = make_dbn(eng, (301, 130, 36, 20), bool(gauss), 11)
        if gauss == 2:
            dbn.rbm_layers[0].error_free = False       # the dream's y_0 carries N(0, 1) noise
        return dbn
    first = run_steps(eng, [net()], None, [data], path)
    again = run_steps(eng, [net()], None, [data], path)
    for key in first:
        assert np.array_equal(first[key], again[key]), "two runs differ in %r" % (key,)


@pytest.mark.parametrize("path", ["fused", "composed"])
def test_four_steps_of_a_two_modality_stack(hip_engine, path):
    eng = hip_engine
    rs = np.random.RandomState(5)
    tables = [rs.normal(0, 1, (48, 140)).astype(np.float32), rs.normal(0, 1, (48, 75)).astype(np.float32)]
    nets = [make_dbn(eng, (140, 24), True, 21), make_dbn(eng, (75, 30, 12), True, 22)]
    joint = make_dbn(eng, (36, 24, 8), False, 23)
    run_steps(eng, nets, joint, tables, path)


# ------------------------------------------------------------------------------------------------------------------ (c) planes
@pytest.mark.parametrize("path", ["fused", "composed"])
def test_no_plane_is_stale_after_a_step(hip_engine, path):
    """A CD step on a plane-eligible shape makes bf16 planes of W; an up-down step then writes W (and W_gen); the next CD
    step at the plane shape and a propdown through W_gen must see the NEW matrices.  No product path makes planes of W_gen
    (only a plane CD step creates some, and none is given W_gen), so the test makes them itself: every path that writes G must
    leave in them the split of the new G."""
    import ctypes as C
    import torch
    from mdbn_amd import RngAddr, _lib, updown
    from oracle import rbm_np
    eng = hip_engine
    V, H, B = 1024, 512, 256            # (whole tiles for the plane path, and ldh = 512: still the one-pass regime at n = 20)
    eng.set_option("gemm_planes", 1)
    assert eng.plane_shape(B, V, H, V, H)
    net = make_dbn(eng, (V, H, 32), False, 31)
    r = net.rbm_layers[0]
    rs = np.random.RandomState(6)
    big = eng.to_device((rs.uniform(size=(B, V)) < 0.3).astype(np.float32))
    eng.cd_step(big, None, r.W.tensor, r.hbias.tensor, r.vbias.tensor, False, 1, RngAddr(1, 9, 0, 0, 0))
    planes, valid = eng.w_planes(r.W.tensor)
    assert planes is not None and valid
    hp = updown.Hyper(0.5, 0.5, 1, 0.0, 0.0, 0.0, 0.0, 20, path)       # a large rate: a stale plane would be far off
    updown.untie(r)
    g_planes, _ = eng.w_planes(r.W_gen.tensor, create=True)
    g_planes.fill_(0x7fc0)                                               # (bf16 NaN everywhere: a piece left unwritten shows)
    W_old = r.W.get_value()
    for _ in range(2):                                                   # (the second step moves W by the first one's speed)
        updown.step([net], None, [big[:20]], hp)
    assert np.abs(r.W.get_value() - W_old).max() > 1e-3
    assert eng.w_planes(r.W.tensor)[1], "the planes of W are marked stale"
    assert eng.w_planes(r.W_gen.tensor)[0] is g_planes and eng.w_planes(r.W_gen.tensor)[1], "the planes of W_gen are marked stale"
    split = torch.empty_like(g_planes)
    _lib.check(eng.lib.mdbn_split_planes(eng.ctx, eng._stream(), C.c_void_p(r.W_gen.tensor.data_ptr()), V, r.W_gen.tensor.stride(0),
                                         C.c_void_p(split.data_ptr())), "mdbn_split_planes")
    assert torch.equal(g_planes, split), "the planes of W_gen are not the split of the new W_gen"
    _, sc = eng.cd_step(big, None, r.W.tensor, r.hbias.tensor, r.vbias.tensor, False, 1, RngAddr(1, 9, 1, 0, 0))
    W, b, c = (a.get_value().astype(np.float64) for a in (r.W, r.hbias, r.vbias))
    v0 = big.cpu().numpy().astype(np.float64)
    check("after an updown step (%s): ph_mean of a plane CD step" % path,
          np.abs(sc.P2.cpu().numpy()[:B] - rbm_np.sigmoid(v0 @ W + b)).max(), 2e-6, "prob")
    hs = sc.hs.cpu().numpy().astype(np.float64)
    check("after an updown step (%s): nv_mean of a plane CD step" % path,
          np.abs(sc.V2.cpu().numpy()[B:] - rbm_np.sigmoid(hs @ W.T + c)).max(), 2e-6, "nv_mean")
    G = r.W_gen.get_value().astype(np.float64)
    assert np.abs(G - W).max() > 1e-3                                    # untied for real
    down = eng.propdown(eng.to_device(hs.astype(np.float32)), r.W_gen.tensor, r.vbias.tensor, rng=RngAddr(1, 9, 2, 0, 0))[1]
    check("after an updown step (%s): propdown through W_gen" % path,
          np.abs(down.cpu().numpy() - rbm_np.sigmoid(hs @ G.T + c)).max(), 2e-6, "prob")
