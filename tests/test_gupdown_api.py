"""Up-down fine-tuning of stacks with categorical visible units through the public classes on the CPU checker engine
(tests/_gupdown_np.py): the C-ABI names, the public classes against the float64 twin along the same draws -- a DBN 9 -> 5 -> 4 -> 3
with K = 3 and a forest (grouped 9 -> 3, Gaussian 4 -> 2, joint 5 -> 4 -> 3) --, the call order, which parameters move, the RNG
accounting, one-hot dreams, what is refused, where the generative weights are used afterwards, and on an enumerable stack that
the twin's exact log p(data) rises.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import _dbn_bound_np as T
import _gbound_np as gb
import _gupdown_np as gud
import _softmax_np as sm
import _updown_np as ud
import mdbn_amd
from mdbn_amd import _lib, updown

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mdbn_updown_gen_grouped_workspace_bytes", "mdbn_updown_gen_step_grouped")
HP = dict(lr=0.05, top_lr=0.03, k=2, momentum=0.5, weightcost=0.001, lambda_1=0.002, lambda_2=0.01, batch_size=10)
KW = {k: v for k, v in HP.items() if k != "batch_size"}
K3 = [0, 3, 6, 9]


def build(layers, eng, shuffle_seed=77):
    """The DBN of a twin net on ``eng`` (its RBMs take the streams 0, 1, ... of the net's seed, as the twin's layers)."""
    mdbn_amd.DBN.verbose = False
    sizes = [layers[0]["W"].shape[0]] + [l["W"].shape[1] for l in layers]
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(0), theano_rng=mdbn_amd.RandomStreams(layers[0]["seed"]), n_ins=sizes[0],
                       gauss=layers[0]["gauss"], hidden_layers_sizes=sizes[1:-1], n_outs=sizes[-1],
                       W_list=[l["W"] for l in layers], b_list=[l["b"] for l in layers], engine=eng,
                       visible_groups=layers[0].get("bounds"))
    for r, l in zip(net.rbm_layers, layers):
        r.vbias.set_value(l["c"])
    net.shuffle_rng = np.random.RandomState(shuffle_seed)
    return net


def k3_stack(eng, scale=0.5, seed=32):
    rs = np.random.RandomState(seed)
    return build(gb.make_net(rs, (9, 5, 4, 3), scale, 3000 + seed, K3), eng)


def forest(eng, scale=0.5):
    rs = np.random.RandomState(33)
    a = build(gb.make_net(rs, (9, 3), scale, 4001, K3), eng)
    b = build(gb.make_net(rs, (4, 2), scale, 4002, gauss=True), eng)
    joint = build(gb.make_net(rs, (5, 4, 3), scale, 4003), eng, shuffle_seed=31)
    return a, b, joint


def steps(nets):
    return [r._rng_step for net in nets for r in net.rbm_layers]


def assert_net_equal(dbn, net, tol=1e-12):
    for r, l in zip(dbn.rbm_layers, net):
        pairs = [(r.W, l["W"]), (r.hbias, l["b"]), (r.vbias, l["c"]), (r.W_speed, l["Ws"]), (r.hbias_speed, l["bs"]),
                 (r.vbias_speed, l["cs"])]
        if r.W_gen is not None:
            pairs += [(r.W_gen, l["G"]), (r.W_gen_speed, l["Gs"])]
        for mine, ref in pairs:
            assert np.abs(mine.tensor.numpy() - ref).max() < tol
        assert r._rng_step == l["step"]


def twin_run(model, tables, epochs, hp, shuffle_seed, batch_size, draws=None):
    rng = np.random.RandomState(shuffle_seed)
    out = []
    for _ in range(epochs):
        batches = mdbn_amd.get_minibatches_idx(len(tables[0]), batch_size, shuffle=True, rng=rng)[1]
        recs = [gud.step(model, [t[b] for t in tables], hp, draws) for b in batches]
        out.append((np.mean([r["gen_cost"] for r in recs]), np.mean([r["top_cost"] for r in recs])))
    return out


def test_the_names_are_in_the_header_the_signatures_and_the_engine():
    header = open(os.path.join(ROOT, "include", "mdbn_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES
    # the arguments of the plain call without gauss, then the table
    plain, grouped = _lib.SIGNATURES["mdbn_updown_gen_step"], _lib.SIGNATURES["mdbn_updown_gen_step_grouped"]
    assert grouped[:-3] == plain[:5] + plain[6:] and len(grouped) == len(plain) + 2
    assert _lib.SIGNATURES["mdbn_updown_gen_grouped_workspace_bytes"] == _lib.SIGNATURES["mdbn_updown_gen_workspace_bytes"]
    assert callable(getattr(mdbn_amd.HipEngine, "updown_gen_step_grouped"))
    assert not hasattr(gud.NoGroupedRule(), "updown_gen_step_grouped") and hasattr(gud.GupdownOracle(), "updown_gen_step_grouped")


# ------------------------------------------------------------------ the public classes against the twin
@pytest.mark.parametrize("n_rows", [23, 21])
def test_a_dbn_with_groups_follows_the_twin_over_ragged_and_one_row_minibatches(n_rows):
    """FAILS on the parent commit, which refuses a layer with groups."""
    eng = gud.GupdownOracle()
    dbn = k3_stack(eng)
    data = sm.one_hot_data(np.random.RandomState(9), n_rows, 9, K3)        # 23 rows: 10, 10, 3; 21 rows: 10, 10, 1
    model = dict(bottoms=[gud.twin_net(dbn)], joint=None)
    r0, r1, top = dbn.rbm_layers
    before = {k: [getattr(r, k).tensor.clone() for r in dbn.rbm_layers] for k in ("W", "hbias", "vbias")}
    s0 = steps([dbn])
    dbn._lower_cache[1] = "stale"
    # one step first: the call order, what moves, the RNG accounting
    rec = updown.step([dbn], None, [eng.as_matrix(torch.from_numpy(data[:10].astype(np.float64)))],
                      updown.Hyper(HP["lr"], HP["top_lr"], HP["k"], HP["momentum"], HP["weightcost"], HP["lambda_1"], HP["lambda_2"],
                                   10, "composed"))
    W0, W1, Wt = id(r0.W.tensor), id(r1.W.tensor), id(top.W.tensor)
    G0, G1 = id(r0.W_gen.tensor), id(r1.W_gen.tensor)
    assert eng.log == [
        ("propup", W0, s0[0]), ("propup", W1, s0[1]),                          # wake: a propup from the one-hot rows
        ("cd_step", Wt, s0[2], True),
        ("propdown", G1, s0[1] + 1), ("propup", W1, None),                     # sleep
        ("propdown", G0, None), ("group_softmax", s0[0] + 1), ("propup", W0, None),    # ... linear through W_gen, one draw per group
        ("apply_update", Wt),
        ("gen_grouped", G0), ("rec", W0), ("gen", G1), ("rec", W1)]
    assert eng.paths == ["composed", "composed"]
    assert steps([dbn]) == [s0[0] + 2, s0[1] + 2, s0[2] + 1]                   # one RNG step per sampled conditional
    y0 = rec.y[0][0].numpy()
    assert np.isin(y0, (0.0, 1.0)).all() and all((y0[:, lo:hi].sum(axis=1) == 1).all() for lo, hi in sm.spans(K3))
    for i, r in enumerate((r0, r1)):
        # (the rule moves a parameter by its OLD speed: after one step from zero speeds the biases stand, their speeds do not)
        assert torch.equal(r.hbias.tensor, before["hbias"][i]) and torch.equal(r.vbias.tensor, before["vbias"][i])
        assert r.hbias_speed.tensor.abs().max() > 0 and r.vbias_speed.tensor.abs().max() > 0
        assert not torch.equal(r.W.tensor, before["W"][i]) and not torch.equal(r.W_gen.tensor, before["W"][i])
    draws = gud.Draws()
    tw = gud.step(model, [data[:10].astype(np.float64)], HP, draws)
    assert np.array_equal(tw["y"][0][0], y0) and len(draws.dreams) == 1
    assert abs(float(rec.gen_cost[0]) - tw["gen_cost"]) < 1e-12 * abs(tw["gen_cost"])
    assert_net_equal(dbn, model["bottoms"][0])
    # a second step: hbias of the generative half and vbias of the recognition half do not move
    hb, vb = [r.hbias.tensor.clone() for r in (r0, r1)], [r.vbias.tensor.clone() for r in (r0, r1)]
    gen, rec_ = eng.updown_gen_step_grouped, eng.updown_rec_step
    seen = []

    def spy_gen(*a, **kw):
        out = gen(*a, **kw)
        seen.append(("gen", torch.equal(r0.hbias.tensor, hb[0]), not torch.equal(r0.vbias.tensor, vb[0])))
        vb[0] = r0.vbias.tensor.clone()
        return out

    def spy_rec(y_lo, *a, **kw):
        first = y_lo.shape[1] == 9
        out = rec_(y_lo, *a, **kw)
        if first:
            seen.append(("rec", not torch.equal(r0.hbias.tensor, hb[0]), torch.equal(r0.vbias.tensor, vb[0])))
        return out
    eng.updown_gen_step_grouped, eng.updown_rec_step = spy_gen, spy_rec
    # ... then whole epochs, ragged and one-row minibatches
    hist = dbn.fine_tune(data, 2, batch_size=10, **KW)
    want = twin_run(model, [data.astype(np.float64)], 2, HP, 77, 10)
    assert seen[:2] == [("gen", True, True), ("rec", True, True)]
    assert_net_equal(dbn, model["bottoms"][0])
    assert np.allclose(np.asarray(hist), np.asarray(want), rtol=1e-12, atol=0)
    assert dbn._lower_cache == {}
    per_epoch = len(mdbn_amd.get_minibatches_idx(n_rows, 10)[1])
    assert steps([dbn]) == [s0[0] + 2 + 4 * per_epoch, s0[1] + 2 + 4 * per_epoch, s0[2] + 1 + 2 * per_epoch]


def test_a_forest_with_a_grouped_modality_follows_the_twin_through_mdbn_fine_tune():
    """FAILS on the parent commit: its MDBN.fine_tune trains the grouped modality as independent sigmoids."""
    eng = gud.GupdownOracle()
    a, b, joint = forest(eng)
    rs = np.random.RandomState(2)
    inputs = [sm.one_hot_data(rs, 13, 9, K3), T.make_data(rs, 13, 4, True)]
    model = dict(bottoms=[gud.twin_net(a), gud.twin_net(b)], joint=gud.twin_net(joint))
    s0 = steps([a, b, joint])
    hist = mdbn_amd.MDBN.fine_tune([a, b], joint, {1: inputs[1], 0: inputs[0]}, 2, batch_size=5, **KW)
    draws = gud.Draws()
    want = twin_run(model, [x.astype(np.float64) for x in inputs], 2, dict(HP, batch_size=5), 31, 5, draws)
    for net, tw in ((a, model["bottoms"][0]), (b, model["bottoms"][1]), (joint, model["joint"])):
        assert_net_equal(net, tw)
    assert np.allclose(np.asarray(hist), np.asarray(want), rtol=1e-12, atol=0)
    # 3 minibatches x 2 epochs: wake + dream per directed layer, one step of the top
    assert steps([a, b, joint]) == [s0[0] + 12, s0[1] + 12, s0[2] + 12, s0[3] + 6]
    kinds = [c[0] for c in eng.log if c[0] in ("gen", "gen_grouped", "rec")]
    assert kinds[:6] == ["gen_grouped", "rec", "gen", "rec", "gen", "rec"]      # a, b, the joint's lower layer
    assert len(draws.dreams) == 6 and all((d[:, lo:hi].sum(axis=1) == 1).all() for d in draws.dreams for lo, hi in sm.spans(K3))
    # every dream row of the public classes holds exactly one 1 per group as well
    rec = updown.step([a, b], joint, [eng.as_matrix(torch.from_numpy(x[:4].astype(np.float64))) for x in inputs],
                      updown.Hyper(0.05, 0.05, 1, 0.0, 0.0, 0.0, 0.0, 4, "auto"))
    y0 = rec.y[0][0].numpy()
    assert np.isin(y0, (0.0, 1.0)).all() and all((y0[:, lo:hi].sum(axis=1) == 1).all() for lo, hi in sm.spans(K3))
    assert torch.equal(rec.y[0][-1], rec.y[2][0][:, :3]) and torch.equal(rec.y[1][-1], rec.y[2][0][:, 3:])


# ------------------------------------------------------------------ what is refused
def test_an_engine_without_the_grouped_rule_refuses_before_anything_moves():
    eng = gud.NoGroupedRule()
    dbn = k3_stack(eng)
    data = sm.one_hot_data(np.random.RandomState(9), 8, 9, K3)
    with pytest.raises(NotImplementedError, match="visible_groups"):
        dbn.fine_tune(data, 1, batch_size=4, lr=0.01)
    assert steps([dbn]) == [0, 0, 0] and eng.log == [] and eng.calls == []
    assert all(r.W_gen is None for r in dbn.rbm_layers)
    # a single RBM with groups: the group refusal comes before the plan's ValueError
    one = build(gb.make_net(np.random.RandomState(1), (9, 3), 0.5, 11, K3), eng)
    with pytest.raises(NotImplementedError, match="visible_groups"):
        one.fine_tune(data, 1, batch_size=4, lr=0.01)
    # MDBN.fine_tune shares the refusal (the parent commit trained the grouped modality as sigmoids here)
    a, b, joint = forest(eng)
    rs = np.random.RandomState(2)
    inputs = [sm.one_hot_data(rs, 6, 9, K3), T.make_data(rs, 6, 4, True)]
    with pytest.raises(NotImplementedError, match="visible_groups"):
        mdbn_amd.MDBN.fine_tune([a, b], joint, inputs, 1, batch_size=3, lr=0.01)
    assert steps([a, b, joint]) == [0] * 4 and eng.log == []
    assert all(r.W_gen is None for net in (a, b, joint) for r in net.rbm_layers)
    # without groups the same engine fine-tunes
    plain = build(gb.make_net(np.random.RandomState(1), (9, 5, 3), 0.5, 12), eng)
    assert len(plain.fine_tune(data, 1, batch_size=4, lr=0.01)) == 1


def test_a_joint_with_groups_and_rows_that_are_not_one_hot_are_refused():
    eng = gud.GupdownOracle()
    rs = np.random.RandomState(33)
    a = build(gb.make_net(rs, (9, 3), 0.5, 4001, K3), eng)
    b = build(gb.make_net(rs, (4, 2), 0.5, 4002, gauss=True), eng)
    joint = build(gb.make_net(rs, (5, 4, 3), 0.5, 4003, [0, 3]), eng)
    inputs = [sm.one_hot_data(rs, 6, 9, K3), T.make_data(rs, 6, 4, True)]
    with pytest.raises(NotImplementedError, match="JOINT"):
        mdbn_amd.MDBN.fine_tune([a, b], joint, inputs, 1, batch_size=3, lr=0.01)
    assert steps([a, b, joint]) == [0] * 4 and eng.log == []
    dbn = k3_stack(eng)
    good = sm.one_hot_data(rs, 8, 9, K3)
    for bad_row in ([1, 1, 0], [0, 0, 0], [0.5, 0.5, 0]):
        bad = good.copy()
        bad[5, 3:6] = bad_row
        with pytest.raises(ValueError, match="exactly one 1"):
            dbn.fine_tune(bad, 1, batch_size=4, lr=0.01)
        with pytest.raises(ValueError, match="exactly one 1"):
            dbn.fine_tune(mdbn_amd.shared(bad, engine=eng), 1, batch_size=4, lr=0.01)
    assert steps([dbn]) == [0, 0, 0] and eng.log == [] and all(r.W_gen is None for r in dbn.rbm_layers)
    # the refusals of the plain stack stand
    with pytest.raises(TypeError):
        dbn.fine_tune(good, 1)
    with pytest.raises(ValueError):
        dbn.fine_tune(good[:, :8], 1, lr=0.1)
    assert len(dbn.fine_tune(good, 1, batch_size=4, lr=0.01)) == 1


# ------------------------------------------------------------------ after fine-tuning
def test_down_pass_and_the_bound_go_through_w_gen_of_the_grouped_layer():
    eng = gud.GupdownOracle()
    dbn = k3_stack(eng)
    rs = np.random.RandomState(5)
    data = sm.one_hot_data(rs, 12, 9, K3)
    dbn.fine_tune(data, 2, batch_size=6, **KW)
    net = gud.twin_net(dbn)
    r0 = dbn.rbm_layers[0]
    assert np.abs(net[0]["G"] - net[0]["W"]).max() > 1e-4
    # down_pass from the first hidden layer: the grouped means of h G_0^T + c_0
    h = (rs.uniform(size=(5, 5)) < 0.5).astype(np.float64)
    want = gud.predict(h, net[0]["G"], net[0]["c"], K3)[1]
    assert np.abs(dbn.down_pass(torch.from_numpy(h), layer=0) - want).max() < 1e-7       # (down_pass returns float32: one ulp)
    assert np.abs(dbn.down_pass(torch.from_numpy(h), layer=0) - gud.predict(h, net[0]["W"], net[0]["c"], K3)[1]).max() > 1e-5
    # the bound's directed term of the input layer reads W_gen; rows equal the twin's on the same samples
    seen = []
    rowll = eng.propdown_row_loglik_grouped
    eng.propdown_row_loglik_grouped = lambda h_, W, *a, **kw: (seen.append(id(W)), rowll(h_, W, *a, **kw))[1]
    steps0 = steps([dbn])
    got = dbn.log_likelihood_bound(data, n_samples=8, log_z=0.0)
    assert seen == [id(r0.W_gen.tensor)]
    layers = []
    for l, s in zip(net, steps0):
        layers.append(dict(W=l["W"], b=l["b"], c=l["c"], gauss=False, seed=l["seed"], stream=l["stream"], step=s))
    layers[0]["bounds"] = K3
    gen = [dict(l, W=t["G"]) for l, t in zip(layers, net)]
    model = dict(bottoms=[layers], joint=None)
    want = bound_with_generative_weights(model, gen, data, 8)
    assert np.abs(got.rows - want).max() < 1e-12


def bound_with_generative_weights(model, gen, data, S):
    """_gbound_np.estimate's rows with the directed terms read through G: the samples and entropies come from the recognition
    weights (the twin's own run), the directed terms are recomputed on those samples."""
    est = gb.estimate(model, [data], S, 0.0)
    layers = model["bottoms"][0]
    samples = est["samples"][0]
    x = [np.repeat(np.asarray(data, dtype=np.float64), S, axis=0)] + [np.asarray(s, dtype=np.float64) for s in samples]
    values = np.asarray(est["values"], dtype=np.float64).reshape(len(data), S).copy()
    for k in range(len(layers) - 1):
        old, new = gb.row_loglik(x[k + 1], layers[k], x[k]), gb.row_loglik(x[k + 1], gen[k], x[k])
        values += (new - old).reshape(len(data), S)
    return values.mean(axis=1)


# ------------------------------------------------------------------ the gain on an enumerable stack
def planted(n=60, seed=0):
    """Rows of four prototypes over 2 groups of 3, the category of a group replaced by a random one with probability 0.1."""
    rs = np.random.RandomState(seed)
    protos = np.array([[0, 0], [1, 1], [2, 2], [0, 2]])
    cats = protos[rs.randint(0, 4, n)]
    noise = rs.uniform(size=cats.shape) < 0.1
    cats = np.where(noise, rs.randint(0, 3, cats.shape), cats)
    x = np.zeros((n, 6), dtype=np.float32)
    x[np.arange(n), cats[:, 0]] = 1.0
    x[np.arange(n), 3 + cats[:, 1]] = 1.0
    return x


GAIN = dict(lr=0.1, top_lr=0.1, k=1, momentum=0.5, weightcost=0.0, lambda_1=0.0, lambda_2=0.0, batch_size=10)


def test_exact_log_p_of_a_planted_one_hot_stack_rises_and_the_public_classes_follow():
    eng = gud.GupdownOracle()
    dbn = build(gb.make_net(np.random.RandomState(8), (6, 4, 3), 0.3, 5008, [0, 3, 6]), eng)
    data = planted()
    model = dict(bottoms=[gud.twin_net(dbn)], joint=None)
    start = gud.exact_log_p(model["bottoms"][0], data).mean()
    rng = np.random.RandomState(77)
    for _ in range(30):
        for b in mdbn_amd.get_minibatches_idx(len(data), 10, shuffle=True, rng=rng)[1]:
            gud.step(model, [data[b].astype(np.float64)], GAIN)
    end = gud.exact_log_p(model["bottoms"][0], data).mean()
    print("exact log p(data) per row: %.6f before, %.6f after 30 epochs (uniform over the 9 states: %.6f)" % (start, end, -np.log(9.0)))
    assert end > start
    dbn.fine_tune(data, 30, batch_size=10, **{k: v for k, v in GAIN.items() if k != "batch_size"})
    assert_net_equal(dbn, model["bottoms"][0])
