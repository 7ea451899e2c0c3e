"""Up-down fine-tuning through the public classes on the CPU checker engine: the C-ABI names, the call order of a step, which
parameters move, the RNG accounting, ragged and one-row minibatches, what is refused, where the generative weights are used
afterwards, the checkpoint round trip, the multimodal stack's blocks, and -- on an enumerable 6 -> 4 -> 3 stack -- that the
twin's exact log p(data) rises over a run which the public classes reproduce to 1e-12 along the same samples.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import _updown_np as ud
import mdbn_amd
from mdbn_amd import _lib, checkpoint, updown
from _oracle_engine import OracleEngine
from oracle import rbm_np
from oracle.philox_np import PhiloxDraws

NAMES = ("mdbn_updown_gen_workspace_bytes", "mdbn_updown_gen_step", "mdbn_updown_rec_workspace_bytes", "mdbn_updown_rec_step")
HP = dict(lr=0.05, top_lr=0.03, k=2, momentum=0.5, weightcost=0.001, lambda_1=0.002, lambda_2=0.01, batch_size=10)


class UpdownOracle(OracleEngine):
    """The checker engine with the two delta-rule calls, COMPOSED as the library composes them: stacked operands, the oracle's
    CD statistics, the unchanged update rule with a throw-away vector for the bias half that must not move.  Logs the
    step-level calls."""

    def __init__(self):
        OracleEngine.__init__(self)
        self.log, self.paths = [], []

    def propup(self, v, W, hbias, rng=None, **kw):
        self.log.append(("propup", id(W), rng.step if rng is not None else None))
        return OracleEngine.propup(self, v, W, hbias, rng=rng, **kw)

    def propdown(self, h, W, vbias, **kw):
        self.log.append(("propdown", id(W), kw["rng"].step if kw.get("rng") is not None else None))
        return OracleEngine.propdown(self, h, W, vbias, **kw)

    def cd_step(self, data, indexes, W, hbias, vbias, gauss, k, rng, **kw):
        self.log.append(("cd_step", id(W), rng.step, kw.pop("keep_f32", None)))
        stats, sc = OracleEngine.cd_step(self, data, indexes, W, hbias, vbias, gauss, k, rng, **kw)
        # the visible sample of the last Gibbs step: what the device leaves in the scratch of a keep_f32 step
        v0 = self.as_matrix(data).numpy()
        out = rbm_np.cd_chain(self._state(W, hbias, vbias, gauss), v0, PhiloxDraws(rng.seed, rng.stream_id, rng.step, rng.row_offset), k)[2]
        sc.vs = self._t(out[2])
        return stats, sc

    def apply_update(self, W, *a, **kw):
        self.log.append(("apply_update", id(W)))
        return OracleEngine.apply_update(self, W, *a, **kw)

    def _rule(self, W, W_speed, hb, hbs, vb, vbs, S, s_h, s_v, rule):
        lr, l1, l2, wc, mu, batch_size, n_rows = rule
        V, H = W.shape
        stats = self._t(np.concatenate([S.ravel(), s_h, s_v, np.zeros(4)]))
        OracleEngine.apply_update(self, W, W_speed, None, hb, hbs, vb, vbs, stats, lr, l1, l2, wc, mu, batch_size, n_rows, 1.0)

    def updown_gen_step(self, x_lo, x_hi, G, G_speed, vbias, vbias_speed, gauss, lr, lambda_1, lambda_2, weightcost, momentum,
                        batch_size, n_rows, cost_scale=1.0, path="auto"):
        self.log.append(("gen", id(G)))
        self.paths.append(path)
        x_lo, x_hi = self.as_matrix(x_lo).numpy(), self.as_matrix(x_hi).numpy()
        pre, g = ud.predict(x_hi, G.numpy(), vbias.numpy(), gauss)
        S, s_h, s_v = rbm_np.cd_statistics(*ud.stacked_gen(x_lo, x_hi, g))
        junk = torch.zeros(G.shape[1], dtype=self.t_dtype)
        self._rule(G, G_speed, junk, junk.clone(), vbias, vbias_speed, S, s_h, s_v,
                   (lr, lambda_1, lambda_2, weightcost, momentum, batch_size, n_rows))
        cost = 0.5 * ((x_lo - g) ** 2).sum() if gauss else (x_lo * ud.softplus(-pre) + (1 - x_lo) * ud.softplus(pre)).sum()
        return torch.tensor(cost * cost_scale, dtype=self.t_dtype)

    def updown_rec_step(self, y_lo, y_hi, r, W, W_speed, hbias, hbias_speed, lr, lambda_1, lambda_2, weightcost, momentum,
                        batch_size, n_rows, path="auto"):
        self.log.append(("rec", id(W)))
        y_lo, y_hi, r = (self.as_matrix(t).numpy() for t in (y_lo, y_hi, r))
        S, s_h, s_v = rbm_np.cd_statistics(*ud.stacked_rec(y_lo, y_hi, r))
        junk = torch.zeros(W.shape[0], dtype=self.t_dtype)
        self._rule(W, W_speed, hbias, hbias_speed, junk, junk.clone(), S, s_h, s_v,
                   (lr, lambda_1, lambda_2, weightcost, momentum, batch_size, n_rows))


def make_dbn(eng, sizes=(9, 6, 5, 4), gauss=False, seed=3, scale=0.5):
    mdbn_amd.DBN.verbose = False
    rs = np.random.RandomState(seed)
    Ws = [(scale * rs.normal(0, 1, (a, b)) / np.sqrt(a)).astype(np.float32) for a, b in zip(sizes[:-1], sizes[1:])]
    bs = [rs.normal(0, 0.3, b).astype(np.float32) for b in sizes[1:]]
    dbn = mdbn_amd.DBN(numpy_rng=np.random.RandomState(seed), theano_rng=mdbn_amd.RandomStreams(100 + seed), n_ins=sizes[0],
                       gauss=gauss, hidden_layers_sizes=list(sizes[1:-1]), n_outs=sizes[-1], W_list=Ws, b_list=bs, engine=eng)
    for r in dbn.rbm_layers:
        r.vbias.set_value(rs.normal(0, 0.3, r.n_visible).astype(np.float32))
    dbn.shuffle_rng = np.random.RandomState(77)
    return dbn


def make_data(n, V, gauss, seed=9):
    rs = np.random.RandomState(seed)
    return rs.normal(0, 1, (n, V)).astype(np.float32) if gauss else (rs.uniform(size=(n, V)) < 0.4).astype(np.float32)


def twin_net(dbn):
    """The twin's layers from a DBN on the checker engine (float64 tensors read directly: ``get_value`` would narrow them)."""
    net = []
    for r in dbn.rbm_layers:
        t = lambda a: None if a is None else a.tensor.numpy().copy()
        net.append(ud.untie(dict(W=t(r.W), b=t(r.hbias), c=t(r.vbias), G=t(r.W_gen), Ws=t(r.W_speed), bs=t(r.hbias_speed),
                                 cs=t(r.vbias_speed), Gs=t(r.W_gen_speed), gauss=r.gauss, noisy=bool(r.gauss and not r.error_free),
                                 seed=r.theano_rng.seed, stream=r.stream_id, step=r._rng_step)))
    return net


def assert_net_equal(dbn, net, tol=1e-12):
    for r, l in zip(dbn.rbm_layers, net):
        pairs = [(r.W, l["W"]), (r.hbias, l["b"]), (r.vbias, l["c"]), (r.W_speed, l["Ws"]), (r.hbias_speed, l["bs"]),
                 (r.vbias_speed, l["cs"])]
        if r.W_gen is not None:
            pairs += [(r.W_gen, l["G"]), (r.W_gen_speed, l["Gs"])]
        for mine, ref in pairs:
            assert np.abs(mine.tensor.numpy() - ref).max() < tol
        assert r._rng_step == l["step"]


def twin_run(model, tables, epochs, hp, shuffle_seed, batch_size):
    rng = np.random.RandomState(shuffle_seed)
    out = []
    for _ in range(epochs):
        batches = mdbn_amd.get_minibatches_idx(len(tables[0]), batch_size, shuffle=True, rng=rng)[1]
        recs = [ud.step(model, [t[b] for t in tables], hp) for b in batches]
        out.append((np.mean([r["gen_cost"] for r in recs]), np.mean([r["top_cost"] for r in recs])))
    return out


def test_the_names_are_in_the_header_the_signatures_and_the_build():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mdbn_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES
    from mdbn_amd import build
    assert "mdbn_updown.hip" in build.SOURCES and "mdbn_updown.h" in build.HEADERS
    assert re.search(r"#define\s+MDBN_VERSION\s+2\b", header)


@pytest.mark.parametrize("gauss", [False, True])
def test_a_step_makes_these_calls_in_this_order_and_moves_these_parameters(gauss):
    eng = UpdownOracle()
    dbn = make_dbn(eng, gauss=gauss)
    r0, r1, top = dbn.rbm_layers
    data = make_data(10, 9, gauss)
    before = {k: [getattr(r, k).tensor.clone() for r in dbn.rbm_layers] for k in ("W", "hbias", "vbias")}
    steps0 = [r._rng_step for r in dbn.rbm_layers]
    # every W that get_output reads must be the pre-step W until the first recognition update
    seen_w = []
    rec = eng.updown_rec_step

    def spy(*a, **kw):
        if not seen_w:
            seen_w.append([torch.equal(r.W.tensor, w) for r, w in zip(dbn.rbm_layers[:2], before["W"][:2])])
        return rec(*a, **kw)
    eng.updown_rec_step = spy
    dbn.fine_tune(data, 1, batch_size=10, path="composed", **{k: v for k, v in HP.items() if k != "batch_size"})
    W0, W1, Wt = id(r0.W.tensor), id(r1.W.tensor), id(top.W.tensor)
    G0, G1 = id(r0.W_gen.tensor), id(r1.W_gen.tensor)
    assert eng.log == [
        ("propup", W0, steps0[0]), ("propup", W1, steps0[1]),                   # wake
        ("cd_step", Wt, steps0[2], True),                                        # top statistics
        ("propdown", G1, steps0[1] + 1), ("propup", W1, None),                   # sleep, and the recognition means of the dream
        ("propdown", G0, steps0[0] + 1), ("propup", W0, None),
        ("apply_update", Wt),                                                    # updates after every pass
        ("gen", G0), ("rec", W0), ("gen", G1), ("rec", W1)]
    assert eng.paths == ["composed", "composed"]
    assert [r._rng_step for r in dbn.rbm_layers] == [steps0[0] + 2, steps0[1] + 2, steps0[2] + 1]
    assert seen_w == [[True, True]]
    for i, r in enumerate((r0, r1)):
        assert not torch.equal(r.W.tensor, before["W"][i])                       # recognition half moved
        # (the rule moves a parameter by its OLD speed: after one step from zero speeds the biases stand, their speeds do not)
        assert torch.equal(r.hbias.tensor, before["hbias"][i]) and r.hbias_speed.tensor.abs().max() > 0
        assert torch.equal(r.vbias.tensor, before["vbias"][i]) and r.vbias_speed.tensor.abs().max() > 0
        assert r.W_speed.tensor.abs().max() > 0 and r.W_gen_speed.tensor.abs().max() > 0
        assert not torch.equal(r.W_gen_speed.tensor, r.W_speed.tensor)           # two rules, two speeds
        assert not torch.equal(r.W_gen.tensor, before["W"][i])                   # (the shrink terms move the weights at once)
        assert r.W_gen.tensor.stride(0) == r.W.tensor.stride(0)
    assert top.W_gen is None and top.W_gen_speed is None
    assert dbn.sigmoid_layers[0].W is r0.W and dbn.sigmoid_layers[1].b is r1.hbias      # still shared with the MLP


def test_the_halves_leave_the_other_bias_alone():
    eng = UpdownOracle()
    rs = np.random.RandomState(1)
    V, H, n = 7, 5, 6
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    G, Gs, c, cs = t(rs.normal(0, 1, (V, H))), t(rs.normal(0, 1, (V, H))), t(rs.normal(0, 1, V)), t(rs.normal(0, 1, V))
    x_lo, x_hi = t(make_data(n, V, False)), t(make_data(n, H, False, 4))
    l = ud.untie(dict(W=G.numpy(), G=G.numpy(), Gs=Gs.numpy(), b=np.zeros(H), c=c.numpy(), cs=cs.numpy(), gauss=False))
    hp = dict(HP, batch_size=8)
    rule = (hp["lr"], hp["lambda_1"], hp["lambda_2"], hp["weightcost"], hp["momentum"], 8, n)
    cost = eng.updown_gen_step(x_lo, x_hi, G, Gs, c, cs, False, *rule, cost_scale=0.5)
    ref = ud.gen_step(l, x_lo.numpy(), x_hi.numpy(), hp, n)
    assert abs(float(cost) - 0.5 * ref) < 1e-12 * abs(ref)
    for mine, want in ((G, l["G"]), (Gs, l["Gs"]), (c, l["c"]), (cs, l["cs"])):
        assert np.abs(mine.numpy() - want).max() < 1e-12
    W, Ws, b, bs = t(rs.normal(0, 1, (V, H))), t(rs.normal(0, 1, (V, H))), t(rs.normal(0, 1, H)), t(rs.normal(0, 1, H))
    l = ud.untie(dict(W=W.numpy(), Ws=Ws.numpy(), b=b.numpy(), bs=bs.numpy(), c=np.zeros(V), gauss=False))
    r = t(ud.delta_rec(x_lo.numpy(), x_hi.numpy(), W.numpy(), b.numpy())[2])
    eng.updown_rec_step(x_lo, x_hi, r, W, Ws, b, bs, *rule)
    ud.rec_step(l, x_lo.numpy(), x_hi.numpy(), hp, n)
    for mine, want in ((W, l["W"]), (Ws, l["Ws"]), (b, l["b"]), (bs, l["bs"])):
        assert np.abs(mine.numpy() - want).max() < 1e-12


@pytest.mark.parametrize("gauss,n_rows", [(False, 23), (True, 21), (False, 10)])
def test_epochs_with_a_ragged_and_a_one_row_minibatch_equal_the_twin(gauss, n_rows):
    eng = UpdownOracle()
    dbn = make_dbn(eng, gauss=gauss)
    if gauss and n_rows == 21:
        dbn.rbm_layers[0].error_free = False         # a noisy Gaussian dream
    data = make_data(n_rows, 9, gauss)               # 23 rows: 10, 10, 3; 21 rows: 10, 10, 1
    model = dict(bottoms=[twin_net(dbn)], joint=None)
    dbn._lower_cache[1] = "stale"
    seen = []
    hist = dbn.fine_tune(data, 2, batch_size=10, on_epoch=lambda e, rec: seen.append((e, rec)),
                         **{k: v for k, v in HP.items() if k != "batch_size"})
    want = twin_run(model, [data.astype(np.float64)], 2, HP, 77, 10)
    assert_net_equal(dbn, model["bottoms"][0])
    assert np.allclose(np.asarray(hist), np.asarray(want), rtol=1e-12, atol=0)
    assert seen == [(1, hist[0]), (2, hist[1])]
    assert dbn._lower_cache == {}
    per_epoch = len(mdbn_amd.get_minibatches_idx(n_rows, 10)[1])
    assert [r._rng_step for r in dbn.rbm_layers] == [4 * per_epoch, 4 * per_epoch, 2 * per_epoch]


def test_what_is_refused(monkeypatch):
    eng = UpdownOracle()
    one = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(1), n_ins=6, gauss=False,
                       hidden_layers_sizes=[], n_outs=4, engine=eng)
    with pytest.raises(ValueError):
        one.fine_tune(make_data(8, 6, False), 1, lr=0.1)
    dbn = make_dbn(eng)
    with pytest.raises(TypeError):
        dbn.fine_tune(make_data(8, 9, False), 1)                # lr has no default
    with pytest.raises(ValueError):
        dbn.fine_tune(make_data(8, 9, False), 1, lr=0.1, path="planes")
    with pytest.raises(ValueError):
        dbn.fine_tune(make_data(8, 7, False), 1, lr=0.1)        # wrong width

    class TwoRanks(object):
        world_size, rank = 2, 0
    monkeypatch.setattr(mdbn_amd.dist, "default_group", lambda: TwoRanks())
    with pytest.raises(NotImplementedError):
        dbn.fine_tune(make_data(8, 9, False), 1, lr=0.1)
    assert all(r.W_gen is None for r in dbn.rbm_layers)         # nothing was untied on the way


def test_tied_layers_make_the_calls_they_made_and_untied_ones_use_w_gen():
    eng = UpdownOracle()
    dbn = make_dbn(eng)
    data = make_data(6, 9, False)
    h = dbn.get_output(data)

    def down_calls():
        eng.log = []
        out = dbn.down_pass(h)
        return [c for c in eng.log if c[0] == "propdown"], out
    tied_calls, tied_out = down_calls()
    assert [c[1] for c in tied_calls] == [id(r.W.tensor) for r in reversed(dbn.rbm_layers)]
    updown.untie(dbn.rbm_layers[0])                              # W_gen == W: the numbers must not move
    calls, out = down_calls()
    assert [c[1] for c in calls] == [id(dbn.rbm_layers[2].W.tensor), id(dbn.rbm_layers[1].W.tensor), id(dbn.rbm_layers[0].W_gen.tensor)]
    assert np.array_equal(out, tied_out)
    dbn.rbm_layers[0].W_gen.tensor.mul_(0.5)
    assert not np.array_equal(dbn.down_pass(h), tied_out)
    assert np.array_equal(dbn.get_output(data), h)               # get_output keeps to W

    # the bound's directed term: row log-likelihoods through the generative weights
    seen = []
    eng.sample_replicas = lambda mean, S, rng: (torch.repeat_interleave((mean > 0.5).to(mean.dtype), S, dim=0), torch.zeros(mean.shape[0], dtype=mean.dtype))
    eng.propdown_row_loglik = lambda h_, W, vb, x, gauss, target_div=1: (seen.append(id(W)), torch.zeros(h_.shape[0], dtype=h_.dtype))[1]
    dbn.log_likelihood_bound(data, n_samples=2, log_z=0.0)
    assert seen == [id(dbn.rbm_layers[0].W_gen.tensor), id(dbn.rbm_layers[1].W.tensor)]


def test_checkpoint_round_trip_with_and_without_w_gen(tmp_path):
    eng = UpdownOracle()
    dbn = make_dbn(eng)
    path = str(tmp_path / "tied.npz")
    checkpoint.save_network(path, {"net": dbn}, resume=True)
    assert "W_gen" not in np.load(path, allow_pickle=True)["net_resume"][0]
    back = checkpoint.load_network(path, engine=eng)["net"]
    assert all(r.W_gen is None and r.W_gen_speed is None for r in back.rbm_layers)
    dbn.fine_tune(make_data(12, 9, False), 1, batch_size=6, lr=0.05, momentum=0.5)
    path = str(tmp_path / "untied.npz")
    checkpoint.save_network(path, {"net": dbn}, resume=True)
    back = checkpoint.load_network(path, engine=eng)["net"]
    for r, q in zip(dbn.rbm_layers, back.rbm_layers):
        assert (r.W_gen is None) == (q.W_gen is None)
        if r.W_gen is not None:
            assert np.array_equal(r.W_gen.get_value(), q.W_gen.get_value())
            assert np.array_equal(r.W_gen_speed.get_value(), q.W_gen_speed.get_value())
            assert q.W_gen.tensor.stride(0) == q.W.tensor.stride(0)
        assert np.array_equal(r.vbias.get_value(), q.vbias.get_value()) and r._rng_step == q._rng_step
    h = dbn.get_output(make_data(4, 9, False))
    assert np.allclose(dbn.down_pass(h), back.down_pass(h), atol=1e-6)      # (the file holds float32)


def test_the_multimodal_stack_concatenates_and_splits_blocks_in_order():
    eng = UpdownOracle()
    a = make_dbn(eng, sizes=(6, 3), gauss=True, seed=4)
    b = make_dbn(eng, sizes=(5, 4, 2), gauss=True, seed=5)
    joint = make_dbn(eng, sizes=(5, 4, 3), gauss=False, seed=6)
    joint.shuffle_rng = np.random.RandomState(31)
    inputs = [make_data(13, 6, True, 1), make_data(13, 5, True, 2)]
    model = dict(bottoms=[twin_net(a), twin_net(b)], joint=twin_net(joint))
    hp = {k: v for k, v in HP.items() if k != "batch_size"}
    hist = mdbn_amd.MDBN.fine_tune([a, b], joint, {1: inputs[1], 0: inputs[0]}, 2, batch_size=5, **hp)
    want = twin_run(model, [x.astype(np.float64) for x in inputs], 2, dict(HP, batch_size=5), 31, 5)
    for net, tw in ((a, model["bottoms"][0]), (b, model["bottoms"][1]), (joint, model["joint"])):
        assert_net_equal(net, tw)
    assert np.allclose(np.asarray(hist), np.asarray(want), rtol=1e-12, atol=0)
    assert all(r.W_gen is not None for r in a.rbm_layers + b.rbm_layers + joint.rbm_layers[:-1])
    assert joint.rbm_layers[-1].W_gen is None
    # one recorded step: the joint's wake input is [top of a | top of b], its dream's bottom splits back the same way
    rec = updown.step([a, b], joint, [eng.as_matrix(x[:4]) for x in inputs],
                      updown.Hyper(0.05, 0.05, 1, 0.0, 0.0, 0.0, 0.0, 4, "auto"))
    assert torch.equal(rec.x[2][0], torch.cat([rec.x[0][-1], rec.x[1][-1]], dim=1))
    assert torch.equal(rec.y[0][-1], rec.y[2][0][:, :3]) and torch.equal(rec.y[1][-1], rec.y[2][0][:, 3:])
    with pytest.raises(ValueError):
        mdbn_amd.MDBN.fine_tune([a, b], joint, [inputs[0]], 1, lr=0.1)
    with pytest.raises(ValueError):
        mdbn_amd.MDBN.fine_tune([b, a, a], joint, inputs + inputs[:1], 1, lr=0.1)     # tops do not fill the joint's inputs


# ------------------------------------------------------------------ the gain on an enumerable stack
def planted(n=60, seed=0):
    """Rows of four 6-bit prototypes with every bit flipped with probability 0.05."""
    rs = np.random.RandomState(seed)
    protos = np.array([[1, 1, 1, 0, 0, 0], [0, 0, 0, 1, 1, 1], [1, 0, 1, 0, 1, 0], [1, 1, 0, 0, 1, 1]], dtype=np.float32)
    rows = protos[rs.randint(0, 4, n)]
    return np.abs(rows - (rs.uniform(size=rows.shape) < 0.05)).astype(np.float32)


GAIN = dict(lr=0.1, top_lr=0.1, k=1, momentum=0.5, weightcost=0.0, lambda_1=0.0, lambda_2=0.0, batch_size=10)


def test_exact_log_p_rises_and_the_public_classes_follow_the_twin():
    eng = UpdownOracle()
    dbn = make_dbn(eng, sizes=(6, 4, 3), seed=8, scale=0.3)
    data = planted()
    model = dict(bottoms=[twin_net(dbn)], joint=None)
    start = ud.exact_log_p(model["bottoms"][0], data).mean()
    curve = [start]
    rng = np.random.RandomState(77)
    for _ in range(30):
        for b in mdbn_amd.get_minibatches_idx(len(data), 10, shuffle=True, rng=rng)[1]:
            ud.step(model, [data[b].astype(np.float64)], GAIN)
        curve.append(ud.exact_log_p(model["bottoms"][0], data).mean())
    # the planted set has about 4 prototypes x flip noise: 6 log 2 = 4.16 nats is the untrained stack's level
    assert curve[-1] > start + 0.5, curve
    assert curve[10] > start and curve[20] > curve[5]
    dbn.fine_tune(data, 30, batch_size=10, **{k: v for k, v in GAIN.items() if k != "batch_size"})
    assert_net_equal(dbn, model["bottoms"][0])
