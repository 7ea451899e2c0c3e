"""The variational lower bound of stacks with categorical visible units on the host (mdbn_amd/bound.py, DBN.log_likelihood_bound,
mdbn_amd.log_likelihood_bound) against the float64 twin (tests/_gbound_np.py) and an enumeration of the model, on the CPU
checker engine; the C declarations of mdbn_propdown_rowll_grouped.  No GPU."""
import itertools
import os
import re

import numpy as np
import pytest

import _dbn_bound_np as T
import _gbound_np as Gb
import _softmax_np as sm
import mdbn_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mdbn_propdown_rowll_grouped", "mdbn_rowll_grouped_workspace_bytes")
S = 64
SCALES = (0.5, 1.5)
STACKS = ("mixed_10_6_4", "k3_9_5_4_3", "forest")


def build(layers, eng):
    """The DBN of a twin net on ``eng`` (its RBMs take the streams 0, 1, ... of the net's seed, as the twin's layers)."""
    mdbn_amd.DBN.verbose = False
    sizes = [layers[0]["W"].shape[0]] + [l["W"].shape[1] for l in layers]
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(0), theano_rng=mdbn_amd.RandomStreams(layers[0]["seed"]), n_ins=sizes[0],
                       gauss=layers[0]["gauss"], hidden_layers_sizes=sizes[1:-1], n_outs=sizes[-1],
                       W_list=[l["W"] for l in layers], b_list=[l["b"] for l in layers], engine=eng,
                       visible_groups=layers[0].get("bounds"))
    for r, l in zip(net.rbm_layers, layers):
        r.vbias.set_value(l["c"])
        assert r.stream_id == l["stream"] and r._rng_step == l["step"] and r.gauss == l["gauss"]
    return net


def build_model(model, eng):
    nets = [build(layers, eng) for layers in model["bottoms"]]
    return nets, (build(model["joint"], eng) if model["joint"] is not None else None)


def run(model, inputs, eng, **kw):
    nets, joint = build_model(model, eng)
    if joint is None:
        return nets[0].log_likelihood_bound(inputs[0], **kw), nets, joint
    return mdbn_amd.log_likelihood_bound(nets, joint, {i: x for i, x in enumerate(inputs)}, **kw), nets, joint


@pytest.fixture(scope="module")
def truth():
    out = {}
    for scale in SCALES:
        for name, (model, inputs) in Gb.stacks(scale).items():
            out[name, scale] = (model, inputs) + Gb.brute_force(model, inputs)
    return out


# ------------------------------------------------------------------ 1. the twin against first principles
def test_twin_row_loglik_is_the_log_of_the_grouped_means_at_the_targets_ones():
    rs = np.random.RandomState(1)
    for V, H, bounds in ((10, 3, [0, 3, 6, 8]), (12, 7, [2, 5, 8, 10]), (70, 9, [1, 3, 67, 70])):
        layer = dict(W=rs.normal(size=(V, H)), c=rs.normal(size=V), gauss=False)
        h = (rs.uniform(size=(11, H)) < 0.5).astype(np.float64)
        t = sm.one_hot_data(rs, 11, V, bounds, p=0.5).astype(np.float64)
        pre = h @ layer["W"].T + layer["c"]
        mean = sm.grouped_softmax(pre, bounds)[0]
        cols = sm.bernoulli_columns(bounds, V)
        want = (t[:, cols] * pre[:, cols] - T.softplus(pre[:, cols])).sum(axis=1)
        for lo, hi in sm.spans(bounds):
            want = want + np.log((t[:, lo:hi] * mean[:, lo:hi]).sum(axis=1))
        got = Gb.row_loglik_grouped(h, layer, t, bounds)
        assert np.abs(got - want).max() < 1e-12
        assert np.abs(Gb.row_loglik(h, dict(layer, bounds=bounds), t) - got).max() == 0.0
        # (a layer without a table is the Bernoulli twin's)
        assert np.array_equal(Gb.row_loglik(h, layer, t), T.row_loglik(h, layer, t))
    # finite where a probability underflows
    layer = dict(W=np.zeros((4, 1)), c=np.array([100.0, -100.0, 0.0, 3.0]), gauss=False)
    got = Gb.row_loglik_grouped(np.zeros((1, 1)), layer, np.array([[0.0, 1.0, 0.0, 1.0]]), [0, 3])
    assert np.isfinite(got).all() and abs(got[0] - (-200.0 + 3.0 - T.softplus(3.0))) < 1e-9


def test_twin_row_loglik_is_the_enumerated_energy_function():
    """Groups (3, 3, 2) plus two Bernoulli units, H = 3: log p(v | h) = -E(v, h) - log sum_v' exp(-E(v', h)) over the 72
    visible states, for each of the 8 hidden states."""
    rs = np.random.RandomState(3)
    bounds, Vs, Hs = [0, 3, 6, 8], 10, 3
    W, hb, vb = rs.normal(size=(Vs, Hs)), rs.normal(size=Hs), rs.normal(size=Vs)
    vis = []
    for a, b, c, d, e in itertools.product(range(3), range(3), range(2), range(2), range(2)):
        v = np.zeros(Vs)
        v[a], v[3 + b], v[6 + c], v[8], v[9] = 1, 1, 1, d, e
        vis.append(v)
    vis = np.array(vis)
    hid = np.array(list(itertools.product((0.0, 1.0), repeat=Hs)))
    neg_e = vis @ vb[:, None] + (hid @ hb)[None, :] + vis @ W @ hid.T                   # -E [72, 8]
    want = neg_e - np.logaddexp.reduce(neg_e, axis=0)[None, :]
    layer = dict(W=W, c=vb, gauss=False)
    for j, h in enumerate(hid):
        got = Gb.row_loglik_grouped(np.repeat(h[None, :], len(vis), axis=0), layer, vis, bounds)
        assert np.abs(got - want[:, j]).max() < 1e-12
        assert abs(np.logaddexp.reduce(got)) < 1e-12                                   # a distribution over the 72 states


# ------------------------------------------------------------------ 2. the exact bound and the sampled estimate
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", STACKS)
def test_exact_bound_is_below_log_p_and_the_estimate_meets_it(truth, name, scale):
    model, inputs, log_p, exact, log_z = truth[name, scale]
    assert (exact <= log_p + 1e-12).all() and (exact < log_p - 1e-6).any()
    est = Gb.estimate(model, inputs, S, log_z)
    print("%s scale %.1f: exact %.6f, estimate %.6f +- %.6f, log p %.6f" % (name, scale, exact.mean(), est["bound"], est["stderr"],
                                                                           log_p.mean()))
    assert est["stderr"] > 0 and abs(est["bound"] - exact.mean()) <= 4 * est["stderr"]
    # (the grouped term matters: the same stack scored as independent sigmoids is another number)
    plain = dict(model, bottoms=[[{k: v for k, v in l.items() if k != "bounds"} for l in net] for net in model["bottoms"]])
    assert abs(T.estimate(plain, inputs, S, log_z)["bound"] - est["bound"]) > 0.1


# ------------------------------------------------------------------ 3. one layer
def test_one_layer_network_with_groups_is_the_rbm_log_likelihood_and_draws_nothing():
    rs = np.random.RandomState(7)
    bounds = [0, 3, 6, 8]
    layers = Gb.make_net(rs, (10, 4), 1.0, 91, bounds)
    x = sm.one_hot_data(rs, 5, 10, bounds, p=0.5)
    eng = Gb.GboundOracle()
    net = build(layers, eng)
    rbm = net.rbm_layers[0]
    rbm._rng_step = 5
    log_z = T.exact_log_z(T.f64(layers[0])) + 0.25                                      # any given value is used as it is
    r = net.log_likelihood_bound(x, log_z=log_z)
    assert eng.calls == [] and rbm._rng_step == 5, "a one-layer bound draws nothing"
    want = -T.free_energy(x, T.f64(layers[0])) - log_z
    assert np.abs(r.rows - want).max() < 1e-12 and r.stderr == 0.0 and (r.row_stderr == 0).all() and r.log_z_stderr == 0.0
    rbm.log_partition = lambda **kw: (log_z, 0.0)
    ll, err = rbm.log_likelihood(x)
    assert abs(r.bound - ll) < 1e-6 * max(1.0, abs(ll)) and err == 0.0                   # (free_energy().get_value() is float32)


# ------------------------------------------------------------------ 4. through the public classes
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", STACKS)
def test_public_calls_on_the_checker_engine_equal_the_twin(truth, name, scale):
    model, inputs, _, _, log_z = truth[name, scale]
    eng = Gb.GboundOracle()
    r, nets, joint = run(model, inputs, eng, n_samples=S, log_z=log_z, trace=True)
    est = Gb.estimate(model, inputs, S, log_z)
    assert np.abs(r.rows - est["rows"]).max() < 1e-10 and np.abs(r.trace["values"] - est["values"]).max() < 1e-10
    assert abs(r.bound - est["bound"]) < 1e-10 and abs(r.stderr - est["stderr"]) < 1e-10
    assert eng.calls.count("propdown_row_loglik_grouped") == 1, "one grouped directed term: the input layer of the grouped net"
    if joint is None:
        assert [x._rng_step for x in nets[0].rbm_layers] == [1] * (nets[0].n_layers - 1) + [0]
    else:
        assert np.abs(r.modality_rows - est["modality_rows"]).max() < 1e-10
        assert np.abs(r.modality_rows.sum(axis=0) + r.joint_rows - r.rows).max() <= 1e-9 * max(1.0, np.abs(r.rows).max())
        assert [x._rng_step for n in nets for x in n.rbm_layers] == [1, 1] and [x._rng_step for x in joint.rbm_layers] == [1, 0]
    assert eng.calls.count("sample_replicas") == sum(x._rng_step for n in nets + ([joint] if joint else []) for x in n.rbm_layers)
    # three data rows per chunk: the same rows
    cut, nets2, joint2 = run(model, inputs, Gb.GboundOracle(), n_samples=S, log_z=log_z, chunk_rows=3 * S)
    whole = run(model, inputs, Gb.GboundOracle(), n_samples=S, log_z=log_z, chunk_rows=16384)[0]
    assert np.array_equal(cut.rows, whole.rows) and np.array_equal(whole.rows, r.rows)
    assert sum(x._rng_step for n in nets2 + ([joint2] if joint2 else []) for x in n.rbm_layers) == eng.calls.count("sample_replicas")


# ------------------------------------------------------------------ 5. refusals
def test_refusals_come_before_any_draw(truth):
    model, inputs = truth["mixed_10_6_4", 0.5][:2]
    forest, finputs = truth["forest", 0.5][:2]

    def steps(nets):
        return [r._rng_step for n in nets for r in n.rbm_layers]

    # an engine that lacks the grouped directed term: the DBN call and the forest call
    plain_eng = sm.GroupedOracle()
    net = build(model["bottoms"][0], plain_eng)
    with pytest.raises(NotImplementedError, match="visible_groups"):
        net.log_likelihood_bound(inputs[0], n_samples=4, log_z=0.0)
    fnets, fjoint = build_model(forest, plain_eng)
    with pytest.raises(NotImplementedError, match="visible_groups"):
        mdbn_amd.log_likelihood_bound(fnets, fjoint, finputs, n_samples=4, log_z=0.0)
    assert steps([net] + fnets + [fjoint]) == [0] * 6
    # two ones in a group; a group of zeros; a value that is neither 0 nor 1
    eng = Gb.GboundOracle()
    net = build(model["bottoms"][0], eng)
    fnets, fjoint = build_model(forest, eng)
    for col, value in ((1, 1.0), (None, 0.0), (0, 0.5)):
        bad, fbad = inputs[0].copy(), finputs[0].copy()
        for x in (bad, fbad):
            c = int(x[2, :3].argmax())
            x[2, (c + 1) % 3 if col == 1 else c] = value
        with pytest.raises(ValueError, match="exactly one 1"):
            net.log_likelihood_bound(bad, n_samples=4, log_z=0.0)
        with pytest.raises(ValueError, match="exactly one 1"):
            net.log_likelihood_bound(mdbn_amd.shared(bad, engine=eng), n_samples=4, log_z=0.0)
        with pytest.raises(ValueError, match="exactly one 1"):
            mdbn_amd.log_likelihood_bound(fnets, fjoint, [fbad, finputs[1]], n_samples=4, log_z=0.0)
    # fine-tuning stays refused
    with pytest.raises(NotImplementedError, match="visible_groups"):
        net.fine_tune(inputs[0], 1, batch_size=3, lr=0.01)
    assert steps([net] + fnets + [fjoint]) == [0] * 6 and eng.calls == []
    # ... and the good rows go through on the same objects
    assert net.log_likelihood_bound(inputs[0], n_samples=2, log_z=0.0).rows.shape == (6,)


# ------------------------------------------------------------------ 6. declarations
def test_declarations_bindings_and_doc_comment():
    from mdbn_amd import _lib
    text = open(os.path.join(ROOT, "include", "mdbn_hip.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert name in comments, "%s is not described in a comment of the header" % name
        decl = code[code.index("int  %s(" % name):]
        assert len(_lib.SIGNATURES[name]) == decl[:decl.index(");")].count(",") + 1, name
    assert len(_lib.SIGNATURES["mdbn_propdown_rowll_grouped"]) == len(_lib.SIGNATURES["mdbn_propdown_rowll"]) - 1 + 3
    decl = code[code.index("int  mdbn_propdown_rowll_grouped("):]
    assert re.sub(r"\s+", " ", decl[:decl.index(");")]).endswith(
        "const int32_t *group_start, const int32_t *group_start_host, int64_t n_groups")
    assert "#define MDBN_VERSION 2" in text
    assert callable(mdbn_amd.HipEngine.propdown_row_loglik_grouped)
