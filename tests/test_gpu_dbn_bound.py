"""The variational lower bound on the device (csrc/mdbn_bound.hip: mdbn_propdown_rowll, mdbn_sample_replicas;
DBN.log_likelihood_bound, mdbn_amd.log_likelihood_bound) against the float64 formulas and the numpy twin
(tests/_dbn_bound_np.py), which draws the uniforms the device draws."""
import numpy as np
import pytest

import _dbn_bound_np as T
import _margins
import _saturated
from oracle import philox_np

pytestmark = pytest.mark.gpu

TOL = _margins.SURVEY["free_energy"]            # 1e-4 max(1, |ref|): the bound of a row-reduced softplus sum
SHAPES = [(6, 5, 5, 1), (37, 40, 15, 3), (130, 129, 33, 1), (300, 200, 70, 7), (500, 24, 129, 64)]      # (V, H, R, target_div)
S = 64


def _rel(got, ref):
    return float((np.abs(np.asarray(got, dtype=np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())


def _case(V, H, R, div, gauss, seed=0):
    rs = np.random.RandomState(seed + V + 7 * H + 13 * R)
    h = (rs.uniform(size=(R, H)) < 0.5).astype(np.float32)
    W = (rs.normal(0, 1, (V, H)) / np.sqrt(H)).astype(np.float32)
    vb = rs.normal(0, 0.5, V).astype(np.float32)
    n_t = (R + div - 1) // div
    target = rs.normal(0, 1, (n_t, V)).astype(np.float32) if gauss else (rs.uniform(size=(n_t, V)) < 0.5).astype(np.float32)
    return h, W, vb, target


def _reference(h, W, vb, target, div, gauss):
    layer = dict(W=W.astype(np.float64), c=vb.astype(np.float64), gauss=gauss)
    return T.row_loglik(h, layer, np.repeat(target.astype(np.float64), div, axis=0)[:len(h)])


def _matrix(eng, a, ld=None, fill=None):
    """``a`` as a device matrix on the leading dimension ``ld``; ``fill``: the value of its pad columns."""
    m = eng.alloc_matrix(a.shape[0], a.shape[1], ld)
    if fill is not None:
        m._base[:, a.shape[1]:] = fill
    m.copy_(eng.to_device(a))
    return m


# ------------------------------------------------------------------ the fused propdown + row log-likelihood
@pytest.mark.parametrize("gauss", (False, True))
@pytest.mark.parametrize("V,H,R,div", SHAPES)
def test_row_loglik_meets_the_float64_formula(hip_engine, V, H, R, div, gauss):
    eng = hip_engine
    h, W, vb, target = _case(V, H, R, div, gauss)
    ref = _reference(h, W, vb, target, div, gauss)
    args = (eng.to_device(h), eng.to_device(W), eng.to_device(vb), eng.to_device(target), gauss, div)
    out = eng.propdown_row_loglik(*args)
    again = eng.propdown_row_loglik(*args)
    got = eng.to_numpy(out)
    assert got.shape == (R,) and np.isfinite(got).all()
    print("rowll V=%d H=%d R=%d div=%d gauss=%d: worst %.3e of %.1e" % (V, H, R, div, gauss, _rel(got, ref), TOL))
    _margins.check("rowll_%s" % ("gauss" if gauss else "bernoulli"), _rel(got, ref), TOL, "free_energy")
    assert np.array_equal(got, eng.to_numpy(again)), "two runs on the same inputs differ"


@pytest.mark.parametrize("gauss", (False, True))
@pytest.mark.parametrize("which", ("h", "W", "target"))
def test_row_loglik_never_reads_its_padding(hip_engine, which, gauss):
    """NaN in the pad columns of one operand (h and W beyond H, target beyond V) changes no bit of the result."""
    eng = hip_engine
    V, H, R, div = 130, 129, 33, 1
    h, W, vb, target = _case(V, H, R, div, gauss)
    ref = _reference(h, W, vb, target, div, gauss)
    outs = []
    for fill in (0.0, float("nan")):
        mats = {k: _matrix(eng, a, 136, fill if k == which else 0.0) for k, a in (("h", h), ("W", W), ("target", target))}
        if fill != 0.0:
            assert bool(mats[which]._base[:, mats[which].shape[1]:].isnan().all())
        outs.append(eng.to_numpy(eng.propdown_row_loglik(mats["h"], mats["W"], eng.to_device(vb), mats["target"], gauss, div)))
    assert np.isfinite(outs[1]).all() and np.array_equal(outs[0], outs[1])
    _margins.check("rowll_padding", _rel(outs[1], ref), TOL, "free_energy")


def test_row_loglik_on_a_saturated_layer(hip_engine):
    """|pre| in the tens (the bias ladder of tests/_saturated.py): every value finite, and still the float64 formula's."""
    eng = hip_engine
    V, H, R, div = 300, 200, 70, 7
    rs = np.random.RandomState(21)
    W, _, vb = _saturated.params(rs, V, H, gauss=False)
    h, _, _, target = _case(V, H, R, div, False)
    pre = h.astype(np.float64) @ W.astype(np.float64).T + vb
    _saturated.assert_bands("rowll", [pre], bands=_saturated.REGIMES)
    ref = _reference(h, W, vb, target, div, False)
    got = eng.to_numpy(eng.propdown_row_loglik(eng.to_device(h), eng.to_device(W), eng.to_device(vb), eng.to_device(target), False, div))
    assert np.isfinite(got).all()
    print("rowll saturated: worst %.3e of %.1e" % (_rel(got, ref), TOL))
    _margins.check("rowll_saturated", _rel(got, ref), TOL, "free_energy")


def test_row_loglik_refuses_bad_arguments(hip_engine):
    eng = hip_engine
    h, W, vb, target = _case(37, 40, 15, 3, False)
    d = [eng.to_device(a) for a in (h, W, vb, target)]
    with pytest.raises(ValueError):
        eng.propdown_row_loglik(d[0], d[1], d[2], d[3], False, 1)          # 15 rows at target_div 1 need 15 target rows
    with pytest.raises(ValueError):
        eng.propdown_row_loglik(d[0], d[1], d[2], d[3], False, 0)
    with pytest.raises(ValueError):
        eng.propdown_row_loglik(d[0][:, :39], d[1], d[2], d[3], False, 3)


# ------------------------------------------------------------------ the replica sampler
def _means(rs, N, H):
    m = rs.uniform(size=(N, H)).astype(np.float32)
    m[0, 0], m[0, 1], m[-1, -1], m[N // 2, H // 2] = 0.0, 1.0, 1.0, 0.0
    return m


@pytest.mark.parametrize("N,S_,H,offset", [(7, 5, 13, 0), (7, 5, 13, 6), (33, 1, 70, 0), (3, 64, 130, 192)])
def test_replica_samples_are_the_philox_uniforms_below_the_mean(hip_engine, N, S_, H, offset):
    from mdbn_amd import RngAddr
    eng = hip_engine
    m = _means(np.random.RandomState(N + H), N, H)
    seed, stream, step = 4242, 3, 17
    sample, ent = eng.sample_replicas(eng.to_device(m), S_, RngAddr(seed, stream, step, 0, offset))
    u = philox_np.uniform(N * S_, H, seed, stream, step, 0, offset)
    want = (u < np.repeat(m, S_, axis=0)).astype(np.float32)          # float32 against float32: exact, no tie to skip
    assert np.array_equal(eng.to_numpy(sample), want)
    assert not bool(sample._base[:, H:].any()), "pad columns of the samples must stay zero"
    dev_u = eng.to_numpy(eng.rng_uniform(N * S_, H, RngAddr(seed, stream, step, 0, offset)))
    assert np.array_equal(dev_u, u)
    ref = T.entropy(m)
    got = eng.to_numpy(ent).astype(np.float64)
    assert np.isfinite(got).all()
    _margins.check("replica_entropy_per_unit", np.abs(got - ref).max() / H, 1e-5)


def test_replica_sampler_chunks_draw_what_one_call_draws(hip_engine):
    from mdbn_amd import RngAddr
    eng = hip_engine
    N, S_, H, cut = 9, 5, 21, 3                                        # the second call starts at replica row 15: inside a Philox block
    m = _means(np.random.RandomState(1), N, H)
    whole, ent = eng.sample_replicas(eng.to_device(m), S_, RngAddr(7, 1, 2, 0, 0))
    a, ent_a = eng.sample_replicas(eng.to_device(m[:cut]), S_, RngAddr(7, 1, 2, 0, 0))
    b, ent_b = eng.sample_replicas(eng.to_device(m[cut:]), S_, RngAddr(7, 1, 2, 0, cut * S_))
    assert np.array_equal(eng.to_numpy(whole), np.concatenate([eng.to_numpy(a), eng.to_numpy(b)]))
    assert np.array_equal(eng.to_numpy(ent), np.concatenate([eng.to_numpy(ent_a), eng.to_numpy(ent_b)]))
    with pytest.raises(ValueError):
        eng.sample_replicas(eng.to_device(m), 0, RngAddr(7, 1, 2, 0, 0))


# ------------------------------------------------------------------ end to end, on the twin's stacks
def _build(layers, eng):
    """The DBN of a twin net (its RBMs take the streams 0, 1, ... of the net's seed, as the twin's layers)."""
    import mdbn_amd
    mdbn_amd.DBN.verbose = False
    sizes = [layers[0]["W"].shape[0]] + [l["W"].shape[1] for l in layers]
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(0), theano_rng=mdbn_amd.RandomStreams(layers[0]["seed"]), n_ins=sizes[0],
                       gauss=layers[0]["gauss"], hidden_layers_sizes=sizes[1:-1], n_outs=sizes[-1],
                       W_list=[l["W"] for l in layers], b_list=[l["b"] for l in layers], engine=eng)
    for r, l in zip(net.rbm_layers, layers):
        r.vbias.set_value(l["c"])
        assert r.stream_id == l["stream"] and r._rng_step == l["step"] and r.gauss == l["gauss"]
    return net


@pytest.fixture(scope="module")
def truth():
    out = {}
    for scale in (0.5, 1.5):
        for name, (model, inputs) in T.stacks(scale).items():
            out[name, scale] = (model, inputs) + T.brute_force(model, inputs)
    return out


def _trace_samples(record):
    return [net["samples"] for net in record.trace["nets"]]


@pytest.mark.parametrize("scale", (0.5, 1.5))
@pytest.mark.parametrize("name", ("bernoulli_8_6_4", "gauss_8_6_4", "deep_7_5_4_3"))
def test_dbn_bound_meets_the_twin_and_the_exact_bound(hip_engine, truth, name, scale):
    model, inputs, _, exact, log_z = truth[name, scale]
    net = _build(model["bottoms"][0], hip_engine)
    r = net.log_likelihood_bound(inputs[0], n_samples=S, log_z=log_z, trace=True)
    assert [x._rng_step for x in net.rbm_layers] == [1] * (net.n_layers - 1) + [0], "one step per sampled layer, none of the top"
    assert r.rows.dtype == np.float64 and r.rows.shape == (6,) and r.log_z == log_z and r.log_z_stderr == 0.0
    # teacher-forced: the twin along the device's own samples
    forced = T.estimate(model, inputs, S, log_z, samples=_trace_samples(r))
    _margins.check("bound_rows_teacher_forced", _rel(r.rows, forced["rows"]), TOL, "free_energy")
    _margins.check("bound_values_teacher_forced", _rel(r.trace["values"], forced["values"]), TOL, "free_energy")
    assert abs(r.bound - r.rows.mean()) <= 1e-12 and abs(r.stderr - forced["stderr"]) <= 1e-4 * max(1.0, forced["stderr"])
    # the device drew the twin's uniforms: the first sampled layer differs from the free-running twin at ties only
    free = T.estimate(model, inputs, S, log_z)
    differ = r.trace["nets"][0]["samples"][0] != free["samples"][0][0]
    assert (np.abs(free["uniforms"][0][0] - free["means"][0][0])[differ] < 4e-6).all() and differ.mean() <= 1e-3
    # and the estimate meets the exact bound within 4 of its standard errors
    assert r.stderr > 0 and abs(r.bound - exact.mean()) <= 4 * r.stderr, (r.bound, exact.mean(), r.stderr)


def test_dbn_bound_does_not_depend_on_the_chunking(hip_engine, truth):
    model, inputs, _, exact, log_z = truth["deep_7_5_4_3", 0.5]
    whole = _build(model["bottoms"][0], hip_engine).log_likelihood_bound(inputs[0], n_samples=S, log_z=log_z, trace=True)
    net = _build(model["bottoms"][0], hip_engine)
    cut = net.log_likelihood_bound(inputs[0], n_samples=S, log_z=log_z, chunk_rows=2 * S, trace=True)
    assert [x._rng_step for x in net.rbm_layers] == [1, 1, 0], "three chunks, one step"
    forced = T.estimate(model, inputs, S, log_z, samples=_trace_samples(cut))
    _margins.check("bound_rows_chunked", _rel(cut.rows, forced["rows"]), TOL, "free_energy")
    assert np.array_equal(cut.trace["nets"][0]["samples"][0], whole.trace["nets"][0]["samples"][0]), "a chunk changed a draw"
    assert abs(cut.bound - exact.mean()) <= 4 * cut.stderr


def test_host_resident_table_streams_to_the_same_rows(hip_engine, truth):
    """A HostTable is gathered chunk by chunk (never mirrored on the device) and gives the rows of the uploaded matrix."""
    import mdbn_amd
    model, inputs, _, _, log_z = truth["gauss_8_6_4", 0.5]
    want = _build(model["bottoms"][0], hip_engine).log_likelihood_bound(inputs[0], n_samples=S, log_z=log_z, trace=True)
    table = mdbn_amd.shared(inputs[0], engine=hip_engine, resident="host")
    got = _build(model["bottoms"][0], hip_engine).log_likelihood_bound(table, n_samples=S, log_z=log_z, chunk_rows=4 * S, trace=True)
    assert table._mirror is None, "the table was uploaded whole"
    assert np.array_equal(got.trace["nets"][0]["samples"][0], want.trace["nets"][0]["samples"][0])
    # (the same samples; the free-energy pass of 256 + 128 rows may group its float32 sums otherwise than that of 384)
    _margins.check("bound_rows_host_table", _rel(got.rows, want.rows), TOL, "free_energy")


@pytest.mark.parametrize("scale", (0.5, 1.5))
def test_tied_transpose_stack_meets_the_first_rbm(hip_engine, truth, scale):
    model, inputs = truth["bernoulli_8_6_4", scale][:2]
    tied = T.tied(model)
    log_z = T.exact_log_z(T.f64(tied["bottoms"][0][1]))
    net = _build(tied["bottoms"][0], hip_engine)
    r = net.log_likelihood_bound(inputs[0], n_samples=S, log_z=log_z)
    first = net.rbm_layers[0]
    rbm1 = -first.free_energy(inputs[0]).get_value().astype(np.float64) - log_z      # log p_RBM1(x_0): Z_1 = Z_2 when tied
    assert r.trace is None
    assert abs(r.bound - rbm1.mean()) <= 4 * r.stderr + TOL * max(1.0, abs(rbm1.mean())), (r.bound, rbm1.mean(), r.stderr)


@pytest.mark.parametrize("gauss", (False, True))
def test_one_layer_network_is_log_likelihood(hip_engine, gauss):
    rs = np.random.RandomState(5)
    layers = T.make_net(rs, (8, 4), gauss, 1.0, 77)
    x = T.make_data(rs, 5, 8, gauss)
    net = _build(layers, hip_engine)
    want, err = net.rbm_layers[0].log_likelihood(x, n_chains=64, n_betas=100)
    used = net.rbm_layers[0]._rng_step
    net.rbm_layers[0]._rng_step = 0
    r = net.log_likelihood_bound(x, n_chains=64, n_betas=100)
    assert net.rbm_layers[0]._rng_step == used, "only the AIS run of log Z consumes random numbers"
    assert abs(r.bound - want) <= 1e-6 * max(1.0, abs(want)) and r.log_z_stderr == err and r.stderr == 0.0
    assert (r.row_stderr == 0).all()
    exact = -T.free_energy(x, T.f64(layers[0])) - r.log_z
    _margins.check("bound_one_layer_rows", _rel(r.rows, exact), TOL, "free_energy")


def test_log_partition_keywords_and_base_rate_pass_through(hip_engine, truth):
    model, inputs = truth["bernoulli_8_6_4", 0.5][:2]
    net = _build(model["bottoms"][0], hip_engine)
    seen = {}

    def fake(**kw):
        seen.update(kw)
        return 1.25, 0.5
    net.rbm_layers[-1].log_partition = fake
    r = net.log_likelihood_bound(inputs[0], n_samples=4, method="tempering", n_sweeps=50)
    assert seen["method"] == "tempering" and seen["n_sweeps"] == 50
    assert np.array_equal(seen["data"], net.get_output(inputs[0], 0)), "base rate: the data seen through the layers below"
    assert r.log_z == 1.25 and r.log_z_stderr == 0.5


@pytest.mark.parametrize("scale", (0.5, 1.5))
def test_two_modality_stack_meets_its_twin(hip_engine, truth, scale):
    import mdbn_amd
    model, inputs, _, exact, log_z = truth["forest", scale]
    nets = [_build(layers, hip_engine) for layers in model["bottoms"]]
    joint = _build(model["joint"], hip_engine)
    r = mdbn_amd.log_likelihood_bound(nets, joint, {0: inputs[0], 1: inputs[1]}, n_samples=S, log_z=log_z, trace=True)
    assert [x._rng_step for n in nets for x in n.rbm_layers] == [1, 1] and [x._rng_step for x in joint.rbm_layers] == [1, 0]
    forced = T.estimate(model, inputs, S, log_z, samples=_trace_samples(r))
    _margins.check("stack_rows_teacher_forced", _rel(r.rows, forced["rows"]), TOL, "free_energy")
    _margins.check("stack_modality_rows", _rel(r.modality_rows, forced["modality_rows"]), TOL, "free_energy")
    _margins.check("stack_joint_rows", _rel(r.joint_rows, forced["joint_rows"]), TOL, "free_energy")
    assert np.abs(r.modality_rows.sum(axis=0) + r.joint_rows - r.rows).max() <= 1e-9 * max(1.0, np.abs(r.rows).max())
    assert r.stderr > 0 and abs(r.bound - exact.mean()) <= 4 * r.stderr, (r.bound, exact.mean(), r.stderr)
