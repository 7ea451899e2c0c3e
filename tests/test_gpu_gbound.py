"""The variational lower bound for categorical visible units on the device (csrc/mdbn_bound.hip: mdbn_propdown_rowll_grouped;
DBN.log_likelihood_bound and mdbn_amd.log_likelihood_bound on a layer with visible_groups) against the float64 formula and the
numpy twin (tests/_gbound_np.py).

The kernel cases (V, H, R, target_div; boundaries), tiles being 128 rows x 128 columns:
  (7, 5, 5, 1)       [1, 4, 7]                      the smallest mixed layer
  (70, 40, 15, 3)    [1, 3, 67, 70]                 K = 2, 64 and 3 behind a Bernoulli column
  (300, 200, 70, 7)  [2, 66, 130, 194, 258, 300]    groups of 64 and 42 across columns 128 and 256; a group across the 64- and
                                                    32-column seams inside a tile (wave and fragment boundaries)
  (500, 24, 129, 64) K = 5 throughout               a group cut at every tile edge; a second row tile with one live row
  (794, 24, 33, 1)   [784, 794]                     a label block in the last, partial tile; V % 4 = 2
  (260, 33, 130, 2)  [100, 103, 167, 170]           Bernoulli columns on both sides; a second row tile with two live rows"""
import ctypes as C

import numpy as np
import pytest

import _dbn_bound_np as T
import _gbound_np as Gb
import _margins
import _saturated
import _softmax_np as sm

pytestmark = pytest.mark.gpu

TOL = _margins.SURVEY["free_energy"]            # 1e-4 max(1, |ref|): the bound of a row-reduced softplus / log-sum-exp sum
S = 64
BIG = (300, 200, 70, 7, [2, 66, 130, 194, 258, 300])
IDS = ["%dx%dx%d" % c[:3] for c in Gb.KERNEL_CASES]


def _rel(got, ref):
    return float((np.abs(np.asarray(got, dtype=np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())


def _matrix(eng, a, ld=None, fill=None):
    """``a`` as a device matrix on the leading dimension ``ld``; ``fill``: the value of its pad columns."""
    m = eng.alloc_matrix(a.shape[0], a.shape[1], ld)
    if fill is not None:
        m._base[:, a.shape[1]:] = fill
    m.copy_(eng.to_device(a))
    return m


def _table(eng, bounds):
    from mdbn_amd.engine import GroupTable
    return GroupTable(eng, np.asarray(bounds, dtype=np.int32))


# ------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("V,H,R,div,bounds", Gb.KERNEL_CASES, ids=IDS)
def test_grouped_row_loglik_meets_the_float64_formula(hip_engine, V, H, R, div, bounds):
    eng = hip_engine
    h, W, vb, target = Gb.kernel_case(V, H, R, div, bounds)
    ref = Gb.kernel_reference(h, W, vb, target, div, bounds)
    args = (eng.to_device(h), eng.to_device(W), eng.to_device(vb), eng.to_device(target), _table(eng, bounds), div)
    out = eng.propdown_row_loglik_grouped(*args)
    again = eng.propdown_row_loglik_grouped(*args)
    got = eng.to_numpy(out)
    assert got.shape == (R,) and np.isfinite(got).all()
    print("grouped rowll V=%d H=%d R=%d div=%d: worst %.3e of %.1e" % (V, H, R, div, _rel(got, ref), TOL))
    _margins.check("rowll_grouped", _rel(got, ref), TOL, "free_energy")
    assert np.array_equal(got, eng.to_numpy(again)), "two runs on the same inputs differ"
    # (the table matters: the same layer scored as sigmoids is another number)
    plain = eng.to_numpy(eng.propdown_row_loglik(args[0], args[1], args[2], args[3], False, div))
    assert np.abs(plain - ref).max() > 0.1


@pytest.mark.parametrize("which", ("h", "W", "target"))
def test_grouped_row_loglik_never_reads_its_padding(hip_engine, which):
    """NaN in the pad columns of one operand (h and W beyond H: ld 208; target beyond V: ld 304) changes no bit."""
    eng = hip_engine
    V, H, R, div, bounds = BIG
    h, W, vb, target = Gb.kernel_case(V, H, R, div, bounds)
    ref = Gb.kernel_reference(h, W, vb, target, div, bounds)
    outs = []
    for fill in (0.0, float("nan")):
        mats = {k: _matrix(eng, a, ld, fill if k == which else 0.0) for k, a, ld in (("h", h, 208), ("W", W, 208), ("target", target, 304))}
        if fill != 0.0:
            assert bool(mats[which]._base[:, mats[which].shape[1]:].isnan().all())
        outs.append(eng.to_numpy(eng.propdown_row_loglik_grouped(mats["h"], mats["W"], eng.to_device(vb), mats["target"],
                                                                 _table(eng, bounds), div)))
    assert np.isfinite(outs[1]).all() and np.array_equal(outs[0], outs[1])
    _margins.check("rowll_grouped_padding", _rel(outs[1], ref), TOL, "free_energy")


def test_grouped_row_loglik_on_a_saturated_layer(hip_engine):
    """|pre| in the tens and beyond (the bias ladder of tests/_saturated.py) and one row whose group of 64 across column 128
    holds pre-activations at +80 and -80 alternately: every value finite, and still the float64 formula's."""
    eng = hip_engine
    V, H, R, div, bounds = BIG
    rs = np.random.RandomState(21)
    W, _, vb = _saturated.params(rs, V, H, gauss=False)
    h, _, _, target = Gb.kernel_case(V, H, R, div, bounds)
    # hidden unit 0 is on in row 0 alone, where nothing else is: its weights set that row's pre-activations
    h[:, 0] = 0.0
    h[0, :] = 0.0
    h[0, 0] = 1.0
    W = W.copy()
    W[66:130, 0] = np.where(np.arange(64) % 2 == 0, 80.0, -80.0).astype(np.float32) - vb[66:130]
    pre = h.astype(np.float64) @ W.astype(np.float64).T + vb
    assert np.abs(np.abs(pre[0, 66:130]) - 80.0).max() < 1e-4
    _saturated.assert_bands("rowll_grouped", [pre], bands=_saturated.REGIMES)
    ref = Gb.kernel_reference(h, W, vb, target, div, bounds)
    got = eng.to_numpy(eng.propdown_row_loglik_grouped(eng.to_device(h), eng.to_device(W), eng.to_device(vb), eng.to_device(target),
                                                       _table(eng, bounds), div))
    assert np.isfinite(got).all()
    print("grouped rowll saturated: worst %.3e of %.1e" % (_rel(got, ref), TOL))
    _margins.check("rowll_grouped_saturated", _rel(got, ref), TOL, "free_energy")


def test_refused_calls_leave_out_untouched(hip_engine):
    """Every MDBN_EINVAL case of mdbn_propdown_rowll_grouped: a message, no launch, ``out`` as it was."""
    import torch
    from mdbn_amd import _lib
    eng = hip_engine
    V, H, R, div = 300, 200, 70, 7
    good = BIG[4]
    h, W, vb, target = Gb.kernel_case(V, H, R, div, good)

    def call(bounds=good, n_groups=None, ld=208, short=0):
        dh, dW, dt = _matrix(eng, h, ld, 0.0), _matrix(eng, W, ld, 0.0), eng.to_device(target)
        dvb = eng.to_device(vb)
        n = C.c_int64()
        _lib.check(eng.lib.mdbn_rowll_grouped_workspace_bytes(eng.ctx, R, V, H, C.byref(n)), "mdbn_rowll_grouped_workspace_bytes")
        ws = torch.empty(n.value // 4 + 64, dtype=torch.float32, device=eng.device)
        out = torch.full((R,), 7.0, dtype=torch.float32, device=eng.device)
        host_t = np.ascontiguousarray(bounds, dtype=np.int32)
        dev_t = torch.from_numpy(host_t.copy()).to(eng.device)
        rc = eng.lib.mdbn_propdown_rowll_grouped(
            eng.ctx, eng._stream(), eng._p(dh), R, dh.stride(0), eng._p(dW), V, H, eng._p(dvb), eng._p(dt), dt.stride(0), div,
            eng._p(out), eng._p(ws), n.value - short if short else ws.numel() * 4, eng._p(dev_t), C.c_void_p(host_t.ctypes.data),
            host_t.size - 1 if n_groups is None else n_groups)
        eng.synchronize()
        return rc, _lib.last_error(), bool((out == 7.0).all())

    rc, _, untouched = call()
    assert rc == 0 and not untouched
    for what, kw in (("n_groups = 0", dict(n_groups=0)),
                     ("a descending table", dict(bounds=[2, 66, 40, 104])),
                     ("a group of 65 columns", dict(bounds=[2, 67, 130])),
                     ("a boundary beyond V", dict(bounds=[250, 301])),
                     ("ldh % 4 != 0", dict(ld=202)),
                     ("a short workspace", dict(short=4))):
        rc, msg, untouched = call(**kw)
        assert rc == -1 and msg and untouched, (what, rc, msg, untouched)


# ------------------------------------------------------------------ end to end
def _build(layers, eng):
    import mdbn_amd
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


def _dbn_case():
    """12 -> 6 -> 4 with four groups of 3, nine rows."""
    bounds = [0, 3, 6, 9, 12]
    rs = np.random.RandomState(41)
    model = dict(bottoms=[Gb.make_net(rs, (12, 6, 4), 1.0, 5001, bounds)], joint=None)
    return model, [sm.one_hot_data(rs, 9, 12, bounds)]


@pytest.fixture(scope="module")
def truth():
    out = {}
    model, inputs = _dbn_case()
    out["dbn"] = (model, inputs) + Gb.brute_force(model, inputs)
    for scale in (0.5, 1.5):
        model, inputs = Gb.stacks(scale)["forest"]
        out["forest", scale] = (model, inputs) + Gb.brute_force(model, inputs)
    return out


def _trace_samples(record):
    return [net["samples"] for net in record.trace["nets"]]


def test_dbn_bound_with_groups_meets_the_twin_and_the_exact_bound(hip_engine, truth):
    import mdbn_amd
    model, inputs, log_p, exact, log_z = truth["dbn"]
    net = _build(model["bottoms"][0], hip_engine)
    r = net.log_likelihood_bound(inputs[0], n_samples=S, log_z=log_z, trace=True)
    assert [x._rng_step for x in net.rbm_layers] == [1, 0] and r.rows.shape == (9,)
    forced = Gb.estimate(model, inputs, S, log_z, samples=_trace_samples(r))
    print("dbn rows: worst %.3e of %.1e" % (_rel(r.rows, forced["rows"]), TOL))
    _margins.check("gbound_rows_teacher_forced", _rel(r.rows, forced["rows"]), TOL, "free_energy")
    _margins.check("gbound_values_teacher_forced", _rel(r.trace["values"], forced["values"]), TOL, "free_energy")
    free = Gb.estimate(model, inputs, S, log_z)
    differ = r.trace["nets"][0]["samples"][0] != free["samples"][0][0]
    assert (np.abs(free["uniforms"][0][0] - free["means"][0][0])[differ] < 4e-6).all() and differ.mean() <= 1e-3
    assert r.stderr > 0 and abs(r.bound - exact.mean()) <= 4 * r.stderr, (r.bound, exact.mean(), r.stderr)
    assert r.bound <= log_p.mean() + 4 * r.stderr
    # three data rows per chunk: the same draws, the same bits
    cut = _build(model["bottoms"][0], hip_engine).log_likelihood_bound(inputs[0], n_samples=S, log_z=log_z, chunk_rows=3 * S, trace=True)
    assert np.array_equal(cut.trace["nets"][0]["samples"][0], r.trace["nets"][0]["samples"][0]), "a chunk changed a draw"
    assert np.array_equal(cut.trace["nets"][0]["directed"][0], r.trace["nets"][0]["directed"][0]), "a chunk changed a directed term"
    assert np.array_equal(cut.rows, r.rows)
    # a host-resident table streams to the same bits
    table = mdbn_amd.shared(inputs[0], engine=hip_engine, resident="host")
    got = _build(model["bottoms"][0], hip_engine).log_likelihood_bound(table, n_samples=S, log_z=log_z, trace=True)
    assert table._mirror is None, "the table was uploaded whole"
    assert np.array_equal(got.trace["nets"][0]["directed"][0], r.trace["nets"][0]["directed"][0])
    assert np.array_equal(got.rows, r.rows)


@pytest.mark.parametrize("scale", (0.5, 1.5))
def test_forest_with_a_grouped_modality_meets_its_twin(hip_engine, truth, scale):
    import mdbn_amd
    model, inputs, _, exact, log_z = truth["forest", scale]
    nets = [_build(layers, hip_engine) for layers in model["bottoms"]]
    joint = _build(model["joint"], hip_engine)
    r = mdbn_amd.log_likelihood_bound(nets, joint, {0: inputs[0], 1: inputs[1]}, n_samples=S, log_z=log_z, trace=True)
    assert [x._rng_step for n in nets for x in n.rbm_layers] == [1, 1] and [x._rng_step for x in joint.rbm_layers] == [1, 0]
    forced = Gb.estimate(model, inputs, S, log_z, samples=_trace_samples(r))
    _margins.check("gstack_rows_teacher_forced", _rel(r.rows, forced["rows"]), TOL, "free_energy")
    _margins.check("gstack_modality_rows", _rel(r.modality_rows, forced["modality_rows"]), TOL, "free_energy")
    _margins.check("gstack_joint_rows", _rel(r.joint_rows, forced["joint_rows"]), TOL, "free_energy")
    assert np.abs(r.modality_rows.sum(axis=0) + r.joint_rows - r.rows).max() <= 1e-9 * max(1.0, np.abs(r.rows).max())
    assert r.stderr > 0 and abs(r.bound - exact.mean()) <= 4 * r.stderr, (r.bound, exact.mean(), r.stderr)
    nets2 = [_build(layers, hip_engine) for layers in model["bottoms"]]
    cut = mdbn_amd.log_likelihood_bound(nets2, _build(model["joint"], hip_engine), inputs, n_samples=S, log_z=log_z, chunk_rows=3 * S)
    assert np.array_equal(cut.rows, r.rows) and np.array_equal(cut.modality_rows, r.modality_rows)


def test_one_layer_network_with_groups_is_log_likelihood(hip_engine):
    rs = np.random.RandomState(5)
    bounds = [0, 3, 6, 8]
    layers = Gb.make_net(rs, (10, 4), 1.0, 77, bounds)
    x = sm.one_hot_data(rs, 5, 10, bounds, p=0.5)
    net = _build(layers, hip_engine)
    want, err = net.rbm_layers[0].log_likelihood(x, n_chains=64, n_betas=100)
    used = net.rbm_layers[0]._rng_step
    net.rbm_layers[0]._rng_step = 0
    r = net.log_likelihood_bound(x, n_chains=64, n_betas=100)
    assert net.rbm_layers[0]._rng_step == used, "only the AIS run of log Z consumes random numbers"
    assert abs(r.bound - want) <= 1e-6 * max(1.0, abs(want)) and r.log_z_stderr == err and r.stderr == 0.0
    exact = -T.free_energy(x, T.f64(layers[0])) - r.log_z
    _margins.check("gbound_one_layer_rows", _rel(r.rows, exact), TOL, "free_energy")
