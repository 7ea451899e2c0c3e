"""Clamped Gibbs sampling above the kernels (no GPU): the Python surface through the CPU checker engine
(tests/_oracle_engine.py: RBM.gibbs_vhv_clamped composes the eager sample_* calls there -- the CPU statement of the
semantics), and the C-ABI's declarations and argument rules, answered on the host before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _clamp_np as Cn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mdbn_gibbs_clamped_workspace_bytes", "mdbn_gibbs_clamped")
MDBN_EINVAL = -1


def _layer(eng, V, H, gauss, seed=7, error_free=True):
    import mdbn_amd
    kw = dict(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(seed), engine=eng)
    rbm = mdbn_amd.GRBM(error_free=error_free, **kw) if gauss else mdbn_amd.RBM(**kw)
    rs = np.random.RandomState(3)
    rbm.W.set_value(rs.normal(0, 0.3, (V, H)).astype(np.float32))
    rbm.hbias.set_value(rs.normal(0, 0.5, H).astype(np.float32))
    rbm.vbias.set_value(rs.normal(0, 0.5, V).astype(np.float32))
    return rbm


def _data(V, gauss, B=12):
    rs = np.random.RandomState(5)
    return rs.normal(size=(B, V)).astype(np.float32) if gauss else (rs.uniform(size=(B, V)) < 0.4).astype(np.float32)


@pytest.mark.parametrize("gauss,error_free", [(False, True), (True, True), (True, False)])
def test_no_mask_is_the_free_chain(oracle_engine, gauss, error_free):
    V, H, n = 30, 12, 5
    one, two = _layer(oracle_engine, V, H, gauss, error_free=error_free), _layer(oracle_engine, V, H, gauss, error_free=error_free)
    x = _data(V, gauss)
    got = one.gibbs_vhv_clamped(x, np.zeros((1, V)), n)
    want = two.gibbs_vhv_chain(x, n)
    assert len(got) == 8 and one._rng_step == two._rng_step == 2 * n
    for g, w in zip(got[:6], want):
        np.testing.assert_array_equal(g.get_value(), w.get_value())
    # burn_in = 0: the averages hold at least the last step's means
    assert got[6].shape == (12, V) and got[7].shape == (12, H)


@pytest.mark.parametrize("gauss", [False, True])
def test_full_mask_never_moves(oracle_engine, gauss):
    V, H, n = 30, 12, 4
    rbm = _layer(oracle_engine, V, H, gauss)
    x = _data(V, gauss)
    out = rbm.gibbs_vhv_clamped(x, np.ones(V), n, burn_in=2, trace=True)         # (two accumulated steps: x + x and / 2 are exact)
    assert rbm._rng_step == 2 * n and len(out) == 10
    np.testing.assert_array_equal(out[5].get_value(), x)
    np.testing.assert_array_equal(out[4].get_value(), x)
    np.testing.assert_array_equal(out[6].get_value(), x)
    for t in range(n):
        np.testing.assert_array_equal(out[9].get_value()[t], x)
    want = Cn.sigmoid(x.astype(np.float64) @ rbm.W.get_value().astype(np.float64) + rbm.hbias.get_value())
    np.testing.assert_allclose(out[1].get_value(), want, rtol=0, atol=1e-6)
    np.testing.assert_allclose(out[7].get_value(), want, rtol=0, atol=1e-6)


@pytest.mark.parametrize("gauss,error_free,sampler", [(False, True, False), (True, True, False), (True, False, False), (True, True, True),
                                                      (False, True, True)])
def test_checker_engine_equals_the_twin(oracle_engine, gauss, error_free, sampler):
    """The eager composition and tests/_clamp_np.py are two statements of the same semantics: same samples, same means."""
    V, H, n, burn = 30, 12, 6, 2
    rbm = _layer(oracle_engine, V, H, gauss, error_free=error_free)
    x = _data(V, gauss)
    mask = Cn.half_mask(V, rows=12)
    rbm._rng_step = 9
    out = rbm.gibbs_vhv_clamped(x, mask, n, burn_in=burn, trace=True, sampler=sampler)
    tw = Cn.clamp_twin(rbm.W.get_value(), rbm.hbias.get_value(), rbm.vbias.get_value(), gauss, x, x, mask, n, burn,
                       rbm.theano_rng.seed, rbm.stream_id, 9, add_noise=not error_free, sampler=sampler)
    assert rbm._rng_step == 9 + 2 * n
    np.testing.assert_array_equal(out[8].get_value(), tw["trace_h"])
    for got, name in ((out[1], "h_mean"), (out[4], "v_mean"), (out[5], "v"), (out[6], "v_avg"), (out[7], "h_avg")):
        np.testing.assert_allclose(got.get_value(), tw[name], rtol=0, atol=2e-6, err_msg=name)
    held = mask != 0
    np.testing.assert_array_equal(out[5].get_value()[held], x[held])


def test_bad_arguments(oracle_engine):
    rbm = _layer(oracle_engine, 10, 4, False)
    x = _data(10, False)
    for n, burn in ((0, 0), (3, 3), (3, -1)):
        with pytest.raises(ValueError):
            rbm.gibbs_vhv_clamped(x, np.ones(10), n, burn_in=burn)
    with pytest.raises(ValueError):
        rbm.gibbs_vhv_clamped(x, np.ones((5, 10)), 3)
    assert rbm._rng_step == 0


def test_impute_shapes_chains_and_observed_entries(oracle_engine):
    V, H, N = 20, 8, 6
    rbm = _layer(oracle_engine, V, H, False)
    x = _data(V, False, B=N)
    mask = Cn.half_mask(V, rows=N)
    x_nan = np.where(mask != 0, x, np.nan).astype(np.float32)         # unobserved entries are never read
    v_hat, h_hat = rbm.impute(x_nan, mask, n_steps=12, burn_in=4, n_chains=3)
    assert v_hat.shape == (N, V) and h_hat.shape == (N, H) and rbm._rng_step == 24
    assert np.isfinite(v_hat).all() and np.isfinite(h_hat).all()
    np.testing.assert_array_equal(v_hat[mask != 0], x[mask != 0])
    assert ((v_hat > 0) & (v_hat < 1))[mask == 0].all()
    # the chains of a row are consecutive Philox rows of one clamped run from the model's base
    base = Cn.sigmoid(rbm.vbias.get_value().astype(np.float64))
    start = np.repeat(np.where(mask != 0, x, base[None]), 3, axis=0)
    tw = Cn.clamp_twin(rbm.W.get_value(), rbm.hbias.get_value(), rbm.vbias.get_value(), False, start, start,
                       np.repeat(mask, 3, axis=0), 12, 4, rbm.theano_rng.seed, rbm.stream_id, 0)
    np.testing.assert_allclose(v_hat, tw["v_avg"].reshape(N, 3, V).mean(axis=1), rtol=0, atol=2e-6)
    np.testing.assert_allclose(h_hat, tw["h_avg"].reshape(N, 3, H).mean(axis=1), rtol=0, atol=2e-6)


def _tiny_mdbn(eng):
    import mdbn_amd
    rng = np.random.RandomState(2)
    nets = [mdbn_amd.DBN(numpy_rng=rng, n_ins=n, hidden_layers_sizes=hid, n_outs=top, engine=eng)
            for n, hid, top in ((14, [9], 5), (10, [], 4), (8, [6], 3))]
    joint = mdbn_amd.DBN(numpy_rng=rng, n_ins=12, gauss=False, hidden_layers_sizes=[7], n_outs=3, engine=eng)
    return nets, joint


def test_down_pass_leaves_every_rng_counter(oracle_engine):
    nets, _ = _tiny_mdbn(oracle_engine)
    x = np.random.RandomState(1).normal(size=(5, 14)).astype(np.float32)
    net = nets[0]
    for r in net.rbm_layers:
        r._rng_step = 17
    back = net.down_pass(net.get_output(x))
    assert back.shape == (5, 14) and np.isfinite(back).all()
    assert [r._rng_step for r in net.rbm_layers] == [17, 17]
    mid = net.down_pass(net.get_output(x, 0), layer=0)
    assert mid.shape == (5, 14)
    # a Gaussian bottom layer gives the linear mean, the layers above it sigmoid means
    top = net.get_output(x).astype(np.float64)
    r1, r0 = net.rbm_layers[1], net.rbm_layers[0]
    h0 = Cn.sigmoid(top @ r1.W.get_value().astype(np.float64).T + r1.vbias.get_value())
    want = h0 @ r0.W.get_value().astype(np.float64).T + r0.vbias.get_value()
    np.testing.assert_allclose(back, want, rtol=0, atol=1e-5)
    assert net.down_pass(None) is None


def test_impute_modalities_block_masks(oracle_engine):
    nets, joint = _tiny_mdbn(oracle_engine)
    rs = np.random.RandomState(4)
    N = 6
    xs = [rs.normal(size=(N, n)).astype(np.float32) for n in (14, 10, 8)]
    import mdbn_amd
    # one modality missing for everybody
    jv, jt, imp = mdbn_amd.MDBN.impute_modalities(nets, joint, [xs[0], None, xs[2]], n_steps=10, burn_in=2, n_chains=2)
    assert jv.shape == (N, 12) and jt.shape == (N, 3) and sorted(imp) == [1] and imp[1].shape == (N, 10)
    np.testing.assert_allclose(jv[:, :5], nets[0].get_output(xs[0]), rtol=0, atol=1e-6)
    np.testing.assert_allclose(jv[:, 9:], nets[2].get_output(xs[2]), rtol=0, atol=1e-6)
    assert ((jv[:, 5:9] > 0) & (jv[:, 5:9] < 1)).all()
    # a different modality missing per row (rows of NaN)
    ys = [x.copy() for x in xs]
    ys[0][0] = np.nan
    ys[1][1] = np.nan
    ys[2][2] = np.nan
    ys[2][0] = np.nan
    jv, jt, imp = mdbn_amd.MDBN.impute_modalities(nets, joint, ys, n_steps=10, burn_in=2, n_chains=2)
    assert sorted(imp) == [0, 1, 2] and [imp[i].shape for i in range(3)] == [(N, 14), (N, 10), (N, 8)]
    assert np.isfinite(jv).all() and np.isfinite(jt).all() and all(np.isfinite(v).all() for v in imp.values())
    np.testing.assert_allclose(jv[3:], np.concatenate([n.get_output(x[3:]) for n, x in zip(nets, xs)], axis=1), rtol=0, atol=1e-6)
    np.testing.assert_allclose(jv[1, :5], nets[0].get_output(xs[0])[1], rtol=0, atol=1e-6)
    with pytest.raises(ValueError):
        mdbn_amd.MDBN.impute_modalities(nets, joint, [None, None, None])


def test_end_to_end_imputation_beats_the_training_mean(oracle_engine):
    """tests/_clamp_e2e.py on the CPU checker engine: a three-modality MDBN (2048->400->40, 512->40, 256->200->20, joint 100->128->3)
    trained for 10 epochs on 192 synthetic patients with a planted class; for the 64 held-out patients the miRNA table is
    withheld and ``impute_modalities`` must put its joint block closer (mean squared error) to the block the withheld data gives
    than the block's training mean is.  Strictly better is all that is claimed (measured here: 0.0970 against 0.1956).  The same
    run, same seeds, is asked of the device in tests/test_gpu_clamp.py.  (The miRNA block is the one withheld because it is the
    informative one of these tables: the mutation block of so short a training barely moves, 6e-5 either way.)"""
    import _clamp_e2e
    mse_imputed, mse_mean = _clamp_e2e.run()
    print("end to end (checker engine): imputed block MSE %.5f, training-mean MSE %.5f" % (mse_imputed, mse_mean))
    assert mse_imputed < mse_mean, (mse_imputed, mse_mean)


def test_partly_missing_row_is_refused(oracle_engine):
    import mdbn_amd
    nets, joint = _tiny_mdbn(oracle_engine)
    rs = np.random.RandomState(4)
    xs = [rs.normal(size=(6, n)).astype(np.float32) for n in (14, 10, 8)]
    xs[1][2, 3] = np.nan
    with pytest.raises(ValueError, match="partly"):
        mdbn_amd.MDBN.impute_modalities(nets, joint, xs, n_steps=4, burn_in=1, n_chains=1)


# ---------------------------------------------------------------------------------- the C-ABI, on the host
@pytest.fixture(scope="module")
def lib(built_lib):
    from mdbn_amd import _lib
    return _lib.load()


def test_declared_exported_and_bound(lib):
    from mdbn_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "mdbn_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int\s+%s\(" % name, header, re.M), "%s is not declared in include/mdbn_hip.h" % name
        assert name in _lib.SIGNATURES, "%s has no ctypes signature" % name
        assert hasattr(lib, name), "%s is not exported by the library" % name
        decl = header[header.index(name + "("):]
        assert len(_lib.SIGNATURES[name]) == decl[:decl.index(");")].count(",") + 1
    assert "mdbn_clamp.hip" in build.SOURCES and "mdbn_clamp.h" in build.HEADERS


def _bytes(lib, B, V, H, path=0):
    n = C.c_int64(-1)
    return lib.mdbn_gibbs_clamped_workspace_bytes(None, B, V, H, path, C.byref(n)), n.value


def test_workspace_bytes_rules(lib):
    from mdbn_amd import _lib
    assert _bytes(lib, 0, 100, 24)[0] == MDBN_EINVAL
    assert _bytes(lib, 64, 100, 24, path=3)[0] == MDBN_EINVAL
    assert _bytes(lib, 64, 4096, 1024, path=1)[0] == MDBN_EINVAL and "LDS-resident" in _lib.last_error()
    assert lib.mdbn_gibbs_clamped_workspace_bytes(None, 64, 100, 24, 0, None) == MDBN_EINVAL
    n = C.c_int64()
    for V, H in ((100, 24), (400, 40)):
        assert _bytes(lib, 170, V, H, path=0) == _bytes(lib, 170, V, H, path=1)
        assert lib.mdbn_workspace_bytes(170, V, H, C.byref(n)) == 0
        assert _bytes(lib, 170, V, H, path=1)[1] < n.value < _bytes(lib, 170, V, H, path=2)[1]
    assert _bytes(lib, 64, 1024, 256, path=0) == _bytes(lib, 64, 1024, 256, path=2)


def _run(lib, B=64, V=100, H=24, n_steps=8, burn_in=0, mask_rows=None, path=0, spl=0, ws_bytes=0, ldv=None, ldh=None, gauss=0):
    # (NULL pointers throughout: every rule below is answered before a pointer is looked at, let alone a kernel launched)
    return lib.mdbn_gibbs_clamped(None, None, None, None, None, B if mask_rows is None else mask_rows, B,
                                  V if ldv is None else ldv, None, V, H, H if ldh is None else ldh, None, None, gauss, 0,
                                  n_steps, burn_in, None, None, None, None, None, None, None, path, spl, None, None, ws_bytes)


def test_run_refuses_bad_arguments_without_a_launch(lib):
    from mdbn_amd import _lib
    assert _run(lib, B=0) == MDBN_EINVAL and "bad shape" in _lib.last_error()
    assert _run(lib, n_steps=0) == MDBN_EINVAL and "n_steps" in _lib.last_error()
    assert _run(lib, burn_in=8) == MDBN_EINVAL and "burn_in" in _lib.last_error()
    assert _run(lib, burn_in=-1) == MDBN_EINVAL and "burn_in" in _lib.last_error()
    assert _run(lib, mask_rows=2) == MDBN_EINVAL and "mask_rows" in _lib.last_error()
    assert _run(lib, path=7) == MDBN_EINVAL and "path" in _lib.last_error()
    assert _run(lib, gauss=3) == MDBN_EINVAL and "gauss" in _lib.last_error()
    assert _run(lib, gauss=-1) == MDBN_EINVAL and "gauss" in _lib.last_error()
    assert _run(lib, spl=-1) == MDBN_EINVAL and "steps_per_launch" in _lib.last_error()
    assert _run(lib, V=4096, H=1024, path=1) == MDBN_EINVAL and "LDS-resident" in _lib.last_error()
    assert _run(lib, ldv=102) == MDBN_EINVAL and "leading" in _lib.last_error()
    for path in (0, 1, 2):
        for mask_rows in (1, 64):
            rc, need = _bytes(lib, 64, 100, 24, path=path)
            assert rc == 0
            assert _run(lib, path=path, mask_rows=mask_rows, ws_bytes=need - 4) == MDBN_EINVAL and "workspace" in _lib.last_error()
            # enough workspace: the next rule in line is the NULL context
            assert _run(lib, path=path, mask_rows=mask_rows, ws_bytes=need) == MDBN_EINVAL and "NULL" in _lib.last_error()
