"""Parallel tempering of a layer with categorical visible units above the kernels (no GPU): the C-ABI's declaration and the
argument rules of mdbn_pt_run_grouped, answered on the host before any launch, and the public classes on a checker engine whose
``temper_grouped`` is the float64 twin (tests/_gtemper_np.py): what reaches the engine, with which table and which base
model, and what stays refused."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import _gais_np as G
import _gtemper_np as GT
import _softmax_np as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mdbn_pt_run_grouped"
MDBN_EINVAL = -1
V0, H0, BOUNDS0 = 12, 7, [2, 5, 8, 10]     # the (3, 3, 2) + 2 + 2 Bernoulli layer of tests/test_softmax_api.py
GOOD = np.arange(0, 101, 5, dtype=np.int32)


@pytest.fixture(scope="module")
def lib(built_lib):
    from mdbn_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------- the C-ABI, on the host
def test_declared_exported_and_bound(lib):
    from mdbn_amd import _lib
    import mdbn_amd
    header = open(os.path.join(ROOT, "include", "mdbn_hip.h")).read()
    assert re.search(r"^int\s+%s\(" % NAME, header, re.M), "%s is not declared in include/mdbn_hip.h" % NAME
    assert NAME in _lib.SIGNATURES, "%s has no ctypes signature" % NAME
    assert hasattr(lib, NAME), "%s is not exported by the library" % NAME
    decl = header[header.index(NAME + "("):]
    sig = _lib.SIGNATURES[NAME]
    assert len(sig) == decl[:decl.index(");")].count(",") + 1
    # the arguments of mdbn_pt_run_z, then the table in its two copies and n_groups
    assert sig[:-3] == _lib.SIGNATURES["mdbn_pt_run_z"] and sig[-3:] == _lib.SIGNATURES["mdbn_ais_run_grouped"][-3:]
    comment = header[:header.index("int  " + NAME + "(")]
    comment = comment[comment.rindex("/*"):]
    for words in ("softmax_c(x_c)", "FIRST column", "rng->step + 3t", "log Z_A = H log 2", "logsumexp"):
        assert words in comment, words
    assert list(inspect.signature(mdbn_amd.HipEngine.temper_grouped).parameters) == [
        "self", "W", "hbias", "vbias", "base_vbias", "betas", "v", "h", "rank", "n_sweeps", "rng", "groups", "burn_in", "sweep0",
        "path", "steps_per_launch", "trace", "zacc", "trace_work"]


def _bytes(lib, M, R, V, H, path=0):
    n = C.c_int64(-1)
    return lib.mdbn_pt_run_z_workspace_bytes(None, M, R, V, H, path, C.byref(n)), n.value


def _run(lib, M=64, R=16, V=100, H=24, n=8, burn_in=0, path=0, spl=0, ws_bytes=0, ldv=None, ldh=None, gauss=0, betas=None, sweep0=0,
         table=GOOD, dev=True, host=True):
    # (NULL pointers throughout: every rule below is answered before a pointer is looked at, let alone a kernel launched; the
    # device copy of the table is never read on the host, so any non-NULL address stands for it)
    if betas is None:
        betas = np.linspace(0, 1, R)
    betas = np.ascontiguousarray(betas, dtype=np.float32)
    t = None if table is None else table.ctypes.data
    return lib.mdbn_pt_run_grouped(None, None, None, V, H, H if ldh is None else ldh, None, None, None, gauss,
                                   betas.ctypes.data_as(C.c_void_p), R, M, V if ldv is None else ldv, None, None, None,
                                   n, burn_in, sweep0, None, None, None, None, None, None, path, spl, None, None, ws_bytes, None, None,
                                   t if dev else None, t if host else None, 0 if table is None else table.size - 1)


def test_run_refuses_gauss_and_a_bad_table_without_a_launch(lib):
    from mdbn_amd import _lib
    assert _run(lib, gauss=1) == MDBN_EINVAL and "Gaussian" in _lib.last_error()
    for what, table in (("not ascending", [0, 10, 5]), ("a group of 1 column", [0, 1]), ("a group of 65 columns", [0, 65]),
                        ("a boundary beyond V", [90, 101])):
        assert _run(lib, table=np.array(table, dtype=np.int32)) == MDBN_EINVAL and "group" in _lib.last_error(), what
    assert _run(lib, host=False) == MDBN_EINVAL and "group_start" in _lib.last_error()
    assert _run(lib, dev=False) == MDBN_EINVAL and "group_start" in _lib.last_error()


def test_run_refuses_what_the_plain_run_refuses(lib):
    from mdbn_amd import _lib
    assert _run(lib, M=0) == MDBN_EINVAL and "bad shape" in _lib.last_error()
    assert _run(lib, R=1, betas=[1.0]) == MDBN_EINVAL and "R = 1" in _lib.last_error()
    assert _run(lib, R=4, betas=[0.0, 0.5, 0.4, 1.0]) == MDBN_EINVAL and "rise strictly" in _lib.last_error()
    assert _run(lib, R=4, betas=[0.0, 0.3, 0.6, 0.9]) == MDBN_EINVAL and "exactly 1" in _lib.last_error()
    assert _run(lib, n=0) == MDBN_EINVAL and "n_sweeps" in _lib.last_error()
    assert _run(lib, burn_in=8) == MDBN_EINVAL and "burn_in" in _lib.last_error()
    assert _run(lib, sweep0=-1) == MDBN_EINVAL and "sweep0" in _lib.last_error()
    assert _run(lib, path=7) == MDBN_EINVAL and "path" in _lib.last_error()
    assert _run(lib, spl=-1) == MDBN_EINVAL and "steps_per_launch" in _lib.last_error()
    assert _run(lib, V=1024, H=256, path=1, table=np.arange(0, 1025, 4, dtype=np.int32)) == MDBN_EINVAL and "LDS-resident" in _lib.last_error()
    assert _run(lib, R=6, path=1) == MDBN_EINVAL and "multiple of 4" in _lib.last_error()
    assert _run(lib, ldv=102) == MDBN_EINVAL and "leading" in _lib.last_error()
    for path in (0, 1, 2):
        for table in (GOOD, None):                       # (n_groups = 0: no table read)
            rc, need = _bytes(lib, 64, 16, 100, 24, path=path)
            assert rc == 0
            assert _run(lib, path=path, ws_bytes=need - 4, table=table) == MDBN_EINVAL and "mdbn_pt_run_z_workspace_bytes" in _lib.last_error()
            # enough workspace: the next rule in line is the NULL context
            assert _run(lib, path=path, ws_bytes=need, table=table) == MDBN_EINVAL and "NULL" in _lib.last_error()


# ---------------------------------------------------------------------------------- the public classes on the checker engine
def _layer(eng, V=V0, H=H0, bounds=BOUNDS0, seed=11):
    import mdbn_amd
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(5), theano_rng=mdbn_amd.RandomStreams(seed),
                       engine=eng, visible_groups=bounds)
    rs = np.random.RandomState(3)
    rbm.W.set_value(rs.normal(0, 0.4, (V, H)).astype(np.float32))
    rbm.hbias.set_value(rs.normal(0, 0.5, H).astype(np.float32))
    rbm.vbias.set_value(rs.normal(0, 0.5, V).astype(np.float32))
    return rbm


def _params(rbm):
    return rbm.W.get_value(), rbm.hbias.get_value(), rbm.vbias.get_value()


def test_tempered_chains_reach_the_grouped_call():
    eng = GT.GtemperOracle()
    rbm = _layer(eng)
    bA = np.random.RandomState(8).normal(0, 0.3, V0).astype(np.float32)
    M, R, n = 3, 4, 6
    rbm._rng_step = 9
    chains = rbm.tempered_chains(M, n_betas=R, base_vbias=bA)
    v_avg, h_avg, acceptance = chains.run(n, burn_in=2)
    assert rbm._rng_step == 9 + 3 * n and chains.n_done == n
    (call,) = eng.temper_calls
    assert call["bounds"] == BOUNDS0 and call["n"] == n and call["burn_in"] == 2 and call["step"] == 9 and call["sweep0"] == 0
    np.testing.assert_array_equal(call["base_vbias"], bA.astype(np.float64))
    W, c, b = _params(rbm)
    tw = GT.pt_twin(W, c, b, bA, BOUNDS0, np.linspace(0, 1, R), np.zeros((M * R, H0)), n, 2, rbm.theano_rng.seed, rbm.stream_id, 9)
    np.testing.assert_array_equal(chains.v.numpy(), tw["v"])
    np.testing.assert_array_equal(chains.rank.numpy(), tw["rank"])
    np.testing.assert_allclose(v_avg.get_value(), tw["v_avg"], rtol=0, atol=1e-6)
    for lo, hi in sm.spans(BOUNDS0):
        assert (chains.v.numpy()[:, lo:hi].sum(axis=1) == 1).all()
        np.testing.assert_allclose(v_avg.get_value()[:, lo:hi].sum(axis=1), 1.0, atol=1e-5)      # softmax means, not sigmoids
    # a second run continues: the parity and the RNG step move on
    chains.run(3)
    assert eng.temper_calls[1]["sweep0"] == n and eng.temper_calls[1]["step"] == 9 + 3 * n
    # sample_tempered
    eng.temper_calls.clear()
    v, h, v_avg, h_avg, acceptance = rbm.sample_tempered(4, n_sweeps=6, burn_in=2, n_betas=4, base_vbias=bA)
    assert len(eng.temper_calls) == 1 and eng.temper_calls[0]["bounds"] == BOUNDS0
    assert v.shape == (4, V0) and all((v[:, lo:hi].sum(axis=1) == 1).all() for lo, hi in sm.spans(BOUNDS0))


def test_log_partition_by_tempering_starts_from_the_grouped_base_model():
    eng = GT.GtemperOracle()
    rbm = _layer(eng)
    W, c, b = _params(rbm)
    exact = G.brute_log_Z(W, c, b, BOUNDS0)
    data = sm.one_hot_data(np.random.RandomState(0), 40, V0, BOUNDS0)
    bA = rbm.base_rate_vbias(data)
    kw = dict(n_ladders=16, n_sweeps=200, burn_in=40)
    r = rbm.tempered_chains(16, n_betas=8, base_vbias=bA).log_partition(200, 40)
    z0 = G.log_Z_base(bA, H0, BOUNDS0)
    assert abs(r.log_z_fwd - (z0 + r.ratios_fwd.sum())) <= 1e-12 and abs(r.log_z_rev - (z0 + r.ratios_rev.sum())) <= 1e-12
    assert eng.temper_calls[-1]["zacc"] and eng.temper_calls[-1]["bounds"] == BOUNDS0
    print("gtemper checker 12->7: log Z^ %.4f +- %.4f (bracket %.4f .. %.4f), exact %.4f" % (r.log_z, r.stderr, r.log_z_fwd, r.log_z_rev, exact))
    assert r.stderr > 0 and abs(r.log_z - exact) <= max(4 * r.stderr, 0.05)
    step = rbm._rng_step
    lz, se = rbm.log_partition(method="tempering", n_betas=8, data=data, **kw)
    assert rbm._rng_step == step + 600 and abs(lz - exact) <= max(4 * se, 0.05)
    np.testing.assert_array_equal(eng.temper_calls[-1]["base_vbias"], bA.astype(np.float64))
    ll, se2 = rbm.log_likelihood(data, method="tempering", n_betas=8, **kw)
    neg_F = -np.asarray(rbm.free_energy(data).get_value(), dtype=np.float64)
    assert se2 > 0 and abs(ll - (neg_F.mean() - exact)) <= max(4 * se2, 0.05)
    # check_log_partition: grouped AIS and the grouped ladder from ONE base-rate model
    eng.temper_calls.clear()
    out = rbm.check_log_partition(data=data, n_chains=64, n_betas=200, n_ladder_betas=8, **kw)
    assert set(out) == {"ais", "ais_stderr", "tempering", "tempering_stderr", "bracket", "z", "detail"} and np.isfinite(out["z"])
    np.testing.assert_array_equal(eng.temper_calls[0]["base_vbias"], bA.astype(np.float64))
    assert abs(out["ais"] - exact) <= 0.1 and abs(out["tempering"] - exact) <= 0.1


def test_training_with_tempering_reaches_the_grouped_call():
    eng = GT.GtemperOracle()
    rbm = _layer(eng)
    data = sm.one_hot_data(np.random.RandomState(0), 30, V0, BOUNDS0)
    np.random.seed(3)
    import mdbn_amd
    mdbn_amd.RBM.training(rbm, data, None, training_epochs=1, batch_size=10, learning_rate=0.05, persistent=True, tempering=4)
    assert len(eng.temper_calls) == 3 and all(c["n"] == 1 and c["bounds"] == BOUNDS0 for c in eng.temper_calls)
    assert [c["sweep0"] for c in eng.temper_calls] == [0, 1, 2] and rbm.tempered.n_done == 3
    for lo, hi in sm.spans(BOUNDS0):
        assert (rbm.tempered.v.numpy()[:, lo:hi].sum(axis=1) == 1).all()


def test_what_stays_refused():
    import mdbn_amd
    data = sm.one_hot_data(np.random.RandomState(0), 10, V0, BOUNDS0)
    for eng in (sm.GroupedOracle(), G.GaisOracle()):                  # engines without temper_grouped
        assert not hasattr(eng, "temper_grouped")
        rbm = _layer(eng)
        for call in (lambda: rbm.tempered_chains(2), lambda: rbm.sample_tempered(2, n_sweeps=2, burn_in=0),
                     lambda: rbm.log_partition(method="tempering"), lambda: rbm.log_likelihood(data, method="tempering"),
                     lambda: rbm.check_log_partition(), lambda: rbm.training(data, None, 1, batch_size=10, tempering=3)):
            with pytest.raises(NotImplementedError, match="visible_groups"):
                call()
        assert rbm._rng_step == 0
    eng = GT.GtemperOracle()
    with pytest.raises(ValueError, match="Gaussian"):
        mdbn_amd.GRBM(n_visible=V0, n_hidden=H0, numpy_rng=np.random.RandomState(5), engine=eng, visible_groups=BOUNDS0)
    grbm = mdbn_amd.GRBM(n_visible=V0, n_hidden=H0, numpy_rng=np.random.RandomState(5), engine=eng)
    with pytest.raises(ValueError, match="Gaussian"):
        grbm.set_visible_groups(BOUNDS0)
    grbm.set_sigma(np.full(V0, 1.5, dtype=np.float32))
    for call in (lambda: grbm.tempered_chains(2), lambda: grbm.check_log_partition(), lambda: grbm.log_partition(method="tempering")):
        with pytest.raises(NotImplementedError, match="log_sigma"):
            call()
    # the bound and fine-tuning of a network whose input layer has groups
    mdbn_amd.DBN.verbose = False
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V0, gauss=False, hidden_layers_sizes=[H0], n_outs=4, engine=eng,
                       visible_groups=BOUNDS0)
    with pytest.raises(NotImplementedError, match="visible_groups"):
        net.log_likelihood_bound(data[:4], n_samples=2)
    with pytest.raises(NotImplementedError, match="visible_groups"):
        net.fine_tune(data, 1, batch_size=10, lr=0.01)
    assert not eng.temper_calls
