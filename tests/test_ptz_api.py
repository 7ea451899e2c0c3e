"""log Z from the tempering ladder above the kernels (no GPU): the Python surface through the CPU checker engine
(TemperedChains composes the sweep and the works from the engine's eager calls there) against the numpy twin, and the C-ABI's
declaration and argument rules of mdbn_pt_run_z, answered on the host before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _ais_np as A
import _ptz_np as Z
import _temper_np as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mdbn_pt_run_z_workspace_bytes", "mdbn_pt_run_z")
MDBN_EINVAL = -1


def _layer(eng, V, H, gauss, seed=7):
    import mdbn_amd
    kw = dict(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(seed), engine=eng)
    rbm = mdbn_amd.GRBM(**kw) if gauss else mdbn_amd.RBM(**kw)
    rs = np.random.RandomState(3)
    rbm.W.set_value(rs.normal(0, 0.3, (V, H)).astype(np.float32))
    rbm.hbias.set_value(rs.normal(0, 0.5, H).astype(np.float32))
    rbm.vbias.set_value(rs.normal(0, 0.5, V).astype(np.float32))
    return rbm


def _params(rbm):
    return rbm.W.get_value(), rbm.hbias.get_value(), rbm.vbias.get_value()


@pytest.fixture()
def ais_engine(oracle_engine):
    """The checker engine with an ``ais`` call answered by the AIS twin (the engine has none of its own)."""
    def ais(W, hbias, vbias, base_vbias, gauss, betas, n_chains, rng, path=0, trace=False):
        return A.ais_twin(W.numpy(), hbias.numpy(), vbias.numpy(), base_vbias, gauss, betas, n_chains, rng.seed, rng.stream_id,
                          rng.step)["logw"]
    oracle_engine.ais = ais
    yield oracle_engine
    del oracle_engine.ais


@pytest.mark.parametrize("gauss", [False, True])
def test_checker_engine_equals_the_twin(oracle_engine, gauss):
    """The works and accumulators of the eager composition against the twin's, from the eager composition's own trace."""
    import torch
    from mdbn_amd.temper import new_works
    V, H, M, R, n, burn = 30, 12, 5, 6, 9, 3
    rbm = _layer(oracle_engine, V, H, gauss)
    bA = np.random.RandomState(8).normal(0, 0.3, V).astype(np.float32)
    h0 = (np.random.RandomState(9).uniform(size=(M * R, H)) < 0.5).astype(np.float32)
    rbm._rng_step = 9
    chains = rbm.tempered_chains(M, n_betas=R, base_vbias=bA, start_h=h0)
    zacc, accepted, works = chains.accumulate_works(n, burn_in=burn, trace_work=True)
    assert rbm._rng_step == 9 + 3 * n and chains.n_done == n and works.shape == (n, M, R - 1, 2)
    W, c, b = _params(rbm)
    tw = T.pt_twin(W, c, b, bA, gauss, np.linspace(0, 1, R), h0, n, burn, rbm.theano_rng.seed, rbm.stream_id, 9)
    np.testing.assert_array_equal(accepted, tw["accepted"])
    np.testing.assert_array_equal(chains.rank.numpy(), tw["rank"])
    want = Z.works_from_trace(W, c, b, bA, gauss, np.linspace(0, 1, R), tw["trace_v"], tw["trace_swaps"])
    np.testing.assert_array_equal(np.isnan(works), np.isnan(want))
    np.testing.assert_array_equal(np.isnan(works[..., 0]), tw["trace_swaps"][:, :, 1, :-1] < 0)
    # (the two statements' Gaussian visible draws agree to 2e-6, test_temper_api.py; a work is linear in v with
    #  sum_i |d work / d v_i| <= db sum_i (sum_j |W_ij| + |v_i - b_i|), about 0.2 * 30 * 4 here: 5e-5)
    assert np.nanmax(np.abs(works - want)) <= (5e-5 if gauss else 1e-9)
    want_z = Z.accumulate(works[burn:])          # (torch's and numpy's float32 exp may differ by an ulp: the maxima are exact)
    np.testing.assert_array_equal(zacc.numpy()[..., 0::2], want_z[..., 0::2])
    np.testing.assert_allclose(zacc.numpy()[..., 1::2], want_z[..., 1::2], rtol=1e-6, atol=0)
    # a fresh accumulator is (-inf, 0)
    z0 = new_works(M, R)
    assert z0.shape == (M, R - 1, 4) and np.isneginf(z0[..., 0::2]).all() and (z0[..., 1::2] == 0).all()
    assert isinstance(zacc, torch.Tensor) and zacc.dtype == torch.float64


def test_run_is_unchanged_and_calls_accumulate(oracle_engine):
    """run() beside accumulate_works(): the same chains, means and acceptance; run(12) + run(8) accumulates what run(20) does."""
    V, H, M, R = 20, 8, 4, 6
    bA = np.random.RandomState(8).normal(0, 0.3, V).astype(np.float32)
    one, two, three = (_layer(oracle_engine, V, H, False) for _ in range(3))
    a = one.tempered_chains(M, n_betas=R, base_vbias=bA)
    plain = a.run(20, burn_in=3)
    assert len(plain) == 3
    b = two.tempered_chains(M, n_betas=R, base_vbias=bA)
    zacc, accepted, works = b.accumulate_works(20, burn_in=3)
    assert works is None
    np.testing.assert_array_equal(a.rank.numpy(), b.rank.numpy())
    np.testing.assert_array_equal(a.h.numpy(), b.h.numpy())
    np.testing.assert_array_equal(a.v.numpy(), b.v.numpy())
    from mdbn_amd.temper import attempts
    np.testing.assert_allclose(plain[2].get_value(), accepted / attempts(M, R, 0, 20), rtol=0, atol=1e-7)
    assert one._rng_step == two._rng_step == 60
    c = three.tempered_chains(M, n_betas=R, base_vbias=bA)
    z1, acc1, _ = c.accumulate_works(12, burn_in=3)
    z2, acc2, _ = c.accumulate_works(8, zacc=z1)
    assert z2 is z1 and c.n_done == 20
    np.testing.assert_array_equal(z2.numpy(), zacc.numpy())
    np.testing.assert_array_equal(acc1 + acc2, accepted)
    np.testing.assert_array_equal(c.h.numpy(), b.h.numpy())


@pytest.mark.parametrize("gauss", [False, True])
def test_log_partition_of_the_chains(oracle_engine, gauss):
    """TemperedChains.log_partition: the fields, the bracket, both methods, the attempts after burn-in; against brute force
    with the AIS criterion (a small layer: 12 -> 6)."""
    V, H, M, R, n, burn = 12, 6, 16, 8, 300, 60
    rbm = _layer(oracle_engine, V, H, gauss)
    W, c, b = _params(rbm)
    exact = A.brute_log_Z(W, c, b, gauss)
    bA = b if gauss else np.zeros(V, dtype=np.float32)
    from mdbn_amd.temper import attempts, LogZ
    for method in ("mid", "bar"):
        chains = rbm.tempered_chains(M, n_betas=R, base_vbias=bA)
        step = rbm._rng_step
        r = chains.log_partition(n, burn, method=method)
        assert isinstance(r, LogZ) and r.method == method and rbm._rng_step == step + 3 * n
        assert r.ratios_fwd.shape == r.ratios_rev.shape == r.acceptance.shape == r.attempts.shape == (R - 1,)
        np.testing.assert_array_equal(r.attempts, attempts(M, R, burn, n - burn))
        assert ((r.acceptance > 0) & (r.acceptance <= 1)).all()
        z0 = A.log_Z_base(bA, H, gauss)
        assert abs(r.log_z_fwd - (z0 + r.ratios_fwd.sum())) <= 1e-12 and abs(r.log_z_rev - (z0 + r.ratios_rev.sum())) <= 1e-12
        if method == "mid":
            assert abs(r.log_z - 0.5 * (r.log_z_fwd + r.log_z_rev)) <= 1e-12
        print("ptz checker %d->%d %s %s: log Z^ %.5f (fwd %.5f, rev %.5f) +- %.5f, exact %.5f"
              % (V, H, "GRBM" if gauss else "RBM", method, r.log_z, r.log_z_fwd, r.log_z_rev, r.stderr, exact))
        assert r.stderr > 0 and abs(r.log_z - exact) <= 4 * r.stderr and abs(r.log_z - exact) <= 0.05


def test_surface_rules(oracle_engine):
    rbm = _layer(oracle_engine, 10, 4, False)
    chains = rbm.tempered_chains(3, betas=[0.1, 0.5, 1.0])
    with pytest.raises(ValueError, match="betas\\[0\\] = 0"):
        chains.log_partition(10, 2)
    chains = rbm.tempered_chains(3, n_betas=4)
    with pytest.raises(ValueError, match="no swap attempt"):
        chains.log_partition(5, 4)               # one sweep after burn-in: the pairs of the other parity are never tried
    for n, burn in ((0, 0), (3, 3), (3, -1)):
        with pytest.raises(ValueError):
            chains.log_partition(n, burn)
    with pytest.raises(ValueError, match="mid"):
        chains.log_partition(10, 2, method="ais")
    with pytest.raises(ValueError, match="tempering"):
        rbm.log_partition(method="exact")
    assert rbm._rng_step == 0 and chains.n_done == 0


def test_ais_is_unchanged_bit_for_bit(ais_engine):
    """method="ais" and the default are the AIS path as it was: the twin's log weights through ais_estimate, to the bit, and
    the same RNG steps; ais_estimate's closed-form log Z_A is the helper the tempering estimate uses."""
    import mdbn_amd
    from mdbn_amd.temper import base_log_partition
    for gauss in (False, True):
        V, H = 12, 6
        bA = np.random.RandomState(8).normal(0, 0.3, V).astype(np.float32)
        got = []
        for kw in (dict(), dict(method="ais")):
            rbm = _layer(ais_engine, V, H, gauss)
            rbm._rng_step = 4
            got.append(rbm.log_partition(n_chains=32, n_betas=20, base_vbias=bA, **kw))
            assert rbm._rng_step == 4 + 2 * 20 - 1
        W, c, b = _params(rbm)
        logw = A.ais_twin(W, c, b, bA, gauss, np.linspace(0, 1, 21), 32, rbm.theano_rng.seed, rbm.stream_id, 4)["logw"]
        want = A.estimate(logw, bA, H, gauss)
        assert got[0] == got[1] == mdbn_amd.ais_estimate(logw, bA, H, gauss) == want
        assert base_log_partition(bA, H, gauss) == A.log_Z_base(bA, H, gauss)


def test_check_log_partition_and_the_layer_methods(ais_engine):
    """check_log_partition returns both estimates from one base-rate model; method="tempering" through log_partition,
    log_likelihood and DBN.layer_log_likelihood."""
    import mdbn_amd
    V, H = 12, 6
    rbm = _layer(ais_engine, V, H, False)
    W, c, b = _params(rbm)
    exact = A.brute_log_Z(W, c, b, False)
    data = (np.random.RandomState(1).uniform(size=(40, V)) < 0.4).astype(np.float32)
    kw = dict(n_ladders=16, n_sweeps=300, burn_in=60)
    r = rbm.check_log_partition(data=data, n_chains=64, n_betas=200, n_ladder_betas=8, **kw)
    assert set(r) == {"ais", "ais_stderr", "tempering", "tempering_stderr", "bracket", "z", "detail"}
    assert r["z"] == abs(r["ais"] - r["tempering"]) / np.hypot(r["ais_stderr"], r["tempering_stderr"])
    assert r["bracket"] == (r["detail"].log_z_fwd, r["detail"].log_z_rev) and r["tempering"] == r["detail"].log_z
    print("check_log_partition 12->6: AIS %.4f +- %.4f, tempering %.4f +- %.4f, bracket (%.4f, %.4f), z %.2f, exact %.4f"
          % (r["ais"], r["ais_stderr"], r["tempering"], r["tempering_stderr"], r["bracket"][0], r["bracket"][1], r["z"], exact))
    assert abs(r["ais"] - exact) <= 0.1 and abs(r["tempering"] - exact) <= 0.1
    step = rbm._rng_step
    lz, se = rbm.log_partition(method="tempering", n_betas=8, data=data, **kw)
    assert rbm._rng_step == step + 900 and abs(lz - exact) <= max(4 * se, 0.05)
    ll, se2 = rbm.log_likelihood(data, method="tempering", n_betas=8, **kw)
    neg_F = -np.asarray(rbm.free_energy(data).get_value(), dtype=np.float64)
    assert se2 > 0 and abs(ll - (neg_F.mean() - exact)) <= max(4 * se2, 0.05)
    # the DBN forwards the keywords to its layer
    dbn = mdbn_amd.DBN(numpy_rng=np.random.RandomState(2), n_ins=V, hidden_layers_sizes=[H, 4], n_outs=2, engine=ais_engine)
    for i in (0, 1):
        layer = dbn.rbm_layers[i]
        step = layer._rng_step
        ll, se = dbn.layer_log_likelihood(i, data, method="tempering", n_betas=8, n_ladders=4, n_sweeps=20, burn_in=4)
        assert np.isfinite(ll) and se > 0 and layer._rng_step == step + 60


# ---------------------------------------------------------------------------------- the C-ABI, on the host
@pytest.fixture(scope="module")
def lib(built_lib):
    from mdbn_amd import _lib
    return _lib.load()


def test_declared_exported_and_bound(lib):
    from mdbn_amd import _lib
    import mdbn_amd
    header = open(os.path.join(ROOT, "include", "mdbn_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int\s+%s\(" % name, header, re.M), "%s is not declared in include/mdbn_hip.h" % name
        assert name in _lib.SIGNATURES, "%s has no ctypes signature" % name
        assert hasattr(lib, name), "%s is not exported by the library" % name
        decl = header[header.index(name + "("):]
        assert len(_lib.SIGNATURES[name]) == decl[:decl.index(");")].count(",") + 1
    assert _lib.SIGNATURES["mdbn_pt_run_z"][:-2] == _lib.SIGNATURES["mdbn_pt_run"]
    assert hasattr(mdbn_amd.TemperedChains, "log_partition") and hasattr(mdbn_amd.RBM, "check_log_partition")


def _bytes(lib, M, R, V, H, path=0, z=True):
    n = C.c_int64(-1)
    fn = lib.mdbn_pt_run_z_workspace_bytes if z else lib.mdbn_pt_workspace_bytes
    return fn(None, M, R, V, H, path, C.byref(n)), n.value


def test_workspace_bytes_rules(lib):
    from mdbn_amd import _lib
    assert _bytes(lib, 0, 16, 100, 24)[0] == MDBN_EINVAL
    assert _bytes(lib, 64, 1, 100, 24)[0] == MDBN_EINVAL and "R = 1" in _lib.last_error()
    assert _bytes(lib, 64, 16, 100, 24, path=3)[0] == MDBN_EINVAL
    assert _bytes(lib, 64, 16, 4096, 1024, path=1)[0] == MDBN_EINVAL and "LDS-resident" in _lib.last_error()
    assert lib.mdbn_pt_run_z_workspace_bytes(None, 64, 16, 100, 24, 0, None) == MDBN_EINVAL
    # the one-launch path keeps the works in the caller's buffer: the workspace of mdbn_pt_run; the general path adds g
    for M, V, H in ((64, 100, 24), (512, 100, 24), (64, 784, 500)):
        for path in (0, 2) + ((1,) if V <= 512 else ()):
            (rc, z), (rc0, plain) = _bytes(lib, M, 16, V, H, path), _bytes(lib, M, 16, V, H, path, z=False)
            assert rc == rc0 == 0
            one_launch = path == 1 or (path == 0 and _bytes(lib, M, 16, V, H, 0, z=False) == _bytes(lib, M, 16, V, H, 1, z=False))
            assert z == plain if one_launch else plain < z <= plain + 256, (M, V, H, path, z, plain)


def _run(lib, M=64, R=16, V=100, H=24, n=8, burn_in=0, path=0, spl=0, ws_bytes=0, ldv=None, ldh=None, gauss=0, betas=None, sweep0=0):
    # (NULL device pointers throughout: every rule below is answered before one is looked at, let alone a kernel launched)
    if betas is None:
        betas = np.linspace(0, 1, R)
    betas = np.ascontiguousarray(betas, dtype=np.float32)
    return lib.mdbn_pt_run_z(None, None, None, V, H, H if ldh is None else ldh, None, None, None, gauss,
                             betas.ctypes.data_as(C.c_void_p), R, M, V if ldv is None else ldv, None, None, None,
                             n, burn_in, sweep0, None, None, None, None, None, None, path, spl, None, None, ws_bytes, None, None)


def test_run_z_refuses_bad_arguments_without_a_launch(lib):
    """The rules of mdbn_pt_run, in its order, with the sizer of its own named in the workspace message."""
    from mdbn_amd import _lib
    assert _run(lib, M=0) == MDBN_EINVAL and "bad shape" in _lib.last_error()
    assert _run(lib, R=1, betas=[1.0]) == MDBN_EINVAL and "R = 1" in _lib.last_error()
    assert _run(lib, R=4, betas=[0.0, 0.5, 0.4, 1.0]) == MDBN_EINVAL and "rise strictly" in _lib.last_error()
    assert _run(lib, R=4, betas=[0.0, 0.3, 0.6, 0.9]) == MDBN_EINVAL and "exactly 1" in _lib.last_error()
    assert _run(lib, R=4, betas=[-0.1, 0.3, 0.6, 1.0]) == MDBN_EINVAL and "negative" in _lib.last_error()
    assert _run(lib, n=0) == MDBN_EINVAL and "n_sweeps" in _lib.last_error()
    assert _run(lib, burn_in=8) == MDBN_EINVAL and "burn_in" in _lib.last_error()
    assert _run(lib, sweep0=-1) == MDBN_EINVAL and "sweep0" in _lib.last_error()
    assert _run(lib, path=7) == MDBN_EINVAL and "path" in _lib.last_error()
    assert _run(lib, gauss=2) == MDBN_EINVAL and "gauss" in _lib.last_error()
    assert _run(lib, spl=-1) == MDBN_EINVAL and "steps_per_launch" in _lib.last_error()
    assert _run(lib, V=4096, H=1024, path=1) == MDBN_EINVAL and "LDS-resident" in _lib.last_error()
    assert _run(lib, R=6, path=1) == MDBN_EINVAL and "multiple of 4" in _lib.last_error()
    assert _run(lib, ldv=102) == MDBN_EINVAL and "leading" in _lib.last_error()
    for path in (0, 1, 2):
        rc, need = _bytes(lib, 64, 16, 100, 24, path=path)
        assert rc == 0
        assert _run(lib, path=path, ws_bytes=need - 4) == MDBN_EINVAL and "mdbn_pt_run_z_workspace_bytes" in _lib.last_error()
        assert _run(lib, path=path, ws_bytes=need) == MDBN_EINVAL and "NULL" in _lib.last_error()
