"""Parallel tempering above the kernels (no GPU): the Python surface through the CPU checker engine (tests/_oracle_engine.py:
TemperedChains composes the sweep from the engine's eager calls there -- the CPU statement of the semantics) against the numpy
twin, and the C-ABI's declarations and argument rules, answered on the host before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _temper_np as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mdbn_pt_workspace_bytes", "mdbn_pt_run")
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


@pytest.mark.parametrize("gauss", [False, True])
def test_checker_engine_equals_the_twin(oracle_engine, gauss):
    """The eager composition and tests/_temper_np.py are two statements of the same semantics: same samples, same swaps."""
    V, H, M, R, n, burn = 30, 12, 5, 6, 9, 3
    rbm = _layer(oracle_engine, V, H, gauss)
    bA = np.random.RandomState(8).normal(0, 0.3, V).astype(np.float32)
    h0 = (np.random.RandomState(9).uniform(size=(M * R, H)) < 0.5).astype(np.float32)
    rbm._rng_step = 9
    chains = rbm.tempered_chains(M, n_betas=R, base_vbias=bA, start_h=h0)
    v_avg, h_avg, acceptance, tv, th, ts = chains.run(n, burn_in=burn, trace=True)
    tw = T.pt_twin(rbm.W.get_value(), rbm.hbias.get_value(), rbm.vbias.get_value(), bA, gauss, np.linspace(0, 1, R), h0, n, burn,
                   rbm.theano_rng.seed, rbm.stream_id, 9)
    assert rbm._rng_step == 9 + 3 * n and chains.n_done == n
    np.testing.assert_array_equal(ts.numpy(), tw["trace_swaps"])
    np.testing.assert_array_equal(th.numpy(), tw["trace_h"])
    np.testing.assert_allclose(tv.numpy(), tw["trace_v"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(v_avg.get_value(), tw["v_avg"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(h_avg.get_value(), tw["h_avg"], rtol=0, atol=2e-6)
    np.testing.assert_array_equal(chains.rank.numpy(), tw["rank"])
    from mdbn_amd.temper import attempts
    tries = attempts(M, R, 0, n)
    assert list(tries) == [M * 5 if rho % 2 == 0 else M * 4 for rho in range(R - 1)]
    np.testing.assert_allclose(acceptance.get_value(), tw["accepted"] / tries, rtol=0, atol=1e-7)           # (read back as float32)
    assert tw["accepted"].sum() > 0
    # a second run continues the parity and the RNG steps: the twin from the state it ended in
    chains.run(4)
    tw2 = T.pt_twin(rbm.W.get_value(), rbm.hbias.get_value(), rbm.vbias.get_value(), bA, gauss, np.linspace(0, 1, R), tw["h"], 4, 0,
                    rbm.theano_rng.seed, rbm.stream_id, 9 + 3 * n, rank0=tw["rank"], sweep0=n)
    np.testing.assert_array_equal(chains.rank.numpy(), tw2["rank"])
    np.testing.assert_array_equal(chains.h.numpy(), tw2["h"])
    v, h = chains.samples()
    top = np.arange(M) * R + np.argmax(tw2["rank"] == R - 1, axis=1)
    np.testing.assert_array_equal(h.get_value(), tw2["h"][top])


def test_surface_rules(oracle_engine):
    import mdbn_amd
    rbm = _layer(oracle_engine, 10, 4, False)
    for betas in ([1.0], [0.0, 0.5], [0.0, 0.6, 0.5, 1.0], [-0.1, 1.0], [0.0, 0.5, 0.5, 1.0]):
        with pytest.raises(ValueError):
            rbm.tempered_chains(3, betas=betas)
    chains = rbm.tempered_chains(3, n_betas=4)
    assert isinstance(chains, mdbn_amd.TemperedChains)
    np.testing.assert_array_equal(chains.base_vbias, rbm.vbias.get_value())          # neither base_vbias nor data: the layer's own
    data = (np.random.RandomState(1).uniform(size=(20, 10)) < 0.3).astype(np.float32)
    np.testing.assert_array_equal(rbm.tempered_chains(3, n_betas=4, data=data).base_vbias, rbm.base_rate_vbias(data))
    for n, burn in ((0, 0), (3, 3), (3, -1)):
        with pytest.raises(ValueError):
            chains.run(n, burn_in=burn)
    with pytest.raises(ValueError):
        rbm.tempered_chains(3, n_betas=4, start_h=np.zeros((5, 4)))
    assert rbm._rng_step == 0
    with pytest.raises(ValueError, match="persistent"):
        rbm.training(data, None, 1, batch_size=5, persistent=False, tempering=4)


def test_persistent_copies_and_sample_tempered(oracle_engine):
    import mdbn_amd
    V, H, M, R = 12, 5, 4, 4
    rbm = _layer(oracle_engine, V, H, False)
    chains = rbm.tempered_chains(M, n_betas=R)
    chains.run(6)
    rank = chains.rank.numpy()
    top = np.arange(M) * R + np.argmax(rank == R - 1, axis=1)
    buf = mdbn_amd.shared(np.zeros((M, H), dtype=np.float32), engine=oracle_engine)
    chains.to_persistent(buf)
    np.testing.assert_array_equal(buf.get_value(), chains.h.numpy()[top])
    new = (np.random.RandomState(2).uniform(size=(M, H)) < 0.5).astype(np.float32)
    before = chains.h.numpy().copy()
    chains.from_persistent(mdbn_amd.shared(new, engine=oracle_engine))
    np.testing.assert_array_equal(chains.h.numpy()[top], new)
    rest = np.setdiff1d(np.arange(M * R), top)
    np.testing.assert_array_equal(chains.h.numpy()[rest], before[rest])
    other = _layer(oracle_engine, V, H, False)
    v, h, v_avg, h_avg, acceptance = other.sample_tempered(6, n_sweeps=10, burn_in=2, n_betas=4)
    assert v.shape == (6, V) and h.shape == (6, H) and v_avg.shape == (6, V) and h_avg.shape == (6, H) and acceptance.shape == (3,)
    assert other._rng_step == 30 and ((v_avg > 0) & (v_avg < 1)).all()


def test_tempered_pcd_is_the_composed_sequence(oracle_engine):
    """RBM.training(persistent=True, tempering=R) against run(1), to_persistent, PCD step, from_persistent by hand; and
    tempering=None leaves the PCD trainer as it was."""
    import mdbn_amd
    eng = oracle_engine
    V, H, B, R = 12, 5, 6, 4
    data = (np.random.RandomState(4).uniform(size=(3 * B, V)) < 0.5).astype(np.float32)
    one, two, three, four = (_layer(eng, V, H, False) for _ in range(4))
    np.random.seed(7)
    one.training(data, None, training_epochs=1, batch_size=B, learning_rate=0.05, persistent=True, tempering=R)
    np.random.seed(7)
    _, batches = mdbn_amd.get_minibatches_idx(3 * B, B, shuffle=True)
    cost, updates = two.get_cost_updates(lr=0.05, k=1, batch_size=B,
                                         persistent=mdbn_amd.shared(np.zeros((B, H), dtype=np.float32), engine=eng))
    ladders = two.tempered_chains(B, n_betas=R)
    step = mdbn_amd.function(updates, mdbn_amd.shared(data, engine=eng))
    for idx in batches:
        ladders.run(1)
        ladders.to_persistent(updates.persistent)
        step(eng.index_tensor(idx), 0.0)
        ladders.from_persistent(updates.persistent)
    step.flush()
    assert one._rng_step == two._rng_step and one.tempered.n_done == 3
    for name in ("W", "hbias", "vbias"):
        np.testing.assert_array_equal(getattr(one, name).get_value(), getattr(two, name).get_value(), err_msg=name)
    np.testing.assert_array_equal(one.tempered.rank.numpy(), ladders.rank.numpy())
    np.random.seed(7)
    three.training(data, None, training_epochs=1, batch_size=B, learning_rate=0.05, persistent=True)
    np.random.seed(7)
    four.training(data, None, training_epochs=1, batch_size=B, learning_rate=0.05, persistent=True, tempering=None)
    np.testing.assert_array_equal(three.W.get_value(), four.W.get_value())
    assert three._rng_step == four._rng_step and not np.array_equal(three.W.get_value(), one.W.get_value())


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
    assert "mdbn_temper.hip" in build.SOURCES and "mdbn_temper.h" in build.HEADERS
    import mdbn_amd
    assert hasattr(mdbn_amd.HipEngine, "temper") and hasattr(mdbn_amd.RBM, "tempered_chains") and hasattr(mdbn_amd.RBM, "sample_tempered")


def _bytes(lib, M, R, V, H, path=0):
    n = C.c_int64(-1)
    return lib.mdbn_pt_workspace_bytes(None, M, R, V, H, path, C.byref(n)), n.value


def test_workspace_bytes_rules(lib):
    from mdbn_amd import _lib
    assert _bytes(lib, 0, 16, 100, 24)[0] == MDBN_EINVAL
    assert _bytes(lib, 64, 1, 100, 24)[0] == MDBN_EINVAL and "R = 1" in _lib.last_error()
    assert _bytes(lib, 64, 16, 100, 24, path=3)[0] == MDBN_EINVAL
    assert _bytes(lib, 64, 16, 4096, 1024, path=1)[0] == MDBN_EINVAL and "LDS-resident" in _lib.last_error()
    assert _bytes(lib, 64, 6, 100, 24, path=1)[0] == MDBN_EINVAL and "multiple of 4" in _lib.last_error()
    assert lib.mdbn_pt_workspace_bytes(None, 64, 16, 100, 24, 0, None) == MDBN_EINVAL
    # path 0 takes the one-launch path only where it was measured to win (two workgroups per CU and >= 512 ladders:
    # 100->24 at M = 512, 24.4 against 30.9 us a sweep), the general path elsewhere -- 4096->1024, which does not fit, and
    # 400->40 at R = 16, which fits (path 1 is accepted) but measured 30.2 against 27.1 us a sweep at M = 64 and 60.6 against 58.7
    # at M = 512: the issue asked for "path 0 == path 1 for 400->40 at R = 16" AND that path 0 never pick the one-launch path
    # where it does not win; the measurement decides between the two
    assert _bytes(lib, 512, 16, 100, 24, path=0) == _bytes(lib, 512, 16, 100, 24, path=1)
    assert _bytes(lib, 64, 16, 100, 24, path=0) == _bytes(lib, 64, 16, 100, 24, path=2)
    for M in (64, 512):
        assert _bytes(lib, M, 16, 400, 40, path=1)[0] == 0
        assert _bytes(lib, M, 16, 400, 40, path=0) == _bytes(lib, M, 16, 400, 40, path=2)
    assert _bytes(lib, 64, 16, 4096, 1024, path=0) == _bytes(lib, 64, 16, 4096, 1024, path=2)
    assert _bytes(lib, 64, 6, 100, 24, path=0) == _bytes(lib, 64, 6, 100, 24, path=2)
    assert _bytes(lib, 64, 16, 400, 40, path=1)[1] < _bytes(lib, 64, 16, 400, 40, path=2)[1]
    # monotone in M and in R, on both paths
    for path, V, H in ((1, 400, 40), (2, 400, 40), (2, 784, 500)):
        by_m = [_bytes(lib, M, 16, V, H, path) for M in (1, 2, 5, 64, 65, 512, 513)]
        by_r = [_bytes(lib, 64, R, V, H, path) for R in (4, 8, 12, 16, 32, 64)]
        for seq in (by_m, by_r):
            assert all(rc == 0 for rc, _ in seq)
            assert all(y[1] >= x[1] for x, y in zip(seq, seq[1:])), (path, V, H, seq)
        assert by_m[-1][1] > by_m[0][1] and by_r[-1][1] > by_r[0][1]


def _run(lib, M=64, R=16, V=100, H=24, n=8, burn_in=0, path=0, spl=0, ws_bytes=0, ldv=None, ldh=None, gauss=0, betas=None, sweep0=0):
    # (NULL device pointers throughout: every rule below is answered before one is looked at, let alone a kernel launched;
    #  betas is a HOST array and is read)
    if betas is None:
        betas = np.linspace(0, 1, R)
    betas = np.ascontiguousarray(betas, dtype=np.float32)
    return lib.mdbn_pt_run(None, None, None, V, H, H if ldh is None else ldh, None, None, None, gauss,
                           betas.ctypes.data_as(C.c_void_p) if betas.size else None, R, M, V if ldv is None else ldv, None, None, None,
                           n, burn_in, sweep0, None, None, None, None, None, None, path, spl, None, None, ws_bytes)


def test_run_refuses_bad_arguments_without_a_launch(lib):
    from mdbn_amd import _lib
    assert _run(lib, M=0) == MDBN_EINVAL and "bad shape" in _lib.last_error()
    assert _run(lib, R=1, betas=[1.0]) == MDBN_EINVAL and "R = 1" in _lib.last_error()
    assert _run(lib, R=4, betas=[0.0, 0.5, 0.4, 1.0]) == MDBN_EINVAL and "rise strictly" in _lib.last_error()
    assert _run(lib, R=4, betas=[0.0, 0.5, 0.5, 1.0]) == MDBN_EINVAL and "rise strictly" in _lib.last_error()
    assert _run(lib, R=4, betas=[0.0, 0.3, 0.6, 0.9]) == MDBN_EINVAL and "exactly 1" in _lib.last_error()
    assert _run(lib, R=4, betas=[0.0, 0.3, 0.6, 1.0 + 2e-7]) == MDBN_EINVAL and "exactly 1" in _lib.last_error()
    assert _run(lib, R=4, betas=[-0.1, 0.3, 0.6, 1.0]) == MDBN_EINVAL and "negative" in _lib.last_error()
    assert _run(lib, n=0) == MDBN_EINVAL and "n_sweeps" in _lib.last_error()
    assert _run(lib, burn_in=8) == MDBN_EINVAL and "burn_in" in _lib.last_error()
    assert _run(lib, burn_in=-1) == MDBN_EINVAL and "burn_in" in _lib.last_error()
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
        assert _run(lib, path=path, ws_bytes=need - 4) == MDBN_EINVAL and "workspace" in _lib.last_error()
        # enough workspace: the next rule in line is the NULL context
        assert _run(lib, path=path, ws_bytes=need) == MDBN_EINVAL and "NULL" in _lib.last_error()
