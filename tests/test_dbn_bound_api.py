"""Host side of the variational lower bound (mdbn_amd/bound.py, DBN.log_likelihood_bound, mdbn_amd.log_likelihood_bound) and
the C declarations of its kernels; no GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mdbn_propdown_rowll", "mdbn_rowll_workspace_bytes", "mdbn_sample_replicas")


def test_record_fields():
    from mdbn_amd import bound
    assert bound.Bound._fields == ("bound", "stderr", "log_z", "log_z_stderr", "rows", "row_stderr", "trace")
    assert bound.StackBound._fields == bound.Bound._fields + ("modality_rows", "joint_rows")
    r = bound.Bound(-1.0, 0.1, 2.0, 0.0, np.zeros(3), np.zeros(3), None)
    assert r.bound == -1.0 and r.stderr == 0.1 and r.log_z == 2.0 and r.trace is None


def test_exports():
    import mdbn_amd
    assert mdbn_amd.log_likelihood_bound is mdbn_amd.MDBN.log_likelihood_bound and "log_likelihood_bound" in mdbn_amd.__all__
    assert callable(mdbn_amd.DBN.log_likelihood_bound)
    assert callable(mdbn_amd.HipEngine.propdown_row_loglik) and callable(mdbn_amd.HipEngine.sample_replicas)


def test_declarations_bindings_and_doc_comment():
    from mdbn_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "mdbn_hip.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert name in comments, "%s is not described in a comment of the header" % name
        decl = code[code.index("int  %s(" % name):]
        assert len(_lib.SIGNATURES[name]) == decl[:decl.index(");")].count(",") + 1, name
    for word in ("softplus", "target_div", "0 log 0", "row_offset", "bit for bit"):
        assert word in comments
    assert "mdbn_bound.hip" in build.SOURCES and "mdbn_bound.h" in build.HEADERS
    assert "#define MDBN_VERSION 2" in text


@pytest.mark.parametrize("n,S,chunk,want", [
    (170, 64, 16384, [(0, 170)]),
    (1000, 64, 16384, [(0, 256), (256, 512), (512, 768), (768, 1000)]),
    (5, 64, 32, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]),          # fewer chunk rows than samples: one data row at a time
    (7, 3, 10, [(0, 3), (3, 6), (6, 7)]),
    (4, 1, 16384, [(0, 4)]),
])
def test_chunk_arithmetic(n, S, chunk, want):
    from mdbn_amd.bound import bound_chunks
    got = bound_chunks(n, S, chunk)
    assert got == want
    assert all((hi - lo) * S <= max(chunk, S) for lo, hi in got)
    assert [lo for lo, _ in got] == [0] + [hi for _, hi in got[:-1]] and got[-1][1] == n


def test_chunk_arguments_are_checked():
    from mdbn_amd.bound import bound_chunks
    for bad in ((10, 0, 100), (10, -1, 100), (10, 4, 0)):
        with pytest.raises(ValueError):
            bound_chunks(*bad)


def _dbn(rs, n_ins, hidden, n_outs, gauss):
    import mdbn_amd
    mdbn_amd.DBN.verbose = False
    return mdbn_amd.DBN(numpy_rng=rs, n_ins=n_ins, gauss=gauss, hidden_layers_sizes=hidden, n_outs=n_outs)


def test_bad_arguments_are_refused_before_any_device_work(oracle_engine):
    import mdbn_amd
    rs = np.random.RandomState(3)
    net = _dbn(rs, 8, [6], 4, False)
    x = (rs.uniform(size=(5, 8)) < 0.5).astype(np.float32)
    steps = [r._rng_step for r in net.rbm_layers]
    for bad in (0, -3):
        with pytest.raises(ValueError, match="n_samples"):
            net.log_likelihood_bound(x, n_samples=bad, log_z=0.0)
    with pytest.raises(ValueError, match="columns"):
        net.log_likelihood_bound(x[:, :7], log_z=0.0)
    assert [r._rng_step for r in net.rbm_layers] == steps, "a refused call consumed random numbers"
    a, b, joint = _dbn(rs, 5, [], 3, True), _dbn(rs, 4, [], 2, True), _dbn(rs, 5, [4], 3, False)
    xa, xb = rs.normal(size=(5, 5)).astype(np.float32), rs.normal(size=(5, 4)).astype(np.float32)
    with pytest.raises(ValueError, match="keys"):
        mdbn_amd.log_likelihood_bound([a, b], joint, {0: xa, 2: xb}, log_z=0.0)
    with pytest.raises(ValueError, match="keys"):
        mdbn_amd.log_likelihood_bound([a, b], joint, {0: xa}, log_z=0.0)
    with pytest.raises(ValueError, match="one input per modality"):
        mdbn_amd.log_likelihood_bound([a, b], joint, [xa], log_z=0.0)
    with pytest.raises(ValueError, match="n_samples"):
        mdbn_amd.log_likelihood_bound([a, b], joint, {0: xa, 1: xb}, n_samples=0, log_z=0.0)
    with pytest.raises(ValueError, match="same number of rows"):
        mdbn_amd.log_likelihood_bound([a, b], joint, [xa, xb[:4]], log_z=0.0)
    with pytest.raises(ValueError, match="joint network"):
        mdbn_amd.log_likelihood_bound([a, a], joint, [xa, xa], log_z=0.0)
