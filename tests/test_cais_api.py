"""The C-ABI of the clamped annealed importance sampling (mdbn_ais_cond_workspace_bytes, mdbn_ais_cond_run): declared,
exported, bound, and its argument rules answered on the host (no GPU, no launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mdbn_ais_cond_workspace_bytes", "mdbn_ais_cond_run")
MDBN_EINVAL = -1


@pytest.fixture(scope="module")
def lib(built_lib):
    from mdbn_amd import _lib
    return _lib.load()


def test_declared_exported_and_bound(lib):
    from mdbn_amd import _lib
    header = open(os.path.join(ROOT, "include", "mdbn_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int\s+%s\(" % name, header, re.M), "%s is not declared in include/mdbn_hip.h" % name
        assert name in _lib.SIGNATURES, "%s has no ctypes signature" % name
        assert hasattr(lib, name), "%s is not exported by the library" % name
        decl = header[header.index(name + "("):]
        assert len(_lib.SIGNATURES[name]) == decl[:decl.index(");")].count(",") + 1, name
    from mdbn_amd import build
    # (the clamped run is mdbn_ais.hip's kernels with a mask: no source of its own)
    assert "mdbn_ais.hip" in build.SOURCES and "mdbn_ais.h" in build.HEADERS and "mdbn_sampler_kit.h" in build.HEADERS


def test_public_names():
    import mdbn_amd
    assert callable(mdbn_amd.modality_log_likelihood) and callable(mdbn_amd.MDBN.modality_log_likelihood)
    for name in ("conditional_log_partition", "conditional_log_likelihood"):
        assert callable(getattr(mdbn_amd.RBM, name)) and callable(getattr(mdbn_amd.GRBM, name))
    assert callable(mdbn_amd.HipEngine.ais_conditional)


def _bytes(lib, N, Cn, V, H, n_betas=9, path=0):
    n = C.c_int64(-1)
    return lib.mdbn_ais_cond_workspace_bytes(None, N, Cn, V, H, n_betas, path, C.byref(n)), n.value


def test_workspace_bytes_rules(lib):
    from mdbn_amd import _lib
    assert _bytes(lib, 0, 4, 100, 24)[0] == MDBN_EINVAL and "bad shape" in _lib.last_error()
    assert _bytes(lib, 16, 0, 100, 24)[0] == MDBN_EINVAL and "bad shape" in _lib.last_error()
    assert _bytes(lib, 1 << 20, 1 << 12, 100, 24)[0] == MDBN_EINVAL and "too many" in _lib.last_error()
    assert _bytes(lib, 16, 4, 100, 24, n_betas=1)[0] == MDBN_EINVAL
    assert _bytes(lib, 16, 4, 100, 24, path=3)[0] == MDBN_EINVAL
    assert _bytes(lib, 16, 4, 4096, 1024, path=1)[0] == MDBN_EINVAL and "LDS-resident" in _lib.last_error()
    assert lib.mdbn_ais_cond_workspace_bytes(None, 16, 4, 100, 24, 9, 0, None) == MDBN_EINVAL
    for V, H in ((100, 24), (400, 40), (1024, 256), (4096, 1024)):
        for path in (0, 2) + ((1,) if V <= 512 else ()):
            sizes = []
            for N, Cn in ((1, 1), (1, 4), (7, 3), (11, 2), (16, 4), (8, 64), (513, 1), (8, 256)):     # N C rising
                rc, n = _bytes(lib, N, Cn, V, H, path=path)
                assert rc == 0 and n > 0
                sizes.append(n)
            assert sizes == sorted(sizes), "workspace of %d -> %d path %d is not monotone in N C: %r" % (V, H, path, sizes)
    # the chains are mdbn_ais_run's: never less than its workspace for N C chains; the one-launch path carries the state only
    n = C.c_int64(-1)
    for path in (1, 2):
        assert lib.mdbn_ais_workspace_bytes(None, 64, 400, 40, 9, path, C.byref(n)) == 0
        assert _bytes(lib, 16, 4, 400, 40, path=path)[1] >= n.value
    assert _bytes(lib, 16, 4, 400, 40, path=0) == _bytes(lib, 16, 4, 400, 40, path=1)
    assert _bytes(lib, 16, 4, 400, 40, path=1)[1] < _bytes(lib, 16, 4, 400, 40, path=2)[1]
    assert _bytes(lib, 16, 4, 4096, 1024, path=0) == _bytes(lib, 16, 4, 4096, 1024, path=2)


def test_workspace_is_the_free_runs_plus_d2_per_row(lib):
    """The one driver behind both runs carves one workspace: the clamped run's is mdbn_ais_run's for its N C chains, and on
    the general path one d2 sum per data row (rounded up to 64 floats) behind it."""
    n = C.c_int64(-1)
    for N, Cn in ((16, 4), (7, 3)):
        for V, H in ((100, 24), (1024, 256)):
            assert lib.mdbn_ais_workspace_bytes(None, N * Cn, V, H, 9, 2, C.byref(n)) == 0
            assert _bytes(lib, N, Cn, V, H, path=2) == (0, n.value + 4 * ((N + 63) // 64 * 64))
            n.value = -1                     # (path 1: equal where the layer is LDS-resident, refused alike where it is not)
            rc = lib.mdbn_ais_workspace_bytes(None, N * Cn, V, H, 9, 1, C.byref(n))
            assert rc == (0 if V <= 512 else MDBN_EINVAL) and (rc != 0 or n.value > 0)
            assert _bytes(lib, N, Cn, V, H, path=1) == (rc, n.value)


def _run(lib, N=16, Cn=4, V=100, H=24, n_betas=9, path=0, ws_bytes=0, ldv=None, ldh=None, mask_rows=None):
    # (NULL pointers throughout: every rule below is answered before a pointer is looked at, let alone a kernel launched)
    return lib.mdbn_ais_cond_run(None, None, None, V, H, H if ldh is None else ldh, None, None, None, 0, None, n_betas,
                                 None, None, N if mask_rows is None else mask_rows, N, Cn, V if ldv is None else ldv,
                                 None, None, None, None, path, None, None, ws_bytes)


def test_run_refuses_bad_arguments_without_a_launch(lib):
    from mdbn_amd import _lib
    assert _run(lib, N=0) == MDBN_EINVAL and "bad shape" in _lib.last_error()
    assert _run(lib, Cn=0) == MDBN_EINVAL and "bad shape" in _lib.last_error()
    assert _run(lib, n_betas=1) == MDBN_EINVAL and "n_betas" in _lib.last_error()
    assert _run(lib, mask_rows=2) == MDBN_EINVAL and "mask_rows" in _lib.last_error()
    assert _run(lib, mask_rows=64) == MDBN_EINVAL and "mask_rows" in _lib.last_error()      # (N C is not a mask's row count)
    assert _run(lib, path=7) == MDBN_EINVAL and "path" in _lib.last_error()
    assert _run(lib, V=4096, H=1024, path=1) == MDBN_EINVAL and "LDS-resident" in _lib.last_error()
    assert _run(lib, ldv=102) == MDBN_EINVAL and "leading" in _lib.last_error()
    for path in (0, 1, 2):
        for mask_rows in (1, 16):
            rc, need = _bytes(lib, 16, 4, 100, 24, path=path)
            assert rc == 0
            assert _run(lib, path=path, ws_bytes=need - 4, mask_rows=mask_rows) == MDBN_EINVAL and "workspace" in _lib.last_error()
            # enough workspace: the next rule in line is the NULL context
            assert _run(lib, path=path, ws_bytes=need, mask_rows=mask_rows) == MDBN_EINVAL and "NULL" in _lib.last_error()


def test_estimate_rows_is_the_twins():
    """mdbn_amd.rbm.ais_estimate_rows (float64 on the host) against tests/_cais_np.estimate_rows, and against ais_estimate row
    by row where no column is held."""
    import _cais_np as CA
    from mdbn_amd.rbm import ais_estimate, ais_estimate_rows
    rs = np.random.RandomState(0)
    bA = rs.normal(size=9)
    logw = 300.0 + rs.normal(size=(5, 7))
    mask = (rs.uniform(size=(5, 9)) < 0.5).astype(np.float32)
    mask[0], mask[1] = 0.0, 1.0
    for gauss in (False, True):
        lz, err = ais_estimate_rows(logw, bA, mask, 6, gauss)
        want_lz, want_err = CA.estimate_rows(logw, bA, mask, 6, gauss)
        np.testing.assert_allclose(lz, want_lz, rtol=0, atol=1e-12)
        np.testing.assert_allclose(err, want_err, rtol=0, atol=1e-12)
        one = ais_estimate(logw[0], bA, 6, gauss)
        assert abs(lz[0] - one[0]) <= 1e-12 and abs(err[0] - one[1]) <= 1e-12
        lz1, _ = ais_estimate_rows(logw, bA, mask[2:3], 6, gauss)                         # one mask row for every data row
        np.testing.assert_allclose(lz1, CA.estimate_rows(logw, bA, mask[2:3], 6, gauss)[0], rtol=0, atol=1e-12)
