"""The C-ABI of the annealed importance sampling (mdbn_ais_workspace_bytes, mdbn_ais_run): declared, exported, bound, and
its argument rules answered on the host (no GPU, no launch)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mdbn_ais_workspace_bytes", "mdbn_ais_run")
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
    decl = header[header.index("mdbn_ais_run("):]
    assert len(_lib.SIGNATURES["mdbn_ais_run"]) == decl[:decl.index(");")].count(",") + 1
    assert lib.mdbn_version() == 2
    from mdbn_amd import build
    assert "mdbn_ais.hip" in build.SOURCES and "mdbn_ais.h" in build.HEADERS and "mdbn_small_passes.h" in build.HEADERS


def _bytes(lib, M, V, H, n_betas=9, path=0):
    n = C.c_int64(-1)
    return lib.mdbn_ais_workspace_bytes(None, M, V, H, n_betas, path, C.byref(n)), n.value


def test_workspace_bytes_rules(lib):
    from mdbn_amd import _lib
    assert _bytes(lib, 0, 100, 24)[0] == MDBN_EINVAL
    assert _bytes(lib, 64, 100, 24, n_betas=1)[0] == MDBN_EINVAL
    assert _bytes(lib, 64, 100, 24, path=3)[0] == MDBN_EINVAL
    assert _bytes(lib, 64, 4096, 1024, path=1)[0] == MDBN_EINVAL and "LDS-resident" in _lib.last_error()
    assert lib.mdbn_ais_workspace_bytes(None, 64, 100, 24, 9, 0, None) == MDBN_EINVAL
    for V, H in ((100, 24), (400, 40), (1024, 256), (4096, 1024)):
        for path in (0, 2) + ((1,) if V <= 512 else ()):
            sizes = []
            for M in (1, 4, 22, 64, 512, 513, 2048):
                rc, n = _bytes(lib, M, V, H, path=path)
                assert rc == 0 and n > 0
                sizes.append(n)
            assert sizes == sorted(sizes), "workspace of %d -> %d path %d is not monotone in M: %r" % (V, H, path, sizes)
    # LDS-resident layers take the one-launch path by shape; its workspace is only the carried visible state
    assert _bytes(lib, 512, 400, 40, path=0) == _bytes(lib, 512, 400, 40, path=1)
    assert _bytes(lib, 512, 400, 40, path=1)[1] < _bytes(lib, 512, 400, 40, path=2)[1]
    assert _bytes(lib, 512, 4096, 1024, path=0) == _bytes(lib, 512, 4096, 1024, path=2)


def _run(lib, M=64, V=100, H=24, n_betas=9, path=0, ws_bytes=0, ldv=None, ldh=None):
    # (NULL pointers throughout: every rule below is answered before a pointer is looked at, let alone a kernel launched)
    return lib.mdbn_ais_run(None, None, None, V, H, H if ldh is None else ldh, None, None, None, 0, None, n_betas, M,
                            V if ldv is None else ldv, None, None, None, None, path, None, None, ws_bytes)


def test_run_refuses_bad_arguments_without_a_launch(lib):
    from mdbn_amd import _lib
    assert _run(lib, M=0) == MDBN_EINVAL and "bad shape" in _lib.last_error()
    assert _run(lib, n_betas=1) == MDBN_EINVAL and "n_betas" in _lib.last_error()
    assert _run(lib, path=7) == MDBN_EINVAL and "path" in _lib.last_error()
    assert _run(lib, V=4096, H=1024, path=1) == MDBN_EINVAL and "LDS-resident" in _lib.last_error()
    assert _run(lib, ldv=102) == MDBN_EINVAL and "leading" in _lib.last_error()
    for path in (0, 1, 2):
        rc, need = _bytes(lib, 64, 100, 24, path=path)
        assert rc == 0
        assert _run(lib, path=path, ws_bytes=need - 4) == MDBN_EINVAL and "workspace" in _lib.last_error()
        # enough workspace: the next rule in line is the NULL context
        assert _run(lib, path=path, ws_bytes=need) == MDBN_EINVAL and "NULL" in _lib.last_error()


def test_estimate_from_log_weights():
    """mdbn_amd.ais_estimate (float64 on the host): equal weights give log Z_A + log w exactly and no standard error."""
    import numpy as np
    import mdbn_amd
    bA = np.array([0.3, -1.0, 2.0])
    lz, err = mdbn_amd.ais_estimate(np.full(16, 250.0), bA, 5, False)
    assert abs(lz - (250.0 + 5 * np.log(2) + np.logaddexp(0, bA).sum())) < 1e-12 and err == 0.0
    lz, err = mdbn_amd.ais_estimate(np.array([700.0, 700.0 + np.log(3.0)]), bA, 5, True)
    assert abs(lz - (700.0 + np.log(2.0) + 5 * np.log(2) + 1.5 * np.log(2 * np.pi))) < 1e-12
    assert abs(err - 0.5 / np.sqrt(2)) < 1e-12
