"""The C-ABI of clamped annealed importance sampling on a layer with categorical visible units (mdbn_ais_cond_run_grouped):
declared, exported, bound, and its argument rules answered on the host (no GPU, no launch); the host finish
``ais_estimate_rows(..., groups=)``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mdbn_ais_cond_run_grouped"
MDBN_EINVAL = -1


@pytest.fixture(scope="module")
def lib(built_lib):
    from mdbn_amd import _lib
    return _lib.load()


def test_declared_exported_and_bound(lib):
    from mdbn_amd import _lib
    header = open(os.path.join(ROOT, "include", "mdbn_hip.h")).read()
    assert re.search(r"^int\s+%s\(" % NAME, header, re.M), "%s is not declared in include/mdbn_hip.h" % NAME
    assert NAME in _lib.SIGNATURES, "%s has no ctypes signature" % NAME
    assert hasattr(lib, NAME), "%s is not exported by the library" % NAME
    decl = header[header.index(NAME + "("):]
    sig = _lib.SIGNATURES[NAME]
    assert len(sig) == decl[:decl.index(");")].count(",") + 1
    # the arguments of mdbn_ais_cond_run without `gauss` (its tenth), then the table in its two copies and n_groups
    plain = _lib.SIGNATURES["mdbn_ais_cond_run"]
    assert sig[:-3] == plain[:9] + plain[10:] and sig[-3:] == _lib.SIGNATURES["mdbn_ais_run_grouped"][-3:]


def test_public_names():
    import mdbn_amd
    assert callable(mdbn_amd.HipEngine.ais_conditional_grouped)
    import inspect
    assert list(inspect.signature(mdbn_amd.HipEngine.ais_conditional_grouped).parameters) == [
        "self", "W", "hbias", "vbias", "base_vbias", "betas", "obs", "mask", "n_chains", "rng", "groups", "path", "trace", "state"]
    assert "groups" in inspect.signature(mdbn_amd.rbm.ais_estimate_rows).parameters


GOOD = np.arange(0, 101, 5, dtype=np.int32)


def _run(lib, N=16, Cn=4, V=100, H=24, n_betas=9, path=0, ws_bytes=0, ldv=None, ldh=None, mask_rows=None, table=GOOD, dev=True,
         host=True):
    # (NULL pointers throughout: every rule below is answered before a pointer is looked at, let alone a kernel launched; the
    # device copy of the table is never read on the host, so any non-NULL address stands for it)
    t = None if table is None else table.ctypes.data
    return lib.mdbn_ais_cond_run_grouped(None, None, None, V, H, H if ldh is None else ldh, None, None, None, None, n_betas,
                                         None, None, N if mask_rows is None else mask_rows, N, Cn, V if ldv is None else ldv,
                                         None, None, None, None, path, None, None, ws_bytes, t if dev else None,
                                         t if host else None, 0 if table is None else table.size - 1)


def test_run_refuses_a_bad_table_without_a_launch(lib):
    from mdbn_amd import _lib
    for what, table in (("not ascending", [0, 10, 5]), ("a group of 1 column", [0, 1]), ("a group of 65 columns", [0, 65]),
                        ("a boundary beyond V", [90, 101])):
        assert _run(lib, table=np.array(table, dtype=np.int32)) == MDBN_EINVAL and "group" in _lib.last_error(), what
    assert _run(lib, host=False) == MDBN_EINVAL and "group_start" in _lib.last_error()
    assert _run(lib, dev=False) == MDBN_EINVAL and "group_start" in _lib.last_error()


def test_run_refuses_what_the_plain_clamped_run_refuses(lib):
    from mdbn_amd import _lib
    assert _run(lib, N=0) == MDBN_EINVAL and "bad shape" in _lib.last_error()
    assert _run(lib, Cn=0) == MDBN_EINVAL and "bad shape" in _lib.last_error()
    assert _run(lib, n_betas=1) == MDBN_EINVAL and "n_betas" in _lib.last_error()
    assert _run(lib, mask_rows=2) == MDBN_EINVAL and "mask_rows" in _lib.last_error()
    assert _run(lib, mask_rows=64) == MDBN_EINVAL and "mask_rows" in _lib.last_error()      # (N C is not a mask's row count)
    assert _run(lib, path=7) == MDBN_EINVAL and "path" in _lib.last_error()
    assert _run(lib, V=1024, H=256, path=1, table=np.arange(0, 1025, 4, dtype=np.int32)) == MDBN_EINVAL \
        and "LDS-resident" in _lib.last_error()
    assert _run(lib, ldv=102) == MDBN_EINVAL and "leading" in _lib.last_error()
    n = C.c_int64(-1)
    for path in (0, 1, 2):
        for mask_rows in (1, 16):
            for table in (GOOD, None):                   # (n_groups = 0: no table read)
                assert lib.mdbn_ais_cond_workspace_bytes(None, 16, 4, 100, 24, 9, path, C.byref(n)) == 0
                assert _run(lib, path=path, ws_bytes=n.value - 4, mask_rows=mask_rows, table=table) == MDBN_EINVAL \
                    and "workspace" in _lib.last_error() and "mdbn_ais_cond_workspace_bytes" in _lib.last_error()
                # enough workspace: the next rule in line is the NULL context
                assert _run(lib, path=path, ws_bytes=n.value, mask_rows=mask_rows, table=table) == MDBN_EINVAL \
                    and "NULL" in _lib.last_error()


def _rows_formula(logw, bA, mask, H, gauss):
    """The arithmetic of ais_estimate_rows before it knew groups, restated."""
    logw = np.asarray(logw, dtype=np.float64)
    free = np.broadcast_to(np.asarray(mask) == 0, (logw.shape[0], np.asarray(mask).shape[1]))
    bA = np.asarray(bA, dtype=np.float64)
    per_col = np.full(bA.shape, 0.5 * np.log(2.0 * np.pi)) if gauss else np.logaddexp(0.0, bA)
    log_ZA = H * np.log(2.0) + (free * per_col[None, :]).sum(axis=1)
    top = logw.max(axis=1)
    w = np.exp(logw - top[:, None])
    mean = w.mean(axis=1)
    return log_ZA + top + np.log(mean), w.std(axis=1) / (mean * np.sqrt(logw.shape[1]))


def test_estimate_rows():
    """``groups=None``: the values from before, bit for bit.  With groups: the twin's, a free group one logsumexp at the mask of
    its FIRST column; no groups in the table: the plain values; every unit free: ``ais_estimate(groups=)`` row by row."""
    import _gcais_np as X
    import _gclamp_np as Gc
    from mdbn_amd.rbm import ais_estimate, ais_estimate_rows
    rs = np.random.RandomState(0)
    V, H, bounds = 12, 6, [2, 5, 8, 10]
    bA = rs.normal(size=V)
    logw = 300.0 + rs.normal(size=(5, 7))
    mask = Gc.unit_mask(V, bounds, rows=5)
    for gauss in (False, True):
        for m in (mask, mask[2:3], (rs.uniform(size=(5, V)) < 0.5).astype(np.float32)):
            got, want = ais_estimate_rows(logw, bA, m, H, gauss), _rows_formula(logw, bA, m, H, gauss)
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[1], want[1])
            np.testing.assert_array_equal(ais_estimate_rows(logw, bA, m, H, gauss, groups=None)[0], want[0])
    for m in (mask, mask[2:3]):
        lz, err = ais_estimate_rows(logw, bA, m, H, False, groups=bounds)
        want_lz, want_err = X.estimate_rows(logw, bA, m, H, bounds)
        np.testing.assert_allclose(lz, want_lz, rtol=0, atol=1e-12)
        np.testing.assert_allclose(err, want_err, rtol=0, atol=1e-12)
    split = mask.copy()
    split[3, 5:8] = (0.0, 1.0, 1.0)                      # the first column decides: the group [5, 8) of row 3 is free
    whole = mask.copy()
    whole[3, 5:8] = 0.0
    np.testing.assert_array_equal(ais_estimate_rows(logw, bA, split, H, False, groups=bounds)[0],
                                  ais_estimate_rows(logw, bA, whole, H, False, groups=bounds)[0])
    np.testing.assert_allclose(ais_estimate_rows(logw, bA, mask, H, False, groups=[V])[0], _rows_formula(logw, bA, mask, H, False)[0],
                               rtol=0, atol=1e-12)
    assert not mask[1].any()                             # (unit_mask: the second row holds nothing)
    one = ais_estimate(logw[1], bA, H, False, groups=bounds)
    lz, err = ais_estimate_rows(logw, bA, mask, H, False, groups=bounds)
    assert abs(lz[1] - one[0]) <= 1e-12 and abs(err[1] - one[1]) <= 1e-12
    with pytest.raises(ValueError):
        ais_estimate_rows(logw, bA, mask, H, True, groups=bounds)
