"""Sizers against what the entry points accept, on the host (no device: the sizing calls need none).

The propagate-only entry points (mdbn_propup_sample, mdbn_propdown_sample, mdbn_gibbs_chain, mdbn_free_energy) accept any
workspace of at least the minimum the header states (MDBN_MIN_WORKSPACE_BYTES, mdbn_min_workspace_bytes) and refuse less
with MDBN_ENOSPC.  The property here: the answer of mdbn_workspace_bytes -- the one sizer include/mdbn_hip.h documents for
them -- is never below that minimum, whatever the shape (the core carve-up of a tiny layer is: 35 KB at 4 x 8 -> 8).  The
minimum is the library's statement, read from it; the test derives nothing."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(4, 8, 8), (1, 1, 1), (20, 100, 24)] + \
         [(B, V, H) for B in (1, 3, 4, 7, 33, 128, 300) for V in (1, 6, 30, 100, 520) for H in (1, 5, 8, 40, 128)]


def _lib():
    from mdbn_amd import _lib
    return _lib.load()


def _minimum(lib):
    n = C.c_int64()
    assert lib.mdbn_min_workspace_bytes(C.byref(n)) == 0
    return n.value


def test_header_states_the_minimum_the_library_enforces(built_lib):
    text = open(os.path.join(ROOT, "include", "mdbn_hip.h")).read()
    m = re.search(r"^#define\s+MDBN_MIN_WORKSPACE_BYTES\s+(\d+)", text, flags=re.M)
    assert m, "include/mdbn_hip.h does not define MDBN_MIN_WORKSPACE_BYTES"
    assert int(m.group(1)) == _minimum(_lib())
    assert "for shapes up to" not in text


@pytest.mark.parametrize("B,V,H", SHAPES)
def test_core_sizer_serves_the_propagation_calls(built_lib, B, V, H):
    lib = _lib()
    n = C.c_int64()
    assert lib.mdbn_workspace_bytes(B, V, H, C.byref(n)) == 0
    assert n.value >= _minimum(lib), "mdbn_workspace_bytes(%d, %d, %d) = %d: the propagation calls refuse it" % (B, V, H, n.value)
    assert n.value % 16 == 0


@pytest.mark.parametrize("B,V,H", SHAPES)
def test_ld_sizer_is_the_core_sizer_on_policy_leading_dimensions(built_lib, B, V, H):
    """mdbn_workspace_bytes_ld on the leading dimensions mdbn_padded_ld hands out, and on the plane path's round_up(H, 128):
    the answers of mdbn_workspace_bytes, bit for bit; wider ones never ask for less."""
    lib = _lib()
    n, m, ld = C.c_int64(), C.c_int64(), C.c_int64()
    assert lib.mdbn_workspace_bytes(B, V, H, C.byref(n)) == 0
    assert lib.mdbn_padded_ld(V, C.byref(ld)) == 0
    ldv = ld.value
    assert lib.mdbn_padded_ld(H, C.byref(ld)) == 0
    for ldh in (ld.value, (H + 127) // 128 * 128):
        assert lib.mdbn_workspace_bytes_ld(B, V, H, ldv, ldh, C.byref(m)) == 0
        assert m.value == n.value, (ldv, ldh, m.value, n.value)
    assert lib.mdbn_workspace_bytes_ld(B, V, H, ldv + 64, (H + 127) // 128 * 128 + 128, C.byref(m)) == 0
    assert m.value >= n.value


def test_ld_sizer_grows_with_the_column_sum_regions(built_lib):
    """200 x 300 -> 40 on ldv = 364, ldh = 256: 50 row groups of column sums on the caller's strides do not fit the regions
    of the policy's (2 * 50 * 128 and 50 * 300 floats)."""
    lib = _lib()
    n, m = C.c_int64(), C.c_int64()
    assert lib.mdbn_workspace_bytes(200, 300, 40, C.byref(n)) == 0
    assert lib.mdbn_workspace_bytes_ld(200, 300, 40, 364, 256, C.byref(m)) == 0
    assert m.value >= n.value + 4 * (2 * 50 * (256 - 128) + 50 * (364 - 300))


def test_ld_sizer_refuses_bad_leading_dimensions(built_lib):
    from mdbn_amd import _lib
    lib = _lib.load()
    m = C.c_int64()
    assert lib.mdbn_workspace_bytes_ld(4, 8, 8, 6, 8, C.byref(m)) == -1          # ldv < V
    assert lib.mdbn_workspace_bytes_ld(4, 8, 8, 8, 10, C.byref(m)) == -1         # ldh % 4
    assert "leading dims" in _lib.last_error()


def test_propagation_seeds_keep_the_oracle_off_ties():
    """The seeds of tests/test_gpu_workspace_exact.py's propagation cases: no uniform of any pass lies within 4e-6 of the
    float64 mean it is compared with (the tie mask is 1e-6, the means' tolerance 2e-6), so on the device a sample that
    differs from the oracle's is a wrong sample, and a three-step chain cannot fork on a tie."""
    import numpy as np
    import test_gpu_workspace_exact as T
    for rows in T.ROWS:
        for call in ("propup", "propdown_rbm", "gibbs"):
            for name, (u, mean) in T._oracle(call, rows)[1].items():
                assert np.abs(u - mean).min() > 4e-6, (rows, call, name, np.abs(u - mean).min())
