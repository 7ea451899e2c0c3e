"""The references of tests/test_gpu_helpers.py, pinned without a GPU (tests/_helpers_np.py): tensor.round against exact
rational arithmetic on the whole edge list, the integer bfloat16 rounding against torch's CPU cast on the whole case list."""
import numpy as np
import pytest
import torch

import _helpers_np as R
from oracle import rbm_np


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_round_half_away_equals_the_rational_result_on_the_edge_list(dtype):
    x = R.round_edges().astype(dtype)
    assert len(x) == 34
    got = R.round_half_away(x)
    assert got.dtype == x.dtype
    for v, g in zip(x, got):
        if np.isnan(v):
            assert np.isnan(g)
        elif np.isinf(v):
            assert g == v
        else:
            neg, mag = R.round_half_away_exact(v)
            assert float(g) == (-mag if neg else mag), (v, g)      # (ints of this size are exact in float64)
        assert np.signbit(g) == np.signbit(v), (v, g)               # the sign survives on zeros and NaN too


def test_round_half_away_on_the_two_defect_cases():
    """What floor(|x| + 0.5), evaluated in float32, gets wrong -- and the rational reference and round_half_away get right."""
    below_half, odd = R.f32([R.BELOW_HALF])[0], np.float32(8388609.0)
    naive = lambda a: np.sign(a) * np.floor(np.abs(a) + np.float32(0.5))
    assert naive(below_half) == 1.0 and naive(odd) == 8388610.0
    assert R.round_half_away_exact(below_half) == (False, 0) and R.round_half_away_exact(odd) == (False, 8388609)
    got = R.round_half_away(np.array([below_half, -below_half, odd, -odd], dtype=np.float32))
    assert got.tolist() == [0.0, -0.0, 8388609.0, -8388609.0] and np.signbit(got[1])


def test_round_half_away_on_every_quarter_and_random_values():
    """Quarters (the inputs of the existing monitoring tests: the old expression is exact there, so nothing moves) and random
    values of every magnitude up to 2^25, in float32, against the rational result."""
    rs = np.random.RandomState(0)
    x = np.concatenate([np.arange(-40, 41) / 4.0, rs.normal(0, 3, 500), np.ldexp(rs.uniform(1, 2, 300), rs.randint(-30, 26, 300))
                        * rs.choice([-1, 1], 300)]).astype(np.float32)
    got = R.round_half_away(x)
    for v, g in zip(x, got):
        neg, mag = R.round_half_away_exact(v)
        assert float(g) == (-mag if neg else mag) and np.signbit(g) == np.signbit(v), (v, g)


def test_oracle_pseudo_likelihood_rounds_exactly_in_float32():
    """rbm_np.pseudo_likelihood_cost in float32 on a column of 0.49999997: the same cost as in float64 (the old line rounded
    that column to 1 in float32 and to 0 in float64, which swaps the two free energies)."""
    V, H, B = 12, 7, 8
    rs = np.random.RandomState(2)
    W = rbm_np.init_W(rs, V, H, np.float64)
    hb, vb = rs.normal(0, 0.5, H), rs.normal(0, 0.5, V)
    x = (rs.uniform(size=(B, V)) < 0.5).astype(np.float32)
    x[:, 3] = R.f32([R.BELOW_HALF])[0]
    costs = {}
    for dt in (np.float32, np.float64):
        st = rbm_np.RBMState(V, H, W=W, hbias=hb, vbias=vb, dtype=dt)
        st.bit_i_idx = 3
        costs[dt] = float(rbm_np.pseudo_likelihood_cost(st, x.astype(dt)))
    assert abs(costs[np.float32] - costs[np.float64]) <= 1e-5 * abs(costs[np.float64])


def test_oracle_engine_round_flip_in_float32():
    from _oracle_engine import OracleEngine
    eng = OracleEngine(dtype=np.float32)
    x = R.cyclic(R.round_edges(), 5, 7)
    got = eng.round_flip(torch.from_numpy(x), 6).numpy()
    want = R.round_half_away(x.astype(np.float64))
    want[:, 6] = 1 - want[:, 6]
    np.testing.assert_array_equal(got, want.astype(np.float32))


def test_bf16_rne_bits_equals_the_torch_cast_bit_for_bit():
    u = np.concatenate([R.bf16_cases(), R.BF16_SUBNORMAL_BITS, R.BF16_SUBNORMAL_BITS | np.uint32(0x80000000)])
    assert len(u) >= 4096 + 60
    got = R.bf16_rne_bits(u)
    cast = torch.from_numpy(R.f32(u).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = R.is_nan_f32_bits(u)
    assert nan.sum() == 6
    assert R.is_nan_bf16(got[nan]).all() and R.is_nan_bf16(cast[nan]).all()
    assert ((got[nan] >> 15) == (u[nan] >> 31)).all()                              # a NaN keeps its sign
    np.testing.assert_array_equal(got[~nan], cast[~nan])
    assert not R.is_nan_bf16(got[~nan]).any()


def test_bf16_rne_bits_named_cases():
    b = lambda *u: R.bf16_rne_bits(np.array(u, dtype=np.uint32)).tolist()
    assert b(0x3F808000, 0x3F818000) == [0x3F80, 0x3F82]                           # ties: to the even upper half
    assert b(0x3F807FFF, 0x3F808001) == [0x3F80, 0x3F81]
    assert b(0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF) == [0x7F80, 0xFF80, 0x7F7F]       # FLT_MAX becomes inf
    assert b(0x80000000, 0x7F800000, 0xFF800000) == [0x8000, 0x7F80, 0xFF80]
    assert b(0x00000001, 0x00008000, 0x00018000, 0x007FFFFF) == [0, 0, 2, 0x0080]  # subnormals, RNE
    assert R.is_nan_bf16(b(0x7F800001, 0xFFA00000)).all()


def test_case_lists_are_what_the_gpu_tests_rely_on():
    u = R.bf16_cases()
    assert len(u) == 2 * 32 + 4096 and len(set(u.tolist())) > 4000
    exp = (u >> 23) & 0xFF
    assert ((exp != 0) | ((u & 0x7FFFFFFF) == 0)).all()                            # no subnormal in the main list
    x, h = R.tanh_values(189, 0)
    assert h == 94 and len(x) == 189 and np.isnan(x[-1]) and not np.isnan(x[:-1]).any()
    np.testing.assert_array_equal(R.bits32(x[h:2 * h]), R.bits32(x[:h]) ^ np.uint32(0x80000000))
    assert (np.abs(x[:h]) < R.TANH_SMALL).sum() >= 30
