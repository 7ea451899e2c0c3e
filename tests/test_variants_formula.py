"""The oracle side of tests/test_gpu_step_variants.py without a GPU: the statistics tests/_variants.py derives from the outputs
of a chain are the ones the oracle's own step function forms."""
import numpy as np
import pytest

from oracle import rbm_np
from oracle.philox_np import PhiloxDraws
from _variants import variant_statistics


@pytest.mark.parametrize("gauss", [False, True], ids=["rbm", "grbm"])
def test_sample_statistics_formula_equals_the_oracle_step(gauss):
    """12 -> 7, B = 5, CD-2, float64, the oracle's own (unforced) chain: S, s_h, s_v from (v0, ph, last visible sample, its
    propup) equal what rbm_np.cd_step(symbolic_grad=True) reports; the Bernoulli sample differs from its mean."""
    V, H, B, k = 12, 7, 5, 2
    rs = np.random.RandomState(2)
    st = rbm_np.RBMState(V, H, W=rbm_np.init_W(rs, V, H, np.float64), hbias=rs.normal(0, 0.2, H), vbias=rs.normal(0, 0.2, V),
                         gauss=gauss)
    v0 = rs.normal(size=(B, V)) if gauss else (rs.uniform(size=(B, V)) < 0.4).astype(np.float64)
    ph, _, out = rbm_np.cd_chain(st, v0, PhiloxDraws(3, 1, 0), k)
    got = variant_statistics(v0, ph, out, gauss, True)
    _, extras = rbm_np.cd_step(st.copy(), v0, PhiloxDraws(3, 1, 0), lr=0.01, k=k, symbolic_grad=True, return_extras=True)
    for name, a in zip(("S", "s_h", "s_v"), got):
        assert np.abs(a - extras[name]).max() <= 1e-13, name
    plain = variant_statistics(v0, ph, out, gauss, False)
    if gauss:
        assert all(np.array_equal(a, b) for a, b in zip(got, plain))        # sample = mean under error_free
    else:
        assert np.isin(out[2], (0.0, 1.0)).all() and np.abs(got[0] - plain[0]).max() > 1e-3
