"""The learned-variance step and the grouped step in every form a minibatch reaches them in (tests/_step_forms.py; bounds of
tests/test_gpu_sigma.py and tests/test_gpu_softmax.py through ``_margins.check``): (1) the ``next_indexes`` hint changes no
bit; (2) a ragged last minibatch, with the idle rows of the full-size staging matrices poisoned; (3) PCD with ``learn_sigma``:
the chain is the recorded one and the pseudo-likelihood is that of the rows in units; (4) a host-resident table equals the
device-resident one bit for bit; (5) int32 and int64 index tensors give the same bits, an index list with a repeated row
meets the twin; (6) the first ``HiddenLayer`` of a pre-trained DBN takes raw rows to units with the GRBM's ``log_sigma``.

The smallest shapes: 60 -> 24 at B = 33 (K = 5 for the groups); (1) and (4) also at 1024 -> 512, B = 256 with
``planes_min_work`` 0 and ``gather_ahead`` 1 -- where a honoured hint would gather the next minibatch's rows inside this
step's statistics kernel."""
import numpy as np
import pytest

import _step_forms as sf
from _margins import check
from oracle import rbm_np

pytestmark = pytest.mark.gpu

REL = 2.0 ** -22
SMALL = (60, 24, 33, 1)                     # V, H, B, k
BIG = (1024, 512, 256, 1)
BIG_OPTS = dict(planes_min_work=0, gather_ahead=1)
SHAPES = [("small", SMALL, {}, 5), ("planes_shape", BIG, BIG_OPTS, 4)]     # id, shape, options, K of the groups


@pytest.fixture
def have_gpu(built_lib):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def grouped_engine(opts=None):
    import mdbn_amd
    return sf.set_options(mdbn_amd.HipEngine(), opts)


def finite(r):
    return np.isfinite(r.costs).all() and all(np.isfinite(a).all() for a in r.params.values()) and \
        all(np.isfinite(V2).all() and np.isfinite(P2).all() for V2, P2 in r.scratch)


# ------------------------------------------------------------------------------------------------------------------ 1. the hint
@pytest.mark.parametrize("name,shape,opts,K", SHAPES, ids=[s[0] for s in SHAPES])
def test_next_indexes_changes_nothing_in_a_sigma_step(have_gpu, name, shape, opts, K):
    V, H, B, k = shape
    without = sf.run_sigma(sf.sigma_engine(False, opts), V, H, B, k, True, "alone")
    hinted = sf.run_sigma(sf.sigma_engine(False, opts), V, H, B, k, True, "alone", hint=True)
    if name == "planes_shape":
        assert all(ride["planes"] for ride in hinted.fn.engine.rides), "the CD step left the plane path"
    tapped = sf.run_sigma(sf.sigma_engine(True, opts), V, H, B, k, True, "alone", hint=True)
    sf.check_sigma("hinted %s" % name, tapped, REL)            # (rows in units: the rows of THIS minibatch, scaled)
    sf.same_bits(hinted, without, "sigma %s: with the hint against without" % name)
    sf.same_bits(hinted, tapped, "sigma %s: taps off against taps on" % name)


@pytest.mark.parametrize("name,shape,opts,K", SHAPES, ids=[s[0] for s in SHAPES])
def test_next_indexes_changes_nothing_in_a_grouped_step(have_gpu, name, shape, opts, K):
    V, H, B, k = shape
    eng = grouped_engine(opts)
    cap = 3 if name == "small" else sf.draw_cap(B, V, H, k, list(range(0, V + 1, K)))
    without = sf.run_grouped(eng, V, H, B, k, K, False, "plain", hint=False, tapped=False)
    hinted = sf.run_grouped(eng, V, H, B, k, K, False, "plain", hint=True, tapped=False)
    tapped = sf.run_grouped(eng, V, H, B, k, K, False, "plain", hint=True, cap=cap)
    sf.check_grouped("hinted %s" % name, tapped)
    sf.same_bits(hinted, without, "grouped %s: with the hint against without" % name)
    sf.same_bits(hinted, tapped, "grouped %s: taps off against taps on" % name)


# ------------------------------------------------------------------------------------------------------------------ 2. ragged
@pytest.mark.parametrize("variant", ["alone", "centered"])
def test_a_ragged_last_minibatch_in_a_sigma_step(have_gpu, variant):
    """33, 33, 13, 33 rows at batch_size 33: the twin divides by batch_size, uses the rows it got and rho = n / batch_size.  The
    13-row step has staging matrices of its own; rows 13 .. 32 of the 33-row ones hold NaN while it runs."""
    V, H, B, k = SMALL
    eng = sf.sigma_engine(True)
    r = sf.run_sigma(eng, V, H, B, k, True, variant, schedule=sf.RAGGED, poison_idle_rows=True)
    assert sorted(r.fn._sigma_rows) == [13, 33] and [ride["u"].shape[0] for ride in eng.rides] == list(sf.RAGGED)
    assert finite(r), "the 13-row step read rows it does not have"
    for m in r.fn._sigma_rows[33]:
        assert np.isfinite(m.cpu().numpy()).all()          # (the next full step wrote every row again)
    sf.check_sigma("ragged %s" % variant, r, REL)
    assert ("offsets" in r.state) == (variant == "centered")


@pytest.mark.parametrize("mode", ["plain", "both"])
def test_a_ragged_last_minibatch_in_a_grouped_step(have_gpu, mode):
    V, H, B, k = SMALL
    r = sf.run_grouped(grouped_engine(), V, H, B, k, 5, False, mode, schedule=sf.RAGGED)
    assert [V2.shape[0] for V2, _ in r.scratch] == [2 * n for n in sf.RAGGED] and finite(r)
    sf.check_grouped("ragged %s" % mode, r)


# ------------------------------------------------------------------------------------------------------------------ 3. PCD
def test_pcd_with_a_learned_sigma_keeps_its_chain_and_monitors_the_rows_in_units(have_gpu):
    V, H, B, k = SMALL
    eng = sf.sigma_engine(True)
    r = sf.run_sigma(eng, V, H, B, k, True, "alone", persistent=True)      # (chain == recorded nh_sample: asserted every step)
    assert r.plan.persistent is not None and r.rbm.bit_i_idx == sf.STEPS and r.st.bit_i_idx == sf.STEPS
    # in raw units the cost is another number: the bound below is met only by the rows the step trained on
    st0 = rbm_np.RBMState(V, H, W=r.st.W, hbias=r.st.hbias, vbias=r.st.vbias, gauss=True)
    st0.bit_i_idx = 0
    raw, units = r.data[:B].astype(np.float64), r.data[:B].astype(np.float64) * np.exp(-r.ls)[None, :]
    assert abs(rbm_np.pseudo_likelihood_cost(st0, raw) - rbm_np.pseudo_likelihood_cost(st0, units)) > 1e-3
    sf.check_sigma("pcd", r, REL, pcd=True)


# ------------------------------------------------------------------------------------------------------------------ 4. host table
@pytest.mark.parametrize("hint", [False, True], ids=["plain", "hinted"])
@pytest.mark.parametrize("name,shape,opts,K", SHAPES, ids=[s[0] for s in SHAPES])
def test_a_host_resident_table_trains_a_sigma_step_to_the_same_bits(have_gpu, name, shape, opts, K, hint):
    V, H, B, k = shape
    device = sf.run_sigma(sf.sigma_engine(False, opts), V, H, B, k, True, "alone", hint=hint)
    host = sf.run_sigma(sf.sigma_engine(False, opts), V, H, B, k, True, "alone", hint=hint, resident="host")
    assert host.fn._host_table() is not None and host.fn._feed is not None and device.fn._feed is None
    if hint:
        assert host.fn._feed.feeder is not None, "the hint never reached the row feeder"
    sf.same_bits(host, device, "sigma %s: host-resident against device-resident" % name)


@pytest.mark.parametrize("hint", [False, True], ids=["plain", "hinted"])
@pytest.mark.parametrize("name,shape,opts,K", SHAPES, ids=[s[0] for s in SHAPES])
def test_a_host_resident_table_trains_a_grouped_step_to_the_same_bits(have_gpu, name, shape, opts, K, hint):
    V, H, B, k = shape
    eng = grouped_engine(opts)
    device = sf.run_grouped(eng, V, H, B, k, K, False, "plain", hint=hint, tapped=False)
    host = sf.run_grouped(eng, V, H, B, k, K, False, "plain", hint=hint, tapped=False, resident="host")
    assert host.fn._host_table() is not None and host.fn._feed is not None and device.fn._feed is None
    if hint:
        assert host.fn._feed.feeder is not None, "the hint never reached the row feeder"
    sf.same_bits(host, device, "grouped %s: host-resident against device-resident" % name)


# ------------------------------------------------------------------------------------------------------------------ 5. index forms
def test_index_forms_of_a_sigma_step(have_gpu):
    V, H, B, k = SMALL
    runs = {}
    for form in ("int32", "int64", "list"):
        runs[form] = sf.run_sigma(sf.sigma_engine(True), V, H, B, k, True, "alone", index_form=form)
        sf.check_sigma("indexes %s" % form, runs[form], REL)
    sf.same_bits(runs["int32"], runs["int64"], "sigma: int32 against int64 indexes")
    assert not np.array_equal(runs["list"].params["W"], runs["int64"].params["W"])        # (the repeated row is another minibatch)


def test_index_forms_of_a_grouped_step(have_gpu):
    V, H, B, k = SMALL
    runs = {}
    for form in ("int32", "int64", "list"):
        runs[form] = sf.run_grouped(grouped_engine(), V, H, B, k, 5, False, "plain", index_form=form)
        sf.check_grouped("indexes %s" % form, runs[form])
    sf.same_bits(runs["int32"], runs["int64"], "grouped: int32 against int64 indexes")
    assert not np.array_equal(runs["list"].params["W"], runs["int64"].params["W"])


# ------------------------------------------------------------------------------------------------------------------ 6. the DBN
def test_the_first_hidden_layer_of_a_dbn_takes_raw_rows_to_units(hip_engine):
    import mdbn_amd
    mdbn_amd.DBN.verbose = False
    eng = hip_engine
    V, H = 60, 24
    _, x = sf.sigma_table(V, 79)
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, hidden_layers_sizes=[H], n_outs=8, engine=eng)
    net.data_parallel = None
    net.shuffle_rng = np.random.RandomState(3)
    net.training(x, batch_size=33, k=1, pretraining_epochs=[4, 2], pretrain_lr=[0.002, 0.05], learn_sigma=0.05)
    rbm, layer = net.rbm_layers[0], net.sigmoid_layers[0]
    assert layer.log_sigma is rbm.log_sigma and net.sigmoid_layers[1].log_sigma is None and net.rbm_layers[1].log_sigma is None
    s = rbm.log_sigma.get_value().astype(np.float64)
    assert np.abs(s).max() > 1e-3
    W, b = layer.W.get_value().astype(np.float64), layer.b.get_value().astype(np.float64)
    assert np.array_equal(layer.W.get_value(), rbm.W.get_value()) and np.array_equal(layer.b.get_value(), rbm.hbias.get_value())
    want = rbm_np.sigmoid((x.astype(np.float64) * np.exp(-s)[None, :]) @ W + b)
    got = eng.to_numpy(layer.forward(x))
    plain = rbm_np.sigmoid(x.astype(np.float64) @ W + b)
    print("DBN 60 -> 24 -> 8: forward of raw rows %.3e (without the scaling: %.3e)" % (np.abs(got - want).max(), np.abs(got - plain).max()))
    check("dbn sigma: HiddenLayer.forward of raw rows", np.abs(got - want).max(), 2e-6, "prob")
    assert np.abs(got - plain).max() > 1e-3
    assert np.array_equal(net.get_output(x, 0), got)
