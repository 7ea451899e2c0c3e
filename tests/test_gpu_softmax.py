"""Categorical visible units on the device: (a) the kernel of csrc/mdbn_groups.hip alone against the float64 twin
(tests/_softmax_np.py) fed the same host-made pre-activations -- means, row sums, one 1 per group, samples outside ties, the
cost, poisoned pad columns, determinism, G = 0 against mdbn_propdown_sample, every MDBN_EINVAL case; (b) whole grouped steps
through the public classes against the twin loop teacher-forced along the device's recorded chain, group_posterior, and a
resumed run."""
import ctypes as C

import numpy as np
import pytest

import _softmax_np as sm
import _step_forms as sf
from _margins import check
from oracle import rbm_np

pytestmark = pytest.mark.gpu

POISON = float("nan")
PARAMS = ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed")


def bits(t):
    return t.detach().cpu().numpy().view(np.int32).copy()


def padded(eng, a, ldv, fill=POISON):
    """Device matrix [B, V] over storage [B, ldv] whose pad columns hold ``fill``."""
    import torch
    full = np.full((a.shape[0], ldv), fill, dtype=np.float32)
    full[:, :a.shape[1]] = a
    return torch.from_numpy(full).to(eng.device)


def kernel_call(eng, table, pre, ldv, mean=None, sample=None, tap=None, v0=None, cost=None, ws=None, seed=0, n_groups=None,
                dev_table=True, host_table=True, ws_bytes=None, V=None, B=None, ctx="engine", rng=True):
    from mdbn_amd import RngAddr
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    r = RngAddr(seed, sm.STREAM, sm.STEP, sm.DRAW, sm.ROW_OFFSET).c()
    return eng.lib.mdbn_group_softmax_sample(
        eng.ctx if ctx == "engine" else ctx, eng._stream(), p(pre), pre.shape[0] if B is None else B, ldv,
        V if V is not None else pre.shape[1],
        p(table.tensor) if (table is not None and dev_table) else None,
        C.c_void_p(table.host.ctypes.data) if (table is not None and host_table) else None,
        (table.n_groups if table is not None else 0) if n_groups is None else n_groups, p(mean), p(sample), p(tap),
        C.byref(r) if rng else None, p(v0), p(cost), p(ws), (ws.numel() * 4 if ws is not None else 0) if ws_bytes is None else ws_bytes)


# ------------------------------------------------------------------------------------------------------------------ (a) the kernel
@pytest.mark.parametrize("V,ldv,bounds,B", sm.KERNEL_CASES, ids=["%dx%d" % (c[3], c[0]) for c in sm.KERNEL_CASES])
def test_kernel_against_the_twin(hip_engine, V, ldv, bounds, B):
    import torch
    from mdbn_amd.engine import GroupTable
    eng = hip_engine
    pre, v0, U, seed = sm.case_inputs(V, ldv, bounds, B)
    table = GroupTable(eng, bounds)
    need = C.c_int64()
    assert eng.lib.mdbn_group_softmax_workspace_bytes(eng.ctx, B, V, C.byref(need)) == 0 and need.value >= 4

    def run():
        d = dict(pre=padded(eng, pre, ldv), mean=padded(eng, np.zeros_like(pre), ldv), sample=padded(eng, np.zeros_like(pre), ldv),
                 tap=padded(eng, np.zeros_like(pre), ldv), v0=padded(eng, v0, ldv),
                 cost=torch.full((4,), 7.0, dtype=torch.float32, device=eng.device),
                 ws=torch.zeros(need.value // 4, dtype=torch.float32, device=eng.device))
        assert kernel_call(eng, table, d["pre"][:, :V], ldv, d["mean"], d["sample"], d["tap"], d["v0"], d["cost"], d["ws"], seed=seed) == 0
        eng.synchronize()
        return d
    d = run()
    got = {k: d[k].cpu().numpy() for k in ("pre", "mean", "sample", "tap", "cost")}
    mean, _, _ = sm.grouped_softmax(pre, bounds)
    tag = "group_softmax B=%d V=%d" % (B, V)
    err = np.abs(got["mean"][:, :V] - mean).max()
    sums = [np.abs(got["mean"][:, lo:hi].astype(np.float64).sum(axis=1) - 1.0).max() / (hi - lo) for lo, hi in sm.spans(bounds)]
    want_cost = sm.grouped_cost(pre, v0, bounds)
    print("%s: mean %.3e, row sums / K %.3e, cost rel %.3e" % (tag, err, max(sums), abs(got["cost"][0] - want_cost) / abs(want_cost)))
    check(tag + ": mean", err, sm.MEAN_TOL, "prob")
    check("group_softmax: |sum of a group's means - 1| / K", max(sums), 6e-8)
    own = sm.grouped_sample(mean, bounds, U)
    _, differ = sm.follow(own, got["sample"][:, :V], mean, bounds, U, what=tag)
    assert differ <= sm.TIE_CAP, "%d draws differ from the twin's" % differ
    assert np.array_equal(got["tap"][:, :V], got["sample"][:, :V])
    check(tag + ": cost rel", abs(got["cost"][0] - want_cost) / abs(want_cost), 1e-5)
    assert np.isfinite(got["cost"][0]) and (got["cost"][1:] == 0).all()
    # pad columns: never read (finite results), never written (bit-unchanged NaN); the input untouched
    for k in ("mean", "sample", "tap"):
        assert np.isfinite(got[k][:, :V]).all(), k
        assert np.isnan(got[k][:, V:]).all() and np.array_equal(got[k][:, V:].view(np.int32), np.full((B, ldv - V), POISON, np.float32).view(np.int32)), k
    assert np.array_equal(got["pre"][:, :V], pre)
    # two runs: bit-identical
    again = run()
    for k in ("mean", "sample", "tap", "cost"):
        assert np.array_equal(bits(again[k]), bits(d[k])), k
    # in place (mean = pre), without sample and cost: the same means
    inplace = padded(eng, pre, ldv)
    assert kernel_call(eng, table, inplace[:, :V], ldv, mean=inplace, rng=False) == 0
    eng.synchronize()
    assert np.array_equal(inplace.cpu().numpy()[:, :V], got["mean"][:, :V]) and np.isnan(inplace.cpu().numpy()[:, V:]).all()


@pytest.mark.parametrize("B,V,H", [(5, 7, 3), (33, 70, 24), (20, 794, 64)])
def test_without_groups_the_kernel_is_the_bernoulli_epilogue_bit_for_bit(hip_engine, B, V, H):
    import torch
    from mdbn_amd import RngAddr
    eng = hip_engine
    rs = np.random.RandomState(V)
    W = eng.to_device(rs.normal(size=(V, H)).astype(np.float32))
    vb = eng.to_device(rs.normal(size=V).astype(np.float32))
    h = eng.to_device((rs.uniform(size=(B, H)) < 0.5).astype(np.float32))
    rng = RngAddr(5, sm.STREAM, sm.STEP, sm.DRAW, sm.ROW_OFFSET)
    _, want_mean, want_sample = eng.propdown(h, W, vb, gauss=False, rng=rng)
    lin = eng.propdown(h, W, vb, gauss=True)[1]
    ldv = lin.stride(0)
    mean, sample = eng.alloc_matrix(B, V, ldv), eng.alloc_matrix(B, V, ldv)
    assert kernel_call(eng, None, lin, ldv, mean, sample, seed=5) == 0
    assert np.array_equal(bits(mean), bits(want_mean)) and np.array_equal(bits(sample), bits(want_sample))


def test_every_einval_case_returns_without_touching_its_outputs(hip_engine):
    import torch
    from mdbn_amd import _lib
    from mdbn_amd.engine import GroupTable
    eng = hip_engine
    V, ldv, B = 70, 72, 5
    pre = padded(eng, np.random.RandomState(1).normal(size=(B, V)).astype(np.float32), ldv, fill=0.0)
    outs = [torch.full((B, ldv), 3.0, dtype=torch.float32, device=eng.device) for _ in range(3)]
    v0 = torch.zeros((B, ldv), dtype=torch.float32, device=eng.device)
    cost = torch.full((4,), 7.0, dtype=torch.float32, device=eng.device)
    ws = torch.full((256,), 9.0, dtype=torch.float32, device=eng.device)
    good = GroupTable(eng, [1, 3, 67, 70])

    def table(bounds):
        t = GroupTable.__new__(GroupTable)
        t.host = np.ascontiguousarray(bounds, dtype=np.int32)
        t.tensor = torch.from_numpy(t.host.copy()).to(eng.device)
        t.n_groups = t.host.size - 1
        return t

    def call(tab=good, **kw):
        full = dict(mean=outs[0], sample=outs[1], tap=outs[2], v0=v0, cost=cost, ws=ws, V=V)
        full.update(kw)
        return kernel_call(eng, tab, pre[:, :V], ldv, **full)

    before = [bits(t) for t in outs + [cost, ws]]
    bad = [dict(tab=table([1, 3, 3, 70])), dict(tab=table([1, 2, 66, 70])), dict(tab=table([0, 66, 70])), dict(tab=table([3, 1, 67, 70])),
           dict(tab=table([1, 3, 67, 71])), dict(tab=table([-1, 3, 67, 70])), dict(tab=table([0, 65, 70])),
           dict(dev_table=False), dict(host_table=False), dict(n_groups=-1), dict(n_groups=40),
           dict(B=0), dict(V=0), dict(V=73), dict(ctx=None), dict(rng=False), dict(v0=None), dict(cost=None), dict(ws=None),
           dict(ws_bytes=0), dict(mean=outs[0].reshape(-1)[1:]), dict(cost=ws[1:5])]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert _lib.last_error(), kw
    eng.synchronize()
    assert all(np.array_equal(a, bits(t)) for a, t in zip(before, outs + [cost, ws])), "a refused call wrote something"
    assert call() == 0 and call(tab=table([0, 64, 70])) == 0              # ... and the good calls go through (K = 64 is served)
    eng.synchronize()
    assert not np.array_equal(bits(outs[0]), before[0])

    # the step driver: a Gaussian layer, sample statistics and a bad table are refused before anything is written
    import mdbn_amd
    from mdbn_amd import RngAddr
    H = 8
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(3), engine=eng, visible_groups=[1, 3, 67, 70])
    data = eng.to_device(sm.one_hot_data(np.random.RandomState(2), B, V, [1, 3, 67, 70]))
    call_ = eng._cd_args(data, None, rbm.W.tensor, rbm.hbias.tensor, rbm.vbias.tensor, False, 1, RngAddr(1, 1, 0), None, False, 0, keep_f32=True)
    a, sc = call_.args, call_.scratch
    call_.stats.fill_(5.0)
    for t in (sc.V2, sc.P2, sc.hs, sc.vs):
        t.fill_(4.0)
    kept = [bits(t) for t in (call_.stats, sc.V2, sc.P2, sc.hs, sc.vs)]

    def step(tab=good, **fields):
        saved = {k: getattr(a, k) for k in fields}
        for k, v in fields.items():
            setattr(a, k, v)
        rc = eng.lib.mdbn_cd_step_grouped(eng.ctx, eng._stream(), C.byref(a), C.c_void_p(tab.tensor.data_ptr()),
                                          C.c_void_p(tab.host.ctypes.data), tab.n_groups)
        for k, v in saved.items():
            setattr(a, k, v)
        return rc
    for kw in (dict(gauss=1), dict(sample_stats=1), dict(tab=table([1, 3, 3, 70])), dict(tab=table([0, 65, 70])), dict(tab=table([1, 3, 67, 71])),
               dict(k=0), dict(vs=None), dict(struct_size=8)):
        assert step(**kw) == -1, kw
        assert _lib.last_error(), kw
    assert step(workspace_bytes=1024) == -3                                  # MDBN_ENOSPC, likewise before any launch
    eng.synchronize()
    assert all(np.array_equal(k, bits(t)) for k, t in zip(kept, (call_.stats, sc.V2, sc.P2, sc.hs, sc.vs))), "a refused step wrote something"
    assert step() == 0
    eng.synchronize()
    assert np.array_equal(sc.V2.cpu().numpy()[:B], data.cpu().numpy())


@pytest.mark.parametrize("B,V,H,groups", [(1, 7, 3, [0, 3, 5]), (33, 70, 24, [1, 3, 67, 70]), (512, 1024, 256, list(range(0, 1025, 4)))])
def test_centred_hidden_statistic_from_the_rows_against_the_twin(hip_engine, B, V, H, groups):
    """mdbn_center_hidden_rows: s_h' = s_h - rho S'^T mu formed from the rows of the scratch, against the float64 twin on the
    device's own inputs; bound and scale of tests/test_gpu_center.py's s_h' check (1e-5 of rho max_j sum_r |d_r P2_rj| here)."""
    import torch
    import types
    eng = hip_engine
    rs = np.random.RandomState(B + V)
    ldv, ldh, rho = (V + 3) & ~3, (H + 3) & ~3, 20.0 / 32.0
    v0, nv = sm.one_hot_data(rs, B, V, groups), sm.grouped_softmax(2 * rs.normal(size=(B, V)), groups)[0].astype(np.float32)
    ph, nh = rs.uniform(size=(B, H)).astype(np.float32), rs.uniform(size=(B, H)).astype(np.float32)
    mu, lam = v0.mean(axis=0).astype(np.float32) if B > 1 else rs.uniform(size=V).astype(np.float32), rs.uniform(size=H).astype(np.float32)
    V2, P2 = padded(eng, np.concatenate([v0, nv]), ldv), padded(eng, np.concatenate([ph, -nh]), ldh)
    st = np.full(V * ldh + ldh + ldv + 4, POISON, dtype=np.float32)
    s_h, s_v = rs.normal(size=H).astype(np.float32) * B, rs.normal(size=V).astype(np.float32)
    st[V * ldh:V * ldh + H], st[V * ldh + ldh:V * ldh + ldh + V] = s_h, s_v
    stats = torch.from_numpy(st).to(eng.device)
    sc = types.SimpleNamespace(V2=V2[:, :V], P2=P2[:, :H])
    dmu, dlam = torch.from_numpy(mu).to(eng.device), torch.from_numpy(lam).to(eng.device)
    got = eng.center_hidden_rows(sc, B, stats, V, H, ldv, ldh, dmu, dlam, rho)
    want = sm.center_hidden_rows(v0, nv, ph, nh, s_h, s_v, mu, lam, rho)
    d = np.concatenate([(v0.astype(np.float64) - mu) @ mu, (nv.astype(np.float64) - mu) @ mu])
    scale = rho * (np.abs(d)[:, None] * np.abs(np.concatenate([ph, nh]))).sum(axis=0).max() + np.abs(s_h).max()
    assert np.isfinite(got.cpu().numpy()).all(), "a pad column was read"
    check("center_hidden_rows %dx%d B=%d: s_h' / scale" % (V, H, B), np.abs(got.cpu().numpy() - want).max() / scale, 1e-5, "stats")
    assert np.array_equal(bits(stats), st.view(np.int32)), "the statistics were written"
    again = eng.center_hidden_rows(sc, B, stats, V, H, ldv, ldh, dmu, dlam, rho)
    assert np.array_equal(bits(again), bits(got)), "two runs differ"
    # ... after a sparsity transform of the statistics: its share of S'^T mu, through the weights and through the biases only
    q, vm = rs.uniform(size=H).astype(np.float32), v0.mean(axis=0).astype(np.float32)
    dq, dvm = torch.from_numpy(q).to(eng.device), torch.from_numpy(vm).to(eng.device)
    for w_scale, b_scale, v_mean in ((0.05 * 32, 0.05 * B, dvm), (0.0, 0.05 * B, None)):
        got_s = eng.center_hidden_rows(sc, B, stats, V, H, ldv, ldh, dmu, dlam, rho, sparsity=(dq, v_mean, 0.1, w_scale, b_scale))
        want_s = sm.center_hidden_rows(v0, nv, ph, nh, s_h, s_v, mu, lam, rho, sparsity=(q, vm if v_mean is not None else None, 0.1, w_scale, b_scale))
        extra = rho * abs(w_scale * float(vm.astype(np.float64) @ mu) - b_scale * float(mu.astype(np.float64) @ mu))
        check("center_hidden_rows %dx%d B=%d after sparsity: s_h' / scale" % (V, H, B), np.abs(got_s.cpu().numpy() - want_s).max() / (scale + extra),
              1e-5, "stats")
    # refused calls leave the output alone
    out = torch.full((H,), 3.0, dtype=torch.float32, device=eng.device)
    ws = torch.zeros(2 * B + 8, dtype=torch.float32, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(V2=V2, P2=P2, B=B, V=V, H=H, ldv=ldv, ldh=ldh, stats=stats, mu=dmu, lam=dlam, rho=rho, out=out, ws=ws, ws_bytes=None, ctx=eng.ctx):
        return eng.lib.mdbn_center_hidden_rows(ctx, eng._stream(), p(V2), ldv, p(P2), ldh, B, V, H, p(stats), p(mu), p(lam), rho, None, None, 0.0, 0.0, 0.0, p(out),
                                               p(ws), (ws.numel() * 4 if ws is not None else 0) if ws_bytes is None else ws_bytes)
    for kw in (dict(B=0), dict(V=0), dict(H=0), dict(ldv=V - 1), dict(ldh=ldh + 2), dict(V2=None), dict(P2=None), dict(stats=None),
               dict(mu=None), dict(lam=None), dict(out=None), dict(ws=None), dict(ctx=None), dict(rho=0.0), dict(rho=float("nan")),
               dict(ws_bytes=8 * B)):
        assert call(**kw) == -1, kw
    eng.synchronize()
    assert (out.cpu().numpy() == 3.0).all(), "a refused call wrote something"
    assert call() == 0
    eng.synchronize()
    assert np.array_equal(bits(out), bits(got))


# ------------------------------------------------------------------------------------------------------------------ (b) whole steps
STEPS = 4
LABEL = [784, 794]
CASES = [  # id, V, H, B, k, boundaries (int: every visible in groups of K), persistent, mode
    ("cd1_60x24_k5", 60, 24, 33, 1, 5, False, "plain"),
    ("cd2_label_block", 794, 64, 20, 2, LABEL, False, "plain"),
    ("pcd1_200x40_k4", 200, 40, 20, 1, 4, True, "plain"),
    ("cd1_1024x256_k4", 1024, 256, 512, 1, 4, False, "plain"),
    ("cd1_1024x256_k4_centered", 1024, 256, 512, 1, 4, False, "centered"),
    ("cd1_1024x256_k4_sparse", 1024, 256, 512, 1, 4, False, "sparse"),
    ("cd1_1024x256_k4_centered_sparse", 1024, 256, 512, 1, 4, False, "both"),
    ("cd1_1024x256_k4_centered_sparse_bias_only", 1024, 256, 512, 1, 4, False, "both_bias"),
    ("cd1_60x24_k5_centered_sparse", 60, 24, 33, 1, 5, False, "both"),
]
HP = sf.GROUPED_HP
assert HP == dict(lr=0.1, weightcost=2e-4) and sf.STEPS == STEPS
_run = sf.run_grouped           # (the whole-step loop lives in tests/_step_forms.py)


@pytest.mark.parametrize("name,V,H,B,k,groups,persistent,mode", CASES, ids=[c[0] for c in CASES])
def test_grouped_steps_against_the_teacher_forced_twin(built_lib, name, V, H, B, k, groups, persistent, mode):
    """Four steps through the public classes against the float64 loop, at tests/test_gpu_center.py's bounds.  The centred
    case takes s_h' from the rows of the scratch (mdbn_center_hidden_rows): through S, the sum over 1024 rows weighted by
    mu_i ~ 1/4 multiplies the float32 error of S 256-fold and hbias_speed came to 2.2e-6 against the 2e-6 bound."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mdbn_amd
    eng = mdbn_amd.HipEngine()                      # product defaults
    r = _run(eng, V, H, B, k, groups, persistent, mode)
    rbm, data = r.rbm, r.data
    assert [p for p, _ in r.errs] == list(PARAMS)
    sf.check_grouped(name, r)                       # (every figure printed, then 2e-6 on each parameter and speed)
    if name == "cd2_label_block":
        # the class prediction of the label block: exact p(label | pixels) against the twin's float64 enumeration
        rows = data[:16]
        got = rbm.group_posterior(rows, 0)
        s = rbm_np.RBMState(V, H, W=rbm.W.get_value(), hbias=rbm.hbias.get_value(), vbias=rbm.vbias.get_value())
        neg_F = np.empty((16, 10))
        for c in range(10):
            x = rows.astype(np.float64).copy()
            x[:, 784:] = 0.0
            x[:, 784 + c] = 1.0
            neg_F[:, c] = -rbm_np.free_energy(s, x)
        want = np.exp(neg_F - neg_F.max(axis=1, keepdims=True))
        want /= want.sum(axis=1, keepdims=True)
        # (a softmax moves by at most the largest error of its arguments, and SURVEY 8d gives a float32 free energy 1e-4 of
        #  its size)
        scale = np.abs(neg_F).max()
        check("group_posterior: probabilities / max|F|", np.abs(got - want).max() / scale, 1e-4, "free_energy")
        assert got.shape == (16, 10) and np.allclose(got.sum(axis=1), 1.0, atol=1e-12)


def test_a_resumed_grouped_run_continues_bit_for_bit(hip_engine, tmp_path):
    import mdbn_amd
    from mdbn_amd import checkpoint
    mdbn_amd.DBN.verbose = False
    eng = hip_engine
    V, H, K = 60, 24, 5
    x = sm.one_hot_data(np.random.RandomState(0), 40, V, list(range(0, V + 1, K)))
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), n_ins=V, gauss=False, hidden_layers_sizes=[], n_outs=H, engine=eng,
                       visible_groups=K)
    rbm = net.rbm_layers[0]
    _, up = rbm.get_cost_updates(0.05, k=1, weightcost=2e-4, batch_size=10)
    fn = mdbn_amd.function(up, mdbn_amd.shared(x, engine=eng), data_parallel=None)
    for t in range(2):
        fn(indexes=np.arange(10) + 10 * t, momentum=0.5)
    path = str(tmp_path / "grouped.npz")
    checkpoint.save_network(path, {'cn': net}, resume=True)
    want = [float(fn(indexes=np.arange(10) + 10 * t, momentum=0.5)) for t in (2, 3)]
    r2 = checkpoint.load_network(path, engine=eng)['cn'].rbm_layers[0]
    assert r2.visible_groups.host.tolist() == list(range(0, V + 1, K))
    _, up2 = r2.get_cost_updates(0.05, k=1, weightcost=2e-4, batch_size=10)
    fn2 = mdbn_amd.function(up2, mdbn_amd.shared(x, engine=eng), data_parallel=None)
    got = [float(fn2(indexes=np.arange(10) + 10 * t, momentum=0.5)) for t in (2, 3)]
    assert got == want
    for n in PARAMS:
        assert np.array_equal(getattr(r2, n).get_value(), getattr(rbm, n).get_value()), n
    # eager sampling on the device: one 1 per group, and the chain call equals the eager calls
    out = r2.gibbs_vhv_chain(x[:7], 2)
    s = out[5].get_value()
    assert (s.reshape(7, V // K, K).sum(axis=2) == 1).all() and np.allclose(out[4].get_value().reshape(7, V // K, K).sum(axis=2), 1.0, atol=1e-6)
