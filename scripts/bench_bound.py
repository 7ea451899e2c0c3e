#!/usr/bin/env python
"""Device time of the fused propdown + row log-likelihood (mdbn_propdown_rowll, csrc/mdbn_bound.hip) beside the yardstick
it replaces: mdbn_propdown_sample with only the pre-activations asked for (the same products plus the [R, V] store), from the
same build, on the layers of the variational bound.  Three arms alternate in one process: the yardstick, the new kernel and
the yardstick AGAIN (the A/A arm: what the noise alone makes of a ratio); every timed window is `--inner` launches between
two events.  The first 128 rows of the new kernel are compared with the float64 reduction of the yardstick's pre-activations.
Then the time of whole DBN.log_likelihood_bound calls on the AML-shaped stack (19937 -> 400 -> 40, N = 170, S = 64), with log Z
given and with the default AIS run.  Writes profiles/bound_bench.json with the source hash.
    python scripts/bench_bound.py [--repeats 7] [--inner 5] [--skip-stack]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, mdbn_amd
from mdbn_amd import _lib, build

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--skip-stack", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bound_bench.json"))
args = ap.parse_args()
eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
mdbn_amd.DBN.verbose = False
dev = eng.device
rows = []
# (V, H, R, target_div): the bottom layer of the AML stack at 170 patients x 64 samples, and upper-layer shapes
for V, H, R, div in ((19937, 400, 10880, 64), (4096, 1024, 8192, 1), (784, 500, 6400, 1), (100, 24, 10880, 1)):
    g = torch.Generator(device=dev).manual_seed(V + H)
    ldh = eng.weight_ld(V, H) or mdbn_amd.engine.padded_ld(H)
    W = eng.alloc_matrix(V, H, ldh)
    W.copy_(torch.randn((V, H), generator=g, device=dev) / np.sqrt(H))
    h = eng.alloc_matrix(R, H, ldh)
    h.copy_((torch.rand((R, H), generator=g, device=dev) < 0.5).float())
    vb = 0.5 * torch.randn(V, generator=g, device=dev)
    target = eng.alloc_matrix((R + div - 1) // div, V)
    target.copy_((torch.rand(target.shape, generator=g, device=dev) < 0.5).float())
    pre = eng.alloc_matrix(R, V)
    ws = eng.workspace(R, V, H)

    def yardstick():
        _lib.check(eng.lib.mdbn_propdown_sample(eng.ctx, eng._stream(), eng._p(h), R, ldh, eng._p(W), V, H, pre.stride(0), eng._p(vb),
                                                0, 0, eng._p(pre), None, None, None, None, None, eng._p(ws), ws.numel() * 4),
                   "mdbn_propdown_sample")

    out = [eng.alloc_vector(R)]
    nb = C.c_int64()
    _lib.check(eng.lib.mdbn_rowll_workspace_bytes(eng.ctx, R, V, H, C.byref(nb)), "mdbn_rowll_workspace_bytes")
    ws2 = torch.empty(nb.value // 4 + 64, dtype=torch.float32, device=dev)

    def fused():                                     # (both arms are the bare library calls on preallocated buffers)
        _lib.check(eng.lib.mdbn_propdown_rowll(eng.ctx, eng._stream(), eng._p(h), R, ldh, eng._p(W), V, H, eng._p(vb), eng._p(target),
                                               target.stride(0), div, 0, eng._p(out[0]), eng._p(ws2), ws2.numel() * 4),
                   "mdbn_propdown_rowll")

    arms = (("yardstick", yardstick), ("rowll", fused), ("yardstick_again", yardstick))
    ms = {name: [] for name, _ in arms}
    for rep in range(args.repeats + 1):              # (the first round warms up); the arms alternate
        for name, fn in arms:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.inner):
                fn()
            t1.record()
            eng.synchronize()
            if rep:
                ms[name].append(t0.elapsed_time(t1) / args.inner)
    # the same quantity from the yardstick's pre-activations, float64, on the first rows
    n = min(128, R)
    p = pre[:n].double()
    t = target[torch.arange(n, device=dev) // div].double()
    ref = (t * p - torch.nn.functional.softplus(p)).sum(dim=1)
    err = float(((out[0][:n].double() - ref).abs() / ref.abs().clamp(min=1.0)).max())
    assert err <= 1e-4, err
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rows.append(dict(V=V, H=H, R=R, target_div=div, ldh=ldh, ms_all=ms, ms_median=med, ms_min={k: min(v) for k, v in ms.items()},
                     ratio=med["rowll"] / med["yardstick"], ratio_aa=med["yardstick_again"] / med["yardstick"],
                     tflops_alg={k: 2e-9 * R * V * H / v for k, v in med.items()}, worst_rel_error_first_rows=err))
    print(json.dumps(rows[-1]))
    del W, h, target, pre

stack = None
if not args.skip_stack:
    rs = np.random.RandomState(0)
    N, S = 170, 64
    net = mdbn_amd.DBN(numpy_rng=rs, n_ins=19937, gauss=True, hidden_layers_sizes=[400], n_outs=40)
    x = rs.normal(size=(N, 19937)).astype(np.float32)
    stack = dict(sizes=[19937, 400, 40], N=N, S=S, ms_log_z_given=[], ms_default_ais=[])
    for key, kw in (("ms_log_z_given", dict(log_z=0.0)), ("ms_default_ais", dict())):
        for rep in range(4):
            eng.synchronize()
            t0 = time.perf_counter()
            r = net.log_likelihood_bound(x, n_samples=S, **kw)
            eng.synchronize()
            if rep:
                stack[key].append(1e3 * (time.perf_counter() - t0))
        assert np.isfinite(r.rows).all()
    stack["bound"], stack["stderr"], stack["log_z_stderr"] = r.bound, r.stderr, r.log_z_stderr
    print(json.dumps(stack))
res = dict(source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), inner=args.inner, kernels=rows, stack=stack)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
print("wrote", args.out)
