#!/usr/bin/env python
"""Device time of the fused propdown + row log-likelihood of a layer with softmax visible groups (mdbn_propdown_rowll_grouped,
csrc/mdbn_bound.hip) beside (a) the yardstick of scripts/bench_bound.py -- mdbn_propdown_sample with only the pre-activations
asked for, the first step of any composed route -- and (b) mdbn_propdown_rowll (gauss = 0) on the same operands: (c) / (a) says
what fusing buys, (c) / (b) what the grouped epilogue costs.  The arms alternate in one process, the yardstick runs AGAIN as the
A/A arm (what the noise alone makes of a ratio); every timed window is `--inner` launches between two events.  The first 128
rows of (c) are compared with the float64 reduction of the yardstick's pre-activations.  Writes profiles/gbound_bench.json with
the source hash.
    python scripts/bench_gbound.py [--repeats 7] [--inner 5]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, mdbn_amd
from mdbn_amd import _lib, build
from mdbn_amd.engine import GroupTable

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gbound_bench.json"))
args = ap.parse_args()
eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
dev = eng.device
rows = []
# (V, H, R, target_div, first grouped column, K): a copy-number table of 4000 genes x 5 states at 170 patients x 64 samples;
# 1024 groups of 4; the label block behind 784 pixels.  The groups run from their first column to V.
for V, H, R, div, lo, K in ((20000, 400, 10880, 64, 0, 5), (4096, 1024, 8192, 1, 0, 4), (794, 500, 6400, 1, 784, 10)):
    g = torch.Generator(device=dev).manual_seed(V + H)
    ldh = eng.weight_ld(V, H) or mdbn_amd.engine.padded_ld(H)
    W = eng.alloc_matrix(V, H, ldh)
    W.copy_(torch.randn((V, H), generator=g, device=dev) / np.sqrt(H))
    h = eng.alloc_matrix(R, H, ldh)
    h.copy_((torch.rand((R, H), generator=g, device=dev) < 0.5).float())
    vb = 0.5 * torch.randn(V, generator=g, device=dev)
    n_t, G = (R + div - 1) // div, (V - lo) // K
    t = (torch.rand((n_t, V), generator=g, device=dev) < 0.5).float()
    codes = torch.randint(K, (n_t, G, 1), generator=g, device=dev)
    t[:, lo:] = torch.zeros((n_t, G, K), device=dev).scatter_(2, codes, 1.0).reshape(n_t, G * K)
    target = eng.alloc_matrix(n_t, V)
    target.copy_(t)
    table = GroupTable(eng, np.arange(lo, V + 1, K, dtype=np.int32))
    pre = eng.alloc_matrix(R, V)
    ws = eng.workspace(R, V, H)

    def yardstick():
        _lib.check(eng.lib.mdbn_propdown_sample(eng.ctx, eng._stream(), eng._p(h), R, ldh, eng._p(W), V, H, pre.stride(0), eng._p(vb),
                                                0, 0, eng._p(pre), None, None, None, None, None, eng._p(ws), ws.numel() * 4),
                   "mdbn_propdown_sample")

    out, out_g = eng.alloc_vector(R), eng.alloc_vector(R)
    nb = C.c_int64()
    _lib.check(eng.lib.mdbn_rowll_workspace_bytes(eng.ctx, R, V, H, C.byref(nb)), "mdbn_rowll_workspace_bytes")
    ws2 = torch.empty(nb.value // 4 + 64, dtype=torch.float32, device=dev)
    _lib.check(eng.lib.mdbn_rowll_grouped_workspace_bytes(eng.ctx, R, V, H, C.byref(nb)), "mdbn_rowll_grouped_workspace_bytes")
    ws3 = torch.empty(nb.value // 4 + 64, dtype=torch.float32, device=dev)

    def plain():                                     # (all arms are the bare library calls on preallocated buffers)
        _lib.check(eng.lib.mdbn_propdown_rowll(eng.ctx, eng._stream(), eng._p(h), R, ldh, eng._p(W), V, H, eng._p(vb), eng._p(target),
                                               target.stride(0), div, 0, eng._p(out), eng._p(ws2), ws2.numel() * 4),
                   "mdbn_propdown_rowll")

    def grouped():
        _lib.check(eng.lib.mdbn_propdown_rowll_grouped(eng.ctx, eng._stream(), eng._p(h), R, ldh, eng._p(W), V, H, eng._p(vb),
                                                       eng._p(target), target.stride(0), div, eng._p(out_g), eng._p(ws3),
                                                       ws3.numel() * 4, eng._p(table.tensor), C.c_void_p(table.host.ctypes.data),
                                                       table.n_groups), "mdbn_propdown_rowll_grouped")

    arms = (("yardstick", yardstick), ("rowll", plain), ("rowll_grouped", grouped), ("yardstick_again", yardstick))
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
    tt = target[torch.arange(n, device=dev) // div].double()
    ref = (tt[:, :lo] * p[:, :lo] - torch.nn.functional.softplus(p[:, :lo])).sum(dim=1)
    ref = ref + (tt[:, lo:] * p[:, lo:]).sum(dim=1) - torch.logsumexp(p[:, lo:].reshape(n, G, K), dim=2).sum(dim=1)
    err = float(((out_g[:n].double() - ref).abs() / ref.abs().clamp(min=1.0)).max())
    assert err <= 1e-4, err
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rows.append(dict(V=V, H=H, R=R, target_div=div, ldh=ldh, first_group_column=lo, K=K, n_groups=G, ms_all=ms, ms_median=med,
                     ms_min={k: min(v) for k, v in ms.items()}, ratio_grouped_to_yardstick=med["rowll_grouped"] / med["yardstick"],
                     ratio_grouped_to_rowll=med["rowll_grouped"] / med["rowll"], ratio_rowll_to_yardstick=med["rowll"] / med["yardstick"],
                     ratio_aa=med["yardstick_again"] / med["yardstick"],
                     tflops_alg={k: 2e-9 * R * V * H / v for k, v in med.items()}, worst_rel_error_first_rows=err))
    print(json.dumps(rows[-1]))
    del W, h, target, pre, t

res = dict(source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), inner=args.inner, kernels=rows)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
print("wrote", args.out)
