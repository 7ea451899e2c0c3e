#!/usr/bin/env python
"""Device time of the generative delta rule of up-down fine-tuning (mdbn_updown_gen_step): the one-pass kernel
(updown_gen_kernel, csrc/mdbn_updown.hip: G and its speed read once and written once) beside the composed path (propdown +
stacked operands + mdbn_cd_stats + mdbn_apply_update: about seven passes over the matrix) and beside two device-to-device
copies that move the same four streams (G and the speed, each copied once by torch's `copy_`: two reads, two writes; no kernel
of this library, two launches, and at these sizes served partly from the 256 MB Infinity Cache, so a reference for the memory
system, not an HBM figure) -- the byte count predicts fused / composed = 4 / 7.
Shapes: the gene-expression layer 19937 -> 400 and 784 -> 500, n = 20 rows.  Then the whole up-down step of a 19937 -> 400 ->
40 DBN at batch 20 on both paths.  Method of scripts/bench_center.py: everything alternates in one process, every arm twice
(A B A B: the two A's and the two B's are identical arms, their ratio is the spread of the run); a window is `--inner` calls
between two events, the medians of `--repeats` windows are reported.  Writes a JSON with the source hash.
    python scripts/bench_updown.py [--repeats 7] [--inner 30] [--out profiles/updown_bench.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, mdbn_amd
from mdbn_amd import build, updown

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--inner", type=int, default=30)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "updown_bench.json"))
args = ap.parse_args()
eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
dev = eng.device
mdbn_amd.DBN.verbose = False


def windows(arms):
    """{arm: [ms per call of every window]}: the arms alternate, the first round warms up."""
    ms = {name: [] for name, _ in arms}
    for rep in range(args.repeats + 1):
        for name, fn in arms:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.inner):
                fn()
            t1.record()
            eng.synchronize()
            if rep:
                ms[name].append(t0.elapsed_time(t1) / args.inner)
    return ms


def summary(ms):
    return {k: dict(median_us=1e3 * float(np.median(v)), min_us=1e3 * min(v), max_us=1e3 * max(v)) for k, v in ms.items()}


rows = []
n = 20
for V, H in ((19937, 400), (784, 500)):
    rs = np.random.RandomState(V)
    ldh = mdbn_amd.engine.padded_ld(H)
    G, Gs = eng.alloc_matrix(V, H, ldh), eng.alloc_matrix(V, H, ldh)
    G.copy_(torch.from_numpy((rs.normal(0, 1, (V, H)) / np.sqrt(H)).astype(np.float32)))
    c, cs = eng.alloc_vector(V), eng.alloc_vector(V)
    x_lo = eng.to_device(rs.normal(size=(n, V)).astype(np.float32))
    x_hi = eng.alloc_matrix(n, H, ldh)
    x_hi.copy_(torch.from_numpy((rs.uniform(size=(n, H)) < 0.4).astype(np.float32)))
    t1, t2 = torch.empty_like(G._base), torch.empty_like(Gs._base)

    def gen(path):
        # (a rate of 1e-6: the same loads, stores and arithmetic; the matrix stays where it is over thousands of calls)
        return lambda: eng.updown_gen_step(x_lo, x_hi, G, Gs, c, cs, True, 1e-6, 0.0, 0.0, 0.0, 0.5, n, n, 1.0 / n, path)

    def copy4():
        t1.copy_(G._base)
        t2.copy_(Gs._base)
    arms = (("fused_a", gen("fused")), ("composed_a", gen("composed")), ("copy4_a", copy4),
            ("fused_b", gen("fused")), ("composed_b", gen("composed")), ("copy4_b", copy4))
    k = summary(windows(arms))
    four = 4.0 * V * H * 4
    rows.append(dict(V=V, H=H, n=n, arms=k, matrix_megabytes=V * ldh * 4 / 1e6,
                     fused_over_composed=k["fused_a"]["median_us"] / k["composed_a"]["median_us"], predicted=4.0 / 7.0,
                     fused_over_copy4=k["fused_a"]["median_us"] / k["copy4_a"]["median_us"],
                     spread_fused=k["fused_b"]["median_us"] / k["fused_a"]["median_us"],
                     spread_composed=k["composed_b"]["median_us"] / k["composed_a"]["median_us"],
                     spread_copy4=k["copy4_b"]["median_us"] / k["copy4_a"]["median_us"],
                     fused_tb_per_s=four / (k["fused_a"]["median_us"] * 1e-6) / 1e12,
                     copy4_tb_per_s=four / (k["copy4_a"]["median_us"] * 1e-6) / 1e12))
    print(json.dumps(rows[-1]))
    del G, Gs, t1, t2

# the whole step of a 19937 -> 400 -> 40 DBN at batch 20
rs = np.random.RandomState(1)
data = eng.to_device(rs.normal(size=(n, 19937)).astype(np.float32))
steps = {}
for path in ("fused", "composed"):
    net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(2), theano_rng=mdbn_amd.RandomStreams(3), n_ins=19937, gauss=True,
                       hidden_layers_sizes=[400], n_outs=40, engine=eng)
    hp = updown.Hyper(1e-6, 1e-6, 1, 0.5, 0.0, 0.0, 0.0, n, path)
    steps[path] = (lambda net=net, hp=hp: updown.step([net], None, [data], hp))
s = summary(windows((("fused_a", steps["fused"]), ("composed_a", steps["composed"]), ("fused_b", steps["fused"]),
                     ("composed_b", steps["composed"]))))
step_row = dict(shape="19937-400-40", batch=n, arms=s, fused_over_composed=s["fused_a"]["median_us"] / s["composed_a"]["median_us"],
                spread_fused=s["fused_b"]["median_us"] / s["fused_a"]["median_us"],
                spread_composed=s["composed_b"]["median_us"] / s["composed_a"]["median_us"])
print(json.dumps(step_row))

res = dict(source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), inner=args.inner, repeats=args.repeats,
           gen_step=rows, whole_step=step_row)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
print("wrote", args.out)
