#!/usr/bin/env python
"""Device time of the generative delta rule of up-down fine-tuning on a layer with softmax groups
(mdbn_updown_gen_step_grouped): (a) the one-pass kernel (updown_gen_grouped_kernel, csrc/mdbn_updown.hip: ranges on group
boundaries, the softmax in LDS, a second walk over the span rows), (b) the composed path (propdown + grouped softmax + stacked
operands + mdbn_cd_stats + mdbn_apply_update) and (c) the plain one-pass call mdbn_updown_gen_step(gauss = 0) on the same buffers:
(a) / (c) is the price of the two barriers and the second walk.
Shapes at n = 20 rows: 20 000 -> 400 with 4000 groups of K = 5 (a copy-number table: the whole layer is span) and 794 -> 500
with the label block [784, 794).  Method of scripts/bench_updown.py: everything alternates in one process, every arm twice (the
two runs of an arm are identical: their ratio is the spread of the run); a window is `--inner` calls between two events, the
medians of `--repeats` windows are reported.  Writes a JSON with the source hash.
    python scripts/bench_gupdown.py [--repeats 7] [--inner 30] [--out profiles/gupdown_bench.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, mdbn_amd
from mdbn_amd import build
from mdbn_amd.engine import GroupTable

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--inner", type=int, default=30)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gupdown_bench.json"))
args = ap.parse_args()
eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())


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
for V, H, bounds in ((20000, 400, list(range(0, 20001, 5))), (794, 500, [784, 794])):
    rs = np.random.RandomState(V)
    ldh = mdbn_amd.engine.padded_ld(H)
    G, Gs = eng.alloc_matrix(V, H, ldh), eng.alloc_matrix(V, H, ldh)
    G.copy_(torch.from_numpy((rs.normal(0, 1, (V, H)) / np.sqrt(H)).astype(np.float32)))
    c, cs = eng.alloc_vector(V), eng.alloc_vector(V)
    x = (rs.uniform(size=(n, V)) < 0.3).astype(np.float32)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        x[:, lo:hi] = 0.0
        x[np.arange(n), lo + rs.randint(hi - lo, size=n)] = 1.0
    x_lo = eng.to_device(x)
    x_hi = eng.alloc_matrix(n, H, ldh)
    x_hi.copy_(torch.from_numpy((rs.uniform(size=(n, H)) < 0.4).astype(np.float32)))
    groups = GroupTable(eng, np.asarray(bounds, dtype=np.int32))
    # (a rate of 1e-6: the same loads, stores and arithmetic; the matrix stays where it is over thousands of calls)
    rule = (1e-6, 0.0, 0.0, 0.0, 0.5, n, n, 1.0 / n)

    def grouped(path):
        return lambda: eng.updown_gen_step_grouped(x_lo, x_hi, G, Gs, c, cs, groups, *rule, path)

    def plain():
        return eng.updown_gen_step(x_lo, x_hi, G, Gs, c, cs, False, *rule, "fused")
    arms = (("fused_a", grouped("fused")), ("composed_a", grouped("composed")), ("plain_a", plain),
            ("fused_b", grouped("fused")), ("composed_b", grouped("composed")), ("plain_b", plain))
    k = summary(windows(arms))
    rows.append(dict(V=V, H=H, n=n, n_groups=len(bounds) - 1, span=[bounds[0], bounds[-1]], arms=k,
                     matrix_megabytes=V * ldh * 4 / 1e6,
                     fused_over_composed=k["fused_a"]["median_us"] / k["composed_a"]["median_us"], guessed=4.0 / 7.0,
                     fused_over_plain=k["fused_a"]["median_us"] / k["plain_a"]["median_us"],
                     spread_fused=k["fused_b"]["median_us"] / k["fused_a"]["median_us"],
                     spread_composed=k["composed_b"]["median_us"] / k["composed_a"]["median_us"],
                     spread_plain=k["plain_b"]["median_us"] / k["plain_a"]["median_us"]))
    print(json.dumps(rows[-1]))
    del G, Gs

res = dict(source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), inner=args.inner, repeats=args.repeats,
           gen_step_grouped=rows)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
print("wrote", args.out)
