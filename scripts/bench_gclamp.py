#!/usr/bin/env python
"""Device time of a clamped Gibbs run on a layer with categorical visible units (mdbn_gibbs_clamped_grouped) against the
plain run (mdbn_gibbs_clamped, Bernoulli) of the same build at the same V, H and rows, 2000 steps, about half the units held:
100 -> 24 x 170 and 400 -> 40 x 170 in groups of 5 on both paths; 4096 -> 1024 x 512 in groups of 4 on the general path.  Each
run is bracketed by events on its stream (the whole engine call).  The arms alternate A B A B ... over 14 rounds; a figure is
the median of 7 windows (the even rounds), and the A/A column is the plain arm's odd rounds over its even rounds -- what two
identical arms differ by.  Writes profiles/gclamp_bench.json with the source hash.
    python scripts/bench_gclamp.py [--steps 2000]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, mdbn_amd
from mdbn_amd import RngAddr, build
from mdbn_amd.engine import GroupTable

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gclamp_bench.json"))
args = ap.parse_args()
eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
n, burn = args.steps, args.steps // 10
ROUNDS = 14
rows = []
for V, H, B, size, path in ((100, 24, 170, 5, 1), (100, 24, 170, 5, 2), (400, 40, 170, 5, 1), (400, 40, 170, 5, 2),
                            (4096, 1024, 512, 4, 2)):
    rs = np.random.RandomState(0)
    W = eng.to_device(rs.normal(0, 0.5 / np.sqrt(V), (V, H)).astype(np.float32))
    c, b = eng.to_device(rs.normal(0, 0.5, H).astype(np.float32)), eng.to_device(rs.normal(0, 0.5, V).astype(np.float32))
    bounds = np.arange(0, V + 1, size, dtype=np.int32)
    table = GroupTable(eng, bounds)
    cat = rs.randint(size, size=(B, V // size))
    obs = np.zeros((B, V), dtype=np.float32)                     # one-hot groups: a valid state of both layers
    obs[np.arange(B)[:, None], bounds[:-1][None, :] + cat] = 1.0
    mask = np.repeat((rs.uniform(size=(1, V // size)) < 0.5).astype(np.float32), size, axis=1)     # constant on groups
    obs, mask = eng.to_device(obs), eng.to_device(mask)
    rng = RngAddr(1, 0, 0, 0, 0)
    arms = {"plain": lambda: eng.gibbs_clamped(obs, obs, mask, W, c, b, False, n, rng, burn_in=burn, path=path),
            "grouped": lambda: eng.gibbs_clamped_grouped(obs, obs, mask, W, c, b, n, rng, table, burn_in=burn, path=path)}
    ms = {name: [] for name in arms}
    for rnd in range(ROUNDS + 1):                    # (the first round warms up: code objects, allocations)
        for name, run in arms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = run()
            t1.record()
            eng.synchronize()
            assert bool(torch.isfinite(out[4]).all())
            if rnd:
                ms[name].append(t0.elapsed_time(t1))
    med = {name: float(np.median(v[0::2])) for name, v in ms.items()}
    rows.append(dict(V=V, H=H, rows=B, group_size=size, steps=n, path=path, plain_ms=med["plain"], grouped_ms=med["grouped"],
                     grouped_over_plain=med["grouped"] / med["plain"], plain_over_plain=float(np.median(ms["plain"][1::2])) / med["plain"],
                     us_per_step_plain=1e3 * med["plain"] / n, us_per_step_grouped=1e3 * med["grouped"] / n,
                     plain_ms_all=ms["plain"], grouped_ms_all=ms["grouped"]))
    print(json.dumps({k: v for k, v in rows[-1].items() if not k.endswith("_all")}))
out = dict(source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), rounds=ROUNDS, windows_per_median=7, runs=rows)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
