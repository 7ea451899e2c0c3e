#!/usr/bin/env python
"""Device time of one clamped Gibbs run (mdbn_gibbs_clamped, csrc/mdbn_clamp.hip) of 2000 steps: 100 -> 24 at 170 and at 1360
rows (8 chains per patient), 400 -> 40 (Gaussian) at 170 rows -- on the one-launch path, on the forced general path, and as
the yardstick the free-running mdbn_gibbs_chain at the same shape and step count (it does strictly less per step: no clamp,
no accumulators).  Each call is bracketed by events on its stream after a warm-up call; the smallest of the repeats counts.
Writes profiles/clamp_bench.json with the source hash: us per step of all three and the ratios.
    python scripts/bench_clamp.py [--steps 2000] [--repeats 3]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, mdbn_amd
from mdbn_amd import RngAddr, build

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clamp_bench.json"))
args = ap.parse_args()
eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
n, burn = args.steps, args.steps // 5
rows = []
for V, H, gauss, B in ((100, 24, False, 170), (100, 24, False, 1360), (400, 40, True, 170)):
    rs = np.random.RandomState(0)
    W = eng.to_device(rs.normal(0, 0.5 / np.sqrt(V), (V, H)).astype(np.float32))
    c, b = eng.to_device(rs.normal(0, 0.5, H).astype(np.float32)), eng.to_device(rs.normal(0, 0.5, V).astype(np.float32))
    obs = eng.to_device(rs.normal(size=(B, V)).astype(np.float32) if gauss else rs.uniform(size=(B, V)).astype(np.float32))
    start = obs if gauss else eng.to_device((rs.uniform(size=(B, V)) < 0.5).astype(np.float32))     # (a free Bernoulli chain starts from 0/1 rows)
    mask = eng.to_device((rs.uniform(size=(B, V)) < 0.5).astype(np.float32))
    calls = {
        "path1": lambda: eng.gibbs_clamped(obs, obs, mask, W, c, b, gauss, n, RngAddr(1, 0, 0, 0, 0), burn_in=burn, path=1),
        "path2": lambda: eng.gibbs_clamped(obs, obs, mask, W, c, b, gauss, n, RngAddr(1, 0, 0, 0, 0), burn_in=burn, path=2),
        "gibbs_chain": lambda: eng.gibbs_chain(start, W, c, b, gauss, n, RngAddr(1, 0, 0, 0, 0), want_pre=False),
    }
    us = {}
    for name, call in calls.items():
        ms = []
        for rep in range(args.repeats + 1):          # (the first run warms up: code objects, allocations)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = call()
            t1.record()
            eng.synchronize()
            if rep:
                ms.append(t0.elapsed_time(t1))
        assert all(bool(torch.isfinite(t).all()) for t in out if t is not None)
        us[name] = dict(us_per_step=1e3 * min(ms) / n, ms_all=ms)
    rows.append(dict(V=V, H=H, gauss=gauss, rows=B, steps=n, burn_in=burn, **us,
                     path2_over_path1=us["path2"]["us_per_step"] / us["path1"]["us_per_step"],
                     gibbs_chain_over_path1=us["gibbs_chain"]["us_per_step"] / us["path1"]["us_per_step"]))
    print(json.dumps(rows[-1]))
out = dict(source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), runs=rows)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
