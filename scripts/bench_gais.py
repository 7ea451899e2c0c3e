#!/usr/bin/env python
"""Device time of an annealed-importance-sampling run on a layer with categorical visible units (mdbn_ais_run_grouped)
against the plain run (mdbn_ais_run) of the same build at the same V, H, M = 512 chains and K = 1000 temperatures: 400 -> 40
in groups of 5 on the one-launch path; 400 -> 40 and 4096 -> 1024 in groups of 4 on the general path.  Each run is bracketed
by events on its stream (the whole engine call).  The arms alternate A B A B ... over 14 rounds; a figure is the median of 7
windows (the even rounds), and the A/A column is the plain arm's odd rounds over its even rounds -- what two identical arms
differ by.  Writes profiles/gais_bench.json with the source hash.
    python scripts/bench_gais.py [--chains 512] [--temperatures 1000]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, mdbn_amd
from mdbn_amd import RngAddr, build
from mdbn_amd.engine import GroupTable

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=512)
ap.add_argument("--temperatures", type=int, default=1000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gais_bench.json"))
args = ap.parse_args()
eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
M, K = args.chains, args.temperatures
ROUNDS = 14
betas = np.linspace(0, 1, K + 1)
rows = []
for V, H, size, path in ((400, 40, 5, 1), (400, 40, 4, 2), (4096, 1024, 4, 2)):
    rs = np.random.RandomState(0)
    W = eng.to_device(rs.normal(0, 0.5 / np.sqrt(V), (V, H)).astype(np.float32))
    c, b = eng.to_device(rs.normal(0, 0.5, H).astype(np.float32)), eng.to_device(rs.normal(0, 0.5, V).astype(np.float32))
    bA = rs.normal(0, 0.3, V).astype(np.float32)
    table = GroupTable(eng, np.arange(0, V + 1, size, dtype=np.int32))
    rng = RngAddr(1, 0, 0, 0, 0)
    arms = {"plain": lambda: eng.ais(W, c, b, bA, False, betas, M, rng, path=path),
            "grouped": lambda: eng.ais_grouped(W, c, b, bA, betas, M, rng, table, path=path)}
    ms = {name: [] for name in arms}
    for rnd in range(ROUNDS + 1):                    # (the first round warms up: code objects, allocations)
        for name, run in arms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            logw = run()
            t1.record()
            eng.synchronize()
            assert np.isfinite(logw).all()
            if rnd:
                ms[name].append(t0.elapsed_time(t1))
    med = {name: float(np.median(v[0::2])) for name, v in ms.items()}
    rows.append(dict(V=V, H=H, group_size=size, chains=M, temperatures=K, path=path, plain_ms=med["plain"], grouped_ms=med["grouped"],
                     grouped_over_plain=med["grouped"] / med["plain"], plain_over_plain=float(np.median(ms["plain"][1::2])) / med["plain"],
                     us_per_temperature_plain=1e3 * med["plain"] / K, us_per_temperature_grouped=1e3 * med["grouped"] / K,
                     plain_ms_all=ms["plain"], grouped_ms_all=ms["grouped"]))
    print(json.dumps({k: v for k, v in rows[-1].items() if not k.endswith("_all")}))
out = dict(source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), rounds=ROUNDS, windows_per_median=7, runs=rows)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
