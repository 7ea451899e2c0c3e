#!/usr/bin/env python
"""Device time of one clamped annealed-importance-sampling run (mdbn_ais_cond_run, csrc/mdbn_ais.hip) beside mdbn_ais_run at
the same number of chains, V, H and K from the same build: what the clamp costs.  N = 16 data rows of C = 64 chains
(N C = 1024), K = 1000 temperatures, a random mask holding about half the columns of every row: 100 -> 24 on the one-launch
path, 1024 -> 256 on the general path (Gaussian and Bernoulli visibles: a Bernoulli layer's held columns may hold real
values, so its propup pass goes without the 0/1 operand hint mdbn_ais_run gives).  The two calls alternate; each run is
bracketed by events on its stream (the whole call, host copy of log w included).  Writes profiles/cais_bench.json with the
source hash.
    python scripts/bench_cais.py [--rows 16] [--chains 64] [--temperatures 1000] [--repeats 7]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, mdbn_amd
from mdbn_amd import RngAddr, build

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=16)
ap.add_argument("--chains", type=int, default=64)
ap.add_argument("--temperatures", type=int, default=1000)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cais_bench.json"))
args = ap.parse_args()
eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
N, C, K = args.rows, args.chains, args.temperatures
betas = np.linspace(0, 1, K + 1)
rows = []
for V, H, gauss, path in ((100, 24, False, 1), (1024, 256, True, 2), (1024, 256, False, 2)):
    rs = np.random.RandomState(0)
    W = eng.to_device(rs.normal(0, 0.5 / np.sqrt(V), (V, H)).astype(np.float32))
    c, b = eng.to_device(rs.normal(0, 0.5, H).astype(np.float32)), eng.to_device(rs.normal(0, 0.5, V).astype(np.float32))
    bA = rs.normal(0, 0.3, V).astype(np.float32)
    obs = eng.to_device(rs.normal(size=(N, V)).astype(np.float32) if gauss else rs.uniform(size=(N, V)).astype(np.float32))
    mask = eng.to_device((rs.uniform(size=(N, V)) < 0.5).astype(np.float32))
    calls = dict(ais=lambda: eng.ais(W, c, b, bA, gauss, betas, N * C, RngAddr(1, 0, 0, 0, 0), path=path),
                 cais=lambda: eng.ais_conditional(W, c, b, bA, gauss, betas, obs, mask, C, RngAddr(1, 0, 0, 0, 0), path=path))
    ms = dict(ais=[], cais=[])
    for rep in range(args.repeats + 1):              # (the first round warms up: code objects, allocations); the two alternate
        for name in ("ais", "cais"):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            logw = calls[name]()
            t1.record()
            eng.synchronize()
            assert np.isfinite(logw).all()
            if rep:
                ms[name].append(t0.elapsed_time(t1))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rows.append(dict(V=V, H=H, gauss=gauss, rows=N, chains_per_row=C, temperatures=K, path=path, ms_all=ms, ms_median=med,
                     ms_min={k: min(v) for k, v in ms.items()},
                     us_per_temperature={k: 1e3 * v / K for k, v in med.items()}, ratio=med["cais"] / med["ais"]))
    print(json.dumps(rows[-1]))
out = dict(source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), runs=rows)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
