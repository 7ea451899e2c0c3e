#!/usr/bin/env python
"""Device time of one annealed-importance-sampling run (mdbn_ais_run, csrc/mdbn_ais.hip) at M = 512 chains and K = 1000
temperatures: 400 -> 40 and 100 -> 24 on the one-launch path AND on the forced general path (the same shape: what the
per-temperature launches cost), 4096 -> 1024 on the general path.  Each run is bracketed by events on its stream (the whole
call: the one-launch path has no GEMM launch for the library's GEMM timers to see); for the general path the sum of the
library's GEMM timers (mdbn_kernel_timing) is recorded beside it.  Writes profiles/ais_bench.json with the source hash.
    python scripts/bench_ais.py [--chains 512] [--temperatures 1000] [--repeats 3]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, mdbn_amd
from mdbn_amd import RngAddr, build

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=512)
ap.add_argument("--temperatures", type=int, default=1000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ais_bench.json"))
args = ap.parse_args()
eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
M, K = args.chains, args.temperatures
betas = np.linspace(0, 1, K + 1)
rows = []
for V, H, gauss, paths in ((400, 40, False, (1, 2)), (100, 24, False, (1, 2)), (4096, 1024, True, (2,))):
    rs = np.random.RandomState(0)
    W = eng.to_device(rs.normal(0, 0.5 / np.sqrt(V), (V, H)).astype(np.float32))
    c, b = eng.to_device(rs.normal(0, 0.5, H).astype(np.float32)), eng.to_device(rs.normal(0, 0.5, V).astype(np.float32))
    bA = rs.normal(0, 0.3, V).astype(np.float32)
    for path in paths:
        ms, gemm_ms, n_gemm = [], 0.0, 0
        for rep in range(args.repeats + 1):          # (the first run warms up: code objects, allocations)
            timed = path == 2 and rep == args.repeats
            eng.kernel_timing(timed)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            logw = eng.ais(W, c, b, bA, gauss, betas, M, RngAddr(1, 0, 0, 0, 0), path=path)
            t1.record()
            eng.synchronize()
            if timed:
                n_gemm, gemm_ms = eng.kernel_timing_read()
                eng.kernel_timing(False)
            if rep:
                ms.append(t0.elapsed_time(t1))
        assert np.isfinite(logw).all()
        rows.append(dict(V=V, H=H, gauss=gauss, chains=M, temperatures=K, path=path, ms_min=min(ms), ms_all=ms,
                         us_per_temperature=1e3 * min(ms) / K, gemm_launches_timed=int(n_gemm), gemm_ms_timed=float(gemm_ms),
                         log_Z=mdbn_amd.ais_estimate(logw, bA, H, gauss)))
        print(json.dumps(rows[-1]))
out = dict(source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), runs=rows)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
