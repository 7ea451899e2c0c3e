#!/usr/bin/env python
"""Device time of a clamped annealed-importance-sampling run on a layer with categorical visible units
(mdbn_ais_cond_run_grouped) against its two halves from the same build at the same V, H, N = 8 data rows x C = 64 chains and
K = 1000 temperatures: the plain clamped run (mdbn_ais_cond_run, the same mask and observed rows) and the free grouped run
(mdbn_ais_run_grouped at M = N C chains).  400 -> 40 in groups of 5 on both paths; 4096 -> 1024 in groups of 4 on the general
path.  About half the UNITS of every data row are held (a group as a whole).  Each run is bracketed by events on its stream
(the whole engine call).  The arms alternate A B C A B C ... over 14 rounds; a figure is the median of 7 windows (the even
rounds), and the A/A column is the plain clamped arm's odd rounds over its even rounds -- what two identical arms differ by.
Writes profiles/gcais_bench.json with the source hash.
    python scripts/bench_gcais.py [--rows 8] [--chains 64] [--temperatures 1000]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, mdbn_amd
from mdbn_amd import RngAddr, build
from mdbn_amd.engine import GroupTable

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=8)
ap.add_argument("--chains", type=int, default=64)
ap.add_argument("--temperatures", type=int, default=1000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gcais_bench.json"))
args = ap.parse_args()
eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
N, Cn, K = args.rows, args.chains, args.temperatures
ROUNDS = 14
betas = np.linspace(0, 1, K + 1)
rows = []
for V, H, size, path in ((400, 40, 5, 1), (400, 40, 5, 2), (4096, 1024, 4, 2)):
    rs = np.random.RandomState(0)
    W = eng.to_device(rs.normal(0, 0.5 / np.sqrt(V), (V, H)).astype(np.float32))
    c, b = eng.to_device(rs.normal(0, 0.5, H).astype(np.float32)), eng.to_device(rs.normal(0, 0.5, V).astype(np.float32))
    bA = rs.normal(0, 0.3, V).astype(np.float32)
    bounds = np.arange(0, V + 1, size, dtype=np.int32)
    table = GroupTable(eng, bounds)
    # observed rows with one-hot groups and a per-row unit mask: every group held or free as a whole, about half of them held
    obs = np.zeros((N, V), dtype=np.float32)
    obs[np.repeat(np.arange(N), V // size), (bounds[:-1][None, :] + rs.randint(size, size=(N, V // size))).ravel()] = 1.0
    mask = np.repeat((rs.uniform(size=(N, V // size)) < 0.5).astype(np.float32), size, axis=1)
    d_obs, d_mask = eng.to_device(obs), eng.to_device(mask)
    rng = RngAddr(1, 0, 0, 0, 0)
    arms = {"clamped": lambda: eng.ais_conditional(W, c, b, bA, False, betas, d_obs, d_mask, Cn, rng, path=path),
            "grouped": lambda: eng.ais_grouped(W, c, b, bA, betas, N * Cn, rng, table, path=path),
            "clamped_grouped": lambda: eng.ais_conditional_grouped(W, c, b, bA, betas, d_obs, d_mask, Cn, rng, table, path=path)}
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
    rows.append(dict(V=V, H=H, group_size=size, data_rows=N, chains_per_row=Cn, temperatures=K, path=path, held_share=float(mask.mean()),
                     clamped_ms=med["clamped"], grouped_ms=med["grouped"], clamped_grouped_ms=med["clamped_grouped"],
                     over_clamped=med["clamped_grouped"] / med["clamped"], over_grouped=med["clamped_grouped"] / med["grouped"],
                     clamped_over_clamped=float(np.median(ms["clamped"][1::2])) / med["clamped"],
                     us_per_temperature=1e3 * med["clamped_grouped"] / K,
                     clamped_ms_all=ms["clamped"], grouped_ms_all=ms["grouped"], clamped_grouped_ms_all=ms["clamped_grouped"]))
    print(json.dumps({k: v for k, v in rows[-1].items() if not k.endswith("_all")}))
out = dict(source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), rounds=ROUNDS, windows_per_median=7, runs=rows)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
