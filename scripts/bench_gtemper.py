#!/usr/bin/env python
"""Device time of a parallel-tempering sweep on a layer with categorical visible units (mdbn_pt_run_grouped) against the plain
run (mdbn_pt_run) of the same build at the same V, H, M ladders and R = 16 temperatures: 100 -> 24 in groups of 5 on the
one-launch path at 512 ladders; 400 -> 40 in groups of 4 on the general path at 512 ladders; 4096 -> 1024 in groups of 4 on the
general path at 64 ladders.  Where the shape fits the one-launch kernel the grouped run is also timed on the OTHER path
(``grouped_other_path_ms``): what the path = 0 choice of a grouped run rests on.  Each run is bracketed by events on its stream
(the whole engine call).  The arms alternate A B A B ... over 14 rounds; a figure is the median of 7 windows (the even
rounds), and the A/A column is the plain arm's odd rounds over its even rounds -- what two identical arms differ by.  Writes
profiles/gtemper_bench.json with the source hash.
    python scripts/bench_gtemper.py [--out profiles/gtemper_bench.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, mdbn_amd
from mdbn_amd import RngAddr, build
from mdbn_amd.engine import GroupTable, padded_ld

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gtemper_bench.json"))
args = ap.parse_args()
eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
R, ROUNDS = 16, 14
betas = np.linspace(0, 1, R).astype(np.float32)
rows = []
for V, H, size, path, M, n in ((100, 24, 5, 1, 512, 200), (400, 40, 4, 2, 512, 100), (4096, 1024, 4, 2, 64, 40)):
    rs = np.random.RandomState(0)
    W = eng.to_device(rs.normal(0, 0.5 / np.sqrt(V), (V, H)).astype(np.float32))
    c, b = eng.to_device(rs.normal(0, 0.5, H).astype(np.float32)), eng.to_device(rs.normal(0, 0.5, V).astype(np.float32))
    bA = eng.to_device(rs.normal(0, 0.3, V).astype(np.float32))
    table = GroupTable(eng, np.arange(0, V + 1, size, dtype=np.int32))
    rng = RngAddr(1, 0, 0, 0, 0)
    v, h = eng.alloc_matrix(M * R, V, padded_ld(V)), eng.alloc_matrix(M * R, H, W.stride(0))
    rank = torch.arange(R, dtype=torch.int32).repeat(M, 1).to(eng.device).contiguous()

    def grouped(p):
        return lambda: eng.temper_grouped(W, c, b, bA, betas, v, h, rank, n, rng, table, burn_in=n // 4, path=p)
    arms = {"plain": lambda: eng.temper(W, c, b, bA, False, betas, v, h, rank, n, rng, burn_in=n // 4, path=path),
            "grouped": grouped(path)}
    other = None
    if V <= 512:                                     # (the shape fits the one-launch kernel: time the grouped run on both paths)
        other = 3 - path
        arms["grouped_other_path"] = grouped(other)
    ms = {name: [] for name in arms}
    for rnd in range(ROUNDS + 1):                    # (the first round warms up: code objects, allocations)
        for name, run in arms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = run()
            t1.record()
            eng.synchronize()
            assert torch.isfinite(out[1]).all()
            if rnd:
                ms[name].append(t0.elapsed_time(t1))
    med = {name: float(np.median(x[0::2])) for name, x in ms.items()}
    row = dict(V=V, H=H, group_size=size, ladders=M, temperatures=R, sweeps=n, path=path, plain_ms=med["plain"], grouped_ms=med["grouped"],
               grouped_over_plain=med["grouped"] / med["plain"], plain_over_plain=float(np.median(ms["plain"][1::2])) / med["plain"],
               us_per_sweep_plain=1e3 * med["plain"] / n, us_per_sweep_grouped=1e3 * med["grouped"] / n,
               plain_ms_all=ms["plain"], grouped_ms_all=ms["grouped"])
    if other is not None:
        row.update(other_path=other, grouped_other_path_ms=med["grouped_other_path"],
                   us_per_sweep_grouped_other_path=1e3 * med["grouped_other_path"] / n, grouped_other_path_ms_all=ms["grouped_other_path"])
    rows.append(row)
    print(json.dumps({k: x for k, x in row.items() if not k.endswith("_all")}))
out = dict(source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), rounds=ROUNDS, windows_per_median=7, runs=rows)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
