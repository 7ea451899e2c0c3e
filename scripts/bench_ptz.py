#!/usr/bin/env python
"""What recording the works costs (mdbn_pt_run_z beside mdbn_pt_run, csrc/mdbn_temper.hip): device time of a parallel-tempering
sweep with and without the accumulators at the cases of profiles/temper_bench.json -- R = 16 temperatures, 100 -> 24
(Bernoulli) and 400 -> 40 (Gaussian), M = 64 and 512 ladders, the one-launch path and the forced general path.  Each case runs
in a child process of its own under a time limit (the parent never opens the GPU, and stops at the first case that fails).
In a child the two versions alternate (plain, works, plain, works, ...) after a warm-up of each, every run bracketed by events
on its stream; the minimum and every repeat are kept.  Writes profiles/ptz_bench.json with the source hash and, beside each
case, the us per sweep profiles/temper_bench.json holds for it (measured before the works existed).
    python scripts/bench_ptz.py [--sweeps 4000] [--repeats 5]"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--sweeps", type=int, default=4000)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--temperatures", type=int, default=16)
ap.add_argument("--timeout", type=int, default=120, help="seconds one case may take")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ptz_bench.json"))
ap.add_argument("--one", nargs=5, metavar=("V", "H", "GAUSS", "M", "PATH"), help="(child) measure one case and print its JSON line")
args = ap.parse_args()


def one(V, H, gauss, M, path):
    import numpy as np, torch, mdbn_amd
    from mdbn_amd import RngAddr
    from mdbn_amd.engine import padded_ld
    from mdbn_amd.temper import new_works
    eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
    R, n = args.temperatures, args.sweeps
    rs = np.random.RandomState(0)
    W = eng.to_device(rs.normal(0, 0.5 / np.sqrt(V), (V, H)).astype(np.float32))
    c, b = eng.to_device(rs.normal(0, 0.5, H).astype(np.float32)), eng.to_device(rs.normal(0, 0.5, V).astype(np.float32))
    bA = eng.to_device(rs.normal(0, 0.3, V).astype(np.float32))
    betas = np.linspace(0, 1, R).astype(np.float32)
    v, h = eng.alloc_matrix(M * R, V, padded_ld(V)), eng.alloc_matrix(M * R, H, W.stride(0))
    rank = torch.arange(R, dtype=torch.int32).repeat(M, 1).to(eng.device).contiguous()
    zacc = torch.from_numpy(new_works(M, R)).to(eng.device)
    ms = {False: [], True: []}
    for rep in range(2 * (args.repeats + 1)):    # (the first run of each version warms up: code objects, allocations)
        works = bool(rep & 1)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        eng.temper(W, c, b, bA, gauss, betas, v, h, rank, n, RngAddr(1, 0, 3 * n * rep, 0, 0), sweep0=n * rep, path=path,
                   **(dict(zacc=zacc) if works else {}))
        t1.record()
        eng.synchronize()
        if rep >= 2:
            ms[works].append(t0.elapsed_time(t1))
    assert bool(torch.isfinite(zacc).all())
    us = {k: 1e3 * min(x) / n for k, x in ms.items()}
    return dict(V=V, H=H, gauss=bool(gauss), ladders=M, temperatures=R, sweeps=n, path=path, us_per_sweep=us[False],
                us_per_sweep_works=us[True], overhead=us[True] / us[False] - 1.0, ms_all=ms[False], ms_all_works=ms[True],
                device=torch.cuda.get_device_name(0))


if args.one:
    V, H, gauss, M, path = (int(x) for x in args.one)
    print("RESULT " + json.dumps(one(V, H, gauss, M, path)))
    sys.exit(0)

from mdbn_amd import build
before = {}
try:
    with open(os.path.join(ROOT, "profiles", "temper_bench.json")) as fh:
        before = {(r["V"], r["H"], r["ladders"], r["path"]): r["us_per_sweep"] for r in json.load(fh)["runs"]}
except (OSError, ValueError, KeyError):
    pass
rows = []
for V, H, gauss in ((100, 24, 0), (400, 40, 1)):
    for M in (64, 512):
        for path in (1, 2):
            cmd = [sys.executable, os.path.abspath(__file__), "--sweeps", str(args.sweeps), "--repeats", str(args.repeats),
                   "--temperatures", str(args.temperatures), "--one", str(V), str(H), str(gauss), str(M), str(path)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=args.timeout, universal_newlines=True)
            line = [l for l in r.stdout.split("\n") if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                sys.exit("case %r failed (exit %d): nothing more is started\n%s" % (cmd[-5:], r.returncode, r.stdout[-2000:]))
            row = json.loads(line[0][7:])
            row["us_per_sweep_temper_bench"] = before.get((V, H, M, path))
            rows.append(row)
            print("%d->%d M=%d path %d: %.2f us / sweep, with the works %.2f (%+.1f %%); temper_bench.json: %s"
                  % (V, H, M, path, row["us_per_sweep"], row["us_per_sweep_works"], 100 * row["overhead"],
                     "%.2f" % row["us_per_sweep_temper_bench"] if row["us_per_sweep_temper_bench"] else "-"), flush=True)
out = dict(source_hash=build.source_hash(), runs=rows)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
