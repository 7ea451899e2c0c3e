#!/usr/bin/env python
"""Device time of a parallel-tempering sweep (mdbn_pt_run, csrc/mdbn_temper.hip) at R = 16 temperatures: 100 -> 24 (Bernoulli)
and 400 -> 40 (Gaussian) with M = 64 and 512 ladders, on the one-launch path AND on the forced general path.  Each case runs
in a child process of its own under a time limit (the parent never opens the GPU, and stops at the first case that fails);
a run is bracketed by events on its stream, best of --repeats after a warm-up.  Writes profiles/temper_bench.json with the
source hash.
    python scripts/bench_temper.py [--sweeps 400] [--repeats 3]"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--sweeps", type=int, default=400)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--temperatures", type=int, default=16)
ap.add_argument("--timeout", type=int, default=120, help="seconds one case may take")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temper_bench.json"))
ap.add_argument("--one", nargs=5, metavar=("V", "H", "GAUSS", "M", "PATH"), help="(child) measure one case and print its JSON line")
args = ap.parse_args()


def one(V, H, gauss, M, path):
    import numpy as np, torch, mdbn_amd
    from mdbn_amd import RngAddr
    from mdbn_amd.engine import padded_ld
    eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
    R, n = args.temperatures, args.sweeps
    rs = np.random.RandomState(0)
    W = eng.to_device(rs.normal(0, 0.5 / np.sqrt(V), (V, H)).astype(np.float32))
    c, b = eng.to_device(rs.normal(0, 0.5, H).astype(np.float32)), eng.to_device(rs.normal(0, 0.5, V).astype(np.float32))
    bA = eng.to_device(rs.normal(0, 0.3, V).astype(np.float32))
    betas = np.linspace(0, 1, R).astype(np.float32)
    v, h = eng.alloc_matrix(M * R, V, padded_ld(V)), eng.alloc_matrix(M * R, H, W.stride(0))
    rank = torch.arange(R, dtype=torch.int32).repeat(M, 1).to(eng.device).contiguous()
    ms = []
    for rep in range(args.repeats + 1):          # (the first run warms up: code objects, allocations)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        accepted = eng.temper(W, c, b, bA, gauss, betas, v, h, rank, n, RngAddr(1, 0, 3 * n * rep, 0, 0), sweep0=n * rep, path=path)[0]
        t1.record()
        eng.synchronize()
        if rep:
            ms.append(t0.elapsed_time(t1))
    tries = M * n * (R - 1) / 2.0
    return dict(V=V, H=H, gauss=bool(gauss), ladders=M, temperatures=R, sweeps=n, path=path, ms_min=min(ms), ms_all=ms,
                us_per_sweep=1e3 * min(ms) / n, acceptance=float(accepted.sum().item() / tries),
                device=torch.cuda.get_device_name(0))


if args.one:
    V, H, gauss, M, path = (int(x) for x in args.one)
    print("RESULT " + json.dumps(one(V, H, gauss, M, path)))
    sys.exit(0)

from mdbn_amd import build
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
            rows.append(json.loads(line[0][7:]))
            print(json.dumps(rows[-1]))
for a, g in zip(rows[0::2], rows[1::2]):
    print("%d->%d M=%d: one launch %.1f us / sweep, general %.1f us / sweep, ratio %.1f"
          % (a["V"], a["H"], a["ladders"], a["us_per_sweep"], g["us_per_sweep"], g["us_per_sweep"] / a["us_per_sweep"]))
out = dict(source_hash=build.source_hash(), runs=rows)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
