#!/usr/bin/env python
"""Device time of the centred CD step (RBM.get_cost_updates(centered=True)) beside the plain one, and of the offset correction
of the statistics (mdbn_center_stats: center_stats_kernel + center_finish_kernel, csrc/mdbn_center.hip) beside a
device-to-device copy of the same S -- the bar: the kernel reads S once and writes it once.  Shapes: the headline layer
4096 -> 1024 at B = 512 and the gene-expression layer 19937 -> 400 at B = 20 (GRBM, CD-1).  Everything alternates in one
process, every arm twice (A B A B: the two A's and the two B's are identical arms, their ratio is the spread of the run);
a window is `--inner` calls between two events, the medians of `--repeats` windows are reported.  The timed kernel runs with
zero offsets (the same loads, stores and arithmetic; its buffer comes back bit for bit, so a window's calls do not compound).
Writes profiles/center_bench.json with the source hash.
    python scripts/bench_center.py [--repeats 7] [--inner 50]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, mdbn_amd
from mdbn_amd import _lib, build

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--inner", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "center_bench.json"))
args = ap.parse_args()
eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
dev = eng.device


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
for V, H, B in ((4096, 1024, 512), (19937, 400, 20)):
    rs = np.random.RandomState(V)
    N = 4 * B
    data = mdbn_amd.shared(rs.normal(size=(N, V)).astype(np.float32), engine=eng)
    order = [eng.index_tensor(rs.permutation(N)[:B], N) for _ in range(8)]
    steps = {}
    for name, centered in (("plain", False), ("centred", True)):
        rbm = mdbn_amd.GRBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(7), engine=eng)
        _, up = rbm.get_cost_updates(lr=1e-4, k=1, lambda_2=0.1, batch_size=B, centered=centered)
        fn = mdbn_amd.function(up, data, data_parallel=None)
        count = [0]

        def step(fn=fn, count=count):
            t = count[0]
            count[0] = t + 1
            fn(indexes=order[t % 8], momentum=0.5, next_indexes=order[(t + 1) % 8])     # (as the trainers call it)
        steps[name] = step
    ms = windows((("plain_a", steps["plain"]), ("centred_a", steps["centred"]), ("plain_b", steps["plain"]), ("centred_b", steps["centred"])))
    s = summary(ms)
    step_row = dict(arms=s, centred_over_plain=s["centred_a"]["median_us"] / s["plain_a"]["median_us"],
                    spread_plain=s["plain_b"]["median_us"] / s["plain_a"]["median_us"],
                    spread_centred=s["centred_b"]["median_us"] / s["centred_a"]["median_us"])

    # the correction alone beside a copy of S
    ldv, ldh = mdbn_amd.engine.padded_ld(V), eng.weight_ld(V, H) or mdbn_amd.engine.padded_ld(H)
    stats = eng.new_stats_buffer(V, H, ldv, ldh)
    stats.normal_()
    before = stats.clone()
    S_src, S_dst = stats[:V * ldh], torch.empty(V * ldh, dtype=torch.float32, device=dev)
    mu, lam = eng.alloc_vector(V), eng.alloc_vector(H)
    sc = eng.cd_scratch(B, V, H, False, ldv, ldh)
    sc.V2.normal_()
    sc.P2.uniform_()
    off_mu, off_lam = eng.alloc_vector(V), eng.alloc_vector(H)
    arms = (("center_stats_a", lambda: eng.center_stats(stats, V, H, ldv, ldh, mu, lam, 1.0)), ("copy_a", lambda: S_dst.copy_(S_src)),
            ("center_stats_b", lambda: eng.center_stats(stats, V, H, ldv, ldh, mu, lam, 1.0)), ("copy_b", lambda: S_dst.copy_(S_src)),
            ("center_offsets", lambda: eng.center_offsets(sc, B, off_mu, off_lam, 0.01)))
    k = summary(windows(arms))
    assert torch.equal(stats.view(torch.int32), before.view(torch.int32)), "zero offsets changed the buffer"
    bytes_S = 2.0 * V * H * 4                      # S read once and written once (live columns)
    kern_row = dict(arms=k, ldh=ldh, S_megabytes=V * ldh * 4 / 1e6,
                    stats_over_copy=k["center_stats_a"]["median_us"] / k["copy_a"]["median_us"],
                    spread_stats=k["center_stats_b"]["median_us"] / k["center_stats_a"]["median_us"],
                    spread_copy=k["copy_b"]["median_us"] / k["copy_a"]["median_us"],
                    stats_tb_per_s=bytes_S / (k["center_stats_a"]["median_us"] * 1e-6) / 1e12,
                    copy_tb_per_s=2.0 * V * ldh * 4 / (k["copy_a"]["median_us"] * 1e-6) / 1e12)
    rows.append(dict(V=V, H=H, B=B, step=step_row, kernels=kern_row))
    print(json.dumps(rows[-1]))
    del data, stats, before, S_dst

res = dict(source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), inner=args.inner, repeats=args.repeats, shapes=rows)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
print("wrote", args.out)
