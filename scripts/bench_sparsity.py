#!/usr/bin/env python
"""Device time of the CD step with a sparsity target (RBM.get_cost_updates(sparsity_target=, sparsity_cost=)) beside the plain
one, of the centred step with and without it, and of the penalty's pass over the statistics (mdbn_sparsity_stats:
sparsity_stats_kernel, csrc/mdbn_sparsity.hip) beside a device-to-device copy of the same S -- the bar: the kernel reads S
once and writes it once -- and of mdbn_sparsity_activity alone.  Shapes: the headline layer 4096 -> 1024 at B = 512 and the
gene-expression layer 19937 -> 400 at B = 20 (GRBM, CD-1).  Everything alternates in one process, every arm twice (A B A B:
the two A's and the two B's are identical arms, their ratio is the spread of the run); a window is `--inner` calls between two
events, the medians of `--repeats` windows are reported.  The timed kernel runs with every unit at the target (the same loads,
stores and arithmetic; it adds exact zeros, so its buffer comes back bit for bit and a window's calls do not compound).
Writes profiles/sparsity_bench.json with the source hash.
    python scripts/bench_sparsity.py [--repeats 7] [--inner 50]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, mdbn_amd
from mdbn_amd import build

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--inner", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparsity_bench.json"))
args = ap.parse_args()
eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
dev = eng.device
TARGET = 0.2


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


def ratio(s, a, b):
    return s[a]["median_us"] / s[b]["median_us"]


rows = []
for V, H, B in ((4096, 1024, 512), (19937, 400, 20)):
    rs = np.random.RandomState(V)
    N = 4 * B
    data = mdbn_amd.shared(rs.normal(size=(N, V)).astype(np.float32), engine=eng)
    order = [eng.index_tensor(rs.permutation(N)[:B], N) for _ in range(8)]
    steps = {}
    for name, kw in (("plain", {}), ("sparse", dict(sparsity_target=TARGET, sparsity_cost=1.0)), ("centred", dict(centered=True)),
                     ("centred_sparse", dict(centered=True, sparsity_target=TARGET, sparsity_cost=1.0))):
        rbm = mdbn_amd.GRBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(7), engine=eng)
        _, up = rbm.get_cost_updates(lr=1e-4, k=1, lambda_2=0.1, batch_size=B, **kw)
        fn = mdbn_amd.function(up, data, data_parallel=None)
        count = [0]

        def step(fn=fn, count=count):
            t = count[0]
            count[0] = t + 1
            fn(indexes=order[t % 8], momentum=0.5, next_indexes=order[(t + 1) % 8])     # (as the trainers call it)
        steps[name] = step
    names = ("plain", "sparse", "centred", "centred_sparse")
    s = summary(windows(tuple((n + "_a", steps[n]) for n in names) + tuple((n + "_b", steps[n]) for n in names)))
    step_row = dict(arms=s, sparse_over_plain=ratio(s, "sparse_a", "plain_a"),
                    centred_sparse_over_centred=ratio(s, "centred_sparse_a", "centred_a"),
                    spread={n: ratio(s, n + "_b", n + "_a") for n in names})

    # the penalty's pass alone beside a copy of S
    ldv, ldh = mdbn_amd.engine.padded_ld(V), eng.weight_ld(V, H) or mdbn_amd.engine.padded_ld(H)
    stats = eng.new_stats_buffer(V, H, ldv, ldh)
    stats.normal_()
    before = stats.clone()
    S_src, S_dst = stats[:V * ldh], torch.empty(V * ldh, dtype=torch.float32, device=dev)
    q, v_mean = torch.full((H,), TARGET, dtype=torch.float32, device=dev), torch.rand(V, dtype=torch.float32, device=dev)
    sc = eng.cd_scratch(B, V, H, False, ldv, ldh)
    sc.V2.normal_()
    sc.P2.uniform_()
    run_q, run_m = eng.alloc_vector(H), eng.alloc_vector(V)
    full = lambda: eng.sparsity_stats(stats, V, H, ldv, ldh, q, v_mean, TARGET, float(B), float(B))
    arms = (("sparsity_stats_a", full), ("copy_a", lambda: S_dst.copy_(S_src)),
            ("sparsity_stats_b", full), ("copy_b", lambda: S_dst.copy_(S_src)),
            ("sparsity_stats_bias_only", lambda: eng.sparsity_stats(stats, V, H, ldv, ldh, q, None, TARGET, 0.0, float(B))),
            ("sparsity_activity", lambda: eng.sparsity_activity(sc, B, run_q, run_m, 0.1)),
            ("sparsity_activity_hidden_only", lambda: eng.sparsity_activity(sc, B, run_q, None, 0.1)))
    k = summary(windows(arms))
    assert torch.equal(stats.view(torch.int32), before.view(torch.int32)), "units at the target changed the buffer"
    bytes_S = 2.0 * V * H * 4                      # S read once and written once (live columns)
    kern_row = dict(arms=k, ldh=ldh, S_megabytes=V * ldh * 4 / 1e6, extra_floats=V + 2 * H,
                    stats_over_copy=ratio(k, "sparsity_stats_a", "copy_a"),
                    spread_stats=ratio(k, "sparsity_stats_b", "sparsity_stats_a"), spread_copy=ratio(k, "copy_b", "copy_a"),
                    stats_tb_per_s=bytes_S / (k["sparsity_stats_a"]["median_us"] * 1e-6) / 1e12,
                    copy_tb_per_s=2.0 * V * ldh * 4 / (k["copy_a"]["median_us"] * 1e-6) / 1e12)
    rows.append(dict(V=V, H=H, B=B, step=step_row, kernels=kern_row))
    print(json.dumps(rows[-1]))
    del data, stats, before, S_dst

res = dict(source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), inner=args.inner, repeats=args.repeats, shapes=rows)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
print("wrote", args.out)
