#!/usr/bin/env python
"""Device time of the learned per-column variance of a Gaussian layer: the two kernels of csrc/mdbn_sigma.hip beside a
device-to-device copy that moves the same bytes (mdbn_sigma_scale_rows reads B V floats and writes B V: one copy of a [B, V]
matrix; mdbn_sigma_update reads 2 B V floats and writes 2 V: the same copy, which reads B V and writes B V), the extra propdown of
a learning step alone (ph_mean -> the conditional means), and the step of a GRBM with log_sigma, frozen and learned, beside the
plain step taken in the same order -- statistics, then update (StepFunction._statistics_step without a transform:
mdbn_cd_step(keep_f32 = 1) + mdbn_apply_update).  Shapes: 19 937 -> 400 at B = 20 (the widest expression table) and the headline
layer 4096 -> 1024 at B = 512.  Everything alternates in one process, every arm twice (A B A B: the ratio of two identical arms
is the spread of the run); a window is `--inner` calls between two events, the medians of `--repeats` windows are reported.
Writes profiles/sigma_bench.json with the source hash.
    python scripts/bench_sigma.py [--repeats 7] [--inner 50]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, mdbn_amd
from mdbn_amd import build

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--inner", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sigma_bench.json"))
args = ap.parse_args()
eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
LO, HI = mdbn_amd.GRBM.log_sigma_range


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


def abab(name_a, fn_a, name_b, fn_b):
    """-> (arms, median of a, median of b, b over a, spread of a, spread of b)"""
    s = summary(windows(((name_a + "_a", fn_a), (name_b + "_a", fn_b), (name_a + "_b", fn_a), (name_b + "_b", fn_b))))
    a, b = s[name_a + "_a"]["median_us"], s[name_b + "_a"]["median_us"]
    return dict(arms=s, **{name_a + "_us": a, name_b + "_us": b, name_b + "_over_" + name_a: b / a,
                           "spread_" + name_a: s[name_a + "_b"]["median_us"] / a, "spread_" + name_b: s[name_b + "_b"]["median_us"] / b})


rows = []
for V, H, B in ((19937, 400, 20), (4096, 1024, 512)):
    rs = np.random.RandomState(V)
    N = 4 * B
    data = mdbn_amd.shared((rs.normal(size=(N, V)) * np.exp(rs.uniform(-1, 1, size=V))[None, :]).astype(np.float32), engine=eng)
    ld = data.tensor.stride(0)
    order = [eng.index_tensor(rs.permutation(N)[:B], N) for _ in range(8)]
    log_sigma = torch.from_numpy(rs.uniform(-1, 1, size=V).astype(np.float32)).to(eng.device)
    speed = eng.alloc_vector(V)
    U, M, T = eng.alloc_matrix(B, V, ld), eng.alloc_matrix(B, V, ld), eng.alloc_matrix(B, V, ld)
    U.normal_()
    M.normal_(0.0, 0.3)
    floats = float(B) * V
    # ---- the kernels alone, beside a copy of the same bytes (the copy walks the padded rows: ld = V or V + 3 at most)
    k_scale = abab("copy", lambda: T.copy_(U), "scale", lambda: eng.sigma_scale_rows(data.tensor, order[0], log_sigma, -1.0, out=T))
    k_scale["scale_tb_per_s"] = 2 * 4 * floats / (k_scale["scale_us"] * 1e-6) / 1e12
    k_scale["copy_tb_per_s"] = 2 * 4 * floats / (k_scale["copy_us"] * 1e-6) / 1e12
    k_update = abab("copy", lambda: T.copy_(U), "update", lambda: eng.sigma_update(U, M, B, 0.0, 0.5, LO, HI, log_sigma, speed))
    k_update["update_tb_per_s"] = 2 * 4 * floats / (k_update["update_us"] * 1e-6) / 1e12
    # ---- the step: statistics, then update -- plain, with a frozen sigma, with a learned one
    steps = {}
    for name, sigma, learn in (("plain", None, None), ("frozen", 1.0, None), ("learned", None, 1e-4)):
        rbm = mdbn_amd.GRBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(7), engine=eng)
        if sigma is not None:
            rbm.set_sigma(sigma)
        _, up = rbm.get_cost_updates(lr=1e-5, k=1, lambda_2=0.1, batch_size=B, learn_sigma=learn)
        fn = mdbn_amd.function(up, data, data_parallel=None)
        count = [0]

        def step(fn=fn, count=count, rbm=rbm):
            t = count[0]
            count[0] = t + 1
            fn._statistics_step(fn._minibatch(order[t % 8]), rbm._take_step(), 1e-5, 0.5, B, None)
        steps[name] = step
        step()
        if name == "learned":       # the extra propdown of a learning step alone: ph_mean of the scratch -> conditional means
            sc, W, vbias = eng.last_scratch, rbm.W.tensor, rbm.vbias.tensor
            k_down = abab("copy", lambda: T.copy_(U), "propdown", lambda: eng.propdown(sc.P2[:B], W, vbias, gauss=True, out=M))
    s_frozen = abab("plain", steps["plain"], "frozen", steps["frozen"])
    s_learned = abab("plain", steps["plain"], "learned", steps["learned"])
    price = dict(scale_us=s_frozen["frozen_us"] - s_frozen["plain_us"], learned_us=s_learned["learned_us"] - s_learned["plain_us"],
                 kernel_scale_us=k_scale["scale_us"], kernel_propdown_us=k_down["propdown_us"], kernel_update_us=k_update["update_us"])
    rows.append(dict(V=V, H=H, B=B, scale_rows=k_scale, sigma_update=k_update, propdown=k_down, step_frozen=s_frozen,
                     step_learned=s_learned, price=price))
    print(json.dumps(rows[-1]))
    del data, U, M, T

res = dict(source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), inner=args.inner, repeats=args.repeats, shapes=rows)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
print("wrote", args.out)
