#!/usr/bin/env python
"""Device time of the categorical visible units: the grouped softmax kernel (mdbn_group_softmax_sample, csrc/mdbn_groups.hip;
means and samples, no cost) beside device-to-device copies that write the same two matrices, and the grouped CD-1 step
(RBM(visible_groups=K)) beside the plain Bernoulli step taken in the same order -- statistics, then update
(StepFunction._statistics_step without a transform: mdbn_cd_step(keep_f32 = 1) + mdbn_apply_update), and the same two layers
with centered=True (the grouped plan adds mdbn_center_hidden_rows to the centred step).  Shapes: 100 000 columns
in groups of 5 at B = 20 (a copy-number table) and 4096 columns in groups of 4 at B = 512.  The kernel reads one matrix and
writes two (3 B V floats); the copy arm is two copies of the input (2 read, 2 written: 4 B V floats), both rates are printed.
Everything alternates in one process, every arm twice (A B A B: the ratio of two identical arms is the spread of the run); a
window is `--inner` calls between two events, the medians of `--repeats` windows are reported.  Also the GEMM launches per
step that the library's timing hook counts.  Writes profiles/softmax_bench.json with the source hash.
    python scripts/bench_softmax.py [--repeats 7] [--inner 50]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, mdbn_amd
from mdbn_amd import _lib, build
from mdbn_amd.engine import GroupTable

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--inner", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax_bench.json"))
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


def one_hot(rs, N, V, K):
    x = np.zeros((N, V // K, K), dtype=np.float32)
    np.put_along_axis(x, rs.randint(K, size=(N, V // K, 1)), 1.0, axis=2)
    return x.reshape(N, V)


rows = []
for V, K, H, B in ((100000, 5, 400, 20), (4096, 4, 1024, 512)):
    rs = np.random.RandomState(V)
    # ---- the kernel alone
    table = GroupTable(eng, np.arange(0, V + 1, K))
    pre = eng.alloc_matrix(B, V)
    pre.normal_(0.0, 2.0)
    mean, sample = eng.alloc_matrix(B, V), eng.alloc_matrix(B, V)
    rng = mdbn_amd.RngAddr(7, 1, 0, 1, 0).c()
    p = lambda t: C.c_void_p(t.data_ptr())

    def kernel():
        _lib.check(eng.lib.mdbn_group_softmax_sample(eng.ctx, eng._stream(), p(pre), B, pre.stride(0), V, p(table.tensor),
                                                     C.c_void_p(table.host.ctypes.data), table.n_groups, p(mean), p(sample), None,
                                                     C.byref(rng), None, None, None, 0), "mdbn_group_softmax_sample")

    def copies():
        mean.copy_(pre)
        sample.copy_(pre)
    k = summary(windows((("softmax_a", kernel), ("copies_a", copies), ("softmax_b", kernel), ("copies_b", copies))))
    floats = float(B) * V
    kern_row = dict(arms=k, kernel_over_copies=k["softmax_a"]["median_us"] / k["copies_a"]["median_us"],
                    spread_kernel=k["softmax_b"]["median_us"] / k["softmax_a"]["median_us"],
                    spread_copies=k["copies_b"]["median_us"] / k["copies_a"]["median_us"],
                    kernel_tb_per_s=3 * 4 * floats / (k["softmax_a"]["median_us"] * 1e-6) / 1e12,
                    copies_tb_per_s=4 * 4 * floats / (k["copies_a"]["median_us"] * 1e-6) / 1e12)
    # ---- the step: statistics, then update, with and without groups
    N = 4 * B
    data = mdbn_amd.shared(one_hot(rs, N, V, K), engine=eng)
    order = [eng.index_tensor(rs.permutation(N)[:B], N) for _ in range(8)]
    steps, launches = {}, {}
    for name, groups, centered in (("plain", None, False), ("grouped", K, False), ("plain_centred", None, True), ("grouped_centred", K, True)):
        rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(7), engine=eng,
                           visible_groups=groups)
        _, up = rbm.get_cost_updates(lr=1e-4, k=1, weightcost=2e-4, batch_size=B, centered=centered)
        fn = mdbn_amd.function(up, data, data_parallel=None)
        count = [0]

        def step(fn=fn, count=count, rbm=rbm):
            t = count[0]
            count[0] = t + 1
            fn._statistics_step(fn._minibatch(order[t % 8]), rbm._take_step(), 1e-4, 0.5, B, None)
        steps[name] = step
        step()
        eng.kernel_timing(True)
        for _ in range(4):
            step()
        launches[name] = eng.kernel_timing_read()[0] / 4.0
        eng.kernel_timing(False)
    s = summary(windows((("plain_a", steps["plain"]), ("grouped_a", steps["grouped"]), ("plain_b", steps["plain"]), ("grouped_b", steps["grouped"]))))
    step_row = dict(arms=s, grouped_over_plain=s["grouped_a"]["median_us"] / s["plain_a"]["median_us"],
                    spread_plain=s["plain_b"]["median_us"] / s["plain_a"]["median_us"],
                    spread_grouped=s["grouped_b"]["median_us"] / s["grouped_a"]["median_us"], gemm_launches_per_step=launches)
    # ... and with centered=True: the grouped plan adds the row route to s_h' (mdbn_center_hidden_rows) to the centred step
    c = summary(windows((("plain_centred_a", steps["plain_centred"]), ("grouped_centred_a", steps["grouped_centred"]),
                         ("plain_centred_b", steps["plain_centred"]), ("grouped_centred_b", steps["grouped_centred"]))))
    step_row["centred"] = dict(arms=c, grouped_over_plain=c["grouped_centred_a"]["median_us"] / c["plain_centred_a"]["median_us"],
                               grouped_centred_over_grouped=c["grouped_centred_a"]["median_us"] / s["grouped_a"]["median_us"],
                               spread_plain=c["plain_centred_b"]["median_us"] / c["plain_centred_a"]["median_us"],
                               spread_grouped=c["grouped_centred_b"]["median_us"] / c["grouped_centred_a"]["median_us"])
    rows.append(dict(V=V, K=K, H=H, B=B, kernel=kern_row, step=step_row))
    print(json.dumps(rows[-1]))
    del data, pre, mean, sample

res = dict(source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), inner=args.inner, repeats=args.repeats, shapes=rows)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
print("wrote", args.out)
