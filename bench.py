#!/usr/bin/env python
"""Headline benchmark: CD-1 training steps of the Gaussian-Bernoulli RBM 4096 -> 1024 at
batch 512 per GPU (BASELINE.json configs[1]; configs[2] with N > 1 ranks).

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]

With --gpus N > 1 and no torchrun environment this process starts the N ranks itself
(`python -m torch.distributed.run --nnodes=1 --nproc-per-node N ...` as a CHILD process, before
anything here has touched the GPU) and relays rank 0's JSON line; under torchrun it is a rank.

One "step" = one call of the compiled step function of reference src/rbm.py:258-376 as
src/dbn.py:302-312 builds it: minibatch gather, positive phase, one gibbs_hvh, the
statistics GEMM, (all-reduce over ranks,) parameter update and monitoring cost -- nothing
skipped.  Inputs are synthetic N(0,1) rows already resident in HBM, generated from fixed seeds.

A plain run sets up, lets the GPU settle for 1 s on a throwaway model (`settle`), runs W warm-up
steps, times ONE window of exactly K steps (the product's default setting; --windows M: M windows,
`ms_per_step` is their median), bracketed by barrier + synchronize on both sides (max over ranks),
and prints ONE JSON line on rank 0.
--dump-outputs DIR: what the last timed step left to its caller -- the monitoring cost and the
updated parameters and speeds -- as DIR/<name>.npy (float32; the cost float64), about 32 MB.
--full adds everything else, as before: >= 5 windows and >= 6 s of timed steps on one GPU (more
windows for short ones, so that a small K gives the same number as a long run); `roofline`
(per-kernel HIP-event times against the matrix pipe each kernel issues on); the exact-f32 MFMA,
bf16-input and host-resident-table variants; the free-energy check against the float64 oracle;
`cpu_baseline` (the numpy float32 oracle on the host cores: Theano is not installable offline,
so kind "port"); with N > 1 the data-parallel sweep (whose fastest point becomes `value`), the
all-reduce alone and the exposed-communication probe.
"""
import argparse
import glob
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

V, H, B_PER_GPU, N_DATA, K_GIBBS = 4096, 1024, 512, 32768, 1
LR, LAMBDA_1, LAMBDA_2 = 0.001, 0.0, 0.1          # lr 0.005 (MDBN.py:49) diverges on this synthetic shape; see DESIGN.md
MFMA_F32_PEAK_TFLOPS = 157.3                      # MI355X_MICROARCH.md: f32-input MFMA, dense
MFMA_BF16_PEAK_TFLOPS = 2500.0                    # MI355X_MICROARCH.md: bf16 MFMA, dense
KIND_NAMES = {1: "propup", 0: "propdown", 3: "statistics"}   # 2 * la + lb of mdbn_kernel_timing_detail


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--windows", type=int, default=0,
                    help="timed windows of --steps steps (0 = auto: one in a plain run, >= 5 with --full)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the cost, parameters and speeds after the last timed step as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also the roofline, the other precisions and configurations, the oracle check, the CPU baseline "
                         "and (N > 1) the data-parallel sweep; the headline then takes >= 5 windows")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--default-only", action="store_true",
                    help="only the default (product) path: no exact-f32 / bf16-input re-runs, no CPU baseline (profiling runs)")
    ap.add_argument("--no-sweep", action="store_true", help="N > 1: keep the default data-parallel setting, no comm_cus sweep")
    ap.add_argument("--sweep-capi", action="store_true",
                    help="N > 1: also sweep with the all-reduce issued through the C-ABI communicator (mdbn_allreduce_stats); off "
                         "by default: it is the same RCCL collective, and a second communicator that failed to build on one "
                         "rank would hang the run that matters")
    ap.add_argument("--sweep-budget", type=float, default=float(os.environ.get("MDBN_BENCH_SWEEP_BUDGET_S", "150")),
                    help="N > 1: wall seconds the whole sweep may take (points that no longer fit are reported as skipped); "
                         "the default setting is always timed first and is what a watchdog prints if anything later hangs")
    ap.add_argument("--no-cta-sweep", action="store_true",
                    help="N > 1 on RCCL: skip the second sweep stage (communicators capped at 8 / 16 / 32 channels)")
    return ap.parse_args()


def launch_ranks(args):
    """Start the N ranks as a child torchrun job and relay its output.  Nothing in this process
    has initialised the GPU (torch is not even imported yet), and the parent only waits."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__),
           "--gpus", str(args.gpus), "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--windows", str(args.windows)]
    if args.full:
        cmd.append("--full")
    if args.dump_outputs:
        cmd += ["--dump-outputs", args.dump_outputs]
    if args.no_cpu_baseline:
        cmd.append("--no-cpu-baseline")
    if args.default_only:
        cmd.append("--default-only")
    if args.no_sweep:
        cmd.append("--no-sweep")
    if args.sweep_capi:
        cmd.append("--sweep-capi")
    if args.no_cta_sweep:
        cmd.append("--no-cta-sweep")
    cmd += ["--sweep-budget", str(args.sweep_budget)]
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    for line in proc.stdout:
        sys.stdout.write(line)
        sys.stdout.flush()
    return proc.wait()


def pmc_traffic(rows=None):
    """HBM bytes per CD STEP, summed over every kernel of the step, from the newest committed PMC profile of the
    default path (FETCH_SIZE / WRITE_SIZE collected in separate rocprofv3 passes and corrected as
    MI355X_MICROARCH.md prescribes; scripts/pmc_traffic.py).  Counters cannot be read from inside this process, so
    the figure is the profiled one -- and only if the profile is of THESE kernels: `rows` are the GEMM launches this run
    just timed (kernel_breakdown); a profile that lacks one of their kernel families is refused (null + the reason)
    instead of being quoted stale; a profile of the same kernels from edited sources is quoted with a note."""
    best = None
    try:
        from mdbn_amd import build
        want_hash = build.source_hash()
    except Exception:
        want_hash = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json"))):
        try:
            with open(path) as f:
                d = json.load(f)
            if "step_bytes" in d:
                # the profile of THESE sources if there is one (whatever its tag sorts like), else the last by name
                if best is None or best[1].get("source_hash") != want_hash or d.get("source_hash") == want_hash:
                    best = (os.path.basename(path), d)
        except Exception:
            pass
    if not best:
        return None, None, None, "no profiles/r*_pmc_traffic.json with step_bytes"
    name, d = best
    kernels = d.get("step_kernels") or {}
    if rows is not None:
        need = set()
        for r in rows.values():
            k = r.get("kernel", "")
            for fam in ("gemm_planes_bal_kernel", "gemm_planes_kernel", "skinny_gemm_kernel", "gemm_bf16x6_kernel"):
                if k.startswith(fam):
                    need.add(fam)
                    break
        have = " ".join(kernels)
        missing = sorted(fam for fam in need if (fam + "<") not in have and (fam + " ") not in have and fam not in have)
        if missing:
            return name, None, None, "refused: the profile has no %s launches, this run timed them" % ", ".join(missing)
    try:
        from mdbn_amd import build
        want = build.source_hash()
        if d.get("source_hash") and d["source_hash"] != want:
            note = "the profiled library (%s...) is not this one (%s...): same kernel families, sources edited since" \
                % (d["source_hash"][:12], want[:12])
        else:
            note = None if d.get("source_hash") else "the profile predates source-hash stamping: kernel families checked only"
    except Exception:
        note = None
    return name, d["step_bytes"], kernels, note


def rccl_summary(path):
    """What RCCL logged about its channels (NCCL_DEBUG=INFO, INIT subsystem); None when nothing is found."""
    import re
    if not path or not os.path.exists(path):
        return None
    try:
        with open(path, errors="replace") as f:
            text = f.read()
    except OSError:
        return None
    out = {"log_bytes": len(text)}
    m = re.findall(r"(\d+) coll channels", text)
    if m:
        out["coll_channels"] = sorted(set(int(x) for x in m))
    m = re.findall(r"Channel (\d+)/(\d+)", text)
    if m:
        out["channels_listed"] = max(int(b) for _, b in m)
    m = re.findall(r"(NCCL_[A-Z_]+) set by environment to ([^\s]+)", text)
    if m:
        out["env"] = dict(m)
    keep = [ln.split("NCCL INFO", 1)[-1].strip() for ln in text.splitlines()
            if ("channels" in ln or "Connected all" in ln or "Init COMPLETE" in ln or "Using network" in ln)]
    out["lines"] = keep[:12]
    return out


def capped_process_group(td, eng, max_ctas, world, deadline_s=60.0):
    """A second RCCL communicator over all ranks whose kernels use at most `max_ctas` workgroups (ncclConfig_t.maxCTAs
    through torch's ProcessGroupNCCL.Options): one channel = one workgroup = one CU taken from the step, so this is the other
    half of the comm_cus trade.  Built and proven (one small all-reduce) on a helper thread that the caller abandons after
    `deadline_s`: a communicator that cannot be built must not hang the run that matters.  Every rank takes the same decision
    through the default communicator.  Returns (process group or None, whether the helper thread was abandoned)."""
    import threading
    import torch
    box = {}

    def make():
        try:
            torch.cuda.set_device(eng.device)
            opts = td.ProcessGroupNCCL.Options()
            opts.config.max_ctas = int(max_ctas)
            pg = td.new_group(backend="nccl", pg_options=opts)
            buf = torch.ones(1024, dtype=torch.float32, device=eng.device)
            work = td.all_reduce(buf, op=td.ReduceOp.SUM, group=pg, async_op=True)
            while not work.is_completed():
                time.sleep(0.01)
            work.wait()
            torch.cuda.synchronize(eng.device)
            box["pg"] = pg if abs(float(buf[0]) - world) < 0.5 else None
        except Exception:
            box["pg"] = None

    th = threading.Thread(target=make, daemon=True)
    th.start()
    th.join(deadline_s)
    abandoned = th.is_alive()
    ok = int(not abandoned and box.get("pg") is not None)
    flag = torch.tensor([ok, int(abandoned)], dtype=torch.int32, device=eng.device)
    td.all_reduce(flag, op=td.ReduceOp.MIN)              # through the default communicator
    all_ok = bool(int(flag[0].item()))
    flag2 = torch.tensor([int(abandoned)], dtype=torch.int32, device=eng.device)
    td.all_reduce(flag2, op=td.ReduceOp.MAX)
    return (box.get("pg") if all_ok else None), bool(int(flag2.item()))


def _blas_threads():
    try:
        from threadpoolctl import threadpool_info
        return max([p.get("num_threads", 1) for p in threadpool_info()] or [1])
    except Exception:
        return os.cpu_count() or 1


def _time_oracle_steps(cfg, budget_s, min_steps):
    """Timed CD-k steps of the numpy float32 oracle on one of the named shapes."""
    from oracle import rbm_np
    from oracle.philox_np import PhiloxDraws
    v, h, b, gauss = cfg["V"], cfg["H"], cfg["B"], cfg["gauss"]
    rs = np.random.RandomState(123)
    rs.randint(2 ** 30)
    st = rbm_np.RBMState(v, h, W=rbm_np.init_W(rs, v, h, np.float32), dtype=np.float32, gauss=gauss)
    if cfg.get("weightcost"):
        st.freeze_W0()
    g = np.random.default_rng(0)
    data = g.standard_normal((4 * b, v), dtype=np.float32) if gauss else \
        (np.round(255 * g.beta(0.1, 0.7, size=(4 * b, v))) / 255).astype(np.float32)
    draws = [PhiloxDraws(1, 0, t) for t in range(4)]
    need = [0, 2] if gauss else [0, 1, 2]
    pre = [{d: (dr.u(d, b, v) if d == 1 else dr.u(d, b, h)) for d in need} for dr in draws]   # RNG not timed
    hp = dict(lr=cfg["lr"], k=1, lambda_1=0.0, lambda_2=cfg.get("lambda_2", 0.0), weightcost=cfg.get("weightcost", 0.0),
              batch_size=b, momentum=cfg.get("momentum", 0.0))
    done, t0 = 0, None
    for it in range(1000000):
        if it == 2:
            t0 = time.perf_counter()
        idx = np.arange(b) + (it % 4) * b
        rbm_np.cd_step(st, data[idx], rbm_np.ArrayDraws(pre[it % 4]), **hp)
        if t0 is not None:
            done += 1
            if time.perf_counter() - t0 > budget_s and done >= min_steps:
                break
    dt = time.perf_counter() - t0
    return done, dt


def cpu_baseline():
    """NumPy float32 restatement of the same step (oracle/rbm_np.py) on the host cores: the headline
    shape (c2) on all BLAS threads = `value`; beside it single-core c2 and the reference's own
    CPU-runnable shape c1 (RBM 784->500, batch 20) on all cores and on one."""
    threads = _blas_threads()
    c2 = dict(V=V, H=H, B=B_PER_GPU, gauss=True, lr=LR, lambda_2=LAMBDA_2)
    c1 = dict(V=784, H=500, B=20, gauss=False, lr=0.1, weightcost=2e-4, momentum=0.6)
    runs = {}
    done, dt = _time_oracle_steps(c2, 6.0, 5)
    runs[int(threads)] = (done, dt)
    d1, t1 = _time_oracle_steps(c1, 2.0, 20)
    c1_runs = {int(threads): (d1, t1)}
    try:
        # more BLAS threads are not always faster on a many-core host: also time 16 threads and one
        # core, and quote the FASTEST as the baseline (cores = the threads it used)
        from threadpoolctl import threadpool_limits
        for n in (16, 1):
            if n < threads:
                with threadpool_limits(limits=n):
                    runs[n] = _time_oracle_steps(c2, 6.0, 3)
                    c1_runs[n] = _time_oracle_steps(c1, 2.0, 20)
    except Exception:                               # threadpoolctl missing: all-thread figures only
        pass
    best = max(runs, key=lambda n: runs[n][0] / runs[n][1])
    done, dt = runs[best]
    out = {"value": done * B_PER_GPU / dt, "unit": "samples/s", "cores": int(best), "kind": "port",
           "steps_per_s": done / dt,
           "sample": "%d CD-1 steps of the same GRBM 4096->1024, B=512, numpy float32 oracle, injected uniforms; fastest of "
                     "BLAS thread counts %s on a host with %d cpus" % (done, sorted(runs), os.cpu_count() or 0),
           "by_threads": {str(n): {"steps_per_s": d / t, "samples_per_s": d * B_PER_GPU / t, "steps": d}
                          for n, (d, t) in sorted(runs.items())},
           "single_core": ({"value": runs[1][0] * B_PER_GPU / runs[1][1], "unit": "samples/s", "cores": 1,
                            "steps_per_s": runs[1][0] / runs[1][1]} if 1 in runs else None),
           # BASELINE configs[0], the reference's own CPU-runnable shape: RBM 784->500, CD-1, batch 20
           "c1_rbm_784_500_b20": {str(n): {"steps_per_s": d / t, "samples_per_s": 20 * d / t, "steps": d}
                                  for n, (d, t) in sorted(c1_runs.items())}}
    return out


def kernel_breakdown(detail):
    """Aggregate mdbn_kernel_timing_detail rows by GEMM: launches, average time, issued and
    algorithmic FLOPs, and the fraction of the matrix pipe the kernel executes on."""
    groups = {}
    for ms, alg, pipe, kind in detail:
        groups.setdefault(kind, []).append((ms, alg, pipe))
    rows = {}
    for kind, v in sorted(groups.items()):
        p = (kind // 100) % 10
        family = {0: "", 1: "_streaming", 2: "_planes", 3: "_planes_balanced"}.get(kind // 1000, "_%d" % (kind // 1000))
        name = KIND_NAMES.get(kind % 10, "gemm%d" % (kind % 10)) + family
        t = sum(x[0] for x in v) * 1e-3
        alg, pipe = sum(x[1] for x in v), sum(x[2] for x in v)
        peak = MFMA_BF16_PEAK_TFLOPS if p else MFMA_F32_PEAK_TFLOPS
        key = name if name not in rows else "%s_%d" % (name, kind)
        rows[key] = {"launches": len(v), "avg_us": 1e6 * t / len(v),
                     "pipe": ("bf16 MFMA, %d product(s) per algorithmic product" % {1: 6, 2: 3, 3: 1}[p]) if p else "f32 MFMA",
                     "kernel": {0: "gemm_bf16x6_kernel / gemm_splitk_kernel (f32 operands in HBM)", 1: "skinny_gemm_kernel",
                                2: "gemm_planes_kernel (pre-split bf16 planes, LDS-DMA)",
                                3: "gemm_planes_bal_kernel (the same on CUs - comm_cus workgroups, equal stage ranges)"
                                }.get(kind // 1000, "?"),
                     "issued_tflops": pipe / t / 1e12, "pipe_peak_tflops": peak, "frac_of_pipe": pipe / t / 1e12 / peak,
                     "algorithmic_f32_tflops": alg / t / 1e12, "fused_epilogue": (kind // 10) % 10}
    return rows


class Watchdog(object):
    """N > 1: the first contact with real hardware must not lose its number.  Once the DEFAULT setting has been timed, its
    complete JSON line is parked here; if anything after that (a sweep point, a second communicator, a collective of the
    reporting tail) has not finished by the deadline, rank 0 prints the parked line -- marked `provisional`, with the phase
    that stalled in `watchdog_phase` -- and every rank leaves with exit code WATCHDOG_RC (3): a stall is never reported as a
    clean run (launch_ranks relays the code; under the driver's own torchrun every rank fails with it).
    Exactly ONE line is ever printed: `finish` and the watchdog exclude each other."""

    WATCHDOG_RC = 3

    def __init__(self, rank):
        import threading
        self.rank, self.line, self.deadline, self.done, self.why = rank, None, None, False, ""
        self.lock = threading.Lock()
        self.thread = threading.Thread(target=self._watch, daemon=True)
        self.thread.start()

    def park(self, out):
        with self.lock:
            self.line = dict(out)

    def arm(self, seconds, why):
        with self.lock:
            self.deadline, self.why = time.time() + seconds, why

    def finish(self, out):
        with self.lock:
            self.done = True
            if out is not None:
                print(json.dumps(out))
                sys.stdout.flush()

    def _watch(self):
        while True:
            time.sleep(0.5)
            with self.lock:
                if self.done:
                    return
                late = self.deadline is not None and time.time() > self.deadline + (0.0 if self.rank == 0 else 3.0)
                if not late:
                    continue
                self.done = True
                if self.rank == 0 and self.line is not None:
                    self.line["provisional"] = True
                    self.line["watchdog_phase"] = self.why
                    self.line["provisional_reason"] = "watchdog: '%s' did not finish in time; this is the DEFAULT setting, " \
                                                      "timed before any sweep; the process exits with code %d" % (self.why, self.WATCHDOG_RC)
                    print(json.dumps(self.line))
                    sys.stdout.flush()
                sys.stderr.write("bench.py watchdog (rank %d): phase '%s' stalled; exiting with code %d\n"
                                 % (self.rank, self.why, self.WATCHDOG_RC))
                sys.stderr.flush()
            os._exit(self.WATCHDOG_RC)


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))

    import torch
    import mdbn_amd
    from mdbn_amd import dist

    rccl_log = None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and not os.environ.get("MDBN_DIST_BACKEND"):
        # let RCCL say what it chose (channels = workgroups = CUs its kernels occupy): INIT lines into a per-rank file
        rccl_log = "/tmp/mdbn_bench_rccl_%d_rank%s.log" % (os.getppid(), os.environ.get("RANK", "0"))
        os.environ.setdefault("NCCL_DEBUG", "INFO")
        os.environ.setdefault("NCCL_DEBUG_SUBSYS", "INIT,ENV")
        os.environ.setdefault("NCCL_DEBUG_FILE", rccl_log)
    rank, local_rank, world = dist.init_from_env()
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
    dev = eng.device
    B_global = B_PER_GPU * world
    td = torch.distributed
    backend_name = td.get_backend() if world > 1 else None
    t_job0 = time.time()

    # synthetic z-scored features, identical on every rank
    g = torch.Generator(device="cpu").manual_seed(0)
    data = torch.randn((N_DATA, V), generator=g, dtype=torch.float32).to(dev)
    train_set_x = mdbn_amd.shared(data, engine=eng)
    rbm = mdbn_amd.GRBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(123), engine=eng)
    _, updates = rbm.get_cost_updates(lr=LR, k=K_GIBBS, lambda_1=LAMBDA_1, lambda_2=LAMBDA_2,
                                      batch_size=B_global)
    step_fn = mdbn_amd.function(updates, train_set_x)
    perm = torch.from_numpy(np.random.RandomState(1).permutation(N_DATA).astype(np.int64)).to(dev)
    n_mb = N_DATA // B_global

    def run(n, first):
        # every call also names the NEXT minibatch, as the reference's trainers can (the epoch's order is drawn up front,
        # dbn.py:446-458): the single-device step then gathers those rows inside its statistics kernel instead of
        # launching a gather first -- every step still gathers exactly one minibatch
        cost = None
        for it in range(first, first + n):
            mb, nb = it % n_mb, (it + 1) % n_mb
            cost = step_fn(indexes=perm[mb * B_global:(mb + 1) * B_global], momentum=0.0,
                           next_indexes=perm[nb * B_global:(nb + 1) * B_global])
        return cost

    def settle(seconds):
        """Back-to-back steps of a throwaway model, on a context of its own, until `seconds` have passed.  The first tens of
        milliseconds of steps after start run slower (one GPU: the first 200-step window after 20 warm-up steps read 0.144
        ms per step, every later window 0.135), so a short plain run would time that ramp; the timed model's own steps stay
        a fixed number whatever the clock says."""
        eng_t = mdbn_amd.HipEngine()
        rbm_t = mdbn_amd.GRBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(123), engine=eng_t)
        _, up = rbm_t.get_cost_updates(lr=LR, k=K_GIBBS, lambda_1=LAMBDA_1, lambda_2=LAMBDA_2, batch_size=B_PER_GPU)
        fn = mdbn_amd.function(up, train_set_x, data_parallel=None)
        t0, it = time.perf_counter(), 0
        while time.perf_counter() - t0 < seconds:
            for _ in range(50):
                mb, nb = it % n_mb, (it + 1) % n_mb
                fn(indexes=perm[mb * B_global:mb * B_global + B_PER_GPU], momentum=0.0,
                   next_indexes=perm[nb * B_global:nb * B_global + B_PER_GPU])
                it += 1
            torch.cuda.synchronize(dev)
        del fn, up, rbm_t, eng_t

    def barrier():
        if world > 1:
            td.barrier()
        torch.cuda.synchronize(dev)

    def timed_window(first):
        barrier()
        t0 = time.perf_counter()
        cost = run(args.steps, first)
        barrier()
        dt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device=dev)
            td.all_reduce(t, op=td.ReduceOp.MAX)
            dt = float(t.item())
        return dt, cost

    def measure(first, min_total=1.0, n_win=None):
        """Median of >= 5 windows of exactly --steps steps; short windows are repeated until >= min_total s of steps has been
        timed (at most 20000 windows), so that a sampler beside the run sees the GPU busy.  n_win > 0: exactly that many."""
        n_win = args.windows if n_win is None else n_win
        wins, cost = [], None
        while True:
            dt, cost = timed_window(first)
            first += args.steps
            wins.append(dt)
            if n_win:
                if len(wins) >= n_win:
                    break
            elif len(wins) >= 5 and (sum(wins) >= min_total or len(wins) >= 20000):
                break
        return wins, cost, first

    def time_kernels(first):
        """Per-kernel durations: HIP events around every GEMM launch on its stream, over min(K, 1000) more steps (the library
        keeps at most 8192 event pairs: time a bounded number of steps and count THOSE)."""
        n = max(1, min(args.steps, 1000))
        eng.kernel_timing(True)
        run(n, first)
        torch.cuda.synchronize(dev)
        detail = eng.kernel_timing_detail()
        n_recorded, _ = eng.kernel_timing_read()
        eng.kernel_timing(False)
        if n_recorded != len(detail):
            raise SystemExit("kernel timing buffer overflowed: %d launches recorded, %d returned" % (n_recorded, len(detail)))
        return detail, n, first + n

    def measure_headline(first, min_total):
        """The timed steps behind `value`: one window of --steps steps in a plain run (--windows M: M windows), the >= 5
        windows of `measure` under --full."""
        return measure(first, min_total) if args.full else measure(first, n_win=args.windows or 1)

    def outputs_of(cost):
        """Host copies of what the last step left to its caller (--dump-outputs)."""
        if not args.dump_outputs:
            return None
        out = {"cost": np.array([float(cost)], dtype=np.float64)}
        for name in ("W", "hbias", "vbias", "W_speed", "hbias_speed", "vbias_speed"):
            out[name] = getattr(rbm, name).get_value().astype(np.float32)
        return out

    def agree(flag):
        """All ranks take rank 0's decision (one small broadcast through the default communicator)."""
        if world == 1:
            return bool(flag)
        t = torch.tensor([int(bool(flag))], dtype=torch.int32, device=dev)
        td.broadcast(t, src=0)
        return bool(int(t.item()))

    def setting_of(fn):
        return {"overlap": bool(getattr(fn, "overlap", False)), "comm_cus": int(getattr(fn, "comm_cus", 0)),
                "collective": "capi" if (getattr(fn, "group", None) is not None and fn.group._comm_engine is not None
                                         and fn.group.native is not False) else "torch",
                "update_inside_statistics_gemm": int(getattr(fn, "fuse_deferred", 0)), "rccl_max_ctas": None}

    def roofline_of(detail, n_timed_steps):
        """The `roofline` block: the GEMM launches of `n_timed_steps` steps timed with HIP events (time_kernels)."""
        rows = kernel_breakdown(detail)
        n_launch = len(detail)
        t_all = sum(d[0] for d in detail) * 1e-3
        issued = sum(d[2] for d in detail)
        alg = sum(d[1] for d in detail)
        on_bf16 = all(((d[3] // 100) % 10) != 0 for d in detail) and n_launch > 0
        peak = MFMA_BF16_PEAK_TFLOPS if on_bf16 else MFMA_F32_PEAK_TFLOPS
        achieved = issued / t_all / 1e12 if n_launch else None
        traffic_file, traffic, traffic_kernels, traffic_note = pmc_traffic(rows)
        algorithmic_bytes = 4.0 * B_PER_GPU * V + 16.0 * V * H       # v0 read once, W and W_speed read + written
        worst = min(rows.items(), key=lambda kv: kv[1]["frac_of_pipe"])[0] if rows else None
        # achieved = FLOPs ISSUED on the matrix pipe the GEMM kernels execute on (six / three bf16 products per
        # algorithmic f32 product), summed over the step's GEMM launches, / their summed HIP-event durations;
        # peak = that pipe's dense peak.  `kernels` has the same per GEMM; the f32-equivalent (algorithmic)
        # rate is a separate, informational field.
        return {"bound": "mfma",
                "kernel": "GEMM launches of the step (%s)" % ("bf16 matrix pipe, split f32 operands" if on_bf16
                                                              else "mixed / f32 matrix pipe"),
                "achieved": achieved, "peak": peak, "unit": "TFLOP/s",
                "frac": (achieved / peak) if achieved else None,
                # HBM bytes per CD STEP over ALL kernels of the step (PMC, profiled run of the default path) beside
                # the algorithmic bytes of SURVEY 8d; their ratio is the re-read / double-storage overhead
                "traffic": traffic, "traffic_unit": "bytes per CD step, all kernels", "traffic_source": traffic_file,
                "traffic_note": traffic_note,
                "traffic_by_kernel": traffic_kernels,
                "algorithmic_bytes": algorithmic_bytes,
                "traffic_over_algorithmic": (traffic / algorithmic_bytes) if traffic else None,
                "launches_timed": n_launch, "launches_per_step": n_launch / float(n_timed_steps),
                "avg_launch_us": 1e6 * t_all / max(n_launch, 1),
                "issued_flop_per_step": issued / float(n_timed_steps),
                "algorithmic_flop_per_step": alg / float(n_timed_steps),
                "algorithmic_f32_tflops": alg / t_all / 1e12 if n_launch else None,
                "furthest_below_roof": worst,
                "kernels": rows}

    def line_for(wins, cost, detail, n_timed_steps, dist_block, extras=None):
        """The complete JSON line of one measured setting (`roofline` when its kernels were timed: --full)."""
        elapsed = float(np.median(wins))
        steps_per_s = args.steps / elapsed
        # algorithmic FLOPs: 2*B*V*H per product, 2k+3 products per CD-k step
        flop_per_step = 2.0 * B_PER_GPU * V * H * (2 * K_GIBBS + 3)
        out = {
            "metric": "CD-k Gibbs steps/sec (samples/sec), GRBM 4096->1024 CD-1",
            "value": steps_per_s * B_global * K_GIBBS,
            "unit": "samples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "timing": "median of %d windows of %d steps, each bracketed by barrier + synchronize (max over ranks)"
                      % (len(wins), args.steps),
            "windows_ms_per_step": [1e3 * w / args.steps for w in wins[:40]],
            "windows_ms_per_step_min_max": [1e3 * min(wins) / args.steps, 1e3 * max(wins) / args.steps],
            "arithmetic": "f32 operands split exactly into 3 bf16 pieces; 6 piece products (3 when one operand holds 0/1 "
                          "samples) on v_mfma_f32_16x16x32_bf16 with f32 accumulation, operands pre-split into bf16 planes in "
                          "HBM (error vs float64 = rocBLAS sgemm's or better); "
                          "exact_f32_mfma_* = the same step on v_mfma_f32_32x32x2_f32",
            "config": {"workload": "GRBM 4096->1024 CD-1, batch %d per GPU, fp32, N(0,1) rows resident in HBM "
                                   "(BASELINE configs[%d])" % (B_PER_GPU, 1 if world == 1 else 2),
                       "global_batch": B_global, "k": K_GIBBS, "n_data": N_DATA,
                       "parallelism": "dp%d" % world},
            "cd_steps_per_s": steps_per_s,
            "step_algorithmic_f32_tflops": flop_per_step * world * steps_per_s / 1e12,          # whole job
            "step_algorithmic_f32_tflops_over_f32_mfma_peak": flop_per_step * steps_per_s / 1e12 / MFMA_F32_PEAK_TFLOPS,
            "final_cost": float(cost),
            "distributed": dist_block,
        }
        if detail is not None:
            out["roofline"] = roofline_of(detail, n_timed_steps)
        if extras:
            out.update(extras)
        return out

    settle(1.0)
    run(args.warmup, 0)
    # ------------------------------------------------------------------ the DEFAULT setting, always first
    # (--full on one GPU: 6 s of back-to-back steps -- a 5-second utilisation sampler beside the run then has a busy sample;
    #  the r04 driver log showed none for 1 s of steps)
    wins, cost, nxt = measure_headline(args.warmup, min_total=6.0 if world == 1 else 1.5)
    outputs = outputs_of(cost)
    detail, n_timed_steps = None, 0
    if args.full:
        detail, n_timed_steps, nxt = time_kernels(nxt)

    dog = None
    dist_block = {"ranks": world, "backend": backend_name, "rccl_ranks": world if backend_name == "nccl" else 0,
                  "allreduce_bytes": 4 * (V * H + H + V + 4) if world > 1 else 0}
    if world > 1:
        dist_block.update(setting_of(step_fn))
        dist_block["update_inside_statistics_gemm"] = int(getattr(step_fn, "fuse_deferred", 0)) >= (2 if getattr(step_fn, "comm_cus", 0) else 1)
        dist_block["collective"] = step_fn.group.collective if getattr(step_fn, "group", None) is not None else None
        # MDBN_DP_COLLECTIVE=auto (default): the C-ABI RCCL collective once it has proven alive on every rank, else torch's
        dist_block["collective_mode"] = os.environ.get("MDBN_DP_COLLECTIVE", "auto")
        dist_block["capi_collective_fallback_reason"] = getattr(step_fn.group, "native_error", None) if getattr(step_fn, "group", None) is not None else None
        dist_block["default_setting_ms_per_step"] = 1e3 * float(np.median(wins)) / args.steps
        dog = Watchdog(rank)
        dog.park(line_for(wins, cost, detail, n_timed_steps, dict(dist_block, note="default setting; nothing after it finished")))
        dog.arm(float(os.environ.get("MDBN_BENCH_TAIL_BUDGET_S", "180")), "per-rank times / all-reduce alone")
        # per-rank times, and the collective on its own: the packed statistics buffer, summed over ranks, HIP events on the
        # stream that waits for it (the step overlaps it with the next step's compute)
        mine = torch.tensor([1e3 * float(np.median(wins)) / args.steps], dtype=torch.float64, device=dev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        td.all_gather(allr, mine)
        dist_block["per_rank_ms_per_step"] = [float(x.item()) for x in allr]
        if args.full:
            buf = torch.zeros(V * H + H + V + 4, dtype=torch.float32, device=dev)
            for _ in range(5):
                td.all_reduce(buf)
            barrier()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                td.all_reduce(buf)
            e1.record()
            torch.cuda.synchronize(dev)
            dist_block["allreduce_alone_us"] = 1e3 * e0.elapsed_time(e1) / 20
        dist_block["rccl"] = rccl_summary(rccl_log) if rank == 0 else None
        dog.park(line_for(wins, cost, detail, n_timed_steps, dict(dist_block, note="default setting; the sweep did not finish")))

    # ------------------------------------------------------------------ N > 1: the tuning curve, under ONE wall budget
    # How many CUs to leave to the collective (and which collective) cannot be known from one GPU -- measure it here: short
    # windows at every setting, all reported in `distributed.sweep`; the fastest is installed and timed like the default
    # (it is `value`).  Rank 0's clock decides what still fits the budget; points that do not are reported as skipped.
    # --full only: a plain run times the default setting.
    sweep, groups, best = None, {}, None
    budget = float(args.sweep_budget)
    if world > 1 and args.full and not args.no_sweep and budget > 0 and getattr(step_fn, "overlap", False):
        sweep = []
        default = setting_of(step_fn)
        t_sweep0 = time.time()
        dog.arm(budget + 120.0, "data-parallel sweep (budget %.0f s)" % budget)
        per_point = [8.0]                                     # seconds a point took so far (rank 0's estimate)

        def left():
            return budget - (time.time() - t_sweep0)

        def install(st, pg):
            step_fn.flush()
            torch.cuda.synchronize(dev)
            step_fn.group.pg, step_fn.group.native = pg, st["collective"] == "capi"
            step_fn.overlap, step_fn.comm_cus = st["overlap"], (st["comm_cus"] if st["overlap"] else 0)
            step_fn.fuse_deferred = st["update_inside_statistics_gemm"]

        def point(st, pg, first):
            """Time one setting in short windows; returns (record, next step index)."""
            t0 = time.time()
            rec = dict(st)
            try:
                install(st, pg)
                run(max(5, args.warmup // 2), first)
                w, _, first = measure(first, min_total=0.15)
                step_fn.flush()
                rec.update(ms_per_step=1e3 * float(np.median(w)) / args.steps, windows=len(w), error=None)
            except Exception as exc:                          # a setting that cannot run is reported, not fatal
                rec.update(ms_per_step=None, windows=0, error=repr(exc)[:200])
            per_point.append(time.time() - t0)
            return rec, first

        default_pg = step_fn.group.pg
        groups = {None: default_pg}
        nxt0 = nxt
        # (overlap, comm_cus, C-ABI collective, deferred update inside the statistics GEMM [comm_cus 0 only]); the default
        # setting itself was timed above and is the first record
        sweep.append(dict(default, ms_per_step=dist_block["default_setting_ms_per_step"], windows=len(wins), error=None,
                          note="the default setting (timed first, full windows)"))
        # every point on the DEFAULT collective; the other collective at the main point (comm_cus 0, update inside the
        # statistics GEMM), so that the line always reports both; --sweep-capi: every point on both
        other = "torch" if default["collective"] == "capi" else "capi"
        shapes = ((True, 0, 1), (True, 0, 0), (True, 8, 0), (True, 16, 0), (True, 32, 0), (True, 32, 2), (True, 64, 0), (False, 0, 0))
        settings = [dict(overlap=ov, comm_cus=cus if ov else 0, collective=default["collective"],
                         update_inside_statistics_gemm=fu, rccl_max_ctas=None) for ov, cus, fu in shapes]
        both = args.sweep_capi or os.environ.get("MDBN_BENCH_SWEEP_CAPI") == "1"
        settings[1:1] = [dict(overlap=ov, comm_cus=cus if ov else 0, collective=other, update_inside_statistics_gemm=fu,
                              rccl_max_ctas=None) for ov, cus, fu in (shapes if both else shapes[:1])]
        settings = [st for st in settings if st != default]
        capi_ok = None
        for st in settings:
            if not agree(left() > 1.5 * max(per_point)):
                sweep.append(dict(st, skipped="wall budget of %.0f s" % budget))
                continue
            if st["collective"] == "capi":
                if backend_name != "nccl":
                    continue                                  # the C-ABI communicator is RCCL: needs one GPU per rank
                if capi_ok is None:
                    capi_ok = step_fn.group.probe_native(eng, deadline_s=30.0)     # (a no-op when the default already runs on it)
                    if not capi_ok:
                        sweep.append({"collective": "capi", "error": "C-ABI collective not swept: %s" % step_fn.group.native_error})
                if not capi_ok:
                    continue
            rec, nxt0 = point(st, default_pg, nxt0)
            sweep.append(rec)
        # Second stage, RCCL only: communicators capped at a few channel counts (one channel = one workgroup = one CU the
        # collective takes; it has a whole step to finish 16.8 MB, so it may not need RCCL's default).  Each cap is timed
        # with the GEMMs as they are (comm_cus 0, update inside the statistics GEMM) and balanced on the other CUs.  Skipped
        # entirely when stage one has eaten the budget; never continued after a communicator had to be abandoned.
        if backend_name == "nccl" and not args.no_cta_sweep:
            for ctas in (8, 16, 32):
                if not agree(left() > 40.0 + 2 * max(per_point)):
                    sweep.append({"rccl_max_ctas": ctas, "skipped": "wall budget of %.0f s" % budget})
                    continue
                pg, abandoned = capped_process_group(td, eng, ctas, world, deadline_s=min(60.0, max(10.0, left() - 20.0)))
                if pg is None:
                    sweep.append({"rccl_max_ctas": ctas, "error": "a communicator with this cap could not be built or did not "
                                                                   "complete a small all-reduce in time on every rank"})
                    if abandoned:                             # a helper thread is still stuck in RCCL: no further communicators
                        break
                    continue
                groups[ctas] = pg
                for cus, fu in ((0, 1), (ctas, 0)):
                    st = dict(overlap=True, comm_cus=cus, collective="torch", update_inside_statistics_gemm=fu, rccl_max_ctas=ctas)
                    if not agree(left() > 1.5 * max(per_point)):
                        sweep.append(dict(st, skipped="wall budget of %.0f s" % budget))
                        continue
                    rec, nxt0 = point(st, pg, nxt0)
                    sweep.append(rec)
        ok = [r for r in sweep if r.get("ms_per_step")]
        best = min(ok, key=lambda r: r["ms_per_step"])
        dist_block["sweep_wall_s"] = time.time() - t_sweep0
        dog.arm(float(os.environ.get("MDBN_BENCH_TAIL_BUDGET_S", "180")), "final timing of the best sweep point")
        if {k: best[k] for k in default} != default:
            # the best point, timed like the default was: it becomes `value`
            install({k: best[k] for k in default}, groups[best.get("rccl_max_ctas")])
            run(args.warmup, nxt0)
            wins, cost, nxt0 = measure(nxt0)
            outputs = outputs_of(cost)
            detail, n_timed_steps, nxt0 = time_kernels(nxt0)
        else:
            install(default, default_pg)
        nxt = nxt0
        dist_block.update({k: best[k] for k in default})
        dist_block["update_inside_statistics_gemm"] = int(step_fn.fuse_deferred) >= (2 if step_fn.comm_cus else 1)
        dist_block["collective"] = step_fn.group.collective
        # the all-reduce alone through each channel-capped communicator of the second stage
        allreduce_by_cap = {}
        for ctas, pg in sorted((k, v) for k, v in groups.items() if k is not None):
            try:
                for _ in range(3):
                    td.all_reduce(buf, group=pg)
                barrier()
                e0.record()
                for _ in range(20):
                    td.all_reduce(buf, group=pg)
                e1.record()
                torch.cuda.synchronize(dev)
                allreduce_by_cap[str(ctas)] = 1e3 * e0.elapsed_time(e1) / 20
            except Exception as exc:
                allreduce_by_cap[str(ctas)] = repr(exc)[:120]
        dist_block["allreduce_alone_us_by_rccl_max_ctas"] = allreduce_by_cap
    if world > 1:
        dist_block["sweep"] = sweep
    if world > 1 and args.full:
        dog.park(line_for(wins, cost, detail, n_timed_steps, dict(dist_block, note="the reporting tail did not finish")))
        dog.arm(float(os.environ.get("MDBN_BENCH_TAIL_BUDGET_S", "180")), "exposed-communication probe")
        # What the collective costs the step: the SAME setting with both all-reduce calls stubbed out (Group.stub_collective:
        # measurement only -- the replicas then train on their own shards' statistics, which is why this comes last).
        try:
            step_fn.flush()
            torch.cuda.synchronize(dev)
            step_fn.group.stub_collective = True
            run(max(5, args.warmup // 2), nxt)
            w, _, nxt = measure(nxt, min_total=0.3)
            step_fn.flush()
            stub_ms = 1e3 * float(np.median(w)) / args.steps
            step_ms = 1e3 * float(np.median(wins)) / args.steps
            stat_us = sum(r["avg_us"] * r["launches"] for k, r in kernel_breakdown(detail).items() if k.startswith("statistics")) \
                / float(n_timed_steps)
            inside = dist_block["update_inside_statistics_gemm"]
            dist_block["exposed_comm_us"] = 1e3 * (step_ms - stub_ms)
            dist_block["step_without_collective_ms"] = stub_ms
            # how long the collective may run before the step waits for it: a whole step when the deferred update follows
            # the step, the step minus its statistics launch when that launch applies the update (it waits first)
            dist_block["cover_us"] = (1e3 * step_ms - stat_us) if (inside and step_fn.overlap) else (1e3 * step_ms if step_fn.overlap else 0.0)
        except Exception as exc:
            dist_block["exposed_comm_us"] = None
            dist_block["exposed_comm_error"] = repr(exc)[:200]
        finally:
            step_fn.group.stub_collective = False
        # ONE place for what the one-GPU proxy predicted and what this run measured (the step alone 146 us,
        # beside a CU-holding stand-in 197-213 us => 5.2-6.1x at 8 GPUs; the >= 6x of the north star is NOT a measured claim
        # until this table comes from an 8-GPU node)
        step_ms_now = 1e3 * float(np.median(wins)) / args.steps
        single_gpu_ms = None
        try:
            cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench.json")))
            for path in reversed(cands):
                with open(path) as fh:
                    rec = json.loads(fh.read().strip().splitlines()[-1])
                if rec.get("n_gpus") == 1 and rec.get("ms_per_step"):
                    single_gpu_ms = float(rec["ms_per_step"])
                    break
        except Exception:
            single_gpu_ms = None
        dist_block["predicted_vs_measured"] = {
            "ranks": world,
            "single_gpu_ms_per_step (newest profiles/r*_bench.json)": single_gpu_ms,
            "predicted_ms_per_step_one_gpu_proxy": [0.197, 0.213],
            "predicted_weak_scaling_at_8": [5.2, 6.1],
            "measured_ms_per_step": step_ms_now,
            "measured_weak_scaling": (world * single_gpu_ms / step_ms_now) if single_gpu_ms else None,
            "step_without_collective_ms": dist_block.get("step_without_collective_ms"),
            "exposed_comm_us": dist_block.get("exposed_comm_us"),
            "cover_us": dist_block.get("cover_us"),
            "allreduce_alone_us": dist_block.get("allreduce_alone_us"),
            "comm_cus": dist_block.get("comm_cus"),
            "collective": dist_block.get("collective"),
            "note": "comm_cus and the collective of `value` are the fastest point of `sweep` (installed and re-timed like the "
                    "default); weak scaling = ranks x single-GPU step time / this step time",
        }

    # the same steps with the GEMMs forced onto the exact-f32 MFMA (v_mfma_f32_32x32x2_f32): by default
    # they run on the bf16 matrix pipe with three-way split operands and f32 accumulation (f32 accuracy,
    # DESIGN.md section 3); both numbers are reported
    exact_ms = None
    exact_rows = None
    if world == 1 and args.full and not args.default_only:
        eng.set_option("gemm_bf16x6", 0)
        eng.set_option("gemm_planes", 0)
        run(args.warmup, 0)
        ewins, _, _ = measure(args.warmup, min_total=0.25)
        exact_ms = 1e3 * float(np.median(ewins)) / args.steps
        eng.kernel_timing(True)
        run(n_timed_steps, args.warmup)
        torch.cuda.synchronize(dev)
        exact_rows = kernel_breakdown(eng.kernel_timing_detail())
        eng.kernel_timing(False)
        eng.set_option("gemm_bf16x6", 3)
        eng.set_option("gemm_planes", 1)

    # BASELINE configs[1] says "bf16/fp32": the same step with the GEMM inputs truncated to bf16 (one product per
    # GEMM instead of six, f32 accumulation) is a REPORTING figure only -- probabilities are then off by ~4e-3, so it
    # is never the parity path and never `value`
    bf16_in = None
    if world == 1 and args.full and not args.default_only:
        eng.set_option("bf16_inputs", 1)
        run(args.warmup, 0)
        bwins, _, _ = measure(args.warmup, min_total=0.25)
        eng.set_option("bf16_inputs", 0)
        bms = 1e3 * float(np.median(bwins)) / args.steps
        bf16_in = {"ms_per_step": bms, "samples_per_s": B_global * K_GIBBS * 1e3 / bms,
                   "note": "GEMM inputs truncated to bf16 (leading piece of the 3-way split), f32 accumulate, one MFMA "
                           "product per algorithmic product; NOT the parity path (probability error ~4e-3), reported "
                           "because BASELINE configs[1] names bf16/fp32"}
        run(args.warmup, 0)               # back on the f32-grade path before the parity check below

    # The boundary also takes a HOST-resident training table (mdbn_amd.shared(x, resident="host"): pinned memory, each
    # minibatch's rows gathered over PCIe into a double buffer one step ahead of the step that uses them).  Its rate is
    # reported beside `value`, never as `value` (the metric is defined with inputs resident in HBM).
    pcie = None
    if world == 1 and args.full and not args.default_only:
        try:
            host_x = mdbn_amd.shared(data.cpu().numpy(), engine=eng, resident="host")
            rbm_h = mdbn_amd.GRBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(123), engine=eng)
            _, up_h = rbm_h.get_cost_updates(lr=LR, k=K_GIBBS, lambda_1=LAMBDA_1, lambda_2=LAMBDA_2, batch_size=B_global)
            fn_h = mdbn_amd.function(up_h, host_x)

            host_perm = perm.cpu()

            def run_host(n, announce):
                views = [perm[(it % n_mb) * B_global:(it % n_mb + 1) * B_global] for it in range(n)]
                if announce:      # the order of the coming steps, as the trainers announce an epoch's
                    fn_h.announce(views, host_indexes=[host_perm[(it % n_mb) * B_global:(it % n_mb + 1) * B_global] for it in range(n)])
                for it in range(n):
                    fn_h(indexes=views[it], momentum=0.0)
            res = {}
            for announce in (True, False):
                run_host(args.warmup, announce)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                run_host(10 * args.steps, announce)
                torch.cuda.synchronize(dev)
                res[announce] = 1e3 * (time.perf_counter() - t0) / (10 * args.steps)
            feed = fn_h._staging["feeder"].stats() if fn_h._staging and fn_h._staging.get("feeder") else None
            pcie = {"ms_per_step": res[True], "samples_per_s": B_global * 1e3 / res[True], "feeder_host_times": feed,
                    "ms_per_step_without_prefetch": res[False],
                    "minibatch_bytes": 4 * B_global * V,
                    "note": "training table in pinned host memory; announced minibatches are gathered by 8 CPU threads into "
                            "pinned staging and moved by one SDMA copy each, three slots deep (mdbn_feeder_*, "
                            "StepFunction.announce); unannounced ones by the library's PCIe gather kernel on the spot; "
                            "NOT `value`"}
            del host_x, fn_h, rbm_h
        except Exception as exc:                    # reporting figure only
            pcie = {"error": repr(exc)[:200]}

    # free-energy parity of the trained model vs the float64 oracle (north star: <= 1e-4 rel)
    fe_rel = fe_rel_elem = None
    if rank == 0 and args.full:
        from oracle import rbm_np
        st = rbm_np.RBMState(V, H, W=rbm.W.get_value(), hbias=rbm.hbias.get_value(),
                             vbias=rbm.vbias.get_value(), gauss=True)
        x = data[:B_PER_GPU].cpu().numpy()
        F = rbm.free_energy(x).get_value()
        F_o = rbm_np.free_energy(st, x.astype(np.float64))
        # relative to the largest |F| of the batch (a row whose two O(V) terms nearly cancel would
        # otherwise dominate with a meaningless ratio); the element-wise maximum is reported too
        fe_rel = float(np.max(np.abs(F - F_o)) / np.max(np.abs(F_o)))
        fe_rel_elem = float(np.max(np.abs(F - F_o) / np.abs(F_o)))

    if rank != 0:
        if dog is not None:
            dog.finish(None)
        return
    dist_block["wall_s_since_start"] = time.time() - t_job0
    extras = {
        "exact_f32_mfma_ms_per_step": exact_ms,
        "exact_f32_mfma_value": (B_global * K_GIBBS * 1e3 / exact_ms) if exact_ms else None,
        "exact_f32_mfma_kernels": exact_rows,
        "bf16_input_mode": bf16_in,
        "pcie_inclusive_host_resident_table": pcie,
        "free_energy_max_rel_err_vs_f64_oracle": fe_rel,
        "free_energy_max_elementwise_rel_err": fe_rel_elem}
    out = line_for(wins, cost, detail, n_timed_steps, dist_block, extras if args.full else None)
    if world == 1 and args.full and not args.no_cpu_baseline and not args.default_only:
        out["cpu_baseline"] = cpu_baseline()
    if outputs is not None:
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, arr in outputs.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), arr)
    if dog is not None:
        dog.finish(out)
    else:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
