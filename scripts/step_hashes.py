"""One SHA-256 line per step-function path: the costs, W, the speeds and the biases after 12 steps with changing indexes,
momentum and lr -- equal lines before and after a change of the host side mean the device computed the same run.
    python scripts/step_hashes.py            # every scenario, each in a process of its own under a time limit
    python scripts/step_hashes.py NAME       # one scenario, in this process
Behind each hash: how many of the 12 steps went through the cached argument structs (full ``cd_train_step`` calls are
counted, the rest were cached) and after how many ``CDScratch.ahead`` said the next minibatch had been prepared."""
import hashlib
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = 12
SCENARIOS = {   # name: V, H, B, gauss, N, options
    "cache 100->24 B=20 rbm": (100, 24, 20, 0, 400, {}),
    "cache 100->24 B=20 rbm hinted": (100, 24, 20, 0, 400, dict(hint=1)),
    "cache 100->24 B=20 grbm hinted": (100, 24, 20, 1, 400, dict(hint=1)),
    "thin 700->512 B=32 grbm hinted": (700, 512, 32, 1, 256, dict(hint=1)),
    "thin 700->512 B=32 rbm": (700, 512, 32, 0, 256, {}),
    # (planes_min_work = 0 does not put 512->128 at B = 128 on the plane path -- its steps go through the cached structs --;
    #  1024->512 at B = 256 is the smallest shape here that it does)
    "512->128 B=128 grbm hinted": (512, 128, 128, 1, 2048, dict(hint=1, planes=1)),
    "planes 1024->512 B=256 grbm hinted": (1024, 512, 256, 1, 2048, dict(hint=1, planes=1)),
    "planes 1024->512 B=256 rbm hinted": (1024, 512, 256, 0, 2048, dict(hint=1, planes=1)),
    "planes 1024->512 B=256 grbm": (1024, 512, 256, 1, 2048, dict(planes=1)),
    # (the next minibatch is gathered inside the statistics kernel on the big plane shapes only: the headline step, product defaults)
    "planes 4096->1024 B=512 grbm hinted": (4096, 1024, 512, 1, 2048, dict(hint=1)),
    "planes 2048->2048 B=512 rbm hinted": (2048, 2048, 512, 0, 2048, dict(hint=1)),
    "host table 512->128 B=128 grbm announced": (512, 128, 128, 1, 2048, dict(planes=1, host=1, announce=1)),
    "host table 512->128 B=128 grbm unannounced": (512, 128, 128, 1, 2048, dict(planes=1, host=1)),
    "host table 1024->512 B=256 grbm announced": (1024, 512, 256, 1, 2048, dict(planes=1, host=1, announce=1)),
    "host table 1024->512 B=256 grbm hinted": (1024, 512, 256, 1, 2048, dict(planes=1, host=1, hint=1)),
    "pcd 100->24 B=20 rbm": (100, 24, 20, 0, 400, dict(pcd=1)),
    "pcd 1024->512 B=256 grbm": (1024, 512, 256, 1, 2048, dict(pcd=1, planes=1)),
    "symbolic_grad 100->24 B=20 rbm hinted": (100, 24, 20, 0, 400, dict(symbolic=1, hint=1)),
    "symbolic_grad 1024->512 B=256 rbm hinted": (1024, 512, 256, 0, 2048, dict(symbolic=1, hint=1, planes=1)),
    "two ranks 1024->512 B=512 grbm hinted overlapped fuse_deferred=0": (1024, 512, 512, 1, 2048, dict(planes=1, hint=1, ranks=2, fuse=0)),
    "two ranks 1024->512 B=512 grbm hinted overlapped fuse_deferred=1": (1024, 512, 512, 1, 2048, dict(planes=1, hint=1, ranks=2, fuse=1)),
    "two ranks 4096->1024 B=1024 grbm hinted overlapped fuse_deferred=0": (4096, 1024, 1024, 1, 2048, dict(hint=1, ranks=2, fuse=0)),
    "two ranks 4096->1024 B=1024 grbm hinted overlapped fuse_deferred=1": (4096, 1024, 1024, 1, 2048, dict(hint=1, ranks=2, fuse=1)),
    "two ranks 100->24 B=20 rbm overlapped fuse_deferred=1": (100, 24, 20, 0, 400, dict(ranks=2, fuse=1)),
    "two ranks host table 1024->512 B=512 grbm announced overlapped": (1024, 512, 512, 1, 2048, dict(planes=1, host=1, announce=1, ranks=2, fuse=1)),
}


def run(name):
    """-> 'sha256 cached=N ahead=N' of one scenario on the current device (and the current process group, if any)."""
    import numpy as np
    import mdbn_amd
    V, H, B, gauss, N, opt = SCENARIOS[name]
    eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
    if opt.get("planes"):
        eng.set_planes_min_work(0)
    rs = np.random.RandomState(4)
    data = rs.normal(size=(N, V)).astype(np.float32) if gauss else (rs.uniform(size=(N, V)) < 0.3).astype(np.float32)
    cls = mdbn_amd.GRBM if gauss else mdbn_amd.RBM
    rbm = cls(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(123), theano_rng=mdbn_amd.RandomStreams(9), engine=eng)
    hp = dict(lr=0.001, lambda_2=0.1) if gauss else dict(lr=0.05, weightcost=2e-4)
    if opt.get("pcd"):
        hp["persistent"] = mdbn_amd.shared(np.zeros((B, H), dtype=np.float32), engine=eng, ld=rbm.W.tensor.stride(0))
    if opt.get("symbolic"):
        hp["symbolic_grad"] = True
    _, up = rbm.get_cost_updates(k=1, batch_size=B, **hp)
    fn = mdbn_amd.function(up, mdbn_amd.shared(data, engine=eng, resident="host" if opt.get("host") else "device"),
                           data_parallel="auto" if opt.get("ranks") else None)
    if "fuse" in opt:
        assert fn.overlap
        fn.fuse_deferred = opt["fuse"]
    order = [rs.permutation(N)[:B] for _ in range(STEPS + 1)]
    batches = [eng.index_tensor(o) for o in order]
    if opt.get("announce"):
        fn.announce(batches[:STEPS], host_indexes=order[:STEPS])
    full, ahead, costs = [0], 0, []
    whole = eng.cd_train_step

    def counted(*args, **kw):
        full[0] += 1
        return whole(*args, **kw)
    eng.cd_train_step = counted
    for t in range(STEPS):
        hint = None
        if opt.get("hint") and t != 4:                      # step 4 announces nothing, step 2 the wrong minibatch
            hint = batches[t + 1] if t != 2 else batches[0]
        base = 0.001 if gauss else 0.05
        costs.append(fn(indexes=batches[t], momentum=0.5 if t < 6 else 0.9, lr=base if t % 2 else 0.4 * base, next_indexes=hint))
        ahead += int(eng.last_scratch is not None and eng.last_scratch.ahead is not None)
    costs = np.array([float(c) for c in costs], dtype=np.float64)
    fn.flush()
    h = hashlib.sha256(costs.tobytes())
    for arr in (rbm.W, rbm.W_speed, rbm.hbias, rbm.hbias_speed, rbm.vbias, rbm.vbias_speed):
        h.update(np.ascontiguousarray(arr.get_value()).tobytes())
    single = not opt.get("ranks") and not opt.get("pcd")
    return "%s cached=%s ahead=%d" % (h.hexdigest(), STEPS - full[0] if single else "-", ahead)


def rank_main(name, rank, port):
    import torch
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2",
                      LOCAL_RANK=str(rank if torch.cuda.device_count() >= 2 else 0), HSA_ENABLE_IPC_MODE_LEGACY="0")
    from mdbn_amd import dist
    dist.init_from_env(backend="gloo")
    line = run(name)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
    print("%s [rank %d, %d GPU(s)]: %s" % (name, rank, torch.cuda.device_count(), line), flush=True)


def main(argv):
    if len(argv) == 3:
        return rank_main(argv[0], int(argv[1]), int(argv[2]))
    if len(argv) == 1:
        print("%s: %s" % (argv[0], run(argv[0])), flush=True)
        return 0
    from mdbn_amd import build
    print("# mdbn_source_hash %s" % build.source_hash(), flush=True)
    for name, spec in SCENARIOS.items():
        me = [sys.executable, os.path.abspath(__file__), name]
        if spec[5].get("ranks"):
            s = socket.socket()
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
            s.close()
            procs = [subprocess.Popen(me + [str(r), str(port)], stdout=subprocess.PIPE, text=True) for r in range(2)]
        else:
            procs = [subprocess.Popen(me, stdout=subprocess.PIPE, text=True)]
        codes, lines = [], []
        for p in procs:
            try:
                lines += [l for l in p.communicate(timeout=120)[0].splitlines() if l.startswith(name)]   # (not the backends' chatter)
                codes.append(p.returncode)
            except subprocess.TimeoutExpired:
                codes.append("time limit")
        print("\n".join(sorted(lines)), flush=True)
        if any(codes):                                      # nothing more is started on a device after a failure
            for p in procs:
                if p.poll() is None:
                    p.kill()
            print("%s: FAILED %r" % (name, codes), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
