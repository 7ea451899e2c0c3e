"""Interleaved A/B of a library option on the full CD-1 step (bench workload).
    python scripts/step_ab.py OPTION VALUE VALUE ...
A value may be repeated (``slab_tail 0 0``): every position is an arm of its own, so two arms with the same setting show
what identical settings differ by on this box.  MDBN_AB_LIBRARY=path times a library built with diagnostic -D flags from the
current sources instead of the in-tree one (scripts/build_variants.py)."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, mdbn_amd
if os.environ.get("MDBN_AB_LIBRARY"):
    from mdbn_amd import _lib
    _lib.use_diagnostic_library(os.environ["MDBN_AB_LIBRARY"])
opt, values = sys.argv[1], [int(v) for v in sys.argv[2:]]
eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
# MDBN_AB_SHAPE="V,H,B,k,gauss" selects another layer (default: the c2 headline shape)
V, H, B, K, GAUSS = [int(x) for x in os.environ.get("MDBN_AB_SHAPE", "4096,1024,512,1,1").split(",")]
N = 32768
g = torch.Generator(device="cpu").manual_seed(0)
if GAUSS:
    data = mdbn_amd.shared(torch.randn((N, V), generator=g).to(eng.device))
    rbm = mdbn_amd.GRBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(123))
    _, up = rbm.get_cost_updates(lr=0.001, k=K, lambda_2=0.1, batch_size=B)
else:
    data = mdbn_amd.shared((torch.rand((N, V), generator=g) < 0.3).float().to(eng.device))
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(123))
    _, up = rbm.get_cost_updates(lr=0.05, k=K, weightcost=2e-4, batch_size=B)
fn = mdbn_amd.function(up, data)
perm = torch.from_numpy(np.random.RandomState(1).permutation(N)).to(eng.device)
def run(n):
    for it in range(n):
        mb, nb = it % (N // B), (it + 1) % (N // B)
        fn(indexes=perm[mb * B:(mb + 1) * B], momentum=0.0, next_indexes=perm[nb * B:(nb + 1) * B])
res = [[] for v in values]
run(20); eng.synchronize()
for rnd in range(int(os.environ.get("MDBN_AB_ROUNDS", "5"))):
    for arm, v in enumerate(values):
        eng.set_option(opt, v)
        run(5); eng.synchronize()
        t0 = time.perf_counter(); run(100); eng.synchronize()
        res[arm].append((time.perf_counter() - t0) * 1e4)
for arm, v in enumerate(values):
    print("arm %d %s=%d: median %.2f us/step (min %.2f, max %.2f)" % (arm, opt, v, np.median(res[arm]), min(res[arm]), max(res[arm])))
# per-GEMM averages (HIP events around each launch) under every value
for v in sorted(set(values)):
    eng.set_option(opt, v)
    run(5); eng.synchronize()
    eng.kernel_timing(True); run(50); eng.synchronize()
    groups = {}
    for ms, alg, pipe, kind in eng.kernel_timing_detail():
        groups.setdefault(kind, []).append(ms)
    eng.kernel_timing(False)
    print("%s=%d GEMM launches: %s" % (opt, v, ", ".join("kind %d: %.1f us x%d" % (k, 1e3 * np.mean(t), len(t) // 50)
                                                          for k, t in sorted(groups.items()))))
