#!/usr/bin/env python
"""What up-down fine-tuning does to the variational bound of a pre-trained stack: a synthetic Bernoulli table (rows of 8
prototypes of 64 bits, every bit flipped with probability 0.05; 400 training rows, 200 held-out rows), a 64 -> 32 -> 16 DBN
pre-trained greedily (DBN.training), then `DBN.log_likelihood_bound` of the held-out rows before and after
`DBN.fine_tune`, log Z of the top RBM re-estimated each time.  Reported, not asserted.  Writes a JSON with the source hash.
    python scripts/updown_bound_demo.py [--epochs 40] [--out profiles/updown_bound_demo.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, mdbn_amd
from mdbn_amd import build

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=40)
ap.add_argument("--lr", type=float, default=0.02)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "updown_bound_demo.json"))
args = ap.parse_args()
eng = mdbn_amd.set_engine(mdbn_amd.HipEngine())
mdbn_amd.DBN.verbose = False

rs = np.random.RandomState(0)
protos = (rs.uniform(size=(8, 64)) < 0.5).astype(np.float32)


def table(n):
    rows = protos[rs.randint(0, 8, n)]
    return np.abs(rows - (rs.uniform(size=rows.shape) < 0.05)).astype(np.float32)


train, held_out = table(400), table(200)
net = mdbn_amd.DBN(numpy_rng=np.random.RandomState(1), theano_rng=mdbn_amd.RandomStreams(2), n_ins=64, gauss=False,
                   hidden_layers_sizes=[32], n_outs=16, engine=eng)
net.shuffle_rng = np.random.RandomState(3)
net.training(train, 20, 1, [60, 60], [0.05, 0.05], lambda_2=0.0)


def bound(tag):
    b = net.log_likelihood_bound(held_out, n_samples=64, n_chains=512, n_betas=4000)
    row = dict(stage=tag, bound=b.bound, stderr=b.stderr, log_z=b.log_z, log_z_stderr=b.log_z_stderr)
    print(json.dumps(row))
    return row


rows = [bound("pre-trained")]
history = net.fine_tune(train, args.epochs, batch_size=20, lr=args.lr, momentum=0.5)
rows.append(bound("fine-tuned, %d epochs" % args.epochs))
res = dict(source_hash=build.source_hash(), lr=args.lr, epochs=args.epochs, stages=rows, history=history,
           baseline_independent_bits=-64 * float(np.log(2.0)))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
print("wrote", args.out)
