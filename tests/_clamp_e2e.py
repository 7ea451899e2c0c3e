"""End to end (TEST-ONLY): a three-modality MDBN with the shapes of examples/train_mdbn_synthetic.py, trained for a few epochs on
synthetic tables whose modalities share a planted patient class, then ``MDBN.impute_modalities`` on held-out patients with one
modality withheld.  Runs on whatever engine is the default (the CPU checker engine or the device) with the same seeds; returns
the mean squared error of the imputed joint block against the block the withheld data really gives, and the error of the
block's training mean -- what one would fill in without a model."""
import numpy as np

ORDER = ("ME", "GE", "SM")                       # column order of the joint layer (examples/train_mdbn_synthetic.py)
PRESETS = {"ME": dict(k=5, layers_sizes=[40], lr=[0.002]),
           "GE": dict(k=1, layers_sizes=[400, 40], lr=[0.002, 0.1]),
           "SM": dict(k=1, layers_sizes=[200, 20], lr=[0.002, 0.1])}


def tables(n_persons, seed=0):
    """Feature-by-person tables: expression ~ lognormal around class centres, mutations sparse 0/1 with class-specific rates."""
    rs = np.random.RandomState(seed)
    groups = rs.randint(0, 3, n_persons)

    def expr(n_feat, scale):
        centers = rs.normal(0, 1, (3, n_feat))
        return np.exp(scale * (centers[groups] + rs.normal(0, 1, (n_persons, n_feat)))).T
    sm = (rs.uniform(size=(n_persons, 256)) < 0.02 + 0.05 * (groups[:, None] == rs.randint(0, 3, 256)[None, :])).T
    return {"GE": expr(2048, 0.5), "ME": expr(512, 0.5), "SM": sm.astype(np.float64)}


def run(withheld="ME", rows=256, epochs=10, batch=32, n_steps=300, burn_in=100, n_chains=4):
    import mdbn_amd
    from mdbn_amd import DBN, shared
    from mdbn_amd.MDBN import train_bottom_layer, impute_modalities
    from mdbn_amd.utils import preprocess_table
    verbose, DBN.verbose = DBN.verbose, False
    try:
        rng = np.random.RandomState(123)
        np.random.seed(0)                       # the trainers shuffle with numpy's global state, as the reference does
        tabs = tables(rows)
        nets, train_out, val_rows, val_out = [], [], [], []
        for name in ORDER:
            p = PRESETS[name]
            train, val = preprocess_table(tabs[name], holdout=0.25, repeats=1, shuffle=False)
            steps = epochs * (len(train) // batch)
            net, out_t, out_v = train_bottom_layer(shared(train), shared(val), batch_size=batch, k=p["k"], layers_sizes=p["layers_sizes"],
                                                   pretraining_epochs=[steps] * len(p["layers_sizes"]), pretrain_lr=p["lr"],
                                                   lambda_1=0.0, lambda_2=0.1, rng=rng)
            nets.append(net); train_out.append(out_t); val_rows.append(val); val_out.append(out_v)
        joint_t, joint_v = np.concatenate(train_out, axis=1), np.concatenate(val_out, axis=1)
        joint = DBN(numpy_rng=rng, n_ins=joint_t.shape[1], gauss=False, hidden_layers_sizes=[128], n_outs=3)
        joint.training(shared(joint_t), batch, k=1, pretraining_epochs=[epochs * (len(joint_t) // batch)] * 2, pretrain_lr=[0.1, 0.1],
                       validation_set_x=shared(joint_v))
        w = ORDER.index(withheld)
        lo = sum(o.shape[1] for o in train_out[:w])
        hi = lo + train_out[w].shape[1]
        inputs = [None if i == w else v for i, v in enumerate(val_rows)]
        jv, jt, imputed = impute_modalities(nets, joint, inputs, n_steps=n_steps, burn_in=burn_in, n_chains=n_chains)
        assert jv.shape == joint_v.shape and jt.shape == (len(joint_v), 3) and sorted(imputed) == [w]
        assert imputed[w].shape == val_rows[w].shape and np.isfinite(imputed[w]).all()
        # the observed blocks pass through untouched
        keep = np.ones(joint_v.shape[1], dtype=bool)
        keep[lo:hi] = False
        np.testing.assert_allclose(jv[:, keep], joint_v[:, keep], rtol=0, atol=1e-5)
        truth = val_out[w].astype(np.float64)
        mse_imputed = float(((jv[:, lo:hi] - truth) ** 2).mean())
        mse_mean = float(((train_out[w].astype(np.float64).mean(axis=0)[None] - truth) ** 2).mean())
        return mse_imputed, mse_mean
    finally:
        DBN.verbose = verbose
