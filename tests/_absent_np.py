"""float64 twin of the absent visible units (mdbn_absent_* / mdbn_cd_step_absent; TEST-ONLY): the split of a table with NaN
into zero-filled rows and observed bits, the masked visible conditional with its own draws, the CD chain of rows with absent
units written out on oracle/rbm_np.py (free or teacher-forced along a recorded chain), the free energy over the observed
units, brute-force log Z_O and exact model expectations for tiny layers, a checker engine with the new engine calls, and
the kernel cases the CPU and the GPU test share.

The model (Salakhutdinov, Mnih & Hinton 2007): row r observes the set O_r; a unit outside O_r is absent from that row's
RBM; all rows share W, b, c.  With m = [i in O_r] and v~ = m o v:  h | v: sigmoid(c + v~ W);  v_i | h for i in O_r as the
plain layer, 0 elsewhere;  S = sum_r v~0' ph - n~v' nh,  s_h = sum_r ph - nh,  s_v = sum_r m (v0 - nv)."""
import itertools

import numpy as np
import torch

from _oracle_engine import OracleEngine, _Scratch
from oracle import rbm_np
from oracle.philox_np import PhiloxDraws, normal, uniform

MEAN_TOL = 2e-6         # _margins.SURVEY["prob"]


# ------------------------------------------------------------------------------------------------------------------ split
def split(x):
    """-> (filled float64, mask bool [B, V], words uint32 [B, (V + 31) // 32], row_count int32 [B]): only NaN is missing."""
    x = np.asarray(x)
    mask = ~np.isnan(x)
    filled = np.where(mask, x, 0.0).astype(np.float64)
    B, V = x.shape
    words = np.zeros((B, (V + 31) // 32), dtype=np.uint32)
    for i in range(V):
        words[:, i >> 5] |= mask[:, i].astype(np.uint32) << np.uint32(i & 31)
    return filled, mask, words, mask.sum(axis=1).astype(np.int32)


def mask_of(words, V):
    words = np.asarray(words).view(np.uint32) if np.asarray(words).dtype == np.int32 else np.asarray(words, dtype=np.uint32)
    cols = np.arange(V)
    return ((words[:, cols >> 5] >> (cols & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


# ------------------------------------------------------------------------------------------------------------------ visible
def visible(pre, mask, gauss, add_noise, U=None, Z=None):
    """-> (mean, sample) of the masked conditional from the linear pre-activations: Bernoulli sigmoid / u < mean; Gaussian
    mean = pre, sample = mean [+ Z].  Absent entries are 0 in both.  ``U`` / ``Z`` None: no draw (sample = mean for a
    noise-free Gaussian layer, None for a Bernoulli one)."""
    pre = np.asarray(pre, dtype=np.float64)
    if gauss:
        mean = pre.copy()
        sample = mean + np.asarray(Z, dtype=np.float64) if add_noise else mean.copy()
    else:
        mean = rbm_np.sigmoid(pre)
        sample = None if U is None else (np.asarray(U, dtype=np.float64) < mean).astype(np.float64)
    mean = np.where(mask, mean, 0.0)
    if sample is not None:
        sample = np.where(mask, sample, 0.0)
    return mean, sample


def cost(pre, v0, mask, gauss):
    """The monitoring cost summed over the OBSERVED entries: cross-entropy, or the reference's (sigmoid(x) - v0)^2."""
    pre, v0 = np.asarray(pre, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    if gauss:
        e = (rbm_np.sigmoid(pre) - v0) ** 2
    else:
        e = v0 * rbm_np.softplus(-pre) + (1.0 - v0) * rbm_np.softplus(pre)
    return float(e[mask].sum())


def tie_draws(mean, mask, U, tol=MEAN_TOL):
    """Observed Bernoulli draws that float32 rounding of the mean could decide either way."""
    return int(((np.abs(np.asarray(U, dtype=np.float64) - mean) < tol) & mask).sum())


# ------------------------------------------------------------------------------------------------------------------ the CD chain
def cd_chain(s, x, draws, k, trace_h=None, trace_v=None, tie=1e-6):
    """The chain of mdbn_cd_step_absent on the rows ``x`` (NaN: absent).  Draw numbering of rbm_np.cd_chain; the Gaussian
    chain is the reference's (the hidden units are driven by the masked nv_mean; noise only without error_free).  With
    ``trace_h`` / ``trace_v`` every sample the chain feeds onward is the recorded one, checked against the twin's own
    outside ties.  -> (v0 zero-filled, mask, ph_mean, [pre_v, nv_mean, v_sample, nh_mean], differing draws)."""
    v0, mask, _, _ = split(x)
    B, forced, flips = v0.shape[0], trace_h is not None, 0
    U0 = draws.u(0, B, s.n_hidden)
    _, ph_mean, h = rbm_np.sample_h_given_v(s, v0, U0)
    if forced:
        h, n = rbm_np._follow(h, trace_h[0], U0, ph_mean, tie, "h0")
        flips += n
    out = None
    for t in range(1, k + 1):
        pre_v = h @ s.W.T + s.vbias
        noisy = s.gauss and not s.error_free
        Uv = None if s.gauss else draws.u(2 * t - 1, B, s.n_visible)
        Zv = draws.z(2 * t - 1, B, s.n_visible) if noisy else None
        nv_mean, v_sample = visible(pre_v, mask, s.gauss, noisy, Uv, Zv)
        if forced and trace_v is not None:
            rec = np.asarray(trace_v[t - 1], dtype=np.float64)
            assert (rec[~mask] == 0.0).all(), "v%d: an absent entry of the recorded sample is not 0" % t
            if s.gauss:
                assert np.abs(rec - v_sample).max() < 1e-4, "v%d: the recorded Gaussian sample is not the twin's" % t
            else:
                v_sample, n = rbm_np._follow(v_sample, rec, Uv, nv_mean, tie, "v%d" % t)
                flips += n
        Uh = draws.u(2 * t, B, s.n_hidden)
        _, nh_mean, h = rbm_np.sample_h_given_v(s, nv_mean if s.gauss else v_sample, Uh)
        if forced and t < k:
            h, n = rbm_np._follow(h, trace_h[t], Uh, nh_mean, tie, "h%d" % t)
            flips += n
        out = [pre_v, nv_mean, v_sample, nh_mean]
    return v0, mask, ph_mean, out, flips


def cd_step_absent(s, x, draws, k, trace_h=None, trace_v=None):
    """-> (S, s_h, s_v, cost, parts): the packed statistics of the step and the cost over the observed entries; ``parts`` =
    (v0, mask, ph_mean, nv_mean, nh_mean, flips)."""
    v0, mask, ph, out, flips = cd_chain(s, x, draws, k, trace_h, trace_v)
    S, s_h, s_v = rbm_np.cd_statistics(v0, ph, out[1], out[3])
    return S, s_h, s_v, cost(out[0], v0, mask, s.gauss), (v0, mask, ph, out[1], out[3], flips)


# ------------------------------------------------------------------------------------------------------------------ energies
def free_energy_absent(s, x):
    """F_O(x_r) over the observed units of every row."""
    v, mask, _, _ = split(x)
    hidden = rbm_np.softplus(v @ s.W + s.hbias).sum(axis=1)
    if s.gauss:
        return 0.5 * (np.where(mask, v - s.vbias, 0.0) ** 2).sum(axis=1) - hidden
    return -(v @ s.vbias) - hidden


def brute_free_energy(s, x):
    """-log sum_h exp(-E(v_O, h)) over all 2^H hidden states, the energy over the observed units only."""
    v, mask, _, _ = split(x)
    out = np.zeros(v.shape[0])
    for r in range(v.shape[0]):
        terms = []
        for h in itertools.product((0.0, 1.0), repeat=s.n_hidden):
            h = np.asarray(h)
            E = -(v[r] @ s.W @ h) - s.hbias @ h
            E += 0.5 * ((v[r] - s.vbias)[mask[r]] ** 2).sum() if s.gauss else -(v[r] @ s.vbias)
            terms.append(-E)
        out[r] = -np.logaddexp.reduce(terms)
    return out


def log_Z_O(s, mask_row):
    """log Z of the RBM over the observed units ``mask_row`` of a BERNOULLI layer, by enumeration of the hidden states (the
    visible sum is closed form): Z_O = sum_h exp(c h) prod_{i in O} (1 + exp(b_i + W_i h))."""
    terms = []
    for h in itertools.product((0.0, 1.0), repeat=s.n_hidden):
        h = np.asarray(h)
        terms.append(s.hbias @ h + rbm_np.softplus(s.vbias + s.W @ h)[mask_row].sum())
    return float(np.logaddexp.reduce(terms))


def log_Z_O_gauss(s, mask_row):
    """... of a GAUSSIAN layer: the visible integral is closed form, Z_O = sum_h exp(c h) prod_{i in O} sqrt(2 pi)
    exp(b_i a_i + a_i^2 / 2) with a = W h."""
    terms = []
    for h in itertools.product((0.0, 1.0), repeat=s.n_hidden):
        h = np.asarray(h)
        a = s.W @ h
        terms.append(s.hbias @ h + (0.5 * np.log(2.0 * np.pi) + s.vbias * a + 0.5 * a * a)[mask_row].sum())
    return float(np.logaddexp.reduce(terms))


def model_expectations(s, mask_row):
    """Exact E[v~ h'], E[h], E[v~] under the RBM over the observed units ``mask_row`` (absent entries 0), by enumeration of h."""
    logZ = log_Z_O_gauss(s, mask_row) if s.gauss else log_Z_O(s, mask_row)
    Evh, Eh, Ev = np.zeros((s.n_visible, s.n_hidden)), np.zeros(s.n_hidden), np.zeros(s.n_visible)
    for h in itertools.product((0.0, 1.0), repeat=s.n_hidden):
        h = np.asarray(h)
        a = s.W @ h
        if s.gauss:
            lw = s.hbias @ h + (0.5 * np.log(2.0 * np.pi) + s.vbias * a + 0.5 * a * a)[mask_row].sum()
            ev = np.where(mask_row, s.vbias + a, 0.0)
        else:
            lw = s.hbias @ h + rbm_np.softplus(s.vbias + a)[mask_row].sum()
            ev = np.where(mask_row, rbm_np.sigmoid(s.vbias + a), 0.0)
        p = np.exp(lw - logZ)
        Evh += p * np.outer(ev, h)
        Eh += p * h
        Ev += p * ev
    return Evh, Eh, Ev


# ------------------------------------------------------------------------------------------------------------------ checker engine
class AbsentOracle(OracleEngine):
    """The checker engine with the calls of the absent visible units, from the twin.  ``calls`` records their names."""

    def __init__(self):
        OracleEngine.__init__(self)
        self.calls = []

    def absent_split(self, x, out=None, want_count=True):
        self.calls.append("absent_split")
        filled, _, words, count = split(self.as_matrix(x).numpy())
        filled = self._t(filled)
        if out is not None:
            out.copy_(filled)
            filled = out
        return filled, torch.from_numpy(words.view(np.int32).copy()), torch.from_numpy(count) if want_count else None

    def absent_visible(self, pre, observed, gauss=False, add_noise=False, rng=None, v0=None, out=None):
        self.calls.append("absent_visible")
        pre = self.as_matrix(pre).numpy()
        B, V = pre.shape
        mask = mask_of(observed.numpy(), V)
        U = self._u(rng, B, V) if (rng is not None and not gauss) else None
        Z = normal(B, V, rng.seed, rng.stream_id, rng.step, rng.draw, rng.row_offset) if (gauss and add_noise) else None
        mean, sample = visible(pre, mask, gauss, add_noise, U, Z)
        res = (self._t(mean), self._t(sample) if (sample is not None and rng is not None) else None)
        if v0 is None:
            return res
        return res + (torch.tensor(cost(pre, self.as_matrix(v0).numpy(), mask, gauss), dtype=self.t_dtype),)

    def cd_step_absent(self, data, indexes, W, hbias, vbias, gauss, k, rng, add_noise=False, stats_slot=0, stats=None):
        self.calls.append("cd_step_absent")
        data = self.as_matrix(data)
        x = (data if indexes is None else data[self.index_tensor(indexes)]).numpy()
        s = self._state(W, hbias, vbias, gauss)
        s.error_free = not add_noise
        S, s_h, s_v, c, (v0, mask, ph, nv, nh, _) = cd_step_absent(s, x, PhiloxDraws(rng.seed, rng.stream_id, rng.step, rng.row_offset), k)
        if stats is None:
            stats = self.stats_buffer(W.shape[0], W.shape[1], stats_slot)
        stats.copy_(self._t(np.concatenate([S.ravel(), s_h, s_v, [c, 0, 0, 0]])))
        sc = _Scratch()
        sc.v0, sc.mask, sc.ph_mean, sc.nv_mean, sc.nh_mean = v0, mask, ph, nv, nh
        self.last = sc
        return stats, sc

    def absent_mark_rows(self, y, row_count):
        self.calls.append("absent_mark_rows")
        y[row_count == 0] = float("nan")
        return y

    def free_energy_absent(self, x, W, hbias, vbias, gauss):
        self.calls.append("free_energy_absent")
        return self._t(free_energy_absent(self._state(W, hbias, vbias, gauss), self.as_matrix(x).numpy()))


# ------------------------------------------------------------------------------------------------------------------ kernel cases
# (V, ldv, B): one column; one short of a mask word, a whole word, one over; two words; one over two; two column blocks; the
# input layer of the label benchmark (four column blocks, a ragged last word); tables wider than 2048 columns -- 65 and 130 mask
# words, so the lanes of absent_count's one wave per row take a second trip, and lanes 0 and 1 a third.  B: one row, a ragged
# 4-row block, whole blocks, many blocks
KERNEL_CASES = [(1, 4, 1), (31, 32, 5), (32, 32, 4), (33, 36, 33), (64, 64, 8), (65, 68, 20), (300, 300, 7), (794, 796, 20),
                (2049, 2052, 3), (4133, 4136, 5)]
COUNT_TRIP = 2048           # columns one trip of absent_count's 64 lanes covers
VARIANTS = [("bernoulli", False, False), ("gauss", True, False), ("gauss_noise", True, True)]
ROW_OFFSET = 6              # not a multiple of 4: the 4-row Philox blocks straddle
# Philox seed of a case: 100 + V + 7 B unless listed here -- a seed under which the twin alone has at most TIE_CAP draws near a
# tie (tests/test_absent_twin.py asserts it), so that the GPU test's cap can only be broken by the kernel
CASE_SEEDS = {}
TIE_CAP = 4
STREAM, STEP, DRAW = 3, 11, 5


def case_seed(V, B):
    return CASE_SEEDS.get((V, B), 100 + V + 7 * B)


def case_pattern(V, B, rs):
    """bool [B, V]: 30 % of the entries missing at random; column 0 missing in every row and the last column observed in
    every row (V > 1); then row 0 wholly missing and the last row wholly observed (B > 1; the rows win where they cross)."""
    mask = rs.uniform(size=(B, V)) >= 0.3
    if V > 1:
        mask[:, 0] = False
        mask[:, V - 1] = True
    if B > 1:
        mask[0, :] = False
        mask[B - 1, :] = True
    return mask


def case_inputs(V, B, gauss):
    """-> (x float32 [B, V] with NaN at the missing entries, pre float32 [B, V], seed).  x: 0 / 1 data for a Bernoulli layer,
    N(0, 1) for a Gaussian one; one observed entry of the last row is +inf-free but large (a value, not a marker).  pre:
    N(0, 2^2); from five rows on, row 1 is all-equal, rows 2 and 3 are saturated (+-40 on every third column)."""
    rs = np.random.RandomState(1000 * V + B)
    mask = case_pattern(V, B, rs)
    x = rs.normal(size=(B, V)).astype(np.float32) if gauss else (rs.uniform(size=(B, V)) < 0.3).astype(np.float32)
    x[~mask] = np.nan
    pre = (2.0 * rs.normal(size=(B, V))).astype(np.float32)
    if B >= 5:
        pre[1, :] = np.float32(0.375)
        pre[2, ::3] += np.float32(40.0)
        pre[3, ::3] -= np.float32(40.0)
    return x, pre, case_seed(V, B)


def case_draws(V, B, seed):
    return (uniform(B, V, seed, STREAM, STEP, DRAW, ROW_OFFSET), normal(B, V, seed, STREAM, STEP, DRAW, ROW_OFFSET))


# ------------------------------------------------------------------------------------------------------------------ end-to-end toy
# A joint-like Bernoulli layer of three blocks with a planted patient class: every block holds the class's prototype bits with
# 10 % flips.  92 % of the training patients lack one block (a block of NaN); held-out patients have the last block withheld
# and it is imputed from the other two.  Chosen on the CPU with this twin: tests/test_absent_twin.py runs it on three seeds
# and DESIGN.md 3.22 has the figures.
TOY = dict(blocks=3, width=8, H=12, classes=4, flip=0.1, n_train=300, n_test=100, lose=0.92, B=10, steps=1200, lr=0.1, momentum=0.5,
           k=1)
TOY_SEEDS = (0, 1, 2)


def toy_problem(seed):
    """-> (train float32 [n_train, V] with a NaN block where a patient lost one, test float32 [n_test, V] complete, the
    column span (lo, hi) of the block the test withholds)."""
    T = TOY
    rs = np.random.RandomState(seed)
    V = T["blocks"] * T["width"]
    proto = (rs.uniform(size=(T["classes"], V)) < 0.5).astype(np.float32)

    def draw(n):
        c = rs.randint(T["classes"], size=n)
        x = proto[c].copy()
        flip = rs.uniform(size=x.shape) < T["flip"]
        x[flip] = 1.0 - x[flip]
        return x
    train, test = draw(T["n_train"]), draw(T["n_test"])
    lost = rs.uniform(size=T["n_train"]) < T["lose"]
    which = rs.randint(T["blocks"], size=T["n_train"])
    for r in np.flatnonzero(lost):
        train[r, which[r] * T["width"]:(which[r] + 1) * T["width"]] = np.nan
    return train, test, ((T["blocks"] - 1) * T["width"], V)


def toy_init(seed, V):
    return (0.01 * np.random.RandomState(1000 + seed).normal(size=(V, TOY["H"]))).astype(np.float32)


def toy_batches(n_rows, seed):
    """The minibatch index lists of the toy's ``steps`` steps (reshuffled epochs; a short last batch is dropped)."""
    assert n_rows >= TOY["B"], "fewer rows than one minibatch"
    rs, out = np.random.RandomState(2000 + seed), []
    while len(out) < TOY["steps"]:
        perm = rs.permutation(n_rows)
        out.extend(perm[i:i + TOY["B"]] for i in range(0, n_rows - TOY["B"] + 1, TOY["B"]))
    return out[:TOY["steps"]]


def toy_train_twin(rows, seed):
    """The toy's training loop on the twin -> RBMState."""
    T = TOY
    V = rows.shape[1]
    s = rbm_np.RBMState(V, T["H"], W=toy_init(seed, V).astype(np.float64), dtype=np.float64)
    for t, idx in enumerate(toy_batches(len(rows), seed)):
        S, s_h, s_v, _, _ = cd_step_absent(s, rows[idx].astype(np.float64), PhiloxDraws(seed, 0, t), T["k"])
        g = rbm_np.rbm_grad(s, S, s_h, s_v, T["B"], T["B"], 0.0)
        rbm_np.apply_update(s, g[0], g[1], g[2], T["lr"], 0.0, 0.0, T["momentum"])
    return s


def toy_exact_impute(s, test, lo, hi):
    """E[v_F | v_O] of every test row for the free block F = [lo, hi), exactly, by enumeration of the hidden states."""
    hs = np.asarray(list(itertools.product((0.0, 1.0), repeat=s.n_hidden)))
    a = hs @ s.W.T + s.vbias                                             # [2^H, V]
    free = np.zeros(s.n_visible, dtype=bool)
    free[lo:hi] = True
    out = np.zeros((len(test), hi - lo))
    for r, v in enumerate(np.asarray(test, dtype=np.float64)):
        lw = hs @ s.hbias + (hs @ s.W.T[:, ~free]) @ v[~free] + rbm_np.softplus(a[:, free]).sum(axis=1)
        p = np.exp(lw - np.logaddexp.reduce(lw))
        out[r] = p @ rbm_np.sigmoid(a[:, free])
    return out


def toy_errors(imputed_all, imputed_complete, train, test, lo, hi):
    """-> (MSE of the model trained on all patients, of the one trained on the complete patients, of the block's training mean)."""
    truth = np.asarray(test[:, lo:hi], dtype=np.float64)
    mean = np.nanmean(np.asarray(train[:, lo:hi], dtype=np.float64), axis=0)
    return (float(((imputed_all - truth) ** 2).mean()), float(((imputed_complete - truth) ** 2).mean()),
            float(((mean[None] - truth) ** 2).mean()))
