"""Parallel tempering of a trained RBM / GRBM: ``TemperedChains`` (RBM.tempered_chains) holds M ladders of R Gibbs chains at
the inverse temperatures 0 <= beta_0 < ... < beta_{R-1} = 1 of the tempered family of the AIS estimate (base-rate visible
bias b_A, b_beta = b_A + beta (b - b_A)) and advances them by sweeps with swaps between neighbouring temperatures
(csrc/mdbn_temper.hip, include/mdbn_hip.h: mdbn_pt_run).  On an engine without ``temper`` (the CPU checker of the tests) the
sweep is composed from the engine's eager calls: the same definitions, stated in Python.  A layer with ``visible_groups``
(categorical visible units) runs through ``engine.temper_grouped`` (mdbn_pt_run_grouped: a group's visible draw is one category
of its softmax at the row's temperature, ``v_avg`` holds softmax means) and is refused on an engine without it.

``TemperedChains.log_partition`` estimates log Z from the works of the swap attempts (mdbn_pt_run_z): the sweeps
accumulate them on the device, ``estimate_log_z`` finishes in float64 numpy."""
import collections

import numpy
import torch

from .engine import RngAddr, padded_ld
from .shared import SharedArray, as_tensor


def attempts(n_ladders, n_betas, sweep0, n_sweeps):
    """Swap attempts per neighbour pair [R - 1] of ``n_sweeps`` sweeps after ``sweep0`` earlier ones: the pair
    (rho, rho + 1) is tried in the sweeps of rho's parity."""
    g = numpy.arange(int(sweep0), int(sweep0) + int(n_sweeps))
    rho = numpy.arange(int(n_betas) - 1)
    return int(n_ladders) * ((g[:, None] - rho[None, :]) % 2 == 0).sum(axis=0)


def base_log_partition(base_vbias, n_hidden, gauss, groups=None):
    """log Z of the base-rate model (beta = 0): H log 2 + sum softplus(b_A) (Bernoulli) | H log 2 + V/2 log 2 pi
    (unit-variance Gaussian visibles), float64.  ``groups`` (a ``GroupTable`` or its boundaries; Bernoulli only): the columns
    of a softmax group hold one 1 between them, so group g contributes logsumexp_{c in g} b_A,c instead of its columns'
    softplus."""
    bA = numpy.asarray(base_vbias, dtype=numpy.float64)
    if groups is None:
        return n_hidden * numpy.log(2.0) + (0.5 * bA.size * numpy.log(2.0 * numpy.pi) if gauss
                                            else numpy.logaddexp(0.0, bA).sum())
    if gauss:
        raise ValueError("groups: a Gaussian visible layer has no categorical units")
    b = numpy.asarray(getattr(groups, "host", groups), dtype=numpy.int64)
    total = n_hidden * numpy.log(2.0) + numpy.logaddexp(0.0, bA[:b[0]]).sum() + numpy.logaddexp(0.0, bA[b[-1]:]).sum()
    for lo, hi in zip(b[:-1], b[1:]):
        total += numpy.logaddexp.reduce(bA[lo:hi])
    return total


LogZ = collections.namedtuple("LogZ", "log_z log_z_fwd log_z_rev stderr ratios_fwd ratios_rev acceptance attempts method")
LogZ.__doc__ = """log Z from the works of a tempering run: ``log_z`` (the chosen estimate: "mid" or "bar"), ``log_z_fwd`` /
``log_z_rev`` (biased low / high: the bracket), ``stderr`` (delete-one-ladder jackknife of ``log_z``), and per neighbour pair
[R - 1] ``ratios_fwd`` / ``ratios_rev`` (the two estimates of log Z_{rho+1} / Z_rho), ``acceptance`` and ``attempts``."""


def new_works(n_ladders, n_betas):
    """The accumulator of the works before the first sweep: float64 [M, R - 1, 4] = {m_f, s_f, m_r, s_r} at (-inf, 0)."""
    z = numpy.zeros((int(n_ladders), int(n_betas) - 1, 4), dtype=numpy.float64)
    z[:, :, 0::2] = -numpy.inf
    return z


def _logsumexp(x, axis):
    top = numpy.max(x, axis=axis, keepdims=True)
    top = numpy.where(numpy.isfinite(top), top, 0.0)
    with numpy.errstate(divide="ignore"):
        return numpy.squeeze(top, axis=axis) + numpy.log(numpy.exp(x - top).sum(axis=axis))


def _bar_root(df, dr, keep=None, start=None):
    """Bennett's self-consistent log ratio r per pair: sum_R f(-d_rev - r) = sum_F f(r - d_fwd), f(x) = 1 / (1 + exp x).
    ``df`` / ``dr`` [P, N]; ``keep`` [N] weights the samples (the jackknife).  Without ``start``: bisection between the
    extremes of d_fwd and -d_rev (the left side rises, the right side falls in r); with it: safeguarded Newton steps."""
    w = numpy.ones(df.shape[1]) if keep is None else keep

    def gap(r):
        with numpy.errstate(over="ignore"):
            a = 1.0 / (1.0 + numpy.exp(-dr - r[:, None]))
            b = 1.0 / (1.0 + numpy.exp(r[:, None] - df))
        return (a - b) @ w, (a * (1.0 - a) + b * (1.0 - b)) @ w

    lo = numpy.minimum(df.min(axis=1), (-dr).min(axis=1))
    hi = numpy.maximum(df.max(axis=1), (-dr).max(axis=1))
    if start is None:
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            up = gap(mid)[0] > 0
            hi, lo = numpy.where(up, mid, hi), numpy.where(up, lo, mid)
        return 0.5 * (lo + hi)
    r = start.copy()
    for _ in range(6):
        g, slope = gap(r)
        r = numpy.clip(r - g / numpy.maximum(slope, 1e-300), lo, hi)
    return r


def estimate_log_z(zacc, tries, log_z0, method="mid", works=None, accepted=None):
    """``LogZ`` from the accumulated works ``zacc`` [M, R - 1, 4], the attempts per pair ``tries`` [R - 1] (``attempts`` over
    the sweeps that accumulated) and log Z of beta = 0; float64 numpy.  Per pair the ladders are pooled by logsumexp:
    ratios_fwd = log mean exp d_fwd, ratios_rev = -log mean exp d_rev; "mid" is their mean (the leading biases are
    opposite), "bar" solves Bennett's acceptance ratio from ``works`` [n, M, R - 1, 2] (the tapped (d_fwd, d_rev) of the
    accumulating sweeps, NaN where a pair was not tried).  ``stderr``: the delete-one-ladder jackknife of the chosen estimate
    (ladders are independent, sweeps are not)."""
    if method not in ("mid", "bar"):
        raise ValueError("method must be 'mid' or 'bar', got %r" % (method,))
    z = numpy.asarray(zacc, dtype=numpy.float64)
    tries = numpy.asarray(tries, dtype=numpy.float64)
    M = z.shape[0]
    if (tries <= 0).any():
        raise ValueError("a neighbour pair has no swap attempt after burn-in: run at least two sweeps after it")
    with numpy.errstate(divide="ignore"):
        lf, lr = z[:, :, 0] + numpy.log(z[:, :, 1]), z[:, :, 2] + numpy.log(z[:, :, 3])       # [M, R - 1]
    fwd = _logsumexp(lf, 0) - numpy.log(tries)
    rev = -(_logsumexp(lr, 0) - numpy.log(tries))
    if method == "bar":
        if works is None:
            raise ValueError("method 'bar' needs the tapped works")
        w = numpy.asarray(works, dtype=numpy.float64)
        tried = ~numpy.isnan(w[:, 0, :, 0])                                                   # [n, R - 1]: the same for every ladder
        df = [w[tried[:, p], :, p, 0] for p in range(w.shape[2])]                             # per pair [n_p, M]
        dr = [w[tried[:, p], :, p, 1] for p in range(w.shape[2])]

        def solve(keep_ladder, start):
            out = numpy.empty(len(df))
            for p in range(len(df)):                # (the pairs of the two parities have different attempt counts)
                keep = None if keep_ladder is None else numpy.tile(keep_ladder, df[p].shape[0])
                out[p] = _bar_root(df[p].reshape(1, -1), dr[p].reshape(1, -1), keep, None if start is None else start[p:p + 1])[0]
            return out
        ratios = solve(None, None)
    else:
        ratios = 0.5 * (fwd + rev)
    est = log_z0 + ratios.sum()
    if M > 1:
        left = numpy.empty(M)
        for m in range(M):
            if method == "bar":
                keep = numpy.ones(M)
                keep[m] = 0.0
                left[m] = solve(keep, ratios).sum()
            else:
                rest = numpy.arange(M) != m
                t = numpy.log(tries * (M - 1.0) / M)
                left[m] = 0.5 * ((_logsumexp(lf[rest], 0) - t) - (_logsumexp(lr[rest], 0) - t)).sum()
        err = float(numpy.sqrt((M - 1.0) / M * ((left - left.mean()) ** 2).sum()))
    else:
        err = float("nan")
    acc = None if accepted is None else numpy.asarray(accepted, dtype=numpy.float64) / tries
    return LogZ(float(est), float(log_z0 + fwd.sum()), float(log_z0 + rev.sum()), err, fwd, rev, acc,
                tries.astype(numpy.int64), method)


class TemperedChains(object):
    """Device state of M ladders: ``v`` [M R, V], ``h`` [M R, H] (row m R + s = slot s of ladder m) and the rank map
    ``rank`` [M, R] (int32: the temperature index a slot holds; swaps exchange ranks, never states)."""

    def __init__(self, rbm, n_ladders, betas, base_vbias, start_h=None):
        eng = self.engine = rbm.engine
        self.rbm = rbm
        self.betas = numpy.ascontiguousarray(betas, dtype=numpy.float32)
        M, R = int(n_ladders), int(self.betas.size)
        if M < 1 or self.betas.ndim != 1 or R < 2:
            raise ValueError("need n_ladders >= 1 and at least 2 betas")
        if self.betas[0] < 0.0 or self.betas[-1] != 1.0 or not (numpy.diff(self.betas) > 0).all():
            raise ValueError("betas must rise strictly from betas[0] >= 0 to exactly 1")
        self.n_ladders, self.n_betas = M, R
        V, H = rbm.n_visible, rbm.n_hidden
        self.base_vbias = numpy.asarray(base_vbias, dtype=numpy.float32).reshape(V)
        self._base = eng.to_device(self.base_vbias)
        W = rbm.W.tensor
        self.v = eng.alloc_matrix(M * R, V, padded_ld(V))
        self.h = eng.alloc_matrix(M * R, H, W.stride(0))
        if start_h is not None:
            s = as_tensor(start_h, eng)
            if tuple(s.shape) == (M, H):             # one row per ladder: every temperature starts there
                s = s.repeat_interleave(R, dim=0)
            if tuple(s.shape) != (M * R, H):
                raise ValueError("start_h must be [%d, %d] or [%d, %d], got %r" % (M, H, M * R, H, tuple(s.shape)))
            self.h.copy_(s)
        self.rank = torch.arange(R, dtype=torch.int32).repeat(M, 1).to(eng.device).contiguous()
        self.n_done = 0                              # sweeps run so far: the swap parity continues across run() calls

    # ------------------------------------------------------------------ sweeps
    def run(self, n_sweeps, burn_in=0, path=0, trace=False, steps_per_launch=0):
        """``n_sweeps`` sweeps.  Returns ``(v_avg [M, V], h_avg [M, H], acceptance [R - 1])``: per ladder the means over the
        sweeps ``burn_in .. n_sweeps - 1`` of the beta = 1 visible mean / hidden mean of the slot that holds the top rank,
        and the accepted share of the swap attempts of every neighbour pair (NaN for a pair never tried); with ``trace``
        followed by ``trace_v [n, M R, V]``, ``trace_h [n, M R, H]``, ``trace_swaps [n, M, 2, R]`` (the rank map after the
        swap; per lower rank 1 / 0 / -1 = accepted / refused / not attempted).  Advances the layer's RNG step by 3 n."""
        out, tries = self._sweeps(n_sweeps, burn_in, path, trace, steps_per_launch)
        tries = tries.astype(numpy.float64)
        with numpy.errstate(divide="ignore"):
            inv = torch.from_numpy(1.0 / tries).to(out[0].device)
        acceptance = out[0].to(torch.float64) * inv
        acceptance[torch.from_numpy(tries == 0).to(out[0].device)] = float("nan")
        wrap = self.rbm._wrap
        return (wrap(out[1]), wrap(out[2]), wrap(acceptance)) + tuple(out[3:])

    def _sweeps(self, n_sweeps, burn_in, path, trace, steps_per_launch, zacc=None, trace_work=False):
        n, burn_in = int(n_sweeps), int(burn_in)
        if n < 1 or not 0 <= burn_in < n:
            raise ValueError("need n_sweeps >= 1 and 0 <= burn_in < n_sweeps, got %d, %d" % (n, burn_in))
        rbm, eng = self.rbm, self.engine
        step = rbm._rng_step
        rng = RngAddr(rbm.theano_rng.seed, rbm.stream_id, step, 0, 0)
        works = {} if zacc is None and not trace_work else dict(zacc=zacc, trace_work=trace_work)
        if rbm.visible_groups is not None:
            if not hasattr(eng, "temper_grouped"):          # (the eager sweep below would draw a group as independent sigmoid units)
                rbm._no_groups("tempering on this engine")
            out = eng.temper_grouped(rbm.W.tensor, rbm.hbias.tensor, rbm.vbias.tensor, self._base, self.betas, self.v, self.h,
                                     self.rank, n, rng, rbm.visible_groups, burn_in=burn_in, sweep0=self.n_done, path=path,
                                     steps_per_launch=steps_per_launch, trace=trace, **works)
        elif hasattr(eng, "temper"):
            out = eng.temper(rbm.W.tensor, rbm.hbias.tensor, rbm.vbias.tensor, self._base, rbm.gauss, self.betas, self.v,
                             self.h, self.rank, n, rng, burn_in=burn_in, sweep0=self.n_done, path=path,
                             steps_per_launch=steps_per_launch, trace=trace, **works)
        else:
            out = self._eager(n, burn_in, rng, trace, **works)
        rbm._rng_step = step + 3 * n
        tries = attempts(self.n_ladders, self.n_betas, self.n_done, n)
        self.n_done += n
        return out, tries

    # ------------------------------------------------------------------ log Z from the works of the swap attempts
    def accumulate_works(self, n_sweeps, burn_in=0, path=0, steps_per_launch=0, zacc=None, trace_work=False):
        """``n_sweeps`` sweeps that add the works of the swap attempts of the sweeps ``burn_in .. n_sweeps - 1`` to ``zacc``
        (float64 tensor [M, R - 1, 4] on the engine's device, updated in place; None: a fresh one from ``new_works``).
        Returns ``(zacc, accepted [R - 1] int64 numpy, works)`` with ``works`` the tapped (d_fwd, d_rev) [n, M, R - 1, 2]
        (float64 numpy, NaN where a pair was not tried) if ``trace_work``, else None.  The chains move exactly as under
        ``run``; calls accumulate: 12 sweeps then 8 leave in ``zacc`` what 20 do."""
        if zacc is None:
            zacc = torch.from_numpy(new_works(self.n_ladders, self.n_betas)).to(self.h.device)
        out, _ = self._sweeps(n_sweeps, burn_in, path, False, steps_per_launch, zacc=zacc, trace_work=trace_work)
        return zacc, out[0].cpu().numpy().astype(numpy.int64), (out[3].cpu().numpy() if trace_work else None)

    def log_partition(self, n_sweeps, burn_in, path=0, method="mid", steps_per_launch=0):
        """``LogZ`` of the layer from ``n_sweeps`` further sweeps of these ladders: the works of the swap attempts of the
        sweeps from ``burn_in`` on bridge every pair of neighbouring temperatures, log Z_{rho+1} / Z_rho = log E_rho[exp d_fwd]
        = -log E_{rho+1}[exp d_rev] (biased low / high: the bracket AIS lacks), chained from the closed-form log Z of
        beta = 0.  ``method``: "mid" = the mean of the two per pair, from accumulators kept on the device (32 bytes per
        ladder and pair, whatever n_sweeps); "bar" = Bennett's acceptance ratio, solved on the host from a tap of every
        work: 16 bytes per sweep, ladder and pair on the device and again on the host (1200 sweeps of 64 x 16 ladders:
        18 MB).  ``stderr`` is the delete-one-ladder jackknife.  Needs betas[0] = 0 and an attempt of every pair after
        burn-in.  Advances the layer's RNG step by 3 n like ``run``."""
        if method not in ("mid", "bar"):
            raise ValueError("method must be 'mid' or 'bar', got %r" % (method,))
        if self.betas[0] != 0.0:
            raise ValueError("log_partition needs betas[0] = 0 (the base-rate model), got %g" % self.betas[0])
        n, burn_in = int(n_sweeps), int(burn_in)
        if n < 1 or not 0 <= burn_in < n:
            raise ValueError("need n_sweeps >= 1 and 0 <= burn_in < n_sweeps, got %d, %d" % (n, burn_in))
        tries = attempts(self.n_ladders, self.n_betas, self.n_done + burn_in, n - burn_in)
        if (tries == 0).any():
            raise ValueError("a neighbour pair has no swap attempt after burn-in: run at least two sweeps after it")
        all_tries = attempts(self.n_ladders, self.n_betas, self.n_done, n)
        zacc, accepted, works = self.accumulate_works(n, burn_in, path, steps_per_launch, trace_work=method == "bar")
        log_z0 = base_log_partition(self.base_vbias, self.rbm.n_hidden, self.rbm.gauss, groups=self.rbm.visible_groups)
        r = estimate_log_z(zacc.cpu().numpy(), tries, log_z0, method, None if works is None else works[burn_in:])
        return r._replace(acceptance=accepted / all_tries.astype(numpy.float64))

    def _eager(self, n, burn_in, rng, trace, zacc=None, trace_work=False):
        """The sweep of include/mdbn_hip.h (mdbn_pt_run / mdbn_pt_run_z) from the engine's eager calls, in the engine's own
        precision; the works are combined and accumulated in float64 with float32 exponentials, as the device does."""
        rbm, eng = self.rbm, self.engine
        W, c, b = rbm.W.tensor, rbm.hbias.tensor, rbm.vbias.tensor
        M, R, gauss = self.n_ladders, self.n_betas, bool(rbm.gauss)
        V, H = W.shape
        dt = W.dtype
        bA = self._base.to(dt)
        db = b - bA
        betas = torch.from_numpy(self.betas).to(dt)
        zero_v = torch.zeros(V, dtype=dt)
        rank = self.rank.to(torch.int64)
        rows = torch.arange(M)[:, None]
        v_sum, h_sum = torch.zeros((M, V), dtype=dt), torch.zeros((M, H), dtype=dt)
        accepted = torch.zeros(R - 1, dtype=torch.int32)
        tv, th, ts, tw = [], [], [], []
        g = float((db.to(torch.float64) ** 2).sum())

        def u(rws, cols, st, normal=False):
            return eng.rng_uniform(rws, cols, RngAddr(rng.seed, rng.stream_id, st, 0, 0), normal)

        h = self.h
        for t in range(n):
            sw, st = self.n_done + t, rng.step + 3 * t
            flat = rank.reshape(-1)
            beta = betas[flat][:, None]
            top = (flat == R - 1)
            # 1. v | h at the row's beta (propdown without bias or activation: the Gaussian pass of a zero bias)
            m = eng.propdown(h, W, zero_v, gauss=True, add_noise=False)[1].to(dt)
            pre = bA[None, :] + beta * db[None, :] + beta * m
            if gauss:
                v = pre + u(M * R, V, st, True).to(dt)
                mean1 = pre
            else:
                v = (u(M * R, V, st).to(dt) < torch.sigmoid(pre)).to(dt)
                mean1 = torch.sigmoid(pre)
            # 2. a = v W + c and the two shares of l(beta_partner) - l(beta_own)
            a = eng.propup(v, W, c, want_mean=False, want_sample=False)[0].to(dt)
            partner = torch.where((flat - sw) % 2 == 0, flat + 1, flat - 1)
            paired = (partner >= 0) & (partner < R)
            bp = torch.where(paired, betas[partner.clamp(0, R - 1)], betas[flat])[:, None]
            sp = torch.nn.functional.softplus
            hsum = (sp(bp * a) - sp(beta * a)).sum(dim=1).reshape(M, R)
            s1 = (((v - bA[None, :]) if gauss else v) * db[None, :]).sum(dim=1).reshape(M, R)
            # 3. the swaps of the pairs of this sweep's parity
            inv = torch.argsort(rank, dim=1)
            logu = torch.log(u(M, R - 1, st + 1).to(torch.float64))
            dec = torch.full((M, R), -1, dtype=torch.int32)
            work = torch.full((M, R - 1, 2), float("nan"), dtype=torch.float64)
            for rho in range(sw % 2, R - 1, 2):
                i, j = inv[:, rho], inv[:, rho + 1]
                delta = (hsum[rows[:, 0], i] + hsum[rows[:, 0], j]
                         + (betas[rho + 1] - betas[rho]) * (s1[rows[:, 0], i] - s1[rows[:, 0], j])).to(torch.float64)
                acc = logu[:, rho] < delta
                if zacc is not None or trace_work:
                    b_lo, b_hi = float(betas[rho]), float(betas[rho + 1])
                    gq = 0.5 * (b_hi * b_hi - b_lo * b_lo) * g if gauss else 0.0
                    f64 = lambda x, k: x[rows[:, 0], k].to(torch.float64)
                    work[:, rho, 0] = f64(hsum, i) + (b_hi - b_lo) * f64(s1, i) - gq
                    work[:, rho, 1] = f64(hsum, j) - (b_hi - b_lo) * f64(s1, j) + gq
                    if zacc is not None and t >= burn_in:
                        for k in (0, 1):
                            d, m0, s0 = work[:, rho, k], zacc[:, rho, 2 * k], zacc[:, rho, 2 * k + 1]
                            m1 = torch.maximum(m0, d)
                            e = lambda x: torch.exp(x.to(torch.float32)).to(torch.float64)
                            zacc[:, rho, 2 * k + 1] = s0 * e(m0 - m1) + e(d - m1)
                            zacc[:, rho, 2 * k] = m1
                dec[:, rho] = acc.to(torch.int32)
                accepted[rho] += int(acc.sum())
                rank[rows[acc, 0], i[acc]] = rho + 1
                rank[rows[acc, 0], j[acc]] = rho
            # 4. h | v at the rank after the swap
            flat = rank.reshape(-1)
            p = torch.sigmoid(betas[flat][:, None] * a)
            h = (u(M * R, H, st + 2).to(dt) < p).to(dt)
            if t >= burn_in:
                v_sum = v_sum + mean1[top]
                h_sum = h_sum + p[flat == R - 1]
            if trace:
                tv.append(v)
                th.append(h)
                ts.append(torch.stack([rank.to(torch.int32), dec], dim=1))
            if trace_work:
                tw.append(work)
        self.v.copy_(v)
        self.h.copy_(h)
        self.rank.copy_(rank.to(torch.int32))
        out = (accepted, v_sum / (n - burn_in), h_sum / (n - burn_in))
        if trace:
            out += (torch.stack(tv), torch.stack(th), torch.stack(ts))
        if trace_work:
            out += (torch.stack(tw),)
        return out

    # ------------------------------------------------------------------ the beta = 1 replicas
    def _top_rows(self):
        """Global row of each ladder's beta = 1 holder (device int64 [M]); no host synchronisation."""
        R = self.n_betas
        slot = (self.rank == R - 1).to(torch.int64).argmax(dim=1)
        return torch.arange(self.n_ladders, device=slot.device) * R + slot

    def samples(self):
        """``(v, h)`` of each ladder's beta = 1 holder: [M, V], [M, H]."""
        rows = self._top_rows()
        return self.rbm._wrap(self.v[rows]), self.rbm._wrap(self.h[rows])

    def to_persistent(self, persistent):
        """Copy the beta = 1 hidden rows into the [n_ladders, H] PCD chain buffer ``persistent`` (exact)."""
        t = persistent.tensor if isinstance(persistent, SharedArray) else persistent
        t.copy_(self.h[self._top_rows()])
        return persistent

    def from_persistent(self, persistent):
        """Copy the [n_ladders, H] PCD chain buffer ``persistent`` into the beta = 1 hidden rows (exact)."""
        t = persistent.tensor if isinstance(persistent, SharedArray) else persistent
        self.h[self._top_rows()] = t.to(self.h.dtype)
        return self
