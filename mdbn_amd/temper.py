"""Parallel tempering of a trained RBM / GRBM: ``TemperedChains`` (RBM.tempered_chains) holds M ladders of R Gibbs chains at
the inverse temperatures 0 <= beta_0 < ... < beta_{R-1} = 1 of the tempered family of the AIS estimate (base-rate visible
bias b_A, b_beta = b_A + beta (b - b_A)) and advances them by sweeps with swaps between neighbouring temperatures
(csrc/mdbn_temper.hip, include/mdbn_hip.h: mdbn_pt_run).  On an engine without ``temper`` (the CPU checker of the tests) the
sweep is composed from the engine's eager calls: the same definitions, stated in Python."""
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
        n, burn_in = int(n_sweeps), int(burn_in)
        if n < 1 or not 0 <= burn_in < n:
            raise ValueError("need n_sweeps >= 1 and 0 <= burn_in < n_sweeps, got %d, %d" % (n, burn_in))
        rbm, eng = self.rbm, self.engine
        step = rbm._rng_step
        rng = RngAddr(rbm.theano_rng.seed, rbm.stream_id, step, 0, 0)
        if hasattr(eng, "temper"):
            out = eng.temper(rbm.W.tensor, rbm.hbias.tensor, rbm.vbias.tensor, self._base, rbm.gauss, self.betas, self.v,
                             self.h, self.rank, n, rng, burn_in=burn_in, sweep0=self.n_done, path=path,
                             steps_per_launch=steps_per_launch, trace=trace)
        else:
            out = self._eager(n, burn_in, rng, trace)
        rbm._rng_step = step + 3 * n
        tries = attempts(self.n_ladders, self.n_betas, self.n_done, n).astype(numpy.float64)
        self.n_done += n
        with numpy.errstate(divide="ignore"):
            inv = torch.from_numpy(1.0 / tries).to(out[0].device)
        acceptance = out[0].to(torch.float64) * inv
        acceptance[torch.from_numpy(tries == 0).to(out[0].device)] = float("nan")
        wrap = rbm._wrap
        return (wrap(out[1]), wrap(out[2]), wrap(acceptance)) + tuple(out[3:])

    def _eager(self, n, burn_in, rng, trace):
        """The sweep of include/mdbn_hip.h (mdbn_pt_run) from the engine's eager calls, in the engine's own precision."""
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
        tv, th, ts = [], [], []

        def u(rws, cols, st, normal=False):
            return eng.rng_uniform(rws, cols, RngAddr(rng.seed, rng.stream_id, st, 0, 0), normal)

        h = self.h
        for t in range(n):
            g, st = self.n_done + t, rng.step + 3 * t
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
            partner = torch.where((flat - g) % 2 == 0, flat + 1, flat - 1)
            paired = (partner >= 0) & (partner < R)
            bp = torch.where(paired, betas[partner.clamp(0, R - 1)], betas[flat])[:, None]
            sp = torch.nn.functional.softplus
            hsum = (sp(bp * a) - sp(beta * a)).sum(dim=1).reshape(M, R)
            s1 = (((v - bA[None, :]) if gauss else v) * db[None, :]).sum(dim=1).reshape(M, R)
            # 3. the swaps of the pairs of this sweep's parity
            inv = torch.argsort(rank, dim=1)
            logu = torch.log(u(M, R - 1, st + 1).to(torch.float64))
            dec = torch.full((M, R), -1, dtype=torch.int32)
            for rho in range(g % 2, R - 1, 2):
                i, j = inv[:, rho], inv[:, rho + 1]
                delta = (hsum[rows[:, 0], i] + hsum[rows[:, 0], j]
                         + (betas[rho + 1] - betas[rho]) * (s1[rows[:, 0], i] - s1[rows[:, 0], j])).to(torch.float64)
                acc = logu[:, rho] < delta
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
        self.v.copy_(v)
        self.h.copy_(h)
        self.rank.copy_(rank.to(torch.int32))
        out = (accepted, v_sum / (n - burn_in), h_sum / (n - burn_in))
        if trace:
            out += (torch.stack(tv), torch.stack(th), torch.stack(ts))
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
