"""HipEngine: the device side of the RBM/DBN classes.

Owns nothing but a context handle and scratch tensors; every method enqueues work on
torch's current HIP stream through the C-ABI (mdbn_amd/_lib.py) and returns device
tensors.  PyTorch is used only as the device-array container (allocation, views,
H2D/D2H copies, streams).  There is no CPU fallback: constructing the engine without
the built library or without a gfx950 GPU raises.

Matrix convention: a device matrix is a torch view [rows, cols] over storage
[rows, ld] with ld = padded_ld(cols) (a multiple of 4) and zero padding (``alloc_matrix``).
"""
import ctypes as C
import os as _os
from collections import namedtuple

import numpy
import torch

from . import _lib


def round_up4(n):
    return (int(n) + 3) & ~3


def padded_ld(cols):
    """Leading dimension of a device matrix (same policy as mdbn_padded_ld in the library):
    round_up(cols, 4).  (Padding power-of-two rows was measured and rejected, see mdbn_capi.hip.)"""
    return round_up4(cols)


_default_engine = None


def get_engine():
    """Process-wide default engine (cuda:current device); created on first use."""
    global _default_engine
    if _default_engine is None:
        _default_engine = HipEngine()
    return _default_engine


def set_engine(engine):
    """Install ``engine`` as the default (tests install a CPU checker here)."""
    global _default_engine
    _default_engine = engine
    return engine


class RngAddr(object):
    """Address of one random matrix: see csrc/philox.h."""
    __slots__ = ("seed", "stream_id", "step", "draw", "row_offset")

    def __init__(self, seed, stream_id, step, draw=0, row_offset=0):
        self.seed, self.stream_id, self.step = int(seed), int(stream_id), int(step)
        self.draw, self.row_offset = int(draw), int(row_offset)

    def c(self):
        return _lib.Rng(self.seed & 0xFFFFFFFFFFFFFFFF, self.stream_id & 0xFFFFFFFF,
                        self.step & 0xFFFFFFFF, self.draw & 0xFFFFFFFF, 0, self.row_offset)


# Ahead: what a step prepared for the next one (CDScratch.ahead; before the call: what it announces) -- the data matrix and the
# index tensor (kept alive) with their version counters, the X2 buffer the rows are in; ``params``: None on the plane path, on
# the thin-batch path, whose hand-over also covers x W, the AheadParams those products were computed from.
# CdCall: what _cd_args resolved for one call (``keep``: what else must live until it is enqueued; ``announce``: an Ahead without
# params, or None; ``thin``: the thin-batch hand-over rules apply); with W the token of cd_forward.
# StepCache: the argument structs a step function keeps for its next single-device call (cd_train_step_cached), their byref()s,
# the key they are valid under (_step_cache_key), the scratch and the tensors the structs point into.
Ahead = namedtuple("Ahead", "data data_version indexes buffer index_version params")
AheadParams = namedtuple("AheadParams", "W_ptr W_version W_serial options_epoch")
CdCall = namedtuple("CdCall", "args stats scratch data indexes keep announce thin")
StepCache = namedtuple("StepCache", "args update args_ref update_ref key scratch W tensors")


class GroupTable(object):
    """The table of a layer with K-ary softmax visible units (``utils.group_boundaries``), in the two copies the library
    takes: ``tensor`` (int32, on the engine's device: what the kernel reads) and ``host`` (int32 numpy: what the library
    checks before a launch).  Immutable: a layer that changes its groups gets a new table."""

    def __init__(self, engine, boundaries):
        self.host = numpy.ascontiguousarray(boundaries, dtype=numpy.int32)
        self.host.setflags(write=False)
        self.tensor = torch.from_numpy(self.host.copy()).to(engine.device)
        self.n_groups = int(self.host.size - 1)

    def spans(self):
        """[(first column, end column), ...] of the groups."""
        return [(int(a), int(b)) for a, b in zip(self.host[:-1], self.host[1:])]


class CDScratch(object):
    """Per-(B, V, H) buffers of one CD step; see mdbn_cd_args in include/mdbn_hip.h."""

    def __init__(self, engine, B, V, H, need_vs, ldv, ldh):
        self.B, self.V, self.H = B, V, H
        self.V2 = engine.alloc_matrix(2 * B, V, ldv)       # same ld as the data matrix
        self.P2 = engine.alloc_matrix(2 * B, H, ldh)       # same ld as W
        self.hs = engine.alloc_matrix(B, H, ldh)
        self.vs = engine.alloc_matrix(B, V, ldv) if need_vs else None
        self.trace_h = self.trace_v = None      # chain taps (HipEngine.trace_chain), [k+1, B, ldh] / [k, B, ldv]
        # bf16 plane scratch (mdbn_cd_args.planes) for shapes made of whole 128-row / 128-column tiles
        self.planes = None
        if engine.plane_shape(B, V, H, ldv, ldh):
            n = C.c_int64()
            _lib.check(engine.lib.mdbn_planes_bytes(B, ldv, ldh, C.byref(n)), "mdbn_planes_bytes")
            self.planes = torch.empty(n.value // 2, dtype=torch.int16, device=engine.device)
        # gather-ahead (mdbn_cd_args.next_indexes): second X2-plane buffer (made on first use), the buffer the current
        # step uses, and what the last step gathered ahead (an Ahead, or None)
        self.planes_alt = None
        self.x_buffer = 0
        self.ahead = None

    def alt_planes(self, engine, ldv):
        if self.planes_alt is None:
            n = C.c_int64()
            _lib.check(engine.lib.mdbn_ahead_bytes_ctx(engine.ctx, self.B, self.V, self.H, ldv, self.P2.stride(0), C.byref(n)),
                       "mdbn_ahead_bytes_ctx")
            self.planes_alt = torch.empty(n.value // 2, dtype=torch.int16, device=engine.device)
        return self.planes_alt


class RowFeeder(object):
    """``mdbn_feeder_*`` (include/mdbn_hip.h): minibatches of a host-resident table, gathered by CPU threads into pinned
    staging and moved by one copy each on the feeder's copy stream, ``slots`` deep.  ``submit`` returns a ticket at once;
    ``acquire(ticket)`` (submission order) makes the current stream wait for that minibatch's copy and returns its device
    rows; ``release(ticket)`` after the work reading them has been enqueued."""

    def __init__(self, engine, host, cols, max_rows, slots, threads):
        self.engine, self.host, self.cols, self.max_rows = engine, host, int(cols), int(max_rows)
        self.bufs = [engine.alloc_matrix(self.max_rows, self.cols, host.stride(0)) for _ in range(slots)]
        ptrs = (C.c_void_p * slots)(*[b.data_ptr() for b in self.bufs])
        self.handle = C.c_void_p()
        _lib.check(engine.lib.mdbn_feeder_create(engine.ctx, C.c_void_p(host.data_ptr()), host.shape[0], self.cols,
                                                 host.stride(0), self.max_rows, slots, ptrs, self.bufs[0].stride(0),
                                                 int(threads), C.byref(self.handle)), "mdbn_feeder_create")

    def submit(self, indexes, n=None):
        """``indexes``: CPU int64 tensor (or None with ``n``: the table's first n rows)."""
        t = C.c_int64()
        if indexes is None:
            _lib.check(self.engine.lib.mdbn_feeder_submit(self.handle, None, int(n), C.byref(t)), "mdbn_feeder_submit")
        else:
            assert indexes.dtype == torch.int64 and indexes.device.type == "cpu" and indexes.is_contiguous()
            _lib.check(self.engine.lib.mdbn_feeder_submit(self.handle, C.c_void_p(indexes.data_ptr()), indexes.numel(),
                                                         C.byref(t)), "mdbn_feeder_submit")
        return t.value

    def acquire(self, ticket, rows):
        slot = C.c_int32()
        _lib.check(self.engine.lib.mdbn_feeder_acquire(self.handle, int(ticket), self.engine._stream(), C.byref(slot)),
                   "mdbn_feeder_acquire")
        return self.bufs[slot.value][:rows]

    def release(self, ticket):
        _lib.check(self.engine.lib.mdbn_feeder_release(self.handle, int(ticket), self.engine._stream()), "mdbn_feeder_release")

    def stats(self):
        """Host-side time per stage since the last call (resets): dict of counts and mean microseconds."""
        out = (C.c_double * 5)()
        _lib.check(self.engine.lib.mdbn_feeder_stats(self.handle, out), "mdbn_feeder_stats")
        return {"fed": int(out[0]), "gather_us": out[1], "copy_enqueue_us": out[2], "acquired": int(out[3]),
                "acquire_wait_us": out[4]}

    def cancel(self):
        _lib.check(self.engine.lib.mdbn_feeder_cancel(self.handle), "mdbn_feeder_cancel")

    def close(self):
        if getattr(self, "handle", None):
            self.engine.lib.mdbn_feeder_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipEngine(object):
    name = "hip"

    def __init__(self, device=None):
        self.lib = _lib.load()                      # raises if the extension is not built
        if not torch.cuda.is_available():
            raise _lib.MdbnError("no HIP device visible: mdbn_amd has no CPU fallback")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.MdbnError("HipEngine needs a HIP device, got %r" % (device,))
        # 'cuda' without an index means the current device: fixed ONCE here (the raw-stream lookup and mdbn_ctx_create both
        # take the index; an engine must not follow later torch.cuda.set_device calls)
        self.device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
        ctx = C.c_void_p()
        _lib.check(self.lib.mdbn_ctx_create(C.byref(ctx), self.device.index), "mdbn_ctx_create")
        self.ctx = ctx
        self._workspace = None
        self._workspace_need = 0        # bytes the shared workspace was allocated for
        self._options_epoch = 0         # bumped by set_option: argument structs cached by step functions are then stale
        self._w_serial = 0              # bumped by every library call that writes parameters (what a positive phase computed
                                        # ahead of its step was computed FROM: _ahead_valid)
        self._ws_need = {}              # (B, V, H) -> bytes the library asks for (options that change it clear this)
        self._stats = {}
        self._scratch = {}
        self._cost_ring = torch.zeros(1024, dtype=torch.float32, device=self.device)
        self._cost_slot = 0
        self.last_scratch = None        # CDScratch of the most recent CD step (inspection / chain taps)
        # MDBN_OPTIONS="name=value,name=value": library knobs of every context this process creates (A/B runs of the
        # bench scripts without editing them; unknown names fail as mdbn_set_option does)
        for item in filter(None, _os.environ.get("MDBN_OPTIONS", "").split(",")):
            name, _, value = item.partition("=")
            self.set_option(name.strip(), int(value))

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.lib.mdbn_ctx_destroy(self.ctx)
        except Exception:
            pass

    # ------------------------------------------------------------------ arrays
    def alloc_matrix(self, rows, cols, ld=None):
        ld = padded_ld(cols) if ld is None else int(ld)
        return torch.zeros((rows, ld), dtype=torch.float32, device=self.device)[:, :cols]

    def alloc_vector(self, n):
        return torch.zeros(int(n), dtype=torch.float32, device=self.device)

    def to_device(self, value):
        """numpy / tensor -> padded device matrix (2-D) or vector (1-D), float32."""
        if isinstance(value, torch.Tensor):
            t = value.to(device=self.device, dtype=torch.float32)
        else:
            t = torch.from_numpy(numpy.ascontiguousarray(value, dtype=numpy.float32)).to(self.device)
        if t.dim() == 2:
            if t.device == self.device and self.is_matrix(t) and t is value:
                return t
            out = self.alloc_matrix(t.shape[0], t.shape[1])
            out.copy_(t)
            return out
        return t.contiguous()

    @staticmethod
    def is_matrix(t):
        return (t.dim() == 2 and t.dtype == torch.float32 and t.stride(1) == 1
                and t.stride(0) % 4 == 0 and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0)

    def as_matrix(self, x):
        """Accept numpy arrays, tensors or SharedArray-likes; return a device matrix."""
        t = getattr(x, "tensor", x)
        if isinstance(t, torch.Tensor) and t.device == self.device and self.is_matrix(t):
            return t
        return self.to_device(t)

    def to_numpy(self, t):
        return t.detach().cpu().numpy()

    trace_chain = False         # True: every CD step also records the samples its Gibbs chain feeds onward
    keep_f32 = False            # True: the plane path also stores the float32 copies of ph / nh / nv / samples in the
                                # CD scratch (CDScratch.P2, V2[B:], hs, vs) for inspection; nothing on the path reads them
    host_feed_threads = 8           # CPU threads of a RowFeeder's gather (85 us per 8.4-MB minibatch on the GPU box's host; 16: 67)
    host_gather_workgroups = 32     # workgroups x threads of the PCIe gather of a host-resident table (mdbn_gather_rows_host)
    host_gather_threads = 256
    check_indexes = False       # True: also range-check index lists that already live on the device (one sync)

    def index_tensor(self, indexes, n_rows=None):
        """Minibatch indices -> device int32/int64 tensor (no copy if already there).  With ``n_rows``
        host index lists are range-checked like numpy fancy indexing (IndexError; negative indices
        count from the end) -- the gather kernel itself clamps instead of faulting."""
        if isinstance(indexes, torch.Tensor):
            if indexes.dtype not in (torch.int32, torch.int64):
                indexes = indexes.to(torch.int64)
            if n_rows is not None and indexes.numel() and (self.check_indexes or indexes.device.type == "cpu"):
                lo, hi = int(indexes.min()), int(indexes.max())
                if lo < -n_rows or hi >= n_rows:
                    raise IndexError("minibatch index out of range for %d rows: [%d, %d]" % (n_rows, lo, hi))
            return indexes.to(self.device).contiguous()
        a = numpy.asarray(indexes)
        if a.dtype not in (numpy.int32, numpy.int64):
            a = a.astype(numpy.int64)
        if n_rows is not None and a.size and (a.min() < -n_rows or a.max() >= n_rows):
            raise IndexError("minibatch index out of range for %d rows: [%d, %d]" % (n_rows, a.min(), a.max()))
        return torch.from_numpy(numpy.ascontiguousarray(a)).to(self.device)

    # ------------------------------------------------------------------ scratch
    def _stream(self):
        # (torch.cuda.current_stream() builds a Stream object: 5 us per call -- a sixth of a small layer's step)
        return C.c_void_p(torch._C._cuda_getCurrentRawStream(self.device.index))

    def workspace(self, B, V, H, ldv=None, ldh=None):
        """One shared workspace, grown to the largest requirement seen.  The requirement is NOT monotone in (B, V, H) (a
        smaller minibatch takes more split-K slabs), so every shape asks the library (cached per shape).  ``ldv`` / ``ldh``:
        the leading dimensions of a CD step (its column-sum regions lie on them: mdbn_workspace_bytes_ld)."""
        key = (B, V, H) if ldv is None else (B, V, H, ldv, ldh)
        need = self._ws_need.get(key)
        if need is None:
            n = C.c_int64()
            if ldv is None:
                _lib.check(self.lib.mdbn_workspace_bytes_ctx(self.ctx, B, V, H, C.byref(n)), "mdbn_workspace_bytes_ctx")
            else:
                _lib.check(self.lib.mdbn_workspace_bytes_ld_ctx(self.ctx, B, V, H, ldv, ldh, C.byref(n)), "mdbn_workspace_bytes_ld_ctx")
            need = self._ws_need[key] = max(n.value, self.WS_FLOOR)
        if self._workspace is None or self._workspace_need < need:
            self._workspace = self._alloc_scratch(need, "workspace")
            self._workspace_need = need
        return self._workspace

    WS_FLOOR = 8 << 20          # the shared workspace is never smaller: one allocation serves nearly every shape of a run
    WS_PAD = 64                 # floats behind every scratch buffer (keeps a regrown buffer off the allocator's size classes)

    def _alloc_scratch(self, nbytes, what):
        """Every caller-owned workspace of a library call comes from here: an uninitialised float32 tensor that holds at
        least ``nbytes`` bytes; ``what`` names its use.  The library is told ``numel() * 4`` bytes."""
        return torch.empty(int(nbytes) // 4 + self.WS_PAD, dtype=torch.float32, device=self.device)

    def new_stats_buffer(self, V, H, ldv=None, ldh=None):
        """A packed [S | s_h | s_v | cost] buffer owned by the caller (a step function whose statistics
        must survive until a deferred update reads them keeps its own, never the engine's shared one)."""
        ldv = padded_ld(V) if ldv is None else ldv
        ldh = padded_ld(H) if ldh is None else ldh
        n = C.c_int64()
        _lib.check(self.lib.mdbn_stats_floats(V, ldv, ldh, C.byref(n)), "mdbn_stats_floats")
        return torch.zeros(n.value, dtype=torch.float32, device=self.device)

    def stats_buffer(self, V, H, slot=0, ldv=None, ldh=None):
        """Engine-wide scratch statistics buffer (consumed before the call that filled it returns)."""
        ldv = padded_ld(V) if ldv is None else ldv
        ldh = padded_ld(H) if ldh is None else ldh
        key = (V, H, slot, ldv, ldh)
        if key not in self._stats:
            self._stats[key] = self.new_stats_buffer(V, H, ldv, ldh)
        return self._stats[key]

    def cd_scratch(self, B, V, H, need_vs, ldv=None, ldh=None):
        ldv = padded_ld(V) if ldv is None else ldv
        ldh = padded_ld(H) if ldh is None else ldh
        key = (B, V, H, bool(need_vs), ldv, ldh)
        if key not in self._scratch:
            if len(self._scratch) > 8:
                self._scratch.clear()
            self._scratch[key] = CDScratch(self, B, V, H, need_vs, ldv, ldh)
        return self._scratch[key]

    @staticmethod
    def _p(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    # ------------------------------------------------------------------ bf16 planes of W
    # The plane path pays for itself on big layers only (measured, scripts/step_ab.py gemm_planes 0 1 with
    # MDBN_AB_SHAPE: 4096->1024 at B = 512 158.7 -> 150 us, 2048->1024 122.9 -> 118.9; but 1024->256 69.2 -> 77.3,
    # 1024->512 at B = 256 68.1 -> 74.9, 2048->512 at B = 128 72.0 -> 80.6, 1024->1024 at B = 1024 112.0 -> 114.0):
    # B * V * H >= planes_min_work and V * H >= 2^21.  Mirrors mdbn_set_option("planes_min_work"); tests set 0.
    planes_min_work = 1 << 30

    def weight_ld(self, V, H):
        """Leading dimension of a [V, H] weight matrix.  A big layer whose hidden width is not a multiple of 128 (the
        reference's 2048 -> 400 gene-expression layer, AMLsm2.py / MDBN.py presets) gets its rows padded to the next
        multiple: the plane path (bf16 planes + LDS-DMA GEMMs, whole 128-column tiles) then serves it on the padded
        width, the pad columns holding exact zeros -- 2048 -> 400 CD-5 at B = 512: 393 us on the exact-f32 tile kernels,
        which is what a ragged width falls back to.  None: the default (padded_ld)."""
        if V % 128 == 0 and H % 128 != 0 and H > 128:
            He = (H + 127) // 128 * 128
            if V * He >= self.weight_ld_min_elems:
                return He
        return None

    weight_ld_min_elems = int(_os.environ.get("MDBN_WEIGHT_LD_MIN", 1 << 21))      # smallest V * padded H that is padded

    def plane_shape(self, B, V, H, ldv, ldh):
        """Shapes the plane path of the library takes under THIS engine's options: asked of the library itself
        (mdbn_planes_eligible_ctx), so the host's buffers and the library's choice of path cannot disagree."""
        ok = C.c_int32()
        _lib.check(self.lib.mdbn_planes_eligible_ctx(self.ctx, B, V, H, ldv, ldh, C.byref(ok)), "mdbn_planes_eligible_ctx")
        return bool(ok.value)

    def set_planes_min_work(self, work):
        """Smallest B * V * H the plane path serves (0: every whole-tile shape).  Library options belong to the context:
        this changes the rule for this engine only."""
        self.planes_min_work = int(work)
        self.set_option("planes_min_work", int(work))

    def set_option(self, name, value):
        """Library tuning knob (mdbn_set_option), e.g. ``set_option('gemm_bk', 32)``; of this engine's context only."""
        _lib.check(self.lib.mdbn_set_option(self.ctx, name.encode(), int(value)), "mdbn_set_option")
        self._options_epoch += 1         # (cached argument structs of step functions: stale)
        self._scratch.clear()            # options decide which scratch a shape needs (planes, slabs)
        self._ws_need.clear()            # ... and how many split-K slabs its workspace holds

    def w_planes(self, W, create=False):
        """(planes, valid) for a weight matrix: the [3, V, ldh] bf16 planes the library keeps in step with W, and
        whether they hold the split of the CURRENT W.  A torch-side write to W (set_value, checkpoint load) bumps
        the tensor's version and invalidates them; the library's own updates rewrite them."""
        # kept ON the tensor object (the one a SharedArray holds for its lifetime), never keyed by address: a new
        # matrix that reuses a freed one's memory must not inherit its planes
        ent = getattr(W, "_mdbn_planes", None)
        if ent is None or tuple(ent[0].shape[1:]) != (W.shape[0], W.stride(0)) or ent[2] != W.data_ptr():
            if not create:
                return None, False
            ent = [torch.empty((3, W.shape[0], W.stride(0)), dtype=torch.int16, device=self.device), None, W.data_ptr()]
            W._mdbn_planes = ent
        return ent[0], ent[1] == W._version

    def _w_planes_written(self, W):
        ent = getattr(W, "_mdbn_planes", None)
        if ent is not None:
            ent[1] = W._version

    # ------------------------------------------------------------------ propagation
    def propup(self, v, W, hbias, rng=None, want_pre=True, want_mean=True, want_sample=True):
        """[pre, mean, sample] of rbm.py:187-213; entries not wanted are None."""
        v = self.as_matrix(v)
        B, V = v.shape
        H = W.shape[1]
        assert W.shape[0] == V, "visible size mismatch: %d vs %d" % (V, W.shape[0])
        ldh = W.stride(0)                               # the C-ABI writes outputs with W's ld
        pre = self.alloc_matrix(B, H, ldh) if want_pre else None
        mean = self.alloc_matrix(B, H, ldh) if want_mean else None
        sample = self.alloc_matrix(B, H, ldh) if want_sample else None
        if B == 0:
            return pre, mean, sample
        ws = self.workspace(min(B, 4096), V, H)
        r = rng.c() if rng is not None else None
        _lib.check(self.lib.mdbn_propup_sample(
            self.ctx, self._stream(), self._p(v), B, v.stride(0), self._p(W), V, H, W.stride(0),
            self._p(hbias), self._p(pre), self._p(mean), 1.0, self._p(sample),
            C.byref(r) if r is not None else None, self._p(ws), ws.numel() * 4), "mdbn_propup_sample")
        return pre, mean, sample

    def propdown(self, h, W, vbias, gauss=False, add_noise=False, rng=None, v0=None, out=None):
        """[pre, mean, sample] of rbm.py:215-240 (RBM) / rbm.py:647-660 (GRBM).
        With ``v0`` also returns the un-normalised reconstruction-cost sum (device scalar).  ``out`` (a noise-free Gaussian
        pass only): the [B, V] matrix that receives the mean -- nothing is allocated and no sample is written; all three
        entries of the result are ``out``."""
        h = self.as_matrix(h)
        B, H = h.shape
        V = W.shape[0]
        assert W.shape[1] == H, "hidden size mismatch"
        if h.stride(0) != W.stride(0):                  # the C-ABI reads h with W's ld
            h2 = self.alloc_matrix(B, H, W.stride(0))
            h2.copy_(h)
            h = h2
        if out is not None:
            assert gauss and not add_noise and v0 is None and tuple(out.shape) == (B, V), "out=: the noise-free Gaussian mean"
            if B > 0:
                ws = self.workspace(min(B, 4096), V, H)
                _lib.check(self.lib.mdbn_propdown_sample(
                    self.ctx, self._stream(), self._p(h), B, h.stride(0), self._p(W), V, H, out.stride(0), self._p(vbias), 1, 0,
                    None, self._p(out), None, None, None, None, self._p(ws), ws.numel() * 4), "mdbn_propdown_sample")
            return out, out, out
        mean = self.alloc_matrix(B, V)
        sample = self.alloc_matrix(B, V)
        pre = mean if gauss else self.alloc_matrix(B, V)     # GRBM: "pre" is the mean (rbm.py:660)
        if B == 0:
            return (pre, mean, sample) if v0 is None else (pre, mean, sample, torch.zeros((), device=self.device))
        ws = self.workspace(min(B, 4096), V, H)
        r = rng.c() if rng is not None else None
        cost = None
        if v0 is not None:
            v0 = self.as_matrix(v0)
            if v0.stride(0) != mean.stride(0):          # target is read with the output's ld
                t = self.alloc_matrix(B, V, mean.stride(0))
                t.copy_(v0)
                v0 = t
            cost = torch.zeros(4, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.mdbn_propdown_sample(
            self.ctx, self._stream(), self._p(h), B, h.stride(0), self._p(W), V, H, mean.stride(0),
            self._p(vbias), int(bool(gauss)), int(bool(add_noise)),
            None if gauss else self._p(pre), self._p(mean), self._p(sample),
            C.byref(r) if r is not None else None, self._p(v0), self._p(cost),
            self._p(ws), ws.numel() * 4), "mdbn_propdown_sample")
        if cost is not None:
            return pre, mean, sample, cost[0]
        return pre, mean, sample

    def gibbs_chain(self, v, W, hbias, vbias, gauss, n_steps, rng, add_noise=False, want_pre=True):
        """n_steps of gibbs_vhv from the visible state ``v`` in ONE library call (mdbn_gibbs_chain): returns
        [pre_h, h_mean, h_sample, pre_v, v_mean, v_sample] of the last step; ``v`` itself is not modified."""
        v = self.as_matrix(v)
        B, V = v.shape
        H = W.shape[1]
        ldh = W.stride(0)
        state = self.alloc_matrix(B, V, v.stride(0))
        state.copy_(v)
        h_mean, h_sample = self.alloc_matrix(B, H, ldh), self.alloc_matrix(B, H, ldh)
        v_mean = self.alloc_matrix(B, V, v.stride(0))
        pre_h = self.alloc_matrix(B, H, ldh) if want_pre else None
        pre_v = self.alloc_matrix(B, V, v.stride(0)) if want_pre else None
        if B == 0:
            return [pre_h, h_mean, h_sample, pre_v, v_mean, state]
        ws = self.workspace(min(B, 4096), V, H)
        r = rng.c()
        _lib.check(self.lib.mdbn_gibbs_chain(
            self.ctx, self._stream(), self._p(state), B, state.stride(0), self._p(W), V, H, ldh, self._p(hbias),
            self._p(vbias), int(bool(gauss)), int(bool(add_noise)), int(n_steps), self._p(pre_h), self._p(h_mean),
            self._p(h_sample), self._p(pre_v), self._p(v_mean), C.byref(r), self._p(ws), ws.numel() * 4),
            "mdbn_gibbs_chain")
        return [pre_h, h_mean, h_sample, pre_v, v_mean, state]

    def _sampler_workspace(self, query, name, dims, H, ldh, path, extra=(), cache_attr=None):
        """The workspace of a sampler call: ``query(ctx, *dims, H, *extra, path, &bytes)`` is the library's sizer ``name``.
        ``cache_attr``: the attribute a buffer is kept under between calls, grown to the largest requirement seen (None: a
        fresh buffer per call)."""
        n, need = C.c_int64(), 0
        for Hq in sorted({H, ldh}):        # (a weight matrix on a padded leading dimension: every buffer is as large as that width's)
            _lib.check(query(self.ctx, *dims, Hq, *extra, int(path) if Hq == H else 2, C.byref(n)), name)
            need = max(need, n.value)
        ws = getattr(self, cache_attr, None) if cache_attr else None
        if ws is None or ws.numel() * 4 < need:
            ws = self._alloc_scratch(need, name)
            if cache_attr:
                setattr(self, cache_attr, ws)
        return ws

    def gibbs_clamped(self, v, obs, mask, W, hbias, vbias, gauss, n_steps, rng, burn_in=0, add_noise=False, path=0,
                      steps_per_launch=0, trace=False, sampler=False):
        """``n_steps`` of gibbs_vhv with the visibles where ``mask`` is 1 held at ``obs`` in ONE library call
        (mdbn_gibbs_clamped): returns device tensors ``(v_final, h_mean, h_sample, v_mean, v_avg, h_avg)`` -- the last
        step's values and the means of v_mean / h_mean over the steps ``burn_in .. n_steps - 1`` -- and, with ``trace``,
        also ``trace_h [n_steps, B, H]`` (hidden samples) and ``trace_v [n_steps, B, V]`` (the state after the clamp).
        ``mask``: [B, V], or [1, V] for the whole batch.  ``path``: 0 = by shape, 1 = the one-launch kernel (LDS-resident
        layers), 2 = the general path.  ``sampler`` (Gaussian visibles; nothing changes for Bernoulli ones): the Gibbs sampler of
        the model -- the hidden SAMPLE goes down and the visible draw always carries its N(0, 1) noise (the library's gauss = 2)
        -- instead of the reference's chain, which feeds the hidden mean down and whose averages are not posterior means.
        ``v`` is not modified; no host synchronisation.  Consumes 2 * n_steps RNG steps."""
        return self._gibbs_clamped(v, obs, mask, W, hbias, vbias, (2 if sampler else 1) if gauss else 0, n_steps, rng, burn_in,
                                   add_noise, path, steps_per_launch, trace)

    def gibbs_clamped_grouped(self, v, obs, mask, W, hbias, vbias, n_steps, rng, groups, burn_in=0, path=0, steps_per_launch=0,
                              trace=False):
        """``gibbs_clamped`` for a Bernoulli layer whose visibles hold the softmax groups ``groups`` (a ``GroupTable``), in ONE
        library call (mdbn_gibbs_clamped_grouped): a free group's visible draw is one category of its softmax, from one uniform
        at the group's first column, and its v_mean the softmax; a group is held or free as a whole, by the mask entry at its
        FIRST column.  Everything else, the returns and the 2 * n_steps RNG steps are ``gibbs_clamped``'s."""
        return self._gibbs_clamped(v, obs, mask, W, hbias, vbias, 0, n_steps, rng, burn_in, False, path, steps_per_launch, trace,
                                   groups=groups)

    def _gibbs_clamped(self, v, obs, mask, W, hbias, vbias, gauss, n_steps, rng, burn_in, add_noise, path, steps_per_launch, trace,
                       groups=None):
        """What ``gibbs_clamped`` (``gauss``: the library's 0 | 1 | 2) and ``gibbs_clamped_grouped`` (``groups``) share."""
        v = self.as_matrix(v)
        B, V = v.shape
        H = W.shape[1]
        ldh, ldv = W.stride(0), padded_ld(V)
        n_steps, burn_in = int(n_steps), int(burn_in)
        mask = self.as_matrix(mask)
        mask_rows = int(mask.shape[0])
        if mask_rows not in (1, B):
            raise ValueError("mask has %d rows: neither 1 nor the batch's %d" % (mask_rows, B))
        obs, mask = self._padded(obs, B, V, ldv), self._padded(mask, mask_rows, V, ldv)
        state = self.alloc_matrix(B, V, ldv)
        state.copy_(v)
        h_mean, h_sample, h_avg = (self.alloc_matrix(B, H, ldh) for _ in range(3))
        v_mean, v_avg = self.alloc_matrix(B, V, ldv), self.alloc_matrix(B, V, ldv)
        trace_h = torch.zeros((n_steps, B, ldh), dtype=torch.float32, device=self.device) if trace else None
        trace_v = torch.zeros((n_steps, B, ldv), dtype=torch.float32, device=self.device) if trace else None
        ws = self._sampler_workspace(self.lib.mdbn_gibbs_clamped_workspace_bytes, "mdbn_gibbs_clamped_workspace_bytes", (B, V), H, ldh,
                                     path, cache_attr="_clamp_ws")
        r = rng.c()
        name, kind, table = "mdbn_gibbs_clamped", (gauss, int(bool(add_noise))), ()
        if groups is not None:
            name, kind = "mdbn_gibbs_clamped_grouped", ()
            table = (self._p(groups.tensor), C.c_void_p(groups.host.ctypes.data), groups.n_groups)
        _lib.check(getattr(self.lib, name)(
            self.ctx, self._stream(), self._p(state), self._p(obs), self._p(mask), mask_rows, B, ldv, self._p(W), V, H, ldh,
            self._p(hbias), self._p(vbias), *kind, n_steps, burn_in, self._p(h_mean),
            self._p(h_sample), self._p(v_mean), self._p(v_avg), self._p(h_avg), self._p(trace_h), self._p(trace_v),
            int(path), int(steps_per_launch), C.byref(r), self._p(ws), ws.numel() * 4, *table), name)
        out = (state, h_mean, h_sample, v_mean, v_avg, h_avg)
        if trace:
            out += (trace_h[:, :, :H], trace_v[:, :, :V])
        return out

    def free_energy(self, x, W, hbias, vbias, gauss):
        x = self.as_matrix(x)
        N, V = x.shape
        H = W.shape[1]
        out = self.alloc_vector(N)
        if N == 0:
            return out
        ws = self.workspace(min(N, 4096), V, H)
        _lib.check(self.lib.mdbn_free_energy(
            self.ctx, self._stream(), self._p(x), N, x.stride(0), self._p(W), V, H, W.stride(0),
            self._p(hbias), self._p(vbias), int(bool(gauss)), self._p(out),
            self._p(ws), ws.numel() * 4), "mdbn_free_energy")
        return out

    def propdown_row_loglik(self, h, W, vbias, target, gauss, target_div=1):
        """``log p(target[r // target_div] | h[r])`` of every row of the 0 / 1 sample matrix ``h`` [R, H] under the layer's
        visible conditional (sigmoid(h W^T + vbias); N(h W^T + vbias, I) with ``gauss``) as a float32 device vector [R]
        (mdbn_propdown_rowll: the propdown GEMM reduced against the target in its epilogue, no [R, V] matrix is written).
        ``target``: [ceil(R / target_div), V].  ``h`` must hold 0 / 1 only."""
        return self._row_loglik(h, W, vbias, target, target_div, "mdbn_propdown_rowll", "mdbn_rowll_workspace_bytes", "_rowll_ws",
                                kind=(int(bool(gauss)),))

    def propdown_row_loglik_grouped(self, h, W, vbias, target, groups, target_div=1):
        """``propdown_row_loglik`` for a Bernoulli layer whose visible columns hold softmax groups (``groups``: its
        ``GroupTable``): every group adds the log-softmax of its pre-activations at the target's 1, every column outside the
        span the sigmoid term (mdbn_propdown_rowll_grouped: the same fused GEMM, no [R, V] matrix is written).  Every group of
        every row of ``target`` must hold exactly one 1 (not checked here)."""
        return self._row_loglik(h, W, vbias, target, target_div, "mdbn_propdown_rowll_grouped", "mdbn_rowll_grouped_workspace_bytes",
                                "_rowll_grouped_ws",
                                table=(self._p(groups.tensor), C.c_void_p(groups.host.ctypes.data), groups.n_groups))

    def _row_loglik(self, h, W, vbias, target, target_div, name, sizer, cache_attr, kind=(), table=()):
        """What ``propdown_row_loglik`` and ``propdown_row_loglik_grouped`` share: the shape checks, the cached workspace (one
        per call name) and the library call ``name`` (``kind``: its arguments before ``out``, ``table``: those after the
        workspace)."""
        h, target = self.as_matrix(h), self.as_matrix(target)
        R, H = (int(x) for x in h.shape)
        V = int(W.shape[0])
        target_div = int(target_div)
        if W.shape[1] != H or target.shape[1] != V:
            raise ValueError("h [%d, %d], W %r and target %r do not fit" % (R, H, tuple(W.shape), tuple(target.shape)))
        if target_div < 1 or target.shape[0] != (R + target_div - 1) // target_div:
            raise ValueError("target has %d rows; %d rows of h at target_div = %d need %d"
                             % (target.shape[0], R, target_div, (R + max(target_div, 1) - 1) // max(target_div, 1)))
        h = self._padded(h, R, H, W.stride(0))          # the C-ABI reads h with W's ld
        out = self.alloc_vector(R)
        if R == 0:
            return out
        n = C.c_int64()
        _lib.check(getattr(self.lib, sizer)(self.ctx, R, V, H, C.byref(n)), sizer)
        ws = getattr(self, cache_attr, None)
        if ws is None or ws.numel() * 4 < n.value:
            ws = self._alloc_scratch(n.value, sizer)
            setattr(self, cache_attr, ws)
        _lib.check(getattr(self.lib, name)(
            self.ctx, self._stream(), self._p(h), R, h.stride(0), self._p(W), V, H, self._p(vbias), self._p(target),
            target.stride(0), target_div, *kind, self._p(out), self._p(ws), ws.numel() * 4, *table), name)
        return out

    def sample_replicas(self, mean, n_samples, rng):
        """``n_samples`` Bernoulli samples of every row of ``mean`` [N, H] (mdbn_sample_replicas): ``(sample, entropy)``,
        device tensors -- ``sample`` [N n_samples, H] on the leading dimension of ``mean``, row n n_samples + s =
        (u[n n_samples + s] < mean[n]) with u the uniforms ``rng_uniform(N n_samples, H, rng)`` yields; ``entropy`` [N] the
        entropy of the factorial Bernoulli distribution of each row.  Consumes one RNG step."""
        mean = self.as_matrix(mean)
        N, H = (int(x) for x in mean.shape)
        S = int(n_samples)
        if S < 1:
            raise ValueError("n_samples must be >= 1, got %r" % (n_samples,))
        sample = self.alloc_matrix(N * S, H, mean.stride(0))
        entropy = self.alloc_vector(N)
        if N == 0:
            return sample, entropy
        r = rng.c()
        _lib.check(self.lib.mdbn_sample_replicas(self.ctx, self._stream(), self._p(mean), N, H, mean.stride(0), S,
                                                 self._p(sample), self._p(entropy), C.byref(r)), "mdbn_sample_replicas")
        return sample, entropy

    def _padded(self, x, rows, V, ldv):
        """``x`` as a [rows, V] device matrix on the leading dimension ``ldv`` (copied where it is on another)."""
        x = self.as_matrix(x)
        if tuple(x.shape) != (rows, V):
            raise ValueError("expected a [%d, %d] matrix, got %r" % (rows, V, tuple(x.shape)))
        if x.stride(0) != ldv:
            t = self.alloc_matrix(rows, V, ldv)
            t.copy_(x)
            x = t
        return x

    def _ais(self, W, hbias, vbias, base_vbias, gauss, betas, M, rng, path, trace, clamp=None, groups=None):
        """What ``ais``, ``ais_grouped``, ``ais_conditional`` and ``ais_conditional_grouped`` share: M chains through
        mdbn_ais_run, or with ``clamp`` = (obs, mask, mask_rows, N, chains per row), padded device matrices, through
        mdbn_ais_cond_run, or with ``groups`` (a ``GroupTable``) through mdbn_ais_run_grouped / mdbn_ais_cond_run_grouped (no
        ``gauss`` argument), whose workspaces are those of the calls without groups.  Returns ``(logw [M] float64 numpy, trace_h,
        trace_v, v_state)``: the traces numpy (None without ``trace``), the final visible state [M, V] a device tensor."""
        V, H = W.shape
        ldh, ldv = W.stride(0), padded_ld(V)
        betas = numpy.ascontiguousarray(betas, dtype=numpy.float32)
        if betas.ndim != 1 or betas.size < 2 or betas[0] != 0.0 or betas[-1] != 1.0 or not (numpy.diff(betas) > 0).all():
            raise ValueError("betas must rise strictly from 0 to 1")
        K = betas.size - 1
        d_betas = torch.from_numpy(betas).to(self.device)
        base = self.to_device(numpy.asarray(base_vbias, dtype=numpy.float32)) if not isinstance(base_vbias, torch.Tensor) \
            else base_vbias.to(device=self.device, dtype=torch.float32).contiguous()
        name = "mdbn_ais_run" if clamp is None else "mdbn_ais_cond_run"
        sizer = name.replace("run", "workspace_bytes")
        table, kind = (), (int(bool(gauss)),)
        if groups is not None:
            name = name + "_grouped"
            if clamp is not None:
                kind = ()
            table = (self._p(groups.tensor), C.c_void_p(groups.host.ctypes.data), groups.n_groups)
        ws = self._sampler_workspace(getattr(self.lib, sizer), sizer, ((M,) if clamp is None else clamp[3:]) + (V,), H, ldh, path,
                                     extra=(K + 1,))
        logw = torch.zeros(M, dtype=torch.float64, device=self.device)
        v_state = self.alloc_matrix(M, V, ldv)
        trace_h = torch.zeros((max(K - 1, 1), M, ldh), dtype=torch.float32, device=self.device) if trace else None
        trace_v = torch.zeros((K, M, ldv), dtype=torch.float32, device=self.device) if trace else None
        r = rng.c()
        chains = (M,) if clamp is None else (self._p(clamp[0]), self._p(clamp[1])) + tuple(clamp[2:])
        _lib.check(getattr(self.lib, name)(
            self.ctx, self._stream(), self._p(W), V, H, ldh, self._p(hbias), self._p(vbias), self._p(base), *kind,
            self._p(d_betas), K + 1, *chains, ldv, self._p(v_state), self._p(logw), self._p(trace_h), self._p(trace_v),
            int(path), C.byref(r), self._p(ws), ws.numel() * 4, *table), name)
        if trace:
            trace_h, trace_v = trace_h.cpu().numpy()[:K - 1, :, :H], trace_v.cpu().numpy()[:, :, :V]
        return logw.cpu().numpy(), trace_h, trace_v, v_state

    def ais(self, W, hbias, vbias, base_vbias, gauss, betas, n_chains, rng, path=0, trace=False):
        """Annealed importance sampling of the layer (W, hbias, vbias) from the base-rate model ``base_vbias`` through
        the inverse temperatures ``betas`` (0 = betas[0] < ... < betas[K] = 1) in ONE library call (mdbn_ais_run):
        the per-chain log importance weights as a float64 numpy vector (one device -> host copy) and, with ``trace``,
        the hidden [K-1, M, H] and visible [K, M, V] samples of every temperature.  ``path``: 0 = by shape, 1 = the
        one-launch kernel (LDS-resident layers), 2 = the general path.  Consumes 2K - 1 RNG steps from ``rng.step``."""
        logw, trace_h, trace_v, _ = self._ais(W, hbias, vbias, base_vbias, gauss, betas, int(n_chains), rng, path, trace)
        return (logw, trace_h, trace_v) if trace else logw

    def ais_grouped(self, W, hbias, vbias, base_vbias, betas, n_chains, rng, groups, path=0, trace=False):
        """``ais`` for a Bernoulli layer whose visibles hold the softmax groups ``groups`` (a ``GroupTable``), in ONE library
        call (mdbn_ais_run_grouped): a group's visible draw is one category of its softmax over the tempered pre-activations,
        from one uniform at the group's first column; everything else, the returns and the 2K - 1 RNG steps are ``ais``'s.
        The per-chain weights belong with the grouped base model (``ais_estimate(..., groups=)``)."""
        logw, trace_h, trace_v, _ = self._ais(W, hbias, vbias, base_vbias, False, betas, int(n_chains), rng, path, trace,
                                              groups=groups)
        return (logw, trace_h, trace_v) if trace else logw

    def ais_conditional(self, W, hbias, vbias, base_vbias, gauss, betas, obs, mask, n_chains, rng, path=0, trace=False, state=False):
        """Annealed importance sampling of the layer with the visibles where ``mask`` is 1 held at ``obs``, ``n_chains`` chains
        for each of the N rows of ``obs``, in ONE library call (mdbn_ais_cond_run): the log importance weights of the
        conditional partition functions as a float64 numpy array [N, n_chains] (one device -> host copy) and, with ``trace``,
        the hidden [K-1, N n_chains, H] and visible [K, N n_chains, V] samples of every temperature (chain m belongs to row
        m // n_chains) and, with ``state``, last of all the final visible state [N n_chains, V].  ``mask``: [N, V], or [1, V] for
        every row.  ``betas``, ``base_vbias`` and ``path`` as ``ais``.  Consumes 2K - 1 RNG steps from ``rng.step``."""
        return self._ais_conditional(W, hbias, vbias, base_vbias, gauss, betas, obs, mask, n_chains, rng, path, trace, state)

    def ais_conditional_grouped(self, W, hbias, vbias, base_vbias, betas, obs, mask, n_chains, rng, groups, path=0, trace=False,
                                state=False):
        """``ais_conditional`` for a Bernoulli layer whose visibles hold the softmax groups ``groups`` (a ``GroupTable``), in
        ONE library call (mdbn_ais_cond_run_grouped): a free group's visible draw is one category of its softmax over the
        tempered pre-activations, from one uniform at the group's first column; a group is held or free as a whole, by the mask
        entry at its FIRST column.  Everything else, the returns and the 2K - 1 RNG steps are ``ais_conditional``'s.  The
        weights belong with the grouped base model (``ais_estimate_rows(..., groups=)``)."""
        return self._ais_conditional(W, hbias, vbias, base_vbias, False, betas, obs, mask, n_chains, rng, path, trace, state,
                                     groups=groups)

    def _ais_conditional(self, W, hbias, vbias, base_vbias, gauss, betas, obs, mask, n_chains, rng, path, trace, state, groups=None):
        """What ``ais_conditional`` and ``ais_conditional_grouped`` (``groups``) share."""
        obs = self.as_matrix(obs)
        N, V = (int(x) for x in obs.shape)
        if V != W.shape[0]:
            raise ValueError("obs has %d columns, the layer %d visible units" % (V, W.shape[0]))
        Cn = int(n_chains)
        if N < 1 or Cn < 1:
            raise ValueError("need at least one row and one chain per row, got %d, %d" % (N, Cn))
        ldv = padded_ld(V)
        mask = self.as_matrix(mask)
        mask_rows = int(mask.shape[0])
        if mask_rows not in (1, N):
            raise ValueError("mask has %d rows: neither 1 nor the %d rows of obs" % (mask_rows, N))
        clamp = (self._padded(obs, N, V, ldv), self._padded(mask, mask_rows, V, ldv), mask_rows, N, Cn)
        logw, trace_h, trace_v, v_state = self._ais(W, hbias, vbias, base_vbias, gauss, betas, N * Cn, rng, path, trace, clamp, groups)
        out = (logw.reshape(N, Cn),)
        if trace:
            out += (trace_h, trace_v)
        if state:
            out += (v_state.cpu().numpy()[:, :V],)
        return out if len(out) > 1 else out[0]

    def temper(self, W, hbias, vbias, base_vbias, gauss, betas, v, h, rank, n_sweeps, rng, burn_in=0, sweep0=0, path=0,
               steps_per_launch=0, trace=False, zacc=None, trace_work=False):
        """``n_sweeps`` parallel-tempering sweeps of M ladders of R replicas in ONE library call (mdbn_pt_run).  ``v``
        [M R, V] (ld = padded_ld(V)), ``h`` [M R, H] (ld = W's) and ``rank`` [M, R] (int32) are the ladders' state and are
        updated IN PLACE; ``betas``: R float32 values on the host, rising strictly to exactly 1; ``base_vbias``: device vector.
        Returns device tensors ``(accepted [R - 1] int32, v_avg [M, V], h_avg [M, H])`` and, with ``trace``, also
        ``trace_v [n, M R, V]``, ``trace_h [n, M R, H]`` and ``trace_swaps [n, M, 2, R]`` (int32: the rank map after the swap;
        per lower rank 1 / 0 / -1 = accepted / refused / not attempted).  ``path``: 0 = by shape, 1 = the one-launch kernel,
        2 = the general path.  No host synchronisation.  Consumes 3 * n_sweeps RNG steps.
        ``zacc`` (a device float64 tensor [M, R - 1, 4], updated IN PLACE) and / or ``trace_work=True`` take the call through
        mdbn_pt_run_z: the works of the swap attempts accumulated as {m_f, s_f, m_r, s_r} per ladder and pair (start it at
        m = -inf, s = 0) and, appended to the returned tuple, ``trace_work [n, M, R - 1, 2]`` (float64: (d_fwd, d_rev), NaN
        where the pair was not tried).  Every other output is bit-identical with and without them."""
        return self._temper(W, hbias, vbias, base_vbias, gauss, betas, v, h, rank, n_sweeps, rng, burn_in, sweep0, path,
                            steps_per_launch, trace, zacc, trace_work)

    def temper_grouped(self, W, hbias, vbias, base_vbias, betas, v, h, rank, n_sweeps, rng, groups, burn_in=0, sweep0=0, path=0,
                       steps_per_launch=0, trace=False, zacc=None, trace_work=False):
        """``temper`` for a Bernoulli layer whose visibles hold the softmax groups ``groups`` (a ``GroupTable``), in ONE library
        call (mdbn_pt_run_grouped): a group's visible draw is one category of its softmax over the tempered pre-activations at
        the beta of the row's rank, from one uniform at the group's first column, and the beta = 1 visible mean in ``v_avg``
        is the group's softmax mean; the swaps, the works, the hidden draw, the returns and the 3 * n_sweeps RNG steps are
        ``temper``'s.  The works belong with the grouped base model (``base_log_partition(..., groups=)``)."""
        return self._temper(W, hbias, vbias, base_vbias, False, betas, v, h, rank, n_sweeps, rng, burn_in, sweep0, path,
                            steps_per_launch, trace, zacc, trace_work, groups=groups)

    def _temper(self, W, hbias, vbias, base_vbias, gauss, betas, v, h, rank, n_sweeps, rng, burn_in, sweep0, path,
                steps_per_launch, trace, zacc, trace_work, groups=None):
        """What ``temper`` and ``temper_grouped`` (``groups``: through mdbn_pt_run_grouped, on the workspace of
        mdbn_pt_run_z) share."""
        V, H = W.shape
        M, R = (int(x) for x in rank.shape)
        ldh, ldv = W.stride(0), padded_ld(V)
        n_sweeps, burn_in = int(n_sweeps), int(burn_in)
        betas = numpy.ascontiguousarray(betas, dtype=numpy.float32)
        if betas.shape != (R,):
            raise ValueError("expected %d betas, got %r" % (R, betas.shape))
        if tuple(v.shape) != (M * R, V) or v.stride(0) != ldv or tuple(h.shape) != (M * R, H) or h.stride(0) != ldh:
            raise ValueError("v / h must be [%d, %d] on ld %d and [%d, %d] on ld %d" % (M * R, V, ldv, M * R, H, ldh))
        if rank.dtype != torch.int32 or not rank.is_contiguous():
            raise ValueError("rank must be a contiguous int32 tensor")
        accepted = torch.zeros(max(R - 1, 1), dtype=torch.int32, device=self.device)
        v_avg, h_avg = self.alloc_matrix(M, V, ldv), self.alloc_matrix(M, H, ldh)
        n_t = max(n_sweeps, 1)
        trace_v = torch.zeros((n_t, M * R, ldv), dtype=torch.float32, device=self.device) if trace else None
        trace_h = torch.zeros((n_t, M * R, ldh), dtype=torch.float32, device=self.device) if trace else None
        trace_s = torch.zeros((n_t, M, 2, R), dtype=torch.int32, device=self.device) if trace else None
        works = zacc is not None or bool(trace_work)
        if zacc is not None and (zacc.dtype != torch.float64 or tuple(zacc.shape) != (M, R - 1, 4) or not zacc.is_contiguous()):
            raise ValueError("zacc must be a contiguous float64 tensor [%d, %d, 4]" % (M, R - 1))
        trace_w = torch.zeros((n_t, M, R - 1, 2), dtype=torch.float64, device=self.device) if trace_work else None
        sizer = "mdbn_pt_run_z_workspace_bytes" if works or groups is not None else "mdbn_pt_workspace_bytes"
        ws = self._sampler_workspace(getattr(self.lib, sizer), sizer, (M, R, V), H, ldh, path, cache_attr="_pt_ws")
        r = rng.c()
        args = (self.ctx, self._stream(), self._p(W), V, H, ldh, self._p(hbias), self._p(vbias), self._p(base_vbias),
                int(bool(gauss)), betas.ctypes.data_as(C.c_void_p), R, M, ldv, self._p(v), self._p(h), self._p(rank), n_sweeps,
                burn_in, int(sweep0), self._p(accepted), self._p(v_avg), self._p(h_avg), self._p(trace_v), self._p(trace_h),
                self._p(trace_s), int(path), int(steps_per_launch), C.byref(r), self._p(ws), ws.numel() * 4)
        if groups is not None:
            table = (self._p(groups.tensor), C.c_void_p(groups.host.ctypes.data), groups.n_groups)
            _lib.check(self.lib.mdbn_pt_run_grouped(*(args + (self._p(zacc), self._p(trace_w)) + table)), "mdbn_pt_run_grouped")
        elif works:
            _lib.check(self.lib.mdbn_pt_run_z(*(args + (self._p(zacc), self._p(trace_w)))), "mdbn_pt_run_z")
        else:
            _lib.check(self.lib.mdbn_pt_run(*args), "mdbn_pt_run")
        out = (accepted[:R - 1], v_avg, h_avg)
        if trace:
            out += (trace_v[:, :, :V], trace_h[:, :, :H], trace_s)
        if trace_work:
            out += (trace_w,)
        return out

    def gather_rows(self, src, indexes):
        src = self.as_matrix(src)
        idx = self.index_tensor(indexes, src.shape[0])
        out = self.alloc_matrix(idx.numel(), src.shape[1])
        if idx.numel() == 0:
            return out
        _lib.check(self.lib.mdbn_gather_rows(
            self.ctx, self._stream(), self._p(src), src.shape[0], src.shape[1], src.stride(0),
            self._p(idx), int(idx.dtype == torch.int64), idx.numel(), self._p(out), out.stride(0)),
            "mdbn_gather_rows")
        return out

    def gather_host_rows(self, host, cols, indexes, out=None):
        """``host[indexes]`` for a PINNED host matrix [n, ld] (shared.HostTable): the gather kernel reads the rows through
        their device-accessible host address, over PCIe, on the current stream.  ``out``: a device matrix to fill."""
        if not host.is_pinned():
            raise _lib.MdbnError("gather_host_rows needs pinned host memory (torch.Tensor.pin_memory)")
        idx = self.index_tensor(indexes, host.shape[0])
        if out is None:
            out = self.alloc_matrix(idx.numel(), cols, host.stride(0))
        assert out.shape[0] == idx.numel() and out.shape[1] == cols
        if idx.numel():
            _lib.check(self.lib.mdbn_gather_rows_host(
                self.ctx, self._stream(), C.c_void_p(host.data_ptr()), host.shape[0], cols, host.stride(0),
                self._p(idx), int(idx.dtype == torch.int64), idx.numel(), self._p(out), out.stride(0),
                int(self.host_gather_workgroups), int(self.host_gather_threads)), "mdbn_gather_rows_host")
        self._keep_alive = (host, idx)           # until the next call: the kernel reads them asynchronously
        return out

    def row_feeder(self, host, cols, max_rows, slots=3, threads=None):
        """A ``RowFeeder`` over the host matrix ``host`` [n, ld] (``mdbn_feeder_*``: CPU gather threads + one SDMA copy per
        minibatch on the feeder's own stream)."""
        return RowFeeder(self, host, cols, max_rows, slots, self.host_feed_threads if threads is None else threads)

    # ------------------------------------------------------------------ CD-k
    @staticmethod
    def _same_index_tensor(a, b):
        return (a is b) or (a is not None and b is not None and a.data_ptr() == b.data_ptr() and a.numel() == b.numel()
                            and a.dtype == b.dtype)

    def _ahead_valid(self, ahead, data, idx, W, thin):
        """Was THIS minibatch prepared by the previous step (CDScratch.ahead)?  Same matrix, unchanged since, same index
        list; thin-batch path, whose record also covers x W: the same parameters, written by nobody since that step
        (torch-side writes move W._version, library-side ones _w_serial) under the same options."""
        if ahead is None or ahead.data.data_ptr() != data.data_ptr() or ahead.data_version != data._version or \
                not self._same_index_tensor(ahead.indexes, idx) or ahead.index_version != idx._version:
            return False
        return not thin or ahead.params == (W.data_ptr(), W._version, self._w_serial, self._options_epoch)

    def _gathered_ahead(self, sc, announce, flag, W, thin):
        """The kernel's ``flag`` says it prepared the announced minibatch: the next call finds the rows (``sc.ahead``).  The flag
        is the caller's: every uncached call replaces the engine's ``_ahead_flag``, so cached structs carry one of their own."""
        if announce is not None and flag:
            params = AheadParams(W.data_ptr(), W._version, self._w_serial, self._options_epoch) if thin else None
            sc.ahead = announce._replace(params=params)

    def _cd_args(self, data, indexes, W, hbias, vbias, gauss, k, rng, persistent, add_noise, stats_slot,
                 sample_stats=False, stats=None, comm_cus=0, next_indexes=None, keep_f32=None):
        data = self.as_matrix(data)
        keep_f32 = self.keep_f32 if keep_f32 is None else bool(keep_f32)      # (of this call only: cd_step(keep_f32=))
        V, H = W.shape
        assert data.shape[1] == V, "data has %d columns, RBM has %d visibles" % (data.shape[1], V)
        idx = self.index_tensor(indexes, data.shape[0]) if indexes is not None else None
        B = idx.numel() if idx is not None else data.shape[0]
        ldv, ldh = data.stride(0), W.stride(0)
        sc = self.cd_scratch(B, V, H, not gauss, ldv, ldh)
        self.last_scratch = sc
        if stats is None:
            stats = self.stats_buffer(V, H, stats_slot, ldv, ldh)
        if persistent is not None and persistent.stride(0) != ldh:
            raise _lib.MdbnError("persistent chain must share W's leading dimension")
        ws = self.workspace(B, V, H, ldv, ldh)
        a = _lib.CdArgs()
        a.data, a.n_data = data.data_ptr(), data.shape[0]
        a.indexes = idx.data_ptr() if idx is not None else None
        a.index_is_64 = int(idx is not None and idx.dtype == torch.int64)
        a.gauss, a.add_noise, a.k = int(bool(gauss)), int(bool(add_noise)), int(k)
        a.sample_stats = int(bool(sample_stats))
        a.keep_f32 = int(bool(keep_f32))
        a.B, a.V, a.H = B, V, H
        a.ldv, a.ldh = ldv, ldh
        a.W, a.hbias, a.vbias = W.data_ptr(), hbias.data_ptr(), vbias.data_ptr()
        a.persistent = persistent.data_ptr() if persistent is not None else None
        a.V2, a.P2, a.hs = sc.V2.data_ptr(), sc.P2.data_ptr(), sc.hs.data_ptr()
        a.vs = sc.vs.data_ptr() if sc.vs is not None else None
        a.stats = stats.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        a.rng = rng.c()
        # W's planes travel with W whenever they exist (the update that follows rewrites them, and a step that finds them
        # stale re-splits them, whichever path it takes); the plane scratch only for shapes the library serves on planes
        wp, valid = self.w_planes(W, create=sc.planes is not None)
        if wp is not None:
            a.W_planes, a.W_planes_valid = wp.data_ptr(), int(valid)
        if sc.planes is not None:
            a.planes, a.planes_bytes = sc.planes.data_ptr(), sc.planes.numel() * 2
        a.comm_cus = int(comm_cus)
        # gather-ahead: was this minibatch gathered by the previous step's statistics kernel?  (same matrix, unchanged since,
        # same index list: the announced tensor has been kept alive, so an equal address means the same list)
        ahead, sc.ahead = sc.ahead, None
        keep, announce = [ws], None
        # ... on the plane path; on the thin-batch path (B <= 32, ldh <= 512: the library decides and reports) the previous
        # step's update kernel gathered the rows AND left the partials of x W, so the parameters must be the ones it wrote
        # (the step variants thin_eligible refuses never take part: nothing would honour the hand-over)
        thin = sc.planes is None and B <= 32 and ldh <= 512 and persistent is None and not sample_stats and \
            not (gauss and add_noise)
        if (sc.planes is not None or thin) and idx is not None and not keep_f32 and not self.trace_chain:
            # (the announcing step keeps the matrix and the index tensor alive, so an equal address is the same object)
            # ... and unchanged: an index buffer refilled IN PLACE between the announcing call and this one has another
            # version counter, and the rows are gathered afresh
            if self._ahead_valid(ahead, data, idx, W, thin):
                sc.x_buffer = ahead.buffer
                a.v0_ready = 1
            if sc.planes_alt is not None or next_indexes is not None:
                a.planes_alt = sc.alt_planes(self, ldv).data_ptr()
                a.x_buffer = sc.x_buffer
            if next_indexes is not None:
                nxt = self.index_tensor(next_indexes, data.shape[0])
                if nxt.numel() == B and nxt.dtype == idx.dtype:
                    a.next_indexes = nxt.data_ptr()
                    self._ahead_flag = C.c_int32(0)
                    a.ahead_done = C.pointer(self._ahead_flag)
                    keep.append(nxt)
                    announce = Ahead(data, data._version, nxt, 0 if thin else 1 - sc.x_buffer, nxt._version, None)
        if self.trace_chain:
            if sc.trace_h is None or sc.trace_h.shape[0] != k + 1:
                sc.trace_h = torch.zeros((k + 1, B, ldh), dtype=torch.float32, device=self.device)
                sc.trace_v = None if gauss else torch.zeros((k, B, ldv), dtype=torch.float32, device=self.device)
            a.trace_h = sc.trace_h.data_ptr()
            a.trace_v = sc.trace_v.data_ptr() if sc.trace_v is not None else None
        return CdCall(a, stats, sc, data, idx, keep, announce, thin)

    def cd_step(self, data, indexes, W, hbias, vbias, gauss, k, rng, persistent=None, add_noise=False,
                stats_slot=0, sample_stats=False, stats=None, comm_cus=0, keep_f32=None):
        """gather + positive phase + k Gibbs steps + statistics (rbm.py:303-345,374).
        Returns (stats, scratch): the packed [S | s_h | s_v | cost_sum] buffer and the
        CDScratch holding ph_mean / nv_mean / nh_mean for inspection.  ``comm_cus`` > 0 (data-parallel
        mode): CUs left to the collective that runs beside this step (mdbn_cd_args.comm_cus).  ``keep_f32``: the engine's
        attribute of that name for this one call (None: the attribute) -- a caller that reads v0 / ph_mean in the scratch
        (the centred step) asks for the float32 copies without changing what other steps of the engine do."""
        call = self._cd_args(data, indexes, W, hbias, vbias, gauss, k, rng, persistent,
                             add_noise, stats_slot, sample_stats, stats, comm_cus, keep_f32=keep_f32)
        _lib.check(self.lib.mdbn_cd_step(self.ctx, self._stream(), C.byref(call.args)), "mdbn_cd_step")
        if call.args.W_planes:
            self._w_planes_written(W)            # (split on entry if they were stale)
        return call.stats, call.scratch

    # ------------------------------------------------------------------ categorical visible units (mdbn_group_softmax_*)
    def group_softmax(self, pre, groups, rng, v0=None):
        """p(v | h) of a layer with softmax groups from the visible pre-activations ``pre`` [B, V] = h W^T + vbias
        (mdbn_group_softmax_sample): ``(mean, sample)`` -- softmax inside every group of ``groups`` (a ``GroupTable``), sigmoid
        on the other columns; one uniform of ``rng`` per group, at its first column, and one per Bernoulli column; ``rng``
        None: no sample (None).  With ``v0`` also the un-normalised cost sum (device scalar): the categorical cross-entropy
        of the groups from the log-sum-exp plus the Bernoulli cross-entropy of the other columns."""
        pre = self.as_matrix(pre)
        B, V = pre.shape
        ldv = pre.stride(0)
        mean = self.alloc_matrix(B, V, ldv)
        sample = self.alloc_matrix(B, V, ldv) if rng is not None else None
        cost = ws = None
        if v0 is not None:
            v0 = self.as_matrix(v0)
            if v0.stride(0) != ldv:                     # the target is read with the output's ld
                t = self.alloc_matrix(B, V, ldv)
                t.copy_(v0)
                v0 = t
            cost = torch.zeros(4, dtype=torch.float32, device=self.device)
        if B == 0:
            return (mean, sample) if v0 is None else (mean, sample, cost[0])
        if v0 is not None:
            n = C.c_int64()
            _lib.check(self.lib.mdbn_group_softmax_workspace_bytes(self.ctx, B, V, C.byref(n)), "mdbn_group_softmax_workspace_bytes")
            ws = getattr(self, "_group_ws", None)
            if ws is None or ws.numel() * 4 < n.value:
                ws = self._group_ws = self._alloc_scratch(n.value, "mdbn_group_softmax_workspace_bytes")
        r = rng.c() if rng is not None else None
        _lib.check(self.lib.mdbn_group_softmax_sample(
            self.ctx, self._stream(), self._p(pre), B, ldv, V, self._p(groups.tensor), C.c_void_p(groups.host.ctypes.data),
            groups.n_groups, self._p(mean), self._p(sample), None, C.byref(r) if r is not None else None, self._p(v0),
            self._p(cost), self._p(ws), ws.numel() * 4 if ws is not None else 0), "mdbn_group_softmax_sample")
        return (mean, sample) if v0 is None else (mean, sample, cost[0])

    def cd_step_grouped(self, data, indexes, W, hbias, vbias, k, rng, groups, persistent=None, stats_slot=0, stats=None,
                        keep_f32=None):
        """``cd_step`` for a Bernoulli layer whose visibles hold the softmax groups ``groups`` (mdbn_cd_step_grouped): the same
        ``(stats, scratch)``, the float32 copies in the scratch always written, the cost slot holding the cross-entropy of
        ``group_softmax`` for the last Gibbs step against v0."""
        call = self._cd_args(data, indexes, W, hbias, vbias, False, k, rng, persistent, False, stats_slot, False, stats,
                             keep_f32=True)
        a = call.args
        a.W_planes, a.W_planes_valid, a.planes, a.planes_bytes = None, 0, None, 0      # (the composed step reads f32 operands only)
        a.planes_alt, a.next_indexes, a.v0_ready, a.ahead_done = None, None, 0, None
        _lib.check(self.lib.mdbn_cd_step_grouped(self.ctx, self._stream(), C.byref(a), self._p(groups.tensor),
                                                 C.c_void_p(groups.host.ctypes.data), groups.n_groups), "mdbn_cd_step_grouped")
        return call.stats, call.scratch

    # ------------------------------------------------------------------ absent visible units (mdbn_absent_*)
    def _sized_scratch(self, attr, need):
        """The engine's scratch buffer ``attr``, regrown to hold ``need`` bytes."""
        ws = getattr(self, attr, None)
        if ws is None or ws.numel() * 4 < need:
            ws = self._alloc_scratch(need, attr)
            setattr(self, attr, ws)
        return ws

    def absent_split(self, x, out=None, want_count=True):
        """A table with missing entries (NaN: "this row did not observe this unit") -> ``(filled, observed, row_count)``
        (mdbn_absent_split): the rows with 0 where missing (``out``: a matrix of x's shape to receive them, may be ``x``
        itself), the observed bits as int32 words [B, (V + 31) // 32] (bit i & 31 of word i >> 5) and the number of
        observed entries of every row (int32 [B]; None without ``want_count``)."""
        x = self.as_matrix(x)
        B, V = x.shape
        filled = self.alloc_matrix(B, V, x.stride(0)) if out is None else out
        observed = torch.zeros((B, (V + 31) // 32), dtype=torch.int32, device=self.device)
        count = torch.zeros(B, dtype=torch.int32, device=self.device) if want_count else None
        if B:
            _lib.check(self.lib.mdbn_absent_split(self.ctx, self._stream(), self._p(x), B, x.stride(0), V, self._p(filled),
                                                  filled.stride(0), self._p(observed), self._p(count)), "mdbn_absent_split")
        return filled, observed, count

    def absent_visible(self, pre, observed, gauss=False, add_noise=False, rng=None, v0=None, out=None):
        """p(v | h) of rows with absent units from the linear pre-activations ``pre`` [B, V] = h W^T + vbias
        (mdbn_absent_visible): ``(mean, sample)``, both exactly 0 where ``observed`` (the words of ``absent_split``) has no
        bit; ``rng`` None: no sample.  ``out``: the matrix that receives the means (may be ``pre``).  With ``v0`` (zero-filled)
        also the un-normalised cost sum over the observed entries (device scalar)."""
        pre = self.as_matrix(pre)
        B, V = pre.shape
        ldv = pre.stride(0)
        mean = self.alloc_matrix(B, V, ldv) if out is None else out
        sample = self.alloc_matrix(B, V, ldv) if rng is not None else None
        cost = ws = None
        n = C.c_int64(0)
        if v0 is not None:
            v0 = self.as_matrix(v0)
            if v0.stride(0) != ldv:                     # the target is read with the output's ld
                t = self.alloc_matrix(B, V, ldv)
                t.copy_(v0)
                v0 = t
            cost = torch.zeros(4, dtype=torch.float32, device=self.device)
            _lib.check(self.lib.mdbn_absent_visible_workspace_bytes(self.ctx, B, V, C.byref(n)), "mdbn_absent_visible_workspace_bytes")
            ws = self._sized_scratch("_absent_ws", n.value)
        r = rng.c() if rng is not None else None
        _lib.check(self.lib.mdbn_absent_visible(
            self.ctx, self._stream(), self._p(pre), B, ldv, V, self._p(observed), int(bool(gauss)), int(bool(add_noise)),
            self._p(mean), self._p(sample), None, C.byref(r) if r is not None else None, self._p(v0), self._p(cost), self._p(ws),
            n.value), "mdbn_absent_visible")           # (the sizers of these calls are exact: the library is told their figure)
        return (mean, sample) if v0 is None else (mean, sample, cost[0])

    def cd_step_absent(self, data, indexes, W, hbias, vbias, gauss, k, rng, add_noise=False, stats_slot=0, stats=None):
        """``cd_step`` on rows with missing entries (mdbn_cd_step_absent; NaN in ``data``: the unit is absent from that row's
        RBM): the same ``(stats, scratch)``, the float32 copies in the scratch always written -- V2 = [v0; nv] zero at the
        absent entries, ``vs`` the masked visible sample for Gaussian layers too --, the cost slot holding the monitoring cost
        summed over the observed entries only."""
        call = self._cd_args(data, indexes, W, hbias, vbias, gauss, k, rng, None, add_noise, stats_slot, False, stats, keep_f32=True)
        a, sc = call.args, call.scratch
        a.W_planes, a.W_planes_valid, a.planes, a.planes_bytes = None, 0, None, 0      # (the composed step reads f32 operands only)
        a.planes_alt, a.next_indexes, a.v0_ready, a.ahead_done = None, None, 0, None
        B, V, H, ldv, ldh = a.B, a.V, a.H, a.ldv, a.ldh
        if sc.vs is None:                               # (a Gaussian layer's scratch: the absent step writes the sample)
            sc.vs = self.alloc_matrix(B, V, ldv)
        a.vs = sc.vs.data_ptr()
        if self.trace_chain and sc.trace_v is None:
            sc.trace_v = torch.zeros((int(k), B, ldv), dtype=torch.float32, device=self.device)
            a.trace_v = sc.trace_v.data_ptr()
        n = C.c_int64()
        _lib.check(self.lib.mdbn_cd_step_absent_workspace_bytes(self.ctx, B, V, H, ldv, ldh, C.byref(n)),
                   "mdbn_cd_step_absent_workspace_bytes")
        ws = self._sized_scratch("_absent_step_ws", n.value)
        a.workspace, a.workspace_bytes = ws.data_ptr(), n.value
        _lib.check(self.lib.mdbn_cd_step_absent(self.ctx, self._stream(), C.byref(a)), "mdbn_cd_step_absent")
        return call.stats, sc

    def absent_mark_rows(self, y, row_count):
        """Rows of ``y`` whose ``row_count`` (int32 [N], of ``absent_split``) is 0 become rows of NaN, in place."""
        N, cols = y.shape
        if N:
            _lib.check(self.lib.mdbn_absent_mark_rows(self.ctx, self._stream(), self._p(y), N, y.stride(0), cols, self._p(row_count)),
                       "mdbn_absent_mark_rows")
        return y

    def free_energy_absent(self, x, W, hbias, vbias, gauss):
        """``free_energy`` over the observed units of every row (NaN in ``x``: absent; mdbn_free_energy_absent)."""
        x = self.as_matrix(x)
        N, V = x.shape
        H = W.shape[1]
        out = self.alloc_vector(N)
        if N == 0:
            return out
        n = C.c_int64()
        _lib.check(self.lib.mdbn_free_energy_absent_workspace_bytes(self.ctx, N, V, H, x.stride(0), C.byref(n)),
                   "mdbn_free_energy_absent_workspace_bytes")
        ws = self._sized_scratch("_absent_fe_ws", n.value)
        _lib.check(self.lib.mdbn_free_energy_absent(
            self.ctx, self._stream(), self._p(x), N, x.stride(0), self._p(W), V, H, W.stride(0), self._p(hbias), self._p(vbias),
            int(bool(gauss)), self._p(out), self._p(ws), n.value), "mdbn_free_energy_absent")
        return out

    # ------------------------------------------------------------------ classification RBM (mdbn_class_*)
    def _class_workspace(self, B, V, H, ldv, ldh, K, mode):
        key = (B, V, H, ldv, ldh, K, mode)
        cache = self.__dict__.setdefault("_class_need", {})
        need = cache.get(key)
        if need is None:
            n = C.c_int64()
            _lib.check(self.lib.mdbn_class_workspace_bytes(self.ctx, B, V, H, ldv, ldh, K, mode, C.byref(n)), "mdbn_class_workspace_bytes")
            need = cache[key] = n.value
        ws = getattr(self, "_class_ws", None)
        if ws is None or ws.numel() * 4 < need:
            ws = self._class_ws = self._alloc_scratch(need, "mdbn_class_workspace_bytes")
        return ws

    def class_posterior(self, v, W, hbias, vbias, lo, K, want_logp=False):
        """Exact p(label | everything else) of the one-hot label block in columns ``lo .. lo + K - 1`` for every row of ``v``
        (mdbn_class_posterior: one propup of the rows with the block set to zero and one class kernel): ``(post, logp)`` --
        float32 device tensors [B, K] and, with ``want_logp``, [B] = log p(y* | x) for the category the block holds (else None)."""
        v = self.as_matrix(v)
        B, V = v.shape
        H, ldv, ldh = W.shape[1], v.stride(0), W.stride(0)
        post = torch.zeros((B, K), dtype=torch.float32, device=self.device)
        logp = torch.zeros(B, dtype=torch.float32, device=self.device) if want_logp else None
        if B == 0:
            return post, logp
        ws = self._class_workspace(B, V, H, ldv, ldh, K, 0)
        _lib.check(self.lib.mdbn_class_posterior(self.ctx, self._stream(), self._p(v), B, ldv, self._p(W), V, H, ldh, self._p(hbias),
                                                 self._p(vbias), int(lo), int(K), self._p(post), int(K), self._p(logp), self._p(ws),
                                                 ws.numel() * 4), "mdbn_class_posterior")
        return post, logp

    def class_stats(self, scratch, v0, B, W, hbias, vbias, lo, K, gen_weight, disc_weight, stats):
        """``gen_weight`` x (the CD statistics of the finished ``cd_step_grouped`` that filled ``scratch``: V2 = [v0; nv],
        P2 = [ph; -nh]) + ``disc_weight`` x (the exact gradient of sum_rows log p(y* | x) for the label block
        ``lo .. lo + K - 1``) into the packed ``stats`` that step left (mdbn_class_stats).  ``gen_weight`` = 0: no step ran,
        ``scratch`` is None, ``v0`` holds the gathered rows, and the cost slot of ``stats`` receives -sum log p.  Returns
        -sum_rows log p(y* | x) as a 0-d device tensor."""
        V2, P2 = (scratch.V2, scratch.P2) if scratch is not None else (self.as_matrix(v0), None)
        V, H = W.shape
        ldv, ldh = V2.stride(0), W.stride(0)
        nll = torch.zeros(1, dtype=torch.float32, device=self.device)
        ws = self._class_workspace(int(B), V, H, ldv, ldh, int(K), 2 if gen_weight > 0.0 else 1)
        _lib.check(self.lib.mdbn_class_stats(self.ctx, self._stream(), self._p(V2), self._p(P2), int(B), self._p(W), V, H, ldv, ldh,
                                             self._p(hbias), self._p(vbias), int(lo), int(K), float(gen_weight), float(disc_weight),
                                             self._p(stats), self._p(nll), self._p(ws), ws.numel() * 4), "mdbn_class_stats")
        return nll[0]

    def center_hidden_rows(self, scratch, B, stats, V, H, ldv, ldh, mu, lam, row_scale, sparsity=None):
        """The centred hidden-bias statistic s_h' = s_h - row_scale S'^T mu from the ROWS of the step's scratch
        (mdbn_center_hidden_rows) instead of from S: [H] device vector.  Call it between ``center_offsets`` and ``center_stats``
        (it reads the raw s_h and s_v of ``stats``) and hand the result to ``center_stats_store_hidden`` afterwards.  On
        one-hot rows the route through S multiplies the float32 error of S by sum(mu).  ``sparsity``: the arguments
        ``(q, v_mean, target, w_scale, b_scale)`` of the ``sparsity_stats`` call that transformed ``stats`` before, or None --
        the rows do not know what that call added to S and s_h, so its share of S'^T mu is added here."""
        V2, P2 = scratch.V2, scratch.P2
        q, v_mean, target, w_scale, b_scale = sparsity if sparsity is not None else (None, None, 0.0, 0.0, 0.0)
        out = self.alloc_vector(H)
        ws = getattr(self, "_center_rows_ws", None)
        if ws is None or ws.numel() < 2 * B + 3:
            ws = self._center_rows_ws = self._alloc_scratch(4 * (2 * int(B) + 3), "mdbn_center_hidden_rows")
        _lib.check(self.lib.mdbn_center_hidden_rows(self.ctx, self._stream(), self._p(V2), V2.stride(0), self._p(P2), P2.stride(0),
                                                    int(B), int(V), int(H), self._p(stats), self._p(mu), self._p(lam),
                                                    float(row_scale), self._p(q), self._p(v_mean), float(target), float(w_scale),
                                                    float(b_scale), self._p(out), self._p(ws), ws.numel() * 4),
                   "mdbn_center_hidden_rows")
        return out

    @staticmethod
    def center_stats_store_hidden(stats, V, H, ldh, s_h):
        """Store ``center_hidden_rows``'s result over the s_h block of the packed statistics (after ``center_stats``)."""
        stats[V * ldh:V * ldh + H].copy_(s_h)

    def cd_forward(self, data, indexes, W, hbias, vbias, gauss, k, rng, add_noise=False, sample_stats=False, stats=None,
                   comm_cus=0, next_indexes=None):
        """The first half of ``cd_step`` (mdbn_cd_forward): gather, positive phase and the Gibbs chain -- everything that
        reads the parameters.  Returns the token ``cd_statistics`` completes the step with."""
        call = self._cd_args(data, indexes, W, hbias, vbias, gauss, k, rng, None, add_noise, 0,
                             sample_stats, stats, comm_cus, next_indexes=next_indexes)
        a = call.args
        _lib.check(self.lib.mdbn_cd_forward(self.ctx, self._stream(), C.byref(a)), "mdbn_cd_forward")
        if a.W_planes:
            self._w_planes_written(W)
            a.W_planes_valid = 1
        return (call, W)

    def cd_statistics(self, token, deferred=None):
        """The second half (mdbn_cd_statistics): bias statistics + statistics GEMM of the step ``cd_forward`` began.
        ``deferred``: the arguments of ``apply_update(..., phase=3)`` for the PREVIOUS step (whose all-reduced statistics
        the current stream has just been made to wait for) -- the library applies that update inside the statistics GEMM
        when it can, as its own launch otherwise; returns (stats, scratch, cost of the deferred update or None)."""
        call, W = token
        a = call.args
        u, cost = (None, None)
        if deferred is not None:
            u, cost = self._update_args(*deferred)
        _lib.check(self.lib.mdbn_cd_statistics(self.ctx, self._stream(), C.byref(a), C.byref(u) if u is not None else None),
                   "mdbn_cd_statistics")
        if u is not None:
            self._w_planes_written(W)
            self._w_serial += 1
        self._gathered_ahead(call.scratch, call.announce, a.ahead_done and self._ahead_flag.value, W, call.thin)
        return call.stats, call.scratch, cost

    def _update_args(self, W, W_speed, W0, hbias, hbias_speed, vbias, vbias_speed, stats, lr, lambda_1,
                     lambda_2, weightcost, momentum, batch_size, n_rows, cost_scale, phase, ldv):
        V, H = W.shape
        cost = self._next_cost_slot()
        u = _lib.UpdateArgs()
        u.W, u.W_speed = W.data_ptr(), W_speed.data_ptr()
        u.W0 = W0.data_ptr() if W0 is not None else None
        u.hbias, u.hbias_speed = hbias.data_ptr(), hbias_speed.data_ptr()
        u.vbias, u.vbias_speed = vbias.data_ptr(), vbias_speed.data_ptr()
        u.V, u.H, u.ldv, u.ldh = V, H, (padded_ld(V) if ldv is None else ldv), W.stride(0)
        u.stats = stats.data_ptr()
        u.lr, u.lambda_1, u.lambda_2 = float(lr), float(lambda_1), float(lambda_2)
        u.weightcost, u.momentum = float(weightcost), float(momentum)
        u.batch_size, u.n_rows, u.cost_scale = float(batch_size), float(n_rows), float(cost_scale)
        u.cost_out = cost.data_ptr()
        u.phase = int(phase)
        wp, _ = self.w_planes(W)
        u.W_planes = wp.data_ptr() if wp is not None else None    # kept in step with W by every update that writes W
        return u, cost

    def _next_cost_slot(self):
        # Step costs are 0-d views into a block of 1024 floats.  A block is never reused: when it is full a fresh one is
        # allocated (4 KB per 1024 steps) and the old one lives as long as a caller still holds one of its views, so a
        # cost kept unread for any number of steps can never show another step's value.
        if self._cost_slot >= self._cost_ring.numel():
            self._cost_ring = torch.zeros(1024, dtype=torch.float32, device=self.device)
            self._cost_slot = 0
        slot = self._cost_slot
        self._cost_slot = slot + 1
        return self._cost_ring[slot]

    def _step_cache_key(self, data, idx, params, batch_size, n_rows):
        """What cached argument structs (StepCache) were built from that a later call may find changed; the one statement of
        it, for filling the cache and for checking it.  ``params``: (W, W_speed, W0, hbias, hbias_speed, vbias, vbias_speed)."""
        W, W_speed, W0, hbias, _, vbias, _ = params
        return (data.data_ptr(), data.shape[0], data.stride(0), idx.dtype, idx.numel(), batch_size, n_rows,
                self._workspace.data_ptr() if self._workspace is not None else 0, self.keep_f32, self.trace_chain,
                self._options_epoch, torch._C._cuda_getCurrentRawStream(self.device.index), W.data_ptr(), W_speed.data_ptr(),
                W0.data_ptr() if W0 is not None else 0, hbias.data_ptr(), vbias.data_ptr())

    def cd_train_step_cached(self, cache, data, idx, params, batch_size, n_rows, rng_step, lr, momentum, next_indexes=None):
        """The step of ``cd_train_step`` through argument structs a step function keeps from its previous call
        (``cache`` = the list ``cd_train_step(..., cache_out=)`` filled): for small layers, whose step is two short launches,
        the host side -- building two ctypes structs of ~70 fields, resolving scratch, statistics and workspace buffers --
        was 32 us per call, more than the GPU's time.  Only what changes from call to call is set: the index list, the Philox
        step, lr / momentum and the cost slot.  Returns None when the cache does not apply (the caller takes the full path)."""
        (c,) = cache
        a, u, sc, W = c.args, c.update, c.scratch, c.W
        # the structs were captured for a W WITHOUT bf16 planes: if another consumer of the same W has created some since
        # (another batch size of the same RBM, planes_min_work = 0), these steps must not go on updating W behind them
        if getattr(W, "_mdbn_planes", None) is not None:
            return None
        if c.key != self._step_cache_key(data, idx, params, batch_size, n_rows):
            return None
        a.indexes = idx.data_ptr()
        a.rng.step = rng_step & 0xFFFFFFFF
        u.lr, u.momentum = float(lr), float(momentum)
        cost = self._next_cost_slot()
        u.cost_out = cost.data_ptr()
        self.last_scratch = sc
        # thin-batch path: positive phase prepared by the previous step / prepare the next one's (see _cd_args)
        ahead, sc.ahead = sc.ahead, None
        announce = None
        if a.planes_alt:
            a.v0_ready = int(self._ahead_valid(ahead, data, idx, W, True))
            a.next_indexes = None
            if next_indexes is not None:
                nxt = self.index_tensor(next_indexes, data.shape[0])
                if nxt.numel() == idx.numel() and nxt.dtype == idx.dtype:
                    a.next_indexes = nxt.data_ptr()
                    announce = Ahead(data, data._version, nxt, 0, nxt._version, None)
        _lib.check(self.lib.mdbn_cd_train_step(self.ctx, self._stream(), c.args_ref, c.update_ref), "mdbn_cd_train_step")
        self._w_serial += 1
        if announce is not None:
            self._gathered_ahead(sc, announce, a.ahead_done and a.ahead_done[0], W, True)
        return cost

    def cd_train_step(self, data, indexes, W, W_speed, W0, hbias, hbias_speed, vbias, vbias_speed, gauss, k,
                      rng, lr, lambda_1, lambda_2, weightcost, momentum, batch_size, n_rows, cost_scale,
                      sample_stats=False, next_indexes=None, cache_out=None):
        """The whole single-device step function (mdbn_cd_train_step): cd_step + update, with the
        finalize / parameter half of the update overlapped under the statistics GEMM.  Returns the
        monitoring cost (0-d device tensor).  ``cache_out``: a list that receives the argument structs of this call when
        the next call of the same step function may reuse them (``cd_train_step_cached``): index list given, no plane
        buffers (the plane path's arguments change from step to step: gather-ahead), no chain taps."""
        call = self._cd_args(data, indexes, W, hbias, vbias, gauss, k, rng, None, False, 0,
                             sample_stats, next_indexes=next_indexes)
        a, stats, sc = call.args, call.stats, call.scratch
        u, cost = self._update_args(W, W_speed, W0, hbias, hbias_speed, vbias, vbias_speed, stats, lr,
                                    lambda_1, lambda_2, weightcost, momentum, batch_size, n_rows, cost_scale,
                                    0, a.ldv)
        _lib.check(self.lib.mdbn_cd_train_step(self.ctx, self._stream(), C.byref(a), C.byref(u)),
                   "mdbn_cd_train_step")
        self._w_planes_written(W)
        self._w_serial += 1
        self._gathered_ahead(sc, call.announce, a.ahead_done and self._ahead_flag.value, W, call.thin)
        if cache_out is not None:
            del cache_out[:]
            dm, idx = call.data, call.indexes
            if idx is not None and sc.planes is None and not a.W_planes and not self.trace_chain and not sample_stats:
                if a.B <= 32 and a.ldh <= 512 and not self.keep_f32:
                    # thin-batch candidates: the cached calls hand the next minibatch to the update kernel (their own flag)
                    flag = C.c_int32(0)
                    a.planes_alt, a.x_buffer, a.ahead_done = sc.alt_planes(self, a.ldv).data_ptr(), 0, C.pointer(flag)
                params = (W, W_speed, W0, hbias, hbias_speed, vbias, vbias_speed)
                cache_out.append(StepCache(a, u, C.byref(a), C.byref(u), self._step_cache_key(dm, idx, params, batch_size, n_rows),
                                           sc, W, (dm, stats) + params))
        return cost

    def apply_update(self, W, W_speed, W0, hbias, hbias_speed, vbias, vbias_speed, stats,
                     lr, lambda_1, lambda_2, weightcost, momentum, batch_size, n_rows, cost_scale, phase=0,
                     ldv=None):
        """rbm.py:347-365; returns the monitoring cost as a 0-d device tensor.
        phase: 0 = whole rule, 1 = speeds (+cost) only, 2 = parameters only (mdbn_update_args)."""
        u, cost = self._update_args(W, W_speed, W0, hbias, hbias_speed, vbias, vbias_speed, stats, lr,
                                    lambda_1, lambda_2, weightcost, momentum, batch_size, n_rows, cost_scale,
                                    phase, ldv)
        _lib.check(self.lib.mdbn_apply_update(self.ctx, self._stream(), C.byref(u)), "mdbn_apply_update")
        self._w_serial += 1
        if phase != 1:
            self._w_planes_written(W)
        return cost

    # ------------------------------------------------------------------ centred gradient (mdbn_center_*)
    def center_offsets(self, scratch, B, mu, lam, nu):
        """Slide the offsets ``mu`` [V] / ``lam`` [H] (device vectors, updated IN PLACE) towards the column means of v0 and
        ph_mean of the step that filled ``scratch`` (rows 0..B-1 of its V2 / P2: a ``cd_step(keep_f32=True)``) by ``nu`` in
        (0, 1]; 1 sets them to those means (mdbn_center_offsets)."""
        V2, P2 = scratch.V2, scratch.P2
        _lib.check(self.lib.mdbn_center_offsets(self.ctx, self._stream(), self._p(V2), V2.stride(0), self._p(P2), P2.stride(0),
                                                int(B), V2.shape[1], P2.shape[1], float(nu), self._p(mu), self._p(lam)),
                   "mdbn_center_offsets")

    def center_stats(self, stats, V, H, ldv, ldh, mu, lam, row_scale):
        """The offset correction of the packed statistics, IN PLACE (mdbn_center_stats): S' = S - mu s_h' - s_v lam',
        s_v' = s_v - row_scale S' lam, s_h' = s_h - row_scale S'^T mu; ``row_scale`` = n_rows / batch_size."""
        n = C.c_int64()
        _lib.check(self.lib.mdbn_center_workspace_bytes(self.ctx, int(V), int(H), C.byref(n)), "mdbn_center_workspace_bytes")
        ws = getattr(self, "_center_ws", None)
        if ws is None or ws.numel() * 4 < n.value:
            ws = self._center_ws = self._alloc_scratch(n.value, "mdbn_center_workspace_bytes")
        _lib.check(self.lib.mdbn_center_stats(self.ctx, self._stream(), self._p(stats), int(V), int(H), int(ldv), int(ldh),
                                              self._p(mu), self._p(lam), float(row_scale), self._p(ws), ws.numel() * 4),
                   "mdbn_center_stats")
        return stats

    # ------------------------------------------------------------------ sparsity target (mdbn_sparsity_*)
    def sparsity_activity(self, scratch, B, q, v_mean, rate):
        """Slide the activity estimate ``q`` [H] (device vector, updated IN PLACE) towards the column means of ph_mean of the
        step that filled ``scratch`` (rows 0..B-1 of its P2: a ``cd_step(keep_f32=True)``) by ``rate`` in (0, 1]; 1 sets it
        to those means.  ``v_mean`` [V]: receives the column means of v0 (rows 0..B-1 of V2); None: the hidden half alone,
        ``scratch.V2`` is not looked at (mdbn_sparsity_activity)."""
        P2 = scratch.P2
        V2 = scratch.V2 if v_mean is not None else None
        _lib.check(self.lib.mdbn_sparsity_activity(self.ctx, self._stream(), self._p(P2), P2.stride(0), self._p(V2),
                                                   V2.stride(0) if V2 is not None else 0, int(B),
                                                   V2.shape[1] if V2 is not None else 0, P2.shape[1], float(rate),
                                                   self._p(q), self._p(v_mean)), "mdbn_sparsity_activity")

    def sparsity_stats(self, stats, V, H, ldv, ldh, q, v_mean, target, w_scale, b_scale):
        """The sparsity penalty's additions to the packed statistics, IN PLACE (mdbn_sparsity_stats): with t = target - q,
        S += w_scale v_mean t', s_h += b_scale t; ``w_scale`` = cost * batch_size (0: S is not touched, ``v_mean`` may be
        None), ``b_scale`` = cost * n_rows."""
        _lib.check(self.lib.mdbn_sparsity_stats(self.ctx, self._stream(), self._p(stats), int(V), int(H), int(ldv), int(ldh),
                                                self._p(q), self._p(v_mean), float(target), float(w_scale), float(b_scale)),
                   "mdbn_sparsity_stats")
        return stats

    # ------------------------------------------------------------------ learned per-column variance (mdbn_sigma_*)
    def sigma_scale_rows(self, src, indexes, log_sigma, sign, out=None):
        """``src[indexes] * exp(sign * log_sigma)`` (mdbn_sigma_scale_rows): ``sign`` = -1 takes raw rows to units -- the
        gather of a training step of a layer with a learned variance --, +1 takes units back to raw.  ``indexes``: None (the
        rows of ``src`` as they are) or an index list / tensor.  ``out``: the [B, V] matrix to fill (its pad columns are
        written as zeros); None: a new one on ``src``'s leading dimension."""
        src = self.as_matrix(src)
        idx = None if indexes is None else self.index_tensor(indexes, src.shape[0])
        B, V = (src.shape[0] if idx is None else idx.numel()), src.shape[1]
        if out is None:
            out = self.alloc_matrix(B, V, src.stride(0))
        assert tuple(out.shape) == (B, V) and log_sigma.numel() == V, "sigma_scale_rows: shapes"
        if B == 0:
            return out
        _lib.check(self.lib.mdbn_sigma_scale_rows(
            self.ctx, self._stream(), self._p(src), src.shape[0], src.stride(0), self._p(idx),
            int(idx is not None and idx.dtype == torch.int64), B, V, self._p(log_sigma), float(sign), self._p(out), out.stride(0)),
            "mdbn_sigma_scale_rows")
        return out

    def sigma_update(self, U, M, n_rows, lr, momentum, lo, hi, log_sigma, log_sigma_speed):
        """The step of ``log_sigma`` [V] and its speed, IN PLACE (mdbn_sigma_update): g = mean over the first ``n_rows`` rows
        of U (U - M), minus 1 -- ``U`` the rows in units (rows of a ``cd_step(keep_f32=True)``'s V2), ``M`` their conditional
        means vbias + ph_mean W^T --, then the visible bias's rule with rate ``lr`` and the clamp [lo, hi]."""
        B, V = U.shape
        n = C.c_int64()
        _lib.check(self.lib.mdbn_sigma_workspace_bytes(self.ctx, int(B), int(V), C.byref(n)), "mdbn_sigma_workspace_bytes")
        ws = getattr(self, "_sigma_ws", None)
        if n.value and (ws is None or ws.numel() * 4 < n.value):
            ws = self._sigma_ws = self._alloc_scratch(n.value, "mdbn_sigma_workspace_bytes")
        _lib.check(self.lib.mdbn_sigma_update(
            self.ctx, self._stream(), self._p(U), U.stride(0), self._p(M), M.stride(0), int(B), int(V), int(n_rows), float(lr),
            float(momentum), float(lo), float(hi), self._p(log_sigma), self._p(log_sigma_speed),
            self._p(ws) if n.value else None, ws.numel() * 4 if n.value else 0), "mdbn_sigma_update")

    # ------------------------------------------------------------------ up-down fine-tuning (mdbn_updown_*)
    UPDOWN_PATHS = {"auto": 0, "fused": 1, "composed": 2}

    def _updown_call(self, kind, n, W, W_speed, bias, bias_speed, ldv, rule, cost_scale, path):
        """What the two delta-rule calls share: the update struct with the half that must not move left NULL, the workspace
        the library asks for under ``path``, the planes of the matrix written.  Returns ``(u, workspace, path number)``."""
        lr, lambda_1, lambda_2, weightcost, momentum, batch_size, n_rows = rule
        V, H = W.shape
        if W_speed.stride(0) != W.stride(0):
            raise _lib.MdbnError("a weight matrix and its speed must share the leading dimension")
        p = self.UPDOWN_PATHS[path]
        u = _lib.UpdateArgs()
        u.W, u.W_speed = W.data_ptr(), W_speed.data_ptr()
        if kind in ("gen", "gen_grouped"):
            u.vbias, u.vbias_speed = bias.data_ptr(), bias_speed.data_ptr()
        else:
            u.hbias, u.hbias_speed = bias.data_ptr(), bias_speed.data_ptr()
        u.V, u.H, u.ldv, u.ldh = V, H, int(ldv), W.stride(0)
        u.lr, u.lambda_1, u.lambda_2 = float(lr), float(lambda_1), float(lambda_2)
        u.weightcost, u.momentum = float(weightcost), float(momentum)
        u.batch_size, u.n_rows, u.cost_scale = float(batch_size), float(n_rows), float(cost_scale)
        wp, _ = self.w_planes(W)
        u.W_planes = wp.data_ptr() if wp is not None else None    # kept in step with the matrix by every path that writes it
        nbytes = C.c_int64()
        if kind == "gen_grouped":
            _lib.check(self.lib.mdbn_updown_gen_grouped_workspace_bytes(self.ctx, int(n), V, H, int(ldv), W.stride(0), p,
                                                                        C.byref(nbytes)), "mdbn_updown_gen_grouped_workspace_bytes")
        elif kind == "gen":
            _lib.check(self.lib.mdbn_updown_gen_workspace_bytes(self.ctx, int(n), V, H, int(ldv), W.stride(0), p, C.byref(nbytes)),
                       "mdbn_updown_gen_workspace_bytes")
        else:
            _lib.check(self.lib.mdbn_updown_rec_workspace_bytes(self.ctx, int(n), V, H, int(ldv), W.stride(0), p, C.byref(nbytes)),
                       "mdbn_updown_rec_workspace_bytes")
        ws = getattr(self, "_updown_ws", None)
        if ws is None or ws.numel() * 4 < nbytes.value:
            ws = self._updown_ws = self._alloc_scratch(nbytes.value, "mdbn_updown_%s_workspace_bytes" % kind)
        return u, ws, p

    def updown_gen_step(self, x_lo, x_hi, G, G_speed, vbias, vbias_speed, gauss, lr, lambda_1, lambda_2, weightcost, momentum,
                        batch_size, n_rows, cost_scale=1.0, path="auto"):
        """The generative delta rule of an untied layer (mdbn_updown_gen_step): g = act(x_hi G^T + vbias) from the parameters as
        they are, S = (x_lo - g)^T x_hi, s_v = sum_r (x_lo - g), and the update rule on G / G_speed / vbias / vbias_speed.
        Returns ``cost_scale`` * sum_r -log p(x_lo | x_hi) (up to the Gaussian constant) as a 0-d device tensor.  ``path``:
        "auto", "fused" (one pass over G: n <= 32, ld <= 512; refused elsewhere) or "composed"."""
        x_lo = self.as_matrix(x_lo)
        n, V = (int(v) for v in x_lo.shape)
        if tuple(G.shape) != (V, x_hi.shape[1]) or x_hi.shape[0] != n:
            raise ValueError("x_lo %r, x_hi %r and G %r do not fit" % (tuple(x_lo.shape), tuple(x_hi.shape), tuple(G.shape)))
        x_hi = self._padded(x_hi, n, G.shape[1], G.stride(0))      # the C-ABI reads x_hi with G's ld
        u, ws, p = self._updown_call("gen", n, G, G_speed, vbias, vbias_speed, x_lo.stride(0),
                                     (lr, lambda_1, lambda_2, weightcost, momentum, batch_size, n_rows), cost_scale, path)
        cost = self._next_cost_slot()
        _lib.check(self.lib.mdbn_updown_gen_step(self.ctx, self._stream(), self._p(x_lo), self._p(x_hi), n, int(bool(gauss)),
                                                 C.byref(u), self._p(cost), p, self._p(ws), ws.numel() * 4), "mdbn_updown_gen_step")
        self._w_serial += 1
        self._w_planes_written(G)
        return cost

    def updown_gen_step_grouped(self, x_lo, x_hi, G, G_speed, vbias, vbias_speed, groups, lr, lambda_1, lambda_2, weightcost,
                                momentum, batch_size, n_rows, cost_scale=1.0, path="auto"):
        """``updown_gen_step`` for the input layer of a network with softmax groups (``groups``: its ``GroupTable``;
        mdbn_updown_gen_step_grouped): g = softmax inside every group, sigmoid on the other columns, of x_hi G^T + vbias; the
        same statistics, rule and ``path``.  Returns ``cost_scale`` * sum_r -log p(x_lo | x_hi), the categorical cross-entropy
        from the log-sum-exp plus the Bernoulli cross-entropy outside the span.  Every group of every row of ``x_lo`` must
        hold exactly one 1 (not checked here)."""
        x_lo = self.as_matrix(x_lo)
        n, V = (int(v) for v in x_lo.shape)
        if tuple(G.shape) != (V, x_hi.shape[1]) or x_hi.shape[0] != n:
            raise ValueError("x_lo %r, x_hi %r and G %r do not fit" % (tuple(x_lo.shape), tuple(x_hi.shape), tuple(G.shape)))
        x_hi = self._padded(x_hi, n, G.shape[1], G.stride(0))      # the C-ABI reads x_hi with G's ld
        u, ws, p = self._updown_call("gen_grouped", n, G, G_speed, vbias, vbias_speed, x_lo.stride(0),
                                     (lr, lambda_1, lambda_2, weightcost, momentum, batch_size, n_rows), cost_scale, path)
        cost = self._next_cost_slot()
        _lib.check(self.lib.mdbn_updown_gen_step_grouped(
            self.ctx, self._stream(), self._p(x_lo), self._p(x_hi), n, C.byref(u), self._p(cost), p, self._p(ws), ws.numel() * 4,
            self._p(groups.tensor), C.c_void_p(groups.host.ctypes.data), groups.n_groups), "mdbn_updown_gen_step_grouped")
        self._w_serial += 1
        self._w_planes_written(G)
        return cost

    def updown_rec_step(self, y_lo, y_hi, r, W, W_speed, hbias, hbias_speed, lr, lambda_1, lambda_2, weightcost, momentum,
                        batch_size, n_rows, path="auto"):
        """The recognition delta rule of an untied layer (mdbn_updown_rec_step): S = y_lo^T (y_hi - r), s_h = sum_r (y_hi - r)
        with r = sigmoid(y_lo W + hbias) given, and the update rule on W / W_speed / hbias / hbias_speed.  ``path`` as
        ``updown_gen_step`` ("fused": the thin-batch step's one-pass update on the stacked operands)."""
        y_lo = self.as_matrix(y_lo)
        n, V = (int(v) for v in y_lo.shape)
        H, ldh = int(W.shape[1]), W.stride(0)
        if W.shape[0] != V or tuple(y_hi.shape) != (n, H) or tuple(r.shape) != (n, H):
            raise ValueError("y_lo %r, y_hi %r, r %r and W %r do not fit" % (tuple(y_lo.shape), tuple(y_hi.shape), tuple(r.shape), tuple(W.shape)))
        y_hi, r = self._padded(y_hi, n, H, ldh), self._padded(r, n, H, ldh)
        u, ws, p = self._updown_call("rec", n, W, W_speed, hbias, hbias_speed, y_lo.stride(0),
                                     (lr, lambda_1, lambda_2, weightcost, momentum, batch_size, n_rows), 1.0, path)
        _lib.check(self.lib.mdbn_updown_rec_step(self.ctx, self._stream(), self._p(y_lo), self._p(y_hi), self._p(r), n, C.byref(u), p,
                                                 self._p(ws), ws.numel() * 4), "mdbn_updown_rec_step")
        self._w_serial += 1
        self._w_planes_written(W)
        return None

    # ------------------------------------------------------------------ monitoring helpers (all HIP)
    def round_flip(self, x, flip_col=-1):
        """tensor.round(x) with column ``flip_col`` replaced by 1 - round(x) (rbm.py:428-436)."""
        x = self.as_matrix(x)
        out = self.alloc_matrix(x.shape[0], x.shape[1], x.stride(0))
        if x.shape[0]:
            _lib.check(self.lib.mdbn_round_flip(self.ctx, self._stream(), self._p(x), x.shape[0], x.shape[1],
                                                x.stride(0), int(flip_col), self._p(out)), "mdbn_round_flip")
        return out

    def pl_cost(self, fe, fe_flip, n_visible):
        """-mean(n_visible * softplus(fe - fe_flip)) (rbm.py:442) as a 0-d device tensor."""
        out = torch.zeros(1, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.mdbn_pl_cost(self.ctx, self._stream(), self._p(fe), self._p(fe_flip), fe.numel(),
                                         int(n_visible), self._p(out)), "mdbn_pl_cost")
        return out[0]

    def recon_cost(self, pre, target, gauss):
        """get_reconstruction_cost on given arrays (rbm.py:449-482, :690-699): 0-d device tensor."""
        pre, target = self.as_matrix(pre), self.as_matrix(target)
        assert pre.shape == target.shape
        out = torch.zeros(1, dtype=torch.float32, device=self.device)
        ws = self.workspace(1, 1, 1)
        _lib.check(self.lib.mdbn_recon_cost(self.ctx, self._stream(), self._p(pre), pre.stride(0), self._p(target),
                                            target.stride(0), pre.shape[0], pre.shape[1], int(bool(gauss)),
                                            self._p(out), self._p(ws), ws.numel() * 4), "mdbn_recon_cost")
        return out[0]

    def tanh_(self, x):
        """In-place tanh on a device matrix (HiddenLayer's default activation, mlp.py:36-110)."""
        x = self.as_matrix(x)
        _lib.check(self.lib.mdbn_tanh(self.ctx, self._stream(), self._p(x), x.shape[0], x.shape[1], x.stride(0)),
                   "mdbn_tanh")
        return x

    def count_nonfinite(self, *tensors):
        """Number of NaN / Inf values in the given device tensors (synchronises): the check the
        reference's commented-out NanGuardMode would make (rbm.py:542-543, dbn.py:311)."""
        count = torch.zeros(1, dtype=torch.int32, device=self.device)
        for t in tensors:
            base = t._base if t._base is not None else t           # a padded matrix: scan the whole storage
            _lib.check(self.lib.mdbn_count_nonfinite(self.ctx, self._stream(), self._p(base), base.numel(),
                                                     self._p(count)), "mdbn_count_nonfinite")
        return int(count.item())

    # ------------------------------------------------------------------ RNG (tests / utilities)
    def rng_uniform(self, rows, cols, rng, normal=False):
        out = self.alloc_matrix(rows, cols)
        r = rng.c()
        fn = self.lib.mdbn_rng_normal if normal else self.lib.mdbn_rng_uniform
        _lib.check(fn(self.ctx, self._stream(), self._p(out), rows, cols, out.stride(0), C.byref(r)),
                   "mdbn_rng_*")
        return out

    def kernel_timing(self, enable):
        """Bracket every GEMM launch with HIP events (measurement only; bench.py)."""
        _lib.check(self.lib.mdbn_kernel_timing(self.ctx, int(bool(enable))), "mdbn_kernel_timing")

    def kernel_timing_read(self):
        n, ms = C.c_int64(), C.c_double()
        _lib.check(self.lib.mdbn_kernel_timing_read(self.ctx, C.byref(n), C.byref(ms)),
                   "mdbn_kernel_timing_read")
        return n.value, ms.value

    def narrow_deep_launches(self):
        """Narrow one-plane propdown launches of this engine that took the 64-deep form of their kernel (tests)."""
        n = C.c_int64()
        _lib.check(self.lib.mdbn_narrow_deep_launches(self.ctx, C.byref(n)), "mdbn_narrow_deep_launches")
        return n.value

    def kernel_timing_detail(self, cap=8192):
        """Per recorded GEMM launch: (ms, algorithmic FLOPs, FLOPs issued on its matrix pipe, kind)."""
        ms, alg, pipe = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
        kind, n = (C.c_int32 * cap)(), C.c_int64()
        _lib.check(self.lib.mdbn_kernel_timing_detail(self.ctx, cap, ms, alg, pipe, kind, C.byref(n)),
                   "mdbn_kernel_timing_detail")
        m = min(cap, n.value)
        return [(ms[i], alg[i], pipe[i], kind[i]) for i in range(m)]

    # ------------------------------------------------------------------ bfloat16 wire format (data-parallel reporting mode)
    def narrow_bf16(self, src, out=None):
        """bfloat16 copy of a float32 buffer (round to nearest even; mdbn_f32_to_bf16): the wire form of the packed statistics
        under MDBN_WIRE_BF16=1.  ``out``: a bfloat16 tensor of the same size to fill (kept by the caller across steps)."""
        if out is None or out.numel() != src.numel():
            out = torch.empty(src.numel(), dtype=torch.bfloat16, device=self.device)
        _lib.check(self.lib.mdbn_f32_to_bf16(self.ctx, self._stream(), self._p(src), C.c_void_p(out.data_ptr()), src.numel()),
                   "mdbn_f32_to_bf16")
        return out

    def widen_bf16(self, wire, dst):
        """dst (float32) = wire (bfloat16), exactly (mdbn_bf16_to_f32)."""
        _lib.check(self.lib.mdbn_bf16_to_f32(self.ctx, self._stream(), C.c_void_p(wire.data_ptr()), self._p(dst), dst.numel()),
                   "mdbn_bf16_to_f32")
        return dst

    def cost_values(self, costs):
        """Python floats of a list of 0-d step costs: ONE device-to-host copy per 1024-cost ring block (costs are views into
        such blocks, `_next_cost_slot`; a block is never reused), no device arithmetic.  Synchronises."""
        out, blocks = [0.0] * len(costs), {}
        for i, c in enumerate(costs):
            base = c._base if getattr(c, "_base", None) is not None else c
            blocks.setdefault(id(base), (base, []))[1].append((i, c.storage_offset() - base.storage_offset()))
        for base, items in blocks.values():
            host = base.detach().reshape(-1).cpu().numpy()
            for i, off in items:
                out[i] = float(host[off])
        return out

    def synchronize(self):
        torch.cuda.synchronize(self.device)
