"""GuardedEngine: the HIP engine on workspaces of EXACTLY the bytes the library's sizers answer (TEST-ONLY).

The product engine never hands the library the figure a sizer returns: HipEngine.workspace takes at least 8 MiB and every
allocation carries a 64-float pad (a performance choice -- one allocation serves a whole run).  A C caller allocates the
sizer's bytes and nothing more.  This engine does what that caller does: every workspace is a 16-byte aligned view of
exactly ``nbytes`` bytes, the library is told ``nbytes``, and the view sits inside one larger allocation

    [ front guard | workspace | back guard ]

with both guards at least 1 MiB and the back guard at least as large as the workspace, so a wrong sizer writes into the
test's own memory.  The guards hold a fixed finite bit pattern and are compared bit for bit by ``check_guards``; the
workspace holds NaN (the product allocates with torch.empty: its content is undefined there too), so a kernel that reads
scratch nobody wrote shows up in the comparison with the oracle.

``watching()`` observes what a REFUSED call wrote.  While it is on, every device tensor the engine allocates (alloc_matrix,
alloc_vector, and torch.zeros / empty / full inside mdbn_amd.engine: the outputs of a call, the copies it makes of its
operands, a step's scratch and statistics) is recorded together with the tensors the test hands in; each library call that
takes a workspace is preceded by a snapshot of all of them, and when it returns an error every one is compared with its
snapshot bit for bit."""
import contextlib

import torch

import mdbn_amd

GUARD_BYTES = 1 << 20
PATTERN = 0x4B3C2D1E            # as float32: 1.2332318e7 -- finite, and no value a kernel here would write by chance

_CACHES = ("_pt_ws", "_clamp_ws", "_group_ws", "_center_ws", "_center_rows_ws", "_sigma_ws", "_updown_ws", "_rowll_ws",
           "_rowll_grouped_ws")


class Arena(object):
    def __init__(self, device, nbytes, what):
        assert nbytes > 0 and nbytes % 4 == 0, (what, nbytes)
        self.what, self.nbytes = what, nbytes
        back = max(GUARD_BYTES, (nbytes + 15) & ~15)
        self.lo, self.hi = GUARD_BYTES // 4, (GUARD_BYTES + nbytes) // 4
        self.raw = torch.full(((GUARD_BYTES + nbytes + back) // 4,), PATTERN, dtype=torch.int32, device=device)
        self.view = self.raw[self.lo:self.hi].view(torch.float32)
        self.view.fill_(float("nan"))
        assert self.view.data_ptr() % 16 == 0 and self.view.numel() * 4 == nbytes

    def damage(self):
        """None, or a message naming the first word of a guard that no longer holds the pattern."""
        for name, part, base in (("front", self.raw[:self.lo], -self.hi), ("back", self.raw[self.hi:], 0)):
            bad = torch.nonzero(part != PATTERN)
            if bad.numel():
                first = int(bad[0])
                return ("%s guard of %r (%d bytes) damaged: %d words, the first %d bytes from the workspace's end, holds 0x%08x"
                        % (name, self.what, self.nbytes, bad.numel(), 4 * (base + first), int(part[first]) & 0xFFFFFFFF))
        return None


class _LibProxy(object):
    """The ctypes library with a snapshot before, and a comparison after, every workspace-taking call of a watching engine."""

    def __init__(self, lib, engine):
        self.__dict__["_lib"], self.__dict__["_engine"] = lib, engine

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        eng = self._engine
        if not callable(fn) or eng._watched is None or name.endswith("_bytes") or name.endswith("_bytes_ctx") or \
                name in ("mdbn_kernel_timing", "mdbn_kernel_timing_detail", "mdbn_set_option", "mdbn_last_error"):
            return fn

        def call(*args):
            eng.synchronize()
            before = [(t, t.clone()) for t in eng._watched]
            rc = fn(*args)
            eng.synchronize()
            if rc != 0:
                eng.refusals.append((name, rc))
                for t, snap in before:
                    if not torch.equal(t.view(torch.uint8), snap.view(torch.uint8)):
                        eng.written_by_refused.append((name, tuple(t.shape), str(t.dtype)))
            return rc
        return call


class _TorchShim(object):
    """`torch` as mdbn_amd.engine sees it while an engine watches: zeros / empty / full on the device are recorded."""

    def __init__(self, engine):
        self._engine = engine

    def __getattr__(self, name):
        attr = getattr(torch, name)
        if name not in ("zeros", "empty", "full"):
            return attr
        eng = self._engine

        def make(*a, **kw):
            t = attr(*a, **kw)
            if t.is_cuda:
                eng._watch(t)
            return t
        return make


class GuardedEngine(mdbn_amd.HipEngine):
    WS_FLOOR = 0                # no floor under the shared workspace ...
    WS_PAD = 0                  # ... and no pad behind any

    def __init__(self, *a, **kw):
        self.arenas = []
        self.log = []               # (what, bytes) of every workspace handed out since the last reset
        self.declare_fewer = 0      # floats a feature call's library entry is NOT told about (the real buffer stays whole;
                                    # the shared "workspace" of a case's set-up calls is always declared whole)
        self._watched = None        # the tensors under watch (watching()), or None
        self.refusals, self.written_by_refused = [], []
        super().__init__(*a, **kw)
        self.lib = _LibProxy(self.lib, self)

    def _watch(self, t):
        if self._watched is not None and t.numel():
            base = t if t._base is None else t._base
            if all(base is not w for w in self._watched):
                self._watched.append(base)
        return t

    def alloc_matrix(self, rows, cols, ld=None):
        return self._watch(super().alloc_matrix(rows, cols, ld))

    def alloc_vector(self, n):
        return self._watch(super().alloc_vector(n))

    @contextlib.contextmanager
    def watching(self, *own):
        """Observe a call that is to be refused: `own` are device tensors of the test (in-place operands)."""
        import mdbn_amd.engine as E
        self._watched, self.refusals, self.written_by_refused = [], [], []
        for t in own:
            self._watch(t)
        real = E.torch
        E.torch = _TorchShim(self)
        try:
            yield self
        finally:
            E.torch = real
            self._watched = None

    def _alloc_scratch(self, nbytes, what):
        nbytes = int(nbytes)
        arena = Arena(self.device, nbytes, what)
        self.arenas.append(arena)
        self.log.append((what, nbytes))
        view = arena.view
        return view[:view.numel() - self.declare_fewer] if self.declare_fewer and what != "workspace" else view

    def workspace(self, B, V, H, ldv=None, ldh=None):
        # the shared workspace is never reused: every call gets the bytes of ITS shape
        self._workspace, self._workspace_need = None, 0
        return super().workspace(B, V, H, ldv, ldh)

    def reset(self):
        """A fresh arena for the next case: every cached workspace and scratch goes."""
        self.synchronize()
        self._ws_need.clear()
        self._workspace, self._workspace_need = None, 0
        for name in _CACHES:
            if getattr(self, name, None) is not None:
                setattr(self, name, None)
        self._scratch.clear()
        self.last_scratch = None
        self.arenas, self.log = [], []

    def check_guards(self):
        """After a library call: every guard of every arena handed out since the last reset, bit for bit."""
        self.synchronize()
        assert self.arenas, "no workspace was handed out: the call under test took none from this engine"
        for arena in self.arenas:
            msg = arena.damage()
            assert msg is None, msg
        return [(a.what, a.nbytes) for a in self.arenas]

