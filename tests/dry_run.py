"""A dry-run launch log: the engine's run_forward / run_backward host code issued without a GPU.

    eng.bind(torch.device("cpu")); P = eng.plan(B)          # inside the context: plan() creates the side stream
    with dry_run(eng, gflat=g) as log: eng.run_forward(P, ...); eng.run_backward(P, g, ...)

Inside the context torch.cuda.Stream / Event / stream / current_stream and ops._stream are fakes that log record / wait_event /
wait_stream, and every launching C-ABI symbol (one that takes pointers: its last pointer argument is the stream) is a stub on the
cached CDLL object that logs its arguments and returns 0.  The host-only symbols (*_supported, *_partial_rows, *_splits*, *_bytes,
*_groups, *_tiles, *_blocks, *_route, the version queries: integer arguments only; and tulip_wgrad_group_regions) go through to
the real library.  Everything is restored on exit.

Entries (tuples, in issue order):
    ("launch", symbol, role, args)       role: "chain" (the stream current at entry), "side" (the first stream created inside the
                                         context: the engine's), or the name given to DryRun.stream(name)
        args: one value per C argument but the stream -- scalars as they are; pointers as (buffer name, byte offset), "?" where
        no known buffer holds the address, None for NULL; a struct as a tuple of (field, value) pairs; a struct array as a tuple
        of such tuples (its length: the int argument behind it)
    ("record", role, event)              events are numbered by creation
    ("wait_event", role, event)
    ("wait_stream", role, other role)
    ("hook", role, tag)                  DryRun.note("hook", tag): what a test's bucket hook logs
"""
from __future__ import annotations

import bisect
import contextlib
import ctypes
import hashlib
import re

import torch

from tulip_amd import _lib, ops


class FakeStream:
    def __init__(self, dry, role):
        self.dry, self.role = dry, role
        self.cuda_stream = dry._new_handle(self)

    def wait_event(self, ev):
        self.dry.log.append(("wait_event", self.role, ev.id))

    def wait_stream(self, other):
        self.dry.log.append(("wait_stream", self.role, other.role))


class FakeEvent:
    def __init__(self, dry):
        self.dry, self.id = dry, dry._n_events
        dry._n_events += 1

    def record(self, stream=None):
        self.dry.log.append(("record", (stream or self.dry.current()).role, self.id))


class DryRun:
    def __init__(self, eng, buffers):
        self.eng, self.extra = eng, dict(buffers)
        self.log = []
        self._n_events = 0
        self._handles = {}
        self._stack = [FakeStream(self, "chain")]
        self._index_key, self._starts, self._spans = None, [], []

    # ---- streams
    def _new_handle(self, st):
        h = 0x1000 + len(self._handles)
        self._handles[h] = st
        return h

    def current(self):
        return self._stack[-1]

    def stream(self, name):
        """a further fake stream (a Trainer's detached-bucket stream)"""
        return FakeStream(self, name)

    def _make_stream(self, *a, **k):
        made = len(self._handles)              # the chain is handle 0; the first stream created is the engine's side stream
        return FakeStream(self, "side" if made == 1 else f"stream{made}")

    @contextlib.contextmanager
    def use(self, st):
        self._stack.append(st)
        try:
            yield
        finally:
            self._stack.pop()

    def note(self, kind, what):
        self.log.append((kind, self.current().role, what))

    # ---- pointers
    def _tensors(self):
        eng = self.eng
        yield from self.extra.items()
        W_ = eng.params
        for n in ("flat", "shadow", "packed", "packed_t"):
            yield "params." + n, getattr(W_, n)
        yield from (("rel_index", eng._rel32), ("drop_keep", eng._keep), ("drop_counter", eng._drop_counter))
        for P in eng.plans.values():
            yield from P.bufs.items()
        # the two slab workspaces: the chain's is eng._ws; the side queue's is the other fp32 tensor of that size the engine (or the
        # object that owns its side queue) holds, under whatever attribute
        ws = eng._ws
        yield "ws", ws
        for owner in (eng, vars(eng).get("side")):
            for v in (vars(owner).values() if owner is not None else ()):
                if isinstance(v, torch.Tensor) and v is not ws and v.dtype == ws.dtype and v.numel() == ws.numel():
                    yield "ws_side", v

    def _reindex(self):
        spans = sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), n) for n, t in self._tensors() if t.numel())
        self._spans, self._starts = spans, [s[0] for s in spans]

    def resolve(self, ptr):
        if not ptr:
            return None
        k = bisect.bisect_right(self._starts, ptr) - 1
        if k >= 0 and ptr < self._spans[k][1]:
            return (self._spans[k][2], ptr - self._spans[k][0])
        return "?"

    # ---- arguments
    def _struct(self, s):
        return tuple((n, self.resolve(getattr(s, n)) if t is ctypes.c_void_p else getattr(s, n)) for n, t in s._fields_)

    def _arg(self, a, argtype, nxt):
        if isinstance(a, ctypes.Array):
            return tuple(self._struct(a[i]) for i in range(nxt))
        if type(a).__name__ == "CArgObject":              # ctypes.byref(struct) / byref(array, byte offset)
            obj = a._obj
            if isinstance(obj, ctypes.Array):
                off = int(re.search(r"\((0x[0-9a-f]+)\)", repr(a)).group(1), 16) - ctypes.addressof(obj)
                first = off // ctypes.sizeof(obj._type_)
                return tuple(self._struct(obj[first + i]) for i in range(nxt))
            return self._struct(obj)
        if argtype is ctypes.c_void_p:
            return self.resolve(a)
        return a

    def _stub(self, name, argtypes):
        si = max(i for i, t in enumerate(argtypes) if t is ctypes.c_void_p)      # the stream: the last pointer argument

        def launch(*args):
            assert len(args) == len(argtypes), name
            key = tuple(len(P.bufs) for P in self.eng.plans.values()), sum(
                t.data_ptr() for P in self.eng.plans.values() for t in P.bufs.values())
            if key != self._index_key:                     # a scratch buffer was created or regrown
                self._index_key = key
                self._reindex()
            role = self._handles[args[si]].role
            vals = tuple(self._arg(a, t, args[i + 1] if i + 1 < len(args) and isinstance(args[i + 1], int) else 0)
                         for i, (a, t) in enumerate(zip(args, argtypes)) if i != si)
            self.log.append(("launch", name, role, vals))
            return 0
        return launch

    # ---- reading the log
    def text(self):
        return "\n".join(repr(e) for e in self.log) + "\n"

    def sha256(self):
        return hashlib.sha256(self.text().encode()).hexdigest()


@contextlib.contextmanager
def dry_run(eng, **buffers):
    """buffers: name=tensor of what the launches address besides the engine's own buffers (gflat, the AdamW state, ...)."""
    dry = DryRun(eng, buffers)
    lib = _lib.load()
    real = {n: getattr(lib, n) for n, at in _lib.SIGNATURES.items() if ctypes.c_void_p in at and n != "tulip_wgrad_group_regions"}
    cuda = torch.cuda
    saved = (cuda.Stream, cuda.Event, cuda.stream, cuda.current_stream, ops._stream)
    try:
        for n in real:
            setattr(lib, n, dry._stub(n, _lib.SIGNATURES[n]))     # (the CDLL object caches its symbols as instance attributes)
        cuda.Stream, cuda.Event = dry._make_stream, (lambda *a, **k: FakeEvent(dry))
        cuda.stream, cuda.current_stream = dry.use, (lambda *a, **k: dry.current())
        ops._stream = lambda: dry.current().cuda_stream
        yield dry
    finally:
        cuda.Stream, cuda.Event, cuda.stream, cuda.current_stream, ops._stream = saved
        for n, fn in real.items():
            setattr(lib, n, fn)
