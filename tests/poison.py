"""Poisoned, guarded allocations for tests/test_cpu_poison.py and tests/test_gpu_poison.py (a plain helper module, imported by name).

Every buffer the package hands to the library comes from one of four uninitialised-allocation spellings: `torch.empty`,
`torch.empty_like`, `Tensor.new_empty`, `torch.empty_strided` (tests/test_cpu_poison.py scans bin_amd/ for a fifth).  Under
`poisoned(byte)` each of them allocates `nbytes + 2 * GUARD` bytes of uint8 instead, fills the payload with `byte` and the two guard
bands with GUARD_BYTE, and returns the payload viewed as the requested dtype, shape and strides.  Two properties follow, with no
sanitizer and no tolerance:

  * a call whose results are the same bits under BYTES = (0x00, 0x47, 0xFF) reads no byte of its buffers that it did not write first
    (0xFF.. is NaN in fp16, fp32 and fp64 and -1 as an integer; 0x47.. is finite in every float type — fp16 7.28, fp32 5.1e4 — and so
    survives a clamp or an fmaxf that would swallow a NaN);
  * guard bands that still hold GUARD_BYTE at exit mean that nothing was WRITTEN up to GUARD bytes before or after a buffer.

What this instrument does not see: out-of-bounds READS (they return whatever lies there, guard bytes included, and leave no trace
unless the value reaches a result), and writes further than GUARD bytes away.

`poison_caches(byte)` fills the buffers that outlive a call (rdn_plan's workspaces, ops' score workspaces, a GradGuard's workspace),
or drops them so that the next call allocates them again under the patch.  Status words, grad records and anything created with
`torch.zeros` are state, not scratch, and are left alone."""
import contextlib
import sys
import threading

import torch

GUARD = 256                    # bytes before and after every payload; a multiple of every vector width, so alignment is kept
GUARD_BYTE = 0xA5
BYTES = (0x00, 0x47, 0xFF)

_MISSING = object()
_local = threading.local()


class GuardError(AssertionError):
    """A guard band of a poisoned allocation was written."""


class Allocation:
    __slots__ = ("base", "nbytes", "dtype", "shape", "site")

    def __init__(self, base, nbytes, dtype, shape, site):
        self.base, self.nbytes, self.dtype, self.shape, self.site = base, nbytes, dtype, shape, site

    def describe(self):
        return f"{self.nbytes} bytes, {self.dtype} {tuple(self.shape)} on {self.base.device}, allocated at {self.site}"


class Record:
    """What `poisoned` yields: the allocations it replaced.  `count` and `nbytes` are what a test prints and asserts on."""

    def __init__(self, byte):
        self.byte, self.allocs = byte, []

    @property
    def count(self):
        return len(self.allocs)

    @property
    def nbytes(self):
        return sum(a.nbytes for a in self.allocs)

    def check_guards(self):
        """Compare every guard band with GUARD_BYTE (one host read per device); raises GuardError naming the allocations."""
        by_dev = {}
        for a in self.allocs:
            head, tail = a.base[:GUARD], a.base[GUARD + a.nbytes:]
            bad = torch.stack(((head != GUARD_BYTE).any(), (tail != GUARD_BYTE).any()))
            by_dev.setdefault(a.base.device, []).append((a, bad))
        broken = []
        for items in by_dev.values():
            flags = torch.stack([b for _, b in items]).cpu()
            for (a, _), (before, after) in zip(items, flags.tolist()):
                if before or after:
                    where = " and ".join(w for w, f in (("before", before), ("after", after)) if f)
                    broken.append(f"guard band {where} the buffer overwritten: {a.describe()}")
        if broken:
            raise GuardError("\n".join(broken))


def _site():
    """file:line (function) of the first frame outside this module: who asked for the allocation."""
    f = sys._getframe(1)
    while f is not None and f.f_code.co_filename == __file__:
        f = f.f_back
    if f is None:
        return "?"
    return f"{f.f_code.co_filename}:{f.f_lineno} ({f.f_code.co_name})"


def _extent(size, stride):
    """Elements of storage a (size, stride) view reaches from its first element."""
    if any(s == 0 for s in size):
        return 0
    return 1 + sum((s - 1) * st for s, st in zip(size, stride))


def _make(orig, rec, devices, fallback_device, args, kwargs, through=None):
    """The replacement body: `orig(*args, **kwargs)` as a poisoned, guarded allocation, or untouched where it passes through
    (`through`: the untouched call, where it is not `orig` itself)."""
    if through is not None:
        if getattr(_local, "inside", False):
            return through()
        real, orig = orig, lambda *a, **k: through() if k.get("device") != "meta" else real(*a, **k)
    if getattr(_local, "inside", False):
        return orig(*args, **kwargs)
    device = kwargs.get("device")
    device = torch.device(device) if device is not None else fallback_device()
    sparse = kwargs.get("layout", torch.strided) is not torch.strided
    if device.type not in devices or kwargs.get("pin_memory") or kwargs.get("out") is not None or sparse:
        return orig(*args, **kwargs)                 # host and pinned memory, out= and sparse layouts: not the package's scratch
    if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        return orig(*args, **kwargs)                 # a capture records no fills of ours, and its pool is private
    _local.inside = True
    try:
        meta_kw = {k: v for k, v in kwargs.items() if k not in ("pin_memory", "requires_grad")}
        meta_kw["device"] = "meta"
        meta = orig(*args, **meta_kw)                # shape, dtype and strides exactly as the real call would choose them
        size, stride = tuple(meta.shape), tuple(meta.stride())
        nbytes = _extent(size, stride) * meta.element_size()
        base = torch.empty(nbytes + 2 * GUARD, dtype=torch.uint8, device=device)     # (current stream; `inside` lets it through)
        base.fill_(GUARD_BYTE)
        payload = base[GUARD:GUARD + nbytes]
        payload.fill_(rec.byte)
        out = payload.view(meta.dtype).as_strided(size, stride)
        if kwargs.get("requires_grad"):
            out.requires_grad_()
        rec.allocs.append(Allocation(base, nbytes, meta.dtype, size, _site()))
        return out
    finally:
        _local.inside = False


@contextlib.contextmanager
def poisoned(byte, devices=("cuda",)):
    """Replace the four allocation spellings (module docstring) for the body; yields the Record.  `devices`: the device types whose
    allocations are poisoned — the package's buffers live on the GPU, so host allocations pass through untouched by default; the CPU
    tests of the instrument itself pass ("cpu",).  On a clean exit the guard bands are checked (GuardError); the replacements are
    restored in any case."""
    rec = Record(int(byte))
    devices = tuple(devices)

    def default_device():
        return torch.get_default_device() if hasattr(torch, "get_default_device") else torch.device("cpu")

    o_empty, o_like, o_strided = torch.empty, torch.empty_like, torch.empty_strided
    o_new_own = torch.Tensor.__dict__.get("new_empty", _MISSING)
    o_new = torch.Tensor.new_empty

    def empty(*args, **kwargs):
        return _make(o_empty, rec, devices, default_device, args, kwargs)

    def empty_like(x, *args, **kwargs):
        return _make(o_like, rec, devices, lambda: x.device, (x,) + args, kwargs)

    def empty_strided(*args, **kwargs):
        return _make(o_strided, rec, devices, default_device, args, kwargs)

    def new_empty(self, *args, **kwargs):
        kw = dict(kwargs)
        kw.setdefault("dtype", self.dtype)
        kw.setdefault("device", self.device)
        return _make(o_empty, rec, devices, lambda: self.device, args, kw, through=lambda: o_new(self, *args, **kwargs))

    torch.empty, torch.empty_like, torch.empty_strided = empty, empty_like, empty_strided
    torch.Tensor.new_empty = new_empty
    try:
        yield rec
    finally:
        torch.empty, torch.empty_like, torch.empty_strided = o_empty, o_like, o_strided
        if o_new_own is _MISSING:
            del torch.Tensor.new_empty
        else:
            torch.Tensor.new_empty = o_new_own
    rec.check_guards()


def poison_caches(byte, owners=(), release=False):
    """Fill every cached scratch buffer that outlives a call with `byte`: the values of bin_amd.rdn_plan._workspaces, of
    bin_amd.ops._score_ws, and the `_workspace` of every object in `owners` (bin_amd.optim.GradGuard keeps one).  `release=True`
    drops them instead, so that the next call allocates them again — under `poisoned`, with guard bands.  Returns the bytes filled."""
    from bin_amd import ops, rdn_plan
    total = 0
    if release:
        rdn_plan.release_workspaces()
        ops._score_ws.clear()
        for o in owners:
            o._workspace = None
        return 0
    bufs = list(rdn_plan._workspaces.values()) + list(ops._score_ws.values())
    bufs += [o._workspace for o in owners if getattr(o, "_workspace", None) is not None]
    for t in bufs:
        t.view(-1).view(torch.uint8).fill_(int(byte))
        total += t.numel() * t.element_size()
    return total


def bits(t):
    """`t` as integers of its element width, so that torch.equal compares NaNs and signed zeros bit for bit."""
    t = t.detach().contiguous()
    if t.dtype.is_floating_point:
        t = t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))
