"""The instrument of tests/test_gpu_poison.py (tests/poison.py) shown to be sensitive, on host memory: a function that writes all of
its output gives the same bits under the three fill bytes, one that leaves an element unwritten does not, a write one element past a
buffer breaks a guard band and is named, a function that allocates nothing is seen as such, host allocations pass through by default,
and the patch goes away after an exception.  The last test scans bin_amd/ for an uninitialised-allocation spelling the helper does not
replace.  No GPU is involved."""
import os
import re

import pytest
import torch

from poison import BYTES, GUARD, GUARD_BYTE, GuardError, poison_caches, poisoned, same_bits

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = ("cpu",)


def _clean(x):
    y = torch.empty(x.shape, dtype=torch.float32)
    z = torch.empty_like(x)
    torch.mul(x, 2.0, out=y)
    z.copy_(y + 1)
    return z


def _leaky(x):
    y = torch.empty(x.numel(), dtype=torch.float32)
    y[:-1] = x.reshape(-1)[:-1] * 2.0                  # the last element is never written
    return y


def _oob(x):
    y = torch.empty(x.numel(), dtype=torch.float32)
    y.copy_(x.reshape(-1))
    y.as_strided((1,), (1,), y.storage_offset() + x.numel()).fill_(3.0)     # one element past the end
    return y


def _runs(fn, x):
    outs, counts = [], []
    for b in BYTES:
        with poisoned(b, devices=CPU) as rec:
            outs.append(fn(x))
        counts.append(rec.count)
    return outs, counts


def test_clean_function_is_identical_under_the_three_bytes():
    x = torch.arange(37, dtype=torch.float32).reshape(1, 37)
    outs, counts = _runs(_clean, x)
    assert counts == [2, 2, 2]
    assert all(same_bits(outs[0], o) for o in outs[1:])
    assert torch.equal(outs[0], x * 2 + 1)


def test_leaky_function_differs_between_bytes():
    x = torch.arange(37, dtype=torch.float32)
    outs, counts = _runs(_leaky, x)
    assert counts == [1, 1, 1]
    assert all(torch.equal(o[:-1], outs[0][:-1]) for o in outs)
    assert float(outs[0][-1]) == 0.0 and bool(torch.isnan(outs[2][-1]))
    assert outs[1][-1:].view(torch.int32).item() == 0x47474747 and bool(torch.isfinite(outs[1][-1]))
    assert not same_bits(outs[0], outs[1]) and not same_bits(outs[0], outs[2]) and not same_bits(outs[1], outs[2])


def test_the_poison_reads_as_documented_in_every_float_type():
    for dt, finite in ((torch.float16, 7.27734375), (torch.float32, 51015.27734375), (torch.float64, None)):
        with poisoned(0x47, devices=CPU):
            t = torch.empty(3, dtype=dt)
        assert bool(torch.isfinite(t).all())
        if finite is not None:
            assert float(t[0]) == finite
        with poisoned(0xFF, devices=CPU):
            t = torch.empty(3, dtype=dt)
        assert bool(torch.isnan(t).all())
    with poisoned(0xFF, devices=CPU):
        assert torch.empty(2, dtype=torch.int32).tolist() == [-1, -1]


def test_out_of_bounds_write_breaks_a_guard_and_is_named():
    x = torch.arange(5, dtype=torch.float32)
    with pytest.raises(GuardError) as e:
        with poisoned(0x00, devices=CPU):
            _oob(x)
    msg = str(e.value)
    assert "after the buffer" in msg and "before" not in msg
    assert "20 bytes" in msg and "torch.float32 (5,)" in msg
    assert "test_cpu_poison.py" in msg and "(_oob)" in msg
    # ... and a write before the buffer
    with pytest.raises(GuardError, match="before the buffer"):
        with poisoned(0x00, devices=CPU) as rec:
            t = torch.empty(4, dtype=torch.uint8)
            rec.allocs[0].base[GUARD - 1] = 0


def test_function_that_allocates_nothing_has_count_zero():
    x = torch.arange(5, dtype=torch.float32)
    with poisoned(0xFF, devices=CPU) as rec:
        y = torch.zeros(5) + x
    assert rec.count == 0 and rec.nbytes == 0
    assert torch.equal(y, x)


def test_every_spelling_is_replaced_and_keeps_shape_dtype_strides_and_alignment():
    src = torch.zeros(3, 5, dtype=torch.float16).t()                   # non-contiguous: empty_like preserves its strides
    with poisoned(0x47, devices=CPU) as rec:
        a = torch.empty(2, 3, dtype=torch.float64)
        b = torch.empty((4,), dtype=torch.int32, device="cpu")
        c = torch.empty_like(src)
        d = torch.empty_like(src, memory_format=torch.contiguous_format)
        e = src.new_empty((7,))
        f = src.new_empty(2, 2, dtype=torch.float32)
        g = torch.empty_strided((2, 3), (1, 2), dtype=torch.float32)
        z = torch.empty(0, dtype=torch.float32)
        ref = [(t.shape, t.dtype, t.stride()) for t in (a, b, c, d, e, f, g, z)]
    assert rec.count == 8
    assert ref == [((2, 3), torch.float64, (3, 1)), ((4,), torch.int32, (1,)), ((5, 3), torch.float16, (1, 5)),
                   ((5, 3), torch.float16, (3, 1)), ((7,), torch.float16, (1,)), ((2, 2), torch.float32, (2, 1)),
                   ((2, 3), torch.float32, (1, 2)), ((0,), torch.float32, (1,))]
    assert rec.nbytes == 48 + 16 + 30 + 30 + 14 + 16 + 24 + 0
    for al, t in zip(rec.allocs, (a, b, c, d, e, f, g, z)):
        assert al.base.numel() == al.nbytes + 2 * GUARD
        assert t.storage_offset() * t.element_size() == GUARD            # GUARD is a multiple of 256: the base's alignment is kept
        assert bool((al.base[:GUARD] == GUARD_BYTE).all()) and bool((al.base[GUARD + al.nbytes:] == GUARD_BYTE).all())
        assert bool((al.base[GUARD:GUARD + al.nbytes] == 0x47).all())
    assert GUARD % 256 == 0


def test_host_and_pinned_allocations_pass_through_by_default(monkeypatch):
    seen = []
    real = torch.empty

    def recording(*args, **kwargs):
        seen.append(kwargs)
        return real(*args, **{k: v for k, v in kwargs.items() if k != "pin_memory"})
    monkeypatch.setattr(torch, "empty", recording)
    with poisoned(0xFF) as rec:                                         # default: only device memory is poisoned
        a = torch.empty(4, dtype=torch.float32)
        b = torch.empty(4, dtype=torch.uint8, pin_memory=True)
        c = torch.empty_like(a)
        d = a.new_empty((3,))
    assert rec.count == 0
    assert seen == [{"dtype": torch.float32}, {"dtype": torch.uint8, "pin_memory": True}]
    assert a.shape == c.shape == (4,) and b.dtype == torch.uint8 and d.shape == (3,)
    seen.clear()
    with poisoned(0xFF, devices=CPU) as rec:                            # pinned memory passes through even where the host is poisoned
        torch.empty(4, dtype=torch.uint8, pin_memory=True)
        torch.empty(4, dtype=torch.float32, out=a)
    assert rec.count == 0 and len(seen) == 2
    assert torch.empty is recording


def test_patch_is_removed_after_an_exception():
    before = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__)
    with pytest.raises(ZeroDivisionError):
        with poisoned(0x47, devices=CPU):
            assert torch.empty is not before[0] and torch.Tensor.new_empty is not before[3]
            t = torch.empty(4, dtype=torch.uint8)
            t.as_strided((1,), (1,), t.storage_offset() + 4).fill_(0)          # a broken guard does not mask the body's own exception
            1 / 0
    after = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__)
    assert all(a is b for a, b in zip(before, after))
    assert bool((torch.zeros(3).new_empty((2,)).shape == (2,)))


def test_poison_caches_fills_or_drops_what_outlives_a_call():
    from bin_amd import ops, rdn_plan

    class Owner:
        _workspace = None
    own = Owner()
    own._workspace = torch.zeros(5, dtype=torch.float64)
    saved_ws, saved_sc = dict(rdn_plan._workspaces), dict(ops._score_ws)
    try:
        rdn_plan._workspaces.clear()
        ops._score_ws.clear()
        rdn_plan._workspaces[("cpu", None, 0, "fwd")] = torch.zeros(33, dtype=torch.uint8)
        ops._score_ws[("k",)] = torch.zeros(64, dtype=torch.uint8)
        assert poison_caches(0xFF, owners=[own]) == 33 + 64 + 40
        assert bool((rdn_plan._workspaces[("cpu", None, 0, "fwd")] == 0xFF).all()) and bool((ops._score_ws[("k",)] == 0xFF).all())
        assert bool(torch.isnan(own._workspace).all())
        assert poison_caches(0x00, owners=[own], release=True) == 0
        assert not rdn_plan._workspaces and not ops._score_ws and own._workspace is None
    finally:
        rdn_plan._workspaces.clear()
        rdn_plan._workspaces.update(saved_ws)
        ops._score_ws.clear()
        ops._score_ws.update(saved_sc)


# Names under which PyTorch hands out uninitialised memory.  The first four are what poison.py replaces; any other one in bin_amd/ would
# escape the instrument, as would binding one of the four to another name at import time.
_REPLACED = (r"\btorch\.empty\(", r"\btorch\.empty_like\(", r"\.new_empty\(", r"\btorch\.empty_strided\(")
_ESCAPES = (r"\bempty_permuted\b", r"\bempty_quantized\b", r"\bnew_empty_strided\b", r"\.new\(", r"\.resize_\(", r"\.resize_as_\(",
            r"\btorch\.(cuda\.)?(Half|Float|Double|Byte|Char|Short|Int|Long|Bool|BFloat16)?(Tensor|Storage)\(",
            r"\bUntypedStorage\b", r"\bTypedStorage\b", r"\bcaching_allocator_alloc\b", r"\b_empty_affine_quantized\b",
            r"\bfrom\s+torch\s+import\b[^\n]*\bempty", r"\bimport\s+torch\s+as\b", r"=\s*torch\.empty(_like|_strided)?\s*(#|$)",
            r"\bgetattr\(\s*torch\s*,", r"\bops\.aten\.(empty|new_empty)", r"\btorch\._C\._")


def test_the_package_allocates_through_the_replaced_spellings_only():
    found, used = [], {p: 0 for p in _REPLACED}
    root = os.path.join(REPO, "bin_amd")
    n_files = 0
    for d, _, files in os.walk(root):
        for f in files:
            if not f.endswith(".py"):
                continue
            n_files += 1
            path = os.path.join(d, f)
            with open(path, encoding="utf-8") as fh:
                for ln, line in enumerate(fh, 1):
                    code = line.split("#", 1)[0] if not line.lstrip().startswith("#") else ""
                    for p in _REPLACED:
                        used[p] += len(re.findall(p, code))
                    # any other way of spelling `empty` on torch or a tensor: torch.<x>empty<y>( or .<x>empty<y>( beyond the four
                    for m in re.finditer(r"(?:\btorch\.|\.)(\w*empty\w*)\(", code):
                        if m.group(1) not in ("empty", "empty_like", "empty_strided", "new_empty", "_empty"):
                            found.append(f"{os.path.relpath(path, REPO)}:{ln}: {m.group(0)}")
                        elif m.group(1) in ("empty", "_empty") and not re.search(r"\b(torch|np|CP)\.empty\($|\b_empty\($", code[:m.end()]):
                            found.append(f"{os.path.relpath(path, REPO)}:{ln}: {m.group(0)} on an unknown owner")
                    for p in _ESCAPES:
                        if re.search(p, code):
                            found.append(f"{os.path.relpath(path, REPO)}:{ln}: {p}")
    assert n_files > 20
    assert used[_REPLACED[0]] > 50 and used[_REPLACED[1]] > 5, used       # the scan sees the package's allocations at all
    assert not found, "uninitialised allocations that tests/poison.py does not replace:\n" + "\n".join(found)
