"""-m gpu: every relayout entry point writes, byte for byte, what the numpy statement of the layout (tests/relayout_cases.py) says
— hi, lo and bias — through the per-op entry (where the case has one), a batch call of one item and one batch call of 24 items (all
cases twice: the second copy lands in the second launch), with and without a lo plane, and nothing past the end of a buffer."""
import ctypes as C

import numpy as np
import pytest
import torch

import relayout_cases as R

pytestmark = pytest.mark.gpu

GUARD = 64                      # elements after every output buffer
GUARD_H, GUARD_F = 0x5a5a, 0x5a5a5a5a


@pytest.fixture(scope="module")
def table():
    """Per case: (device sources, device bias or None, expected hi / lo as int16 and bias_out as int32 device tensors)."""
    rows = []
    for c in R.CASES:
        srcs, bias = R.case_sources(c)
        hi, lo, bp = R.case_expected(c, srcs, bias)
        rows.append(([torch.from_numpy(s).cuda() for s in srcs], torch.from_numpy(bias).cuda() if bias is not None else None,
                     torch.from_numpy(hi.view(np.int16)).cuda(), torch.from_numpy(lo.view(np.int16)).cuda(),
                     torch.from_numpy(bp.view(np.int32)).cuda()))
    return rows


class Out:
    """Output buffers of one relayout, each followed by a guard pattern."""

    def __init__(self, c, with_lo):
        n = c.rows_pad * c.chunks * c.k * c.k * 16
        self.n, self.rows = n, c.rows_pad
        self.hi = torch.full((n + GUARD,), GUARD_H, dtype=torch.int16, device="cuda")
        self.lo = torch.full((n + GUARD,), GUARD_H, dtype=torch.int16, device="cuda") if with_lo else None
        self.bias = torch.full((c.rows_pad + GUARD,), GUARD_F, dtype=torch.int32, device="cuda")

    def check(self, row, what):
        _, _, hi, lo, bp = row
        assert self.n == hi.numel() and self.rows == bp.numel()
        for name, got, want in (("hi", self.hi, hi), ("lo", self.lo, lo), ("bias", self.bias, bp)):
            if got is None:
                continue
            pattern = GUARD_F if name == "bias" else GUARD_H
            assert bool((got[want.numel():] == pattern).all()), (what, name, "guard")
            bad = int((got[:want.numel()] != want).sum())
            assert bad == 0, (what, name, "%d of %d differ" % (bad, want.numel()))


def _item(c, row, out):
    from bin_amd import _lib as L
    it = L.BinRelayoutItem()
    for i, s in enumerate(row[0]):
        it.w[i] = s.data_ptr()
    it.bias = row[1].data_ptr() if row[1] is not None else None
    it.w_hi, it.w_lo, it.bias_out = out.hi.data_ptr(), (out.lo.data_ptr() if out.lo is not None else None), out.bias.data_ptr()
    it.kind, it.cout, it.cin, it.ksize, it.rows_pad, it.cin_chunks, it.cout_block, it.shuffle_or_group = \
        c.kind, c.cout, c.cin, c.k, c.rows_pad, c.chunks, c.cb, c.sg
    if c.shape is not None and c.shape != (96, 4, 32):          # bin_stage4's block goes as all zero, the default
        it.shape.G0, it.shape.C, it.shape.G = c.shape
    return it


def _per_op(lib, c, row, out):
    """The per-op entry of the case's kind, or None where the ABI has none (a dense block other than bin_stage4's)."""
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    null = C.c_void_p(0)
    if c.kind == R.FWD:
        return lib.binhip_weights_relayout(p(row[0][0]), p(row[1]), c.cout, c.cin, c.k, c.rows_pad, c.chunks, c.cb, c.sg,
                                           p(out.hi), p(out.lo), p(out.bias), null)
    if c.kind == R.DGRAD:
        return lib.binhip_weights_relayout_dgrad(p(row[0][0]), c.cout, c.cin, c.k, c.rows_pad, c.chunks, c.cb, c.sg,
                                                 p(out.hi), p(out.lo), p(out.bias), null)
    if c.shape != (96, 4, 32):
        return None
    arr = (C.c_void_p * 4)(*[s.data_ptr() if i >= c.sg else None for i, s in enumerate(row[0])])   # entries < group may be NULL
    return lib.binhip_weights_relayout_rdb_gather(arr, c.sg, c.cb, p(out.hi), p(out.lo), p(out.bias), null)


@pytest.mark.parametrize("with_lo", [True, False], ids=["hi+lo", "hi"])
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=[R.case_id(c) for c in R.CASES])
def test_per_op_and_single_item_batch_write_the_stated_layout(i, with_lo, table):
    from bin_amd import _lib as L
    lib, c, row = L.lib(), R.CASES[i], table[i]
    out = Out(c, with_lo)
    rc = _per_op(lib, c, row, out)
    if rc is not None:
        assert rc == 0
        torch.cuda.synchronize()
        out.check(row, "per-op")
    out = Out(c, with_lo)
    it = _item(c, row, out)
    assert lib.binhip_weights_relayout_batch(C.byref(it), 1, C.c_void_p(0)) == 0
    torch.cuda.synchronize()
    out.check(row, "batch of one")


@pytest.mark.parametrize("with_lo", [True, False], ids=["hi+lo", "hi"])
def test_one_batch_call_of_24_items_writes_the_stated_layout(with_lo, table):
    """All twelve cases twice, into separate buffers, in ONE call: items 22 and 23 go out in a second launch."""
    from bin_amd import _lib as L
    lib = L.lib()
    order = list(range(len(R.CASES))) * 2
    assert len(order) == 24
    outs = [Out(R.CASES[i], with_lo) for i in order]
    items = [_item(R.CASES[i], table[i], o) for i, o in zip(order, outs)]
    arr = (L.BinRelayoutItem * len(items))(*items)
    assert lib.binhip_weights_relayout_batch(arr, len(items), C.c_void_p(0)) == 0
    torch.cuda.synchronize()
    for n, (i, o) in enumerate(zip(order, outs)):
        o.check(table[i], "item %d (%s)" % (n, R.case_id(R.CASES[i])))
