"""CPU: the numpy statement of the weight relayout (tests/relayout_cases.py) means what include/binhip.h says — its operators are the
forward convolution, PixelShuffle's channel order, the transposed convolution and the dense block's input gradient, in float64 — and
every return code of the relayout entry points' validation, which happens before any HIP call."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import relayout_cases as R

# both sides add the same float64 products in different orders
RTOL = 1e-12


def _close(a, b):
    return float((a - b).abs().max()) <= RTOL * max(1.0, float(b.abs().max()))


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("cout,cin,k,rows_pad,chunks", [(40, 24, 3, 64, 2), (12, 24, 5, 32, 2), (64, 16, 1, 64, 1)])
def test_fwd_operator_is_the_convolution(cout, cin, k, rows_pad, chunks):
    w, b, x = _rand(1, cout, cin, k, k), _rand(2, cout), _rand(3, 2, cin, 7, 9)
    wp, bp = R.fwd_operator(w.numpy(), b.numpy(), rows_pad, chunks, 0)
    xp = F.pad(x, (0, 0, 0, 0, 0, 16 * chunks - cin))                      # the planes' zero channels
    y = F.conv2d(xp, torch.from_numpy(wp), torch.from_numpy(bp), padding=k // 2)
    assert _close(y[:, :cout], F.conv2d(x, w, b, padding=k // 2))
    assert float(y[:, cout:].abs().max()) == 0.0 if cout < rows_pad else True


def test_fwd_operator_with_shuffle_is_the_convolution_in_pixelshuffle_order():
    """Rows [sub][cout / 4]: sub-position `sub` of PixelShuffle(2) is one contiguous group of rows, i.e. a plain plane store."""
    w, b, x = _rand(4, 64, 16, 3, 3), _rand(5, 64), _rand(6, 2, 16, 6, 5)
    wp, bp = R.fwd_operator(w.numpy(), b.numpy(), 64, 1, 1)
    y = F.conv2d(x, torch.from_numpy(wp), torch.from_numpy(bp), padding=1)                # [n, sub * 16 + c, h, w]
    n, _, h, wd = y.shape
    shuffled = y.view(n, 2, 2, 16, h, wd).permute(0, 3, 4, 1, 5, 2).reshape(n, 16, 2 * h, 2 * wd)
    assert _close(shuffled, F.pixel_shuffle(F.conv2d(x, w, b, padding=1), 2))


@pytest.mark.parametrize("cout,cin,k,rows_pad,chunks,shuffle", [(3, 64, 3, 64, 1, 0), (64, 40, 3, 64, 4, 1), (24, 12, 5, 32, 2, 0)])
def test_dgrad_operator_is_the_transposed_convolution(cout, cin, k, rows_pad, chunks, shuffle):
    w, gy = _rand(7, cout, cin, k, k), _rand(8, 2, cout, 6, 7)
    wp, bp = R.dgrad_operator(w.numpy(), rows_pad, chunks, shuffle)
    g_in = gy
    if shuffle:                                                            # the gradient arrives in UPNet.0's permuted row order
        g_in = gy[:, [R.permuted(j, cout) for j in range(cout)]]
    g_in = F.pad(g_in, (0, 0, 0, 0, 0, 16 * chunks - cout))
    gx = F.conv2d(g_in, torch.from_numpy(wp), padding=k // 2)
    assert _close(gx[:, :cin], F.conv_transpose2d(gy, w, padding=k // 2))
    assert not bp.any() and (cin == rows_pad or float(gx[:, cin:].abs().max()) == 0.0)


@pytest.mark.parametrize("shape", [(96, 4, 32), (64, 3, 64)])
def test_gather_operators_sum_to_the_dense_block_input_gradient(shape):
    """The construction of tests/test_cpu_oracle.py::test_rdb_backward_data_gather_form_identity, with the gather weights taken from
    the relayout oracle: group g (g = 0: the block's inputs, g >= 1: conv g-1's outputs) is ONE conv of the stacked masked output
    gradients of convs g..C-1; chained from the last group down, group 0 is the autograd gradient of the block's input."""
    G0, Cn, G = shape
    ws = [_rand(10 + c, G, G0 + G * c, 3, 3) * 0.1 for c in range(Cn)]
    x = _rand(20, 1, G0, 6, 7).requires_grad_()
    gys = [_rand(30 + c, 1, G, 6, 7) for c in range(Cn)]                    # the upstream gradient on each conv's output
    acts, cat = [], x
    for c in range(Cn):
        acts.append(F.relu(F.conv2d(cat, ws[c], padding=1)))
        cat = torch.cat((cat, acts[-1]), 1)
    (gx_ref,) = torch.autograd.grad(cat[:, G0:], x, torch.cat(gys, 1))
    ops_ = [torch.from_numpy(R.gather_operator([w.numpy() for w in ws], g, shape)[0]) for g in range(Cn)]
    Gm = [None] * Cn                                                        # masked output gradients of conv 0 .. C-1
    Gm[Cn - 1] = gys[Cn - 1] * (acts[Cn - 1] > 0)
    for g in range(Cn - 1, 0, -1):                                          # group g holds conv g-1's output
        Gm[g - 1] = (gys[g - 1] + F.conv2d(torch.cat(Gm[g:], 1), ops_[g], padding=1)) * (acts[g - 1] > 0)
    gx = F.conv2d(torch.cat(Gm, 1), ops_[0], padding=1)
    assert _close(gx, gx_ref.detach())


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_planes_place_and_round_the_operator(case):
    """Slot placement and hi / lo on rows 0, 7, 8, 15, 24 of every row block, written out per slot: rows 8-15 and 24-31 carry their
    two 8-channel slots swapped; hi = fp16(w), lo = fp16(w - hi)."""
    srcs, bias = R.case_sources(case)
    wp, _ = R.case_operator(case, srcs, bias)
    hi, lo, _ = R.case_expected(case, srcs, bias)
    nzb, kk = case.rows_pad // case.cb, case.k * case.k
    assert hi.size == lo.size == case.rows_pad * case.chunks * kk * 16
    hi, lo = (torch.from_numpy(t).view(nzb, case.chunks, kk, case.cb, 2, 8) for t in (hi, lo))
    w = torch.from_numpy(wp).view(nzb, case.cb, case.chunks, 2, 8, kk)      # [zb][row][chunk][half][8][tap]
    for row in (0, 7, 8, 15, 24):
        s = (row >> 3) & 1
        for slot in range(2):
            want = w[:, row, :, slot ^ s].permute(0, 1, 3, 2)               # [zb][chunk][tap][8]
            assert torch.equal(hi[:, :, :, row, slot], want.half())
            assert torch.equal(lo[:, :, :, row, slot], (want - want.half().float()).half())
    assert float(hi.float().abs().max()) > 0 and float(lo.float().abs().max()) > 0
    tiny = lo.float().abs()
    assert bool(((tiny > 0) & (tiny < 2.0 ** -14)).any())                   # the cases do reach fp16 subnormals in lo


# ---------------------------------------------------------------------------------------------------- return codes
E_ARG, E_SHAPE = -1, -2
NULL, ONE = C.c_void_p(0), C.c_void_p(16)              # ONE: any non-null value; validation must fail before it is touched


@pytest.fixture(scope="module")
def lib():
    from bin_amd import _lib as L
    return L.lib()


def _fwd(lib, w=ONE, cout=32, cin=32, k=3, cout_pad=32, chunks=2, cb=32, shuffle=0, w_hi=ONE, bias_out=ONE):
    return lib.binhip_weights_relayout(w, NULL, cout, cin, k, cout_pad, chunks, cb, shuffle, w_hi, NULL, bias_out, NULL)


def _dgrad(lib, w=ONE, cout=32, cin=96, k=3, rows_pad=96, chunks=2, cb=96, shuffle=0, w_hi=ONE, bias_out=ONE):
    return lib.binhip_weights_relayout_dgrad(w, cout, cin, k, rows_pad, chunks, cb, shuffle, w_hi, NULL, bias_out, NULL)


def _gather(lib, srcs=(16, 16, 16, 16), group=0, cb=None, w_hi=ONE, bias_out=ONE):
    arr = (C.c_void_p * 4)(*srcs) if srcs is not None else None
    cb = (96 if group == 0 else 32) if cb is None else cb
    return lib.binhip_weights_relayout_rdb_gather(arr, group, cb, w_hi, NULL, bias_out, NULL)


def _item(kind, w=(16,), w_hi=16, bias_out=16, cout=32, cin=32, k=3, rows_pad=32, chunks=2, cb=32, sg=0, shape=(0, 0, 0, 0)):
    from bin_amd import _lib as L
    it = L.BinRelayoutItem()
    for i, p in enumerate(w):
        it.w[i] = p
    it.w_hi, it.bias_out = w_hi, bias_out
    it.kind, it.cout, it.cin, it.ksize, it.rows_pad, it.cin_chunks, it.cout_block, it.shuffle_or_group = \
        kind, cout, cin, k, rows_pad, chunks, cb, sg
    it.shape.G0, it.shape.D, it.shape.C, it.shape.G = shape
    return it


def _batch(lib, *items):
    from bin_amd import _lib as L
    return lib.binhip_weights_relayout_batch((L.BinRelayoutItem * len(items))(*items), len(items), NULL)


def _gitem(g=0, w=(16,) * 4, rows_pad=None, chunks=None, cb=None, shape=(0, 0, 0, 0), **kw):
    G0, Cn, G = (shape[0] if shape[0] > 0 else 96), (shape[2] if shape[2] > 0 else 4), (shape[3] if shape[3] > 0 else 32)
    rows = G0 if g == 0 else G
    return _item(R.GATHER, w=w, k=kw.pop("k", 3), rows_pad=rows if rows_pad is None else rows_pad,
                 chunks=(Cn - g) * G // 16 if chunks is None else chunks, cb=rows if cb is None else cb, sg=g, shape=shape, **kw)


def test_forward_entry_return_codes(lib):
    assert _fwd(lib, w=NULL) == E_ARG and _fwd(lib, w_hi=NULL) == E_ARG and _fwd(lib, bias_out=NULL) == E_ARG
    assert _fwd(lib, w_hi=NULL, cout_pad=48) == E_ARG                       # pointers before shapes
    assert _fwd(lib, cout_pad=48, cb=16) == E_SHAPE                         # cout_pad % 32
    assert _fwd(lib, cb=0) == E_SHAPE and _fwd(lib, cb=-32) == E_SHAPE      # cout_block <= 0
    assert _fwd(lib, cout=64, cout_pad=64, cb=96) == E_SHAPE                # cout_pad % cout_block
    assert _fwd(lib, cb=16) == E_SHAPE                                      # cout_block % 32
    assert _fwd(lib, cin=33) == E_SHAPE                                     # cin > 16 cin_chunks
    assert _fwd(lib, cout=40) == E_SHAPE                                    # cout > cout_pad
    assert _fwd(lib, cout=28, shuffle=1) == E_SHAPE                         # shuffle: cout != cout_pad
    assert _fwd(lib, cout=30, shuffle=1) == E_SHAPE                         # shuffle: cout % 4


def test_dgrad_entry_return_codes(lib):
    assert _dgrad(lib, w=NULL) == E_ARG and _dgrad(lib, w_hi=NULL) == E_ARG and _dgrad(lib, bias_out=NULL) == E_ARG
    assert _dgrad(lib, bias_out=NULL, rows_pad=80) == E_ARG
    assert _dgrad(lib, rows_pad=80, cb=16) == E_SHAPE                       # rows_pad % 32
    assert _dgrad(lib, cb=0) == E_SHAPE and _dgrad(lib, cb=-96) == E_SHAPE
    assert _dgrad(lib, cb=64) == E_SHAPE                                    # rows_pad % cout_block
    assert _dgrad(lib, cb=48) == E_SHAPE                                    # cout_block % 32
    assert _dgrad(lib, cin=97) == E_SHAPE                                   # cin > rows_pad
    assert _dgrad(lib, cout=33) == E_SHAPE                                  # cout > 16 cin_chunks
    assert _dgrad(lib, cout=30, shuffle=1) == E_SHAPE                       # shuffle: cout % 4


def test_gather_entry_return_codes(lib):
    assert _gather(lib, srcs=None) == E_ARG
    assert _gather(lib, w_hi=NULL) == E_ARG and _gather(lib, bias_out=NULL) == E_ARG
    assert _gather(lib, group=-1) == E_ARG and _gather(lib, group=4) == E_ARG
    assert _gather(lib, group=7, cb=40) == E_ARG                            # the group is decided before the shapes
    assert _gather(lib, group=0, cb=0) == E_SHAPE and _gather(lib, group=0, cb=64) == E_SHAPE      # 96 % 64
    assert _gather(lib, group=1, cb=64) == E_SHAPE and _gather(lib, group=2, cb=16) == E_SHAPE
    assert _gather(lib, srcs=(16, 16, 0, 16), group=2) == E_ARG             # a source this group reads
    assert _gather(lib, srcs=(16, 16, 16, 0), group=0) == E_ARG
    assert _gather(lib, srcs=(0, 0, 0, 0), group=1, cb=40) == E_SHAPE       # ... is looked at after the shapes


def test_batch_entry_return_codes(lib):
    from bin_amd import _lib as L
    ok = _item(R.FWD)
    assert lib.binhip_weights_relayout_batch(None, 1, NULL) == E_ARG
    assert lib.binhip_weights_relayout_batch(C.byref(ok), 0, NULL) == E_ARG
    assert lib.binhip_weights_relayout_batch(C.byref(ok), -3, NULL) == E_ARG
    for kind in (R.FWD, R.DGRAD, R.GATHER):
        assert _batch(lib, _item(kind, w=(0,))) == E_ARG
        assert _batch(lib, _item(kind, w_hi=0)) == E_ARG and _batch(lib, _item(kind, bias_out=0)) == E_ARG
        assert _batch(lib, _item(kind, w_hi=0, rows_pad=48)) == E_ARG       # pointers before shapes
    assert _batch(lib, _item(3)) == E_ARG and _batch(lib, _item(-1)) == E_ARG
    assert _batch(lib, _item(3, rows_pad=48)) == E_ARG
    assert _batch(lib, ok, _item(R.FWD, rows_pad=48)) == E_SHAPE            # every item is validated before the first launch
    # FWD
    f = lambda **kw: _batch(lib, _item(R.FWD, **kw))
    assert f(rows_pad=48, cb=16) == E_SHAPE and f(cb=0) == E_SHAPE and f(cb=-32) == E_SHAPE
    assert f(cout=64, rows_pad=64, cb=96) == E_SHAPE and f(cb=16) == E_SHAPE
    assert f(cin=33) == E_SHAPE and f(cout=40) == E_SHAPE
    assert f(cout=28, sg=1) == E_SHAPE and f(cout=30, sg=1) == E_SHAPE
    # DGRAD
    d = lambda **kw: _batch(lib, _item(R.DGRAD, **dict(dict(cout=32, cin=96, rows_pad=96, cb=96), **kw)))
    assert d(rows_pad=80, cb=16) == E_SHAPE and d(cb=0) == E_SHAPE and d(cb=-96) == E_SHAPE
    assert d(cb=64) == E_SHAPE and d(cb=48) == E_SHAPE
    assert d(cin=97) == E_SHAPE and d(cout=33) == E_SHAPE and d(cout=30, sg=1) == E_SHAPE
    # RDB_GATHER: the block first, then the group, then the item's geometry, then the sources
    g = lambda *a, **kw: _batch(lib, _gitem(*a, **kw))
    assert g(shape=(96, 0, 8, 32), w=(16,) * 8) == E_SHAPE                  # C > BINHIP_RDN_MAX_CONVS
    assert g(shape=(48, 0, 4, 32)) == E_SHAPE and g(shape=(96, 0, 4, 16)) == E_SHAPE
    assert g(9, shape=(48, 0, 4, 32)) == E_SHAPE                            # the block before the group
    assert g(-1) == E_ARG and g(4) == E_ARG and g(3, shape=(64, 0, 3, 64), w=(16,) * 3) == E_ARG
    assert g(4, rows_pad=64) == E_ARG                                       # the group before the geometry
    assert g(0, rows_pad=32) == E_SHAPE and g(1, rows_pad=96, cb=32) == E_SHAPE
    assert g(1, chunks=8) == E_SHAPE and g(0, k=1) == E_SHAPE
    assert g(0, cb=0) == E_SHAPE and g(0, cb=64) == E_SHAPE and g(1, cb=16, rows_pad=32) == E_SHAPE
    assert g(2, w=(16, 16, 0, 16)) == E_ARG and g(0, w=(16, 16, 16, 0)) == E_ARG
    assert g(1, w=(16, 0, 0, 0), cb=64) == E_SHAPE                          # the sources after the geometry
    assert g(1, w=(0, 16, 16, 16)) == E_ARG                                 # an item names w[0] whatever its group
    # each zero of `shape` takes bin_stage4's value on its own: (64, -, 0, 0) is a (64, 4, 32) block
    assert g(0, shape=(64, 0, 0, 0), rows_pad=96, cb=96) == E_SHAPE and g(4, shape=(64, 0, 0, 0)) == E_ARG
    assert g(2, shape=(0, 0, 2, 0), w=(16, 16)) == E_ARG                    # (96, -, 2, 32): groups 0 and 1 only
    assert L.RDN_MAX_CONVS == 7
