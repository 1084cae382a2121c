"""GPU: the held form of the fp32-class 3x3 kernels (BINHIP_CONV_HOLD_WEIGHTS, BINHIP_TAIL_HOLD_WEIGHTS, BINHIP_PLAN_HOLD_WEIGHTS: a
chunk's hi-plane weight fragments stay in registers from its hi to its lo sub-stage) against the reloading form and against float64.

Through the per-op entry points (binhip_conv2d_fwd, binhip_rdb_tail_fwd), at the smallest shapes where holding can go wrong: one chunk
(no neighbour), two (both weight buffers), seven (an odd count: the buffer parity at the last chunk), one pixel, ragged tiles in both
directions, a batch, the dense-block layers with ReLU, a 96-row layer (three workgroup columns).  The two forms must store the same
bits in both planes, and EACH must meet the float64 convolution of the stored operands to the bar tests/test_gpu_conv.py holds the
fp32-class path to (identity of two wrong kernels does not pass).  Last, nothing may depend on what the output planes or the plan's
workspace held before the call."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from poison import BYTES

pytestmark = pytest.mark.gpu

TOL = 2e-5                   # tests/test_gpu_conv.py TOL_OPS[3]: max-abs error over the reference's max-abs, fp32-class mode
E_ARG = -1                   # BINHIP_E_ARG
NAN16 = 0x7E00               # an fp16 NaN; the poison bytes 0x47 / 0xFF give 7.28 and another NaN

# name: (N, h, w, cin, cout, relu)
CONV_CASES = {
    "a_one_chunk": (1, 5, 7, 16, 32, False),
    "b_two_chunks": (1, 5, 7, 32, 32, False),
    "c_seven_chunks": (1, 5, 7, 112, 32, False),
    "d_one_pixel": (1, 1, 1, 96, 32, True),
    "e_ragged_17x33": (1, 17, 33, 96, 32, False),
    "f_batch_2": (2, 17, 33, 48, 32, False),
    "g_dense_96": (1, 17, 33, 96, 32, True),
    "g_dense_128": (1, 17, 33, 128, 32, True),
    "g_dense_160": (1, 17, 33, 160, 32, True),
    "wide_96_rows": (1, 17, 33, 96, 96, False),
}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _fill16(t, word):
    t.view(torch.int16).fill_(word - 0x10000 if word >= 0x8000 else word)


def _conv(x, cw, relu, hold, fill=NAN16):
    """binhip_conv2d_fwd (3x3, planes, nterms 3) into planes filled with the 16-bit word `fill`; returns the CP on the device."""
    from bin_amd import _lib as L, ops
    _, n, h, w, _ = x.hi.shape
    y = ops.CP.empty(ops.chunks(cw.cout), n, h, w, 3, x.hi.device, cw.cout)
    _fill16(y.hi, fill)
    _fill16(y.lo, fill)
    d = L.BinConvDesc(N=n, H=h, W=w, ksize=3, cin_chunks=cw.cin_chunks, cout=cw.cout, cout_pad=cw.cout_pad, nterms=3, epilogue=L.EPI_PLANES,
                      relu=int(relu), x_cpg=0, x_group_stride=0, n_images=0, reserved=L.CONV_HOLD_WEIGHTS if hold else 0,
                      status=ops.status_word(y.hi.device).data_ptr())
    rc = L.lib().binhip_conv2d_fwd(C.byref(d), _p(x.hi), _p(x.lo), _p(cw.w_hi), _p(cw.w_lo), _p(cw.bias), None, None, _p(y.hi), _p(y.lo),
                                   None, None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    ops.check_status()
    return y


def _conv_case(key):
    from bin_amd import ops
    n, h, w, cin, cout, relu = CONV_CASES[key]
    gen = torch.Generator().manual_seed(1000 * h + 10 * w + cin + cout)
    x = torch.randn(n, cin, h, w, generator=gen)
    wt = torch.randn(cout, cin, 3, 3, generator=gen) / (cin * 9) ** 0.5
    b = torch.randn(cout, generator=gen)
    xp = ops.nchw_to_planes(x.cuda(), 3)
    # the operand the kernels see is the stored pair hi + lo (|x - (hi + lo)| <= 2^-23 |x|: far below the bar either way)
    ref = F.conv2d(ops.planes_to_nchw(xp, cin).double().cpu(), wt.double(), b.double(), padding=1)
    return xp, ops.ConvWeights(wt.cuda(), b.cuda(), nterms=3), relu, (ref.relu() if relu else ref)


@pytest.mark.parametrize("key", sorted(CONV_CASES))
def test_held_conv_stores_the_reloading_forms_bits_and_both_meet_float64(key):
    from bin_amd import ops
    xp, cw, relu, ref = _conv_case(key)
    old, new = _conv(xp, cw, relu, False), _conv(xp, cw, relu, True)
    e_old = _rel(ops.planes_to_nchw(old, cw.cout).double().cpu(), ref)
    e_new = _rel(ops.planes_to_nchw(new, cw.cout).double().cpu(), ref)
    print(f"{key}: vs float64: reloading {e_old:.3e}, held {e_new:.3e} (bar {TOL:.0e})")
    assert e_old <= TOL and e_new <= TOL
    assert torch.equal(new.hi.view(torch.int16), old.hi.view(torch.int16))
    assert torch.equal(new.lo.view(torch.int16), old.lo.view(torch.int16))


# ------------------------------------------------------------------------------------------------ the fused dense-block tail
_tail_operands = {}


def _tail_case(h, w):
    """Block buffer (192 input channels + room for o3), conv #3 and LFF weights, and the float64 o3 / y of the stored operands."""
    from bin_amd import ops
    if (h, w) not in _tail_operands:
        gen = torch.Generator().manual_seed(77 + h + w)
        x = torch.randn(1, 192, h, w, generator=gen)
        w3 = torch.randn(32, 192, 3, 3, generator=gen) / (192 * 9) ** 0.5
        b3 = torch.randn(32, generator=gen)
        wl = torch.randn(96, 224, 1, 1, generator=gen) / 224 ** 0.5
        bl = torch.randn(96, generator=gen)
        xin = ops.nchw_to_planes(x.cuda(), 3)
        xs = ops.planes_to_nchw(xin, 192).double().cpu()
        o3 = (F.conv2d(xs, w3.double(), b3.double(), padding=1)).relu()
        y = F.conv2d(torch.cat([xs, o3], 1), wl.double(), bl.double()) + xs[:, :96]
        _tail_operands[(h, w)] = (xin, ops.ConvWeights(w3.cuda(), b3.cuda(), nterms=3), ops.ConvWeights(wl.cuda(), bl.cuda(), nterms=3), o3, y)
    return _tail_operands[(h, w)]


def _tail(xin, cw3, cwl, store_o3, hold, fill=NAN16):
    """binhip_rdb_tail_fwd on a fresh 14-chunk block buffer whose o3 planes and whose output hold `fill`; returns (y, o3) CPs."""
    from bin_amd import _lib as L, ops
    _, n, h, w, _ = xin.hi.shape
    dev = xin.hi.device
    blk, y = ops.CP.empty(14, n, h, w, 3, dev, 224), ops.CP.empty(6, n, h, w, 3, dev, 96)
    for t in (blk.hi, blk.lo, y.hi, y.lo):
        _fill16(t, fill)
    blk.hi[:12].copy_(xin.hi)
    blk.lo[:12].copy_(xin.lo)
    flags = (L.TAIL_STORE_O3 if store_o3 else 0) | (L.TAIL_HOLD_WEIGHTS if hold else 0)
    rc = L.lib().binhip_rdb_tail_fwd(n, h, w, 3, _p(blk.hi), _p(blk.lo), _p(cw3.w_hi), _p(cw3.w_lo), _p(cw3.bias), _p(cwl.w_hi), _p(cwl.w_lo),
                                     _p(cwl.bias), _p(y.hi), _p(y.lo), flags, _p(ops.status_word(dev)),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    ops.check_status()
    return y, blk.sub(12, 2)


@pytest.mark.parametrize("store_o3", [False, True], ids=["inference", "keep_acts"])
@pytest.mark.parametrize("h,w", [(17, 33), (16, 32)])
def test_held_tail_stores_the_reloading_forms_bits_and_both_meet_float64(h, w, store_o3):
    from bin_amd import ops
    xin, cw3, cwl, ref_o3, ref_y = _tail_case(h, w)
    (y_old, o_old), (y_new, o_new) = _tail(xin, cw3, cwl, store_o3, False), _tail(xin, cw3, cwl, store_o3, True)
    e_old = _rel(ops.planes_to_nchw(y_old, 96).double().cpu(), ref_y)
    e_new = _rel(ops.planes_to_nchw(y_new, 96).double().cpu(), ref_y)
    print(f"tail {h} x {w} store_o3 {store_o3}: vs float64: reloading {e_old:.3e}, held {e_new:.3e} (bar {TOL:.0e})")
    assert e_old <= TOL and e_new <= TOL
    for a, b in ((y_new, y_old), (o_new, o_old)):          # (without store_o3 the o3 planes keep their fill in both forms)
        assert torch.equal(a.hi.view(torch.int16), b.hi.view(torch.int16))
        assert torch.equal(a.lo.view(torch.int16), b.lo.view(torch.int16))
    if store_o3:
        assert _rel(ops.planes_to_nchw(o_new, 32).double().cpu(), ref_o3) <= TOL
    else:
        assert bool(torch.isnan(o_new.hi).all())


# ------------------------------------------------------------------------------------------------ what the buffers held before
def test_held_results_do_not_depend_on_what_the_outputs_held():
    """17 x 33, per-op calls: the output planes (and the o3 planes of the block buffer) hold NaN or a poison byte before the call."""
    xp, cw, relu, _ = _conv_case("g_dense_160")
    xin, cw3, cwl, _, _ = _tail_case(17, 33)
    base_c = _conv(xp, cw, relu, True)
    base_t = _tail(xin, cw3, cwl, True, True)
    for byte in BYTES:
        word = byte * 0x0101
        c = _conv(xp, cw, relu, True, fill=word)
        assert torch.equal(c.hi.view(torch.int16), base_c.hi.view(torch.int16)) and torch.equal(c.lo.view(torch.int16), base_c.lo.view(torch.int16))
        t = _tail(xin, cw3, cwl, True, True, fill=word)
        for a, b in zip(t, base_t):
            assert torch.equal(a.hi.view(torch.int16), b.hi.view(torch.int16)) and torch.equal(a.lo.view(torch.int16), b.lo.view(torch.int16))


def test_held_plan_equals_the_reloading_plan_whatever_the_workspace_held(canon_gpu):
    """A whole RDN call at half resolution 17 x 33 with BINHIP_PLAN_HOLD_WEIGHTS: NaN in the output, each poison byte in the
    workspace; the same bits every time, and the bits of the plan without the flag."""
    from bin_amd import _lib as L, ops
    from bin_amd.rdn_plan import RdnWeights, rdn_forward
    k, n, H, W = 3, 1, 34, 66
    wts = RdnWeights(canon_gpu, k, 3, prefix="model2.")
    gen = torch.Generator().manual_seed(5)
    ins = [torch.rand(n, 3, H, W, generator=gen).cuda() for _ in range(k)]
    ws = torch.zeros(L.lib().binhip_rdn_workspace_bytes(n, H, W, k, 3, None), dtype=torch.uint8, device="cuda")
    base = L.PLAN_FUSED_UPNET | L.PLAN_UPNET_FOLD

    def run(flags, byte):
        ws.fill_(byte)
        out = torch.full((n, 3, H, W), float("nan"), device="cuda")
        rdn_forward(wts, ins, out=out, ws=ws, flags=flags)
        ops.check_status()
        return out.cpu()
    ref = run(base, 0)
    assert bool(torch.isfinite(ref).all())
    for byte in BYTES:
        assert torch.equal(run(base | L.PLAN_HOLD_WEIGHTS, byte), ref)
    # the per-conv launches of fp32-class inference are the only ones with the form: the Python side drops the flag elsewhere
    assert torch.equal(run(base | L.PLAN_HOLD_WEIGHTS | L.PLAN_RDB3, 0x47), ref)


def test_hold_bits_are_refused_where_the_form_does_not_exist():
    from bin_amd import _lib as L, ops
    lib = L.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = ops.nchw_to_planes(torch.rand(1, 16, 8, 32).cuda(), 3)
    y = ops.CP.empty(2, 1, 8, 32, 3, x.hi.device)
    w5 = ops.ConvWeights(torch.rand(32, 16, 5, 5).cuda() * 0.1, torch.zeros(32).cuda(), nterms=3)
    w1 = ops.ConvWeights(torch.rand(32, 16, 3, 3).cuda() * 0.1, torch.zeros(32).cuda(), nterms=1)

    def fwd(ks, nt, cw):
        d = L.BinConvDesc(N=1, H=8, W=32, ksize=ks, cin_chunks=1, cout=32, cout_pad=32, nterms=nt, epilogue=L.EPI_PLANES, relu=0,
                          x_cpg=0, x_group_stride=0, n_images=0, reserved=L.CONV_HOLD_WEIGHTS, status=None)
        return lib.binhip_conv2d_fwd(C.byref(d), _p(x.hi), _p(x.lo) if nt == 3 else None, _p(cw.w_hi), _p(cw.w_lo), _p(cw.bias), None, None,
                                     _p(y.hi), _p(y.lo) if nt == 3 else None, None, None, s)
    assert fwd(5, 3, w5) == E_ARG and fwd(3, 1, w1) == E_ARG
    xin, cw3, cwl, _, _ = _tail_case(16, 32)
    blk, out = ops.CP.empty(14, 1, 16, 32, 3, x.hi.device), ops.CP.empty(6, 1, 16, 32, 3, x.hi.device)

    def tail(nt, flags):
        return lib.binhip_rdb_tail_fwd(1, 16, 32, nt, _p(blk.hi), _p(blk.lo), _p(cw3.w_hi), _p(cw3.w_lo), _p(cw3.bias), _p(cwl.w_hi), _p(cwl.w_lo),
                                       _p(cwl.bias), _p(out.hi), _p(out.lo), flags, None, s)
    assert tail(1, L.TAIL_HOLD_WEIGHTS) == E_ARG and tail(3, 4) == E_ARG
    torch.cuda.synchronize()
