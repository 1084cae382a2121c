"""GPU: the folded main launch of the fused UPNet (BINHIP_PLAN_UPNET_FOLD) against the 5x5 main launch and against the float64
two-layer UPNet.  Whole RDN calls at tiny frames; the oracle is UPNet's two layers (RDN.py:203-207, 221) in float64 on the features the
call itself left in its workspace (G1, hi + lo planes), so what is compared is the UPNet alone.  The algebra of the fold is pinned on the
CPU (tests/test_cpu_upnet_fold.py)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (input frames, N, half-resolution h, w): everything is ring; 2 x 2 (4 interior blocks); a tile edge in both directions with an odd
# height (the row pair's second row leaves the image); exactly one 16 x 32 tile; a batch
CASES = [(2, 1, 1, 1), (3, 1, 2, 2), (5, 1, 17, 33), (2, 1, 16, 32), (3, 2, 17, 33)]
PREFIX = {2: "model1.", 3: "model2.", 5: "model3."}
_weights = {}


def _rdn_weights(k, canon_gpu):
    from bin_amd.rdn_plan import RdnWeights
    if k not in _weights:
        _weights[k] = RdnWeights(canon_gpu, k, 3, prefix=PREFIX[k])
    return _weights[k]


def _g1(ws, dims):
    """G1 = GFF.1 + F1, the UPNet's input, out of a forward call's workspace: float64 [N, 96, h, w] (hi + lo)."""
    from bin_amd import _lib as L
    from bin_amd.range_stats import _layout, _view
    n, H, W = dims[:3]
    v = _layout(L.lib().binhip_rdn_workspace_layout, dims, L.RDN_LAYOUT_WORDS)
    off, size = v[11], v[12]
    planes = _view(ws, off, size).double() + _view(ws, off + size, size).double()
    return planes.view(6, n, H // 2, W // 2, 16).permute(1, 0, 4, 2, 3).reshape(n, 96, H // 2, W // 2)


@pytest.mark.parametrize("k,n,h,w", CASES)
def test_folded_upnet_equals_the_5x5_launch_and_the_float64_two_layer_form(k, n, h, w, canon_gpu):
    from bin_amd import _lib as L, ops
    from bin_amd.rdn_plan import rdn_forward
    wts = _rdn_weights(k, canon_gpu)
    H, W = 2 * h, 2 * w
    gen = torch.Generator().manual_seed(11 + k + 7 * h + w)
    ins = [torch.rand(n, 3, H, W, generator=gen).cuda() for _ in range(k)]
    nbytes = L.lib().binhip_rdn_workspace_bytes(n, H, W, k, 3, None)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    ops.check_status()
    outs = {}
    for name, flags in (("off", L.PLAN_FUSED_UPNET), ("on", L.PLAN_FUSED_UPNET | L.PLAN_UPNET_FOLD)):
        out = torch.full((n, 3, H, W), float("nan"), device="cuda")          # a pixel nobody stores stays NaN
        rdn_forward(wts, ins, out=out, ws=ws, flags=flags)
        ops.check_status()                                                      # the status word is clean
        outs[name] = out.cpu()
    assert wts.fused_fold is not None
    x = _g1(ws, (n, H, W, k, 3)).cpu()
    w0, b0 = canon_gpu[f"{PREFIX[k]}UPNet.0.weight"].double().cpu(), canon_gpu[f"{PREFIX[k]}UPNet.0.bias"].double().cpu()
    w2, b2 = canon_gpu[f"{PREFIX[k]}UPNet.2.weight"].double().cpu(), canon_gpu[f"{PREFIX[k]}UPNet.2.bias"].double().cpu()
    ref = F.conv2d(F.pixel_shuffle(F.conv2d(x, w0, b0, padding=1), 2), w2, b2, padding=1)
    ref = ref + sum(t.double().cpu() for t in ins) / k
    on, off = outs["on"], outs["off"]
    assert bool(torch.isfinite(on).all()) and bool(torch.isfinite(off).all())
    ring = torch.ones(n, 3, H, W, dtype=torch.bool)
    ring[..., 1:-1, 1:-1] = False
    assert torch.equal(on[ring], off[ring])                                     # the ring launch and its operands did not change
    e_off, e_on = float((off.double() - ref).abs().max()), float((on.double() - ref).abs().max())
    d = float((on - off).abs().max())
    scale = max(1.0, float(ref.abs().max()))
    print(f"k {k} n {n} {h} x {w}: vs float64 two-layer: 5x5 {e_off:.3e}, folded {e_on:.3e}; folded vs 5x5 {d:.3e}; |out| {scale:.2f}")
    # the 5x5 launch's own error, times 1.5 for fp32 summation-order noise; inside the bar the fused form already has to meet
    bar = 1.5 * e_off
    assert bar <= 2e-6 * scale
    assert e_on <= bar
    # more than the bar asks: per channel the folded walk meets the operator's non-zero taps in the order the 5x5 walk does (column-major,
    # low-precision weight plane first), and the taps it skips added exact zeros — the same fp32 sums, bit for bit
    assert torch.equal(on, off)


def test_folded_main_launch_alone_stores_everything_but_the_ring(canon_gpu):
    """The main launch by itself (binhip_conv2d_fwd, BINHIP_CONV_UPNET_FOLD) into a NaN-filled output, next to the 5x5 launch on the
    same planes: the folded kernel is the one that ran (the border ring, which the 5x5 launch writes, stays NaN: nothing is stored
    on the last row / column the ring launch owns, nor on the first), and every other pixel is stored and equals the 5x5 launch's."""
    import ctypes as C
    from bin_amd import _lib as L, ops
    k, n, h, w = 3, 2, 17, 33
    wts = _rdn_weights(k, canon_gpu)
    main = wts.ensure_fused_upnet()[0]
    gen = torch.Generator().manual_seed(3)
    x = ops.nchw_to_planes(torch.randn(n, 96, h, w, generator=gen).cuda(), 3)
    ims = [torch.rand(n, 3, 2 * h, 2 * w, generator=gen).cuda() for _ in range(k)]
    arr = (C.c_void_p * k)(*[im.data_ptr() for im in ims])
    p = lambda t: C.c_void_p(t.data_ptr())
    ops.check_status()

    def launch(w_hi, w_lo, reserved):
        y = torch.full((n, 3, 2 * h, 2 * w), float("nan"), device="cuda")
        d = L.BinConvDesc(N=n, H=h, W=w, ksize=5, cin_chunks=6, cout=12, cout_pad=32, nterms=3, epilogue=L.EPI_FINAL_SUBPIX, relu=0,
                          x_cpg=0, x_group_stride=0, n_images=k, reserved=reserved, status=ops.status_word(y.device).data_ptr())
        rc = L.lib().binhip_conv2d_fwd(C.byref(d), p(x.hi), p(x.lo), p(w_hi), p(w_lo), p(main.bias), None, None, None, None, p(y), arr,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        ops.check_status()
        return y.cpu()
    plain = launch(main.w_hi, main.w_lo, 0)
    folded = launch(*wts.fused_fold, L.CONV_UPNET_FOLD)
    ring = torch.ones(n, 3, 2 * h, 2 * w, dtype=torch.bool)
    ring[..., 1:-1, 1:-1] = False
    assert bool(torch.isfinite(plain).all())
    assert bool(torch.isnan(folded[ring]).all())
    assert torch.equal(folded[~ring], plain[~ring])
    # the bit is refused where the folded slab has no meaning
    d = L.BinConvDesc(N=n, H=h, W=w, ksize=5, cin_chunks=6, cout=12, cout_pad=32, nterms=1, epilogue=L.EPI_FINAL_SUBPIX, relu=0, x_cpg=0,
                      x_group_stride=0, n_images=k, reserved=L.CONV_UPNET_FOLD, status=None)
    y = torch.zeros(n, 3, 2 * h, 2 * w, device="cuda")
    assert L.lib().binhip_conv2d_fwd(C.byref(d), p(x.hi), None, p(main.w_hi), None, p(main.bias), None, None, None, None, p(y), arr,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)) < 0
    torch.cuda.synchronize()
