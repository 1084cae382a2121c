"""Case table and helpers of tests/test_gpu_backward_shapes.py (the backward at ragged shapes, batches and border-ring edges), and the
op-by-op dense-block forward / gather-form backward shared with tests/test_gpu_conv.py.

Frames are (N, H, W) at full resolution; the network runs at half resolution h = H / 2, w = W / 2.  The fused UPNet's ring kernels
(binhip_misc.hip: upnet_ring_dgrad_kernel's band of rows {0, 1, 2, h-3, h-2, h-1} with its h <= 6 / w <= 6 branches,
upnet_ring_wgrad_kernel's twelve (variant, sub-pixel) pairs and per-image partials) are only reached in full at half-resolution sizes
below 7, odd, and with N > 1 — what the aligned shapes of the older tests never are."""
import torch

SET_FOR_K = {2: "model1", 3: "model2", 5: "model3"}        # the weight set bin_stage4 uses for each class (RDN.py:342-363)

# whole-RDN backward vs float64 autograd of the oracle: tag -> (k, N, H, W, mode).  mode: "f16x3" (fp32-class, fused UPNet),
# "mixed" (f16x3 forward + single-product backward), "two_layer" (f16x3 with BIN_AMD_FUSED_UPNET_TRAIN=0)
RDN_CASES = {
    "k2_1x2x2": (2, 1, 2, 2, "f16x3"),            # half-res 1 x 1: every full-resolution pixel is ring
    "k2_1x2x14": (2, 1, 2, 14, "f16x3"),          # one half-resolution row
    "k2_2x12x14": (2, 2, 12, 14, "f16x3"),        # 6 x 7: the h <= 6 band, w = 7, N = 2
    "k2_1x14x12": (2, 1, 14, 12, "f16x3"),        # 7 x 6: one middle row, w <= 6
    "k2_3x22x38": (2, 3, 22, 38, "f16x3"),
    "k2_1x66x130": (2, 1, 66, 130, "f16x3"),      # 33 x 65
    "k3_1x2x2": (3, 1, 2, 2, "f16x3"),
    "k3_1x10x4": (3, 1, 10, 4, "f16x3"),
    "k3_2x12x14": (3, 2, 12, 14, "f16x3"),
    "k3_3x22x38": (3, 3, 22, 38, "f16x3"),
    "k3_2x36x70": (3, 2, 36, 70, "f16x3"),
    "k3_1x66x130": (3, 1, 66, 130, "f16x3"),
    "k5_1x2x14": (5, 1, 2, 14, "f16x3"),
    "k5_1x10x4": (5, 1, 10, 4, "f16x3"),
    "k5_1x14x12": (5, 1, 14, 12, "f16x3"),
    "k5_2x36x70": (5, 2, 36, 70, "f16x3"),
    "k5_1x66x130": (5, 1, 66, 130, "f16x3"),
    "k2_2x12x14_mixed": (2, 2, 12, 14, "mixed"),
    "k3_3x22x38_mixed": (3, 3, 22, 38, "mixed"),
    "k5_1x10x4_mixed": (5, 1, 10, 4, "mixed"),
    "k2_1x66x130_mixed": (2, 1, 66, 130, "mixed"),
    "k2_1x2x2_two_layer": (2, 1, 2, 2, "two_layer"),
    "k3_2x12x14_two_layer": (3, 2, 12, 14, "two_layer"),
    "k5_1x14x12_two_layer": (5, 1, 14, 12, "two_layer"),
    "k2_3x22x38_two_layer": (2, 3, 22, 38, "two_layer"),
}
RDN_BARS = {"f16x3": 3e-5, "mixed": 1e-2, "two_layer": 3e-5}

# the fused UPNet's ring at these half-resolution sizes (frames 2h x 2w, k = 2), with an upstream gradient restricted to the
# full-resolution border ring, to its four corners, or to everything but the ring
RING_HALF_SIZES = [(1, 1), (2, 3), (5, 2), (6, 7), (7, 6), (18, 35)]
RING_KINDS = ("ring", "corners", "interior")

# per-op backward at ragged tiles: (N, h, w) of the convolution
OP_SHAPES = [(1, 7, 5), (2, 33, 65), (3, 17, 31)]


def rel(a, b):
    """max-abs error / max|ref| of one tensor."""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-12))


def ring_mask(H, W):
    """bool [H, W]: the outermost full-resolution pixel ring."""
    m = torch.zeros(H, W, dtype=torch.bool)
    m[0, :] = m[-1, :] = True
    m[:, 0] = m[:, -1] = True
    return m


def corner_mask(H, W):
    m = torch.zeros(H, W, dtype=torch.bool)
    for y in (0, H - 1):
        for x in (0, W - 1):
            m[y, x] = True
    return m


def restrict(g, kind):
    """Upstream gradient `g` [N, 3, H, W] restricted to the ring, its corners or the interior (ring zeroed)."""
    H, W = g.shape[-2:]
    m = {"ring": ring_mask(H, W), "corners": corner_mask(H, W), "interior": ~ring_mask(H, W)}[kind]
    return g * m.to(g.dtype)


def rdb_block_fwd_bwd(x, gy, canon_gpu, nterms, pre="model1.RDBs.0."):
    """RDB(96, 32, 4) forward and backward through the per-op C ABI, as binhip_plan.hip's dense-block section issues it: three
    plane-concat convs + the fused tail, then LFF wgrad / dgrad and per conv its wgrad and the GATHER-form backward-data (every concat
    group written once).  x, gy: fp32 NCHW on the device.  Returns (y, gx, {param name: grad}) with the block's local names."""
    from bin_amd import ops
    n, _, h, w = x.shape
    W = [canon_gpu[f"{pre}convs.{c}.conv.0.weight"] for c in range(4)]
    Bc = [canon_gpu[f"{pre}convs.{c}.conv.0.bias"] for c in range(4)]
    WL, BL = canon_gpu[pre + "LFF.weight"], canon_gpu[pre + "LFF.bias"]
    cw = [ops.ConvWeights(W[c], Bc[c], nterms=nterms) for c in range(4)]
    cwl = ops.ConvWeights(WL, BL, nterms=nterms)
    # ---- forward (RDN.py:135-165): blk planes 0-5 = x, conv c writes planes 6+2c, 7+2c, the tail keeps o3 in 12, 13
    blk = ops.CP.empty(14, n, h, w, nterms, x.device)
    xin = ops.nchw_to_planes(x, nterms)
    blk.hi[0:6].copy_(xin.hi)
    if nterms == 3:
        blk.lo[0:6].copy_(xin.lo)
    for c in range(3):
        ops.conv2d(blk, cw[c], relu=True, out=blk.sub(6 + 2 * c, 2), cin_chunks=6 + 2 * c)
    y = ops.planes_to_nchw(ops.rdb_tail(blk, cw[3], cwl, store_o3=True), 96)
    # ---- backward (autograd of the same lines), gather form
    gyp = ops.nchw_to_planes(gy, nterms)
    grads = {}
    grads["LFF.weight"], grads["LFF.bias"] = ops.conv2d_bwd_weight(blk, gyp, 96, 224, 1, nterms)
    gcat = ops.conv2d_bwd_data(gyp, ops.DgradWeights(WL, nterms), res=gyp, res_chunks=6, mask=blk, mask_from=12)
    assert gcat.hi.shape[0] == 14
    gx = None
    for c in (3, 2, 1, 0):
        gyc = gcat.sub(6 + 2 * c, 2 * (4 - c))                     # stacked output gradients of convs c..3
        grads[f"convs.{c}.conv.0.weight"], grads[f"convs.{c}.conv.0.bias"] = ops.conv2d_bwd_weight(blk, gyc, 32, 96 + 32 * c, 3, nterms)
        gw = ops.RdbGatherWeights(W, c, nterms)
        if c > 0:
            slot = gcat.sub(4 + 2 * c, 2)                          # conv c-1's output slot: G_{c-1} = relu'(L_c + sum dgrads)
            ops.conv2d_bwd_data(gyc, gw, res=slot, mask=blk.sub(4 + 2 * c, 2), mask_from=0, out=slot)
        else:
            gx = ops.planes_to_nchw(ops.conv2d_bwd_data(gyc, gw, res=gcat.sub(0, 6)), 96)
    torch.cuda.synchronize()
    ops.check_status()
    return y, gx, grads
