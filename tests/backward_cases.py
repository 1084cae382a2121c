"""Case table and helpers of tests/test_gpu_backward_shapes.py (the backward at ragged shapes, batches and border-ring edges), and the
op-by-op dense-block forward / gather-form backward shared with tests/test_gpu_conv.py; the saved ReLU masks and the float64 reference
with its tie rule are shared with tests/test_gpu_rdn_configs.py (any (G0, D, C, G)).

Frames are (N, H, W) at full resolution; the network runs at half resolution h = H / 2, w = W / 2.  The fused UPNet's ring kernels
(binhip_upnet_bwd.hip: upnet_ring_dgrad_kernel's band of rows {0, 1, 2, h-3, h-2, h-1} with its h <= 6 / w <= 6 branches,
upnet_ring_wgrad_kernel's twelve (variant, sub-pixel) pairs and per-image partials) are only reached in full at half-resolution sizes
below 7, odd, and with N > 1 — what the aligned shapes of the older tests never are."""
import torch
import torch.nn.functional as F

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


# A ReLU whose float64 pre-activation lies within rounding of zero is a tie that any fp32-class computation (plain float32 torch
# autograd of the oracle included) may decide either way; at ~1e6 ReLU units per call (22 x 38 frames, N = 3) about one such unit
# is expected, and ONE flipped unit moves that conv's weight gradient by ~1 / sqrt(pixels) (measured 3e-3 .. 5e-2).  So the float64
# reference takes the kernels' own mask at a tie, |z| <= TIE * max|z| of the layer, and everywhere else asserts that the kernels'
# masks ARE float64's: a mask read from the wrong pixel, channel or image still fails.
TIE = 1e-5


def saved_relu_masks(ws, dims, shape):
    """The ReLU masks the backward reads (saved post-ReLU hi plane > 0) of every dense-block conv of one training forward of an RDN
    of `shape` = (G0, D, C, G): [D * C] bool tensors [N, G, h, w] in call order, from the saved workspace
    (binhip_rdn_workspace_layout).  `dims`: the (N, H, W, frames, nterms) the module's debug hook receives."""
    from bin_amd import _lib as L
    from bin_amd.range_stats import _layout, _view
    n, H, W = dims[:3]
    v = _layout(L.lib().binhip_rdn_workspace_layout, dims, L.RDN_LAYOUT_WORDS, shape)
    G0, D, Cc, G = shape
    c0, cg, cb = G0 // 16, G // 16, (G0 + Cc * G) // 16
    P, blk = v[0], v[7]
    masks = []
    for d in range(D):
        for c in range(Cc):
            hi = _view(ws, blk + (d * cb + c0 + cg * c) * P, cg * P).view(cg, n, H // 2, W // 2, 16)
            masks.append((hi.permute(1, 0, 4, 2, 3).reshape(n, cg * 16, H // 2, W // 2) > 0).cpu())
    return masks


def oracle_rdn_grads(W, set_name, leaves, frames, gouts, masks):
    """float64 autograd of oracle.rdn with every dense-block ReLU decided by TIE: `W` {full name: float64 tensor} (the ones to
    differentiate require grad), `leaves` {result name: tensor of W or of `frames`} to differentiate, `frames` float64 tensors that
    require grad, `masks` the kernels' ReLU masks in call order (saved_relu_masks).  Returns ([{name: gradient} per upstream gradient
    in `gouts`], ReLU ties, ties decided otherwise than float64 by the kernels)."""
    from oracle import rdn_oracle as O
    it = iter(masks)
    ties = [0, 0]

    def rdb_conv(x, w, b):                       # oracle.rdb_conv with the mask decided as above
        z = F.conv2d(x, w, b, padding=1)
        zd, mk = z.detach(), next(it)
        own = zd > 0
        tie = zd.abs() <= TIE * zd.abs().max()
        off = int(((mk != own) & ~tie).sum())
        assert off == 0, f"the kernels' ReLU mask differs from float64's at {off} units that are not ties"
        ties[0] += int(tie.sum())
        ties[1] += int((mk != own).sum())
        return torch.cat((x, z * torch.where(tie, mk, own).to(z.dtype)), 1)
    orig = O.rdb_conv
    O.rdb_conv = rdb_conv
    try:
        out = O.rdn(frames, W, set_name)
    finally:
        O.rdb_conv = orig
    assert next(it, None) is None
    names = list(leaves)
    res = []
    for i, g in enumerate(gouts):
        gr = torch.autograd.grad(out, [leaves[n] for n in names], g.double(), retain_graph=i + 1 < len(gouts))
        res.append(dict(zip(names, gr)))
    return res, ties[0], ties[1]


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
