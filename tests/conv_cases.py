"""Case table of the forward and backward-data convolution kernels (binhip_conv.hip, binhip_conv_x3.hip, binhip_fused.hip,
binhip_fused_x3.hip) for the bit pin of tests/test_gpu_conv.py: one case per row of bh_dispatch_conv that a call through the C ABI can
reach, at both precisions, plus the fused dense-block tail.  tests/golden/make_conv_bits.py records the sha256 of every output buffer
of every case into tests/golden/conv_bits.json; test_conv_bits_are_the_recorded_ones computes them again.

`rows` names, per nterms, the dispatcher row (kernel and template arguments) the case is in the table for.  Three rows of the nterms = 3
branch cannot be reached: bh_conv_cout_block() answers 32 for every fp32-class 3x3 convolution, so `e == S && cp == 256`, `cb == 64` and
`cb == 96` of that branch (launch_cfg<3,1,2,4,2,1,3,2,S>, <3,2,1,2,4,1,3,2,P>, <3,3,1,1,8,1,3,2,P>) never see a call; UNREACHABLE names them.

Shapes (N, H, W), the smallest at which a tile front end can go wrong: one pixel (every patch slot but one out of range); 17 x 33 (one
row past a 16-row tile and so three past an 8-row tile's second, one column past a 32-column tile); 2 x 18 x 44 (ragged both ways, a
second image).  The store through the inverse PixelShuffle needs even H and W (bh_prepare_conv refuses others): that one case runs at
the next even sizes, 2 x 2 and 18 x 34, which keep the same properties.

Operands are white noise from a seeded CPU generator, weights scaled by 1 / sqrt(fan in) so that outputs stay of order one.  Output
buffers are zero-filled before the call, so padding the kernels leave alone cannot change a digest.

white_noise_bits is two halves: white_noise_operands() draws the operands, call_library() makes the call on any operands of that
form.  tests/conv_ref_cases.py holds the same calls — on these operands and on two exact families — to float64.
"""
import hashlib
from collections import namedtuple

import torch

SHAPES = ((1, 1, 1), (1, 17, 33), (2, 18, 44))
EVEN_SHAPES = ((1, 2, 2), (1, 18, 34), (2, 18, 44))
NTERMS = (3, 1)

UNREACHABLE = ("nterms=3 e==S k==3 cp==256: launch_cfg<3,1,2,4,2,1,3,2,S>", "nterms=3 e==P k==3 cb==64: launch_cfg<3,2,1,2,4,1,3,2,P>",
               "nterms=3 e==P k==3 cb==96: launch_cfg<3,3,1,1,8,1,3,2,P>")

# kind: "fwd" binhip_conv2d_fwd, "bwd" binhip_conv2d_bwd_data (the weight is the FORWARD layer's OIHW tensor [cout][cin]: the call
# computes cin output channels from cout), "tail" binhip_rdb_tail_fwd
Case = namedtuple("Case", "tag kind ks cin cout opts rows")


def _c(tag, kind, ks, cin, cout, rows, **opts):
    return Case(tag, kind, ks, cin, cout, opts, rows)


CASES = (
    # ---- plane epilogue
    _c("p3_32", "fwd", 3, 96, 32, {1: "launch_cfg<3,1,1,2,8,1,1,2,P>", 3: "conv_x3_kernel<3,P,WIDE=0>"}, relu=True),
    _c("p3_64_res", "fwd", 3, 64, 64, {1: "launch_cfg<3,2,1,2,4,1,1,2,P> XTRA", 3: "conv_x3_kernel<3,P,WIDE=1> XTRA, 2 columns"},
       relu=True, res=True),
    _c("p3_96", "fwd", 3, 96, 96, {1: "launch_cfg<3,3,1,2,4,1,1,2,P>", 3: "conv_x3_kernel<3,P,WIDE=1>, 3 columns"}),
    _c("p3_256", "fwd", 3, 96, 256, {1: "launch_cfg<3,2,2,4,4,1,1,2,P>, 2 columns", 3: "conv_x3_kernel<3,P,WIDE=1>, 8 columns"}),
    _c("p3_grouped", "fwd", 3, 96, 32, {1: "launch_cfg<3,1,1,2,8,1,1,2,P>, x_cpg = 3", 3: "conv_x3_kernel<3,P,WIDE=0>, x_cpg = 3"},
       relu=True, x_cpg=3),
    _c("p1_32", "fwd", 1, 96, 32, {1: "launch_cfg<1,1,1,4,4,4,1,2,P>", 3: "launch_cfg<1,1,1,4,4,2,3,2,P>"}),
    _c("p1_96_lff", "fwd", 1, 224, 96, {1: "launch_cfg<1,3,1,1,8,2,1,2,P> XTRA", 3: "launch_cfg<1,3,1,1,8,1,3,2,P> XTRA"}, res=True),
    _c("p1_96_gff0", "fwd", 1, 512, 96, {1: "launch_cfg<1,3,1,2,4,2,1,2,P> (32 chunks)", 3: "launch_cfg<1,3,1,2,4,1,3,2,P> (32 chunks)"}),
    _c("p5_sfe1_24", "fwd", 5, 24, 96, {1: "launch_cfg<5,1,1,2,8,1,1,2,P>, 3 columns", 3: "conv_x3_kernel<5,P>, tap pairs"}),
    _c("p5_sfe1_36", "fwd", 5, 36, 96, {1: "launch_cfg<5,1,1,2,8,1,1,2,P>, 3 columns", 3: "conv_x3_kernel<5,P>, tap pairs"}),
    _c("p5_sfe1_60", "fwd", 5, 60, 96, {1: "launch_cfg<5,1,1,2,8,1,1,2,P>, 3 columns", 3: "conv_x3_kernel<5,P>, plain last chunk"}),
    # ---- PixelShuffle, FINAL, FINAL_SUBPIX
    _c("s3_256", "fwd", 3, 96, 256, {1: "launch_cfg<3,2,2,4,4,1,1,2,S>", 3: "conv_x3_kernel<3,S,WIDE=1>"}, epilogue="shuffle"),
    _c("f3_cout4", "fwd", 3, 64, 4, {1: "launch_cfg<3,1,1,2,8,1,1,2,F>", 3: "conv_x3_kernel<3,F>"}, epilogue="final", nimg=2),
    _c("f3_c64_2", "fwd", 3, 64, 3, {1: "final_dot2_kernel", 3: "final_m16_kernel"}, epilogue="final", nimg=2),
    _c("f3_c64_5", "fwd", 3, 64, 3, {1: "final_dot2_kernel", 3: "final_m16_kernel"}, epilogue="final", nimg=5),
    _c("f3_c80_3", "fwd", 3, 80, 3, {1: "final_dot2_kernel, 5 chunks", 3: "conv_x3_kernel<3,F> (5 chunks: not final_m16)"},
       epilogue="final", nimg=3),
    _c("f5_subpix", "fwd", 5, 96, 12, {1: "launch_cfg<5,1,1,2,8,1,1,2,FINAL_SUBPIX>", 3: "conv_x3_kernel<5,FINAL_SUBPIX>"},
       epilogue="subpix", nimg=3),
    # ---- backward-data (the XTRA epilogues)
    _c("b3_res", "bwd", 3, 96, 32, {1: "launch_cfg<3,3,1,2,4,1,1,2,P> XTRA", 3: "conv_x3_kernel<3,P,WIDE=1> XTRA"}, res=True, res_chunks=4),
    _c("b3_acc", "bwd", 3, 96, 32, {1: "launch_cfg<3,3,1,2,4,1,1,2,P> XTRA", 3: "conv_x3_kernel<3,P,WIDE=1> XTRA"}, acc=True),
    _c("b3_mask", "bwd", 3, 32, 64, {1: "launch_cfg<3,1,1,2,8,1,1,2,P> XTRA", 3: "conv_x3_kernel<3,P,WIDE=0> XTRA"}, res=True, mask_from=1),
    _c("b3_unshuf", "bwd", 3, 64, 3, {1: "launch_cfg<3,2,1,2,4,1,1,2,P> XTRA", 3: "conv_x3_kernel<3,P,WIDE=1> XTRA"}, y_unshuf=4),
    _c("b5_sfe1", "bwd", 5, 24, 96, {1: "launch_cfg<5,1,1,2,8,1,1,2,P> XTRA", 3: "conv_x3_kernel<5,P> XTRA"}, acc=True),
    _c("b1_lffd", "bwd", 1, 224, 96, {1: "launch_cfg<1,7,1,1,8,2,1,2,P> XTRA", 3: "launch_cfg_x<1,7,1,1,8,1,3,2,PLANES_LFFD>"},
       res=True, res_chunks=6, mask_from=12),
    _c("b1_224", "bwd", 1, 224, 96, {1: "launch_cfg<1,7,1,1,8,2,1,2,P>", 3: "launch_cfg<1,7,1,1,8,1,3,2,P>"}),
    _c("b1_gff0", "bwd", 1, 1152, 96, {1: "launch_cfg<1,6,1,1,8,2,1,2,P>, 6 columns", 3: "launch_cfg<1,6,1,1,8,1,3,2,P>, 6 columns"}),
    # ---- the fused dense-block tail
    _c("tail", "tail", 3, 192, 32, {1: "rdb_tail_kernel<1,2>", 3: "rdb_tail_x3_kernel"}),
    _c("tail_o3", "tail", 3, 192, 32, {1: "rdb_tail_kernel<1,2>, o3 kept", 3: "rdb_tail_x3_kernel, o3 kept"}, store_o3=True),
)
BY_TAG = {c.tag: c for c in CASES}
TAGS = tuple(c.tag for c in CASES)


def shapes(case):
    return EVEN_SHAPES if case.opts.get("y_unshuf") else SHAPES


def key(tag, nterms, shape):
    return "%s/%d/%dx%dx%d" % ((tag, nterms) + tuple(shape))


KEYS = tuple(key(c.tag, nt, s) for c in CASES for nt in NTERMS for s in shapes(c))


def parse_key(k):
    tag, nt, s = k.split("/")
    return BY_TAG[tag], int(nt), tuple(int(v) for v in s.split("x"))


def _gen(case, shape):
    n, h, w = shape
    return torch.Generator().manual_seed(1000003 * TAGS.index(case.tag) + 7919 * h + 31 * w + n)


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _plane_digests(cp, prefix=""):
    d = {prefix + "hi": _sha(cp.hi.view(torch.int16))}
    if cp.lo is not None:
        d[prefix + "lo"] = _sha(cp.lo.view(torch.int16))
    return d


def white_noise_operands(case, shape):
    """The case's white noise as fp32 CPU tensors, drawn in the order the fixture was recorded with.  tail: blk, w3, b3, wl, bl;
    bwd: w, gy, res, acc, mask (None where the case has none; each of chunks(cin) * 16 channels, as the planes are indexed like
    the output); fwd: w, b, x (with its gap planes when x_cpg is set), imgs (a list), res."""
    n, h, w = shape
    o = case.opts
    g = _gen(case, shape)
    randn = lambda *s: torch.randn(*s, generator=g)
    if case.kind == "tail":
        return {"blk": randn(n, 224, h, w), "w3": randn(32, 192, 3, 3) / (192 * 9) ** 0.5, "b3": randn(32),
                "wl": randn(96, 224, 1, 1) / 224 ** 0.5, "bl": randn(96)}
    wt = randn(case.cout, case.cin, case.ks, case.ks) / (case.cin * case.ks * case.ks) ** 0.5
    if case.kind == "bwd":
        gy = randn(n, case.cout, h, w)
        extra = lambda: randn(n, chunks(case.cin) * 16, h, w)
        res = extra() if o.get("res") else None
        acc = extra() if o.get("acc") else None
        mask = extra() if "mask_from" in o else None
        return {"w": wt, "gy": gy, "res": res, "acc": acc, "mask": mask}
    b = randn(case.cout)
    x = randn(n, x_buffer_channels(case), h, w)
    epi = o.get("epilogue", "planes")
    imgs, res = [], None
    if epi in ("final", "subpix"):
        up = 2 if epi == "subpix" else 1
        imgs = [randn(n, case.cout // (up * up), up * h, up * w) for _ in range(o.get("nimg", 0))]
    elif o.get("res"):
        res = randn(n, case.cout, h, w)
    return {"w": wt, "b": b, "x": x, "imgs": imgs, "res": res}


def chunks(c):
    return (c + 15) // 16


def x_buffer_channels(case):
    """Channels of a forward case's input buffer: cin, or with x_cpg groups of x_cpg planes with one unused plane between them —
    chunk c is plane (c / x_cpg) * (x_cpg + 1) + c % x_cpg of the buffer."""
    cpg = case.opts.get("x_cpg")
    return (chunks(case.cin) // cpg) * (cpg + 1) * 16 if cpg else case.cin


def call_library(case, nterms, shape, opnd, out=None, zero_fill=True, **bwd_args):
    """One call of the library on the operands `opnd` (the dict white_noise_operands describes; needs a GPU).  Returns
    (outputs, inputs): outputs {"y": CP} for plane stores, {"f32": tensor} for the FINAL epilogues, {"y": CP, "o3": CP} for the
    tail that keeps o3; inputs the activation planes as uploaded, by operand name.  `out`: the output planes (default: zero-filled,
    so that padding the kernels leave alone cannot change a digest; `zero_fill=False`: left to the wrapper, which allocates them
    uninitialised — tests/test_gpu_poison.py); `bwd_args`: further arguments of ops.conv2d_bwd_data."""
    from bin_amd import _lib as L, ops
    n, h, w = shape
    o = case.opts
    planes = lambda t: None if t is None else ops.nchw_to_planes(t.cuda(), nterms)
    dev = torch.device("cuda")

    def zeros(nch, hh, ww, channels=None):
        if not zero_fill:
            return None
        cp = ops.CP.empty(nch, n, hh, ww, nterms, dev, channels)
        cp.hi.zero_()
        if cp.lo is not None:
            cp.lo.zero_()
        return cp

    if case.kind == "tail":
        blk = planes(opnd["blk"])
        cw3 = ops.ConvWeights(opnd["w3"].cuda(), opnd["b3"].cuda(), nterms=nterms)
        cwl = ops.ConvWeights(opnd["wl"].cuda(), opnd["bl"].cuda(), nterms=nterms)
        read = ops.CP(blk.hi.clone(), None if blk.lo is None else blk.lo.clone(), 224)      # (store_o3 writes planes 12, 13 of blk)
        y = ops.rdb_tail(blk, cw3, cwl, out=out if out is not None else zeros(6, h, w), store_o3=bool(o.get("store_o3")))
        outs = {"y": y}
        if o.get("store_o3"):
            outs["o3"] = blk.sub(12, 2)
        return outs, {"blk": read}

    if case.kind == "bwd":
        gy = planes(opnd["gy"])
        dw = ops.DgradWeights(opnd["w"].cuda(), nterms=nterms)
        nch = ops.chunks(case.cin)
        res, acc, mask = planes(opnd["res"]), planes(opnd["acc"]), planes(opnd["mask"])
        yu = o.get("y_unshuf", 0)
        if out is None:
            out = zeros(4 * yu, h // 2, w // 2) if yu else zeros(nch, h, w, case.cin)
        y = ops.conv2d_bwd_data(gy, dw, res=res, res_chunks=o.get("res_chunks", 0), acc=acc, mask=mask, mask_from=o.get("mask_from", 0),
                                out=out, y_unshuf=yu, **bwd_args)
        return {"y": y}, {"gy": gy, "res": res, "acc": acc, "mask": mask}

    epi = o.get("epilogue", "planes")
    cw = ops.ConvWeights(opnd["w"].cuda(), opnd["b"].cuda(), nterms=nterms, shuffle=epi == "shuffle")
    kw = {}
    if o.get("x_cpg"):
        cpg = o["x_cpg"]
        kw = dict(x_cpg=cpg, x_group_stride=(cpg + 1) * n * h * w * 16)
    x = planes(opnd["x"])
    if epi in ("final", "subpix"):
        imgs = [t.cuda() for t in opnd["imgs"]]
        y = ops.conv2d(x, cw, epilogue=L.EPI_FINAL if epi == "final" else L.EPI_FINAL_SUBPIX, images=imgs, **kw)
        if epi == "subpix":                  # the same buffer as the kernel fills it: fp32 NCHW [N, cout / 4, 2 H, 2 W]
            y = y.view(n, case.cout // 4, 2 * h, 2 * w)
        return {"f32": y}, {"x": x}
    res = planes(opnd["res"])
    if epi == "shuffle":
        y = ops.conv2d(x, cw, epilogue=L.EPI_SHUFFLE,
                       out=out if out is not None else zeros(ops.chunks(case.cout // 4), 2 * h, 2 * w, case.cout // 4), **kw)
    else:
        y = ops.conv2d(x, cw, relu=bool(o.get("relu")), residual=res,
                       out=out if out is not None else zeros(ops.chunks(case.cout), h, w, case.cout), **kw)
    return {"y": y}, {"x": x, "res": res}


def white_noise_bits(case, nterms, shape):
    """{buffer name: sha256} of every output buffer of one call of the library on the case's white noise (needs a GPU)."""
    outs, _ = call_library(case, nterms, shape, white_noise_operands(case, shape))
    if "f32" in outs:
        return {"f32": _sha(outs["f32"].view(torch.int32))}
    d = _plane_digests(outs["y"])
    if "o3" in outs:
        d.update(_plane_digests(outs["o3"], "o3_"))
    return d
