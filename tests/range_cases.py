"""Case table of the fp16 range contract (include/binhip.h, "Dynamic range"): every store path that writes fp16 chunk planes, with the
entry point that reaches it, the kernel variant behind it and the precision modes it runs in.  Importable without a GPU:
tests/test_gpu_fp16_range.py runs the cases, tests/test_cpu_host.py checks that the table accounts for every saturating store in
bin_amd/csrc/.

CASES[id]: "entry" the C ABI entry point, "variant" the kernel (instantiation) it reaches, "nterms" the modes, plus the parameters the GPU
test needs ("kind" selects its runner).  Cases that split one path by mode name it in "path" (the LFF backward-data instantiation is
its own in each mode).
SITES[(file, function)]: the saturating calls in that function — split_hi( / split_pair( / atomicOr(..., BINHIP_FLAG_SATURATED) — and the
cases that reach it.  A store path added without a case here, or a case dropped from a site's list, fails the CPU guard."""

BOTH = (3, 1)

# The extreme values each per-op case stores, one launch per value.  "how": where the value is placed —
#   "sum"   two input channels feeding the target channel hold a and b (fp16, exact), so the accumulator is a + b exactly;
#   "bias"  the target channel's fp32 bias is the value (the whole channel);
#   "plane" the value is written into one input hi plane element (spreads over the kernel footprint: 0 * NaN = NaN);
#   "extra" the value is written into a residual / accumulator plane element the epilogue adds (backward-data, residual convs).
# Values given as ints are fp32 bit patterns (NaN of either sign).
F16_MAX = 65504.0
NAN_POS, NAN_NEG = 0x7FC00000, 0xFFC00000
VALUES = [
    ("+0", "sum", (0.0, 0.0)),
    ("-0", "sum", (-0.0, -0.0)),
    ("subnormal", "sum", (2.0 ** -24, 0.0)),
    ("-subnormal", "sum", (-3 * 2.0 ** -24, 0.0)),
    ("+65504", "sum", (F16_MAX, 0.0)),
    ("-65504", "sum", (-F16_MAX, 0.0)),
    ("65504.004", "sum", (F16_MAX, 2.0 ** -8)),          # the next fp32 above 65504 (0x477fe001)
    ("-65504.004", "sum", (-F16_MAX, -2.0 ** -8)),
    ("65519", "sum", (F16_MAX, 15.0)),                   # rounds to 65504 in fp16, still outside the range
    ("65520", "sum", (F16_MAX, 16.0)),                   # rounds to inf in fp16
    ("-65520", "sum", (-F16_MAX, -16.0)),
    ("1e5", "sum", (F16_MAX, 34496.0)),
    ("-1e5", "sum", (-F16_MAX, -34496.0)),
    ("1e30", "bias", 1e30),
    ("-1e30", "bias", -1e30),
    ("+inf", "bias", float("inf")),
    ("-inf", "bias", float("-inf")),
    ("+nan bias", "bias", NAN_POS),
    ("-nan bias", "bias", NAN_NEG),
    ("+nan plane", "plane", NAN_POS),
    ("-nan plane", "plane", NAN_NEG),
]
# The backward-data epilogue has no bias: the fp32 values reach it through a residual / accumulator plane instead
EXTRA_VALUES = [
    ("+65504 extra", "extra", F16_MAX),
    ("+inf extra", "extra", float("inf")),
    ("-inf extra", "extra", float("-inf")),
    ("+nan extra", "extra", NAN_POS),
    ("-nan extra", "extra", NAN_NEG),
]


def _fwd(ks, cout_pad, relu, variant, nterms=BOTH):
    return dict(kind="conv_fwd", entry="binhip_conv2d_fwd", variant=variant, nterms=nterms, ks=ks, cout_pad=cout_pad, relu=relu,
                residual=False)


CASES = {}
# ---- packers (scalar split_hi / split_lo)
CASES["nchw_to_planes"] = dict(kind="nchw", entry="binhip_nchw_to_planes", variant="nchw_to_planes_kernel", nterms=BOTH, scale=None)
CASES["nchw_to_planes_scaled"] = dict(kind="nchw", entry="binhip_nchw_to_planes_scaled", variant="nchw_to_planes_kernel (scale)",
                                      nterms=BOTH, scale=4.0)
for k in (2, 3, 5):
    CASES[f"pack_inputs_{k}"] = dict(kind="pack", entry="binhip_pack_inputs", variant="pack_inputs_kernel", nterms=BOTH, frames=k)

# ---- conv2d_fwd PLANES without extras, 32 input channels: the (ksize, cout block) tile variants of both modes that a short-K layer
#      reaches (bh_dispatch_conv).  Not reached: the 1x1 192-row block (GFF.0 backward-data, cout_pad 1152) and the 1x1 96-row
#      long-K tile (>= 32 input chunks); they share conv_epilogue with the cases here.
#      nterms 3: 3x3 -> the plane-split kernel (binhip_conv_x3.hip), 5x5 -> its 5x5 form, 1x1 -> MT 1 / 3 / 7 / 1 (x8 columns)
#      nterms 1: 3x3 -> MT 1 (cout_pad 32, 224), 3 (96), 4 (256: 128-row block); 5x5 -> the plane-split 5x5; 1x1 as above
for ks in (1, 3, 5):
    for cp in ((32, 96, 224, 256) if ks != 5 else (32, 96)):
        for relu in (0, 1):
            CASES[f"conv_planes_k{ks}_c{cp}_relu{relu}"] = _fwd(ks, cp, relu, f"conv_mfma_kernel<KS={ks}> PLANES, cout_pad {cp}")
CASES["conv_planes_k3_c64_relu1"] = _fwd(3, 64, 1, "conv_mfma_kernel<KS=3, MT=2> PLANES (64-row block)")
# ---- PLANES with a residual (the XTRA instantiation: ReLU folded into the clamp after the residual add)
for relu in (0, 1):
    CASES[f"conv_residual_k3_relu{relu}"] = dict(_fwd(3, 96, relu, "conv_mfma_kernel<..., XTRA> PLANES + residual"), residual=True)
    CASES[f"conv_residual_k1_relu{relu}"] = dict(_fwd(1, 96, relu, "conv_mfma_kernel<KS=1, MT=3, XTRA> PLANES + residual"),
                                                 residual=True)
# ---- SHUFFLE (UPNet.0) and FINAL (fp32 output: no clamp, no status bit)
CASES["conv_shuffle"] = dict(kind="conv_shuffle", entry="binhip_conv2d_fwd", variant="conv_mfma_kernel<KS=3> SHUFFLE, cout_pad 256",
                             nterms=BOTH)
CASES["conv_final"] = dict(kind="conv_final", entry="binhip_conv2d_fwd", variant="FINAL: final_m16 (nterms 3) / final_dot2 (nterms 1)",
                           nterms=BOTH)
# ---- fused dense-block tail: conv #3 (ReLU, o3) + LFF + residual
for so in (0, 1):
    for where in ("o3", "y"):
        CASES[f"rdb_tail_store{so}_{where}"] = dict(kind="rdb_tail", entry="binhip_rdb_tail_fwd",
                                                    variant="rdb_tail_x3_kernel (nterms 3) / rdb_tail_kernel<1> (nterms 1)",
                                                    nterms=BOTH, store_o3=so, where=where)
# ---- backward-data epilogues (binhip_conv2d_bwd_data)
_BWD = dict(kind="bwd_data", entry="binhip_conv2d_bwd_data", nterms=BOTH, res=False, acc=False, mask=False, y_unshuf=False, lffd=False)
CASES["bwd_plain"] = dict(_BWD, variant="conv_mfma_kernel<KS=3> PLANES (no extras)")
CASES["bwd_res"] = dict(_BWD, variant="conv_mfma_kernel<KS=3, XTRA> + residual (res_chunks)", res=True)
CASES["bwd_acc"] = dict(_BWD, variant="conv_mfma_kernel<KS=3, XTRA> + accumulator aliasing the output", acc=True)
CASES["bwd_mask"] = dict(_BWD, variant="conv_mfma_kernel<KS=3, XTRA> + residual + ReLU mask (mask_from)", res=True, mask=True)
CASES["bwd_unshuf"] = dict(_BWD, variant="conv_mfma_kernel<KS=3, XTRA> inverse-PixelShuffle store (y_unshuf)", y_unshuf=True)
CASES["bwd_lffd"] = dict(_BWD, variant="conv_mfma_kernel<KS=1, MT=7, EPI=PLANES_LFFD> (res_chunks 6, mask_from 12)", res=True,
                         mask=True, lffd=True, nterms=(3,), path="bwd_lff")
CASES["bwd_lff_generic"] = dict(_BWD, variant="conv_mfma_kernel<KS=1, MT=7> LFF backward-data, single-product mode", res=True,
                                mask=True, lffd=True, nterms=(1,), path="bwd_lff")
# ---- whole-RDN plans (binhip_rdn_forward): per-conv path, fused tail, three-phase dense-block launch; KEEP_ACTS stores o3
CASES["rdn_forward"] = dict(kind="rdn_fwd", entry="binhip_rdn_forward", variant="plan: default / NO_FUSE / RDB3 (nterms 3), +- KEEP_ACTS",
                            nterms=BOTH)
# ---- backward glue: the fused UPNet's gradient packer and ring kernel, the two-layer path's scaled gout packer
CASES["rdn_backward"] = dict(kind="rdn_bwd", entry="binhip_rdn_backward",
                             variant="BINHIP_BWD_FUSED_UPNET: upnet_gsub_kernel + upnet_ring_dgrad_kernel; two-layer: "
                                     "nchw_to_planes_scaled of gout", nterms=BOTH, modes=("f16x3", "mixed", "two_layer"))
# ---- the same glue stores read back from the backward workspace, element by element, with every later store kept inside the range
CASES["rdn_backward_glue"] = dict(kind="glue", entry="binhip_rdn_backward",
                                  variant="upnet_gsub_kernel + upnet_ring_dgrad_kernel (fused UPNet); nchw_to_planes_kernel (two-layer)",
                                  nterms=BOTH, modes=("f16x3", "mixed", "two_layer"))
# ---- the null status word through the raw ABI
CASES["status_null"] = dict(kind="status_null", entry="binhip_conv2d_fwd / binhip_pack_inputs / binhip_rdb_tail_fwd",
                            variant="status = NULL", nterms=BOTH)

# Every case id is written out here (no list derived from CASES): dropping a case from CASES leaves a name below that the CPU guard
# rejects, and dropping it here too is a visible second edit.
_CONV_FWD = ["conv_planes_k1_c32_relu0", "conv_planes_k1_c32_relu1", "conv_planes_k1_c96_relu0", "conv_planes_k1_c96_relu1",
             "conv_planes_k1_c224_relu0", "conv_planes_k1_c224_relu1", "conv_planes_k1_c256_relu0", "conv_planes_k1_c256_relu1",
             "conv_planes_k3_c32_relu0", "conv_planes_k3_c32_relu1", "conv_planes_k3_c96_relu0", "conv_planes_k3_c96_relu1",
             "conv_planes_k3_c224_relu0", "conv_planes_k3_c224_relu1", "conv_planes_k3_c256_relu0", "conv_planes_k3_c256_relu1",
             "conv_planes_k5_c32_relu0", "conv_planes_k5_c32_relu1", "conv_planes_k5_c96_relu0", "conv_planes_k5_c96_relu1",
             "conv_planes_k3_c64_relu1",
             "conv_residual_k3_relu0", "conv_residual_k3_relu1", "conv_residual_k1_relu0", "conv_residual_k1_relu1"]
_BWD_IDS = ["bwd_plain", "bwd_res", "bwd_acc", "bwd_mask", "bwd_unshuf", "bwd_lffd", "bwd_lff_generic"]
_TAIL = ["rdb_tail_store0_o3", "rdb_tail_store0_y", "rdb_tail_store1_o3", "rdb_tail_store1_y"]
SITES = {
    ("binhip_layout.hip", "nchw_to_planes_kernel"): dict(split_hi=1, atomicOr=1,
                                                       cases=["nchw_to_planes", "nchw_to_planes_scaled", "rdn_backward",
                                                             "rdn_backward_glue"]),
    ("binhip_layout.hip", "pack_inputs_kernel"): dict(split_hi=1, atomicOr=1,
                                                    cases=["pack_inputs_2", "pack_inputs_3", "pack_inputs_5", "status_null"]),
    ("binhip_upnet_bwd.hip", "upnet_gsub_kernel"): dict(split_hi=1, atomicOr=1, cases=["rdn_backward", "rdn_backward_glue"]),
    ("binhip_upnet_bwd.hip", "upnet_ring_dgrad_kernel"): dict(split_hi=1, atomicOr=1,
                                                         cases=["rdn_backward", "rdn_backward_glue"]),
    # the LFF backward-data instantiation's two split_pair calls and the generic epilogue's two, one status store
    ("binhip_conv_common.h", "conv_epilogue"): dict(split_pair=4, atomicOr=1,
                                                    cases=_CONV_FWD + _BWD_IDS + ["conv_shuffle", "rdb_tail_store0_y", "rdb_tail_store1_y",
                                                                                  "rdn_forward", "status_null"]),
    # nterms 1: conv #3 with the ReLU folded (o3), the LFF + residual output
    ("binhip_fused.hip", "rdb_tail_kernel"): dict(split_pair=4, atomicOr=1, cases=_TAIL + ["rdn_forward"]),
    ("binhip_fused_x3.hip", "rdb_tail_x3_kernel"): dict(split_pair=2, atomicOr=1, cases=_TAIL + ["rdn_forward", "status_null"]),
}
# fp32 stores, outside the range contract: run as the contrast case (1e30 / inf / NaN pass through, no status bit)
FP32_CASES = ["conv_final"]
# paths that store fp32 and are therefore outside the table: ConvLSTM, the losses, FINAL (run as the contrast case "conv_final")


def runs(kinds):
    """(case id, nterms) pairs of the cases of these kinds, for pytest parametrisation."""
    return [(c, nt) for c, v in CASES.items() if v["kind"] in kinds for nt in v["nterms"]]
