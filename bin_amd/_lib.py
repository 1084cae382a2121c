"""ctypes binding of the eleven shared objects of bin_amd/build.py's table (libbinhip.so and the ten small libraries beside it,
include/<name>.h) and of those of its EXTRA_LIBRARIES (libbinexpose.so) and ADDON_LIBRARIES (libbinssim.so, libbinlap.so, libbincrop.so), each loaded
on first use.  The product path has NO fallback: if a library is missing, of another version or a call fails this raises, it never routes
to PyTorch/CPU code."""
import ctypes as C
import os
from functools import partial

from . import build as _build
from .build import BY_NAME, LIB_PATH  # noqa: F401  (LIB_PATH: callers read libbinhip.so's path as _lib.LIB_PATH)

RDN_LAYERS = 66              # bin_stage4's layer count; BinRdnPlan arrays hold RDN_MAX_LAYERS
RDN_MAX_LAYERS, RDN_MAX_CONVS = 192, 7
PLAN_KEEP_ACTS, PLAN_NO_FUSE, PLAN_RDB3, PLAN_FUSED_UPNET, PLAN_FUSED_UPNET_TRAIN = 1, 2, 4, 8, 16
PLAN_UPNET_FOLD = 32         # BINHIP_PLAN_UPNET_FOLD
PLAN_HOLD_WEIGHTS = 64       # BINHIP_PLAN_HOLD_WEIGHTS
BWD_ACCUMULATE = 1          # BinRdnBwdPlan.reserved flag (BINHIP_BWD_ACCUMULATE)
BWD_SAVED_X3 = 2            # BINHIP_BWD_SAVED_X3
BWD_FUSED_UPNET = 4         # BINHIP_BWD_FUSED_UPNET
EPI_PLANES, EPI_SHUFFLE, EPI_FINAL, EPI_FINAL_SUBPIX = 0, 1, 2, 4
PROF_WGRAD = 16             # BINHIP_PROF_WGRAD
LOSS_CHARBONNIER, LOSS_L1_SUM, LOSS_L2_SUM = 0, 1, 2
RDN_LAYOUT_WORDS, RDN_BWD_LAYOUT_WORDS = 16, 24


class BinConvDesc(C.Structure):
    _fields_ = [("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("ksize", C.c_int32),
                ("cin_chunks", C.c_int32), ("cout", C.c_int32), ("cout_pad", C.c_int32),
                ("nterms", C.c_int32), ("epilogue", C.c_int32), ("relu", C.c_int32),
                ("x_cpg", C.c_int32), ("x_group_stride", C.c_int64), ("n_images", C.c_int32),
                ("reserved", C.c_int32), ("status", C.c_void_p)]


LOSS_MAX_TERMS = 24          # BINHIP_LOSS_MAX_TERMS
CONV_HALF_LAST_CHUNK = 1     # BinConvDesc.reserved flag of binhip_conv2d_fwd (BINHIP_CONV_HALF_LAST_CHUNK)
CONV_UPNET_FOLD = 2          # BINHIP_CONV_UPNET_FOLD
CONV_HOLD_WEIGHTS = 4        # BINHIP_CONV_HOLD_WEIGHTS
TAIL_STORE_O3, TAIL_HOLD_WEIGHTS = 1, 2      # binhip_rdb_tail_fwd's store_o3 bits (BINHIP_TAIL_*)


class BinLossTerms(C.Structure):
    _fields_ = [("x", C.c_void_p * LOSS_MAX_TERMS), ("y", C.c_void_p * LOSS_MAX_TERMS), ("n_terms", C.c_int32)]


class BinLossGrads(C.Structure):
    _fields_ = [("out", C.c_void_p * LOSS_MAX_TERMS), ("term_a", C.c_int32 * LOSS_MAX_TERMS),
                ("term_b", C.c_int32 * LOSS_MAX_TERMS), ("sign_a", C.c_float * LOSS_MAX_TERMS),
                ("sign_b", C.c_float * LOSS_MAX_TERMS), ("n_out", C.c_int32)]


class BinRdnShape(C.Structure):
    """(G0, D, C, G) of an RDN sub-network (include/binhip.h); all zero = bin_stage4's (96, 12, 4, 32)."""
    _fields_ = [("G0", C.c_int32), ("D", C.c_int32), ("C", C.c_int32), ("G", C.c_int32)]


class BinRdnPlan(C.Structure):
    _fields_ = [("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("n_inputs", C.c_int32),
                ("nterms", C.c_int32), ("reserved", C.c_int32), ("shape", BinRdnShape),
                ("w_hi", C.c_void_p * RDN_MAX_LAYERS), ("w_lo", C.c_void_p * RDN_MAX_LAYERS),
                ("bias", C.c_void_p * RDN_MAX_LAYERS), ("status", C.c_void_p), ("profiler", C.c_void_p)]


class BinRdnBwdPlan(C.Structure):
    _fields_ = [("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("n_inputs", C.c_int32),
                ("nterms", C.c_int32), ("reserved", C.c_int32), ("shape", BinRdnShape),
                ("wt_hi", C.c_void_p * RDN_MAX_LAYERS), ("wt_lo", C.c_void_p * RDN_MAX_LAYERS),
                ("zero_bias", C.c_void_p),
                ("dw", C.c_void_p * RDN_MAX_LAYERS), ("db", C.c_void_p * RDN_MAX_LAYERS), ("gin", C.c_void_p * 5),
                ("status", C.c_void_p), ("aux_stream", C.c_void_p), ("profiler", C.c_void_p)]


class BinRelayoutItem(C.Structure):
    _fields_ = [("w", C.c_void_p * (RDN_MAX_CONVS + 1)), ("bias", C.c_void_p), ("w_hi", C.c_void_p), ("w_lo", C.c_void_p),
                ("bias_out", C.c_void_p), ("kind", C.c_int32), ("cout", C.c_int32), ("cin", C.c_int32),
                ("ksize", C.c_int32), ("rows_pad", C.c_int32), ("cin_chunks", C.c_int32), ("cout_block", C.c_int32),
                ("shuffle_or_group", C.c_int32), ("shape", BinRdnShape)]


RELAYOUT_FWD, RELAYOUT_DGRAD, RELAYOUT_RDB_GATHER = 0, 1, 2
SCORE_SSIM_G11, SCORE_SSIM_U7 = 1, 2   # BINHIP_SCORE_SSIM_* flags of binhip_image_score / binhip_frame_score
SCORE_MAX_PAIRS = 32                   # BINHIP_SCORE_MAX_PAIRS

ADAM_MAX_TENSORS = 64                  # BINOPT_ADAM_MAX_TENSORS (include/binopt.h, libbinopt.so)


class BinAdamTensor(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("numel", C.c_int64),
                ("step_size", C.c_float), ("inv_sqrt_bc2", C.c_float)]


GRAD_MAX_TENSORS = 128                 # BINGRAD_MAX_TENSORS (include/bingrad.h, libbingrad.so)
GRAD_FLAG_NONFINITE, GRAD_FLAG_STATUS = 1, 2   # BINGRAD_FLAG_*


class BinGradTensor(C.Structure):
    _fields_ = [("g", C.c_void_p), ("numel", C.c_int64)]


class BinGradRecord(C.Structure):
    _fields_ = [("sumsq", C.c_double), ("norm", C.c_float), ("coef", C.c_float), ("flags", C.c_int32), ("status", C.c_uint32),
                ("reserved", C.c_int32 * 2)]


EMA_MAX_TENSORS = 136                  # BINEMA_MAX_TENSORS (include/binema.h, libbinema.so)


class BinEmaTensor(C.Structure):
    _fields_ = [("e", C.c_void_p), ("p", C.c_void_p), ("numel", C.c_int64)]


ENS_FLIP_W, ENS_FLIP_H = 1, 2          # BINENS_FLIP_* (include/binens.h, libbinens.so)
ENS_MAX_ORIENT, ENS_MAX_SOURCES, ENS_MAX_SLOTS = 8, 6, 14   # BINENS_MAX_*


class BinEnsOrient(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p * ENS_MAX_ORIENT), ("flip", C.c_uint8 * ENS_MAX_ORIENT), ("n_dst", C.c_int32)]


class BinEnsMerge(C.Structure):
    _fields_ = [("src", C.c_void_p * ENS_MAX_ORIENT), ("dst", C.c_void_p)]


YUV_CHROMA_420, YUV_CHROMA_444 = 420, 444                # BINYUV_CHROMA_* (include/binyuv.h, libbinyuv.so)
YUV_MATRIX_BT601, YUV_MATRIX_BT709 = 0, 1                 # BINYUV_MATRIX_*
YUV_RANGE_LIMITED, YUV_RANGE_FULL = 0, 1                  # BINYUV_RANGE_*


class BinYuvFormat(C.Structure):
    _fields_ = [("chroma", C.c_int32), ("matrix", C.c_int32), ("range", C.c_int32)]


SCENE_BINS = 64                        # BINSCENE_BINS (include/binscene.h, libbinscene.so)


class BinSceneRecord(C.Structure):
    _fields_ = [("sad", C.c_uint64), ("hist", C.c_uint32 * SCENE_BINS)]


CHAIN_MAX_ITEMS = 24                   # BINCHAIN_MAX_ITEMS (include/binchain.h, libbinchain.so)


class BinChainItem(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p)]


PLANE_SSIM_G11, PLANE_SSIM_U7 = 1, 2    # BINSCORE_SSIM_* (include/binscore.h, libbinscore.so)


class BinPlaneScores(C.Structure):
    _fields_ = [("sse", C.c_uint64 * 3), ("sad", C.c_uint64 * 3), ("ssim_g11", C.c_double), ("ssim_u7", C.c_double)]


_SIGNATURES = {
    "binhip_version": (C.c_int, []),
    "binhip_device_cus": (C.c_int, []),
    "binhip_conv_cout_block": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "binhip_weights_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "binhip_weights_relayout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "binhip_weights_relayout_batch": (C.c_int, [C.POINTER(BinRelayoutItem), C.c_int, C.c_void_p]),
    "binhip_conv2d_fwd": (C.c_int, [C.POINTER(BinConvDesc)] + [C.c_void_p] * 10 +
                          [C.POINTER(C.c_void_p), C.c_void_p]),
    "binhip_nchw_to_planes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "binhip_planes_to_nchw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p]),
    "binhip_pixel_unshuffle_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p]),
    "binhip_pack_inputs": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "binhip_u8_to_frame": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p]),
    "binhip_frame_to_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p]),
    "binhip_convlstm_fwd": (C.c_int, [C.c_void_p] * 5 + [C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                          C.c_void_p, C.c_void_p]),
    "binhip_lstm_gates_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "binhip_lstm_gates_bwd": (C.c_int, [C.c_void_p] * 4 + [C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "binhip_charbonnier_partials": (C.c_int, [C.c_int64]),
    "binhip_charbonnier_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "binhip_charbonnier_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "binhip_pixel_loss_fwd": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "binhip_pixel_loss_bwd": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "binhip_multi_loss_fwd": (C.c_int, [C.c_int, C.POINTER(BinLossTerms), C.c_int64, C.c_float, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "binhip_multi_loss_bwd": (C.c_int, [C.c_int, C.POINTER(BinLossTerms), C.c_int64, C.c_float, C.c_void_p,
                                        C.POINTER(BinLossGrads), C.c_void_p]),
    "binhip_dgrad_rows_pad": (C.c_int, [C.c_int, C.c_int]),
    "binhip_weights_relayout_dgrad": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "binhip_weights_relayout_rdb_gather": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p]),
    "binhip_conv2d_bwd_data": (C.c_int, [C.POINTER(BinConvDesc)] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "binhip_wgrad_workspace_bytes": (C.c_size_t, [C.c_int] * 6),
    "binhip_conv2d_bwd_weight": (C.c_int, [C.POINTER(BinConvDesc)] + [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p,
                                           C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "binhip_grad_scale": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "binhip_nchw_to_planes_scaled": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "binhip_unshuffle_planes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "binhip_unpack_input_grads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.POINTER(C.c_void_p), C.c_void_p]),
    "binhip_convlstm_bwd_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "binhip_convlstm_bwd": (C.c_int, [C.c_void_p] * 5 + [C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_size_t] + [C.c_void_p] * 6),
    "binhip_rdn_backward_workspace_bytes": (C.c_size_t, [C.c_int] * 5 + [C.POINTER(BinRdnShape)]),
    "binhip_rdn_backward": (C.c_int, [C.POINTER(BinRdnBwdPlan), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                      C.c_size_t, C.c_void_p]),
    "binhip_profiler_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "binhip_profiler_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "binhip_profiler_destroy": (None, [C.c_void_p]),
    "binhip_rdb_tail_fwd": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 10 +
                            [C.c_int, C.c_void_p, C.c_void_p]),
    "binhip_rdn_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(BinRdnShape)]),
    "binhip_rdn_workspace_layout": (C.c_int, [C.c_int] * 5 + [C.POINTER(BinRdnShape), C.POINTER(C.c_int64), C.c_int]),
    "binhip_rdn_backward_workspace_layout": (C.c_int, [C.c_int] * 5 + [C.POINTER(BinRdnShape), C.POINTER(C.c_int64), C.c_int]),
    "binhip_rdn_forward": (C.c_int, [C.POINTER(BinRdnPlan), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p,
                                     C.c_size_t, C.c_void_p]),
    "binhip_image_score_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "binhip_image_score": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                     C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "binhip_frame_score_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "binhip_frame_score": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(C.c_double), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "binhip_gather_windows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p]),
    "binhip_gather_windows_blur": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 5 +
                                   [C.c_void_p, C.c_void_p]),
}

# libbinopt.so (include/binopt.h): the optimizer library, loaded on first use
OPT_VERSION = 100                      # BINOPT_VERSION
_OPT_SIGNATURES = {
    "binopt_version": (C.c_int, []),
    "binopt_adam_step": (C.c_int, [C.POINTER(BinAdamTensor), C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
}

# libbingrad.so (include/bingrad.h): the gradient-guard library, loaded on first use
GRAD_VERSION = 100                     # BINGRAD_VERSION
_GRAD_SIGNATURES = {
    "bingrad_version": (C.c_int, []),
    "bingrad_norm_workspace_bytes": (C.c_int64, [C.POINTER(BinGradTensor), C.c_int]),
    "bingrad_norm": (C.c_int, [C.POINTER(BinGradTensor), C.c_int, C.c_float, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                               C.c_void_p]),
    "bingrad_scale": (C.c_int, [C.POINTER(BinGradTensor), C.c_int, C.c_void_p, C.c_void_p]),
}

# libbinema.so (include/binema.h): the weight-average library, loaded on first use
EMA_VERSION = 100                      # BINEMA_VERSION
_EMA_SIGNATURES = {
    "binema_version": (C.c_int, []),
    "binema_step": (C.c_int, [C.POINTER(BinEmaTensor), C.c_int, C.c_float, C.c_void_p]),
}

# libbinens.so (include/binens.h): the self-ensemble library, loaded on first use
ENS_VERSION = 100                      # BINENS_VERSION
_ENS_SIGNATURES = {
    "binens_version": (C.c_int, []),
    "binens_orient": (C.c_int, [C.POINTER(BinEnsOrient), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "binens_merge": (C.c_int, [C.POINTER(BinEnsMerge), C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_void_p]),
}

# libbinyuv.so (include/binyuv.h): the video library, loaded on first use
YUV_VERSION = 100                      # BINYUV_VERSION
_YUV_SIGNATURES = {
    "binyuv_version": (C.c_int, []),
    "binyuv_to_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(BinYuvFormat), C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.c_void_p, C.c_void_p]),
    "binyuv_from_frame": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(BinYuvFormat), C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
}

# libbinscene.so (include/binscene.h): the scene library, loaded on first use
SCENE_VERSION = 100                    # BINSCENE_VERSION
_SCENE_SIGNATURES = {
    "binscene_version": (C.c_int, []),
    "binscene_luma_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
}

# libbinchain.so (include/binchain.h): the chain library, loaded on first use
CHAIN_VERSION = 100                    # BINCHAIN_VERSION
_CHAIN_SIGNATURES = {
    "binchain_version": (C.c_int, []),
    "binchain_reframe": (C.c_int, [C.POINTER(BinChainItem), C.c_int] + [C.c_int] * 11 + [C.c_void_p]),
}

# libbinrate.so (include/binrate.h): the rate library, loaded on first use
RATE_VERSION = 100                     # BINRATE_VERSION
RATE_E_ARG, RATE_E_SHAPE = -1, -2      # BINRATE_E_ARG, BINRATE_E_SHAPE
_RATE_SIGNATURES = {
    "binrate_version": (C.c_int, []),
    "binrate_blend_to_yuv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float] + [C.c_int] * 6 + [C.POINTER(BinYuvFormat), C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
}

# libbinscore.so (include/binscore.h): the score library, loaded on first use
SCORE_VERSION = 100                    # BINSCORE_VERSION
SCORE_E_ARG, SCORE_E_SHAPE, SCORE_E_WORKSPACE = -1, -2, -3   # BINSCORE_E_*
_SCORE_SIGNATURES = {
    "binscore_version": (C.c_int, []),
    "binscore_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "binscore_planes": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 4 + [C.POINTER(C.c_double), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
}

# libbinclip.so (include/binclip.h): the clip library, loaded on first use
CLIP_VERSION = 100                     # BINCLIP_VERSION
CLIP_E_ARG, CLIP_E_SHAPE = -1, -2      # BINCLIP_E_ARG, BINCLIP_E_SHAPE
_CLIP_SIGNATURES = {
    "binclip_version": (C.c_int, []),
    "binclip_yuv_to_bgr": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(BinYuvFormat), C.c_void_p, C.c_void_p]),
}

# libbinexpose.so (include/binexpose.h): the exposure library, loaded on first use
EXPOSE_VERSION = 100                   # BINEXPOSE_VERSION
EXPOSE_E_ARG, EXPOSE_E_SHAPE = -1, -2  # BINEXPOSE_E_ARG, BINEXPOSE_E_SHAPE
EXPOSE_ONE, EXPOSE_TABLE = (1 << 24) - 1, 256   # BINEXPOSE_ONE, BINEXPOSE_TABLE
_EXPOSE_SIGNATURES = {
    "binexpose_version": (C.c_int, []),
    "binexpose_check_curve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "binexpose_gather": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_void_p]),
}

# libbinssim.so (include/binssim.h): the SSIM-criterion library, loaded on first use
SSIM_VERSION = 100                     # BINSSIM_VERSION
SSIM_E_ARG, SSIM_E_SHAPE, SSIM_E_WORKSPACE = -1, -2, -3   # BINSSIM_E_*
SSIM_MAX_TERMS = 24                    # BINSSIM_MAX_TERMS
SSIM_FWD_TILE = (16, 118)              # BINSSIM_FWD_TILE_H, BINSSIM_FWD_TILE_W: windows per workgroup of the forward
SSIM_BWD_TILE = (32, 32)               # BINSSIM_BWD_TILE_H, BINSSIM_BWD_TILE_W: pixels per workgroup of the backward


class BinSsimTerms(C.Structure):
    _fields_ = [("x", C.c_void_p * SSIM_MAX_TERMS), ("y", C.c_void_p * SSIM_MAX_TERMS), ("gx", C.c_void_p * SSIM_MAX_TERMS),
                ("gy", C.c_void_p * SSIM_MAX_TERMS), ("n_terms", C.c_int32)]


_SSIM_SIGNATURES = {
    "binssim_version": (C.c_int, []),
    "binssim_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "binssim_forward": (C.c_int, [C.POINTER(BinSsimTerms), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p, C.c_size_t,
                                  C.c_void_p, C.c_void_p]),
    "binssim_backward": (C.c_int, [C.POINTER(BinSsimTerms), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p, C.c_void_p]),
}

# libbinlap.so (include/binlap.h): the pyramid-criterion library, loaded on first use
LAP_VERSION = 100                      # BINLAP_VERSION
LAP_E_ARG, LAP_E_SHAPE, LAP_E_WORKSPACE = -1, -2, -3   # BINLAP_E_*
LAP_MAX_TERMS, LAP_MAX_LEVELS = 24, 8  # BINLAP_MAX_TERMS, BINLAP_MAX_LEVELS
LAP_DOWN_TILE = (16, 32)               # BINLAP_DOWN_TILE_H, BINLAP_DOWN_TILE_W: coarse pixels per workgroup of the reduce / E^T kernels
LAP_UP_TILE = (32, 64)                 # BINLAP_UP_TILE_H, BINLAP_UP_TILE_W: fine pixels per workgroup of the band / R^T kernels


class BinLapTerms(C.Structure):
    _fields_ = [("x", C.c_void_p * LAP_MAX_TERMS), ("y", C.c_void_p * LAP_MAX_TERMS), ("gx", C.c_void_p * LAP_MAX_TERMS),
                ("gy", C.c_void_p * LAP_MAX_TERMS), ("n_terms", C.c_int32)]


_LAP_SIGNATURES = {
    "binlap_version": (C.c_int, []),
    "binlap_forward_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "binlap_backward_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "binlap_forward": (C.c_int, [C.POINTER(BinLapTerms), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_size_t,
                                 C.c_void_p, C.c_void_p]),
    "binlap_backward": (C.c_int, [C.POINTER(BinLapTerms), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                  C.c_size_t, C.c_void_p]),
}

# libbincrop.so (include/bincrop.h): the crop-decode library, loaded on first use
CROP_VERSION = 100                     # BINCROP_VERSION
CROP_E_ARG, CROP_E_SHAPE = -1, -2      # BINCROP_E_ARG, BINCROP_E_SHAPE
CROP_FORMATS = 4                       # BINCROP_FORMATS: format index = 2 * matrix + range


class BinCropRow(C.Structure):
    _fields_ = [("offset", C.c_int64), ("H", C.c_int32), ("W", C.c_int32), ("y0", C.c_int32), ("x0", C.c_int32), ("format", C.c_int32),
                ("reserved", C.c_int32)]


_CROP_SIGNATURES = {
    "bincrop_version": (C.c_int, []),
    "bincrop_yuv_crops_to_bgr": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
}

STATUS_SATURATED = 1            # BINHIP_STATUS_SATURATED
STATUS_SYNC_TIMEOUT = 2         # BINHIP_STATUS_SYNC_TIMEOUT

# name (a row of build.LIBRARIES) -> (signatures, the value <name>_version() must return; None: no gate, binders check binhip_version())
_LIBRARIES = {"binhip": (_SIGNATURES, None), "binopt": (_OPT_SIGNATURES, OPT_VERSION), "bingrad": (_GRAD_SIGNATURES, GRAD_VERSION),
              "binema": (_EMA_SIGNATURES, EMA_VERSION), "binens": (_ENS_SIGNATURES, ENS_VERSION), "binyuv": (_YUV_SIGNATURES, YUV_VERSION),
              "binscene": (_SCENE_SIGNATURES, SCENE_VERSION), "binchain": (_CHAIN_SIGNATURES, CHAIN_VERSION),
              "binrate": (_RATE_SIGNATURES, RATE_VERSION), "binscore": (_SCORE_SIGNATURES, SCORE_VERSION),
              "binclip": (_CLIP_SIGNATURES, CLIP_VERSION)}
# the same for the rows of build.EXTRA_LIBRARIES
_EXTRA_LIBRARIES = {"binexpose": (_EXPOSE_SIGNATURES, EXPOSE_VERSION)}
# the same for the rows of build.ADDON_LIBRARIES, the open-ended table
_ADDON_LIBRARIES = {"binssim": (_SSIM_SIGNATURES, SSIM_VERSION), "binlap": (_LAP_SIGNATURES, LAP_VERSION),
                    "bincrop": (_CROP_SIGNATURES, CROP_VERSION)}
_loaded = {}                    # name -> the CDLL, once library(name) has loaded it


def _entry(name):
    for table in (_LIBRARIES, _EXTRA_LIBRARIES):
        if name in table:
            return table[name]
    return _ADDON_LIBRARIES[name]


def exported_symbols(name="binhip"):
    """Names every include/<name>.h entry point must resolve to (checked by the CPU test-suite)."""
    return sorted(_entry(name)[0])


def library(name):
    """Load lib<name>.so (once) and type its entry points.  Raises RuntimeError with the build hint when it is absent, and when
    its <name>_version() is not the value this binding is for."""
    if name not in _loaded:
        signatures, version = _entry(name)
        built = path = _build.row(name).path
        if name == "binhip":        # BIN_AMD_LIB: developer knob: the timeline side build, another commit's library
            path = os.environ.get("BIN_AMD_LIB", built)
        if not os.path.exists(path):
            raise RuntimeError(
                f"bin_amd: HIP library {built} not built. Run `python -c 'import __graft_entry__ as g; "
                f"g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback by design.")
        h = C.CDLL(path)
        for sym, (res, args) in signatures.items():
            fn = getattr(h, sym)
            fn.restype = res
            fn.argtypes = args
        if version is not None and getattr(h, name + "_version")() != version:
            raise RuntimeError(f"bin_amd: {path} is version {getattr(h, name + '_version')()}, this binding is for {version}")
        _loaded[name] = h
    return _loaded[name]


def lib():
    """Load libbinhip.so (once).  Raises RuntimeError with the build hint when it is absent."""
    return library("binhip")


optlib = partial(library, "binopt")
gradlib = partial(library, "bingrad")
emalib = partial(library, "binema")
enslib = partial(library, "binens")
yuvlib = partial(library, "binyuv")
scenelib = partial(library, "binscene")
chainlib = partial(library, "binchain")
ratelib = partial(library, "binrate")
scorelib = partial(library, "binscore")
cliplib = partial(library, "binclip")
exposelib = partial(library, "binexpose")
ssimlib = partial(library, "binssim")
laplib = partial(library, "binlap")
croplib = partial(library, "bincrop")


def check(rc, what):
    if rc != 0:
        kind = {-1: "bad argument", -2: "unsupported shape", -3: "workspace too small"}.get(rc, f"hipError {rc}")
        raise RuntimeError(f"bin_amd: {what} failed: {kind}")
