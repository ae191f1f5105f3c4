"""ctypes binding of libmvfnet_hip.so (the C ABI in include/mvfnet_hip.h).

The library is built in-tree by `python -m mvfnet_amd.build` (or __graft_entry__.build()).
There is NO fallback: if the shared object is missing or fails to load, importing this module
raises, and every op in mvfnet_amd.ops raises with it.
"""
import ctypes as C
import os

import torch  # noqa: F401  -- FIRST: torch bundles its own libamdhip64; ours must resolve to that same runtime

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MVF_LIB_PATH") or os.path.join(_HERE, "libmvfnet_hip.so")      # (override: tooling only, e.g. timing-ablation builds)

MVF_F32, MVF_BF16 = 0, 1
MVF_NCHW, MVF_NHWC = 0, 1
VIEW_T, VIEW_H, VIEW_W = 1, 2, 4
MODE_BITS = {"T": 1, "TH": 3, "THW": 7}
METRICS_ROWS, METRICS_BAD_LABEL, METRICS_NAN_ROWS, METRICS_HITS, METRICS_MAX_K, METRICS_CONFUSION = 0, 1, 2, 8, 8, 16      # state words of mvf_metrics_update
MULTILABEL_SLOTS, MULTILABEL_NAN_ROWS, MULTILABEL_OVERFLOW, MULTILABEL_SEEN, MULTILABEL_STATE_WORDS = 0, 1, 2, 3, 8      # state words of mvf_multilabel_record
ERRNAMES = {-1: "MVF_EINVAL", -2: "MVF_ESHAPE", -3: "MVF_EWS", -4: "MVF_EHIP", -5: "MVF_EUNSUPPORTED"}


class MvfDesc(C.Structure):
    _fields_ = [("nt", C.c_int32), ("c", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("n_segment", C.c_int32),
                ("cs", C.c_int32), ("mode", C.c_int32), ("layout", C.c_int32), ("dtype", C.c_int32)]


class ConvDesc(C.Structure):
    _fields_ = [("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32),
                ("kh", C.c_int32), ("kw", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32),
                ("ho", C.c_int32), ("wo", C.c_int32), ("x_pix_stride", C.c_int32),
                ("dtype", C.c_int32), ("relu", C.c_int32), ("split_c", C.c_int32), ("x2_pix_stride", C.c_int32), ("in_dil", C.c_int32),
                ("res_c0", C.c_int32), ("x_c0", C.c_int32)]


class ConvLaunchInfo(C.Structure):
    """mvf_conv_launch_info_t: which kernel the calling thread's last mvf_conv2d_* call launched (host-side record)."""
    _fields_ = [("family", C.c_int32), ("epi_asked", C.c_int32), ("epi_run", C.c_int32), ("pointwise", C.c_int32), ("buffers", C.c_int32),
                ("tile_m", C.c_int32), ("tile_n", C.c_int32), ("dtype", C.c_int32), ("k_chunks", C.c_int32), ("half_k", C.c_int32),
                ("launches", C.c_int32)]


CONV_FAMILIES = {0: "none", 1: "reg", 2: "x3", 3: "lds_dma", 4: "t256_2b", 5: "t256_p4", 6: "dbuf", 7: "dbuf_pf2", 8: "streamk", 9: "generic",
                 10: "mvf_loader", 11: "stem_direct", 12: "pw_sums", 13: "c3x3_c64"}


class WgradLaunchInfo(C.Structure):
    """mvf_wgrad_launch_info_t: which kernel the calling thread's last mvf_conv2d_nhwc_wgrad[_wgs] call launched (host-side record)."""
    _fields_ = [("family", C.c_int32), ("stages", C.c_int32), ("tile_co", C.c_int32), ("tile_k", C.c_int32), ("dtype", C.c_int32),
                ("nsplit", C.c_int32), ("rows_per_split", C.c_int32), ("xcd_rr", C.c_int32), ("split_operand", C.c_int32), ("gram", C.c_int32),
                ("wgs_target", C.c_int32), ("launches", C.c_int32)]


WGRAD_FAMILIES = {0: "none", 1: "f32_reg", 2: "f32_dma", 3: "x3", 4: "bf16_widen", 5: "bf16_reg", 6: "bf16_dma2", 7: "bf16_pipe", 8: "t256_2b", 9: "t256_p4",
                  10: "c3x3_c64", 11: "stem"}


class StencilLaunchInfo(C.Structure):
    """mvf_stencil_launch_info_t: which kernel the calling thread's last mvf_nhwc_stencil* call launched (host-side record)."""
    _fields_ = [("kernel", C.c_int32), ("dtype", C.c_int32), ("frames_per_chunk", C.c_int32), ("rows_per_band", C.c_int32), ("chan_per_wg", C.c_int32),
                ("bands", C.c_int32), ("pixels_per_wg", C.c_int32), ("grid_x", C.c_int32), ("grid_y", C.c_int32), ("partial_rows", C.c_int32),
                ("flags", C.c_int32), ("launches", C.c_int32)]


STENCIL_KERNELS = {0: "none", 1: "walk1", 2: "walk4", 3: "chunked", 4: "lds"}
STENCIL_FLIP, STENCIL_HSWISH, STENCIL_ADDEND, STENCIL_ADDEND_BITS, STENCIL_OUT_GATE, STENCIL_STATS, STENCIL_TAIL_COPY = 1, 2, 4, 8, 16, 32, 64


class TapgradLaunchInfo(C.Structure):
    """mvf_tapgrad_launch_info_t: which kernel the calling thread's last mvf_nhwc_tapgrad call launched (host-side record)."""
    _fields_ = [("kernel", C.c_int32), ("dtype", C.c_int32), ("nblk", C.c_int32), ("rows_per_blk", C.c_int32), ("cgp", C.c_int32), ("grid_y", C.c_int32),
                ("launches", C.c_int32)]


TAPGRAD_KERNELS = {0: "none", 1: "rows", 2: "bands"}


class BnLaunchInfo(C.Structure):
    """mvf_bn_launch_info_t: which kernels the calling thread's last BatchNorm / max-pool call of csrc/train_ops.hip launched (host-side record)."""
    _fields_ = [("entry", C.c_int32), ("dtype", C.c_int32), ("vn", C.c_int32), ("cqb", C.c_int32), ("rows", C.c_int32), ("gx", C.c_int32), ("gy", C.c_int32),
                ("mask_mode", C.c_int32), ("specialised", C.c_int32), ("finalize", C.c_int32), ("part_rows", C.c_int32), ("pool", C.c_int32),
                ("launches", C.c_int32)]


BN_ENTRIES = {0: "none", 1: "train_stats", 2: "train_finalize", 3: "apply", 4: "apply_colmeans", 5: "bwd_reduce", 6: "bwd_finalize", 7: "bwd_apply", 8: "bwd_pair",
              9: "bwd_pair_wgrad", 10: "pool_fwd", 11: "pool_bwd", 12: "pool_bwd_sums", 13: "pool_bwd_apply"}
BN_FINALIZE_FORMS = {0: "none", 1: "row_major", 2: "cm_workgroup", 3: "cm_wave"}
POOL_FORMS = {0: "none", 1: "element", 2: "rows", 3: "block", 4: "rows_sums", 5: "rows_apply"}


class PackJob(C.Structure):
    _fields_ = [("w", C.c_void_p), ("out", C.c_void_p), ("cout", C.c_int32), ("cin", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32),
                ("kw_pad", C.c_int32), ("cin_pad", C.c_int32), ("kind", C.c_int32), ("first_block", C.c_int32)]


class PlanOp(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n_int", C.c_int32), ("n_flt", C.c_int32), ("reserved", C.c_int32), ("fn", C.c_void_p), ("word0", C.c_longlong),
                ("float0", C.c_longlong)]


class SgdSegment(C.Structure):
    _fields_ = [("first", C.c_int64), ("lr_mult", C.c_float), ("decay_mult", C.c_float)]


class AdamwHyper(C.Structure):
    """mvf_adamw_hyper_t: the hyper-parameters of mvf_adamw_step, doubles in HOST memory (the library rounds 1 - beta and 1 - lr * wd to fp32 once)."""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double), ("decoupled", C.c_int32)]


class FocalParams(C.Structure):
    """mvf_focal_params_t: the settings of mvf_focal_loss / mvf_head_train_fwd_focal, in HOST memory, read at every call (alpha < 0 and a NaN
    target_threshold = off)."""
    _fields_ = [("gamma_pos", C.c_float), ("gamma_neg", C.c_float), ("margin", C.c_float), ("alpha", C.c_float), ("target_threshold", C.c_float),
                ("sum_classes", C.c_int32), ("reserved", C.c_int32 * 2)]


TRN_MAX_FRAMES, TRN_KSPLIT_MAX = 16, 8


class TrnScale(C.Structure):
    """mvf_trn_scale_t: the operands of one relation scale of mvf_trn_head_fwd / mvf_trn_head_bwd (device addresses), in a HOST array read at every call."""
    _fields_ = [("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
                ("dw1", C.c_void_p), ("db1", C.c_void_p), ("dw2", C.c_void_p), ("db2", C.c_void_p)]


class TrnLaunchInfo(C.Structure):
    """mvf_trn_launch_info_t: the calling thread's last mvf_trn_head_fwd / mvf_trn_head_bwd call (host-side record)."""
    _fields_ = [("entry", C.c_int32), ("dtype", C.c_int32), ("rows", C.c_int32), ("n_scales", C.c_int32), ("launches", C.c_int32)]


class LambHyper(C.Structure):
    """mvf_lamb_hyper_t: the hyper-parameters of mvf_lamb_step, doubles in HOST memory (the library rounds 1 - beta and lr_k * r_k to fp32 once)."""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double), ("trust_clip", C.c_int32),
                ("always_adapt", C.c_int32)]


class StatSegment(C.Structure):
    """mvf_stat_segment_t: one BatchNorm statistic buffer in the flat shadow layout of the precise-BN entry points (csrc/precise_bn.hip)."""
    _fields_ = [("ptr", C.c_void_p), ("first", C.c_long)]


# Every entry point that launches nothing: sizes, row / split counts, tile and split plans, the host-side launch records, the ABI version and the error
# text.  Their return value is an answer, not a status, so a launch plan never holds them (launch_plan.RecordingLib calls them and records nothing); every
# declared function that does not return a status must be named here (tests/test_abi_cpu.py).
QUERIES = frozenset((
    "mvf_abi_version", "mvf_last_error",
    "mvf_fwd_train_workspace_bytes", "mvf_bwd_workspace_bytes", "mvf_conv2d_workspace_bytes", "mvf_conv2d_wgrad_workspace_bytes", "mvf_bn_workspace_bytes",
    "mvf_bn_bwd_wgrad_slab_bytes", "mvf_nhwc_tapgrad_workspace_bytes", "mvf_sgd_workspace_bytes", "mvf_adamw_workspace_bytes", "mvf_lamb_workspace_bytes",
    "mvf_flat_stats_workspace_bytes", "mvf_metrics_state_words",
    "mvf_conv2d_stats_rows", "mvf_nhwc_stencil_stats_rows", "mvf_maxpool_bwd_sums_rows",
    "mvf_bn_bwd_wgrad_splits", "mvf_conv1x1_bwd_fused_splits", "mvf_nhwc_stencil_tile_plan",
    "mvf_conv2d_last_launch", "mvf_conv2d_wgrad_last_launch", "mvf_bn_last_launch", "mvf_nhwc_stencil_last_launch", "mvf_nhwc_tapgrad_last_launch",
    "mvf_trn_head_last_launch",
))


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "mvfnet_amd: %s not found. Build it with `python -m mvfnet_amd.build` (needs hipcc, "
            "--offload-arch=gfx950). There is no CPU or PyTorch fallback for the hot path." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, fp, sz, i32, f32 = C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_float
    dp = C.POINTER(MvfDesc)
    lib.mvf_abi_version.restype = i32
    lib.mvf_abi_version.argtypes = []
    lib.mvf_last_error.restype = C.c_char_p
    lib.mvf_last_error.argtypes = []
    lib.mvf_fwd_infer.restype = i32
    lib.mvf_fwd_infer.argtypes = [dp, vp, vp, fp, fp, fp, fp, fp, vp]
    lib.mvf_fwd_train_workspace_bytes.restype = sz
    lib.mvf_fwd_train_workspace_bytes.argtypes = [dp]
    lib.mvf_fwd_train.restype = i32
    lib.mvf_fwd_train.argtypes = [dp, vp, vp, fp, fp, fp, fp, fp, f32, f32, fp, fp, fp, fp, vp, sz, vp]
    lib.mvf_bwd_workspace_bytes.restype = sz
    lib.mvf_bwd_workspace_bytes.argtypes = [dp]
    lib.mvf_bwd.restype = i32
    lib.mvf_bwd.argtypes = [dp, vp, vp, fp, fp, fp, fp, fp, fp, fp, i32, vp, fp, fp, fp, fp, fp, vp, sz, vp]
    lib.mvf_fwd_infer_slice.restype = i32
    lib.mvf_fwd_infer_slice.argtypes = [dp, vp, vp, fp, fp, fp, fp, fp, vp]
    cp = C.POINTER(ConvDesc)
    lib.mvf_conv2d_nhwc_fwd.restype = i32
    lib.mvf_conv2d_nhwc_fwd.argtypes = [cp, vp, vp, vp, fp, vp, vp, vp]
    lib.mvf_conv2d_workspace_bytes.restype = sz
    lib.mvf_conv2d_workspace_bytes.argtypes = [cp]
    lib.mvf_conv2d_nhwc_fwd_ws.restype = i32
    lib.mvf_conv2d_nhwc_fwd_ws.argtypes = [cp, vp, vp, vp, fp, vp, vp, vp, sz, vp]
    lib.mvf_conv2d_nhwc_dgrad_bnsums.restype = i32
    lib.mvf_conv2d_nhwc_dgrad_bnsums.argtypes = [cp, vp, vp, vp, vp, fp, fp, fp, fp, fp, vp, sz, vp]
    lib.mvf_bn_bwd_finalize.restype = i32
    lib.mvf_bn_bwd_finalize.argtypes = [fp, i32, i32, fp, fp, vp]
    lib.mvf_conv2d_nhwc_fwd_bnapply.restype = i32
    lib.mvf_conv2d_nhwc_fwd_bnapply.argtypes = [cp, vp, vp, vp, fp, fp, vp, fp, fp, vp, vp, vp, sz, vp]
    lib.mvf_conv2d_nhwc_fwd_bnbwd_sums.restype = i32
    lib.mvf_conv2d_nhwc_fwd_bnbwd_sums.argtypes = [cp, vp, vp, vp, vp, vp, fp, fp, fp, vp, sz, vp]
    lib.mvf_conv2d_nhwc_fwd_bnbwd_apply.restype = i32
    lib.mvf_conv2d_nhwc_fwd_bnbwd_apply.argtypes = [cp, vp, vp, vp, vp, vp, fp, fp, fp, fp, fp, vp, vp, sz, vp]
    lib.mvf_conv2d_nhwc_fwd_resmask.restype = i32
    lib.mvf_conv2d_nhwc_fwd_resmask.argtypes = [cp, vp, vp, vp, fp, vp, vp, vp, vp, sz, vp]
    i64_ = C.c_long
    lib.mvf_conv2d_nhwc_fwd_resmask_gate.restype = i32
    lib.mvf_conv2d_nhwc_fwd_resmask_gate.argtypes = [cp, vp, vp, vp, fp, vp, vp, vp, vp, vp, sz, vp]
    lib.mvf_conv2d_nhwc_fwd_resmask_gate_colsums.restype = i32
    lib.mvf_conv2d_nhwc_fwd_resmask_gate_colsums.argtypes = [cp, vp, vp, vp, vp, vp, vp, vp, fp, vp, sz, vp]
    lib.mvf_nhwc_stencil_gate_colsums.restype = i32
    lib.mvf_nhwc_stencil_gate_colsums.argtypes = [dp, vp, i32, vp, i32, fp, fp, fp, i32, vp, i32, vp, vp, fp, vp]
    lib.mvf_conv2d_nhwc_dgrad_bnsums_split.restype = i32
    lib.mvf_conv2d_nhwc_dgrad_bnsums_split.argtypes = [cp, vp, vp, vp, fp, vp, vp, fp, fp, fp, fp, fp, vp, sz, vp]
    lib.mvf_bn_bwd_dzfree_prep.restype = i32
    lib.mvf_bn_bwd_dzfree_prep.argtypes = [vp, i32, i32, fp, fp, fp, fp, fp, i64_, vp, fp, i32, vp]
    lib.mvf_bn_bwd_dzfree_wgrad.restype = i32
    lib.mvf_bn_bwd_dzfree_wgrad.argtypes = [fp, vp, fp, fp, fp, fp, fp, fp, fp, i64_, i32, i32, i32, vp]
    lib.mvf_bn_bwd_dzfree_sums.restype = i32
    lib.mvf_bn_bwd_dzfree_sums.argtypes = [fp, vp, i32, i32, fp, fp, fp, i32, i32, fp, i32, fp, fp, i32, vp]
    lib.mvf_nhwc_stencil_stats_rows.restype = i32
    lib.mvf_nhwc_stencil_stats_rows.argtypes = [dp, i32, i32]
    lib.mvf_nhwc_stencil_tile_plan.restype = i32
    lib.mvf_nhwc_stencil_tile_plan.argtypes = [dp, i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.mvf_nhwc_stencil_stats.restype = i32
    lib.mvf_nhwc_stencil_stats.argtypes = [dp, vp, i32, vp, i32, fp, fp, fp, fp, fp, vp]
    lib.mvf_nhwc_stencil_gate.restype = i32
    lib.mvf_nhwc_stencil_gate.argtypes = [dp, vp, i32, vp, i32, fp, fp, fp, fp, fp, i32, vp, i32, vp, vp, vp]
    lib.mvf_conv2d_stats_rows.restype = i32
    lib.mvf_conv2d_stats_rows.argtypes = [cp]
    lib.mvf_conv2d_nhwc_fwd_stats.restype = i32
    lib.mvf_conv2d_nhwc_fwd_stats.argtypes = [cp, vp, vp, vp, vp, fp, fp, vp, sz, vp]
    lib.mvf_conv2d_last_launch.restype = i32
    lib.mvf_conv2d_last_launch.argtypes = [C.POINTER(ConvLaunchInfo)]
    lib.mvf_pack_conv_weight.restype = i32
    lib.mvf_pack_conv_weight.argtypes = [fp, i32, i32, i32, i32, i32, i32, fp, vp, i32, vp]
    lib.mvf_pack_conv_weights_batched.restype = i32
    lib.mvf_pack_conv_weights_batched.argtypes = [vp, i32, i32, i32, vp]
    lib.mvf_bn_fold.restype = i32
    lib.mvf_bn_fold.argtypes = [fp, fp, fp, fp, f32, i32, fp, fp, vp]
    lib.mvf_stem_prep.restype = i32
    lib.mvf_stem_prep.argtypes = [fp, i32, i32, i32, i32, i32, i32, vp, i32, vp]
    lib.mvf_frames_prep_u8.restype = i32
    lib.mvf_frames_prep_u8.argtypes = [vp, i32, i32, i32, vp, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                       i32, i32, i32, i32, vp, vp, i32, vp]
    lib.mvf_frames_resample_u8.restype = i32
    lib.mvf_frames_resample_u8.argtypes = [vp, i32, i32, i32, vp, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                           i32, i32, i32, i32, vp, vp, i32, vp]
    lib.mvf_frames_resample_color_u8.restype = i32
    lib.mvf_frames_resample_color_u8.argtypes = [vp, i32, i32, i32, vp, vp, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                 i32, i32, i32, i32, vp, vp, i32, vp]
    lib.mvf_frames_gather_resample_u8.restype = i32
    lib.mvf_frames_gather_resample_u8.argtypes = [vp, i32, i32, i32, vp, i32, vp, vp, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                  i32, i32, i32, i32, vp, vp, i32, vp]
    lib.mvf_frames_yuv420_gather_resample_u8.restype = i32
    lib.mvf_frames_yuv420_gather_resample_u8.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, vp, i32, vp, vp, i32, i32, C.POINTER(C.c_float),
                                                         C.POINTER(C.c_float), i32, i32, i32, i32, vp, vp, i32, vp]
    lib.mvf_frames_addressed_resample_u8.restype = i32
    lib.mvf_frames_addressed_resample_u8.argtypes = [vp, C.c_longlong, i32, i32, i32, i32, vp, vp, vp, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                     i32, i32, i32, i32, vp, vp, i32, vp]
    lib.mvf_maxpool3x3s2_nhwc.restype = i32
    lib.mvf_maxpool3x3s2_nhwc.argtypes = [vp, i32, i32, i32, i32, vp, i32, vp]
    lib.mvf_head_pool_fc.restype = i32
    lib.mvf_head_pool_fc.argtypes = [vp, i32, i32, i32, i32, fp, fp, i32, fp, fp, i32, vp]
    lib.mvf_average_clip.restype = i32
    lib.mvf_average_clip.argtypes = [fp, i32, i32, i32, fp, vp]
    i64, ll = C.c_long, C.c_void_p
    lib.mvf_bn_workspace_bytes.restype = sz
    lib.mvf_bn_workspace_bytes.argtypes = [i64, i32]
    lib.mvf_bn_train_stats.restype = i32
    lib.mvf_bn_train_stats.argtypes = [vp, i64, i32, fp, fp, f32, f32, fp, fp, fp, fp, fp, fp, vp, sz, i32, vp]
    lib.mvf_bn_train_finalize.restype = i32
    lib.mvf_bn_train_finalize.argtypes = [fp, i32, i64, i32, fp, fp, f32, f32, fp, fp, fp, fp, fp, fp, vp]
    lib.mvf_bn_train_stats_gram.restype = i32
    lib.mvf_bn_train_stats_gram.argtypes = [fp, fp, vp, i64, i32, i32, fp, fp, f32, f32, fp, fp, fp, fp, fp, fp, i32, vp]
    lib.mvf_bn_apply_colmeans.restype = i32
    lib.mvf_bn_apply_colmeans.argtypes = [vp, i64, i32, fp, fp, i32, vp, fp, vp, sz, i32, vp]
    lib.mvf_bn_apply.restype = i32
    lib.mvf_bn_apply.argtypes = [vp, i64, i32, fp, fp, vp, fp, fp, i32, vp, i32, vp]
    lib.mvf_bn_apply_bits.restype = i32
    lib.mvf_bn_apply_bits.argtypes = [vp, i64, i32, fp, fp, vp, fp, fp, i32, vp, vp, i32, vp]
    lib.mvf_bn_apply_bits_rowscale.restype = i32
    lib.mvf_bn_apply_bits_rowscale.argtypes = [vp, i64, i32, fp, fp, vp, fp, fp, fp, i32, i32, vp, vp, i32, vp]
    lib.mvf_gate_rowscale.restype = i32
    lib.mvf_gate_rowscale.argtypes = [vp, i32, vp, fp, i32, i64, i32, vp, i32, vp]
    lib.mvf_bn_bwd_apply_masked.restype = i32
    lib.mvf_bn_bwd_apply_masked.argtypes = [vp, i32, vp, vp, i64, i32, fp, fp, fp, fp, fp, fp, fp, i32, vp, i32, vp]
    lib.mvf_bn_bwd_reduce.restype = i32
    lib.mvf_bn_bwd_reduce.argtypes = [vp, i32, vp, vp, i64, i32, fp, fp, fp, fp, i32, vp, fp, fp, vp, sz, i32, vp]
    lib.mvf_bn_bwd_apply.restype = i32
    lib.mvf_bn_bwd_apply.argtypes = [vp, i32, vp, i64, i32, fp, fp, fp, fp, fp, fp, fp, i32, vp, i32, vp]
    lib.mvf_maxpool_bn_relu_fwd.restype = i32
    lib.mvf_maxpool_bn_relu_fwd.argtypes = [vp, i32, i32, i32, i32, fp, fp, vp, vp, i32, vp]
    lib.mvf_maxpool_bn_relu_bwd.restype = i32
    lib.mvf_maxpool_bn_relu_bwd.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, vp]
    lib.mvf_maxpool_bwd_sums_rows.restype = i32
    lib.mvf_maxpool_bwd_sums_rows.argtypes = [i32, i32]
    lib.mvf_maxpool_bn_relu_bwd_apply.restype = i32
    lib.mvf_maxpool_bn_relu_bwd_apply.argtypes = [vp, vp, i32, i32, i32, i32, vp, fp, fp, fp, fp, fp, fp, fp, vp, i32, vp]
    lib.mvf_maxpool_bn_relu_bwd_sums.restype = i32
    lib.mvf_maxpool_bn_relu_bwd_sums.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, fp, fp, fp, fp, fp, i32, vp]
    lib.mvf_bn_last_launch.restype = i32
    lib.mvf_bn_last_launch.argtypes = [C.POINTER(BnLaunchInfo)]
    lib.mvf_head_train_fwd.restype = i32
    lib.mvf_head_train_fwd.argtypes = [vp, i32, i32, i32, i32, fp, fp, i32, ll, fp, fp, fp, fp, fp, fp, i32, vp]
    lib.mvf_conv2d_nhwc_fwd_mvf.restype = i32
    lib.mvf_conv2d_nhwc_fwd_mvf.argtypes = [cp, vp, vp, fp, fp, i32, i32, i32, vp, vp, sz, vp]
    lib.mvf_bn_bwd_pair.restype = i32
    lib.mvf_bn_bwd_pair.argtypes = [vp, i32, vp, vp, vp, i64, i32, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, vp, vp, vp, sz, i32, vp]
    lib.mvf_bn_bwd_wgrad_splits.restype = i32
    lib.mvf_bn_bwd_wgrad_splits.argtypes = [i64, i32, i32, i32, i32]
    lib.mvf_bn_bwd_wgrad_slab_bytes.restype = sz
    lib.mvf_bn_bwd_wgrad_slab_bytes.argtypes = [i64, i32, i32, i32, i32]
    lib.mvf_bn_bwd_apply_wgrad.restype = i32
    lib.mvf_bn_bwd_apply_wgrad.argtypes = [vp, i32, vp, vp, i64, i32, fp, fp, fp, fp, fp, fp, fp, i32, vp, vp, i32, i32, fp, sz, i32, vp]
    lib.mvf_bn_bwd_pair_wgrad.restype = i32
    lib.mvf_bn_bwd_pair_wgrad.argtypes = [vp, i32, vp, vp, vp, i64, i32, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, vp, vp, vp, i32, vp, i32, i32,
                                          fp, fp, sz, vp, sz, i32, vp]
    lib.mvf_conv1x1_bwd_fused_splits.restype = i32
    lib.mvf_conv1x1_bwd_fused_splits.argtypes = [i64, i32, i32]
    lib.mvf_conv1x1_bwd_fused.restype = i32
    lib.mvf_conv1x1_bwd_fused.argtypes = [vp, i32, vp, vp, i32, vp, i64, i32, i32, fp, fp, fp, fp, fp, vp, fp, fp, fp, fp, vp, fp, i32, fp, sz, i32, vp]
    lib.mvf_conv1x1_bnbwd_sums_pair.restype = i32
    lib.mvf_conv1x1_bnbwd_sums_pair.argtypes = [vp, i32, vp, vp, i32, vp, vp, i32, vp, i64, i32, i32, fp, fp, fp, fp, fp, fp, i32, i32, vp]
    lib.mvf_wgrad_slab_reduce.restype = i32
    lib.mvf_wgrad_slab_reduce.argtypes = [fp, i32, i32, i32, fp, vp]
    lib.mvf_ce_loss.restype = i32
    lib.mvf_ce_loss.argtypes = [fp, ll, i32, i32, fp, fp, fp, vp]
    lib.mvf_stem_blend.restype = i32
    lib.mvf_stem_blend.argtypes = [vp, i32, i32, i32, i32, i32, vp, fp, vp, i32, vp]
    lib.mvf_stem_erase.restype = i32
    lib.mvf_stem_erase.argtypes = [vp, i32, i32, i32, i32, vp, i32, fp, vp, i32, vp]
    lib.mvf_frames_randaug_u8.restype = i32
    lib.mvf_frames_randaug_u8.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, i32, C.c_uint, vp, vp, vp, C.c_longlong, vp]
    lib.mvf_soft_targets.restype = i32
    lib.mvf_soft_targets.argtypes = [ll, vp, fp, i32, i32, f32, fp, vp]
    lib.mvf_ce_loss_soft.restype = i32
    lib.mvf_ce_loss_soft.argtypes = [fp, fp, i32, i32, fp, fp, fp, vp]
    lib.mvf_head_train_fwd_soft.restype = i32
    lib.mvf_head_train_fwd_soft.argtypes = [vp, i32, i32, i32, i32, fp, fp, i32, fp, fp, fp, fp, fp, fp, fp, i32, vp]
    lib.mvf_distill_loss.restype = i32
    lib.mvf_distill_loss.argtypes = [fp, fp, i32, i32, f32, f32, fp, fp, fp, fp, vp]
    lib.mvf_bce_loss.restype = i32
    lib.mvf_bce_loss.argtypes = [fp, fp, i32, i32, fp, f32, i32, fp, fp, fp, vp]
    lib.mvf_head_train_fwd_bce.restype = i32
    lib.mvf_head_train_fwd_bce.argtypes = [vp, i32, i32, i32, i32, fp, fp, i32, fp, fp, fp, f32, i32, fp, fp, fp, fp, fp, i32, vp]
    lib.mvf_focal_loss.restype = i32
    lib.mvf_focal_loss.argtypes = [fp, fp, i32, i32, fp, C.POINTER(FocalParams), fp, fp, fp, vp]
    lib.mvf_head_train_fwd_focal.restype = i32
    lib.mvf_head_train_fwd_focal.argtypes = [vp, i32, i32, i32, i32, fp, fp, i32, fp, fp, fp, C.POINTER(FocalParams), fp, fp, fp, fp, fp, i32, vp]
    lib.mvf_trn_head_fwd.restype = i32
    lib.mvf_trn_head_fwd.argtypes = [vp, i32, i32, i32, i32, fp, fp, i32, C.POINTER(TrnScale), i32, i32, i32, vp, i32, fp, fp, fp, fp, fp, fp, i32, vp]
    lib.mvf_trn_head_bwd.restype = i32
    lib.mvf_trn_head_bwd.argtypes = [fp, fp, fp, fp, fp, C.POINTER(TrnScale), i32, i32, i32, vp, i32, fp, i32, i32, i32, i32, i32, fp, fp, fp, fp, fp, vp, i32, vp]
    lib.mvf_trn_head_last_launch.restype = i32
    lib.mvf_trn_head_last_launch.argtypes = [C.POINTER(TrnLaunchInfo)]
    lib.mvf_average_clip_sigmoid.restype = i32
    lib.mvf_average_clip_sigmoid.argtypes = [fp, i32, i32, fp, vp]
    lib.mvf_multilabel_record.restype = i32
    lib.mvf_multilabel_record.argtypes = [fp, vp, i32, i32, fp, vp, C.c_long, ll, vp]
    lib.mvf_multilabel_ap.restype = i32
    lib.mvf_multilabel_ap.argtypes = [fp, vp, C.c_long, i32, ll, vp, vp, vp, ll, vp]
    lib.mvf_multilabel_sample_ap.restype = i32
    lib.mvf_multilabel_sample_ap.argtypes = [fp, vp, C.c_long, i32, ll, vp, vp, vp]
    lib.mvf_multilabel_prf.restype = i32
    lib.mvf_multilabel_prf.argtypes = [fp, vp, C.c_long, i32, ll, f32, fp, ll, vp]
    lib.mvf_multilabel_best_f1.restype = i32
    lib.mvf_multilabel_best_f1.argtypes = [fp, vp, vp, ll, C.c_long, i32, ll, vp, vp, fp, vp]
    lib.mvf_head_train_bwd.restype = i32
    lib.mvf_head_train_bwd.argtypes = [fp, fp, fp, fp, i32, i32, i32, i32, i32, fp, fp, fp, vp, i32, vp]
    lib.mvf_conv2d_wgrad_workspace_bytes.restype = sz
    lib.mvf_conv2d_wgrad_workspace_bytes.argtypes = [cp]
    lib.mvf_conv2d_nhwc_wgrad.restype = i32
    lib.mvf_conv2d_nhwc_wgrad.argtypes = [cp, vp, vp, vp, i32, i32, i32, i32, fp, vp, sz, vp]
    lib.mvf_conv2d_nhwc_wgrad_wgs.restype = i32
    lib.mvf_conv2d_nhwc_wgrad_wgs.argtypes = [cp, vp, vp, vp, i32, i32, i32, i32, fp, vp, sz, i32, vp]
    lib.mvf_conv2d_wgrad_last_launch.restype = i32
    lib.mvf_conv2d_wgrad_last_launch.argtypes = [C.POINTER(WgradLaunchInfo)]
    lib.mvf_pack_conv_weight_dgrad.restype = i32
    lib.mvf_pack_conv_weight_dgrad.argtypes = [fp, i32, i32, i32, i32, vp, i32, vp]
    lib.mvf_nhwc_stencil.restype = i32
    lib.mvf_nhwc_stencil.argtypes = [dp, vp, i32, vp, i32, fp, fp, fp, fp, fp, i32, vp, i32, vp, vp]
    lib.mvf_nhwc_tapgrad_workspace_bytes.restype = sz
    lib.mvf_nhwc_tapgrad_workspace_bytes.argtypes = [dp]
    lib.mvf_nhwc_tapgrad.restype = i32
    lib.mvf_nhwc_tapgrad.argtypes = [dp, vp, i32, vp, i32, fp, fp, fp, vp, sz, vp]
    lib.mvf_nhwc_stencil_last_launch.restype = i32
    lib.mvf_nhwc_stencil_last_launch.argtypes = [C.POINTER(StencilLaunchInfo)]
    lib.mvf_nhwc_tapgrad_last_launch.restype = i32
    lib.mvf_nhwc_tapgrad_last_launch.argtypes = [C.POINTER(TapgradLaunchInfo)]
    lib.mvf_sgd_workspace_bytes.restype = sz
    lib.mvf_sgd_workspace_bytes.argtypes = [i64]
    lib.mvf_sgd_nesterov_step.restype = i32
    lib.mvf_sgd_nesterov_step.argtypes = [fp, fp, fp, i64, f32, f32, f32, f32, f32, i32, fp, vp, sz, vp]
    lib.mvf_sgd_step_segments.restype = i32
    lib.mvf_sgd_step_segments.argtypes = [fp, fp, fp, i64, f32, f32, f32, f32, f32, i32, i32, vp, i32, fp, vp, sz, vp]
    lib.mvf_grad_accumulate.restype = i32
    lib.mvf_grad_accumulate.argtypes = [fp, fp, i64, i32, vp]
    lib.mvf_sgd_nesterov_step_ema.restype = i32
    lib.mvf_sgd_nesterov_step_ema.argtypes = [fp, fp, fp, i64, f32, f32, f32, f32, f32, i32, fp, f32, fp, vp, sz, vp]
    lib.mvf_sgd_step_segments_ema.restype = i32
    lib.mvf_sgd_step_segments_ema.argtypes = [fp, fp, fp, i64, f32, f32, f32, f32, f32, i32, i32, vp, i32, fp, f32, fp, vp, sz, vp]
    lib.mvf_ema_update.restype = i32
    lib.mvf_ema_update.argtypes = [fp, fp, i64, f32, vp]
    lib.mvf_ema_swap.restype = i32
    lib.mvf_ema_swap.argtypes = [fp, fp, i64, vp]
    lib.mvf_bn_stats_accumulate.restype = i32
    lib.mvf_bn_stats_accumulate.argtypes = [vp, i32, i64, vp, vp]
    lib.mvf_bn_stats_finalize.restype = i32
    lib.mvf_bn_stats_finalize.argtypes = [vp, i32, i64, vp, i64, fp, vp]
    lib.mvf_bn_stats_exchange.restype = i32
    lib.mvf_bn_stats_exchange.argtypes = [vp, i32, i64, fp, i32, vp]
    lib.mvf_sgd_step_guarded.restype = i32
    lib.mvf_sgd_step_guarded.argtypes = [fp, fp, fp, i64, f32, f32, f32, f32, f32, i32, i32, vp, i32, fp, f32, vp, fp, vp, sz, vp]
    lib.mvf_bn_stats_snapshot.restype = i32
    lib.mvf_bn_stats_snapshot.argtypes = [vp, i32, i64, fp, vp, i64, vp, vp]
    lib.mvf_bn_stats_restore.restype = i32
    lib.mvf_bn_stats_restore.argtypes = [vp, i32, i64, fp, vp, i64, vp, vp, vp]
    lib.mvf_adamw_workspace_bytes.restype = sz
    lib.mvf_adamw_workspace_bytes.argtypes = [i64]
    lib.mvf_adamw_step.restype = i32
    lib.mvf_adamw_step.argtypes = [fp, fp, fp, fp, i64, f32, f32, C.POINTER(AdamwHyper), vp, i32, fp, f32, vp, vp, fp, vp, sz, vp]
    lib.mvf_lamb_workspace_bytes.restype = sz
    lib.mvf_lamb_workspace_bytes.argtypes = [i64, i32]
    lib.mvf_lamb_step.restype = i32
    lib.mvf_lamb_step.argtypes = [fp, fp, fp, fp, i64, f32, f32, C.POINTER(LambHyper), vp, i32, fp, f32, vp, vp, fp, fp, vp, sz, vp]
    lib.mvf_metrics_state_words.restype = sz
    lib.mvf_metrics_state_words.argtypes = [i32, i32]
    lib.mvf_metrics_update.restype = i32
    lib.mvf_metrics_update.argtypes = [fp, i32, i32, ll, vp, i32, ll, i32, vp, vp, vp]
    lib.mvf_flat_stats_workspace_bytes.restype = sz
    lib.mvf_flat_stats_workspace_bytes.argtypes = [i64, i32]
    lib.mvf_flat_segment_stats.restype = i32
    lib.mvf_flat_segment_stats.argtypes = [fp, fp, i64, vp, i32, vp, vp, vp, vp, sz, vp]
    lib.mvf_bn_stats_nonfinite.restype = i32
    lib.mvf_bn_stats_nonfinite.argtypes = [vp, i32, i64, vp, vp, vp]
    lib.mvf_plan_run.restype = i32
    lib.mvf_plan_run.argtypes = [C.POINTER(PlanOp), i32, C.POINTER(C.c_ulonglong), C.POINTER(C.c_float), C.POINTER(C.c_int)]
    # Callers pass device pointers as plain Python ints (train_engine._p): without declared argtypes ctypes would truncate them to c_int silently.  Every
    # function the header declares must therefore have its signature declared above.
    missing = [n for n in declared_symbols() if hasattr(lib, n) and getattr(lib, n).argtypes is None]
    if missing:
        raise ImportError("mvfnet_amd._lib: no argtypes declared for %s" % missing)
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = lib.mvf_last_error().decode("utf-8", "replace")
        raise RuntimeError("%s failed: %s (%s)" % (what or "libmvfnet_hip", ERRNAMES.get(rc, rc), msg))


def declared_symbols():
    """Every function name declared in include/mvfnet_hip.h (parsed; used by the symbol-export test)."""
    import re
    hdr = os.path.join(os.path.dirname(_HERE), "include", "mvfnet_hip.h")
    txt = open(hdr).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b((?:mvf|mvfnet)_[a-z0-9_]+)\s*\(", txt)))


lib = _load()
