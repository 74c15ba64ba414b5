"""ctypes binding of libaxvs.so (C-ABI declared in include/axvs.h).

There is no CPU or PyTorch fallback: if the HIP library is missing, importing succeeds but the
first call raises, loudly.  Build it with ``python -c "import __graft_entry__ as g; g.build()"``.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# AXVS_LIB_PATH: diagnostic builds of the same library (tools/ only: -DAXVS_STAMPS, ablations)
LIB_PATH = os.environ.get("AXVS_LIB_PATH") or os.path.join(_HERE, "libaxvs.so")

AXVS_F16 = 0
AXVS_BF16 = 1
AXVS_F32 = 2      # fp32 / uint8 inputs: only where an entry point says so (axvs_video_matcher)
AXVS_U8 = 3
DTYPES = {"f16": AXVS_F16, "fp16": AXVS_F16, "float16": AXVS_F16, "bf16": AXVS_BF16, "bfloat16": AXVS_BF16}

_fp = C.c_void_p  # device pointers travel as integers


class AxvsTrajParams(C.Structure):
    _fields_ = [(n, _fp) for n in ("q_w", "q_b", "k_w", "k_b", "v_w", "v_b", "proj_q_w", "proj_q_b",
                                   "proj_kv_w", "proj_kv_b", "proj_w", "proj_b")]


class AxvsAxialLayerParams(C.Structure):
    _fields_ = [("height_attn", AxvsTrajParams), ("width_attn", AxvsTrajParams)] + \
               [(n, _fp) for n in ("norm1_w", "norm1_b", "linear1_w", "linear1_b", "linear2_w", "linear2_b",
                                   "norm2_w", "norm2_b")]


class AxvsTrajLayerParams(C.Structure):
    _fields_ = [("temporal_attn", AxvsTrajParams)] + [(n, _fp) for n in ("norm1_w", "norm1_b", "linear1_w", "linear1_b", "linear2_w",
                                                                          "linear2_b", "norm2_w", "norm2_b")]


class AxvsSinePos3D(C.Structure):
    _fields_ = [("temperature", C.c_float), ("normalize", C.c_int), ("scale", C.c_float), ("level_embed", _fp)]


class AxvsBN(C.Structure):
    _fields_ = [(n, _fp) for n in ("w", "b", "mean", "var")]


class AxvsCCLayerParams(C.Structure):
    _fields_ = [("attn", AxvsTrajParams), ("norm_w", _fp), ("norm_b", _fp), ("aspp_w", _fp * 3), ("aspp_b", _fp * 3),
                ("aspp_proj_w", _fp), ("aspp_norm_w", _fp), ("aspp_norm_b", _fp), ("conv_norm_w", _fp), ("conv_norm_b", _fp)]


class AxvsCCHeadParams(C.Structure):
    _fields_ = [("class_proj_w", _fp), ("class_proj_bn", AxvsBN), ("mask_proj_w", _fp), ("mask_proj_bn", AxvsBN),
                ("mask_head_w", _fp), ("mask_head_bn", AxvsBN), ("class_head_w", _fp), ("class_head_b", _fp),
                ("act_head_w", _fp), ("act_head_b", _fp), ("pixel_bn", AxvsBN)]


class AxvsBNGrads(C.Structure):
    _fields_ = [("w", _fp), ("b", _fp)]


class AxvsCCHeadGrads(C.Structure):
    _fields_ = [("class_proj_w", _fp), ("class_proj_bn", AxvsBNGrads), ("mask_proj_w", _fp), ("mask_proj_bn", AxvsBNGrads),
                ("mask_head_w", _fp), ("mask_head_bn", AxvsBNGrads), ("class_head_w", _fp), ("class_head_b", _fp),
                ("act_head_w", _fp), ("act_head_b", _fp), ("pixel_bn", AxvsBNGrads)]


class AxvsPanopticCfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("N", "K1", "T", "h", "w", "image_h", "image_w", "two_stage", "crop_h", "crop_w", "H", "W",
                                       "align_corners", "label_divisor")] + \
               [(n, C.c_double) for n in ("pixel_confidence_threshold", "overlap_threshold", "class_threshold_thing", "class_threshold_stuff",
                                          "reorder_class_weight", "reorder_mask_weight")]


class AxvsVisCfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("Q", "K1", "T", "num_frames", "h", "w", "image_h", "image_w", "crop_h", "crop_w", "H", "W", "num_things",
                                       "k_cand", "k_out", "mask_bits")]


class AxvsTLLossCfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("L", "B", "Q", "K1", "T", "h", "w", "Hg", "Wg", "num_points", "num_cand", "num_kept", "target_dtype")] + \
               [(n, C.c_float) for n in ("cost_cls", "cost_mask", "cost_dice", "loss_cls", "loss_mask", "loss_dice", "dice_eps")]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


class AxvsCCTrainCfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("B", "Q", "Tc", "V", "H", "W", "K1", "num_layers")] + \
               [("rates", C.c_int * 3), ("p_attn_drop", C.c_float), ("p_aspp_drop", C.c_float), ("seed", C.c_uint),
                ("allreduce", ALLREDUCE_FN), ("allreduce_user", C.c_void_p), ("chain_only", C.c_int)]


class AxvsTLHeadParams(C.Structure):
    _fields_ = [(n, _fp) for n in ("post_norm_w", "post_norm_b", "activation_proj_w", "activation_proj_b", "cls_embed_w",
                                   "cls_embed_b")] + [("mask_embed_w", _fp * 3), ("mask_embed_b", _fp * 3)]


class AxvsTLHeadGrads(C.Structure):      # field order of AxvsTLHeadParams
    _fields_ = AxvsTLHeadParams._fields_


class AxvsTLHeadTrainCfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("B", "Q", "Tc", "frames_per_clip", "h", "w", "K1", "Cm", "num_layers")]


class AxvsM2fLayerParams(C.Structure):
    _fields_ = [(n, _fp) for n in ("cross_in_w", "cross_in_b", "cross_out_w", "cross_out_b", "norm0_w", "norm0_b", "self_in_w", "self_in_b",
                                   "self_out_w", "self_out_b", "norm1_w", "norm1_b", "ffn1_w", "ffn1_b", "ffn2_w", "ffn2_b", "norm2_w", "norm2_b")]


class AxvsM2fHeadParams(C.Structure):
    _fields_ = [(n, _fp) for n in ("post_norm_w", "post_norm_b", "query_embed", "query_feat", "level_embed")] + \
               [("mask_embed_w", _fp * 3), ("mask_embed_b", _fp * 3), ("cls_embed_w", _fp), ("cls_embed_b", _fp)]


class AxvsM2fCfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("N", "Q", "T", "C", "heads", "ffn", "num_layers", "num_levels", "K1", "h", "w")] + \
               [("lh", C.c_int * 3), ("lw", C.c_int * 3), ("return_predictions", C.c_int), ("pos_normalize", C.c_int),
                ("pos_temperature", C.c_float), ("pos_scale", C.c_float)]


KMAX_PREDICTOR_FIELDS = ("dw_w", "dw_b", "ph1_w", "ph1_b", "ph2_w", "ph2_b", "mh_w", "mh_b", "cls_w", "cls_b", "mask_ab")
KMAX_LAYER_FIELDS = (("pix1_w", "pix1_b", "q1_w", "q1_b") + tuple("pred." + n for n in KMAX_PREDICTOR_FIELDS)
                     + ("kv_w", "kv_b", "k3_w", "k3_b", "qkv_w", "qkv_b", "sim_ab", "rv_ab", "a3_w", "a3_b", "f1_w", "f1_b", "f2_w", "f2_b"))
KMAX_HEAD_FIELDS = ("centers", "cep_w", "cep_b", "mep_w", "mep_b") + tuple("pred." + n for n in KMAX_PREDICTOR_FIELDS)


class AxvsKmaxLayerParams(C.Structure):      # (the nested predictor struct is all pointers: flat here, "pred." -> "pred_")
    _fields_ = [(n.replace(".", "_"), _fp) for n in KMAX_LAYER_FIELDS]


class AxvsKmaxHeadParams(C.Structure):
    _fields_ = [(n.replace(".", "_"), _fp) for n in KMAX_HEAD_FIELDS]


class AxvsKmaxCfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("B", "T", "L", "K1", "num_layers")] + \
               [("layer_level", C.c_int * 16), ("in_channels", C.c_int * 3), ("h", C.c_int * 3), ("w", C.c_int * 3)] + \
               [(n, C.c_int) for n in ("pan_channels", "H", "W", "heads", "base_filters", "want_masks", "want_pixel_feature")]


KPIX_AXIS_FIELDS = ("qkv_w", "qkv_b", "eq", "ek", "ev", "sim_a", "out_ab")
KPIX_BLOCK_FIELDS = (("sc_w", "sc_b", "c1_w", "c1_b", "c2_w", "c2_b") + tuple("height." + n for n in KPIX_AXIS_FIELDS)
                     + tuple("width." + n for n in KPIX_AXIS_FIELDS) + ("c3_w", "c3_b"))
KPIX_FUSE_FIELDS = ("ln_w", "ln_b", "low_w", "low_b", "high_w", "high_b")


class AxvsKpixBlockParams(C.Structure):      # (the nested axis structs are all pointers: flat here, "height." -> "height_")
    _fields_ = [(n.replace(".", "_"), _fp) for n in KPIX_BLOCK_FIELDS]


class AxvsKpixFuseParams(C.Structure):
    _fields_ = [(n, _fp) for n in KPIX_FUSE_FIELDS]


class AxvsKpixCfg(C.Structure):
    _fields_ = [("N", C.c_int)] + [(n, C.c_int * 4) for n in ("in_channels", "h", "w", "base", "blocks", "axial")] + [("heads", C.c_int)]


CNX_DOWN_FIELDS = ("ln_w", "ln_b", "w", "b")
CNX_BLOCK_FIELDS = ("dw_w", "dw_b", "ln_w", "ln_b", "w1", "b1", "w2", "b2", "grn_gamma")


class AxvsCnxDownParams(C.Structure):
    _fields_ = [(n, _fp) for n in CNX_DOWN_FIELDS]


class AxvsCnxBlockParams(C.Structure):
    _fields_ = [(n, _fp) for n in CNX_BLOCK_FIELDS]


class AxvsCnxCfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("N", "H", "W")] + [(n, C.c_int * 4) for n in ("dims", "depths", "h", "w")] + [("v2", C.c_int)]


RN_STEM_FIELDS = ("w", "b")
RN_BLOCK_FIELDS = ("w1", "b1", "w2", "b2", "w3", "b3", "ws", "bs")


class AxvsRnStemParams(C.Structure):
    _fields_ = [(n, _fp) for n in RN_STEM_FIELDS]


class AxvsRnBlockParams(C.Structure):
    _fields_ = [(n, _fp) for n in RN_BLOCK_FIELDS]


class AxvsRnCfg(C.Structure):
    _fields_ = ([(n, C.c_int) for n in ("N", "H", "W", "in_channels", "stem_channels")]
                + [(n, C.c_int * 4) for n in ("width", "out_channels", "blocks", "stride", "dilation", "h", "w")] + [("stride_in_1x1", C.c_int)])


class AxvsMsdaParams(C.Structure):
    _fields_ = [(n, _fp) for n in ("value_proj_w", "value_proj_b", "sampling_offsets_w", "sampling_offsets_b",
                                   "attention_weights_w", "attention_weights_b", "output_proj_w", "output_proj_b")]


class AxvsMsdaLayerParams(C.Structure):
    _fields_ = [("self_attn", AxvsMsdaParams)] + [(n, _fp) for n in ("norm1_w", "norm1_b", "linear1_w", "linear1_b", "linear2_w",
                                                                      "linear2_b", "norm2_w", "norm2_b")]


class AxvsConvGnParams(C.Structure):
    _fields_ = [(n, _fp) for n in ("conv_w", "conv_b", "gn_w", "gn_b")]


class AxvsFfnParams(C.Structure):
    _fields_ = [(n, _fp) for n in ("norm1_w", "norm1_b", "linear1_w", "linear1_b", "linear2_w", "linear2_b", "norm2_w", "norm2_b")]


class AxvsFpnLevelParams(C.Structure):
    _fields_ = [(n, _fp) for n in ("lateral_w", "lateral_gn_w", "lateral_gn_b", "output_w", "output_gn_w", "output_gn_b", "mask_w", "mask_b")]


def ptrs(ts) -> C.Array:
    """Host array of the tensors' device pointers (NULL for None): what an entry point takes as `const T* const*`."""
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def fill(cls, ptrs):
    """A `cls` with `ptrs` assigned to its fields in declaration order: a nested Structure is filled recursively, a ctypes array takes
    as many pointers as it has elements.  A gradient struct has its parameter struct's layout (include/axvs.h), so this fills both."""
    ptrs = list(ptrs)
    s, n = _fill(cls, ptrs, 0)
    if n != len(ptrs):
        raise ValueError(f"{cls.__name__} takes {n} pointers, got {len(ptrs)}")
    return s


def _fill(cls, ptrs, i):
    s = cls()
    for name, t in cls._fields_:
        if issubclass(t, C.Structure):
            v, i = _fill(t, ptrs, i)
        elif issubclass(t, C.Array):
            v, i = t(*ptrs[i:i + t._length_]), i + t._length_
        else:
            v, i = (ptrs[i] if i < len(ptrs) else None), i + 1      # (too few pointers: counted to the end, refused by fill)
        setattr(s, name, v)
    return s, i


class AxvsTestGemm(C.Structure):      # test hook (include/axvs.h): one call of the training tier's GEMM dispatch
    _fields_ = [("op", C.c_int), ("a", _fp), ("b", _fp), ("c", _fp), ("M", C.c_longlong), ("N", C.c_int), ("K", C.c_int),
                ("lda", C.c_longlong), ("ldb", C.c_longlong), ("ldc", C.c_longlong), ("al_a", C.c_int), ("al_b", C.c_int), ("al_c", C.c_int),
                ("a2", _fp), ("aff", _fp), ("aff_rows", C.c_int), ("ksteps", C.c_int), ("zsplits", C.c_int), ("bias", _fp), ("mul", C.c_float),
                ("relu", C.c_int), ("drop_seed", C.c_uint), ("drop_site", C.c_uint), ("drop_thr", C.c_uint), ("drop_scale", C.c_float),
                ("beta", C.c_float), ("res", _fp), ("res2", _fp), ("out16", _fp), ("kind16", C.c_int), ("zero_rows", _fp), ("db", _fp),
                ("exact", C.c_int), ("stat_part", _fp), ("stat_shift", _fp), ("stat_nblk", C.c_int), ("stat_blk0", C.c_int),
                ("stat_rows", C.c_int), ("grp_rows", C.c_int), ("grp_ld", C.c_longlong), ("variant", C.c_int)]


TEST_GEMM_OPS = {"nt": 0, "fwd": 1, "wgrad": 2, "dgrad": 3, "tn_direct": 4}


# name -> (restype, argtypes); must list every symbol of include/axvs.h
SIGNATURES = {
    "axvs_version": (C.c_int, []),
    "axvs_has_bf16": (C.c_int, []),
    "axvs_last_error": (C.c_char_p, []),
    "axvs_set_status_buffer": (C.c_int, [_fp]),
    "axvs_check_status": (C.c_int, []),
    "axvs_set_sync_buffer": (C.c_int, [_fp, C.c_size_t]),
    "axvs_profile_stages": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "axvs_profile_stage_count": (C.c_int, []),
    "axvs_profile_stage_name": (C.c_char_p, [C.c_int]),
    "axvs_set_option": (C.c_int, [C.c_char_p, C.c_int]),
    "axvs_plan_regular_tiles": (C.c_int, []),
    "axvs_traj_packed_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "axvs_traj_pack": (C.c_int, [C.POINTER(AxvsTrajParams), _fp, C.c_int, C.c_int, C.c_int, _fp]),
    "axvs_axial_layer_packed_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "axvs_axial_layer_pack": (C.c_int, [C.POINTER(AxvsAxialLayerParams), _fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "axvs_traj_attn_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "axvs_traj_attn_fwd": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _fp] + [C.c_int] * 6 + [_fp, C.c_size_t, _fp]),
    "axvs_axial_layer_workspace_bytes": (C.c_size_t, [C.c_int] * 7),
    "axvs_axial_layer_fwd": (C.c_int, [_fp, _fp, _fp, _fp] + [C.c_int] * 8 + [_fp, C.c_size_t, _fp, _fp, _fp]),
    "axvs_traj_layer_packed_bytes": (C.c_size_t, [C.c_int] * 3),
    "axvs_traj_layer_pack": (C.c_int, [C.POINTER(AxvsTrajLayerParams), _fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "axvs_traj_layer_workspace_bytes": (C.c_size_t, [C.c_int] * 6),
    "axvs_traj_layer_fwd": (C.c_int, [_fp, _fp, _fp, _fp] + [C.c_int] * 7 + [_fp, C.c_size_t, _fp]),
    "axvs_axial_layer_train_saved_bytes": (C.c_size_t, [C.c_int] * 7),
    "axvs_axial_layer_train_scratch_bytes": (C.c_size_t, [C.c_int] * 8),
    "axvs_axial_layer_train_fwd": (C.c_int, [_fp, _fp, _fp, C.POINTER(AxvsAxialLayerParams)] + [C.c_int] * 7 +
                                   [C.c_float, C.c_float, C.c_uint, _fp, C.c_size_t, _fp, C.c_size_t, _fp]),
    "axvs_axial_layer_train_bwd": (C.c_int, [_fp, _fp, _fp, C.POINTER(AxvsAxialLayerParams), C.POINTER(AxvsAxialLayerParams), _fp, _fp] +
                                   [C.c_int] * 7 + [C.c_float, C.c_float, C.c_uint, C.c_int, _fp, C.c_size_t, _fp, C.c_size_t, _fp]),
    "axvs_traj_layer_train_saved_bytes": (C.c_size_t, [C.c_int] * 6),
    "axvs_traj_layer_train_scratch_bytes": (C.c_size_t, [C.c_int] * 7),
    "axvs_traj_layer_train_fwd": (C.c_int, [_fp, _fp, _fp, C.POINTER(AxvsTrajLayerParams)] + [C.c_int] * 6 +
                                  [C.c_float, C.c_float, C.c_uint, _fp, C.c_size_t, _fp, C.c_size_t, _fp]),
    "axvs_traj_layer_train_bwd": (C.c_int, [_fp, _fp, _fp, C.POINTER(AxvsTrajLayerParams), C.POINTER(AxvsTrajLayerParams), _fp, _fp] +
                                  [C.c_int] * 6 + [C.c_float, C.c_float, C.c_uint, C.c_int, _fp, C.c_size_t, _fp, C.c_size_t, _fp]),
    "axvs_cc_module_train_saved_bytes": (C.c_size_t, [C.POINTER(AxvsCCTrainCfg)]),
    "axvs_cc_module_train_scratch_bytes": (C.c_size_t, [C.POINTER(AxvsCCTrainCfg), C.c_int]),
    "axvs_cc_module_train_bn_stats_floats": (C.c_size_t, [C.POINTER(AxvsCCTrainCfg)]),
    "axvs_cc_module_train_fwd": (C.c_int, [_fp] * 5 + [C.POINTER(AxvsCCLayerParams), C.POINTER(AxvsCCHeadParams), C.POINTER(AxvsCCTrainCfg),
                                           _fp, C.c_size_t, _fp, C.c_size_t, _fp]),
    "axvs_cc_module_train_bwd": (C.c_int, [_fp] * 4 + [C.POINTER(AxvsCCLayerParams), C.POINTER(AxvsCCHeadParams), C.POINTER(AxvsCCLayerParams),
                                           C.POINTER(AxvsCCHeadGrads), _fp, C.POINTER(AxvsCCTrainCfg), _fp, C.c_size_t, _fp, C.c_size_t, _fp]),
    "axvs_cc_layers_train_fwd": (C.c_int, [_fp, _fp, C.POINTER(AxvsCCLayerParams), C.POINTER(AxvsCCTrainCfg), _fp, C.c_size_t, _fp, C.c_size_t, _fp]),
    "axvs_cc_layers_train_bwd": (C.c_int, [_fp, _fp, C.POINTER(AxvsCCLayerParams), C.POINTER(AxvsCCLayerParams), _fp, C.POINTER(AxvsCCTrainCfg),
                                           _fp, C.c_size_t, _fp, C.c_size_t, _fp]),
    "axvs_axial_pass_fwd": (C.c_int, [_fp, _fp, _fp, _fp] + [C.c_int] * 9 + [_fp, C.c_size_t, _fp]),
    "axvs_axial_layer_workspace_bytes_ex": (C.c_size_t, [C.c_int] * 9),
    "axvs_axial_layer_sine3d_workspace_bytes": (C.c_size_t, [C.c_int] * 7),
    "axvs_axial_layer_fwd_sine3d": (C.c_int, [_fp, C.POINTER(AxvsSinePos3D), _fp, _fp] + [C.c_int] * 8 + [_fp, C.c_size_t, _fp, _fp, _fp]),
    "axvs_axial_layer_strided_ok": (C.c_int, [C.c_int] * 3),
    "axvs_axial_layer_workspace_bytes_strided": (C.c_size_t, [C.c_int] * 7 + [C.c_longlong]),
    "axvs_axial_layer_fwd_sine3d_strided": (C.c_int, [_fp, C.POINTER(AxvsSinePos3D), _fp, _fp] + [C.c_int] * 8 + [C.c_longlong, _fp, C.c_size_t, _fp]),
    "axvs_ffn_workspace_bytes": (C.c_size_t, [C.c_longlong, C.c_int, C.c_int]),
    "axvs_ffn_fwd": (C.c_int, [_fp, _fp, _fp, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, _fp, C.c_size_t, _fp]),
    "axvs_cc_layer_packed_bytes": (C.c_size_t, []),
    "axvs_cc_layer_pack": (C.c_int, [C.POINTER(AxvsCCLayerParams), _fp, C.c_int, _fp]),
    "axvs_cc_layer_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "axvs_cc_layer_fwd": (C.c_int, [_fp, _fp, _fp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _fp, C.c_size_t, _fp]),
    "axvs_cc_heads_packed_bytes": (C.c_size_t, [C.c_int]),
    "axvs_cc_heads_pack": (C.c_int, [C.POINTER(AxvsCCHeadParams), _fp, C.c_int, C.c_int, _fp]),
    "axvs_cc_heads_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "axvs_cc_heads_fwd": (C.c_int, [_fp, _fp, _fp, _fp, _fp] + [C.c_int] * 8 + [_fp, C.c_size_t, _fp]),
    "axvs_ffn_packed_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "axvs_ffn_pack": (C.c_int, [C.POINTER(AxvsFfnParams), _fp, C.c_int, C.c_int, C.c_int, _fp]),
    "axvs_ffn_packed_fwd": (C.c_int, [_fp, _fp, _fp, C.c_longlong, C.c_int, C.c_int, C.c_int, _fp, C.c_size_t, _fp]),
    "axvs_fpn_level_packed_bytes": (C.c_size_t, [C.c_int] * 3),
    "axvs_fpn_level_pack": (C.c_int, [C.POINTER(AxvsFpnLevelParams), _fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "axvs_fpn_level_workspace_bytes": (C.c_size_t, [C.c_int] * 6),
    "axvs_fpn_level_fwd": (C.c_int, [_fp, _fp, C.c_longlong, C.c_longlong, C.c_int, C.c_int, _fp, _fp, _fp] + [C.c_int] * 7 +
                           [C.c_float, C.c_int, _fp, C.c_size_t, _fp]),
    "axvs_conv1x1_gn_packed_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "axvs_conv1x1_gn_pack": (C.c_int, [C.POINTER(AxvsConvGnParams), _fp, C.c_int, C.c_int, C.c_int, _fp]),
    "axvs_conv1x1_gn_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "axvs_conv1x1_gn_fwd": (C.c_int, [_fp, C.c_int, C.c_longlong, C.c_longlong, _fp, C.c_int, C.c_longlong, C.c_longlong, _fp] +
                            [C.c_int] * 5 + [C.c_float, C.c_int, _fp, C.c_size_t, _fp]),
    "axvs_conv1x1_gn_train_saved_bytes": (C.c_size_t, [C.c_int] * 6 + [C.c_longlong, C.c_longlong]),
    "axvs_conv1x1_gn_train_scratch_bytes": (C.c_size_t, [C.c_int] * 6),
    "axvs_conv1x1_gn_train_fwd": (C.c_int, [_fp, C.c_int, C.c_longlong, C.c_longlong, _fp, C.c_int, C.c_longlong, C.c_longlong, C.POINTER(AxvsConvGnParams)] +
                                  [C.c_int] * 5 + [C.c_float, _fp, C.c_size_t, _fp, C.c_size_t, _fp]),
    "axvs_conv1x1_gn_train_bwd": (C.c_int, [_fp, C.c_int, C.c_longlong, C.c_longlong, _fp, C.c_int, C.c_longlong, C.c_longlong, C.POINTER(AxvsConvGnParams),
                                            C.POINTER(AxvsConvGnParams), _fp] + [C.c_int] * 5 + [_fp, C.c_size_t, _fp, C.c_size_t, _fp]),
    "axvs_linear_sum_assignment": (C.c_int, [_fp, _fp, C.c_int, C.c_int, _fp]),
    "axvs_match_embds_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "axvs_match_embds": (C.c_int, [_fp, _fp, _fp, C.c_int, C.c_int, _fp, C.c_size_t, _fp]),
    "axvs_match_clips_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "axvs_match_clips": (C.c_int, [_fp, _fp] + [C.c_int] * 4 + [_fp, C.c_size_t, _fp]),
    "axvs_linear_sum_assignment_rect": (C.c_int, [_fp, C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_int), _fp, _fp, C.c_int, _fp]),
    "axvs_video_matcher_workspace_bytes": (C.c_size_t, [C.c_int] * 4 + [C.c_longlong]),
    "axvs_video_matcher": (C.c_int, [C.POINTER(_fp), C.c_int, C.POINTER(_fp), _fp, C.c_int, _fp, C.POINTER(C.c_int)] + [C.c_int] * 4 +
                           [C.c_longlong, C.c_int, C.c_int] + [_fp] * 5 + [_fp, C.c_size_t, _fp]),
    "axvs_set_criterion_saved_bytes": (C.c_size_t, [C.c_int] * 3),
    "axvs_set_criterion_workspace_bytes": (C.c_size_t, [C.c_int] * 4 + [C.c_longlong]),
    "axvs_set_criterion_fwd": (C.c_int, [C.POINTER(_fp), C.POINTER(_fp), _fp, C.c_int, _fp, C.POINTER(C.c_int)] + [_fp] * 4 + [C.c_int] * 5 +
                               [C.c_longlong, C.c_int, C.c_int, _fp, _fp, _fp, C.c_longlong, _fp]),
    "axvs_set_criterion_bwd": (C.c_int, [_fp, C.POINTER(_fp), C.POINTER(_fp), _fp, C.c_int, C.POINTER(C.c_int)] + [C.c_int] * 4 +
                               [C.c_longlong, C.c_int, C.c_int, _fp, C.POINTER(_fp), C.POINTER(_fp), _fp]),
    "axvs_tl_loss_saved_bytes": (C.c_size_t, [C.POINTER(AxvsTLLossCfg), C.POINTER(C.c_int)]),
    "axvs_tl_loss_workspace_bytes": (C.c_size_t, [C.POINTER(AxvsTLLossCfg), C.POINTER(C.c_int)]),
    "axvs_tl_loss_fwd": (C.c_int, [C.POINTER(AxvsTLLossCfg), C.POINTER(_fp), C.POINTER(_fp), _fp, _fp, C.POINTER(C.c_int)] + [_fp] * 12 +
                         [C.c_longlong, _fp]),
    "axvs_tl_loss_bwd": (C.c_int, [C.POINTER(AxvsTLLossCfg), _fp, C.POINTER(_fp), C.POINTER(_fp), _fp, C.POINTER(C.c_int), _fp, _fp, _fp,
                                   C.POINTER(_fp), C.POINTER(_fp), _fp]),
    "axvs_pixel_sample": (C.c_int, [_fp, C.c_int, C.POINTER(C.c_int), _fp] + [C.c_int] * 4 + [C.c_longlong, C.POINTER(_fp), C.POINTER(C.c_int),
                                    C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_int, _fp, _fp, _fp, C.c_int, _fp]),
    "axvs_pixel_insdis_saved_bytes": (C.c_size_t, [C.c_int] * 3),
    "axvs_pixel_insdis_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "axvs_pixel_insdis_fwd": (C.c_int, [C.POINTER(_fp), _fp, C.c_int, C.POINTER(C.c_int), _fp] + [C.c_int] * 6 + [C.c_longlong, _fp, C.c_int, C.c_int,
                                        _fp, _fp, _fp, C.c_longlong, _fp]),
    "axvs_pixel_insdis_bwd": (C.c_int, [_fp, C.POINTER(_fp), _fp, C.c_int, C.POINTER(C.c_int), _fp] + [C.c_int] * 6 + [C.c_longlong, _fp, C.c_int,
                                        C.c_int, _fp, C.POINTER(_fp), _fp, C.c_longlong, _fp]),
    "axvs_pixel_semantic_saved_bytes": (C.c_size_t, [C.c_int] * 2),
    "axvs_pixel_semantic_fwd": (C.c_int, [_fp, _fp, _fp] + [C.c_int] * 4 + [C.c_longlong, C.c_int, _fp, _fp, _fp]),
    "axvs_pixel_semantic_bwd": (C.c_int, [_fp, _fp, _fp, _fp] + [C.c_int] * 4 + [C.c_longlong, C.c_int, _fp, _fp, _fp]),
    "axvs_video_panoptic_workspace_bytes": (C.c_size_t, [C.POINTER(AxvsPanopticCfg)]),
    "axvs_video_panoptic_table_ints": (C.c_size_t, [C.c_int]),
    "axvs_video_panoptic_fwd": (C.c_int, [C.POINTER(AxvsPanopticCfg), _fp, _fp, C.c_int] + [_fp] * 6 + [C.c_longlong, _fp]),
    "axvs_video_instance_workspace_bytes": (C.c_size_t, [C.POINTER(AxvsVisCfg)]),
    "axvs_video_instance_fwd": (C.c_int, [C.POINTER(AxvsVisCfg), _fp, _fp, C.c_int] + [_fp] * 4 + [C.c_longlong, _fp]),
    "axvs_m2f_decoder_packed_bytes": (C.c_size_t, [C.POINTER(AxvsM2fCfg)]),
    "axvs_m2f_decoder_pack": (C.c_int, [C.POINTER(AxvsM2fLayerParams), C.POINTER(AxvsM2fHeadParams), C.POINTER(AxvsM2fCfg), _fp, _fp]),
    "axvs_m2f_decoder_workspace_bytes": (C.c_size_t, [C.POINTER(AxvsM2fCfg)]),
    "axvs_m2f_decoder_fwd": (C.c_int, [C.POINTER(AxvsM2fCfg), _fp, _fp, C.POINTER(_fp)] + [_fp] * 6 + [C.c_longlong, _fp]),
    "axvs_m2f_attn_mask_workspace_bytes": (C.c_size_t, [C.POINTER(AxvsM2fCfg), C.c_int]),
    "axvs_m2f_attn_mask_fwd": (C.c_int, [C.POINTER(AxvsM2fCfg), _fp, _fp, _fp, C.c_int, _fp, _fp, _fp, C.c_longlong, _fp]),
    "axvs_m2f_layer_workspace_bytes": (C.c_size_t, [C.POINTER(AxvsM2fCfg), C.c_int]),
    "axvs_m2f_layer_fwd": (C.c_int, [C.POINTER(AxvsM2fCfg), _fp, C.c_int] + [_fp] * 6 + [C.c_longlong, _fp]),
    "axvs_kmax_decoder_packed_bytes": (C.c_size_t, [C.POINTER(AxvsKmaxCfg)]),
    "axvs_kmax_decoder_pack": (C.c_int, [C.POINTER(AxvsKmaxLayerParams), C.POINTER(AxvsKmaxHeadParams), C.POINTER(AxvsKmaxCfg), _fp, _fp]),
    "axvs_kmax_decoder_workspace_bytes": (C.c_size_t, [C.POINTER(AxvsKmaxCfg)]),
    "axvs_kmax_decoder_fwd": (C.c_int, [C.POINTER(AxvsKmaxCfg), _fp, C.POINTER(_fp)] + [_fp] * 8 + [C.c_longlong, _fp]),
    "axvs_kmax_stage_workspace_bytes": (C.c_size_t, [C.POINTER(AxvsKmaxCfg), C.c_int, C.c_int]),
    "axvs_kmax_assign_fwd": (C.c_int, [C.POINTER(AxvsKmaxCfg), _fp, C.c_int] + [_fp] * 5 + [C.c_longlong, _fp]),
    "axvs_kmax_layer_fwd": (C.c_int, [C.POINTER(AxvsKmaxCfg), _fp, C.c_int] + [_fp] * 5 + [C.c_longlong, _fp]),
    "axvs_kmax_pix_packed_bytes": (C.c_size_t, [C.POINTER(AxvsKpixCfg)]),
    "axvs_kmax_pix_pack": (C.c_int, [C.POINTER(AxvsKpixBlockParams), C.POINTER(AxvsKpixFuseParams), _fp, _fp, C.POINTER(AxvsKpixCfg), _fp, _fp]),
    "axvs_kmax_pix_workspace_bytes": (C.c_size_t, [C.POINTER(AxvsKpixCfg)]),
    "axvs_kmax_pix_decoder_fwd": (C.c_int, [C.POINTER(AxvsKpixCfg), _fp, C.POINTER(_fp), C.POINTER(_fp), _fp, C.c_longlong, _fp]),
    "axvs_kmax_pix_axial_attn_fwd": (C.c_int, [C.POINTER(AxvsKpixCfg), _fp, C.c_int, C.c_int, _fp, _fp, _fp]),
    "axvs_kmax_pix_block_fwd": (C.c_int, [C.POINTER(AxvsKpixCfg), _fp, C.c_int, _fp, _fp, _fp, C.c_longlong, _fp]),
    "axvs_kmax_pix_fuse_fwd": (C.c_int, [C.POINTER(AxvsKpixCfg), _fp, C.c_int, _fp, _fp, _fp, _fp, C.c_longlong, _fp]),
    "axvs_cnx_packed_bytes": (C.c_size_t, [C.POINTER(AxvsCnxCfg)]),
    "axvs_cnx_pack": (C.c_int, [C.POINTER(AxvsCnxDownParams), C.POINTER(AxvsCnxBlockParams), C.POINTER(AxvsCnxCfg), _fp, _fp]),
    "axvs_cnx_workspace_bytes": (C.c_size_t, [C.POINTER(AxvsCnxCfg)]),
    "axvs_cnx_fwd": (C.c_int, [C.POINTER(AxvsCnxCfg), _fp, _fp, C.POINTER(_fp), _fp, C.c_longlong, _fp]),
    "axvs_cnx_stem_fwd": (C.c_int, [C.POINTER(AxvsCnxCfg), _fp, _fp, _fp, _fp, C.c_longlong, _fp]),
    "axvs_cnx_down_fwd": (C.c_int, [C.POINTER(AxvsCnxCfg), _fp, C.c_int, _fp, _fp, _fp, C.c_longlong, _fp]),
    "axvs_cnx_dwln_fwd": (C.c_int, [C.POINTER(AxvsCnxCfg), _fp, C.c_int, _fp, _fp, _fp]),
    "axvs_cnx_block_fwd": (C.c_int, [C.POINTER(AxvsCnxCfg), _fp, C.c_int, _fp, _fp, _fp, C.c_longlong, _fp]),
    "axvs_rn_packed_bytes": (C.c_size_t, [C.POINTER(AxvsRnCfg)]),
    "axvs_rn_pack": (C.c_int, [C.POINTER(AxvsRnStemParams), C.POINTER(AxvsRnBlockParams), C.POINTER(AxvsRnCfg), _fp, _fp]),
    "axvs_rn_workspace_bytes": (C.c_size_t, [C.POINTER(AxvsRnCfg)]),
    "axvs_rn_fwd": (C.c_int, [C.POINTER(AxvsRnCfg), _fp, _fp, C.POINTER(_fp), _fp, _fp, C.c_longlong]),      # (the workspace goes last)
    "axvs_rn_stem_fwd": (C.c_int, [C.POINTER(AxvsRnCfg), _fp, _fp, _fp, _fp]),
    "axvs_rn_conv3_fwd": (C.c_int, [C.POINTER(AxvsRnCfg), _fp, C.c_int, _fp, _fp, _fp]),
    "axvs_rn_block_fwd": (C.c_int, [C.POINTER(AxvsRnCfg), _fp, C.c_int, _fp, _fp, _fp, _fp, C.c_longlong]),
    "axvs_add_channel_vector": (C.c_int, [_fp, _fp, C.c_size_t, C.c_int, _fp]),
    "axvs_pos2d": (C.c_int, [_fp, _fp] + [C.c_int] * 4 + [C.c_longlong, C.c_longlong, C.c_float, C.c_int, C.c_float, _fp]),
    "axvs_msda_packed_bytes": (C.c_size_t, [C.c_int] * 4),
    "axvs_msda_pack": (C.c_int, [C.POINTER(AxvsMsdaParams), _fp] + [C.c_int] * 5 + [_fp]),
    "axvs_msda_workspace_bytes": (C.c_size_t, [C.c_int] * 7),
    "axvs_msda_fwd": (C.c_int, [_fp, _fp, C.c_int, _fp, _fp, C.POINTER(C.c_int), _fp, _fp] + [C.c_int] * 8 + [_fp, C.c_size_t, _fp]),
    "axvs_msda_sample_fwd": (C.c_int, [_fp, _fp, _fp, C.c_int, _fp, _fp, C.POINTER(C.c_int), _fp, _fp] + [C.c_int] * 8 + [_fp, C.c_size_t, _fp]),
    "axvs_msda_output_proj_fwd": (C.c_int, [_fp, _fp, _fp, _fp, C.c_longlong] + [C.c_int] * 5 + [_fp]),
    "axvs_msda_layer_packed_bytes": (C.c_size_t, [C.c_int] * 5),
    "axvs_msda_layer_pack": (C.c_int, [C.POINTER(AxvsMsdaLayerParams), _fp] + [C.c_int] * 6 + [_fp]),
    "axvs_msda_layer_workspace_bytes": (C.c_size_t, [C.c_int] * 7),
    "axvs_msda_layer_fwd": (C.c_int, [_fp, _fp, _fp, C.c_int, _fp, C.POINTER(C.c_int), _fp, _fp] + [C.c_int] * 8 + [_fp, C.c_size_t, _fp]),
    "axvs_msda_core_fwd": (C.c_int, [_fp, C.POINTER(C.c_int), _fp, _fp, _fp] + [C.c_int] * 7 + [_fp]),
    "axvs_msda_core_bwd": (C.c_int, [_fp, C.POINTER(C.c_int), _fp, _fp, _fp, _fp, _fp, _fp] + [C.c_int] * 7 + [_fp]),
    "axvs_msda_layer_train_saved_bytes": (C.c_size_t, [C.c_int] * 7),
    "axvs_msda_layer_train_scratch_bytes": (C.c_size_t, [C.c_int] * 8),
    "axvs_msda_layer_train_fwd": (C.c_int, [_fp, _fp, _fp, C.c_int, _fp, C.POINTER(C.c_int), _fp, C.POINTER(AxvsMsdaLayerParams)] + [C.c_int] * 7 +
                                  [C.c_float, C.c_float, C.c_uint, _fp, C.c_size_t, _fp, C.c_size_t, _fp]),
    "axvs_msda_layer_train_bwd": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int, _fp, C.POINTER(C.c_int), C.POINTER(AxvsMsdaLayerParams),
                                            C.POINTER(AxvsMsdaLayerParams), _fp, _fp] + [C.c_int] * 7 +
                                  [C.c_float, C.c_float, C.c_uint, C.c_int, _fp, C.c_size_t, _fp, C.c_size_t, _fp]),
    "axvs_cc_module_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "axvs_cc_module_fwd": (C.c_int, [_fp] * 5 + [C.POINTER(_fp), _fp] + [C.c_int] * 8 + [C.POINTER(C.c_int), C.c_int, _fp, C.c_size_t, _fp]),
    "axvs_tl_cc_module_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "axvs_tl_cc_module_fwd": (C.c_int, [_fp] * 5 + [C.POINTER(_fp), _fp] + [C.c_int] * 9 + [C.POINTER(C.c_int), C.c_int, _fp, C.c_size_t, _fp]),
    "axvs_tl_heads_packed_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "axvs_tl_heads_pack": (C.c_int, [C.POINTER(AxvsTLHeadParams), _fp, C.c_int, C.c_int, C.c_int, _fp]),
    "axvs_tl_heads_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "axvs_tl_heads_fwd": (C.c_int, [_fp, _fp, _fp, _fp, _fp] + [C.c_int] * 9 + [_fp, C.c_size_t, _fp]),
    "axvs_tl_heads_train_saved_bytes": (C.c_size_t, [C.POINTER(AxvsTLHeadTrainCfg)]),
    "axvs_tl_heads_train_scratch_bytes": (C.c_size_t, [C.POINTER(AxvsTLHeadTrainCfg), C.c_int]),
    "axvs_tl_heads_train_fwd": (C.c_int, [_fp] * 4 + [C.POINTER(AxvsTLHeadParams), C.POINTER(AxvsTLHeadTrainCfg), _fp, C.c_size_t, _fp,
                                          C.c_size_t, _fp]),
    "axvs_tl_heads_train_bwd": (C.c_int, [_fp] * 4 + [C.POINTER(AxvsTLHeadParams), C.POINTER(AxvsTLHeadGrads), _fp, _fp,
                                          C.POINTER(AxvsTLHeadTrainCfg), _fp, C.c_size_t, _fp, C.c_size_t, _fp]),
    "axvs_pos3d": (C.c_int, [_fp] + [C.c_int] * 5 + [C.c_float, C.c_int, C.c_float, _fp]),
    "axvs_pos3d_masked": (C.c_int, [_fp, _fp] + [C.c_int] * 5 + [C.c_float, C.c_int, C.c_float, _fp]),
    "axvs_scaled_residual": (C.c_int, [_fp, _fp, _fp, _fp, C.c_size_t, C.c_int, _fp]),
    "axvs_test_train_gemm_scratch_bytes": (C.c_size_t, [C.POINTER(AxvsTestGemm)]),
    "axvs_test_train_gemm": (C.c_int, [C.POINTER(AxvsTestGemm), _fp, _fp]),
}

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load libaxvs.so (once) and attach the prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"axial_vs_amd: {LIB_PATH} is missing -- the HIP extension has not been built and there is no "
                "fallback path.  Run `python -c 'import __graft_entry__ as g; g.build()'` in the repo root.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


ERR_STATE = -4          # include/axvs.h AXVS_ERR_STATE: an earlier merged launch reported a hand-off timeout
_state_handler = None   # set by axial_vs_amd.modules: puts the sync words / status word back in order before the error is raised


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().axvs_last_error().decode(errors="replace")
        if rc == ERR_STATE and _state_handler is not None:
            _state_handler()
        raise RuntimeError(f"axial_vs_amd: {what} failed (code {rc}): {msg}")


def size_query(name: str, *args) -> int:
    """`name(*args)` of a `*_bytes` function whose refusal is 0 (the configuration is outside the kernels' bounds): raised with the
    library's message."""
    need = getattr(lib(), name)(*args)
    if need == 0:
        check(-1, name)
    return need


# ---- torch.autocast -> 16-bit products in the training tier -------------------------------------------------------------------------
# Under autocast the reference's nn.Linear layers multiply 16-bit operands with fp32 accumulation.  The training tier does the same
# when it is called under autocast: library option "train_amp" (1: bf16 pieces, 2: fp16 pieces, one per operand) for the duration
# of the forward call, and again for the backward call of the same graph.  `AMP_COMPUTE = False` (or `module.amp_compute = False`)
# keeps the split-precision (fp32-accurate) products under autocast.
AMP_COMPUTE = True
_AMP_MODE = 0


def autocast_mode(owner=None) -> int:
    import torch
    if not torch.is_autocast_enabled() or not AMP_COMPUTE or (owner is not None and not getattr(owner, "amp_compute", True)):
        return 0
    return 2 if torch.get_autocast_dtype("cuda") == torch.float16 else 1


def current_amp() -> int:
    return _AMP_MODE


_AMP_LOCK = threading.RLock()


class train_amp:
    """Context manager: the library's X W^T GEMMs of the training tier run with `mode` (0 off, 1 bf16, 2 fp16) inside.
    The option is process-wide in the library (forward and backward threads must agree on it), so training-tier calls are
    serialised on a lock while one holds the option: a concurrent call from another thread (a second model, a DataParallel
    replica) waits instead of running its GEMMs at the other call's precision."""

    def __init__(self, mode: int):
        self.mode = int(mode)

    def __enter__(self):
        global _AMP_MODE
        _AMP_LOCK.acquire()
        self.prev = _AMP_MODE
        _AMP_MODE = self.mode
        try:
            if self.mode != self.prev:
                check(lib().axvs_set_option(b"train_amp", self.mode), "axvs_set_option")
        except BaseException:       # __exit__ will not run: put the mode back and let the other threads in
            _AMP_MODE = self.prev
            _AMP_LOCK.release()
            raise
        return self

    def __exit__(self, *exc):
        global _AMP_MODE
        _AMP_MODE = self.prev
        try:
            if self.mode != self.prev:
                check(lib().axvs_set_option(b"train_amp", self.prev), "axvs_set_option")
        finally:
            _AMP_LOCK.release()
        return False
