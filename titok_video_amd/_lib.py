"""ctypes binding of libtitok_hip.so (C-ABI declared in include/titok_hip.h).

The library is loaded on first use.  If it is missing the call raises: there is no eager-PyTorch or CPU
fallback behind these entry points.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import torch

from . import switches

TTV_BF16, TTV_F32 = 0, 1
TTV_ENCODER, TTV_DECODER = 0, 1
TTV_MAX_FSQ = 8
TTV_MAX_TOKEN = 64
TTV_MAX_CLIPS_PER_LAUNCH = 64
TTV_DISC_HEAD_GENERATOR, TTV_DISC_HEAD_DISCRIMINATOR = 0, 1
TTV_TAPE_STORED, TTV_TAPE_RECOMPUTE = 0, 1          # tape modes of the training entry points (ttv_*_ex)

# ttv_debug_set bits: the TTV_DBG_* enum of include/titok_hip.h under the same names (tests/test_cabi_cpu.py holds the two equal).
# A value with two names is read by two kernels with two meanings; tools/README.md says what each bit forces.
DBG_NO_STORES = 1
DBG_K256_NO_PANEL_DMA = 2
DBG_MLP_NO_WEIGHT_DMA = 2
DBG_K256_NO_TILE_RELOAD = 4
DBG_MLP_NO_GEGLU = 4
DBG_K256_NO_EPILOGUE_MATH = 8
DBG_MLP_TILES8 = 8
DBG_MLP_NO_P2 = 16
DBG_MLP_PAIRS_ONLY = 32
DBG_MLP_TILES4 = 64
DBG_GEMM_TILE160 = 128
DBG_GEMM_TILE128 = 256
DBG_GEMM_T256 = 512
DBG_MLP_TILES9 = 512
DBG_GEMM_NO_T256 = 1024
DBG_MX_UNFUSED_QUANT = 2048
DBG_SPLIT3_NO_IMAGES = 4096
DBG_SPLIT3_NO_DMA = 8192
DBG_K256_GENERAL = 16384
DBG_QKV256_OFF = 32768
DBG_QKV256_WS = 131072
DBG_ENC_ALL_ROWS = 524288
DBG_ATTN_NO_SWP = 1048576
DBG_DEC_ALL_BLOCKS = 2097152
DBG_DEC_L0_NO_CONST = 4194304
DBG_ENC_LAST_QKV_ALL = 8388608
DBG_PATCH_EMBED_UNFUSED = 16777216

_HERE = os.path.dirname(os.path.abspath(__file__))
# TTV_LIB_PATH: diagnostics only (an instrumented build of the same sources, tools/attn_stamps.py)
LIB_PATH = switches.text("TTV_LIB_PATH") or os.path.join(_HERE, "libtitok_hip.so")

i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p


class FsqParams(C.Structure):
    _fields_ = [("n", i32), ("levels", i32 * TTV_MAX_FSQ), ("basis", i32 * TTV_MAX_FSQ),
                ("half_l", f32 * TTV_MAX_FSQ), ("offset", f32 * TTV_MAX_FSQ), ("shift", f32 * TTV_MAX_FSQ),
                ("half_width", f32 * TTV_MAX_FSQ)]


class TowerDims(C.Structure):
    _fields_ = [("kind", i32), ("dtype", i32), ("width", i32), ("layers", i32), ("q_heads", i32), ("kv_heads", i32),
                ("head_dim", i32), ("inner", i32), ("patch_t", i32), ("patch_h", i32), ("patch_w", i32),
                ("pix_channels", i32), ("token_size", i32), ("eps", f32), ("alpha", f32)]


class NextQkv(C.Structure):
    _fields_ = [("qkv", vp), ("ld", i32), ("rope_cs", vp), ("rows", i32), ("rope_q_end", i32), ("rope_k_begin", i32), ("rope_k_end", i32)]


class LayerWeights(C.Structure):
    _fields_ = [("pre_ln", vp), ("to_qkv", vp), ("out_proj", vp), ("ffd_norm", vp), ("w12", vp), ("w3", vp),
                ("attn_post_ln", vp), ("ffd_post_ln", vp), ("to_qkv_pn", vp), ("w12_pn", vp), ("mlp_pack", vp), ("mlp_pack_qkv_rows", i32), ("qkv_q_prescaled", i32),
                ("to_qkv_qs", vp), ("to_qkv_f8", vp), ("to_qkv_f8_scale", vp), ("w12_f8", vp), ("w12_f8_scale", vp),
                ("to_qkv_mx", vp), ("w12_mx", vp), ("out_proj_f8", vp), ("out_proj_f8_scale", vp), ("out_proj_mx", vp),
                ("w3_f8", vp), ("w3_f8_scale", vp), ("w3_mx", vp)]


class TowerWeights(C.Structure):
    _fields_ = [("proj_in_w", vp), ("proj_in_b", vp), ("mask_token", vp), ("ln_pre_t", vp), ("ln_pre_p", vp),
                ("ln_post", vp), ("proj_out_w", vp), ("proj_out_b", vp), ("layers", C.POINTER(LayerWeights)), ("proj_out_pn", vp),
                ("f32_split3", i32), ("attn_pv8", i32)]


class Batch(C.Structure):
    _fields_ = [("n_clips", i32), ("total_rows", i32), ("sum_tokens", i32), ("sum_patches", i32),
                ("max_patches_per_clip", i32), ("n_qblocks", i32), ("cu_seqlens", vp), ("latent_rows", vp),
                ("patch_rows", vp), ("clip_desc", vp), ("qblocks", vp), ("rope_cs", vp), ("blocks64", vp), ("row_seq", vp),
                ("n_blocks64", i32), ("qblocks_paired", i32), ("qblocks_all_full", i32), ("items64", vp), ("n_items64", i32),
                ("rope_ids", vp), ("rope_base", vp), ("qblocks_latent", vp), ("n_qblocks_latent", i32), ("qblocks_patch", vp),
                ("n_qblocks_patch", i32), ("tokens_per_clip", i32)]


class PlanSizes(C.Structure):
    _fields_ = [("n_clips", i32), ("total_rows", i32), ("sum_tokens", i32), ("sum_patches", i32), ("max_patches_per_clip", i32),
                ("max_seqlen", i32), ("n_rope_ids", i32), ("n_blocks64", i32), ("host_words", i64), ("off_cu_seqlens", i64),
                ("off_clip_desc", i64), ("off_blocks64", i64), ("dev_words", i64), ("off_latent_rows", i64), ("off_patch_rows", i64),
                ("off_row_seq", i64), ("off_rope_ids", i64)]


class PlanAttn(C.Structure):
    _fields_ = [("n_qblocks", i32), ("qblocks_all_full", i32), ("n_qblocks_latent", i32), ("n_qblocks_patch", i32), ("n_qblocks_l0", i32),
                ("tokens_per_clip", i32), ("words", i64), ("off_qblocks", i64), ("off_qblocks_latent", i64), ("off_qblocks_patch", i64),
                ("off_qblocks_l0", i64)]


class DecL0Const(C.Structure):
    _fields_ = [("rows", vp), ("latent_rows", i32), ("patch_rows", i32), ("state", vp), ("qblocks", vp), ("n_qblocks", i32)]


class LayerWeightsT(C.Structure):
    _fields_ = [("to_qkv_t", vp), ("out_proj_t", vp), ("w12_t", vp), ("w3_t", vp)]


class TowerWeightsT(C.Structure):
    _fields_ = [("proj_in_t", vp), ("proj_out_t", vp), ("layers", C.POINTER(LayerWeightsT))]


class LayerGrads(C.Structure):
    _fields_ = [("pre_ln", vp), ("to_qkv", vp), ("out_proj", vp), ("ffd_norm", vp), ("w12", vp), ("w3", vp),
                ("attn_post_ln", vp), ("ffd_post_ln", vp)]


class TowerGrads(C.Structure):
    _fields_ = [("proj_in_w", vp), ("proj_in_b", vp), ("mask_token", vp), ("ln_pre_t", vp), ("ln_pre_p", vp), ("ln_post", vp),
                ("proj_out_w", vp), ("proj_out_b", vp), ("layers", C.POINTER(LayerGrads)), ("layer_done_events", C.POINTER(vp))]


TTV_OPT_SCHEDULE_NONE, TTV_OPT_SCHEDULE_COSINE = 0, 1
TTV_OPT_SKIP_NONFINITE = 1


class OptState(C.Structure):
    _fields_ = [("updates", i64), ("skipped", i64), ("schedule_index", i64), ("skip_now", i32), ("lr", f32), ("bc1", f32),
                ("bc2_sqrt", f32), ("clip_coef", f32), ("norm", f32)]


class OptSchedule(C.Structure):
    _fields_ = [("kind", i32), ("reserved", i32), ("warmup_steps", i64), ("training_steps", i64), ("base_lr", C.c_double),
                ("end_lr", C.c_double), ("num_cycles", C.c_double), ("initial_lr", C.c_double), ("first", i64), ("stride", i64)]


class LpipsWeights(C.Structure):
    _fields_ = [("w", vp * 13), ("wd", vp * 13), ("b", vp * 13), ("lin", vp * 5)]


TTV_I3D_CONVS = 58
TTV_I3D_FEATURES = 400


class I3dWeights(C.Structure):
    _fields_ = [("w", vp * TTV_I3D_CONVS), ("scale", vp * TTV_I3D_CONVS), ("shift", vp * TTV_I3D_CONVS)]


TTV_INCEPTION_UNITS = 94
TTV_INCEPTION_FEATURES = 2048
TTV_INCEPTION_CLASSES = 1000
TTV_INCEPTION_INPUT = 299
TTV_INCEPTION_POOL_AVG3, TTV_INCEPTION_POOL_MAX3S2 = 0, 1


class InceptionUnit(C.Structure):
    _fields_ = [("w", vp), ("scale", vp), ("shift", vp)]


class InceptionWeights(C.Structure):
    _fields_ = [("unit", InceptionUnit * TTV_INCEPTION_UNITS), ("fc_w", vp), ("fc_b", vp)]


TTV_VJEPA_WIDTH = 1024
TTV_VJEPA_TOKENS = 1568
TTV_VJEPA_PATCH_K = 1536
TTV_VJEPA_EPI_STORE, TTV_VJEPA_EPI_GELU, TTV_VJEPA_EPI_RESID = 0, 1, 2


class VjepaLayer(C.Structure):
    _fields_ = [("norm1_w", vp), ("norm1_b", vp), ("qkv_w", vp), ("qkv_b", vp), ("proj_w", vp), ("proj_b", vp), ("norm2_w", vp),
                ("norm2_b", vp), ("fc1_w", vp), ("fc1_b", vp), ("fc2_w", vp), ("fc2_b", vp)]


class VjepaWeights(C.Structure):
    _fields_ = [("width", i32), ("heads", i32), ("depth", i32), ("patch_w", vp), ("patch_b", vp), ("pos_embed", vp),
                ("layers", C.POINTER(VjepaLayer)), ("norm_w", vp), ("norm_b", vp), ("query_tokens", vp), ("pool_q", vp),
                ("pool_norm1_w", vp), ("pool_norm1_b", vp), ("pool_kv_w", vp), ("pool_kv_b", vp), ("pool_proj_w", vp),
                ("pool_proj_b", vp), ("pool_norm2_w", vp), ("pool_norm2_b", vp), ("pool_fc1_w", vp), ("pool_fc1_b", vp),
                ("pool_fc2_w", vp), ("pool_fc2_b", vp)]


class VideoPlan(C.Structure):
    _fields_ = [("T", i32), ("H", i32), ("W", i32), ("frame_stride", i32), ("tile", i32 * 3), ("overlap", i32 * 3), ("count", i32 * 3)]


class Yuv420(C.Structure):
    _fields_ = [("y", vp), ("u", vp), ("v", vp), ("y_frame", i64), ("c_frame", i64), ("y_pitch", i32), ("c_pitch", i32), ("c_step", i32),
                ("matrix", i32), ("range", i32), ("siting", i32)]


YUV_MATRIX = {"bt601": 0, "bt709": 1}             # TTV_YUV_BT601, TTV_YUV_BT709
YUV_RANGE = {"limited": 0, "full": 1}             # TTV_YUV_LIMITED, TTV_YUV_FULL
YUV_SITING = {"left": 0, "center": 1}             # TTV_YUV_LEFT, TTV_YUV_CENTER

_lib = None
_lock = threading.Lock()

# every symbol include/titok_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "ttv_error_string": (C.c_char_p, []),
    "ttv_version": (C.c_int, []),
    "ttv_fsq_forward": (C.c_int, [C.POINTER(FsqParams), vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp]),
    "ttv_fsq_indices_to_codes": (C.c_int, [C.POINTER(FsqParams), vp, C.c_int, vp, C.c_int, vp]),
    "ttv_vq_codebook_norms": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "ttv_vq_workspace_bytes": (C.c_int64, [C.c_int]),
    "ttv_vq_l2_argmin": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int64, vp]),
    "ttv_vq_lookup": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp]),
    "ttv_vq_lookup_backward": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp]),
    "ttv_vq_train_workspace_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "ttv_vq_commit_forward": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int64, vp]),
    "ttv_vq_commit_backward": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp, C.c_int, vp]),
    "ttv_vq_ema_stats": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, f32, C.c_uint64, vp, C.c_int, C.c_int, vp, vp, C.c_int64, vp]),
    "ttv_vq_ema_update": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, f32, f32, f32, f32, vp, C.c_int64, vp]),
    "ttv_quant_rows_fp8": (C.c_int, [vp, C.c_int, C.c_int, vp, f32, vp, C.c_int, vp, C.c_int, C.c_int, vp]),
    "ttv_linear_fp8": (C.c_int, [vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp]),
    "ttv_split3_pack": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]),
    "ttv_linear_split3": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ttv_mx_scale_bytes_per_row": (C.c_int64, [C.c_int]),
    "ttv_quant_mx_fp8": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp]),
    "ttv_linear_fp8_mx": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int,
                                    vp, C.c_int, f32, vp]),
    "ttv_rmsnorm": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, f32, vp]),
    "ttv_rope_apply": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "ttv_linear": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ttv_linear_qkv_rope": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
    "ttv_linear_geglu": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ttv_linear_residual": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, f32, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, vp]),
    "ttv_linear_residual_norm": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, f32, vp, f32, vp, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, vp]),
    "ttv_mlp_pack_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "ttv_mlp_pack": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "ttv_layer_tail_fused": (C.c_int, [vp, C.c_int, vp, f32, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, f32, f32, C.c_int, C.c_int,
                                       C.c_int, vp, vp]),
    "ttv_mlp_fused": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, f32, f32, C.c_int, C.c_int, C.c_int, vp]),
    "ttv_fill_const_rows": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, f32, vp]),
    "ttv_decoder_embed": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, f32, vp]),
    "ttv_attention": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ttv_attention64": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    # the fused MX producers one by one (tests only)
    "ttv_rmsnorm_mx": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, f32, vp, vp, vp, vp]),
    "ttv_attention_pv8_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "ttv_quant_v_pv8": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "ttv_attention_pv8": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "ttv_attention_mxout": (C.c_int, [vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "ttv_linear_fp8_mx_geglu_q": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    # the folded pre-norm of the wide bf16 layer launch by launch (tests only)
    "ttv_row_rstd": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, f32, vp]),
    "ttv_linear_rowscale": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ttv_patch_gather": (C.c_int, [C.POINTER(vp), vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int,
                                   C.c_int, C.c_int, vp]),
    "ttv_patch_embed_norm": (C.c_int, [C.POINTER(vp), vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, f32,
                                       vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ttv_patch_scatter": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp),
                                    C.c_int, C.c_int, vp]),
    "ttv_tower_workspace_bytes": (i64, [C.POINTER(TowerDims), C.POINTER(Batch)]),
    "ttv_encoder_forward": (C.c_int, [C.POINTER(TowerDims), C.POINTER(TowerWeights), C.POINTER(Batch), C.POINTER(vp),
                                      C.POINTER(FsqParams), vp, vp, vp, vp, vp, i64, vp]),
    "ttv_decoder_forward": (C.c_int, [C.POINTER(TowerDims), C.POINTER(TowerWeights), C.POINTER(Batch), vp, C.POINTER(vp),
                                      vp, i64, vp]),
    "ttv_dec_l0_const_bytes": (i64, [C.POINTER(TowerDims), C.c_int]),
    "ttv_dec_l0_const_build": (C.c_int, [C.POINTER(TowerDims), C.POINTER(TowerWeights), vp, vp, vp, vp, C.c_int, vp, i64, C.POINTER(i64), C.POINTER(i64), vp]),
    "ttv_decoder_forward_const": (C.c_int, [C.POINTER(TowerDims), C.POINTER(TowerWeights), C.POINTER(Batch), vp, C.POINTER(vp),
                                            vp, i64, C.POINTER(DecL0Const), vp]),
    "ttv_tower_tape_bytes": (i64, [C.POINTER(TowerDims), C.POINTER(Batch)]),
    "ttv_tower_bwd_workspace_bytes": (i64, [C.POINTER(TowerDims), C.POINTER(Batch)]),
    "ttv_encoder_forward_train": (C.c_int, [C.POINTER(TowerDims), C.POINTER(TowerWeights), C.POINTER(Batch), C.POINTER(vp), vp, vp,
                                            i64, vp]),
    "ttv_encoder_backward": (C.c_int, [C.POINTER(TowerDims), C.POINTER(TowerWeights), C.POINTER(TowerWeightsT), C.POINTER(Batch), vp,
                                       vp, C.POINTER(TowerGrads), C.POINTER(vp), vp, i64, vp]),
    "ttv_decoder_forward_train": (C.c_int, [C.POINTER(TowerDims), C.POINTER(TowerWeights), C.POINTER(Batch), vp, C.POINTER(vp), vp,
                                            i64, vp, i64, vp]),
    "ttv_decoder_backward": (C.c_int, [C.POINTER(TowerDims), C.POINTER(TowerWeights), C.POINTER(TowerWeightsT), C.POINTER(Batch), vp,
                                       C.POINTER(vp), vp, C.POINTER(TowerGrads), vp, vp, i64, vp]),
    # the six above with a tape mode (TTV_TAPE_*) as their last argument
    "ttv_tower_tape_bytes_ex": (i64, [C.POINTER(TowerDims), C.POINTER(Batch), C.c_int]),
    "ttv_tower_bwd_workspace_bytes_ex": (i64, [C.POINTER(TowerDims), C.POINTER(Batch), C.c_int]),
    "ttv_encoder_forward_train_ex": (C.c_int, [C.POINTER(TowerDims), C.POINTER(TowerWeights), C.POINTER(Batch), C.POINTER(vp), vp, vp,
                                               i64, vp, C.c_int]),
    "ttv_encoder_backward_ex": (C.c_int, [C.POINTER(TowerDims), C.POINTER(TowerWeights), C.POINTER(TowerWeightsT), C.POINTER(Batch), vp,
                                          vp, C.POINTER(TowerGrads), C.POINTER(vp), vp, i64, vp, C.c_int]),
    "ttv_decoder_forward_train_ex": (C.c_int, [C.POINTER(TowerDims), C.POINTER(TowerWeights), C.POINTER(Batch), vp, C.POINTER(vp), vp,
                                               i64, vp, i64, vp, C.c_int]),
    "ttv_decoder_backward_ex": (C.c_int, [C.POINTER(TowerDims), C.POINTER(TowerWeights), C.POINTER(TowerWeightsT), C.POINTER(Batch), vp,
                                          C.POINTER(vp), vp, C.POINTER(TowerGrads), vp, vp, i64, vp, C.c_int]),
    "ttv_fsq_backward": (C.c_int, [C.POINTER(FsqParams), vp, vp, C.c_int, vp, C.c_int, vp]),
    # the tape's elementwise and small-projection ops one by one (tests only)
    "ttv_gate_forward": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ttv_gate_backward": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "ttv_geglu_forward": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ttv_geglu_backward": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ttv_scale_cast": (C.c_int, [vp, f32, vp, vp, C.c_int, C.c_int64, vp]),
    "ttv_cast_to_f32": (C.c_int, [vp, C.c_int, vp, C.c_int64, C.c_int, vp]),
    "ttv_expand_small": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "ttv_reduce_small": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]),
    "ttv_const_rows_backward": (C.c_int, [vp, vp, vp, C.c_int, f32, vp, vp, C.c_int, vp]),
    "ttv_rope_apply_conj": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "ttv_decoder_embed_tape": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, f32, vp, vp]),
    "ttv_rmsnorm_backward_chain": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, C.c_float, vp, C.c_int,
                                              C.c_int, C.c_int, C.c_float, C.c_int, vp]),
    "ttv_opt_grad_sumsq": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp]),
    "ttv_opt_adamw_step": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.c_int] + [C.c_float] * 10 + [vp, vp]),
    "ttv_opt_prepare": (C.c_int, [vp, OptSchedule, C.c_double, C.c_double, C.c_double, C.c_float, vp, C.c_int, C.c_int, vp, vp]),
    "ttv_opt_adamw_step_dev": (C.c_int, [vp, vp, C.c_int, C.c_int, vp] + [C.c_float] * 6 + [vp]),
    "ttv_opt_param_norms": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp]),
    "ttv_opt_ema_update": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_float, vp]),
    "ttv_opt_ema_exchange": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "ttv_linear_wgrad_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "ttv_linear_wgrad": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int64, vp]),
    "ttv_rmsnorm_backward": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, C.c_int, f32, C.c_int, vp]),
    "ttv_attention_backward": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int,
                                         C.c_int, C.c_int, C.c_int, vp, vp]),
    "ttv_attention_backward_qlim": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int,
                                              C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "ttv_attention_lse": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "ttv_codebook_histogram": (C.c_int, [vp, C.c_int, vp, C.c_int, vp]),
    "ttv_rope_table_build": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp]),
    "ttv_plan_rows_sizes": (C.c_int, [vp, vp, C.c_int, vp, C.POINTER(PlanSizes)]),
    "ttv_plan_rows_fill": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, vp, i64]),
    "ttv_plan_rows_build": (C.c_int, [C.POINTER(PlanSizes), vp, vp, vp, vp, C.c_int, vp, vp, C.POINTER(Batch), vp]),
    "ttv_plan_attn_sizes": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PlanAttn)]),
    "ttv_plan_attn_fill": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, i64]),
    "ttv_plan_attn_set": (C.c_int, [C.POINTER(PlanAttn), vp, vp, C.POINTER(Batch), vp]),
    "ttv_rope_base_table": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, vp, vp]),
    "ttv_l1_loss": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp]),
    "ttv_clip_from_u8": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
    "ttv_clip_resample_u8": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp]),
    "ttv_recon_panels_u8": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp]),
    "ttv_video_tiles_u8": (C.c_int, [vp, C.POINTER(VideoPlan), C.c_int, C.c_int, vp, C.c_int, vp]),
    "ttv_video_blend_u8": (C.c_int, [vp, vp, C.POINTER(VideoPlan), C.c_int, C.c_int, C.c_int, vp, vp]),
    "ttv_video_tile_sse_u8": (C.c_int, [vp, C.POINTER(VideoPlan), C.c_int, C.c_int, vp, vp, C.c_int, vp, vp]),
    "ttv_video_tiles_yuv420": (C.c_int, [C.POINTER(Yuv420), C.POINTER(VideoPlan), C.c_int, C.c_int, vp, C.c_int, vp]),
    "ttv_video_blend_yuv420": (C.c_int, [vp, vp, C.POINTER(VideoPlan), C.c_int, C.c_int, C.c_int, C.POINTER(Yuv420), vp]),
    "ttv_video_tile_sse_yuv420": (C.c_int, [C.POINTER(Yuv420), C.POINTER(VideoPlan), C.c_int, C.c_int, vp, vp, C.c_int, vp, vp]),
    "ttv_video_frame_sse_u8": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "ttv_video_frame_sse_yuv420": (C.c_int, [C.POINTER(Yuv420), C.POINTER(Yuv420), C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "ttv_video_frame_ssim_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ttv_video_frame_ssim_u8": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int64, vp]),
    "ttv_video_frame_ssim_yuv420": (C.c_int, [C.POINTER(Yuv420), C.POINTER(Yuv420), C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int64,
                                              vp]),
    "ttv_sq_err_accumulate": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "ttv_ssim_workspace_bytes": (C.c_int64, [vp, C.c_int]),
    "ttv_ssim_accumulate": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int64, vp]),
    "ttv_lpips_tape_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ttv_lpips_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ttv_lpips_forward": (C.c_int, [C.POINTER(LpipsWeights), vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int64, vp]),
    "ttv_lpips_backward": (C.c_int, [C.POINTER(LpipsWeights), vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int64, vp]),
    "ttv_lpips_eval_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ttv_lpips_eval_accumulate": (C.c_int, [C.POINTER(LpipsWeights), vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp,
                                            C.c_int64, vp]),
    "ttv_lpips_conv_workspace_bytes": (C.c_int64, [C.c_int] * 6),
    "ttv_lpips_conv3x3": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int64, vp]),
    "ttv_lpips_maxpool": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
    "ttv_lpips_maxpool_backward": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
    "ttv_lpips_crops_forward": (C.c_int, [vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp]),
    "ttv_lpips_crops_backward": (C.c_int, [vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp]),
    "ttv_gp_noise_add": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_uint64, C.c_uint64, f32, C.c_int, vp]),
    "ttv_disc_head": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32, f32, vp, vp, vp]),
    "ttv_i3d_workspace_bytes": (C.c_int64, [C.c_int]),
    "ttv_fvd_preprocess": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "ttv_i3d_features": (C.c_int, [C.POINTER(I3dWeights), vp, C.c_int, vp, vp, C.c_int64, vp]),
    "ttv_i3d_conv3d": (C.c_int, [vp] + [C.c_int] * 7 + [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp]),
    "ttv_i3d_maxpool3d": (C.c_int, [vp] + [C.c_int] * 11 + [vp, vp]),
    "ttv_inception_workspace_bytes": (C.c_int64, [C.c_int]),
    "ttv_inception_preprocess": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "ttv_inception_features": (C.c_int, [C.POINTER(InceptionWeights), vp, C.c_int, vp, vp, vp, C.c_int64, vp]),
    "ttv_inception_conv2d": (C.c_int, [vp] + [C.c_int] * 10 + [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp]),
    "ttv_inception_pool2d": (C.c_int, [vp] + [C.c_int] * 5 + [vp, C.c_int, C.c_int, vp]),
    "ttv_jedi_preprocess":(C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp]),
    "ttv_vjepa_workspace_bytes": (C.c_int64, [C.c_int]),
    "ttv_vjepa_features": (C.c_int, [C.POINTER(VjepaWeights), vp, C.c_int, vp, C.c_int, vp, C.c_int64, vp]),
    "ttv_vjepa_layernorm": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_float, vp, vp, C.c_float, vp, C.c_int, vp, C.c_int, vp]),
    "ttv_vjepa_linear": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp]),
    "ttv_vjepa_pool_attention": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp]),
    # deterministic mode: the process-wide switch, the siblings with scratch of the ops that have no workspace argument, and the tower
    # backward's three small reductions on their own (tests)
    "ttv_set_deterministic": (C.c_int, [C.c_int]),
    "ttv_get_deterministic": (C.c_int, []),
    "ttv_vq_lookup_backward_det_scratch_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "ttv_vq_lookup_backward_det": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int64, vp]),
    "ttv_rmsnorm_backward_det_scratch_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "ttv_rmsnorm_backward_chain_det_scratch_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "ttv_rmsnorm_backward_chain_det": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, C.c_float, vp, C.c_int,
                                                  C.c_int, C.c_int, C.c_float, C.c_int, vp, C.c_int64, vp]),
    "ttv_rmsnorm_backward_det": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, C.c_int, f32, C.c_int, vp, vp, vp, vp,
                                            C.c_int64, vp]),
    "ttv_colsum_det_scratch_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "ttv_sumall_det_scratch_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "ttv_outer_small_det_scratch_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "ttv_colsum_accumulate": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.c_int64, vp]),
    "ttv_sumall_accumulate": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, f32, vp, vp, C.c_int64, vp]),
    "ttv_outer_small_accumulate": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp,
                                              C.c_int64, vp]),
    "ttv_l1_loss_det_scratch_bytes": (C.c_int64, [vp, C.c_int]),
    "ttv_l1_loss_det": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int64, vp]),
    "ttv_sq_err_accumulate_det_scratch_bytes": (C.c_int64, [vp, C.c_int]),
    "ttv_sq_err_accumulate_det": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int64, vp]),
    "ttv_debug_set": (C.c_int, [C.c_int]),
    "ttv_debug_stamps": (C.c_int, [vp]),
    "ttv_prof_begin": (C.c_int, [C.c_int, C.c_int]),
    "ttv_prof_end": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_int)]),
}

KERNEL_CLASSES = {"attention": 1, "gemm_qkv": 2, "gemm_geglu": 3, "gemm_resid": 4, "gemm_store": 5, "rmsnorm": 6,
                  "patch": 7, "rows": 8}


def lib():
    """The loaded library (raises RuntimeError when it has not been built)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"titok_video_amd: {LIB_PATH} is missing - build it with `python -c 'import __graft_entry__ as g; "
                        "g.build()'` (or titok_video_amd/csrc/build.sh). There is no non-HIP fallback.")
                handle = C.CDLL(LIB_PATH)
                for name, (res, args) in SYMBOLS.items():
                    fn = getattr(handle, name)
                    fn.restype, fn.argtypes = res, args
                # TTV_DETERMINISTIC=1: the process starts in deterministic mode (set_deterministic() changes it later)
                if switches.flag("TTV_DETERMINISTIC", False):
                    handle.ttv_set_deterministic(1)
                _lib = handle
    return _lib


def set_deterministic(flag: bool) -> bool:
    """Fixed-order sums in place of every float atomic of the training path (ttv_set_deterministic); returns the previous setting."""
    return bool(lib().ttv_set_deterministic(1 if flag else 0))


def is_deterministic() -> bool:
    return bool(lib().ttv_get_deterministic())


class DetScratch:
    """Device scratch for the block partials of a *_det entry point: one tensor per (device, stream), grown as needed and kept.
    A launch and its fold are ordered on their stream, so calls on one stream share a buffer safely and calls on two streams never
    do.  While a graph is being captured nothing is kept: the tensor comes from the graph's own pool and stays there, so an eager
    call never writes into memory a replay uses."""

    def __init__(self):
        self._bufs = {}

    def get(self, nbytes: int, device) -> torch.Tensor:
        device = torch.device(device)
        stream = torch.cuda.current_stream(device)
        if torch.cuda.is_current_stream_capturing():
            return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        key = (device.index if device.index is not None else torch.cuda.current_device(), stream.cuda_stream)
        buf = self._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = self._bufs[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        return buf


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().ttv_error_string().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.bfloat16:
        return TTV_BF16
    if dt == torch.float32:
        return TTV_F32
    raise TypeError(f"titok_video_amd supports bfloat16 and float32 activations, got {dt}")


def require_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensor is on {t.device}; titok_video_amd runs on MI355X (HIP) only, there is no CPU path")


def stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def ptr_array(tensors):
    arr = (vp * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr
