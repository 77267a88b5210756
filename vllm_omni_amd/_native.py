"""ctypes binding of libomni_cdna4.so — the C-ABI declared in include/omni_cdna4.h.

The product path has NO CPU / PyTorch fallback: if the shared library is missing or a call returns a
non-zero status, an exception is raised (the worker turns it into `DiffusionOutput.error`, mirroring
the reference's error path at vllm_omni/diffusion/worker/gpu_worker.py:266-274).
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libomni_cdna4.so")   # fixed: dev sweeps assign this attribute (tools/devlib.py)
ABI_VERSION = 14

c_bf16_p = C.c_void_p  # device pointer to uint16_t bf16 bits
c_i32_p = C.c_void_p
c_f32_p = C.c_void_p


class OmniNativeError(RuntimeError):
    pass


class GemmGroup(C.Structure):
    _fields_ = [
        ("A", c_bf16_p), ("lda", C.c_int64), ("a_row_map", c_i32_p), ("M", C.c_int32),
        ("W", c_bf16_p), ("bias", c_bf16_p),
        ("out", c_bf16_p), ("out1", c_bf16_p), ("out2", c_bf16_p), ("ldo", C.c_int64),
        ("out_row_map", c_i32_p),
        ("res", c_bf16_p), ("ldres", C.c_int64),
        ("gate", c_bf16_p), ("gate_item_stride", C.c_int64),
        ("row_item_map", c_i32_p), ("rows_per_item", C.c_int32),
        ("qk_norm_q_w", c_bf16_p), ("qk_norm_k_w", c_bf16_p), ("qk_rope_cos", c_bf16_p), ("qk_rope_sin", c_bf16_p),
        ("qk_row_pos", c_i32_p), ("qk_eps", C.c_float),
        ("a_k32_rows", C.c_int32), ("out_k32_rows", C.c_int32), ("qk_q_scale", C.c_float),      # qk_q_scale: ABI v5
        ("tile_skip", c_i32_p),
        ("a_scale", C.c_void_p), ("w_scale", C.c_void_p),                                        # ABI v7 (fp8)
    ]


class GemmParams(C.Structure):
    _fields_ = [
        ("ngroups", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("epilogue", C.c_int32),
        ("split_n", C.c_int32), ("w_k32_blocked", C.c_int32), ("g", GemmGroup * 2),
        ("splitk_ws", C.c_void_p), ("splitk_ws_floats", C.c_int64),          # ABI v4
        ("kernel_hint", C.c_int32), ("fp8", C.c_int32),                      # ABI v6: kernel_hint; v7: fp8 operands
    ]


class AdalnStream(C.Structure):
    """omni_adaln_stream (ABI v12): one row group of omni_adaln_modulate_pair."""
    _fields_ = [
        ("x", c_bf16_p), ("y", c_bf16_p), ("rows", C.c_int32), ("scale", c_bf16_p), ("shift", c_bf16_p),
        ("row_item_map", c_i32_p), ("rows_per_item", C.c_int32), ("y_k32_rows", C.c_int32),
        ("y8", C.c_void_p), ("y8_rows", C.c_int32), ("y8_scale", C.c_void_p),
    ]


class FinishAdalnStream(C.Structure):
    """omni_finish_adaln_stream (ABI v13): one row group of omni_splitk_finish_adaln_pair."""
    _fields_ = [
        ("rows", C.c_int32), ("ws_row0", C.c_int32), ("bias", c_bf16_p), ("hidden", c_bf16_p), ("gate", c_bf16_p),
        ("scale", c_bf16_p), ("shift", c_bf16_p), ("row_item_map", c_i32_p), ("rows_per_item", C.c_int32),
        ("y", c_bf16_p), ("y_k32_rows", C.c_int32),
    ]


class AttnParams(C.Structure):
    """omni_attn_params (ABI v11): the general attention of the SDPA plug-in point — cross-attention, masks, causal, dh 64 / 128."""
    _fields_ = [
        ("q", c_bf16_p), ("k", c_bf16_p), ("v", c_bf16_p), ("out", c_bf16_p),
        ("ldq", C.c_int64), ("ldk", C.c_int64), ("ldv", C.c_int64), ("ldo", C.c_int64),
        ("cu_seqlens_q", c_i32_p), ("cu_seqlens_k", c_i32_p),
        ("B", C.c_int32), ("H", C.c_int32), ("H_kv", C.c_int32), ("head_dim", C.c_int32),
        ("max_seqlen_q", C.c_int32), ("max_seqlen_k", C.c_int32),
        ("softmax_scale", C.c_float), ("causal", C.c_int32),
        ("mask", C.c_void_p), ("mask_type", C.c_int32), ("elem_type", C.c_int32),      # elem_type: former padding
        ("mask_stride_b", C.c_int64), ("mask_stride_h", C.c_int64), ("mask_stride_q", C.c_int64), ("mask_stride_k", C.c_int64),
        ("qk_int8", C.c_int32), ("out_k32_rows", C.c_int32), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),  # ABI v14
        ("item_skip", c_i32_p),
    ]


class CfgEulerReq(C.Structure):
    """omni_cfg_euler_req: one request of omni_cfg_euler_step_ragged (an array of these lives in DEVICE memory)."""
    _fields_ = [
        ("lat_row", C.c_int32), ("rows", C.c_int32), ("pos_row", C.c_int32), ("neg_row", C.c_int32),
        ("dst_row", C.c_int32 * 2), ("dt_index", C.c_int32), ("cfg_scale", C.c_float),
    ]


class LoraMergeParams(C.Structure):
    """omni_lora_merge_params: one row range of one weight matrix and its low-rank update (omni_lora_merge)."""
    _fields_ = [
        ("w_base", c_bf16_p), ("w_out", c_bf16_p), ("up", c_bf16_p), ("down", c_bf16_p),
        ("N", C.c_int32), ("K", C.c_int32), ("R", C.c_int32), ("row0", C.c_int32), ("rows", C.c_int32),
        ("w_k32_blocked", C.c_int32), ("ldw", C.c_int64), ("scale", C.c_float),
    ]


class TextLayerWeights(C.Structure):
    """omni_text_layer_weights: device pointers of one Qwen2.5-VL decoder layer (fused q|k|v and gate|up matrices)."""
    _fields_ = [(n, c_bf16_p) for n in ("input_norm_w", "qkv_w", "qkv_b", "o_w", "post_norm_w", "gate_up_w", "down_w")]


class TextWeights(C.Structure):
    """omni_text_weights: geometry, embedding, RoPE tables and the HOST array of layers of omni_qwen2_text_forward."""
    _fields_ = [
        ("num_layers", C.c_int32), ("hidden_size", C.c_int32), ("num_heads", C.c_int32), ("num_kv_heads", C.c_int32),
        ("head_dim", C.c_int32), ("intermediate_size", C.c_int32), ("vocab_size", C.c_int32), ("gemm_w_k32_blocked", C.c_int32),
        ("rms_norm_eps", C.c_float), ("rope_npos", C.c_int32),
        ("embed_tokens", c_bf16_p), ("final_norm_w", c_bf16_p), ("ones", c_bf16_p), ("rope_cos", c_f32_p), ("rope_sin", c_f32_p),
        ("layers", C.POINTER(TextLayerWeights)),
    ]


class TextBatch(C.Structure):
    """omni_text_batch: the packed tokens of up to 64 prompts, the output and the caller-owned workspace."""
    _fields_ = [
        ("n_prompts", C.c_int32), ("total_rows", C.c_int32), ("max_seqlen", C.c_int32), ("reserved", C.c_int32),
        ("input_ids", c_i32_p), ("cu_seqlens", c_i32_p), ("row_pos", c_i32_p), ("out", c_bf16_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


class TextBatchMm(C.Structure):
    """omni_text_batch_mm: omni_text_batch plus the three M-RoPE position rows and the vision rows of the picture tokens."""
    _fields_ = TextBatch._fields_ + [
        ("row_pos3", c_i32_p), ("vision_rows", c_bf16_p), ("vision_row_of", c_i32_p),
        ("n_vision_rows", C.c_int32), ("mrope_section", C.c_int32 * 3),
    ]


class GemvParams(C.Structure):
    """omni_gemv_params: one weight-streaming GEMV of M <= 8 rows (omni_gemv_bf16)."""
    _fields_ = [
        ("A", c_bf16_p), ("lda", C.c_int64), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("w_k32_blocked", C.c_int32),
        ("W", c_bf16_p), ("bias", c_bf16_p), ("res", c_bf16_p), ("ldres", C.c_int64),
        ("out", c_bf16_p), ("out_f32", c_f32_p), ("ldo", C.c_int64),
    ]


class DecodeAttnParams(C.Structure):
    """omni_decode_attn_params: one query row per sequence against the KV cache (omni_decode_attention)."""
    _fields_ = [
        ("q", c_bf16_p), ("ldq", C.c_int64), ("k_cache", c_bf16_p), ("v_cache", c_bf16_p), ("out", c_bf16_p), ("ldo", C.c_int64),
        ("lens", c_i32_p), ("done", c_i32_p), ("len_add", C.c_int32), ("n_seq", C.c_int32), ("H", C.c_int32), ("H_kv", C.c_int32),
        ("head_dim", C.c_int32), ("capacity", C.c_int32), ("softmax_scale", C.c_float), ("reserved", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


class PenalizedArgmaxParams(C.Structure):
    """omni_penalized_argmax_params: repetition penalty + argmax + EOS + the step's bookkeeping (omni_text_penalized_argmax)."""
    _fields_ = [
        ("logits", c_f32_p), ("ld", C.c_int64), ("seen", C.c_void_p), ("seen_stride", C.c_int64), ("ctrl", c_i32_p),
        ("out_tokens", c_i32_p), ("set_len_cu", c_i32_p), ("vocab", C.c_int32), ("n_seq", C.c_int32), ("max_new", C.c_int32),
        ("n_eos", C.c_int32), ("eos_ids", C.c_int32 * 8), ("penalty", C.c_float), ("reserved", C.c_int32),
    ]


class TextDecodeLayout(C.Structure):
    """omni_text_decode_layout: byte offsets of the parts of the decode state a caller reads or writes."""
    _fields_ = [(n, C.c_size_t) for n in ("ctrl", "out_tokens", "seen", "seen_stride", "k_cache", "v_cache", "logits", "qkv", "total")]


class TextDecodeState(C.Structure):
    """omni_text_decode_state: the KV cache and the per-sequence decode words of omni_qwen2_text_prefill / _decode_step."""
    _fields_ = [
        ("n_seq", C.c_int32), ("capacity", C.c_int32), ("max_new", C.c_int32), ("n_eos", C.c_int32), ("eos_ids", C.c_int32 * 8),
        ("repetition_penalty", C.c_float), ("reserved", C.c_int32), ("lm_head", c_bf16_p),
        ("state", C.c_void_p), ("state_bytes", C.c_size_t), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("logits_out", c_f32_p),
    ]


class VisionLayerWeights(C.Structure):
    """omni_vision_layer_weights: device pointers of one Qwen2.5-VL vision block (padded as the header says)."""
    _fields_ = [(n, c_bf16_p) for n in ("norm1_w", "qkv_w", "qkv_b", "proj_w", "proj_b", "norm2_w", "gate_up_w", "gate_up_b",
                                        "down_w", "down_b")] + [("full_attention", C.c_int32), ("reserved", C.c_int32)]


class VisionWeights(C.Structure):
    """omni_vision_weights: geometry, patch embedding, merger and the HOST array of blocks of omni_qwen2_vision_forward."""
    _fields_ = [
        ("num_layers", C.c_int32), ("hidden_size", C.c_int32), ("num_heads", C.c_int32), ("head_dim", C.c_int32),
        ("intermediate_size", C.c_int32), ("patch_k", C.c_int32), ("out_hidden_size", C.c_int32), ("gemm_w_k32_blocked", C.c_int32),
        ("rms_norm_eps", C.c_float), ("reserved", C.c_int32),
        ("patch_w", c_bf16_p), ("ones", c_bf16_p), ("merger_norm_w", c_bf16_p), ("merger_fc1_w", c_bf16_p),
        ("merger_fc1_b", c_bf16_p), ("merger_fc2_w", c_bf16_p), ("merger_fc2_b", c_bf16_p),
        ("layers", C.POINTER(VisionLayerWeights)),
    ]


class VisionBatch(C.Structure):
    """omni_vision_batch: the packed patch rows of all pictures in window order, their windows, pictures and RoPE tables."""
    _fields_ = [
        ("rows", C.c_int32), ("n_windows", C.c_int32), ("n_images", C.c_int32), ("max_window", C.c_int32),
        ("max_image", C.c_int32), ("reserved", C.c_int32),
        ("pixels", c_bf16_p), ("cu_window", c_i32_p), ("cu_image", c_i32_p), ("rope_cos", c_f32_p), ("rope_sin", c_f32_p),
        ("out", c_bf16_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


class ConvParams(C.Structure):
    _fields_ = [
        ("x", c_bf16_p), ("w", c_bf16_p), ("bias", c_bf16_p), ("gamma", c_bf16_p), ("res", c_bf16_p), ("y", c_bf16_p),
        ("B", C.c_int32), ("Hin", C.c_int32), ("Win", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32),
        ("ksize", C.c_int32), ("upsample2x", C.c_int32), ("silu", C.c_int32),
        ("clamp_lo", C.c_float), ("clamp_hi", C.c_float), ("downsample2x", C.c_int32),
        ("x_padded", C.c_int32), ("y_padded", C.c_int32),
        ("norm_gamma", c_bf16_p), ("y_norm", c_bf16_p), ("norm_silu", C.c_int32),                 # ABI v10
    ]


_LAYER_FIELDS = [
    "img_mod_w", "img_mod_b", "txt_mod_w", "txt_mod_b",
    "to_qkv_w", "to_qkv_b", "add_qkv_w", "add_qkv_b",
    "norm_q_w", "norm_k_w", "norm_added_q_w", "norm_added_k_w",
    "to_out_w", "to_out_b", "to_add_out_w", "to_add_out_b",
    "img_mlp_w1", "img_mlp_b1", "img_mlp_w2", "img_mlp_b2",
    "txt_mlp_w1", "txt_mlp_b1", "txt_mlp_w2", "txt_mlp_b2",
]


class DitLayerWeights(C.Structure):
    _fields_ = [(n, c_bf16_p) for n in _LAYER_FIELDS]


_FP8_FIELDS = ["to_qkv", "add_qkv", "to_out", "to_add_out", "img_mlp_w1", "img_mlp_w2", "txt_mlp_w1", "txt_mlp_w2"]


class DitFp8Layer(C.Structure):
    """omni_dit_fp8_layer: e4m3 copies (K64-blocked) of a layer's eight GEMM weights, then their per-channel fp32 scales."""
    _fields_ = [(f + ("_w8" if "mlp" not in f else "_8"), C.c_void_p) for f in _FP8_FIELDS] + [(f + "_s", C.c_void_p) for f in _FP8_FIELDS]


class DitWeights(C.Structure):
    _fields_ = [
        ("num_layers", C.c_int32), ("num_heads", C.c_int32), ("head_dim", C.c_int32), ("joint_dim", C.c_int32),
        ("in_channels", C.c_int32), ("out_channels_packed", C.c_int32), ("gemm_w_k32_blocked", C.c_int32),
        ("t_lin1_w", c_bf16_p), ("t_lin1_b", c_bf16_p), ("t_lin2_w", c_bf16_p), ("t_lin2_b", c_bf16_p),
        ("txt_norm_w", c_bf16_p), ("img_in_w", c_bf16_p), ("img_in_b", c_bf16_p), ("txt_in_w", c_bf16_p),
        ("txt_in_b", c_bf16_p),
        ("norm_out_w", c_bf16_p), ("norm_out_b", c_bf16_p), ("proj_out_w", c_bf16_p), ("proj_out_b", c_bf16_p),
        ("layers", C.POINTER(DitLayerWeights)),
        ("fp8_layers", C.POINTER(DitFp8Layer)),                                                    # ABI v7, nullable
    ]


class TeaCache(C.Structure):
    """omni_teacache: device-side TeaCache state of one step-batch (include/omni_cdna4.h)."""
    _fields_ = [
        ("rel_l1_thresh", C.c_float), ("coeff", C.c_float * 5),
        ("prev_mod", c_bf16_p), ("prev_res", c_bf16_p), ("acc_dist", c_f32_p), ("cnt", c_i32_p), ("skip", c_i32_p),
        ("skip_total", c_i32_p), ("scratch", c_f32_p), ("tile_skip_img", c_i32_p), ("tile_skip_txt", c_i32_p),
        ("txt_cu", c_i32_p),
    ]


class DitBatch(C.Structure):
    _fields_ = [
        ("n_items", C.c_int32), ("n_img_rows", C.c_int32), ("n_txt_rows", C.c_int32), ("n_joint_rows", C.c_int32),
        ("n_temb", C.c_int32), ("max_seqlen", C.c_int32),
        ("latents", c_bf16_p), ("prompt_embeds", c_bf16_p), ("timestep", c_f32_p),
        ("cu_seqlens", c_i32_p), ("img_item", c_i32_p), ("txt_item", c_i32_p),
        ("img_joint_row", c_i32_p), ("txt_joint_row", c_i32_p), ("joint_pos", c_i32_p),
        ("txt_pos_end", C.c_int32), ("attn_qk_int8", C.c_int32),       # attn_qk_int8: ABI v14, former padding
        ("rope_cos", c_bf16_p), ("rope_sin", c_bf16_p),
        ("noise_pred", c_bf16_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("teacache", C.POINTER(TeaCache)),
        ("temb_add", c_bf16_p),                                                                    # ABI v9, nullable
        ("mod_table", c_bf16_p),                                                                   # ABI v9, nullable
    ]


# name -> (restype, argtypes); must list every symbol include/omni_cdna4.h declares
PROTOTYPES = {
    "omni_abi_version": (C.c_int, []),
    "omni_build_arch": (C.c_char_p, []),
    "omni_status_string": (C.c_char_p, [C.c_int]),
    "omni_features": (C.c_uint32, []),            # capability bits; OPTIONAL (see lib()): a library of the same ABI version may lack it
    "omni_gemm_bf16": (C.c_int, [C.POINTER(GemmParams), C.c_void_p]),
    "omni_quantize_fp8_rows": (C.c_int, [c_bf16_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                         C.c_void_p, C.c_void_p]),
    "omni_adaln_modulate": (C.c_int, [c_bf16_p, C.c_int64, c_bf16_p, C.c_int64, C.c_int32, C.c_int32, c_bf16_p,
                                      c_bf16_p, C.c_int64, c_i32_p, C.c_int32, C.c_float, C.c_void_p]),
    "omni_adaln_modulate_ex": (C.c_int, [c_bf16_p, C.c_int64, c_bf16_p, C.c_int64, C.c_int32, C.c_int32, c_bf16_p,
                                         c_bf16_p, C.c_int64, c_i32_p, C.c_int32, C.c_float, C.c_int32, C.c_void_p]),
    "omni_adaln_modulate_fp8": (C.c_int, [c_bf16_p, C.c_int64, C.c_int32, C.c_int32, c_bf16_p, c_bf16_p, C.c_int64, c_i32_p,
                                          C.c_int32, C.c_float, c_bf16_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                          C.c_void_p]),
    "omni_adaln_modulate_pair": (C.c_int, [C.POINTER(AdalnStream), C.POINTER(AdalnStream), C.c_int32, C.c_int64, C.c_float,
                                           C.c_void_p]),                                                        # ABI v12
    "omni_gemm_splitk_factor": (C.c_int, [C.POINTER(GemmParams)]),                                              # ABI v13
    "omni_splitk_finish_adaln_pair": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.POINTER(FinishAdalnStream),
                                                C.POINTER(FinishAdalnStream), C.c_int32, C.c_int64, C.c_float, C.c_void_p]),  # ABI v13
    "omni_rmsnorm": (C.c_int, [c_bf16_p, C.c_int64, c_bf16_p, C.c_int64, C.c_int32, C.c_int32, c_bf16_p, C.c_float,
                               C.c_void_p]),
    "omni_qk_norm_rope": (C.c_int, [c_bf16_p, C.c_int64, C.c_int32, C.c_int32, c_bf16_p, c_bf16_p, c_bf16_p, c_bf16_p,
                                    c_i32_p, C.c_int32, C.c_float, C.c_void_p]),
    "omni_rope_interleaved": (C.c_int, [c_bf16_p, c_bf16_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_bf16_p,
                                        c_bf16_p, C.c_void_p]),
    "omni_flash_attn_fwd": (C.c_int, [c_bf16_p, c_bf16_p, c_bf16_p, c_bf16_p, C.c_int64, C.c_int64, C.c_int64,
                                      C.c_int64, c_i32_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                      C.c_void_p]),
    "omni_flash_attn_fwd_ex": (C.c_int, [c_bf16_p, c_bf16_p, c_bf16_p, c_bf16_p, C.c_int64, C.c_int64, C.c_int64,
                                         C.c_int64, c_i32_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                         C.c_int32, C.c_void_p]),
    "omni_flash_attn_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),                         # ABI v11
    "omni_flash_attn_fwd_ws": (C.c_int, [c_bf16_p, c_bf16_p, c_bf16_p, c_bf16_p, C.c_int64, C.c_int64, C.c_int64,
                                         C.c_int64, c_i32_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                         C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),         # ABI v11
    "omni_flash_attn_general": (C.c_int, [C.POINTER(AttnParams), C.c_void_p]),                      # ABI v11
    "omni_attn_quant_workspace_bytes": (C.c_size_t, [C.POINTER(AttnParams)]),                        # ABI v14
    "omni_linear_smallbatch": (C.c_int, [c_bf16_p, C.c_int64, C.c_int32, c_bf16_p, c_bf16_p, C.c_int64, C.c_int32,
                                         c_bf16_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "omni_timestep_sinusoid": (C.c_int, [c_f32_p, C.c_int32, C.c_int32, C.c_float, c_bf16_p, C.c_void_p]),
    "omni_cfg_euler_step": (C.c_int, [c_bf16_p, c_bf16_p, c_bf16_p, C.c_int32, C.c_int32, C.c_float, c_f32_p,
                                      C.c_int32, C.c_void_p]),
    "omni_cfg_euler_step_ex": (C.c_int, [c_bf16_p, c_bf16_p, c_bf16_p, C.c_int32, C.c_int32, C.c_float, c_f32_p,
                                         C.c_int32, C.c_int32, C.c_void_p]),                      # ABI v9
    "omni_vae_conv2d": (C.c_int, [C.POINTER(ConvParams), C.c_void_p]),
    "omni_vae_conv2d_fuses_norm": (C.c_int, [C.POINTER(ConvParams)]),                              # ABI v10
    "omni_vae_upsample2x_bordered": (C.c_int, [c_bf16_p, c_bf16_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "omni_vae_rmsnorm_silu": (C.c_int, [c_bf16_p, c_bf16_p, C.c_int64, C.c_int32, c_bf16_p, C.c_int32, C.c_void_p]),
    "omni_softmax_rows": (C.c_int, [c_bf16_p, C.c_int64, C.c_int64, C.c_int32, C.c_float, C.c_void_p]),
    "omni_vae_attention": (C.c_int, [c_bf16_p, c_bf16_p, c_bf16_p, c_bf16_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                     C.c_int64, C.c_int64, C.c_float, C.c_void_p]),                 # ABI v10
    "omni_dit_workspace_bytes": (C.c_size_t, [C.POINTER(DitWeights), C.c_int32, C.c_int32, C.c_int32]),
    "omni_dit_modulation_table_workspace_bytes": (C.c_size_t, [C.POINTER(DitWeights), C.c_int32]),
    "omni_dit_modulation_table": (C.c_int, [C.POINTER(DitWeights), c_bf16_p, C.c_int32, c_bf16_p, C.c_void_p, C.c_size_t,
                                            C.c_void_p]),
    "omni_dit_forward": (C.c_int, [C.POINTER(DitWeights), C.POINTER(DitBatch), C.c_void_p]),
    "omni_dit_block": (C.c_int, [C.POINTER(DitWeights), C.c_int32, C.POINTER(DitBatch), c_bf16_p, c_bf16_p, c_bf16_p,
                                 C.c_void_p]),
    "omni_dit_block_qkv": (C.c_int, [C.POINTER(DitWeights), C.c_int32, C.POINTER(DitBatch), c_bf16_p, c_bf16_p, c_bf16_p,
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p]),
    "omni_dit_block_post": (C.c_int, [C.POINTER(DitWeights), C.c_int32, C.POINTER(DitBatch), c_bf16_p, c_bf16_p, c_bf16_p,
                                      c_bf16_p, C.c_void_p]),
}

# Entry points added to ABI v14 after its first release.  The exported FUNCTIONS of a version are fixed (PROTOTYPES: exactly what
# `nm -D` lists as text), so such an entry point is exported as a const function POINTER of the same name, announced by a
# capability bit of `omni_features()`; a C caller calls it like a function, `lib()` binds the pointer's target with the same
# restype / argtypes discipline as PROTOTYPES.  name -> (restype, argtypes, feature bit)
FEATURE_PROTOTYPES = {
    "omni_cfg_euler_step_ragged": (C.c_int, [c_bf16_p, C.c_int32, c_bf16_p, C.c_int32, c_bf16_p, C.c_int32, C.c_void_p, C.c_int32,
                                             C.c_int32, C.c_int32, c_f32_p, C.c_int32, C.c_int32, C.c_void_p], 4),
    "omni_lora_merge": (C.c_int, [C.POINTER(LoraMergeParams), C.c_void_p], 8),
    "omni_qwen2_text_forward": (C.c_int, [C.POINTER(TextWeights), C.POINTER(TextBatch), C.c_void_p], 16),
    "omni_qwen2_text_workspace_bytes": (C.c_size_t, [C.POINTER(TextWeights), C.c_int32], 16),
    "omni_text_rope_neox": (C.c_int, [c_bf16_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, c_f32_p, c_f32_p, C.c_int32, c_i32_p,
                                      c_i32_p, C.c_void_p], 16),
    "omni_text_swiglu": (C.c_int, [c_bf16_p, C.c_int64, c_bf16_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p], 16),
    "omni_text_embed_gather": (C.c_int, [c_bf16_p, C.c_int32, C.c_int32, c_i32_p, C.c_int32, c_bf16_p, C.c_int64, c_i32_p,
                                         C.c_void_p], 16),
    "omni_qwen2_vision_forward": (C.c_int, [C.POINTER(VisionWeights), C.POINTER(VisionBatch), C.c_void_p], 32),
    "omni_qwen2_vision_workspace_bytes": (C.c_size_t, [C.POINTER(VisionWeights), C.c_int32], 32),
    "omni_vision_rope_pad": (C.c_int, [c_bf16_p, C.c_int64, c_bf16_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, c_f32_p, c_f32_p,
                                       C.c_void_p], 32),
    "omni_gelu_erf": (C.c_int, [c_bf16_p, C.c_int64, c_bf16_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p], 32),
    "omni_text_mrope": (C.c_int, [c_bf16_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, c_f32_p, c_f32_p, C.c_int32, c_i32_p,
                                  C.POINTER(C.c_int32), c_i32_p, C.c_void_p], 32),
    "omni_qwen2_text_forward_mm": (C.c_int, [C.POINTER(TextWeights), C.POINTER(TextBatchMm), C.c_void_p], 32),
    "omni_gemv_bf16": (C.c_int, [C.POINTER(GemvParams), C.c_void_p], 64),
    "omni_decode_attention": (C.c_int, [C.POINTER(DecodeAttnParams), C.c_void_p], 64),
    "omni_decode_attention_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32], 64),
    "omni_text_penalized_argmax": (C.c_int, [C.POINTER(PenalizedArgmaxParams), C.c_void_p], 64),
    "omni_qwen2_text_decode_state_bytes": (C.c_size_t, [C.POINTER(TextWeights), C.c_int32, C.c_int32, C.c_int32,
                                                        C.POINTER(TextDecodeLayout)], 64),
    "omni_qwen2_text_prefill": (C.c_int, [C.POINTER(TextWeights), C.POINTER(TextBatchMm), C.POINTER(TextDecodeState), C.c_void_p], 64),
    "omni_qwen2_text_decode_step": (C.c_int, [C.POINTER(TextWeights), C.POINTER(TextDecodeState), C.c_void_p], 64),
}

# symbols a library of the SAME ABI version may lack: they were added together with a field that went into former struct
# padding, which keeps the version.  `features()` is how callers ask.
OPTIONAL_SYMBOLS = ("omni_features",)
FEATURE_ATTN_F16 = 1                              # OMNI_FEATURE_ATTN_F16
FEATURE_TEACACHE_RAGGED = 2                       # OMNI_FEATURE_TEACACHE_RAGGED
FEATURE_CFG_EULER_RAGGED = 4                      # OMNI_FEATURE_CFG_EULER_RAGGED: omni_cfg_euler_step_ragged is exported
FEATURE_LORA_MERGE = 8                            # OMNI_FEATURE_LORA_MERGE: omni_lora_merge is exported
FEATURE_TEXT_ENCODER = 16                         # OMNI_FEATURE_TEXT_ENCODER: omni_qwen2_text_forward and its companions are exported
FEATURE_VISION_ENCODER = 32                       # OMNI_FEATURE_VISION_ENCODER: omni_qwen2_vision_forward, omni_qwen2_text_forward_mm and companions
FEATURE_TEXT_DECODE = 64                          # OMNI_FEATURE_TEXT_DECODE: omni_qwen2_text_prefill / _decode_step and their kernels
DECODE_ATTN_CHUNK = 64                            # OMNI_DECODE_ATTN_CHUNK: keys per workgroup of omni_decode_attention
DECODE_CUR_LEN, DECODE_ROPE_DELTA, DECODE_CUR_ID, DECODE_DONE, DECODE_N_GENERATED, DECODE_POS = range(6)   # rows of the control words
DECODE_CTRL_WORDS, DECODE_MAX_SEQ = 8, 8
ELEM_BF16, ELEM_F16 = 0, 1                        # omni_attn_params.elem_type

_lib = None
_lock = threading.Lock()


def lib() -> C.CDLL:
    """Load (once) and return the native library; raise loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise OmniNativeError(
                f"{LIB_PATH} is missing: build it with `python vllm_omni_amd/csrc/build.py` "
                "(or __graft_entry__.build()).  There is no CPU fallback for the DiT hot path.")
        dll = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            try:
                fn = getattr(dll, name)
            except AttributeError as e:  # pragma: no cover
                if name in OPTIONAL_SYMBOLS:
                    continue
                raise OmniNativeError(f"{LIB_PATH} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        for name, (res, args, _bit) in FEATURE_PROTOTYPES.items():
            try:
                entry = C.c_void_p.in_dll(dll, name).value      # the exported object is a POINTER to the function
            except ValueError:
                continue                                         # optional: callers ask features() first
            setattr(dll, name, C.CFUNCTYPE(res, *args)(entry))
        got = dll.omni_abi_version()
        if got != ABI_VERSION:
            raise OmniNativeError(f"ABI mismatch: library {got}, binding {ABI_VERSION}")
        _lib = dll
    return _lib


def check(status: int, what: str) -> None:
    if status != 0:
        msg = lib().omni_status_string(status).decode()
        raise OmniNativeError(f"{what} failed: status {status} ({msg})")


def features() -> int:
    """omni_features(): the capability bits of the loaded library; 0 for a library that does not export the symbol."""
    fn = getattr(lib(), "omni_features", None)
    return int(fn()) if fn is not None else 0
