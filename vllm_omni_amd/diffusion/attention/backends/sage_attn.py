"""SAGE_ATTN attention backend — the reference's `SageAttentionBackend` / `SageAttentionImpl`
(vllm_omni/diffusion/attention/backends/sage_attn.py), which calls `sageattn(q, k, v, tensor_layout="NHD", is_causal=...,
sm_scale=...)`: SageAttention v1, int8 Q K^T with per-block scales and a smoothed K, fp32 softmax, 16-bit P V.  Here the same
algorithm runs in HIP (csrc/attention_sage.hip, `omni_flash_attn_general` with `qk_int8 = 1`; host model tests/_sage_model.py).

Divergences from the reference, all of them refusals instead of a silently different computation:
  * `attn_metadata.attn_mask` — the reference's forward drops it without a word; this build raises ValueError;
  * `causal=True` and head sizes other than 64 / 128 raise ValueError at construction (the reference advertises 32 .. 256);
  * inputs must be bf16 (the kernel's operands); fp16 / fp32 raise ValueError rather than being cast.
The Qwen-Image DiT does not come through this class: it reads the same selector and runs the int8 attention inside its native
block (`omni_dit_batch.attn_qk_int8`)."""
import torch

from .... import ops
from .abstract import AttentionBackend, AttentionImpl, AttentionMetadata

HEAD_SIZES = (64, 128)


class SageAttentionImpl(AttentionImpl):
    def __init__(self, num_heads: int, head_size: int, softmax_scale: float, causal: bool = False,
                 num_kv_heads: int | None = None, prefix: str = "", **extra_impl_args) -> None:
        super().__init__(num_heads, head_size, softmax_scale, causal, num_kv_heads, prefix)
        if head_size not in HEAD_SIZES:
            raise ValueError(f"SAGE_ATTN is built for head sizes {HEAD_SIZES}, got {head_size}")
        if causal:
            raise ValueError("SAGE_ATTN does not take causal attention (unset DIFFUSION_ATTENTION_BACKEND for CDNA4_FLASH)")
        if num_heads % self.num_kv_heads:
            raise ValueError("num_heads must be a multiple of num_kv_heads")
        self._cu = {}
        self._ws = None

    def _cu_seqlens(self, B: int, S: int, device) -> torch.Tensor:
        cu = self._cu.get((B, S, device))
        if cu is None:
            cu = (torch.arange(B + 1, dtype=torch.int32) * S).to(device)
            self._cu[(B, S, device)] = cu
        return cu

    def forward(self, query, key, value, attn_metadata: AttentionMetadata = None) -> torch.Tensor:
        if attn_metadata is not None and attn_metadata.attn_mask is not None:
            raise ValueError("SAGE_ATTN takes no attention mask (the reference's sageattn call drops it; this build refuses "
                             "instead): unset DIFFUSION_ATTENTION_BACKEND for CDNA4_FLASH, which honours masks")
        if any(t.dtype != torch.bfloat16 for t in (query, key, value)):
            raise ValueError(f"SAGE_ATTN takes bf16 q / k / v, got {query.dtype} / {key.dtype} / {value.dtype}")
        B, Sq, H, dh = query.shape
        Sk, Hkv = key.shape[1], key.shape[2]
        if H != self.num_heads or dh != self.head_size or Hkv != self.num_kv_heads or value.shape != key.shape or key.shape[0] != B:
            raise ValueError(f"q {tuple(query.shape)} / k {tuple(key.shape)} / v {tuple(value.shape)} do not match "
                             f"num_heads {self.num_heads}, num_kv_heads {self.num_kv_heads}, head_size {self.head_size}")
        need = ops.attn_quant_workspace_bytes(B, H, Hkv, dh, Sq, Sk)
        if self._ws is None or self._ws.numel() < need or self._ws.device != query.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=query.device)
        q2 = query.reshape(B * Sq, H * dh)
        k2, v2 = key.reshape(B * Sk, Hkv * dh), value.reshape(B * Sk, Hkv * dh)
        out = ops.flash_attn_general(q2, k2, v2, self._cu_seqlens(B, Sq, query.device), self._cu_seqlens(B, Sk, query.device),
                                     H, Hkv, Sq, Sk, self.softmax_scale, qk_int8=True, workspace=self._ws)
        return out.view(B, Sq, H, dh)


class SageAttentionBackend(AttentionBackend):
    accept_output_buffer = True
    NAME = "SAGE_ATTN"
    IMPL = SageAttentionImpl
    HEAD_SIZES = HEAD_SIZES
