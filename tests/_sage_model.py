"""Host model of the SAGE_ATTN algorithm (SageAttention v1: int8 Q K^T with per-block scales and a smoothed K, fp32 softmax,
bf16 P V), the arithmetic csrc/attention_sage.hip implements.  Per item (cu_seqlens segment) and per head:

  1. km = mean_j k[j] (fp32); k' = k - km                        (adds q . km to every logit of a row: softmax unchanged)
  2. q *= softmax_scale * log2(e) (unless prescaled); per 64-row block from the item's first row: sq = amax|q| / 127,
     q8 = rne(q / sq) clamped to +-127
  3. same on k' per 64-row block: sk, k8; an all-zero block gets scale 1
  4. s = float(q8 . k8^T) * sq * sk (log2 domain); p = exp2(s - max); P rounded to bf16; out = (P V) / sum(p), bf16

Also the test-data generator the host and GPU tests share: RMS-normed q / k with a large per-channel k offset (what real
checkpoints' k carry and what the smoothing step exists for)."""
import math

import torch

LOG2E = 1.4426950408889634
BLK = 64


def quant_blocks(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """x [L, H, dh] fp32 -> (int8 [L, H, dh], fp32 scales [ceil(L/64), H]); blocks of 64 rows from row 0."""
    L, H, dh = x.shape
    nb = (L + BLK - 1) // BLK
    pad = torch.zeros(nb * BLK, H, dh, dtype=torch.float32, device=x.device)
    pad[:L] = x
    amax = pad.view(nb, BLK, H, dh).abs().amax(dim=(1, 3))                       # [nb, H]
    sc = torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))
    q8 = torch.round(pad.view(nb, BLK, H, dh) / sc[:, None, :, None]).clamp(-127, 127)
    return q8.reshape(nb * BLK, H, dh)[:L].to(torch.int8), sc


def quantize_item(q: torch.Tensor, k: torch.Tensor, scale_log2: float, smooth: bool = True):
    """q [Lq, H, dh], k [Lk, H, dh] (any float dtype) -> q8, sq, k8, sk, km [H, dh].  scale_log2 = softmax_scale * log2(e),
    or 1.0 for a prescaled q."""
    qf = q.float() * scale_log2 if scale_log2 != 1.0 else q.float()
    kf = k.float()
    km = kf.mean(dim=0) if smooth else torch.zeros(kf.shape[1:], dtype=torch.float32, device=kf.device)
    q8, sq = quant_blocks(qf)
    k8, sk = quant_blocks(kf - km)
    return q8, sq, k8, sk, km


def attend_int8(q8, sq, k8, sk, v: torch.Tensor) -> torch.Tensor:
    """One item: int8 operands + scales -> [Lq, H, dh] fp32 (before the final bf16 rounding)."""
    Lq, H, dh = q8.shape
    Lk = k8.shape[0]
    dev = q8.device
    rq = torch.arange(Lq, device=dev) // BLK
    rk = torch.arange(Lk, device=dev) // BLK
    out = torch.empty(Lq, H, dh, dtype=torch.float32, device=dev)
    vf = v.float()
    for h in range(H):
        # exact: |q8 . k8| <= 127^2 * 256 < 2^24, so fp32 products and sums of integers are exact (torch has no int GEMM on GPU)
        s = q8[:, h].float() @ k8[:, h].float().T
        s = s * sq[rq, h][:, None] * sk[rk, h][None, :]
        m = s.amax(dim=1, keepdim=True)
        p = torch.exp2(s - m)
        lsum = p.sum(dim=1, keepdim=True)
        out[:, h] = (p.bfloat16().float() @ vf[:, h]) / lsum
    return out


def sage_attention(q, k, v, cu_q, cu_k, softmax_scale: float, smooth: bool = True, prescaled: bool = False) -> torch.Tensor:
    """q [Rq, H, dh], k / v [Rk, H, dh]; cu_q / cu_k host int lists (B + 1 prefix sums).  Returns [Rq, H, dh] fp32."""
    out = torch.zeros(q.shape, dtype=torch.float32, device=q.device)
    c = 1.0 if prescaled else softmax_scale * LOG2E
    for b in range(len(cu_q) - 1):
        qs, qe, ks, ke = cu_q[b], cu_q[b + 1], cu_k[b], cu_k[b + 1]
        if qe == qs or ke == ks:
            continue
        q8, sq, k8, sk, _ = quantize_item(q[qs:qe], k[ks:ke], c, smooth)
        out[qs:qe] = attend_int8(q8, sq, k8, sk, v[ks:ke])
    return out


def sdpa_fp32(q, k, v, cu_q, cu_k, softmax_scale: float) -> torch.Tensor:
    out = torch.zeros(q.shape, dtype=torch.float32, device=q.device)
    for b in range(len(cu_q) - 1):
        qs, qe, ks, ke = cu_q[b], cu_q[b + 1], cu_k[b], cu_k[b + 1]
        if qe == qs or ke == ks:
            continue
        qh, kh, vh = (t.float().permute(1, 0, 2) for t in (q[qs:qe], k[ks:ke], v[ks:ke]))
        o = torch.nn.functional.scaled_dot_product_attention(qh[None], kh[None], vh[None], scale=softmax_scale)[0]
        out[qs:qe] = o.permute(1, 0, 2)
    return out


def make_qkv(rows_q: int, rows_k: int, H: int, dh: int, seed: int = 0, k_offset: float = 3.0, norm_weight: float = 0.75,
             device="cpu"):
    """bf16 q / k / v [rows, H, dh]: q, k RMS-normed per head with norm weights around `norm_weight` (the model's q/k norm;
    0.75 gives logits of about 0.6 standard deviations), then k shifted by a per-(head, channel) offset of `k_offset` (the
    shared key direction of real checkpoints, which the smoothing removes); v unit Gaussian."""
    g = torch.Generator().manual_seed(seed)

    def rms(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * w

    wq = norm_weight * (1.0 + 0.2 * torch.randn(H, dh, generator=g))
    wk = norm_weight * (1.0 + 0.2 * torch.randn(H, dh, generator=g))
    q = rms(torch.randn(rows_q, H, dh, generator=g), wq)
    k = rms(torch.randn(rows_k, H, dh, generator=g), wk) + k_offset * torch.randn(H, dh, generator=g)
    v = torch.randn(rows_k, H, dh, generator=g)
    return tuple(t.bfloat16().to(device) for t in (q, k, v))


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.float(), b.float()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def default_scale(dh: int) -> float:
    return 1.0 / math.sqrt(dh)
