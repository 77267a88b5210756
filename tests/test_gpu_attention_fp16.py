"""GPU parity of the fp16 instances of `flash_attn_general_kernel` (omni_attn_params.elem_type = OMNI_ELEM_F16), mostly through
the CDNA4_FLASH backend — the plug-in point through which the reference's other DiTs reach this library, and which the reference
runs in fp16 as well as bf16 (vllm_omni/diffusion/data.py:418-436).

Checker: `O.sdpa_nhd_general` in fp32 on the fp16-rounded inputs (the oracle of tests/test_gpu_attention_general.py).
Bars, for every case:
  1. the fixed bars of the bf16 file: rel_l2 <= 4e-3 and max |err| <= 2e-2;
  2. on the SAME fp32 draw, the fp16 run's rel_l2 (against the oracle on its own rounded inputs) does not exceed that of the bf16
     general kernel (against the oracle on ITS rounded inputs).  The bf16 kernel is unchanged code, so it is the yardstick; fp16
     rounds P and the output to 11 significant bits against 8, so this holds with a factor of several to spare.  Both are printed;
  3. the output is fp16 and finite.
Measured on an MI355X (this file's own output): every case passes; fp16 / bf16 rel_l2 lies between 0.111 and 0.131 (2^-3) — see
profiles/attention_fp16_first_measurement.txt for the table and the subnormal-P finding of the flat-tail case.
"""
import ctypes
import math

import pytest
import torch

import qwen_image_oracle as O
from _util import rel_l2

pytestmark = pytest.mark.gpu
F16, BF16 = torch.float16, torch.bfloat16
DEV = "cuda:0"


def draw(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def rounded(t, dtype):
    return t.to(dtype).to(torch.float32)


def g_(t, dtype):
    return t.to(DEV, dtype).contiguous()


def impl_for(H, dh, causal=False, Hkv=None):
    from vllm_omni_amd.diffusion.attention.backends.cdna4_flash import CDNA4FlashBackend

    return CDNA4FlashBackend.get_impl_cls()(num_heads=H, head_size=dh, softmax_scale=1 / math.sqrt(dh), causal=causal, num_kv_heads=Hkv)


def general(q, k, v, scale, causal=False, mask=None):
    """`omni_flash_attn_general` on [B, S, H, dh] tensors, whatever their dtype and geometry (the backend sends bf16 self-attention
    of head size 128 to the tuned kernels; the yardstick of bar 2 is the GENERAL kernel)."""
    from vllm_omni_amd import ops
    from vllm_omni_amd.diffusion.attention.backends.cdna4_flash import _mask_strides

    B, Sq, H, dh = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    cq = (torch.arange(B + 1, dtype=torch.int32) * Sq).to(DEV)
    ck = (torch.arange(B + 1, dtype=torch.int32) * Sk).to(DEV)
    m, st = (None, None) if mask is None else _mask_strides(mask.to(DEV), B, H, Sq, Sk)
    out = ops.flash_attn_general(q.reshape(B * Sq, H * dh), k.reshape(B * Sk, Hkv * dh), v.reshape(B * Sk, Hkv * dh), cq, ck, H, Hkv,
                                 Sq, Sk, scale, causal=causal, mask=m, mask_strides=st)
    return out.view(B, Sq, H, dh)


def check(got, ref, what="", vscale=1.0):
    """Bars 1 and 3.  `vscale`: the magnitude V was drawn at (the kernel is linear in V: the absolute bar, which the bf16 file
    states for unit-scale V, scales with it — used by the large-magnitude case only)."""
    torch.cuda.synchronize()
    assert got.dtype == F16
    assert torch.isfinite(got.float()).all()
    r, mx = rel_l2(got, ref), float((got.float().cpu() - ref).abs().max())
    print(f"{what} fp16: rel_l2 {r:.3e} max|err| {mx:.3e}")
    assert r <= 4e-3, r
    assert mx <= 2e-2 * vscale, mx
    return r


def check_against_bf16(name, q, k, v, scale, *, causal=False, mask=None, Hkv=None, vscale=1.0):
    """All three bars for one fp32 draw (q, k, v): the fp16 run through the backend, the bf16 general kernel next to it."""
    from vllm_omni_amd.diffusion.attention.backends.abstract import AttentionMetadata

    H, dh = q.shape[2], q.shape[3]
    rm = mask.float() if mask is not None and mask.dtype not in (torch.bool, torch.float32) else mask     # the oracle adds fp32
    refs = {dt: O.sdpa_nhd_general(rounded(q, dt), rounded(k, dt), rounded(v, dt), scale, attn_mask=rm, is_causal=causal) for dt in (F16, BF16)}
    md = AttentionMetadata(attn_mask=None if mask is None else mask.to(DEV))
    got = impl_for(H, dh, causal=causal, Hkv=Hkv).forward(g_(q, F16), g_(k, F16), g_(v, F16), md)
    assert got.shape == q.shape
    r16 = check(got, refs[F16], name, vscale)
    yard = general(g_(q, BF16), g_(k, BF16), g_(v, BF16), scale, causal=causal, mask=mask)
    torch.cuda.synchronize()
    rbf = rel_l2(yard, refs[BF16])
    print(f"{name} rel_l2 fp16 {r16:.3e}  bf16 general kernel {rbf:.3e}  ratio {r16 / max(rbf, 1e-30):.3f}")
    assert r16 <= rbf, (r16, rbf)
    return got, refs[F16]


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("B,Sq,Sk,H", [(2, 300, 77, 4), (1, 1560, 512, 12), (3, 64, 1000, 2), (2, 129, 1, 3), (1, 1, 130, 2)])
def test_cross_attention_fp16(dh, B, Sq, Sk, H):
    q, k, v = draw((B, Sq, H, dh), 1), draw((B, Sk, H, dh), 2), draw((B, Sk, H, dh), 3)
    check_against_bf16(f"cross dh{dh} {B}x{Sq}x{Sk}x{H}", q, k, v, 1 / math.sqrt(dh))


def test_self_attention_head_size_64_fp16():
    """sd3 geometry: 24 heads of 64, S = 4096 + 154."""
    B, S, H = 1, 4096 + 154, 24
    q, k, v = draw((B, S, H, 64), 4), draw((B, S, H, 64), 5), draw((B, S, H, 64), 6)
    check_against_bf16("self dh64 S4250 H24", q, k, v, 0.125)


def test_self_attention_head_size_128_no_mask_fp16_runs_on_the_general_kernel(monkeypatch):
    """S = 4160, head size 128, no mask: the shape bf16 sends to the tuned kernels.  In fp16 the backend must NOT (they are
    bf16-only) — it goes to the general kernel and returns fp16."""
    from vllm_omni_amd import ops

    tuned = []
    orig = ops.flash_attn_varlen
    monkeypatch.setattr(ops, "flash_attn_varlen", lambda *a, **kw: tuned.append(1) or orig(*a, **kw))
    B, S, H = 1, 4160, 4
    q, k, v = draw((B, S, H, 128), 7), draw((B, S, H, 128), 8), draw((B, S, H, 128), 9)
    check_against_bf16("self dh128 S4160 H4", q, k, v, 1 / math.sqrt(128))
    assert not tuned


@pytest.mark.parametrize("dh", [64, 128])
def test_key_padding_bool_mask_fp16(dh):
    B, Sq, Sk, H = 3, 200, 190, 4
    q, k, v = draw((B, Sq, H, dh), 10), draw((B, Sk, H, dh), 11), draw((B, Sk, H, dh), 12)
    mask = torch.zeros(B, 1, 1, Sk, dtype=torch.bool)
    for i, n in enumerate([190, 77, 1]):
        mask[i, ..., :n] = True
    check_against_bf16(f"keypad dh{dh}", q, k, v, 1 / math.sqrt(dh), mask=mask)


@pytest.mark.parametrize("mdtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", ["bhqk", "b11k"])
@pytest.mark.parametrize("dh", [64, 128])
def test_additive_masks_fp16(mdtype, shape, dh):
    """fp32 and bf16 additive masks reach the kernel as they are (a bf16 mask stays bf16 next to fp16 q / k / v); an fp16 mask
    arrives as fp32 (`_mask_strides`)."""
    B, Sq, Sk, H = 2, 150, 210, 3
    q, k, v = draw((B, Sq, H, dh), 13), draw((B, Sk, H, dh), 14), draw((B, Sk, H, dh), 15)
    full = {"bhqk": (B, H, Sq, Sk), "b11k": (B, 1, 1, Sk)}[shape]
    bias = (draw(full, 16) * 2.0).to(mdtype)
    bias.view(-1)[::7] = float("-inf")
    check_against_bf16(f"additive {mdtype} {shape} dh{dh}", q, k, v, 1 / math.sqrt(dh), mask=bias)


def test_fully_masked_rows_give_zeros_fp16():
    B, Sq, Sk, H, dh = 1, 140, 100, 2, 64
    q, k, v = draw((B, Sq, H, dh), 17), draw((B, Sk, H, dh), 18), draw((B, Sk, H, dh), 19)
    mask = torch.rand(B, H, Sq, Sk, generator=torch.Generator().manual_seed(20)) > 0.4
    mask[0, 0, 5] = False
    mask[0, 1, 139] = False
    got, _ = check_against_bf16("dense bool with dead rows", q, k, v, 0.125, mask=mask)
    assert float(got[0, 5, 0].abs().max()) == 0.0 and float(got[0, 139, 1].abs().max()) == 0.0


@pytest.mark.parametrize("dh,Sq,Sk", [(128, 300, 300), (64, 513, 513), (128, 100, 260), (64, 260, 100)])
def test_causal_fp16(dh, Sq, Sk):
    B, H = 2, 3
    q, k, v = draw((B, Sq, H, dh), 21), draw((B, Sk, H, dh), 22), draw((B, Sk, H, dh), 23)
    check_against_bf16(f"causal dh{dh} {Sq}x{Sk}", q, k, v, 1 / math.sqrt(dh), causal=True)


@pytest.mark.parametrize("dh", [64, 128])
def test_grouped_kv_heads_fp16(dh):
    B, Sq, Sk, H, Hkv = 2, 130, 200, 8, 2
    q, k, v = draw((B, Sq, H, dh), 24), draw((B, Sk, Hkv, dh), 25), draw((B, Sk, Hkv, dh), 26)
    check_against_bf16(f"gqa dh{dh}", q, k, v, 1 / math.sqrt(dh), Hkv=Hkv)


@pytest.mark.parametrize("dh", [64, 128])
def test_unequal_cu_seqlens_fp16(dh):
    """Different lengths per item on both sides, a strided q (a column slice of a fused projection), through the ops wrapper."""
    from vllm_omni_amd import ops

    H = 4
    ql, kl = [130, 1, 300], [77, 512, 65]
    qkv = draw((sum(ql), 3 * H * dh), 27, 0.5)
    k, v = draw((sum(kl), H * dh), 28, 0.5), draw((sum(kl), H * dh), 29)
    cq = torch.tensor([0] + list(torch.tensor(ql).cumsum(0)), dtype=torch.int32, device=DEV)
    ck = torch.tensor([0] + list(torch.tensor(kl).cumsum(0)), dtype=torch.int32, device=DEV)
    scale = 1 / math.sqrt(dh)
    outs = {dt: ops.flash_attn_general(g_(qkv, dt)[:, H * dh:2 * H * dh], g_(k, dt), g_(v, dt), cq, ck, H, H, max(ql), max(kl), scale)
            for dt in (F16, BF16)}
    torch.cuda.synchronize()
    assert outs[F16].dtype == F16 and outs[BF16].dtype == BF16
    refs = {}
    for dt in (F16, BF16):
        q_, k_, v_ = rounded(qkv[:, H * dh:2 * H * dh], dt), rounded(k, dt), rounded(v, dt)
        parts, qo, ko = [], 0, 0
        for a, b in zip(ql, kl):
            parts.append(O.sdpa_nhd_general(q_[qo:qo + a].reshape(1, a, H, dh), k_[ko:ko + b].reshape(1, b, H, dh),
                                            v_[ko:ko + b].reshape(1, b, H, dh), scale).reshape(a, H * dh))
            qo, ko = qo + a, ko + b
        refs[dt] = torch.cat(parts)
    r16 = check(outs[F16], refs[F16], f"ragged dh{dh}")
    rbf = rel_l2(outs[BF16], refs[BF16])
    print(f"ragged dh{dh} rel_l2 fp16 {r16:.3e}  bf16 general kernel {rbf:.3e}")
    assert r16 <= rbf


@pytest.mark.parametrize("dh", [64, 128])
def test_flat_tail_keeps_its_mass_fp16(dh):
    """The subnormal question.  One dominant key and 4095 keys whose logits sit 10 to 13 nats below it: every tail P =
    exp(-10 .. -13) = 4.5e-5 .. 2.3e-6 lies below fp16's smallest normal number (6.1e-5), yet together the tail carries a few
    per cent of the softmax mass.  V tells the two apart: channel 0 is 0 at the dominant key and +1 on the tail, so output
    channel 0 IS the tail's share.  A kernel that lost the tail (P flushed on its way through the fp16 MFMA) would return 0
    there while the row sum still counted it: an error of the whole share, above the absolute bar."""
    B, Sq, Sk, H = 1, 64, 4096, 2
    scale = 1 / math.sqrt(dh)
    q = torch.zeros(B, Sq, H, dh)
    q[..., 0] = 1 / scale                                   # logit of key j = k[j, 0]
    q[..., 1:] = draw((B, Sq, H, dh - 1), 30) * 0.01          # (the other channels of k are 0)
    k = torch.zeros(B, Sk, H, dh)
    k[..., 0] = torch.rand(B, Sk, H, generator=torch.Generator().manual_seed(31)) * 3.0       # tail: 0 .. 3
    dom = 1000                                             # not in the first tile: the running max moves late
    k[:, dom, :, 0] = 13.0                                   # dominant key: 10 .. 13 nats above every tail key
    v = draw((B, Sk, H, dh), 32)
    v[..., 0] = 1.0
    v[:, dom, :, 0] = 0.0
    ref = O.sdpa_nhd_general(rounded(q, F16), rounded(k, F16), rounded(v, F16), scale)
    share = ref[..., 0]
    print(f"flat tail dh{dh}: tail share of the softmax mass in the fp32 oracle: min {float(share.min()):.4f} max {float(share.max()):.4f}")
    assert 0.02 < float(share.min()) and float(share.max()) < 0.10            # a few per cent, by construction
    got, _ = check_against_bf16(f"flat tail dh{dh}", q, k, v, scale)
    kept = got[..., 0].float().cpu()
    print(f"flat tail dh{dh}: tail share the fp16 kernel returns: min {float(kept.min()):.4f} max {float(kept.max()):.4f}")
    assert float((kept - share).abs().max()) <= 2e-2 and rel_l2(kept, share) <= 4e-3


@pytest.mark.parametrize("dh", [64, 128])
def test_large_magnitude_v_stays_finite_fp16(dh):
    """|v| up to 6e4 (fp16's largest finite number is 65504).  A softmax average cannot exceed max |v|, the accumulators are
    fp32, so nothing may overflow.  The absolute bar of the bf16 file is stated for unit-scale V; the kernel is linear in V, so
    here it is that bar times the scale V was drawn at (half an fp16 ulp at 4096 is already 2: no fp16 result of this size
    can meet 2e-2 unscaled).  The relative bar and the comparison with the bf16 kernel need no scaling."""
    B, Sq, Sk, H = 2, 200, 333, 3
    vmax = 6.0e4
    q, k = draw((B, Sq, H, dh), 33), draw((B, Sk, H, dh), 34)
    v = (torch.rand(B, Sk, H, dh, generator=torch.Generator().manual_seed(35)) * 2 - 1) * vmax
    v[0, 0], v[1, 5] = vmax, -vmax
    q[0, 0] = k[0, 0] * 4.0                                  # one query that attends almost only to the all-6e4 key
    got, _ = check_against_bf16(f"large V dh{dh}", q, k, v, 1 / math.sqrt(dh), vscale=vmax)
    assert float(got.float().abs().max()) <= float(rounded(v, F16).abs().max())
    assert float(got[0, 0].float().min()) > 0.9 * vmax


def test_qk_int8_with_fp16_is_unsupported():
    from vllm_omni_amd import _native as N
    from vllm_omni_amd import ops

    x = torch.zeros(128, 128, device=DEV, dtype=F16)
    cu = torch.tensor([0, 128], dtype=torch.int32, device=DEV)
    with pytest.raises(N.OmniNativeError, match=r"status -2"):
        ops.flash_attn_general(x, x, x, cu, cu, 1, 1, 128, 128, 0.1, qk_int8=True)


def test_unknown_elem_type_is_a_bad_argument():
    from vllm_omni_amd import _native as N

    x = torch.zeros(128, 128, device=DEV, dtype=F16)
    o = torch.empty_like(x)
    cu = torch.tensor([0, 128], dtype=torch.int32, device=DEV)
    p = N.AttnParams()
    p.q = p.k = p.v = x.data_ptr()
    p.out = o.data_ptr()
    p.ldq = p.ldk = p.ldv = p.ldo = 128
    p.cu_seqlens_q = p.cu_seqlens_k = cu.data_ptr()
    p.B, p.H, p.H_kv, p.head_dim, p.max_seqlen_q, p.max_seqlen_k, p.softmax_scale = 1, 1, 1, 128, 128, 128, 0.1
    for bad in (7, 2, -1):
        p.elem_type = bad
        assert N.lib().omni_flash_attn_general(ctypes.byref(p), torch.cuda.current_stream().cuda_stream) == -1     # OMNI_ERR_BAD_ARG
    for good in (0, 1):
        p.elem_type = good
        assert N.lib().omni_flash_attn_general(ctypes.byref(p), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()


def test_fp16_is_refused_when_the_library_lacks_the_feature_bit(monkeypatch):
    from vllm_omni_amd import _native as N

    monkeypatch.setattr(N, "features", lambda: 0)
    q = torch.zeros(1, 64, 2, 64, device=DEV, dtype=F16)
    with pytest.raises(N.OmniNativeError, match="OMNI_FEATURE_ATTN_F16"):
        impl_for(2, 64).forward(q, q, q, None)
    impl_for(2, 64).forward(q.to(BF16), q.to(BF16), q.to(BF16), None)           # bf16 does not ask
    torch.cuda.synchronize()


def test_bf16_results_do_not_change_around_an_fp16_call():
    """elem_type left 0: the same bf16 call before and after an fp16 call gives the same bits (one pair of runs)."""
    B, Sq, Sk, H, dh = 2, 300, 333, 4, 128
    q, k, v = draw((B, Sq, H, dh), 36), draw((B, Sk, H, dh), 37), draw((B, Sk, H, dh), 38)
    scale = 1 / math.sqrt(dh)
    before = general(g_(q, BF16), g_(k, BF16), g_(v, BF16), scale).clone()
    between = general(g_(q, F16), g_(k, F16), g_(v, F16), scale)
    after = general(g_(q, BF16), g_(k, BF16), g_(v, BF16), scale)
    torch.cuda.synchronize()
    assert between.dtype == F16 and before.dtype == BF16
    assert torch.equal(before, after)
    check(between, O.sdpa_nhd_general(rounded(q, F16), rounded(k, F16), rounded(v, F16), scale), "interleaved")
