"""GPU: the native Qwen2.5-VL prompt encoder - its three row kernels against fp32 torch, the whole forward against the SAME HF
model run in fp32, and a text-to-image request from prompt strings with the native encoder against the HF encoder.

Bars:
  row kernels      |err| <= 2^-7 (|ref| + rms(ref)) per element: the project's elementwise bar (one bf16 rounding of fp32 arithmetic).
  whole forward    the oracle is HF in fp32 on the same bf16 weights and tokens.  d_eager = rel-L2 of HF's own bf16 eager pass
                   against it - what the path being replaced loses to bf16 - and the native pass may lose at most a quarter more:
                   d_native <= 1.25 d_eager, cos >= 0.9995.  The quarter covers a different summation order (MFMA tiles, split-K)
                   and HF's additional bf16 roundings (bf16 RoPE tables, every elementwise op rounded) cutting either way at a
                   depth of one or two layers.
  pipeline         final latents within the project's <= 4-layer forward bar: rel-L2 <= 1e-2, cos >= 0.9995.
The HF models are built in fp32 and cast to bf16 with their rotary frequencies kept in fp32, as a checkpoint load leaves them (a
plain `.to(bfloat16)` of the module would round the inv_freq buffer as well and hand HF eager different angles than its config)."""
import copy

import pytest
import torch

from _util import cosine, rel_l2

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = torch.device("cuda:0")


def elem_close(got, ref, what=""):
    ref, got = ref.float().cpu(), got.float().cpu()
    rms = ref.pow(2).mean().sqrt()
    err = ((got - ref).abs() / (ref.abs() + rms)).max().item()
    print(f"{what}: max scaled err {err:.3e} (bar {2 ** -7:.3e})")
    assert err <= 2 ** -7, f"{what}: max scaled err {err}"


# ------------------------------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("heads", [(4, 2), (28, 4)])
@pytest.mark.parametrize("rows", [1, 63, 65, 257])
def test_text_rope_neox_against_fp32(rows, heads):
    from vllm_omni_amd import ops
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import text_rope_tables

    H, Hkv = heads
    g = torch.Generator().manual_seed(100 * rows + H)
    qkv = torch.randn(rows, (H + 2 * Hkv) * 128, generator=g).to(BF16)
    pos = torch.randint(0, 1101, (rows,), generator=g, dtype=torch.int32)
    pos[0], pos[-1] = 0, 1100                                          # (one row: position 1100)
    cos, sin = text_rope_tables(1000000.0, 1101)
    x = qkv.float().view(rows, H + 2 * Hkv, 128)
    c, s = cos[pos.long()][:, None, :], sin[pos.long()][:, None, :]
    lo, hi = x[..., :64], x[..., 64:]
    ref = x.clone()
    ref[:, :H + Hkv] = torch.cat([lo * c - hi * s, hi * c + lo * s], dim=-1)[:, :H + Hkv]
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = ops.text_rope_neox_(qkv.to(DEV), H, Hkv, cos.to(DEV), sin.to(DEV), pos.to(DEV), err=err).cpu().view(rows, -1, 128)
    elem_close(got[:, :H + Hkv], ref[:, :H + Hkv], f"rope rows={rows} heads={heads}")
    assert torch.equal(got[:, H + Hkv:], qkv.view(rows, -1, 128)[:, H + Hkv:])       # v: untouched, bit for bit
    assert int(err.item()) == 0


def test_text_rope_neox_row_stride_and_position_clamp():
    from vllm_omni_amd import ops
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import text_rope_tables

    H, Hkv, rows, ld = 4, 2, 5, 8 * 128 + 64
    g = torch.Generator().manual_seed(3)
    buf = torch.randn(rows, ld, generator=g).to(BF16)
    pos = torch.tensor([0, 7, 1100, 1101, -1], dtype=torch.int32)      # the last two lie outside the table: clamped, reported
    cos, sin = text_rope_tables(1000000.0, 1101)
    pc = pos.clamp(0, 1100).long()
    x = buf[:, :8 * 128].float().view(rows, 8, 128)
    c, s = cos[pc][:, None, :], sin[pc][:, None, :]
    rot = torch.cat([x[..., :64] * c - x[..., 64:] * s, x[..., 64:] * c + x[..., :64] * s], dim=-1)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    dbuf = buf.to(DEV)
    ops.text_rope_neox_(dbuf[:, :8 * 128], H, Hkv, cos.to(DEV), sin.to(DEV), pos.to(DEV), err=err)
    got = dbuf.cpu()
    elem_close(got[:, :6 * 128].reshape(rows, 6, 128), rot[:, :6], "rope row stride")
    assert torch.equal(got[:, 6 * 128:], buf[:, 6 * 128:])             # v and the 64 columns behind the row: untouched
    assert int(err.item()) != 0


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("inter", [192, 18944])
@pytest.mark.parametrize("rows", [1, 65, 257])
def test_text_swiglu_against_fp32(rows, inter, blocked):
    from vllm_omni_amd import ops

    g = torch.Generator().manual_seed(rows + inter)
    gu = (torch.randn(rows, 2 * inter, generator=g) * 2).to(BF16)
    ref = torch.nn.functional.silu(gu[:, :inter].float()) * gu[:, inter:].float()
    got = ops.text_swiglu(gu.to(DEV), out_k32_blocked=blocked)
    if blocked:
        got = ops.k32_blocked_to_rows(got)
    elem_close(got, ref, f"swiglu rows={rows} I={inter} blocked={blocked}")


def test_embedding_gather_is_exact_and_never_reads_out_of_range():
    from vllm_omni_amd import ops

    g = torch.Generator().manual_seed(9)
    table = torch.randn(259, 3584, generator=g).to(BF16)
    ids = torch.randint(0, 259, (131,), generator=g, dtype=torch.int32)
    ids[0], ids[-1] = 0, 258
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = ops.text_embed_gather(table.to(DEV), ids.to(DEV), err)
    assert torch.equal(got.cpu(), table[ids.long()]) and int(err.item()) == 0
    bad = ids.clone()
    bad[5], bad[77] = 259, -1
    got = ops.text_embed_gather(table.to(DEV), bad.to(DEV), err).cpu()
    assert int(err.item()) == 1
    assert not got[5].any() and not got[77].any()                      # zero rows, not whatever lies behind the table
    keep = torch.ones(131, dtype=torch.bool)
    keep[[5, 77]] = False
    assert torch.equal(got[keep], table[ids.long()][keep])


# ------------------------------------------------------------------------------------------------------------ whole forward
def _hf_pair(hidden, layers, heads, kv, inter, seed, qk_gain=1.0):
    """(HF bf16 model, the same model in fp32) on the GPU: random weights with biases and norm weights away from their trivial
    initial values, q / k projections scaled so that the attention is not near-uniform at a small width."""
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import QwenPromptEncoder

    with torch.device(DEV):
        m = QwenPromptEncoder.random_init(hidden_size=hidden, num_layers=layers, num_heads=heads, num_kv_heads=kv,
                                          intermediate_size=inter, device=DEV, dtype=torch.float32, seed=seed).model
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    with torch.no_grad():
        for L in m.layers:
            for p in (L.self_attn.q_proj, L.self_attn.k_proj):
                p.weight.mul_(qk_gain)
            for p in (L.self_attn.q_proj, L.self_attn.k_proj, L.self_attn.v_proj):
                p.bias.copy_(torch.randn(p.bias.shape, generator=g, device=DEV) * 0.2)
            for n in (L.input_layernorm, L.post_attention_layernorm):
                n.weight.copy_(1 + 0.1 * torch.randn(n.weight.shape, generator=g, device=DEV))
        m.norm.weight.copy_(1 + 0.1 * torch.randn(m.norm.weight.shape, generator=g, device=DEV))
    inv = m.rotary_emb.inv_freq.clone()
    eager = m.to(BF16)
    eager.rotary_emb.inv_freq = inv                                    # fp32, as after a checkpoint load
    return eager.eval(), copy.deepcopy(eager).float().eval()


def _encoders(eager, oracle, **kw):
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import ByteTokenizer, NativeQwenPromptEncoder, QwenPromptEncoder

    tok = ByteTokenizer()
    return (NativeQwenPromptEncoder.from_hf(eager, tok, **kw), QwenPromptEncoder(eager, tok, dtype=BF16, **kw),
            QwenPromptEncoder(oracle, tok, dtype=torch.float32, **kw))


def _check_against_oracle(native, hf_eager, hf_oracle, prompts, what):
    ref, ref_mask = hf_oracle.get_qwen_prompt_embeds(prompts)
    eag, eag_mask = hf_eager.get_qwen_prompt_embeds(prompts)
    got, got_mask = native.get_qwen_prompt_embeds(prompts)
    again, _ = native.get_qwen_prompt_embeds(prompts)
    torch.cuda.synchronize()
    assert got.shape == eag.shape and got.dtype == eag.dtype == BF16 and got.device == eag.device
    assert torch.equal(got_mask, eag_mask) and torch.equal(got_mask, ref_mask) and got_mask.dtype == eag_mask.dtype
    assert not got[~got_mask.bool()].any()                             # padded rows: exactly zero
    assert torch.equal(got, again)                                     # two identical calls: bit-equal
    d_native, d_eager, c = rel_l2(got, ref), rel_l2(eag, ref), cosine(got, ref)
    print(f"{what}: d_native {d_native:.4e}  d_eager {d_eager:.4e}  ratio {d_native / d_eager:.3f} (bar 1.25)  cos {c:.6f} (bar 0.9995)")
    assert d_native <= 1.25 * d_eager, (what, d_native, d_eager)
    assert c >= 0.9995, (what, c)


@pytest.fixture(scope="module")
def small_models():
    return _hf_pair(512, 2, 4, 2, 192, seed=21, qk_gain=4.0)


def test_small_model_against_hf_fp32(small_models):
    """hidden 512, 4 / 2 heads of 128, I = 192, 2 layers; prompts of 33, 70 and 260 tokens (a two-token template prefix): the packed
    rows cross 32, 64 and 256, the second and third prompt start inside a 32-query wave / a 128-query block of the attention.
    Measured on MI355X: see BASELINE.md section 3."""
    eager, oracle = small_models
    native, hf_eager, hf_oracle = _encoders(eager, oracle, template="ab{}c", drop_idx=2)
    prompts = ["p" * 30, "".join(chr(97 + i % 26) for i in range(67)), "".join(chr(65 + (7 * i) % 26) for i in range(257))]
    _check_against_oracle(native, hf_eager, hf_oracle, prompts, "small model")
    assert native.get_qwen_prompt_embeds(prompts)[0].shape == (3, 258, 512)


def test_real_width_layer_against_hf_fp32():
    """One layer of the real geometry (3584 / 28 over 4 heads / 18944), prompts of about 40 and 120 tokens."""
    eager, oracle = _hf_pair(3584, 1, 28, 4, 18944, seed=22)
    native, hf_eager, hf_oracle = _encoders(eager, oracle, template="<|user|>{}<|end|>", drop_idx=8)
    prompts = ["a red cube on a wooden table", "a watercolour of a lighthouse at dusk, gulls over the breakers, " * 2]
    prompts[1] = prompts[1][:120 - 15]
    _check_against_oracle(native, hf_eager, hf_oracle, prompts, "real width")


def test_bad_token_id_is_reported_by_the_next_call_not_read(small_models):
    from vllm_omni_amd._native import OmniNativeError
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import ByteTokenizer, NativeQwenPromptEncoder

    native = NativeQwenPromptEncoder.from_hf(small_models[0], ByteTokenizer(), template="ab{}c", drop_idx=2)
    ids = torch.tensor([5, 6, 259, 8, 9], dtype=torch.int32, device=DEV)           # 259 = one past the vocabulary
    cu = torch.tensor([0, 5], dtype=torch.int32, device=DEV)
    pos = torch.arange(5, dtype=torch.int32, device=DEV)
    native.encode_packed(ids, cu, pos, 5)                              # runs (the row embeds as zeros) and raises the error word
    with pytest.raises(OmniNativeError, match="bad argument"):
        native.encode_packed(ids.clamp(max=258), cu, pos, 5)           # ... which the next call over the workspace reports
    out = native.encode_packed(ids.clamp(max=258), cu, pos, 5)         # and clears
    assert out.shape == (5, 512) and torch.isfinite(out.float()).all()
    with pytest.raises(ValueError, match="token ids"):                 # the host path refuses a bad id before it is uploaded
        class Tok(ByteTokenizer):
            def __call__(self, *a, **k):
                t = super().__call__(*a, **k)
                t.input_ids[0, 0] = 300
                return t
        NativeQwenPromptEncoder.from_hf(small_models[0], Tok(), template="ab{}c", drop_idx=2).get_qwen_prompt_embeds(["x"])


# ------------------------------------------------------------------------------------------------------------ pipeline
def test_pipeline_from_prompt_strings_native_against_hf_encoder(small_models):
    """A QwenImagePipeline (2-layer DiT at the text model's width) generating from prompt strings at 64 x 64 / 2 steps with true
    CFG: the native encoder against the HF encoder on the same weights, same starting latents."""
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.models.qwen_image.autoencoder_kl_qwenimage import AutoencoderKLQwenImage
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline
    from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest

    native, hf_eager, _ = _encoders(small_models[0], small_models[1])  # the pipeline's own template and drop index
    tr = QwenImageTransformer2DModel(num_layers=2, num_attention_heads=2, joint_attention_dim=512, device=DEV)
    tr.init_random_(seed=11)
    vae = AutoencoderKLQwenImage(device=DEV).init_random_(seed=12)
    lat = torch.randn(1, 16, 64, generator=torch.Generator().manual_seed(4)).to(BF16)
    outs = {}
    for name, enc in (("hf", hf_eager), ("native", native)):
        pipe = QwenImagePipeline(od_config=OmniDiffusionConfig(use_hip_graph=False), device=DEV, transformer=tr, vae=vae,
                                 text_encoder=enc)
        req = OmniDiffusionRequest(prompt="a red cube on a table", negative_prompt="blurry", height=64, width=64,
                                   num_inference_steps=2, true_cfg_scale=4.0, latents=lat.clone(), output_type="latent")
        outs[name] = pipe.generate([req], output_type="latent")[0].output.float().cpu()
    e, c = rel_l2(outs["native"], outs["hf"]), cosine(outs["native"], outs["hf"])
    print(f"pipeline latents: rel-L2 {e:.4e} (bar 1e-2)  cos {c:.6f} (bar 0.9995)")
    assert torch.isfinite(outs["native"]).all()
    assert e <= 1e-2 and c >= 0.9995, (e, c)
