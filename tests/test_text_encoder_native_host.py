"""CPU: the native Qwen2.5-VL prompt encoder (omni_qwen2_text_forward, NativeQwenPromptEncoder,
`OmniDiffusionConfig.native_text_encoder`) - everything about it that needs no device.

  1. ABI: the three new structs against gcc, the feature bit, the entry points as data symbols outside `PROTOTYPES`;
  2. every documented refusal of the driver, answered BEFORE any launch (the pointers are made-up addresses, never dereferenced);
  3. `from_hf`: fused matrices, the RoPE table against HF's rotary embedding, token packing against HF's positions;
  4. the config flag: off by default, honoured by the text-to-image pipeline, refused by the Edit family; an unsupported
     geometry is refused with its reason."""
import ctypes as C
import os
import subprocess
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, UNSUPPORTED, LAUNCH, ALIGN = 0, -1, -2, -3, -4
P = 0x7F0000010000          # a "device pointer": 16-byte aligned, never dereferenced
ENTRY_POINTS = ("omni_qwen2_text_forward", "omni_qwen2_text_workspace_bytes", "omni_text_rope_neox", "omni_text_swiglu",
                "omni_text_embed_gather")


# ---------------------------------------------------------------------------------------------------------------- 1
def test_text_structs_match_gcc(tmp_path):
    from vllm_omni_amd import _native as N

    pairs = [("omni_text_layer_weights", N.TextLayerWeights), ("omni_text_weights", N.TextWeights), ("omni_text_batch", N.TextBatch)]
    body = ""
    for cname, cls in pairs:
        body += f'  printf("%zu", sizeof({cname}));\n'
        body += "".join(f'  printf(" %zu", offsetof({cname}, {f}));\n' for f, _ in cls._fields_) + '  printf("\\n");\n'
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "omni_cdna4.h"\nint main(void) {\n' + body
                   + '  printf("%u\\n", OMNI_FEATURE_TEXT_ENCODER);\n  return 0;\n}\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    for (cname, cls), line in zip(pairs, lines):
        out = [int(v) for v in line.split()]
        assert out[0] == C.sizeof(cls), cname
        assert out[1:] == [getattr(cls, f).offset for f, _ in cls._fields_], cname
    assert int(lines[3]) == N.FEATURE_TEXT_ENCODER == 16


def test_feature_bit_and_data_symbols():
    from vllm_omni_amd import _native as N

    assert N.features() & N.FEATURE_TEXT_ENCODER
    assert N.lib().omni_abi_version() == N.ABI_VERSION == 14
    dyn = subprocess.run(["nm", "-D", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    kinds = {ln.split()[-1]: ln.split()[-2] for ln in dyn.splitlines() if len(ln.split()) >= 3}
    for name in ENTRY_POINTS:
        assert name not in N.PROTOTYPES and name in N.FEATURE_PROTOTYPES
        assert N.FEATURE_PROTOTYPES[name][2] == N.FEATURE_TEXT_ENCODER
        assert kinds[name] in ("D", "R"), (name, kinds[name])          # a data symbol (a const pointer), not text
        assert callable(getattr(N.lib(), name))


# ---------------------------------------------------------------------------------------------------------------- 2
def _weights(n_layers=2, **kw):
    from vllm_omni_amd import _native as N

    arr = (N.TextLayerWeights * n_layers)()
    for rec in arr:
        for i, (f, _) in enumerate(N.TextLayerWeights._fields_):
            setattr(rec, f, P + 0x1000 * (i + 1))
    w = N.TextWeights()
    vals = dict(num_layers=n_layers, hidden_size=3584, num_heads=28, num_kv_heads=4, head_dim=128, intermediate_size=18944,
                vocab_size=152064, gemm_w_k32_blocked=1, rms_norm_eps=1e-6, rope_npos=2048, embed_tokens=P, final_norm_w=P,
                ones=P, rope_cos=P, rope_sin=P)
    vals.update(kw)
    for k, v in vals.items():
        setattr(w, k, v)
    if "layers" not in kw:
        w.layers = arr
    w._keep = arr
    return w


def _batch(**kw):
    from vllm_omni_amd import _native as N

    b = N.TextBatch()
    vals = dict(n_prompts=2, total_rows=160, max_seqlen=90, input_ids=P, cu_seqlens=P, row_pos=P, out=P, workspace=P,
                workspace_bytes=1 << 40)
    vals.update(kw)
    for k, v in vals.items():
        setattr(b, k, v)
    return b


@pytest.mark.parametrize("wkw,bkw,want", [
    (dict(head_dim=64), {}, UNSUPPORTED), (dict(head_dim=32, hidden_size=128, num_heads=4, num_kv_heads=2), {}, UNSUPPORTED),
    (dict(hidden_size=3600), {}, UNSUPPORTED), (dict(intermediate_size=18950), {}, UNSUPPORTED),
    (dict(hidden_size=16384), {}, UNSUPPORTED),
    (dict(num_heads=28, num_kv_heads=8), {}, UNSUPPORTED),
    ({}, dict(n_prompts=65, total_rows=650, max_seqlen=10), UNSUPPORTED),
    (dict(embed_tokens=None), {}, BAD_ARG), (dict(final_norm_w=None), {}, BAD_ARG), (dict(ones=None), {}, BAD_ARG),
    (dict(rope_cos=None), {}, BAD_ARG), (dict(rope_sin=None), {}, BAD_ARG), (dict(layers=None), {}, BAD_ARG),
    (dict(num_layers=0), {}, BAD_ARG), (dict(vocab_size=0), {}, BAD_ARG), (dict(rope_npos=0), {}, BAD_ARG),
    (dict(gemm_w_k32_blocked=2), {}, BAD_ARG),
    ({}, dict(input_ids=None), BAD_ARG), ({}, dict(cu_seqlens=None), BAD_ARG), ({}, dict(row_pos=None), BAD_ARG),
    ({}, dict(out=None), BAD_ARG), ({}, dict(workspace=None), BAD_ARG),
    ({}, dict(n_prompts=0), BAD_ARG), ({}, dict(total_rows=0), BAD_ARG), ({}, dict(max_seqlen=0), BAD_ARG),
    ({}, dict(max_seqlen=161), BAD_ARG),
    ({}, dict(workspace_bytes=4096), BAD_ARG),                      # shorter than omni_qwen2_text_workspace_bytes says
    ({}, dict(workspace=P + 8), ALIGN),
])
def test_driver_refusals_before_any_launch(wkw, bkw, want):
    from vllm_omni_amd import _native as N

    w, b = _weights(**wkw), _batch(**bkw)
    assert N.lib().omni_qwen2_text_forward(C.byref(w), C.byref(b), None) == want, (wkw, bkw)
    if wkw:
        assert N.lib().omni_qwen2_text_workspace_bytes(C.byref(w), 160) == 0


def test_driver_null_arguments_and_layer_pointers():
    from vllm_omni_amd import _native as N

    L = N.lib()
    w, b = _weights(), _batch()
    assert L.omni_qwen2_text_forward(None, C.byref(b), None) == BAD_ARG
    assert L.omni_qwen2_text_forward(C.byref(w), None, None) == BAD_ARG
    assert L.omni_qwen2_text_workspace_bytes(None, 160) == 0
    assert L.omni_qwen2_text_workspace_bytes(C.byref(w), 0) == 0
    w._keep[1].down_w = None                                          # one missing matrix of one layer
    assert L.omni_qwen2_text_forward(C.byref(w), C.byref(b), None) == BAD_ARG


def test_workspace_size_covers_every_buffer():
    from vllm_omni_amd import _native as N

    w, R = _weights(), 160
    need = N.lib().omni_qwen2_text_workspace_bytes(C.byref(w), R)
    D, I, nqkv = 3584, 18944, (28 + 8) * 128
    bufs = 2 * R * (D + D + nqkv + D + 2 * I + I)                     # h, xn, qkv, attn, gate|up, act (bf16)
    assert need >= 256 + bufs + 4 * 8 * R * nqkv                      # + the error word's slot + the split-K partials
    assert need % 256 == 0 and need < 2 * (256 + bufs + 4 * 8 * R * nqkv)
    assert N.lib().omni_qwen2_text_workspace_bytes(C.byref(w), 2 * R) > need


def test_row_kernel_entry_points_check_their_arguments():
    from vllm_omni_amd import _native as N

    L = N.lib()
    assert L.omni_text_rope_neox(None, 4608, 4, 28, 4, P, P, 2048, P, None, None) == BAD_ARG
    assert L.omni_text_rope_neox(P, 4600, 4, 28, 4, P, P, 2048, P, None, None) == BAD_ARG       # rows would overlap
    assert L.omni_text_rope_neox(P, 4612, 4, 28, 4, P, P, 2048, P, None, None) == ALIGN
    assert L.omni_text_swiglu(P, 384, None, 192, 4, 192, 0, None) == BAD_ARG
    assert L.omni_text_swiglu(P, 384, P, 192, 4, 196, 0, None) == UNSUPPORTED
    assert L.omni_text_swiglu(P, 200, P, 192, 4, 192, 0, None) == BAD_ARG
    assert L.omni_text_swiglu(P, 384, P, 192, 4, 192, 3, None) == BAD_ARG                             # blocked rows < rows
    assert L.omni_text_embed_gather(P, 259, 512, P, 4, P, 512, None, None) == BAD_ARG                 # the error word is required
    assert L.omni_text_embed_gather(P, 259, 516, P, 4, P, 520, P, None) == UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------- 3
def _small_hf(**kw):
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import QwenPromptEncoder

    args = dict(hidden_size=512, num_layers=2, num_heads=4, num_kv_heads=2, intermediate_size=192, seed=5)
    args.update(kw)
    return QwenPromptEncoder.random_init(**args)


def test_from_hf_fuses_rows_exactly_and_can_free_the_source():
    from vllm_omni_amd import ops
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import NativeQwenPromptEncoder

    hf = _small_hf()
    ref = [{k: v.clone() for k, v in L.state_dict().items()} for L in hf.model.layers]
    enc = NativeQwenPromptEncoder.from_hf(hf.model, hf.tokenizer, w_k32_blocked=False)
    assert len(hf.model.layers) == 2                                   # free_source defaults to off: the HF model is intact
    assert enc.prompt_template_encode_start_idx == hf.prompt_template_encode_start_idx
    assert enc.geometry["eps"] == hf.model.config.rms_norm_eps and enc.geometry["theta"] == 1000000.0
    assert torch.equal(enc.embed_tokens, hf.model.embed_tokens.weight) and torch.equal(enc.final_norm_w, hf.model.norm.weight)
    for L, r in zip(enc.layers, ref):
        assert torch.equal(L["qkv_w"], torch.cat([r[f"self_attn.{n}_proj.weight"] for n in "qkv"]))
        assert torch.equal(L["qkv_b"], torch.cat([r[f"self_attn.{n}_proj.bias"] for n in "qkv"]))
        assert torch.equal(L["gate_up_w"], torch.cat([r["mlp.gate_proj.weight"], r["mlp.up_proj.weight"]]))
        assert torch.equal(L["o_w"], r["self_attn.o_proj.weight"]) and torch.equal(L["down_w"], r["mlp.down_proj.weight"])
        assert torch.equal(L["input_norm_w"], r["input_layernorm.weight"])
        assert torch.equal(L["post_norm_w"], r["post_attention_layernorm.weight"])
        assert L["qkv_w"].shape == (4 * 128 + 2 * 2 * 128, 512) and L["gate_up_w"].shape == (384, 512)
    blocked = NativeQwenPromptEncoder.from_hf(hf.model, hf.tokenizer, free_source=True)      # the default layout: K32-blocked
    assert len(hf.model.layers) == 0                                   # the HF decoder layers are gone
    for L, U in zip(blocked.layers, enc.layers):
        for name in ("qkv_w", "o_w", "gate_up_w", "down_w"):
            assert torch.equal(ops.k32_blocked_to_rows(L[name]), U[name]), name


def test_rope_table_equals_hf_rotary_embedding():
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import NativeQwenPromptEncoder

    # built in fp32, as a checkpoint load leaves the rotary frequencies (a later `.to(bfloat16)` of the whole module would round
    # the inv_freq buffer too: not what the checkpoint's model computes, and not what the table is compared with)
    hf = _small_hf(dtype=torch.float32)
    enc = NativeQwenPromptEncoder.from_hf(hf.model, hf.tokenizer)
    assert enc.embed_tokens.dtype == torch.bfloat16 and enc.layers[0]["qkv_w"].dtype == torch.bfloat16
    assert enc.rope_cos.shape == (enc.rope_npos, 64) and enc.rope_cos.dtype == torch.float32 and enc.rope_npos >= 1024 + 34
    pos = torch.tensor([0, 1, 2, 33, 34, 299, 1057, enc.rope_npos - 1])
    pid = pos[None, None, :].expand(3, 1, -1)                          # text-only: the three M-RoPE rows are equal
    cos, sin = hf.model.rotary_emb(torch.zeros(1, pos.numel(), 512, dtype=torch.float32), pid)
    sec = hf.model.config.rope_parameters["mrope_section"] * 2
    for tab, got in ((enc.rope_cos, cos), (enc.rope_sin, sin)):
        mixed = torch.cat([m[i % 3] for i, m in enumerate(got.split(sec, dim=-1))], dim=-1)[0]      # what attention applies
        assert torch.equal(mixed[:, :64], mixed[:, 64:])
        assert (tab[pos] - mixed[:, :64]).abs().max().item() <= 1e-6


def test_packing_gives_hf_positions_for_a_right_padded_batch():
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import (PROMPT_TEMPLATE_ENCODE, ByteTokenizer, masked_drop_pad,
                                                                        pack_tokens, packed_drop_pad)

    tok = ByteTokenizer()
    drop = tok.template_prefix_tokens(PROMPT_TEMPLATE_ENCODE)
    tail = len(PROMPT_TEMPLATE_ENCODE.split("{}")[1].encode())
    want = [1, 37, 300]                                                # tokens past the template prefix
    prompts = ["x" * (n - tail) if n > tail else "" for n in want]
    # (a prompt cannot be shorter than the template's tail: the length-1 case is a sequence truncated right behind the prefix)
    toks = tok([PROMPT_TEMPLATE_ENCODE.format(p) for p in prompts])
    ids, mask = toks.input_ids.clone(), toks.attention_mask.clone()
    mask[0, drop + 1:] = 0
    ids[0, drop + 1:] = 0
    lens_full = mask.sum(1).tolist()
    assert [n - drop for n in lens_full] == want and mask.shape[1] == drop + 300
    pid, cu, pos, lens = pack_tokens(ids, mask)
    assert lens == lens_full and cu.tolist() == [0, drop + 1, 2 * drop + 38, 3 * drop + 338] and cu.dtype == torch.int32
    assert pid.dtype == torch.int32 and pos.dtype == torch.int32 and pid.numel() == sum(lens)
    # HF's text model numbers a right-padded row 0 .. L - 1 (cache_position); on the valid tokens that is cumsum(mask) - 1
    hf_pos = torch.arange(mask.shape[1])[None].expand(3, -1)
    assert torch.equal(pos.long(), hf_pos[mask.bool()])
    assert torch.equal(pid.long(), ids[mask.bool()])
    for i in range(3):
        assert pos[cu[i]:cu[i + 1]].tolist() == list(range(lens[i]))
    # ... and unpacking is masked_drop_pad's: same rows, same zero padding, same mask
    hidden = torch.randn(3, mask.shape[1], 8)
    e0, m0 = masked_drop_pad(hidden, mask, drop)
    e1, m1 = packed_drop_pad(hidden[mask.bool()], lens, drop)
    assert torch.equal(e0, e1) and torch.equal(m0, m1) and m1.sum(1).tolist() == want and m1.dtype == torch.long
    assert e1.shape == (3, 300, 8) and not e1[0, 1:].any() and not e1[1, 37:].any()


# ---------------------------------------------------------------------------------------------------------------- 4
def _pipeline(**cfg):
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline

    class QwenImageTransformer2DModel:
        teacache = None

    vae = types.SimpleNamespace(config=types.SimpleNamespace(latents_mean=[0.0] * 16, latents_std=[1.0] * 16))
    return QwenImagePipeline(od_config=OmniDiffusionConfig(**cfg), device="cpu", transformer=QwenImageTransformer2DModel(), vae=vae)


def _fake_checkpoint(tmp_path, monkeypatch, hf):
    import transformers

    (tmp_path / "text_encoder").mkdir()
    (tmp_path / "tokenizer").mkdir()
    wrapper = torch.nn.Module()                                        # Qwen2_5_VLForConditionalGeneration: .model.language_model
    wrapper.model = torch.nn.Module()
    wrapper.model.language_model = hf.model
    monkeypatch.setattr(transformers.Qwen2_5_VLForConditionalGeneration, "from_pretrained",
                        classmethod(lambda cls, *a, **k: wrapper))
    monkeypatch.setattr(transformers.AutoTokenizer, "from_pretrained", classmethod(lambda cls, *a, **k: hf.tokenizer))
    return str(tmp_path)


def test_flag_is_off_by_default_and_then_nothing_new_is_built(tmp_path, monkeypatch):
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import QwenPromptEncoder

    assert OmniDiffusionConfig().native_text_encoder is False
    hf = _small_hf()
    pipe = _pipeline()
    assert pipe.text_encoder is None
    pipe.load_text_encoder(_fake_checkpoint(tmp_path, monkeypatch, hf))
    assert type(pipe.text_encoder) is QwenPromptEncoder and len(hf.model.layers) == 2


def test_flag_builds_the_native_encoder_and_frees_the_hf_layers(tmp_path, monkeypatch):
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import NativeQwenPromptEncoder

    hf = _small_hf()
    pipe = _pipeline(native_text_encoder=True)
    pipe.load_text_encoder(_fake_checkpoint(tmp_path, monkeypatch, hf))
    assert type(pipe.text_encoder) is NativeQwenPromptEncoder
    assert len(hf.model.layers) == 0 and len(pipe.text_encoder.layers) == 2
    given = object()                                                   # an explicit text_encoder= is used as it is
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline

    vae = types.SimpleNamespace(config=types.SimpleNamespace(latents_mean=[0.0] * 16, latents_std=[1.0] * 16))
    p2 = QwenImagePipeline(od_config=OmniDiffusionConfig(native_text_encoder=True), device="cpu", transformer=object(), vae=vae,
                           text_encoder=given)
    assert p2.text_encoder is given


@pytest.mark.parametrize("module,name", [
    ("pipeline_qwen_image_edit", "QwenImageEditPipeline"), ("pipeline_qwen_image_edit_plus", "QwenImageEditPlusPipeline"),
    ("pipeline_qwen_image_layered", "QwenImageLayeredPipeline")])
def test_edit_family_refuses_the_flag(module, name):
    import importlib

    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig

    cls = getattr(importlib.import_module(f"vllm_omni_amd.diffusion.models.qwen_image.{module}"), name)
    with pytest.raises(NotImplementedError, match="native_text_encoder"):
        cls(od_config=OmniDiffusionConfig(native_text_encoder=True), device="cpu", transformer=object(), vae=object())


def test_unsupported_geometry_is_refused_with_its_reason():
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import NativeQwenPromptEncoder

    hf = _small_hf(hidden_size=128, intermediate_size=256)             # the engine tests' encoder: head size 32
    with pytest.raises(ValueError, match="head size 32"):
        NativeQwenPromptEncoder.from_hf(hf.model, hf.tokenizer)
    assert len(hf.model.layers) == 2                                   # refused before anything was touched
    with pytest.raises(ValueError, match="intermediate size 200"):
        hf2 = _small_hf(intermediate_size=200)
        NativeQwenPromptEncoder.from_hf(hf2.model, hf2.tokenizer, free_source=True)
    with pytest.raises(TypeError, match="text model"):
        NativeQwenPromptEncoder.from_hf(torch.nn.Linear(2, 2), hf.tokenizer)
