"""Prompt encoding for Qwen-Image — mirror of `_get_qwen_prompt_embeds` (reference
vllm_omni/diffusion/models/qwen_image/pipeline_qwen_image.py:351-392): the prompt is wrapped in the chat template, run
through the Qwen2.5-VL language model (HF `transformers`, as in the reference: `Qwen2_5_VLForConditionalGeneration`,
`output_hidden_states=True`, last hidden state), the 34 template tokens are dropped, sequences are zero-padded to the longest
and returned with their mask.

This is the REQUEST-SIDE BOUNDARY, not the DiT hot path: it runs once per request, on the same HF eager
kernels the reference uses; its output feeds `prompt_embeds` of the native denoise loop.  No checkpoint can be downloaded
here, so tests build a small random-weight Qwen2.5-VL text model and a byte-level tokenizer stand-in with the same call
signature (`ByteTokenizer`); with a real checkpoint pass `Qwen2Tokenizer` and the loaded model.

Opt-in (`OmniDiffusionConfig.native_text_encoder`): `NativeQwenPromptEncoder` runs the same text model on this library - all
decoder layers in one `omni_qwen2_text_forward` over the packed valid tokens - with the same tokenizer, template, drop index,
outputs and mask (text-only prompts).  Opt-in (`OmniDiffusionConfig.native_vl_encoder`): `NativeQwenEditPromptEncoder` does the
same for the Edit pipelines' prompts WITH pictures - the vision tower in one `omni_qwen2_vision_forward`, the language model with
real M-RoPE and the image embeddings in the token rows in one `omni_qwen2_text_forward_mm`; the HF Edit encoder stays the default.
Opt-in (`OmniDiffusionConfig.native_captioner`): `NativeQwenCaptioner` GENERATES the Layered pipeline's auto-caption on this library
- prefill into a KV cache, then greedy decode steps queued without a host round trip per token."""
from __future__ import annotations

import torch

PROMPT_TEMPLATE_ENCODE = ("<|im_start|>system\nDescribe the image by detailing the color, shape, size, texture, quantity, text, "
                          "spatial relationships of the objects and background:<|im_end|>\n<|im_start|>user\n{}<|im_end|>\n"
                          "<|im_start|>assistant\n")
PROMPT_TEMPLATE_ENCODE_START_IDX = 34            # tokens of the template prefix under the Qwen2 tokenizer (:282)


class ByteTokenizer:
    """Stand-in with the `Qwen2Tokenizer.__call__` signature used by the pipeline: UTF-8 bytes + 3 (0 = pad)."""

    pad_token_id = 0
    vocab_size = 259

    def __call__(self, text, max_length=None, padding=True, truncation=True, return_tensors="pt"):
        text = [text] if isinstance(text, str) else list(text)
        ids = [[b + 3 for b in t.encode("utf-8")] for t in text]
        if truncation and max_length:
            ids = [x[:max_length] for x in ids]
        L = max(len(x) for x in ids)
        input_ids = torch.tensor([x + [0] * (L - len(x)) for x in ids], dtype=torch.long)
        mask = torch.tensor([[1] * len(x) + [0] * (L - len(x)) for x in ids], dtype=torch.long)
        return _Tokens(input_ids, mask)

    def template_prefix_tokens(self, template: str) -> int:
        return len(template.split("{}")[0].encode("utf-8"))


class _Tokens:
    def __init__(self, input_ids, attention_mask):
        self.input_ids, self.attention_mask = input_ids, attention_mask

    def to(self, device):
        return _Tokens(self.input_ids.to(device), self.attention_mask.to(device))


class QwenPromptEncoder:
    def __init__(self, text_model, tokenizer, dtype=torch.bfloat16, tokenizer_max_length: int = 1024,
                 template: str = PROMPT_TEMPLATE_ENCODE, drop_idx: int | None = None):
        self.model, self.tokenizer, self.dtype = text_model, tokenizer, dtype
        self.tokenizer_max_length = tokenizer_max_length
        self.prompt_template_encode = template
        if drop_idx is None:
            drop_idx = tokenizer.template_prefix_tokens(template) if hasattr(tokenizer, "template_prefix_tokens") \
                else PROMPT_TEMPLATE_ENCODE_START_IDX
        self.prompt_template_encode_start_idx = drop_idx

    @classmethod
    def random_init(cls, hidden_size: int = 3584, num_layers: int = 2, num_heads: int = 28, num_kv_heads: int = 4,
                    intermediate_size: int = 512, device="cpu", dtype=torch.bfloat16, seed: int = 0):
        """Random-weight Qwen2.5-VL TEXT model of the real width (3584 -> joint_attention_dim) with few layers: what the
        end-to-end tests use in place of the 7B checkpoint."""
        from transformers import Qwen2_5_VLTextConfig, Qwen2_5_VLTextModel

        torch.manual_seed(seed)
        tok = ByteTokenizer()
        half = hidden_size // num_heads // 2                       # rotary pairs per head; Qwen2.5-VL: 64 -> [16, 24, 24]
        sec = [half // 4, (half - half // 4) // 2]
        sec.append(half - sum(sec))
        cfg = Qwen2_5_VLTextConfig(vocab_size=tok.vocab_size, hidden_size=hidden_size, num_hidden_layers=num_layers,
                                   num_attention_heads=num_heads, num_key_value_heads=num_kv_heads,
                                   intermediate_size=intermediate_size, max_position_embeddings=4096,
                                   bos_token_id=1, eos_token_id=2, pad_token_id=0,
                                   rope_scaling={"type": "default", "mrope_section": sec, "rope_type": "default"})
        model = Qwen2_5_VLTextModel(cfg).to(device=device, dtype=dtype).eval()
        return cls(model, tok, dtype=dtype)

    @torch.no_grad()
    def get_qwen_prompt_embeds(self, prompt, device=None, dtype=None):
        """-> (prompt_embeds [B, Tmax, hidden] zero-padded, mask [B, Tmax] long)   (reference :359-392)."""
        prompt = [prompt] if isinstance(prompt, str) else list(prompt)
        dev = device if device is not None else next(self.model.parameters()).device
        drop = self.prompt_template_encode_start_idx
        txt = [self.prompt_template_encode.format(e) for e in prompt]
        toks = self.tokenizer(txt, max_length=self.tokenizer_max_length + drop, padding=True, truncation=True,
                              return_tensors="pt").to(next(self.model.parameters()).device)
        out = self.model(input_ids=toks.input_ids, attention_mask=toks.attention_mask, output_hidden_states=True)
        emb, msk = masked_drop_pad(out.hidden_states[-1], toks.attention_mask, drop)
        return emb.to(device=dev, dtype=dtype or self.dtype), msk.to(dev)


def masked_drop_pad(hidden: torch.Tensor, attention_mask: torch.Tensor, drop: int):
    """`_extract_masked_hidden` + drop of the template tokens + zero-padding to the longest sequence + mask, shared by the
    text-to-image (pipeline_qwen_image.py:351-357,380-390) and the Edit pipelines (pipeline_qwen_image_edit.py:298-305,
    383-393)."""
    mask = attention_mask.bool()
    return packed_drop_pad(hidden[mask], mask.sum(dim=1).tolist(), drop)


def packed_drop_pad(packed: torch.Tensor, lens: list[int], drop: int):
    """The same from the valid tokens already packed ([sum(lens), hidden], prompt after prompt): what `masked_drop_pad` does
    after its gather, and what the native encoder's output is to begin with."""
    split = [h[drop:] for h in torch.split(packed, lens, dim=0)]
    T = max(e.shape[0] for e in split)
    emb = torch.stack([torch.cat([u, u.new_zeros(T - u.shape[0], u.shape[1])]) for u in split])
    msk = torch.stack([torch.cat([torch.ones(u.shape[0], dtype=torch.long, device=u.device),
                                  torch.zeros(T - u.shape[0], dtype=torch.long, device=u.device)]) for u in split])
    return emb, msk


# ---- the native prompt encoder: the same text model on this library's kernels (omni_qwen2_text_forward) ----------------------
TEXT_HEAD_SIZE = 128               # the head size the attention and RoPE kernels of the native encoder are built for
MAX_PROMPTS_PER_FORWARD = 64       # omni_text_batch.n_prompts


def text_model_of(model):
    """The `Qwen2_5_VLTextModel` inside what the pipelines load: the text model itself, or the `.model.language_model` /
    `.language_model` of a `Qwen2_5_VLForConditionalGeneration`."""
    for path in ((), ("model", "language_model"), ("language_model",)):
        m = model
        for a in path:
            m = getattr(m, a, None)
            if m is None:
                break
        if m is not None and hasattr(m, "layers") and hasattr(m, "embed_tokens") and hasattr(m, "norm"):
            return m
    raise TypeError(f"{type(model).__name__} holds no Qwen2.5-VL text model (embed_tokens / layers / norm)")


def check_text_geometry(cfg) -> dict:
    """The geometry of an HF text config as the native encoder needs it, or ValueError naming what it does not take
    (omni_qwen2_text_forward would answer OMNI_ERR_UNSUPPORTED; the reason is better said here, at construction)."""
    hidden, heads, kv = int(cfg.hidden_size), int(cfg.num_attention_heads), int(cfg.num_key_value_heads)
    inter = int(cfg.intermediate_size)
    head = int(getattr(cfg, "head_dim", None) or hidden // heads)
    rope = dict(getattr(cfg, "rope_parameters", None) or getattr(cfg, "rope_scaling", None) or {})
    theta = rope.get("rope_theta", getattr(cfg, "rope_theta", None))
    why = None
    if head != TEXT_HEAD_SIZE:
        why = f"head size {head}: the native attention and RoPE kernels are built for head size {TEXT_HEAD_SIZE}"
    elif hidden % 64 or inter % 64 or hidden > 8192:
        why = f"hidden size {hidden} / intermediate size {inter}: both must be multiples of 64, hidden at most 8192"
    elif heads % kv:
        why = f"{heads} query heads over {kv} key/value heads: not a whole group per key/value head"
    elif getattr(cfg, "hidden_act", "silu") != "silu":
        why = f"activation {cfg.hidden_act!r}: the MLP kernel is SwiGLU"
    elif rope.get("rope_type", rope.get("type", "default")) != "default":
        why = f"rope type {rope.get('rope_type', rope.get('type'))!r}: only the default frequencies are built"
    elif theta is None:
        why = "no rope_theta in the config"
    elif getattr(cfg, "use_sliding_window", False):
        why = "sliding-window attention"
    if why:
        raise ValueError(f"the native Qwen2.5-VL prompt encoder does not take this text model - {why}")
    return dict(hidden=hidden, heads=heads, kv_heads=kv, head=head, inter=inter, layers=int(cfg.num_hidden_layers),
                vocab=int(cfg.vocab_size), eps=float(cfg.rms_norm_eps), theta=float(theta))


def text_rope_tables(theta: float, npos: int, head: int = TEXT_HEAD_SIZE, device="cpu"):
    """fp32 cos / sin [npos, head / 2] of the default rotary frequencies, computed as HF's rotary embedding computes them
    (inv_freq = theta^(-2i / head) in fp32, angle = position * inv_freq in fp32).  A text-only prompt hands M-RoPE three equal
    position rows, so column i of every section reads this table at the token's one position."""
    inv = 1.0 / (theta ** (torch.arange(0, head, 2, dtype=torch.int64).float() / head))
    ang = torch.arange(npos, dtype=torch.float32)[:, None] * inv[None, :]
    return ang.cos().contiguous().to(device), ang.sin().contiguous().to(device)


def pack_tokens(input_ids: torch.Tensor, attention_mask: torch.Tensor):
    """[B, L] ids + mask -> (ids int32 [R], cu_seqlens int32 [B + 1], row_pos int32 [R], lens): the valid tokens prompt after
    prompt, each with its position cumsum(mask) - 1 (what HF derives from the mask; for right padding simply 0 .. len - 1)."""
    mask = attention_mask.bool()
    lens = mask.sum(dim=1)
    pos = (attention_mask.long().cumsum(dim=1) - 1)[mask]
    cu = torch.zeros(mask.shape[0] + 1, dtype=torch.int32)
    cu[1:] = lens.cumsum(0)
    return input_ids[mask].to(torch.int32), cu, pos.to(torch.int32), lens.tolist()


class NativeQwenPromptEncoder:
    """`QwenPromptEncoder` with the text model on this library: same tokenizer, template, drop index, outputs and mask; the
    28 decoder layers run as ONE omni_qwen2_text_forward over the packed valid tokens (no pad rows).  Built by `from_hf`;
    anything the kernels do not take raises there - there is no fall-back to the HF model."""

    def __init__(self, geometry: dict, embed_tokens, final_norm_w, layers: list[dict], tokenizer, dtype=torch.bfloat16,
                 tokenizer_max_length: int = 1024, template: str = PROMPT_TEMPLATE_ENCODE, drop_idx: int | None = None,
                 w_k32_blocked: bool = True, rope_npos: int | None = None):
        from .... import _native as N

        if not N.features() & N.FEATURE_TEXT_ENCODER:
            raise N.OmniNativeError("this libomni_cdna4.so does not report OMNI_FEATURE_TEXT_ENCODER: it has no "
                                    "omni_qwen2_text_forward - rebuild it (python vllm_omni_amd/csrc/build.py); the native "
                                    "prompt encoder never falls back to the HF model")
        if dtype != torch.bfloat16:
            raise ValueError(f"the native prompt encoder computes in bfloat16, not {dtype}")
        self.geometry, self.embed_tokens, self.final_norm_w, self.layers = geometry, embed_tokens, final_norm_w, layers
        self.tokenizer, self.dtype, self.w_k32_blocked = tokenizer, dtype, bool(w_k32_blocked)
        self.tokenizer_max_length = tokenizer_max_length
        self.prompt_template_encode = template
        if drop_idx is None:
            drop_idx = tokenizer.template_prefix_tokens(template) if hasattr(tokenizer, "template_prefix_tokens") \
                else PROMPT_TEMPLATE_ENCODE_START_IDX
        self.prompt_template_encode_start_idx = drop_idx
        self.rope_npos = int(rope_npos) if rope_npos else max(2048, tokenizer_max_length + drop_idx)
        self.rope_cos, self.rope_sin = text_rope_tables(geometry["theta"], self.rope_npos, device=embed_tokens.device)
        self.ones = torch.ones(geometry["hidden"], dtype=torch.bfloat16, device=embed_tokens.device)
        self._desc = self._layer_array = self._workspace = None

    @classmethod
    def from_hf(cls, text_model, tokenizer, free_source: bool = False, **kw):
        """From an HF `Qwen2_5_VLTextModel` (or the `Qwen2_5_VLForConditionalGeneration` around one), on the device its weights
        are on: q|k|v weights and biases and gate|up weights are concatenated into the fused matrices once (K32-blocked unless
        `w_k32_blocked=False`), embed_tokens and the norm weights are kept as they are.  `free_source`: each HF decoder layer is
        dropped as soon as its fused copy exists, so the 13 GB are never held twice (the HF model cannot run afterwards)."""
        from .... import ops

        tm = text_model_of(text_model)
        g = check_text_geometry(tm.config)
        blocked = bool(kw.get("w_k32_blocked", True))
        bf = lambda t: t.detach().to(torch.bfloat16).contiguous()
        mat = (lambda t: ops.w_to_k32_blocked(t)) if blocked else (lambda t: t.contiguous())
        layers = []
        for i in range(len(tm.layers)):
            L = tm.layers[i]
            a, m = L.self_attn, L.mlp
            if a.q_proj.bias is None or a.k_proj.bias is None or a.v_proj.bias is None or a.o_proj.bias is not None or \
                    any(getattr(m, n).bias is not None for n in ("gate_proj", "up_proj", "down_proj")):
                raise ValueError("the native Qwen2.5-VL prompt encoder does not take this text model - it expects biases on "
                                 "q_proj / k_proj / v_proj and none on o_proj and the MLP")
            layers.append(dict(
                input_norm_w=bf(L.input_layernorm.weight), post_norm_w=bf(L.post_attention_layernorm.weight),
                qkv_w=mat(bf(torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight]))),
                qkv_b=bf(torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias])),
                o_w=mat(bf(a.o_proj.weight)),
                gate_up_w=mat(bf(torch.cat([m.gate_proj.weight, m.up_proj.weight]))),
                down_w=mat(bf(m.down_proj.weight))))
            if free_source:
                tm.layers[i] = torch.nn.Identity()
        if len(layers) != g["layers"]:
            raise ValueError(f"the text model has {len(layers)} decoder layers, its config says {g['layers']}")
        enc = cls(g, bf(tm.embed_tokens.weight), bf(tm.norm.weight), layers, tokenizer, **kw)
        if free_source:
            tm.layers = torch.nn.ModuleList()
        return enc

    def _descriptor(self):
        """omni_text_weights over the tensors this object keeps alive (built at the first encode: needs device pointers)."""
        if self._desc is None:
            from .... import _native as N
            from ....ops import _p

            g = self.geometry
            arr = (N.TextLayerWeights * len(self.layers))()
            for rec, L in zip(arr, self.layers):
                for name, _ in N.TextLayerWeights._fields_:
                    setattr(rec, name, _p(L[name], name=name))
            w = N.TextWeights()
            w.num_layers, w.hidden_size, w.num_heads, w.num_kv_heads = len(self.layers), g["hidden"], g["heads"], g["kv_heads"]
            w.head_dim, w.intermediate_size, w.vocab_size = g["head"], g["inter"], self.embed_tokens.shape[0]
            w.gemm_w_k32_blocked, w.rms_norm_eps, w.rope_npos = int(self.w_k32_blocked), g["eps"], self.rope_npos
            w.embed_tokens, w.final_norm_w = _p(self.embed_tokens, name="embed_tokens"), _p(self.final_norm_w, name="norm")
            w.ones = _p(self.ones, name="ones")
            w.rope_cos, w.rope_sin = _p(self.rope_cos, torch.float32, "rope_cos"), _p(self.rope_sin, torch.float32, "rope_sin")
            w.layers = arr
            self._desc, self._layer_array = w, arr
        return self._desc

    @torch.no_grad()
    def encode_packed(self, ids: torch.Tensor, cu_seqlens: torch.Tensor, row_pos: torch.Tensor, max_seqlen: int) -> torch.Tensor:
        """Packed int32 tokens (on the weights' device) -> last hidden state [rows, hidden] bf16."""
        from .... import ops

        w = self._descriptor()
        need = ops.qwen2_text_workspace_bytes(w, ids.numel())
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.zeros(need, dtype=torch.uint8, device=ids.device)      # zeroed: the error word in front
        return ops.qwen2_text_forward(w, ids, cu_seqlens, row_pos, max_seqlen, self._workspace)

    @torch.no_grad()
    def get_qwen_prompt_embeds(self, prompt, device=None, dtype=None):
        """-> (prompt_embeds [B, Tmax, hidden] zero-padded, mask [B, Tmax] long), as `QwenPromptEncoder` returns them."""
        prompt = [prompt] if isinstance(prompt, str) else list(prompt)
        wdev = self.embed_tokens.device
        dev = device if device is not None else wdev
        drop = self.prompt_template_encode_start_idx
        txt = [self.prompt_template_encode.format(e) for e in prompt]
        toks = self.tokenizer(txt, max_length=self.tokenizer_max_length + drop, padding=True, truncation=True, return_tensors="pt")
        input_ids, attention_mask = toks.input_ids.cpu(), toks.attention_mask.cpu()
        ids, cu, pos, lens = pack_tokens(input_ids, attention_mask)
        # the tokens are still on the host: a bad id or an over-long prompt is refused here (the kernels would zero / clamp it
        # and report through the device error word on the NEXT call)
        if ids.numel() == 0 or int(ids.min()) < 0 or int(ids.max()) >= self.embed_tokens.shape[0]:
            raise ValueError(f"token ids outside the embedding table [0, {self.embed_tokens.shape[0]})")
        if max(lens) > self.rope_npos:
            raise ValueError(f"a prompt of {max(lens)} tokens exceeds the RoPE table of {self.rope_npos} positions")
        parts = []
        for b0 in range(0, len(lens), MAX_PROMPTS_PER_FORWARD):                            # (one forward unless > 64 prompts)
            sub = lens[b0:b0 + MAX_PROMPTS_PER_FORWARD]
            r0, n, R = int(cu[b0]), len(sub), sum(sub)
            packed = torch.cat([ids[r0:r0 + R], cu[b0:b0 + n + 1] - r0, pos[r0:r0 + R]]).to(wdev)      # one upload
            parts.append(self.encode_packed(packed[:R], packed[R:R + n + 1], packed[R + n + 1:], max(sub)))
        hidden = parts[0] if len(parts) == 1 else torch.cat(parts)
        emb, msk = packed_drop_pad(hidden, lens, drop)
        return emb.to(device=dev, dtype=dtype or self.dtype), msk.to(dev)


# ---- image-editing prompts: the Qwen2.5-VL VISION tower sees the picture(s) ------------------------------
EDIT_PROMPT_TEMPLATE_ENCODE = (     # reference pipeline_qwen_image_edit.py:240 (one picture, marker inside the template)
    "<|im_start|>system\nDescribe the key features of the input image (color, shape, size, texture, objects, background), then "
    "explain how the user's text instruction should alter or modify the image. Generate a new image that meets the user's "
    "requirements while maintaining consistency with the original input where appropriate.<|im_end|>\n<|im_start|>user\n"
    "<|vision_start|><|image_pad|><|vision_end|>{}<|im_end|>\n<|im_start|>assistant\n")
EDIT_PLUS_PROMPT_TEMPLATE_ENCODE = (  # reference pipeline_qwen_image_edit_plus.py:203-209 (markers come with the pictures)
    "<|im_start|>system\nDescribe the key features of the input image (color, shape, size, texture, objects, background), then "
    "explain how the user's text instruction should alter or modify the image. Generate a new image that meets the user's "
    "requirements while maintaining consistency with the original input where appropriate.<|im_end|>\n<|im_start|>user\n{}"
    "<|im_end|>\n<|im_start|>assistant\n")
EDIT_PROMPT_TEMPLATE_ENCODE_START_IDX = 64       # both Edit pipelines (:241 / :210)
EDIT_PLUS_IMG_PROMPT = "Picture {}: <|vision_start|><|image_pad|><|vision_end|>"     # edit_plus :285


def to_processor_image(x):
    """What the HF image processor takes: PIL images pass through; a tensor [3, H, W] / [1, 3, H, W] / [3, 1, H, W] /
    [1, 3, 1, H, W] in [-1, 1] (the layouts the VAE encoder takes: one picture, optional batch and frame axes of size 1) becomes
    a uint8 HWC array.  Anything else (a batch of several pictures, a wrong channel count) raises — one bad
    `req.extra['image']` must not hang or crash the worker."""
    if isinstance(x, torch.Tensor):
        t = x.detach().float().cpu()
        shape = tuple(t.shape)
        if t.dim() == 5 and t.shape[0] == 1 and t.shape[2] == 1:        # [1, 3, 1, H, W]
            t = t[0, :, 0]
        elif t.dim() == 4 and t.shape[0] == 1:                          # [1, 3, H, W]
            t = t[0]
        elif t.dim() == 4 and t.shape[1] == 1:                          # [3, 1, H, W]
            t = t[:, 0]
        if t.dim() != 3 or t.shape[0] != 3:
            raise ValueError(f"cannot interpret a tensor of shape {shape} as ONE RGB picture "
                             "([3,H,W], [1,3,H,W], [3,1,H,W] or [1,3,1,H,W])")
        return ((t.clamp(-1, 1) + 1) * 127.5).round().to(torch.uint8).permute(1, 2, 0).numpy()
    return x


def resize_picture(x, height: int, width: int):
    """diffusers `VaeImageProcessor.resize(image, height, width)` as the reference calls it for the vision-tower copies of the
    condition images (pipeline_qwen_image_edit_plus.py:116,650; third-party, restated: PIL -> `Image.resize((w, h), LANCZOS)`,
    tensor -> `F.interpolate(size=(h, w))`, i.e. nearest)."""
    if isinstance(x, torch.Tensor):
        t = x
        lead = t.dim()
        if lead == 3:
            t = t.unsqueeze(0)
        elif lead == 5:
            t = t[:, :, 0]
        t = torch.nn.functional.interpolate(t.float(), size=(height, width)).to(x.dtype)
        return t[0] if lead == 3 else (t.unsqueeze(2) if lead == 5 else t)
    from PIL import Image

    return x.resize((width, height), resample=Image.LANCZOS)


class QwenEditPromptEncoder:
    """`_get_qwen_prompt_embeds` of the Edit pipelines (pipeline_qwen_image_edit.py:352-397, multi_image=False;
    pipeline_qwen_image_edit_plus.py:274-330, multi_image=True): template -> `processor(text=, images=)` -> HF
    `Qwen2_5_VLForConditionalGeneration` with `pixel_values` / `image_grid_thw` (vision tower + language model),
    last hidden state, first 64 tokens dropped, zero-padded + mask.  `processor` is the checkpoint's `Qwen2VLProcessor`
    (tests: oracle/vl_stubs.StubVLProcessor, same call signature)."""

    def __init__(self, vl_model, processor, dtype=torch.bfloat16, multi_image: bool = False, template: str | None = None,
                 drop_idx: int = EDIT_PROMPT_TEMPLATE_ENCODE_START_IDX):
        self.model, self.processor, self.dtype, self.multi_image = vl_model, processor, dtype, multi_image
        self.prompt_template_encode = template or (EDIT_PLUS_PROMPT_TEMPLATE_ENCODE if multi_image else EDIT_PROMPT_TEMPLATE_ENCODE)
        self.prompt_template_encode_start_idx = drop_idx
        self.tokenizer_max_length = 1024

    @torch.no_grad()
    def get_qwen_prompt_embeds(self, prompt, image=None, device=None, dtype=None):
        prompt = [prompt] if isinstance(prompt, str) else list(prompt)
        mdev = next(self.model.parameters()).device
        dev = device if device is not None else mdev
        if isinstance(image, (list, tuple)):
            image = [to_processor_image(im) for im in image]
        elif image is not None:
            image = to_processor_image(image)
        if self.multi_image:
            n = len(image) if isinstance(image, list) else (0 if image is None else 1)
            base = "".join(EDIT_PLUS_IMG_PROMPT.format(i + 1) for i in range(n))
            txt = [self.prompt_template_encode.format(base + e) for e in prompt]
        else:
            txt = [self.prompt_template_encode.format(e) for e in prompt]
        inputs = self.processor(text=txt, images=image, padding=True, return_tensors="pt").to(mdev)
        kw = {}
        if getattr(inputs, "pixel_values", None) is not None:
            kw = dict(pixel_values=inputs.pixel_values, image_grid_thw=inputs.image_grid_thw)
        out = self.model(input_ids=inputs.input_ids, attention_mask=inputs.attention_mask, output_hidden_states=True, **kw)
        emb, msk = masked_drop_pad(out.hidden_states[-1], inputs.attention_mask, self.prompt_template_encode_start_idx)
        return emb.to(device=dev, dtype=dtype or self.dtype), msk.to(dev)


# ---- the native Edit prompt encoder: vision tower + language model with M-RoPE on this library ---------------------------------
VISION_HEAD_PAD = 128              # the head size the vision q / k / v are zero-padded to (the attention kernel's)
VISION_ROPE_THETA = 10000.0        # Qwen2_5_VisionRotaryEmbedding's default; the config carries no other
EDIT_ROPE_NPOS = 8192              # rows of the language model's RoPE table: 1024 text tokens + 64 + the picture tokens fit


def _pad_to(n: int, m: int = 64) -> int:
    return (n + m - 1) // m * m


def vision_model_of(model):
    """The vision tower inside what the Edit pipelines load (`.model.visual` / `.visual` of a
    `Qwen2_5_VLForConditionalGeneration`)."""
    for path in (("model", "visual"), ("visual",)):
        m = model
        for a in path:
            m = getattr(m, a, None)
            if m is None:
                break
        if m is not None and hasattr(m, "blocks") and hasattr(m, "merger") and hasattr(m, "patch_embed"):
            return m
    raise TypeError(f"{type(model).__name__} holds no Qwen2.5-VL vision tower (patch_embed / blocks / merger)")


def check_vision_geometry(vcfg, text_hidden: int | None = None) -> dict:
    """The geometry of an HF vision config as omni_qwen2_vision_forward needs it, or ValueError naming what it does not take."""
    hidden, heads, inter = int(vcfg.hidden_size), int(vcfg.num_heads), int(vcfg.intermediate_size)
    head = hidden // heads
    out = int(vcfg.out_hidden_size)
    merge, patch, tps, cin = int(vcfg.spatial_merge_size), int(vcfg.patch_size), int(vcfg.temporal_patch_size), int(vcfg.in_channels)
    window = int(vcfg.window_size)
    why = None
    if hidden % heads:
        why = f"hidden size {hidden} over {heads} heads: not a whole head size"
    elif head % 16 or head > VISION_HEAD_PAD:
        why = f"vision head size {head}: the RoPE + padding kernel takes multiples of 16 up to {VISION_HEAD_PAD}"
    elif hidden % 64 or hidden > 8192 or out % 64:
        why = f"vision hidden size {hidden} / output size {out}: both must be multiples of 64, hidden at most 8192"
    elif getattr(vcfg, "hidden_act", "silu") != "silu":
        why = f"vision activation {vcfg.hidden_act!r}: the MLP kernel is SwiGLU"
    elif merge != 2:
        why = f"spatial merge size {merge}: the merger is built for 2 x 2 units of four consecutive rows"
    elif window % (merge * patch) or window < merge * patch:
        why = f"window size {window}: not a whole number of {merge * patch}-pixel merge units"
    elif text_hidden is not None and out != text_hidden:
        why = f"vision output size {out} is not the language model's hidden size {text_hidden}"
    if why:
        raise ValueError(f"the native Qwen2.5-VL Edit prompt encoder does not take this vision tower - {why}")
    return dict(hidden=hidden, heads=heads, head=head, inter=inter, inter_pad=_pad_to(inter), out=out, merge=merge, patch=patch,
                window=window, patch_k=cin * tps * patch * patch, patch_k_pad=_pad_to(cin * tps * patch * patch),
                layers=int(vcfg.depth), full=sorted(int(i) for i in vcfg.fullatt_block_indexes), eps=1e-6)


def check_mrope_section(cfg) -> list[int]:
    rope = dict(getattr(cfg, "rope_parameters", None) or getattr(cfg, "rope_scaling", None) or {})
    sec = [int(v) for v in (rope.get("mrope_section") or [])]
    if len(sec) != 3 or sum(sec) != TEXT_HEAD_SIZE // 2 or any(v % 8 or v < 0 for v in sec):
        raise ValueError(f"the native Qwen2.5-VL Edit prompt encoder does not take this text model - mrope_section {sec}: three "
                         f"multiples of 8 that sum to {TEXT_HEAD_SIZE // 2} (the checkpoints have [16, 24, 24])")
    return sec


def _grids(grid_thw) -> list[tuple[int, int, int]]:
    g = grid_thw.tolist() if isinstance(grid_thw, torch.Tensor) else grid_thw
    return [(int(t), int(h), int(w)) for t, h, w in g]


def check_picture_grids(grid_thw, merge: int = 2) -> list[tuple[int, int, int]]:
    grids = _grids(grid_thw)
    for t, h, w in grids:
        if t != 1:
            raise ValueError(f"a temporal grid of {t}: the native Edit prompt encoder takes still pictures (t = 1), not videos")
        if h <= 0 or w <= 0 or h % merge or w % merge:
            raise ValueError(f"a patch grid of {h} x {w}: both sides must be positive multiples of the merge size {merge}")
    return grids


def vision_window_index(grid_thw, merge: int, window_size: int, patch: int):
    """(window_index long [rows / merge^2], cu_window int32 [n_windows + 1]): HF `get_vision_window_index` - the order of the
    merge units in which every attention window is contiguous, and the windows' prefix sums in PATCH rows with empty windows
    (consecutive duplicates) removed."""
    side, unit = window_size // merge // patch, merge * merge
    index, cu, base = [], [0], 0
    for t, h, w in _grids(grid_thw):
        gh, gw = h // merge, w // merge
        idx = torch.arange(t * gh * gw).reshape(t, gh, gw)
        ph, pw = side - gh % side, side - gw % side               # (HF pads a whole extra window when the side divides)
        nh, nw = (gh + ph) // side, (gw + pw) // side
        pad = torch.nn.functional.pad(idx, (0, pw, 0, ph), "constant", -100)
        pad = pad.reshape(t, nh, side, nw, side).permute(0, 1, 3, 2, 4).reshape(t, nh * nw, side, side)
        lens = (pad != -100).sum([2, 3]).reshape(-1)
        flat = pad.reshape(-1)
        index.append(flat[flat != -100] + base)
        cu.extend((lens.cumsum(0) * unit + cu[-1]).tolist())
        base += t * gh * gw
    cu = torch.unique_consecutive(torch.tensor(cu, dtype=torch.int32))
    return torch.cat(index), cu


def vision_row_order(window_index: torch.Tensor, unit: int = 4) -> torch.Tensor:
    """The permutation of the processor's PATCH rows into window order: merge unit u holds rows unit * u .. unit * u + unit - 1."""
    return (window_index[:, None] * unit + torch.arange(unit)[None, :]).reshape(-1)


def vision_cu_image(grid_thw) -> torch.Tensor:
    """int32 [n + 1] prefix sums of the pictures' patch rows (one attention segment per frame: HF `get_vision_cu_seqlens`)."""
    lens = [h * w for t, h, w in _grids(grid_thw) for _ in range(t)]
    return torch.tensor([0] + lens, dtype=torch.int32).cumsum(0).to(torch.int32)


def vision_patch_positions(grid_thw, merge: int) -> torch.Tensor:
    """long [rows, 2]: the (h, w) grid position of every patch row in the processor's order (merge-block major): HF
    `get_vision_position_ids`."""
    out = []
    for t, h, w in _grids(grid_thw):
        hp, wp = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        shape = (h // merge, merge, w // merge, merge)
        hp, wp = hp.reshape(shape).transpose(1, 2).flatten(), wp.reshape(shape).transpose(1, 2).flatten()
        out.append(torch.stack([hp, wp], dim=-1).repeat(t, 1))
    return torch.cat(out)


def vision_rope_tables(pos_hw: torch.Tensor, head: int, theta: float = VISION_ROPE_THETA):
    """fp32 cos / sin [rows, head / 2] as `Qwen2_5_VisionRotaryEmbedding` + the tower's forward compute them: head / 4
    frequencies theta^(-2 i / (head / 2)), the first head / 4 columns turn with the row's h, the rest with its w; HF then repeats
    the head / 2 columns for the second half of the head, which the kernel does by addressing."""
    dim = head // 2
    inv = 1.0 / (theta ** (torch.arange(0, dim, 2, dtype=torch.float) / dim))
    ang = (pos_hw.unsqueeze(-1) * inv).flatten(1)
    return ang.cos().contiguous(), ang.sin().contiguous()


def mrope_positions(ids: torch.Tensor, lens: list[int], image_token_id: int, grid_thw, merge: int = 2) -> torch.Tensor:
    """int32 [3, sum(lens)]: Qwen2.5-VL's 3-D token positions (`Qwen2_5_VLModel.get_rope_index`) of the packed valid tokens.  Text
    runs count on in all three rows; a run of picture tokens takes the next grid: temporal = the run's start, height / width =
    start + the merged row / column; the count then moves on by max(h, w) / merge."""
    grids = iter(_grids(grid_thw))
    out = []
    for row in torch.split(ids, lens):
        is_img = (row == image_token_id).tolist()
        cur, i, parts = 0, 0, []
        while i < len(is_img):
            j = i
            while j < len(is_img) and is_img[j] == is_img[i]:
                j += 1
            if not is_img[i]:
                parts.append(torch.arange(j - i).view(1, -1).expand(3, -1) + cur)
                cur += j - i
            else:
                try:
                    t, h, w = next(grids)
                except StopIteration:
                    raise ValueError("more runs of picture tokens than pictures") from None
                gh, gw = h // merge, w // merge
                if j - i != t * gh * gw:
                    raise ValueError(f"a run of {j - i} picture tokens for a picture of {t * gh * gw} merged patches")
                tt, hh, ww = torch.meshgrid(torch.arange(t), torch.arange(gh) + cur, torch.arange(gw) + cur, indexing="ij")
                parts.append(torch.stack([tt + cur, hh, ww]).reshape(3, -1))
                cur += max(h, w) // merge
            i = j
        out.append(torch.cat(parts, dim=1) if parts else torch.zeros(3, 0, dtype=torch.long))
    if next(grids, None) is not None:
        raise ValueError("more pictures than runs of picture tokens")
    return torch.cat(out, dim=1).to(torch.int32).contiguous()


def vision_row_map(ids: torch.Tensor, image_token_id: int, window_index: torch.Tensor | None) -> torch.Tensor:
    """int32 [rows]: for every packed token the row of the tower's WINDOW-ORDER output it takes (-1: its token embedding).  HF
    scatters merger output k (in the processor's order) into the k-th picture token; output k sits at row argsort(window_index)[k]
    of the window-order result, so the reverse permutation is folded into the map."""
    img = ids == image_token_id
    out = torch.full((ids.numel(),), -1, dtype=torch.int32)
    n = int(img.sum())
    have = 0 if window_index is None else window_index.numel()
    if n != have:
        raise ValueError(f"{n} picture tokens in the prompt for {have} merged patch rows of the pictures")
    if n:
        out[img] = torch.argsort(window_index).to(torch.int32)
    return out


def pad_vision_block(blk, g: dict) -> dict:
    """One HF vision block's tensors as omni_vision_layer_weights wants them (bf16, row-major, zero-padded - all exact): the
    projection's input columns from `head` to 128 per head, the intermediate size to a multiple of 64 in gate | up (rows, bias)
    and down (columns)."""
    bf = lambda t: t.detach().to(torch.bfloat16)
    D, H, hd, I, Ip = g["hidden"], g["heads"], g["head"], g["inter"], g["inter_pad"]
    a, m = blk.attn, blk.mlp
    proj = bf(a.proj.weight).new_zeros(D, H, VISION_HEAD_PAD)
    proj[:, :, :hd] = bf(a.proj.weight).view(D, H, hd)
    gu_w = proj.new_zeros(2 * Ip, D)
    gu_w[:I], gu_w[Ip:Ip + I] = bf(m.gate_proj.weight), bf(m.up_proj.weight)
    gu_b = proj.new_zeros(2 * Ip)
    gu_b[:I], gu_b[Ip:Ip + I] = bf(m.gate_proj.bias), bf(m.up_proj.bias)
    down = proj.new_zeros(D, Ip)
    down[:, :I] = bf(m.down_proj.weight)
    return dict(norm1_w=bf(blk.norm1.weight).contiguous(), qkv_w=bf(a.qkv.weight).contiguous(), qkv_b=bf(a.qkv.bias).contiguous(),
                proj_w=proj.view(D, H * VISION_HEAD_PAD), proj_b=bf(a.proj.bias).contiguous(),
                norm2_w=bf(blk.norm2.weight).contiguous(), gate_up_w=gu_w, gate_up_b=gu_b, down_w=down,
                down_b=bf(m.down_proj.bias).contiguous())


_VISION_MATRICES = ("qkv_w", "proj_w", "gate_up_w", "down_w")


class NativeQwenEditPromptEncoder:
    """`QwenEditPromptEncoder` on this library: same processor, templates, drop index 64, outputs and mask.  The vision tower runs
    as ONE omni_qwen2_vision_forward over the patch rows of all pictures in window order, the language model as ONE
    omni_qwen2_text_forward_mm over the packed valid tokens, with Qwen2.5-VL's 3-D positions (`get_rope_index`) and the image
    embeddings gathered into the picture tokens' rows.  Built by `from_hf`; anything the kernels do not take raises ValueError
    there (or, for an input such as a video, at the call) - there is no fall-back to the HF model.
    The vision result of the last picture set is kept: a request's negative prompt reuses its positive prompt's vision forward."""

    def __init__(self, text: "NativeQwenPromptEncoder", vgeom: dict, vweights: dict, vlayers: list[dict], processor,
                 image_token_id: int, mrope_section: list[int], video_token_id: int | None = None, multi_image: bool = False,
                 template: str | None = None, drop_idx: int = EDIT_PROMPT_TEMPLATE_ENCODE_START_IDX, dtype=torch.bfloat16,
                 w_k32_blocked: bool = True):
        from .... import _native as N

        if not N.features() & N.FEATURE_VISION_ENCODER:
            raise N.OmniNativeError("this libomni_cdna4.so does not report OMNI_FEATURE_VISION_ENCODER: it has no "
                                    "omni_qwen2_vision_forward / omni_qwen2_text_forward_mm - rebuild it (python "
                                    "vllm_omni_amd/csrc/build.py); the native Edit prompt encoder never falls back to the HF model")
        if dtype != torch.bfloat16:
            raise ValueError(f"the native Edit prompt encoder computes in bfloat16, not {dtype}")
        self.text, self.vgeom, self.vweights, self.vlayers = text, vgeom, vweights, vlayers
        self.processor, self.dtype, self.multi_image = processor, dtype, multi_image
        self.image_token_id, self.video_token_id, self.mrope_section = int(image_token_id), video_token_id, list(mrope_section)
        self.prompt_template_encode = template or (EDIT_PLUS_PROMPT_TEMPLATE_ENCODE if multi_image else EDIT_PROMPT_TEMPLATE_ENCODE)
        self.prompt_template_encode_start_idx = drop_idx
        self.tokenizer_max_length = 1024
        self.w_k32_blocked = bool(w_k32_blocked)
        self.vones = torch.ones(vgeom["hidden"], dtype=torch.bfloat16, device=vweights["patch_w"].device)
        self._vdesc = self._vlayer_array = self._vworkspace = None
        self._vision_cache = None          # (grids, pixel_values on the host, window-order output on the device, window_index)

    @classmethod
    def from_hf(cls, vl_model, processor, multi_image: bool = False, free_source: bool = False, **kw):
        """From an HF `Qwen2_5_VLForConditionalGeneration`, on the device its weights are on: the vision and text weights are
        fused and zero-padded once (K32-blocked unless `w_k32_blocked=False`).  `free_source`: every HF block / decoder layer is
        dropped as soon as its copy exists (the HF model cannot run afterwards)."""
        from .... import ops

        vis, tm = vision_model_of(vl_model), text_model_of(vl_model)
        cfg = vl_model.config
        vcfg = getattr(cfg, "vision_config", None) or vis.config
        tg = check_text_geometry(tm.config)                        # refusals first: nothing is touched before all of them passed
        sec = check_mrope_section(tm.config)
        g = check_vision_geometry(vcfg, tg["hidden"])
        if len(vis.blocks) != g["layers"]:
            raise ValueError(f"the vision tower has {len(vis.blocks)} blocks, its config says {g['layers']}")
        blocked = bool(kw.get("w_k32_blocked", True))
        bf = lambda t: t.detach().to(torch.bfloat16).contiguous()
        mat = (lambda t: ops.w_to_k32_blocked(t.contiguous())) if blocked else (lambda t: t.contiguous())
        D = g["hidden"]
        pw = bf(vis.patch_embed.proj.weight).reshape(D, -1)
        if pw.shape[1] != g["patch_k"]:
            raise ValueError(f"the patch embedding has {pw.shape[1]} inputs per patch, its config says {g['patch_k']}")
        patch_w = pw.new_zeros(D, g["patch_k_pad"])
        patch_w[:, :g["patch_k"]] = pw
        mg = vis.merger
        vweights = dict(patch_w=mat(patch_w), merger_norm_w=bf(mg.ln_q.weight), merger_fc1_w=mat(bf(mg.mlp[0].weight)),
                        merger_fc1_b=bf(mg.mlp[0].bias), merger_fc2_w=mat(bf(mg.mlp[2].weight)), merger_fc2_b=bf(mg.mlp[2].bias))
        vlayers = []
        for i in range(len(vis.blocks)):
            L = pad_vision_block(vis.blocks[i], g)
            for n in _VISION_MATRICES:
                L[n] = mat(L[n])
            L["full_attention"] = int(i in g["full"])
            vlayers.append(L)
            if free_source:
                vis.blocks[i] = torch.nn.Identity()
        if free_source:
            vis.blocks = torch.nn.ModuleList()
        text = NativeQwenPromptEncoder.from_hf(tm, None, free_source=free_source, drop_idx=EDIT_PROMPT_TEMPLATE_ENCODE_START_IDX,
                                               rope_npos=EDIT_ROPE_NPOS, w_k32_blocked=blocked)
        return cls(text, g, vweights, vlayers, processor, cfg.image_token_id, sec, video_token_id=getattr(cfg, "video_token_id", None),
                   multi_image=multi_image, **kw)

    def _vision_descriptor(self):
        if self._vdesc is None:
            from .... import _native as N
            from ....ops import _p

            g = self.vgeom
            arr = (N.VisionLayerWeights * len(self.vlayers))()
            for rec, L in zip(arr, self.vlayers):
                for name, _ in N.VisionLayerWeights._fields_:
                    if name == "full_attention":
                        rec.full_attention = L[name]
                    elif name != "reserved":
                        setattr(rec, name, _p(L[name], name=name))
            w = N.VisionWeights()
            w.num_layers, w.hidden_size, w.num_heads, w.head_dim = len(self.vlayers), g["hidden"], g["heads"], g["head"]
            w.intermediate_size, w.patch_k, w.out_hidden_size = g["inter_pad"], g["patch_k_pad"], g["out"]
            w.gemm_w_k32_blocked, w.rms_norm_eps = int(self.w_k32_blocked), g["eps"]
            for name, t in self.vweights.items():
                setattr(w, name, _p(t, name=name))
            w.ones = _p(self.vones, name="ones")
            w.layers = arr
            self._vdesc, self._vlayer_array = w, arr
        return self._vdesc

    @torch.no_grad()
    def vision_forward(self, pixel_values: torch.Tensor, grid_thw):
        """The processor's `pixel_values` [rows, 1176] and `image_grid_thw` -> (the merger's output in WINDOW order
        [rows / 4, out] bf16 on the device, window_index).  HF's order is `out[argsort(window_index)]`."""
        from .... import ops

        g = self.vgeom
        grids = check_picture_grids(grid_thw, g["merge"])
        px = pixel_values.detach().cpu()
        if px.dim() != 2 or px.shape[1] != g["patch_k"] or px.shape[0] != sum(t * h * w for t, h, w in grids):
            raise ValueError(f"pixel_values of shape {tuple(px.shape)} for grids {grids} and {g['patch_k']} values per patch")
        c = self._vision_cache
        if c is not None and c[0] == grids and c[1].shape == px.shape and c[1].dtype == px.dtype and torch.equal(c[1], px):
            return c[2], c[3]
        dev = self.vones.device
        window_index, cu_window = vision_window_index(grids, g["merge"], g["window"], g["patch"])
        order = vision_row_order(window_index, g["merge"] ** 2)
        cu_image = vision_cu_image(grids)
        cos, sin = vision_rope_tables(vision_patch_positions(grids, g["merge"])[order], g["head"])
        pixels = torch.zeros(px.shape[0], g["patch_k_pad"], dtype=torch.bfloat16)
        pixels[:, :g["patch_k"]] = px[order].to(torch.bfloat16)      # (HF casts the fp32 pixels to the tower's dtype as well)
        cu = torch.cat([cu_window, cu_image]).to(dev)
        tabs = torch.cat([cos, sin]).to(dev)
        w = self._vision_descriptor()
        need = ops.qwen2_vision_workspace_bytes(w, px.shape[0])
        if self._vworkspace is None or self._vworkspace.numel() < need:
            self._vworkspace = torch.empty(need, dtype=torch.uint8, device=dev)
        out = ops.qwen2_vision_forward(w, pixels.to(dev), cu[:cu_window.numel()], cu[cu_window.numel():],
                                       int((cu_window[1:] - cu_window[:-1]).max()), int((cu_image[1:] - cu_image[:-1]).max()),
                                       tabs[:cos.shape[0]], tabs[cos.shape[0]:], self._vworkspace)
        self._vision_cache = (grids, px.clone(), out, window_index)
        return out, window_index

    @torch.no_grad()
    def get_image_features(self, pixel_values, grid_thw) -> torch.Tensor:
        """The merger's output in the processor's (HF's) order: what `Qwen2_5_VLModel.get_image_features` concatenates."""
        out, window_index = self.vision_forward(pixel_values, grid_thw)
        return out[torch.argsort(window_index).to(out.device)]

    @torch.no_grad()
    def encode_packed(self, ids, cu_seqlens, row_pos3, max_seqlen: int, vision_rows=None, vision_row_of=None) -> torch.Tensor:
        """Packed int32 tokens, their [3, rows] positions and the vision rows (all on the weights' device) -> last hidden state."""
        from .... import ops

        w = self.text._descriptor()
        need = ops.qwen2_text_workspace_bytes(w, ids.numel())
        if self.text._workspace is None or self.text._workspace.numel() < need:
            self.text._workspace = torch.zeros(need, dtype=torch.uint8, device=ids.device)   # zeroed: the error word in front
        return ops.qwen2_text_forward_mm(w, ids, cu_seqlens, row_pos3, self.mrope_section, max_seqlen, self.text._workspace,
                                         vision_rows=vision_rows, vision_row_of=vision_row_of)

    @torch.no_grad()
    def get_qwen_prompt_embeds(self, prompt, image=None, device=None, dtype=None):
        prompt = [prompt] if isinstance(prompt, str) else list(prompt)
        wdev = self.text.embed_tokens.device
        dev = device if device is not None else wdev
        drop = self.prompt_template_encode_start_idx
        if isinstance(image, (list, tuple)):
            image = [to_processor_image(im) for im in image]
        elif image is not None:
            image = to_processor_image(image)
        if self.multi_image:
            n = len(image) if isinstance(image, list) else (0 if image is None else 1)
            base = "".join(EDIT_PLUS_IMG_PROMPT.format(i + 1) for i in range(n))
            txt = [self.prompt_template_encode.format(base + e) for e in prompt]
        else:
            txt = [self.prompt_template_encode.format(e) for e in prompt]
        inputs = self.processor(text=txt, images=image, padding=True, return_tensors="pt")
        if getattr(inputs, "pixel_values_videos", None) is not None or getattr(inputs, "video_grid_thw", None) is not None:
            raise ValueError("video inputs: the native Edit prompt encoder takes still pictures only")
        ids, cu, _, lens = pack_tokens(inputs.input_ids.cpu(), inputs.attention_mask.cpu())
        if len(lens) > MAX_PROMPTS_PER_FORWARD:
            raise ValueError(f"{len(lens)} prompts in one call: at most {MAX_PROMPTS_PER_FORWARD}")
        vocab = self.text.embed_tokens.shape[0]
        if ids.numel() == 0 or int(ids.min()) < 0 or int(ids.max()) >= vocab:
            raise ValueError(f"token ids outside the embedding table [0, {vocab})")
        if self.video_token_id is not None and bool((ids == self.video_token_id).any()):
            raise ValueError("video tokens in the prompt: the native Edit prompt encoder takes still pictures only")
        grids, vision_rows, window_index = [], None, None
        if getattr(inputs, "pixel_values", None) is not None:
            grids = check_picture_grids(inputs.image_grid_thw, self.vgeom["merge"])
            vision_rows, window_index = self.vision_forward(inputs.pixel_values, grids)
        row_of = vision_row_map(ids, self.image_token_id, window_index)
        pos3 = mrope_positions(ids, lens, self.image_token_id, grids, self.vgeom["merge"])
        if int(pos3.max()) >= self.text.rope_npos:
            raise ValueError(f"a token position of {int(pos3.max())} exceeds the RoPE table of {self.text.rope_npos} positions")
        R, n = ids.numel(), len(lens)
        packed = torch.cat([ids, cu, pos3.reshape(-1), row_of]).to(wdev)                    # one upload
        hidden = self.encode_packed(packed[:R], packed[R:R + n + 1], packed[R + n + 1:4 * R + n + 1].view(3, R), max(lens),
                                    vision_rows=vision_rows,
                                    vision_row_of=packed[4 * R + n + 1:] if vision_rows is not None else None)
        emb, msk = packed_drop_pad(hidden, lens, drop)
        return emb.to(device=dev, dtype=dtype or self.dtype), msk.to(dev)


# ---- the native captioner: greedy decode with a KV cache on this library (the Layered pipeline's auto-caption) -----------------
CAPTION_DECODE_CHUNK = 16          # decode steps queued between two reads of the stop flags
CAPTION_CAPACITY_ROUND = 64        # the cache capacity is rounded up to whole key chunks of the decode attention
# generation settings that would change a greedy result if honoured, with the value at which they do nothing
_GENERATION_NEUTRAL = dict(num_beam_groups=1, penalty_alpha=None, no_repeat_ngram_size=0, encoder_no_repeat_ngram_size=0,
                           bad_words_ids=None, force_words_ids=None, constraints=None, forced_bos_token_id=None,
                           forced_eos_token_id=None, min_length=0, min_new_tokens=None, encoder_repetition_penalty=1.0,
                           suppress_tokens=None, begin_suppress_tokens=None, sequence_bias=None, guidance_scale=None,
                           diversity_penalty=0.0, exponential_decay_length_penalty=None, prompt_lookup_num_tokens=None,
                           renormalize_logits=False, remove_invalid_values=False, dola_layers=None, watermarking_config=None,
                           stop_strings=None, token_healing=False, max_time=None)


def check_generation_config(gc) -> dict:
    """What the native captioner takes from an HF `generation_config`: {"repetition_penalty", "eos_ids"}.  Greedy search
    (`num_beams == 1`, `do_sample=False`), or sampling with `top_k == 1` - one survivor, so the result IS the penalised argmax and
    temperature / top_p cannot change it (what the Qwen2.5-VL instruct checkpoints ship).  A setting is honoured or refused, never
    ignored: anything else raises NotImplementedError naming the field."""
    def refuse(field, why):
        raise NotImplementedError(f"the native captioner does not take generation_config.{field} = {getattr(gc, field, None)!r}: {why}")

    beams = getattr(gc, "num_beams", 1)
    if beams not in (None, 1):
        refuse("num_beams", "it decodes greedily, one sequence")
    if getattr(gc, "do_sample", False):
        if getattr(gc, "top_k", None) != 1:
            refuse("top_k", "do_sample=True is taken only with top_k == 1, where one token survives and sampling is the argmax")
    for field, neutral in _GENERATION_NEUTRAL.items():
        v = getattr(gc, field, neutral)
        if v is not None and v != neutral and not (isinstance(v, (list, tuple, dict)) and len(v) == 0):
            refuse(field, "only repetition_penalty and eos_token_id shape the greedy decode")
    pen = getattr(gc, "repetition_penalty", None)
    pen = 1.0 if pen is None else float(pen)
    if not pen > 0:
        refuse("repetition_penalty", "it must be positive")
    eos = getattr(gc, "eos_token_id", None)
    eos = [] if eos is None else ([int(eos)] if isinstance(eos, int) else [int(e) for e in eos])
    if len(eos) > 8:
        refuse("eos_token_id", "at most 8 ids")
    return dict(repetition_penalty=pen, eos_ids=eos)


class NativeQwenCaptioner:
    """`text_encoder.generate(**inputs, max_new_tokens=...)` of the Layered pipeline's auto-caption on this library: the vision
    tower (the composed `NativeQwenEditPromptEncoder`), a prefill that fills a KV cache (omni_qwen2_text_prefill) and a greedy
    decode of one token per omni_qwen2_text_decode_step - steps are queued in chunks with no host round trip per token; between
    chunks one small read of the stop flags.  Built by `from_hf`; generation settings the decode does not implement raise there."""

    def __init__(self, encoder: "NativeQwenEditPromptEncoder", lm_head: torch.Tensor, generation: dict):
        from .... import _native as N

        if not N.features() & N.FEATURE_TEXT_DECODE:
            raise N.OmniNativeError("this libomni_cdna4.so does not report OMNI_FEATURE_TEXT_DECODE: it has no "
                                    "omni_qwen2_text_prefill / omni_qwen2_text_decode_step - rebuild it (python "
                                    "vllm_omni_amd/csrc/build.py); the native captioner never falls back to the HF model")
        vocab, hidden = encoder.text.embed_tokens.shape
        if tuple(lm_head.shape) != (vocab, hidden) or lm_head.dtype != torch.bfloat16 or not lm_head.is_contiguous():
            raise ValueError(f"lm_head must be a contiguous bfloat16 [{vocab}, {hidden}] matrix, got {tuple(lm_head.shape)} {lm_head.dtype}")
        self.encoder, self.lm_head, self.processor = encoder, lm_head, encoder.processor
        self.repetition_penalty, self.eos_ids = float(generation["repetition_penalty"]), list(generation["eos_ids"])
        self._state = None

    @classmethod
    def from_hf(cls, vl_model, processor, free_source: bool = False, generation_config=None, **kw):
        """From an HF `Qwen2_5_VLForConditionalGeneration` and its processor.  The generation settings come from
        `vl_model.generation_config` (or `generation_config`) and are checked FIRST: a server fails at load, not at the first
        empty prompt."""
        generation = check_generation_config(generation_config if generation_config is not None else vl_model.generation_config)
        head = getattr(vl_model, "lm_head", None)
        if head is None or getattr(head, "bias", None) is not None:
            raise ValueError("the native captioner needs the model's lm_head (a Linear without bias)")
        lm_head = head.weight.detach().to(torch.bfloat16).contiguous()
        enc = NativeQwenEditPromptEncoder.from_hf(vl_model, processor, multi_image=False, free_source=free_source, **kw)
        return cls(enc, lm_head, generation)

    def _inputs(self, text: str, picture):
        """processor -> vision tower -> the packed prefill batch on the device, as `get_qwen_prompt_embeds` builds it."""
        enc = self.encoder
        wdev = enc.text.embed_tokens.device
        inputs = self.processor(text=[text] if isinstance(text, str) else list(text),
                                images=None if picture is None else to_processor_image(picture), padding=True, return_tensors="pt")
        if getattr(inputs, "pixel_values_videos", None) is not None or getattr(inputs, "video_grid_thw", None) is not None:
            raise ValueError("video inputs: the native captioner takes still pictures only")
        ids, cu, _, lens = pack_tokens(inputs.input_ids.cpu(), inputs.attention_mask.cpu())
        if len(lens) != 1:
            raise ValueError(f"{len(lens)} prompts in one call: the captioner writes one caption per call")
        vocab = enc.text.embed_tokens.shape[0]
        if ids.numel() == 0 or int(ids.min()) < 0 or int(ids.max()) >= vocab:
            raise ValueError(f"token ids outside the embedding table [0, {vocab})")
        grids, vision_rows, window_index = [], None, None
        if getattr(inputs, "pixel_values", None) is not None:
            grids = check_picture_grids(inputs.image_grid_thw, enc.vgeom["merge"])
            vision_rows, window_index = enc.vision_forward(inputs.pixel_values, grids)
        row_of = vision_row_map(ids, enc.image_token_id, window_index)
        pos3 = mrope_positions(ids, lens, enc.image_token_id, grids, enc.vgeom["merge"])
        R = ids.numel()
        packed = torch.cat([ids, cu, pos3.reshape(-1), row_of]).to(wdev)                    # one upload
        return dict(ids=packed[:R], cu=packed[R:R + 2], pos3=packed[R + 2:4 * R + 2].view(3, R), rows=R, max_pos=int(pos3.max()),
                    vision_rows=vision_rows, vision_row_of=packed[4 * R + 2:] if vision_rows is not None else None,
                    host_ids=ids)

    def _decode_state(self, rows: int, max_new_tokens: int):
        from .... import ops

        enc = self.encoder
        w = enc.text._descriptor()
        need = ops.qwen2_text_workspace_bytes(w, rows)
        if enc.text._workspace is None or enc.text._workspace.numel() < need:
            enc.text._workspace = torch.zeros(need, dtype=torch.uint8, device=self.lm_head.device)   # zeroed: the error word in front
            self._state = None                                                                   # (it names the workspace)
        capacity = -(-(rows + max_new_tokens) // CAPTION_CAPACITY_ROUND) * CAPTION_CAPACITY_ROUND
        st = self._state
        if st is None or st.capacity < capacity or st.max_new != max_new_tokens:
            st = self._state = ops.qwen2_decode_state(w, self.lm_head, enc.text._workspace, 1, capacity, max_new_tokens,
                                                      eos_ids=self.eos_ids, repetition_penalty=self.repetition_penalty)
        return w, st

    @torch.no_grad()
    def prefill(self, text: str, picture, max_new_tokens: int = 512):
        """Vision tower + prefill: -> (weights descriptor, decode state with the first token picked, the prompt's token count)."""
        from .... import ops

        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be at least 1")
        x = self._inputs(text, picture)
        if x["max_pos"] + max_new_tokens >= self.encoder.text.rope_npos:
            raise ValueError(f"position {x['max_pos']} + {max_new_tokens} new tokens exceed the RoPE table of "
                             f"{self.encoder.text.rope_npos} positions")
        w, st = self._decode_state(x["rows"], max_new_tokens)
        ops.qwen2_text_prefill(w, st, x["ids"], x["cu"], x["pos3"], self.encoder.mrope_section, x["rows"],
                               vision_rows=x["vision_rows"], vision_row_of=x["vision_row_of"])
        return w, st, x["rows"]

    @torch.no_grad()
    def generate_ids(self, text: str, picture, max_new_tokens: int = 512, chunk: int = CAPTION_DECODE_CHUNK) -> list[int]:
        """The generated token ids (what HF's `generate` returns behind the prompt), the EOS token included when one ended it."""
        from .... import _native as N
        from .... import ops

        w, st, _ = self.prefill(text, picture, max_new_tokens)
        left = max_new_tokens - 1                                       # the prefill picked the first token
        while True:
            flags = st.ctrl[N.DECODE_DONE:N.DECODE_N_GENERATED + 1, :1].cpu()      # the one small read between chunks
            if int(flags[0, 0]) or left <= 0:
                break
            n = min(int(chunk), left)
            ops.qwen2_text_decode_step(w, st, n)
            left -= n
        return st.out_tokens[0, :int(flags[1, 0])].cpu().tolist()

    def generate(self, text: str, picture, max_new_tokens: int = 512, chunk: int = CAPTION_DECODE_CHUNK) -> str:
        """The caption, decoded exactly as the reference decodes it (pipeline_qwen_image_layered.py:509-513)."""
        toks = self.generate_ids(text, picture, max_new_tokens, chunk)
        for i, t in enumerate(toks):
            if t in self.eos_ids:
                toks = toks[:i]
                break
        return self.processor.batch_decode([toks], skip_special_tokens=True, clean_up_tokenization_spaces=False)[0].strip()
