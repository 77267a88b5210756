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
outputs and mask (text-only prompts; the Edit encoders below stay on HF)."""
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
                 w_k32_blocked: bool = True):
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
        self.rope_npos = max(2048, tokenizer_max_length + drop_idx)
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
