"""Shared by the native Edit prompt encoder's tests (not collected): random-weight HF Qwen2.5-VL models at a geometry the native
kernels take, the stub processor at a matching size, and the thin wrapper that calls HF with EXPLICIT 3-D position_ids.

Under the installed transformers `Qwen2_5_VLModel.compute_3d_position_ids` builds the 3-D positions only when the caller passes
`mm_token_type_ids`; the Edit encoders do not, so HF would number picture tokens sequentially.  The native encoder implements
Qwen2.5-VL's definition (`get_rope_index`); every comparison here therefore hands HF `position_ids=get_rope_index(...)`."""
import copy

import torch

import vl_stubs as V

SMALL = dict(vision=dict(depth=2, hidden_size=320, out_hidden_size=512, num_heads=4, intermediate_size=420, window_size=112,
                         fullatt_block_indexes=[1]),
             text=dict(hidden_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, intermediate_size=192))
REAL_WIDTH = dict(vision=dict(depth=2, hidden_size=1280, out_hidden_size=3584, num_heads=16, intermediate_size=3420, window_size=112,
                              fullatt_block_indexes=[1]),
                  text=dict(hidden_size=3584, num_hidden_layers=1, num_attention_heads=28, num_key_value_heads=4,
                            intermediate_size=18944))


def make_vl_model(geom: dict, seed: int, device="cpu", qk_gain: float = 1.0):
    """An fp32 `Qwen2_5_VLForConditionalGeneration` of `geom` with weights, biases and norm weights away from their trivial
    initial values (what tests/test_gpu_text_encoder.py::_hf_pair does for the text model alone)."""
    from transformers import Qwen2_5_VLConfig, Qwen2_5_VLForConditionalGeneration

    cfg = Qwen2_5_VLConfig(
        text_config=dict(vocab_size=V.VOCAB, max_position_embeddings=8192, bos_token_id=1, eos_token_id=2, pad_token_id=0,
                         rope_scaling={"type": "default", "mrope_section": [16, 24, 24], "rope_type": "default"}, **geom["text"]),
        vision_config=dict(patch_size=14, spatial_merge_size=2, temporal_patch_size=2, in_channels=3, **geom["vision"]),
        image_token_id=V.IMAGE_TOKEN, video_token_id=499, vision_start_token_id=V.VISION_START, vision_end_token_id=V.VISION_END)
    torch.manual_seed(seed)
    with torch.device(device):
        m = Qwen2_5_VLForConditionalGeneration(cfg).float().eval()
    g = torch.Generator(device=device).manual_seed(seed + 1)
    rnd = lambda t, s: torch.randn(t.shape, generator=g, device=t.device) * s
    with torch.no_grad():
        for L in m.model.language_model.layers:
            for p in (L.self_attn.q_proj, L.self_attn.k_proj):
                p.weight.mul_(qk_gain)
            for p in (L.self_attn.q_proj, L.self_attn.k_proj, L.self_attn.v_proj):
                p.bias.copy_(rnd(p.bias, 0.2))
            for n in (L.input_layernorm, L.post_attention_layernorm):
                n.weight.copy_(1 + rnd(n.weight, 0.1))
        m.model.language_model.norm.weight.copy_(1 + rnd(m.model.language_model.norm.weight, 0.1))
        vis = m.model.visual
        for B in vis.blocks:
            for p in (B.attn.qkv, B.attn.proj, B.mlp.gate_proj, B.mlp.up_proj, B.mlp.down_proj):
                p.bias.copy_(rnd(p.bias, 0.2))
            B.attn.qkv.weight[:2 * geom["vision"]["hidden_size"]].mul_(qk_gain)
            for n in (B.norm1, B.norm2):
                n.weight.copy_(1 + rnd(n.weight, 0.1))
        vis.merger.ln_q.weight.copy_(1 + rnd(vis.merger.ln_q.weight, 0.1))
        for p in (vis.merger.mlp[0], vis.merger.mlp[2]):
            p.bias.copy_(rnd(p.bias, 0.2))
    return m


def hf_pair(geom: dict, seed: int, device, qk_gain: float = 1.0):
    """(HF bf16 model, the same model in fp32): cast to bf16 with the rotary frequencies of both towers kept in fp32, as a
    checkpoint load leaves them; the fp32 twin holds the SAME (bf16-rounded) weights."""
    m = make_vl_model(geom, seed, device, qk_gain)
    inv_t, inv_v = m.model.language_model.rotary_emb.inv_freq.clone(), m.model.visual.rotary_pos_emb.inv_freq.clone()
    eager = m.to(torch.bfloat16)
    eager.model.language_model.rotary_emb.inv_freq = inv_t
    eager.model.language_model.rotary_emb.original_inv_freq = inv_t.clone()
    eager.model.visual.rotary_pos_emb.inv_freq = inv_v
    oracle = copy.deepcopy(eager).float().eval()
    return eager.eval(), oracle


class HFWithPositions:
    """What `QwenEditPromptEncoder` calls as its model, with `position_ids=get_rope_index(...)` added to the call."""

    def __init__(self, model):
        self.model = model
        self.config = model.config

    def parameters(self):
        return self.model.parameters()

    def positions(self, input_ids, attention_mask, image_grid_thw):
        mm = (input_ids == self.model.config.image_token_id).int()
        return self.model.model.get_rope_index(input_ids, mm, image_grid_thw=image_grid_thw, attention_mask=attention_mask)[0]

    def __call__(self, input_ids=None, attention_mask=None, output_hidden_states=True, pixel_values=None, image_grid_thw=None):
        kw = {} if pixel_values is None else dict(pixel_values=pixel_values, image_grid_thw=image_grid_thw)
        return self.model(input_ids=input_ids, attention_mask=attention_mask, output_hidden_states=True,
                          position_ids=self.positions(input_ids, attention_mask, image_grid_thw), **kw)


def processor(max_side_patches: int = 22):
    """The stub processor with room for pictures of up to `max_side_patches`^2 14-pixel patches."""
    return V.StubVLProcessor(min_pixels=56 * 56, max_pixels=(14 * max_side_patches) ** 2)


def pictures(grids, seed: int = 3):
    """PIL pictures whose processor grids are exactly `grids` [(h, w) in patches, both even]."""
    import numpy as np
    from PIL import Image

    rng = np.random.RandomState(seed)
    return [Image.fromarray(rng.randint(0, 256, size=(14 * h, 14 * w, 3), dtype=np.uint8)) for h, w in grids]
