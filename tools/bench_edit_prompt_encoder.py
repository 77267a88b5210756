#!/usr/bin/env python3
"""First measurement of Edit prompt encoding: HF eager `Qwen2_5_VLForConditionalGeneration` (vision tower + language model) against
the native encoder (omni_qwen2_vision_forward + omni_qwen2_text_forward_mm), same process, same random weights, real geometry
(vision: 32 blocks at 1280 / 16 heads of 80 / 3420, window 112, full attention in blocks 7, 15, 23, 31, merger to 3584;
text: 28 layers at 3584 / 28 over 4 heads / 18944).

    python tools/bench_edit_prompt_encoder.py [--vision-layers 32] [--text-layers 28] [--iters 10] [--warmup 3]
                                              [--out profiles/edit_prompt_encoder_first_measurement.txt]

Two requests, each a positive and a negative prompt over the same pictures, timed through `get_qwen_prompt_embeds` (processor,
upload, forward, drop + pad: what a request pays):
  (a) one 1036 x 1036 picture (74 x 74 patches, 1369 picture tokens): Edit;
  (b) three 392 x 392 pictures (28 x 28 patches each, 3 x 196 picture tokens): Edit-Plus.
HF is called through a wrapper that passes `position_ids=get_rope_index(...)`, so both sides compute Qwen2.5-VL's 3-D positions.
The processor is the test stand-in (oracle/vl_stubs.py: HF's real image processor + a word tokenizer); its share is printed.
Times are medians of host-clock intervals around single calls ending in a synchronise (the HF path synchronises inside its window
loop, so an event interval would not differ), after warm-up, the two encoders alternating.  The vision tower and the language model
are also timed on their own; the native negative prompt is timed with the vision cache (what a request pays) and without it."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]


class HFWithPositions:
    """The HF model as `QwenEditPromptEncoder` calls it, with explicit 3-D position_ids."""

    def __init__(self, model):
        self.model = model

    def parameters(self):
        return self.model.parameters()

    def __call__(self, input_ids=None, attention_mask=None, output_hidden_states=True, pixel_values=None, image_grid_thw=None):
        mm = (input_ids == self.model.config.image_token_id).int()
        pos = self.model.model.get_rope_index(input_ids, mm, image_grid_thw=image_grid_thw, attention_mask=attention_mask)[0]
        kw = {} if pixel_values is None else dict(pixel_values=pixel_values, image_grid_thw=image_grid_thw)
        return self.model(input_ids=input_ids, attention_mask=attention_mask, output_hidden_states=True, position_ids=pos, **kw)


def build_model(vision_layers: int, text_layers: int, dev):
    import vl_stubs as V
    from transformers import Qwen2_5_VLConfig, Qwen2_5_VLForConditionalGeneration

    full = [i for i in (7, 15, 23, 31) if i < vision_layers] or [vision_layers - 1]
    cfg = Qwen2_5_VLConfig(
        text_config=dict(vocab_size=V.VOCAB, hidden_size=3584, num_hidden_layers=text_layers, num_attention_heads=28,
                         num_key_value_heads=4, intermediate_size=18944, max_position_embeddings=8192, bos_token_id=1,
                         eos_token_id=2, pad_token_id=0,
                         rope_scaling={"type": "default", "mrope_section": [16, 24, 24], "rope_type": "default"}),
        vision_config=dict(depth=vision_layers, hidden_size=1280, out_hidden_size=3584, num_heads=16, intermediate_size=3420,
                           patch_size=14, spatial_merge_size=2, temporal_patch_size=2, window_size=112,
                           fullatt_block_indexes=full, in_channels=3),
        image_token_id=V.IMAGE_TOKEN, video_token_id=499, vision_start_token_id=V.VISION_START, vision_end_token_id=V.VISION_END)
    torch.manual_seed(0)
    with torch.device(dev):
        m = Qwen2_5_VLForConditionalGeneration(cfg).eval()
    inv_t, inv_v = m.model.language_model.rotary_emb.inv_freq.clone(), m.model.visual.rotary_pos_emb.inv_freq.clone()
    m = m.to(torch.bfloat16)                       # ... with the rotary frequencies in fp32, as a checkpoint load leaves them
    m.model.language_model.rotary_emb.inv_freq = inv_t
    m.model.visual.rotary_pos_emb.inv_freq = inv_v
    return m


def wall(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.float(), b.float()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--vision-layers", type=int, default=32)
    ap.add_argument("--text-layers", type=int, default=28)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_prompt_encoder_first_measurement.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_edit_prompt_encoder: no GPU - nothing is measured without one", file=sys.stderr)
        return 2

    import numpy as np
    import vl_stubs as V
    from PIL import Image

    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import NativeQwenEditPromptEncoder, QwenEditPromptEncoder

    dev = torch.device("cuda", torch.cuda.current_device())
    model = build_model(args.vision_layers, args.text_layers, dev)
    proc = V.StubVLProcessor(min_pixels=56 * 56, max_pixels=1036 * 1036)
    rng = np.random.RandomState(1)
    pic = lambda side: Image.fromarray(rng.randint(0, 256, size=(side, side, 3), dtype=np.uint8))
    cases = [("a", "one 1036 x 1036 picture (Edit)", False, [pic(1036)]), ("b", "three 392 x 392 pictures (Edit-Plus)", True,
                                                                          [pic(392) for _ in range(3)])]
    pos_prompt = "replace the sky with a thunderstorm and keep the house, the fence and the light on the porch as they are"
    neg_prompt = "blurry, low contrast, washed out colours"
    med = statistics.median
    lines = [f"Edit prompt encoding, HF eager vs native (omni_qwen2_vision_forward + omni_qwen2_text_forward_mm); "
             f"{torch.cuda.get_device_name(dev)}",
             f"geometry: vision {args.vision_layers} blocks 1280 / 16 x 80 / 3420, text {args.text_layers} layers 3584 / 28 over 4 / 18944, "
             "random weights, stub processor, HF called with position_ids=get_rope_index(...)",
             f"median of {args.iters} single calls after {args.warmup} warm-up calls, encoders alternating; host clock around the call "
             "ending in a synchronise, ms", ""]
    for tag, what, multi, pics in cases:
        hf = QwenEditPromptEncoder(HFWithPositions(model), proc, multi_image=multi)
        native = NativeQwenEditPromptEncoder.from_hf(model, proc, multi_image=multi)
        image = pics if multi else pics[0]
        px = proc.image_processor(images=pics, return_tensors="pt")
        pv, thw = px["pixel_values"], px["image_grid_thw"]
        pv_dev, thw_dev = pv.to(dev), thw.to(dev)
        t_proc = med([wall(lambda: proc.image_processor(images=pics, return_tensors="pt")) for _ in range(3)])

        def native_cold(prompt):
            native._vision_cache = None
            return native.get_qwen_prompt_embeds(prompt, image=image)

        def native_vision():
            native._vision_cache = None
            return native.vision_forward(pv, thw)

        runs = {
            "hf positive": lambda: hf.get_qwen_prompt_embeds(pos_prompt, image=image),
            "hf negative": lambda: hf.get_qwen_prompt_embeds(neg_prompt, image=image),
            "hf vision tower alone": lambda: model.model.get_image_features(pv_dev, thw_dev),
            "native positive (vision + text)": lambda: native_cold(pos_prompt),
            "native negative, vision cached": lambda: native.get_qwen_prompt_embeds(neg_prompt, image=image),
            "native negative, no cache": lambda: native_cold(neg_prompt),
            "native vision tower alone": native_vision,
        }
        with torch.no_grad():
            for _ in range(args.warmup):
                for fn in runs.values():
                    fn()
            t = {k: [] for k in runs}
            for _ in range(args.iters):                               # alternate: all see the same neighbours on the box
                for k, fn in runs.items():
                    t[k].append(wall(fn))
            e_hf, _ = hf.get_qwen_prompt_embeds(pos_prompt, image=image)
            e_na, _ = native.get_qwen_prompt_embeds(pos_prompt, image=image)
        m = {k: med(v) for k, v in t.items()}
        lines.append(f"case ({tag}): {what}; patch rows {pv.shape[0]}, prompt rows {e_hf.shape[1] + 64} positive; "
                     f"image processor alone {t_proc:.1f}")
        for k in runs:
            lines.append(f"  {k:34s} {m[k]:9.2f}   (min {min(t[k]):.2f}, max {max(t[k]):.2f})")
        hf_req = m["hf positive"] + m["hf negative"]
        na_req = m["native positive (vision + text)"] + m["native negative, vision cached"]
        na_req_nc = m["native positive (vision + text)"] + m["native negative, no cache"]
        lines.append(f"  hf language model + host (positive - vision alone)      {m['hf positive'] - m['hf vision tower alone']:9.2f}")
        lines.append(f"  native language model + host (negative, vision cached)  {m['native negative, vision cached']:9.2f}")
        lines.append(f"  request (positive + negative): hf {hf_req:.2f}, native {na_req:.2f} = {na_req / hf_req:.3f} x; "
                     f"without the vision cache {na_req_nc:.2f} = {na_req_nc / hf_req:.3f} x")
        lines.append(f"  vision tower alone: native / hf = {m['native vision tower alone'] / m['hf vision tower alone']:.3f}; "
                     f"outputs: rel-L2 native vs hf eager {rel_l2(e_na, e_hf):.3e}")
        lines.append("")
        del native, hf
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
