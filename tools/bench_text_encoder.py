#!/usr/bin/env python3
"""First measurement of prompt encoding: HF eager `Qwen2_5_VLTextModel` against the native encoder (omni_qwen2_text_forward),
same process, same random weights, real geometry (hidden 3584, 28 query heads over 4 K/V heads, intermediate 18944, 28 layers).

    python tools/bench_text_encoder.py [--layers 28] [--iters 20] [--warmup 5] [--out profiles/text_encoder_first_measurement.txt]

Two shapes, each timed through `get_qwen_prompt_embeds` (tokenizer, upload, forward, drop + pad: what a request pays):
  (a) a positive and a negative prompt of about 80 tokens each - the usual text-to-image request;
  (b) eight prompts of about 300 tokens.
`ByteTokenizer` stands in for the checkpoint's tokenizer (one token per byte), with a short template so that the token counts
are the ones named above.  Times are medians of HIP-event intervals around single calls after warm-up, the two encoders
alternating; a host clock around the same calls (ending in a synchronise) is printed next to them.  The floor is the decoder
weights streamed once at 8 TB/s.  bench.py feeds `prompt_embeds` and never sees this stage."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEMPLATE, DROP = "<|user|>{}<|end|>", 8            # 15 template tokens under ByteTokenizer
HBM_BYTES_PER_S = 8.0e12


def prompts_for(shape: str) -> list[str]:
    text = "a watercolour of a lighthouse at dusk, gulls over the breakers, warm light in the lantern room, long shadows; "
    if shape == "a":
        return [(text * 2)[:65], ("blurry, low contrast, " * 4)[:62]]                      # 80 and 77 tokens
    return [(text * 4)[:265 + 10 * i] for i in range(8)]                                    # 280 .. 350 tokens


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.float(), b.float()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def timed(fn, iters: int):
    ev, wall = [], []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return ev, wall


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_encoder_first_measurement.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_text_encoder: no GPU - nothing is measured without one", file=sys.stderr)
        return 2

    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import ByteTokenizer, NativeQwenPromptEncoder, QwenPromptEncoder

    dev = torch.device("cuda", torch.cuda.current_device())
    with torch.device(dev):
        model = QwenPromptEncoder.random_init(hidden_size=3584, num_layers=args.layers, num_heads=28, num_kv_heads=4,
                                              intermediate_size=18944, device=dev, dtype=torch.bfloat16, seed=0).model
    # the rotary frequencies in fp32, as a checkpoint load leaves them (random_init's `.to(bfloat16)` rounds the buffer too)
    model.rotary_emb.inv_freq = 1.0 / (1e6 ** (torch.arange(0, 128, 2, dtype=torch.int64, device=dev).float() / 128))
    tok = ByteTokenizer()
    hf = QwenPromptEncoder(model, tok, template=TEMPLATE, drop_idx=DROP)
    native = NativeQwenPromptEncoder.from_hf(model, tok, template=TEMPLATE, drop_idx=DROP)
    wbytes = sum(t.numel() * t.element_size() for L in native.layers for t in L.values())
    floor_ms = wbytes / HBM_BYTES_PER_S * 1e3

    lines = [f"prompt encoding, HF eager vs native (omni_qwen2_text_forward); {torch.cuda.get_device_name(dev)}",
             f"geometry: hidden 3584, 28 / 4 heads of 128, intermediate 18944, {args.layers} layers, random weights, ByteTokenizer",
             f"decoder weights {wbytes / 1e9:.2f} GB -> floor {floor_ms:.2f} ms at 8 TB/s (weights streamed once)",
             f"median of {args.iters} single calls of get_qwen_prompt_embeds after {args.warmup} warm-up calls, encoders alternating;",
             "ev = HIP-event interval around the call, wall = host clock around the call ending in a synchronise", ""]
    ok = True
    for shape in ("a", "b"):
        prompts = prompts_for(shape)
        ntok = [len(TEMPLATE.format(p).encode()) for p in prompts]
        for _ in range(args.warmup):
            e_hf, _ = hf.get_qwen_prompt_embeds(prompts)
            e_na, _ = native.get_qwen_prompt_embeds(prompts)
        res = {"hf": ([], []), "native": ([], [])}
        for _ in range(args.iters):                                   # alternate: both see the same neighbours on the box
            for name, enc in (("hf", hf), ("native", native)):
                ev, wall = timed(lambda: enc.get_qwen_prompt_embeds(prompts), 1)
                res[name][0].extend(ev)
                res[name][1].extend(wall)
        med = {k: (statistics.median(v[0]), statistics.median(v[1]), min(v[0]), max(v[0])) for k, v in res.items()}
        lines.append(f"shape ({shape}): {len(prompts)} prompts, tokens {ntok} (sum {sum(ntok)})")
        for k in ("hf", "native"):
            m = med[k]
            lines.append(f"  {k:7s} ev {m[0]:8.3f} ms (min {m[2]:.3f}, max {m[3]:.3f})   wall {m[1]:8.3f} ms   "
                         f"{m[0] / floor_ms:6.2f} x floor")
        lines.append(f"  native / hf = {med['native'][0] / med['hf'][0]:.3f} (ev), {med['native'][1] / med['hf'][1]:.3f} (wall); "
                     f"outputs: rel-L2 native vs hf eager {rel_l2(e_na, e_hf):.3e}")
        if shape == "a" and med["native"][0] > med["hf"][0]:
            ok = False
            lines.append("  NATIVE IS SLOWER THAN HF EAGER AT SHAPE (a): the condition of the feature is not met")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
