#!/usr/bin/env python3
"""First measurement of the auto-caption: HF `generate` against the native captioner (omni_qwen2_text_prefill +
omni_qwen2_text_decode_step), same process, same random weights, real geometry (hidden 3584, 28 query heads over 4 K/V heads,
intermediate 18944, 28 layers, an untied lm_head of 152064 rows; the real vision tower).

    python tools/bench_captioner.py [--layers 28] [--tokens 256] [--iters 3] [--out profiles/captioner_first_measurement.txt]

  (a) a caption of `--tokens` tokens for one picture: seconds per caption and ms per decoded token (the prefill and the vision
      tower are timed apart), HF `generate` and the native captioner alternating, no EOS so that both write every token;
  (b) the GEMV alone: the M = 1 products of one decode step (q|k|v, o, gate|up, down over all layers, then the lm_head) through
      omni_gemv_bf16 and through omni_gemm_bf16 (the 256-row-tile MFMA kernels, all the library had for them), each pass over the
      weights of ALL layers so that nothing is served from the 256 MiB cache.
Every time is printed next to its floor: the bytes of the weights it must stream over 8 TB/s.  Times are host-clock intervals
around work that ends in a synchronise, medians of `--iters` runs after one warm-up run.  The stub processor of the tests stands
in for the checkpoint's (token ids below 512: any row of the embedding is as good as another for a time).  bench.py never sees
this stage."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

HBM_BYTES_PER_S = 8.0e12
PROMPT = "<|im_start|>user\n<|vision_start|><|image_pad|><|vision_end|>describe the picture<|im_end|>\n<|im_start|>assistant\n"


class _Processor:
    """The tests' stub processor plus a `batch_decode`."""

    def __init__(self):
        import vl_stubs as V

        self.stub = V.StubVLProcessor(min_pixels=56 * 56, max_pixels=(14 * 32) ** 2)
        self.image_processor = self.stub.image_processor

    def __call__(self, *a, **k):
        return self.stub(*a, **k)

    def batch_decode(self, rows, skip_special_tokens=True, clean_up_tokenization_spaces=False):
        return [" ".join(str(int(t)) for t in row) for row in rows]


def wall(fn, iters: int) -> list[float]:
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--skip-hf", action="store_true", help="do not time HF generate")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "captioner_first_measurement.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_captioner: no GPU - nothing is measured without one", file=sys.stderr)
        return 2

    import numpy as np
    from PIL import Image
    from transformers import GenerationConfig, Qwen2_5_VLConfig, Qwen2_5_VLForConditionalGeneration

    from vllm_omni_amd import ops
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import NativeQwenCaptioner

    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = Qwen2_5_VLConfig(
        text_config=dict(vocab_size=152064, hidden_size=3584, num_hidden_layers=args.layers, num_attention_heads=28,
                         num_key_value_heads=4, intermediate_size=18944, max_position_embeddings=8192, bos_token_id=1,
                         eos_token_id=2, pad_token_id=0, tie_word_embeddings=False,
                         rope_scaling={"type": "default", "mrope_section": [16, 24, 24], "rope_type": "default"}),
        vision_config=dict(depth=32, hidden_size=1280, out_hidden_size=3584, num_heads=16, intermediate_size=3420, window_size=112,
                           fullatt_block_indexes=[7, 15, 23, 31], patch_size=14, spatial_merge_size=2, temporal_patch_size=2,
                           in_channels=3),
        image_token_id=500, video_token_id=499, vision_start_token_id=501, vision_end_token_id=502)
    torch.manual_seed(0)
    with torch.device(dev):
        model = Qwen2_5_VLForConditionalGeneration(cfg).to(torch.bfloat16).eval()
    # the rotary frequencies in fp32, as a checkpoint load leaves them
    lm = model.model.language_model
    lm.rotary_emb.inv_freq = 1.0 / (1e6 ** (torch.arange(0, 128, 2, dtype=torch.int64, device=dev).float() / 128))
    gen = GenerationConfig(do_sample=False, repetition_penalty=1.05, eos_token_id=None, pad_token_id=0)
    model.generation_config = gen
    proc = _Processor()
    pic = Image.fromarray(np.random.RandomState(3).randint(0, 256, size=(14 * 24, 14 * 32, 3), dtype=np.uint8))
    cap = NativeQwenCaptioner.from_hf(model, proc)
    T = args.tokens

    layer_bytes = sum(t.numel() * t.element_size() for n, t in cap.encoder.text.layers[0].items() if n.endswith("_w") and t.dim() == 2)
    head_bytes = cap.lm_head.numel() * 2
    step_bytes = layer_bytes * args.layers + head_bytes
    floor_ms = step_bytes / HBM_BYTES_PER_S * 1e3
    lines = [f"auto-caption, HF generate vs native captioner; {torch.cuda.get_device_name(dev)}",
             f"geometry: hidden 3584, 28 / 4 heads of 128, intermediate 18944, {args.layers} layers, lm_head 152064 x 3584, "
             f"vision tower 32 x 1280; random weights; one picture of 24 x 32 patches",
             f"one decoded token streams {step_bytes / 1e9:.2f} GB ({args.layers} x {layer_bytes / 1e6:.0f} MB + lm_head "
             f"{head_bytes / 1e9:.2f} GB) -> floor {floor_ms:.2f} ms at 8 TB/s, {floor_ms * T / 1e3:.2f} s per {T} tokens",
             f"host clock around work ending in a synchronise; median of {args.iters} after one warm-up", ""]

    # ---- (a) captions
    inputs = proc(text=[PROMPT], images=pic, padding=True, return_tensors="pt").to(dev)
    P = int(inputs.input_ids.shape[1])
    state = {}

    def native_prefill():
        state["p"] = cap.prefill(PROMPT, pic, max_new_tokens=T)

    def native_decode():
        w, st, _ = state["p"]
        ops.qwen2_text_decode_step(w, st, T - 1)

    cap.generate_ids(PROMPT, pic, max_new_tokens=T)                    # warm-up (and the vision result is cached from here on)
    t_pre = statistics.median(wall(native_prefill, args.iters))
    t_dec = statistics.median(wall(native_decode, args.iters))
    t_all = statistics.median(wall(lambda: cap.generate_ids(PROMPT, pic, max_new_tokens=T), args.iters))
    cap.encoder._vision_cache = None
    t_cold = statistics.median(wall(lambda: (setattr(cap.encoder, "_vision_cache", None),
                                             cap.generate_ids(PROMPT, pic, max_new_tokens=T)), args.iters))
    n_pic = int((inputs.input_ids == cfg.image_token_id).sum())
    lines += [f"(a) prompt of {P} tokens ({n_pic} of them the picture), {T} new tokens",
              f"  native  caption {t_cold:7.3f} s with the vision tower, {t_all:7.3f} s with its result cached "
              f"(steps in chunks of 16, one read of the stop flags between chunks)",
              f"          prefill {t_pre * 1e3:8.2f} ms;  {T - 1} decode steps queued back to back {t_dec:7.3f} s = "
              f"{t_dec / (T - 1) * 1e3:6.3f} ms per token = {t_dec / (T - 1) * 1e3 / floor_ms:5.2f} x floor"]
    if not args.skip_hf:
        def hf_generate(n):
            with torch.no_grad():
                return model.generate(**{k: v for k, v in inputs.__dict__.items()}, max_new_tokens=n, min_new_tokens=n, generation_config=gen)

        hf_generate(8)
        t_hf = statistics.median(wall(lambda: hf_generate(T), max(1, args.iters - 1)))
        t_hf1 = statistics.median(wall(lambda: hf_generate(1), max(1, args.iters - 1)))
        per = (t_hf - t_hf1) / (T - 1) * 1e3
        lines += [f"  hf      caption {t_hf:7.3f} s (vision tower + prefill + first token {t_hf1 * 1e3:8.2f} ms);  {per:6.3f} ms per "
                  f"further token = {per / floor_ms:5.2f} x floor",
                  f"  native / hf = {t_cold / t_hf:.3f} per caption, {t_dec / (T - 1) * 1e3 / per:.3f} per decoded token"]
    lines.append("")

    # ---- (b) the GEMV alone, M = 1, over the weights of all layers
    enc = cap.encoder.text
    D, I, Nqkv = 3584, 18944, 4608
    x_d = torch.randn(1, D, device=dev).to(torch.bfloat16)
    x_i = torch.randn(1, I, device=dev).to(torch.bfloat16)
    classes = [("q|k|v", "qkv_w", Nqkv, D, x_d), ("o", "o_w", D, D, x_d), ("gate|up", "gate_up_w", 2 * I, D, x_d), ("down", "down_w", D, I, x_i)]
    lines.append(f"(b) the M = 1 products of one step, each class over all {args.layers} layers (K32-blocked weights), lm_head row-major")
    tot = {"gemv": 0.0, "gemm": 0.0, "floor": 0.0}

    def measure(name, mats, N, K, x, blocked):
        out = torch.empty(1, N, dtype=torch.bfloat16, device=dev)

        def gemv():
            for wt in mats:
                ops.gemv_bf16(x, wt, out=out, w_k32_blocked=blocked)

        def gemm():
            for wt in mats:
                ops.gemm([ops.GemmGroupArgs(x, wt, None, out)], w_k32_blocked=blocked)

        gemv(), gemm()
        a = statistics.median(wall(gemv, args.iters + 2)) * 1e3
        b = statistics.median(wall(gemm, args.iters + 2)) * 1e3
        fl = len(mats) * N * K * 2 / HBM_BYTES_PER_S * 1e3
        tot["gemv"] += a
        tot["gemm"] += b
        tot["floor"] += fl
        lines.append(f"  {name:8s} N {N:6d} K {K:5d} x {len(mats):2d}: omni_gemv_bf16 {a:8.3f} ms ({a / fl:5.2f} x floor {fl:6.3f} ms)   "
                     f"omni_gemm_bf16 {b:8.3f} ms ({b / fl:5.2f} x floor)   gemv / gemm = {a / b:.3f}")

    for name, key, N, K, x in classes:
        measure(name, [L[key] for L in enc.layers], N, K, x, True)
    measure("lm_head", [cap.lm_head], 152064, D, x_d, False)
    lines.append(f"  one step's products: omni_gemv_bf16 {tot['gemv']:.3f} ms, omni_gemm_bf16 {tot['gemm']:.3f} ms, floor {tot['floor']:.3f} ms")
    lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
