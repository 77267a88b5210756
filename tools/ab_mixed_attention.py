#!/usr/bin/env python3
"""A/B of the native library on ragged forwards whose items differ in length: the compact attention grid (csrc/common.h
omni_attn_compact_slots) against a library without it, driven by the SAME host code — the C-ABI and omni_dit_batch are the same.

    python tools/ab_mixed_attention.py [--lib /path/to/other/libomni_cdna4.so] [--iters 20] [--shapes mixed_B,bench]

Per shape: median ms of a 2-layer full-width forward (HIP events, warmed) and the sha256 of its output — two libraries that differ
only in which workgroup runs a q-block print the same digest.  Run it under `rocprofv3 --kernel-trace --stats -- python ...` for
the per-launch attention time."""
import argparse
import hashlib
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

G1328, G1664, G512, G1024, G256 = (1, 83, 83), (1, 58, 104), (1, 32, 32), (1, 64, 64), (1, 16, 16)
SHAPES = {   # name: (per-item grids, per-item prompt lengths, temb rows)
    "mixed_B": ([G1328, G1328, G512, G512, G512] * 2, [64, 81, 98, 115, 132, 12, 17, 22, 27, 32], list(range(5)) * 2),
    "mixed_3": ([G1328, G1664, G512] * 2, [64, 290, 20, 11, 37, 5], list(range(3)) * 2),
    "bench_10x4160": ([G1024] * 10, [64] * 10, list(range(5)) * 2),
    "cfg_pair_256": ([G256] * 2, [11, 5], [0, 0]),
    "one_grid_T20_T700": ([G1024] * 2, [20, 700], [0, 0]),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    from vllm_omni_amd import _native

    if a.lib:
        _native.LIB_PATH = os.path.abspath(a.lib)
    import torch

    from vllm_omni_amd.diffusion.batch import attention_compact_slots, build_ragged_batch
    from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel

    dev = "cuda:0"
    m = QwenImageTransformer2DModel(num_layers=2, device=dev).init_random_(seed=1)
    print(f"library: {_native.LIB_PATH}", flush=True)
    for name in a.shapes.split(","):
        grids, lens, temb = SHAPES[name]
        rb = build_ragged_batch(lens, list(grids), temb_rows=temb)
        prep = m.prepare_batch(rb)
        g = torch.Generator(device=dev).manual_seed(3)
        lat = torch.randn(rb.n_img_rows, 64, device=dev, generator=g).bfloat16()
        txt = torch.randn(rb.n_txt_rows, 3584, device=dev, generator=g).bfloat16()
        sig = torch.linspace(0.2, 0.9, rb.n_temb, device=dev).bfloat16().float()
        out = torch.empty(rb.n_img_rows, 64, dtype=torch.bfloat16, device=dev)
        for _ in range(3):
            m.forward_ragged(prep, lat, txt, sig, out=out)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            m.forward_ragged(prep, lat, txt, sig, out=out)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        seq = [t + s for t, s in zip(rb.txt_lens, rb.s_imgs)]
        digest = hashlib.sha256(out.cpu().view(torch.int16).numpy().tobytes()).hexdigest()[:16]
        print(f"{name}: {rb.n_items} items, {rb.n_joint_rows} joint rows, compact slots/head at Q=256: "
              f"{attention_compact_slots(seq, 256)} (legacy {rb.n_items * -(-max(seq) // 256)}) | forward median "
              f"{statistics.median(ts):.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}) | sha256 {digest}", flush=True)


if __name__ == "__main__":
    main()
