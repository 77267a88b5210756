#!/usr/bin/env python3
"""SAGE_ATTN (int8 Q K^T, csrc/attention_sage.hip: quantisation pass + sage_attn_fwd_kernel) against the bf16 joint-attention
kernel of the DiT hot path (omni_flash_attn_fwd_ws: flash_attn_fwd_w64_kernel) at the Qwen-Image shapes, interleaved in one
process.  Prints one line per shape: median ms of each and the ratio.

    python tools/bench_sage_attn.py [--iters 20]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from vllm_omni_amd import ops  # noqa: E402

SHAPES = [("1024^2 x10 (R=5 CFG)", 4160, 10), ("2048^2 CFG pair", 16448, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev, H, dh = "cuda:0", 24, 128
    for name, S, B in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        q, k, v = (torch.randn(B * S, H * dh, device=dev, generator=g).bfloat16() for _ in range(3))
        cu = torch.arange(B + 1, dtype=torch.int32, device=dev) * S
        sc = dh ** -0.5
        ws_bf16 = torch.empty(ops.flash_attn_workspace_floats(B, H), dtype=torch.float32, device=dev)
        ws_int8 = torch.empty(ops.attn_quant_workspace_bytes(B, H, H, dh, S, S), dtype=torch.uint8, device=dev)
        out = torch.empty_like(q)
        runs = {
            "bf16_w64": lambda: ops.flash_attn_varlen(q, k, v, cu, H, S, sc, out=out, workspace=ws_bf16),
            "int8_sage": lambda: ops.flash_attn_general(q, k, v, cu, cu, H, H, S, S, sc, out=out, qk_int8=True, workspace=ws_int8),
        }
        times = {n: [] for n in runs}
        for f in runs.values():
            f()
        torch.cuda.synchronize()
        for _ in range(a.iters):
            for n, f in runs.items():                # interleaved: both see the same clocks / thermal state
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                times[n].append(e0.elapsed_time(e1))
        med = {n: statistics.median(t) for n, t in times.items()}
        flop = 4.0 * B * H * S * S * dh
        print(f"{name}: bf16 w64 {med['bf16_w64']:.3f} ms ({flop / med['bf16_w64'] / 1e9:.0f} TF/s)  int8 sage (quant + attention) "
              f"{med['int8_sage']:.3f} ms ({flop / med['int8_sage'] / 1e9:.0f} TF/s)  bf16/int8 = "
              f"{med['bf16_w64'] / med['int8_sage']:.3f}", flush=True)


if __name__ == "__main__":
    main()
