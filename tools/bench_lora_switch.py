#!/usr/bin/env python3
"""What a LoRA adapter costs on the serving path: one ACTIVATION (every `omni_lora_merge` launch of a switch) against the traffic
floor, and a forward with an adapter active against a forward with none.

    python tools/bench_lora_switch.py [--layers 60] [--rank 64] [--repeats 3] [--out profiles/lora_merge_first_measurement.txt]

Setup: full-width DiT (random weights), a rank-`--rank` adapter on all twelve linears of every layer.
  1. activation: HIP events around `set_lora_adapters([name]); _native_weights()` with `max_resident_loras = 1` and two adapters
     activated alternately, so every activation merges; `--repeats` repeats.  The yardstick on the same box: a plain
     device-to-device copy of the same matrices (read once + write once - what the merge must move at least).  Both and their ratio.
  2. forward at the bench shape (1024^2, CFG pair) and at 256^2: adapter active against none, interleaved repeats; the launches are
     the same, so the expectation is "within the run-to-run spread of the no-adapter repeats" - that spread is printed next to
     the difference.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from vllm_omni_amd.diffusion.batch import build_ragged_batch  # noqa: E402
from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel  # noqa: E402

DEV = "cuda:0"
BF16 = torch.bfloat16


def adapter(model, rank, seed):
    g = torch.Generator().manual_seed(seed)
    t = {}
    for mod, (n, k, _blocked) in model.lora_targets.items():
        if not mod.startswith("transformer_blocks."):
            continue
        t[mod + ".lora_A.weight"] = (torch.randn(rank, k, generator=g) * 0.01).to(BF16)
        t[mod + ".lora_B.weight"] = (torch.randn(n, rank, generator=g) * 0.01).to(BF16)
    return t


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    m = QwenImageTransformer2DModel(num_layers=a.layers, device=DEV).init_random_(seed=1)
    m.load_lora_adapter("a", adapter(m, a.rank, 1))
    m.load_lora_adapter("b", adapter(m, a.rank, 2))
    m._native_weights()
    params = dict(m.named_parameters())
    mats = [params[mod + ".weight"].data for mod in m.lora_targets if mod.startswith("transformer_blocks.")]
    gb = sum(t.numel() * 2 for t in mats) / 1e9
    say(f"# LoRA switch: {a.layers} layers, rank {a.rank}, {len(mats)} targeted matrices, {gb:.2f} GB of weights "
        f"({torch.cuda.get_device_name(0)})")

    def activate(name):
        m.set_lora_adapters([name])
        m._native_weights()

    outs = [torch.empty_like(t) for t in mats]         # allocated once: the yardstick times the copies, not the allocator

    def copy_all():
        for o, t in zip(outs, mats):
            o.copy_(t)

    activate("a")
    copy_all()                                         # warm-up of both (allocator, code objects)
    t_merge, t_copy = [], []
    for i in range(a.repeats):
        t_merge.append(timed(lambda: activate("b" if i % 2 == 0 else "a")))
        t_copy.append(timed(copy_all))
    del outs
    for i, (tm, tc) in enumerate(zip(t_merge, t_copy)):
        say(f"repeat {i}: activation {tm:8.2f} ms ({2 * gb / tm:6.2f} TB/s of read + write)   "
            f"device-to-device copy {tc:8.2f} ms   ratio {tm / tc:.2f}")
    say(f"median: activation {statistics.median(t_merge):.2f} ms, copy {statistics.median(t_copy):.2f} ms, "
        f"ratio {statistics.median(t_merge) / statistics.median(t_copy):.2f}")

    for label, hw, items in (("bench shape 1024^2, CFG pair", 1024, 2), ("256^2, CFG pair", 256, 2)):
        S = (hw // 16) ** 2
        g = torch.Generator(device=DEV).manual_seed(3)
        lat = torch.randn(items * S, 64, device=DEV, generator=g).bfloat16()
        lens = [40, 12][:items]
        txt = torch.randn(sum(lens), m.joint_attention_dim, device=DEV, generator=g).bfloat16()
        sig = torch.full((1,), 0.6, device=DEV)
        prepared = m.prepare_batch(build_ragged_batch(lens, (1, hw // 16, hw // 16), temb_rows=[0] * items))
        fwd = lambda: m.forward_ragged(prepared, lat, txt, sig)  # noqa: E731
        res = {"none": [], "adapter": []}
        for _ in range(a.repeats):
            for key, names in (("none", []), ("adapter", ["a"])):
                m.set_lora_adapters(names)
                fwd()                                      # the switch (and its merge) stays outside the timed forward
                res[key].append(min(timed(fwd) for _ in range(3)))
        none, ad = res["none"], res["adapter"]
        say(f"forward, {label}: none {['%.3f' % v for v in none]} ms, adapter {['%.3f' % v for v in ad]} ms; "
            f"difference of medians {statistics.median(ad) - statistics.median(none):+.3f} ms, "
            f"spread of the no-adapter repeats {max(none) - min(none):.3f} ms")
    m.set_lora_adapters([])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
