#!/usr/bin/env python3
"""Dev tool (GPU): `omni_flash_attn_general` in fp16 against the same kernel in bf16, in ONE process on one device.

    python tools/attn_fp16_ab.py [--repeats 9] [--iters 10] [--out FILE]

The yardstick is the bf16 general kernel (the instances that did not change when the kernel was templated on the element
type).  Per shape: warm-up of both, then `repeats` rounds that alternate bf16 / fp16, each timing `iters` back-to-back launches
between two HIP events; reported are the medians, the bf16 kernel's own run-to-run spread ((max - min) / median over its repeats)
and the fp16 / bf16 ratio of medians.  The acceptance margin for "parity" is that spread, not a constant.  For information the
tuned bf16 self-attention kernels (omni_flash_attn_fwd) are timed on the Qwen-Image shape: what fp16 self-attention gives up by
running on the general kernel.  Also prints the flat-tail result (does a P below fp16's smallest normal number survive the fp16
MFMA?) so that the measurement file holds both findings.
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tools.devlib  # noqa: E402,F401
from vllm_omni_amd import _native as N  # noqa: E402
from vllm_omni_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("attn_fp16_ab.py measures on the GPU; there is none here")
dev = torch.device("cuda:0")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3            # us per call


def ab(name, B, Sq, Sk, H, dh, tuned=False):
    g = torch.Generator(device=dev).manual_seed(0)
    x = {n: torch.randn(B * s, H * dh, device=dev, generator=g) for n, s in (("q", Sq), ("k", Sk), ("v", Sk))}
    cq = (torch.arange(B + 1, dtype=torch.int32) * Sq).to(dev)
    ck = (torch.arange(B + 1, dtype=torch.int32) * Sk).to(dev)
    scale = 1 / math.sqrt(dh)
    fns = {}
    for label, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        q, k, v = (x[n].to(dt) for n in "qkv")
        out = torch.empty_like(q)
        fns[label] = (lambda q=q, k=k, v=v, out=out: ops.flash_attn_general(q, k, v, cq, ck, H, H, Sq, Sk, scale, out=out))
    if tuned:
        q, k, v = (x[n].to(torch.bfloat16) for n in "qkv")
        out = torch.empty_like(q)
        fns["tuned bf16"] = (lambda q=q, k=k, v=v, out=out: ops.flash_attn_varlen(q, k, v, cq, H, Sq, scale, out=out))
    for fn in fns.values():                          # warm-up: code objects, clocks
        window(fn, 3)
    t = {label: [] for label in fns}
    for _ in range(args.repeats):                    # interleaved: A B (C) A B (C) ...
        for label, fn in fns.items():
            t[label].append(window(fn, args.iters))
    flop = 4.0 * B * H * Sq * Sk * dh
    med = {label: statistics.median(v) for label, v in t.items()}
    spread = {label: (max(v) - min(v)) / med[label] for label, v in t.items()}
    say(f"{name}: B {B} S_q {Sq} S_k {Sk} H {H} dh {dh}  ({args.repeats} interleaved repeats x {args.iters} launches)")
    for label in fns:
        say(f"    {label:11s} median {med[label]:9.1f} us  min {min(t[label]):9.1f}  max {max(t[label]):9.1f}  spread {spread[label] * 100:5.2f} %"
            f"  {flop / med[label] / 1e6:7.1f} TF/s")
    ratio = med["fp16"] / med["bf16"]
    verdict = "within" if abs(ratio - 1) <= spread["bf16"] else ("FASTER than" if ratio < 1 else "SLOWER than")
    say(f"    fp16 / bf16 = {ratio:.4f}: {verdict} the bf16 kernel's own spread ({spread['bf16'] * 100:.2f} %)")
    if tuned:
        say(f"    general fp16 / tuned bf16 = {med['fp16'] / med['tuned bf16']:.3f} (what fp16 self-attention gives up on this shape)")
    say()


def flat_tail(dh):
    """One dominant key, 4095 keys 10..13 nats below it (every tail P below 6.1e-5); V channel 0 = 1 on the tail, 0 at the
    dominant key: output channel 0 is the tail's share of the softmax mass."""
    Sq, Sk, H = 64, 4096, 2
    scale = 1 / math.sqrt(dh)
    gen = torch.Generator().manual_seed(31)
    q = torch.zeros(Sq, H, dh)
    q[..., 0] = 1 / scale
    k = torch.zeros(Sk, H, dh)
    k[..., 0] = torch.rand(Sk, H, generator=gen) * 3.0
    k[1000, :, 0] = 13.0
    v = torch.zeros(Sk, H, dh)
    v[..., 0] = 1.0
    v[1000, :, 0] = 0.0
    cq = torch.tensor([0, Sq], dtype=torch.int32, device=dev)
    ck = torch.tensor([0, Sk], dtype=torch.int32, device=dev)
    res = {}
    for label, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        qd, kd, vd = (t.to(dt) for t in (q, k, v))
        logits = (qd.float()[0, 0, 0] * scale) * kd.float()[:, 0, 0].double()
        w = torch.softmax(logits, 0)
        want = float(w.sum() - w[1000])
        got = ops.flash_attn_general(qd.reshape(Sq, H * dh).to(dev), kd.reshape(Sk, H * dh).to(dev), vd.reshape(Sk, H * dh).to(dev),
                                     cq, ck, H, H, Sq, Sk, scale)
        torch.cuda.synchronize()
        res[label] = (want, float(got[0, 0]))
    say(f"flat tail dh {dh}: tail share of the softmax mass   " +
        "   ".join(f"{label}: exact {w_:.5f} kernel {g_:.5f}" for label, (w_, g_) in res.items()))


say(f"library {N.LIB_PATH}  features {N.features():#x}  device {torch.cuda.get_device_name(0)}")
say()
ab("Qwen-Image joint self-attention, 10 items", 10, 4160, 4160, 24, 128, tuned=True)
ab("sd3 joint self-attention (head size 64)", 1, 4250, 4250, 24, 64)
ab("wan2.2 cross-attention (512 text keys)", 1, 32760, 512, 40, 128)
flat_tail(64)
flat_tail(128)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
