#!/usr/bin/env python3
"""Mixed-resolution step batching (`OmniDiffusionConfig.mixed_step_batch`) against one-key-per-forward serving, same process,
same weights, interleaved repeats.  Two workloads of 20-step true-CFG text-to-image requests submitted together to one
ContinuousStepBatcher (random weights, latents out, no VAE):

    A  aspect-ratio mix: 1328x1328, 1664x928, 928x1664, 1584x1056
    B  small next to large: 2 x 1328x1328 + 3 x 512x512

Prints, per workload and setting, the wall time of every repeat (host clock around submit .. drain .. device idle) and the
number of DiT forwards, and next to it the device time inside the steps (the batcher's own HIP events around every whole step,
`ContinuousStepBatcher.stats()`).  Both settings run in THIS build: with the option off the pipeline takes the code path it had
before the option existed (uniform serve states, one fused CFG + Euler launch).

    python tools/bench_mixed_batch.py [--layers 60] [--steps 20] [--repeats 3]

With `--teacache THRESH` the DiT runs with TeaCache at that threshold and the two settings become: `mixed_step_batch` alone
(TeaCache keeps the grid in the batch key: what serving did before `mixed_step_batch_teacache` existed) against both flags on.
Workload B is timed, and as a control the equal-grid case C (five 1024x1024 requests), which never forms a mixed group: its
time is the cost of the TeaCache kernels reading per-item row ranges.  `--lib PATH` loads another build of libomni_cdna4.so
(same-box A/B of the control against the library of another commit).  Images/s and the skipped forwards per request are
printed next to the times.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from vllm_omni_amd.diffusion.data import OmniDiffusionConfig  # noqa: E402
from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline  # noqa: E402
from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel  # noqa: E402
from vllm_omni_amd.diffusion.request import OmniDiffusionRequest  # noqa: E402
from vllm_omni_amd.diffusion.step_batcher import ContinuousStepBatcher  # noqa: E402

WORKLOADS = {
    "A aspect-ratio mix": [(1328, 1328), (928, 1664), (1664, 928), (1056, 1584)],          # (height, width)
    "B small next to large": [(1328, 1328), (1328, 1328), (512, 512), (512, 512), (512, 512)],
}
TEACACHE_WORKLOADS = {
    "B small next to large": WORKLOADS["B small next to large"],
    "C equal grid (control)": [(1024, 1024)] * 5,
}
DEV = "cuda:0"


def requests(sizes, steps):
    g = torch.Generator(device=DEV).manual_seed(1)
    out = []
    for i, (h, w) in enumerate(sizes):
        S = (h // 16) * (w // 16)
        rnd = lambda *s: torch.randn(*s, device=DEV, generator=g).bfloat16()  # noqa: E731
        out.append(OmniDiffusionRequest(height=h, width=w, num_inference_steps=steps, true_cfg_scale=4.0, latents=rnd(1, S, 64),
                                        prompt_embeds=rnd(1, 40 + 17 * i, 3584), negative_prompt_embeds=rnd(1, 12 + 5 * i, 3584),
                                        output_type="latent"))
    return out


def run(pipe, tr, reqs):
    calls, orig = [0], tr.forward_ragged

    def counted(*a, **k):
        calls[0] += 1
        return orig(*a, **k)

    tr.forward_ragged = counted
    try:
        b = ContinuousStepBatcher(pipe)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, r in enumerate(reqs):
            b.add(r, i)
        done = b.drain()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        busy = b.stats()["busy_s"]
    finally:
        tr.forward_ragged = orig
    assert len(done) == len(reqs) and all(o.error is None for _, o in done), [o.error for _, o in done]
    return dt, calls[0], busy


def run_teacache(pipe, tr, reqs):
    """`run`, plus the skipped forwards of every request's (positive, negative) branch, read after the loop."""
    skipped, orig = {}, pipe._export_sample

    def export(a):
        orig(a)
        if a.state.get("tc"):
            skipped[a.tag] = tuple(int(x["skip_total"][0]) for x in a.state["tc"])

    pipe._export_sample = export
    try:
        dt, calls, busy = run(pipe, tr, reqs)
    finally:
        del pipe._export_sample
    return dt, calls, busy, [skipped.get(i) for i in range(len(reqs))]


def main_teacache(a):
    from vllm_omni_amd import _native as N
    from vllm_omni_amd.diffusion.cache.teacache.config import TeaCacheConfig

    if a.lib:
        N.LIB_PATH = os.path.abspath(a.lib)
    print(f"library {N.LIB_PATH}: features {N.features():#x}; TeaCache rel_l1_thresh {a.teacache}, {a.layers} layers, {a.steps} steps", flush=True)
    tr = QwenImageTransformer2DModel(num_layers=a.layers, device=DEV).init_random_(seed=1)
    tr.teacache = TeaCacheConfig(rel_l1_thresh=a.teacache)
    cfgs = {"grid in key": dict(mixed_step_batch=True)}
    if N.features() & N.FEATURE_TEACACHE_RAGGED:
        cfgs["both flags"] = dict(mixed_step_batch=True, mixed_step_batch_teacache=True)
    pipes = {k: QwenImagePipeline(od_config=OmniDiffusionConfig(max_step_batch=5, **c), device=DEV, transformer=tr) for k, c in cfgs.items()}
    for name, sizes in TEACACHE_WORKLOADS.items():
        if a.only and not name.startswith(a.only):
            continue
        reqs = requests(sizes, a.steps)
        for p in pipes.values():
            run(p, tr, requests(sizes, 2))
        times, fwd, skips = {k: [] for k in pipes}, {}, {}
        for _ in range(a.repeats):
            for k, p in pipes.items():
                dt, fwd[k], _, skips[k] = run_teacache(p, tr, reqs)
                times[k].append(dt)
        for k in pipes:
            t = times[k]
            print(f"{name} | {k}: {fwd[k]} forwards, wall s per repeat {' '.join(f'{x:.3f}' for x in t)} (median "
                  f"{statistics.median(t):.3f}, spread {max(t) - min(t):.3f}) = {len(reqs) / statistics.median(t):.3f} images/s; "
                  f"skipped forwards per request (pos, neg) {skips[k]}", flush=True)
        if len(pipes) == 2:
            print(f"{name} | both flags / grid in key (medians) = "
                  f"{statistics.median(times['both flags']) / statistics.median(times['grid in key']):.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--teacache", type=float, default=None, metavar="THRESH")
    ap.add_argument("--lib", default=None, help="another build of libomni_cdna4.so (with --teacache)")
    ap.add_argument("--only", default=None, help="with --teacache: the workload whose name starts with this (B or C)")
    a = ap.parse_args()
    if a.teacache is not None:
        return main_teacache(a)
    tr = QwenImageTransformer2DModel(num_layers=a.layers, device=DEV).init_random_(seed=1)
    pipes = {"flag off": QwenImagePipeline(od_config=OmniDiffusionConfig(max_step_batch=5), device=DEV, transformer=tr),
             "flag on": QwenImagePipeline(od_config=OmniDiffusionConfig(max_step_batch=5, mixed_step_batch=True), device=DEV,
                                          transformer=tr)}
    for name, sizes in WORKLOADS.items():
        reqs = requests(sizes, a.steps)
        for p in pipes.values():                             # warm-up: buffers, modulation tables, lazy library state
            run(p, tr, requests(sizes, 2))
        times = {k: [] for k in pipes}
        busy = {k: [] for k in pipes}
        fwd = {}
        for _ in range(a.repeats):
            for k, p in pipes.items():                       # interleaved: both settings see the same clocks / thermal state
                dt, fwd[k], bs = run(p, tr, reqs)
                times[k].append(dt)
                busy[k].append(bs)
        for k in pipes:
            t = times[k]
            print(f"{name} | {k}: {fwd[k]} forwards, wall s per repeat {' '.join(f'{x:.3f}' for x in t)} "
                  f"(median {statistics.median(t):.3f}, spread {max(t) - min(t):.3f}); device s inside steps (HIP events) "
                  f"{' '.join(f'{x:.3f}' for x in busy[k])}", flush=True)
        print(f"{name} | flag on / flag off (medians) = "
              f"{statistics.median(times['flag on']) / statistics.median(times['flag off']):.3f}", flush=True)


if __name__ == "__main__":
    main()
