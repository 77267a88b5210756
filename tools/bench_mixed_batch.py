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

With `--edit` the workload is Edit traffic: three Edit requests near 1024^2 with different aspect ratios (1024x1024, 1376x768,
896x1184; each carries the condition rows of a picture of its own size), true-CFG with different scales.  Settings:
`mixed_step_batch` alone (a sample with condition rows keeps its grid in the key: one request per forward, what serving did
before `mixed_step_batch_edit`), run TWICE per repeat to state the spread of that box, against both flags on.  Then the step
update alone: one launch of the ragged CFG + Euler kernel against the R per-request launches and the 2R + 1 copies it
replaces, on the same buffers (HIP events around 200 iterations).
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


EDIT_SIZES = [(1024, 1024, 4.0), (768, 1376, 2.5), (1184, 896, 3.0)]            # (height, width, true_cfg_scale)


def edit_requests(steps):
    g = torch.Generator(device=DEV).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g).bfloat16()  # noqa: E731
    out = []
    for i, (h, w, cfg) in enumerate(EDIT_SIZES):
        S = (h // 16) * (w // 16)
        out.append(OmniDiffusionRequest(height=h, width=w, num_inference_steps=steps, true_cfg_scale=cfg, latents=rnd(1, S, 64),
                                        prompt_embeds=rnd(1, 200 + 17 * i, 3584), negative_prompt_embeds=rnd(1, 180 + 5 * i, 3584),
                                        output_type="latent",
                                        extra={"image_latents": rnd(S, 64), "image_latent_grid": (h // 16, w // 16)}))
    return out


def time_step_update(iters=200):
    """One ragged launch against what it replaces, for the three Edit requests as a CFG pair group."""
    from vllm_omni_amd import ops
    from vllm_omni_amd.diffusion.batch import ragged_step_descriptors

    S = [(h // 16) * (w // 16) for h, w, _ in EDIT_SIZES]
    R, scales = len(S), [c for _, _, c in EDIT_SIZES]
    lay = ragged_step_descriptors(S, S, True, scales)
    lo, io, n_lat = lay["lat_off"], lay["item_off"], lay["total_rows"]
    g = torch.Generator(device=DEV).manual_seed(2)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g).bfloat16()  # noqa: E731
    lat, pred, lat_in = rnd(n_lat, 64), rnd(io[-1], 64), rnd(io[-1], 64)
    pred_c = torch.empty(2 * n_lat, 64, dtype=torch.bfloat16, device=DEV)
    dt = torch.full((R,), -1e-4, device=DEV)
    reqs = torch.from_numpy(lay["reqs"].view("<i4").reshape(R, 8).copy()).to(DEV)

    def ragged():
        ops.cfg_euler_step_ragged_(lat, pred, lat_in, reqs, R, n_lat, dt)

    def replaced():                                          # 2R copies lat -> lat_in, 2R copies pred -> pred_c, R launches
        for r in range(R):
            for i in (r, R + r):
                lat_in[io[i]:io[i] + S[r]].copy_(lat[lo[r]:lo[r + 1]])
                pred_c[(i // R) * n_lat + lo[r]:(i // R) * n_lat + lo[r + 1]].copy_(pred[io[i]:io[i] + S[r]])
        for r in range(R):
            ops.cfg_euler_step_(lat[lo[r]:lo[r + 1]], pred_c[lo[r]:lo[r + 1]], pred_c[n_lat + lo[r]:n_lat + lo[r + 1]], scales[r],
                                dt[r:r + 1], dt_rows_per_item=0)

    out = {}
    for name, fn in (("ragged kernel, 1 launch", ragged), (f"replaced: {4 * R} copies + {R} launches", replaced)):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        rep = []
        for _ in range(3):
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            rep.append(e0.elapsed_time(e1) * 1e3 / iters)
        out[name] = rep
        print(f"step update of {S} rows + as many condition rows, CFG pairs | {name}: us per step "
              f"{' '.join(f'{x:.1f}' for x in rep)}", flush=True)
    return out


def main_edit(a):
    from vllm_omni_amd.diffusion.models.qwen_image.autoencoder_kl_qwenimage import AutoencoderKLQwenImage
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image_edit import QwenImageEditPipeline

    print(f"Edit workload {EDIT_SIZES}: {a.layers} layers, {a.steps} steps, true-CFG", flush=True)
    tr = QwenImageTransformer2DModel(num_layers=a.layers, device=DEV).init_random_(seed=1)
    vae = AutoencoderKLQwenImage(device=DEV, with_encoder=True)
    mk = lambda **c: QwenImageEditPipeline(od_config=OmniDiffusionConfig(max_step_batch=5, mixed_step_batch=True, **c),  # noqa: E731
                                           device=DEV, transformer=tr, vae=vae)
    pipes = {"flag off": mk(), "flag off again": mk(), "flag on": mk(mixed_step_batch_edit=True)}
    for p in pipes.values():
        run(p, tr, edit_requests(2))
    reqs = edit_requests(a.steps)
    times, busy, fwd = {k: [] for k in pipes}, {k: [] for k in pipes}, {}
    for _ in range(a.repeats):
        for k, p in pipes.items():
            dt, fwd[k], bs = run(p, tr, reqs)
            times[k].append(dt)
            busy[k].append(bs)
    for k in pipes:
        t = times[k]
        print(f"Edit x3 | {k}: {fwd[k]} forwards, wall s per repeat {' '.join(f'{x:.3f}' for x in t)} (median "
              f"{statistics.median(t):.3f}, spread {max(t) - min(t):.3f}) = {statistics.median(t) / a.steps * 1e3:.1f} ms per step of "
              f"three requests; device s inside steps {' '.join(f'{x:.3f}' for x in busy[k])}", flush=True)
    off = statistics.median(times["flag off"] + times["flag off again"])
    print(f"Edit x3 | flag on / flag off (medians) = {statistics.median(times['flag on']) / off:.3f}; flag off again / flag off = "
          f"{statistics.median(times['flag off again']) / statistics.median(times['flag off']):.3f}", flush=True)
    time_step_update()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edit", action="store_true", help="Edit traffic: mixed_step_batch_edit against one request per forward")
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--teacache", type=float, default=None, metavar="THRESH")
    ap.add_argument("--lib", default=None, help="another build of libomni_cdna4.so (with --teacache)")
    ap.add_argument("--only", default=None, help="with --teacache: the workload whose name starts with this (B or C)")
    a = ap.parse_args()
    if a.edit:
        return main_edit(a)
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
