"""GPU: requests of different resolutions and true-CFG scales in one DiT forward (`OmniDiffusionConfig.mixed_step_batch`).

Checker throughout: the fp32 oracle run ON THE GPU for every item / request ALONE (per-request B = 1 semantics); calibration:
the same oracle in bf16 (the reference's algorithm in the reference's dtype), as tests/test_gpu_bench_shape_parity.py.

  * attention on mixed `cu_seqlens` through the public entry point (legacy grid sized by the longest item: it has no total row
    count to size a compact grid with), and one full-width `omni_dit_block` on the same lengths (compact head-major slot grid,
    csrc/common.h omni_attn_compact_slots) against the oracle block of every item alone;
  * forward parity at full width, 2 layers, one mixed CFG group {1328x1328, 1664x928, 512x512}, ragged prompts;
  * the step batcher end to end at reduced depth: three requests, two sizes, two scales, different step counts, a late
    joiner; fewer forwards than with the flag off; a hipGraph replay gives the latents of the uncaptured steps;
  * refusals: TeaCache and condition rows in a mixed group.

Measured on an MI355X (random N(0, 0.02^2) weights, 2 layers; product vs fp32 oracle, in brackets bf16-eager vs fp32 oracle):
one mixed forward 5.22e-3 .. 5.26e-3 (6.92e-3 .. 7.04e-3); step-batcher final latents 1.05e-2 .. 1.42e-2 (1.24e-2 .. 1.63e-2);
BASELINE.md 3 ("Mixed step batches"); one block on mixed lengths 3.85e-3 .. 3.92e-3 (image and text).  Compact grid against legacy grid on the same forward, by output digest: profiles/mixed_attention_compact_grid_ab.txt."""
import math

import pytest
import torch

import qwen_image_oracle as O
from _util import cosine, rel_l2

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda:0"
H = 24


def _rnd(*shape, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g).to(BF16)


def _perturbed_random_model(layers: int, seed: int):
    """Full-width product model, random weights drawn on the device, non-zero biases and jittered norm weights (the model of
    tests/test_gpu_bench_shape_parity.py)."""
    from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel

    m = QwenImageTransformer2DModel(num_layers=layers, device=DEV)
    m.init_random_(seed=seed)
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    for n, p in m.named_parameters():
        if p.dim() == 1 and "norm" in n:
            p.data.add_(0.1 * torch.randn(p.shape, device=DEV, generator=g).to(BF16))
        elif p.dim() == 1:
            p.data.copy_((0.02 * torch.randn(p.shape, device=DEV, generator=g)).to(BF16))
    return m


def _oracle_params(m, dtype=torch.float32):
    return {n: p.detach().to(dtype) for n, p in m.named_parameters()}      # BEFORE the first forward (row-major layout)


def _oracle_denoise(P, lat, pos, neg, grid, steps, cfg, dtype):
    """reference diffuse() (pipeline_qwen_image.py:530-586) with the oracle DiT in `dtype`; latents kept in bf16 (:585)."""
    ts, sig = O.flow_match_sigmas(steps, lat.shape[1])
    x = lat.float()
    for i, t in enumerate(ts):
        s_in = (t.bfloat16() / 1000).bfloat16().float().expand(1).to(lat.device)
        p = O.dit_forward(P, x.to(dtype), pos.to(dtype), s_in, grid, num_heads=H).float()
        n = O.dit_forward(P, x.to(dtype), neg.to(dtype), s_in, grid, num_heads=H).float()
        x = O.euler_step(x, O.cfg_combine(p, n, cfg), float(sig[i]), float(sig[i + 1])).bfloat16().float()
    return x


# ------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("lens", [[6920, 6065, 1058, 290], [6920, 6065, 1058, 290] * 2, [290, 1058]],
                         ids=["mix4_w64", "mix4_cfg_doubled_w64", "small_mix_pipe"])
def test_attention_on_mixed_seqlens_matches_fp32_sdpa_per_item(lens):
    from vllm_omni_amd import ops

    rows = sum(lens)
    q, k, v = (_rnd(rows, H * 128, seed=s) for s in (1, 2, 3))
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
    scale = 1 / math.sqrt(128)
    a = ops.flash_attn_varlen(q, k, v, cu, H, max(lens), scale)
    b = ops.flash_attn_varlen(q, k, v, cu, H, max(lens), scale)
    torch.cuda.synchronize()
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)                 # deterministic
    o = 0
    for i, n in enumerate(lens):
        qi, ki, vi = (t[o:o + n].float().view(1, n, H, 128).permute(0, 2, 1, 3) for t in (q, k, v))
        ref = torch.nn.functional.scaled_dot_product_attention(qi, ki, vi).permute(0, 2, 1, 3).reshape(n, H * 128)
        r = rel_l2(a[o:o + n], ref)
        print(f"   item {i} ({n} rows): rel_l2 vs fp32 SDPA {r:.3e}")
        assert r <= 4e-3, (i, n, r)
        del ref
        o += n


@pytest.mark.parametrize("case", ["mix4", "mix4_cfg_doubled", "small_mix_pipe"])
def test_one_fullwidth_block_on_mixed_lengths_matches_the_oracle_block_per_item(case):
    """Joint lengths [6920, 6065, 1058, 290] (and their CFG doubling) through omni_dit_block: the attention launch inside the
    forward knows n_joint_rows and takes the compact grid of the w64 kernel (8 items: 119 slots per head instead of 224
    blocks).  The small mix [1058, 290]: 2 x 24 x ceil(1058 / 256) = 240 < 512 workgroups keeps the launch on the 4-wave pipe
    kernel (128-query blocks), whose compact grid has 12 slots per head instead of 18 blocks."""
    import ctypes as C

    from vllm_omni_amd import _native as N
    from vllm_omni_amd.diffusion.batch import attention_compact_slots, build_ragged_batch

    torch.backends.cuda.matmul.allow_tf32 = False
    m = _perturbed_random_model(1, seed=78)
    P32 = _oracle_params(m)
    if case == "small_mix_pipe":
        grids, txt_lens, want = [(1, 32, 32), (1, 16, 16)], [34, 34], [1058, 290]
    else:
        rep = 2 if case == "mix4_cfg_doubled" else 1
        grids, txt_lens = [(1, 83, 83), (1, 58, 104), (1, 32, 32), (1, 16, 16)] * rep, [31, 33, 34, 34] * rep
        want = [6920, 6065, 1058, 290] * rep
    n, D = len(grids), m.inner_dim
    rb = build_ragged_batch(txt_lens, grids)
    seq = [t + s for t, s in zip(rb.txt_lens, rb.s_imgs)]
    assert seq == want
    # which kernel the launcher picks (attention.hip: w64 from 512 workgroups of 256 queries; below that 4-wave pipe blocks of 128
    # queries while the grid is under 6 x 256 such workgroups) and that the launch takes the compact grid there
    w64 = n * H * -(-max(seq) // 256) >= 512
    assert w64 == (case != "small_mix_pipe")
    Q = 256 if w64 else 128
    assert 0 < attention_compact_slots(seq, Q) < n * -(-max(seq) // Q)
    hid = [_rnd(s, D, seed=40 + i) for i, s in enumerate(rb.s_imgs)]
    enc = [_rnd(t, D, seed=60 + i) for i, t in enumerate(txt_lens)]
    temb = _rnd(n, D, seed=80)
    h_all, e_all = torch.cat(hid).contiguous(), torch.cat(enc).contiguous()
    lib, w, b = m._descriptor(m.prepare_batch(rb), rb.n_img_rows, rb.n_txt_rows)
    N.check(lib.omni_dit_block(C.byref(w), 0, C.byref(b), h_all.data_ptr(), e_all.data_ptr(), temb.data_ptr(),
                               torch.cuda.current_stream().cuda_stream), "omni_dit_block")
    torch.cuda.synchronize()
    assert torch.isfinite(h_all.float()).all() and torch.isfinite(e_all.float()).all()
    io, to = rb.img_offsets, [0]
    for t in txt_lens:
        to.append(to[-1] + t)
    with torch.no_grad():
        for i in range(n):
            vid_cs, txt_cs = O.rope_tables(*grids[i], txt_lens[i])
            e_ref, h_ref = O.dit_block(P32, 0, hid[i][None].float(), enc[i][None].float(), temb[i:i + 1].float(), vid_cs, txt_cs, H)
            hi, ei = h_all[io[i]:io[i + 1]][None], e_all[to[i]:to[i + 1]][None]
            r = (rel_l2(hi, h_ref), cosine(hi, h_ref), rel_l2(ei, e_ref), cosine(ei, e_ref))
            print(f"   item {i} ({seq[i]} joint rows): image rel_l2 {r[0]:.3e} cos {r[1]:.6f}; text rel_l2 {r[2]:.3e} cos {r[3]:.6f}")
            assert r[0] <= 1e-2 and r[1] >= 0.9995 and r[2] <= 1e-2 and r[3] >= 0.9995, (i, r)
            del e_ref, h_ref


# ------------------------------------------------------------------------------------------------------- one forward
def test_forward_parity_of_a_mixed_cfg_group_at_full_width():
    from vllm_omni_amd.diffusion.batch import build_ragged_batch

    torch.backends.cuda.matmul.allow_tf32 = False
    m = _perturbed_random_model(2, seed=77)
    P32, Pb = _oracle_params(m), _oracle_params(m, BF16)
    grids = [(1, 83, 83), (1, 58, 104), (1, 32, 32)]                         # 1328x1328, 1664x928, 512x512
    R = len(grids)
    t_pos, t_neg = [64, 290, 20], [11, 37, 5]                                # ragged prompts
    lens = t_pos + t_neg
    item_grid = grids * 2                                                    # pos_0..pos_2, neg_0..neg_2
    S = [g[1] * g[2] for g in item_grid]
    lat_r = [_rnd(S[r], 64, seed=10 + r) for r in range(R)]
    lat = lat_r * 2                                                          # a CFG pair shares its latents
    txt = [_rnd(t, 3584, seed=30 + i) for i, t in enumerate(lens)]
    sig = torch.tensor([0.6015625, 0.25, 0.90625], device=DEV)               # one step index per request, exact in bf16
    rb = build_ragged_batch(lens, item_grid, temb_rows=list(range(R)) * 2)
    assert rb.mixed and rb.max_seqlen == 83 * 83 + 64
    out = m.forward_ragged(m.prepare_batch(rb), torch.cat(lat), torch.cat(txt), sig).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and out.shape == (sum(S), 64)
    off = rb.img_offsets
    rows = []
    with torch.no_grad():
        for i in range(2 * R):
            s1 = sig[i % R:i % R + 1]
            ref = O.dit_forward(P32, lat[i][None].float(), txt[i][None].float(), s1, item_grid[i], num_heads=H)
            eag = O.dit_forward(Pb, lat[i][None], txt[i][None], s1.to(BF16), item_grid[i], num_heads=H)
            got = out[off[i]:off[i + 1]][None]
            rows.append((rel_l2(got, ref), cosine(got, ref), rel_l2(eag, ref)))
            del ref, eag
    for i, (r, c, e) in enumerate(rows):
        print(f"   item {i} grid {item_grid[i]} T {lens[i]}: product vs fp32 oracle {r:.3e} cos {c:.6f}; bf16-eager {e:.3e}")
    for r, c, e in rows:
        assert r <= 1e-2 and c >= 0.9995                                     # the forward bar
        assert r <= 1.1 * e                                                  # no further from fp32 than the bf16-eager algorithm


# ------------------------------------------------------------------------------------------------------- step batcher
def _requests():
    """Three true-CFG requests: two sizes, two scales, three step counts."""
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest

    spec = [("a", 512, 512, 4, 4.0, 21, 9), ("b", 480, 832, 3, 2.5, 64, 5), ("c", 512, 512, 2, 2.5, 13, 30)]
    out = {}
    for i, (tag, h, w, steps, cfg, tp, tn) in enumerate(spec):
        S = (h // 16) * (w // 16)
        lat, pos, neg = _rnd(1, S, 64, seed=100 + i), _rnd(1, tp, 3584, seed=200 + i), _rnd(1, tn, 3584, seed=300 + i)
        out[tag] = dict(grid=(1, h // 16, w // 16), steps=steps, cfg=cfg, lat=lat, pos=pos, neg=neg,
                        req=lambda h=h, w=w, steps=steps, cfg=cfg, lat=lat, pos=pos, neg=neg: OmniDiffusionRequest(
                            height=h, width=w, num_inference_steps=steps, true_cfg_scale=cfg, latents=lat, prompt_embeds=pos,
                            negative_prompt_embeds=neg, output_type="latent"))
    return out


def _serve(m, spec, **cfg):
    """a and b start together, c joins after their first step.  -> ({tag: final latents}, forwards, serve-state keys)."""
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline
    from vllm_omni_amd.diffusion.step_batcher import ContinuousStepBatcher

    pipe = QwenImagePipeline(od_config=OmniDiffusionConfig(max_step_batch=4, **cfg), device=DEV, transformer=m)
    calls, orig = [], m.forward_ragged

    def counted(prepared, *a, **k):
        calls.append(tuple(prepared["batch"].s_imgs))
        return orig(prepared, *a, **k)

    m.forward_ragged = counted
    try:
        b = ContinuousStepBatcher(pipe)
        b.add(spec["a"]["req"](), "a")
        b.add(spec["b"]["req"](), "b")
        n_warm = len(calls)
        done = dict(b.step())
        b.add(spec["c"]["req"](), "c")
        done.update(b.drain())
        torch.cuda.synchronize()
    finally:
        m.forward_ragged = orig
    for t, o in done.items():
        assert o.error is None, (t, o.error)
    return {t: o.output.clone() for t, o in done.items()}, calls[n_warm:], dict(pipe._serve_states)


def test_step_batcher_mixes_sizes_and_scales_end_to_end():
    torch.backends.cuda.matmul.allow_tf32 = False
    m = _perturbed_random_model(2, seed=77)
    spec = _requests()
    ref, eager = {}, {}
    with torch.no_grad():
        P32 = _oracle_params(m)
        for t, s in spec.items():
            ref[t] = _oracle_denoise(P32, s["lat"], s["pos"], s["neg"], s["grid"], s["steps"], s["cfg"], torch.float32)
        del P32
        Pb = _oracle_params(m, BF16)
        for t, s in spec.items():
            eager[t] = _oracle_denoise(Pb, s["lat"], s["pos"], s["neg"], s["grid"], s["steps"], s["cfg"], BF16)
        del Pb
    off, calls_off, _ = _serve(m, spec, use_hip_graph=False)
    on, calls_on, keys = _serve(m, spec, use_hip_graph=False, mixed_step_batch=True)
    graph, calls_g, states_g = _serve(m, spec, use_hip_graph=True, mixed_step_batch=True)
    print(f"   forwards: flag off {len(calls_off)}, flag on {len(calls_on)} (hipGraph run: {len(calls_g)} uncaptured calls)")
    for t in spec:
        r_on, r_off, r_e = rel_l2(on[t], ref[t]), rel_l2(off[t], ref[t]), rel_l2(eager[t], ref[t])
        print(f"   request {t} {spec[t]['grid']} {spec[t]['steps']} steps cfg {spec[t]['cfg']}: final latents vs fp32 oracle — "
              f"mixed {r_on:.3e} cos {cosine(on[t], ref[t]):.6f}; flag off {r_off:.3e}; bf16-eager {r_e:.3e}")
    # a forward really held two sizes, with the longest item first, and there were fewer forwards than with the flag off
    assert any(len(set(c)) > 1 for c in calls_on) and not any(len(set(c)) > 1 for c in calls_off)
    assert all(list(c[:len(c) // 2]) == sorted(c[:len(c) // 2], reverse=True) for c in calls_on)
    assert len(calls_on) < len(calls_off)
    assert sum(spec[t]["steps"] for t in spec) > len(calls_on) >= max(spec[t]["steps"] for t in spec)
    assert any(k[0] == "mixed" for k in keys)
    # the hipGraph run really captured every mixed composition and replayed it: forward_ragged is entered only by a state's
    # warm-up + capture (2 per composition), never per step
    mixed_g = [st for k, st in states_g.items() if k[0] == "mixed"]
    assert mixed_g and all(st["graph"] is not None for st in mixed_g)
    assert len(calls_g) == 2 * len(states_g) and len(states_g) < len(calls_on)
    for t in spec:
        assert torch.isfinite(on[t].float()).all()
        assert rel_l2(on[t], ref[t]) <= 1.1 * rel_l2(eager[t], ref[t]), t
        assert torch.equal(graph[t], on[t]), t                               # a replayed composition == the uncaptured steps


# ------------------------------------------------------------------------------------------------------- refusals
def test_mixed_group_refuses_teacache_and_condition_rows():
    from vllm_omni_amd.diffusion.cache.teacache.config import TeaCacheConfig
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline
    from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel
    from vllm_omni_amd.diffusion.step_batcher import ActiveSample

    m = QwenImageTransformer2DModel(num_layers=1, device=DEV).init_random_(seed=3)
    pipe = QwenImagePipeline(od_config=OmniDiffusionConfig(mixed_step_batch=True, use_hip_graph=False), device=DEV, transformer=m)
    spec = _requests()
    group = []
    for i, t in enumerate(("a", "b")):
        a = ActiveSample(tag=t, sample=pipe.resolve_request(spec[t]["req"]())[0], seq=i)
        pipe.begin_sample(a)
        group.append(a)
    group[0].state["cond"] = _rnd(16, 64, seed=1)
    with pytest.raises(NotImplementedError, match="condition-image rows"):
        pipe.denoise_one_step(group)
    group[0].state["cond"] = None
    m.teacache = TeaCacheConfig(transformer_type=type(m).__name__)
    try:
        with pytest.raises(NotImplementedError, match="TeaCache"):
            pipe.denoise_one_step(group)
        assert pipe.batch_key(group[0]) != pipe.batch_key(group[1])           # ... and the batcher would not have built that group
    finally:
        m.teacache = None
    assert pipe.batch_key(group[0]) == pipe.batch_key(group[1])
    pipe.denoise_one_step(group)                                             # the same group without either: runs
    torch.cuda.synchronize()
