"""SAGE_ATTN on the GPU: the quantisation pass and the int8 attention kernel (csrc/attention_sage.hip) against the host model
(tests/_sage_model.py) and fp32 SDPA, the plug-in backend, and the Qwen-Image DiT forward with attn_qk_int8."""
import pytest
import torch

import _sage_model as M
import qwen_image_oracle as O
from _util import bf16_round, golden_params, load_golden, rel_l2

BF16 = torch.bfloat16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1.5e-2          # int8 attention vs fp32 SDPA (the host model's bar)
KERNEL_BAR = 4e-3     # kernel vs the host model on the same int8 operands


def _cu(lengths):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    return cu


def _run(q, k, v, cu_q, cu_k, sc, out_k32=False):
    from vllm_omni_amd import ops

    Rq, H, dh = q.shape
    Hkv = k.shape[1]
    mq = max(b - a for a, b in zip(cu_q, cu_q[1:]))
    mk = max(b - a for a, b in zip(cu_k, cu_k[1:]))
    B = len(cu_q) - 1
    ws = torch.empty(ops.attn_quant_workspace_bytes(B, H, Hkv, dh, mq, mk), dtype=torch.uint8, device=DEV)
    cq = torch.tensor(cu_q, dtype=torch.int32, device=DEV)
    ck = torch.tensor(cu_k, dtype=torch.int32, device=DEV)
    o = ops.flash_attn_general(q.reshape(Rq, H * dh), k.reshape(-1, Hkv * dh), v.reshape(-1, Hkv * dh), cq, ck, H, Hkv, mq, mk,
                               sc, qk_int8=True, workspace=ws, out_k32_blocked=out_k32)
    torch.cuda.synchronize()
    if out_k32:
        o = o.view(H * dh // 32, Rq, 32).permute(1, 0, 2).reshape(Rq, H * dh)
    return o.view(Rq, H, dh), ws, (B, H, Hkv, dh, mq, mk)


def _carve(ws, B, H, Hkv, dh, mq, mk):
    """The workspace layout of attention_sage.hip (sage_carve): q8, k8, sq, sk, km, each 256-byte aligned."""
    al = lambda n: (n + 255) // 256 * 256          # noqa: E731
    nbq, nbk = (mq + 63) // 64, (mk + 63) // 64
    sizes = [B * mq * H * dh, B * mk * Hkv * dh, B * nbq * H * 4, B * nbk * Hkv * 4, B * Hkv * dh * 4]
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + al(s))
    part = lambda i: ws[offs[i]:offs[i] + sizes[i]]  # noqa: E731
    return (part(0).view(torch.int8).view(B, mq, H, dh), part(1).view(torch.int8).view(B, mk, Hkv, dh),
            part(2).view(torch.float32).view(B, nbq, H), part(3).view(torch.float32).view(B, nbk, Hkv),
            part(4).view(torch.float32).view(B, Hkv, dh))


def _ulps(a, b) -> int:
    return int((a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs().max())


SHAPES = [
    ("ragged_odd", [83 * 83 + 37, 50, 37, 1], None, 4, 128, range(4)),
    ("dh64_cross", [300, 77], [77, 300], 4, 64, range(4)),
    ("1024sq_x10", [4160] * 10, None, 24, 128, range(0, 24, 6)),
    ("2048sq_cfg_pair", [16448] * 2, None, 24, 128, range(0, 24, 12)),
]


@pytest.mark.parametrize("name,lq,lk,H,dh,heads", SHAPES, ids=[s[0] for s in SHAPES])
def test_quant_pass_and_kernel_match_the_host_model_and_sdpa(name, lq, lk, H, dh, heads):
    cu_q = _cu(lq)
    cu_k = _cu(lk) if lk else cu_q
    q, k, v = M.make_qkv(cu_q[-1], cu_k[-1], H, dh, seed=5, device=DEV)
    sc = M.default_scale(dh)
    out, ws, dims = _run(q, k, v, cu_q, cu_k, sc)
    q8, k8, sq, sk, km = _carve(ws, *dims)
    out2, _, _ = _run(q, k, v, cu_q, cu_k, sc)
    assert torch.equal(out, out2), "two launches differ"
    hs = list(heads)
    e_host, e_sdpa, flips, n = [], [], 0, 0
    for b in range(len(cu_q) - 1):
        qs, qe, ks, ke = cu_q[b], cu_q[b + 1], cu_k[b], cu_k[b + 1]
        hq8, hsq, hk8, hsk, hkm = M.quantize_item(q[qs:qe][:, hs], k[ks:ke][:, hs], sc * M.LOG2E)
        gkm = km[b][hs]
        assert float((gkm - hkm).norm() / hkm.norm().clamp_min(1e-30)) <= 1e-6
        # the K quantisation is checked on the GPU's own key mean: a 1e-6 change of a large mean moves k' by several ulps
        hk8, hsk = M.quant_blocks(k[ks:ke][:, hs].float() - gkm)
        # within 1 ulp: torch on the GPU divides by a scalar as a multiplication by its reciprocal; k' also carries the key
        # mean's summation order
        assert _ulps(sq[b, :hsq.shape[0]][:, hs], hsq) <= 1
        assert _ulps(sk[b, :hsk.shape[0]][:, hs], hsk) <= 1
        gq8, gk8 = q8[b, :qe - qs][:, hs], k8[b, :ke - ks][:, hs]
        dq, dk = (gq8.int() - hq8.int()).abs(), (gk8.int() - hk8.int()).abs()
        assert int(dq.max()) <= 1 and int(dk.max()) <= 1
        flips += int(dq.sum() + dk.sum())
        n += dq.numel() + dk.numel()
        # the kernel on the GPU's own int8 operands vs the host model's attention on the same operands
        ref_int8 = M.attend_int8(gq8, sq[b, :hsq.shape[0]][:, hs], gk8, sk[b, :hsk.shape[0]][:, hs], v[ks:ke][:, hs])
        e_host.append(rel_l2(out[qs:qe][:, hs], ref_int8))
        ref = M.sdpa_fp32(q[qs:qe][:, hs], k[ks:ke][:, hs], v[ks:ke][:, hs], [0, qe - qs], [0, ke - ks], sc)
        e_sdpa.append(rel_l2(out[qs:qe][:, hs], ref))
    print(f"{name}: kernel vs host model {max(e_host):.2e}, vs fp32 SDPA {max(e_sdpa):.2e}, int8 +-1 flips {flips / n:.1e}")
    assert flips <= 1e-4 * n
    assert max(e_host) <= KERNEL_BAR
    assert max(e_sdpa) <= BAR


def test_k32_blocked_output_is_the_same_result():
    cu = _cu([83 * 83 + 37, 50])
    q, k, v = M.make_qkv(cu[-1], cu[-1], 4, 128, seed=6, device=DEV)
    a, _, _ = _run(q, k, v, cu, cu, M.default_scale(128))
    b, _, _ = _run(q, k, v, cu, cu, M.default_scale(128), out_k32=True)
    assert torch.equal(a, b)


def test_general_entry_refuses_mask_causal_and_a_short_workspace():
    from vllm_omni_amd import _native as N
    from vllm_omni_amd import ops

    q = torch.zeros(64, 128, dtype=torch.bfloat16, device=DEV)
    cu = torch.tensor([0, 64], dtype=torch.int32, device=DEV)
    with pytest.raises(N.OmniNativeError, match="UNSUPPORTED|-2"):
        ops.flash_attn_general(q, q, q, cu, cu, 1, 1, 64, 64, 0.1, causal=True, qk_int8=True)
    small = torch.empty(16, dtype=torch.uint8, device=DEV)
    with pytest.raises(N.OmniNativeError, match="BAD_ARG|-1"):
        ops.flash_attn_general(q, q, q, cu, cu, 1, 1, 64, 64, 0.1, qk_int8=True, workspace=small)


def test_plugin_backend_dh64_nhd(monkeypatch):
    from vllm_omni_amd.diffusion.attention.backends.abstract import AttentionMetadata
    from vllm_omni_amd.diffusion.attention.selector import get_attn_backend

    monkeypatch.setenv("DIFFUSION_ATTENTION_BACKEND", "SAGE_ATTN")
    get_attn_backend.cache_clear()
    try:
        impl = get_attn_backend(-1).get_impl_cls()(num_heads=4, head_size=64, softmax_scale=0.125)
    finally:
        get_attn_backend.cache_clear()
    q, k, v = (t.view(2, 333, 4, 64) for t in M.make_qkv(666, 666, 4, 64, seed=7, device=DEV))
    out = impl.forward(q, k, v)
    ref = torch.nn.functional.scaled_dot_product_attention(*(t.float().permute(0, 2, 1, 3) for t in (q, k, v)),
                                                           scale=0.125).permute(0, 2, 1, 3)
    err = rel_l2(out, ref)
    print(f"SageAttentionImpl dh 64 vs SDPA: {err:.2e}")
    assert out.shape == q.shape and err <= BAR
    with pytest.raises(ValueError):
        impl.forward(q, k, v, AttentionMetadata(attn_mask=torch.ones(666, dtype=torch.bool, device=DEV)))


def _dit_error(monkeypatch, backend):
    from vllm_omni_amd.diffusion.attention.selector import get_attn_backend
    from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel

    if backend is None:
        monkeypatch.delenv("DIFFUSION_ATTENTION_BACKEND", raising=False)
    else:
        monkeypatch.setenv("DIFFUSION_ATTENTION_BACKEND", backend)
    get_attn_backend.cache_clear()
    z, meta, c = load_golden("dit_fullwidth_1layer_fp32")
    P = golden_params(c)
    m = QwenImageTransformer2DModel(num_layers=c["layers"], num_attention_heads=c["heads"], joint_attention_dim=c["joint"],
                                    device=DEV)
    m.load_weights(P.items())
    gh, gw = c["grid"]
    sig = torch.from_numpy(z["sigma"])
    out = m(hidden_states=torch.from_numpy(z["latents"]).to(DEV, torch.bfloat16),
            encoder_hidden_states=torch.from_numpy(z["prompt_embeds"]).to(DEV, torch.bfloat16), timestep=sig.to(DEV),
            img_shapes=[[(1, gh, gw)]] * c["B"], txt_seq_lens=[c["T"]] * c["B"], return_dict=False)[0]
    torch.cuda.synchronize()
    get_attn_backend.cache_clear()
    Pb = {kk: bf16_round(vv) for kk, vv in P.items()}
    oracle = O.dit_forward(Pb, bf16_round(torch.from_numpy(z["latents"])), bf16_round(torch.from_numpy(z["prompt_embeds"])),
                           bf16_round(sig), (1, gh, gw), num_heads=c["heads"])
    return rel_l2(out, oracle), m


def test_dit_forward_with_int8_attention(monkeypatch):
    e_bf16, m0 = _dit_error(monkeypatch, None)
    e_int8, m1 = _dit_error(monkeypatch, "SAGE_ATTN")
    print(f"full-width 1-layer DiT vs fp32 oracle: bf16 attention {e_bf16:.3e}, int8 attention {e_int8:.3e}")
    assert m0._qk_int8 is False and m1._qk_int8 is True
    assert e_int8 <= 2 * e_bf16 and e_int8 <= 2e-2


def test_item_skip_leaves_skipped_items_untouched():
    from vllm_omni_amd import ops

    lens = [83 * 83 + 37, 50, 700]
    cu = _cu(lens)
    H, dh = 4, 128
    q, k, v = M.make_qkv(cu[-1], cu[-1], H, dh, seed=8, device=DEV)
    cq = torch.tensor(cu, dtype=torch.int32, device=DEV)
    args = (q.reshape(-1, H * dh), k.reshape(-1, H * dh), v.reshape(-1, H * dh), cq, cq, H, H, max(lens), max(lens), 0.088)
    full = ops.flash_attn_general(*args, qk_int8=True)
    sentinel = torch.full_like(full, 7.0)
    skip = torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV)
    part = ops.flash_attn_general(*args, qk_int8=True, out=sentinel.clone(), item_skip=skip)
    torch.cuda.synchronize()
    assert torch.equal(part[cu[1]:cu[2]], sentinel[cu[1]:cu[2]])           # the skipped item's rows: not written
    assert torch.equal(part[:cu[1]], full[:cu[1]]) and torch.equal(part[cu[2]:], full[cu[2]:])


def _int8(m, on: bool):
    m._qk_int8 = on            # what the first forward decides from DIFFUSION_ATTENTION_BACKEND (see test_dit_forward_with_int8_attention)
    return m


def test_teacache_and_hip_graph_on_the_int8_path():
    """TeaCache's per-item skip predicate reaches the int8 kernels inside omni_dit_forward, and a hipGraph-captured loop replays
    the int8 forwards bit-identically to the eager loop."""
    from test_gpu_teacache import _loop_inputs, _model, _native_loop

    steps = 6
    m, _ = _model()
    lat, pos, neg = _loop_inputs(steps)
    plain_bf16, _ = _native_loop(_int8(m, False), None, lat, pos, neg, steps, False)
    plain, _ = _native_loop(_int8(m, True), None, lat, pos, neg, steps, False)
    graphed, _ = _native_loop(m, None, lat, pos, neg, steps, True)
    assert torch.equal(graphed, plain), "hipGraph replay of the int8 forward differs from eager"
    never, skips = _native_loop(m, 1e-12, lat, pos, neg, steps, False)
    assert skips == [0, 0] and torch.equal(never, plain)
    always, skips = _native_loop(m, 1e12, lat, pos, neg, steps, False)
    assert skips == [steps - 1, steps - 1]
    always_g, skips_g = _native_loop(m, 1e12, lat, pos, neg, steps, True)
    assert skips_g == skips and torch.equal(always_g, always)
    always_bf16, _ = _native_loop(_int8(m, False), 1e12, lat, pos, neg, steps, False)
    print(f"int8 vs bf16 attention, 6-step loop: uncached {rel_l2(plain, plain_bf16):.2e}, always-skip {rel_l2(always, always_bf16):.2e}")
    assert rel_l2(plain, plain_bf16) <= BAR and rel_l2(always, always_bf16) <= BAR


def test_step_batched_int8_requests_equal_solo_runs():
    from test_gpu_teacache import _loop_inputs, _model
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest

    m, _ = _model()
    pipe = QwenImagePipeline(device=DEV, transformer=_int8(m, True))
    reqs = []
    for i in range(2):
        lat, pos, neg = _loop_inputs(3, seed=20 + i)
        reqs.append(OmniDiffusionRequest(height=256, width=256, num_inference_steps=3, true_cfg_scale=4.0, latents=lat.to(BF16),
                                         prompt_embeds=pos.to(BF16), negative_prompt_embeds=neg.to(BF16), output_type="latent"))
    both = pipe.generate(reqs, output_type="latent")
    for r, b in zip(reqs, both):
        solo = pipe.generate([r], output_type="latent")[0].output
        assert rel_l2(b.output, solo) <= 5e-3       # per-item quantisation blocks: only GEMM tile grouping differs


def test_sequence_parallel_path_runs_int8_attention():
    from test_gpu_sequence_parallel import _emulate
    from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel

    heads, joint, layers, grid, T = 4, 128, 3, (1, 16, 8), 13
    Pm = O.make_dit_params(layers, seed=1234, bias_std=0.02, norm_jitter=0.1, num_heads=heads, joint_dim=joint)
    m = QwenImageTransformer2DModel(num_layers=layers, num_attention_heads=heads, joint_attention_dim=joint, device=DEV)
    m.load_weights(Pm.items())
    g = torch.Generator().manual_seed(3)
    lat, txt, sig = bf16_round(torch.randn(128, 64, generator=g)), bf16_round(torch.randn(T, joint, generator=g)), torch.tensor([0.4375])
    run = lambda: m(hidden_states=lat.to(DEV, BF16).unsqueeze(0), encoder_hidden_states=txt.to(DEV, BF16).unsqueeze(0),  # noqa: E731
                    timestep=sig.to(DEV), img_shapes=[[grid]], txt_seq_lens=[T], return_dict=False)[0][0]
    _int8(m, True)
    ref8 = run()
    _int8(m, False)
    ref16 = run()
    _int8(m, True)
    outs, _ = _emulate(m, 2, lat.to(DEV, BF16), txt.to(DEV, BF16), sig.to(DEV), grid)
    sp_ws = m._sage_ws
    torch.cuda.synchronize()
    print(f"SP (2 ranks) int8 vs single-device int8 {rel_l2(outs[0], ref8):.2e}, vs bf16 {rel_l2(outs[0], ref16):.2e}")
    assert sp_ws is not None, "the sequence-parallel path did not run the int8 attention"
    assert rel_l2(outs[0], ref8) <= 4e-3 and rel_l2(outs[0], ref16) <= BAR


def test_pipeline_256px_end_to_end_with_the_environment_variable(monkeypatch):
    from vllm_omni_amd.diffusion.attention.selector import get_attn_backend
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline
    from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest

    g = torch.Generator().manual_seed(42)
    lat = bf16_round(torch.randn(1, 256, 64, generator=g))
    pos, neg = bf16_round(torch.randn(1, 11, 3584, generator=g)), bf16_round(torch.randn(1, 5, 3584, generator=g))
    P = O.make_dit_params(2, seed=1234, bias_std=0.02, norm_jitter=0.1, num_heads=24, joint_dim=3584)
    outs = {}
    for backend in (None, "SAGE_ATTN"):
        if backend is None:
            monkeypatch.delenv("DIFFUSION_ATTENTION_BACKEND", raising=False)
        else:
            monkeypatch.setenv("DIFFUSION_ATTENTION_BACKEND", backend)
        get_attn_backend.cache_clear()
        m = QwenImageTransformer2DModel(num_layers=2, device=DEV)
        m.load_weights(P.items())
        pipe = QwenImagePipeline(device=DEV, transformer=m)
        req = OmniDiffusionRequest(height=256, width=256, num_inference_steps=4, true_cfg_scale=4.0, latents=lat.to(BF16),
                                   prompt_embeds=pos.to(BF16), negative_prompt_embeds=neg.to(BF16), output_type="latent")
        outs[backend] = pipe.generate([req], output_type="latent")[0].output
        assert m._qk_int8 is (backend == "SAGE_ATTN")
    get_attn_backend.cache_clear()
    from test_gpu_pipeline import oracle_denoise

    ref = oracle_denoise({kk: bf16_round(vv) for kk, vv in P.items()}, lat, pos, neg, (1, 16, 16), 4, 24)
    e16, e8 = rel_l2(outs[None], ref), rel_l2(outs["SAGE_ATTN"], ref)
    print(f"256^2 4-step true-CFG pipeline vs fp32 oracle: bf16 attention {e16:.2e}, SAGE_ATTN {e8:.2e}; "
          f"SAGE_ATTN vs bf16 {rel_l2(outs['SAGE_ATTN'], outs[None]):.2e}")
    # CFG 4.0 amplifies the attention's error into the latent, so the yardstick is the fp32 oracle, as test_gpu_pipeline.py's
    # config-0 test (2e-2) uses, next to the bf16 path's own error in the same run
    assert e8 <= 2e-2 and e8 <= 2 * e16


def test_60_layers_1024px_4step_cfg_loop_against_the_fp32_oracle():
    """The headline shape at real depth: the int8 path's final-latent error against the fp32 oracle, next to the bf16 path's in
    the same test (test_gpu_bench_shape_parity.py's model and oracle)."""
    from test_gpu_bench_shape_parity import _oracle_denoise, _oracle_params, _perturbed_random_model, _product_trajectory
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest

    torch.backends.cuda.matmul.allow_tf32 = False
    steps = 4
    m = _perturbed_random_model(60, seed=1234)
    grid, S = (1, 64, 64), 4096
    g = torch.Generator(device=DEV).manual_seed(42)
    lat = torch.randn(1, S, 64, device=DEV, generator=g).to(BF16)
    pos = torch.randn(1, 64, 3584, device=DEV, generator=g).to(BF16)
    neg = torch.randn(1, 48, 3584, device=DEV, generator=g).to(BF16)
    with torch.no_grad():
        P32 = _oracle_params(m)
        ref, _ = _oracle_denoise(P32, lat, pos, neg, grid, steps, 4.0, torch.float32, [])
        del P32
        torch.cuda.empty_cache()
    pipe = QwenImagePipeline(od_config=OmniDiffusionConfig(use_hip_graph=False), device=DEV, transformer=m)
    req = OmniDiffusionRequest(height=1024, width=1024, num_inference_steps=steps, true_cfg_scale=4.0, latents=lat,
                               prompt_embeds=pos, negative_prompt_embeds=neg, output_type="latent")
    _int8(m, False)
    out16, _ = _product_trajectory(pipe, req)
    _int8(m, True)
    out8, _ = _product_trajectory(pipe, req)
    e16, e8 = rel_l2(out16, ref), rel_l2(out8, ref)
    print(f"60 layers @ 1024^2, 4-step true-CFG loop vs fp32 oracle: bf16 attention {e16:.3e}, int8 attention {e8:.3e}, "
          f"ratio {e8 / e16:.3f}")
    assert torch.isfinite(out8.float()).all()
    assert e8 <= 1.5 * e16
