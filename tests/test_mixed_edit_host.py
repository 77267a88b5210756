"""CPU: mixed step batches for Edit / Edit-Plus requests (`OmniDiffusionConfig.mixed_step_batch_edit`) — the host side.

  1. the flag is an opt-in on top of `mixed_step_batch`;
  2. `batch_key`: Edit samples on different grids and scales share a key only with the flag; Layered samples keep theirs;
     under TeaCache only with `mixed_step_batch_teacache` as well;
  3. the row layout of a step (`ragged_step_descriptors`): descriptor records and `lat_in` / `pred` offsets of a group of three
     requests, against the forward's own image-row offsets (`build_ragged_batch` on the multi-entry grids);
  4. the batcher: longest TOTAL rows first, `max_step_tokens` counts condition rows;
  5. the new entry point is bound outside `PROTOTYPES`, announced by a feature bit, and the ABI version did not move."""
import ctypes
import types

import numpy as np
import pytest
import torch

from vllm_omni_amd.diffusion.batch import build_ragged_batch

# the three requests of the GPU tests: (target grid, condition grids); 72 + 70, 272 + 30 and 64 + (45 + 16) rows
EDIT_GROUP = [((1, 9, 8), [(1, 10, 7)]), ((1, 16, 17), [(1, 6, 5)]), ((1, 8, 8), [(1, 5, 9), (1, 4, 4)])]


def _pipeline(**cfg):
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline

    class QwenImageTransformer2DModel:                       # (TeaCache looks its coefficients up by this class name)
        teacache = None

    vae = types.SimpleNamespace(config=types.SimpleNamespace(latents_mean=[0.0] * 16, latents_std=[1.0] * 16))
    return QwenImagePipeline(od_config=OmniDiffusionConfig(**cfg), device="cpu", transformer=QwenImageTransformer2DModel(), vae=vae)


def _edit_sample(target, conds, cfg, do_cfg=True, **extra):
    rows = sum(g[0] * g[1] * g[2] for g in conds)
    return types.SimpleNamespace(sample=dict(grid=(target, *conds), cfg=cfg, do_cfg=do_cfg, cond=torch.zeros(rows, 64), **extra))


# ---------------------------------------------------------------------------------------------------------------- 1
def test_flag_needs_mixed_step_batch():
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig

    assert OmniDiffusionConfig().mixed_step_batch_edit is False
    with pytest.raises(ValueError, match="mixed_step_batch_edit"):
        OmniDiffusionConfig(mixed_step_batch_edit=True)
    assert OmniDiffusionConfig(mixed_step_batch=True, mixed_step_batch_edit=True).mixed_step_batch_edit


# ---------------------------------------------------------------------------------------------------------------- 2
def test_batch_key_of_edit_samples():
    (ga, ca), (gb, cb), (gc, cc) = EDIT_GROUP
    a, b, c = _edit_sample(ga, ca, 4.0), _edit_sample(gb, cb, 2.5), _edit_sample(gc, cc, 3.0)
    on = _pipeline(mixed_step_batch=True, mixed_step_batch_edit=True)
    half, off = _pipeline(mixed_step_batch=True), _pipeline()
    assert on.batch_key(a) == on.batch_key(b) == on.batch_key(c)                 # Edit and Edit-Plus, three grids, three scales
    for p in (half, off):                                                        # without the flag: the key there was
        assert p.batch_key(a) != p.batch_key(b)
        assert p.batch_key(a) == ((ga, *ca), True, 4.0, True, None)
    # what a forward still cannot mix keeps its place in the key
    assert on.batch_key(a) != on.batch_key(_edit_sample(ga, ca, 4.0, do_cfg=False))
    assert on.batch_key(a) != on.batch_key(_edit_sample(ga, ca, 4.0, cfg_normalize=False))
    # text-to-image samples mix among themselves, never with Edit samples (their step update is another kernel)
    t2i = types.SimpleNamespace(sample=dict(grid=ga, cfg=4.0, do_cfg=True))
    assert on.batch_key(t2i) == half.batch_key(t2i) and on.batch_key(t2i) != on.batch_key(a)
    # Layered samples (explicit frame indices and / or additional_t_cond) keep today's key, flag or not
    lay4 = _edit_sample((1, 8, 8, 0), [(1, 8, 8, 1), (1, 4, 6, -1)], 4.0, t_cond=0, cfg_normalize=False)
    lay3 = _edit_sample((1, 8, 8), [(1, 8, 8), (1, 4, 6)], 4.0, t_cond=0, cfg_normalize=False)
    for s in (lay4, lay3):
        assert on.batch_key(s) == off.batch_key(s) == (s.sample["grid"], True, 4.0, False, 0)
    # TeaCache configured: mixed Edit groups form only with mixed_step_batch_teacache as well
    tea = _pipeline(mixed_step_batch=True, mixed_step_batch_edit=True, cache_backend="tea_cache")
    assert tea.transformer.teacache is not None
    assert tea.batch_key(a) != tea.batch_key(b) and tea.batch_key(a) == off.batch_key(a)
    both = _pipeline(mixed_step_batch=True, mixed_step_batch_edit=True, mixed_step_batch_teacache=True, cache_backend="tea_cache")
    assert both.batch_key(a) == both.batch_key(b) == on.batch_key(a)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("do_cfg", [True, False])
def test_step_layout_of_the_three_edit_requests(do_cfg):
    from vllm_omni_amd import _native as N
    from vllm_omni_amd.diffusion.batch import CFG_EULER_REQ_DTYPE, ragged_step_descriptors

    # the batcher's order: longest total rows first -> (1,16,17) 272 + 30, (1,9,8) 72 + 70, (1,8,8) 64 + 61
    order = [1, 0, 2]
    grids = [(EDIT_GROUP[i][0], *EDIT_GROUP[i][1]) for i in order]
    S, Sc, scales = [272, 72, 64], [30, 70, 61], [2.5, 4.0, 3.0]
    lay = ragged_step_descriptors(S, Sc, do_cfg, scales)
    n_br = 2 if do_cfg else 1
    rb = build_ragged_batch([5, 9, 3] * n_br, grids * n_br, temb_rows=[0, 1, 2] * n_br)
    assert rb.s_imgs == [302, 142, 125] * n_br
    assert lay["lat_off"] == [0, 272, 344, 408] and lay["total_rows"] == 408
    assert lay["item_off"] == rb.img_offsets == ([0, 302, 444, 569, 871, 1013, 1138] if do_cfg else [0, 302, 444, 569])
    q = lay["reqs"]
    assert q.dtype == CFG_EULER_REQ_DTYPE and q.dtype.itemsize == ctypes.sizeof(N.CfgEulerReq) == 32
    assert [(n, q.dtype.fields[n][1]) for n in q.dtype.names] == [(n, getattr(N.CfgEulerReq, n).offset) for n, _ in N.CfgEulerReq._fields_]
    assert q["lat_row"].tolist() == [0, 272, 344] and q["rows"].tolist() == S
    assert q["pos_row"].tolist() == [0, 302, 444]
    assert q["neg_row"].tolist() == ([569, 871, 1013] if do_cfg else [-1, -1, -1])
    assert q["dst_row"].tolist() == ([[0, 569], [302, 871], [444, 1013]] if do_cfg else [[0, -1], [302, -1], [444, -1]])
    assert q["dt_index"].tolist() == [0, 1, 2]
    assert q["cfg_scale"].tolist() == [2.5, 4.0, 3.0]
    # the words the device sees: eight int32 per request, the scale as its fp32 bits
    words = q.view("<i4").reshape(3, 8)
    assert words[1].tolist()[:7] == [272, 72, 302, 871 if do_cfg else -1, 302, 871 if do_cfg else -1, 1]
    assert words[1, 7] == np.float32(4.0).view(np.int32)
    # what the kernel may touch: target rows only — every condition row of lat_in / pred lies outside all [first, first + rows)
    touched = np.zeros(lay["item_off"][-1], bool)
    for r in range(3):
        for first in [q["pos_row"][r]] + ([q["neg_row"][r]] if do_cfg else []):
            assert not touched[first:first + S[r]].any()
            touched[first:first + S[r]] = True
    for i in range(3 * n_br):
        o0, o1, s = lay["item_off"][i], lay["item_off"][i + 1], S[i % 3]
        assert touched[o0:o0 + s].all() and not touched[o0 + s:o1].any()
    with pytest.raises(ValueError):
        ragged_step_descriptors([1] * 65, [0] * 65, True, [1.0] * 65)
    with pytest.raises(ValueError):
        ragged_step_descriptors([4, 0], [0, 0], True, [1.0, 1.0])


# ---------------------------------------------------------------------------------------------------------------- 4
def test_batcher_orders_and_admits_by_total_rows():
    from _fake_pipeline import FakePipeline
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest
    from vllm_omni_amd.diffusion.step_batcher import ContinuousStepBatcher

    cond_rows = {"a": 70, "b": 30, "c": 300}

    class EditFake(FakePipeline):
        def resolve_request(self, req, index=0):
            out = super().resolve_request(req, index)
            for sm in out:
                sm["cond"] = torch.zeros(cond_rows[req.extra["tag"]], 4)
            return out

        @staticmethod
        def batch_key(a):
            return ("mixed_edit", a.sample["do_cfg"])

    def req(tag, hw):
        return OmniDiffusionRequest(height=hw, width=hw, num_inference_steps=1, seed=1, prompt_embeds=torch.ones(1, 3, 8),
                                    output_type="latent", extra={"tag": tag})

    def groups(**cfg):
        b = ContinuousStepBatcher(EditFake(OmniDiffusionConfig(max_step_batch=8, mixed_step_batch=True, **cfg)))
        for tag, hw in (("a", 128), ("b", 256), ("c", 64)):          # target rows 64, 256, 16
            b.add(req(tag, hw), tag)
        return [a.tag for a in b.next_group()]

    # total rows a 134, b 286, c 316: with the flag the group is ordered by them, without it by the target rows as before
    assert groups(mixed_step_batch_edit=True) == ["c", "b", "a"]
    assert groups() == ["b", "a", "c"]
    # the token budget counts condition rows with the flag: a + b = 420 fit into 450, c (316 more) does not; without it the
    # target rows alone are counted (64 + 256 + 16 = 336)
    assert groups(mixed_step_batch_edit=True, max_step_tokens=450) == ["b", "a"]
    assert groups(max_step_tokens=450) == ["b", "a", "c"]


# ---------------------------------------------------------------------------------------------------------------- 5
def test_new_entry_point_is_bound_beside_prototypes():
    from vllm_omni_amd import _native as N

    name = "omni_cfg_euler_step_ragged"
    assert N.ABI_VERSION == 14
    assert name not in N.PROTOTYPES and name in N.FEATURE_PROTOTYPES
    res, args, bit = N.FEATURE_PROTOTYPES[name]
    assert res is ctypes.c_int and len(args) == 14 and bit == N.FEATURE_CFG_EULER_RAGGED == 4
    lib = N.lib()                                                        # loads without a GPU
    assert lib.omni_abi_version() == 14
    assert N.features() & N.FEATURE_CFG_EULER_RAGGED
    fn = getattr(lib, name)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(args)
    assert fn(None, 1, None, 1, None, 1, None, 1, 1, 64, None, 1, 1, None) == -1       # bound: answers with a status, no launch
    # the exported object is a pointer to the function (the exported functions of ABI v14 are what they were)
    assert ctypes.c_void_p.in_dll(ctypes.CDLL(N.LIB_PATH), name).value
