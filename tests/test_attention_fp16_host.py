"""CPU: fp16 at the attention plug-in point (CDNA4_FLASH -> omni_flash_attn_general with omni_attn_params.elem_type) and a
`dtype` that is honoured or refused, never ignored.

  * ABI: `elem_type` sits in the four bytes that were padding behind `mask_type` — the C compiler and the ctypes mirror agree, the
    struct's size and the appended v14 fields do not move; `omni_features` is bound with a non-status restype.
  * `OmniDiffusionConfig.dtype` takes the reference's strings (vllm_omni/diffusion/data.py:418-436).
  * `CDNA4FlashImpl.forward` validates dtypes before it touches the library.
  * The fused Qwen-Image path (worker, the four pipelines) refuses a non-bf16 config at construction.
  * The bf16 instances of flash_attn_general_kernel are, instruction for instruction, what they were before the kernel was
    templated on the element type (compared against the previous commit's source when git can show it).
"""
import ctypes
import logging
import os
import re
import subprocess
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vllm_omni_amd", "csrc")


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_elem_type_sits_in_the_former_padding_of_omni_attn_params(tmp_path):
    from vllm_omni_amd import _native as N

    src = tmp_path / "attn_f16_abi.c"
    src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "omni_cdna4.h"
int main(void) {
  omni_attn_params p = {0};
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %u\\n", sizeof(omni_attn_params), offsetof(omni_attn_params, mask_type),
         offsetof(omni_attn_params, elem_type), offsetof(omni_attn_params, mask_stride_b), offsetof(omni_attn_params, qk_int8),
         offsetof(omni_attn_params, out_k32_rows), offsetof(omni_attn_params, workspace),
         offsetof(omni_attn_params, workspace_bytes), offsetof(omni_attn_params, item_skip), OMNI_ELEM_BF16 + p.elem_type,
         OMNI_ELEM_F16, OMNI_FEATURE_ATTN_F16);
  return 0;
}
''')
    exe = tmp_path / "attn_f16_abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    A = N.AttnParams
    assert got[:9] == [ctypes.sizeof(A), A.mask_type.offset, A.elem_type.offset, A.mask_stride_b.offset, A.qk_int8.offset,
                       A.out_k32_rows.offset, A.workspace.offset, A.workspace_bytes.offset, A.item_skip.offset]
    assert got[9:] == [N.ELEM_BF16, N.ELEM_F16, N.FEATURE_ATTN_F16] == [0, 1, 1]
    # former padding: mask_type ends at 124, the strides start at 128; nothing else moves
    assert A.mask_type.offset == 120 and A.elem_type.offset == A.mask_type.offset + 4
    assert A.mask_stride_b.offset == A.elem_type.offset + 4 == 128
    # the size the struct had before the field existed: the same fields without it, laid out by the same rules
    before = type("Before", (ctypes.Structure,), {"_fields_": [f for f in A._fields_ if f[0] != "elem_type"]})
    assert ctypes.sizeof(A) == ctypes.sizeof(before) == got[0]
    for name in ("mask_stride_b", "qk_int8", "out_k32_rows", "workspace", "workspace_bytes", "item_skip"):
        assert getattr(A, name).offset == getattr(before, name).offset, name
    assert N.ABI_VERSION == 14
    assert N.AttnParams().elem_type == 0                       # a zeroed struct asks for bf16


def test_omni_features_is_bound_and_is_not_a_status_function():
    from vllm_omni_amd import _native as N

    assert "omni_features" in N.PROTOTYPES
    res, args = N.PROTOTYPES["omni_features"]
    assert res is not ctypes.c_int and res is ctypes.c_uint32 and args == []
    assert "omni_features" in N.OPTIONAL_SYMBOLS               # a library of the same ABI version may lack it
    assert os.path.exists(N.LIB_PATH), "run __graft_entry__.build() first"
    dll = ctypes.CDLL(N.LIB_PATH)                              # loads without a GPU; no compute call is made
    dll.omni_features.restype = ctypes.c_uint32
    assert dll.omni_features() & N.FEATURE_ATTN_F16
    assert N.features() & N.FEATURE_ATTN_F16


def test_features_of_a_library_without_the_symbol_is_zero(monkeypatch):
    from vllm_omni_amd import _native as N

    monkeypatch.setattr(N, "lib", lambda: types.SimpleNamespace())
    assert N.features() == 0


def test_ops_refuses_dtypes_before_any_pointer_is_taken():
    from vllm_omni_amd import _native as N
    from vllm_omni_amd import ops

    cu = torch.tensor([0, 4], dtype=torch.int32)
    h, b, f = (torch.zeros(4, 64, dtype=d) for d in (torch.float16, torch.bfloat16, torch.float32))
    with pytest.raises(N.OmniNativeError, match=r"share one dtype.*float16.*bfloat16"):
        ops.flash_attn_general(h, b, b, cu, cu, 1, 1, 4, 4, 0.125)
    with pytest.raises(N.OmniNativeError, match=r"share one dtype.*float32"):
        ops.flash_attn_general(f, f, f, cu, cu, 1, 1, 4, 4, 0.125)
    with pytest.raises(N.OmniNativeError, match=r"share one dtype"):
        ops.flash_attn_general(h, h, h, cu, cu, 1, 1, 4, 4, 0.125, out=torch.zeros(4, 64, dtype=torch.bfloat16))
    # one dtype, CPU tensors: the dtype check passes and the device check (the first pointer) is what fires
    with pytest.raises(N.OmniNativeError, match="must live on the GPU"):
        ops.flash_attn_general(h, h, h, cu, cu, 1, 1, 4, 4, 0.125)
    # every other wrapper stays bf16-strict
    with pytest.raises(N.OmniNativeError):
        ops.flash_attn_varlen(h, h, h, cu, 1, 4, 0.125)


def test_ops_refuses_fp16_on_a_library_without_the_feature_bit(monkeypatch):
    from vllm_omni_amd import _native as N
    from vllm_omni_amd import ops

    monkeypatch.setattr(N, "features", lambda: 0)
    cu = torch.tensor([0, 4], dtype=torch.int32)
    h = torch.zeros(4, 64, dtype=torch.float16)
    with pytest.raises(N.OmniNativeError, match="OMNI_FEATURE_ATTN_F16"):
        ops.flash_attn_general(h, h, h, cu, cu, 1, 1, 4, 4, 0.125)


# ---------------------------------------------------------------------------------------------------------------- config
@pytest.mark.parametrize("text,want", [("auto", torch.bfloat16), ("bfloat16", torch.bfloat16), ("bf16", torch.bfloat16),
                                       ("float16", torch.float16), ("fp16", torch.float16), ("half", torch.float16),
                                       ("float32", torch.float32), ("fp32", torch.float32), ("float", torch.float32),
                                       ("FP16", torch.float16), ("Half", torch.float16)])
def test_config_coerces_the_reference_dtype_strings(text, want):
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig

    assert OmniDiffusionConfig(dtype=text).dtype is want


def test_config_unknown_dtype_string_warns_and_gives_bf16(caplog):
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig

    with caplog.at_level(logging.WARNING):
        cfg = OmniDiffusionConfig(dtype="float8_e9m9")
    assert cfg.dtype is torch.bfloat16
    assert any("float8_e9m9" in r.getMessage() for r in caplog.records)
    # construction stays permissive for torch dtypes: plug-in users pass this config with fp16
    assert OmniDiffusionConfig(dtype=torch.float16).dtype is torch.float16
    assert OmniDiffusionConfig().dtype is torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------- backend
def _impl(H=2, dh=64, **kw):
    from vllm_omni_amd.diffusion.attention.backends.cdna4_flash import CDNA4FlashBackend

    return CDNA4FlashBackend.get_impl_cls()(num_heads=H, head_size=dh, softmax_scale=0.125, **kw)


def test_backend_validates_dtypes_before_touching_the_library(monkeypatch):
    from vllm_omni_amd import _native as N

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(N, "lib", no_library)
    q = torch.zeros(1, 5, 2, 64)
    with pytest.raises(ValueError, match=r"bfloat16 / torch\.float16.*float32"):
        _impl().forward(q, q, q, None)
    with pytest.raises(ValueError, match=r"bfloat16 / torch\.float16.*q torch\.float16.*k torch\.bfloat16"):
        _impl().forward(q.half(), q.bfloat16(), q.half(), None)
    with pytest.raises(ValueError, match=r"v torch\.float64"):
        _impl().forward(q.bfloat16(), q.bfloat16(), q.double(), None)


@pytest.mark.parametrize("dtype,tuned", [(torch.bfloat16, True), (torch.float16, False)])
def test_backend_dispatch_fp16_always_takes_the_general_kernel(monkeypatch, dtype, tuned):
    """No mask, head size 128, S_q == S_kv: bf16 keeps going to the tuned kernels, fp16 goes to the general one."""
    from vllm_omni_amd import ops

    calls = []
    monkeypatch.setattr(ops, "flash_attn_varlen", lambda q, *a, **k: calls.append("tuned") or torch.zeros_like(q))
    monkeypatch.setattr(ops, "flash_attn_general", lambda q, *a, **k: calls.append("general") or torch.zeros_like(q))
    q = torch.zeros(1, 6, 2, 128, dtype=dtype)
    out = _impl(2, 128).forward(q, q, q, None)
    assert calls == ["tuned" if tuned else "general"]
    assert out.shape == q.shape and out.dtype == dtype


# ---------------------------------------------------------------------------------------------------------------- fused path
def _fake_parts(layered=False):
    class QwenImageTransformer2DModel:
        teacache = None
        use_layer3d_rope = use_additional_t_cond = layered

    vae = types.SimpleNamespace(config=types.SimpleNamespace(latents_mean=[0.0] * 16, latents_std=[1.0] * 16), with_encoder=True)
    return dict(device="cpu", transformer=QwenImageTransformer2DModel(), vae=vae)


def _pipeline_classes():
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image_edit import QwenImageEditPipeline
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image_edit_plus import QwenImageEditPlusPipeline
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image_layered import QwenImageLayeredPipeline

    return [QwenImagePipeline, QwenImageEditPipeline, QwenImageEditPlusPipeline, QwenImageLayeredPipeline]


@pytest.mark.parametrize("which", range(4))
@pytest.mark.parametrize("dtype", ["half", torch.float16, torch.float32])
def test_fused_pipelines_refuse_a_dtype_they_cannot_compute_in(which, dtype):
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig

    cls = _pipeline_classes()[which]
    with pytest.raises(NotImplementedError, match=r"(?s)fused DiT / VAE kernels.*bf16.*attention plug-in point.*not be what was asked"):
        cls(od_config=OmniDiffusionConfig(dtype=dtype), **_fake_parts(layered=which == 3))


@pytest.mark.parametrize("which", range(4))
def test_fused_pipelines_construct_with_bf16_as_before(which):
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig

    cls = _pipeline_classes()[which]
    for cfg in (None, OmniDiffusionConfig(), OmniDiffusionConfig(dtype="bf16")):
        assert cls(od_config=cfg, **_fake_parts(layered=which == 3)).od_config.dtype is torch.bfloat16


def test_worker_refuses_a_dtype_the_fused_path_cannot_compute_in():
    from _fake_pipeline import FakePipeline
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.worker.gpu_worker import GPUWorker

    with pytest.raises(NotImplementedError, match=r"(?s)GPUWorker.*float16.*fused DiT / VAE kernels.*attention plug-in point"):
        GPUWorker(0, 0, OmniDiffusionConfig(dtype="half"), pipeline=FakePipeline())
    w = GPUWorker(0, 0, OmniDiffusionConfig(), pipeline=FakePipeline())
    assert w.od_config.dtype is torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------- kernel
def _kernel_bodies(asm_lines):
    """{mangled name: instruction lines} of every flash_attn_general_kernel instance, comments stripped, local labels
    renumbered (hipcc numbers them by the function's position in the file)."""
    out, fn = {}, None
    for line in asm_lines:
        m = re.match(r"^(_Z\w*flash_attn_general_kernel\w*):", line)
        if m:
            fn = m.group(1)
            out[fn] = []
            continue
        if fn is None:
            continue
        if line.startswith(".Lfunc_end"):
            fn = None
            continue
        code = re.sub(r"\.LBB\d+_", ".LBBn_", line.split(";")[0]).rstrip()
        if code:
            out[fn].append(code.replace(fn, "SYM"))
    return out


def test_fp16_instances_use_the_fp16_mfma_and_round_to_nearest_even():
    from vllm_omni_amd.csrc import build as B

    bodies = _kernel_bodies(B.device_asm(os.path.join(CSRC, "attention_general.hip")))
    f16 = {k: "\n".join(v) for k, v in bodies.items() if "Lb1E" in k}
    bf16 = {k: "\n".join(v) for k, v in bodies.items() if "Lb0E" in k}
    assert len(f16) == 2 and len(bf16) == 2, sorted(bodies)
    for name, text in f16.items():
        dh = 128 if "Li128E" in name else 64
        assert text.count("v_mfma_f32_32x32x16_f16") == 2 * dh // 16 + 4 * dh // 32, name      # S^T and O^T, both on the fp16 MFMA
        assert "v_mfma_f32_32x32x16_bf16" not in text and "bf16_f32" not in text, name
        assert "v_cvt_pk_f16_f32" in text or "v_cvt_f16_f32" in text, name                     # nearest even
        assert "pkrtz" not in text, name                                                        # ... never the truncating pack
    for name, text in bf16.items():
        assert "_f16" not in text, name


def test_bf16_instances_are_instruction_for_instruction_what_they_were():
    """Templating the kernel on the element type cost the bf16 instances nothing: a bf16 instance and the fp16 instance of
    the same head size are the SAME instruction stream — same registers, same order — except for the two things the element
    policy (attention_common.h attn_elem) names: the 32x32x16 MFMA and the nearest-even pack.  (When the template was
    introduced this was checked against the untemplated kernel of the commit before; that comparison needs that commit and
    cannot outlive a change of the kernel, this one holds for every later form of it.)"""
    from vllm_omni_amd.csrc import build as B

    bodies = _kernel_bodies(B.device_asm(os.path.join(CSRC, "attention_general.hip")))

    def as_bf16(lines):
        return [ln.replace("v_mfma_f32_32x32x16_f16", "v_mfma_f32_32x32x16_bf16").replace("v_cvt_pk_f16_f32", "v_cvt_pk_bf16_f32")
                for ln in lines]

    for dh in (64, 128):
        a = [v for k, v in bodies.items() if f"Li{dh}ELb0E" in k]
        b = [v for k, v in bodies.items() if f"Li{dh}ELb1E" in k]
        assert len(a) == 1 and len(b) == 1
        assert any("v_cvt_pk_f16_f32" in ln for ln in b[0]) and any("v_mfma_f32_32x32x16_f16" in ln for ln in b[0])
        assert a[0] == as_bf16(b[0]), f"dh {dh}: the bf16 and fp16 instances differ in more than the MFMA and the pack"
