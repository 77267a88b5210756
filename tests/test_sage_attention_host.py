"""SAGE_ATTN on the host: the backend selector entry, what the backend refuses, the ABI mirrors of the appended fields, and the
host model of the int8 algorithm (tests/_sage_model.py) against fp32 SDPA — the accuracy premise of the feature."""
import ctypes
import os
import subprocess

import pytest
import torch

import _sage_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1.5e-2          # fixed rel-L2 bar of the int8 attention vs fp32 SDPA


@pytest.fixture
def sage_env(monkeypatch):
    from vllm_omni_amd.diffusion.attention.selector import get_attn_backend

    monkeypatch.setenv("DIFFUSION_ATTENTION_BACKEND", "SAGE_ATTN")
    get_attn_backend.cache_clear()
    yield get_attn_backend
    get_attn_backend.cache_clear()


def test_selector_offers_sage_attn(sage_env):
    be = sage_env(-1)
    assert be.get_name() == "SAGE_ATTN"
    assert be.get_supported_head_sizes() == [64, 128]
    assert be.get_impl_cls().__name__ == "SageAttentionImpl"


def test_backend_refuses_what_it_cannot_honour(sage_env):
    from vllm_omni_amd.diffusion.attention.backends.abstract import AttentionMetadata

    impl_cls = sage_env(-1).get_impl_cls()
    with pytest.raises(ValueError):
        impl_cls(num_heads=2, head_size=96, softmax_scale=96 ** -0.5)
    with pytest.raises(ValueError):
        impl_cls(num_heads=2, head_size=64, softmax_scale=0.125, causal=True)
    impl = impl_cls(num_heads=2, head_size=64, softmax_scale=0.125, causal=False, num_kv_heads=None, prefix="attn")
    q = torch.zeros(1, 8, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="mask"):
        impl.forward(q, q, q, AttentionMetadata(attn_mask=torch.ones(1, 1, 8, 8, dtype=torch.bool)))
    with pytest.raises(ValueError, match="bf16"):
        h = q.half()
        impl.forward(h, h, h)


class _Captured(Exception):
    pass


def _model_qkv(grid, T, seed=7):
    """q / k / v exactly as the model hands them to the attention: the oracle's full-width layer (the committed fixture
    dit_fullwidth_1layer_fp32's weights) up to its joint attention — q/k RMS-normed with the model's norm weights, RoPE applied,
    joint order [text ; image] — rounded to bf16 like the product's activations.  Returns [rows, H, dh] each."""
    import qwen_image_oracle as O
    from _util import golden_params, load_golden

    z, meta, c = load_golden("dit_fullwidth_1layer_fp32")
    P = golden_params(c)
    got = {}
    orig = O.sdpa_nhd

    def tap(q, k, v, scale):
        got.update(q=q, k=k, v=v)
        raise _Captured

    O.sdpa_nhd = tap
    try:
        g = torch.Generator().manual_seed(seed)
        gh, gw = grid
        if (gh, gw) == tuple(c["grid"]):
            lat, txt, sig = (torch.from_numpy(z[n]).float() for n in ("latents", "prompt_embeds", "sigma"))
        else:
            lat, txt, sig = torch.randn(1, gh * gw, 64, generator=g), torch.randn(1, T, c["joint"], generator=g), torch.tensor([0.7])
        with pytest.raises(_Captured):
            O.dit_forward(P, lat, txt, sig, (1, gh, gw), num_heads=c["heads"])
    finally:
        O.sdpa_nhd = orig
    return tuple(got[n][0].bfloat16() for n in ("q", "k", "v"))


@pytest.mark.parametrize("grid,T,heads", [((16, 16), 16, 24), ((64, 64), 64, 4)], ids=["fixture_272_rows", "1024sq_4160_rows"])
def test_host_model_on_the_models_own_q_k_within_the_bar(grid, T, heads):
    """The accuracy premise on q/k taken from the model path (not on a synthetic distribution): the host model of the int8
    algorithm against fp32 SDPA at the fixture's own shape and at the 1024^2 joint length."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    q, k, v = (t[:, :heads].contiguous() for t in _model_qkv(grid, T))
    cu = [0, q.shape[0]]
    sc = M.default_scale(q.shape[-1])
    ref = M.sdpa_fp32(q, k, v, cu, cu, sc)
    err = M.rel_l2(M.sage_attention(q, k, v, cu, cu, sc).bfloat16(), ref)
    print(f"model q/k, {q.shape[0]} rows, {heads} heads: int8 rel_l2 {err:.3e} (bar {BAR})")
    assert err <= BAR               # measured 7.9e-3 (272 rows), 5.6e-3 (4160 rows)


def test_smoothing_makes_the_result_independent_of_a_shared_key_offset():
    """Adding one vector to every key of an item leaves exact attention unchanged.  With smoothing the int8 result is unchanged
    too (to the key mean's rounding); without it, the offset eats the int8 range of K and the error leaves the bar.  The offset
    is 6x the keys' RMS, in a random direction per head — the claim tested is the invariance, not a particular offset size."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    q, k, v = (t[:, :8].contiguous() for t in _model_qkv((16, 16), 16))
    cu = [0, q.shape[0]]
    sc = M.default_scale(q.shape[-1])
    ref = M.sdpa_fp32(q, k, v, cu, cu, sc)
    g = torch.Generator().manual_seed(11)
    rms = k.float().pow(2).mean(dim=(0, 2), keepdim=True).sqrt()                       # per head
    ko = (k.float() + 6.0 * rms * torch.randn(1, k.shape[1], k.shape[2], generator=g)).bfloat16()
    ref_o = M.sdpa_fp32(q, ko, v, cu, cu, sc)          # the exact result on the offset keys as they are stored (bf16)
    base = M.rel_l2(M.sage_attention(q, k, v, cu, cu, sc).bfloat16(), ref)
    with_off = M.rel_l2(M.sage_attention(q, ko, v, cu, cu, sc).bfloat16(), ref_o)
    raw = M.rel_l2(M.sage_attention(q, ko, v, cu, cu, sc, smooth=False).bfloat16(), ref_o)
    print(f"int8 rel_l2: model q/k {base:.3e}, + shared key offset {with_off:.3e}, same without smoothing {raw:.3e}")
    assert with_off <= BAR and abs(with_off - base) <= 0.25 * base
    assert raw > BAR


def test_host_model_quantisation_rules():
    x = torch.zeros(130, 1, 8)
    x[:64] = torch.linspace(-2, 2, 64 * 8).view(64, 1, 8)
    x[64:128, 0, 3] = 0.5                            # block 1: one non-zero channel
    x8, sc = M.quant_blocks(x)                       # block 2 (rows 128, 129): all zero
    assert sc.shape == (3, 1)
    assert float(sc[0, 0]) == pytest.approx(2 / 127) and float(sc[2, 0]) == 1.0
    assert int(x8[:64].abs().max()) == 127 and int(x8[128:].abs().max()) == 0
    assert int(x8[64, 0, 3]) == 127
    # smoothing leaves the softmax unchanged in exact arithmetic
    q, k, v = M.make_qkv(70, 70, 1, 64, seed=3)
    cu = [0, 70]
    km = k.double().mean(0)
    a = M.sdpa_fp32(q.double(), k.double(), v.double(), cu, cu, 0.125)
    b = M.sdpa_fp32(q.double(), k.double() - km, v.double(), cu, cu, 0.125)
    assert M.rel_l2(a, b) < 1e-5


def test_appended_abi_fields_match_the_c_compiler(tmp_path):
    from vllm_omni_amd import _native as N

    src = tmp_path / "abi14.c"
    src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "omni_cdna4.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(omni_attn_params), offsetof(omni_attn_params, qk_int8),
         offsetof(omni_attn_params, out_k32_rows), offsetof(omni_attn_params, workspace),
         offsetof(omni_attn_params, workspace_bytes), sizeof(omni_dit_batch), offsetof(omni_dit_batch, attn_qk_int8),
         offsetof(omni_dit_batch, rope_cos), offsetof(omni_dit_batch, mod_table));
  return 0;
}
''')
    exe = tmp_path / "abi14"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    A, D = N.AttnParams, N.DitBatch
    assert got == [ctypes.sizeof(A), A.qk_int8.offset, A.out_k32_rows.offset, A.workspace.offset, A.workspace_bytes.offset,
                   ctypes.sizeof(D), D.attn_qk_int8.offset, D.rope_cos.offset, D.mod_table.offset]
    # the int8 flag of the DiT batch sits in former padding: the descriptor's size and every other offset are unchanged
    assert D.attn_qk_int8.offset == D.txt_pos_end.offset + 4 and D.rope_cos.offset == D.attn_qk_int8.offset + 4
    assert N.ABI_VERSION == 14


def test_quant_workspace_size_is_exported():
    from vllm_omni_amd import _native as N
    from vllm_omni_amd import ops

    n = ops.attn_quant_workspace_bytes(2, 4, 4, 128, 100, 100)
    # int8 q and k (2 items x 100 rows x 512), two block-scale tables and the key means, each piece 256-byte aligned
    assert n == 102400 + 102400 + 256 + 256 + 4096
    assert ops.attn_quant_workspace_bytes(2, 4, 4, 96, 100, 100) == 0
    assert "omni_attn_quant_workspace_bytes" in N.PROTOTYPES
