"""CPU: the SAGE_ATTN attention kernel (csrc/attention_sage.hip) as the code-object loader sees it — its innermost KV loop
issues the int8 MFMA, and its register allocation fits the plan DESIGN.md states: at most 256 registers per lane (VGPR + AGPR),
i.e. two waves per SIMD (two 4-wave workgroups per CU), with no scratch anywhere."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "vllm_omni_amd", "csrc", "attention_sage.hip")


@pytest.fixture(scope="module")
def asm():
    from vllm_omni_amd.csrc import build as B

    return B.device_asm(SRC)


def _fn_bodies(asm_lines):
    """{function: its lines after the label} — the same split build.mfma_loops makes (its loop start / end index these)."""
    out, fn = {}, None
    for line in asm_lines:
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            fn = m.group(1)
            out[fn] = []
        elif fn is not None:
            out[fn].append(line)
    return out


def test_innermost_loop_issues_the_int8_mfma(asm):
    from vllm_omni_amd.csrc import build as B

    loops = {k: v for k, v in B.mfma_loops(asm).items() if "sage_attn_fwd_kernel" in k}
    assert len(loops) == 2, sorted(loops)                    # dh 64 and dh 128
    bodies = _fn_bodies(asm)
    for fn, lps in loops.items():
        inner = [lp for lp in lps if lp["innermost"]]
        assert inner and all(lp["scratch"] == 0 for lp in lps), (fn, lps)
        text = "\n".join("\n".join(bodies[fn][lp["start"]:lp["end"] + 1]) for lp in inner)
        assert "v_mfma_i32_32x32x32_i8" in text, fn          # Q K^T in int8
        assert "v_mfma_f32_32x32x16_bf16" in text, fn        # P V in bf16


def test_register_plan_two_waves_per_simd(asm):
    from vllm_omni_amd.csrc import build as B

    res = {k: r for k, r in B.kernel_resources(asm).items() if "sage_" in k}
    assert len(res) == 6, sorted(res)                        # kmean, quant, attention x (dh 64, dh 128)
    for k, r in res.items():
        alloc = (r["vgpr_count"] + 7) // 8 * 8               # unified VGPR + AGPR file, granule 8
        assert r["private_segment_fixed_size"] == 0, k       # no scratch
        if "sage_attn_fwd_kernel" in k:
            assert alloc <= 256, (k, alloc)                  # 512 / 256 = 2 waves per SIMD
