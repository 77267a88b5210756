"""CPU: omni_lora_merge's documented statuses (include/omni_cdna4.h), each answered BEFORE any launch - the pointers are made-up
addresses that are never dereferenced - and the layout of omni_lora_merge_params against what gcc sees."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, UNSUPPORTED, LAUNCH, ALIGN = 0, -1, -2, -3, -4
P = 0x7F0000010000          # a "device pointer": 16-byte aligned, never dereferenced


def _params(**kw):
    from vllm_omni_amd import _native as N

    p = N.LoraMergeParams()
    vals = dict(w_base=P, w_out=P + 0x100000, up=P + 0x200000, down=P + 0x300000, N=9216, K=3072, R=64, row0=3072, rows=3072,
                w_k32_blocked=1, ldw=3072, scale=1.0)
    vals.update(kw)
    for k, v in vals.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw,want", [
    (dict(w_base=None), BAD_ARG), (dict(w_out=None), BAD_ARG), (dict(up=None), BAD_ARG), (dict(down=None), BAD_ARG),
    (dict(K=3080), UNSUPPORTED), (dict(K=48, w_k32_blocked=0, ldw=48), UNSUPPORTED),
    (dict(R=0), UNSUPPORTED), (dict(R=257), UNSUPPORTED), (dict(R=-3), UNSUPPORTED),
    (dict(rows=0), BAD_ARG), (dict(rows=-1), BAD_ARG), (dict(row0=-1), BAD_ARG), (dict(row0=6145), BAD_ARG),
    (dict(row0=0, rows=9217), BAD_ARG), (dict(row0=9216, rows=1), BAD_ARG),
    (dict(w_base=P + 8), ALIGN), (dict(w_out=P + 2), ALIGN), (dict(up=P + 4), ALIGN), (dict(down=P + 8), ALIGN),
    (dict(w_k32_blocked=0, ldw=3076), ALIGN),                       # a row pitch that is not 16-byte aligned
    (dict(w_k32_blocked=0, ldw=3040), BAD_ARG),                     # rows would overlap
    (dict(w_k32_blocked=2), BAD_ARG),
    # the order a binder sees: null before shape before range before alignment
    (dict(w_base=None, K=3080), BAD_ARG), (dict(K=3080, up=P + 4), UNSUPPORTED), (dict(R=300, rows=0), UNSUPPORTED),
    (dict(rows=0, up=P + 4), BAD_ARG),
])
def test_lora_merge_statuses_before_any_launch(kw, want):
    from vllm_omni_amd import _native as N

    assert N.features() & N.FEATURE_LORA_MERGE
    p = _params(**kw)
    assert N.lib().omni_lora_merge(C.byref(p), None) == want, kw


def test_lora_merge_null_params():
    from vllm_omni_amd import _native as N

    assert N.lib().omni_lora_merge(None, None) == BAD_ARG


def test_lora_merge_params_layout_matches_gcc(tmp_path):
    from vllm_omni_amd import _native as N

    fields = [f for f, _ in N.LoraMergeParams._fields_]
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "omni_cdna4.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(omni_lora_merge_params));\n'
                   + "".join(f'  printf(" %zu", offsetof(omni_lora_merge_params, {f}));\n' for f in fields)
                   + '  printf(" %u\\n", OMNI_FEATURE_LORA_MERGE);\n  return 0;\n}\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(N.LoraMergeParams)
    assert out[1:-1] == [getattr(N.LoraMergeParams, f).offset for f in fields]
    assert out[-1] == N.FEATURE_LORA_MERGE == 8
