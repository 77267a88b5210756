#!/usr/bin/env python3
"""Builds libomni_cdna4.so (the C-ABI HIP library) for gfx950, in-tree, with plain hipcc.

    python vllm_omni_amd/csrc/build.py [--force]

One `hipcc -c` per .hip translation unit (run concurrently), then one `hipcc -shared` link.  hipcc
cross-compiles without a GPU, so this also runs in the GPU-less authoring container.  The built .so is
git-ignored but travels with gpurun snapshots.
"""
from __future__ import annotations

import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = ["gemm.hip", "attention.hip", "attention_w64.hip", "attention_general.hip", "attention_sage.hip", "elementwise.hip", "vae.hip", "dit_forward.hip",
           "lora.hip", "text_forward.hip", "vision_forward.hip", "text_decode.hip"]
LIB = os.path.join(os.path.dirname(HERE), "libomni_cdna4.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++20", "-fPIC", "-fno-gpu-rdc", "-fvisibility=hidden", "-Wno-unused-result"]


def _stale(target: str, deps: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


_AGPR = re.compile(r"\ba(\d+|\[\d+(:\d+)?\])")


def agpr_violations(asm_lines) -> dict[str, list[tuple[int, str]]]:
    """{kernel: [(line, instruction), ...]} for every function of a device-assembly listing that carries the OMNI_OWNS_AGPRS
    marker and yet has compiler-generated instructions (outside #ASMSTART/#ASMEND) naming an AGPR."""
    out: dict[str, list[tuple[int, str]]] = {}
    fn, owned, inasm, hits = None, False, False, []
    for n, line in enumerate(asm_lines, 1):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            fn, owned, inasm, hits = m.group(1), False, False, []
            continue
        if "#ASMSTART" in line:
            inasm = True
        elif "#ASMEND" in line:
            inasm = False
        elif inasm:
            owned = owned or "omni: AGPRs owned by asm" in line
        else:
            code = line.split(";")[0].strip()
            if code and not code.startswith(".") and _AGPR.search(code):
                hits.append((n, code))
        if line.startswith(".Lfunc_end") and fn is not None:
            if owned and hits:
                out[fn] = hits
            fn, hits = None, []
    return out


def mfma_loop_lane_spills(asm_lines) -> dict[str, int]:
    """{function: max number of SGPR-spill lane operations (v_writelane / v_readlane) inside any loop that issues MFMAs}.

    hipcc spills SGPRs to VGPR lanes (no scratch) when a kernel runs out of scalar registers; in an epilogue that is free, inside
    the K-loop it is per-iteration VALU work on the MFMA issue port.  Round-3 verdict item 16 asked which it is for the GEMM
    kernels: `tests/test_host_logic.py` compiles gemm.hip to assembly and asserts 0 for every gemm_bf16_pp_kernel instance (the
    ring FALLBACK kernel does spill inside its loop; it runs only for shapes the ping-pong kernel does not take)."""
    out: dict[str, int] = {}
    fn, body = None, []
    for line in asm_lines:
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            fn, body = m.group(1), []
            continue
        if fn is None:
            continue
        if line.startswith(".Lfunc_end"):
            labels = {}
            for j, ln in enumerate(body):
                lm = re.match(r"^(\.LBB\d+_\d+):", ln)
                if lm:
                    labels[lm.group(1)] = j
            worst = 0
            for j, ln in enumerate(body):
                bm = re.search(r"\bs_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
                if bm and labels.get(bm.group(1), j) < j:          # backward branch = a loop
                    loop = body[labels[bm.group(1)]:j]
                    if any("s_endpgm" in x for x in loop):          # an out-of-line block behind the kernel's end that jumps back
                        continue                                   # into it (see mfma_loops): a backward branch, not a loop
                    if any("v_mfma" in x for x in loop):
                        worst = max(worst, sum(1 for x in loop if re.search(r"\bv_(write|read)lane_b32", x)))
            out[fn] = worst
            fn = None
        else:
            body.append(line)
    return out


def kernel_resources(asm_lines) -> dict[str, dict[str, int]]:
    """{kernel symbol: {vgpr_count, agpr_count, sgpr_count, vgpr_spill_count, sgpr_spill_count, private_segment_fixed_size,
    group_segment_fixed_size, max_flat_workgroup_size}} from the `.amdgpu_metadata` block of a device-assembly listing — what
    the code-object loader will see.  `tests/test_kernel_resources.py` holds every product kernel to its budget (no scratch,
    the occupancy its launch bounds promise) without a GPU."""
    out: dict[str, dict[str, int]] = {}
    inmeta, cur = False, None
    keys = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
            "group_segment_fixed_size", "max_flat_workgroup_size")
    for line in asm_lines:
        if ".amdgpu_metadata" in line and ".end_amdgpu_metadata" not in line:
            inmeta = True
            continue
        if ".end_amdgpu_metadata" in line:
            inmeta = False
        if not inmeta:
            continue
        if re.match(r"^\s*- \.agpr_count:", line) or re.match(r"^\s*- \.args:", line):      # first key of a kernel entry
            if cur and "name" in cur:
                out[cur.pop("name")] = cur
            cur = {}
        m = re.match(r"^\s*(?:- )?\.(\w+):\s*(\S+)\s*$", line)
        if m and cur is not None:
            k, v = m.group(1), m.group(2)
            if k == "name" and "name" not in cur and v.startswith("_Z"):
                cur["name"] = v
            elif k in keys and k not in cur:
                try:
                    cur[k] = int(v)
                except ValueError:
                    pass
    if cur and "name" in cur:
        out[cur.pop("name")] = cur
    return out


_ASM_CACHE: dict[tuple[str, float], list[str]] = {}


def device_asm(src: str) -> list[str]:
    """Device assembly listing of one translation unit (for the build checks and their tests); cached per (file, mtime) for
    the life of the process — several tests look at the same listing."""
    key = (os.path.abspath(src), os.path.getmtime(src))
    if key not in _ASM_CACHE:
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, "k.s")
            subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-S", src, "-o", out], check=True, stderr=subprocess.DEVNULL)
            with open(out) as f:
                _ASM_CACHE[key] = f.read().splitlines()
    return _ASM_CACHE[key]


def mfma_loops(asm_lines) -> dict[str, list[dict]]:
    """{function: [{"start", "end", "mfma", "scratch", "innermost"}, ...]} — every loop (backward branch) of a device-assembly
    listing that issues MFMAs, with the number of scratch (spill) accesses inside it.  `innermost`: no other MFMA loop lies
    inside — the K-loop / KV-loop proper, where a spill reload is per-iteration VMEM traffic whose `vmcnt` wait drains the
    LDS-DMA in flight (the VAE attention kernel ran 10x slower that way before its Q fragments moved to AGPRs)."""
    out: dict[str, list[dict]] = {}
    fn, body = None, []
    for line in asm_lines:
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            fn, body = m.group(1), []
            continue
        if fn is None:
            continue
        if not line.startswith(".Lfunc_end"):
            body.append(line)
            continue
        labels = {}
        for j, ln in enumerate(body):
            lm = re.match(r"^(\.LBB\d+_\d+):", ln)
            if lm:
                labels[lm.group(1)] = j
        loops = []
        for j, ln in enumerate(body):
            bm = re.search(r"\bs_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
            if bm and labels.get(bm.group(1), j) < j:
                a = labels[bm.group(1)]
                if any("s_endpgm" in x for x in body[a:j]):            # an out-of-line entry block behind the kernel's end that
                    continue                                          # jumps back into it: a backward branch, not a loop
                nm = sum(1 for x in body[a:j] if "v_mfma" in x)
                if nm:
                    loops.append({"start": a, "end": j, "mfma": nm,
                                  "scratch": sum(1 for x in body[a:j] if re.search(r"\b(scratch_|buffer_(load|store)\w* .*offen.*s\[0:3\])", x))})
        # several backward branches to ONE header are one natural loop (hipcc rotates loops: a conditional latch plus an
        # out-of-line block that jumps back): keep the widest extent per header
        widest: dict[int, dict] = {}
        for lp in loops:
            if lp["start"] not in widest or lp["end"] > widest[lp["start"]]["end"]:
                widest[lp["start"]] = lp
        loops = sorted(widest.values(), key=lambda d: (d["start"], d["end"]))
        for lp in loops:
            lp["innermost"] = not any(o is not lp and o["start"] >= lp["start"] and o["end"] <= lp["end"] for o in loops)
        if loops:
            out[fn] = loops
        fn = None
    return out


def check_agpr_ownership(src: str, verbose: bool = True) -> None:
    """A kernel that keeps its accumulators in literal `a[...]` registers inside asm statements (marker: OMNI_OWNS_AGPRS, the
    all-AGPR clobber statement of common.h) is only correct while hipcc itself never allocates an AGPR in it: under register
    pressure the allocator parks spilled VGPRs and constants there, silently overwriting the kernel's data (seen in round 3:
    one O^T register of the attention kernel corrupted only when a late rescale branch was taken).  There is no way to
    reserve them, so the build CHECKS: the device assembly of such a kernel must not name an AGPR outside the kernel's own
    asm statements.  Raises RuntimeError otherwise."""
    if "OMNI_OWNS_AGPRS" not in open(src).read():
        return
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-S", src, "-o", out], check=True, stderr=subprocess.DEVNULL)
        with open(out) as f:
            bad = agpr_violations(f)
    for fn, hits in bad.items():
        raise RuntimeError(f"{os.path.basename(src)}: hipcc allocated AGPRs in {fn}, which owns a[0:255] through asm "
                           f"({len(hits)} instructions, first: line {hits[0][0]}: {hits[0][1]}) - lower the VGPR pressure")
    if verbose:
        print(f"agpr ownership check: {os.path.basename(src)} ok", flush=True)


def build(force: bool = False, verbose: bool = True) -> str:
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    headers = [os.path.join(HERE, "common.h"), os.path.join(HERE, "attention_common.h"),
               os.path.join(HERE, "..", "..", "include", "omni_cdna4.h")]
    srcs = [os.path.join(HERE, s) for s in SOURCES if os.path.exists(os.path.join(HERE, s))]
    objs = [os.path.join(objdir, os.path.basename(s)[:-4] + ".o") for s in srcs]

    def compile_one(src, obj):
        if not force and not _stale(obj, [src] + headers):
            return
        cmd = [HIPCC, *FLAGS, "-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        check_agpr_ownership(src, verbose)

    with cf.ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        list(ex.map(compile_one, srcs, objs))
    if force or _stale(LIB, objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
