"""LoRA adapter files -> a merge plan for the Qwen-Image DiT (host only: no GPU, no native library).

The reference names LoRA in three config fields (data.py:280-286) and two commented lines (qwen_image_transformer.py:731-733) and
builds nothing behind them, so there is no implementation to mirror; the specification is the usual definition

    W' = W + (alpha / rank) * weight * lora_B @ lora_A          (lora_B = "up" [out, rank], lora_A = "down" [rank, in])

An adapter file is turned into `LoraAdapter.updates`: {(module, row0, rows): (up, down, scale)} with `module` the HF name of a
targetable linear of `QwenImageTransformer2DModel` as `load_weights` spells it (fused: `...attn.to_qkv`, `...attn.add_kv_proj`).
Split q / k / v keys become the row ranges idx * D of the fused matrix; a FUSED key is cut into the same three ranges (sharing its
`down`), so that split and fused spellings, and stacks of adapters that mix them, address identical (matrix, row range) keys.

`stack` folds several active adapters into ONE update per key - the device merge (`ops.lora_merge`) then reads every weight
element once, from the BASE value, and rounds it once, however many adapters are active.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field

import torch

MAX_RANK = 256                       # omni_lora_merge: R <= 256 (the stacked total)
BF16 = torch.bfloat16

# (fused module suffix, split module suffix, index of the D-row block): the table of QwenImageTransformer2DModel.load_weights
STACKED = ((".to_qkv", ".to_q", 0), (".to_qkv", ".to_k", 1), (".to_qkv", ".to_v", 2),
           (".add_kv_proj", ".add_q_proj", 0), (".add_kv_proj", ".add_k_proj", 1), (".add_kv_proj", ".add_v_proj", 2))
_PREFIXES = ("transformer.", "diffusion_model.")
# key suffix -> role.  Anything else (DoRA's lora_magnitude_vector, LoHa's hada_*, rank patterns ...) is refused by key name
_SUFFIXES = ((".lora_A.weight", "down"), (".lora_B.weight", "up"), (".lora_down.weight", "down"), (".lora_up.weight", "up"),
             (".alpha", "alpha"))


def target_shapes(num_layers: int, D: int, joint_dim: int, in_channels: int, out_packed: int) -> dict[str, tuple[int, int, bool]]:
    """{module: (N, K, k32_blockable)} of every linear an adapter may target: per layer the eight GEMM matrices (held K32-blocked
    by the native runner) and the two modulation linears, plus img_in, txt_in, proj_out, norm_out.linear and the two
    timestep-embedder linears (row-major)."""
    t: dict[str, tuple[int, int, bool]] = {}
    for i in range(num_layers):
        p = f"transformer_blocks.{i}."
        t[p + "attn.to_qkv"] = t[p + "attn.add_kv_proj"] = (3 * D, D, True)
        t[p + "attn.to_out.0"] = t[p + "attn.to_add_out"] = (D, D, True)
        for s in ("img_mlp", "txt_mlp"):
            t[p + s + ".net.0.proj"] = (4 * D, D, True)
            t[p + s + ".net.2"] = (D, 4 * D, True)
        t[p + "img_mod.1"] = t[p + "txt_mod.1"] = (6 * D, D, False)
    t["img_in"] = (D, in_channels, False)
    t["txt_in"] = (D, joint_dim, False)
    t["proj_out"] = (out_packed, D, False)
    t["norm_out.linear"] = (2 * D, D, False)
    t["time_text_embed.timestep_embedder.linear_1"] = (D, 256, False)
    t["time_text_embed.timestep_embedder.linear_2"] = (D, D, False)
    return t


def read_adapter(source) -> dict[str, torch.Tensor]:
    """An adapter's tensors by key: a `.safetensors` file, a `.pt` / `.bin` file (torch.load(weights_only=True)), or a dict."""
    if isinstance(source, dict):
        return dict(source)
    path = os.fspath(source)
    if path.endswith(".safetensors"):
        from safetensors import safe_open

        with safe_open(path, framework="pt", device="cpu") as f:
            return {k: f.get_tensor(k) for k in f.keys()}
    if path.endswith((".pt", ".bin", ".pth")):
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(sd, dict):
            raise ValueError(f"{path}: expected a dict of tensors, got {type(sd).__name__}")
        return dict(sd)
    raise ValueError(f"{path}: adapter files are .safetensors, .pt or .bin")


@dataclass
class LoraAdapter:
    """One parsed adapter.  updates[(module, row0, rows)] = (up bf16 [rows, R], down bf16 [R, K], scale = alpha / R or 1)."""
    name: str
    updates: dict[tuple[str, int, int], tuple[torch.Tensor, torch.Tensor, float]] = field(default_factory=dict)


def _split_key(key: str) -> tuple[str, str]:
    for suf, role in _SUFFIXES:
        if key.endswith(suf):
            mod = key[:-len(suf)]
            for pre in _PREFIXES:
                if mod.startswith(pre):
                    mod = mod[len(pre):]
                    break
            return mod, role
    raise KeyError(f"adapter key {key!r}: not a lora_A / lora_B / lora_down / lora_up / alpha key (DoRA, LoHa and rank-pattern "
                   "formats are not built)")


def parse_adapter(name: str, tensors: dict[str, torch.Tensor], targets: dict[str, tuple[int, int, bool]], D: int,
                  target_modules=None) -> LoraAdapter:
    """Tensors of one adapter -> LoraAdapter.  Accepted spellings: `<module>.lora_A.weight` / `.lora_B.weight` (PEFT, diffusers),
    `<module>.lora_down.weight` / `.lora_up.weight` (kohya, Lightning), optional `<module>.alpha`, optional leading `transformer.`
    or `diffusion_model.`.  scale = alpha / rank where alpha is present, else 1.  The factors are rounded to bf16 once here (the
    device merge takes bf16 operands).  Nothing is skipped silently: an unknown module or key raises KeyError, a missing partner
    KeyError, a shape that does not fit ValueError - each naming the module.  `target_modules` (suffix match against the module
    name as the FILE spells it, e.g. "to_q", "attn.to_out.0") is the only way to drop keys."""
    mods: dict[str, dict[str, torch.Tensor]] = {}
    for key, t in tensors.items():
        mod, role = _split_key(key)
        if role in mods.setdefault(mod, {}):
            raise KeyError(f"adapter {name!r}: module {mod!r} carries two {role} tensors (two key spellings of one factor)")
        mods[mod][role] = t
    out = LoraAdapter(name)
    for mod, parts in mods.items():
        if target_modules is not None and not any(mod == s or mod.endswith("." + s.lstrip(".")) for s in target_modules):
            continue
        for role, spelt in (("up", "lora_B / lora_up"), ("down", "lora_A / lora_down")):
            if role not in parts:
                raise KeyError(f"adapter {name!r}: module {mod!r} has no {spelt} tensor")
        fused, idx = mod, None
        for fsuf, ssuf, i in STACKED:
            if mod.endswith(ssuf):
                fused, idx = mod[:-len(ssuf)] + fsuf, i
                break
        if fused not in targets:
            raise KeyError(f"adapter {name!r}: module {mod!r} is not a LoRA target of this transformer")
        N, K, _ = targets[fused]
        up, down = parts["up"], parts["down"]
        if up.dim() != 2 or down.dim() != 2 or up.shape[1] != down.shape[0]:
            raise ValueError(f"adapter {name!r}: module {mod!r}: up {tuple(up.shape)} and down {tuple(down.shape)} are not "
                             "[out, rank] x [rank, in]")
        rank = int(down.shape[0])
        want_rows = D if idx is not None else N
        if up.shape[0] != want_rows or down.shape[1] != K or rank < 1:
            raise ValueError(f"adapter {name!r}: module {mod!r}: up {tuple(up.shape)} / down {tuple(down.shape)} do not fit a "
                             f"[{want_rows}, {K}] matrix")
        scale = 1.0
        if "alpha" in parts:
            scale = float(parts["alpha"].float().reshape(-1)[0]) / rank
        up_b, down_b = up.to(BF16).contiguous(), down.to(BF16).contiguous()
        if idx is not None:
            ranges = [(idx * D, D, up_b)]
        elif fused.endswith((".to_qkv", ".add_kv_proj")):          # a fused key: the same three ranges a split file addresses
            ranges = [(i * D, D, up_b[i * D:(i + 1) * D].contiguous()) for i in range(3)]
        else:
            ranges = [(0, N, up_b)]
        for row0, rows, u in ranges:
            k = (fused, row0, rows)
            if k in out.updates:
                raise ValueError(f"adapter {name!r}: module {mod!r}: rows {row0}..{row0 + rows - 1} of {fused} are given twice")
            out.updates[k] = (u, down_b, scale)
    return out


def stack(active: list[tuple[LoraAdapter, float]]) -> dict[tuple[str, int, int], tuple[torch.Tensor, torch.Tensor, float]]:
    """Several active adapters -> ONE update per (module, row0, rows): `down` concatenated along the rank, `up` concatenated along
    the rank, the per-adapter fp32 scales (alpha / rank * user weight) folded into one `scale`:
      - where the scales of a key agree (always, with one adapter) `up` keeps its bf16 values and `scale` carries the factor, which
        the kernel applies in fp32 after the sum;
      - where they differ, each `up` is multiplied by its scale in fp32 and rounded to bf16 ONCE, and `scale` is 1.
    Either way every weight element is rounded once, from the base value.  A total rank above 256 is refused, naming the module."""
    per: dict[tuple[str, int, int], list[tuple[torch.Tensor, torch.Tensor, float]]] = {}
    for ad, weight in active:
        for key, (up, down, scale) in ad.updates.items():
            per.setdefault(key, []).append((up, down, scale * float(weight)))
    plan = {}
    for key, parts in per.items():
        total = sum(int(d.shape[0]) for _, d, _ in parts)
        if total > MAX_RANK:
            raise ValueError(f"LoRA stack {[a.name for a, _ in active]}: total rank {total} on {key[0]} (rows {key[1]}.."
                             f"{key[1] + key[2] - 1}) exceeds {MAX_RANK}")
        scales = {s for _, _, s in parts}
        if len(scales) == 1:
            ups, scale = [u for u, _, _ in parts], scales.pop()
        else:
            ups, scale = [(u.float() * s).to(BF16) for u, _, s in parts], 1.0
        up = ups[0] if len(ups) == 1 else torch.cat(ups, dim=1).contiguous()
        down = parts[0][1] if len(parts) == 1 else torch.cat([d for _, d, _ in parts], dim=0).contiguous()
        plan[key] = (up, down, scale)
    return plan


def normalize_combo(lora, lora_scale: float = 1.0) -> tuple[tuple[str, float], ...]:
    """A request's `lora` / `lora_scale` as the ordered ((name, weight), ...) tuple that identifies an adapter combination;
    () = the base model."""
    if lora is None:
        return ()
    if isinstance(lora, str):
        return ((lora, float(lora_scale)),)
    return tuple((str(n), float(w)) for n, w in lora)
