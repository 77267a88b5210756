"""Per-element checking of GEMM outputs: an fp64 reference of every epilogue, the project's elementwise bar, guard bands.

  reference()          fp64 result of Y = epilogue(A . W^T + bias) from the bf16-rounded inputs, in LOGICAL row order, on the device
                       the inputs live on (plain torch in fp64: CPU, or the GPU for the large shapes — no kernel of this project).
  assert_elementwise() |got - ref| <= 2^-7 * (|ref| + rms(ref)) + extra for EVERY element (tests/test_gpu_ops.py
                       elem_close).  bf16 rounds to u = 2^-8 relative: the bar is 2u of the value plus 2u of the tensor's rms (fp32
                       accumulation error and cancellation: an output near zero is a sum of terms of the size of the rms).
  guarded()            an output buffer inside a larger allocation filled with a bit pattern + a check that nothing outside the
                       elements the call may write has changed.

GATE_RES rounds twice (omni_cdna4.h, csrc/gemm.hip "GATE_RES note"): c = bf16(A . W^T + bias), y = bf16(res + gate * c).  The
reference follows it — ref = res + gate * bf16(c64) — and because the kernel's c may land on the other side of a rounding
boundary than bf16(c64), the bar gets extra = 2^-7 * |gate| * |c64|: one bf16 unit of the intermediate, carried through the gate,
with the same factor 2 over u as the main term.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

BF16 = torch.bfloat16
U = 2.0 ** -7                                   # the bar: 2 * bf16 unit roundoff
EPI_BIAS, EPI_GELU, EPI_GATE_RES, EPI_SPLIT3 = 0, 1, 2, 3      # = vllm_omni_amd.ops.EPI_*
GUARD_BITS = 0x7A5C                             # as bf16: 2.86e35 — finite, never a GEMM result here, two distinct bytes


def gelu_tanh64(x: torch.Tensor) -> torch.Tensor:
    """gelu_tanh in fp64 as x * sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3): the same function as 0.5 x (1 + tanh u) without the
    cancellation of 1 + tanh(u) for u << 0."""
    x = x.double()
    u = 0.7978845608028654 * (x + 0.044715 * x * x * x)
    return x * torch.sigmoid(2.0 * u)


@dataclass
class Ref:
    ref: torch.Tensor        # fp64 [M, N], logical rows (SPLIT3: the three destinations side by side, columns q | k | v)
    c64: torch.Tensor        # fp64 [M, N]: A . W^T + bias before the epilogue
    extra: torch.Tensor | float   # additive term of the bar (GATE_RES), else 0.0


def reference(a, w, bias=None, epilogue: int = EPI_BIAS, *, a_row_map=None, res=None, out_row_map=None, gate=None,
              row_item_map=None, rows_per_item: int = 0, a_scale=None, w_scale=None) -> Ref:
    """a [R, K], w [N, K], bias [N]: bf16 (or any float dtype holding the values the kernel sees; fp8 callers pass the dequantised
    values and the fp32 scales: c = (A . W^T) * a_scale[stored row] * w_scale[col] + bias).  a_row_map [M] gathers A rows.
    GATE_RES: res [Rout, N] is indexed like the output (by out_row_map[r], else r), gate [items, N] by row_item_map[r], else
    r // rows_per_item.  out_row_map does not move anything else: the result is in logical row order, the caller gathers the
    kernel's output with the same map.  SPLIT3 is the BIAS result (column block j of the result belongs to destination j)."""
    A = a.double()
    sa = None if a_scale is None else a_scale.double()
    if a_row_map is not None:
        A = A[a_row_map.long()]
        sa = None if sa is None else sa[a_row_map.long()]
    c = A @ w.double().t()
    if sa is not None:
        c = c * sa[: c.shape[0], None] * w_scale.double()[None, :]
    if bias is not None:
        c = c + bias.double()[None, :]
    M = c.shape[0]
    if epilogue in (EPI_BIAS, EPI_SPLIT3):
        return Ref(c, c, 0.0)
    if epilogue == EPI_GELU:
        return Ref(gelu_tanh64(c), c, 0.0)
    if epilogue != EPI_GATE_RES:
        raise ValueError(f"no reference for epilogue {epilogue}")
    rows = torch.arange(M, device=c.device)
    item = row_item_map.long() if row_item_map is not None else rows // rows_per_item
    orow = out_row_map.long() if out_row_map is not None else rows
    g = gate.double()[item]
    r = res.double()[orow]
    return Ref(r + g * c.to(BF16).double(), c, U * g.abs() * c.abs())


def scaled_error(got: torch.Tensor, ref: torch.Tensor, extra=0.0) -> float:
    """max over ALL elements of |got - ref| / (|ref| + rms(ref) + extra / 2^-7): <= 2^-7 exactly when the bar holds."""
    ref = ref.double()
    got = got.double().to(ref.device)
    if got.shape != ref.shape:
        raise AssertionError(f"shape {tuple(got.shape)} != reference {tuple(ref.shape)}")
    rms = ref.pow(2).mean().sqrt()
    den = ref.abs() + rms + (extra if isinstance(extra, float) else extra.double()) / U
    q = (got - ref).abs() / den
    q = torch.where(torch.isfinite(q), q, torch.full_like(q, float("inf")))      # a NaN / inf output is the worst error, not none
    return float(q.max())


def assert_elementwise(got: torch.Tensor, ref: torch.Tensor, extra=0.0, what: str = "") -> float:
    """Every element, no exclusions, no sampling: |got - ref| <= 2^-7 * (|ref| + rms(ref)) + extra.  Prints and returns the worst
    scaled error (to be read against 2^-7 = 7.8e-3)."""
    worst = scaled_error(got, ref, extra)
    print(f"gemm elementwise {what}: worst scaled error {worst:.3e} (bar {U:.3e})")
    if not worst <= U:
        ref64 = ref.double()
        den = ref64.abs() + ref64.pow(2).mean().sqrt() + (extra if isinstance(extra, float) else extra.double()) / U
        q = (got.double().to(ref64.device) - ref64).abs() / den
        q = torch.where(torch.isfinite(q), q, torch.full_like(q, float("inf")))
        idx = int(q.argmax())
        r, c = divmod(idx, ref64.shape[-1]) if ref64.dim() == 2 else (0, idx)
        raise AssertionError(f"{what}: scaled error {worst:.3e} > 2^-7 at [{r}, {c}]: got {float(got.flatten()[idx])}, "
                             f"reference {float(ref64.flatten()[idx])}; {int((q > U).sum())} of {q.numel()} elements over the bar")
    return worst


def guarded(rows: int, cols: int, ld: int | None = None, lead: int = 4096, device="cpu", dtype=BF16, tail: int = 4096):
    """A [rows, cols] view with row stride ld inside an allocation of lead + rows * ld + tail elements, all of it (the view too)
    filled with GUARD_BITS.  Returns (view, check); check(written=None) asserts that every element OUTSIDE what the call may write
    still holds the pattern: the leading band, the trailing band, the ld - cols slack columns of every row and — with `written`, a
    bool mask [rows, cols] (or [rows]: whole rows) of the elements the call may write — everything else inside the view.  All of it
    lies well inside the allocation: the bands are there to be looked at, not to be hit."""
    if dtype.itemsize != 2:
        raise ValueError("guarded() compares through an int16 view: 2-byte element types only")
    ld = cols if ld is None else ld
    if ld < cols or rows < 1 or lead < 0 or tail < 1:
        raise ValueError("bad guarded() geometry")
    raw = torch.full((lead + rows * ld + tail,), GUARD_BITS, dtype=torch.int16, device=device)
    view = raw[lead:lead + rows * ld].view(rows, ld)[:, :cols].view(dtype)

    def check(written=None, what: str = "output"):
        snap = raw.clone()
        inner = snap[lead:lead + rows * ld].view(rows, ld)[:, :cols]
        if written is None:
            inner.fill_(GUARD_BITS)
        else:
            m = written.to(snap.device)
            inner[m if m.dim() == 2 else m[:, None].expand(rows, cols)] = GUARD_BITS
        bad = (snap != GUARD_BITS).nonzero().flatten()
        if bad.numel():
            off = int(bad[0]) - lead
            where = ("the leading band" if off < 0 else "the trailing band" if off >= rows * ld else
                     f"row {off // ld}, column {off % ld}" + (" (slack)" if off % ld >= cols else " (a row / element the call must not write)"))
            raise AssertionError(f"{what}: {bad.numel()} element(s) outside the written region changed; first at offset {off} from "
                                 f"the view = {where}")

    return view, check


def bf16_ulp_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Distance in bf16 steps (bit patterns mapped to a monotone integer line; +0 and -0 coincide)."""
    def line(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (line(a.to(BF16)) - line(b.to(BF16).to(a.device))).abs()
