"""Tensor-level wrappers over the C-ABI (raw device pointers + the current HIP stream).

PyTorch is plumbing here (device memory, streams); all arithmetic happens in libomni_cdna4.so.
Every wrapper raises if a tensor is not a bf16/int32/fp32 CUDA(HIP) tensor of the expected layout —
there is no eager fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as N

BF16 = torch.bfloat16

EPI_BIAS, EPI_BIAS_GELU_TANH, EPI_BIAS_GATE_RES, EPI_BIAS_SPLIT3, EPI_BIAS_SPLIT3_QKNORM_ROPE = 0, 1, 2, 3, 4


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: torch.Tensor | None, dtype=BF16, name: str = "tensor") -> int | None:
    if t is None:
        return None
    if not t.is_cuda:
        raise N.OmniNativeError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise N.OmniNativeError(f"{name} must be {dtype}, got {t.dtype}")
    if t.dim() >= 1 and t.stride(-1) != 1:
        raise N.OmniNativeError(f"{name} must be contiguous in its last dimension")
    return t.data_ptr()


def _rows2d(t: torch.Tensor, name: str) -> tuple[int, int, int]:
    """(rows, cols, row_stride) of a 2-D row-major view."""
    if t.dim() != 2:
        raise N.OmniNativeError(f"{name} must be 2-D, got shape {tuple(t.shape)}")
    return t.shape[0], t.shape[1], t.stride(0)


class GemmGroupArgs:
    """Python-side mirror of omni_gemm_group (one stream of a grouped GEMM)."""

    def __init__(self, a, w, bias=None, out=None, *, a_row_map=None, out_row_map=None, out1=None, out2=None,
                 res=None, gate=None, gate_item_stride=0, row_item_map=None, rows_per_item=0,
                 a_k32_blocked=False, out_k32_blocked=False, qk_norm_q_w=None, qk_norm_k_w=None, qk_rope_cos=None,
                 qk_rope_sin=None, qk_row_pos=None, qk_eps=1e-6, a_scale=None, w_scale=None, tile_skip=None):
        self.a_k32_blocked, self.out_k32_blocked = a_k32_blocked, out_k32_blocked
        self.a_scale, self.w_scale = a_scale, w_scale            # fp8 operands (gemm(..., fp8=True)): fp32 row / channel scales
        self.qk = (qk_norm_q_w, qk_norm_k_w, qk_rope_cos, qk_rope_sin, qk_row_pos, qk_eps)
        self.a, self.w, self.bias, self.out = a, w, bias, out
        self.a_row_map, self.out_row_map, self.out1, self.out2 = a_row_map, out_row_map, out1, out2
        self.res, self.gate, self.gate_item_stride = res, gate, gate_item_stride
        self.row_item_map, self.rows_per_item = row_item_map, rows_per_item
        self.tile_skip = tile_skip                                # int32 [ceil(M / 256)] device flags: non-zero = that row tile is skipped


GEMM_KERNEL_AUTO, GEMM_KERNEL_RING, GEMM_KERNEL_SPLITK_TALL, GEMM_KERNEL_NO_TAIL_SPLIT = 0, 1, 2, 3      # omni_gemm_params.kernel_hint
GEMM_KERNEL_SPLITK_IN_LAUNCH = 4                                                                      # ABI v12
GEMM_KERNEL_SPLITK_DEFER_FINISH = 5                                                                   # ABI v13


def w_to_k32_blocked(w: torch.Tensor) -> torch.Tensor:
    """[N, K] row-major -> the same values in K32-blocked order [K/32][N][32] (omni_gemm_params.w_k32_blocked = 1),
    returned as an [N, K]-shaped contiguous tensor so that shape checks and pointer plumbing stay unchanged."""
    n, k = w.shape
    if k % 32:
        raise ValueError("K must be a multiple of 32")
    return w.view(n, k // 32, 32).transpose(0, 1).contiguous().view(n, k)


def gemm(groups: list[GemmGroupArgs], epilogue: int = EPI_BIAS, split_n: int = 0, m_override: list[int] | None = None,
         w_k32_blocked: bool = False, splitk_ws: torch.Tensor | None = None, kernel_hint: int = 0, fp8: bool = False):
    p = _gemm_params(groups, epilogue, split_n, m_override, w_k32_blocked, splitk_ws, kernel_hint, fp8)
    N.check(N.lib().omni_gemm_bf16(C.byref(p), _stream()), "omni_gemm_bf16")


def gemm_splitk_factor(groups: list[GemmGroupArgs], epilogue: int = EPI_BIAS, split_n: int = 0, m_override: list[int] | None = None,
                       w_k32_blocked: bool = False, splitk_ws: torch.Tensor | None = None, kernel_hint: int = 0,
                       fp8: bool = False) -> int:
    """omni_gemm_splitk_factor (ABI v13): the whole-launch split-K factor `gemm` would use for these arguments (1 = no split).
    A caller that wants the partials left for `splitk_finish_adaln_pair` asks this first and then calls `gemm` with
    kernel_hint = GEMM_KERNEL_SPLITK_DEFER_FINISH."""
    p = _gemm_params(groups, epilogue, split_n, m_override, w_k32_blocked, splitk_ws, kernel_hint, fp8)
    s = int(N.lib().omni_gemm_splitk_factor(C.byref(p)))
    if s <= 0:
        raise N.OmniNativeError("omni_gemm_splitk_factor: not a valid GEMM call")
    return s


def _gemm_params(groups, epilogue, split_n, m_override, w_k32_blocked, splitk_ws, kernel_hint, fp8):
    """Y_g = epilogue(A_g @ W_g.T + bias_g) for up to two groups sharing N, K (omni_gemm_bf16).  `splitk_ws`: optional fp32
    device workspace; with it, launches of at most 128 tiles in at most 10 row tiles split their K loop (ABI v4).
    `kernel_hint`: 0 = automatic, GEMM_KERNEL_RING = force the fallback (ring) kernel (ABI v6; cross-checks),
    GEMM_KERNEL_SPLITK_TALL = automatic + split-K also for tall launches (ABI v10).
    `fp8`: A and W are uint8 tensors of OCP e4m3 values in the K64-blocked order (`quantize_fp8_rows`), with fp32
    `a_scale` / `w_scale` per group (ABI v7): Y = epilogue((A8 @ W8.T) * a_scale[:, None] * w_scale[None, :] + bias)."""
    p = N.GemmParams()
    p.kernel_hint = int(kernel_hint)
    p.fp8 = 1 if fp8 else 0
    op_dtype = torch.uint8 if fp8 else BF16
    if splitk_ws is not None:
        if splitk_ws.dtype != torch.float32 or not splitk_ws.is_cuda or not splitk_ws.is_contiguous():
            raise N.OmniNativeError("splitk_ws must be a contiguous float32 GPU tensor")
        p.splitk_ws, p.splitk_ws_floats = splitk_ws.data_ptr(), splitk_ws.numel()
    p.ngroups = len(groups)
    p.epilogue = epilogue
    p.split_n = split_n
    p.w_k32_blocked = 1 if w_k32_blocked else 0
    N_, K_ = groups[0].w.shape
    p.N, p.K = N_, K_
    for i, g in enumerate(groups):
        G = p.g[i]
        m, k, lda = _rows2d(g.a, "A")
        if g.w.shape != (N_, K_) or not g.w.is_contiguous():
            raise N.OmniNativeError("all groups must share a contiguous [N, K] weight shape")
        G.A, G.lda = _p(g.a, op_dtype, name="A"), lda
        G.M = m_override[i] if m_override else (g.a_row_map.numel() if g.a_row_map is not None else m)
        if g.a_row_map is None and k != K_:
            raise N.OmniNativeError(f"A has K={k}, W has K={K_}")
        G.a_row_map = _p(g.a_row_map, torch.int32, "a_row_map")
        G.W, G.bias = _p(g.w, op_dtype, name="W"), _p(g.bias, name="bias")
        if fp8:
            G.a_scale, G.w_scale = _p(g.a_scale, torch.float32, "a_scale"), _p(g.w_scale, torch.float32, "w_scale")
        G.out, G.ldo = _p(g.out, name="out"), g.out.stride(0)
        G.out1, G.out2 = _p(g.out1, name="out1"), _p(g.out2, name="out2")
        G.out_row_map = _p(g.out_row_map, torch.int32, "out_row_map")
        if g.res is not None:
            G.res, G.ldres = _p(g.res, name="res"), g.res.stride(0)
        G.gate, G.gate_item_stride = _p(g.gate, name="gate"), g.gate_item_stride
        G.row_item_map = _p(g.row_item_map, torch.int32, "row_item_map")
        G.rows_per_item = g.rows_per_item
        qw, kw, cos, sin, pos, eps = g.qk
        G.qk_norm_q_w, G.qk_norm_k_w = _p(qw, name="qk_norm_q_w"), _p(kw, name="qk_norm_k_w")
        G.qk_rope_cos, G.qk_rope_sin = _p(cos, name="qk_rope_cos"), _p(sin, name="qk_rope_sin")
        G.qk_row_pos, G.qk_eps = _p(pos, torch.int32, "qk_row_pos"), eps
        G.a_k32_rows = g.a.shape[0] if g.a_k32_blocked else 0       # blocked tensors keep their [rows, K] shape
        G.out_k32_rows = g.out.shape[0] if g.out_k32_blocked else 0
        G.tile_skip = _p(g.tile_skip, torch.int32, "tile_skip")
    return p


def quantize_fp8_rows(x: torch.Tensor, *, x_k32_blocked: bool = False, out: torch.Tensor | None = None,
                      scale: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """Dynamic per-row fp8 quantisation (omni_quantize_fp8_rows): x [rows, K] bf16 (row-major, or K32-blocked with
    x_k32_blocked) -> (y8 uint8 [rows, K] holding e4m3 bytes in the K64-blocked order [K/64][rows][64], scale fp32 [rows]) with
    x[r, k] ~= e4m3(y8)[r, k] * scale[r].  Rows of activations = tokens; rows of a weight = output channels."""
    rows, K, ldx = _rows2d(x, "x")
    y8 = torch.empty(rows, K, dtype=torch.uint8, device=x.device) if out is None else out
    sc = torch.empty(rows, dtype=torch.float32, device=x.device) if scale is None else scale
    N.check(N.lib().omni_quantize_fp8_rows(_p(x, name="x"), ldx, rows if x_k32_blocked else 0, rows, K,
                                           _p(y8, torch.uint8, "y8"), y8.shape[0], _p(sc, torch.float32, "scale"), _stream()),
            "omni_quantize_fp8_rows")
    return y8, sc


def adaln_modulate_fp8(x, scale, shift, *, mod_item_stride: int, row_item_map=None, rows_per_item: int = 0, eps: float = 1e-6,
                       want_bf16: bool = False):
    """AdaLN-modulate with the fp8 quantisation fused in (omni_adaln_modulate_fp8): -> (y8 uint8 [rows, D] K64-blocked,
    scale fp32 [rows], y bf16 [rows, D] K32-blocked or None)."""
    rows, D, ldx = _rows2d(x, "x")
    y8 = torch.empty(rows, D, dtype=torch.uint8, device=x.device)
    sc = torch.empty(rows, dtype=torch.float32, device=x.device)
    y = torch.empty(rows, D, dtype=BF16, device=x.device) if want_bf16 else None
    N.check(N.lib().omni_adaln_modulate_fp8(_p(x, name="x"), ldx, rows, D, _p(scale, name="scale"), _p(shift, name="shift"),
                                            mod_item_stride, _p(row_item_map, torch.int32, "row_item_map"), rows_per_item, eps,
                                            _p(y, name="y"), rows if want_bf16 else 0, _p(y8, torch.uint8, "y8"), rows,
                                            _p(sc, torch.float32, "scale_out"), _stream()), "omni_adaln_modulate_fp8")
    return y8, sc, y


def k64_blocked_fp8_to_rows(y8: torch.Tensor) -> torch.Tensor:
    """[rows, K]-shaped uint8 tensor holding [K/64][rows][64] -> row-major float8_e4m3fn view [rows, K] (tests / debugging)."""
    r, k = y8.shape
    return y8.view(k // 64, r, 64).transpose(0, 1).contiguous().view(r, k).view(torch.float8_e4m3fn)


def linear(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, *, gelu: bool = False,
           w_k32_blocked: bool = False) -> torch.Tensor:
    """Single-group convenience: x [M,K] @ w[N,K].T + bias (optionally GELU-tanh)."""
    out = torch.empty(x.shape[0], w.shape[0], dtype=BF16, device=x.device)
    gemm([GemmGroupArgs(x, w, bias, out)], EPI_BIAS_GELU_TANH if gelu else EPI_BIAS, w_k32_blocked=w_k32_blocked)
    return out


def k32_blocked_to_rows(t: torch.Tensor) -> torch.Tensor:
    """Inverse of the K32-blocked activation / weight layout: an [R, K]-shaped tensor holding [K/32][R][32] -> row-major."""
    r, k = t.shape
    return t.view(k // 32, r, 32).transpose(0, 1).contiguous().view(r, k)


def adaln_modulate(x, scale, shift, *, mod_item_stride: int, row_item_map=None, rows_per_item: int = 0,
                   eps: float = 1e-6, out=None, out_k32_blocked: bool = False):
    """out_k32_blocked: y (same [rows, D] shape) holds the K32-blocked order [D/32][rows][32] (omni_adaln_modulate_ex)."""
    rows, D, ldx = _rows2d(x, "x")
    y = torch.empty(rows, D, dtype=BF16, device=x.device) if out is None else out
    N.check(N.lib().omni_adaln_modulate_ex(_p(x, name="x"), ldx, _p(y, name="y"), y.stride(0), rows, D,
                                           _p(scale, name="scale"), _p(shift, name="shift"), mod_item_stride,
                                           _p(row_item_map, torch.int32, "row_item_map"), rows_per_item, eps,
                                           y.shape[0] if out_k32_blocked else 0, _stream()),
            "omni_adaln_modulate_ex")
    return y


def adaln_modulate_pair(streams, *, mod_item_stride: int, eps: float = 1e-6, out_k32_blocked: bool = False, fp8: bool = False,
                        want_bf16: bool = True):
    """omni_adaln_modulate_pair (ABI v12): AdaLN-modulate of TWO row groups (the image and the text stream of a DiT block) in one
    launch.  `streams` = two (x [rows, D] contiguous, scale, shift, row_item_map) tuples.  Returns per stream what the single
    calls return: y (row-major, or K32-blocked with `out_k32_blocked`); with `fp8` (y8, scale, y-or-None: the bf16 copy is
    K32-blocked) as `adaln_modulate_fp8`."""
    assert len(streams) == 2
    recs, outs = (N.AdalnStream * 2)(), []
    D = streams[0][0].shape[1]
    for i, (x, scale, shift, item_map) in enumerate(streams):
        rows, d, ldx = _rows2d(x, "x")
        if d != D or ldx != D:
            raise N.OmniNativeError("adaln_modulate_pair: both streams are contiguous [rows, D] with one D")
        g = recs[i]
        g.x, g.rows, g.scale, g.shift = _p(x, name="x"), rows, _p(scale, name="scale"), _p(shift, name="shift")
        g.row_item_map, g.rows_per_item = _p(item_map, torch.int32, "row_item_map"), 0
        y = torch.empty(rows, D, dtype=BF16, device=x.device) if (want_bf16 or not fp8) else None
        g.y, g.y_k32_rows = _p(y, name="y"), rows if (y is not None and (out_k32_blocked or fp8)) else 0
        if fp8:
            y8 = torch.empty(rows, D, dtype=torch.uint8, device=x.device)
            sc = torch.empty(rows, dtype=torch.float32, device=x.device)
            g.y8, g.y8_rows, g.y8_scale = _p(y8, torch.uint8, "y8"), rows, _p(sc, torch.float32, "scale_out")
            outs.append((y8, sc, y))
        else:
            outs.append(y)
    N.check(N.lib().omni_adaln_modulate_pair(C.byref(recs[0]), C.byref(recs[1]), D, mod_item_stride, eps, _stream()),
            "omni_adaln_modulate_pair")
    return outs


def splitk_finish_adaln_pair(splitk_ws: torch.Tensor, nsplit: int, ws_rows: int, streams, *, mod_item_stride: int,
                             eps: float = 1e-6, out_k32_blocked: bool = False):
    """omni_splitk_finish_adaln_pair (ABI v13): the finish of a DEFERRED split-K GEMM with the gated-residual epilogue + the AdaLN
    that follows it, both streams of a DiT block in one launch.  `splitk_ws` = the fp32 partials [nsplit][ws_rows][D] the GEMM left;
    `streams` = two (ws_row0, bias-or-None, hidden [rows, D] contiguous, gate, scale, shift, row_item_map) tuples.  `hidden` is
    updated IN PLACE (hidden + gate * (sum of partials + bias)); returns the two AdaLN outputs (row-major, or K32-blocked)."""
    assert len(streams) == 2
    recs, outs = (N.FinishAdalnStream * 2)(), []
    D = streams[0][2].shape[1]
    for i, (row0, bias, hidden, gate, scale, shift, item_map) in enumerate(streams):
        rows, d, ld = _rows2d(hidden, "hidden")
        if d != D or ld != D:
            raise N.OmniNativeError("splitk_finish_adaln_pair: both streams are contiguous [rows, D] with one D")
        g = recs[i]
        g.rows, g.ws_row0, g.bias, g.hidden = rows, int(row0), _p(bias, name="bias"), _p(hidden, name="hidden")
        g.gate, g.scale, g.shift = _p(gate, name="gate"), _p(scale, name="scale"), _p(shift, name="shift")
        g.row_item_map, g.rows_per_item = _p(item_map, torch.int32, "row_item_map"), 0
        y = torch.empty(rows, D, dtype=BF16, device=hidden.device)
        g.y, g.y_k32_rows = _p(y, name="y"), rows if out_k32_blocked else 0
        outs.append(y)
    N.check(N.lib().omni_splitk_finish_adaln_pair(_p(splitk_ws, torch.float32, "splitk_ws"), int(nsplit), int(ws_rows),
                                                  C.byref(recs[0]), C.byref(recs[1]), D, mod_item_stride, eps, _stream()),
            "omni_splitk_finish_adaln_pair")
    return outs


def rmsnorm(x, weight, eps: float = 1e-6, out=None):
    rows, D, ldx = _rows2d(x, "x")
    y = torch.empty_like(x) if out is None else out
    N.check(N.lib().omni_rmsnorm(_p(x, name="x"), ldx, _p(y, name="y"), y.stride(0), rows, D, _p(weight, name="w"),
                                 eps, _stream()), "omni_rmsnorm")
    return y


def qk_norm_rope_(x, num_heads, w_img, w_txt, cos_tab, sin_tab, row_pos, txt_pos_end, eps: float = 1e-6):
    rows, _, ldx = _rows2d(x, "x")
    N.check(N.lib().omni_qk_norm_rope(_p(x, name="x"), ldx, rows, num_heads, _p(w_img, name="w_img"),
                                      _p(w_txt, name="w_txt"), _p(cos_tab, name="cos"), _p(sin_tab, name="sin"),
                                      _p(row_pos, torch.int32, "row_pos"), txt_pos_end, eps, _stream()),
            "omni_qk_norm_rope")
    return x


def rope_interleaved(x, cos_tab, sin_tab, out=None):
    """x [B,S,H,dh] contiguous bf16; cos/sin [S, dh/2] bf16."""
    if x.dim() != 4 or not x.is_contiguous():
        raise N.OmniNativeError("rope_interleaved expects a contiguous [B,S,H,dh] tensor")
    B, S, H, dh = x.shape
    y = torch.empty_like(x) if out is None else out
    N.check(N.lib().omni_rope_interleaved(_p(x, name="x"), _p(y, name="y"), B, S, H, dh,
                                          _p(cos_tab.contiguous(), name="cos"), _p(sin_tab.contiguous(), name="sin"),
                                          _stream()), "omni_rope_interleaved")
    return y


def flash_attn_varlen(q, k, v, cu_seqlens, num_heads: int, max_seqlen: int, softmax_scale: float, out=None,
                      out_k32_blocked: bool = False, workspace: torch.Tensor | None = None):
    """q,k,v [rows, H*128] (row strides free), cu_seqlens int32 [B+1] on device.  out_k32_blocked: out (same shape)
    holds the K32-blocked order [H*128/32][rows][32] (omni_flash_attn_fwd_ex).  `workspace`: optional fp32 device tensor of
    `flash_attn_workspace_floats(B, H)` elements — lets the kernel split the key range of a short last q-block
    (omni_flash_attn_fwd_ws, ABI v11)."""
    rows, HD, ldq = _rows2d(q, "q")
    o = torch.empty(rows, HD, dtype=BF16, device=q.device) if out is None else out
    wsp, wsb = (None, 0) if workspace is None else (_p(workspace, torch.float32, "workspace"), workspace.numel() * 4)
    N.check(N.lib().omni_flash_attn_fwd_ws(_p(q, name="q"), _p(k, name="k"), _p(v, name="v"), _p(o, name="out"), ldq,
                                           k.stride(0), v.stride(0), o.stride(0),
                                           _p(cu_seqlens, torch.int32, "cu_seqlens"), cu_seqlens.numel() - 1, num_heads,
                                           HD // num_heads, max_seqlen, softmax_scale,
                                           o.shape[0] if out_k32_blocked else 0, wsp, wsb, _stream()),
            "omni_flash_attn_fwd_ws")
    return o


def flash_attn_workspace_floats(B: int, H: int) -> int:
    return int(N.lib().omni_flash_attn_workspace_bytes(B, H)) // 4


_MASK_TYPES = {torch.bool: 1, torch.uint8: 1, torch.bfloat16: 2, torch.float32: 3}
ATTN_ELEM_TYPES = {torch.bfloat16: N.ELEM_BF16, torch.float16: N.ELEM_F16}      # omni_attn_params.elem_type


def flash_attn_general(q, k, v, cu_seqlens_q, cu_seqlens_k, num_heads: int, num_kv_heads: int, max_seqlen_q: int,
                       max_seqlen_k: int, softmax_scale: float, causal: bool = False, mask: torch.Tensor | None = None,
                       mask_strides: tuple[int, int, int, int] | None = None, out=None, *, qk_int8: bool = False,
                       workspace: torch.Tensor | None = None, out_k32_blocked: bool = False,
                       item_skip: torch.Tensor | None = None):
    """omni_flash_attn_general (ABI v11): q / out [rows_q, H * dh], k / v [rows_k, H_kv * dh], dh 64 or 128; per-item row ranges
    from the two int32 prefix-sum vectors.  `mask`: bool / uint8 (True = attend), bf16 or fp32 (additive) DEVICE tensor whose
    element (b, h, i, j) sits `mask_strides` (in elements, 0 = broadcast) apart — `mask.expand(B, H, Sq, Sk).stride()`.
    `qk_int8` (ABI v14): SAGE_ATTN — int8 Q K^T with smoothed K (include/omni_cdna4.h omni_attn_params.qk_int8); no mask, not
    causal.  Its device workspace is `workspace` (uint8, at least attn_quant_workspace_bytes(...) bytes) or allocated here.
    `out_k32_blocked` (int8 path only): out holds the K32-blocked order [H*dh/32][rows][32].  `item_skip` (int8 path only):
    int32 DEVICE [B]; items with a non-zero entry are not computed and their output rows are left as they are.
    q, k, v (and `out`) share ONE dtype, bf16 or fp16 (omni_attn_params.elem_type); the output has it too.  fp16 needs a
    library that reports OMNI_FEATURE_ATTN_F16 and has no qk_int8 path.  A bf16 mask stays bf16 whatever q is."""
    dts = [t.dtype for t in (q, k, v) + (() if out is None else (out,))]
    if q.dtype not in ATTN_ELEM_TYPES or any(d != q.dtype for d in dts):
        raise N.OmniNativeError("q, k, v and out must share one dtype out of torch.bfloat16 / torch.float16, got "
                                + ", ".join(str(d) for d in dts))
    et = q.dtype
    if et == torch.float16 and not N.features() & N.FEATURE_ATTN_F16:
        raise N.OmniNativeError("this libomni_cdna4.so does not report OMNI_FEATURE_ATTN_F16: it would read fp16 q / k / v as "
                                "bf16 bits — rebuild it (python vllm_omni_amd/csrc/build.py)")
    rows, HD, ldq = _rows2d(q, "q")
    o = torch.empty(rows, HD, dtype=et, device=q.device) if out is None else out
    p = N.AttnParams()
    p.q, p.k, p.v, p.out = _p(q, et, name="q"), _p(k, et, name="k"), _p(v, et, name="v"), _p(o, et, name="out")
    p.elem_type = ATTN_ELEM_TYPES[et]
    p.ldq, p.ldk, p.ldv, p.ldo = ldq, k.stride(0), v.stride(0), o.stride(0)
    p.cu_seqlens_q, p.cu_seqlens_k = _p(cu_seqlens_q, torch.int32, "cu_seqlens_q"), _p(cu_seqlens_k, torch.int32, "cu_seqlens_k")
    p.B, p.H, p.H_kv, p.head_dim = cu_seqlens_q.numel() - 1, num_heads, num_kv_heads, HD // num_heads
    p.max_seqlen_q, p.max_seqlen_k = max_seqlen_q, max_seqlen_k
    p.softmax_scale, p.causal = softmax_scale, int(bool(causal))
    if mask is not None:
        if mask.dtype not in _MASK_TYPES:
            raise N.OmniNativeError(f"attention mask must be bool, uint8, bfloat16 or float32, got {mask.dtype}")
        if not mask.is_cuda:
            raise N.OmniNativeError("attention mask must live on the GPU")
        if mask_strides is None or len(mask_strides) != 4:
            raise N.OmniNativeError("mask_strides = the four element strides of the mask over (B, H, S_q, S_k)")
        p.mask, p.mask_type = mask.data_ptr(), _MASK_TYPES[mask.dtype]
        p.mask_stride_b, p.mask_stride_h, p.mask_stride_q, p.mask_stride_k = (int(x) for x in mask_strides)
    if qk_int8:
        p.qk_int8 = 1
        p.out_k32_rows = rows if out_k32_blocked else 0
        need = int(N.lib().omni_attn_quant_workspace_bytes(C.byref(p)))
        if workspace is None:
            workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=q.device)
        if not workspace.is_cuda or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
            raise N.OmniNativeError("the qk_int8 workspace must be a contiguous uint8 DEVICE tensor")
        p.workspace, p.workspace_bytes = workspace.data_ptr(), workspace.numel()
        if item_skip is not None:
            p.item_skip = _p(item_skip, torch.int32, "item_skip")
    elif out_k32_blocked or item_skip is not None:
        raise N.OmniNativeError("out_k32_blocked and item_skip are options of the qk_int8 path")
    N.check(N.lib().omni_flash_attn_general(C.byref(p), _stream()), "omni_flash_attn_general")
    return o


def attn_quant_workspace_bytes(B: int, num_heads: int, num_kv_heads: int, head_dim: int, max_seqlen_q: int,
                               max_seqlen_k: int) -> int:
    """omni_attn_quant_workspace_bytes: bytes of the qk_int8 (SAGE_ATTN) workspace for these bounds (0: not supported)."""
    p = N.AttnParams()
    p.B, p.H, p.H_kv, p.head_dim, p.max_seqlen_q, p.max_seqlen_k = B, num_heads, num_kv_heads, head_dim, max_seqlen_q, max_seqlen_k
    p.qk_int8 = 1
    return int(N.lib().omni_attn_quant_workspace_bytes(C.byref(p)))


def linear_smallbatch(x, w, bias=None, act_in: int = 0, act_out: int = 0, out=None):
    B, K, ldx = _rows2d(x, "x")
    Nn = w.shape[0]
    y = torch.empty(B, Nn, dtype=BF16, device=x.device) if out is None else out
    N.check(N.lib().omni_linear_smallbatch(_p(x, name="x"), ldx, B, _p(w, name="W"), _p(bias, name="bias"), Nn, K,
                                           _p(y, name="y"), y.stride(0), act_in, act_out, _stream()),
            "omni_linear_smallbatch")
    return y


def timestep_sinusoid(t: torch.Tensor, dim: int = 256, scale: float = 1000.0):
    out = torch.empty(t.numel(), dim, dtype=BF16, device=t.device)
    N.check(N.lib().omni_timestep_sinusoid(_p(t, torch.float32, "t"), t.numel(), dim, scale, _p(out), _stream()),
            "omni_timestep_sinusoid")
    return out


def cfg_euler_step_(latents, pos, neg, true_cfg_scale: float, dt: torch.Tensor, dt_rows_per_item: int = 0,
                    normalize: bool = True):
    """latents [rows,64] bf16 updated in place; dt fp32 device tensor.  normalize=False: the true-CFG combination without the
    norm rescale (the Layered pipeline's default)."""
    rows, Cc, _ = _rows2d(latents, "latents")
    if not (latents.is_contiguous() and pos.is_contiguous() and (neg is None or neg.is_contiguous())):
        raise N.OmniNativeError("cfg_euler_step_ needs contiguous [rows, 64] tensors")
    N.check(N.lib().omni_cfg_euler_step_ex(_p(pos, name="pos"), _p(neg, name="neg"), _p(latents, name="latents"), rows,
                                           Cc, true_cfg_scale, _p(dt, torch.float32, "dt"), dt_rows_per_item,
                                           1 if normalize else 0, _stream()),
            "omni_cfg_euler_step_ex")
    return latents


def cfg_euler_step_ragged_(latents, pred, lat_in, reqs, n_reqs: int, total_rows: int, dt: torch.Tensor, normalize: bool = True):
    """omni_cfg_euler_step_ragged: ONE launch updates the `n_reqs` requests that `reqs` describes (int32 [n_reqs, 8] on the
    device: the bytes of omni_cfg_euler_req, built by diffusion/batch.py `ragged_step_descriptors`), each with its own row
    count, scale and dt entry.  `latents` [*, 64] is updated in place from the prediction rows of `pred` [*, 64]; the new rows
    are also written to their rows of `lat_in` [*, 64], the next forward's input.  `total_rows`: the requests' rows summed."""
    if not N.features() & N.FEATURE_CFG_EULER_RAGGED:
        raise N.OmniNativeError("this libomni_cdna4.so does not report OMNI_FEATURE_CFG_EULER_RAGGED: it has no "
                                "omni_cfg_euler_step_ragged (the step update of mixed Edit groups)")
    for t, name in ((latents, "latents"), (pred, "pred"), (lat_in, "lat_in")):
        if t.dim() != 2 or not t.is_contiguous():
            raise N.OmniNativeError(f"cfg_euler_step_ragged_: {name} must be a contiguous [rows, 64] tensor")
    if reqs.dim() != 2 or reqs.shape[1] != 8 or not reqs.is_contiguous() or reqs.shape[0] < n_reqs:
        raise N.OmniNativeError("cfg_euler_step_ragged_: reqs must be a contiguous int32 [>= n_reqs, 8] tensor")
    N.check(N.lib().omni_cfg_euler_step_ragged(_p(pred, name="pred"), pred.shape[0], _p(latents, name="latents"), latents.shape[0],
                                               _p(lat_in, name="lat_in"), lat_in.shape[0], _p(reqs, torch.int32, "reqs"), n_reqs,
                                               total_rows, latents.shape[1], _p(dt, torch.float32, "dt"), dt.numel(),
                                               1 if normalize else 0, _stream()),
            "omni_cfg_euler_step_ragged")
    return latents


def lora_merge(w_base, w_out, up, down, scale: float, *, row0: int = 0, rows: int | None = None, k32_blocked: bool = False):
    """omni_lora_merge: w_out[n] = bf16(w_base[n] + scale * up[n - row0] @ down) for n in [row0, row0 + rows), fp32 accumulate,
    one rounding; other rows of w_out are not touched.  w_base / w_out [N, K] bf16 (the same tensor = in place), row-major
    (a row stride is honoured) or, `k32_blocked`, holding the K32-blocked order of `w_to_k32_blocked`; up [rows, R] and down
    [R, K] contiguous bf16, R <= 256.  Returns w_out."""
    if not N.features() & N.FEATURE_LORA_MERGE:
        raise N.OmniNativeError("this libomni_cdna4.so does not report OMNI_FEATURE_LORA_MERGE: it has no omni_lora_merge "
                                "(the device-side merge of LoRA adapters); there is no torch fallback")
    n, k, ldw = _rows2d(w_base, "w_base")
    if tuple(w_out.shape) != (n, k) or w_out.dim() != 2 or w_out.stride(0) != ldw:
        raise N.OmniNativeError(f"lora_merge: w_out must match w_base's shape and row stride ({n}, {k}; {ldw})")
    if k32_blocked and not (w_base.is_contiguous() and w_out.is_contiguous()):
        raise N.OmniNativeError("lora_merge: a K32-blocked matrix is one contiguous [K/32][N][32] buffer")
    rows = n - row0 if rows is None else rows
    if up.dim() != 2 or down.dim() != 2 or not up.is_contiguous() or not down.is_contiguous():
        raise N.OmniNativeError("lora_merge: up [rows, R] and down [R, K] must be contiguous 2-D tensors")
    if up.shape[0] != rows or up.shape[1] != down.shape[0] or down.shape[1] != k:
        raise N.OmniNativeError(f"lora_merge: up {tuple(up.shape)} / down {tuple(down.shape)} do not fit rows {rows} of a "
                                f"[{n}, {k}] matrix")
    p = N.LoraMergeParams()
    p.w_base, p.w_out = _p(w_base, name="w_base"), _p(w_out, name="w_out")
    p.up, p.down = _p(up, name="up"), _p(down, name="down")
    p.N, p.K, p.R, p.row0, p.rows = n, k, up.shape[1], row0, rows
    p.w_k32_blocked, p.ldw, p.scale = (1 if k32_blocked else 0), ldw, float(scale)
    N.check(N.lib().omni_lora_merge(C.byref(p), _stream()), "omni_lora_merge")
    return w_out


def _need_text_encoder(what: str) -> None:
    if not N.features() & N.FEATURE_TEXT_ENCODER:
        raise N.OmniNativeError(f"this libomni_cdna4.so does not report OMNI_FEATURE_TEXT_ENCODER: it has no {what} (the native "
                                "Qwen2.5-VL prompt encoder); there is no torch fallback")


def text_rope_neox_(qkv, num_heads: int, num_kv_heads: int, cos_tab, sin_tab, row_pos, err=None):
    """omni_text_rope_neox: rotate-half RoPE in place on the q and k column blocks of qkv [rows, >= (H + 2 H_kv) * 128] bf16 (a row
    stride is honoured); cos_tab / sin_tab fp32 [npos, 64] contiguous, row_pos int32 [rows].  The v block is not touched.
    `err` (int32 [1] on the device) is set when a position had to be clamped into the table."""
    _need_text_encoder("omni_text_rope_neox")
    rows, _, ld = _rows2d(qkv, "qkv")
    if cos_tab.shape != sin_tab.shape or cos_tab.dim() != 2 or cos_tab.shape[1] != 64 or not (cos_tab.is_contiguous() and sin_tab.is_contiguous()):
        raise N.OmniNativeError("text_rope_neox_: cos_tab / sin_tab are contiguous fp32 [npos, 64] tables")
    if row_pos.numel() != rows:
        raise N.OmniNativeError(f"text_rope_neox_: row_pos has {row_pos.numel()} entries for {rows} rows")
    N.check(N.lib().omni_text_rope_neox(_p(qkv, name="qkv"), ld, rows, num_heads, num_kv_heads, _p(cos_tab, torch.float32, "cos"),
                                        _p(sin_tab, torch.float32, "sin"), cos_tab.shape[0], _p(row_pos, torch.int32, "row_pos"),
                                        _p(err, torch.int32, "err"), _stream()), "omni_text_rope_neox")
    return qkv


def text_swiglu(gate_up, out=None, *, out_k32_blocked: bool = False):
    """omni_text_swiglu: gate_up [rows, 2 I] bf16 (gate | up, the fused GEMM's output) -> silu(gate) * up [rows, I];
    out_k32_blocked: the result (same shape) holds the K32-blocked order [I/32][rows][32] for a GEMM's `a_k32_blocked`."""
    _need_text_encoder("omni_text_swiglu")
    rows, two_i, ld = _rows2d(gate_up, "gate_up")
    if two_i % 2:
        raise N.OmniNativeError("text_swiglu: gate_up has an odd number of columns")
    y = torch.empty(rows, two_i // 2, dtype=BF16, device=gate_up.device) if out is None else out
    if out_k32_blocked and not y.is_contiguous():
        raise N.OmniNativeError("text_swiglu: a K32-blocked output is one contiguous buffer")
    N.check(N.lib().omni_text_swiglu(_p(gate_up, name="gate_up"), ld, _p(y, name="out"), y.stride(0), rows, two_i // 2,
                                     rows if out_k32_blocked else 0, _stream()), "omni_text_swiglu")
    return y


def text_embed_gather(table, ids, err, out=None):
    """omni_text_embed_gather: out[r] = table[ids[r]] (table [vocab, D] bf16 contiguous, ids int32 [rows]); an id outside the
    table writes a zero row and sets `err` (int32 [1] on the device) instead of reading."""
    _need_text_encoder("omni_text_embed_gather")
    vocab, D, ld = _rows2d(table, "table")
    if ld != D:
        raise N.OmniNativeError("text_embed_gather: the table must be contiguous")
    y = torch.empty(ids.numel(), D, dtype=BF16, device=table.device) if out is None else out
    N.check(N.lib().omni_text_embed_gather(_p(table, name="table"), vocab, D, _p(ids, torch.int32, "ids"), ids.numel(),
                                           _p(y, name="out"), y.stride(0), _p(err, torch.int32, "err"), _stream()),
            "omni_text_embed_gather")
    return y


def qwen2_text_workspace_bytes(weights: "N.TextWeights", total_rows: int) -> int:
    _need_text_encoder("omni_qwen2_text_workspace_bytes")
    return int(N.lib().omni_qwen2_text_workspace_bytes(C.byref(weights), int(total_rows)))


def qwen2_text_forward(weights: "N.TextWeights", input_ids, cu_seqlens, row_pos, max_seqlen: int, workspace, out=None):
    """omni_qwen2_text_forward: the whole Qwen2.5-VL text model over the packed tokens of `cu_seqlens.numel() - 1` prompts.
    `weights`: the filled descriptor (models/qwen_image/text_encoder.py builds and owns it); input_ids / row_pos int32 [rows],
    cu_seqlens int32 [n + 1], all on the device; `workspace`: uint8 device tensor of at least qwen2_text_workspace_bytes(...)
    bytes whose first 256 bytes were zero when it was allocated.  -> last hidden state [rows, hidden] bf16."""
    _need_text_encoder("omni_qwen2_text_forward")
    rows = input_ids.numel()
    if row_pos.numel() != rows:
        raise N.OmniNativeError(f"qwen2_text_forward: row_pos has {row_pos.numel()} entries for {rows} tokens")
    if not workspace.is_cuda or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise N.OmniNativeError("qwen2_text_forward: the workspace must be a contiguous uint8 DEVICE tensor")
    y = torch.empty(rows, weights.hidden_size, dtype=BF16, device=input_ids.device) if out is None else out
    if not y.is_contiguous():
        raise N.OmniNativeError("qwen2_text_forward: out must be contiguous")
    b = N.TextBatch()
    b.n_prompts, b.total_rows, b.max_seqlen = cu_seqlens.numel() - 1, rows, int(max_seqlen)
    b.input_ids, b.cu_seqlens = _p(input_ids, torch.int32, "input_ids"), _p(cu_seqlens, torch.int32, "cu_seqlens")
    b.row_pos, b.out = _p(row_pos, torch.int32, "row_pos"), _p(y, name="out")
    b.workspace, b.workspace_bytes = workspace.data_ptr(), workspace.numel()
    N.check(N.lib().omni_qwen2_text_forward(C.byref(weights), C.byref(b), _stream()), "omni_qwen2_text_forward")
    return y


def _need_vision_encoder(what: str) -> None:
    if not N.features() & N.FEATURE_VISION_ENCODER:
        raise N.OmniNativeError(f"this libomni_cdna4.so does not report OMNI_FEATURE_VISION_ENCODER: it has no {what} (the native "
                                "Qwen2.5-VL vision tower / Edit prompt encoder); there is no torch fallback")


def vision_rope_pad(qkv, num_heads: int, head_dim: int, cos_tab, sin_tab, out=None):
    """omni_vision_rope_pad: qkv [rows, >= 3 H hd] bf16 (q | k | v, a row stride is honoured) -> [rows, 3 H 128]: q and k rotated
    by the per-row fp32 tables cos_tab / sin_tab [rows, hd / 2] (rotate-half, partner at + hd / 2), v copied, columns hd .. 127 of
    every head zero.  `out` may be a wider row-strided view."""
    _need_vision_encoder("omni_vision_rope_pad")
    rows, _, ld = _rows2d(qkv, "qkv")
    want = (rows, head_dim // 2)
    if tuple(cos_tab.shape) != want or tuple(sin_tab.shape) != want or not (cos_tab.is_contiguous() and sin_tab.is_contiguous()):
        raise N.OmniNativeError(f"vision_rope_pad: cos_tab / sin_tab are contiguous fp32 {list(want)} tables, one row per qkv row")
    y = torch.empty(rows, 3 * num_heads * 128, dtype=BF16, device=qkv.device) if out is None else out
    if y.shape[0] != rows:
        raise N.OmniNativeError(f"vision_rope_pad: out has {y.shape[0]} rows for {rows}")
    N.check(N.lib().omni_vision_rope_pad(_p(qkv, name="qkv"), ld, _p(y, name="out"), y.stride(0), rows, num_heads, head_dim,
                                         _p(cos_tab, torch.float32, "cos"), _p(sin_tab, torch.float32, "sin"), _stream()),
            "omni_vision_rope_pad")
    return y


def gelu_erf(x, out=None, *, out_k32_blocked: bool = False):
    """omni_gelu_erf: exact-erf GELU (torch.nn.GELU()) of x [rows, n] bf16; `out=x` runs in place; out_k32_blocked: the result
    (same shape) holds the K32-blocked order [n/32][rows][32] for a GEMM's `a_k32_blocked`."""
    _need_vision_encoder("omni_gelu_erf")
    rows, n, ld = _rows2d(x, "x")
    y = torch.empty(rows, n, dtype=BF16, device=x.device) if out is None else out
    if out_k32_blocked and not y.is_contiguous():
        raise N.OmniNativeError("gelu_erf: a K32-blocked output is one contiguous buffer")
    N.check(N.lib().omni_gelu_erf(_p(x, name="x"), ld, _p(y, name="out"), y.stride(0), rows, n, rows if out_k32_blocked else 0,
                                  _stream()), "omni_gelu_erf")
    return y


def text_mrope_(qkv, num_heads: int, num_kv_heads: int, cos_tab, sin_tab, row_pos3, mrope_section, err=None):
    """omni_text_mrope: `text_rope_neox_` with the three M-RoPE position rows row_pos3 int32 [3, rows] (contiguous) and
    mrope_section (three ints that sum to 64, multiples of 8): rotary pair i reads the tables at the row of its section."""
    _need_vision_encoder("omni_text_mrope")
    rows, _, ld = _rows2d(qkv, "qkv")
    if cos_tab.shape != sin_tab.shape or cos_tab.dim() != 2 or cos_tab.shape[1] != 64 or not (cos_tab.is_contiguous() and sin_tab.is_contiguous()):
        raise N.OmniNativeError("text_mrope_: cos_tab / sin_tab are contiguous fp32 [npos, 64] tables")
    if tuple(row_pos3.shape) != (3, rows) or not row_pos3.is_contiguous():
        raise N.OmniNativeError(f"text_mrope_: row_pos3 must be a contiguous [3, {rows}] tensor, got {tuple(row_pos3.shape)}")
    sec = (C.c_int32 * 3)(*[int(v) for v in mrope_section])
    N.check(N.lib().omni_text_mrope(_p(qkv, name="qkv"), ld, rows, num_heads, num_kv_heads, _p(cos_tab, torch.float32, "cos"),
                                    _p(sin_tab, torch.float32, "sin"), cos_tab.shape[0], _p(row_pos3, torch.int32, "row_pos3"),
                                    sec, _p(err, torch.int32, "err"), _stream()), "omni_text_mrope")
    return qkv


def qwen2_vision_workspace_bytes(weights: "N.VisionWeights", rows: int) -> int:
    _need_vision_encoder("omni_qwen2_vision_workspace_bytes")
    return int(N.lib().omni_qwen2_vision_workspace_bytes(C.byref(weights), int(rows)))


def qwen2_vision_forward(weights: "N.VisionWeights", pixels, cu_window, cu_image, max_window: int, max_image: int, cos_tab, sin_tab,
                         workspace, out=None):
    """omni_qwen2_vision_forward: the whole Qwen2.5-VL vision tower over the packed patch rows of all pictures IN WINDOW ORDER.
    pixels [rows, patch_k] bf16 (zero-padded columns), cu_window / cu_image int32 prefix sums, cos_tab / sin_tab fp32
    [rows, head_dim / 2], all on the device -> [rows / 4, out_hidden] bf16, still in window order."""
    _need_vision_encoder("omni_qwen2_vision_forward")
    rows, kp, ld = _rows2d(pixels, "pixels")
    if ld != kp or kp != weights.patch_k:
        raise N.OmniNativeError(f"qwen2_vision_forward: pixels must be contiguous [rows, {weights.patch_k}], got {tuple(pixels.shape)}")
    want = (rows, weights.head_dim // 2)
    if tuple(cos_tab.shape) != want or tuple(sin_tab.shape) != want or not (cos_tab.is_contiguous() and sin_tab.is_contiguous()):
        raise N.OmniNativeError(f"qwen2_vision_forward: cos_tab / sin_tab are contiguous fp32 {list(want)} tables")
    if not workspace.is_cuda or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise N.OmniNativeError("qwen2_vision_forward: the workspace must be a contiguous uint8 DEVICE tensor")
    y = torch.empty(rows // 4, weights.out_hidden_size, dtype=BF16, device=pixels.device) if out is None else out
    if not y.is_contiguous():
        raise N.OmniNativeError("qwen2_vision_forward: out must be contiguous")
    b = N.VisionBatch()
    b.rows, b.n_windows, b.n_images = rows, cu_window.numel() - 1, cu_image.numel() - 1
    b.max_window, b.max_image = int(max_window), int(max_image)
    b.pixels, b.cu_window, b.cu_image = _p(pixels, name="pixels"), _p(cu_window, torch.int32, "cu_window"), _p(cu_image, torch.int32, "cu_image")
    b.rope_cos, b.rope_sin, b.out = _p(cos_tab, torch.float32, "cos"), _p(sin_tab, torch.float32, "sin"), _p(y, name="out")
    b.workspace, b.workspace_bytes = workspace.data_ptr(), workspace.numel()
    N.check(N.lib().omni_qwen2_vision_forward(C.byref(weights), C.byref(b), _stream()), "omni_qwen2_vision_forward")
    return y


def qwen2_text_forward_mm(weights: "N.TextWeights", input_ids, cu_seqlens, row_pos3, mrope_section, max_seqlen: int, workspace,
                          vision_rows=None, vision_row_of=None, out=None):
    """omni_qwen2_text_forward_mm: `qwen2_text_forward` with the three M-RoPE position rows row_pos3 int32 [3, rows] and, where
    vision_row_of int32 [rows] is >= 0, vision_rows [n, hidden] bf16 in place of the token embedding (both None: text only)."""
    _need_vision_encoder("omni_qwen2_text_forward_mm")
    rows = input_ids.numel()
    if tuple(row_pos3.shape) != (3, rows) or not row_pos3.is_contiguous():
        raise N.OmniNativeError(f"qwen2_text_forward_mm: row_pos3 must be a contiguous [3, {rows}] tensor, got {tuple(row_pos3.shape)}")
    if (vision_rows is None) != (vision_row_of is None):
        raise N.OmniNativeError("qwen2_text_forward_mm: vision_rows and vision_row_of come together")
    if vision_rows is not None and (vision_row_of.numel() != rows or not vision_rows.is_contiguous()
                                    or vision_rows.dim() != 2 or vision_rows.shape[1] != weights.hidden_size):
        raise N.OmniNativeError(f"qwen2_text_forward_mm: vision_rows is contiguous [n, {weights.hidden_size}], vision_row_of has "
                                f"one entry per token ({rows})")
    if not workspace.is_cuda or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise N.OmniNativeError("qwen2_text_forward_mm: the workspace must be a contiguous uint8 DEVICE tensor")
    y = torch.empty(rows, weights.hidden_size, dtype=BF16, device=input_ids.device) if out is None else out
    if not y.is_contiguous():
        raise N.OmniNativeError("qwen2_text_forward_mm: out must be contiguous")
    b = N.TextBatchMm()
    b.n_prompts, b.total_rows, b.max_seqlen = cu_seqlens.numel() - 1, rows, int(max_seqlen)
    b.input_ids, b.cu_seqlens = _p(input_ids, torch.int32, "input_ids"), _p(cu_seqlens, torch.int32, "cu_seqlens")
    b.row_pos3, b.out = _p(row_pos3, torch.int32, "row_pos3"), _p(y, name="out")
    b.workspace, b.workspace_bytes = workspace.data_ptr(), workspace.numel()
    if vision_rows is not None:
        b.vision_rows, b.vision_row_of = _p(vision_rows, name="vision_rows"), _p(vision_row_of, torch.int32, "vision_row_of")
        b.n_vision_rows = vision_rows.shape[0]
    b.mrope_section = (C.c_int32 * 3)(*[int(v) for v in mrope_section])
    N.check(N.lib().omni_qwen2_text_forward_mm(C.byref(weights), C.byref(b), _stream()), "omni_qwen2_text_forward_mm")
    return y


# ---- greedy decode with a KV cache (OMNI_FEATURE_TEXT_DECODE) ------------------------------------------------------------------
def _need_text_decode(what: str) -> None:
    if not N.features() & N.FEATURE_TEXT_DECODE:
        raise N.OmniNativeError(f"this libomni_cdna4.so does not report OMNI_FEATURE_TEXT_DECODE: it has no {what} (the native "
                                "captioner); there is no torch fallback")


def gemv_bf16(a, w, bias=None, *, res=None, out=None, out_f32: bool = False, w_k32_blocked: bool = False):
    """omni_gemv_bf16: a [M <= 8, K] bf16 (a row stride is honoured) times w [N, K] bf16 - row-major or, w_k32_blocked, the
    K32-blocked order `w_to_k32_blocked` returns - with fp32 accumulation.  bias [N]; res [M, N]: out = res + bf16(a w^T + bias);
    out_f32: the result is fp32 [M, N] (no res).  `out` may be given (res may alias it)."""
    _need_text_decode("omni_gemv_bf16")
    M, K, lda = _rows2d(a, "a")
    n, kw, ldw = _rows2d(w, "w")
    if kw != K or ldw != K:
        raise N.OmniNativeError(f"gemv_bf16: w must be contiguous [N, {K}], got {tuple(w.shape)}")
    y = out if out is not None else torch.empty(M, n, dtype=torch.float32 if out_f32 else BF16, device=a.device)
    p = N.GemvParams()
    p.A, p.lda, p.M, p.N, p.K, p.w_k32_blocked = _p(a, name="a"), lda, M, n, K, int(w_k32_blocked)
    p.W, p.bias = _p(w, name="w"), _p(bias, name="bias")
    if res is not None:
        p.res, p.ldres = _p(res, name="res"), res.stride(0)
    if out_f32:
        p.out_f32 = _p(y, torch.float32, "out")
    else:
        p.out = _p(y, name="out")
    p.ldo = y.stride(0)
    N.check(N.lib().omni_gemv_bf16(C.byref(p), _stream()), "omni_gemv_bf16")
    return y


def decode_attention(q, k_cache, v_cache, lens, *, num_heads: int, len_add: int = 0, done=None, softmax_scale: float | None = None,
                     out=None):
    """omni_decode_attention: q [n_seq, >= H * 128] bf16 (one query row per sequence), k_cache / v_cache
    [n_seq, H_kv, capacity, 128] bf16 contiguous, lens int32 [n_seq] on the device: sequence s attends to its first
    lens[s] + len_add cache rows.  -> [n_seq, H * 128] bf16.  A sequence with done[s] != 0 is skipped (its row is not written)."""
    _need_text_decode("omni_decode_attention")
    n_seq, _, ldq = _rows2d(q, "q")
    if k_cache.dim() != 4 or k_cache.shape != v_cache.shape or k_cache.shape[0] != n_seq or not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise N.OmniNativeError("decode_attention: k_cache / v_cache are contiguous [n_seq, H_kv, capacity, 128] tensors")
    _, hkv, cap, hd = k_cache.shape
    y = torch.empty(n_seq, num_heads * 128, dtype=BF16, device=q.device) if out is None else out
    need = int(N.lib().omni_decode_attention_workspace_bytes(n_seq, num_heads, cap))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=q.device)
    p = N.DecodeAttnParams()
    p.q, p.ldq, p.k_cache, p.v_cache = _p(q, name="q"), ldq, _p(k_cache, name="k_cache"), _p(v_cache, name="v_cache")
    p.out, p.ldo, p.lens, p.done = _p(y, name="out"), y.stride(0), _p(lens, torch.int32, "lens"), _p(done, torch.int32, "done")
    p.len_add, p.n_seq, p.H, p.H_kv, p.head_dim, p.capacity = int(len_add), n_seq, int(num_heads), hkv, hd, cap
    p.softmax_scale = float(softmax_scale if softmax_scale is not None else hd ** -0.5)
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
    N.check(N.lib().omni_decode_attention(C.byref(p), _stream()), "omni_decode_attention")
    return y


def penalized_argmax(logits, seen, ctrl, out_tokens, *, penalty: float = 1.0, eos_ids=(), set_len_cu=None):
    """omni_text_penalized_argmax on logits fp32 [n_seq, vocab], seen uint8 [n_seq, >= vocab], ctrl int32 [8, 8] (the control
    words, rows N.DECODE_*), out_tokens int32 [n_seq, max_new]: all updated in place."""
    _need_text_decode("omni_text_penalized_argmax")
    n_seq, vocab, ld = _rows2d(logits, "logits")
    if seen.dtype != torch.uint8 or seen.dim() != 2 or seen.stride(1) != 1 or not seen.is_cuda:
        raise N.OmniNativeError("penalized_argmax: seen is a uint8 [n_seq, >= vocab] DEVICE tensor")
    if tuple(ctrl.shape) != (N.DECODE_CTRL_WORDS, N.DECODE_MAX_SEQ) or not ctrl.is_contiguous():
        raise N.OmniNativeError("penalized_argmax: ctrl is a contiguous int32 [8, 8] tensor")
    if out_tokens.dim() != 2 or not out_tokens.is_contiguous():
        raise N.OmniNativeError("penalized_argmax: out_tokens is a contiguous int32 [n_seq, max_new] tensor")
    p = N.PenalizedArgmaxParams()
    p.logits, p.ld, p.seen, p.seen_stride = _p(logits, torch.float32, "logits"), ld, seen.data_ptr(), seen.stride(0)
    p.ctrl, p.out_tokens, p.set_len_cu = _p(ctrl, torch.int32, "ctrl"), _p(out_tokens, torch.int32, "out_tokens"), _p(set_len_cu, torch.int32, "set_len_cu")
    p.vocab, p.n_seq, p.max_new, p.n_eos, p.penalty = vocab, n_seq, out_tokens.shape[1], len(eos_ids), float(penalty)
    p.eos_ids = (C.c_int32 * 8)(*[int(e) for e in list(eos_ids)[:8]])
    N.check(N.lib().omni_text_penalized_argmax(C.byref(p), _stream()), "omni_text_penalized_argmax")


class Qwen2DecodeState:
    """The decode state of `qwen2_text_prefill` / `qwen2_text_decode_step`: one device buffer carved by the library, with views of
    the parts a caller touches - `ctrl` int32 [8, 8] (rows N.DECODE_CUR_LEN .. ), `out_tokens` int32 [n_seq, max_new], `seen`,
    `k_cache` / `v_cache` bf16 [layers, n_seq, H_kv, capacity, 128], `logits` fp32 [n_seq, vocab] (the raw logits of the last call),
    `qkv` (the last step's q | k | v rows of the last layer)."""

    def __init__(self, weights: "N.TextWeights", lm_head, workspace, n_seq: int, capacity: int, max_new: int, eos_ids=(),
                 repetition_penalty: float = 1.0, buffer=None):
        _need_text_decode("omni_qwen2_text_decode_state_bytes")
        lay = N.TextDecodeLayout()
        total = int(N.lib().omni_qwen2_text_decode_state_bytes(C.byref(weights), int(n_seq), int(capacity), int(max_new), C.byref(lay)))
        if total == 0:
            raise N.OmniNativeError(f"omni_qwen2_text_decode_state_bytes refuses n_seq {n_seq}, capacity {capacity}, max_new {max_new} "
                                    "for these weights")
        if len(eos_ids) > 8:
            raise N.OmniNativeError(f"{len(eos_ids)} EOS ids: at most 8")
        dev = lm_head.device
        if buffer is None:
            buffer = torch.zeros(total, dtype=torch.uint8, device=dev)
        elif not buffer.is_cuda or buffer.dtype != torch.uint8 or not buffer.is_contiguous() or buffer.numel() < total:
            raise N.OmniNativeError(f"the decode state needs a contiguous uint8 DEVICE buffer of {total} bytes")
        self.buffer, self.state_bytes = buffer, total
        self.logits = torch.zeros(n_seq, weights.vocab_size, dtype=torch.float32, device=dev)
        self.layout, self.weights, self.lm_head, self.workspace = lay, weights, lm_head, workspace
        self.n_seq, self.capacity, self.max_new = int(n_seq), int(capacity), int(max_new)
        L, hkv = weights.num_layers, weights.num_kv_heads
        b = self.buffer
        self.ctrl = b[lay.ctrl:lay.ctrl + 256].view(torch.int32).view(N.DECODE_CTRL_WORDS, N.DECODE_MAX_SEQ)
        self.out_tokens = b[lay.out_tokens:lay.out_tokens + 4 * n_seq * max_new].view(torch.int32).view(n_seq, max_new)
        self.seen = b[lay.seen:lay.seen + n_seq * lay.seen_stride].view(n_seq, lay.seen_stride)
        cache = L * n_seq * hkv * capacity * 128 * 2
        self.k_cache = b[lay.k_cache:lay.k_cache + cache].view(BF16).view(L, n_seq, hkv, capacity, 128)
        self.v_cache = b[lay.v_cache:lay.v_cache + cache].view(BF16).view(L, n_seq, hkv, capacity, 128)
        nqkv = (weights.num_heads + 2 * hkv) * 128
        self.qkv = b[lay.qkv:lay.qkv + n_seq * nqkv * 2].view(BF16).view(n_seq, nqkv)
        st = N.TextDecodeState()
        st.n_seq, st.capacity, st.max_new, st.n_eos = self.n_seq, self.capacity, self.max_new, len(eos_ids)
        st.eos_ids = (C.c_int32 * 8)(*[int(e) for e in eos_ids])
        st.repetition_penalty = float(repetition_penalty)
        st.lm_head = _p(lm_head, name="lm_head")
        st.state, st.state_bytes = b.data_ptr(), total
        st.workspace, st.workspace_bytes = workspace.data_ptr(), workspace.numel()
        st.logits_out = self.logits.data_ptr()
        self.desc = st


def qwen2_decode_state(weights: "N.TextWeights", lm_head, workspace, n_seq: int, capacity: int, max_new: int, eos_ids=(),
                       repetition_penalty: float = 1.0, buffer=None) -> Qwen2DecodeState:
    """Allocate (zeroed; or carve the caller's `buffer`) and describe a decode state; `workspace` is the prefill's workspace (its
    error word is the decode's)."""
    return Qwen2DecodeState(weights, lm_head, workspace, n_seq, capacity, max_new, eos_ids, repetition_penalty, buffer)


def qwen2_text_prefill(weights: "N.TextWeights", state: Qwen2DecodeState, input_ids, cu_seqlens, row_pos3, mrope_section,
                       max_seqlen: int, vision_rows=None, vision_row_of=None, out=None):
    """omni_qwen2_text_prefill: `qwen2_text_forward_mm` over `state.workspace` that also fills the KV cache of `state`, computes
    the logits of every sequence's last row and picks its first token.  -> last hidden state [rows, hidden] bf16."""
    _need_text_decode("omni_qwen2_text_prefill")
    rows = input_ids.numel()
    if tuple(row_pos3.shape) != (3, rows) or not row_pos3.is_contiguous():
        raise N.OmniNativeError(f"qwen2_text_prefill: row_pos3 must be a contiguous [3, {rows}] tensor, got {tuple(row_pos3.shape)}")
    if (vision_rows is None) != (vision_row_of is None):
        raise N.OmniNativeError("qwen2_text_prefill: vision_rows and vision_row_of come together")
    if vision_rows is not None and (vision_row_of.numel() != rows or not vision_rows.is_contiguous()
                                    or vision_rows.dim() != 2 or vision_rows.shape[1] != weights.hidden_size):
        raise N.OmniNativeError(f"qwen2_text_prefill: vision_rows is contiguous [n, {weights.hidden_size}], vision_row_of has "
                                f"one entry per token ({rows})")
    y = torch.empty(rows, weights.hidden_size, dtype=BF16, device=input_ids.device) if out is None else out
    if not y.is_contiguous():
        raise N.OmniNativeError("qwen2_text_prefill: out must be contiguous")
    b = N.TextBatchMm()
    b.n_prompts, b.total_rows, b.max_seqlen = cu_seqlens.numel() - 1, rows, int(max_seqlen)
    b.input_ids, b.cu_seqlens = _p(input_ids, torch.int32, "input_ids"), _p(cu_seqlens, torch.int32, "cu_seqlens")
    b.row_pos3, b.out = _p(row_pos3, torch.int32, "row_pos3"), _p(y, name="out")
    b.workspace, b.workspace_bytes = state.workspace.data_ptr(), state.workspace.numel()
    if vision_rows is not None:
        b.vision_rows, b.vision_row_of = _p(vision_rows, name="vision_rows"), _p(vision_row_of, torch.int32, "vision_row_of")
        b.n_vision_rows = vision_rows.shape[0]
    b.mrope_section = (C.c_int32 * 3)(*[int(v) for v in mrope_section])
    N.check(N.lib().omni_qwen2_text_prefill(C.byref(weights), C.byref(b), C.byref(state.desc), _stream()), "omni_qwen2_text_prefill")
    return y


def qwen2_text_decode_step(weights: "N.TextWeights", state: Qwen2DecodeState, steps: int = 1) -> None:
    """omni_qwen2_text_decode_step, `steps` times back to back: enqueue-only (no host read between them)."""
    _need_text_decode("omni_qwen2_text_decode_step")
    fn, s = N.lib().omni_qwen2_text_decode_step, _stream()
    for _ in range(int(steps)):
        N.check(fn(C.byref(weights), C.byref(state.desc), s), "omni_qwen2_text_decode_step")


def vae_conv2d(x, w, bias=None, *, gamma=None, silu=True, res=None, upsample2x=False, downsample2x=False, clamp=None,
               out=None, x_bordered=False, y_bordered=False, norm_gamma=None, norm_silu=True, keep_raw=True):
    """NHWC bf16 conv (3x3 pad 1 or 1x1): x [B,H,W,Cin], w [Cout,ks,ks,Cin].  downsample2x: the encoder's zero-pad
    (right/bottom) + stride-2 3x3 conv.  x_bordered: x (and res) are zero-bordered rasters [B,H+2,W+2,C]; y_bordered: so is
    the output (the decoder's LDS-DMA-fed shifted-GEMM kernel; needs x_bordered, Cin % 32 == 0, Cout % 8 == 0).

    norm_gamma [Cout]: ALSO return silu?(rmsnorm(y) * norm_gamma) — the norm + activation that follows this conv in the decoder —
    from the same launch where the kernel holds all channels of a pixel (omni_vae_conv2d_fuses_norm), from a second pass
    otherwise.  Returns (y, y_norm); with keep_raw=False y is None when the kernel did not have to write it."""
    B, Hin, Win, Cin = x.shape
    if x_bordered:
        Hin, Win = Hin - 2, Win - 2
    Cout, ks = w.shape[0], w.shape[1]
    Hout, Wout = (2 * Hin, 2 * Win) if upsample2x else ((Hin // 2, Win // 2) if downsample2x else (Hin, Win))
    shape = (B, Hout + 2 * int(y_bordered), Wout + 2 * int(y_bordered), Cout)
    p = N.ConvParams()
    p.x, p.w, p.bias, p.gamma = _p(x.contiguous(), name="x"), _p(w, name="w"), _p(bias, name="bias"), _p(gamma)
    p.res = _p(res, name="res")
    p.B, p.Hin, p.Win, p.Cin, p.Cout, p.ksize = B, Hin, Win, Cin, Cout, ks
    p.upsample2x, p.silu, p.downsample2x = int(upsample2x), int(silu), int(downsample2x)
    p.x_padded, p.y_padded = int(x_bordered), int(y_bordered)
    p.clamp_lo, p.clamp_hi = clamp if clamp else (0.0, 0.0)
    yn = None
    if norm_gamma is not None:
        yn = torch.empty(shape, dtype=BF16, device=x.device)
        p.norm_gamma, p.y_norm, p.norm_silu = _p(norm_gamma, name="norm_gamma"), _p(yn), int(norm_silu)
        keep_raw = keep_raw or out is not None or not N.lib().omni_vae_conv2d_fuses_norm(C.byref(p))
    y = None
    if norm_gamma is None or keep_raw:
        y = torch.empty(shape, dtype=BF16, device=x.device) if out is None else out
    p.y = _p(y, name="y")
    N.check(N.lib().omni_vae_conv2d(C.byref(p), _stream()), "omni_vae_conv2d")
    return y if norm_gamma is None else (y, yn)


def vae_upsample2x_bordered(x):
    """Nearest-exact x2 upsample between zero-bordered rasters: [B,H+2,W+2,C] -> [B,2H+2,2W+2,C]."""
    B, Hp, Wp, Cc = x.shape
    y = torch.empty(B, 2 * (Hp - 2) + 2, 2 * (Wp - 2) + 2, Cc, dtype=BF16, device=x.device)
    N.check(N.lib().omni_vae_upsample2x_bordered(_p(x.contiguous(), name="x"), _p(y), B, Hp - 2, Wp - 2, Cc, _stream()),
            "omni_vae_upsample2x_bordered")
    return y


def vae_rmsnorm_silu(x, gamma, silu: bool = True):
    y = torch.empty_like(x)
    Cc = x.shape[-1]
    N.check(N.lib().omni_vae_rmsnorm_silu(_p(x.contiguous(), name="x"), _p(y), x.numel() // Cc, Cc, _p(gamma),
                                          int(silu), _stream()), "omni_vae_rmsnorm_silu")
    return y


VAE_ATTENTION_CHANNELS = 384          # the head dim omni_vae_attention is built for


def vae_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float) -> torch.Tensor:
    """Single-head attention per image: q, k, v [B, tokens, 384] (row-strided views of one fused projection are fine: the last
    dim must be contiguous, images must be tokens * row_stride apart) -> [B, tokens, 384] = softmax(scale q k^T) v."""
    B, tok, Cc = q.shape
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        if t.shape != q.shape or t.stride(2) != 1 or (B > 1 and t.stride(0) != tok * t.stride(1)):
            raise N.OmniNativeError(f"{n}: expected [B, tokens, C] with contiguous channels and images tokens * row_stride apart")
    out = torch.empty(B, tok, Cc, dtype=BF16, device=q.device)
    N.check(N.lib().omni_vae_attention(_p(q, name="q"), _p(k, name="k"), _p(v, name="v"), _p(out), B, tok, Cc, q.stride(1),
                                       k.stride(1), v.stride(1), Cc, float(scale), _stream()), "omni_vae_attention")
    return out


def softmax_rows_(s: torch.Tensor, scale: float):
    rows, cols, ld = _rows2d(s, "scores")
    N.check(N.lib().omni_softmax_rows(_p(s, name="scores"), ld, rows, cols, scale, _stream()), "omni_softmax_rows")
    return s
