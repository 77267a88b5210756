// Qwen2.5-VL VISION tower forward (HF transformers Qwen2_5_VisionTransformerPretrainedModel: what the Edit pipelines' prompt encoder
// runs on the condition pictures, reference vllm_omni/diffusion/models/qwen_image/pipeline_qwen_image_edit.py:352-397) as ONE native
// call: omni_qwen2_vision_forward enqueues every kernel of all vision blocks and of the patch merger over the packed patch rows of
// all pictures, in window order, on a HIP stream.  The GEMMs, RMSNorm, SwiGLU and the general attention are the library's existing
// kernels; this file holds the two row kernels that were missing and the driver.
//
// Both kernels are HBM-trivial and follow text_forward.hip: one wave per row segment, 16 bytes per lane per access, fp32 arithmetic,
// one rounding to bf16.
//   vision_rope_pad_kernel   reads the fused qkv GEMM output [rows, 3 H hd] (hd = 80 at real width), writes q | k | v as
//                            [rows, 3 H 128]: q and k rotated by the 2-D rotate-half RoPE (partner at + hd / 2, per-row fp32 tables),
//                            v copied, columns hd .. 127 of every head zero.  With zero pad columns the general attention kernel at
//                            head size 128 and softmax_scale hd^-0.5 computes head-size-hd attention: Q K^T gains zero terms, the
//                            extra P V columns are zero and meet zero columns of the projection weight.
//                            bytes/row = 2 x 3 H hd read (q, k twice: L1 hits) + 2 x 3 H 128 written + 2 x 2 hd of tables.
//   gelu_erf_kernel          y = 0.5 x (1 + erf(x / sqrt 2)): the patch merger's nn.GELU() (the GEMM's fused GELU is the tanh form),
//                            row-major or K32-blocked output.  bytes/row = 2 n read + 2 n written.
#include "common.h"

namespace {

constexpr int VIS_HEAD = 128;              // the padded head size: the attention kernel's

OMNI_DEVINL void unpack8(const u32x4_t& w, float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = bf16_lo(w[i]);
    f[2 * i + 1] = bf16_hi(w[i]);
  }
}
OMNI_DEVINL u32x4_t pack8(const float* f) {
  u32x4_t w;
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = pack_bf16x2(f[2 * i], f[2 * i + 1]);
  return w;
}

// 16 lanes per OUTPUT head slot (q, k and v heads alike: 3 H slots per row): lane g of a slot owns output columns 8 g .. 8 g + 7 of
// the 128.  hd is a multiple of 16, so hd / 2 is a multiple of 8 and the rotate-half partners of a lane's 8 elements are one
// other 16-byte granule of the same head.  unit = row * nseg + segment of 4 slots.
__global__ __launch_bounds__(256) void vision_rope_pad_kernel(const uint16_t* __restrict__ qkv, int64_t ld_in, uint16_t* __restrict__ out,
                                                              int64_t ld_out, int rows, int H, int hd,
                                                              const float* __restrict__ cos_tab, const float* __restrict__ sin_tab) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int nslots = 3 * H, nseg = (nslots + 3) >> 2;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t row = unit / nseg;
  if (row >= rows) return;
  const int slot = (int)(unit - row * nseg) * 4 + (lane >> 4);
  if (slot >= nslots) return;
  const int e = (lane & 15) * 8;                                 // first of this lane's 8 output columns
  uint16_t* dst = out + row * ld_out + (int64_t)slot * VIS_HEAD + e;
  u32x4_t y = {0u, 0u, 0u, 0u};
  if (e < hd) {
    const uint16_t* x = qkv + row * ld_in + (int64_t)slot * hd;
    y = *reinterpret_cast<const u32x4_t*>(x + e);
    if (slot < 2 * H) {                                          // q or k: rotate; v goes out as it came in
      const int half = hd >> 1;
      const bool low = e < half;
      const int t = low ? e : e - half;                          // the table column
      const u32x4_t pw = *reinterpret_cast<const u32x4_t*>(x + (low ? e + half : e - half));
      const float* cp = cos_tab + row * half + t;
      const float* sp = sin_tab + row * half + t;
      const f32x4_t c0 = *reinterpret_cast<const f32x4_t*>(cp), c1 = *reinterpret_cast<const f32x4_t*>(cp + 4);
      const f32x4_t s0 = *reinterpret_cast<const f32x4_t*>(sp), s1 = *reinterpret_cast<const f32x4_t*>(sp + 4);
      float a[8], b[8], o[8];
      unpack8(y, a);
      unpack8(pw, b);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float c = i < 4 ? c0[i & 3] : c1[i & 3], s = i < 4 ? s0[i & 3] : s1[i & 3];
        // HF: x * cos + rotate_half(x) * sin, rotate_half = (-x2, x1)
        o[i] = low ? __builtin_fmaf(a[i], c, -(b[i] * s)) : __builtin_fmaf(a[i], c, b[i] * s);
      }
      y = pack8(o);
    }
  }
  *reinterpret_cast<u32x4_t*>(dst) = y;
}

// unit = row * nseg + segment of 512 columns; a lane owns 8 consecutive columns
__global__ __launch_bounds__(256) void gelu_erf_kernel(const uint16_t* __restrict__ x, int64_t ldx, uint16_t* __restrict__ y, int64_t ldy,
                                                       int rows, int n, int y_k32_rows) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int nseg = (n + 511) >> 9;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t row = unit / nseg;
  if (row >= rows) return;
  const int e = ((int)(unit - row * nseg) * 64 + lane) * 8;
  if (e >= n) return;
  float f[8], o[8];
  unpack8(*reinterpret_cast<const u32x4_t*>(x + row * ldx + e), f);
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = 0.5f * f[i] * (1.0f + erff(f[i] * 0.70710678118654752440f));
  uint16_t* dst = y_k32_rows ? y + ((int64_t)(e >> 5) * y_k32_rows + row) * 32 + (e & 31) : y + row * ldy + e;
  *reinterpret_cast<u32x4_t*>(dst) = pack8(o);
}

inline unsigned wave_blocks(int64_t units) { return (unsigned)((units + 3) / 4); }

int vision_rope_pad(const omni_bf16* qkv, int64_t ld_in, omni_bf16* out, int64_t ld_out, int32_t rows, int32_t H, int32_t hd,
                    const float* cos_tab, const float* sin_tab, omni_stream stream) {
  if (!qkv || !out || !cos_tab || !sin_tab || rows <= 0 || H <= 0 || hd <= 0) return OMNI_ERR_BAD_ARG;
  if (hd % 16 || hd > VIS_HEAD) return OMNI_ERR_UNSUPPORTED;
  if (ld_in < 3 * (int64_t)H * hd || ld_out < 3 * (int64_t)H * VIS_HEAD) return OMNI_ERR_BAD_ARG;
  if (!omni_aligned16(qkv) || !omni_aligned16(out) || !omni_aligned16(cos_tab) || !omni_aligned16(sin_tab) || (ld_in % 8) || (ld_out % 8))
    return OMNI_ERR_ALIGN;
  const int64_t units = (int64_t)rows * ((3 * (int64_t)H + 3) / 4);
  if (units > 0x7fffffffLL) return OMNI_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(vision_rope_pad_kernel, dim3(wave_blocks(units)), dim3(256), 0, static_cast<hipStream_t>(stream), qkv, ld_in, out,
                     ld_out, rows, H, hd, cos_tab, sin_tab);
  OMNI_CHECK_LAUNCH();
  return OMNI_OK;
}

int gelu_erf(const omni_bf16* x, int64_t ldx, omni_bf16* y, int64_t ldy, int32_t rows, int32_t n, int32_t y_k32_rows,
             omni_stream stream) {
  if (!x || !y || rows <= 0 || n <= 0 || y_k32_rows < 0) return OMNI_ERR_BAD_ARG;
  if (n % 8 || (y_k32_rows && n % 32)) return OMNI_ERR_UNSUPPORTED;
  if (ldx < n || (y_k32_rows ? y_k32_rows < rows : ldy < n)) return OMNI_ERR_BAD_ARG;
  if (x == y && (y_k32_rows || ldy != ldx)) return OMNI_ERR_BAD_ARG;       // in place: the same element order only
  if (!omni_aligned16(x) || !omni_aligned16(y) || (ldx % 8) || (!y_k32_rows && (ldy % 8))) return OMNI_ERR_ALIGN;
  const int64_t units = (int64_t)rows * ((n + 511) / 512);
  if (units > 0x7fffffffLL) return OMNI_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gelu_erf_kernel, dim3(wave_blocks(units)), dim3(256), 0, static_cast<hipStream_t>(stream), x, ldx, y, ldy, rows, n,
                     y_k32_rows);
  OMNI_CHECK_LAUNCH();
  return OMNI_OK;
}

// ---- driver ---------------------------------------------------------------------------------------------------------------
struct VisionWorkspace {
  omni_bf16 *h, *xn, *qkv, *qkvp, *attn, *gu, *act, *m1, *m2;
  float* splitk;                // as in text_forward.hip: few row tiles -> the narrow launches may split K
  int64_t splitk_floats;
  size_t total;
};

inline size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

VisionWorkspace carve(void* base, const omni_vision_weights* w, int64_t R) {
  const int64_t D = w->hidden_size, I = w->intermediate_size, H = w->num_heads, hd = w->head_dim;
  size_t off = 0;
  char* b = static_cast<char*>(base);
  auto take = [&](int64_t elems) {
    omni_bf16* p = reinterpret_cast<omni_bf16*>(b + off);
    off += align_up((size_t)elems * sizeof(omni_bf16));
    return p;
  };
  VisionWorkspace ws;
  ws.h = take(R * D);
  ws.xn = take(R * D);
  ws.qkv = take(R * 3 * H * hd);
  ws.qkvp = take(R * 3 * H * VIS_HEAD);
  ws.attn = take(R * H * VIS_HEAD);
  ws.gu = take(R * 2 * I);
  ws.act = take(R * I);
  ws.m1 = take(R * D);          // [R / 4, 4 D]
  ws.m2 = take(R * D);
  const int64_t n1 = 3 * H * hd, n2 = w->out_hidden_size;
  const int64_t nmax = n1 > n2 ? (n1 > D ? n1 : D) : (n2 > D ? n2 : D);
  ws.splitk_floats = R <= 10 * 256 ? 8 * R * nmax : 0;
  ws.splitk = ws.splitk_floats ? reinterpret_cast<float*>(take(ws.splitk_floats * 2)) : nullptr;
  ws.total = off;
  return ws;
}

// everything a call can refuse before it touches the device
int vision_check_weights(const omni_vision_weights* w) {
  if (!w || !w->layers || !w->patch_w || !w->ones || !w->merger_norm_w || !w->merger_fc1_w || !w->merger_fc1_b || !w->merger_fc2_w ||
      !w->merger_fc2_b)
    return OMNI_ERR_BAD_ARG;
  if (w->num_layers <= 0 || w->hidden_size <= 0 || w->num_heads <= 0 || w->head_dim <= 0 || w->intermediate_size <= 0 ||
      w->patch_k <= 0 || w->out_hidden_size <= 0)
    return OMNI_ERR_BAD_ARG;
  if (w->gemm_w_k32_blocked != 0 && w->gemm_w_k32_blocked != 1) return OMNI_ERR_BAD_ARG;
  if (w->head_dim % 16 != 0 || w->head_dim > VIS_HEAD) return OMNI_ERR_UNSUPPORTED;
  if (w->hidden_size % 64 != 0 || w->intermediate_size % 64 != 0 || w->patch_k % 64 != 0 || w->out_hidden_size % 64 != 0 ||
      w->hidden_size > 8192)
    return OMNI_ERR_UNSUPPORTED;
  if ((int64_t)w->num_heads * w->head_dim != w->hidden_size) return OMNI_ERR_BAD_ARG;
  return OMNI_OK;
}

size_t vision_workspace_bytes(const omni_vision_weights* w, int32_t rows) {
  if (vision_check_weights(w) != OMNI_OK || rows <= 0 || rows % 4) return 0;
  return carve(nullptr, w, rows).total;
}

struct Gemm {
  const omni_vision_weights* w;
  const VisionWorkspace& ws;
  omni_stream stream;
  // out = A W^T + bias (A row-major [M, K], or K32-blocked when a_k32_rows)
  int plain(const omni_bf16* A, int32_t a_k32_rows, int32_t M, int32_t K, const omni_bf16* W, const omni_bf16* bias, int32_t N,
            omni_bf16* out) const {
    omni_gemm_params p = {};
    p.ngroups = 1; p.N = N; p.K = K; p.epilogue = OMNI_EPI_BIAS; p.w_k32_blocked = w->gemm_w_k32_blocked;
    p.g[0].A = A; p.g[0].lda = K; p.g[0].a_k32_rows = a_k32_rows; p.g[0].M = M; p.g[0].W = W; p.g[0].bias = bias;
    p.g[0].out = out; p.g[0].ldo = N;
    p.splitk_ws = ws.splitk; p.splitk_ws_floats = ws.splitk_floats;
    return omni_gemm_bf16(&p, stream);
  }
  // h = h + 1 * (A W^T + bias): the gated-residual epilogue with the bf16 ones gate, as text_forward.hip's residual_gemm
  int residual(const omni_bf16* A, int32_t a_k32_rows, int32_t M, int32_t K, const omni_bf16* W, const omni_bf16* bias) const {
    const int32_t D = w->hidden_size;
    omni_gemm_params p = {};
    p.ngroups = 1; p.N = D; p.K = K; p.epilogue = OMNI_EPI_BIAS_GATE_RES; p.w_k32_blocked = w->gemm_w_k32_blocked;
    p.g[0].A = A; p.g[0].lda = K; p.g[0].a_k32_rows = a_k32_rows; p.g[0].M = M; p.g[0].W = W; p.g[0].bias = bias;
    p.g[0].out = ws.h; p.g[0].ldo = D; p.g[0].res = ws.h; p.g[0].ldres = D;
    p.g[0].gate = w->ones; p.g[0].gate_item_stride = 0; p.g[0].rows_per_item = M;
    p.splitk_ws = ws.splitk; p.splitk_ws_floats = ws.splitk_floats;
    return omni_gemm_bf16(&p, stream);
  }
};

int vision_forward(const omni_vision_weights* w, const omni_vision_batch* b, omni_stream stream) {
  if (!b) return OMNI_ERR_BAD_ARG;
  OMNI_TRY_STATUS(vision_check_weights(w));
  if (!b->pixels || !b->cu_window || !b->cu_image || !b->rope_cos || !b->rope_sin || !b->out || !b->workspace) return OMNI_ERR_BAD_ARG;
  if (b->rows <= 0 || b->n_windows <= 0 || b->n_images <= 0 || b->max_window <= 0 || b->max_image <= 0 || b->max_window > b->rows ||
      b->max_image > b->rows || b->n_windows > b->rows || b->n_images > b->rows)
    return OMNI_ERR_BAD_ARG;
  if (b->rows % 4) return OMNI_ERR_UNSUPPORTED;
  if (!omni_aligned16(b->workspace) || !omni_aligned16(b->out) || !omni_aligned16(b->pixels)) return OMNI_ERR_ALIGN;
  for (int l = 0; l < w->num_layers; ++l) {
    const omni_vision_layer_weights& L = w->layers[l];
    if (!L.norm1_w || !L.qkv_w || !L.qkv_b || !L.proj_w || !L.proj_b || !L.norm2_w || !L.gate_up_w || !L.gate_up_b || !L.down_w ||
        !L.down_b)
      return OMNI_ERR_BAD_ARG;
    if (L.full_attention != 0 && L.full_attention != 1) return OMNI_ERR_BAD_ARG;
  }
  const int32_t R = b->rows, D = w->hidden_size, I = w->intermediate_size, H = w->num_heads, hd = w->head_dim;
  const int32_t Nqkv = 3 * H * hd, Np = H * VIS_HEAD;
  const VisionWorkspace ws = carve(b->workspace, w, R);
  if (ws.total > b->workspace_bytes) return OMNI_ERR_BAD_ARG;
  const Gemm gemm = {w, ws, stream};

  // patch embedding: the Conv3d with stride = kernel is a GEMM over the flattened patch vectors
  OMNI_TRY_STATUS(gemm.plain(b->pixels, 0, R, w->patch_k, w->patch_w, nullptr, D, ws.h));
  const float sm_scale = 1.0f / sqrtf((float)hd);
  for (int l = 0; l < w->num_layers; ++l) {
    const omni_vision_layer_weights& L = w->layers[l];
    OMNI_TRY_STATUS(omni_rmsnorm(ws.h, D, ws.xn, D, R, D, L.norm1_w, w->rms_norm_eps, stream));
    OMNI_TRY_STATUS(gemm.plain(ws.xn, 0, R, D, L.qkv_w, L.qkv_b, Nqkv, ws.qkv));
    OMNI_TRY_STATUS(vision_rope_pad(ws.qkv, Nqkv, ws.qkvp, 3 * (int64_t)Np, R, H, hd, b->rope_cos, b->rope_sin, stream));
    {
      omni_attn_params ap = {};
      ap.q = ws.qkvp; ap.k = ws.qkvp + Np; ap.v = ws.qkvp + 2 * (int64_t)Np; ap.out = ws.attn;
      ap.ldq = ap.ldk = ap.ldv = 3 * (int64_t)Np; ap.ldo = Np;
      ap.cu_seqlens_q = ap.cu_seqlens_k = L.full_attention ? b->cu_image : b->cu_window;
      ap.B = L.full_attention ? b->n_images : b->n_windows; ap.H = H; ap.H_kv = H; ap.head_dim = VIS_HEAD;
      ap.max_seqlen_q = ap.max_seqlen_k = L.full_attention ? b->max_image : b->max_window;
      ap.softmax_scale = sm_scale; ap.causal = 0;
      OMNI_TRY_STATUS(omni_flash_attn_general(&ap, stream));
    }
    OMNI_TRY_STATUS(gemm.residual(ws.attn, 0, R, Np, L.proj_w, L.proj_b));
    OMNI_TRY_STATUS(omni_rmsnorm(ws.h, D, ws.xn, D, R, D, L.norm2_w, w->rms_norm_eps, stream));
    OMNI_TRY_STATUS(gemm.plain(ws.xn, 0, R, D, L.gate_up_w, L.gate_up_b, 2 * I, ws.gu));
    OMNI_TRY_STATUS(omni_text_swiglu(ws.gu, 2 * (int64_t)I, ws.act, I, R, I, R, stream));
    OMNI_TRY_STATUS(gemm.residual(ws.act, R, R, I, L.down_w, L.down_b));
  }
  // patch merger: ln_q per patch row, then 4 consecutive rows (one 2 x 2 merge unit) are one row of the MLP
  const int32_t Rm = R / 4, Dm = 4 * D;
  OMNI_TRY_STATUS(omni_rmsnorm(ws.h, D, ws.xn, D, R, D, w->merger_norm_w, w->rms_norm_eps, stream));
  OMNI_TRY_STATUS(gemm.plain(ws.xn, 0, Rm, Dm, w->merger_fc1_w, w->merger_fc1_b, Dm, ws.m1));
  OMNI_TRY_STATUS(gelu_erf(ws.m1, Dm, ws.m2, Dm, Rm, Dm, Rm, stream));
  return gemm.plain(ws.m2, Rm, Rm, Dm, w->merger_fc2_w, w->merger_fc2_b, w->out_hidden_size, b->out);
}

}  // namespace

// exported as const pointers, not as functions: see the header (the exported functions of ABI v14 are fixed).  Host pass only.
#if !defined(__HIP_DEVICE_COMPILE__)
extern "C" int (*const omni_qwen2_vision_forward)(const omni_vision_weights*, const omni_vision_batch*, omni_stream) = vision_forward;
extern "C" size_t (*const omni_qwen2_vision_workspace_bytes)(const omni_vision_weights*, int32_t) = vision_workspace_bytes;
extern "C" int (*const omni_vision_rope_pad)(const omni_bf16*, int64_t, omni_bf16*, int64_t, int32_t, int32_t, int32_t, const float*,
                                             const float*, omni_stream) = vision_rope_pad;
extern "C" int (*const omni_gelu_erf)(const omni_bf16*, int64_t, omni_bf16*, int64_t, int32_t, int32_t, int32_t, omni_stream) = gelu_erf;
#endif
