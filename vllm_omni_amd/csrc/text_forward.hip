// Qwen2.5-VL TEXT model forward (HF transformers Qwen2_5_VLTextModel: the prompt encoder of the Qwen-Image pipelines, reference
// vllm_omni/diffusion/models/qwen_image/pipeline_qwen_image.py:351-392) as ONE native call: omni_qwen2_text_forward enqueues every
// kernel of all decoder layers over the PACKED valid tokens of all prompts (no pad rows: cu_seqlens + row_pos) on a HIP stream.
// The GEMMs, RMSNorm and the causal grouped-head attention are the library's existing kernels; this file holds the three row
// kernels that were missing and the driver.
//
// All three kernels are HBM-trivial: one wave per row segment, 16 bytes per lane per access, fp32 arithmetic, one rounding to bf16.
//   text_rope_neox_kernel    rotate-half (NeoX) RoPE in place on the q and k column blocks of the fused QKV buffer.  A text-only
//                            prompt gives the three M-RoPE position rows (temporal, height, width) EQUAL values, so whatever
//                            mrope_section selects, every rotary pair of a token sees the same position: this kernel IS
//                            Qwen2.5-VL's multimodal rotary embedding for such prompts.
//   text_mrope_kernel        the same with three position rows and mrope_section: prompts with pictures (the Edit pipelines,
//                            omni_qwen2_text_forward_mm); with equal rows it reproduces text_rope_neox_kernel bit for bit.
//                            bytes/row = 2 x 2 x (H + H_kv) x 128 + the row's 512 B of the cos / sin tables (L2-resident).
//   text_swiglu_kernel       y = silu(gate) * up from the [rows, 2 I] output of the fused gate|up GEMM, row-major or K32-blocked.
//                            bytes/row = 2 x 2 I read + 2 I written.
//   text_embed_gather_kernel h[r] = E[ids[r]]; an id outside [0, vocab) writes zeros and raises the error word, it never reads.
//   text_embed_gather_mm_kernel  ... or h[r] = V[vision_row_of[r]] where that is >= 0: the vision tower's rows scattered into the
//                            picture tokens, with the same rule for an index outside the rows.
#include "common.h"

namespace {

constexpr int TEXT_HEAD = 128;             // the only head size (the attention kernel's and the RoPE kernel's)
constexpr int TEXT_MAX_PROMPTS = 64;
constexpr size_t TEXT_ERR_BYTES = 256;     // the error word's slot at the front of the workspace

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

// the rotation of one lane's 8 pairs (i, i + 64) of one head: x points at element 8 j of the head, cp / sp at column 8 j of the
// position's table rows.  Shared by the one-position and the three-position kernel: the same loads and the same arithmetic.
OMNI_DEVINL void rope_rotate8(uint16_t* x, const float* cp, const float* sp) {
#pragma clang fp contract(off)
  const u32x4_t lo = *reinterpret_cast<const u32x4_t*>(x), hi = *reinterpret_cast<const u32x4_t*>(x + 64);
  const f32x4_t c0 = *reinterpret_cast<const f32x4_t*>(cp), c1 = *reinterpret_cast<const f32x4_t*>(cp + 4);
  const f32x4_t s0 = *reinterpret_cast<const f32x4_t*>(sp), s1 = *reinterpret_cast<const f32x4_t*>(sp + 4);
  float a[8], b[8], oa[8], ob[8];
  unpack8(lo, a);
  unpack8(hi, b);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float c = i < 4 ? c0[i & 3] : c1[i & 3], s = i < 4 ? s0[i & 3] : s1[i & 3];
    oa[i] = __builtin_fmaf(a[i], c, -(b[i] * s));
    ob[i] = __builtin_fmaf(b[i], c, a[i] * s);
  }
  *reinterpret_cast<u32x4_t*>(x) = pack8(oa);
  *reinterpret_cast<u32x4_t*>(x + 64) = pack8(ob);
}

// 8 lanes per head: lane j of a head holds elements 8 j .. 8 j + 7 AND their partners 64 + 8 j .. of the rotate-half pairs, so a
// wave covers 8 heads of one row and nothing crosses lanes.  unit = row * nseg + segment of 8 heads.
__global__ __launch_bounds__(256) void text_rope_neox_kernel(uint16_t* __restrict__ qkv, int64_t ld, int rows, int H, int H_kv,
                                                             const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
                                                             int npos, const int32_t* __restrict__ row_pos, int32_t* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int nheads = H + H_kv, nseg = (nheads + 7) >> 3;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t row = unit / nseg;
  if (row >= rows) return;
  const int head = (int)(unit - row * nseg) * 8 + (lane >> 3);
  if (head >= nheads) return;
  const int j = lane & 7;
  int p = row_pos[row];
  if (p < 0 || p >= npos) {                // never an out-of-range read of the tables: clamp, and say so
    if (err && j == 0) *err = 2;
    p = p < 0 ? 0 : npos - 1;
  }
  rope_rotate8(qkv + row * ld + (int64_t)head * TEXT_HEAD + 8 * j, cos_tab + (int64_t)p * 64 + 8 * j, sin_tab + (int64_t)p * 64 + 8 * j);
}

// Qwen2.5-VL's multimodal RoPE: the same kernel with three position rows [3][rows]; pairs 0 .. s0 - 1 of a head read the tables
// at the temporal position, s0 .. s0 + s1 - 1 at the height, the rest at the width position.  The sections are multiples of 8, so
// the 8 pairs of a lane lie in ONE section and the lane still reads one table row.
__global__ __launch_bounds__(256) void text_mrope_kernel(uint16_t* __restrict__ qkv, int64_t ld, int rows, int H, int H_kv,
                                                         const float* __restrict__ cos_tab, const float* __restrict__ sin_tab, int npos,
                                                         const int32_t* __restrict__ row_pos3, int s0, int s01,
                                                         int32_t* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int nheads = H + H_kv, nseg = (nheads + 7) >> 3;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t row = unit / nseg;
  if (row >= rows) return;
  const int head = (int)(unit - row * nseg) * 8 + (lane >> 3);
  if (head >= nheads) return;
  const int j = lane & 7;
  const int sec = 8 * j < s0 ? 0 : (8 * j < s01 ? 1 : 2);
  int p = row_pos3[(int64_t)sec * rows + row];
  if (p < 0 || p >= npos) {
    if (err) *err = 2;
    p = p < 0 ? 0 : npos - 1;
  }
  rope_rotate8(qkv + row * ld + (int64_t)head * TEXT_HEAD + 8 * j, cos_tab + (int64_t)p * 64 + 8 * j, sin_tab + (int64_t)p * 64 + 8 * j);
}

// unit = row * nseg + segment of 512 columns; a lane owns 8 consecutive columns of gate and the same 8 of up
__global__ __launch_bounds__(256) void text_swiglu_kernel(const uint16_t* __restrict__ gu, int64_t ldgu, uint16_t* __restrict__ y,
                                                          int64_t ldy, int rows, int I, int y_k32_rows) {
  const int lane = threadIdx.x & 63;
  const int nseg = (I + 511) >> 9;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t row = unit / nseg;
  if (row >= rows) return;
  const int e = ((int)(unit - row * nseg) * 64 + lane) * 8;
  if (e >= I) return;
  const uint16_t* g = gu + row * ldgu + e;
  const u32x4_t gw = *reinterpret_cast<const u32x4_t*>(g), uw = *reinterpret_cast<const u32x4_t*>(g + I);
  float gf[8], uf[8], o[8];
  unpack8(gw, gf);
  unpack8(uw, uf);
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = silu_f(gf[i]) * uf[i];
  // K32-blocked output: the 8 elements stay one 16-B granule, at ((e/32) * R + row) * 32 + e%32
  uint16_t* dst = y_k32_rows ? y + ((int64_t)(e >> 5) * y_k32_rows + row) * 32 + (e & 31) : y + row * ldy + e;
  *reinterpret_cast<u32x4_t*>(dst) = pack8(o);
}

__global__ __launch_bounds__(256) void text_embed_gather_kernel(const uint16_t* __restrict__ table, int vocab, int D,
                                                                const int32_t* __restrict__ ids, int rows,
                                                                uint16_t* __restrict__ h, int64_t ldh, int32_t* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int nseg = (D + 511) >> 9;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t row = unit / nseg;
  if (row >= rows) return;
  const int seg = (int)(unit - row * nseg);
  const int e = (seg * 64 + lane) * 8;
  const int id = ids[row];
  const bool ok = id >= 0 && id < vocab;
  if (!ok && err && seg == 0 && lane == 0) *err = 1;
  if (e >= D) return;
  u32x4_t v = {0u, 0u, 0u, 0u};
  if (ok) v = *reinterpret_cast<const u32x4_t*>(table + (int64_t)id * D + e);
  *reinterpret_cast<u32x4_t*>(h + row * ldh + e) = v;
}

// the same with the picture rows: a token row whose vision_row_of entry is >= 0 takes that row of the vision tower's output in
// place of its token embedding (HF's masked_scatter); an entry outside [-1, n_vision) writes zeros and raises the error word
__global__ __launch_bounds__(256) void text_embed_gather_mm_kernel(const uint16_t* __restrict__ table, int vocab, int D,
                                                                   const int32_t* __restrict__ ids,
                                                                   const uint16_t* __restrict__ vision, int n_vision,
                                                                   const int32_t* __restrict__ vision_row_of, int rows,
                                                                   uint16_t* __restrict__ h, int64_t ldh, int32_t* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int nseg = (D + 511) >> 9;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t row = unit / nseg;
  if (row >= rows) return;
  const int seg = (int)(unit - row * nseg);
  const int e = (seg * 64 + lane) * 8;
  const int vr = vision_row_of[row];
  const uint16_t* src = nullptr;
  int code = 0;
  if (vr >= 0) {
    if (vr < n_vision) src = vision + (int64_t)vr * D;
    else code = 3;
  } else if (vr == -1) {
    const int id = ids[row];
    if (id >= 0 && id < vocab) src = table + (int64_t)id * D;
    else code = 1;
  } else {
    code = 3;
  }
  if (code && err && seg == 0 && lane == 0) *err = code;
  if (e >= D) return;
  u32x4_t v = {0u, 0u, 0u, 0u};
  if (src) v = *reinterpret_cast<const u32x4_t*>(src + e);
  *reinterpret_cast<u32x4_t*>(h + row * ldh + e) = v;
}

inline unsigned wave_blocks(int64_t units) { return (unsigned)((units + 3) / 4); }

int text_rope_neox(omni_bf16* qkv, int64_t ld, int32_t rows, int32_t H, int32_t H_kv, const float* cos_tab, const float* sin_tab,
                   int32_t npos, const int32_t* row_pos, int32_t* err, omni_stream stream) {
  if (!qkv || !cos_tab || !sin_tab || !row_pos || rows <= 0 || H <= 0 || H_kv <= 0 || npos <= 0) return OMNI_ERR_BAD_ARG;
  if (ld < (int64_t)(H + 2 * H_kv) * TEXT_HEAD) return OMNI_ERR_BAD_ARG;
  if (!omni_aligned16(qkv) || !omni_aligned16(cos_tab) || !omni_aligned16(sin_tab) || (ld % 8)) return OMNI_ERR_ALIGN;
  const int64_t units = (int64_t)rows * ((H + H_kv + 7) / 8);
  if (units > 0x7fffffffLL) return OMNI_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(text_rope_neox_kernel, dim3(wave_blocks(units)), dim3(256), 0, static_cast<hipStream_t>(stream), qkv, ld, rows,
                     H, H_kv, cos_tab, sin_tab, npos, row_pos, err);
  OMNI_CHECK_LAUNCH();
  return OMNI_OK;
}

int text_mrope(omni_bf16* qkv, int64_t ld, int32_t rows, int32_t H, int32_t H_kv, const float* cos_tab, const float* sin_tab,
               int32_t npos, const int32_t* row_pos3, const int32_t* sec, int32_t* err, omni_stream stream) {
  if (!qkv || !cos_tab || !sin_tab || !row_pos3 || !sec || rows <= 0 || H <= 0 || H_kv <= 0 || npos <= 0) return OMNI_ERR_BAD_ARG;
  if (ld < (int64_t)(H + 2 * H_kv) * TEXT_HEAD) return OMNI_ERR_BAD_ARG;
  if (sec[0] < 0 || sec[1] < 0 || sec[2] < 0 || (int64_t)sec[0] + sec[1] + sec[2] != TEXT_HEAD / 2) return OMNI_ERR_BAD_ARG;
  if (sec[0] % 8 || sec[1] % 8 || sec[2] % 8) return OMNI_ERR_UNSUPPORTED;
  if (!omni_aligned16(qkv) || !omni_aligned16(cos_tab) || !omni_aligned16(sin_tab) || (ld % 8)) return OMNI_ERR_ALIGN;
  const int64_t units = (int64_t)rows * ((H + H_kv + 7) / 8);
  if (units > 0x7fffffffLL) return OMNI_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(text_mrope_kernel, dim3(wave_blocks(units)), dim3(256), 0, static_cast<hipStream_t>(stream), qkv, ld, rows, H,
                     H_kv, cos_tab, sin_tab, npos, row_pos3, sec[0], sec[0] + sec[1], err);
  OMNI_CHECK_LAUNCH();
  return OMNI_OK;
}

int text_swiglu(const omni_bf16* gate_up, int64_t ldgu, omni_bf16* y, int64_t ldy, int32_t rows, int32_t I, int32_t y_k32_rows,
                omni_stream stream) {
  if (!gate_up || !y || rows <= 0 || I <= 0 || y_k32_rows < 0) return OMNI_ERR_BAD_ARG;
  if (I % 8 || (y_k32_rows && I % 32)) return OMNI_ERR_UNSUPPORTED;
  if (ldgu < 2 * (int64_t)I || (y_k32_rows ? y_k32_rows < rows : ldy < I)) return OMNI_ERR_BAD_ARG;
  if (!omni_aligned16(gate_up) || !omni_aligned16(y) || (ldgu % 8) || (!y_k32_rows && (ldy % 8))) return OMNI_ERR_ALIGN;
  const int64_t units = (int64_t)rows * ((I + 511) / 512);
  if (units > 0x7fffffffLL) return OMNI_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(text_swiglu_kernel, dim3(wave_blocks(units)), dim3(256), 0, static_cast<hipStream_t>(stream), gate_up, ldgu, y,
                     ldy, rows, I, y_k32_rows);
  OMNI_CHECK_LAUNCH();
  return OMNI_OK;
}

int text_embed_gather(const omni_bf16* table, int32_t vocab, int32_t D, const int32_t* ids, int32_t rows, omni_bf16* h, int64_t ldh,
                      int32_t* err, omni_stream stream) {
  if (!table || !ids || !h || !err || vocab <= 0 || D <= 0 || rows <= 0 || ldh < D) return OMNI_ERR_BAD_ARG;
  if (D % 8) return OMNI_ERR_UNSUPPORTED;
  if (!omni_aligned16(table) || !omni_aligned16(h) || (ldh % 8)) return OMNI_ERR_ALIGN;
  const int64_t units = (int64_t)rows * ((D + 511) / 512);
  if (units > 0x7fffffffLL) return OMNI_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(text_embed_gather_kernel, dim3(wave_blocks(units)), dim3(256), 0, static_cast<hipStream_t>(stream), table, vocab,
                     D, ids, rows, h, ldh, err);
  OMNI_CHECK_LAUNCH();
  return OMNI_OK;
}

int text_embed_gather_mm(const omni_bf16* table, int32_t vocab, int32_t D, const int32_t* ids, const omni_bf16* vision,
                         int32_t n_vision, const int32_t* vision_row_of, int32_t rows, omni_bf16* h, int64_t ldh, int32_t* err,
                         omni_stream stream) {
  if (!table || !ids || !h || !err || !vision || !vision_row_of || vocab <= 0 || D <= 0 || rows <= 0 || n_vision <= 0 || ldh < D)
    return OMNI_ERR_BAD_ARG;
  if (D % 8) return OMNI_ERR_UNSUPPORTED;
  if (!omni_aligned16(table) || !omni_aligned16(vision) || !omni_aligned16(h) || (ldh % 8)) return OMNI_ERR_ALIGN;
  const int64_t units = (int64_t)rows * ((D + 511) / 512);
  if (units > 0x7fffffffLL) return OMNI_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(text_embed_gather_mm_kernel, dim3(wave_blocks(units)), dim3(256), 0, static_cast<hipStream_t>(stream), table,
                     vocab, D, ids, vision, n_vision, vision_row_of, rows, h, ldh, err);
  OMNI_CHECK_LAUNCH();
  return OMNI_OK;
}

// ---- driver ---------------------------------------------------------------------------------------------------------------
struct TextWorkspace {
  int32_t* err;                 // the device error word (its own 256 bytes at the front)
  omni_bf16 *h, *xn, *qkv, *attn, *gu, *act;
  float* splitk;                // fp32 partial tiles of the split-K GEMMs: a request's few hundred rows are one or two row tiles,
  int64_t splitk_floats;        // so the N = D / (H + 2 H_kv) 128 launches would stream their weights through 14 .. 18 workgroups
  size_t total;
};

inline size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

TextWorkspace carve(void* base, const omni_text_weights* w, int64_t R) {
  const int64_t D = w->hidden_size, I = w->intermediate_size;
  const int64_t Nq = (int64_t)w->num_heads * TEXT_HEAD, Nqkv = Nq + 2 * (int64_t)w->num_kv_heads * TEXT_HEAD;
  size_t off = 0;
  char* b = static_cast<char*>(base);
  auto take = [&](int64_t elems) {
    omni_bf16* p = reinterpret_cast<omni_bf16*>(b + off);
    off += align_up((size_t)elems * sizeof(omni_bf16));
    return p;
  };
  TextWorkspace ws;
  ws.err = reinterpret_cast<int32_t*>(take((int64_t)(TEXT_ERR_BYTES / sizeof(omni_bf16))));
  ws.h = take(R * D);
  ws.xn = take(R * D);
  ws.qkv = take(R * Nqkv);
  ws.attn = take(R * Nq);
  ws.gu = take(R * 2 * I);
  ws.act = take(R * I);
  // up to 8 splits x rows x the widest N that splits (the gate|up launch has too many tiles to split at real width; where it is
  // narrow enough to, it takes whatever factor this size allows); beyond ten row tiles no launch splits and there is no buffer
  const int64_t nmax = Nqkv > D ? Nqkv : D;
  ws.splitk_floats = R <= 10 * 256 ? 8 * R * nmax : 0;
  ws.splitk = ws.splitk_floats ? reinterpret_cast<float*>(take(ws.splitk_floats * 2)) : nullptr;
  ws.total = off;
  return ws;
}

// everything a call can refuse before it touches the device
int text_check_weights(const omni_text_weights* w) {
  if (!w || !w->layers || !w->embed_tokens || !w->final_norm_w || !w->ones || !w->rope_cos || !w->rope_sin) return OMNI_ERR_BAD_ARG;
  if (w->num_layers <= 0 || w->hidden_size <= 0 || w->intermediate_size <= 0 || w->num_heads <= 0 || w->num_kv_heads <= 0 ||
      w->vocab_size <= 0 || w->rope_npos <= 0)
    return OMNI_ERR_BAD_ARG;
  if (w->gemm_w_k32_blocked != 0 && w->gemm_w_k32_blocked != 1) return OMNI_ERR_BAD_ARG;
  if (w->head_dim != TEXT_HEAD) return OMNI_ERR_UNSUPPORTED;
  if (w->hidden_size % 64 != 0 || w->intermediate_size % 64 != 0 || w->hidden_size > 8192) return OMNI_ERR_UNSUPPORTED;
  if (w->num_heads % w->num_kv_heads != 0) return OMNI_ERR_UNSUPPORTED;
  return OMNI_OK;
}

size_t text_workspace_bytes(const omni_text_weights* w, int32_t total_rows) {
  if (text_check_weights(w) != OMNI_OK || total_rows <= 0) return 0;
  return carve(nullptr, w, total_rows).total;
}

// y = res + 1 * (A W^T): the existing gated-residual epilogue with a gate vector of bf16 ones and no bias (exact: the product is
// rounded to bf16 and added to the residual stream, as HF's `residual + hidden_states` does)
int residual_gemm(const omni_text_weights* w, const TextWorkspace& ws, const omni_bf16* A, int32_t a_k32_rows, int32_t K,
                  const omni_bf16* W, int32_t R, omni_stream stream) {
  const int32_t D = w->hidden_size;
  omni_gemm_params p = {};
  p.ngroups = 1; p.N = D; p.K = K; p.epilogue = OMNI_EPI_BIAS_GATE_RES; p.w_k32_blocked = w->gemm_w_k32_blocked;
  p.g[0].A = A; p.g[0].lda = K; p.g[0].a_k32_rows = a_k32_rows; p.g[0].M = R; p.g[0].W = W;
  p.g[0].out = ws.h; p.g[0].ldo = D; p.g[0].res = ws.h; p.g[0].ldres = D;
  p.g[0].gate = w->ones; p.g[0].gate_item_stride = 0; p.g[0].rows_per_item = R;       // every row is item 0
  p.splitk_ws = ws.splitk; p.splitk_ws_floats = ws.splitk_floats;
  return omni_gemm_bf16(&p, stream);
}

// what omni_qwen2_text_forward_mm adds to a batch; null for omni_qwen2_text_forward
struct TextMm {
  const int32_t* row_pos3;
  const int32_t* section;
  const omni_bf16* vision_rows;
  const int32_t* vision_row_of;
  int32_t n_vision_rows;
};

// the one driver of both entry points: `b` holds the fields the two batch structs share
// (`sink`, the prefill of the greedy decode: each layer's K and V rows are also written into the KV cache, after RoPE)
int text_forward_impl(const omni_text_weights* w, const omni_text_batch* b, const TextMm* mm, omni_stream stream,
                      const omni_text_kv_sink* sink = nullptr) {
  OMNI_TRY_STATUS(text_check_weights(w));
  if (!b->input_ids || !b->cu_seqlens || !b->out || !b->workspace) return OMNI_ERR_BAD_ARG;
  if (mm) {
    if (!mm->row_pos3 || mm->n_vision_rows < 0 || (mm->n_vision_rows > 0 && (!mm->vision_rows || !mm->vision_row_of)))
      return OMNI_ERR_BAD_ARG;
    const int32_t* sec = mm->section;
    if (sec[0] < 0 || sec[1] < 0 || sec[2] < 0 || (int64_t)sec[0] + sec[1] + sec[2] != TEXT_HEAD / 2) return OMNI_ERR_BAD_ARG;
    if (sec[0] % 8 || sec[1] % 8 || sec[2] % 8) return OMNI_ERR_UNSUPPORTED;
    if (mm->vision_rows && !omni_aligned16(mm->vision_rows)) return OMNI_ERR_ALIGN;
  } else if (!b->row_pos) {
    return OMNI_ERR_BAD_ARG;
  }
  if (b->n_prompts <= 0 || b->total_rows <= 0 || b->max_seqlen <= 0 || b->max_seqlen > b->total_rows) return OMNI_ERR_BAD_ARG;
  if (b->n_prompts > TEXT_MAX_PROMPTS) return OMNI_ERR_UNSUPPORTED;
  if (!omni_aligned16(b->workspace) || !omni_aligned16(b->out)) return OMNI_ERR_ALIGN;
  for (int l = 0; l < w->num_layers; ++l) {
    const omni_text_layer_weights& L = w->layers[l];
    if (!L.input_norm_w || !L.qkv_w || !L.qkv_b || !L.o_w || !L.post_norm_w || !L.gate_up_w || !L.down_w) return OMNI_ERR_BAD_ARG;
  }
  const int32_t R = b->total_rows, D = w->hidden_size, I = w->intermediate_size, H = w->num_heads, Hkv = w->num_kv_heads;
  const int32_t Nq = H * TEXT_HEAD, Nqkv = (H + 2 * Hkv) * TEXT_HEAD;
  const TextWorkspace ws = carve(b->workspace, w, R);
  if (ws.total > b->workspace_bytes) return OMNI_ERR_BAD_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);

  // the error word of the PREVIOUS forward over this workspace (a token id outside the vocabulary, a position outside the RoPE
  // table): reported now, and cleared.  The only host read of the call, in front of its first launch.
  int32_t prev = 0;
  if (hipMemcpyAsync(&prev, ws.err, sizeof(prev), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return OMNI_ERR_LAUNCH;
  if (prev != 0) {
    if (hipMemsetAsync(ws.err, 0, sizeof(int32_t), s) != hipSuccess) return OMNI_ERR_LAUNCH;
    return OMNI_ERR_BAD_ARG;
  }

  if (mm && mm->n_vision_rows > 0)
    OMNI_TRY_STATUS(text_embed_gather_mm(w->embed_tokens, w->vocab_size, D, b->input_ids, mm->vision_rows, mm->n_vision_rows,
                                         mm->vision_row_of, R, ws.h, D, ws.err, stream));
  else
    OMNI_TRY_STATUS(text_embed_gather(w->embed_tokens, w->vocab_size, D, b->input_ids, R, ws.h, D, ws.err, stream));
  const float sm_scale = 1.0f / sqrtf((float)TEXT_HEAD);
  for (int l = 0; l < w->num_layers; ++l) {
    const omni_text_layer_weights& L = w->layers[l];
    // input_layernorm -> fused q|k|v projection (HF Qwen2_5_VLDecoderLayer.forward / Qwen2_5_VLAttention.forward)
    OMNI_TRY_STATUS(omni_rmsnorm(ws.h, D, ws.xn, D, R, D, L.input_norm_w, w->rms_norm_eps, stream));
    {
      omni_gemm_params p = {};
      p.ngroups = 1; p.N = Nqkv; p.K = D; p.epilogue = OMNI_EPI_BIAS; p.w_k32_blocked = w->gemm_w_k32_blocked;
      p.g[0].A = ws.xn; p.g[0].lda = D; p.g[0].M = R; p.g[0].W = L.qkv_w; p.g[0].bias = L.qkv_b;
      p.g[0].out = ws.qkv; p.g[0].ldo = Nqkv;
      p.splitk_ws = ws.splitk; p.splitk_ws_floats = ws.splitk_floats;
      OMNI_TRY_STATUS(omni_gemm_bf16(&p, stream));
    }
    // (q is not pre-scaled as the DiT path does it: the general attention kernel multiplies the fp32 scores by softmax_scale *
    // log2(e) either way, so a scale folded into q would save nothing and 1 / sqrt(128), no power of two, would add a rounding)
    if (mm)
      OMNI_TRY_STATUS(text_mrope(ws.qkv, Nqkv, R, H, Hkv, w->rope_cos, w->rope_sin, w->rope_npos, mm->row_pos3, mm->section, ws.err,
                                 stream));
    else
      OMNI_TRY_STATUS(text_rope_neox(ws.qkv, Nqkv, R, H, Hkv, w->rope_cos, w->rope_sin, w->rope_npos, b->row_pos, ws.err, stream));
    if (sink) OMNI_TRY_STATUS(omni_internal_text_kv_write(ws.qkv, Nqkv, R, H, Hkv, sink, l, b->cu_seqlens, nullptr, stream));
    {
      omni_attn_params ap = {};
      ap.q = ws.qkv; ap.k = ws.qkv + Nq; ap.v = ws.qkv + Nq + Hkv * TEXT_HEAD; ap.out = ws.attn;
      ap.ldq = ap.ldk = ap.ldv = Nqkv; ap.ldo = Nq;
      ap.cu_seqlens_q = ap.cu_seqlens_k = b->cu_seqlens;
      ap.B = b->n_prompts; ap.H = H; ap.H_kv = Hkv; ap.head_dim = TEXT_HEAD;
      ap.max_seqlen_q = ap.max_seqlen_k = b->max_seqlen;
      ap.softmax_scale = sm_scale; ap.causal = 1;
      OMNI_TRY_STATUS(omni_flash_attn_general(&ap, stream));
    }
    OMNI_TRY_STATUS(residual_gemm(w, ws, ws.attn, 0, Nq, L.o_w, R, stream));
    // post_attention_layernorm -> fused gate|up -> SwiGLU (K32-blocked: only the down-projection reads it) -> down + residual
    OMNI_TRY_STATUS(omni_rmsnorm(ws.h, D, ws.xn, D, R, D, L.post_norm_w, w->rms_norm_eps, stream));
    {
      omni_gemm_params p = {};
      p.ngroups = 1; p.N = 2 * I; p.K = D; p.epilogue = OMNI_EPI_BIAS; p.w_k32_blocked = w->gemm_w_k32_blocked;
      p.g[0].A = ws.xn; p.g[0].lda = D; p.g[0].M = R; p.g[0].W = L.gate_up_w;
      p.g[0].out = ws.gu; p.g[0].ldo = 2 * (int64_t)I;
      p.splitk_ws = ws.splitk; p.splitk_ws_floats = ws.splitk_floats;
      OMNI_TRY_STATUS(omni_gemm_bf16(&p, stream));
    }
    OMNI_TRY_STATUS(text_swiglu(ws.gu, 2 * (int64_t)I, ws.act, I, R, I, R, stream));
    OMNI_TRY_STATUS(residual_gemm(w, ws, ws.act, R, I, L.down_w, R, stream));
  }
  // HF's hidden_states[-1] is the output of the final norm
  return omni_rmsnorm(ws.h, D, b->out, D, R, D, w->final_norm_w, w->rms_norm_eps, stream);
}

int text_forward(const omni_text_weights* w, const omni_text_batch* b, omni_stream stream) {
  if (!b) return OMNI_ERR_BAD_ARG;
  return text_forward_impl(w, b, nullptr, stream);
}

int text_forward_mm_sink(const omni_text_weights* w, const omni_text_batch_mm* b, const omni_text_kv_sink* sink, omni_stream stream) {
  if (!b) return OMNI_ERR_BAD_ARG;
  omni_text_batch base = {};
  base.n_prompts = b->n_prompts; base.total_rows = b->total_rows; base.max_seqlen = b->max_seqlen;
  base.input_ids = b->input_ids; base.cu_seqlens = b->cu_seqlens; base.out = b->out;
  base.workspace = b->workspace; base.workspace_bytes = b->workspace_bytes;
  const TextMm mm = {b->row_pos3, b->mrope_section, b->vision_rows, b->vision_row_of, b->n_vision_rows};
  return text_forward_impl(w, &base, &mm, stream, sink);
}

int text_forward_mm(const omni_text_weights* w, const omni_text_batch_mm* b, omni_stream stream) {
  return text_forward_mm_sink(w, b, nullptr, stream);
}

}  // namespace

int omni_internal_text_forward_mm(const omni_text_weights* w, const omni_text_batch_mm* b, const omni_text_kv_sink* sink, void* stream) {
  return text_forward_mm_sink(w, b, sink, stream);
}
int omni_internal_text_check_weights(const omni_text_weights* w) { return text_check_weights(w); }

// exported as const pointers, not as functions: see the header (the exported functions of ABI v14 are fixed).  Host pass only:
// a namespace-scope const would otherwise be emitted for the device as well, where its initialiser does not exist
#if !defined(__HIP_DEVICE_COMPILE__)
extern "C" int (*const omni_qwen2_text_forward)(const omni_text_weights*, const omni_text_batch*, omni_stream) = text_forward;
extern "C" size_t (*const omni_qwen2_text_workspace_bytes)(const omni_text_weights*, int32_t) = text_workspace_bytes;
extern "C" int (*const omni_text_rope_neox)(omni_bf16*, int64_t, int32_t, int32_t, int32_t, const float*, const float*, int32_t,
                                            const int32_t*, int32_t*, omni_stream) = text_rope_neox;
extern "C" int (*const omni_qwen2_text_forward_mm)(const omni_text_weights*, const omni_text_batch_mm*, omni_stream) = text_forward_mm;
extern "C" int (*const omni_text_mrope)(omni_bf16*, int64_t, int32_t, int32_t, int32_t, const float*, const float*, int32_t,
                                        const int32_t*, const int32_t*, int32_t*, omni_stream) = text_mrope;
extern "C" int (*const omni_text_swiglu)(const omni_bf16*, int64_t, omni_bf16*, int64_t, int32_t, int32_t, int32_t,
                                         omni_stream) = text_swiglu;
extern "C" int (*const omni_text_embed_gather)(const omni_bf16*, int32_t, int32_t, const int32_t*, int32_t, omni_bf16*, int64_t,
                                               int32_t*, omni_stream) = text_embed_gather;
#endif
