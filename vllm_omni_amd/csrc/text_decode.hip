// Greedy decode of the Qwen2.5-VL text model with a KV cache (the auto-caption of the Layered pipeline, reference
// pipeline_qwen_image_layered.py:495-513 `text_encoder.generate`): omni_qwen2_text_prefill fills the cache through
// text_forward.hip's driver and picks the first token; omni_qwen2_text_decode_step enqueues one token for every live sequence
// and reads nothing back - position, length and the stop flags are device memory, so the host queues steps back to back.
//
// A step is M = n_seq <= 8 rows against 14 GB of weights: pure weight streaming.  The kernels of this file:
//   gemv_kernel<M, BLOCKED>   out[m, n] = sum_k A[m, k] W[n, k] for 8 columns per workgroup.  A lane owns ONE column and 8
//                             consecutive k (one 16-byte load, straight to VGPRs: nothing is shared between waves, an LDS round
//                             trip would be overhead); lane = (k-block parity, column, quarter of the 32-k block), so a wave
//                             instruction reads two 512-byte runs of the K32-blocked layout [K/32][N][32] and eight full 128-byte
//                             lines of the row-major one - the weights are read where they lie.  The four waves take every
//                             fourth pair of k-blocks; their fp32 partial sums meet in LDS (64 floats per row), not in HBM.
//                             Grid ceil(N / 8): 448 workgroups of 4 waves at N = 3584, 19008 at the lm_head.
//                             bytes = N K 2 (weights, once) + M K 2 per workgroup from L2.
//   decode_attn_score_kernel<G> / decode_attn_pv_kernel<G>   one workgroup per (key chunk of 64, K/V head, sequence); 16 lanes
//                             hold one key row (16 bytes each), a wave instruction four keys; the G <= 8 query heads of the K/V
//                             head share every K and V load.  The arithmetic is the prefill attention's, tile for tile (see
//                             there), so a step and a prefill over the same tokens round in the same places; its one
//                             sequential piece, the running maximum, is a prefix maximum over the chunk maxima the score kernel
//                             writes.  One fp32 partial (m, l, 128 values) per (head, chunk).  Workgroups behind the
//                             sequence's length exit: the grid is sized by the capacity because the host never reads the length.
//   decode_attn_combine_kernel  the chunks of one (sequence, head) folded with exp2(m_chunk - m_row) -> bf16.
//   penalized_argmax_kernel   HF's repetition penalty, argmax with the lowest index on ties, EOS test, and the step's bookkeeping.
//   kv_write_kernel           K / V rows of the fused q|k|v buffer -> cache (prefill: all rows; step: one row per sequence).
//   decode_begin / prefill_mark / gather_rows: the few words of glue.
// Counters and flags are written by ordinary vector stores of one lane.
#include "common.h"

namespace {

constexpr int DEC_HEAD = 128;
constexpr int DEC_MAX_SEQ = 8;
constexpr int DEC_CHUNK = OMNI_DECODE_ATTN_CHUNK;
constexpr float DEC_NEG = -1.0e30f;

OMNI_DEVINL void dec_unpack8(const u32x4_t& w, float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = bf16_lo(w[i]);
    f[2 * i + 1] = bf16_hi(w[i]);
  }
}

// ---- GEMV -----------------------------------------------------------------------------------------------------------------
template <int M, bool BLOCKED>
__global__ __launch_bounds__(256) void gemv_kernel(omni_gemv_params p) {
  __shared__ float red[4][M][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = (lane >> 2) & 7, q = lane & 3, ks = lane >> 5;
  const int N = p.N, K = p.K, nkb = K >> 5;
  const int n = min((int)blockIdx.x * 8 + c, N - 1);                 // a column behind N re-reads the last one and stores nothing
  const uint16_t* wp = BLOCKED ? p.W + ((int64_t)n * 32 + q * 8) : p.W + ((int64_t)n * K + q * 8);
  const int64_t wstep = BLOCKED ? (int64_t)N * 32 : 32;              // elements from one k-block of a column to the next
  const uint16_t* ap = p.A + q * 8;
  float acc[M];
#pragma unroll
  for (int m = 0; m < M; ++m) acc[m] = 0.f;
#pragma unroll 4
  for (int kb = wave * 2 + ks; kb < nkb; kb += 8) {
    const u32x4_t wv = *reinterpret_cast<const u32x4_t*>(wp + kb * wstep);
    float wf[8];
    dec_unpack8(wv, wf);
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const u32x4_t av = *reinterpret_cast<const u32x4_t*>(ap + m * p.lda + kb * 32);
      float af[8];
      dec_unpack8(av, af);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[m] = __builtin_fmaf(af[i], wf[i], acc[m]);
    }
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    float v = acc[m];
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 32, 64);
    if (q == 0 && ks == 0) red[wave][m][c] = v;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t >= M * 8) return;
  const int m = t >> 3, cc = t & 7, col = (int)blockIdx.x * 8 + cc;
  if (col >= N) return;
  float v = (red[0][m][cc] + red[1][m][cc]) + (red[2][m][cc] + red[3][m][cc]);
  if (p.bias) v += bf16_bits_to_f32(p.bias[col]);
  if (p.out_f32) {
    p.out_f32[m * p.ldo + col] = v;
    return;
  }
  uint16_t y = f32_to_bf16_bits(v);
  if (p.res) y = f32_to_bf16_bits(bf16_bits_to_f32(p.res[m * p.ldres + col]) + bf16_bits_to_f32(y));   // bf16(product), then the add
  p.out[m * p.ldo + col] = y;
}

template <bool BLOCKED>
void gemv_launch(const omni_gemv_params& p, hipStream_t s) {
  const dim3 grid((unsigned)((p.N + 7) / 8)), block(256);
  switch (p.M) {
    case 1: hipLaunchKernelGGL((gemv_kernel<1, BLOCKED>), grid, block, 0, s, p); break;
    case 2: hipLaunchKernelGGL((gemv_kernel<2, BLOCKED>), grid, block, 0, s, p); break;
    case 3: hipLaunchKernelGGL((gemv_kernel<3, BLOCKED>), grid, block, 0, s, p); break;
    case 4: hipLaunchKernelGGL((gemv_kernel<4, BLOCKED>), grid, block, 0, s, p); break;
    case 5: hipLaunchKernelGGL((gemv_kernel<5, BLOCKED>), grid, block, 0, s, p); break;
    case 6: hipLaunchKernelGGL((gemv_kernel<6, BLOCKED>), grid, block, 0, s, p); break;
    case 7: hipLaunchKernelGGL((gemv_kernel<7, BLOCKED>), grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL((gemv_kernel<8, BLOCKED>), grid, block, 0, s, p); break;
  }
}

int gemv_bf16(const omni_gemv_params* p, omni_stream stream) {
  if (!p || !p->A || !p->W || (!p->out && !p->out_f32)) return OMNI_ERR_BAD_ARG;
  if (p->M < 1 || p->N < 1 || p->K < 1 || p->lda < p->K || p->ldo < p->N) return OMNI_ERR_BAD_ARG;
  if (p->res && p->ldres < p->N) return OMNI_ERR_BAD_ARG;
  if (p->w_k32_blocked != 0 && p->w_k32_blocked != 1) return OMNI_ERR_BAD_ARG;
  if (p->M > 8 || p->K % 32 != 0 || (p->out && p->out_f32) || (p->out_f32 && p->res)) return OMNI_ERR_UNSUPPORTED;
  if (!omni_aligned16(p->A) || !omni_aligned16(p->W) || p->lda % 8 != 0) return OMNI_ERR_ALIGN;
  if (p->w_k32_blocked) gemv_launch<true>(*p, static_cast<hipStream_t>(stream));
  else gemv_launch<false>(*p, static_cast<hipStream_t>(stream));
  OMNI_CHECK_LAUNCH();
  return OMNI_OK;
}

// ---- decode attention -----------------------------------------------------------------------------------------------------
// The arithmetic is the prefill attention's (attention_common.h attn_softmax_pv_tile, tiles of 64 keys from key 0), so that a
// decode step and a prefill over the same tokens round in the same places: scores = (q . k) * (scale log2 e) in fp32; tile t
// uses m_t = the maximum over tiles 0 .. t; p = exp2(s - m_t), summed in fp32 and ROUNDED TO bf16 for the product with V;
// the partial sums of tile t carry the factor exp2(m_t - m_last); out = bf16(o * (1 / l)).  The running maximum is the one
// sequential piece: it is a prefix maximum over the per-chunk maxima, which the score kernel leaves in the workspace.
struct AttnWs {
  float* acc;                   // [n_seq][H][nchunk][128]
  float* ml;                    // [n_seq][H][nchunk][2]
  float* score;                 // [n_seq][H][nchunk * 64]
  float* cmax;                  // [n_seq][H][nchunk]
  size_t total;
};
inline size_t dec_align(size_t x) { return (x + 255) & ~size_t(255); }
inline int dec_chunks(int capacity) { return (capacity + DEC_CHUNK - 1) / DEC_CHUNK; }
AttnWs attn_carve(void* base, int64_t n_seq, int64_t H, int64_t capacity) {
  const int64_t units = n_seq * H * dec_chunks((int)capacity);
  AttnWs w;
  char* b = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t floats) {
    float* p = reinterpret_cast<float*>(b + off);
    off += dec_align(floats * sizeof(float));
    return p;
  };
  w.acc = take((size_t)units * DEC_HEAD);
  w.ml = take((size_t)units * 2);
  w.score = take((size_t)units * DEC_CHUNK);
  w.cmax = take((size_t)units);
  w.total = off;
  return w;
}

// scores of one chunk of 64 keys for the G query heads of one K/V head, and the chunk's maximum per head
template <int G>
__global__ __launch_bounds__(256) void decode_attn_score_kernel(omni_decode_attn_params p, float* __restrict__ score,
                                                                float* __restrict__ cmax) {
  __shared__ float s_m[4][G];
  const int chunk = blockIdx.x, kh = blockIdx.y, s = blockIdx.z;
  if (p.done && p.done[s]) return;
  const int n_keys = min(p.lens[s] + p.len_add, p.capacity);
  if (chunk * DEC_CHUNK >= n_keys) return;                        // (also n_keys < 1)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane >> 4, j = lane & 15;
  const int nchunk = (p.capacity + DEC_CHUNK - 1) / DEC_CHUNK;
  const float sl2 = p.softmax_scale * OMNI_LOG2E;
  float qf[G][8], m[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const u32x4_t qv = *reinterpret_cast<const u32x4_t*>(p.q + s * p.ldq + (int64_t)(kh * G + g) * DEC_HEAD + j * 8);
    dec_unpack8(qv, qf[g]);
    m[g] = -__builtin_inff();
  }
  const int64_t base = ((int64_t)s * p.H_kv + kh) * p.capacity;
#pragma unroll
  for (int it = 0; it < DEC_CHUNK / 16; ++it) {
    const int kl = wave * (DEC_CHUNK / 4) + it * 4 + sub, key = chunk * DEC_CHUNK + kl;
    const bool valid = key < n_keys;
    const u32x4_t kv = *reinterpret_cast<const u32x4_t*>(p.k_cache + (base + (valid ? key : n_keys - 1)) * DEC_HEAD + j * 8);
    float kf[8];
    dec_unpack8(kv, kf);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) d = __builtin_fmaf(qf[g][i], kf[i], d);
      d = row16_sum(d) * sl2;
      if (valid) {
        m[g] = fmaxf(m[g], d);
        if (j == 0) score[(((int64_t)s * p.H + kh * G + g) * nchunk + chunk) * DEC_CHUNK + kl] = d;
      }
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float mo = fmaxf(m[g], __shfl_xor(m[g], 16, 64));
    mo = fmaxf(mo, __shfl_xor(mo, 32, 64));
    if (lane == 0) s_m[wave][g] = mo;
  }
  __syncthreads();
  if (threadIdx.x < G) {
    const int g = threadIdx.x;
    cmax[((int64_t)s * p.H + kh * G + g) * nchunk + chunk] = fmaxf(fmaxf(s_m[0][g], s_m[1][g]), fmaxf(s_m[2][g], s_m[3][g]));
  }
}

// p = exp2(score - prefix maximum), l += p (fp32), o += bf16(p) * v: one fp32 partial (m, l, 128 values) per (head, chunk)
template <int G>
__global__ __launch_bounds__(256) void decode_attn_pv_kernel(omni_decode_attn_params p, const float* __restrict__ score,
                                                             const float* __restrict__ cmax, float* __restrict__ part_acc,
                                                             float* __restrict__ part_ml) {
  __shared__ float s_l[4][G];
  __shared__ float s_acc[4][G][DEC_HEAD];
  const int chunk = blockIdx.x, kh = blockIdx.y, s = blockIdx.z;
  if (p.done && p.done[s]) return;
  const int n_keys = min(p.lens[s] + p.len_add, p.capacity);
  if (chunk * DEC_CHUNK >= n_keys) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane >> 4, j = lane & 15;
  const int nchunk = (p.capacity + DEC_CHUNK - 1) / DEC_CHUNK;
  float acc[G][8], m[G], l[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float* cm = cmax + ((int64_t)s * p.H + kh * G + g) * nchunk;
    float mo = cm[0];
    for (int c = 1; c <= chunk; ++c) mo = fmaxf(mo, cm[c]);
    m[g] = mo;
    l[g] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[g][i] = 0.f;
  }
  const int64_t base = ((int64_t)s * p.H_kv + kh) * p.capacity;
#pragma unroll
  for (int it = 0; it < DEC_CHUNK / 16; ++it) {
    const int kl = wave * (DEC_CHUNK / 4) + it * 4 + sub, key = chunk * DEC_CHUNK + kl;
    const bool valid = key < n_keys;
    const u32x4_t vv = *reinterpret_cast<const u32x4_t*>(p.v_cache + (base + (valid ? key : n_keys - 1)) * DEC_HEAD + j * 8);
    float vf[8];
    dec_unpack8(vv, vf);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float pr = 0.f;
      if (valid) pr = __builtin_amdgcn_exp2f(score[(((int64_t)s * p.H + kh * G + g) * nchunk + chunk) * DEC_CHUNK + kl] - m[g]);
      l[g] += pr;
      const float pb = bf16_bits_to_f32(f32_to_bf16_bits(pr));
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[g][i] = __builtin_fmaf(pb, vf[i], acc[g][i]);
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float lv = l[g];
    lv += __shfl_xor(lv, 16, 64);
    lv += __shfl_xor(lv, 32, 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float a = acc[g][i];
      a += __shfl_xor(a, 16, 64);
      a += __shfl_xor(a, 32, 64);
      if (sub == 0) s_acc[wave][g][j * 8 + i] = a;
    }
    if (lane == 0) s_l[wave][g] = lv;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < G * DEC_HEAD; idx += 256) {
    const int g = idx >> 7, d = idx & 127;
    const int64_t unit = ((int64_t)s * p.H + kh * G + g) * nchunk + chunk;
    part_acc[unit * DEC_HEAD + d] = (s_acc[0][g][d] + s_acc[1][g][d]) + (s_acc[2][g][d] + s_acc[3][g][d]);
    if (d == 0) {
      float mo = cmax[unit - chunk];
      for (int c = 1; c <= chunk; ++c) mo = fmaxf(mo, cmax[unit - chunk + c]);
      part_ml[unit * 2] = mo;
      part_ml[unit * 2 + 1] = (s_l[0][g] + s_l[1][g]) + (s_l[2][g] + s_l[3][g]);
    }
  }
}

__global__ __launch_bounds__(128) void decode_attn_combine_kernel(omni_decode_attn_params p, const float* __restrict__ part_acc,
                                                                  const float* __restrict__ part_ml) {
  const int h = blockIdx.x, s = blockIdx.y, d = threadIdx.x;
  if (p.done && p.done[s]) return;
  const int n_keys = min(p.lens[s] + p.len_add, p.capacity);
  if (n_keys < 1) return;
  const int nchunk = (p.capacity + DEC_CHUNK - 1) / DEC_CHUNK, used = (n_keys + DEC_CHUNK - 1) / DEC_CHUNK;
  const int64_t unit0 = ((int64_t)s * p.H + h) * nchunk;
  const float mo = part_ml[(unit0 + used - 1) * 2];                // a prefix maximum: the last chunk's is the whole row's
  float a = 0.f, lv = 0.f;
  for (int c = 0; c < used; ++c) {
    const float sc = __builtin_amdgcn_exp2f(part_ml[(unit0 + c) * 2] - mo);
    lv = __builtin_fmaf(part_ml[(unit0 + c) * 2 + 1], sc, lv);
    a = __builtin_fmaf(part_acc[(unit0 + c) * DEC_HEAD + d], sc, a);
  }
  p.out[s * p.ldo + (int64_t)h * DEC_HEAD + d] = f32_to_bf16_bits(a * (1.0f / lv));
}

size_t decode_attention_workspace_bytes(int32_t n_seq, int32_t H, int32_t capacity) {
  if (n_seq < 1 || H < 1 || capacity < 1) return 0;
  return attn_carve(nullptr, n_seq, H, capacity).total;
}

int decode_attention(const omni_decode_attn_params* p, omni_stream stream) {
  if (!p || !p->q || !p->k_cache || !p->v_cache || !p->out || !p->lens || !p->workspace) return OMNI_ERR_BAD_ARG;
  if (p->n_seq < 1 || p->H < 1 || p->H_kv < 1 || p->capacity < 1) return OMNI_ERR_BAD_ARG;
  if (p->ldq < (int64_t)p->H * DEC_HEAD || p->ldo < (int64_t)p->H * DEC_HEAD) return OMNI_ERR_BAD_ARG;
  if (p->head_dim != DEC_HEAD || p->n_seq > DEC_MAX_SEQ || p->H % p->H_kv != 0 || p->H / p->H_kv > 8) return OMNI_ERR_UNSUPPORTED;
  if ((int64_t)dec_chunks(p->capacity) > 65535) return OMNI_ERR_UNSUPPORTED;
  const AttnWs ws = attn_carve(p->workspace, p->n_seq, p->H, p->capacity);
  if (ws.total > p->workspace_bytes) return OMNI_ERR_BAD_ARG;
  if (!omni_aligned16(p->q) || !omni_aligned16(p->out) || !omni_aligned16(p->k_cache) || !omni_aligned16(p->v_cache) ||
      !omni_aligned16(p->workspace) || p->ldq % 8 != 0 || p->ldo % 8 != 0)
    return OMNI_ERR_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)dec_chunks(p->capacity), (unsigned)p->H_kv, (unsigned)p->n_seq), block(256);
#define DEC_ATTN_LAUNCH(G)                                                                                          \
  hipLaunchKernelGGL(decode_attn_score_kernel<G>, grid, block, 0, s, *p, ws.score, ws.cmax);                       \
  hipLaunchKernelGGL(decode_attn_pv_kernel<G>, grid, block, 0, s, *p, ws.score, ws.cmax, ws.acc, ws.ml)
  switch (p->H / p->H_kv) {
    case 1: DEC_ATTN_LAUNCH(1); break;
    case 2: DEC_ATTN_LAUNCH(2); break;
    case 3: DEC_ATTN_LAUNCH(3); break;
    case 4: DEC_ATTN_LAUNCH(4); break;
    case 5: DEC_ATTN_LAUNCH(5); break;
    case 6: DEC_ATTN_LAUNCH(6); break;
    case 7: DEC_ATTN_LAUNCH(7); break;
    default: DEC_ATTN_LAUNCH(8); break;
  }
#undef DEC_ATTN_LAUNCH
  OMNI_CHECK_LAUNCH();
  hipLaunchKernelGGL(decode_attn_combine_kernel, dim3((unsigned)p->H, (unsigned)p->n_seq), dim3(128), 0, s, *p, ws.acc, ws.ml);
  OMNI_CHECK_LAUNCH();
  return OMNI_OK;
}

// ---- penalty + argmax + EOS + bookkeeping ---------------------------------------------------------------------------------
OMNI_DEVINL bool arg_better(float x, int i, float best, int bi) { return x > best || (x == best && i < bi); }

__global__ __launch_bounds__(1024) void penalized_argmax_kernel(omni_penalized_argmax_params p) {
  __shared__ float s_v[16];
  __shared__ int s_i[16];
  const int s = blockIdx.x, t = threadIdx.x;
  int32_t* done = p.ctrl + OMNI_DECODE_DONE * 8;
  int32_t* n_gen = p.ctrl + OMNI_DECODE_N_GENERATED * 8;
  if (done[s] != 0 || n_gen[s] >= p.max_new) return;             // uniform over the workgroup
  const float* x = p.logits + s * p.ld;
  const uint8_t* seen = p.seen + s * p.seen_stride;
  float best = -__builtin_inff();
  int bi = 0x7fffffff;
  for (int v = t; v < p.vocab; v += 1024) {
    float f = x[v];
    if (seen[v]) f = f < 0.f ? f * p.penalty : f / p.penalty;
    if (arg_better(f, v, best, bi)) {
      best = f;
      bi = v;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (arg_better(ob, oi, best, bi)) {
      best = ob;
      bi = oi;
    }
  }
  if ((t & 63) == 0) {
    s_v[t >> 6] = best;
    s_i[t >> 6] = bi;
  }
  __syncthreads();
  if (t != 0) return;
  for (int w = 1; w < 16; ++w)
    if (arg_better(s_v[w], s_i[w], best, bi)) {
      best = s_v[w];
      bi = s_i[w];
    }
  const int tok = bi == 0x7fffffff ? 0 : bi;                      // (every logit a NaN)
  const int n = n_gen[s];
  p.out_tokens[(int64_t)s * p.max_new + n] = tok;
  n_gen[s] = n + 1;
  p.seen[s * p.seen_stride + tok] = 1;
  p.ctrl[OMNI_DECODE_CUR_ID * 8 + s] = tok;
  int32_t* cur_len = p.ctrl + OMNI_DECODE_CUR_LEN * 8;
  cur_len[s] = p.set_len_cu ? p.set_len_cu[s + 1] - p.set_len_cu[s] : cur_len[s] + 1;
  bool stop = n + 1 >= p.max_new;
  for (int e = 0; e < p.n_eos; ++e) stop = stop || tok == p.eos_ids[e];
  if (stop) done[s] = 1;
}

int penalized_argmax(const omni_penalized_argmax_params* p, omni_stream stream) {
  if (!p || !p->logits || !p->seen || !p->ctrl || !p->out_tokens) return OMNI_ERR_BAD_ARG;
  if (p->vocab < 1 || p->n_seq < 1 || p->max_new < 1 || !(p->penalty > 0.f) || p->n_eos < 0 || p->ld < p->vocab ||
      p->seen_stride < p->vocab)
    return OMNI_ERR_BAD_ARG;
  if (p->n_seq > DEC_MAX_SEQ || p->n_eos > 8) return OMNI_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(penalized_argmax_kernel, dim3((unsigned)p->n_seq), dim3(1024), 0, static_cast<hipStream_t>(stream), *p);
  OMNI_CHECK_LAUNCH();
  return OMNI_OK;
}

// ---- glue kernels ---------------------------------------------------------------------------------------------------------
// one thread per 16 bytes of a row's K | V block
__global__ __launch_bounds__(256) void kv_write_kernel(const uint16_t* __restrict__ qkv, int64_t ld, int rows, int H, int H_kv,
                                                       uint16_t* __restrict__ kc, uint16_t* __restrict__ vc, int n_seq, int capacity,
                                                       const int32_t* __restrict__ cu, const int32_t* __restrict__ ctrl) {
  const int per_row = 2 * H_kv * 16;
  const int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = unit / per_row;
  if (row >= rows) return;
  const int c = (int)(unit - row * per_row);
  int s, pos;
  if (cu) {
    s = 0;
    while (s + 1 < n_seq && row >= cu[s + 1]) ++s;
    pos = (int)row - cu[s];
    if (pos < 0) return;
  } else {
    s = (int)row;
    if (ctrl[OMNI_DECODE_DONE * 8 + s] != 0) return;
    pos = ctrl[OMNI_DECODE_CUR_LEN * 8 + s];
  }
  if (pos < 0 || pos >= capacity || s >= n_seq) return;
  const int isv = c / (H_kv * 16), head = (c >> 4) % H_kv, j = c & 15;
  const u32x4_t v = *reinterpret_cast<const u32x4_t*>(qkv + row * ld + (int64_t)(H + isv * H_kv + head) * DEC_HEAD + j * 8);
  uint16_t* dst = (isv ? vc : kc) + (((int64_t)s * H_kv + head) * capacity + pos) * DEC_HEAD + j * 8;
  *reinterpret_cast<u32x4_t*>(dst) = v;
}

// the front of a step: a sequence that cannot take another token is set done (a full cache also raises the error word);
// pos = cur_len + rope_delta for the RoPE kernel
__global__ void decode_begin_kernel(int32_t* __restrict__ ctrl, int n_seq, int capacity, int max_new, int32_t* __restrict__ err) {
  const int s = threadIdx.x;
  if (s >= n_seq) return;
  const int len = ctrl[OMNI_DECODE_CUR_LEN * 8 + s];
  if (ctrl[OMNI_DECODE_DONE * 8 + s] == 0) {
    if (len >= capacity) {
      ctrl[OMNI_DECODE_DONE * 8 + s] = 1;
      *err = 4;
    } else if (ctrl[OMNI_DECODE_N_GENERATED * 8 + s] >= max_new) {
      ctrl[OMNI_DECODE_DONE * 8 + s] = 1;
    }
  }
  ctrl[OMNI_DECODE_POS * 8 + s] = len + ctrl[OMNI_DECODE_ROPE_DELTA * 8 + s];
}

// one workgroup per sequence: the prompt's ids into the seen map, rope_delta = max position + 1 - length
__global__ __launch_bounds__(256) void prefill_mark_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ cu,
                                                           const int32_t* __restrict__ pos3, int rows, int vocab,
                                                           uint8_t* __restrict__ seen, int64_t seen_stride, int32_t* __restrict__ ctrl) {
  __shared__ int s_max[4];
  const int s = blockIdx.x, r0 = cu[s], r1 = min(cu[s + 1], rows);
  int mx = 0;
  for (int r = r0 + (int)threadIdx.x; r < r1; r += 256) {
    const int id = ids[r];
    if (id >= 0 && id < vocab) seen[s * seen_stride + id] = 1;
    mx = max(mx, max(pos3[r], max(pos3[rows + r], pos3[2 * rows + r])));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) ctrl[OMNI_DECODE_ROPE_DELTA * 8 + s] = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])) + 1 - (r1 - r0);
}

// dst[s, :] = src[cu[s + 1] - 1, :]: each sequence's last row
__global__ __launch_bounds__(256) void gather_last_rows_kernel(const uint16_t* __restrict__ src, int64_t lds, int D, int rows,
                                                               const int32_t* __restrict__ cu, uint16_t* __restrict__ dst) {
  const int s = blockIdx.y, e = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 8;
  if (e >= D) return;
  const int r = cu[s + 1] - 1;
  if (r < 0 || r >= rows) return;
  *reinterpret_cast<u32x4_t*>(dst + (int64_t)s * D + e) = *reinterpret_cast<const u32x4_t*>(src + r * lds + e);
}

// ---- state and drivers ----------------------------------------------------------------------------------------------------
struct DecState {
  omni_text_decode_layout lay;
  int32_t* ctrl;
  int32_t* out_tokens;
  uint8_t* seen;
  omni_bf16 *kc, *vc;
  float* logits;
  omni_bf16 *h, *xn, *qkv, *attn, *gu, *act;
  void* attn_ws;
  size_t attn_ws_bytes;
};

DecState dec_carve(void* base, const omni_text_weights* w, int64_t n_seq, int64_t capacity, int64_t max_new) {
  const int64_t D = w->hidden_size, I = w->intermediate_size, H = w->num_heads, Hkv = w->num_kv_heads;
  const int64_t Nq = H * DEC_HEAD, Nqkv = (H + 2 * Hkv) * DEC_HEAD;
  DecState st = {};
  char* b = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t at = off;
    off += dec_align(bytes);
    return at;
  };
  st.lay.ctrl = take(OMNI_DECODE_CTRL_WORDS * 8 * sizeof(int32_t));
  st.lay.out_tokens = take((size_t)n_seq * max_new * sizeof(int32_t));
  st.lay.seen_stride = (size_t)((w->vocab_size + 15) & ~15);
  st.lay.seen = take((size_t)n_seq * st.lay.seen_stride);
  const size_t cache = (size_t)w->num_layers * n_seq * Hkv * capacity * DEC_HEAD * sizeof(omni_bf16);
  st.lay.k_cache = take(cache);
  st.lay.v_cache = take(cache);
  st.lay.logits = take((size_t)n_seq * w->vocab_size * sizeof(float));
  st.lay.qkv = take((size_t)n_seq * Nqkv * sizeof(omni_bf16));
  const size_t h = take((size_t)n_seq * D * 2), xn = take((size_t)n_seq * D * 2), attn = take((size_t)n_seq * Nq * 2);
  const size_t gu = take((size_t)n_seq * 2 * I * 2), act = take((size_t)n_seq * I * 2);
  st.attn_ws_bytes = attn_carve(nullptr, n_seq, H, capacity).total;
  const size_t aws = take(st.attn_ws_bytes);
  st.lay.total = off;
  st.ctrl = reinterpret_cast<int32_t*>(b + st.lay.ctrl);
  st.out_tokens = reinterpret_cast<int32_t*>(b + st.lay.out_tokens);
  st.seen = reinterpret_cast<uint8_t*>(b + st.lay.seen);
  st.kc = reinterpret_cast<omni_bf16*>(b + st.lay.k_cache);
  st.vc = reinterpret_cast<omni_bf16*>(b + st.lay.v_cache);
  st.logits = reinterpret_cast<float*>(b + st.lay.logits);
  st.qkv = reinterpret_cast<omni_bf16*>(b + st.lay.qkv);
  st.h = reinterpret_cast<omni_bf16*>(b + h);
  st.xn = reinterpret_cast<omni_bf16*>(b + xn);
  st.attn = reinterpret_cast<omni_bf16*>(b + attn);
  st.gu = reinterpret_cast<omni_bf16*>(b + gu);
  st.act = reinterpret_cast<omni_bf16*>(b + act);
  st.attn_ws = b + aws;
  return st;
}

int dec_check_geometry(const omni_text_weights* w, int32_t n_seq, int32_t capacity, int32_t max_new) {
  OMNI_TRY_STATUS(omni_internal_text_check_weights(w));
  if (n_seq < 1 || capacity < 1 || max_new < 1) return OMNI_ERR_BAD_ARG;
  if (n_seq > DEC_MAX_SEQ || w->num_heads / w->num_kv_heads > 8) return OMNI_ERR_UNSUPPORTED;
  if ((int64_t)dec_chunks(capacity) > 65535) return OMNI_ERR_UNSUPPORTED;
  return OMNI_OK;
}

size_t decode_state_bytes(const omni_text_weights* w, int32_t n_seq, int32_t capacity, int32_t max_new,
                          omni_text_decode_layout* layout) {
  if (dec_check_geometry(w, n_seq, capacity, max_new) != OMNI_OK) return 0;
  const DecState st = dec_carve(nullptr, w, n_seq, capacity, max_new);
  if (layout) *layout = st.lay;
  return st.lay.total;
}

// everything both calls refuse before they touch the device
int dec_check_state(const omni_text_weights* w, const omni_text_decode_state* st) {
  if (!st) return OMNI_ERR_BAD_ARG;
  // head_dim / n_seq / n_eos first: what the geometry cannot take is UNSUPPORTED whatever else is missing
  if (w && w->head_dim != DEC_HEAD && w->head_dim > 0) return OMNI_ERR_UNSUPPORTED;
  if (st->n_seq > DEC_MAX_SEQ || st->n_eos > 8) return OMNI_ERR_UNSUPPORTED;
  OMNI_TRY_STATUS(dec_check_geometry(w, st->n_seq, st->capacity, st->max_new));
  if (!st->lm_head || !st->state || !st->workspace || st->n_eos < 0 || !(st->repetition_penalty > 0.f)) return OMNI_ERR_BAD_ARG;
  if (st->workspace_bytes < 256 || dec_carve(nullptr, w, st->n_seq, st->capacity, st->max_new).lay.total > st->state_bytes)
    return OMNI_ERR_BAD_ARG;
  for (int l = 0; l < w->num_layers; ++l) {
    const omni_text_layer_weights& L = w->layers[l];
    if (!L.input_norm_w || !L.qkv_w || !L.qkv_b || !L.o_w || !L.post_norm_w || !L.gate_up_w || !L.down_w) return OMNI_ERR_BAD_ARG;
  }
  if (!omni_aligned16(st->state) || !omni_aligned16(st->workspace) || !omni_aligned16(st->lm_head) ||
      (st->logits_out && !omni_aligned16(st->logits_out)))
    return OMNI_ERR_ALIGN;
  return OMNI_OK;
}

int dec_gemv(const omni_bf16* A, int64_t lda, int32_t M, const omni_bf16* W, int32_t N, int32_t K, int32_t blocked,
             const omni_bf16* bias, omni_bf16* res, omni_bf16* out, float* out_f32, omni_stream stream) {
  omni_gemv_params p = {};
  p.A = A; p.lda = lda; p.M = M; p.N = N; p.K = K; p.w_k32_blocked = blocked; p.W = W; p.bias = bias;
  p.res = res; p.ldres = N; p.out = out; p.out_f32 = out_f32; p.ldo = N;
  return gemv_bf16(&p, stream);
}

// final norm rows in xn -> lm_head -> penalty, argmax, bookkeeping
int dec_head(const omni_text_weights* w, const omni_text_decode_state* st, const DecState& d, const int32_t* set_len_cu,
             omni_stream stream) {
  float* logits = st->logits_out ? st->logits_out : d.logits;
  OMNI_TRY_STATUS(dec_gemv(d.xn, w->hidden_size, st->n_seq, st->lm_head, w->vocab_size, w->hidden_size, 0, nullptr, nullptr, nullptr,
                           logits, stream));
  omni_penalized_argmax_params a = {};
  a.logits = logits; a.ld = w->vocab_size; a.seen = d.seen; a.seen_stride = (int64_t)d.lay.seen_stride; a.ctrl = d.ctrl;
  a.out_tokens = d.out_tokens; a.set_len_cu = set_len_cu; a.vocab = w->vocab_size; a.n_seq = st->n_seq; a.max_new = st->max_new;
  a.n_eos = st->n_eos; a.penalty = st->repetition_penalty;
  for (int e = 0; e < st->n_eos; ++e) a.eos_ids[e] = st->eos_ids[e];
  return penalized_argmax(&a, stream);
}

int text_prefill(const omni_text_weights* w, const omni_text_batch_mm* b, const omni_text_decode_state* st, omni_stream stream) {
  if (!b) return OMNI_ERR_BAD_ARG;
  OMNI_TRY_STATUS(dec_check_state(w, st));
  if (b->n_prompts != st->n_seq || b->max_seqlen > st->capacity) return OMNI_ERR_BAD_ARG;
  if (!b->row_pos3 || !b->input_ids || !b->cu_seqlens || !b->out) return OMNI_ERR_BAD_ARG;
  const DecState d = dec_carve(st->state, w, st->n_seq, st->capacity, st->max_new);
  const omni_text_kv_sink sink = {d.kc, d.vc, st->n_seq, st->capacity};
  hipStream_t s = static_cast<hipStream_t>(stream);
  OMNI_TRY_STATUS(omni_internal_text_forward_mm(w, b, &sink, stream));
  if (hipMemsetAsync(d.ctrl, 0, OMNI_DECODE_CTRL_WORDS * 8 * sizeof(int32_t), s) != hipSuccess ||
      hipMemsetAsync(d.seen, 0, (size_t)st->n_seq * d.lay.seen_stride, s) != hipSuccess)
    return OMNI_ERR_LAUNCH;
  hipLaunchKernelGGL(prefill_mark_kernel, dim3((unsigned)st->n_seq), dim3(256), 0, s, b->input_ids, b->cu_seqlens, b->row_pos3,
                     b->total_rows, w->vocab_size, d.seen, (int64_t)d.lay.seen_stride, d.ctrl);
  OMNI_CHECK_LAUNCH();
  const int D = w->hidden_size;
  hipLaunchKernelGGL(gather_last_rows_kernel, dim3((unsigned)((D / 8 + 255) / 256), (unsigned)st->n_seq), dim3(256), 0, s, b->out,
                     (int64_t)D, D, b->total_rows, b->cu_seqlens, d.xn);
  OMNI_CHECK_LAUNCH();
  return dec_head(w, st, d, b->cu_seqlens, stream);
}

int text_decode_step(const omni_text_weights* w, const omni_text_decode_state* st, omni_stream stream) {
  OMNI_TRY_STATUS(dec_check_state(w, st));
  const DecState d = dec_carve(st->state, w, st->n_seq, st->capacity, st->max_new);
  const int32_t M = st->n_seq, D = w->hidden_size, I = w->intermediate_size, H = w->num_heads, Hkv = w->num_kv_heads;
  const int32_t Nq = H * DEC_HEAD, Nqkv = (H + 2 * Hkv) * DEC_HEAD, blocked = w->gemm_w_k32_blocked;
  int32_t* err = static_cast<int32_t*>(st->workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const omni_text_kv_sink sink = {d.kc, d.vc, st->n_seq, st->capacity};
  hipLaunchKernelGGL(decode_begin_kernel, dim3(1), dim3(64), 0, s, d.ctrl, M, st->capacity, st->max_new, err);
  OMNI_CHECK_LAUNCH();
  OMNI_TRY_STATUS(omni_text_embed_gather(w->embed_tokens, w->vocab_size, D, d.ctrl + OMNI_DECODE_CUR_ID * 8, M, d.h, D, err, stream));
  omni_decode_attn_params ap = {};
  ap.q = d.qkv; ap.ldq = Nqkv; ap.out = d.attn; ap.ldo = Nq; ap.lens = d.ctrl + OMNI_DECODE_CUR_LEN * 8;
  ap.done = d.ctrl + OMNI_DECODE_DONE * 8; ap.len_add = 1; ap.n_seq = M; ap.H = H; ap.H_kv = Hkv; ap.head_dim = DEC_HEAD;
  ap.capacity = st->capacity; ap.softmax_scale = 1.0f / sqrtf((float)DEC_HEAD);
  ap.workspace = d.attn_ws; ap.workspace_bytes = d.attn_ws_bytes;
  const int64_t layer_elems = (int64_t)M * Hkv * st->capacity * DEC_HEAD;
  for (int l = 0; l < w->num_layers; ++l) {
    const omni_text_layer_weights& L = w->layers[l];
    OMNI_TRY_STATUS(omni_rmsnorm(d.h, D, d.xn, D, M, D, L.input_norm_w, w->rms_norm_eps, stream));
    OMNI_TRY_STATUS(dec_gemv(d.xn, D, M, L.qkv_w, Nqkv, D, blocked, L.qkv_b, nullptr, d.qkv, nullptr, stream));
    // the three M-RoPE rows of a generated token are equal: rotate-half RoPE at the one position IS its M-RoPE
    OMNI_TRY_STATUS(omni_text_rope_neox(d.qkv, Nqkv, M, H, Hkv, w->rope_cos, w->rope_sin, w->rope_npos,
                                        d.ctrl + OMNI_DECODE_POS * 8, err, stream));
    OMNI_TRY_STATUS(omni_internal_text_kv_write(d.qkv, Nqkv, M, H, Hkv, &sink, l, nullptr, d.ctrl, stream));
    ap.k_cache = d.kc + l * layer_elems;
    ap.v_cache = d.vc + l * layer_elems;
    OMNI_TRY_STATUS(decode_attention(&ap, stream));
    OMNI_TRY_STATUS(dec_gemv(d.attn, Nq, M, L.o_w, D, Nq, blocked, nullptr, d.h, d.h, nullptr, stream));
    OMNI_TRY_STATUS(omni_rmsnorm(d.h, D, d.xn, D, M, D, L.post_norm_w, w->rms_norm_eps, stream));
    OMNI_TRY_STATUS(dec_gemv(d.xn, D, M, L.gate_up_w, 2 * I, D, blocked, nullptr, nullptr, d.gu, nullptr, stream));
    OMNI_TRY_STATUS(omni_text_swiglu(d.gu, 2 * (int64_t)I, d.act, I, M, I, 0, stream));
    OMNI_TRY_STATUS(dec_gemv(d.act, I, M, L.down_w, D, I, blocked, nullptr, d.h, d.h, nullptr, stream));
  }
  OMNI_TRY_STATUS(omni_rmsnorm(d.h, D, d.xn, D, M, D, w->final_norm_w, w->rms_norm_eps, stream));
  return dec_head(w, st, d, nullptr, stream);
}

}  // namespace

int omni_internal_text_kv_write(const omni_bf16* qkv, int64_t ld, int32_t rows, int32_t H, int32_t H_kv,
                                const omni_text_kv_sink* sink, int32_t layer, const int32_t* cu_seqlens, const int32_t* ctrl,
                                void* stream) {
  if (!qkv || !sink || !sink->k_cache || !sink->v_cache || rows < 1 || (!cu_seqlens && !ctrl)) return OMNI_ERR_BAD_ARG;
  if (!cu_seqlens && rows > sink->n_seq) return OMNI_ERR_BAD_ARG;
  const int64_t layer_elems = (int64_t)sink->n_seq * H_kv * sink->capacity * DEC_HEAD;
  const int64_t units = (int64_t)rows * 2 * H_kv * 16;
  if ((units + 255) / 256 > 0x7fffffffLL) return OMNI_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(kv_write_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), qkv, ld,
                     rows, H, H_kv, sink->k_cache + layer * layer_elems, sink->v_cache + layer * layer_elems, sink->n_seq,
                     sink->capacity, cu_seqlens, ctrl);
  OMNI_CHECK_LAUNCH();
  return OMNI_OK;
}

#if !defined(__HIP_DEVICE_COMPILE__)
extern "C" int (*const omni_gemv_bf16)(const omni_gemv_params*, omni_stream) = gemv_bf16;
extern "C" int (*const omni_decode_attention)(const omni_decode_attn_params*, omni_stream) = decode_attention;
extern "C" size_t (*const omni_decode_attention_workspace_bytes)(int32_t, int32_t, int32_t) = decode_attention_workspace_bytes;
extern "C" int (*const omni_text_penalized_argmax)(const omni_penalized_argmax_params*, omni_stream) = penalized_argmax;
extern "C" size_t (*const omni_qwen2_text_decode_state_bytes)(const omni_text_weights*, int32_t, int32_t, int32_t,
                                                              omni_text_decode_layout*) = decode_state_bytes;
extern "C" int (*const omni_qwen2_text_prefill)(const omni_text_weights*, const omni_text_batch_mm*, const omni_text_decode_state*,
                                                omni_stream) = text_prefill;
extern "C" int (*const omni_qwen2_text_decode_step)(const omni_text_weights*, const omni_text_decode_state*, omni_stream) =
    text_decode_step;
#endif
