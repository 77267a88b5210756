// SAGE_ATTN for gfx950: int8 Q K^T flash attention (SageAttention v1 — "qk_int8, pv 16-bit, fp32 accumulation"), the
// arithmetic behind the reference's third attention backend (vllm_omni/diffusion/attention/backends/sage_attn.py).
// Per item (cu_seqlens segment) and per head:
//   1. km = mean_j k[j] (fp32, a deterministic per-(item, head) reduction: fixed row partition, fixed combine order);
//      k' = k - km — adds q . km to every logit of a row, so the softmax is unchanged
//   2. q *= softmax_scale * log2(e) (unless the caller prescaled q); per block of 64 query rows from the item's first row:
//      sq = amax|q| / 127, q8 = rne(q / sq) clamped to +-127
//   3. the same on k' per block of 64 key rows: sk, k8; an all-zero block gets scale 1 and zeros
//   4. s = float(q8 . k8^T) * sq * sk is in the log2 domain; online softmax with exp2 in fp32; P rounded to bf16; bf16 P V MFMA
//      with an fp32 accumulator; bf16 output (row-major, or K32-blocked for the out-projection GEMM)
// Host model of the same steps: tests/_sage_model.py.
//
// Launches: sage_kmean_kernel (K mean), sage_quant_kernel twice (Q, K' -> int8 + block scales, into a caller-owned workspace),
// sage_attn_fwd_kernel.  The attention kernel has attention_general.hip's structure (one workgroup = 4 waves x 32 queries of one
// (item, head); 64-key tiles (= one K scale block) staged global -> registers -> LDS with the next tile's loads in flight; hipcc
// schedules the loop) and shares everything from the row max on with it (attention_common.h: online softmax, bf16 P V MFMA with
// V^T by transposed reads, epilogue).  Its own is the front end: S^T = K Q^T with swapped operands on v_mfma_i32_32x32x32_i8
// (A = K fragment from the int8 K image — the shared K image at a row pitch of DH bytes —, B = the lane's int8 Q fragment, 16
// bytes per k-step, kept in registers: half the registers of the bf16 Q); the int32 scores are converted and scaled by sq (per
// lane: one query) * sk (per tile).  The MFMA k order inside a fragment does not matter for Q K^T: both operands are loaded with
// the same channel map and the product sums over all of it.
// Every launch honours an optional per-item skip predicate (TeaCache, omni_dit_forward): a skipped item costs nothing and its
// output rows are left untouched.
#include "attention_common.h"

namespace {

constexpr int SQ_WAVES = 4;
constexpr int SQBLK = 32 * SQ_WAVES;   // queries per workgroup (two 64-row scale blocks)
constexpr int SKV = ATTN_KV;           // keys per tile = rows per scale block
constexpr int SBLK = 64;

typedef __attribute__((ext_vector_type(4))) int i32x4_t;
typedef __attribute__((ext_vector_type(16))) int i32x16_t;

// Workspace carve: every piece 256-byte aligned.  int8 rows are indexed (item, row within the item), so the layout depends on the
// host-known bounds only (B, max_seqlen), never on the device cu_seqlens.
struct SageWs {
  int8_t *q8, *k8;
  float *sq, *sk, *km;
  size_t total;
};
inline size_t s_align(size_t x) { return (x + 255) & ~size_t(255); }
__host__ __device__ inline int s_blocks(int32_t len) { return (len + SBLK - 1) / SBLK; }
SageWs sage_carve(char* base, const omni_attn_params* p) {
  const int64_t dh = p->head_dim;
  SageWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* r = base ? base + off : nullptr; off += s_align(bytes); return r; };
  w.q8 = reinterpret_cast<int8_t*>(take((size_t)p->B * p->max_seqlen_q * p->H * dh));
  w.k8 = reinterpret_cast<int8_t*>(take((size_t)p->B * p->max_seqlen_k * p->H_kv * dh));
  w.sq = reinterpret_cast<float*>(take((size_t)p->B * s_blocks(p->max_seqlen_q) * p->H * 4));
  w.sk = reinterpret_cast<float*>(take((size_t)p->B * s_blocks(p->max_seqlen_k) * p->H_kv * 4));
  w.km = reinterpret_cast<float*>(take((size_t)p->B * p->H_kv * dh * 4));
  w.total = off;
  return w;
}

// km[b][h][c] = mean over the item's key rows of k[., h, c], fp32.  Thread (row group rg, 8-channel chunk ch) sums rows
// rg, rg + RPI, ... in order; the RPI partial sums are added in row-group order: the same bits on every launch.
template <int DH>
__global__ __launch_bounds__(256) void sage_kmean_kernel(const uint16_t* __restrict__ k, int64_t ldk, const int32_t* __restrict__ cu,
                                                         int Hkv, const int32_t* __restrict__ item_skip, float* __restrict__ km) {
  constexpr int NCH = DH / 8, RPI = 256 / NCH;
  __shared__ float part[RPI][DH];
  const int b = blockIdx.x / Hkv, h = blockIdx.x - b * Hkv;
  if (item_skip && item_skip[b]) return;
  const int start = cu[b], len = cu[b + 1] - start;
  const int ch = threadIdx.x % NCH, rg = threadIdx.x / NCH;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const uint16_t* kp = k + (int64_t)start * ldk + h * DH + ch * 8;
  for (int r = rg; r < len; r += RPI) {
    const u32x4_t w = *reinterpret_cast<const u32x4_t*>(kp + (int64_t)r * ldk);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[2 * e] += bf16_lo(w[e]);
      acc[2 * e + 1] += bf16_hi(w[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[rg][ch * 8 + e] = acc[e];
  __syncthreads();
  if (threadIdx.x < DH) {
    float s = 0.f;
#pragma unroll 4
    for (int g = 0; g < RPI; ++g) s += part[g][threadIdx.x];
    km[((int64_t)b * Hkv + h) * DH + threadIdx.x] = len > 0 ? s / (float)len : 0.f;
  }
}

// One (item, 64-row block, head): x = float(src) * mul (Q) or float(src) - km (K); scale = amax|x| / 127 (1 for an all-zero
// block); dst = rne(x / scale) clamped to +-127, int8 rows [(item, row)][nh * DH]; scale at [(item, block)][head].
template <int DH>
__global__ __launch_bounds__(256) void sage_quant_kernel(const uint16_t* __restrict__ src, int64_t ld, const int32_t* __restrict__ cu,
                                                         int nh, int maxlen, int maxblk, float mul, const float* __restrict__ km,
                                                         const int32_t* __restrict__ item_skip, int8_t* __restrict__ dst,
                                                         float* __restrict__ scale) {
  constexpr int NCH = DH / 8;                  // 8-channel pieces per row
  constexpr int NP = SBLK * NCH / 256;         // pieces per thread (4 at dh 128, 2 at dh 64)
  __shared__ float wmax[4];
  const int h = blockIdx.x % nh;
  const int bb = blockIdx.x / nh;
  const int b = bb / maxblk, blk = bb - b * maxblk;
  if (item_skip && item_skip[b]) return;
  const int start = cu[b], len = min(cu[b + 1] - start, maxlen);   // rows past the bound the workspace was sized for: not written
  const int r0 = blk * SBLK;
  if (r0 >= len) return;
  float x[NP][8];
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int c = threadIdx.x + i * 256;
    const int r = r0 + c / NCH, ch = c % NCH;
    if (r < len) {
      const u32x4_t w = *reinterpret_cast<const u32x4_t*>(src + (int64_t)(start + r) * ld + h * DH + ch * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        x[i][2 * e] = bf16_lo(w[e]);
        x[i][2 * e + 1] = bf16_hi(w[e]);
      }
      if (km) {
        const float* m = km + ((int64_t)b * nh + h) * DH + ch * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) x[i][e] -= m[e];
      } else if (mul != 1.0f) {
#pragma unroll
        for (int e = 0; e < 8; ++e) x[i][e] *= mul;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) x[i][e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(x[i][e]));
  }
  amax = wave_max<64>(amax);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  const float sc = amax > 0.f ? amax / 127.0f : 1.0f;
  if (threadIdx.x == 0) scale[((int64_t)b * maxblk + blk) * nh + h] = sc;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int c = threadIdx.x + i * 256;
    const int r = r0 + c / NCH, ch = c % NCH;
    if (r >= len) continue;
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float qv = fminf(fmaxf(rintf(x[i][e] / sc), -127.f), 127.f);
      w[e >> 2] |= ((uint32_t)(int32_t)qv & 0xffu) << (8 * (e & 3));
    }
    *reinterpret_cast<u32x2_t*>(dst + ((int64_t)b * maxlen + r) * nh * DH + h * DH + ch * 8) = u32x2_t{w[0], w[1]};
  }
}

template <int DH>
__global__ __launch_bounds__(SQ_WAVES * 64, 2) void sage_attn_fwd_kernel(const omni_attn_params P, SageWs W, int qblocks,
                                                                      const int32_t* __restrict__ item_skip) {
  constexpr int KROW = DH;                 // bytes per int8 K row in LDS
  constexpr int NKS = DH / 32;             // i8 MFMA k-steps of the QK^T product
  constexpr int NDB = DH / 32;             // 32-row blocks of O^T
  constexpr int K_BYTES = SKV * KROW;
  constexpr int V_BYTES = SKV * DH * 2;
  constexpr int NLK = K_BYTES / 16 / (SQ_WAVES * 64);   // 16-byte K pieces per thread per tile (2 at dh 128, 1 at dh 64)
  constexpr int NLV = V_BYTES / 16 / (SQ_WAVES * 64);   // 16-byte V pieces per thread per tile (4 / 2)
  typedef attn_elem<false> E;              // P, V and the output are bf16
  __shared__ __attribute__((aligned(16))) char smem[K_BYTES + V_BYTES];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;

  const int hb = blockIdx.x / qblocks, qb = blockIdx.x - hb * qblocks;
  const int b = hb / P.H, h = hb - b * P.H;
  if (item_skip && item_skip[b]) return;
  const int hk = h / (P.H / P.H_kv);
  const int q_start = P.cu_seqlens_q[b], q_len = min(P.cu_seqlens_q[b + 1] - q_start, P.max_seqlen_q);
  const int k_len = min(P.cu_seqlens_k[b + 1] - P.cu_seqlens_k[b], P.max_seqlen_k);
  const int q0 = qb * SQBLK;
  if (q0 >= q_len) return;
  const int qi = q0 + wave * 32 + l31;                       // this lane's query (within the item); rows past q_len are clamped
  const int qrow = min(qi, q_len - 1);
  const int kblk = s_blocks(P.max_seqlen_k);

  // int8 Q fragment of k-step ks: channels 32 ks + 16 hi .. + 16 (any map works as long as K uses the same one)
  i32x4_t qf[NKS];
  {
    const int8_t* qp = W.q8 + ((int64_t)b * P.max_seqlen_q + qrow) * P.H * DH + h * DH + hi * 16;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const i32x4_t*>(qp + ks * 32);
  }
  const float sq = W.sq[((int64_t)b * s_blocks(P.max_seqlen_q) + qrow / SBLK) * P.H + h];
  const float* skp = W.sk + (int64_t)b * kblk * P.H_kv + hk;
  f32x16_t o[NDB];
#pragma unroll
  for (int d = 0; d < NDB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[d][i] = 0.0f;
  float m_run = -INFINITY, l_run = 0.0f;
  const int ntiles = (k_len + SKV - 1) / SKV;

  const int8_t* kbase = W.k8 + (int64_t)b * P.max_seqlen_k * P.H_kv * DH + hk * DH;
  const uint16_t* vbase = P.v + (int64_t)P.cu_seqlens_k[b] * P.ldv + hk * DH;
  const int64_t ld8k = (int64_t)P.H_kv * DH;
  u32x4_t kreg[NLK], vreg[NLV];
  auto load_tile = [&](int t) {
    attn_load_tile<KROW, SQ_WAVES * 64>(kreg, kbase, ld8k, t, k_len, tid);
    attn_load_tile<2 * DH, SQ_WAVES * 64>(vreg, vbase, P.ldv, t, k_len, tid);
  };
  auto store_tile = [&]() {
    attn_store_tile<KROW, SQ_WAVES * 64, false>(smem, kreg, tid);
    attn_store_tile<2 * DH, SQ_WAVES * 64, true>(smem + K_BYTES, vreg, tid);
  };
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  uint32_t k_addr[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) k_addr[ks] = attn_k_frag_addr<KROW>(lds0, lane, ks);
  const uint32_t v_addr = attn_vt_lane_addr(lds0 + K_BYTES, lane);

  if (ntiles > 0) {
    load_tile(0);
    store_tile();
  }
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) load_tile(t + 1);                    // in flight while tile t is consumed
    // ---- S^T = K8 Q8^T: two 32-key sub-blocks, int32 accumulators
    typedef __attribute__((address_space(3))) const i32x4_t lds_i32x4;
    i32x16_t si[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int i = 0; i < 16; ++i) si[j][i] = 0;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const i32x4_t kf = *reinterpret_cast<lds_i32x4*>((uintptr_t)(k_addr[ks] + j * 32 * KROW));
        si[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(kf, qf[ks], si[j], 0, 0, 0);
      }
    }
    // ---- dequantise (sq of this lane's query x sk of this tile); the ragged last tile masks its keys past k_len
    const float scl = sq * skp[(int64_t)t * P.H_kv];
    const int kv0 = t * SKV;
    f32x16_t s[2];
    float mx = -INFINITY;
    if (kv0 + SKV <= k_len) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s[j][r] = (float)si[j][r] * scl;
          mx = fmaxf(mx, s[j][r]);
        }
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s[j][r] = attn_key_of(kv0, j, r, hi) < k_len ? (float)si[j][r] * scl : -INFINITY;
          mx = fmaxf(mx, s[j][r]);
        }
    }
    attn_softmax_pv_tile<E>(s, mx, v_addr, m_run, l_run, o);
    __syncthreads();                                         // every wave is done with tile t
    if (t + 1 < ntiles) {
      store_tile();
      __syncthreads();
    }
  }

  attn_store_out<E>(o, l_run, P.out, P.ldo, P.out_k32_rows, q_start + qi, h, hi, qi < q_len);
}

template <int DH>
int launch_sage(const omni_attn_params* p, const SageWs& w, const int32_t* item_skip, int q_prescaled, hipStream_t s) {
  const int qb = s_blocks(p->max_seqlen_q), kb = s_blocks(p->max_seqlen_k);
  const long g_mean = (long)p->B * p->H_kv, g_q = (long)p->B * qb * p->H, g_k = (long)p->B * kb * p->H_kv;
  const int qblocks = (p->max_seqlen_q + SQBLK - 1) / SQBLK;
  const long g_attn = (long)p->B * p->H * qblocks;
  if (g_q > 0x7fffffffL || g_k > 0x7fffffffL || g_attn > 0x7fffffffL) return OMNI_ERR_UNSUPPORTED;
  const float mul = q_prescaled ? 1.0f : p->softmax_scale * OMNI_LOG2E;
  hipLaunchKernelGGL((sage_kmean_kernel<DH>), dim3((unsigned)g_mean), dim3(256), 0, s, p->k, p->ldk, p->cu_seqlens_k, p->H_kv,
                     item_skip, w.km);
  OMNI_CHECK_LAUNCH();
  hipLaunchKernelGGL((sage_quant_kernel<DH>), dim3((unsigned)g_q), dim3(256), 0, s, p->q, p->ldq, p->cu_seqlens_q, p->H,
                     p->max_seqlen_q, qb, mul, (const float*)nullptr, item_skip, w.q8, w.sq);
  OMNI_CHECK_LAUNCH();
  hipLaunchKernelGGL((sage_quant_kernel<DH>), dim3((unsigned)g_k), dim3(256), 0, s, p->k, p->ldk, p->cu_seqlens_k, p->H_kv,
                     p->max_seqlen_k, kb, 1.0f, (const float*)w.km, item_skip, w.k8, w.sk);
  OMNI_CHECK_LAUNCH();
  if (p->max_seqlen_k > 0)
    hipLaunchKernelGGL((sage_attn_fwd_kernel<DH>), dim3((unsigned)g_attn), dim3(SQ_WAVES * 64), 0, s, *p, w, qblocks, item_skip);
  OMNI_CHECK_LAUNCH();
  return OMNI_OK;
}

}  // namespace

extern "C" size_t omni_attn_quant_workspace_bytes(const omni_attn_params* p) {
  if (!p || p->B <= 0 || p->H <= 0 || p->H_kv <= 0 || p->max_seqlen_q <= 0 || p->max_seqlen_k < 0) return 0;
  if (p->head_dim != 64 && p->head_dim != 128) return 0;
  return sage_carve(nullptr, p).total;
}

// omni_flash_attn_general with qk_int8 = 1 (validated there) and the DiT forward's joint attention (item_skip, prescaled q)
int omni_internal_sage_attn(const omni_attn_params* p, const int32_t* item_skip, int32_t q_prescaled, void* stream) {
  if (!p->workspace || p->workspace_bytes < omni_attn_quant_workspace_bytes(p)) return OMNI_ERR_BAD_ARG;
  if (!omni_aligned16(p->workspace)) return OMNI_ERR_ALIGN;
  const SageWs w = sage_carve(static_cast<char*>(p->workspace), p);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return p->head_dim == 128 ? launch_sage<128>(p, w, item_skip, q_prescaled, s) : launch_sage<64>(p, w, item_skip, q_prescaled, s);
}
