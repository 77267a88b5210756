// General flash attention forward for gfx950: everything `F.scaled_dot_product_attention` accepts at the reference's
// attention plug-in point (vllm_omni/diffusion/attention/backends/sdpa.py:46-66) that the two tuned kernels of the Qwen-Image
// hot path (attention.hip, attention_w64.hip: self-attention, head size 128, no mask) do not take:
//   * separate query / key sequences (cross-attention: wan2_2_transformer.py:243,340 attends video tokens to text tokens),
//   * head size 64 as well as 128 (sd3_transformer.py:108),
//   * attention masks: boolean (True = attend) or additive (bf16 / fp32), any layout broadcastable to [B, H, S_q, S_k]
//     (element strides, 0 = broadcast) — key-padding masks, block masks, dense biases,
//   * is_causal (top-left aligned like torch: key index <= query index),
//   * grouped K / V heads (num_kv_heads < num_heads),
//   * q / k / v / out in fp16 as well as bf16 (omni_attn_params.elem_type; the reference runs its DiTs in either, data.py:418-436):
//     the kernel is a template on the element type, the bf16 instances are what they were.
// The arithmetic scheme of attention.hip (swapped operands: a lane owns ONE query; K / V images, V^T by transposed reads, the
// half-wave exchange: attention_common.h), with hipcc scheduling the loop (no hand-placed waits: this is the general path, not
// the roofline kernel):
//   one workgroup = 4 waves x 32 queries of one (item, head); K / V tiles of 64 keys staged global -> registers -> LDS, the
//   next tile's global loads in flight while the current tile is consumed.
// This file holds what is the general kernel's own: the 16-bit Q / K front end (v_mfma_f32_32x32x16_bf16 / _f16), the scale in
// fp32 (q is NOT pre-rounded with the scale), masks and `causal`.  From the row max on — online softmax in the exp2 domain, P
// packed to bf16 / fp16, O^T += V^T P^T, the epilogue — it runs the steps it shares with attention_sage.hip (attention_common.h).
// Rows whose every key is masked produce zeros (torch's math path yields NaN there, its fused paths zeros).
// Roofline: MFMA-bound, 4 * S_q * S_k * dh flop per (item, head); measured numbers in DESIGN.md (kernel table).
#include "attention_common.h"

namespace {

constexpr int GQ_WAVES = 4;
constexpr int GQBLK = 32 * GQ_WAVES;   // queries per workgroup
constexpr int GKV = ATTN_KV;           // keys per tile

// F16: q / k / v / out are IEEE fp16 and both products run on v_mfma_f32_32x32x16_f16; P and the output are rounded to fp16
// (nearest even).  P = exp2(s - m) <= 1 goes to the MFMA as it is, also where it is an fp16 SUBNORMAL (below 6.1e-5): measured,
// the fp16 MFMA does not flush subnormal operands (a tail of 4095 keys 10 - 13 nats below the maximum keeps its 5.5 % of the
// mass: DESIGN.md kernel table, tests/test_gpu_attention_fp16.py flat tail), so no exponent shift of P is needed.
template <int DH, bool F16>
__global__ __launch_bounds__(GQ_WAVES * 64) void flash_attn_general_kernel(const omni_attn_params P, int qblocks) {
  typedef attn_elem<F16> E;
  typedef typename E::frag frag_t;
  constexpr int NCH = DH / 8;              // 16-byte chunks per K / V row
  constexpr int ROWB = DH * 2;             // bytes per K row in LDS
  constexpr int NKS = DH / 16;             // MFMA k-steps of the QK^T product
  constexpr int NDB = DH / 32;             // 32-row blocks of O^T
  constexpr int K_BYTES = GKV * ROWB;
  constexpr int NLD = GKV * NCH / (GQ_WAVES * 64);   // 16-byte pieces per thread per operand per tile (4 at dh 128, 2 at dh 64)
  __shared__ __attribute__((aligned(16))) char smem[2 * K_BYTES];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;

  const int hb = blockIdx.x / qblocks, qb = blockIdx.x - hb * qblocks;
  const int b = hb / P.H, h = hb - b * P.H;
  const int hk = h / (P.H / P.H_kv);
  const int q_start = P.cu_seqlens_q[b], q_len = P.cu_seqlens_q[b + 1] - q_start;
  const int k_start = P.cu_seqlens_k[b], k_len = P.cu_seqlens_k[b + 1] - k_start;
  const int q0 = qb * GQBLK;
  if (q0 >= q_len) return;
  const int qi = q0 + wave * 32 + l31;                       // this lane's query (within the item); rows past q_len are clamped
  const int qrow = min(qi, q_len - 1);

  // Q fragments: B operand of S^T = K Q^T — lane (query l31, half hi) holds k = 16 ks + 8 hi .. + 8
  frag_t qf[NKS];
  {
    const uint16_t* qp = P.q + (int64_t)(q_start + qrow) * P.ldq + h * DH + hi * 8;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const frag_t*>(qp + ks * 16);
  }
  f32x16_t o[NDB];
#pragma unroll
  for (int d = 0; d < NDB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[d][i] = 0.0f;
  float m_run = -INFINITY, l_run = 0.0f;
  const float sl2 = P.softmax_scale * OMNI_LOG2E;

  // keys this workgroup has to visit: all of them, or (causal) those up to its last query
  int k_end = k_len;
  if (P.causal) k_end = min(k_len, q0 + GQBLK);
  const int ntiles = (k_end + GKV - 1) / GKV;

  const uint16_t* kbase = P.k + (int64_t)k_start * P.ldk + hk * DH;
  const uint16_t* vbase = P.v + (int64_t)k_start * P.ldv + hk * DH;
  u32x4_t kreg[NLD], vreg[NLD];
  auto load_tile = [&](int t) {
    attn_load_tile<ROWB, GQ_WAVES * 64>(kreg, kbase, P.ldk, t, k_len, tid);
    attn_load_tile<ROWB, GQ_WAVES * 64>(vreg, vbase, P.ldv, t, k_len, tid);
  };
  auto store_tile = [&]() {
    attn_store_tile<ROWB, GQ_WAVES * 64, false>(smem, kreg, tid);
    attn_store_tile<ROWB, GQ_WAVES * 64, true>(smem + K_BYTES, vreg, tid);
  };
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  uint32_t k_addr[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) k_addr[ks] = attn_k_frag_addr<ROWB>(lds0, lane, ks);
  const uint32_t v_addr = attn_vt_lane_addr(lds0 + K_BYTES, lane);

  const char* mrow = nullptr;              // this lane's mask row (element (b, h, qi, 0))
  const int msz = P.mask_type == 1 ? 1 : (P.mask_type == 2 ? 2 : 4);
  if (P.mask_type) mrow = reinterpret_cast<const char*>(P.mask) +
                          ((int64_t)b * P.mask_stride_b + (int64_t)h * P.mask_stride_h + (int64_t)qrow * P.mask_stride_q) * msz;

  if (ntiles > 0) {
    load_tile(0);
    store_tile();
  }
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) load_tile(t + 1);                    // in flight while tile t is consumed
    // ---- S^T = K Q^T: two 32-key sub-blocks
    typedef __attribute__((address_space(3))) const frag_t lds_frag;
    f32x16_t s[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int i = 0; i < 16; ++i) s[j][i] = 0.0f;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const frag_t kf = *reinterpret_cast<lds_frag*>((uintptr_t)(k_addr[ks] + j * 32 * ROWB));
        s[j] = E::mfma(kf, qf[ks], s[j]);
      }
    }
    // ---- scale and mask (register r of sub-block j <-> key attn_key_of(kv0, j, r, hi))
    const int kv0 = t * GKV;
    // which tiles need per-element work: the ragged last tile; with `causal` only the tiles that reach past this WAVE's smallest
    // query index (everything before the diagonal is attended as it is); with a mask every tile
    const bool tail = kv0 + GKV > k_len;
    const bool diag = P.causal && kv0 + GKV - 1 > q0 + wave * 32;
    float mx = -INFINITY;
    if (!(tail || diag || P.mask_type)) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s[j][r] *= sl2;
          mx = fmaxf(mx, s[j][r]);
        }
    } else {
      // mask values of a lane's four CONSECUTIVE keys (r & 3) come in one load when the mask is contiguous along the keys and
      // the address allows it (the usual cases: a [B, 1, 1, S_k] padding mask, a dense [.., S_q, S_k] bias); else one by one
      const bool vec = P.mask_type && P.mask_stride_k == 1;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const int kb = attn_key_of(kv0, j, 4 * rq, hi);               // first of this lane's four consecutive keys
          float add[4] = {0.f, 0.f, 0.f, 0.f};
          bool ok[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) ok[e] = kb + e < k_len && (!P.causal || kb + e <= qi);
          if (P.mask_type && kb < k_len) {
            const char* mp = mrow + (int64_t)kb * P.mask_stride_k * msz;
            const bool whole = vec && kb + 3 < k_len && (reinterpret_cast<uintptr_t>(mp) & (4 * msz - 1)) == 0;
            if (P.mask_type == 1) {
              uint32_t w = 0;
              if (whole) w = *reinterpret_cast<const uint32_t*>(mp);
              else
                for (int e = 0; e < 4; ++e)
                  if (kb + e < k_len) w |= (uint32_t)(*reinterpret_cast<const uint8_t*>(mp + (int64_t)e * P.mask_stride_k) != 0) << (8 * e);
#pragma unroll
              for (int e = 0; e < 4; ++e) ok[e] = ok[e] && ((w >> (8 * e)) & 0xffu) != 0;
            } else if (P.mask_type == 2) {
              if (whole) {
                const u32x2_t w = *reinterpret_cast<const u32x2_t*>(mp);
                add[0] = bf16_lo(w[0]); add[1] = bf16_hi(w[0]); add[2] = bf16_lo(w[1]); add[3] = bf16_hi(w[1]);
              } else {
                for (int e = 0; e < 4; ++e)
                  if (kb + e < k_len) add[e] = bf16_bits_to_f32(*reinterpret_cast<const uint16_t*>(mp + (int64_t)e * P.mask_stride_k * 2));
              }
            } else {
              if (whole) {
                const f32x4_t w = *reinterpret_cast<const f32x4_t*>(mp);
                add[0] = w[0]; add[1] = w[1]; add[2] = w[2]; add[3] = w[3];
              } else {
                for (int e = 0; e < 4; ++e)
                  if (kb + e < k_len) add[e] = *reinterpret_cast<const float*>(mp + (int64_t)e * P.mask_stride_k * 4);
              }
            }
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float x = ok[e] ? s[j][rq * 4 + e] * sl2 + add[e] * OMNI_LOG2E : -INFINITY;
            s[j][rq * 4 + e] = x;
            mx = fmaxf(mx, x);
          }
        }
    }
    attn_softmax_pv_tile<E>(s, mx, v_addr, m_run, l_run, o);
    __syncthreads();                                         // every wave is done with tile t
    if (t + 1 < ntiles) {
      store_tile();
      __syncthreads();
    }
  }

  attn_store_out<E>(o, l_run, P.out, P.ldo, 0, q_start + qi, h, hi, qi < q_len);   // (out_k32_rows != 0 is rejected at validation)
}

template <int DH, bool F16>
int launch_general(const omni_attn_params* p, hipStream_t s) {
  const int qblocks = (p->max_seqlen_q + GQBLK - 1) / GQBLK;
  const long grid = (long)p->B * p->H * qblocks;
  if (grid <= 0 || grid > 0x7fffffffL) return OMNI_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((flash_attn_general_kernel<DH, F16>), dim3((unsigned)grid), dim3(GQ_WAVES * 64), 0, s, *p, qblocks);
  OMNI_CHECK_LAUNCH();
  return OMNI_OK;
}

}  // namespace

extern "C" int omni_flash_attn_general(const omni_attn_params* p, omni_stream stream) {
  if (!p || !p->q || !p->k || !p->v || !p->out || !p->cu_seqlens_q || !p->cu_seqlens_k) return OMNI_ERR_BAD_ARG;
  if (p->B <= 0 || p->H <= 0 || p->H_kv <= 0 || p->max_seqlen_q <= 0 || p->max_seqlen_k < 0) return OMNI_ERR_BAD_ARG;
  if (p->H % p->H_kv != 0) return OMNI_ERR_BAD_ARG;
  if (p->causal != 0 && p->causal != 1) return OMNI_ERR_BAD_ARG;
  if (p->mask_type < 0 || p->mask_type > 3 || (p->mask_type != 0) != (p->mask != nullptr)) return OMNI_ERR_BAD_ARG;
  if (p->head_dim != 64 && p->head_dim != 128) return OMNI_ERR_UNSUPPORTED;
  if (p->qk_int8 != 0 && p->qk_int8 != 1) return OMNI_ERR_BAD_ARG;
  if (p->out_k32_rows < 0) return OMNI_ERR_BAD_ARG;
  if (p->elem_type != OMNI_ELEM_BF16 && p->elem_type != OMNI_ELEM_F16) return OMNI_ERR_BAD_ARG;
  if (p->qk_int8 == 1 && (p->mask_type != 0 || p->causal)) return OMNI_ERR_UNSUPPORTED;
  if (p->qk_int8 == 1 && p->elem_type != OMNI_ELEM_BF16) return OMNI_ERR_UNSUPPORTED;           // SAGE_ATTN is bf16 only
  if (p->qk_int8 == 0 && (p->out_k32_rows != 0 || p->item_skip)) return OMNI_ERR_UNSUPPORTED;   // the int8 path's options
  if (!omni_aligned16(p->q) || !omni_aligned16(p->k) || !omni_aligned16(p->v) || (reinterpret_cast<uintptr_t>(p->out) & 7) ||
      (p->ldq % 8) || (p->ldk % 8) || (p->ldv % 8) || (p->ldo % 4))
    return OMNI_ERR_ALIGN;
  if (p->mask_type == 2 && (reinterpret_cast<uintptr_t>(p->mask) & 1)) return OMNI_ERR_ALIGN;
  if (p->mask_type == 3 && (reinterpret_cast<uintptr_t>(p->mask) & 3)) return OMNI_ERR_ALIGN;
  if (p->qk_int8 == 1) return omni_internal_sage_attn(p, p->item_skip, 0, stream);     // SAGE_ATTN: attention_sage.hip
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (p->elem_type == OMNI_ELEM_F16) return p->head_dim == 128 ? launch_general<128, true>(p, s) : launch_general<64, true>(p, s);
  return p->head_dim == 128 ? launch_general<128, false>(p, s) : launch_general<64, false>(p, s);
}

// Optional capabilities of this build that the ABI version does not tell (fields that went into former struct padding keep
// the version, so a caller has to be able to ask whether the library reads them).
extern "C" uint32_t omni_features(void) {
  return OMNI_FEATURE_ATTN_F16 | OMNI_FEATURE_TEACACHE_RAGGED | OMNI_FEATURE_CFG_EULER_RAGGED | OMNI_FEATURE_LORA_MERGE |
         OMNI_FEATURE_TEXT_ENCODER | OMNI_FEATURE_VISION_ENCODER | OMNI_FEATURE_TEXT_DECODE;
}
