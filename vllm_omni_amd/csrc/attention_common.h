// The attention scheme of attention.hip's header comment as code, each piece once: shared by the four attention*.hip
// translation units and the VAE mid-block attention kernel (vae.hip).  Device-only.
//   * half-wave exchange (v_permlane32_swap) for the row max / row sum of a query that two half-waves share
//   * transposed V reads (ds_read_b64_tr_b16)
//   * the LDS images of a 64-key tile: K row-major with XOR-swizzled 16-B chunks, V blocked [d/32][key/4][4 keys][32 d];
//     the per-lane fragment addresses into them; the C-layout key order of the swapped 32x32 product
//   * the tail that attention_general.hip and attention_sage.hip share: tile staging, the online-softmax + P.V step, the
//     epilogue store
#pragma once
#include "common.h"

#ifdef __HIPCC__

// ---- half-wave exchange: max / sum over the two half-waves WITHOUT touching LDS (a ds_bpermute would break the counted
// lgkmcnt waits of the fragment pipelines): v_permlane32_swap exchanges a[32..63] with b[0..31].  Inline asm with two distinct
// registers — the builtin called with the same value for both operands is folded to one register by hipcc.
OMNI_DEVINL float xhalf_max(float x) {
  uint32_t a = __builtin_bit_cast(uint32_t, x), b = a;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
  return fmaxf(__builtin_bit_cast(float, a), __builtin_bit_cast(float, b));
}
OMNI_DEVINL float xhalf_sum(float x) {
  uint32_t a = __builtin_bit_cast(uint32_t, x), b = a;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
  return __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b);
}

// ---- transposed V reads (hardware 4x4 transpose of 16-bit elements)
// two reads -> the 8 k-elements of one MFMA A fragment; visible to hipcc's waitcnt pass
template <typename FRAG>
OMNI_DEVINL FRAG tr_read_pair(uint32_t lds_addr_a, uint32_t lds_addr_b) {
  typedef __attribute__((ext_vector_type(4))) short s16x4_t;
  typedef __attribute__((ext_vector_type(8))) short s16x8_t;
  typedef __attribute__((address_space(3))) s16x4_t lds_s16x4;
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)lds_addr_a);
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)lds_addr_b);
  return __builtin_bit_cast(FRAG, (s16x8_t)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
// one read (half a fragment) with an immediate offset; invisible to hipcc's waitcnt pass: waits are counted by hand
template <int OFF>
OMNI_DEVINL u32x2_t tr_read8(uint32_t addr) {
  u32x2_t v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
  return v;
}

// ---- LDS images of one 64-key tile (byte offsets within the image)
constexpr int ATTN_KV = 64;                // keys per tile
// K: row-major, PITCH bytes per key (2 * DH for bf16 / fp16, DH for the int8 K of SAGE_ATTN); the 16-B chunk index is XORed
// with the key (mod the chunks of a row): a ds_read_b128 of 32 keys at one logical chunk is conflict-free.  The swizzle is its
// own inverse: an LDS-DMA kernel applies it to the SOURCE chunk of the lane that lands at LDS chunk `ch`.
template <int PITCH>
constexpr OMNI_DEVINL uint32_t attn_k_chunk(int key, int ch) { return (uint32_t)(ch ^ (key & (PITCH / 16 - 1))); }
template <int PITCH>
constexpr OMNI_DEVINL uint32_t attn_k_off(int key, int ch) { return (uint32_t)(key * PITCH) + (attn_k_chunk<PITCH>(key, ch) << 4); }
// this lane's K fragment of k-step ks in the image at `base` (A operand of S^T = K Q^T: key lane & 31 of a 32-key sub-block,
// chunk 2 ks + hi)
template <int PITCH>
constexpr OMNI_DEVINL uint32_t attn_k_frag_addr(uint32_t base, int lane, int ks) {
  return base + (lane & 31) * PITCH + (attn_k_chunk<PITCH>(lane & 31, ks * 2 + (lane >> 5)) << 4);
}
// V (16-bit elements): [d/32][key/4][4 keys][32 d] — each 32-lane half of a tr-read covers one contiguous 256 B
constexpr OMNI_DEVINL uint32_t attn_v_off(int key, int ch) {
  return (uint32_t)((ch >> 2) * (ATTN_KV * 64) + (key >> 2) * 256 + (key & 3) * 64 + (ch & 3) * 16);
}
// this lane's V^T fragment base in the image at `base`: a tr-read's 16-lane group covers 4 keys x 16 d; the upper half-wave
// reads the next 4 keys
template <typename T>   // (T = the caller's own address type: the sum is formed in it, as if written in place)
constexpr OMNI_DEVINL uint32_t attn_vt_lane_addr(T base, int lane) {
  return base + ((lane & 15) >> 2) * 64 + ((lane >> 4) & 1) * 32 + (lane & 3) * 8 + (lane >> 5) * 256;
}
// P.V step (32-row block d of O^T, 32-key sub-block j, 16-key half hf): offset of its V^T fragment from the lane base; the
// second read of the pair is 512 B on
constexpr OMNI_DEVINL int attn_pv_off(int d, int j, int hf) { return d * (ATTN_KV * 64) + (j * 8 + hf * 4) * 256; }
// C layout of the swapped 32x32 product: register r of sub-block j in half-wave hi <-> key, in a tile that starts at key kv0
constexpr OMNI_DEVINL int attn_key_of(int kv0, int j, int r, int hi) { return kv0 + j * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi; }

// ---- the tail that the general and the SAGE_ATTN kernel share (hipcc schedules it: no hand-placed waits)
// The element type of q / k / v / out: the 8-element MFMA fragment, the 32x32x16 MFMA and the round-to-nearest-even pack of two
// fp32 values.  Everything else (addresses, softmax, masks) is type-blind.
template <bool F16>
struct attn_elem;
template <>
struct attn_elem<false> {
  typedef bf16x8_t frag;
  static OMNI_DEVINL f32x16_t mfma(frag a, frag b, f32x16_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
  static OMNI_DEVINL uint32_t pack2(float lo, float hi) { return pack_bf16x2(lo, hi); }
};
template <>
struct attn_elem<true> {
  typedef f16x8_t frag;
  static OMNI_DEVINL f32x16_t mfma(frag a, frag b, f32x16_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
  static OMNI_DEVINL uint32_t pack2(float lo, float hi) { return pack_f16x2(lo, hi); }
};

// Staging, global -> registers: tile t of rows of PITCH bytes (K or V; `ld` in elements of T), 16 B per thread and piece, NTHR
// threads.  Keys past k_len re-read the last one (the caller masks them).
template <int PITCH, int NTHR, typename T>
OMNI_DEVINL void attn_load_tile(u32x4_t (&reg)[ATTN_KV * PITCH / 16 / NTHR], const T* base, int64_t ld, int t, int k_len, int tid) {
  constexpr int NCH = PITCH / 16;
#pragma unroll
  for (int i = 0; i < ATTN_KV * NCH / NTHR; ++i) {
    const int c = tid + i * NTHR;
    const int key = min(t * ATTN_KV + c / NCH, k_len - 1), ch = c % NCH;
    reg[i] = *reinterpret_cast<const u32x4_t*>(base + (int64_t)key * ld + ch * (16 / (int)sizeof(T)));
  }
}
// ... registers -> the K / V image
template <int PITCH, int NTHR, bool V_IMAGE>
OMNI_DEVINL void attn_store_tile(char* image, const u32x4_t (&reg)[ATTN_KV * PITCH / 16 / NTHR], int tid) {
  constexpr int NCH = PITCH / 16;
#pragma unroll
  for (int i = 0; i < ATTN_KV * NCH / NTHR; ++i) {
    const int c = tid + i * NTHR;
    const int key = c / NCH, ch = c % NCH;
    *reinterpret_cast<u32x4_t*>(image + (V_IMAGE ? attn_v_off(key, ch) : attn_k_off<PITCH>(key, ch))) = reg[i];
  }
}

// One tile of the online softmax and O^T += V^T P^T.  s = the two 32-key score accumulators in the log2 domain (masked keys
// at -inf), mx = this lane's max over them; v_addr = attn_vt_lane_addr of the tile's V image.
// A row with nothing attendable so far (m_new == -inf: masks, causal) uses 0 as its reference, so that every p is exp2(-inf) = 0
// instead of exp2(nan).  For the SAGE_ATTN kernel the guard is dead (every tile it visits has at least one
// valid key: it has no masks): it changes none of its values.
template <typename E, int NDB>
OMNI_DEVINL void attn_softmax_pv_tile(const f32x16_t (&s)[2], float mx, uint32_t v_addr, float& m_run, float& l_run,
                                      f32x16_t (&o)[NDB]) {
  typedef typename E::frag frag_t;
  mx = xhalf_max(mx);
  const float m_new = fmaxf(m_run, mx);
  const float m_use = m_new == -INFINITY ? 0.0f : m_new;
  const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
  m_run = m_new;
  float psum = 0.0f;
  uint32_t pk[2][2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      const float p0 = __builtin_amdgcn_exp2f(s[j][r] - m_use), p1 = __builtin_amdgcn_exp2f(s[j][r + 1] - m_use);
      psum += p0 + p1;
      pk[j][r >> 3][(r >> 1) & 3] = E::pack2(p0, p1);
    }
  l_run = l_run * alpha + psum;
#pragma unroll
  for (int d = 0; d < NDB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[d][i] *= alpha;
  // four 16-key steps (sub-block j, half hf) x NDB 32-row blocks of d; P^T's C-layout key order is the MFMA k order
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const u32x4_t p4 = {pk[j][hf][0], pk[j][hf][1], pk[j][hf][2], pk[j][hf][3]};
      const frag_t pf = __builtin_bit_cast(frag_t, p4);
#pragma unroll
      for (int d = 0; d < NDB; ++d) {
        const uint32_t va = v_addr + attn_pv_off(d, j, hf);
        o[d] = E::mfma(tr_read_pair<frag_t>(va, va + 512), pf, o[d]);
      }
    }
}

// Epilogue: lane (query l31, half hi), register r of block d <-> channel 32 d + (r & 3) + 8 (r >> 2) + 4 hi of head h.  `row` =
// the lane's output row, `valid` = it has one.  out_k32_rows = 0: row-major [rows][ldo]; else K32-blocked
// [H * DH / 32][out_k32_rows][32] (what the out-projection GEMM's A operand reads).  Rows without an attendable key get zeros.
template <typename E, int NDB>
OMNI_DEVINL void attn_store_out(const f32x16_t (&o)[NDB], float l_run, uint16_t* out, int64_t ldo, int out_k32_rows, int64_t row,
                                int h, int hi, bool valid) {
  const float l = xhalf_sum(l_run);
  const float inv = l > 0.0f ? 1.0f / l : 0.0f;
  if (valid && (out_k32_rows == 0 || row < out_k32_rows)) {
#pragma unroll
    for (int d = 0; d < NDB; ++d) {
      uint16_t* op = out_k32_rows > 0 ? out + (((int64_t)h * NDB + d) * out_k32_rows + row) * 32 + hi * 4
                                      : out + row * ldo + (h * NDB + d) * 32 + hi * 4;
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        u32x2_t w;
        w[0] = E::pack2(o[d][qd * 4 + 0] * inv, o[d][qd * 4 + 1] * inv);
        w[1] = E::pack2(o[d][qd * 4 + 2] * inv, o[d][qd * 4 + 3] * inv);
        *reinterpret_cast<u32x2_t*>(op + qd * 8) = w;
      }
    }
  }
}

#endif  // __HIPCC__
