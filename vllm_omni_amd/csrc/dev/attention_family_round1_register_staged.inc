// round-1 register-staged flash-attention kernels (NQ = 1 / 2).
// Textually included by ../attention.hip in -DOMNI_DEV builds only (tools/build_variants.sh); never part of the product library.
// NQ = 32-query blocks per wave.  NQ = 1: 4 waves x 32 queries, 2 workgroups / CU (two waves per SIMD overlap each other).
// NQ = 2: 4 waves x 64 queries, ONE wave per SIMD with ~400 registers: every K / V^T fragment read from LDS feeds TWO
// MFMAs, and staging traffic + barriers per query halve (the NQ = 1 loop is LDS-traffic-bound: each wave re-reads all
// of K and V for only 32 queries).
template <int NQ>
__global__ __launch_bounds__(NWAVES * 64, (NQ == 1 ? 2 : 1)) void flash_attn_fwd_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
    uint16_t* __restrict__ out, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
    const int32_t* __restrict__ cu_seqlens, int n_heads_total, int H, float scale_log2e) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;

  // heads fastest -> block b runs on XCD b%8, so every q-block of a head lands on the same XCD's L2
  const int hb = blockIdx.x % n_heads_total;
  const int qb = blockIdx.x / n_heads_total;
  const int b = hb / H, h = hb - b * H;
  const int seq_start = cu_seqlens[b];
  const int seq_len = cu_seqlens[b + 1] - seq_start;
  constexpr int QBLK = 32 * NWAVES * NQ;   // queries per workgroup
  if (qb * QBLK >= seq_len) return;

  const uint16_t* kbase = k + (int64_t)seq_start * ldk + h * DH;
  const uint16_t* vbase = v + (int64_t)seq_start * ldv + h * DH;

  // ---- Q fragments (B operand): lane holds q = l31, d = ks*16 + hi*8 .. +8 ---------------------
  bf16x8_t qf[NQ][8];
#pragma unroll
  for (int bq = 0; bq < NQ; ++bq) {
    const int qrow = min(qb * QBLK + (wave * NQ + bq) * 32 + l31, seq_len - 1);
    const uint16_t* qp = q + (int64_t)(seq_start + qrow) * ldq + h * DH + hi * 8;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[bq][ks] = *reinterpret_cast<const bf16x8_t*>(qp + ks * 16);
    // make the fragments opaque: otherwise hipcc REMATERIALISES these global loads inside the KV loop (to save
    // VGPRs) and every QK^T MFMA then waits on an L2 round trip (seen as vmcnt(7..0) waits in the loop)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) asm volatile("" : "+v"(qf[bq][ks]));
  }

  // ---- staging: thread t moves 16-B chunks id = t + 256*i; key = id>>4, c = id&15 -----------------------
  // Loads go through buffer descriptors: the per-thread byte offset is loop-invariant (voffset), the tile
  // offset is an SGPR (soffset) -> ZERO per-tile address VALU (the flat-address form cost ~90 VALU per tile,
  // much of it quarter-rate 64-bit multiplies), and rows past the sequence end are out of the descriptor's range
  // and read as 0 (no clamp; those keys are masked to -inf anyway).
  u32x4_t kreg[4], vreg[4];
  uint32_t k_wr_off[4], v_wr_off[4], k_ld_off[4], v_ld_off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = tid + 256 * i;
    const int key = id >> 4, c = id & 15;
    k_wr_off[i] = key * 256 + ((c ^ (key & 15)) << 4);
    v_wr_off[i] = K_TILE_BYTES + (c >> 2) * 4096 + (key >> 2) * 256 + (key & 3) * 64 + (c & 3) * 16;
    k_ld_off[i] = (uint32_t)(key * ldk * 2 + c * 16);
    v_ld_off[i] = (uint32_t)(key * ldv * 2 + c * 16);
  }
  const uint32_t k_bytes = (uint32_t)((int64_t)(seq_len - 1) * ldk * 2 + DH * 2);
  const uint32_t v_bytes = (uint32_t)((int64_t)(seq_len - 1) * ldv * 2 + DH * 2);
  const __amdgpu_buffer_rsrc_t k_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)kbase, 0, k_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t v_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)vbase, 0, v_bytes, 0x00020000);
  const uint32_t k_tile_stride = (uint32_t)(KVBLK * ldk * 2), v_tile_stride = (uint32_t)(KVBLK * ldv * 2);
  auto load_tile = [&](int t) {
    const uint32_t ks_ = __builtin_amdgcn_readfirstlane(t * k_tile_stride);
    const uint32_t vs_ = __builtin_amdgcn_readfirstlane(t * v_tile_stride);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      kreg[i] = __builtin_amdgcn_raw_buffer_load_b128(k_rsrc, k_ld_off[i], ks_, 0);
      vreg[i] = __builtin_amdgcn_raw_buffer_load_b128(v_rsrc, v_ld_off[i], vs_, 0);
    }
  };
  auto store_tile = [&](int stage) {
    char* sb = smem + stage * STAGE_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<u32x4_t*>(sb + k_wr_off[i]) = kreg[i];
      *reinterpret_cast<u32x4_t*>(sb + v_wr_off[i]) = vreg[i];
    }
  };

  // ---- fragment read addresses ------------------------------------------------------------------
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  // K: row key = j*32 + l31, chunk (ks*2+hi) ^ (key&15)      (j*32 keeps key&15 = l31&15)
  uint32_t k_addr[8];   // per k-step: key-row offset + swizzled 16-B chunk (sub-block j adds 32*256 as an immediate)
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) k_addr[ks] = l31 * 256 + ((((uint32_t)(ks * 2 + hi)) ^ (l31 & 15)) << 4);
  // V (tr read): g = lane>>4, m = lane&15:  base = (m>>2)*64 + (g&1)*32 + (m&3)*8 + hi*256
  const uint32_t v_lane_off = K_TILE_BYTES + ((lane & 15) >> 2) * 64 + ((lane >> 4) & 1) * 32 + (lane & 3) * 8 + hi * 256;

  f32x16_t o[NQ][4];
  float m_run[NQ], l_run[NQ];
#pragma unroll
  for (int bq = 0; bq < NQ; ++bq) {
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int i = 0; i < 16; ++i) o[bq][d][i] = 0.0f;
    m_run[bq] = -INFINITY;
    l_run[bq] = 0.0f;
  }

  const int ntiles = (seq_len + KVBLK - 1) / KVBLK;
  load_tile(0);
  store_tile(0);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    const int kv0 = t * KVBLK;
    if (t + 1 < ntiles) load_tile(t + 1);  // in flight under this tile's MFMAs
    const char* sb = smem + cur * STAGE_BYTES;

    // ---- Sᵀ = K Qᵀ : two 32-key sub-blocks = 16 MFMAs; K fragments are read 4 deep ahead of their MFMA
    // (hand-issued ds_read_b128 + counted lgkmcnt: hipcc otherwise waits lgkmcnt(0) before every single MFMA).
    f32x16_t s[NQ][2];
#pragma unroll
    for (int bq = 0; bq < NQ; ++bq)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) s[bq][j][i] = 0.0f;
    {
      const uint32_t kst = lds0 + cur * STAGE_BYTES;
      bf16x8_t kf[4];
#define OMNI_KREAD(i) \
  kf[(i) & 3] = (((i) >> 3) ? lds_read16<32 * 256>(k_addr[(i) & 7] + kst) : lds_read16<0>(k_addr[(i) & 7] + kst))
      OMNI_KREAD(0); OMNI_KREAD(1); OMNI_KREAD(2); OMNI_KREAD(3);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (i <= 12) asm volatile("s_waitcnt lgkmcnt(3)" ::: "memory");
        else if (i == 13) asm volatile("s_waitcnt lgkmcnt(2)" ::: "memory");
        else if (i == 14) asm volatile("s_waitcnt lgkmcnt(1)" ::: "memory");
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int bq = 0; bq < NQ; ++bq)
          s[bq][i >> 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[i & 3], qf[bq][i & 7], s[bq][i >> 3], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (i + 4 < 16) OMNI_KREAD(i + 4);
      }
      __builtin_amdgcn_s_setprio(0);
#undef OMNI_KREAD
    }
    // ---- mask the ragged tail (last tile only; wave-uniform branch) ---------------------------
    if (kv0 + KVBLK > seq_len) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kv0 + j * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
          if (key >= seq_len) {
#pragma unroll
            for (int bq = 0; bq < NQ; ++bq) s[bq][j][r] = -INFINITY;
          }
        }
    }
    // ---- online softmax (lane-local; one cross-half exchange for the max), per 32-query block -----------
    bf16x8_t pf[NQ][2][2];
#pragma unroll
    for (int bq = 0; bq < NQ; ++bq) {
      float mx = s[bq][0][0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[bq][0][r]);
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[bq][1][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      // defer-max (cdna guide T13): while the row max grows by less than 2^DEFER (in the exponent's log2 units) keep
      // the OLD reference max — P is then bounded by 2^DEFER instead of 1 (harmless in bf16/fp32) and the 64-register
      // rescale of O is skipped.  The decision is taken AFTER the previous tile's P·V is complete and BEFORE this
      // tile's P is exponentiated, so O, l and P always share one reference max.
      constexpr float DEFER = 6.0f;
      if (!__all((mx - m_run[bq]) * scale_log2e <= DEFER)) {
        const float m_new = fmaxf(m_run[bq], mx);
        const float alpha = __builtin_amdgcn_exp2f((m_run[bq] - m_new) * scale_log2e);
        m_run[bq] = m_new;
        l_run[bq] *= alpha;
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
          for (int i = 0; i < 16; ++i) o[bq][d][i] *= alpha;
      }
      const float mneg = -m_run[bq] * scale_log2e;
      float psum = 0.0f;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int ss = 0; ss < 2; ++ss)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[bq][j][ss * 8 + e], scale_log2e, mneg));
            psum += p;
            pf[bq][j][ss][e] = (__bf16)p;
          }
      l_run[bq] += psum;
    }

    // 16 MFMAs, i -> (j = i>>3, ss = (i>>2)&1, d = i&3); each needs one Vᵀ fragment = two transposed reads.
    // Fragments are fetched THREE MFMAs ahead (hand-issued + counted lgkmcnt; hipcc keeps only one ahead and
    // every MFMA then eats an LDS round trip).
    {
      const uint32_t vb = lds0 + cur * STAGE_BYTES + v_lane_off;
      u32x2_t vlo[4], vhi[4];
#define OMNI_VOFF(i) (((i) & 3) * 4096 + ((((i) >> 3) * 8 + (((i) >> 2) & 1) * 4) * 256))
#define OMNI_VREAD(i)                                   \
  do {                                                  \
    vlo[(i) & 3] = tr_read8<OMNI_VOFF(i)>(vb);      \
    vhi[(i) & 3] = tr_read8<OMNI_VOFF(i) + 512>(vb); \
  } while (0)
#define OMNI_PV(i)                                                                                             \
  do {                                                                                                         \
    if ((i) <= 13) asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");                                          \
    else if ((i) == 14) asm volatile("s_waitcnt lgkmcnt(2)" ::: "memory");                                     \
    else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                         \
    {                                                                                                          \
      typedef __attribute__((ext_vector_type(4))) uint32_t u4_;                                                \
      const u4_ w_ = {vlo[(i) & 3][0], vlo[(i) & 3][1], vhi[(i) & 3][0], vhi[(i) & 3][1]};                     \
      _Pragma("unroll") for (int bq = 0; bq < NQ; ++bq)                                                         \
        o[bq][(i) & 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, w_),             \
                                                  pf[bq][(i) >> 3][((i) >> 2) & 1], o[bq][(i) & 3], 0, 0, 0);  \
    }                                                                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                                         \
  } while (0)
      OMNI_VREAD(0); OMNI_VREAD(1); OMNI_VREAD(2);
      __builtin_amdgcn_s_setprio(1);
      OMNI_PV(0);  OMNI_VREAD(3);  OMNI_PV(1);  OMNI_VREAD(4);  OMNI_PV(2);  OMNI_VREAD(5);  OMNI_PV(3);  OMNI_VREAD(6);
      OMNI_PV(4);  OMNI_VREAD(7);  OMNI_PV(5);  OMNI_VREAD(8);  OMNI_PV(6);  OMNI_VREAD(9);  OMNI_PV(7);  OMNI_VREAD(10);
      OMNI_PV(8);  OMNI_VREAD(11); OMNI_PV(9);  OMNI_VREAD(12); OMNI_PV(10); OMNI_VREAD(13); OMNI_PV(11); OMNI_VREAD(14);
      OMNI_PV(12); OMNI_VREAD(15); OMNI_PV(13); OMNI_PV(14); OMNI_PV(15);
      __builtin_amdgcn_s_setprio(0);
#undef OMNI_PV
#undef OMNI_VREAD
#undef OMNI_VOFF
    }

    if (t + 1 < ntiles) store_tile(cur ^ 1);
    __syncthreads();
  }

  // ---- epilogue: O[q][d] = Oᵀ / l ; lane holds q = l31, d = dblk*32 + 8*qd + 4*hi + {0..3} -------
#pragma unroll
  for (int bq = 0; bq < NQ; ++bq) {
    const float l_tot = l_run[bq] + __shfl_xor(l_run[bq], 32, 64);
    const float inv = 1.0f / l_tot;
    const int qrow = qb * QBLK + (wave * NQ + bq) * 32 + l31;
    if (qrow < seq_len) {
      uint16_t* op = out + (int64_t)(seq_start + qrow) * ldo + h * DH + hi * 4;
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
          u32x2_t w;
          w[0] = pack_bf16x2(o[bq][d][qd * 4 + 0] * inv, o[bq][d][qd * 4 + 1] * inv);
          w[1] = pack_bf16x2(o[bq][d][qd * 4 + 2] * inv, o[bq][d][qd * 4 + 3] * inv);
          *reinterpret_cast<u32x2_t*>(op + d * 32 + qd * 8) = w;
        }
    }
  }
}

