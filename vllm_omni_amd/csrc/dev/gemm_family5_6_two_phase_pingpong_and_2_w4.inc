// dev families 5 / 6 (two-phase ping-pong: <= the four-phase kernel, DESIGN.md 7 item 15) and 2 (hipcc-scheduled 4 waves x 128x128).
// Textually included by ../gemm.hip in -DOMNI_DEV builds only (tools/build_variants.sh); never part of the product library.
// (what these kernels shared with the product ping-pong kernel's round-2 form and the product no longer carries)
#ifndef OMNI_PP_SETPRIO
#define OMNI_PP_SETPRIO 1
#endif
#ifndef OMNI_PP_ABL
#define OMNI_PP_ABL 0
#endif
OMNI_DEVINL void pp_mfma(f32x16_t& acc, const bf16x8_t& a, const bf16x8_t& b) {
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
// ------------------------------------------------------------------------------------------------
// Two-phase ping-pong variant (OMNI_GEMM_VARIANT=5): same half-tiles, accumulators and k order as gemm_bf16_pp_kernel, but a
// K-tile is consumed in TWO phases of 16 MFMAs (512 matrix-pipe cycles): phase a = A rows of mq 0 x both nq (reads h0, h1,
// h2: 16 ds_read_b128), phase b = mq 1 x both nq (reads h3: 8).  Half the barriers per K-tile, and a load section has 512
// instead of 256 partner-MFMA cycles to hide its reads and its four DMA pieces.  The LDS ring has 10 half-tile slots (all
// 160 KiB; half-tile j = 4*tile + h in slot j % 10), which lets the DMA run further ahead:
//   phase a of tile t issues h2 of tile t+1, then h0 of tile t+2;  phase b issues h3 of tile t+1, then h1 of tile t+2
//   (leads of 2 / 4 / 2 / 3 phases; within a phase the half-tile that is needed sooner goes first).
//   RAW: at the end of a load section everything the NEXT phase reads was issued at least one phase ago and FIRST in its
//        phase; the three half-tiles issued after it may stay in flight: vmcnt(6).
//   WAR: the previous occupant of a slot (half-tile j - 10) was last read >= 2 phases before the slot is re-issued.
// ------------------------------------------------------------------------------------------------
constexpr int P2_SLOTS = 10;
static_assert(P2_SLOTS * PSLOT_BYTES <= RLDS_BYTES, "10-slot ring must fit the 160 KiB allocation");

template <int EPI, bool DMA_FIRST>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_bf16_pp2_kernel(const omni_gemm_params P, int mtiles0, int tiles_m,
                                                                      int tiles_n, int GROUP_M) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwg = tiles_m * tiles_n;
  const int bid = blockIdx.x;
  const int lid = omni_xcd_contiguous(bid, nwg);
  const int band_sz = GROUP_M * tiles_n;
  const int band = lid / band_sz, in_band = lid - band * band_sz;
  const int first_m = band * GROUP_M;
  const int gm = min(GROUP_M, tiles_m - first_m);
  const int mt = first_m + in_band % gm;
  const int nt = in_band / gm;
  const int gi = (mt >= mtiles0) ? 1 : 0;
  const omni_gemm_group G = pick_group(P, gi);
  const int m0 = (gi ? mt - mtiles0 : mt) * BM;
  const int n0 = nt * BN;
  const int M = G.M, N = P.N, K = P.K;
  if (G.tile_skip && G.tile_skip[gi ? mt - mtiles0 : mt]) return;   // device-side predicate (omni_teacache)
  const int wm = wave >> 2, wn = wave & 3;
  const int l31 = lane & 31, hi = lane >> 5;

  uint32_t a_off[2][2], w_off[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int lr = (wave * 2 + i) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((lr >> 1) & 7);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      int ar = min(m0 + (lr >> 6) * 128 + q * 64 + (lr & 63), M - 1);
      if (G.a_row_map) ar = G.a_row_map[ar];
      const int64_t ae = G.a_k32_rows ? ((int64_t)(c >> 2) * G.a_k32_rows + ar) * 32 + (c & 3) * 8
                                      : (int64_t)ar * G.lda + c * 8;
      a_off[q][i] = (uint32_t)(ae * 2);
      const int wr = min(n0 + (lr >> 5) * 64 + q * 32 + (lr & 31), N - 1);
      const int64_t we = P.w_k32_blocked ? ((int64_t)(c >> 2) * N + wr) * 32 + (c & 3) * 8 : (int64_t)wr * K + c * 8;
      w_off[q][i] = (uint32_t)(we * 2);
    }
  }
  const int64_t astep = G.a_k32_rows ? (int64_t)G.a_k32_rows * 128 : 128;
  const int64_t wstep = P.w_k32_blocked ? (int64_t)N * 128 : 128;
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  const int nkt = K / PBK;
  const char* const Ab = reinterpret_cast<const char*>(G.A);
  const char* const Wb = reinterpret_cast<const char*>(G.W);
  auto mod10 = [](int x) { return x - (x >= 10 ? 10 : 0) - (x >= 20 ? 10 : 0); };   // x < 30
  // half-tile h (compile time) of K-tile `tile`, whose ring slot is `slot` (uniform)
#define OMNI_P2_ISSUE(h, tile, slot)                                                                        \
  do {                                                                                                      \
    const int t_ = (tile);                                                                                  \
    const uint32_t dst_ = lds0 + (uint32_t)(slot) * PSLOT_BYTES + (wave * 2) * 1024;                          \
    if ((h) == 0 || (h) == 3) {                                                                             \
      const char* b_ = Ab + t_ * astep;                                                                     \
      glds16_saddr(b_, a_off[(h) == 3][0], dst_);                                                           \
      glds16_saddr(b_, a_off[(h) == 3][1], dst_ + 1024);                                                    \
    } else {                                                                                                \
      const char* b_ = Wb + t_ * wstep;                                                                     \
      glds16_saddr(b_, w_off[(h) == 2][0], dst_);                                                           \
      glds16_saddr(b_, w_off[(h) == 2][1], dst_ + 1024);                                                    \
    }                                                                                                       \
  } while (0)

  uint32_t a_rd[4], w_rd[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const uint32_t chunk = ((uint32_t)(ks * 2 + hi) ^ ((l31 >> 1) & 7)) << 4;
    a_rd[ks] = lds0 + (wm * 64 + l31) * 128 + chunk;
    w_rd[ks] = lds0 + (wn * 32 + l31) * 128 + chunk;
  }

  // ---- prologue: issue order h0(0) h1(0) h2(0) h0(1) h3(0) h1(1) (= the steady-state schedule of phases -4 .. -1) ----
  OMNI_P2_ISSUE(0, 0, 0); OMNI_P2_ISSUE(1, 0, 1); OMNI_P2_ISSUE(2, 0, 2);
  if (nkt > 1) OMNI_P2_ISSUE(0, 1, 4);
  OMNI_P2_ISSUE(3, 0, 3);
  if (nkt > 1) OMNI_P2_ISSUE(1, 1, 5);
  f32x16_t acc[2][4];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    float bini[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = n0 + wn * 64 + hi * 4 + nb * 32 + q * 8;
      u32x2_t b = {0u, 0u};
      if (G.bias && n < N) b = *reinterpret_cast<const u32x2_t*>(G.bias + n);
      bini[q * 4 + 0] = bf16_lo(b[0]); bini[q * 4 + 1] = bf16_hi(b[0]);
      bini[q * 4 + 2] = bf16_lo(b[1]); bini[q * 4 + 3] = bf16_hi(b[1]);
    }
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[nb][mb][i] = bini[i];
  }
  if (nkt > 1) {
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  if (wm) __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  bf16x8_t wf[2][4], af[2][4];
#define OMNI_P2_READ_A(slot)                                                               \
  do {                                                                                     \
    const uint32_t sb_ = (uint32_t)(slot) * PSLOT_BYTES;                                   \
    _Pragma("unroll") for (int ks_ = 0; ks_ < 4; ++ks_) {                                  \
      af[0][ks_] = lds_read16<0>(a_rd[ks_] + sb_);                                         \
      af[1][ks_] = lds_read16<32 * 128>(a_rd[ks_] + sb_);                                  \
    }                                                                                      \
  } while (0)
#define OMNI_P2_READ_W(nq, slot)                                                           \
  do {                                                                                     \
    const uint32_t sb_ = (uint32_t)(slot) * PSLOT_BYTES;                                   \
    _Pragma("unroll") for (int ks_ = 0; ks_ < 4; ++ks_) wf[nq][ks_] = lds_read16<0>(w_rd[ks_] + sb_); \
  } while (0)
#define OMNI_P2_MMA(mq, steady)                                                                            \
  do {                                                                                                     \
    if (steady) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");                                           \
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                  \
    __builtin_amdgcn_s_barrier();                                                                          \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
    if (OMNI_PP_SETPRIO) __builtin_amdgcn_s_setprio(1);                                                    \
    _Pragma("unroll") for (int ks_ = 0; ks_ < 4; ++ks_) {                                                  \
      pp_mfma(acc[0][2 * (mq)], wf[0][ks_], af[0][ks_]);                                                   \
      pp_mfma(acc[0][2 * (mq) + 1], wf[0][ks_], af[1][ks_]);                                               \
      pp_mfma(acc[1][2 * (mq)], wf[1][ks_], af[0][ks_]);                                                   \
      pp_mfma(acc[1][2 * (mq) + 1], wf[1][ks_], af[1][ks_]);                                               \
    }                                                                                                      \
    if (OMNI_PP_SETPRIO) __builtin_amdgcn_s_setprio(0);                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
    __builtin_amdgcn_s_barrier();                                                                          \
    asm volatile("" ::: "memory");                                                                         \
  } while (0)

  int tb = 0;                                    // (4 * t) % 10: ring slot of half-tile h0 of the current K-tile
#pragma unroll 1
  for (int t = 0; t < nkt; ++t) {
    const bool n1 = t + 1 < nkt, n2 = t + 2 < nkt;
    const int s_h1 = mod10(tb + 1), s_h2 = mod10(tb + 2), s_h3 = mod10(tb + 3);
    const int s1_h2 = mod10(tb + 6), s1_h3 = mod10(tb + 7), s2_h0 = mod10(tb + 8), s2_h1 = mod10(tb + 9);
    // phase a: A rows of mq 0 x both nq
    if (DMA_FIRST) {
      if (n1) OMNI_P2_ISSUE(2, t + 1, s1_h2);
      if (n2) OMNI_P2_ISSUE(0, t + 2, s2_h0);
    }
    OMNI_P2_READ_A(tb);
    OMNI_P2_READ_W(0, s_h1);
    OMNI_P2_READ_W(1, s_h2);
    if (!DMA_FIRST) {
      if (n1) OMNI_P2_ISSUE(2, t + 1, s1_h2);
      if (n2) OMNI_P2_ISSUE(0, t + 2, s2_h0);
    }
    OMNI_P2_MMA(0, n2);
    // phase b: A rows of mq 1 x both nq
    if (DMA_FIRST) {
      if (n1) OMNI_P2_ISSUE(3, t + 1, s1_h3);
      if (n2) OMNI_P2_ISSUE(1, t + 2, s2_h1);
    }
    OMNI_P2_READ_A(s_h3);
    if (!DMA_FIRST) {
      if (n1) OMNI_P2_ISSUE(3, t + 1, s1_h3);
      if (n2) OMNI_P2_ISSUE(1, t + 2, s2_h1);
    }
    OMNI_P2_MMA(1, n2);
    tb = mod10(tb + 4);
  }
  if (!wm) __builtin_amdgcn_s_barrier();
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
#undef OMNI_P2_MMA
#undef OMNI_P2_READ_W
#undef OMNI_P2_READ_A
#undef OMNI_P2_ISSUE

  gemm_epilogue_lds<EPI>(P, G, acc, m0, n0, wm, wn, l31, hi, smem, tid);
}


// ------------------------------------------------------------------------------------------------
// W4 variant: 4 waves x (128 x 128), ONE wave per SIMD owning the whole 512-entry register file (256 accumulator
// registers + double-buffered fragments).  Same 5-stage BK=32 LDS ring and continuous pipeline as the ring kernel.
// Why: the ablation (tools/bench_ablate_ring.py) shows DMA landings and fragment reads fighting for LDS bandwidth on
// real data; a 128x128 wave tile needs 8 fragment reads per 16 MFMAs instead of 6 per 8 (-33 % LDS read bytes) and
// the barrier only joins 4 waves.  All latency hiding is intra-wave: reads run two k-steps ahead, one DMA piece and
// one or two reads ride in the issue shadow of every group of 4 MFMAs.
// ------------------------------------------------------------------------------------------------
constexpr int W4_THREADS = 256;

template <int EPI>
__global__ __launch_bounds__(W4_THREADS, 1) void gemm_bf16_w4_kernel(const omni_gemm_params P, int mtiles0, int tiles_m,
                                                                      int tiles_n, int GROUP_M) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int lid = omni_xcd_contiguous(bid, nwg);
  const int band_sz = GROUP_M * tiles_n;
  const int band = lid / band_sz, in_band = lid - band * band_sz;
  const int first_m = band * GROUP_M;
  const int gm = min(GROUP_M, tiles_m - first_m);
  const int mt = first_m + in_band % gm;
  const int nt = in_band / gm;
  const int gi = (mt >= mtiles0) ? 1 : 0;
  const omni_gemm_group G = pick_group(P, gi);
  const int m0 = (gi ? mt - mtiles0 : mt) * BM;
  const int n0 = nt * BN;
  const int M = G.M, N = P.N, K = P.K;

  // DMA sources: a stage is 16 A pieces + 16 W pieces of (16 rows x 64 B); wave w moves pieces w*4 .. w*4+3 of each
  const uint16_t* a_src[4];
  const uint16_t* w_src[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = (wave * 4 + j) * 16 + (lane >> 2);
    const int c = (lane & 3) ^ ((r >> 2) & 3);
    int ar = min(m0 + r, M - 1);
    if (G.a_row_map) ar = G.a_row_map[ar];
    a_src[j] = G.A + (int64_t)ar * G.lda + c * 8;
    const int wr = min(n0 + r, N - 1);
    w_src[j] = G.W + (int64_t)wr * K + c * 8;
  }
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  auto issue_piece = [&](int slot, int st, int piece) {   // piece 0..7 = A0, W0, A1, W1, ...
    const uint32_t base = lds0 + slot * RSTAGE_BYTES + (wave * 4) * 1024;
    const int koff = st * RBK, part = piece >> 1;
    if (piece & 1) glds16(w_src[part] + koff, base + ROP_BYTES + part * 1024);
    else glds16(a_src[part] + koff, base + part * 1024);
  };
  auto issue_stage = [&](int slot, int st) {
#pragma unroll
    for (int p = 0; p < 8; ++p) issue_piece(slot, st, p);
  };

  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, hi = lane >> 5;
  uint32_t a_base[2], w_base[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const uint32_t chunk = ((uint32_t)(ks * 2 + hi) ^ ((l31 >> 2) & 3)) << 4;
    a_base[ks] = (wm * 128 + l31) * 64 + chunk;
    w_base[ks] = ROP_BYTES + (wn * 128 + l31) * 64 + chunk;
  }

  f32x16_t acc[4][4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[nb][mb][i] = 0.0f;

  const int nst = K / RBK;
  constexpr int LEAD = RSTAGES - 1;
#pragma unroll
  for (int st = 0; st < LEAD; ++st)
    if (st < nst) issue_stage(st, st);
  bf16x8_t wf[2][4], af[2][4];
  constexpr int BS = 32 * 64;   // bytes between 32-row blocks
#define W4_ADDR(slot_, ks)                                  \
  const uint32_t sa_ = lds0 + (slot_) * RSTAGE_BYTES;       \
  const uint32_t aa_ = a_base[ks] + sa_, wa_ = w_base[ks] + sa_;
#define W4_READ_ALL(buf, slot_, ks)                         \
  do {                                                      \
    W4_ADDR(slot_, ks)                                      \
    wf[buf][0] = lds_read16<0>(wa_);                        \
    wf[buf][1] = lds_read16<BS>(wa_);                       \
    wf[buf][2] = lds_read16<2 * BS>(wa_);                   \
    wf[buf][3] = lds_read16<3 * BS>(wa_);                   \
    af[buf][0] = lds_read16<0>(aa_);                        \
    af[buf][1] = lds_read16<BS>(aa_);                       \
    af[buf][2] = lds_read16<2 * BS>(aa_);                   \
    af[buf][3] = lds_read16<3 * BS>(aa_);                   \
  } while (0)
#define W4_GROUP(buf, mb)                                                                                     \
  acc[0][mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[buf][0], af[buf][mb], acc[0][mb], 0, 0, 0);         \
  acc[1][mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[buf][1], af[buf][mb], acc[1][mb], 0, 0, 0);         \
  acc[2][mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[buf][2], af[buf][mb], acc[2][mb], 0, 0, 0);         \
  acc[3][mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[buf][3], af[buf][mb], acc[3][mb], 0, 0, 0);         \
  __builtin_amdgcn_sched_barrier(0);
// 16 MFMAs of one k-step; in their issue shadows: the 8 reads of k-step g+2 (same buffer) and 4 DMA pieces
#define W4_MMA(buf, PREFETCH, nslot_, ks, D0, D1, D2, D3)          \
  do {                                                             \
    W4_ADDR(nslot_, ks)                                            \
    __builtin_amdgcn_sched_barrier(0);                             \
    W4_GROUP(buf, 0)                                               \
    if (PREFETCH) af[buf][0] = lds_read16<0>(aa_);                 \
    D0;                                                            \
    __builtin_amdgcn_sched_barrier(0);                             \
    W4_GROUP(buf, 1)                                               \
    if (PREFETCH) af[buf][1] = lds_read16<BS>(aa_);                \
    D1;                                                            \
    __builtin_amdgcn_sched_barrier(0);                             \
    W4_GROUP(buf, 2)                                               \
    if (PREFETCH) af[buf][2] = lds_read16<2 * BS>(aa_);            \
    D2;                                                            \
    __builtin_amdgcn_sched_barrier(0);                             \
    W4_GROUP(buf, 3)                                               \
    if (PREFETCH) {                                                \
      af[buf][3] = lds_read16<3 * BS>(aa_);                        \
      wf[buf][0] = lds_read16<0>(wa_);                             \
      wf[buf][1] = lds_read16<BS>(wa_);                            \
      wf[buf][2] = lds_read16<2 * BS>(wa_);                        \
      wf[buf][3] = lds_read16<3 * BS>(wa_);                        \
    }                                                              \
    D3;                                                            \
    __builtin_amdgcn_sched_barrier(0);                             \
  } while (0)
  // B_0: own pieces of stages 0,1 landed (stages 2,3 = 16 DMAs may stay in flight)
  if (LEAD - 1 < nst) {
    asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  if (LEAD < nst) issue_stage(LEAD, LEAD);
  W4_READ_ALL(0, 0, 0);
  W4_READ_ALL(1, 0, 1);
  int slot = 0, pslot = RSTAGES - 1;
  for (int st = 0; st + 1 < nst; ++st) {
    const int nslot = (slot + 1 == RSTAGES) ? 0 : slot + 1;
    const bool dma = st > 0 && st + LEAD < nst;
    const int dst = st + LEAD;
#define W4_D(p) if (dma) issue_piece(pslot, dst, p)
    asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
    W4_MMA(0, true, nslot, 0, W4_D(0), W4_D(1), W4_D(2), W4_D(3));
    asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
    W4_MMA(1, true, nslot, 1, W4_D(4), W4_D(5), W4_D(6), W4_D(7));
#undef W4_D
    if (st + LEAD < nst) {
      asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    pslot = slot;
    slot = nslot;
  }
  asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
  W4_MMA(0, false, 0, 0, (void)0, (void)0, (void)0, (void)0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  W4_MMA(1, false, 0, 1, (void)0, (void)0, (void)0, (void)0);
#undef W4_MMA
#undef W4_GROUP
#undef W4_READ_ALL
#undef W4_ADDR
  gemm_epilogue_t<EPI, 4, 4>(P, G, acc, m0 + wm * 128, n0 + wn * 128, l31, hi);
}


