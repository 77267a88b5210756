// dev family 0: the first 2-stage BK=64 kernel of round 1 and its timing ablations.
// Textually included by ../gemm.hip in -DOMNI_DEV builds only (tools/build_variants.sh); never part of the product library.
template <int EPI, int ABL = 0>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_bf16_kernel(const omni_gemm_params P, int mtiles0, int tiles_m,
                                                                  int tiles_n, int GROUP_M) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- tile id: XCD-aware bijective remap, then GROUP_M banding -------------------------------
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

  // ---- per-lane DMA source pointers: 4 A rows + 4 W rows, fixed over the K loop ---------------
  const uint16_t* a_src[4];
  const uint16_t* w_src[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = (wave * 4 + j) * 8 + (lane >> 3);            // tile row this lane feeds
    const int c = (lane & 7) ^ ((r >> 1) & 7);                 // logical k-chunk landing in phys chunk lane&7
    int ar = min(m0 + r, M - 1);
    if (G.a_row_map) ar = G.a_row_map[ar];
    a_src[j] = G.A + (int64_t)ar * G.lda + c * 8;
    const int wr = min(n0 + r, N - 1);
    w_src[j] = G.W + (int64_t)wr * K + c * 8;
  }
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;  // LDS byte address of the dynamic region
  auto issue_part = [&](int stage, int kt, int part) {   // part 0..3: one A piece + one W piece (1 KiB each)
    const uint32_t base = lds0 + stage * STAGE_BYTES + (wave * 4) * 1024;
    const int koff = kt * BK;
    glds16(a_src[part] + koff, base + part * 1024);
    glds16(w_src[part] + koff, base + TILE_BYTES + part * 1024);
  };
  auto issue_stage = [&](int stage, int kt) {
#pragma unroll
    for (int j = 0; j < 4; ++j) issue_part(stage, kt, j);
  };

  // ---- per-lane fragment read offsets ---------------------------------------------------------
  const int wm = wave >> 2, wn = wave & 3;
  const int l31 = lane & 31, hi = lane >> 5;
  // per-lane fragment byte offsets per k-step: row*128 + ((ks*2+hi) ^ swz)*16, swz = (row>>1)&7 = (l31>>1)&7
  uint32_t a_base[4], w_base[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const uint32_t chunk = ((uint32_t)(ks * 2 + hi) ^ ((l31 >> 1) & 7)) << 4;
    a_base[ks] = (wm * 128 + l31) * 128 + chunk;
    w_base[ks] = (wn * 64 + l31) * 128 + chunk;
  }

  f32x16_t acc[2][4];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[nb][mb][i] = 0.0f;

  const int nkt = K / BK;
  issue_stage(0, 0);
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    if (ABL != 4 && ABL != 5) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    if (ABL != 1 && ABL != 5 && kt + 1 < nkt) issue_stage(cur ^ 1, kt + 1);
    mma_stage<4, 32 * 128, TILE_BYTES, ABL>(acc, a_base, w_base, lds0 + cur * STAGE_BYTES, [](int) {});
  }

  gemm_epilogue<EPI>(P, G, acc, m0, n0, wm, wn, l31, hi);
}

