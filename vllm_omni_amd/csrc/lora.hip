// omni_lora_merge: W_out[n, k] = bf16( float(W_base[n, k]) + scale * sum_r up[n - row0, r] * down[r, k] ) for one row range of one
// weight matrix, in either weight layout of the project (row-major [N][K] or K32-blocked [K/32][N][32]).
//
// The contraction runs over the adapter rank only (R <= 256: at most 8 MFMA steps of depth 32), so the kernel is an epilogue
// with a little matrix work in front of it: read the W tile, add, round once, store.  One workgroup (4 waves) owns a tile of
// 128 rows n x 64 columns k = two K32 blocks; a wave owns 32 rows = two 16-row MFMA tiles.
//
// MFMA roles (v_mfma_f32_16x16x32_bf16, D[i][j] = sum_kk A[i][kk] B[kk][j]):
//   i = a column k of W, j = a row n of W, kk = the rank index r.
//   A[i][kk] = down[r][k]: needs r contiguous for a fixed k, i.e. down TRANSPOSED - the tile's 64 columns of down are staged
//              once per workgroup into LDS as dT[k][r], zero-filled for r in [R, Rpad) and k >= K (the rank tail is masked here,
//              never by the host).
//   B[kk][j] = up[n][r]: 8 consecutive r of one row - read from global memory in the operand's own layout.
// The accumulator of a 16x16 tile holds, in lane l, column j = l & 15 and rows i = 4 (l >> 4) + reg.  Operand row i of tile
// t (0, 1) is given W column  k = 32 kb + 8 (i / 4) + 4 t + i % 4, so that lane l ends up with the EIGHT consecutive columns
// k = 32 kb + 8 (l >> 4) + 0..7 of row n = l & 15 in its two accumulators: one 16-byte load and one 16-byte store of W per lane, and
// in the K32-blocked layout the four lane groups of a row cover its whole 64-byte [32] piece, contiguous over n: a wave's store
// is 1 KiB of consecutive memory.
// Every element of the row range is read once and written once by the same lane, so W_out may be W_base.
#include "common.h"

namespace {

constexpr int LM_NT = 128;        // rows n per workgroup (32 per wave)
constexpr int LM_KT = 64;         // columns k per workgroup: two K32 blocks
constexpr int LM_RMAX = 256;      // largest rank
constexpr int LM_PAD = 8;         // elements behind each dT row: keeps rows 16-byte aligned and off one bank

struct LoraMergeArgs {
  const uint16_t* w_base;
  uint16_t* w_out;
  const uint16_t* up;
  const uint16_t* down;
  int N, K, R, row0, rows, blocked;
  int64_t ldw;
  float scale;
};

// 8 consecutive r of one row of `up` as an MFMA operand; elements at r >= R (and whole rows outside the range) are zero
OMNI_DEVINL bf16x8_t load_up_frag(const uint16_t* __restrict__ up, int R, bool row_ok, size_t row_off, int r, bool vec) {
  u32x4_t v = {0u, 0u, 0u, 0u};
  if (row_ok) {
    if (vec) {                                    // R % 8 == 0: a chunk of 8 lies wholly inside or wholly outside [0, R)
      if (r < R) v = *reinterpret_cast<const u32x4_t*>(up + row_off + r);
    } else {
      uint32_t e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] = (r + j < R) ? (uint32_t)up[row_off + r + j] : 0u;
      v[0] = e[0] | (e[1] << 16);
      v[1] = e[2] | (e[3] << 16);
      v[2] = e[4] | (e[5] << 16);
      v[3] = e[6] | (e[7] << 16);
    }
  }
  return __builtin_bit_cast(bf16x8_t, v);
}

__global__ __launch_bounds__(256) void lora_merge_kernel(const LoraMergeArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t dT[LM_KT * (LM_RMAX + LM_PAD)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = a.R, Rpad = (R + 31) & ~31, pitch = Rpad + LM_PAD;
  const int k0 = blockIdx.x * LM_KT;
  const int n_end = a.row0 + a.rows;

  // ---- stage down[0..R)[k0..k0+64) transposed: dT[kk][r]; global reads run along k (128 bytes per wave)
  {
    const int kk = tid & 63;
    const bool k_ok = k0 + kk < a.K;
    for (int r = tid >> 6; r < Rpad; r += 4) {
      uint16_t v = 0;
      if (k_ok && r < R) v = a.down[(size_t)r * a.K + k0 + kk];
      dT[kk * pitch + r] = v;
    }
  }

  const int g = lane >> 4, j16 = lane & 15;
  const int n_w = a.row0 + blockIdx.y * LM_NT + wave * 32;        // first row of this wave
  const int nkb = (a.K - k0) >= LM_KT ? 2 : 1;                    // K % 32 == 0: the tile holds one or two whole K32 blocks

  // ---- this lane's W pieces: row n = n_w + 16 nt + j16, columns 32 kb + 8 g + 0..7 of the tile
  size_t w_off[2][2];
  bool ok[2][2];
  u32x4_t wv[2][2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int n = n_w + nt * 16 + j16;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int kbg = (k0 >> 5) + kb;
      ok[nt][kb] = n < n_end && kb < nkb;
      w_off[nt][kb] = a.blocked ? ((size_t)kbg * a.N + n) * 32 + 8 * g : (size_t)n * a.ldw + (size_t)kbg * 32 + 8 * g;
      wv[nt][kb] = u32x4_t{0u, 0u, 0u, 0u};
      if (ok[nt][kb]) wv[nt][kb] = *reinterpret_cast<const u32x4_t*>(a.w_base + w_off[nt][kb]);
    }
  }

  f32x4_t acc[2][2][2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[nt][kb][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  __syncthreads();

  const bool vec = (R & 7) == 0;
  const bool row_ok0 = n_w + j16 < n_end, row_ok1 = n_w + 16 + j16 < n_end;
  const size_t up_off0 = (size_t)(n_w + j16 - a.row0) * R, up_off1 = (size_t)(n_w + 16 + j16 - a.row0) * R;
  // operand row i = j16 of tile t reads dT row  32 kb + 8 (i / 4) + 4 t + i % 4
  const int arow = 8 * (j16 >> 2) + (j16 & 3);
  for (int c = 0; c < Rpad; c += 32) {
    const int r = c + 8 * g;
    const bf16x8_t b0 = load_up_frag(a.up, R, row_ok0, up_off0, r, vec);
    const bf16x8_t b1 = load_up_frag(a.up, R, row_ok1, up_off1, r, vec);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(&dT[(32 * kb + arow + 4 * t) * pitch + r]);
        acc[0][kb][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, b0, acc[0][kb][t], 0, 0, 0);
        acc[1][kb][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, b1, acc[1][kb][t], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: scale in fp32 after the sum, one rounding to bf16; scale == 0 hands the base bits through (-0 stays -0)
  const float s = a.scale;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      if (!ok[nt][kb]) continue;
      u32x4_t o = wv[nt][kb];
      if (s != 0.f) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {             // word q = columns 2 q, 2 q + 1 of the lane's eight: tile t = q / 2
          const f32x4_t d = acc[nt][kb][q >> 1];
          const float lo = __builtin_fmaf(s, d[(q & 1) * 2], bf16_lo(wv[nt][kb][q]));
          const float hi = __builtin_fmaf(s, d[(q & 1) * 2 + 1], bf16_hi(wv[nt][kb][q]));
          o[q] = pack_bf16x2(lo, hi);
        }
      }
      *reinterpret_cast<u32x4_t*>(a.w_out + w_off[nt][kb]) = o;
    }
  }
}

int lora_merge(const omni_lora_merge_params* p, omni_stream stream) {
  if (!p || !p->w_base || !p->w_out || !p->up || !p->down) return OMNI_ERR_BAD_ARG;
  if (p->N <= 0 || p->K <= 0) return OMNI_ERR_BAD_ARG;
  if (p->K % 32 != 0) return OMNI_ERR_UNSUPPORTED;
  if (p->R < 1 || p->R > LM_RMAX) return OMNI_ERR_UNSUPPORTED;
  if (p->rows < 1 || p->row0 < 0 || p->row0 > p->N - p->rows) return OMNI_ERR_BAD_ARG;
  if (p->w_k32_blocked != 0 && p->w_k32_blocked != 1) return OMNI_ERR_BAD_ARG;
  if (!p->w_k32_blocked && p->ldw < p->K) return OMNI_ERR_BAD_ARG;
  if (!omni_aligned16(p->w_base) || !omni_aligned16(p->w_out) || !omni_aligned16(p->up) || !omni_aligned16(p->down))
    return OMNI_ERR_ALIGN;
  if (!p->w_k32_blocked && (p->ldw % 8) != 0) return OMNI_ERR_ALIGN;       // (K % 32 == 0 aligns down's pitch and the [32] pieces)
  LoraMergeArgs a{p->w_base, p->w_out, p->up, p->down, p->N, p->K, p->R, p->row0, p->rows, p->w_k32_blocked,
                  p->w_k32_blocked ? (int64_t)p->K : p->ldw, p->scale};
  const dim3 grid((p->K + LM_KT - 1) / LM_KT, (p->rows + LM_NT - 1) / LM_NT);
  lora_merge_kernel<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(a);
  OMNI_CHECK_LAUNCH();
  return OMNI_OK;
}

}  // namespace

// exported as a const pointer, not as a function: see the header (the exported functions of ABI v14 are fixed).  Host pass only:
// a namespace-scope const would otherwise be emitted for the device as well, where its initialiser does not exist
#if !defined(__HIP_DEVICE_COMPILE__)
extern "C" int (*const omni_lora_merge)(const omni_lora_merge_params*, omni_stream) = lora_merge;
#endif
