/*
 * omni_cdna4.h — C ABI of libomni_cdna4.so: the MI355X (gfx950 / CDNA4) kernels behind the
 * Qwen-Image DiT denoising hot path of vllm-omni.
 *
 * The reference (vllm-project/vllm-omni) is 100 % Python and has NO FFI for this path; every GPU
 * kernel it runs comes from PyTorch / vLLM / flash-attn / diffusers.  The entry points below are
 * what a binding for its L0 plug-in points would call.  Each one cites the
 * reference call site (path:line relative to the reference root) whose arithmetic it replaces.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, explicit sizes/strides, a hipStream_t passed as void*;
 *     no torch / ATen types, no allocation inside any call (the caller owns every buffer).
 *   - bf16 tensors are `uint16_t` bit patterns (storage bf16, all arithmetic fp32, one rounding).
 *   - every function returns OMNI_OK (0) or a negative omni_status; it never throws or aborts.
 *     Launch errors are reported through hipGetLastError() -> OMNI_ERR_LAUNCH.
 *   - thread-safe for concurrent calls on different streams; no global mutable state.
 *   - "rows" are tokens.  Batches are RAGGED: B items are concatenated along the row axis
 *     and described by `cu_seqlens` (B+1 prefix sums) or per-row int32 maps, so step-batched
 *     requests with different text lengths need no padding.
 */
#ifndef OMNI_CDNA4_H
#define OMNI_CDNA4_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the functions declared in this header are exported. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef uint16_t omni_bf16;
typedef void* omni_stream; /* hipStream_t */

typedef enum {
  OMNI_OK = 0,
  OMNI_ERR_BAD_ARG = -1,     /* null pointer, non-positive size                       */
  OMNI_ERR_UNSUPPORTED = -2, /* shape outside what the kernel is built for (see each) */
  OMNI_ERR_LAUNCH = -3,      /* hipGetLastError() != hipSuccess after the launch      */
  OMNI_ERR_ALIGN = -4        /* pointer / stride not 16-byte aligned where required   */
} omni_status;

/* Library identity: ABI version (bumped on any signature change) and the gfx target it was built for. */
int omni_abi_version(void);
const char* omni_build_arch(void);
const char* omni_status_string(int status);
/* Optional capabilities, as a bit set.  A field that moves into former struct padding (omni_attn_params.elem_type) keeps the
 * ABI version, so the version cannot tell a library that reads it from one that does not: a caller that is about to set such
 * a field asks here first (and treats a library without this symbol as having no optional capability). */
#define OMNI_FEATURE_ATTN_F16 1u /* omni_flash_attn_general reads omni_attn_params.elem_type and has fp16 kernels */
#define OMNI_FEATURE_TEACACHE_RAGGED 2u /* omni_dit_forward's TeaCache kernels address every item by its own image-row range:
                                         * the items of a batch with omni_dit_batch.teacache set may differ in image rows */
#define OMNI_FEATURE_CFG_EULER_RAGGED 4u /* the library exports omni_cfg_euler_step_ragged: a function pointer, see there */
#define OMNI_FEATURE_LORA_MERGE 8u /* the library exports omni_lora_merge: a function pointer, see there */
#define OMNI_FEATURE_TEXT_ENCODER 16u /* the library exports omni_qwen2_text_forward and its companions: function pointers */
#define OMNI_FEATURE_VISION_ENCODER 32u /* the library exports omni_qwen2_vision_forward, omni_qwen2_text_forward_mm and their
                                        * companions: function pointers */
#define OMNI_FEATURE_TEXT_DECODE 64u /* the library exports omni_qwen2_text_prefill, omni_qwen2_text_decode_step and their
                                      * companions (KV-cache greedy decode of the Qwen2.5-VL text model): function pointers */
uint32_t omni_features(void);

/* ------------------------------------------------------------------------------------------------
 * Grouped GEMM with fused epilogue:  Y_g = epilogue(A_g · W_gᵀ + bias_g)  for g < ngroups (<= 2).
 * Replaces the hipBLASLt GEMMs behind F.linear at
 *   vllm_omni/diffusion/models/qwen_image/qwen_image_transformer.py:380,384 (to_qkv / add_kv_proj),
 *   :452,456 (to_out[0] / to_add_out), :491,501,591,596 (FeedForward), :743,759,798 (img_in/txt_in/proj_out)
 * plus the elementwise ops the reference runs after them (:586-587,592,597 gated residuals,
 * GELU-tanh inside FeedForward, torch.cat at :414-416 for the QKV split-to-joint write).
 * Both groups (image stream, text stream) share N, K and the epilogue and run in ONE launch.
 *
 * A_g  [M_g, K] bf16 row-major, row stride lda (elements); optional a_row_map[M_g] gathers rows.
 * W_g  [N, K]   bf16 row-major ([out, in], the nn.Linear layout; fused QKV rows ordered q|k|v).
 * K % 32 == 0 and N % 8 == 0 (else OMNI_ERR_UNSUPPORTED; K % 64 == 32 runs on the fallback kernel; fp8: K % 128 == 0); M_g >= 1
 * arbitrary (row and column tails of a 256x256 tile are predicated).  Alignment (else OMNI_ERR_ALIGN): A, W 16 bytes and
 * lda % 8 == 0; out 8 bytes and ldo % 4 == 0; GATE_RES ldres % 4 == 0 and gate_item_stride % 4 == 0.  The bias, res, gate,
 * out1 and out2 POINTERS are not checked: the kernels read and write them as 8-byte vectors and assume 8-byte alignment.  Outputs,
 * bias, residual and gate that are all 16-byte aligned with strides % 8 == 0 take the row-coalesced epilogue (required for
 * K32-blocked outputs and SPLIT3_QKNORM_ROPE); anything less takes the fallback kernel's direct epilogue — the same bits.
 * ---------------------------------------------------------------------------------------------- */
typedef enum {
  OMNI_EPI_BIAS = 0,          /* y = acc + bias                                              */
  OMNI_EPI_BIAS_GELU_TANH = 1,/* y = gelu_tanh(acc + bias)                                   */
  OMNI_EPI_BIAS_GATE_RES = 2, /* y = res + gate[item(row)] * (acc + bias)   (res may alias y) */
  OMNI_EPI_BIAS_SPLIT3 = 3,   /* y = acc + bias, column block n/split_n selects out/out1/out2 */
  OMNI_EPI_BIAS_SPLIT3_QKNORM_ROPE = 4 /* SPLIT3, and the out / out1 blocks (q, k) additionally get the per-head
                               * RMSNorm(128) * w and the interleaved RoPE of omni_qk_norm_rope applied to the bf16-rounded
                               * linear output before the store (bit-identical to SPLIT3 followed by omni_qk_norm_rope);
                               * needs split_n % 128 == 0 and the qk_* fields of every group */
} omni_epilogue;

typedef struct {
  const omni_bf16* A;
  int64_t lda;
  const int32_t* a_row_map; /* nullable: source row of logical row r (gather)              */
  int32_t M;
  const omni_bf16* W;       /* [N, K], ld = K                                              */
  const omni_bf16* bias;    /* [N], nullable                                               */
  omni_bf16* out;           /* [*, ldo]                                                    */
  omni_bf16* out1;          /* SPLIT3 only: columns [split_n, 2*split_n)                   */
  omni_bf16* out2;          /* SPLIT3 only: columns [2*split_n, 3*split_n)                 */
  int64_t ldo;
  const int32_t* out_row_map; /* nullable: destination row of logical row r (scatter)      */
  const omni_bf16* res;     /* GATE_RES: residual, same row indexing as out                */
  int64_t ldres;
  const omni_bf16* gate;    /* GATE_RES: gate[item * gate_item_stride + n]                 */
  int64_t gate_item_stride;
  const int32_t* row_item_map; /* nullable: item (batch element) of logical row r          */
  int32_t rows_per_item;    /* used when row_item_map == NULL: item = r / rows_per_item    */
  /* SPLIT3_QKNORM_ROPE only: RMSNorm weights [128] of the q and k heads of this stream, RoPE tables [npos, 64] and the
   * table row of every OUTPUT row (indexed by out_row_map[r], or r) */
  const omni_bf16* qk_norm_q_w;
  const omni_bf16* qk_norm_k_w;
  const omni_bf16* qk_rope_cos;
  const omni_bf16* qk_rope_sin;
  const int32_t* qk_row_pos;
  float qk_eps;
  int32_t a_k32_rows;       /* 0: A is row-major [*, lda].  R > 0: A is K32-blocked [K/32][R][32] (element (r,k) at
                             * ((k/32)*R + r)*32 + k%32; lda ignored; a_row_map still picks r).  Same idea as
                             * omni_gemm_params.w_k32_blocked, for activations produced by this library's own kernels */
  int32_t out_k32_rows;     /* 0: out is row-major [*, ldo].  R > 0: out is written K32-blocked [N/32][R][32] (ldo
                             * ignored; BIAS / BIAS_GELU_TANH epilogues only) so that the next GEMM can read it blocked */
  float qk_q_scale;         /* SPLIT3_QKNORM_ROPE only, ABI v5 (occupies former padding): 0 or 1 = off; otherwise the q block is
                             * additionally multiplied by this factor in fp32 BEFORE its single bf16 rounding (folded into the
                             * RMSNorm weight).  omni_dit_forward passes softmax_scale * log2(e), so that the attention kernel's
                             * QK^T accumulator is the exp2 argument directly (csrc/attention.hip OMNI_ATTN_BAKE) */
  const int32_t* tile_skip; /* nullable DEVICE array, one int32 per 256-row tile of this group: non-zero = the workgroups of
                             * that row tile return at once (its rows belong to items whose block stack is skipped this
                             * forward, omni_teacache).  A device-side predicate: no host round trip.  ABI v3. */
  /* ABI v7 — omni_gemm_params.fp8 only: fp32 dequantisation scales, a_scale[r] of A's STORED row r (the row a_row_map picks,
   * or the logical row) and w_scale[n] of output channel n:  Y = epilogue((A8 . W8^T) * a_scale[r] * w_scale[n] + bias[n]).
   * Both come from omni_quantize_fp8_rows. */
  const float* a_scale;
  const float* w_scale;
} omni_gemm_group;

typedef struct {
  int32_t ngroups; /* 1 or 2 */
  int32_t N, K;
  int32_t epilogue; /* omni_epilogue */
  int32_t split_n;  /* SPLIT3: width of each output (multiple of 32) */
  int32_t w_k32_blocked; /* 0: W is [N, K] row-major (the reference's nn.Linear.weight).  1: W is the SAME values in
                          * K32-blocked order [K/32][N][32] (element (n,k) at ((k/32)*N + n)*32 + k%32): a 32-wide k-slab of
                          * 16 consecutive rows is then 1 KiB contiguous, so every LDS-DMA piece of the weight operand
                          * fetches whole 128-B lines instead of 16 half lines (the L1 request-slot limit).
                          * A one-time re-layout at weight-load time; occupies the struct's former padding. */
  omni_gemm_group g[2];
  /* ABI v4 — optional split-K workspace (DEVICE, 16-byte aligned, caller-owned; NULL = never split).  When the launch has so
   * few tiles that at least half of the CUs would idle (<= 128 tiles in <= 10 row tiles: a forward over one or two small images
   * streams its N = 3072 weight panels through 36 workgroups), the K loop is split s ways (s <= 8), the fp32 partial tiles go to
   * splitk_ws[s][M0 + M1][N] and a second kernel sums them in split order and runs the epilogue.  Needs
   * s * (M0 + M1) * N <= splitk_ws_floats; results agree with the unsplit kernel to fp32 summation order
   * (ABI v12: OMNI_GEMM_KERNEL_SPLITK_IN_LAUNCH below moves the reduction into the launch.) */
  float* splitk_ws;
  int64_t splitk_ws_floats;
  /* ABI v6 — kernel choice, normally 0 = automatic (the ping-pong kernel where its preconditions hold, else the ring kernel).
   * OMNI_GEMM_KERNEL_RING forces the ring kernel (the fallback family): the two accumulate every output element in the same
   * k order and must agree bit for bit, which is how callers (and tests/) cross-check one against the other.  Values
   * >= 16 select development families and are honoured only by libraries built with -DOMNI_DEV; the product library ignores
   * them.  The library itself has no switches: no environment variable and no process-global setter changes what a call does. */
  int32_t kernel_hint;
  /* ABI v7 — fp8 = 1: A and W hold OCP fp8 e4m3 values (one byte each) instead of bf16, in the K64-blocked order
   * [K/64][rows][64] (what omni_quantize_fp8_rows writes; a_k32_rows / w_k32_blocked then carry the row counts R / 1 as for
   * bf16 — byte for byte it is the K32-blocked layout of a bf16 matrix with K/2 columns), with per-row / per-output-channel
   * fp32 scales in omni_gemm_group.a_scale / w_scale.  K counts fp8 elements and must be a multiple of 128.  The products run
   * on v_mfma_scale_f32_16x16x128_f8f6f4 (twice the bf16 MFMA rate; block scales fixed at 1, the fp32 scales are applied
   * to the fp32 accumulators in the epilogue).  No split-K.  Outputs, bias and every epilogue stay bf16 as without it. */
  int32_t fp8;
} omni_gemm_params;
#define OMNI_GEMM_KERNEL_AUTO 0
#define OMNI_GEMM_KERNEL_RING 1
/* ABI v10 — automatic kernel choice, and the split-K rule above without its "<= 10 row tiles" clause: for a TALL launch with a
 * long K and few tiles (the VAE mid-block attention's P.V: 8192 x 384 x 16384 = 64 tiles).  The clause exists so that a batch
 * and its shards take the same decision; a caller that passes this vouches that nothing compares the result across batch
 * compositions bit for bit. */
#define OMNI_GEMM_KERNEL_SPLITK_TALL 2
/* ABI v11 — TAIL SPLIT (automatic with a split-K workspace, this hint turns it off).  A launch of more than one round of 256x256
 * tiles whose last round is thin (tiles % CUs at most a quarter of the CUs: 1548 tiles on 256 CUs = 6 rounds + 12 tiles, the
 * N = 3072 GEMMs of one 2048x2048 request) runs the tiles of the full rounds unsplit — bit-identical to a launch without workspace — and splits the K
 * loop of the remaining tiles s ways (s = 4 or 8: 12 / 24 K-tiles per piece; fp32 partials splitk_ws[tail tile][s][256][256] as far
 * as splitk_ws_floats allows — up to 64 x 8 x 65536 floats — a small second kernel runs their epilogue), so the partial round
 * costs its share of the work instead of a whole tile time.  The tail tiles then agree with the unsplit
 * kernel to fp32 summation order; WHICH tiles are tail tiles depends on the launch's tile count, i.e. on the batch composition —
 * a caller that compares results bit for bit across batch compositions passes OMNI_GEMM_KERNEL_NO_TAIL_SPLIT (or no workspace). */
#define OMNI_GEMM_KERNEL_NO_TAIL_SPLIT 3
/* ABI v12 — split-K (the ABI v4 rule) with the reduction INSIDE the launch, opt-in: needs 512 floats behind the partials
 * (s * (M0 + M1) * N + 512 <= splitk_ws_floats) and the grid 8 * ceil(tiles / 8) * s within one round of the CUs, else the
 * two-kernel path runs.  The s workgroups of a tile (all resident at once, placed on one XCD) publish their fp32 partials
 * write-through, meet at an arrival counter and each runs the epilogue for its share of the tile's rows — no second kernel, the
 * same bits (the sum is formed in split order by the same code).  The last 512 words of the workspace hold the counters: the
 * call zeroes them on the stream before its launch and the launch leaves them zero; a wait that cannot complete (a device
 * whose usable CUs are fewer than it reports) gives up after about a second, sets word 256 and returns wrong rows rather than
 * hanging the device.  Measured on MI355X it pays only for 2-way splits on grids that nearly fill the chip (+1.1 .. 1.3 % per
 * forward) and loses for deep splits: not the default. */
#define OMNI_GEMM_KERNEL_SPLITK_IN_LAUNCH 4
/* ABI v13 — split-K (the ABI v4 rule) WITHOUT its finish kernel: the call launches only the K-split main kernel and leaves the
 * fp32 partials splitk_ws[s][M0 + M1][N] (group 1's rows behind group 0's; no bias, no epilogue applied) for a consumer that
 * folds the reduction into its own pass — omni_splitk_finish_adaln_pair below for OMNI_EPI_BIAS_GATE_RES.  The caller asks
 * omni_gemm_splitk_factor first: the hint is valid only for a call whose factor is > 1 (anything else returns
 * OMNI_ERR_UNSUPPORTED — the library never silently runs a different path).  The output / residual / gate / bias fields of the
 * groups are not touched by such a call. */
#define OMNI_GEMM_KERNEL_SPLITK_DEFER_FINISH 5

int omni_gemm_bf16(const omni_gemm_params* p, omni_stream stream);
/* ABI v13 — the whole-launch split-K factor omni_gemm_bf16 would use for `p` on the current device (a function of the tile counts,
 * K and the workspace size only): 1 = the call does not split, 0 = `p` is not a valid call. */
int omni_gemm_splitk_factor(const omni_gemm_params* p);

/* ABI v7 — dynamic per-row fp8 (OCP e4m3) quantisation of a bf16 matrix for omni_gemm_params.fp8:
 *   scale[r] = max(amax_k |x[r, k]|, tiny) / 448;   y8[r, k] = e4m3_rn(x[r, k] / scale[r])
 * x: [rows, K] bf16, row-major with stride ldx, or K32-blocked [K/32][x_k32_rows][32] when x_k32_rows > 0 (ldx ignored).
 * y8: K64-blocked bytes [K/64][y_rows][64] (y_rows >= rows: the row count of the buffer, = omni_gemm_group.a_k32_rows of
 * the consuming GEMM); scale: fp32 [rows].  K % 64 == 0, K <= 16384.  One wave per row, the row held in registers: x is
 * read once (2 B/element) and y8 written once (1 B/element): HBM-bound.  Used for activations (per token) and, once at
 * load time, for weights (per output channel).  (vLLM's dynamic per-token fp8 recipe; the reference has no fp8 path —
 * BASELINE.json config 5 asks for one.) */
int omni_quantize_fp8_rows(const omni_bf16* x, int64_t ldx, int32_t x_k32_rows, int32_t rows, int32_t K, uint8_t* y8,
                           int32_t y_rows, float* scale, omni_stream stream);

/* ------------------------------------------------------------------------------------------------
 * AdaLN-modulate:  y = LayerNorm(x; eps, no affine) * (1 + scale[item]) + shift[item]
 * Replaces AdaLayerNorm.forward_hip -> forward_native, vllm_omni/diffusion/layers/adalayernorm.py:70-76,94-102
 * (nn.LayerNorm + mul + add = 3 passes -> 1), and the LayerNorm half of diffusers
 * AdaLayerNormContinuous (call site qwen_image_transformer.py:797).
 * x,y [rows, D] bf16 (row strides ldx/ldy); scale/shift bf16 vectors of length D per item with
 * stride mod_item_stride; item(row) = row_item_map ? row_item_map[row] : row / rows_per_item.
 * D % 8 == 0 and D <= 8192.
 * ---------------------------------------------------------------------------------------------- */
int omni_adaln_modulate(const omni_bf16* x, int64_t ldx, omni_bf16* y, int64_t ldy, int32_t rows, int32_t D,
                        const omni_bf16* scale, const omni_bf16* shift, int64_t mod_item_stride,
                        const int32_t* row_item_map, int32_t rows_per_item, float eps, omni_stream stream);
/* Same, with the output optionally K32-blocked: y_k32_rows = 0 -> row-major (ldy); R > 0 -> y is [D/32][R][32]
 * (omni_gemm_group.a_k32_rows of the GEMM that consumes it; D % 32 == 0; ldy ignored). */
int omni_adaln_modulate_ex(const omni_bf16* x, int64_t ldx, omni_bf16* y, int64_t ldy, int32_t rows, int32_t D,
                           const omni_bf16* scale, const omni_bf16* shift, int64_t mod_item_stride,
                           const int32_t* row_item_map, int32_t rows_per_item, float eps, int32_t y_k32_rows,
                           omni_stream stream);

/* ABI v7 — AdaLN-modulate with the result quantised to fp8 in the same pass (the row is in registers anyway):
 * y8 / y8_scale as omni_quantize_fp8_rows would produce them from the bf16-ROUNDED result (bit-identical to running the two
 * kernels one after the other), K64-blocked with y8_rows rows.  y (nullable): additionally the bf16 result, K32-blocked with
 * y_k32_rows rows (TeaCache reads the modulated input of the first block).  D % 64 == 0. */
int omni_adaln_modulate_fp8(const omni_bf16* x, int64_t ldx, int32_t rows, int32_t D, const omni_bf16* scale,
                            const omni_bf16* shift, int64_t mod_item_stride, const int32_t* row_item_map,
                            int32_t rows_per_item, float eps, omni_bf16* y, int32_t y_k32_rows, uint8_t* y8,
                            int32_t y8_rows, float* y8_scale, omni_stream stream);

/* ABI v12 — AdaLN-modulate of TWO row groups in ONE launch: the image stream's rows and the text stream's rows of a DiT block
 * (reference qwen_image_transformer.py:564-567 and :590,:595 run `img_norm1` / `txt_norm1`, `img_norm2` / `txt_norm2` back to
 * back).  Each group is what omni_adaln_modulate_ex / omni_adaln_modulate_fp8 take for one call — x row-major [rows, D] with
 * row stride D; y (nullable when y8 is given) row-major with row stride D, or K32-blocked with y_k32_rows rows; y8 / y8_scale
 * (nullable pair) the fp8 copy, K64-blocked with y8_rows rows — and gets the same bits; D, eps and the modulation stride are
 * shared.  At small batches (one 256x256 CFG pair: 512 + 128 rows) the two launches are latency, not bandwidth. */
typedef struct omni_adaln_stream {
  const omni_bf16* x;
  omni_bf16* y;
  int32_t rows;
  const omni_bf16* scale;
  const omni_bf16* shift;
  const int32_t* row_item_map;
  int32_t rows_per_item;
  int32_t y_k32_rows;
  uint8_t* y8;
  int32_t y8_rows;
  float* y8_scale;
} omni_adaln_stream;
int omni_adaln_modulate_pair(const omni_adaln_stream* a, const omni_adaln_stream* b, int32_t D, int64_t mod_item_stride,
                             float eps, omni_stream stream);

/* ABI v13 — the finish of a DEFERRED split-K GEMM with the gated-residual epilogue (omni_gemm_bf16 with
 * OMNI_GEMM_KERNEL_SPLITK_DEFER_FINISH, epilogue OMNI_EPI_BIAS_GATE_RES, N = D) fused with the AdaLN-modulate that follows it in a
 * DiT block: the attention output projection -> norm2 (qwen_image_transformer.py:586-590,595) and the MLP down projection -> the
 * NEXT block's norm1 (:592,597 -> :564-567).  One wave per row, both streams of the block in ONE launch:
 *   c      = bf16(sum_s partial[s][row] + bias)                  (split order, the finish kernel's arithmetic)
 *   hidden = bf16(hidden + gate[item(row)] * c)                  (written back in place: the residual stream)
 *   y      = bf16(LN(hidden) * (1 + scale[item]) + shift[item])   (omni_adaln_modulate_ex's arithmetic on the rounded row)
 * — the same bits as the finish kernel followed by omni_adaln_modulate_pair, without the second pass over the residual stream,
 * two of the three launches and their boundaries (at one 256x256 CFG pair the three are latency, not bandwidth).
 * Per stream: `rows` rows, `ws_row0` = its first row inside the partials' M0 + M1 rows; hidden row-major [rows, D] (row stride D);
 * y row-major (row stride D) or K32-blocked with y_k32_rows rows; gate / scale / shift rows of mod_item_stride elements indexed by
 * row_item_map[row] (or row / rows_per_item).  nsplit in {2, 3, 4, 6, 8}; D % 8 == 0, D <= 4096. */
typedef struct omni_finish_adaln_stream {
  int32_t rows;
  int32_t ws_row0;
  const omni_bf16* bias; /* [D], nullable */
  omni_bf16* hidden;
  const omni_bf16* gate;
  const omni_bf16* scale;
  const omni_bf16* shift;
  const int32_t* row_item_map;
  int32_t rows_per_item;
  omni_bf16* y;
  int32_t y_k32_rows;
} omni_finish_adaln_stream;
int omni_splitk_finish_adaln_pair(const float* splitk_ws, int32_t nsplit, int64_t ws_rows, const omni_finish_adaln_stream* a,
                                  const omni_finish_adaln_stream* b, int32_t D, int64_t mod_item_stride, float eps,
                                  omni_stream stream);

/* RMSNorm over the last dim with learned weight: y = x * rsqrt(mean(x^2) + eps) * w.
 * Replaces vllm RMSNorm at qwen_image_transformer.py:758 (txt_norm, D = 3584).  D % 8 == 0, D <= 8192. */
int omni_rmsnorm(const omni_bf16* x, int64_t ldx, omni_bf16* y, int64_t ldy, int32_t rows, int32_t D,
                 const omni_bf16* weight, float eps, omni_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Per-head RMSNorm (head_dim 128, learned weight) + interleaved RoPE, in place on a [rows, H*128] tensor.
 * Replaces qwen_image_transformer.py:397-400 (vllm RMSNorm on q,k) and :403-410
 * (RotaryEmbedding(is_neox_style=False), vllm_omni/diffusion/layers/rope.py:12-36,108-127):
 *   xn = x * rsqrt(mean_128(x^2) + eps) * w[stream(row)]
 *   out[2i] = xn[2i]*cos[p,i] - xn[2i+1]*sin[p,i] ; out[2i+1] = xn[2i+1]*cos[p,i] + xn[2i]*sin[p,i]
 * cos/sin: bf16 tables [npos, 64] (the reference casts them to the activation dtype first, :403-406).
 * row_pos[row] (int32) = table row; weight = w_txt if row_pos[row] < txt_pos_end else w_img.
 * ---------------------------------------------------------------------------------------------- */
int omni_qk_norm_rope(omni_bf16* x, int64_t ldx, int32_t rows, int32_t num_heads,
                      const omni_bf16* w_img, const omni_bf16* w_txt, const omni_bf16* cos_tab,
                      const omni_bf16* sin_tab, const int32_t* row_pos, int32_t txt_pos_end, float eps,
                      omni_stream stream);

/* Standalone interleaved RoPE on [B, S, H, dh] (the RotaryEmbedding.forward_hip plug-in point,
 * vllm_omni/diffusion/layers/rope.py:108-127).  cos/sin bf16 [S, dh/2]; x -> y (may alias). dh % 16 == 0. */
int omni_rope_interleaved(const omni_bf16* x, omni_bf16* y, int32_t B, int32_t S, int32_t H, int32_t dh,
                          const omni_bf16* cos_tab, const omni_bf16* sin_tab, omni_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Flash attention forward, non-causal, no mask, head_dim 128, bf16 in/out, fp32 softmax/accumulate.
 * Replaces F.scaled_dot_product_attention at vllm_omni/diffusion/attention/backends/sdpa.py:46-66
 * (and flash_attn_func in the flash_attn sibling backend; the int8 `sageattn` of sage_attn.py is omni_attn_params.qk_int8).
 * q,k,v,out: [total_rows, H*128] with row strides ld* (the reference's [B,S,H,dh] "NHD" layout
 * flattened over B,S); item b owns rows [cu_seqlens[b], cu_seqlens[b+1]).  cu_seqlens is a
 * DEVICE int32 array of B+1 entries.  max_seqlen bounds the grid.
 * ---------------------------------------------------------------------------------------------- */
int omni_flash_attn_fwd(const omni_bf16* q, const omni_bf16* k, const omni_bf16* v, omni_bf16* out,
                        int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, const int32_t* cu_seqlens,
                        int32_t B, int32_t H, int32_t head_dim, int32_t max_seqlen, float softmax_scale,
                        omni_stream stream);
/* Same, with the output optionally K32-blocked: out_k32_rows = R > 0 -> out is [H*128/32][R][32] over the R rows of the
 * whole buffer (ldo ignored); 0 -> row-major. */
int omni_flash_attn_fwd_ex(const omni_bf16* q, const omni_bf16* k, const omni_bf16* v, omni_bf16* out,
                        int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, const int32_t* cu_seqlens,
                        int32_t B, int32_t H, int32_t head_dim, int32_t max_seqlen, float softmax_scale,
                        int32_t out_k32_rows, omni_stream stream);

/* ABI v11 — the same with an optional caller-owned fp32 DEVICE workspace (16-byte aligned, omni_flash_attn_workspace_bytes(B, H)
 * bytes; NULL = omni_flash_attn_fwd_ex).  With it, a grid whose per-item LAST 256-query block is short (<= 64 rows: 4160 = 16 x 256 +
 * 64 joint rows at 1024^2, 16448 = 64 x 256 + 64 at 2048^2) and would open a thin extra round of workgroups (one 2048^2 request:
 * 48 x 65 = 3120 workgroups = 12 rounds of 256 CUs + 48) splits that block's KEY range over s workgroups (s <= 8, picked from a
 * makespan model), which leave un-normalised fp32 partials (O, running max, row sum) in the workspace; a second small kernel merges
 * them (flash-decoding style).  Results agree with the unsplit kernel to fp32 summation order on those rows, bit for bit elsewhere. */
size_t omni_flash_attn_workspace_bytes(int32_t B, int32_t H);
int omni_flash_attn_fwd_ws(const omni_bf16* q, const omni_bf16* k, const omni_bf16* v, omni_bf16* out,
                           int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, const int32_t* cu_seqlens,
                           int32_t B, int32_t H, int32_t head_dim, int32_t max_seqlen, float softmax_scale,
                           int32_t out_k32_rows, void* workspace, size_t workspace_bytes, omni_stream stream);

/* ABI v11 — the attention of the WHOLE plug-in point: everything `SDPAImpl.forward` hands to
 * F.scaled_dot_product_attention (vllm_omni/diffusion/attention/backends/sdpa.py:46-66; the backend selector is process-global,
 * attention/selector.py:49-77, so a registered backend also serves the other in-tree DiTs) beyond the self-attention above:
 * separate query / key sequences (cross-attention, wan2_2_transformer.py:243,340), head size 64 or 128 (sd3_transformer.py:108),
 * an attention mask, is_causal, grouped K / V heads.
 *   q, out: [total_q_rows, H * dh]; k, v: [total_k_rows, H_kv * dh]; item b owns query rows [cu_seqlens_q[b], cu_seqlens_q[b+1])
 *   and key rows [cu_seqlens_k[b], cu_seqlens_k[b+1]) (DEVICE int32 arrays of B + 1 entries; the two may be the same array).
 *   mask (nullable, mask_type 0): element (b, h, i, j) at mask[b * mask_stride_b + h * mask_stride_h + i * mask_stride_q +
 *   j * mask_stride_k] with strides in ELEMENTS, 0 = broadcast (what `mask.expand(B, H, S_q, S_k).stride()` returns);
 *   mask_type 1: one byte per element, non-zero = attend (torch.bool); 2: bf16 added to the scaled scores; 3: fp32 added.
 *   causal = 1: key j takes part in query i only if j <= i (torch's is_causal: aligned to the top-left corner).
 *   out = softmax(scale * q k^T + mask) v per (item, head), fp32 softmax; rows with no key to attend to produce zeros.
 * head_dim 64 or 128 (OMNI_ERR_UNSUPPORTED otherwise); H % H_kv == 0.
 *   elem_type (needs OMNI_FEATURE_ATTN_F16): OMNI_ELEM_BF16 (0) — q, k, v and out are bf16, as in every other entry point;
 *   OMNI_ELEM_F16 (1) — q, k, v and out are ALL IEEE fp16 bit patterns: both products run on the fp16 MFMA, P and the output
 *   are rounded to fp16 (nearest even), the softmax stays fp32.  The mask does not follow: mask_type 2 still means bf16 (hand
 *   an fp16 additive mask over as fp32).  qk_int8 = 1 with fp16 is OMNI_ERR_UNSUPPORTED; any other elem_type value is
 *   OMNI_ERR_BAD_ARG.  The field occupies what used to be padding behind mask_type — size and every other offset are
 *   unchanged — so callers MUST zero the whole struct (memset / `= {0}` / `= {}`) before filling it in; a caller that never
 *   heard of the field then asks for bf16. */
#define OMNI_ELEM_BF16 0
#define OMNI_ELEM_F16 1
typedef struct {
  const omni_bf16 *q, *k, *v;
  omni_bf16* out;
  int64_t ldq, ldk, ldv, ldo;          /* row strides in elements (multiples of 8; ldo of 4) */
  const int32_t* cu_seqlens_q;
  const int32_t* cu_seqlens_k;
  int32_t B, H, H_kv, head_dim;
  int32_t max_seqlen_q, max_seqlen_k;  /* bounds of the per-item lengths (max_seqlen_q sizes the grid) */
  float softmax_scale;
  int32_t causal;
  const void* mask;
  int32_t mask_type;                   /* 0 none, 1 bool bytes, 2 bf16 additive, 3 fp32 additive */
  int32_t elem_type;                   /* OMNI_ELEM_BF16 / OMNI_ELEM_F16: type of q, k, v, out (sits in former padding) */
  int64_t mask_stride_b, mask_stride_h, mask_stride_q, mask_stride_k;
  /* ABI v14 — appended; all zero = the bf16 kernel above, bit for bit.
   * qk_int8 = 1: SAGE_ATTN (the reference's sage_attn.py backend, SageAttention v1: int8 Q K^T, fp32 softmax, bf16 P V), per item
   * and head: km = mean of the item's key rows (fp32); k' = k - km (softmax unchanged); q *= softmax_scale * log2(e); per block
   * of 64 rows from the item's first row, q and k' are quantised to int8 with scale amax|x| / 127 (all-zero block: 1), round to
   * nearest even; s = float(q8 . k8^T) * sq * sk; exp2-domain online softmax in fp32; P rounded to bf16; bf16 P V with an fp32
   * accumulator.  No mask, not causal (OMNI_ERR_UNSUPPORTED), head_dim 64 or 128; `workspace` (16-byte aligned DEVICE memory of
   * at least omni_attn_quant_workspace_bytes(p) bytes) receives the int8 q / k, the block scales and the key means
   * (OMNI_ERR_BAD_ARG when missing or short).  out_k32_rows = R > 0 (qk_int8 only): out is K32-blocked [H * dh / 32][R][32]
   * over the R rows of the whole buffer (ldo ignored), as omni_flash_attn_fwd_ex; R must cover cu_seqlens_q[B] (query rows at or
   * past R are not written).  item_skip (nullable DEVICE int32 [B], qk_int8 only): item b with item_skip[b] != 0 costs nothing
   * and its output rows are left untouched (the TeaCache predicate of omni_dit_forward). */
  int32_t qk_int8;
  int32_t out_k32_rows;
  void* workspace;
  size_t workspace_bytes;
  const int32_t* item_skip;
} omni_attn_params;
int omni_flash_attn_general(const omni_attn_params* p, omni_stream stream);
/* ABI v14 — bytes of the qk_int8 workspace for these bounds (B, H, H_kv, head_dim, max_seqlen_q, max_seqlen_k); 0 for
 * parameters qk_int8 does not take. */
size_t omni_attn_quant_workspace_bytes(const omni_attn_params* p);

/* ------------------------------------------------------------------------------------------------
 * Small-batch weight-streaming linear:  y[b, n] = act_out( sum_k act_in(x[b, k]) * W[n, k] + bias[n] ).
 * Replaces the GEMVs at qwen_image_transformer.py:51-52 (TimestepEmbedding), :552,557
 * (img_mod / txt_mod = SiLU -> Linear(D -> 6D), 13.6 GB of weights per forward) and the Linear inside
 * AdaLayerNormContinuous (:797).  HBM-bound: W is read exactly once.  B <= 8, K % 8 == 0, K <= 4096.
 * act codes: 0 none, 1 SiLU.
 * ---------------------------------------------------------------------------------------------- */
int omni_linear_smallbatch(const omni_bf16* x, int64_t ldx, int32_t B, const omni_bf16* W, const omni_bf16* bias,
                           int64_t N, int32_t K, omni_bf16* y, int64_t ldy, int32_t act_in, int32_t act_out,
                           omni_stream stream);

/* Sinusoidal timestep projection, diffusers Timesteps(256, flip_sin_to_cos=True, shift 0, scale 1000)
 * (qwen_image_transformer.py:44,51; body in-tree at pipeline_qwen_image.py:135-184): out[b] = [cos | sin]. */
int omni_timestep_sinusoid(const float* t, int32_t B, int32_t dim, float scale, omni_bf16* out, omni_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Step epilogue: true-CFG combine + norm rescale + Flow-Match Euler update, fused.
 * Replaces pipeline_qwen_image.py:580-583 and scheduler.step at :585:
 *   comb = neg + s*(pos - neg); pred = comb * (||pos|| / ||comb||)   (norms over the last dim C)
 *   latents <- bf16( float(latents) + dt * pred )            (neg == NULL: pred = pos)
 * pos/neg/latents: [rows, C] bf16 contiguous, C == 64.  dt = sigma_next - sigma (per-row item via dt_item
 * when dt_rows_per_item > 0: dt[row / dt_rows_per_item], else dt[0]).  dt is a DEVICE fp32 array.
 * ---------------------------------------------------------------------------------------------- */
int omni_cfg_euler_step(const omni_bf16* pos, const omni_bf16* neg, omni_bf16* latents, int32_t rows, int32_t C,
                        float true_cfg_scale, const float* dt, int32_t dt_rows_per_item, omni_stream stream);
/* ABI v9 — same with the norm rescale optional: normalize = 0 -> pred = comb (the Layered pipeline's default,
 * pipeline_qwen_image_layered.py:599-605 `cfg_normalize`); normalize = 1 == omni_cfg_euler_step. */
int omni_cfg_euler_step_ex(const omni_bf16* pos, const omni_bf16* neg, omni_bf16* latents, int32_t rows, int32_t C,
                           float true_cfg_scale, const float* dt, int32_t dt_rows_per_item, int32_t normalize,
                           omni_stream stream);

/* The same update for R <= 64 requests of DIFFERENT row counts in ONE launch, reading the predictions where a ragged forward
 * wrote them and writing the new rows into the forward's input buffer as well (optional symbol of ABI v14: ask
 * omni_features() & OMNI_FEATURE_CFG_EULER_RAGGED).  Request r is described by reqs[r], an array in DEVICE memory:
 *   lat_row            first of its `rows` rows in `latents`  [n_lat_rows, C]   (updated in place)
 *   pos_row, neg_row   first row of its positive / negative prediction in `pred` [n_pred_rows, C]: the request's first `rows`
 *                      rows of an item that may hold further (condition-image) rows behind them; neg_row < 0: no CFG
 *   dst_row[0..1]      first rows in `lat_in` [n_in_rows, C] that receive a copy of the updated rows (the next forward's input
 *                      rows of the positive and the negative item); < 0: none.  No other row of `lat_in` is touched
 *   dt_index           its entry of the DEVICE fp32 array dt[n_dt];  cfg_scale: its true-CFG scale
 * Arithmetic per row: omni_cfg_euler_step_ex's, bit for bit.  total_rows = the sum of reqs[r].rows (sizes the launch: rows
 * behind it are not updated; a larger value is harmless).  The row ranges of different requests must not overlap.  The device
 * descriptors cannot be validated by the host: the kernel skips a request whose ranges leave [0, n_*_rows) or [0, n_dt), so
 * nothing outside the three buffers is read or written.  C == 64 and R <= 64, else OMNI_ERR_UNSUPPORTED; pred / latents /
 * lat_in 16-byte aligned, reqs / dt 4-byte aligned, else OMNI_ERR_ALIGN. */
typedef struct omni_cfg_euler_req {
  int32_t lat_row, rows, pos_row, neg_row;
  int32_t dst_row[2];
  int32_t dt_index;
  float cfg_scale;
} omni_cfg_euler_req; /* 32 bytes */
/* Exported as a const function POINTER, not as a function: the set of exported functions identifies ABI v14 and stays what
 * it was, so an entry point added within the version is a data symbol.  C callers call it with the syntax of
 * a function call; a dlsym / ctypes caller reads the pointer and calls its target. */
extern int (*const omni_cfg_euler_step_ragged)(const omni_bf16* pred, int32_t n_pred_rows, omni_bf16* latents,
                                               int32_t n_lat_rows, omni_bf16* lat_in, int32_t n_in_rows,
                                               const omni_cfg_euler_req* reqs, int32_t R, int32_t total_rows, int32_t C,
                                               const float* dt, int32_t n_dt, int32_t normalize, omni_stream stream);

/* ------------------------------------------------------------------------------------------------
 * LoRA merge: one row range of one weight matrix receives its low-rank update, on the device (optional symbol of ABI v14:
 * ask omni_features() & OMNI_FEATURE_LORA_MERGE).  The reference has no implementation to mirror (only the config fields,
 * data.py:280-286); this is the usual definition:
 *   W_out[n, k] = bf16_rne( float(W_base[n, k]) + scale * sum_{r < R} float(up[n - row0, r]) * float(down[r, k]) )
 * for n in [row0, row0 + rows); rows outside the range are neither read nor written.  fp32 accumulation on the matrix cores,
 * `scale` applied in fp32 after the sum, ONE rounding to bf16; scale == 0 copies the base bits.  W_out may be W_base (each
 * element is read once and written once by the same lane); any other overlap of the two is undefined.
 *   W     [N, K]: row-major with row pitch ldw (elements), or - w_k32_blocked = 1, the layout of omni_gemm_params.w_k32_blocked -
 *         K32-blocked [K/32][N][32] (ldw ignored).  W_base and W_out share layout and pitch.
 *   up    [rows, R] bf16 row-major, dense (lora_B / lora_up rows of the range);  down [R, K] bf16 row-major, dense (lora_A).
 * Any R in 1..256 (the rank tail is masked inside the kernel), any row0 / rows inside [0, N).
 * Status, before any launch: null pointer, N / K < 1, rows < 1, a range that leaves [0, N), ldw < K -> OMNI_ERR_BAD_ARG;
 * K % 32 != 0, R < 1, R > 256 -> OMNI_ERR_UNSUPPORTED; a pointer not 16-byte aligned, ldw % 8 != 0 -> OMNI_ERR_ALIGN. */
typedef struct omni_lora_merge_params {
  const omni_bf16* w_base;
  omni_bf16* w_out;
  const omni_bf16* up;
  const omni_bf16* down;
  int32_t N, K, R;
  int32_t row0, rows;
  int32_t w_k32_blocked;
  int64_t ldw;
  float scale;
} omni_lora_merge_params;
/* a const function POINTER like omni_cfg_euler_step_ragged, for the same reason */
extern int (*const omni_lora_merge)(const omni_lora_merge_params* p, omni_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Prompt encoder: the Qwen2.5-VL TEXT model (HF transformers `Qwen2_5_VLTextModel`, 28 decoder layers at hidden 3584 / 28 query
 * heads over 4 K/V heads / intermediate 18944) as one native call (optional symbols of ABI v14: ask
 * omni_features() & OMNI_FEATURE_TEXT_ENCODER).  Replaces the HF eager pass behind `_get_qwen_prompt_embeds`
 * (vllm_omni/diffusion/models/qwen_image/pipeline_qwen_image.py:351-392) for prompts WITHOUT pictures: their three M-RoPE position
 * rows are equal, so the rotary embedding is plain rotate-half RoPE at one position per token.
 * Per layer: RMSNorm -> fused q|k|v GEMM (+ bias) -> RoPE on q, k -> causal attention with grouped K/V heads -> o_proj + residual
 * -> RMSNorm -> fused gate|up GEMM -> silu(gate) * up -> down_proj + residual; after the last layer the final RMSNorm (HF's
 * `hidden_states[-1]` is post-norm).  Runs over the PACKED valid tokens of all prompts: no pad rows.
 * ---------------------------------------------------------------------------------------------- */
typedef struct omni_text_layer_weights {
  const omni_bf16* input_norm_w; /* [D] */
  const omni_bf16* qkv_w;        /* [(H + 2 H_kv) * 128, D]: rows of q_proj | k_proj | v_proj */
  const omni_bf16* qkv_b;        /* [(H + 2 H_kv) * 128] */
  const omni_bf16* o_w;          /* [D, H * 128], no bias */
  const omni_bf16* post_norm_w;  /* [D] */
  const omni_bf16* gate_up_w;    /* [2 I, D]: rows of gate_proj | up_proj, no bias */
  const omni_bf16* down_w;       /* [D, I], no bias */
} omni_text_layer_weights;

typedef struct omni_text_weights {
  int32_t num_layers, hidden_size, num_heads, num_kv_heads, head_dim, intermediate_size, vocab_size;
  int32_t gemm_w_k32_blocked;    /* 1: qkv_w, o_w, gate_up_w, down_w of every layer are stored K32-blocked
                                  * (omni_gemm_params.w_k32_blocked); everything else is always row-major */
  float rms_norm_eps;
  int32_t rope_npos;             /* rows of the RoPE tables */
  const omni_bf16* embed_tokens; /* [vocab_size, D] */
  const omni_bf16* final_norm_w; /* [D] */
  const omni_bf16* ones;         /* [D] bf16 1.0: the gate of the residual adds (OMNI_EPI_BIAS_GATE_RES with gate 1 is exact) */
  const float* rope_cos;         /* [rope_npos, 64] fp32: cos(p * theta^(-i / 64)), built once on the host from rope_theta */
  const float* rope_sin;
  const omni_text_layer_weights* layers; /* HOST array [num_layers] of device pointers */
} omni_text_weights;

typedef struct omni_text_batch {
  int32_t n_prompts, total_rows; /* prompts (<= 64) and the sum of their token counts */
  int32_t max_seqlen;            /* at least the longest prompt's token count (sizes the attention grid) */
  int32_t reserved;              /* 0 */
  const int32_t* input_ids;      /* [total_rows] token ids, prompt after prompt */
  const int32_t* cu_seqlens;     /* [n_prompts + 1] prefix sums of the token counts */
  const int32_t* row_pos;        /* [total_rows] position of each token inside its prompt = RoPE table row */
  omni_bf16* out;                /* [total_rows, D] the last hidden state (after the final norm) */
  void* workspace;               /* DEVICE, 16-byte aligned, as many bytes as omni_qwen2_text_workspace_bytes answers for
                                  * (w, total_rows); its first 256 bytes hold the error word below: ZERO them once when the
                                  * buffer is allocated */
  size_t workspace_bytes;
} omni_text_batch;
/* const function POINTERS like omni_lora_merge, for the same reason.
 * omni_qwen2_text_forward: one call enqueues the whole forward on `stream`; no allocation.  Status before any launch: null
 * pointer, non-positive count, short workspace -> OMNI_ERR_BAD_ARG; head_dim != 128, hidden_size or intermediate_size not a
 * multiple of 64, hidden_size > 8192, num_heads % num_kv_heads != 0, more than 64 prompts -> OMNI_ERR_UNSUPPORTED.
 * Device-side errors: a token id outside [0, vocab_size) yields a ZERO embedding row (never an out-of-range read), a position
 * outside [0, rope_npos) is clamped; either sets the error word at the front of the workspace, which the NEXT call over the same
 * workspace reads back (4 bytes, in front of its first launch: the one host read of a call), clears and reports as
 * OMNI_ERR_BAD_ARG without running. */
extern int (*const omni_qwen2_text_forward)(const omni_text_weights* w, const omni_text_batch* b, omni_stream stream);
/* 0 for weights the forward refuses */
extern size_t (*const omni_qwen2_text_workspace_bytes)(const omni_text_weights* w, int32_t total_rows);
/* The three row kernels of the forward on their own (same feature bit).
 * omni_text_rope_neox: rotate-half RoPE in place on the q and k blocks of qkv [rows, ld >= (H + 2 H_kv) * 128]; for pair
 * (i, i + 64) of a head: out[i] = x[i] cos[p, i] - x[i + 64] sin[p, i]; out[i + 64] = x[i + 64] cos[p, i] + x[i] sin[p, i] with
 * p = row_pos[row]; the v block is not touched.
 * err (nullable DEVICE int32): set non-zero when a position had to be clamped into [0, npos). */
extern int (*const omni_text_rope_neox)(omni_bf16* qkv, int64_t ld, int32_t rows, int32_t H, int32_t H_kv, const float* cos_tab,
                                        const float* sin_tab, int32_t npos, const int32_t* row_pos, int32_t* err, omni_stream stream);
/* omni_text_swiglu: y[r, j] = silu(gate_up[r, j]) * gate_up[r, I + j]; y row-major (ldy) or, y_k32_rows = R > 0, K32-blocked
 * [I / 32][R][32] (omni_gemm_group.a_k32_rows of the GEMM that reads it; I % 32 == 0).  I % 8 == 0. */
extern int (*const omni_text_swiglu)(const omni_bf16* gate_up, int64_t ldgu, omni_bf16* y, int64_t ldy, int32_t rows, int32_t I,
                                     int32_t y_k32_rows, omni_stream stream);
/* omni_text_embed_gather: h[r, :] = table[ids[r], :]; an id outside [0, vocab) writes zeros and sets *err (DEVICE int32) to 1. */
extern int (*const omni_text_embed_gather)(const omni_bf16* table, int32_t vocab, int32_t D, const int32_t* ids, int32_t rows,
                                           omni_bf16* h, int64_t ldh, int32_t* err, omni_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Prompts WITH pictures (the Edit pipelines, pipeline_qwen_image_edit.py:352-397 / pipeline_qwen_image_edit_plus.py:274-330): the
 * Qwen2.5-VL vision tower (HF `Qwen2_5_VisionTransformerPretrainedModel`: 32 blocks at hidden 1280 / 16 heads of 80 /
 * intermediate 3420, patch merger to 3584) as one native call, and the text forward with real M-RoPE and the image embeddings
 * in the token rows (optional symbols of ABI v14: ask omni_features() & OMNI_FEATURE_VISION_ENCODER; const function POINTERS
 * like omni_qwen2_text_forward, for the same reason).
 *
 * The tower runs over the packed patch rows of all pictures IN WINDOW ORDER (the host permutes the processor's pixel_values
 * rows by HF's window_index: the patch embedding is row-wise, so that equals HF's reorder behind it).  Per block: RMSNorm ->
 * fused qkv GEMM (+ bias) -> omni_vision_rope_pad -> omni_flash_attn_general (head_dim 128, softmax_scale head_dim^-0.5,
 * non-causal, cu_window or - full_attention - cu_image) -> projection + bias + residual -> RMSNorm -> fused gate|up GEMM
 * (+ bias) -> omni_text_swiglu -> down + bias + residual.  Merger: RMSNorm per patch row -> [rows / 4, 4 D] -> GEMM + bias ->
 * omni_gelu_erf -> GEMM + bias -> [rows / 4, out_hidden_size], still in window order.
 * Zero padding done ONCE by the host, exact: the patch vector (3 * 2 * 14 * 14 = 1176) to patch_k in pixels and patch_w; the
 * projection's K from head_dim to 128 columns per head; the intermediate size to a multiple of 64 in gate_up_w / gate_up_b
 * (rows) and down_w (columns).
 * ---------------------------------------------------------------------------------------------- */
typedef struct omni_vision_layer_weights {
  const omni_bf16* norm1_w;     /* [D] */
  const omni_bf16* qkv_w;       /* [3 * H * head_dim, D]: HF attn.qkv as it is (q | k | v, each H heads of head_dim) */
  const omni_bf16* qkv_b;       /* [3 * H * head_dim] */
  const omni_bf16* proj_w;      /* [D, H * 128]: column h * 128 + j is HF's column h * head_dim + j, zero for j >= head_dim */
  const omni_bf16* proj_b;      /* [D] */
  const omni_bf16* norm2_w;     /* [D] */
  const omni_bf16* gate_up_w;   /* [2 I, D]: rows of gate_proj | up_proj, each zero-padded to I rows */
  const omni_bf16* gate_up_b;   /* [2 I] */
  const omni_bf16* down_w;      /* [D, I]: zero-padded columns */
  const omni_bf16* down_b;      /* [D] */
  int32_t full_attention;       /* 1: this block attends over whole pictures (cu_image), 0: inside windows (cu_window) */
  int32_t reserved;             /* 0 */
} omni_vision_layer_weights;

typedef struct omni_vision_weights {
  int32_t num_layers, hidden_size, num_heads, head_dim; /* head_dim: a multiple of 16, <= 128, num_heads * head_dim = hidden */
  int32_t intermediate_size;    /* I: the PADDED intermediate size, a multiple of 64 */
  int32_t patch_k;              /* the padded patch vector, a multiple of 64 */
  int32_t out_hidden_size;      /* a multiple of 64 */
  int32_t gemm_w_k32_blocked;   /* 1: every GEMM weight (patch_w, qkv_w, proj_w, gate_up_w, down_w, merger_fc1_w, merger_fc2_w) is K32-blocked */
  float rms_norm_eps;
  int32_t reserved;             /* 0 */
  const omni_bf16* patch_w;     /* [D, patch_k]: the Conv3d kernel flattened (no bias) */
  const omni_bf16* ones;        /* [D] bf16 1.0 (the gate of the residual adds) */
  const omni_bf16* merger_norm_w; /* [D] */
  const omni_bf16* merger_fc1_w;  /* [4 D, 4 D] */
  const omni_bf16* merger_fc1_b;  /* [4 D] */
  const omni_bf16* merger_fc2_w;  /* [out_hidden_size, 4 D] */
  const omni_bf16* merger_fc2_b;  /* [out_hidden_size] */
  const omni_vision_layer_weights* layers; /* HOST array [num_layers] */
} omni_vision_weights;

typedef struct omni_vision_batch {
  int32_t rows;                 /* patch rows of all pictures, a multiple of 4 (the 2 x 2 merge units are 4 consecutive rows) */
  int32_t n_windows, n_images;
  int32_t max_window, max_image; /* at least the longest window / picture in rows (they size the attention grids) */
  int32_t reserved;             /* 0 */
  const omni_bf16* pixels;      /* [rows, patch_k] the processor's pixel_values in window order, zero-padded columns */
  const int32_t* cu_window;     /* DEVICE [n_windows + 1] prefix sums of the window lengths (no empty window) */
  const int32_t* cu_image;      /* DEVICE [n_images + 1] prefix sums of the pictures' rows */
  const float* rope_cos;        /* DEVICE [rows, head_dim / 2] fp32, per row: see omni_vision_rope_pad */
  const float* rope_sin;
  omni_bf16* out;               /* [rows / 4, out_hidden_size] */
  void* workspace;              /* DEVICE, 16-byte aligned, as many bytes as omni_qwen2_vision_workspace_bytes answers for (w, rows) */
  size_t workspace_bytes;
} omni_vision_batch;
/* One call enqueues the whole tower on `stream`; no allocation, no host read.  Status before any launch: null pointer,
 * non-positive count, max_window / max_image above rows, num_heads * head_dim != hidden_size, short workspace ->
 * OMNI_ERR_BAD_ARG; head_dim not a multiple of 16 or above 128, hidden_size / intermediate_size / patch_k / out_hidden_size
 * not a multiple of 64, hidden_size > 8192, rows not a multiple of 4 -> OMNI_ERR_UNSUPPORTED; a workspace or output that is
 * not 16-byte aligned -> OMNI_ERR_ALIGN. */
extern int (*const omni_qwen2_vision_forward)(const omni_vision_weights* w, const omni_vision_batch* b, omni_stream stream);
/* 0 for weights the forward refuses */
extern size_t (*const omni_qwen2_vision_workspace_bytes)(const omni_vision_weights* w, int32_t rows);
/* omni_vision_rope_pad: qkv [rows, ld_in >= 3 * H * hd] (the fused GEMM's output: q | k | v, each H heads of hd) ->
 * out [rows, ld_out >= 3 * H * 128]: q | k | v, each H heads of 128 columns.  hd: a multiple of 16, <= 128.  For a q or k head x
 * and the row's tables c = cos[row], s = sin[row] (fp32 [rows, hd / 2], built by the host: HF `apply_rotary_pos_emb_vision`):
 *   y[i] = x[i] c[i] - x[i + hd/2] s[i],  y[i + hd/2] = x[i + hd/2] c[i] + x[i] s[i]   (i < hd / 2; fp32, one rounding to bf16)
 * v is copied bit for bit; columns hd .. 127 of every head are written as zeros, so that attention at head size 128 with
 * softmax_scale hd^-0.5 IS attention at head size hd. */
extern int (*const omni_vision_rope_pad)(const omni_bf16* qkv, int64_t ld_in, omni_bf16* out, int64_t ld_out, int32_t rows,
                                         int32_t H, int32_t hd, const float* cos_tab, const float* sin_tab, omni_stream stream);
/* omni_gelu_erf: y = 0.5 x (1 + erf(x / sqrt 2)) (torch.nn.GELU(), NOT the tanh form of OMNI_EPI_BIAS_GELU_TANH) on [rows, n],
 * n % 8 == 0; y row-major (ldy; y == x with ldy == ldx is in place) or, y_k32_rows = R >= rows, K32-blocked [n / 32][R][32]
 * (n % 32 == 0, y != x). */
extern int (*const omni_gelu_erf)(const omni_bf16* x, int64_t ldx, omni_bf16* y, int64_t ldy, int32_t rows, int32_t n,
                                  int32_t y_k32_rows, omni_stream stream);
/* omni_text_mrope: omni_text_rope_neox with Qwen2.5-VL's three position rows: rotary pair i of a head reads the tables at
 * row_pos3[sec(i)][row], sec(i) = 0 (temporal) for i < s0, 1 (height) for i < s0 + s1, else 2 (width), with
 * mrope_section = {s0, s1, s2}, s0 + s1 + s2 = 64, each a multiple of 8 (else OMNI_ERR_UNSUPPORTED; the checkpoints have
 * 16, 24, 24).  row_pos3: DEVICE [3][rows].  With three equal rows the output equals omni_text_rope_neox's bit for bit. */
extern int (*const omni_text_mrope)(omni_bf16* qkv, int64_t ld, int32_t rows, int32_t H, int32_t H_kv, const float* cos_tab,
                                    const float* sin_tab, int32_t npos, const int32_t* row_pos3, const int32_t* mrope_section,
                                    int32_t* err, omni_stream stream);

typedef struct omni_text_batch_mm {
  int32_t n_prompts, total_rows, max_seqlen, reserved; /* as in omni_text_batch */
  const int32_t* input_ids;
  const int32_t* cu_seqlens;
  const int32_t* row_pos;        /* not read (row_pos3 takes its place); may be null */
  omni_bf16* out;
  void* workspace;               /* as in omni_text_batch, sized by omni_qwen2_text_workspace_bytes */
  size_t workspace_bytes;
  const int32_t* row_pos3;       /* DEVICE [3][total_rows]: temporal, height, width position of every token (HF get_rope_index) */
  const omni_bf16* vision_rows;  /* DEVICE [n_vision_rows, D]: the vision tower's output; null with n_vision_rows = 0 */
  const int32_t* vision_row_of;  /* DEVICE [total_rows]: >= 0: the token row takes vision_rows[that row] instead of its token
                                  * embedding (HF's masked_scatter, with any permutation of the rows folded in); -1: the token
                                  * embedding; null with n_vision_rows = 0 */
  int32_t n_vision_rows;
  int32_t mrope_section[3];      /* see omni_text_mrope */
} omni_text_batch_mm;
/* omni_qwen2_text_forward with the two additions; the same driver, statuses and error word.  A vision_row_of entry outside
 * [-1, n_vision_rows) yields a ZERO row (never a read) and sets the error word.  With n_vision_rows = 0 and three equal position
 * rows the launches and the output are those of omni_qwen2_text_forward, bit for bit. */
extern int (*const omni_qwen2_text_forward_mm)(const omni_text_weights* w, const omni_text_batch_mm* b, omni_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Greedy decode of the Qwen2.5-VL text model with a KV cache: the auto-caption of the Layered pipeline
 * (pipeline_qwen_image_layered.py:495-513: `text_encoder.generate(**inputs, max_new_tokens=512)`), the one place where the
 * Qwen-Image pipelines GENERATE tokens.  Optional symbols of ABI v14: ask omni_features() & OMNI_FEATURE_TEXT_DECODE; const
 * function POINTERS like omni_qwen2_text_forward_mm, for the same reason.  No existing struct changes.
 *
 * A decode step streams every weight once for M = n_seq <= 8 rows: nothing of the 256-row-tile MFMA GEMM fits, so the step
 * runs on three kernels of its own (exported on their own as well):
 *   omni_gemv_bf16            weight-streaming GEMV family, M <= 8 rows
 *   omni_decode_attention     one query row per sequence against the cache, split over key chunks, log-sum-exp combine
 *   omni_text_penalized_argmax  repetition penalty + argmax + EOS test + the bookkeeping of the step
 * ---------------------------------------------------------------------------------------------- */
/* omni_gemv_bf16: out[m, n] = epilogue(sum_k A[m, k] W[n, k] + bias[n]), m < M <= 8, fp32 accumulation.
 * A [M, K] bf16 row-major (lda); W [N, K] bf16 where it already lies: row-major or (w_k32_blocked = 1) K32-blocked
 * [K/32][N][32].  Epilogues: bias (nullable); res (nullable): out = res + bf16(acc + bias) - the product is rounded to bf16,
 * then added, as OMNI_EPI_BIAS_GATE_RES with a gate of ones does (res may alias out); out_f32 (nullable) takes the fp32 value
 * instead of out (no res then).  Exactly one of out / out_f32.  One workgroup = 8 columns x all of K over four waves, whose
 * partial sums meet in LDS (no fp32 round trip through HBM): ceil(N / 8) workgroups, 448 at N = 3584.
 * Status before the launch: null A / W / output, M, N or K < 1, lda < K, ldo < N -> OMNI_ERR_BAD_ARG; M > 8, K % 32 != 0, both
 * outputs, out_f32 with res -> OMNI_ERR_UNSUPPORTED; A or W not 16-byte aligned, lda % 8 != 0 -> OMNI_ERR_ALIGN. */
typedef struct omni_gemv_params {
  const omni_bf16* A;
  int64_t lda;
  int32_t M, N, K, w_k32_blocked;
  const omni_bf16* W;
  const omni_bf16* bias;   /* [N], nullable */
  const omni_bf16* res;    /* [M, ldres], nullable */
  int64_t ldres;
  omni_bf16* out;          /* [M, ldo] */
  float* out_f32;          /* [M, ldo] */
  int64_t ldo;
} omni_gemv_params;
extern int (*const omni_gemv_bf16)(const omni_gemv_params* p, omni_stream stream);

/* omni_decode_attention: out[s, h, :] = softmax(scale * q[s, h, :] . K[s, h / G, 0 .. n_s - 1, :]) V[...], G = H / H_kv <= 8 query
 * heads sharing each K/V head, n_s = min(lens[s] + len_add, capacity) keys; the length is DEVICE memory (the host does not
 * know it without a read): the grid is sized by capacity, ceil(capacity / OMNI_DECODE_ATTN_CHUNK) x H_kv x n_seq workgroups,
 * and those whose key chunk lies behind n_s exit.  Cache rows at and behind n_s are never read.  A sequence with done[s] != 0
 * (done nullable) or n_s < 1 is skipped: its output row is not written.
 * k_cache / v_cache: bf16 [n_seq][H_kv][capacity][128]; q [n_seq, ldq >= H * 128]; out [n_seq, ldo >= H * 128].
 * workspace: fp32 partial results, as many bytes as omni_decode_attention_workspace_bytes answers for n_seq, H and capacity.
 * Status before any launch: null pointer, non-positive count, short workspace -> OMNI_ERR_BAD_ARG; head_dim != 128, n_seq > 8,
 * H % H_kv != 0, H / H_kv > 8 -> OMNI_ERR_UNSUPPORTED; q, out, caches or workspace not 16-byte aligned, ldq % 8, ldo % 8 ->
 * OMNI_ERR_ALIGN. */
#define OMNI_DECODE_ATTN_CHUNK 64
typedef struct omni_decode_attn_params {
  const omni_bf16* q;
  int64_t ldq;
  const omni_bf16* k_cache;
  const omni_bf16* v_cache;
  omni_bf16* out;
  int64_t ldo;
  const int32_t* lens;     /* DEVICE [n_seq] */
  const int32_t* done;     /* DEVICE [n_seq], nullable */
  int32_t len_add;         /* keys = lens[s] + len_add (the decode step: cur_len + 1, the row it has just appended) */
  int32_t n_seq, H, H_kv, head_dim, capacity;
  float softmax_scale;
  int32_t reserved;        /* 0 */
  void* workspace;
  size_t workspace_bytes;
} omni_decode_attn_params;
extern int (*const omni_decode_attention)(const omni_decode_attn_params* p, omni_stream stream);
extern size_t (*const omni_decode_attention_workspace_bytes)(int32_t n_seq, int32_t H, int32_t capacity);

/* The per-sequence decode control words: int32 [OMNI_DECODE_CTRL_WORDS][8] on the device, word w of sequence s at
 * ctrl[w * 8 + s].  They are written by ordinary vector stores of one lane. */
#define OMNI_DECODE_CUR_LEN 0      /* filled cache positions = the position of the token the next step consumes */
#define OMNI_DECODE_ROPE_DELTA 1   /* HF's mrope_position_deltas: the RoPE position of that token is cur_len + rope_delta */
#define OMNI_DECODE_CUR_ID 2       /* the token the next step consumes */
#define OMNI_DECODE_DONE 3
#define OMNI_DECODE_N_GENERATED 4
#define OMNI_DECODE_POS 5          /* scratch of a step: cur_len + rope_delta */
#define OMNI_DECODE_CTRL_WORDS 8   /* (256 bytes) */
/* omni_text_penalized_argmax: per sequence s with done == 0 and n_generated < max_new: x[v] = logits[s, v], for seen[s, v] != 0
 * x < 0 ? x * penalty : x / penalty (HF RepetitionPenaltyLogitsProcessor), t = the LOWEST index of the maximum (a NaN never
 * wins); then out_tokens[s, n_generated] = t, n_generated += 1, seen[s, t] = 1, cur_id = t, cur_len += 1 (set_len_cu non-null,
 * the prefill: cur_len = set_len_cu[s + 1] - set_len_cu[s]), done = 1 when t is one of eos_ids or n_generated reached max_new.
 * A sequence with done != 0 is left untouched.  One workgroup per sequence.
 * Status: null logits / seen / ctrl / out_tokens, vocab, n_seq or max_new < 1, penalty <= 0, n_eos < 0, ld < vocab,
 * seen_stride < vocab -> OMNI_ERR_BAD_ARG; n_seq > 8, n_eos > 8 -> OMNI_ERR_UNSUPPORTED. */
typedef struct omni_penalized_argmax_params {
  const float* logits;     /* [n_seq, ld] */
  int64_t ld;
  uint8_t* seen;           /* [n_seq, seen_stride] */
  int64_t seen_stride;
  int32_t* ctrl;           /* the control words */
  int32_t* out_tokens;     /* [n_seq, max_new] */
  const int32_t* set_len_cu; /* nullable */
  int32_t vocab, n_seq, max_new, n_eos;
  int32_t eos_ids[8];
  float penalty;
  int32_t reserved;        /* 0 */
} omni_penalized_argmax_params;
extern int (*const omni_text_penalized_argmax)(const omni_penalized_argmax_params* p, omni_stream stream);

/* The decode state: ONE caller-owned device buffer of as many bytes as omni_qwen2_text_decode_state_bytes answers, carved by the library;
 * `layout` (nullable) receives the byte offsets of the parts a caller reads or writes (cur_id for teacher forcing, done /
 * n_generated between chunks of steps, out_tokens at the end, the caches in tests). */
typedef struct omni_text_decode_layout {
  size_t ctrl;           /* int32 [OMNI_DECODE_CTRL_WORDS][8] */
  size_t out_tokens;     /* int32 [n_seq][max_new] */
  size_t seen;           /* uint8 [n_seq][seen_stride]: the tokens of the prompt and of the output so far */
  size_t seen_stride;
  size_t k_cache;        /* bf16 [num_layers][n_seq][H_kv][capacity][128], K after RoPE */
  size_t v_cache;        /* the same for V */
  size_t logits;         /* fp32 [n_seq][vocab_size]: the last step's logits (where logits_out is null) */
  size_t qkv;            /* bf16 [n_seq][(H + 2 H_kv) * 128]: the last step's q | k | v row of the LAST layer, after RoPE */
  size_t total;
} omni_text_decode_layout;
/* 0 for weights or counts the decode refuses */
extern size_t (*const omni_qwen2_text_decode_state_bytes)(const omni_text_weights* w, int32_t n_seq, int32_t capacity,
                                                          int32_t max_new, omni_text_decode_layout* layout);

typedef struct omni_text_decode_state {
  int32_t n_seq;               /* sequences, <= 8 */
  int32_t capacity;            /* cache positions per sequence */
  int32_t max_new;             /* rows of out_tokens */
  int32_t n_eos;               /* <= 8 */
  int32_t eos_ids[8];
  float repetition_penalty;    /* > 0; 1 = none */
  int32_t reserved;            /* 0 */
  const omni_bf16* lm_head;    /* [vocab_size, D] bf16 row-major (untied from embed_tokens in the 7B checkpoint) */
  void* state;                 /* DEVICE, 16-byte aligned */
  size_t state_bytes;
  void* workspace;             /* the prefill's workspace (omni_text_batch_mm.workspace): its error word is the decode's too */
  size_t workspace_bytes;
  float* logits_out;           /* nullable: fp32 [n_seq, vocab_size], the raw logits (before the penalty) of the last call */
} omni_text_decode_state;
/* omni_qwen2_text_prefill: the driver of omni_qwen2_text_forward_mm - b->out is bit-identical - which also writes every layer's
 * K (after RoPE) and V rows into the cache, then: logits of each sequence's last row through lm_head, the prompt ids marked in
 * the seen map, the first token picked (omni_text_penalized_argmax: out_tokens[s, 0], n_generated = 1, EOS test), cur_len = the
 * prompt's length, rope_delta = max position + 1 - length.  b->n_prompts == st->n_seq, b->max_seqlen <= st->capacity.
 * omni_qwen2_text_decode_step: one token for every sequence that is not done.  ENQUEUE-ONLY: no host read, no allocation;
 * position and length are device memory, so any number of steps may be queued back to back.  Per layer: RMSNorm ->
 * omni_gemv_bf16 q|k|v + bias -> RoPE at cur_len + rope_delta -> K, V appended at cur_len -> omni_decode_attention -> o_proj +
 * residual -> RMSNorm -> gate|up -> omni_text_swiglu -> down + residual; then final norm -> lm_head (fp32 logits) ->
 * omni_text_penalized_argmax.  A sequence with done set neither advances nor writes to the cache; cur_len >= capacity or
 * n_generated >= max_new never writes and sets done, a full cache also the workspace's error word (reported, as always, by
 * the next omni_qwen2_text_forward* / prefill over that workspace).
 * Status before any launch (both): null pointer, non-positive count, penalty <= 0, short state or workspace ->
 * OMNI_ERR_BAD_ARG; n_seq > 8, n_eos > 8, head_dim != 128, more than 8 query heads per K/V head (and whatever
 * omni_qwen2_text_forward refuses) -> OMNI_ERR_UNSUPPORTED; state, workspace or lm_head not 16-byte aligned -> OMNI_ERR_ALIGN. */
extern int (*const omni_qwen2_text_prefill)(const omni_text_weights* w, const omni_text_batch_mm* b,
                                            const omni_text_decode_state* st, omni_stream stream);
extern int (*const omni_qwen2_text_decode_step)(const omni_text_weights* w, const omni_text_decode_state* st, omni_stream stream);

/* ------------------------------------------------------------------------------------------------
 * VAE kernels (AutoencoderKLQwenImage.decode — and .encode for the Edit pipelines — for one frame,
 * vllm_omni/diffusion/models/qwen_image/autoencoder_kl_qwenimage.py:839-863 / diffusers twin).
 * Activations are NHWC bf16 ([B, H, W, C]); conv weights are pre-packed [Cout, 3, 3, Cin] bf16 from temporal
 * slice [-1] of the causal Conv3d weights (:69-84: the two zero front frames make the other slices dead).
 * ---------------------------------------------------------------------------------------------- */
/* 3x3 (pad 1) or 1x1 convolution as implicit GEMM on MFMA.  Optional fused prologue
 * RMS-norm(channels)*gamma -> SiLU on the input (QwenImageRMS_norm :108-109 + SiLU, :262-265),
 * optional nearest-exact x2 upsample of the input (QwenImageUpsample :112-124), optional residual add. */
typedef struct {
  const omni_bf16* x;     /* [B, Hin, Win, Cin] */
  const omni_bf16* w;     /* [Cout, ks, ks, Cin] */
  const omni_bf16* bias;  /* [Cout], nullable */
  const omni_bf16* gamma; /* [Cin], nullable -> no norm/SiLU prologue */
  const omni_bf16* res;   /* [B, Hout, Wout, Cout], nullable */
  omni_bf16* y;           /* [B, Hout, Wout, Cout] */
  int32_t B, Hin, Win, Cin, Cout;
  int32_t ksize;          /* 1 or 3 */
  int32_t upsample2x;     /* 1: Hout = 2*Hin (input index = out/2), else Hout = Hin */
  int32_t silu;           /* with gamma: apply SiLU after the norm */
  float clamp_lo, clamp_hi; /* applied if clamp_lo < clamp_hi */
  int32_t downsample2x;   /* 1 (3x3 only): ZeroPad2d((0,1,0,1)) + stride-2 conv of the VAE ENCODER's downsample2d/3d
                           * (autoencoder_kl_qwenimage.py:162-166): Hout = Hin / 2, source = 2*dst + tap.  ABI v3 */
  int32_t x_padded;       /* ABI v8.  1: x (and res) are ZERO-BORDERED rasters [B, Hin + 2, Win + 2, C]: the conv's zero padding
                           * (F.pad in QwenImageCausalConv3d.forward, :80-84) is resident in memory instead of re-created per tap */
  int32_t y_padded;       /* ABI v8.  1: y is written as a zero-bordered raster too (needs x_padded, Cin % 32 == 0,
                           * Cout % 8 == 0, no downsample): the decoder's 3x3 / 1x1 convs run as a GEMM over nine row-shifted
                           * views of x, LDS-DMA fed (vae.hip conv_bordered_kernel).  ABI v10: with upsample2x (3x3, no res) x is
                           * the half-resolution bordered raster [B, Hin + 2, Win + 2, Cin] and y [B, 2 Hin + 2, 2 Win + 2, Cout]:
                           * the operand fetch reads source pixel ((Y - 1) / 2 + 1, (X - 1) / 2 + 1) for pixel (Y, X) of the
                           * upsampled raster — the same result as omni_vae_upsample2x_bordered followed by the conv, bit for bit */
  /* ABI v10: the norm + activation that FOLLOWS this conv in the decoder (QwenImageResidualBlock.forward norm1 / norm2 + SiLU,
   * autoencoder_kl_qwenimage.py:262-275; norm_out :735-737) as a second output of the same launch:
   *   y_norm = silu?(F.normalize(y, dim=C) * sqrt(C) * norm_gamma)      computed from y as rounded to bf16
   * (== omni_vae_rmsnorm_silu(y) bit for bit up to the summation order of the squares).  norm_gamma NULL -> off. */
  const omni_bf16* norm_gamma; /* [Cout], nullable */
  omni_bf16* y_norm;           /* same shape as y; required with norm_gamma */
  int32_t norm_silu;           /* apply SiLU after the norm */
} omni_conv_params;
/* With norm_gamma: the conv kernel itself writes y_norm when one workgroup holds all channels of a pixel
 * (omni_vae_conv2d_fuses_norm(p) == 1: zero-bordered rasters, Cout <= 96, or Cout <= 192 on rasters that fill the chip with
 * 192-channel tiles); then y may be NULL (only the normed output is wanted).  Otherwise the call runs the conv into y (required)
 * and omni_vae_rmsnorm_silu from y into y_norm. */
int omni_vae_conv2d(const omni_conv_params* p, omni_stream stream);
int omni_vae_conv2d_fuses_norm(const omni_conv_params* p);

/* Nearest-exact x2 upsample (QwenImageUpsample, autoencoder_kl_qwenimage.py:112-124) between zero-bordered rasters:
 * x [B, H + 2, W + 2, C] -> y [B, 2H + 2, 2W + 2, C].  C % 8 == 0.  ABI v8 */
int omni_vae_upsample2x_bordered(const omni_bf16* x, omni_bf16* y, int32_t B, int32_t H, int32_t W, int32_t C,
                                 omni_stream stream);

/* Channel RMS-norm (F.normalize(dim=C) * sqrt(C) * gamma) with optional SiLU: NHWC rows of C channels. */
int omni_vae_rmsnorm_silu(const omni_bf16* x, omni_bf16* y, int64_t rows, int32_t C, const omni_bf16* gamma,
                          int32_t silu, omni_stream stream);

/* ABI v10 — the single-head attention of the VAE mid block (QwenImageAttentionBlock.forward,
 * autoencoder_kl_qwenimage.py:305-330: F.scaled_dot_product_attention over all tokens of an image, ONE head of C = 384 channels)
 * as one flash kernel: q, k, v [B][tokens][C] bf16 with row strides ldq / ldk / ldv (elements; images tokens * ld apart, so the
 * three may be column slices of one fused [B * tokens, 3 C] projection), out [B][tokens][C] with row stride ldo;
 * out = softmax(scale * q k^T) v per image.  C must be 384 (OMNI_ERR_UNSUPPORTED otherwise: callers fall back to
 * GEMM -> omni_softmax_rows -> GEMM); any token count (ragged tails are masked); tokens * ld * 2 < 4 GiB. */
int omni_vae_attention(const omni_bf16* q, const omni_bf16* k, const omni_bf16* v, omni_bf16* out, int32_t B, int32_t tokens,
                       int32_t C, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale, omni_stream stream);

/* In-place row softmax p = softmax(scale * s) over rows of `cols` bf16 scores (row stride ld).  Used for the
 * single-head mid-block attention of the VAE (F.scaled_dot_product_attention at
 * autoencoder_kl_qwenimage.py:319), which runs as GEMM(QK^T) -> this -> GEMM(PV).  cols % 8 == 0. */
int omni_softmax_rows(omni_bf16* s, int64_t ld, int64_t rows, int32_t cols, float scale, omni_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Whole DiT forward as one native call: enqueues every kernel of
 * QwenImageTransformer2DModel.forward (qwen_image_transformer.py:692-802) on `stream` from a
 * descriptor of device pointers.  No host synchronisation, no allocation; hipGraph-capturable.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const omni_bf16 *img_mod_w, *img_mod_b, *txt_mod_w, *txt_mod_b;   /* [6D, D], [6D] */
  const omni_bf16 *to_qkv_w, *to_qkv_b, *add_qkv_w, *add_qkv_b;     /* [3D, D], [3D] */
  const omni_bf16 *norm_q_w, *norm_k_w, *norm_added_q_w, *norm_added_k_w; /* [128] */
  const omni_bf16 *to_out_w, *to_out_b, *to_add_out_w, *to_add_out_b; /* [D, D], [D] */
  const omni_bf16 *img_mlp_w1, *img_mlp_b1, *img_mlp_w2, *img_mlp_b2; /* [4D, D],[4D],[D,4D],[D] */
  const omni_bf16 *txt_mlp_w1, *txt_mlp_b1, *txt_mlp_w2, *txt_mlp_b2;
} omni_dit_layer_weights;

/* ABI v7 — optional fp8 copies of a layer's eight GEMM weights (BASELINE.json config 5): OCP e4m3 bytes in the K64-blocked
 * order + one fp32 scale per output channel, both written by omni_quantize_fp8_rows(weight [out, in]).  With
 * omni_dit_weights.fp8_layers set, every block GEMM runs as omni_gemm_params.fp8: its bf16 input (AdaLN output, attention
 * output, GELU output) is quantised per token by omni_quantize_fp8_rows right in front of it; biases, epilogues, the residual
 * streams, q/k/v, the attention and everything outside the block GEMMs stay bf16.
 * ABI v9 — per GEMM class: the four classes are (to_qkv, add_qkv), (to_out, to_add_out), (img/txt mlp w1), (img/txt mlp w2);
 * a class whose two weight pointers are NULL runs in bf16 from omni_dit_layer_weights as without fp8 (mixed recipes). */
typedef struct {
  const uint8_t *to_qkv_w8, *add_qkv_w8, *to_out_w8, *to_add_out_w8, *img_mlp_w1_8, *img_mlp_w2_8, *txt_mlp_w1_8, *txt_mlp_w2_8;
  const float *to_qkv_s, *add_qkv_s, *to_out_s, *to_add_out_s, *img_mlp_w1_s, *img_mlp_w2_s, *txt_mlp_w1_s, *txt_mlp_w2_s;
} omni_dit_fp8_layer;

typedef struct {
  int32_t num_layers, num_heads, head_dim, joint_dim, in_channels, out_channels_packed; /* 60,24,128,3584,64,64 */
  int32_t gemm_w_k32_blocked; /* 1: the eight [out,in] matrices of every layer (to_qkv, add_qkv, to_out, to_add_out,
                               * img/txt mlp w1, w2) are stored K32-blocked (omni_gemm_params.w_k32_blocked); all other
                               * weights are always row-major.  ABI v2. */
  const omni_bf16 *t_lin1_w, *t_lin1_b, *t_lin2_w, *t_lin2_b; /* TimestepEmbedding */
  const omni_bf16 *txt_norm_w, *img_in_w, *img_in_b, *txt_in_w, *txt_in_b;
  const omni_bf16 *norm_out_w, *norm_out_b, *proj_out_w, *proj_out_b;
  const omni_dit_layer_weights* layers; /* HOST array [num_layers] of device pointers */
  const omni_dit_fp8_layer* fp8_layers; /* ABI v7: nullable HOST array [num_layers]; NULL = bf16 GEMMs */
} omni_dit_weights;

/* ------------------------------------------------------------------------------------------------
 * TeaCache state of one step-batch (vllm_omni/diffusion/cache/teacache/hook.py:82-217, state.py, config.py), kept ON THE
 * DEVICE and evaluated by kernels inside omni_dit_forward, PER ITEM (request x CFG branch — the reference keeps one state
 * per CFG branch of its single request, hook.py:113-121):
 *   rel = mean|mod - prev_mod| / (mean|prev_mod| + 1e-8)   over the item's first-block modulated input (:195-206)
 *   acc += |poly(rel)|;  cnt == 0 -> compute (acc = 0);  acc < thresh -> SKIP the 60 blocks, else compute and acc = 0
 *   skip   : hidden_img += prev_res                       (:127-134; the encoder residual is dead code there: only
 *   compute: prev_res = hidden_img_after - hidden_img_before   (:135-157)   hidden_states reaches norm_out / proj_out)
 * The reference reads the decision back with .cpu().item() (a host sync per forward); here the decision stays on the
 * device: skipped items' GEMM row tiles and attention blocks return immediately (omni_gemm_group.tile_skip), so the launch
 * sequence is fixed, sync-free and hipGraph-capturable, and step-batched items keep their own B=1 decisions.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  float rel_l1_thresh;
  float coeff[5];        /* polynomial, highest power first (numpy.poly1d order, config.py:9-31) */
  omni_bf16* prev_mod;   /* [n_img_rows * D] previous modulated input (layout = whatever the first AdaLN writes) */
  omni_bf16* prev_res;   /* [n_img_rows, D] cached residual of the image stream */
  float* acc_dist;       /* [n_items] accumulated rescaled distance */
  int32_t* cnt;          /* [n_items] forwards seen since reset (0 -> always compute) */
  int32_t* skip;         /* [n_items] out: this forward's decision (1 = blocks skipped) */
  int32_t* skip_total;   /* [n_items] out: running count of skipped forwards (statistics) */
  float* scratch;        /* [2 * n_items] zero-initialised partial sums (left zeroed by every forward) */
  int32_t* tile_skip_img;/* [ceil(n_img_rows / 256)] scratch */
  int32_t* tile_skip_txt;/* [ceil(n_txt_rows / 256)] scratch */
  const int32_t* txt_cu; /* [n_items + 1] prefix sums of the text rows */
} omni_teacache;

typedef struct {
  /* ragged batch of n_items sequences; item i: T_i text rows then S_img image rows in the joint order */
  int32_t n_items, n_img_rows, n_txt_rows, n_joint_rows, n_temb, max_seqlen;
  /* max_seqlen: at least the joint rows (text + image) of the longest item.  It sizes the attention grid and, with `teacache`
   * set, the grids of the TeaCache kernels (an item's image rows never exceed its joint rows): too small a value leaves rows
   * of the longest item unvisited without an error. */
  const omni_bf16* latents;       /* [n_img_rows, in_channels] packed latents           */
  const omni_bf16* prompt_embeds; /* [n_txt_rows, joint_dim]                            */
  const float* timestep;          /* [n_temb] sigma (the pipeline's t/1000)             */
  const int32_t* cu_seqlens;      /* [n_items+1] joint-row prefix sums                  */
  const int32_t* img_item;        /* [n_img_rows] -> temb row of that token             */
  const int32_t* txt_item;        /* [n_txt_rows] -> temb row                            */
  const int32_t* img_joint_row;   /* [n_img_rows] -> joint row                           */
  const int32_t* txt_joint_row;   /* [n_txt_rows] -> joint row                           */
  const int32_t* joint_pos;       /* [n_joint_rows] -> rope table row                    */
  int32_t txt_pos_end;            /* rope rows < this are text positions                 */
  int32_t attn_qk_int8;           /* ABI v14.  NOT appended at the end: it occupies the former padding behind txt_pos_end, so
                                   * the descriptor keeps its size and every other offset (a caller built against v13 that
                                   * zero-initialises the struct gets 0 here).  1 = the joint attention of every block runs as
                                   * omni_attn_params.qk_int8 (SAGE_ATTN) on q / k / v of the block; its int8 copies live in
                                   * the MLP hidden buffer of the workspace, dead during the attention (same workspace size) */
  const omni_bf16 *rope_cos, *rope_sin; /* [npos, 64] bf16                               */
  omni_bf16* noise_pred;          /* [n_img_rows, out_channels_packed]                   */
  /* workspace (caller-allocated, sizes from omni_dit_workspace_bytes) */
  void* workspace;
  size_t workspace_bytes;
  const omni_teacache* teacache;  /* nullable: TeaCache off.  ABI v3.  Item i owns the image rows [img_cu[i], img_cu[i + 1]) with
                                   * img_cu[i] = cu_seqlens[i] - teacache->txt_cu[i]: at most 64 items, each with at least one
                                   * image row; they may differ in size in a library that reports OMNI_FEATURE_TEACACHE_RAGGED
                                   * (one without that bit refuses unequal items with OMNI_ERR_UNSUPPORTED) */
  const omni_bf16* temb_add;      /* ABI v9, nullable: [n_temb, D] bf16 added to the timestep embedding — the Layered variant's
                                   * addition_t_embedding(additional_t_cond) rows (qwen_image_transformer.py:47-62) */
  const omni_bf16* mod_table;     /* ABI v9, nullable: [num_layers][2 (image, text stream)][n_temb][6 D] bf16 — the blocks'
                                   * modulation vectors for THIS forward's conditioning rows, taken from
                                   * omni_dit_modulation_table; the 2 x num_layers weight-streaming GEMVs are then skipped */
} omni_dit_batch;

size_t omni_dit_workspace_bytes(const omni_dit_weights* w, int32_t n_img_rows, int32_t n_txt_rows, int32_t n_temb);

/* ABI v9 — the modulation vectors of every block for M conditioning rows in ONE pass over the modulation weights:
 *   table[l][s][m] = Linear_{l,s}(SiLU(temb[m]))   s = 0: img_mod, 1: txt_mod   (qwen_image_transformer.py:478-481,494-497,552-561)
 * temb [M, D] bf16 = the timestep embeddings (time_text_embed) of all the denoising steps of a request — they are known
 * before the loop starts — table [num_layers][2][M][6 D] bf16.  The reference re-streams these 13.6 GB of weights in EVERY
 * forward (226 MB per block for 0.23 GFLOP); a request of N steps x 2 CFG branches reads them 2N times, here
 * once.  At 256^2 (a forward is ~10 ms of which 2.7 ms is this stream) that is a quarter of the latency.  SiLU output is
 * rounded to bf16 before the product, as in the reference's eager nn.Sequential(SiLU, Linear).  Caller-owned workspace. */
size_t omni_dit_modulation_table_workspace_bytes(const omni_dit_weights* w, int32_t M);
int omni_dit_modulation_table(const omni_dit_weights* w, const omni_bf16* temb, int32_t M, omni_bf16* table, void* workspace,
                              size_t workspace_bytes, omni_stream stream);
int omni_dit_forward(const omni_dit_weights* w, const omni_dit_batch* b, omni_stream stream);

/* One dual-stream block (QwenImageTransformerBlock.forward, qwen_image_transformer.py:541-605) on caller-owned residual
 * streams: hidden_img [n_img_rows, D], hidden_txt [n_txt_rows, D] (updated in place), temb [n_temb, D].  Same kernels and
 * the same batch descriptor as omni_dit_forward (latents / prompt_embeds / timestep / noise_pred of `b` are not read).
 * This is the entry point behind the module-level plug-in surface that cache hooks walk
 * (cache/teacache/extractors.py:216-233 calls `block(hidden_states=..., encoder_hidden_states=..., temb=...)`). */
int omni_dit_block(const omni_dit_weights* w, int32_t layer, const omni_dit_batch* b, omni_bf16* hidden_img,
                   omni_bf16* hidden_txt, const omni_bf16* temb, omni_stream stream);

/* The two halves of a block around the attention, for SEQUENCE-PARALLEL callers (Ulysses: all-to-all of q/k/v before the
 * attention and of its output after it — reference vllm_omni/diffusion/attention/parallel/ulysses.py:59-135,
 * qwen_image_transformer.py:735-742,776-781,800-801).  `b` describes THIS RANK's rows (its chunk of the image tokens + the
 * replicated text tokens).  omni_dit_block_qkv runs modulation + norm1 + the fused QKV projection (+ q/k norm + RoPE) and
 * returns pointers to the joint-order [n_joint_rows, D] q/k/v inside the workspace; the caller exchanges them, runs
 * omni_flash_attn_fwd on the head slice it owns, exchanges back, and hands the row-major [n_joint_rows, D] attention output of
 * its own rows to omni_dit_block_post, which finishes the block (output projections, gated residuals, norm2, MLP). */
int omni_dit_block_qkv(const omni_dit_weights* w, int32_t layer, const omni_dit_batch* b, omni_bf16* hidden_img,
                       omni_bf16* hidden_txt, const omni_bf16* temb, omni_bf16** q, omni_bf16** k, omni_bf16** v,
                       omni_stream stream);
int omni_dit_block_post(const omni_dit_weights* w, int32_t layer, const omni_dit_batch* b, omni_bf16* hidden_img,
                        omni_bf16* hidden_txt, const omni_bf16* temb, const omni_bf16* attn, omni_stream stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* OMNI_CDNA4_H */
