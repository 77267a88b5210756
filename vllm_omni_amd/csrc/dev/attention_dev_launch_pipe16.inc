// dev knobs + host launcher of the 16x16x32 form of the pipelined kernel.
// Textually included by ../attention.hip in -DOMNI_DEV builds only (tools/build_variants.sh); never part of the product library.
int attn_mfma_shape() {
  // dev knob: OMNI_ATTN_MFMA = 32 (default: flash_attn_fwd_pipe_kernel, 32x32x16) | 16 (flash_attn_fwd_pipe16_kernel, 16x16x32)
  static int v = -1;
  if (v < 0) {
    v = omni_dev_env_int("OMNI_ATTN_MFMA", 32);
    if (v != 16) v = 32;
  }
  return v;
}
int attn_pingpong() {
  // dev knob: OMNI_ATTN_PP = 0 (default) | 1 (wave groups half an iteration apart in the 8-wave kernel: measured 878 vs 912 TF/s)
  static int v = -1;
  if (v < 0) {
    v = omni_dev_env_int("OMNI_ATTN_PP", 0);
  }
  return v;
}
template <int NW>
int launch_pipe16(const omni_bf16* q, const omni_bf16* k, const omni_bf16* v, omni_bf16* out, int64_t ldq, int64_t ldk,
                  int64_t ldv, int64_t ldo, const int32_t* cu_seqlens, int32_t B, int32_t H, int32_t max_seqlen,
                  float softmax_scale, int out_k32_rows, hipStream_t s, const int32_t* item_skip) {
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(flash_attn_fwd_pipe16_kernel<NW>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess)
      return OMNI_ERR_LAUNCH;
    attr_set = true;
  }
  const int qblocks = (max_seqlen + 32 * NW - 1) / (32 * NW);
  const int nh = B * H;
  hipLaunchKernelGGL((flash_attn_fwd_pipe16_kernel<NW>), dim3(nh * qblocks), dim3(NW * 64), LDS_BYTES, s, q, k, v, out, ldq,
                     ldk, ldv, ldo, cu_seqlens, nh, H, softmax_scale * OMNI_LOG2E, out_k32_rows, attn_block_order(), item_skip);
  OMNI_CHECK_LAUNCH();
  return OMNI_OK;
}
