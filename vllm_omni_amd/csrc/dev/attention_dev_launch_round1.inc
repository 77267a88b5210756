// host launcher of the round-1 register-staged kernels.
// Textually included by ../attention.hip in -DOMNI_DEV builds only (tools/build_variants.sh); never part of the product library.
template <int NQ>
int launch_attn(const omni_bf16* q, const omni_bf16* k, const omni_bf16* v, omni_bf16* out, int64_t ldq, int64_t ldk,
                int64_t ldv, int64_t ldo, const int32_t* cu_seqlens, int32_t B, int32_t H, int32_t max_seqlen,
                float softmax_scale, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(flash_attn_fwd_kernel<NQ>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess)
      return OMNI_ERR_LAUNCH;
    attr_set = true;
  }
  constexpr int QBLK = 32 * NWAVES * NQ;
  const int qblocks = (max_seqlen + QBLK - 1) / QBLK;
  const int nh = B * H;
  hipLaunchKernelGGL(flash_attn_fwd_kernel<NQ>, dim3(nh * qblocks), dim3(NWAVES * 64), LDS_BYTES, s, q, k, v, out, ldq,
                     ldk, ldv, ldo, cu_seqlens, nh, H, softmax_scale * OMNI_LOG2E);
  OMNI_CHECK_LAUNCH();
  return OMNI_OK;
}
