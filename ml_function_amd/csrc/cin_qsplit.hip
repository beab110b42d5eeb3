// Instantiations + dispatch of the split-bf16 kernels of the merged quadratic tail (cin_qsplit.h): NP = 3 planes per operand (the split,
// FIL_CIN_BF16X3) or one (FIL_CIN_PREC_BF16).
#include "cin_qsplit.h"

namespace fil {

bool cin_launch_fwdq_b(hipStream_t st, int NP, int JT, const float* x2T, int XL, const u32x4* Wb, int NT, const float* bias1, const float* wsn, int JTG,
                       const float* cvec, float* x1T, float* RT, int HS, float* pool1, float* pool_p, float* pool_L, int M, int F, int H, CinHeadFold hf) {
  // (4-wave workgroups, two per CU, each with a ring of three; one 8-wave workgroup per CU sharing a ring of four measured the same:
  // 127.7 against 129.7 us.  One plane: rings of kQbStages 8-KB steps)
  const size_t sh = NP == 1 ? (size_t)kQbStages * qs_stage_bytes(1) : (size_t)3 * kQsStageBytes;
#define FIL_FQB(JTV, NPV)                                                                                                                             \
  case JTV:                                                                                                                                           \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cin_fwdq_b_kernel<JTV, 4, NPV>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);   \
    hipLaunchKernelGGL((cin_fwdq_b_kernel<JTV, 4, NPV>), dim3(cdiv(M, 128)), dim3(256), sh, st, x2T, XL, Wb, NT, bias1, wsn, JTG, cvec, x1T, RT, HS,  \
                       pool1, pool_p, pool_L, M, F, H, hf);                                                                                           \
    break;
  if (NP == 3) {
    switch (JT) { FIL_FQB(2, 3) FIL_FQB(4, 3) FIL_FQB(6, 3) FIL_FQB(8, 3) FIL_FQB(10, 3) FIL_FQB(12, 3) default: return false; }
  } else if (NP == 1) {
    switch (JT) { FIL_FQB(2, 1) FIL_FQB(4, 1) FIL_FQB(6, 1) FIL_FQB(8, 1) FIL_FQB(10, 1) FIL_FQB(12, 1) default: return false; }
  } else {
    return false;
  }
#undef FIL_FQB
  return true;
}

bool cin_launch_dz2_b(hipStream_t st, int NP, int JT, const float* g1T, const float* g2T, int HS, const float* dsc, int ldp, int K, const u32x4* Wzb1,
                      const u32x4* Wzb2, const float* xT, float* dxT, int accumulate, int M, int F, int H1, int H2, int periods, float* dx,
                      const float* cvec) {
  // (blocks of four slots only: F >= HPP + 2 JT, as cin_launch_dz2 picks them; other shapes keep the exact kernel)
  if (!(JT >= 4 && F >= cin_dz_h_per_period(JT) + 2 * JT)) return false;
  const int FR = cin_dz2_rows(F, JT);
  const size_t sh = (size_t)FR * kDz2FieldStride * sizeof(float);
#define FIL_Z2B(JTV, NPV)                                                                                                                            \
  case JTV:                                                                                                                                          \
    if (sh > 48 * 1024)                                                                                                                              \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cin_dz2_b_kernel<JTV, 4, NPV>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh); \
    hipLaunchKernelGGL((cin_dz2_b_kernel<JTV, 4, NPV>), dim3(cdiv(M, 128)), dim3(kCinThreads), sh, st, g1T, g2T, HS, dsc, ldp, K, Wzb1, Wzb2, xT,   \
                       dxT, accumulate, M, F, H1, H2, periods, FR, dx, cvec);                                                                        \
    break;
  if (NP == 3) {
    switch (JT) { FIL_Z2B(4, 3) FIL_Z2B(6, 3) FIL_Z2B(8, 3) FIL_Z2B(10, 3) FIL_Z2B(12, 3) default: return false; }
  } else if (NP == 1) {
    switch (JT) { FIL_Z2B(4, 1) FIL_Z2B(6, 1) FIL_Z2B(8, 1) FIL_Z2B(10, 1) FIL_Z2B(12, 1) default: return false; }
  } else {
    return false;
  }
#undef FIL_Z2B
  return true;
}

void cin_launch_dwq_b(hipStream_t st, int NP, const DwqbPlan& p, const float* gT, const float* x1T, int HS, const float* xe, int XE, float* part, int M,
                      int F, int symD) {
  if (NP == 1) {
    const size_t sh = (size_t)dwqb_lds_bytes(1);   // (below 48 KB: no attribute)
    hipLaunchKernelGGL((cin_dwq_b_kernel<3, 1>), dim3((p.wgs + 7) / 8 * 8), dim3(256), sh, st, gT, x1T, HS, xe, XE, part, M, F, symD, p.rows_per_split,
                       p.splits, p.groups, p.items);
    return;
  }
  const size_t sh = (size_t)kDwqbHalfBytes;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cin_dwq_b_kernel<3>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
  hipLaunchKernelGGL(cin_dwq_b_kernel<3>, dim3((p.wgs + 7) / 8 * 8), dim3(256), sh, st, gT, x1T, HS, xe, XE, part, M, F, symD, p.rows_per_split, p.splits,
                     p.groups, p.items);
}

}  // namespace fil
