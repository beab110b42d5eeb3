// What optim.hip (Adam, O1) and optim_amsgrad.hip (Adam with amsgrad, O7) share: the step's coefficients, the rate of a step, the
// one definition of a table element's m and v rounding (adam_touched, adam_untouched), the sweep's field table and the
// hyper-parameter check.  The AMSGrad forms sit beside Adam's and form m and v THROUGH them, so the table m and v of an amsgrad run
// are the bits of an Adam run on the same gradients by construction.
#pragma once
#include "common.h"
#include "optim_rows.h"

namespace fil {

struct AdamCoef {
  float alpha, omb1, omb2, eps;
};

__device__ __forceinline__ AdamCoef adam_coef(const int64_t* step, float lr, float b1, float b2, float eps) {
  const float t = (float)(*step + 1);                 // Keras: local_step = cast(iterations + 1, float32)
  const float b1p = powf(b1, t), b2p = powf(b2, t);
  AdamCoef c;
  c.alpha = lr * sqrtf(1.f - b2p) / (1.f - b1p);
  c.omb1 = 1.f - b1;
  c.omb2 = 1.f - b2;
  c.eps = eps;
  return c;
}

// the step's rate: the by-value one, or the word fil_lr_schedule_eval left on the device (the *_lrdev entry points).  A
// wave-uniform load, once per kernel.
__device__ __forceinline__ float rate_of(float lr, const float* __restrict__ lr_dev) { return lr_dev ? *lr_dev : lr; }

// The embedding-table kernels, Keras mode and deferred mode alike, update a row through the two helpers below and nothing else: one
// definition of each update's rounding, written with contraction off and explicit fmas, so the deferred replays give the Keras-mode
// bits by construction, whatever the compiler makes of each kernel's context.
//
// the untouched-row update of the sweep (g = 2 l2[f] p); fused_m: its 16-byte path (K % 4 == 0, 16-byte aligned arrays) rounds
// m += (g - m)(1 - b1) as one fma, its element path rounds the product first
template <bool fused_m>
__device__ __forceinline__ void adam_untouched(float& p, float& m, float& v, float l2x2, const AdamCoef& c) {
#pragma clang fp contract(off)
  const float g = l2x2 * p;
  const float d = __builtin_fmaf(l2x2, p, -m);
  const float gg = __builtin_fmaf(g, g, -v);
  m = fused_m ? __builtin_fmaf(c.omb1, d, m) : m + c.omb1 * d;
  v = __builtin_fmaf(c.omb2, gg, v);
  p = p - (m * c.alpha) / (sqrtf(v) + c.eps);
}

// the touched-row update of the runs and merged kernels: g = (run sum) + 2 l2 p
__device__ __forceinline__ void adam_touched(float& p, float& m, float& v, float acc, float l2x2, const AdamCoef& c) {
#pragma clang fp contract(off)
  const float g = __builtin_fmaf(l2x2, p, acc);
  const float d = g - m;
  const float gg = __builtin_fmaf(g, g, -v);
  m = m + c.omb1 * d;
  v = __builtin_fmaf(c.omb2, gg, v);
  p = p - (m * c.alpha) / (sqrtf(v) + c.eps);
}

// ---- AMSGrad (Keras' Adam(amsgrad=True); TF 2.1 ApplyAdamWithAmsgrad): m and v as Adam's, then
//   vhat = (vhat < v) ? v : vhat        Eigen's cwiseMax order: a NaN v leaves vhat alone (NOT fmaxf, which would also drop a NaN vhat)
//   p -= (m alpha) / (sqrt(vhat) + eps)
// the vhat step and the move with the vhat denominator, rounded as written
__device__ __forceinline__ void amsgrad_move(float& p, float m, float v, float& vhat, const AdamCoef& c) {
#pragma clang fp contract(off)
  vhat = (vhat < v) ? v : vhat;
  p = p - (m * c.alpha) / (sqrtf(vhat) + c.eps);
}

// the untouched-row update of the AMSGrad sweep: adam_untouched's m and v (its move of p is dropped: the copy q is dead)
template <bool fused_m>
__device__ __forceinline__ void amsgrad_untouched(float& p, float& m, float& v, float& vhat, float l2x2, const AdamCoef& c) {
  float q = p;
  adam_untouched<fused_m>(q, m, v, l2x2, c);
  amsgrad_move(p, m, v, vhat, c);
}

// the touched-row update of the AMSGrad runs and merged kernels: adam_touched's m and v
__device__ __forceinline__ void amsgrad_touched(float& p, float& m, float& v, float& vhat, float acc, float l2x2, const AdamCoef& c) {
  float q = p;
  adam_touched(q, m, v, acc, l2x2, c);
  amsgrad_move(p, m, v, vhat, c);
}

// the sweep's view of the fields, in LDS: a row's field is the last f with off[f] <= row; l2x2 = 2 l2[f], NaN for a frozen field
struct FieldTab {
  int64_t off[kSweepMaxF];
  float l2x2[kSweepMaxF];
};

__device__ __forceinline__ void load_field_tab(FieldTab* s, const int64_t* __restrict__ offsets, const float* __restrict__ field_l2,
                                               const unsigned char* __restrict__ frozen, int F) {
  for (int f = threadIdx.x; f < F; f += blockDim.x) {
    s->off[f] = offsets[f];
    s->l2x2[f] = (frozen && frozen[f]) ? __builtin_nanf("") : (field_l2 ? 2.f * field_l2[f] : 0.f);
  }
}

__device__ __forceinline__ float field_l2x2(const FieldTab* s, int F, int64_t row) {
  const int f = sweep_field(s->off, F, row);
  return f >= 0 ? s->l2x2[f] : 0.f;
}

inline int check_hyper(const char* who, float lr, float b1, float b2, float eps) {
  if (!(lr >= 0.f) || !(b1 >= 0.f && b1 < 1.f) || !(b2 >= 0.f && b2 < 1.f) || !(eps >= 0.f))
    return fail(FIL_ERR_ARG, "%s: hyper-parameters lr=%g beta_1=%g beta_2=%g epsilon=%g (lr, epsilon >= 0; betas in [0, 1))", who,
                (double)lr, (double)b1, (double)b2, (double)eps);
  return FIL_OK;
}

}  // namespace fil
