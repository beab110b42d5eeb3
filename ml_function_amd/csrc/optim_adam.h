// Keras' Adam, shared by optim.hip (O1) and optim_amsgrad.hip (O7, Adam with amsgrad): the step's coefficients, the rate of a step,
// the one definition of a table element's m and v rounding (adam_touched, adam_untouched), the sweep's field table, the
// hyper-parameter check -- and the Keras-mode table kernels (runs update, sweep, merged update) with their host launchers, each
// defined once and templated on `bool kAms`: with it a fourth array, the slot `vhat`, travels behind `v`.  optim.hip instantiates
// the <false> forms (vhat NULL, never looked at), optim_amsgrad.hip the <true> ones.  The dense launcher is one body too, over the
// descriptor type; each file brings its dense kernel (the walk of optim_rows.h around adam_elem, amsgrad_elem).  The AMSGrad element
// forms sit beside Adam's and form m and v THROUGH them, so the table m and v of an amsgrad run are the bits of an Adam run on the
// same gradients by construction.
#pragma once
#include "common.h"
#include "embed_runs.h"
#include "optim_rows.h"
#include <hip/hip_bf16.h>

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

// the Keras / lazy mode of Adam's runs and merged updates (AMSGrad has no lazy mode)
inline int check_mode(const char* who, int mode, const int32_t* stamp) {
  if (mode != FIL_ADAM_KERAS && mode != FIL_ADAM_LAZY) return fail(FIL_ERR_ARG, "%s: mode %d (FIL_ADAM_KERAS or FIL_ADAM_LAZY)", who, mode);
  if (mode == FIL_ADAM_KERAS && stamp == nullptr)
    return fail(FIL_ERR_ARG, "%s: FIL_ADAM_KERAS needs the row stamps (fil_embed_adam_sweep skips the rows stamped here)", who);
  return FIL_OK;
}

// ==== The Keras-mode table kernels.  kAms: the update is AMSGrad's and `vhat` is its slot; without it `vhat` is NULL and neither
// read nor written.

// one element of a touched row in place
template <bool kAms>
__device__ __forceinline__ void adam_touched_at(float* __restrict__ table, float* __restrict__ m, float* __restrict__ v,
                                                float* __restrict__ vhat, int64_t e, float acc, float l2x2, const AdamCoef& c) {
  float p = table[e], mm = m[e], vv = v[e], hh = 0.f;
  if constexpr (kAms) {
    hh = vhat[e];
    amsgrad_touched(p, mm, vv, hh, acc, l2x2, c);
  } else {
    adam_touched(p, mm, vv, acc, l2x2, c);
  }
  table[e] = p;
  m[e] = mm;
  v[e] = vv;
  if constexpr (kAms) vhat[e] = hh;
}

// ---- the runs update (fil_embed_adam_runs, fil_embed_amsgrad_runs): the run sums of embed_runs.h with the rule as epilogue.  Row
// `row` of field f = perm % F takes g = run sum + 2 l2[f] p; with stamps (Keras mode; lazy mode passes NULL) the row is stamped with
// the step it was updated at: the sweep skips stamped rows.
template <bool kAms, typename GT>
__global__ __launch_bounds__(256) void embed_adam_runs_kernel(const GT* __restrict__ g, const int64_t* __restrict__ perm,
                                                              const int64_t* __restrict__ sorted_ids, long R, int K, int F,
                                                              const float* __restrict__ field_l2, float* __restrict__ table,
                                                              float* __restrict__ m, float* __restrict__ v, float* __restrict__ vhat,
                                                              int32_t* __restrict__ stamp, const int64_t* __restrict__ step, float lr,
                                                              float b1, float b2, float eps, const float* __restrict__ lr_dev) {
  const AdamCoef c = adam_coef(step, rate_of(lr, lr_dev), b1, b2, eps);
  const int32_t tag = step_tag(step);
  embed_run_sums(g, perm, sorted_ids, R, K, [=](int64_t row, int kq, const float (&acc)[4], int64_t first) {
    const float l2x2 = field_l2 ? 2.f * field_l2[first % F] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (kq * 4 + i < K) adam_touched_at<kAms>(table, m, v, vhat, row * K + kq * 4 + i, acc[i], l2x2, c);
    if (stamp && kq == 0) stamp[row] = tag;
  });
}

// ---- the sweep (fil_embed_adam_sweep, fil_embed_amsgrad_sweep): every row the run pass did not stamp at this step takes
// g = 2 l2[f] p (or 0); frozen fields are left alone.  The field of a row comes from a binary search of the offsets held in LDS
// (FieldTab).  The vhat store is skipped where it would write back the bits it read.
template <bool kAms>
__global__ __launch_bounds__(256) void embed_adam_sweep_kernel(float* __restrict__ table, float* __restrict__ m, float* __restrict__ v,
                                                               float* __restrict__ vhat, const int32_t* __restrict__ stamp, int64_t V,
                                                               int K, const int64_t* __restrict__ offsets,
                                                               const float* __restrict__ field_l2,
                                                               const unsigned char* __restrict__ frozen, int F,
                                                               const int64_t* __restrict__ step, float lr, float b1, float b2, float eps,
                                                               int vec, const float* __restrict__ lr_dev) {
  __shared__ FieldTab s;
  load_field_tab(&s, offsets, field_l2, frozen, F);
  __syncthreads();
  const AdamCoef c = adam_coef(step, rate_of(lr, lr_dev), b1, b2, eps);
  const int32_t tag = step_tag(step);
  const int64_t n = V * K;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (vec) {                                  // K % 4 == 0 and 16-byte aligned arrays: a lane moves 4 elements of one row
    const int64_t nq = n / 4;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += stride) {
      const int64_t row = q * 4 / K;
      if (stamp[row] == tag) continue;
      const float l2x2 = field_l2x2(&s, F, row);
      if (l2x2 != l2x2) continue;             // frozen
      f32x4 p = reinterpret_cast<const f32x4*>(table)[q];
      f32x4 mm = reinterpret_cast<const f32x4*>(m)[q];
      f32x4 vv = reinterpret_cast<const f32x4*>(v)[q];
      f32x4 hh = {0.f, 0.f, 0.f, 0.f};
      if constexpr (kAms) hh = reinterpret_cast<const f32x4*>(vhat)[q];
      bool held = true;                       // the lane's four vhat keep their bits (an unregularised field: always)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float pi = p[i], mi = mm[i], vi = vv[i], hi = hh[i];
        if constexpr (kAms) {
          amsgrad_untouched<true>(pi, mi, vi, hi, l2x2, c);
          held = held && __float_as_uint(hi) == __float_as_uint(hh[i]);
        } else {
          adam_untouched<true>(pi, mi, vi, l2x2, c);
        }
        p[i] = pi;
        mm[i] = mi;
        vv[i] = vi;
        hh[i] = hi;
      }
      __builtin_nontemporal_store(p, reinterpret_cast<f32x4*>(table) + q);
      __builtin_nontemporal_store(mm, reinterpret_cast<f32x4*>(m) + q);
      __builtin_nontemporal_store(vv, reinterpret_cast<f32x4*>(v) + q);
      if constexpr (kAms)
        if (!held) __builtin_nontemporal_store(hh, reinterpret_cast<f32x4*>(vhat) + q);
    }
    return;
  }
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const int64_t row = e / K;
    if (stamp[row] == tag) continue;
    const float l2x2 = field_l2x2(&s, F, row);
    if (l2x2 != l2x2) continue;
    float p = table[e], mm = m[e], vv = v[e], hh = 0.f;
    if constexpr (kAms) hh = vhat[e];
    const float h0 = hh;
    if constexpr (kAms) amsgrad_untouched<false>(p, mm, vv, hh, l2x2, c);
    else adam_untouched<false>(p, mm, vv, l2x2, c);
    __builtin_nontemporal_store(p, table + e);
    __builtin_nontemporal_store(mm, m + e);
    __builtin_nontemporal_store(vv, v + e);
    if constexpr (kAms)
      if (__float_as_uint(hh) != __float_as_uint(h0)) __builtin_nontemporal_store(hh, vhat + e);
  }
}

// ---- the merged update (fil_embed_adam_merged, fil_embed_amsgrad_merged): the merged walk of the gathered lists (merged_row_sums,
// optim_rows.h); the owner of a row adds the field's l2 term and updates the row exactly as embed_adam_runs_kernel does.
template <bool kAms>
__global__ __launch_bounds__(256) void embed_adam_merged_kernel(const int64_t* __restrict__ ids, const float* __restrict__ values,
                                                                const int64_t* __restrict__ counts, int W, long cap, int K,
                                                                const int64_t* __restrict__ offsets, const float* __restrict__ field_l2,
                                                                int F, float* __restrict__ table, float* __restrict__ m,
                                                                float* __restrict__ v, float* __restrict__ vhat,
                                                                int32_t* __restrict__ stamp, int64_t V,
                                                                const int64_t* __restrict__ step, float lr, float b1, float b2, float eps,
                                                                const float* __restrict__ lr_dev) {
  __shared__ int64_t s_off[kSweepMaxF];
  for (int f = threadIdx.x; f < F; f += blockDim.x) s_off[f] = offsets[f];
  __syncthreads();
  const AdamCoef c = adam_coef(step, rate_of(lr, lr_dev), b1, b2, eps);
  const int32_t tag = step_tag(step);
  const auto epi = [=](int64_t row, int f, float l2x2, int k0, const float (&acc)[kMergeChunk]) {
#pragma unroll
    for (int e = 0; e < kMergeChunk; ++e)
      if (k0 + e < K) adam_touched_at<kAms>(table, m, v, vhat, row * K + k0 + e, acc[e], l2x2, c);
  };
  merged_row_sums((long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x, ids, values, counts, W, cap, K, V, s_off,
                  field_l2, F, epi, [=](int64_t row) { if (stamp) stamp[row] = tag; });
}

// ==== The host launchers: one body per launch, behind the O1 entry points, their _lrdev twins (lr = 0, lr_dev the device rate) and
// the O7 entry points (lr AND lr_dev).  `who` names the entry point that was called.  AMSGrad needs `vhat` and the stamps; Adam's
// runs and merged updates take a mode.

// the dense launch: `kernel` walks descriptors of type T and moves `bytes` per element (28: p, g, m, v read, p, m, v written; 36
// with vhat)
template <typename T>
int adam_multi_launch(const char* who, const char* scope, double bytes,
                      void (*kernel)(const T*, int, const int64_t*, float, float, float, float, const float*), const T* tensors, int n,
                      int64_t total_numel, int64_t* step, float lr, const float* lr_dev, float beta_1, float beta_2, float epsilon,
                      int advance, void* stream) {
  FIL_CHECK_ARG_W(who, n >= 0 && total_numel >= 0);
  FIL_CHECK_ARG_W(who, step != nullptr);
  FIL_CHECK_ARG_W(who, n == 0 || tensors != nullptr);
  if (int rc = check_hyper(who, lr_dev ? 0.f : lr, beta_1, beta_2, epsilon)) return rc;
  if (advance != 0 && advance != 1) return fail(FIL_ERR_ARG, "%s: advance %d (0 or 1)", who, advance);
  hipStream_t st = (hipStream_t)stream;
  if (n > 0) {
    ProfScope ps(scope, st, bytes * (double)total_numel);
    const long chunks = std::max<long>(1, (long)((total_numel + kMultiChunk - 1) / kMultiChunk));
    const dim3 grid((int)std::min<long>(chunks, 256 * 8));
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, tensors, n, step, lr, beta_1, beta_2, epsilon, lr_dev);
    FIL_CHECK_LAUNCH_W(who);
  }
  if (advance) {
    launch_step_advance(step, st);
    FIL_CHECK_LAUNCH_W(who);
  }
  return FIL_OK;
}

template <bool kAms>
int embed_adam_runs_launch(const char* who, const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype,
                           int F, const float* field_l2, float* table, float* m, float* v, float* vhat, int32_t* stamp,
                           const int64_t* step, float lr, const float* lr_dev, float beta_1, float beta_2, float epsilon, int mode,
                           void* stream) {
  FIL_CHECK_ARG_W(who, R >= 0 && K >= 1 && F >= 1);
  if (g_dtype != FIL_F32 && g_dtype != FIL_BF16) return fail(FIL_ERR_ARG, "%s: g_dtype %d (f32 or bf16)", who, g_dtype);
  if (!kAms)
    if (int rc = check_mode(who, mode, stamp)) return rc;
  if (int rc = check_table_shape(who, K, 0)) return rc;
  if (int rc = check_hyper(who, lr_dev ? 0.f : lr, beta_1, beta_2, epsilon)) return rc;
  if (R == 0) return FIL_OK;
  FIL_CHECK_ARG_W(who, g && perm && sorted_ids && table && m && v && step);
  if (kAms) FIL_CHECK_ARG_W(who, vhat && stamp);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(kAms ? "embed_amsgrad_runs" : "embed_adam_runs", st,
               (double)R * K * (g_dtype == FIL_F32 ? 4 : 2) + (kAms ? 32.0 : 24.0) * R * K);
  const dim3 grid = run_sums_grid(R, K);
  int32_t* const stamps = (kAms || mode == FIL_ADAM_KERAS) ? stamp : nullptr;
  if (g_dtype == FIL_F32)
    hipLaunchKernelGGL((embed_adam_runs_kernel<kAms, float>), grid, dim3(256), 0, st, static_cast<const float*>(g), perm, sorted_ids, R,
                       K, F, field_l2, table, m, v, vhat, stamps, step, lr, beta_1, beta_2, epsilon, lr_dev);
  else
    hipLaunchKernelGGL((embed_adam_runs_kernel<kAms, __hip_bfloat16>), grid, dim3(256), 0, st, static_cast<const __hip_bfloat16*>(g),
                       perm, sorted_ids, R, K, F, field_l2, table, m, v, vhat, stamps, step, lr, beta_1, beta_2, epsilon, lr_dev);
  FIL_CHECK_LAUNCH_W(who);
  return FIL_OK;
}

template <bool kAms>
int embed_adam_sweep_launch(const char* who, float* table, float* m, float* v, float* vhat, const int32_t* stamp, int64_t V, int K,
                            const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F, const int64_t* step,
                            float lr, const float* lr_dev, float beta_1, float beta_2, float epsilon, void* stream) {
  FIL_CHECK_ARG_W(who, V >= 0 && K >= 1 && F >= 1);
  if (int rc = check_table_shape(who, 0, F)) return rc;
  if (int rc = check_hyper(who, lr_dev ? 0.f : lr, beta_1, beta_2, epsilon)) return rc;
  if (V == 0) return FIL_OK;
  FIL_CHECK_ARG_W(who, table && m && v && stamp && offsets && step);
  if (kAms) FIL_CHECK_ARG_W(who, vhat);
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = V * K;
  const int vec = sweep_vec(K, table, m, v) && (((uintptr_t)vhat & 15) == 0) ? 1 : 0;      // (Adam's NULL vhat is aligned)
  const int64_t work = vec ? n / 4 : n;
  ProfScope ps(kAms ? "embed_amsgrad_sweep" : "embed_adam_sweep", st, (kAms ? 32.0 : 24.0) * (double)n + 4.0 * (double)V);
  const dim3 grid = stride_grid(work);
  hipLaunchKernelGGL(embed_adam_sweep_kernel<kAms>, grid, dim3(256), 0, st, table, m, v, vhat, stamp, V, K, offsets, field_l2, frozen, F,
                     step, lr, beta_1, beta_2, epsilon, vec, lr_dev);
  FIL_CHECK_LAUNCH_W(who);
  return FIL_OK;
}

template <bool kAms>
int embed_adam_merged_launch(const char* who, const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                             const int64_t* offsets, const float* field_l2, int F, float* table, float* m, float* v, float* vhat,
                             int32_t* stamp, int64_t V, const int64_t* step, float lr, const float* lr_dev, float beta_1, float beta_2,
                             float epsilon, int mode, void* stream) {
  FIL_CHECK_ARG_W(who, W >= 1 && cap >= 0 && K >= 1 && F >= 1 && V >= 0);
  if (!kAms)
    if (int rc = check_mode(who, mode, stamp)) return rc;
  if (int rc = check_table_shape(who, K, F)) return rc;
  if (int rc = check_hyper(who, lr_dev ? 0.f : lr, beta_1, beta_2, epsilon)) return rc;
  if (cap == 0 || V == 0) return FIL_OK;
  FIL_CHECK_ARG_W(who, ids && values && counts && offsets && table && m && v && step);
  if (kAms) FIL_CHECK_ARG_W(who, vhat && stamp);
  hipStream_t st = (hipStream_t)stream;
  const long n = (long)W * cap;
  ProfScope ps(kAms ? "embed_amsgrad_merged" : "embed_adam_merged", st,
               8.0 * n + 4.0 * (double)n * K + (kAms ? 32.0 : 24.0) * (double)cap * K);
  const dim3 grid = stride_grid(n);
  hipLaunchKernelGGL(embed_adam_merged_kernel<kAms>, grid, dim3(256), 0, st, ids, values, counts, W, cap, K, offsets, field_l2, F, table,
                     m, v, vhat, (kAms || mode == FIL_ADAM_KERAS) ? stamp : nullptr, V, step, lr, beta_1, beta_2, epsilon, lr_dev);
  FIL_CHECK_LAUNCH_W(who);
  return FIL_OK;
}

}  // namespace fil
