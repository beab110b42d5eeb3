// O7  Keras' Adam(amsgrad=True) for gfx950: optim.hip's Keras-mode set -- the dense launch, the runs update, the sweep, the merged
// update -- each with a fourth array, the slot `vhat`.
//
// The rule is restated from TF 2.1 (ApplyAdamWithAmsgrad, and Adam._resource_apply_sparse with amsgrad), in fp32.  TensorFlow cannot
// be installed beside this project, so parity with it is unpinned, like the rest of oracle/:
//   t = step + 1;  alpha = lr sqrt(1 - b2^t) / (1 - b1^t)            (as O1: powf on the device from the int64 counter)
//   m += (g - m)(1 - b1);  v += (g^2 - v)(1 - b2)
//   vhat = (vhat < v) ? v : vhat                                      (Eigen's cwiseMax order: a NaN v leaves vhat; not fmaxf)
//   p -= (m alpha) / (sqrt(vhat) + eps)
// On a table Keras' sparse apply decays m and v over the whole variable, takes the max over the whole variable and moves every row:
// a touched row takes g = run sum + 2 l2[f] p, an untouched one g = 2 l2[f] p (0 without l2), a frozen field never changes.  An
// untouched row's v decays while its vhat holds, so the row keeps moving on the old, larger denominator.
//
// The table kernels form m and v through adam_touched / adam_untouched of optim_adam.h, Adam's own helpers (contraction off, explicit
// fmas): the table m and v of an amsgrad run are the bits of an Adam run on the same gradients.  amsgrad_move, beside them, is the
// vhat step and the move.  No lazy and no deferred mode: every runs update stamps, every step sweeps.
//
// The dense launch and the sweep stream: 16 bytes per lane and array where the arrays allow it (the sweep: 4 loads + 4 non-temporal
// stores of 16 B per lane, 32 bytes per element and step against Adam's 24), element-wise otherwise and in the tail.  The sweep
// skips a lane's vhat store when the bits it would write are the bits it read -- always so on an unregularised field, where an
// untouched row's v only decays: 28 bytes per element there (measured: 3.79 -> 3.38 ms at 33.8 M rows x K=16).  Every
// launch only READS the counter; fil_amsgrad_multi(advance = 1) bumps it in the one-thread launch behind its update.
#include "common.h"
#include "embed_runs.h"
#include "optim_rows.h"
#include "optim_adam.h"
#include <hip/hip_bf16.h>

namespace fil {

static_assert(sizeof(fil_amsgrad_tensor) == 56, "fil_amsgrad_tensor is 56 bytes (fil.h)");

// one element of ApplyAdamWithAmsgrad (Eigen's order of operations), left to the compiler's contraction like adam_elem: the dense
// tensors only
__device__ __forceinline__ void amsgrad_elem(float& p, float& m, float& v, float& vhat, float g, const AdamCoef& c) {
  m += (g - m) * c.omb1;
  v += (g * g - v) * c.omb2;
  vhat = (vhat < v) ? v : vhat;
  p -= (m * c.alpha) / (sqrtf(vhat) + c.eps);
}

// ---- fil_amsgrad_multi: multi_tensor_walk_slots (optim_rows.h) over the five-array descriptor: the same chunks, dealt the same way
__global__ __launch_bounds__(256) void amsgrad_multi_kernel(const fil_amsgrad_tensor* __restrict__ ts, int n,
                                                            const int64_t* __restrict__ step, float lr, float b1, float b2, float eps,
                                                            const float* __restrict__ lr_dev) {
  const AdamCoef c = adam_coef(step, rate_of(lr, lr_dev), b1, b2, eps);
  const long G = gridDim.x;
  long base = 0;
  for (int d = 0; d < n; ++d) {
    float* __restrict__ P = ts[d].param;
    const float* __restrict__ Gr = ts[d].grad;
    float* __restrict__ M = ts[d].m;
    float* __restrict__ V = ts[d].v;
    float* __restrict__ H = ts[d].vhat;
    const long numel = ts[d].numel;
    const float l2x2 = 2.f * ts[d].l2;
    const long nc = (numel + kMultiChunk - 1) / kMultiChunk;
    const bool vec = ((((uintptr_t)P | (uintptr_t)Gr | (uintptr_t)M | (uintptr_t)V | (uintptr_t)H) & 15) == 0);
    long r = ((long)blockIdx.x - base) % G;
    if (r < 0) r += G;
    for (long ch = r; ch < nc; ch += G) {
      const long e = ch * kMultiChunk + threadIdx.x * 4;
      if (vec && e + 4 <= numel) {
        f32x4 p = *reinterpret_cast<const f32x4*>(P + e);
        f32x4 g = Gr ? *reinterpret_cast<const f32x4*>(Gr + e) : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 m = *reinterpret_cast<const f32x4*>(M + e);
        f32x4 v = *reinterpret_cast<const f32x4*>(V + e);
        f32x4 h = *reinterpret_cast<const f32x4*>(H + e);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float pi = p[i], mi = m[i], vi = v[i], hi = h[i], gi = g[i];
          if (l2x2 != 0.f) gi += l2x2 * pi;
          amsgrad_elem(pi, mi, vi, hi, gi, c);
          p[i] = pi;
          m[i] = mi;
          v[i] = vi;
          h[i] = hi;
        }
        *reinterpret_cast<f32x4*>(P + e) = p;
        *reinterpret_cast<f32x4*>(M + e) = m;
        *reinterpret_cast<f32x4*>(V + e) = v;
        *reinterpret_cast<f32x4*>(H + e) = h;
      } else {
        for (long i = e; i < e + 4 && i < numel; ++i) {
          float p = P[i], m = M[i], v = V[i], h = H[i], g = Gr ? Gr[i] : 0.f;
          if (l2x2 != 0.f) g += l2x2 * p;
          amsgrad_elem(p, m, v, h, g, c);
          P[i] = p;
          M[i] = m;
          V[i] = v;
          H[i] = h;
        }
      }
    }
    base += nc;
  }
}

// one element of a touched row in place
__device__ __forceinline__ void amsgrad_touched_at(float* __restrict__ table, float* __restrict__ m, float* __restrict__ v,
                                                   float* __restrict__ vhat, int64_t e, float acc, float l2x2, const AdamCoef& c) {
  float p = table[e], mm = m[e], vv = v[e], hh = vhat[e];
  amsgrad_touched(p, mm, vv, hh, acc, l2x2, c);
  table[e] = p;
  m[e] = mm;
  v[e] = vv;
  vhat[e] = hh;
}

// ---- fil_embed_amsgrad_runs: the run sums of embed_runs.h with the rule as epilogue, as embed_adam_runs_kernel in Keras mode; the
// rows it updates are stamped with the step's tag
template <typename GT>
__global__ __launch_bounds__(256) void embed_amsgrad_runs_kernel(const GT* __restrict__ g, const int64_t* __restrict__ perm,
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
      if (kq * 4 + i < K) amsgrad_touched_at(table, m, v, vhat, row * K + kq * 4 + i, acc[i], l2x2, c);
    if (kq == 0) stamp[row] = tag;
  });
}

// ---- fil_embed_amsgrad_sweep: every row the run pass did not stamp at this step, of every non-frozen field, takes g = 2 l2[f] p
// (or 0): embed_adam_sweep_kernel with the fourth array, whose store is skipped where it would write back the bits it read
__global__ __launch_bounds__(256) void embed_amsgrad_sweep_kernel(float* __restrict__ table, float* __restrict__ m, float* __restrict__ v,
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
      f32x4 hh = reinterpret_cast<const f32x4*>(vhat)[q];
      bool held = true;                       // the lane's four vhat keep their bits (an unregularised field: always)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float pi = p[i], mi = mm[i], vi = vv[i], hi = hh[i];
        amsgrad_untouched<true>(pi, mi, vi, hi, l2x2, c);
        held = held && __float_as_uint(hi) == __float_as_uint(hh[i]);
        p[i] = pi;
        mm[i] = mi;
        vv[i] = vi;
        hh[i] = hi;
      }
      __builtin_nontemporal_store(p, reinterpret_cast<f32x4*>(table) + q);
      __builtin_nontemporal_store(mm, reinterpret_cast<f32x4*>(m) + q);
      __builtin_nontemporal_store(vv, reinterpret_cast<f32x4*>(v) + q);
      if (!held) __builtin_nontemporal_store(hh, reinterpret_cast<f32x4*>(vhat) + q);
    }
    return;
  }
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const int64_t row = e / K;
    if (stamp[row] == tag) continue;
    const float l2x2 = field_l2x2(&s, F, row);
    if (l2x2 != l2x2) continue;
    float p = table[e], mm = m[e], vv = v[e], hh = vhat[e];
    const float h0 = hh;
    amsgrad_untouched<false>(p, mm, vv, hh, l2x2, c);
    __builtin_nontemporal_store(p, table + e);
    __builtin_nontemporal_store(mm, m + e);
    __builtin_nontemporal_store(vv, v + e);
    if (__float_as_uint(hh) != __float_as_uint(h0)) __builtin_nontemporal_store(hh, vhat + e);
  }
}

// ---- fil_embed_amsgrad_merged: the merged walk of the gathered lists (merged_row_sums, optim_rows.h); the owner of a row adds the
// field's l2 term and updates the row exactly as embed_amsgrad_runs_kernel does
__global__ __launch_bounds__(256) void embed_amsgrad_merged_kernel(const int64_t* __restrict__ ids, const float* __restrict__ values,
                                                                   const int64_t* __restrict__ counts, int W, long cap, int K,
                                                                   const int64_t* __restrict__ offsets,
                                                                   const float* __restrict__ field_l2, int F, float* __restrict__ table,
                                                                   float* __restrict__ m, float* __restrict__ v, float* __restrict__ vhat,
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
      if (k0 + e < K) amsgrad_touched_at(table, m, v, vhat, row * K + k0 + e, acc[e], l2x2, c);
  };
  merged_row_sums((long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x, ids, values, counts, W, cap, K, V, s_off,
                  field_l2, F, epi, [=](int64_t row) { stamp[row] = tag; });
}

}  // namespace fil

using namespace fil;

extern "C" int fil_amsgrad_multi(const fil_amsgrad_tensor* tensors, int n, int64_t total_numel, int64_t* step, float lr,
                                 const float* lr_dev, float beta_1, float beta_2, float epsilon, int advance, void* stream) {
  const char* who = "fil_amsgrad_multi";
  FIL_CHECK_ARG_W(who, n >= 0 && total_numel >= 0);
  FIL_CHECK_ARG_W(who, step != nullptr);
  FIL_CHECK_ARG_W(who, n == 0 || tensors != nullptr);
  if (int rc = check_hyper(who, lr_dev ? 0.f : lr, beta_1, beta_2, epsilon)) return rc;
  if (advance != 0 && advance != 1) return fail(FIL_ERR_ARG, "%s: advance %d (0 or 1)", who, advance);
  hipStream_t st = (hipStream_t)stream;
  if (n > 0) {
    ProfScope ps("amsgrad_multi", st, 36.0 * (double)total_numel);
    const long chunks = std::max<long>(1, (long)((total_numel + kMultiChunk - 1) / kMultiChunk));
    const dim3 grid((int)std::min<long>(chunks, 256 * 8));
    hipLaunchKernelGGL(amsgrad_multi_kernel, grid, dim3(256), 0, st, tensors, n, step, lr, beta_1, beta_2, epsilon, lr_dev);
    FIL_CHECK_LAUNCH_W(who);
  }
  if (advance) {
    launch_step_advance(step, st);
    FIL_CHECK_LAUNCH_W(who);
  }
  return FIL_OK;
}

extern "C" int fil_embed_amsgrad_runs(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                      const float* field_l2, float* table, float* m, float* v, float* vhat, int32_t* stamp,
                                      const int64_t* step, float lr, const float* lr_dev, float beta_1, float beta_2, float epsilon,
                                      void* stream) {
  const char* who = "fil_embed_amsgrad_runs";
  FIL_CHECK_ARG_W(who, R >= 0 && K >= 1 && F >= 1);
  if (g_dtype != FIL_F32 && g_dtype != FIL_BF16) return fail(FIL_ERR_ARG, "%s: g_dtype %d (f32 or bf16)", who, g_dtype);
  if (int rc = check_table_shape(who, K, 0)) return rc;
  if (int rc = check_hyper(who, lr_dev ? 0.f : lr, beta_1, beta_2, epsilon)) return rc;
  if (R == 0) return FIL_OK;
  FIL_CHECK_ARG_W(who, g && perm && sorted_ids && table && m && v && vhat && stamp && step);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("embed_amsgrad_runs", st, (double)R * K * (g_dtype == FIL_F32 ? 4 : 2) + 32.0 * R * K);
  const dim3 grid = run_sums_grid(R, K);
  if (g_dtype == FIL_F32)
    hipLaunchKernelGGL(embed_amsgrad_runs_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(g), perm, sorted_ids, R, K, F,
                       field_l2, table, m, v, vhat, stamp, step, lr, beta_1, beta_2, epsilon, lr_dev);
  else
    hipLaunchKernelGGL(embed_amsgrad_runs_kernel<__hip_bfloat16>, grid, dim3(256), 0, st, static_cast<const __hip_bfloat16*>(g), perm,
                       sorted_ids, R, K, F, field_l2, table, m, v, vhat, stamp, step, lr, beta_1, beta_2, epsilon, lr_dev);
  FIL_CHECK_LAUNCH_W(who);
  return FIL_OK;
}

extern "C" int fil_embed_amsgrad_sweep(float* table, float* m, float* v, float* vhat, const int32_t* stamp, int64_t V, int K,
                                       const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F,
                                       const int64_t* step, float lr, const float* lr_dev, float beta_1, float beta_2, float epsilon,
                                       void* stream) {
  const char* who = "fil_embed_amsgrad_sweep";
  FIL_CHECK_ARG_W(who, V >= 0 && K >= 1 && F >= 1);
  if (int rc = check_table_shape(who, 0, F)) return rc;
  if (int rc = check_hyper(who, lr_dev ? 0.f : lr, beta_1, beta_2, epsilon)) return rc;
  if (V == 0) return FIL_OK;
  FIL_CHECK_ARG_W(who, table && m && v && vhat && stamp && offsets && step);
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = V * K;
  const int vec = sweep_vec(K, table, m, v) && (((uintptr_t)vhat & 15) == 0) ? 1 : 0;
  const int64_t work = vec ? n / 4 : n;
  ProfScope ps("embed_amsgrad_sweep", st, 32.0 * (double)n + 4.0 * (double)V);
  const dim3 grid = stride_grid(work);
  hipLaunchKernelGGL(embed_amsgrad_sweep_kernel, grid, dim3(256), 0, st, table, m, v, vhat, stamp, V, K, offsets, field_l2, frozen, F,
                     step, lr, beta_1, beta_2, epsilon, vec, lr_dev);
  FIL_CHECK_LAUNCH_W(who);
  return FIL_OK;
}

extern "C" int fil_embed_amsgrad_merged(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                        const int64_t* offsets, const float* field_l2, int F, float* table, float* m, float* v,
                                        float* vhat, int32_t* stamp, int64_t V, const int64_t* step, float lr, const float* lr_dev,
                                        float beta_1, float beta_2, float epsilon, void* stream) {
  const char* who = "fil_embed_amsgrad_merged";
  FIL_CHECK_ARG_W(who, W >= 1 && cap >= 0 && K >= 1 && F >= 1 && V >= 0);
  if (int rc = check_table_shape(who, K, F)) return rc;
  if (int rc = check_hyper(who, lr_dev ? 0.f : lr, beta_1, beta_2, epsilon)) return rc;
  if (cap == 0 || V == 0) return FIL_OK;
  FIL_CHECK_ARG_W(who, ids && values && counts && offsets && table && m && v && vhat && stamp && step);
  hipStream_t st = (hipStream_t)stream;
  const long n = (long)W * cap;
  ProfScope ps("embed_amsgrad_merged", st, 8.0 * n + 4.0 * (double)n * K + 32.0 * (double)cap * K);
  const dim3 grid = stride_grid(n);
  hipLaunchKernelGGL(embed_amsgrad_merged_kernel, grid, dim3(256), 0, st, ids, values, counts, W, cap, K, offsets, field_l2, F, table, m,
                     v, vhat, stamp, V, step, lr, beta_1, beta_2, epsilon, lr_dev);
  FIL_CHECK_LAUNCH_W(who);
  return FIL_OK;
}
