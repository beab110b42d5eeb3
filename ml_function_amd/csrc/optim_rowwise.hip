// O2  Keras-exact Adagrad and Ftrl for gfx950: every dense fp32 tensor of a model in one launch, and the embedding tables updated in
// place from the batch's gradient runs (no dense [V,K] gradient), as optim.hip does for Adam.
//
// The updates are TF 2.1's ApplyAdagradV2 and ApplyFtrl / ApplyFtrlV2 functors in fp32 (Keras' Adagrad and Ftrl drive them):
//   Adagrad  acc += g g;  p -= g lr / (sqrt(acc) + eps)
//   Ftrl     gs = g + 2 l2_shrinkage p;  n' = n + g g;  sigma = (n'^-lr_power - n^-lr_power) / lr  (sqrt for lr_power = -0.5);
//            z += gs - sigma p;  q = n'^-lr_power / lr + 2 l2;  p = |z| > l1 ? (sign(z) l1 - z) / q : 0;  n = n'
// Neither rule depends on the step, and a row with g = 0 under Adagrad keeps its bits: so Keras' semantics are the batch's rows plus,
// where Keras really updates every row (a field with l2(emb_reg) > 0: a dense regulariser gradient), one sweep over those fields'
// rows only.  The rule functions are written with contraction off: every kernel below rounds a row's update the same way, so the
// merged data-parallel update at W = 1 is bit-identical to the runs update, and the untouched-row update is one definition.
#include "common.h"
#include "embed_runs.h"
#include "optim_rows.h"
#include <hip/hip_bf16.h>

namespace fil {

struct RowHyper {
  float lr, eps, lr_power, l1, l2x2, shrink2;   // shrink2 = 2 l2_shrinkage, l2x2 = 2 l2 (Ftrl's, not a field's regulariser)
  int sqrt_power;                               // lr_power == -0.5: sqrtf instead of powf (TF's special case)
};

static RowHyper row_hyper(const fil_rowopt_hyper& h) {
  RowHyper r;
  r.lr = h.lr;
  r.eps = h.epsilon;
  r.lr_power = h.lr_power;
  r.l1 = h.l1;
  r.l2x2 = 2.f * h.l2;
  r.shrink2 = 2.f * h.l2_shrinkage;
  r.sqrt_power = h.lr_power == -0.5f ? 1 : 0;
  return r;
}

// (the *_lrdev entry points: the kernels take the rate from the word fil_lr_schedule_eval left on the device, `if (lr_dev) h.lr =
// *lr_dev` -- one wave-uniform load at the top of each kernel; a by-value launch passes NULL)
// one element of the rule: s = the accumulator, z = Ftrl's linear slot (unused by Adagrad)
template <int RULE>
__device__ __forceinline__ void rule_elem(float& p, float& s, float& z, float g, const RowHyper& h) {
#pragma clang fp contract(off)
  if constexpr (RULE == FIL_OPT_ADAGRAD) {
    s = s + g * g;
    p = p - g * h.lr / (sqrtf(s) + h.eps);
  } else {
    const float gs = h.shrink2 != 0.f ? g + h.shrink2 * p : g;
    const float n1 = s + g * g;
    const float a1 = h.sqrt_power ? sqrtf(n1) : powf(n1, -h.lr_power);
    const float a0 = h.sqrt_power ? sqrtf(s) : powf(s, -h.lr_power);
    const float sigma = (a1 - a0) / h.lr;
    z = z + (gs - sigma * p);
    const float q = a1 / h.lr + h.l2x2;
    p = fabsf(z) > h.l1 ? (copysignf(h.l1, z) - z) / q : 0.f;
    s = n1;
  }
}

// ---- fil_rowopt_multi: the dense descriptors (multi_tensor_walk, optim_rows.h) with the rule; Ftrl's linear slot (`v`) joins the
// 16-byte alignment test, Adagrad has none
template <int RULE>
__global__ __launch_bounds__(256) void rowopt_multi_kernel(const fil_adam_tensor* __restrict__ ts, int n, RowHyper h,
                                                           const float* __restrict__ lr_dev) {
  if (lr_dev) h.lr = *lr_dev;
  multi_tensor_walk<RULE == FIL_OPT_FTRL>(ts, n, [=](float& p, float& s, float& z, float g, float l2x2) {
    rule_elem<RULE>(p, s, z, with_l2(g, l2x2, p), h);
  });
}

// one row's K elements (this lane's quad kq) with g = acc + 2 l2 p
template <int RULE>
__device__ __forceinline__ void rule_row_quad(float* __restrict__ table, float* __restrict__ S, float* __restrict__ Z, int64_t row,
                                              int K, int kq, const float (&acc)[4], float l2x2, const RowHyper& h) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (kq * 4 + i < K) {
      const int64_t e = row * K + kq * 4 + i;
      float p = table[e], s = S[e], z = RULE == FIL_OPT_FTRL ? Z[e] : 0.f;
      rule_elem<RULE>(p, s, z, with_l2(acc[i], l2x2, p), h);
      table[e] = p;
      S[e] = s;
      if (RULE == FIL_OPT_FTRL) Z[e] = z;
    }
  }
}

// ---- fil_embed_rowopt_runs: the run sums of embed_runs.h with the rule as epilogue.  The run of row `row`, field f = perm % F, takes
// g = run sum + 2 field_l2[f] p; the row is stamped with t when a sweep follows (stamp != NULL).
template <int RULE, typename GT>
__global__ __launch_bounds__(256) void embed_rowopt_runs_kernel(const GT* __restrict__ g, const int64_t* __restrict__ perm,
                                                                const int64_t* __restrict__ sorted_ids, long R, int K, int F,
                                                                const float* __restrict__ field_l2, float* __restrict__ table,
                                                                float* __restrict__ S, float* __restrict__ Z, int32_t* __restrict__ stamp,
                                                                const int64_t* __restrict__ step, RowHyper h,
                                                                const float* __restrict__ lr_dev) {
  if (lr_dev) h.lr = *lr_dev;
  const int32_t tag = stamp ? (int32_t)(uint32_t)(*step + 1) : 0;
  embed_run_sums(g, perm, sorted_ids, R, K, [=](int64_t row, int kq, const float (&acc)[4], int64_t first) {
    const float l2x2 = field_l2 ? 2.f * field_l2[first % F] : 0.f;
    rule_row_quad<RULE>(table, S, Z, row, K, kq, acc, l2x2, h);
    if (stamp && kq == 0) stamp[row] = tag;
  });
}

// ---- fil_embed_rowopt_sweep.  Only the rows of regularised, non-frozen fields move when untouched, so the grid walks those fields'
// rows only: every workgroup compacts the field table in LDS into "virtual" row ranges (an integer scan over F <= 1024 fields, a
// few hundred cycles) and strides over the virtual rows; a virtual row maps back to its table row by a binary search.  The grid is
// sized by the table (no data-dependent size: capturable); workgroups past the regularised rows leave at once.
template <int RULE>
__global__ __launch_bounds__(256) void embed_rowopt_sweep_kernel(float* __restrict__ table, float* __restrict__ S, float* __restrict__ Z,
                                                                 const int32_t* __restrict__ stamp, int64_t V, int K,
                                                                 const int64_t* __restrict__ offsets, const float* __restrict__ field_l2,
                                                                 const unsigned char* __restrict__ frozen, int F,
                                                                 const int64_t* __restrict__ step, RowHyper h, int vec,
                                                                 const float* __restrict__ lr_dev) {
  constexpr bool kZ = RULE == FIL_OPT_FTRL;
  if (lr_dev) h.lr = *lr_dev;
  __shared__ RegTab t;
  load_reg_tab(&t, offsets, field_l2, frozen, F, V);
  const int64_t n = t.vbeg[t.n] * K;               // elements of the regularised fields
  const int32_t tag = (int32_t)(uint32_t)(*step + 1);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (vec) {                                        // K % 4 == 0 and 16-byte aligned arrays: a lane moves 4 elements of one row
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n / 4; q += stride) {
      const int64_t vr = q * 4 / K;
      const int c = reg_field(&t, vr);
      const int64_t row = t.rbeg[c] + (vr - t.vbeg[c]);
      const float l2x2 = t.l2x2[c];
      const int64_t e = row * K + (q * 4 - vr * K);
      if (stamp[row] == tag) continue;
      f32x4 p = *reinterpret_cast<const f32x4*>(table + e);
      f32x4 s = *reinterpret_cast<const f32x4*>(S + e);
      f32x4 z = kZ ? *reinterpret_cast<const f32x4*>(Z + e) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float pi = p[i], si = s[i], zi = z[i];
        rule_elem<RULE>(pi, si, zi, with_l2(0.f, l2x2, pi), h);
        p[i] = pi;
        s[i] = si;
        z[i] = zi;
      }
      __builtin_nontemporal_store(p, reinterpret_cast<f32x4*>(table + e));
      __builtin_nontemporal_store(s, reinterpret_cast<f32x4*>(S + e));
      if (kZ) __builtin_nontemporal_store(z, reinterpret_cast<f32x4*>(Z + e));
    }
    return;
  }
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += stride) {
    const int64_t vr = x / K;
    const int c = reg_field(&t, vr);
    const int64_t row = t.rbeg[c] + (vr - t.vbeg[c]);
    if (stamp[row] == tag) continue;
    const int64_t e = row * K + (x - vr * K);
    float p = table[e], s = S[e], z = kZ ? Z[e] : 0.f;
    rule_elem<RULE>(p, s, z, with_l2(0.f, t.l2x2[c], p), h);
    __builtin_nontemporal_store(p, table + e);
    __builtin_nontemporal_store(s, S + e);
    if (kZ) __builtin_nontemporal_store(z, Z + e);
  }
}

// ---- fil_embed_rowopt_merged: the merged walk of the gathered lists (merged_row_sums, optim_rows.h) with the rule
template <int RULE>
__global__ __launch_bounds__(256) void embed_rowopt_merged_kernel(const int64_t* __restrict__ ids, const float* __restrict__ values,
                                                                  const int64_t* __restrict__ counts, int W, long cap, int K,
                                                                  const int64_t* __restrict__ offsets, const float* __restrict__ field_l2,
                                                                  int F, float* __restrict__ table, float* __restrict__ S,
                                                                  float* __restrict__ Z, int32_t* __restrict__ stamp, int64_t V,
                                                                  const int64_t* __restrict__ step, RowHyper h,
                                                                  const float* __restrict__ lr_dev) {
  if (lr_dev) h.lr = *lr_dev;
  __shared__ int64_t s_off[kSweepMaxF];
  for (int f = threadIdx.x; f < F; f += blockDim.x) s_off[f] = offsets[f];
  __syncthreads();
  const int32_t tag = stamp ? (int32_t)(uint32_t)(*step + 1) : 0;
  const auto epi = [=](int64_t row, int f, float l2x2, int k0, const float (&acc)[kMergeChunk]) {
#pragma unroll
    for (int e = 0; e < kMergeChunk; ++e) {
      if (k0 + e < K) {
        const int64_t x = row * K + k0 + e;
        float p = table[x], s = S[x], z = RULE == FIL_OPT_FTRL ? Z[x] : 0.f;
        rule_elem<RULE>(p, s, z, with_l2(acc[e], l2x2, p), h);
        table[x] = p;
        S[x] = s;
        if (RULE == FIL_OPT_FTRL) Z[x] = z;
      }
    }
  };
  merged_row_sums((long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x, ids, values, counts, W, cap, K, V, s_off,
                  field_l2, F, epi, [=](int64_t row) { if (stamp) stamp[row] = tag; });
}

// the rule and its hyper-parameters (read here, on the host: a captured launch keeps the values it was captured with)
static int check_rule(const char* who, int rule, const fil_rowopt_hyper* h) {
  if (rule != FIL_OPT_ADAGRAD && rule != FIL_OPT_FTRL)
    return fail(FIL_ERR_ARG, "%s: rule %d (FIL_OPT_ADAGRAD or FIL_OPT_FTRL)", who, rule);
  if (h == nullptr) return fail(FIL_ERR_ARG, "%s: no hyper-parameters (hyper is NULL)", who);
  if (rule == FIL_OPT_ADAGRAD && (!(h->lr >= 0.f) || !(h->epsilon >= 0.f)))
    return fail(FIL_ERR_ARG, "%s: Adagrad hyper-parameters lr=%g epsilon=%g (both >= 0)", who, (double)h->lr, (double)h->epsilon);
  if (rule == FIL_OPT_FTRL && (!(h->lr >= 0.f) || !(h->lr_power <= 0.f) || !(h->l1 >= 0.f) || !(h->l2 >= 0.f) || !(h->l2_shrinkage >= 0.f)))
    return fail(FIL_ERR_ARG, "%s: Ftrl hyper-parameters lr=%g lr_power=%g l1=%g l2=%g l2_shrinkage=%g (lr_power <= 0, the others >= 0)",
                who, (double)h->lr, (double)h->lr_power, (double)h->l1, (double)h->l2, (double)h->l2_shrinkage);
  return FIL_OK;
}

// the arrays one element of a rule moves (param, accumulator, linear for Ftrl)
static double rule_arrays(int rule) { return rule == FIL_OPT_FTRL ? 3.0 : 2.0; }

}  // namespace fil

using namespace fil;

static int rowopt_multi_impl(const char* who, const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule,
                                const fil_rowopt_hyper* hyper, int advance, void* stream, const float* lr_dev) {
  FIL_CHECK_ARG_W(who, n >= 0 && total_numel >= 0);
  FIL_CHECK_ARG_W(who, step != nullptr);
  FIL_CHECK_ARG_W(who, n == 0 || tensors != nullptr);
  if (int rc = check_rule(who, rule, hyper)) return rc;
  if (advance != 0 && advance != 1) return fail(FIL_ERR_ARG, "%s: advance %d (0 or 1)", who, advance);
  hipStream_t st = (hipStream_t)stream;
  const RowHyper h = row_hyper(*hyper);
  if (n > 0) {
    ProfScope ps(rule == FIL_OPT_FTRL ? "ftrl_multi" : "adagrad_multi", st, (4.0 + 8.0 * rule_arrays(rule)) * (double)total_numel);
    const long chunks = std::max<long>(1, (long)((total_numel + kMultiChunk - 1) / kMultiChunk));
    const dim3 grid((int)std::min<long>(chunks, 256 * 8));
    if (rule == FIL_OPT_FTRL) hipLaunchKernelGGL(rowopt_multi_kernel<FIL_OPT_FTRL>, grid, dim3(256), 0, st, tensors, n, h, lr_dev);
    else hipLaunchKernelGGL(rowopt_multi_kernel<FIL_OPT_ADAGRAD>, grid, dim3(256), 0, st, tensors, n, h, lr_dev);
    FIL_CHECK_LAUNCH_W(who);
  }
  if (advance) {
    launch_step_advance(step, st);
    FIL_CHECK_LAUNCH_W(who);
  }
  return FIL_OK;
}

extern "C" int fil_rowopt_multi(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule,
                                const fil_rowopt_hyper* hyper, int advance, void* stream) {
  return rowopt_multi_impl("fil_rowopt_multi", tensors, n, total_numel, step, rule, hyper, advance, stream, nullptr);
}

extern "C" int fil_rowopt_multi_lrdev(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule,
                                const fil_rowopt_hyper* hyper, const float* lr_dev, int advance, void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_rowopt_multi_lrdev: no device rate (lr_dev is NULL)");
  return rowopt_multi_impl("fil_rowopt_multi_lrdev", tensors, n, total_numel, step, rule, hyper, advance, stream, lr_dev);
}

static int embed_rowopt_runs_impl(const char* who, const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype,
                                  int F,
                                     const float* field_l2, float* table, float* accum, float* linear, int32_t* stamp,
                                     const int64_t* step, int rule, const fil_rowopt_hyper* hyper, void* stream, const float* lr_dev) {
  FIL_CHECK_ARG_W(who, R >= 0 && K >= 1 && F >= 1);
  if (g_dtype != FIL_F32 && g_dtype != FIL_BF16) return fail(FIL_ERR_ARG, "%s: g_dtype %d (f32 or bf16)", who, g_dtype);
  if (K > 256) return fail(FIL_ERR_UNSUPPORTED, "%s: K=%d > 256", who, K);
  if (int rc = check_rule(who, rule, hyper)) return rc;
  if (R == 0) return FIL_OK;
  FIL_CHECK_ARG_W(who, g && perm && sorted_ids && table && accum && step);
  if (rule == FIL_OPT_FTRL && linear == nullptr) return fail(FIL_ERR_ARG, "%s: Ftrl needs its linear slot", who);
  hipStream_t st = (hipStream_t)stream;
  const RowHyper h = row_hyper(*hyper);
  ProfScope ps(rule == FIL_OPT_FTRL ? "embed_ftrl_runs" : "embed_adagrad_runs", st,
               (double)R * K * (g_dtype == FIL_F32 ? 4 : 2) + 8.0 * rule_arrays(rule) * R * K);
  const int C = 64 / ((K + 3) / 4);
  const dim3 grid((int)std::min<long>((R + 4 * C - 1) / (4 * C), 256 * 32));
  float* Z = rule == FIL_OPT_FTRL ? linear : nullptr;
#define FIL_ROWOPT_RUNS(RULE, GT) \
  hipLaunchKernelGGL((embed_rowopt_runs_kernel<RULE, GT>), grid, dim3(256), 0, st, static_cast<const GT*>(g), perm, sorted_ids, R, K, F, \
                     field_l2, table, accum, Z, stamp, step, h, lr_dev)
  if (rule == FIL_OPT_FTRL) {
    if (g_dtype == FIL_F32) FIL_ROWOPT_RUNS(FIL_OPT_FTRL, float);
    else FIL_ROWOPT_RUNS(FIL_OPT_FTRL, __hip_bfloat16);
  } else {
    if (g_dtype == FIL_F32) FIL_ROWOPT_RUNS(FIL_OPT_ADAGRAD, float);
    else FIL_ROWOPT_RUNS(FIL_OPT_ADAGRAD, __hip_bfloat16);
  }
#undef FIL_ROWOPT_RUNS
  FIL_CHECK_LAUNCH_W(who);
  return FIL_OK;
}

extern "C" int fil_embed_rowopt_runs(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                     const float* field_l2, float* table, float* accum, float* linear, int32_t* stamp,
                                     const int64_t* step, int rule, const fil_rowopt_hyper* hyper, void* stream) {
  return embed_rowopt_runs_impl("fil_embed_rowopt_runs", g, perm, sorted_ids, R, K, g_dtype, F, field_l2, table, accum, linear, stamp, step,
                                rule, hyper, stream, nullptr);
}

extern "C" int fil_embed_rowopt_runs_lrdev(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                     const float* field_l2, float* table, float* accum, float* linear, int32_t* stamp,
                                     const int64_t* step, int rule, const fil_rowopt_hyper* hyper, const float* lr_dev, void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_rowopt_runs_lrdev: no device rate (lr_dev is NULL)");
  return embed_rowopt_runs_impl("fil_embed_rowopt_runs_lrdev", g, perm, sorted_ids, R, K, g_dtype, F, field_l2, table, accum, linear, stamp,
                                step, rule, hyper, stream, lr_dev);
}

static int embed_rowopt_sweep_impl(const char* who, float* table, float* accum, float* linear, const int32_t* stamp, int64_t V, int K,
                                      const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F,
                                      const int64_t* step, int rule, const fil_rowopt_hyper* hyper, void* stream, const float* lr_dev) {
  FIL_CHECK_ARG_W(who, V >= 0 && K >= 1 && F >= 1);
  if (F > kSweepMaxF) return fail(FIL_ERR_UNSUPPORTED, "%s: F=%d > %d fields", who, F, kSweepMaxF);
  if (int rc = check_rule(who, rule, hyper)) return rc;
  if (V == 0 || field_l2 == nullptr) return FIL_OK;          // no regularised field: no untouched row moves
  FIL_CHECK_ARG_W(who, table && accum && stamp && offsets && step);
  if (rule == FIL_OPT_FTRL && linear == nullptr) return fail(FIL_ERR_ARG, "%s: Ftrl needs its linear slot", who);
  hipStream_t st = (hipStream_t)stream;
  const RowHyper h = row_hyper(*hyper);
  float* Z = rule == FIL_OPT_FTRL ? linear : nullptr;
  const int64_t n = V * K;
  const int vec = (K % 4 == 0 && ((((uintptr_t)table | (uintptr_t)accum | (uintptr_t)Z) & 15) == 0)) ? 1 : 0;
  const int64_t work = vec ? n / 4 : n;
  // (bytes of a whole-table sweep: the kernel moves only the regularised fields' share of them)
  ProfScope ps(rule == FIL_OPT_FTRL ? "embed_ftrl_sweep" : "embed_adagrad_sweep", st, 8.0 * rule_arrays(rule) * (double)n + 4.0 * (double)V);
  const dim3 grid((int)std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, 256 * 8)));
  if (rule == FIL_OPT_FTRL)
    hipLaunchKernelGGL(embed_rowopt_sweep_kernel<FIL_OPT_FTRL>, grid, dim3(256), 0, st, table, accum, Z, stamp, V, K, offsets, field_l2,
                       frozen, F, step, h, vec, lr_dev);
  else
    hipLaunchKernelGGL(embed_rowopt_sweep_kernel<FIL_OPT_ADAGRAD>, grid, dim3(256), 0, st, table, accum, Z, stamp, V, K, offsets,
                       field_l2, frozen, F, step, h, vec, lr_dev);
  FIL_CHECK_LAUNCH_W(who);
  return FIL_OK;
}

extern "C" int fil_embed_rowopt_sweep(float* table, float* accum, float* linear, const int32_t* stamp, int64_t V, int K,
                                      const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F,
                                      const int64_t* step, int rule, const fil_rowopt_hyper* hyper, void* stream) {
  return embed_rowopt_sweep_impl("fil_embed_rowopt_sweep", table, accum, linear, stamp, V, K, offsets, field_l2, frozen, F, step, rule,
                                 hyper, stream, nullptr);
}

extern "C" int fil_embed_rowopt_sweep_lrdev(float* table, float* accum, float* linear, const int32_t* stamp, int64_t V, int K,
                                      const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F,
                                      const int64_t* step, int rule, const fil_rowopt_hyper* hyper, const float* lr_dev, void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_rowopt_sweep_lrdev: no device rate (lr_dev is NULL)");
  return embed_rowopt_sweep_impl("fil_embed_rowopt_sweep_lrdev", table, accum, linear, stamp, V, K, offsets, field_l2, frozen, F, step, rule,
                                 hyper, stream, lr_dev);
}

static int embed_rowopt_merged_impl(const char* who, const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                       const int64_t* offsets, const float* field_l2, int F, float* table, float* accum, float* linear,
                                       int32_t* stamp, int64_t V, const int64_t* step, int rule, const fil_rowopt_hyper* hyper,
                                       void* stream, const float* lr_dev) {
  FIL_CHECK_ARG_W(who, W >= 1 && cap >= 0 && K >= 1 && F >= 1 && V >= 0);
  if (K > 256) return fail(FIL_ERR_UNSUPPORTED, "%s: K=%d > 256", who, K);
  if (F > kSweepMaxF) return fail(FIL_ERR_UNSUPPORTED, "%s: F=%d > %d fields", who, F, kSweepMaxF);
  if (int rc = check_rule(who, rule, hyper)) return rc;
  if (cap == 0 || V == 0) return FIL_OK;
  FIL_CHECK_ARG_W(who, ids && values && counts && offsets && table && accum && step);
  if (rule == FIL_OPT_FTRL && linear == nullptr) return fail(FIL_ERR_ARG, "%s: Ftrl needs its linear slot", who);
  hipStream_t st = (hipStream_t)stream;
  const RowHyper h = row_hyper(*hyper);
  float* Z = rule == FIL_OPT_FTRL ? linear : nullptr;
  const long n = (long)W * cap;
  ProfScope ps(rule == FIL_OPT_FTRL ? "embed_ftrl_merged" : "embed_adagrad_merged", st,
               8.0 * n + 4.0 * (double)n * K + 8.0 * rule_arrays(rule) * (double)cap * K);
  const dim3 grid((int)std::max<long>(1, std::min<long>((n + 255) / 256, 256 * 8)));
  if (rule == FIL_OPT_FTRL)
    hipLaunchKernelGGL(embed_rowopt_merged_kernel<FIL_OPT_FTRL>, grid, dim3(256), 0, st, ids, values, counts, W, cap, K, offsets, field_l2,
                       F, table, accum, Z, stamp, V, step, h, lr_dev);
  else
    hipLaunchKernelGGL(embed_rowopt_merged_kernel<FIL_OPT_ADAGRAD>, grid, dim3(256), 0, st, ids, values, counts, W, cap, K, offsets,
                       field_l2, F, table, accum, Z, stamp, V, step, h, lr_dev);
  FIL_CHECK_LAUNCH_W(who);
  return FIL_OK;
}

extern "C" int fil_embed_rowopt_merged(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                       const int64_t* offsets, const float* field_l2, int F, float* table, float* accum, float* linear,
                                       int32_t* stamp, int64_t V, const int64_t* step, int rule, const fil_rowopt_hyper* hyper,
                                       void* stream) {
  return embed_rowopt_merged_impl("fil_embed_rowopt_merged", ids, values, counts, W, cap, K, offsets, field_l2, F, table, accum, linear,
                                  stamp, V, step, rule, hyper, stream, nullptr);
}

extern "C" int fil_embed_rowopt_merged_lrdev(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                       const int64_t* offsets, const float* field_l2, int F, float* table, float* accum, float* linear,
                                       int32_t* stamp, int64_t V, const int64_t* step, int rule, const fil_rowopt_hyper* hyper, const float* lr_dev,
                                       void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_rowopt_merged_lrdev: no device rate (lr_dev is NULL)");
  return embed_rowopt_merged_impl("fil_embed_rowopt_merged_lrdev", ids, values, counts, W, cap, K, offsets, field_l2, F, table, accum,
                                  linear, stamp, V, step, rule, hyper, stream, lr_dev);
}
