// O4  Keras-exact SGD (plain, momentum, Nesterov) and RMSprop for gfx950: every dense fp32 tensor of a model in one launch, and the
// embedding tables updated in place from the batch's gradient runs (no dense [V,K] gradient), on the walks of optim_rows.h.
//
// The updates are TF 2.1's (keras/optimizer_v2/gradient_descent.py, rmsprop.py; ApplyKerasMomentum, ApplyRMSProp and their Sparse
// twins in core/kernels/training_ops.cc), fp32, every operation rounded as written (contraction off).  Five variants:
//   SGD       momentum == 0   p -= g lr                                                             no slot: m, v are never touched
//   SGD       momentum  > 0   a = a momentum - g lr;  p += a        (Nesterov: p += a momentum - g lr)             slot a in `m`
//   RMSprop   momentum == 0   rms = rho rms + (1 - rho) g g;  p -= lr g / (sqrt(rms) + eps)    (Keras' Python ops)  slot rms in `m`
//   RMSprop   momentum  > 0   dense    rms += (g g - rms)(1 - rho);  mom = mom momentum + (g lr) / sqrt(rms + eps);  p -= mom
//                             touched  rms = rms rho + (g g)(1 - rho);  mom = mom momentum + ((1 / sqrt(rms + eps)) lr) g;  p -= mom
//                             (the fused ops; epsilon inside the root; rms in `m`, mom in `v`)
// Which rows move: all variants but RMSprop with momentum == 0 are row-local -- the batch's rows, plus the untouched rows of the
// regularised fields (dense form, g = 2 l2 p) in a sweep of fil_embed_rowopt_sweep's shape.  RMSprop with momentum == 0 is not: Keras
// assigns rms = rms rho over the WHOLE variable before it scatters the batch's rows, so its sweep walks every non-frozen field --
// decay-only rows read and write rms alone (8 bytes per element), regularised rows take the full rule.
#include "common.h"
#include "embed_runs.h"
#include "optim_rows.h"
#include <hip/hip_bf16.h>

namespace fil {

enum { MV_SGD = 0, MV_SGDM = 1, MV_SGDN = 2, MV_RMS = 3, MV_RMSM = 4 };

struct MomHyper {
  float lr, eps, rho, omr, mom;   // omr = 1 - rho, formed once in fp32
};

static MomHyper mom_hyper(const fil_momopt_hyper& h) {
  MomHyper r;
  r.lr = h.lr;
  r.eps = h.epsilon;
  r.rho = h.rho;
  r.omr = 1.f - h.rho;
  r.mom = h.momentum;
  return r;
}

constexpr bool has_m(int var) { return var != MV_SGD; }
constexpr bool has_v(int var) { return var == MV_RMSM; }

// one element of the variant: s = the first slot (SGD's momentum accumulator, RMSprop's rms), z = RMSprop's momentum slot.  kTouched:
// the row arrived as IndexedSlices (the Sparse* op's form), else the dense op's form -- they differ for RMSprop only (for momentum
// == 0 only in the order of the factors, which rounds the same)
template <int VAR, bool kTouched>
__device__ __forceinline__ void mom_elem(float& p, float& s, float& z, float g, const MomHyper& h) {
#pragma clang fp contract(off)
  if constexpr (VAR == MV_SGD) {
    p = p - g * h.lr;
  } else if constexpr (VAR == MV_SGDM) {
    s = s * h.mom - g * h.lr;
    p = p + s;
  } else if constexpr (VAR == MV_SGDN) {
    s = s * h.mom - g * h.lr;
    p = p + (s * h.mom - g * h.lr);
  } else if constexpr (VAR == MV_RMS) {
    s = kTouched ? s * h.rho + (g * g) * h.omr : h.rho * s + h.omr * (g * g);
    p = p - h.lr * g / (sqrtf(s) + h.eps);
  } else {
    if (kTouched) {
      s = s * h.rho + (g * g) * h.omr;
      z = z * h.mom + ((1.f / sqrtf(s + h.eps)) * h.lr) * g;
    } else {
      s = s + (g * g - s) * h.omr;
      z = z * h.mom + (g * h.lr) / sqrtf(s + h.eps);
    }
    p = p - z;
  }
}

// ---- fil_momopt_multi: the dense descriptors (multi_tensor_walk_slots, optim_rows.h); a slot the variant lacks is never dereferenced
template <int VAR>
__global__ __launch_bounds__(256) void momopt_multi_kernel(const fil_adam_tensor* __restrict__ ts, int n, MomHyper h,
                                                           const float* __restrict__ lr_dev) {
  if (lr_dev) h.lr = *lr_dev;
  multi_tensor_walk_slots<has_m(VAR), has_v(VAR)>(ts, n, [=](float& p, float& s, float& z, float g, float l2x2) {
    mom_elem<VAR, false>(p, s, z, with_l2(g, l2x2, p), h);
  });
}

// one element of a touched row: g = acc + 2 l2 p
template <int VAR>
__device__ __forceinline__ void mom_touched_at(float* __restrict__ table, float* __restrict__ S, float* __restrict__ Z, int64_t e, float acc,
                                               float l2x2, const MomHyper& h) {
  float p = table[e], s = has_m(VAR) ? S[e] : 0.f, z = has_v(VAR) ? Z[e] : 0.f;
  mom_elem<VAR, true>(p, s, z, with_l2(acc, l2x2, p), h);
  table[e] = p;
  if (has_m(VAR)) S[e] = s;
  if (has_v(VAR)) Z[e] = z;
}

// ---- fil_embed_momopt_runs: the run sums of embed_runs.h with the variant as epilogue (touched form); the row is stamped with t when
// a sweep follows (stamp != NULL)
template <int VAR, typename GT>
__global__ __launch_bounds__(256) void embed_momopt_runs_kernel(const GT* __restrict__ g, const int64_t* __restrict__ perm,
                                                                const int64_t* __restrict__ sorted_ids, long R, int K, int F,
                                                                const float* __restrict__ field_l2, float* __restrict__ table,
                                                                float* __restrict__ S, float* __restrict__ Z, int32_t* __restrict__ stamp,
                                                                const int64_t* __restrict__ step, MomHyper h,
                                                                const float* __restrict__ lr_dev) {
  if (lr_dev) h.lr = *lr_dev;
  const int32_t tag = stamp ? (int32_t)(uint32_t)(*step + 1) : 0;
  embed_run_sums(g, perm, sorted_ids, R, K, [=](int64_t row, int kq, const float (&acc)[4], int64_t first) {
    const float l2x2 = field_l2 ? 2.f * field_l2[first % F] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (kq * 4 + i < K) mom_touched_at<VAR>(table, S, Z, row * K + kq * 4 + i, acc[i], l2x2, h);
    if (stamp && kq == 0) stamp[row] = tag;
  });
}

// ---- fil_embed_momopt_sweep.  The grid strides over the virtual rows of the sweep's field table (optim_rows.h): the regularised
// fields for the row-local variants; every non-frozen field for RMSprop with momentum == 0, where an unstamped row of an unregularised
// field takes rms *= rho and nothing else of it is read or written (one 16-byte load and one non-temporal 16-byte store of rms per
// lane), a regularised one the dense rule with g = 2 l2 p.  The branch is uniform per row (K / 4 neighbouring lanes).  The grid is
// sized by the table (no data-dependent size: capturable); workgroups past the walked rows leave at once.
template <int VAR>
__global__ __launch_bounds__(256) void embed_momopt_sweep_kernel(float* __restrict__ table, float* __restrict__ S, float* __restrict__ Z,
                                                                 const int32_t* __restrict__ stamp, int64_t V, int K,
                                                                 const int64_t* __restrict__ offsets, const float* __restrict__ field_l2,
                                                                 const unsigned char* __restrict__ frozen, int F,
                                                                 const int64_t* __restrict__ step, MomHyper h, int vec,
                                                                 const float* __restrict__ lr_dev) {
  constexpr bool kM = has_m(VAR), kZ = has_v(VAR), kAll = VAR == MV_RMS;
  if (lr_dev) h.lr = *lr_dev;
  __shared__ RegTab t;
  load_reg_tab<kAll>(&t, offsets, field_l2, frozen, F, V);
  const int64_t n = t.vbeg[t.n] * K;               // elements of the walked fields
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
      if (kAll && l2x2 == 0.f) {                    // decay only
        f32x4 s = *reinterpret_cast<const f32x4*>(S + e);
        s *= h.rho;
        __builtin_nontemporal_store(s, reinterpret_cast<f32x4*>(S + e));
        continue;
      }
      f32x4 p = *reinterpret_cast<const f32x4*>(table + e);
      f32x4 s = kM ? *reinterpret_cast<const f32x4*>(S + e) : f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 z = kZ ? *reinterpret_cast<const f32x4*>(Z + e) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float pi = p[i], si = s[i], zi = z[i];
        mom_elem<VAR, false>(pi, si, zi, with_l2(0.f, l2x2, pi), h);
        p[i] = pi;
        s[i] = si;
        z[i] = zi;
      }
      __builtin_nontemporal_store(p, reinterpret_cast<f32x4*>(table + e));
      if (kM) __builtin_nontemporal_store(s, reinterpret_cast<f32x4*>(S + e));
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
    if (kAll && t.l2x2[c] == 0.f) {
      __builtin_nontemporal_store(S[e] * h.rho, S + e);
      continue;
    }
    float p = table[e], s = kM ? S[e] : 0.f, z = kZ ? Z[e] : 0.f;
    mom_elem<VAR, false>(p, s, z, with_l2(0.f, t.l2x2[c], p), h);
    __builtin_nontemporal_store(p, table + e);
    if (kM) __builtin_nontemporal_store(s, S + e);
    if (kZ) __builtin_nontemporal_store(z, Z + e);
  }
}

// ---- fil_embed_momopt_merged: the merged walk of the gathered lists (merged_row_sums, optim_rows.h) with the variant (touched form)
template <int VAR>
__global__ __launch_bounds__(256) void embed_momopt_merged_kernel(const int64_t* __restrict__ ids, const float* __restrict__ values,
                                                                  const int64_t* __restrict__ counts, int W, long cap, int K,
                                                                  const int64_t* __restrict__ offsets, const float* __restrict__ field_l2,
                                                                  int F, float* __restrict__ table, float* __restrict__ S,
                                                                  float* __restrict__ Z, int32_t* __restrict__ stamp, int64_t V,
                                                                  const int64_t* __restrict__ step, MomHyper h,
                                                                  const float* __restrict__ lr_dev) {
  if (lr_dev) h.lr = *lr_dev;
  __shared__ int64_t s_off[kSweepMaxF];
  for (int f = threadIdx.x; f < F; f += blockDim.x) s_off[f] = offsets[f];
  __syncthreads();
  const int32_t tag = stamp ? (int32_t)(uint32_t)(*step + 1) : 0;
  const auto epi = [=](int64_t row, int f, float l2x2, int k0, const float (&acc)[kMergeChunk]) {
#pragma unroll
    for (int e = 0; e < kMergeChunk; ++e)
      if (k0 + e < K) mom_touched_at<VAR>(table, S, Z, row * K + k0 + e, acc[e], l2x2, h);
  };
  merged_row_sums((long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x, ids, values, counts, W, cap, K, V, s_off,
                  field_l2, F, epi, [=](int64_t row) { if (stamp) stamp[row] = tag; });
}

// the rule and its hyper-parameters (read here, on the host: a captured launch keeps the values it was captured with) -> the variant
static int check_variant(const char* who, int rule, const fil_momopt_hyper* h, int* var) {
  if (rule != FIL_OPT_SGD && rule != FIL_OPT_RMSPROP)
    return fail(FIL_ERR_ARG, "%s: rule %d (FIL_OPT_SGD or FIL_OPT_RMSPROP)", who, rule);
  if (h == nullptr) return fail(FIL_ERR_ARG, "%s: no hyper-parameters (hyper is NULL)", who);
  if ((h->flags & ~FIL_MOMOPT_NESTEROV) != 0 || h->reserved != 0)
    return fail(FIL_ERR_ARG, "%s: flags %d reserved %d (FIL_MOMOPT_NESTEROV or 0; reserved 0)", who, (int)h->flags, (int)h->reserved);
  if (rule == FIL_OPT_SGD) {
    if (!(h->lr >= 0.f) || !(h->momentum >= 0.f && h->momentum <= 1.f))
      return fail(FIL_ERR_ARG, "%s: SGD hyper-parameters lr=%g momentum=%g (lr >= 0, momentum in [0, 1])", who, (double)h->lr,
                  (double)h->momentum);
    *var = h->momentum == 0.f ? MV_SGD : ((h->flags & FIL_MOMOPT_NESTEROV) ? MV_SGDN : MV_SGDM);
    return FIL_OK;
  }
  if (!(h->lr >= 0.f) || !(h->epsilon >= 0.f) || !(h->rho >= 0.f && h->rho <= 1.f) || !(h->momentum >= 0.f && h->momentum <= 1.f) ||
      (h->flags & FIL_MOMOPT_NESTEROV))
    return fail(FIL_ERR_ARG, "%s: RMSprop hyper-parameters lr=%g epsilon=%g rho=%g momentum=%g flags=%d (lr, epsilon >= 0; rho, momentum "
                "in [0, 1]; no Nesterov)", who, (double)h->lr, (double)h->epsilon, (double)h->rho, (double)h->momentum, (int)h->flags);
  *var = h->momentum == 0.f ? MV_RMS : MV_RMSM;
  return FIL_OK;
}

static bool var_has_m(int var) { return var != MV_SGD; }
static bool var_has_v(int var) { return var == MV_RMSM; }

// the slots the variant needs are there
static int check_slots(const char* who, int var, const float* slot0, const float* slot1) {
  if (var_has_m(var) && slot0 == nullptr)
    return fail(FIL_ERR_ARG, "%s: the variant needs its first slot (SGD's momentum accumulator, RMSprop's rms)", who);
  if (var_has_v(var) && slot1 == nullptr) return fail(FIL_ERR_ARG, "%s: RMSprop with momentum > 0 needs its momentum slot", who);
  return FIL_OK;
}

// the arrays one element of a variant moves (param and its slots)
static double var_arrays(int var) { return 1.0 + (var_has_m(var) ? 1.0 : 0.0) + (var_has_v(var) ? 1.0 : 0.0); }

// profile scope names (string literals: the profiler keeps the pointer), [launch][variant]
enum { SC_MULTI = 0, SC_RUNS = 1, SC_SWEEP = 2, SC_MERGED = 3 };
static const char* const kScope[4][5] = {
    {"sgd_multi", "sgd_momentum_multi", "sgd_nesterov_multi", "rmsprop_multi", "rmsprop_momentum_multi"},
    {"embed_sgd_runs", "embed_sgd_momentum_runs", "embed_sgd_nesterov_runs", "embed_rmsprop_runs", "embed_rmsprop_momentum_runs"},
    {"embed_sgd_sweep", "embed_sgd_momentum_sweep", "embed_sgd_nesterov_sweep", "embed_rmsprop_sweep", "embed_rmsprop_momentum_sweep"},
    {"embed_sgd_merged", "embed_sgd_momentum_merged", "embed_sgd_nesterov_merged", "embed_rmsprop_merged", "embed_rmsprop_momentum_merged"}};

}  // namespace fil

using namespace fil;

#define FIL_MOM_DISPATCH(var, LAUNCH) \
  switch (var) {                      \
    case MV_SGD: LAUNCH(MV_SGD); break;   \
    case MV_SGDM: LAUNCH(MV_SGDM); break; \
    case MV_SGDN: LAUNCH(MV_SGDN); break; \
    case MV_RMS: LAUNCH(MV_RMS); break;   \
    default: LAUNCH(MV_RMSM); break;      \
  }

static int momopt_multi_impl(const char* who, const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule,
                             const fil_momopt_hyper* hyper, int advance, void* stream, const float* lr_dev) {
  FIL_CHECK_ARG_W(who, n >= 0 && total_numel >= 0);
  FIL_CHECK_ARG_W(who, step != nullptr);
  FIL_CHECK_ARG_W(who, n == 0 || tensors != nullptr);
  int var = 0;
  if (int rc = check_variant(who, rule, hyper, &var)) return rc;
  if (advance != 0 && advance != 1) return fail(FIL_ERR_ARG, "%s: advance %d (0 or 1)", who, advance);
  hipStream_t st = (hipStream_t)stream;
  const MomHyper h = mom_hyper(*hyper);
  if (n > 0) {
      ProfScope ps(kScope[SC_MULTI][var], st, (4.0 + 8.0 * var_arrays(var)) * (double)total_numel);
    const long chunks = std::max<long>(1, (long)((total_numel + kMultiChunk - 1) / kMultiChunk));
    const dim3 grid((int)std::min<long>(chunks, 256 * 8));
#define FIL_MOM_MULTI(VAR) hipLaunchKernelGGL(momopt_multi_kernel<VAR>, grid, dim3(256), 0, st, tensors, n, h, lr_dev)
    FIL_MOM_DISPATCH(var, FIL_MOM_MULTI)
#undef FIL_MOM_MULTI
    FIL_CHECK_LAUNCH_W(who);
  }
  if (advance) {
    launch_step_advance(step, st);
    FIL_CHECK_LAUNCH_W(who);
  }
  return FIL_OK;
}

extern "C" int fil_momopt_multi(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule,
                                const fil_momopt_hyper* hyper, int advance, void* stream) {
  return momopt_multi_impl("fil_momopt_multi", tensors, n, total_numel, step, rule, hyper, advance, stream, nullptr);
}

extern "C" int fil_momopt_multi_lrdev(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule,
                                      const fil_momopt_hyper* hyper, const float* lr_dev, int advance, void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_momopt_multi_lrdev: no device rate (lr_dev is NULL)");
  return momopt_multi_impl("fil_momopt_multi_lrdev", tensors, n, total_numel, step, rule, hyper, advance, stream, lr_dev);
}

static int embed_momopt_runs_impl(const char* who, const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype,
                                  int F, const float* field_l2, float* table, float* slot0, float* slot1, int32_t* stamp,
                                  const int64_t* step, int rule, const fil_momopt_hyper* hyper, void* stream, const float* lr_dev) {
  FIL_CHECK_ARG_W(who, R >= 0 && K >= 1 && F >= 1);
  if (g_dtype != FIL_F32 && g_dtype != FIL_BF16) return fail(FIL_ERR_ARG, "%s: g_dtype %d (f32 or bf16)", who, g_dtype);
  if (K > 256) return fail(FIL_ERR_UNSUPPORTED, "%s: K=%d > 256", who, K);
  int var = 0;
  if (int rc = check_variant(who, rule, hyper, &var)) return rc;
  if (R == 0) return FIL_OK;
  FIL_CHECK_ARG_W(who, g && perm && sorted_ids && table && step);
  if (int rc = check_slots(who, var, slot0, slot1)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const MomHyper h = mom_hyper(*hyper);
  ProfScope ps(kScope[SC_RUNS][var], st, (double)R * K * (g_dtype == FIL_F32 ? 4 : 2) + 8.0 * var_arrays(var) * R * K);
  const int C = 64 / ((K + 3) / 4);
  const dim3 grid((int)std::min<long>((R + 4 * C - 1) / (4 * C), 256 * 32));
  float* S = var_has_m(var) ? slot0 : nullptr;
  float* Z = var_has_v(var) ? slot1 : nullptr;
#define FIL_MOM_RUNS(VAR)                                                                                                                \
  if (g_dtype == FIL_F32)                                                                                                                \
    hipLaunchKernelGGL((embed_momopt_runs_kernel<VAR, float>), grid, dim3(256), 0, st, static_cast<const float*>(g), perm, sorted_ids, R, K, \
                       F, field_l2, table, S, Z, stamp, step, h, lr_dev);                                                                \
  else                                                                                                                                   \
    hipLaunchKernelGGL((embed_momopt_runs_kernel<VAR, __hip_bfloat16>), grid, dim3(256), 0, st, static_cast<const __hip_bfloat16*>(g), perm, \
                       sorted_ids, R, K, F, field_l2, table, S, Z, stamp, step, h, lr_dev)
  FIL_MOM_DISPATCH(var, FIL_MOM_RUNS)
#undef FIL_MOM_RUNS
  FIL_CHECK_LAUNCH_W(who);
  return FIL_OK;
}

extern "C" int fil_embed_momopt_runs(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                     const float* field_l2, float* table, float* slot0, float* slot1, int32_t* stamp,
                                     const int64_t* step, int rule, const fil_momopt_hyper* hyper, void* stream) {
  return embed_momopt_runs_impl("fil_embed_momopt_runs", g, perm, sorted_ids, R, K, g_dtype, F, field_l2, table, slot0, slot1, stamp, step,
                                rule, hyper, stream, nullptr);
}

extern "C" int fil_embed_momopt_runs_lrdev(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                           const float* field_l2, float* table, float* slot0, float* slot1, int32_t* stamp,
                                           const int64_t* step, int rule, const fil_momopt_hyper* hyper, const float* lr_dev,
                                           void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_momopt_runs_lrdev: no device rate (lr_dev is NULL)");
  return embed_momopt_runs_impl("fil_embed_momopt_runs_lrdev", g, perm, sorted_ids, R, K, g_dtype, F, field_l2, table, slot0, slot1, stamp,
                                step, rule, hyper, stream, lr_dev);
}

static int embed_momopt_sweep_impl(const char* who, float* table, float* slot0, float* slot1, const int32_t* stamp, int64_t V, int K,
                                   const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F, const int64_t* step,
                                   int rule, const fil_momopt_hyper* hyper, void* stream, const float* lr_dev) {
  FIL_CHECK_ARG_W(who, V >= 0 && K >= 1 && F >= 1);
  if (F > kSweepMaxF) return fail(FIL_ERR_UNSUPPORTED, "%s: F=%d > %d fields", who, F, kSweepMaxF);
  int var = 0;
  if (int rc = check_variant(who, rule, hyper, &var)) return rc;
  // a row-local variant without a regularised field: no untouched row moves.  RMSprop with momentum == 0 decays rms everywhere.
  if (V == 0 || (var != MV_RMS && field_l2 == nullptr)) return FIL_OK;
  FIL_CHECK_ARG_W(who, table && stamp && offsets && step);
  if (int rc = check_slots(who, var, slot0, slot1)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const MomHyper h = mom_hyper(*hyper);
  float* S = var_has_m(var) ? slot0 : nullptr;
  float* Z = var_has_v(var) ? slot1 : nullptr;
  const int64_t n = V * K;
  const int vec = (K % 4 == 0 && ((((uintptr_t)table | (uintptr_t)S | (uintptr_t)Z) & 15) == 0)) ? 1 : 0;
  const int64_t work = vec ? n / 4 : n;
  // (bytes of a whole-table sweep at the full rule: the kernel moves only the walked fields' share, 8 per element where it only decays)
  ProfScope ps(kScope[SC_SWEEP][var], st, 8.0 * var_arrays(var) * (double)n + 4.0 * (double)V);
  const dim3 grid((int)std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, 256 * 8)));
#define FIL_MOM_SWEEP(VAR)                                                                                                          \
  hipLaunchKernelGGL(embed_momopt_sweep_kernel<VAR>, grid, dim3(256), 0, st, table, S, Z, stamp, V, K, offsets, field_l2, frozen, F, step, \
                     h, vec, lr_dev)
  FIL_MOM_DISPATCH(var, FIL_MOM_SWEEP)
#undef FIL_MOM_SWEEP
  FIL_CHECK_LAUNCH_W(who);
  return FIL_OK;
}

extern "C" int fil_embed_momopt_sweep(float* table, float* slot0, float* slot1, const int32_t* stamp, int64_t V, int K,
                                      const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F,
                                      const int64_t* step, int rule, const fil_momopt_hyper* hyper, void* stream) {
  return embed_momopt_sweep_impl("fil_embed_momopt_sweep", table, slot0, slot1, stamp, V, K, offsets, field_l2, frozen, F, step, rule,
                                 hyper, stream, nullptr);
}

extern "C" int fil_embed_momopt_sweep_lrdev(float* table, float* slot0, float* slot1, const int32_t* stamp, int64_t V, int K,
                                            const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F,
                                            const int64_t* step, int rule, const fil_momopt_hyper* hyper, const float* lr_dev,
                                            void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_momopt_sweep_lrdev: no device rate (lr_dev is NULL)");
  return embed_momopt_sweep_impl("fil_embed_momopt_sweep_lrdev", table, slot0, slot1, stamp, V, K, offsets, field_l2, frozen, F, step, rule,
                                 hyper, stream, lr_dev);
}

static int embed_momopt_merged_impl(const char* who, const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                    const int64_t* offsets, const float* field_l2, int F, float* table, float* slot0, float* slot1,
                                    int32_t* stamp, int64_t V, const int64_t* step, int rule, const fil_momopt_hyper* hyper, void* stream,
                                    const float* lr_dev) {
  FIL_CHECK_ARG_W(who, W >= 1 && cap >= 0 && K >= 1 && F >= 1 && V >= 0);
  if (K > 256) return fail(FIL_ERR_UNSUPPORTED, "%s: K=%d > 256", who, K);
  if (F > kSweepMaxF) return fail(FIL_ERR_UNSUPPORTED, "%s: F=%d > %d fields", who, F, kSweepMaxF);
  int var = 0;
  if (int rc = check_variant(who, rule, hyper, &var)) return rc;
  if (cap == 0 || V == 0) return FIL_OK;
  FIL_CHECK_ARG_W(who, ids && values && counts && offsets && table && step);
  if (int rc = check_slots(who, var, slot0, slot1)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const MomHyper h = mom_hyper(*hyper);
  float* S = var_has_m(var) ? slot0 : nullptr;
  float* Z = var_has_v(var) ? slot1 : nullptr;
  const long n = (long)W * cap;
  ProfScope ps(kScope[SC_MERGED][var], st, 8.0 * n + 4.0 * (double)n * K + 8.0 * var_arrays(var) * (double)cap * K);
  const dim3 grid((int)std::max<long>(1, std::min<long>((n + 255) / 256, 256 * 8)));
#define FIL_MOM_MERGED(VAR)                                                                                                             \
  hipLaunchKernelGGL(embed_momopt_merged_kernel<VAR>, grid, dim3(256), 0, st, ids, values, counts, W, cap, K, offsets, field_l2, F, table, S, \
                     Z, stamp, V, step, h, lr_dev)
  FIL_MOM_DISPATCH(var, FIL_MOM_MERGED)
#undef FIL_MOM_MERGED
  FIL_CHECK_LAUNCH_W(who);
  return FIL_OK;
}

extern "C" int fil_embed_momopt_merged(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                       const int64_t* offsets, const float* field_l2, int F, float* table, float* slot0, float* slot1,
                                       int32_t* stamp, int64_t V, const int64_t* step, int rule, const fil_momopt_hyper* hyper,
                                       void* stream) {
  return embed_momopt_merged_impl("fil_embed_momopt_merged", ids, values, counts, W, cap, K, offsets, field_l2, F, table, slot0, slot1,
                                  stamp, V, step, rule, hyper, stream, nullptr);
}

extern "C" int fil_embed_momopt_merged_lrdev(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                             const int64_t* offsets, const float* field_l2, int F, float* table, float* slot0,
                                             float* slot1, int32_t* stamp, int64_t V, const int64_t* step, int rule,
                                             const fil_momopt_hyper* hyper, const float* lr_dev, void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_momopt_merged_lrdev: no device rate (lr_dev is NULL)");
  return embed_momopt_merged_impl("fil_embed_momopt_merged_lrdev", ids, values, counts, W, cap, K, offsets, field_l2, F, table, slot0,
                                  slot1, stamp, V, step, rule, hyper, stream, lr_dev);
}
