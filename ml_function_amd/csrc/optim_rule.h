// The row-rule optimizers (optim_rowwise.hip: Adagrad, Ftrl; optim_momentum.hip: SGD, RMSprop; optim_adaptive.hip: Adadelta, Adamax;
// optim_nadam.hip: Nadam),
// each kernel shape and each host launcher written once on the walks of optim_rows.h.  A rule is a row-local per-element update whose
// coefficients do not depend on the step, or (kStepped) depend on it through one wave-uniform prepare() per kernel (Adam's sweep is not
// row-local: optim.hip stays apart); its file supplies a Rule per variant and one Family:
//   Rule    Hyper                        the device hyper-parameters, passed by value; `lr` is a member (the device rate replaces it)
//           kHasS, kHasZ                 the rule has the first / the second slot: one it lacks is never dereferenced and may be NULL
//           kSweepAll                    the sweep walks every non-frozen field, an unstamped row of an unregularised one takes decay()
//           elem<kTouched>(p, s, z, g, h)  one element, contraction off; kTouched: the row came with the batch (the Sparse op's form)
//           decay(s, h)                  -> the decayed first slot; only where kSweepAll
//           kDecayZ, decay_z(z, h)       opt-in (a rule without the member decays its first slot only), only where kSweepAll: a decay-only
//                                        row decays the second slot too -- one more 16-byte load and non-temporal store beside S's
//           kStepped, prepare(h, it)     opt-in (a rule without the member is not stepped): every kernel replaces its hyper-parameters by
//                                        prepare(h, *step) once at its top, after the device rate has replaced lr -- `it` is the count of
//                                        completed steps (Keras' iterations), the same in every launch of a step: the counter advances last
//           scope(SC_*)                  the profile scope name of each launch (string literals: the profiler keeps the pointer)
//   Family  Raw                          the hyper-parameter struct of fil.h
//           resolve(who, rule, raw, &var)  checks rule and hyper-parameters (on the host: a capture keeps the values) -> the variant
//           device(raw)                  -> Hyper
//           check_slots(who, var, s, z)  reports a slot the variant needs and did not get
//           dispatch(var, f)             returns f(Rule{}) of the variant's Rule
//           advance(step, raw, stream)   opt-in (a family without the member advances the counter with launch_step_advance): the ONE
//                                        one-thread launch that ends a step, for a family that keeps device state beside the counter
// The bytes a launch is charged for count 8 per element and array: the parameter and the slots the rule has.
#pragma once
#include "common.h"
#include "embed_runs.h"
#include "optim_rows.h"
#include <hip/hip_bf16.h>
#include <type_traits>

namespace fil {

enum { SC_MULTI = 0, SC_RUNS = 1, SC_SWEEP = 2, SC_MERGED = 3 };

template <typename Rule, typename = void>
struct rule_stepped : std::false_type {};
template <typename Rule>
struct rule_stepped<Rule, std::void_t<decltype(Rule::kStepped)>> : std::bool_constant<Rule::kStepped> {};

template <typename Rule, typename = void>
struct rule_decays_z : std::false_type {};
template <typename Rule>
struct rule_decays_z<Rule, std::void_t<decltype(Rule::kDecayZ)>> : std::bool_constant<Rule::kDecayZ> {};

template <typename Fam, typename = void>
struct family_advances : std::false_type {};
template <typename Fam>
struct family_advances<Fam, std::void_t<decltype(&Fam::advance)>> : std::true_type {};

// the top of every kernel: the step's rate, then the step's coefficients (nothing is read or computed for a rule that is not stepped)
template <typename Rule>
__device__ __forceinline__ void rule_hyper_of_step(typename Rule::Hyper& h, const float* __restrict__ lr_dev, const int64_t* __restrict__ step) {
  if (lr_dev) h.lr = *lr_dev;
  if constexpr (rule_stepped<Rule>::value) h = Rule::prepare(h, *step);
}

template <typename Rule>
constexpr double rule_arrays() { return 1.0 + (Rule::kHasS ? 1.0 : 0.0) + (Rule::kHasZ ? 1.0 : 0.0); }

// (the *_lrdev entry points: the kernels take the rate from the word fil_lr_schedule_eval left on the device, `if (lr_dev) h.lr =
// *lr_dev` -- one wave-uniform load at the top of each kernel; a by-value launch passes NULL)

// ---- the dense launch: the descriptors (multi_tensor_walk_slots) with the rule in its dense form; `m` is the first slot, `v` the second
template <typename Rule>
__global__ __launch_bounds__(256) void rule_multi_kernel(const fil_adam_tensor* __restrict__ ts, int n, typename Rule::Hyper h,
                                                         const float* __restrict__ lr_dev, const int64_t* __restrict__ step) {
  rule_hyper_of_step<Rule>(h, lr_dev, step);
  multi_tensor_walk_slots<Rule::kHasS, Rule::kHasZ>(ts, n, [=](float& p, float& s, float& z, float g, float l2x2) {
    Rule::template elem<false>(p, s, z, with_l2(g, l2x2, p), h);
  });
}

// one element of a touched row: g = acc + 2 l2 p
template <typename Rule>
__device__ __forceinline__ void rule_touched_at(float* __restrict__ table, float* __restrict__ S, float* __restrict__ Z, int64_t e, float acc,
                                                float l2x2, const typename Rule::Hyper& h) {
  float p = table[e], s = Rule::kHasS ? S[e] : 0.f, z = Rule::kHasZ ? Z[e] : 0.f;
  Rule::template elem<true>(p, s, z, with_l2(acc, l2x2, p), h);
  table[e] = p;
  if (Rule::kHasS) S[e] = s;
  if (Rule::kHasZ) Z[e] = z;
}

// ---- the runs update: the run sums of embed_runs.h with the rule as epilogue (touched form).  The run of row `row`, field f = perm % F,
// takes g = run sum + 2 field_l2[f] p; the row is stamped with t when a sweep follows (stamp != NULL).
template <typename Rule, typename GT>
__global__ __launch_bounds__(256) void embed_rule_runs_kernel(const GT* __restrict__ g, const int64_t* __restrict__ perm,
                                                              const int64_t* __restrict__ sorted_ids, long R, int K, int F,
                                                              const float* __restrict__ field_l2, float* __restrict__ table,
                                                              float* __restrict__ S, float* __restrict__ Z, int32_t* __restrict__ stamp,
                                                              const int64_t* __restrict__ step, typename Rule::Hyper h,
                                                              const float* __restrict__ lr_dev) {
  rule_hyper_of_step<Rule>(h, lr_dev, step);
  const int32_t tag = stamp ? step_tag(step) : 0;
  embed_run_sums(g, perm, sorted_ids, R, K, [=](int64_t row, int kq, const float (&acc)[4], int64_t first) {
    const float l2x2 = field_l2 ? 2.f * field_l2[first % F] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (kq * 4 + i < K) rule_touched_at<Rule>(table, S, Z, row * K + kq * 4 + i, acc[i], l2x2, h);
    if (stamp && kq == 0) stamp[row] = tag;
  });
}

// ---- the sweep: the untouched rows that move.  The grid strides over the virtual rows of the sweep's field table (RegTab,
// optim_rows.h): the regularised, non-frozen fields, whose unstamped rows take the dense rule with g = 2 l2 p; with kSweepAll every
// non-frozen field, where an unstamped row of an unregularised field takes decay() and nothing but its first slot is read or written
// (one 16-byte load and one non-temporal 16-byte store per lane; with kDecayZ the same for its second slot).  The branch is uniform
// per row (K / 4 neighbouring lanes).  The grid is sized by the table (no data-dependent size: capturable); workgroups past the
// walked rows leave at once.
template <typename Rule>
__global__ __launch_bounds__(256) void embed_rule_sweep_kernel(float* __restrict__ table, float* __restrict__ S, float* __restrict__ Z,
                                                               const int32_t* __restrict__ stamp, int64_t V, int K,
                                                               const int64_t* __restrict__ offsets, const float* __restrict__ field_l2,
                                                               const unsigned char* __restrict__ frozen, int F,
                                                               const int64_t* __restrict__ step, typename Rule::Hyper h, int vec,
                                                               const float* __restrict__ lr_dev) {
  constexpr bool kM = Rule::kHasS, kZ = Rule::kHasZ, kAll = Rule::kSweepAll;
  rule_hyper_of_step<Rule>(h, lr_dev, step);
  __shared__ RegTab t;
  load_reg_tab<kAll>(&t, offsets, field_l2, frozen, F, V);
  const int64_t n = t.vbeg[t.n] * K;               // elements of the walked fields
  const int32_t tag = step_tag(step);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (vec) {                                        // K % 4 == 0 and 16-byte aligned arrays: a lane moves 4 elements of one row
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n / 4; q += stride) {
      const int64_t vr = q * 4 / K;
      const int c = reg_field(&t, vr);
      const int64_t row = t.rbeg[c] + (vr - t.vbeg[c]);
      const float l2x2 = t.l2x2[c];
      const int64_t e = row * K + (q * 4 - vr * K);
      if (stamp[row] == tag) continue;
      if constexpr (kAll) {
        if (l2x2 == 0.f) {                          // decay only
          f32x4 s = *reinterpret_cast<const f32x4*>(S + e);
          if constexpr (rule_decays_z<Rule>::value) {  // both loads in flight before either store
            f32x4 z = *reinterpret_cast<const f32x4*>(Z + e);
#pragma unroll
            for (int i = 0; i < 4; ++i) z[i] = Rule::decay_z(z[i], h);
            __builtin_nontemporal_store(z, reinterpret_cast<f32x4*>(Z + e));
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) s[i] = Rule::decay(s[i], h);
          __builtin_nontemporal_store(s, reinterpret_cast<f32x4*>(S + e));
          continue;
        }
      }
      f32x4 p = *reinterpret_cast<const f32x4*>(table + e);
      f32x4 s = kM ? *reinterpret_cast<const f32x4*>(S + e) : f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 z = kZ ? *reinterpret_cast<const f32x4*>(Z + e) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float pi = p[i], si = s[i], zi = z[i];
        Rule::template elem<false>(pi, si, zi, with_l2(0.f, l2x2, pi), h);
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
    if constexpr (kAll) {
      if (t.l2x2[c] == 0.f) {
        __builtin_nontemporal_store(Rule::decay(S[e], h), S + e);
        if constexpr (rule_decays_z<Rule>::value) __builtin_nontemporal_store(Rule::decay_z(Z[e], h), Z + e);
        continue;
      }
    }
    float p = table[e], s = kM ? S[e] : 0.f, z = kZ ? Z[e] : 0.f;
    Rule::template elem<false>(p, s, z, with_l2(0.f, t.l2x2[c], p), h);
    __builtin_nontemporal_store(p, table + e);
    if (kM) __builtin_nontemporal_store(s, S + e);
    if (kZ) __builtin_nontemporal_store(z, Z + e);
  }
}

// ---- the merged update: the merged walk of the gathered lists (merged_row_sums, optim_rows.h) with the rule (touched form)
template <typename Rule>
__global__ __launch_bounds__(256) void embed_rule_merged_kernel(const int64_t* __restrict__ ids, const float* __restrict__ values,
                                                                const int64_t* __restrict__ counts, int W, long cap, int K,
                                                                const int64_t* __restrict__ offsets, const float* __restrict__ field_l2,
                                                                int F, float* __restrict__ table, float* __restrict__ S,
                                                                float* __restrict__ Z, int32_t* __restrict__ stamp, int64_t V,
                                                                const int64_t* __restrict__ step, typename Rule::Hyper h,
                                                                const float* __restrict__ lr_dev) {
  rule_hyper_of_step<Rule>(h, lr_dev, step);
  __shared__ int64_t s_off[kSweepMaxF];
  for (int f = threadIdx.x; f < F; f += blockDim.x) s_off[f] = offsets[f];
  __syncthreads();
  const int32_t tag = stamp ? step_tag(step) : 0;
  const auto epi = [=](int64_t row, int f, float l2x2, int k0, const float (&acc)[kMergeChunk]) {
#pragma unroll
    for (int e = 0; e < kMergeChunk; ++e)
      if (k0 + e < K) rule_touched_at<Rule>(table, S, Z, row * K + k0 + e, acc[e], l2x2, h);
  };
  merged_row_sums((long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x, ids, values, counts, W, cap, K, V, s_off,
                  field_l2, F, epi, [=](int64_t row) { if (stamp) stamp[row] = tag; });
}

// ---- the host launchers.  `who` names the entry point that was called; lr_dev NULL: the rate of the hyper-parameters.

template <typename Fam>
int rule_multi_launch(const char* who, const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule,
                      const typename Fam::Raw* hyper, int advance, void* stream, const float* lr_dev) {
  FIL_CHECK_ARG_W(who, n >= 0 && total_numel >= 0);
  FIL_CHECK_ARG_W(who, step != nullptr);
  FIL_CHECK_ARG_W(who, n == 0 || tensors != nullptr);
  int var = 0;
  if (int rc = Fam::resolve(who, rule, hyper, &var)) return rc;
  if (advance != 0 && advance != 1) return fail(FIL_ERR_ARG, "%s: advance %d (0 or 1)", who, advance);
  hipStream_t st = (hipStream_t)stream;
  if (n > 0) {
    const auto h = Fam::device(*hyper);
    const long chunks = std::max<long>(1, (long)((total_numel + kMultiChunk - 1) / kMultiChunk));
    const dim3 grid((int)std::min<long>(chunks, 256 * 8));
    if (int rc = Fam::dispatch(var, [&](auto r) -> int {
          using Rule = decltype(r);
          ProfScope ps(Rule::scope(SC_MULTI), st, (4.0 + 8.0 * rule_arrays<Rule>()) * (double)total_numel);
          hipLaunchKernelGGL(rule_multi_kernel<Rule>, grid, dim3(256), 0, st, tensors, n, h, lr_dev, step);
          FIL_CHECK_LAUNCH_W(who);
          return FIL_OK;
        }))
      return rc;
  }
  if (advance) {
    if constexpr (family_advances<Fam>::value) Fam::advance(step, *hyper, st);
    else launch_step_advance(step, st);
    FIL_CHECK_LAUNCH_W(who);
  }
  return FIL_OK;
}

template <typename Fam>
int embed_rule_runs_launch(const char* who, const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                           const float* field_l2, float* table, float* slot0, float* slot1, int32_t* stamp, const int64_t* step, int rule,
                           const typename Fam::Raw* hyper, void* stream, const float* lr_dev) {
  FIL_CHECK_ARG_W(who, R >= 0 && K >= 1 && F >= 1);
  if (g_dtype != FIL_F32 && g_dtype != FIL_BF16) return fail(FIL_ERR_ARG, "%s: g_dtype %d (f32 or bf16)", who, g_dtype);
  if (int rc = check_table_shape(who, K, 0)) return rc;
  int var = 0;
  if (int rc = Fam::resolve(who, rule, hyper, &var)) return rc;
  if (R == 0) return FIL_OK;
  FIL_CHECK_ARG_W(who, g && perm && sorted_ids && table && step);
  if (int rc = Fam::check_slots(who, var, slot0, slot1)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const auto h = Fam::device(*hyper);
  const dim3 grid = run_sums_grid(R, K);
  return Fam::dispatch(var, [&](auto r) -> int {
    using Rule = decltype(r);
    ProfScope ps(Rule::scope(SC_RUNS), st, (double)R * K * (g_dtype == FIL_F32 ? 4 : 2) + 8.0 * rule_arrays<Rule>() * R * K);
    float* S = Rule::kHasS ? slot0 : nullptr;
    float* Z = Rule::kHasZ ? slot1 : nullptr;
    if (g_dtype == FIL_F32)
      hipLaunchKernelGGL((embed_rule_runs_kernel<Rule, float>), grid, dim3(256), 0, st, static_cast<const float*>(g), perm, sorted_ids, R, K,
                         F, field_l2, table, S, Z, stamp, step, h, lr_dev);
    else
      hipLaunchKernelGGL((embed_rule_runs_kernel<Rule, __hip_bfloat16>), grid, dim3(256), 0, st, static_cast<const __hip_bfloat16*>(g), perm,
                         sorted_ids, R, K, F, field_l2, table, S, Z, stamp, step, h, lr_dev);
    FIL_CHECK_LAUNCH_W(who);
    return FIL_OK;
  });
}

template <typename Fam>
int embed_rule_sweep_launch(const char* who, float* table, float* slot0, float* slot1, const int32_t* stamp, int64_t V, int K,
                            const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F, const int64_t* step, int rule,
                            const typename Fam::Raw* hyper, void* stream, const float* lr_dev) {
  FIL_CHECK_ARG_W(who, V >= 0 && K >= 1 && F >= 1);
  if (int rc = check_table_shape(who, 0, F)) return rc;
  int var = 0;
  if (int rc = Fam::resolve(who, rule, hyper, &var)) return rc;
  return Fam::dispatch(var, [&](auto r) -> int {
    using Rule = decltype(r);
    // without a regularised field no untouched row moves, unless the rule decays its slot everywhere
    if (V == 0 || (!Rule::kSweepAll && field_l2 == nullptr)) return FIL_OK;
    FIL_CHECK_ARG_W(who, table && stamp && offsets && step);
    if (int rc = Fam::check_slots(who, var, slot0, slot1)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const auto h = Fam::device(*hyper);
    float* S = Rule::kHasS ? slot0 : nullptr;
    float* Z = Rule::kHasZ ? slot1 : nullptr;
    const int64_t n = V * K;
    const int vec = sweep_vec(K, table, S, Z);
    const int64_t work = vec ? n / 4 : n;
    // (bytes of a whole-table sweep at the full rule: the kernel moves only the walked fields' share, 8 per element where it only decays)
    ProfScope ps(Rule::scope(SC_SWEEP), st, 8.0 * rule_arrays<Rule>() * (double)n + 4.0 * (double)V);
    const dim3 grid = stride_grid(work);
    hipLaunchKernelGGL(embed_rule_sweep_kernel<Rule>, grid, dim3(256), 0, st, table, S, Z, stamp, V, K, offsets, field_l2, frozen, F, step, h,
                       vec, lr_dev);
    FIL_CHECK_LAUNCH_W(who);
    return FIL_OK;
  });
}

template <typename Fam>
int embed_rule_merged_launch(const char* who, const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                             const int64_t* offsets, const float* field_l2, int F, float* table, float* slot0, float* slot1, int32_t* stamp,
                             int64_t V, const int64_t* step, int rule, const typename Fam::Raw* hyper, void* stream, const float* lr_dev) {
  FIL_CHECK_ARG_W(who, W >= 1 && cap >= 0 && K >= 1 && F >= 1 && V >= 0);
  if (int rc = check_table_shape(who, K, F)) return rc;
  int var = 0;
  if (int rc = Fam::resolve(who, rule, hyper, &var)) return rc;
  if (cap == 0 || V == 0) return FIL_OK;
  FIL_CHECK_ARG_W(who, ids && values && counts && offsets && table && step);
  if (int rc = Fam::check_slots(who, var, slot0, slot1)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const auto h = Fam::device(*hyper);
  const long n = (long)W * cap;
  const dim3 grid = stride_grid(n);
  return Fam::dispatch(var, [&](auto r) -> int {
    using Rule = decltype(r);
    ProfScope ps(Rule::scope(SC_MERGED), st, 8.0 * n + 4.0 * (double)n * K + 8.0 * rule_arrays<Rule>() * (double)cap * K);
    float* S = Rule::kHasS ? slot0 : nullptr;
    float* Z = Rule::kHasZ ? slot1 : nullptr;
    hipLaunchKernelGGL(embed_rule_merged_kernel<Rule>, grid, dim3(256), 0, st, ids, values, counts, W, cap, K, offsets, field_l2, F, table, S,
                       Z, stamp, V, step, h, lr_dev);
    FIL_CHECK_LAUNCH_W(who);
    return FIL_OK;
  });
}

}  // namespace fil
