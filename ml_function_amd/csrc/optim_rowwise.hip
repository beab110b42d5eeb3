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
// The kernels and the host launchers are optim_rule.h's; this file holds what is Adagrad's and Ftrl's own.
#include "optim_rule.h"

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

static const char* const kRowScope[2][4] = {{"adagrad_multi", "embed_adagrad_runs", "embed_adagrad_sweep", "embed_adagrad_merged"},
                                            {"ftrl_multi", "embed_ftrl_runs", "embed_ftrl_sweep", "embed_ftrl_merged"}};

// s = the accumulator, z = Ftrl's linear slot (unused by Adagrad); the touched and the dense form are one
template <int RULE>
struct RowRule {
  using Hyper = RowHyper;
  static constexpr bool kHasS = true, kHasZ = RULE == FIL_OPT_FTRL, kSweepAll = false;
  static const char* scope(int launch) { return kRowScope[RULE == FIL_OPT_FTRL][launch]; }

  template <bool kTouched>
  static __device__ __forceinline__ void elem(float& p, float& s, float& z, float g, const RowHyper& h) {
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
};

struct RowFamily {
  using Raw = fil_rowopt_hyper;
  static RowHyper device(const Raw& h) { return row_hyper(h); }

  // the rule and its hyper-parameters (read here, on the host: a captured launch keeps the values it was captured with)
  static int resolve(const char* who, int rule, const Raw* h, int* var) {
    if (rule != FIL_OPT_ADAGRAD && rule != FIL_OPT_FTRL)
      return fail(FIL_ERR_ARG, "%s: rule %d (FIL_OPT_ADAGRAD or FIL_OPT_FTRL)", who, rule);
    if (h == nullptr) return fail(FIL_ERR_ARG, "%s: no hyper-parameters (hyper is NULL)", who);
    if (rule == FIL_OPT_ADAGRAD && (!(h->lr >= 0.f) || !(h->epsilon >= 0.f)))
      return fail(FIL_ERR_ARG, "%s: Adagrad hyper-parameters lr=%g epsilon=%g (both >= 0)", who, (double)h->lr, (double)h->epsilon);
    if (rule == FIL_OPT_FTRL && (!(h->lr >= 0.f) || !(h->lr_power <= 0.f) || !(h->l1 >= 0.f) || !(h->l2 >= 0.f) || !(h->l2_shrinkage >= 0.f)))
      return fail(FIL_ERR_ARG, "%s: Ftrl hyper-parameters lr=%g lr_power=%g l1=%g l2=%g l2_shrinkage=%g (lr_power <= 0, the others >= 0)",
                  who, (double)h->lr, (double)h->lr_power, (double)h->l1, (double)h->l2, (double)h->l2_shrinkage);
    *var = rule;
    return FIL_OK;
  }

  static int check_slots(const char* who, int var, const float* accum, const float* linear) {
    FIL_CHECK_ARG_W(who, accum != nullptr);
    if (var == FIL_OPT_FTRL && linear == nullptr) return fail(FIL_ERR_ARG, "%s: Ftrl needs its linear slot", who);
    return FIL_OK;
  }

  template <typename Fn>
  static int dispatch(int var, Fn&& f) {
    return var == FIL_OPT_FTRL ? f(RowRule<FIL_OPT_FTRL>{}) : f(RowRule<FIL_OPT_ADAGRAD>{});
  }
};

}  // namespace fil

using namespace fil;

extern "C" int fil_rowopt_multi(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule,
                                const fil_rowopt_hyper* hyper, int advance, void* stream) {
  return rule_multi_launch<RowFamily>("fil_rowopt_multi", tensors, n, total_numel, step, rule, hyper, advance, stream, nullptr);
}

extern "C" int fil_rowopt_multi_lrdev(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule,
                                const fil_rowopt_hyper* hyper, const float* lr_dev, int advance, void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_rowopt_multi_lrdev: no device rate (lr_dev is NULL)");
  return rule_multi_launch<RowFamily>("fil_rowopt_multi_lrdev", tensors, n, total_numel, step, rule, hyper, advance, stream, lr_dev);
}

extern "C" int fil_embed_rowopt_runs(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                     const float* field_l2, float* table, float* accum, float* linear, int32_t* stamp,
                                     const int64_t* step, int rule, const fil_rowopt_hyper* hyper, void* stream) {
  return embed_rule_runs_launch<RowFamily>("fil_embed_rowopt_runs", g, perm, sorted_ids, R, K, g_dtype, F, field_l2, table, accum, linear, stamp, step,
                                rule, hyper, stream, nullptr);
}

extern "C" int fil_embed_rowopt_runs_lrdev(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                     const float* field_l2, float* table, float* accum, float* linear, int32_t* stamp,
                                     const int64_t* step, int rule, const fil_rowopt_hyper* hyper, const float* lr_dev, void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_rowopt_runs_lrdev: no device rate (lr_dev is NULL)");
  return embed_rule_runs_launch<RowFamily>("fil_embed_rowopt_runs_lrdev", g, perm, sorted_ids, R, K, g_dtype, F, field_l2, table, accum, linear, stamp,
                                step, rule, hyper, stream, lr_dev);
}

extern "C" int fil_embed_rowopt_sweep(float* table, float* accum, float* linear, const int32_t* stamp, int64_t V, int K,
                                      const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F,
                                      const int64_t* step, int rule, const fil_rowopt_hyper* hyper, void* stream) {
  return embed_rule_sweep_launch<RowFamily>("fil_embed_rowopt_sweep", table, accum, linear, stamp, V, K, offsets, field_l2, frozen, F, step, rule,
                                 hyper, stream, nullptr);
}

extern "C" int fil_embed_rowopt_sweep_lrdev(float* table, float* accum, float* linear, const int32_t* stamp, int64_t V, int K,
                                      const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F,
                                      const int64_t* step, int rule, const fil_rowopt_hyper* hyper, const float* lr_dev, void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_rowopt_sweep_lrdev: no device rate (lr_dev is NULL)");
  return embed_rule_sweep_launch<RowFamily>("fil_embed_rowopt_sweep_lrdev", table, accum, linear, stamp, V, K, offsets, field_l2, frozen, F, step, rule,
                                 hyper, stream, lr_dev);
}

extern "C" int fil_embed_rowopt_merged(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                       const int64_t* offsets, const float* field_l2, int F, float* table, float* accum, float* linear,
                                       int32_t* stamp, int64_t V, const int64_t* step, int rule, const fil_rowopt_hyper* hyper,
                                       void* stream) {
  return embed_rule_merged_launch<RowFamily>("fil_embed_rowopt_merged", ids, values, counts, W, cap, K, offsets, field_l2, F, table, accum, linear,
                                  stamp, V, step, rule, hyper, stream, nullptr);
}

extern "C" int fil_embed_rowopt_merged_lrdev(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                       const int64_t* offsets, const float* field_l2, int F, float* table, float* accum, float* linear,
                                       int32_t* stamp, int64_t V, const int64_t* step, int rule, const fil_rowopt_hyper* hyper, const float* lr_dev,
                                       void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_rowopt_merged_lrdev: no device rate (lr_dev is NULL)");
  return embed_rule_merged_launch<RowFamily>("fil_embed_rowopt_merged_lrdev", ids, values, counts, W, cap, K, offsets, field_l2, F, table, accum,
                                  linear, stamp, V, step, rule, hyper, stream, lr_dev);
}
