// O5  Keras-exact Adadelta and Adamax for gfx950: every dense fp32 tensor of a model in one launch, and the embedding tables updated in
// place from the batch's gradient runs (no dense [V,K] gradient), on the walks of optim_rows.h.
//
// The updates are TF 2.1's (keras/optimizer_v2/adadelta.py, adamax.py; ApplyAdadelta / SparseApplyAdadelta and ApplyAdaMax in
// core/kernels/training_ops.cc; Adamax' IndexedSlices form is the Python of adamax.py), fp32, every operation rounded as written
// (contraction off), rsqrt(x) = 1 / sqrt(x):
//   Adadelta  dense = touched   ag = ag rho + (g g)(1 - rho);  upd = (sqrt(av + eps) (1 / sqrt(ag + eps))) g;  p = p - upd lr;
//                               av = av rho + (upd upd)(1 - rho)                                     accum_grad in `m`, accum_var in `v`
//   Adamax    dense             m += (g - m)(1 - b1);  v = max(b2 v, |g|);  p -= c (m / (v + eps))
//             touched           m = m b1 + g (1 - b1);  v = max(v b2, |g|);  p += (-c)(m / (v + eps))                  m in `m`, v in `v`
//             c = lr / (1 - powf(b1, (float)(iterations + 1))), formed once per kernel (Rule::prepare) from the device's step counter and
//             the step's rate -- by value or the device word of a schedule -- so a captured step takes the coefficient of each replay
// Both are row-local: the batch's rows (touched form), plus the untouched rows of the regularised fields (dense form, g = 2 l2 p) in a
// sweep of fil_embed_rowopt_sweep's shape; every other row and its slots keep their bits.
// The kernels and the host launchers are optim_rule.h's; this file holds what is Adadelta's and Adamax' own.
#include "optim_rule.h"

namespace fil {

enum { AV_ADADELTA = 0, AV_ADAMAX = 1 };

struct AdaHyper {
  float lr, eps, rho, omr, b1, omb1, b2;   // omr = 1 - rho, omb1 = 1 - beta_1, formed once in fp32; Adamax: lr becomes c in prepare()
};

static AdaHyper ada_hyper(const fil_adaopt_hyper& h) {
  AdaHyper r;
  r.lr = h.lr;
  r.eps = h.epsilon;
  r.rho = h.rho;
  r.omr = 1.f - h.rho;
  r.b1 = h.beta_1;
  r.omb1 = 1.f - h.beta_1;
  r.b2 = h.beta_2;
  return r;
}

// profile scope names, [launch][variant]
static const char* const kAdaScope[4][2] = {{"adadelta_multi", "adamax_multi"},
                                            {"embed_adadelta_runs", "embed_adamax_runs"},
                                            {"embed_adadelta_sweep", "embed_adamax_sweep"},
                                            {"embed_adadelta_merged", "embed_adamax_merged"}};

// s = the first slot (accum_grad / m), z = the second (accum_var / v)
template <int VAR>
struct AdaRule {
  using Hyper = AdaHyper;
  static constexpr bool kHasS = true, kHasZ = true, kSweepAll = false, kStepped = VAR == AV_ADAMAX;
  static const char* scope(int launch) { return kAdaScope[launch][VAR]; }

  // Adamax: the step size of step t = it + 1 (Keras: local_step = cast(iterations + 1, float32)) in place of the rate
  static __device__ __forceinline__ AdaHyper prepare(AdaHyper h, int64_t it) {
#pragma clang fp contract(off)
    h.lr = h.lr / (1.f - powf(h.b1, (float)(it + 1)));
    return h;
  }

  template <bool kTouched>
  static __device__ __forceinline__ void elem(float& p, float& s, float& z, float g, const AdaHyper& h) {
#pragma clang fp contract(off)
    if constexpr (VAR == AV_ADADELTA) {
      s = s * h.rho + (g * g) * h.omr;
      const float upd = (sqrtf(z + h.eps) * (1.f / sqrtf(s + h.eps))) * g;
      p = p - upd * h.lr;
      z = z * h.rho + (upd * upd) * h.omr;
    } else {
      if (kTouched) {
        s = s * h.b1 + g * h.omb1;
        z = fmaxf(z * h.b2, fabsf(g));
        p = p + (-h.lr) * (s / (z + h.eps));
      } else {
        s = s + (g - s) * h.omb1;
        z = fmaxf(h.b2 * z, fabsf(g));
        p = p - h.lr * (s / (z + h.eps));
      }
    }
  }
};

struct AdaFamily {
  using Raw = fil_adaopt_hyper;
  static AdaHyper device(const Raw& h) { return ada_hyper(h); }

  // the rule and its hyper-parameters (read here, on the host: a captured launch keeps the values it was captured with) -> the variant
  static int resolve(const char* who, int rule, const Raw* h, int* var) {
    if (rule != FIL_OPT_ADADELTA && rule != FIL_OPT_ADAMAX)
      return fail(FIL_ERR_ARG, "%s: rule %d (FIL_OPT_ADADELTA or FIL_OPT_ADAMAX)", who, rule);
    if (h == nullptr) return fail(FIL_ERR_ARG, "%s: no hyper-parameters (hyper is NULL)", who);
    if (rule == FIL_OPT_ADADELTA) {
      if (!(h->lr >= 0.f) || !(h->epsilon >= 0.f) || !(h->rho >= 0.f && h->rho <= 1.f))
        return fail(FIL_ERR_ARG, "%s: Adadelta hyper-parameters lr=%g rho=%g epsilon=%g (lr, epsilon >= 0; rho in [0, 1])", who,
                    (double)h->lr, (double)h->rho, (double)h->epsilon);
      *var = AV_ADADELTA;
      return FIL_OK;
    }
    if (!(h->lr >= 0.f) || !(h->epsilon >= 0.f) || !(h->beta_1 >= 0.f && h->beta_1 < 1.f) || !(h->beta_2 >= 0.f && h->beta_2 < 1.f))
      return fail(FIL_ERR_ARG, "%s: Adamax hyper-parameters lr=%g beta_1=%g beta_2=%g epsilon=%g (lr, epsilon >= 0; betas in [0, 1))", who,
                  (double)h->lr, (double)h->beta_1, (double)h->beta_2, (double)h->epsilon);
    *var = AV_ADAMAX;
    return FIL_OK;
  }

  // both rules have both slots
  static int check_slots(const char* who, int var, const float* slot0, const float* slot1) {
    if (slot0 == nullptr)
      return fail(FIL_ERR_ARG, "%s: the rule needs its first slot (Adadelta's accum_grad, Adamax' m)", who);
    if (slot1 == nullptr)
      return fail(FIL_ERR_ARG, "%s: the rule needs its second slot (Adadelta's accum_var, Adamax' v)", who);
    (void)var;
    return FIL_OK;
  }

  template <typename Fn>
  static int dispatch(int var, Fn&& f) {
    return var == AV_ADAMAX ? f(AdaRule<AV_ADAMAX>{}) : f(AdaRule<AV_ADADELTA>{});
  }
};

}  // namespace fil

using namespace fil;

extern "C" int fil_adaopt_multi(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule,
                                const fil_adaopt_hyper* hyper, int advance, void* stream) {
  return rule_multi_launch<AdaFamily>("fil_adaopt_multi", tensors, n, total_numel, step, rule, hyper, advance, stream, nullptr);
}

extern "C" int fil_adaopt_multi_lrdev(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule,
                                      const fil_adaopt_hyper* hyper, const float* lr_dev, int advance, void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_adaopt_multi_lrdev: no device rate (lr_dev is NULL)");
  return rule_multi_launch<AdaFamily>("fil_adaopt_multi_lrdev", tensors, n, total_numel, step, rule, hyper, advance, stream, lr_dev);
}

extern "C" int fil_embed_adaopt_runs(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                     const float* field_l2, float* table, float* slot0, float* slot1, int32_t* stamp,
                                     const int64_t* step, int rule, const fil_adaopt_hyper* hyper, void* stream) {
  return embed_rule_runs_launch<AdaFamily>("fil_embed_adaopt_runs", g, perm, sorted_ids, R, K, g_dtype, F, field_l2, table, slot0, slot1, stamp, step,
                                rule, hyper, stream, nullptr);
}

extern "C" int fil_embed_adaopt_runs_lrdev(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                           const float* field_l2, float* table, float* slot0, float* slot1, int32_t* stamp,
                                           const int64_t* step, int rule, const fil_adaopt_hyper* hyper, const float* lr_dev,
                                           void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_adaopt_runs_lrdev: no device rate (lr_dev is NULL)");
  return embed_rule_runs_launch<AdaFamily>("fil_embed_adaopt_runs_lrdev", g, perm, sorted_ids, R, K, g_dtype, F, field_l2, table, slot0, slot1, stamp,
                                step, rule, hyper, stream, lr_dev);
}

extern "C" int fil_embed_adaopt_sweep(float* table, float* slot0, float* slot1, const int32_t* stamp, int64_t V, int K,
                                      const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F,
                                      const int64_t* step, int rule, const fil_adaopt_hyper* hyper, void* stream) {
  return embed_rule_sweep_launch<AdaFamily>("fil_embed_adaopt_sweep", table, slot0, slot1, stamp, V, K, offsets, field_l2, frozen, F, step, rule,
                                 hyper, stream, nullptr);
}

extern "C" int fil_embed_adaopt_sweep_lrdev(float* table, float* slot0, float* slot1, const int32_t* stamp, int64_t V, int K,
                                            const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F,
                                            const int64_t* step, int rule, const fil_adaopt_hyper* hyper, const float* lr_dev,
                                            void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_adaopt_sweep_lrdev: no device rate (lr_dev is NULL)");
  return embed_rule_sweep_launch<AdaFamily>("fil_embed_adaopt_sweep_lrdev", table, slot0, slot1, stamp, V, K, offsets, field_l2, frozen, F, step, rule,
                                 hyper, stream, lr_dev);
}

extern "C" int fil_embed_adaopt_merged(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                       const int64_t* offsets, const float* field_l2, int F, float* table, float* slot0, float* slot1,
                                       int32_t* stamp, int64_t V, const int64_t* step, int rule, const fil_adaopt_hyper* hyper,
                                       void* stream) {
  return embed_rule_merged_launch<AdaFamily>("fil_embed_adaopt_merged", ids, values, counts, W, cap, K, offsets, field_l2, F, table, slot0, slot1,
                                  stamp, V, step, rule, hyper, stream, nullptr);
}

extern "C" int fil_embed_adaopt_merged_lrdev(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                             const int64_t* offsets, const float* field_l2, int F, float* table, float* slot0,
                                             float* slot1, int32_t* stamp, int64_t V, const int64_t* step, int rule,
                                             const fil_adaopt_hyper* hyper, const float* lr_dev, void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_adaopt_merged_lrdev: no device rate (lr_dev is NULL)");
  return embed_rule_merged_launch<AdaFamily>("fil_embed_adaopt_merged_lrdev", ids, values, counts, W, cap, K, offsets, field_l2, F, table, slot0,
                                  slot1, stamp, V, step, rule, hyper, stream, lr_dev);
}
