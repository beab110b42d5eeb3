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
// The kernels and the host launchers are optim_rule.h's; this file holds what is SGD's and RMSprop's own.
#include "optim_rule.h"

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

// profile scope names, [launch][variant]
static const char* const kMomScope[4][5] = {
    {"sgd_multi", "sgd_momentum_multi", "sgd_nesterov_multi", "rmsprop_multi", "rmsprop_momentum_multi"},
    {"embed_sgd_runs", "embed_sgd_momentum_runs", "embed_sgd_nesterov_runs", "embed_rmsprop_runs", "embed_rmsprop_momentum_runs"},
    {"embed_sgd_sweep", "embed_sgd_momentum_sweep", "embed_sgd_nesterov_sweep", "embed_rmsprop_sweep", "embed_rmsprop_momentum_sweep"},
    {"embed_sgd_merged", "embed_sgd_momentum_merged", "embed_sgd_nesterov_merged", "embed_rmsprop_merged", "embed_rmsprop_momentum_merged"}};

// s = the first slot (SGD's momentum accumulator, RMSprop's rms), z = RMSprop's momentum slot.  kTouched: the row arrived as
// IndexedSlices (the Sparse* op's form), else the dense op's form -- they differ for RMSprop only (for momentum == 0 only in the order
// of the factors, which rounds the same)
template <int VAR>
struct MomRule {
  using Hyper = MomHyper;
  static constexpr bool kHasS = VAR != MV_SGD, kHasZ = VAR == MV_RMSM, kSweepAll = VAR == MV_RMS;
  static const char* scope(int launch) { return kMomScope[launch][VAR]; }

  template <bool kTouched>
  static __device__ __forceinline__ void elem(float& p, float& s, float& z, float g, const MomHyper& h) {
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

  // RMSprop with momentum == 0: an untouched row of an unregularised field
  static __device__ __forceinline__ float decay(float s, const MomHyper& h) { return s * h.rho; }
};

struct MomFamily {
  using Raw = fil_momopt_hyper;
  static MomHyper device(const Raw& h) { return mom_hyper(h); }

  // the rule and its hyper-parameters (read here, on the host: a captured launch keeps the values it was captured with) -> the variant
  static int resolve(const char* who, int rule, const Raw* h, int* var) {
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

  // the slots the variant needs are there
  static int check_slots(const char* who, int var, const float* slot0, const float* slot1) {
    if (var != MV_SGD && slot0 == nullptr)
      return fail(FIL_ERR_ARG, "%s: the variant needs its first slot (SGD's momentum accumulator, RMSprop's rms)", who);
    if (var == MV_RMSM && slot1 == nullptr) return fail(FIL_ERR_ARG, "%s: RMSprop with momentum > 0 needs its momentum slot", who);
    return FIL_OK;
  }

  template <typename Fn>
  static int dispatch(int var, Fn&& f) {
    switch (var) {
      case MV_SGD: return f(MomRule<MV_SGD>{});
      case MV_SGDM: return f(MomRule<MV_SGDM>{});
      case MV_SGDN: return f(MomRule<MV_SGDN>{});
      case MV_RMS: return f(MomRule<MV_RMS>{});
      default: return f(MomRule<MV_RMSM>{});
    }
  }
};

}  // namespace fil

using namespace fil;

extern "C" int fil_momopt_multi(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule,
                                const fil_momopt_hyper* hyper, int advance, void* stream) {
  return rule_multi_launch<MomFamily>("fil_momopt_multi", tensors, n, total_numel, step, rule, hyper, advance, stream, nullptr);
}

extern "C" int fil_momopt_multi_lrdev(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule,
                                      const fil_momopt_hyper* hyper, const float* lr_dev, int advance, void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_momopt_multi_lrdev: no device rate (lr_dev is NULL)");
  return rule_multi_launch<MomFamily>("fil_momopt_multi_lrdev", tensors, n, total_numel, step, rule, hyper, advance, stream, lr_dev);
}

extern "C" int fil_embed_momopt_runs(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                     const float* field_l2, float* table, float* slot0, float* slot1, int32_t* stamp,
                                     const int64_t* step, int rule, const fil_momopt_hyper* hyper, void* stream) {
  return embed_rule_runs_launch<MomFamily>("fil_embed_momopt_runs", g, perm, sorted_ids, R, K, g_dtype, F, field_l2, table, slot0, slot1, stamp, step,
                                rule, hyper, stream, nullptr);
}

extern "C" int fil_embed_momopt_runs_lrdev(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                           const float* field_l2, float* table, float* slot0, float* slot1, int32_t* stamp,
                                           const int64_t* step, int rule, const fil_momopt_hyper* hyper, const float* lr_dev,
                                           void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_momopt_runs_lrdev: no device rate (lr_dev is NULL)");
  return embed_rule_runs_launch<MomFamily>("fil_embed_momopt_runs_lrdev", g, perm, sorted_ids, R, K, g_dtype, F, field_l2, table, slot0, slot1, stamp,
                                step, rule, hyper, stream, lr_dev);
}

extern "C" int fil_embed_momopt_sweep(float* table, float* slot0, float* slot1, const int32_t* stamp, int64_t V, int K,
                                      const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F,
                                      const int64_t* step, int rule, const fil_momopt_hyper* hyper, void* stream) {
  return embed_rule_sweep_launch<MomFamily>("fil_embed_momopt_sweep", table, slot0, slot1, stamp, V, K, offsets, field_l2, frozen, F, step, rule,
                                 hyper, stream, nullptr);
}

extern "C" int fil_embed_momopt_sweep_lrdev(float* table, float* slot0, float* slot1, const int32_t* stamp, int64_t V, int K,
                                            const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F,
                                            const int64_t* step, int rule, const fil_momopt_hyper* hyper, const float* lr_dev,
                                            void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_momopt_sweep_lrdev: no device rate (lr_dev is NULL)");
  return embed_rule_sweep_launch<MomFamily>("fil_embed_momopt_sweep_lrdev", table, slot0, slot1, stamp, V, K, offsets, field_l2, frozen, F, step, rule,
                                 hyper, stream, lr_dev);
}

extern "C" int fil_embed_momopt_merged(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                       const int64_t* offsets, const float* field_l2, int F, float* table, float* slot0, float* slot1,
                                       int32_t* stamp, int64_t V, const int64_t* step, int rule, const fil_momopt_hyper* hyper,
                                       void* stream) {
  return embed_rule_merged_launch<MomFamily>("fil_embed_momopt_merged", ids, values, counts, W, cap, K, offsets, field_l2, F, table, slot0, slot1,
                                  stamp, V, step, rule, hyper, stream, nullptr);
}

extern "C" int fil_embed_momopt_merged_lrdev(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                             const int64_t* offsets, const float* field_l2, int F, float* table, float* slot0,
                                             float* slot1, int32_t* stamp, int64_t V, const int64_t* step, int rule,
                                             const fil_momopt_hyper* hyper, const float* lr_dev, void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_momopt_merged_lrdev: no device rate (lr_dev is NULL)");
  return embed_rule_merged_launch<MomFamily>("fil_embed_momopt_merged_lrdev", ids, values, counts, W, cap, K, offsets, field_l2, F, table, slot0,
                                  slot1, stamp, V, step, rule, hyper, stream, lr_dev);
}
