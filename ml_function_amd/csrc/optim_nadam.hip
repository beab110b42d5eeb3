// O6  Keras-exact Nadam for gfx950: every dense fp32 tensor of a model in one launch, and the embedding tables updated in place from
// the batch's gradient runs (no dense [V,K] gradient), on the walks of optim_rows.h.
//
// The update is TF 2.1's (keras/optimizer_v2/nadam.py), fp32, every operation rounded as written (contraction off; correctly rounded
// division and square root).  Per step, with it = the completed steps, t = (float)(it + 1), n = (float)(it + 2), sd = schedule_decay and
// cache = the momentum cache (one fp32 word on the device, 1.0 before the first step):
//   mt  = b1 (1 - 0.5 powf(0.96, sd t))      mt1 = b1 (1 - 0.5 powf(0.96, sd n))      msn = cache mt      msx = msn mt1
//   omm = 1 - mt   omsn = 1 - msn   omsx = 1 - msx   vden = 1 - powf(b2, t)   omb1 = 1 - b1   omb2 = 1 - b2
// formed once per kernel (Rule::prepare: one wave-uniform load of the cache, one of the counter); per element
//   gp = g / omsn;  m = b1 m + omb1 g;  mp = m / omsx;  v = b2 v + omb2 (g g);  vp = v / vden
//   mbar = omm gp + mt1 mp;  p = p - (lr mbar) / (sqrt(vp) + eps)                                        m in `m`, v in `v`
// Keras' dense form and its IndexedSlices form are ONE fp32 computation here: they differ in the order of the factors of a product,
// which rounds the same, and in p + (-lr mbar) / d against p - (lr mbar) / d, which are the same bits.  So elem ignores kTouched.
// Which rows move: Keras assigns m = m b1 and v = v b2 over the WHOLE variable before it scatters the batch's rows, so the rule is not
// row-local -- like RMSprop with momentum == 0 its sweep walks every non-frozen field: an untouched row of an unregularised field decays
// both slots (16 bytes per element; the header's kDecayZ) and keeps p, one of a regularised field takes the rule with g = 2 l2 p.
// The step ends with ONE one-thread launch (Family::advance) that writes cache = cache mt(it) and then advances the counter, so every
// launch of a step reads the same cache and the same counter, and a captured step moves both on every replay.
// The kernels and the host launchers are optim_rule.h's; this file holds what is Nadam's own.
#include "optim_rule.h"

namespace fil {

struct NadamHyper {
  float lr, eps, b1, b2, sd;
  const float* cache;                                     // the momentum cache of the completed steps
  float mt, mt1, omm, omsn, omsx, vden, omb1, omb2;       // the step's eight coefficients: prepare()
};

// the momentum of step x (as a float: it + 1, or it + 2 for the look-ahead)
__device__ __forceinline__ float nadam_momentum(float b1, float sd, float x) {
#pragma clang fp contract(off)
  return b1 * (1.f - 0.5f * powf(0.96f, sd * x));
}

static const char* const kNadamScope[4] = {"nadam_multi", "embed_nadam_runs", "embed_nadam_sweep", "embed_nadam_merged"};

// s = m, z = v
struct NadamRule {
  using Hyper = NadamHyper;
  static constexpr bool kHasS = true, kHasZ = true, kSweepAll = true, kStepped = true, kDecayZ = true;
  static const char* scope(int launch) { return kNadamScope[launch]; }

  static __device__ __forceinline__ NadamHyper prepare(NadamHyper h, int64_t it) {
#pragma clang fp contract(off)
    const float t = (float)(it + 1), n = (float)(it + 2);
    const float cache = *h.cache;
    h.mt = nadam_momentum(h.b1, h.sd, t);
    h.mt1 = nadam_momentum(h.b1, h.sd, n);
    const float msn = cache * h.mt;
    const float msx = msn * h.mt1;
    h.omm = 1.f - h.mt;
    h.omsn = 1.f - msn;
    h.omsx = 1.f - msx;
    h.vden = 1.f - powf(h.b2, t);
    h.omb1 = 1.f - h.b1;
    h.omb2 = 1.f - h.b2;
    return h;
  }

  template <bool kTouched>
  static __device__ __forceinline__ void elem(float& p, float& s, float& z, float g, const NadamHyper& h) {
#pragma clang fp contract(off)
    const float gp = g / h.omsn;
    s = h.b1 * s + h.omb1 * g;
    const float mp = s / h.omsx;
    z = h.b2 * z + h.omb2 * (g * g);
    const float vp = z / h.vden;
    const float mbar = h.omm * gp + h.mt1 * mp;
    p = p - (h.lr * mbar) / (sqrtf(vp) + h.eps);
  }

  // an untouched row of an unregularised field: Keras' m = m beta_1, v = v beta_2 over the whole variable
  static __device__ __forceinline__ float decay(float s, const NadamHyper& h) { return s * h.b1; }
  static __device__ __forceinline__ float decay_z(float z, const NadamHyper& h) { return z * h.b2; }
};

// the last launch of a step: the cache takes the step's momentum, then the counter advances (one graph node)
__global__ void nadam_advance_kernel(int64_t* step, float* cache, float b1, float sd) {
#pragma clang fp contract(off)
  const int64_t it = *step;
  *cache = *cache * nadam_momentum(b1, sd, (float)(it + 1));
  *step = it + 1;
}

struct NadamFamily {
  using Raw = fil_nadam_hyper;

  static NadamHyper device(const Raw& h) {
    NadamHyper r = {};
    r.lr = h.lr;
    r.eps = h.epsilon;
    r.b1 = h.beta_1;
    r.b2 = h.beta_2;
    r.sd = h.schedule_decay;
    r.cache = h.m_cache;
    return r;
  }

  // the rule and its hyper-parameters (read here, on the host: a captured launch keeps the values it was captured with)
  static int resolve(const char* who, int rule, const Raw* h, int* var) {
    if (rule != FIL_OPT_NADAM) return fail(FIL_ERR_ARG, "%s: rule %d (FIL_OPT_NADAM)", who, rule);
    if (h == nullptr) return fail(FIL_ERR_ARG, "%s: no hyper-parameters (hyper is NULL)", who);
    if (h->m_cache == nullptr) return fail(FIL_ERR_ARG, "%s: no momentum cache (m_cache is NULL)", who);
    if (h->reserved != 0) return fail(FIL_ERR_ARG, "%s: reserved %d (0)", who, (int)h->reserved);
    if (!(h->lr >= 0.f) || !(h->epsilon >= 0.f) || !(h->schedule_decay >= 0.f) || !(h->beta_1 >= 0.f && h->beta_1 < 1.f) ||
        !(h->beta_2 >= 0.f && h->beta_2 < 1.f))
      return fail(FIL_ERR_ARG, "%s: Nadam hyper-parameters lr=%g beta_1=%g beta_2=%g epsilon=%g schedule_decay=%g (lr, epsilon, "
                  "schedule_decay >= 0; betas in [0, 1))", who, (double)h->lr, (double)h->beta_1, (double)h->beta_2, (double)h->epsilon,
                  (double)h->schedule_decay);
    *var = 0;
    return FIL_OK;
  }

  static int check_slots(const char* who, int var, const float* slot0, const float* slot1) {
    if (slot0 == nullptr) return fail(FIL_ERR_ARG, "%s: the rule needs its first slot (Nadam's m)", who);
    if (slot1 == nullptr) return fail(FIL_ERR_ARG, "%s: the rule needs its second slot (Nadam's v)", who);
    (void)var;
    return FIL_OK;
  }

  template <typename Fn>
  static int dispatch(int var, Fn&& f) {
    (void)var;
    return f(NadamRule{});
  }

  static void advance(int64_t* step, const Raw& h, hipStream_t st) {
    hipLaunchKernelGGL(nadam_advance_kernel, dim3(1), dim3(1), 0, st, step, h.m_cache, h.beta_1, h.schedule_decay);
  }
};

}  // namespace fil

using namespace fil;

extern "C" int fil_nadam_multi(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule,
                               const fil_nadam_hyper* hyper, int advance, void* stream) {
  return rule_multi_launch<NadamFamily>("fil_nadam_multi", tensors, n, total_numel, step, rule, hyper, advance, stream, nullptr);
}

extern "C" int fil_embed_nadam_runs(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                    const float* field_l2, float* table, float* slot0, float* slot1, int32_t* stamp, const int64_t* step,
                                    int rule, const fil_nadam_hyper* hyper, void* stream) {
  return embed_rule_runs_launch<NadamFamily>("fil_embed_nadam_runs", g, perm, sorted_ids, R, K, g_dtype, F, field_l2, table, slot0, slot1,
                                             stamp, step, rule, hyper, stream, nullptr);
}

extern "C" int fil_embed_nadam_sweep(float* table, float* slot0, float* slot1, const int32_t* stamp, int64_t V, int K,
                                     const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F,
                                     const int64_t* step, int rule, const fil_nadam_hyper* hyper, void* stream) {
  return embed_rule_sweep_launch<NadamFamily>("fil_embed_nadam_sweep", table, slot0, slot1, stamp, V, K, offsets, field_l2, frozen, F, step,
                                              rule, hyper, stream, nullptr);
}

extern "C" int fil_embed_nadam_merged(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                      const int64_t* offsets, const float* field_l2, int F, float* table, float* slot0, float* slot1,
                                      int32_t* stamp, int64_t V, const int64_t* step, int rule, const fil_nadam_hyper* hyper,
                                      void* stream) {
  return embed_rule_merged_launch<NadamFamily>("fil_embed_nadam_merged", ids, values, counts, W, cap, K, offsets, field_l2, F, table, slot0,
                                               slot1, stamp, V, step, rule, hyper, stream, nullptr);
}
