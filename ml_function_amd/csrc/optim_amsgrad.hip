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
// This file holds the dense element and kernel and the four O7 entry points.  The table kernels and every launcher body are Adam's
// own, defined once in optim_adam.h and instantiated here with the amsgrad slot: they form m and v through adam_touched /
// adam_untouched (contraction off, explicit fmas), so the table m and v of an amsgrad run are the bits of an Adam run on the same
// gradients; amsgrad_move, beside them, is the vhat step and the move.  The dense kernel is the walk of optim_rows.h over the
// five-array descriptor.  No lazy and no deferred mode: every runs update stamps, every step sweeps.
//
// The dense launch and the sweep stream: 16 bytes per lane and array where the arrays allow it (the sweep: 4 loads + 4 non-temporal
// stores of 16 B per lane, 32 bytes per element and step against Adam's 24), element-wise otherwise and in the tail.  The sweep
// skips a lane's vhat store when the bits it would write are the bits it read -- always so on an unregularised field, where an
// untouched row's v only decays: 28 bytes per element there (measured: 3.79 -> 3.38 ms at 33.8 M rows x K=16).  Every
// launch only READS the counter; fil_amsgrad_multi(advance = 1) bumps it in the one-thread launch behind its update.
#include "common.h"
#include "optim_rows.h"
#include "optim_adam.h"

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

// ---- fil_amsgrad_multi: the dense descriptors (multi_tensor_walk_desc, optim_rows.h) with the third slot, g += 2 l2 p where l2 is set
__global__ __launch_bounds__(256) void amsgrad_multi_kernel(const fil_amsgrad_tensor* __restrict__ ts, int n,
                                                            const int64_t* __restrict__ step, float lr, float b1, float b2, float eps,
                                                            const float* __restrict__ lr_dev) {
  const AdamCoef c = adam_coef(step, rate_of(lr, lr_dev), b1, b2, eps);
  multi_tensor_walk_desc<fil_amsgrad_tensor, true, true, true>(ts, n, [=](float& p, float& m, float& v, float& vhat, float g, float l2x2) {
    if (l2x2 != 0.f) g += l2x2 * p;
    amsgrad_elem(p, m, v, vhat, g, c);
  });
}

}  // namespace fil

using namespace fil;

extern "C" int fil_amsgrad_multi(const fil_amsgrad_tensor* tensors, int n, int64_t total_numel, int64_t* step, float lr,
                                 const float* lr_dev, float beta_1, float beta_2, float epsilon, int advance, void* stream) {
  return adam_multi_launch("fil_amsgrad_multi", "amsgrad_multi", 36.0, amsgrad_multi_kernel, tensors, n, total_numel, step, lr, lr_dev,
                           beta_1, beta_2, epsilon, advance, stream);
}

extern "C" int fil_embed_amsgrad_runs(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                      const float* field_l2, float* table, float* m, float* v, float* vhat, int32_t* stamp,
                                      const int64_t* step, float lr, const float* lr_dev, float beta_1, float beta_2, float epsilon,
                                      void* stream) {
  return embed_adam_runs_launch<true>("fil_embed_amsgrad_runs", g, perm, sorted_ids, R, K, g_dtype, F, field_l2, table, m, v, vhat, stamp,
                                      step, lr, lr_dev, beta_1, beta_2, epsilon, FIL_ADAM_KERAS, stream);
}

extern "C" int fil_embed_amsgrad_sweep(float* table, float* m, float* v, float* vhat, const int32_t* stamp, int64_t V, int K,
                                       const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F,
                                       const int64_t* step, float lr, const float* lr_dev, float beta_1, float beta_2, float epsilon,
                                       void* stream) {
  return embed_adam_sweep_launch<true>("fil_embed_amsgrad_sweep", table, m, v, vhat, stamp, V, K, offsets, field_l2, frozen, F, step, lr,
                                       lr_dev, beta_1, beta_2, epsilon, stream);
}

extern "C" int fil_embed_amsgrad_merged(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                        const int64_t* offsets, const float* field_l2, int F, float* table, float* m, float* v,
                                        float* vhat, int32_t* stamp, int64_t V, const int64_t* step, float lr, const float* lr_dev,
                                        float beta_1, float beta_2, float epsilon, void* stream) {
  return embed_adam_merged_launch<true>("fil_embed_amsgrad_merged", ids, values, counts, W, cap, K, offsets, field_l2, F, table, m, v, vhat,
                                        stamp, V, step, lr, lr_dev, beta_1, beta_2, epsilon, FIL_ADAM_KERAS, stream);
}
