// O3  Keras' learning-rate schedules (tf.keras.optimizers.schedules, TF 2.1) and OptimizerV2's legacy `decay`, evaluated on the
// device from the step counter: one one-thread launch per (step, device) writes the step's rate as one fp32, and every update
// launch of the step reads that word (the *_lrdev entry points of optim.hip / optim_rowwise.hip).  One place of rounding: the dense
// launch, the runs update, the sweep, the merged update and the deferred ring entry all see the same bits.
//
// Keras casts the step and every constant to fp32 and computes in fp32: each operation below rounds as written (contraction off),
// except the two powers, taken in fp64 and rounded once -- one thread, so fp64 is free, and the result is within one fp32 ulp of
// the formula with an exact power, whatever libm the host reference has.
#include "common.h"

namespace fil {

static_assert(sizeof(fil_lr_schedule) == 432, "fil_lr_schedule is 432 bytes (fil.h)");

__device__ __forceinline__ float pow_once(float base, float p) { return (float)pow((double)base, (double)p); }

__global__ void lr_schedule_eval_kernel(const fil_lr_schedule* __restrict__ sc, const int64_t* __restrict__ step,
                                        float* __restrict__ lr_out) {
#pragma clang fp contract(off)
  const int64_t it = *step;
  const float s = (float)it;
  float lr = sc->initial_lr;
  switch (sc->kind) {
    case FIL_LR_EXPONENTIAL: {
      float p = s / sc->decay_steps;
      if (sc->flag) p = floorf(p);
      lr = sc->initial_lr * pow_once(sc->decay_rate, p);
      break;
    }
    case FIL_LR_INVERSE_TIME: {
      float p = s / sc->decay_steps;
      if (sc->flag) p = floorf(p);
      const float denom = 1.f + sc->decay_rate * p;
      lr = sc->initial_lr / denom;
      break;
    }
    case FIL_LR_POLYNOMIAL: {
      float sr = s, d = sc->decay_steps;
      if (sc->flag) {
        const float mult = sr == 0.f ? 1.f : ceilf(sr / sc->decay_steps);
        d = d * mult;
      } else {
        sr = fminf(sr, sc->decay_steps);
      }
      const float p = sr / d;
      const float base = 1.f - p;
      const float pw = sc->power == 1.f ? base : pow_once(base, sc->power);
      const float span = sc->initial_lr - sc->end_lr;
      const float prod = span * pw;
      lr = prod + sc->end_lr;
      break;
    }
    case FIL_LR_PIECEWISE: {
      const int n = sc->n_boundaries < FIL_LR_MAX_BOUNDARIES ? sc->n_boundaries : FIL_LR_MAX_BOUNDARIES;
      int i = 0;
      while (i < n && it > sc->boundaries[i]) ++i;
      lr = sc->values[i];
      break;
    }
    default:
      break;
  }
  if (sc->decay > 0.f) {
    const float prod = sc->decay * s;
    const float denom = 1.f + prod;
    lr = lr / denom;
  }
  *lr_out = lr;
}

}  // namespace fil

using namespace fil;

extern "C" int fil_lr_schedule_check(const fil_lr_schedule* host_sched) {
  const fil_lr_schedule* s = host_sched;
  if (s == nullptr) return fail(FIL_ERR_ARG, "fil_lr_schedule_check: no descriptor (host_sched is NULL)");
  if (s->kind < FIL_LR_CONSTANT || s->kind > FIL_LR_PIECEWISE)
    return fail(FIL_ERR_ARG, "fil_lr_schedule_check: kind %d (FIL_LR_CONSTANT ... FIL_LR_PIECEWISE)", (int)s->kind);
  if (!(s->decay >= 0.f)) return fail(FIL_ERR_ARG, "fil_lr_schedule_check: decay %g (>= 0)", (double)s->decay);
  if ((s->kind == FIL_LR_EXPONENTIAL || s->kind == FIL_LR_INVERSE_TIME || s->kind == FIL_LR_POLYNOMIAL) && !(s->decay_steps > 0.f))
    return fail(FIL_ERR_ARG, "fil_lr_schedule_check: decay_steps %g (> 0)", (double)s->decay_steps);
  if (s->kind == FIL_LR_PIECEWISE) {
    if (s->n_boundaries < 1 || s->n_boundaries > FIL_LR_MAX_BOUNDARIES)
      return fail(FIL_ERR_ARG, "fil_lr_schedule_check: %d boundaries (1 ... FIL_LR_MAX_BOUNDARIES = %d)", (int)s->n_boundaries,
                  FIL_LR_MAX_BOUNDARIES);
    for (int i = 1; i < s->n_boundaries; ++i)
      if (s->boundaries[i] < s->boundaries[i - 1])
        return fail(FIL_ERR_ARG, "fil_lr_schedule_check: boundaries not sorted (boundaries[%d] = %lld < boundaries[%d] = %lld)", i,
                    (long long)s->boundaries[i], i - 1, (long long)s->boundaries[i - 1]);
  }
  return FIL_OK;
}

extern "C" int fil_lr_schedule_eval(const fil_lr_schedule* sched, const int64_t* step, float* lr_out, void* stream) {
  FIL_CHECK_ARG(sched != nullptr);
  FIL_CHECK_ARG(step != nullptr);
  FIL_CHECK_ARG(lr_out != nullptr);
  hipLaunchKernelGGL(lr_schedule_eval_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, sched, step, lr_out);
  FIL_CHECK_LAUNCH();
  return FIL_OK;
}
