// O1  Keras-exact Adam for gfx950: every dense fp32 tensor of a model in one launch, and the embedding tables updated in place from
// the batch's gradient runs (no dense [V,K] gradient, no zeroed table).
//
// The update is TensorFlow's ApplyAdam as Keras 'adam' (TF 2.1) drives it, in fp32:
//   t = step + 1;  alpha = lr sqrt(1 - b2^t) / (1 - b1^t);  m += (g - m)(1 - b1);  v += (g^2 - v)(1 - b2);  p -= (m alpha) / (sqrt(v) + eps)
// with b1^t, b2^t = powf(beta, (float)t) computed on the device from the int64 step counter, so a captured graph advances it on every
// replay.  Every launch only READS the counter; fil_adam_multi(advance = 1) bumps it in a one-thread launch behind its update.
//
// All three kernels are streaming: fil_adam_multi and fil_embed_adam_sweep move 16 bytes per lane and array where the arrays allow it
// (4 loads + 3 stores of 16 B per lane; 256-lane workgroups, a few per CU: ~64 KiB of loads in flight per CU), scalar otherwise and in
// the tail.  The sweep's stores are non-temporal (a 2 GB table pass must not evict the MALL).  fil_embed_adam_runs reuses the run sums
// of fil_embed_run_sum (embed_runs.h): the same order, so a row's gradient is bit-identical to what the dense path materialises.
// Data parallel: fil_embed_adam_merged applies the W gathered lists of fil_embed_runs_compact (runs_compact.hip) -- every row once,
// by its lowest rank, summed in rank order -- before the sweep, so every replica computes the same bits.
// This file holds Adam's dense kernel, the deferred mode and the O1 entry points.  The Keras-mode table kernels (runs, sweep, merged)
// and the launcher bodies of the dense, runs, sweep and merged launches are defined once in optim_adam.h, templated on whether the
// amsgrad slot travels along; the entry points here instantiate them without it, optim_amsgrad.hip (O7) with it.  The deferred
// kernels sit on a few pieces of their own: four elements of a row in and out (row_load4, row_store4) and one replayed step
// (replay_step); the field table of a sweep (FieldTab), the coefficients and the two table-element updates come from optim_adam.h,
// and what the launchers compute the same way as the row-rule optimizers' (grids, the step tag, sweep_vec, the shape check) from
// optim_rows.h and embed_runs.h.
#include "common.h"
#include "embed_runs.h"
#include "optim_rows.h"
#include "optim_adam.h"
#include <hip/hip_bf16.h>

namespace fil {

static_assert(sizeof(fil_adam_tensor) == 48, "fil_adam_tensor is 48 bytes (fil.h)");

// (the step's coefficients, adam_touched / adam_untouched -- the one definition of a table element's rounding, DESIGN 6e -- the
// sweep's field table, the hyper-parameter check and the Keras-mode runs, sweep and merged kernels: optim_adam.h, shared with
// optim_amsgrad.hip)

// one element of ApplyAdam (Eigen's order of operations), left to the compiler's contraction: fil_adam_multi only, whose dense
// tensors nothing replays
__device__ __forceinline__ void adam_elem(float& p, float& m, float& v, float g, const AdamCoef& c) {
  m += (g - m) * c.omb1;
  v += (g * g - v) * c.omb2;
  p -= (m * c.alpha) / (sqrtf(v) + c.eps);
}

// four elements of a row in and out: lane kq of the row's lane group holds elements kq * 4 ... kq * 4 + 3, those below K (the others
// read as 0 and are never stored)
__device__ __forceinline__ void row_load4(const float* __restrict__ table, const float* __restrict__ m, const float* __restrict__ v,
                                          int64_t row, int K, int kq, float (&p)[4], float (&mm)[4], float (&vv)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t e = row * K + kq * 4 + i;
    const bool in = kq * 4 + i < K;
    p[i] = in ? table[e] : 0.f;
    mm[i] = in ? m[e] : 0.f;
    vv[i] = in ? v[e] : 0.f;
  }
}

// kNT: non-temporal stores (the roll, as the sweep)
template <bool kNT>
__device__ __forceinline__ void row_store4(float* __restrict__ table, float* __restrict__ m, float* __restrict__ v, int64_t row, int K,
                                           int kq, const float (&p)[4], const float (&mm)[4], const float (&vv)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (kq * 4 + i < K) {
      const int64_t e = row * K + kq * 4 + i;
      if (kNT) {
        __builtin_nontemporal_store(p[i], table + e);
        __builtin_nontemporal_store(mm[i], m + e);
        __builtin_nontemporal_store(vv[i], v + e);
      } else {
        table[e] = p[i];
        m[e] = mm[i];
        v[e] = vv[i];
      }
    }
  }
}

// one replayed step on NE elements in registers.  vec: the sweep would take its 16-byte path on this table -- the only place that
// picks the rounding of a replay, which deferred mode's bit-identity to Keras mode rests on
template <int NE>
__device__ __forceinline__ void replay_step(float (&p)[NE], float (&m)[NE], float (&v)[NE], float l2x2, const AdamCoef& c, int vec) {
  if (vec) {
#pragma unroll
    for (int i = 0; i < NE; ++i) adam_untouched<true>(p[i], m[i], v[i], l2x2, c);
  } else {
#pragma unroll
    for (int i = 0; i < NE; ++i) adam_untouched<false>(p[i], m[i], v[i], l2x2, c);
  }
}

__global__ void step_advance_kernel(int64_t* step) { *step += 1; }

void launch_step_advance(int64_t* step, hipStream_t st) { hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, st, step); }

// ---- fil_adam_multi: the dense descriptors (multi_tensor_walk, optim_rows.h), g += 2 l2 p where l2 is set
__global__ __launch_bounds__(256) void adam_multi_kernel(const fil_adam_tensor* __restrict__ ts, int n, const int64_t* __restrict__ step,
                                                         float lr, float b1, float b2, float eps,
                                                         const float* __restrict__ lr_dev) {
  const AdamCoef c = adam_coef(step, rate_of(lr, lr_dev), b1, b2, eps);
  multi_tensor_walk<true>(ts, n, [=](float& p, float& m, float& v, float g, float l2x2) {
    if (l2x2 != 0.f) g += l2x2 * p;
    adam_elem(p, m, v, g, c);
  });
}

// ==== Deferred mode (optim.Adam(sweep_period=N)).  A row the batch did not touch takes g = 2 l2 p: an update that depends
// on the row's own (p, m, v), its field's l2 and the step's coefficients only.  So the steps a row misses can be applied later, with
// the same fp32 operations in the same order, and give the sweep's bits.  Persistent state per table:
//   stamp [V] int32  stamp[r] = s: row r is current through completed step s (low 32 bits of the step count);
//   ring  [D] AdamCoef (D a power of two >= N + 1): entry t mod D = adam_coef of step t (1-based), or the skip entry of a step at
//         which the table had no record (Keras mode leaves such a table alone).  Written once, by fil_embed_adam_roll of step t.
// fil_embed_adam_roll catches up slice (t mod N) of ceil(V/N) rows through step t at every step, so no row is ever more than N steps
// behind: every replay reads at most the N newest entries, and D >= N + 1 keeps the entry being written out of their way.
constexpr int kRingMax = 1024;                 // D <= 1024 (the roll keeps the ring in LDS): sweep_period <= 1023

// The replays go through adam_untouched, the sweep's own update (optim_adam.h): a replayed step rounds as the sweep would have rounded it.
__device__ __forceinline__ bool coef_is_skip(const AdamCoef& c) { return c.omb1 != c.omb1; }   // (1 - beta_1 is never NaN)

__device__ __forceinline__ AdamCoef coef_skip() {
  const float nan = __builtin_nanf("");
  return AdamCoef{nan, nan, nan, nan};
}

static int ring_len(int N) {
  if (N < 1 || N >= kRingMax) return 0;
  int D = 1;
  while (D < N + 1) D <<= 1;
  return D;
}

// the last completed step a row stamped `st` must replay from to reach `to`: `to` itself when it is current.  Never more than N
// steps back (a longer gap only comes from a broken protocol: the replay stays bounded, it does not hang)
__device__ __forceinline__ int32_t replay_from(int32_t st, int32_t to, int N) {
  if (st >= to) return to;
  return st < to - N ? to - N : st;
}

// steps (from, to] of the ring (global memory) on NE elements in registers
template <int NE>
__device__ __forceinline__ void replay(float (&p)[NE], float (&m)[NE], float (&v)[NE], float l2x2, int32_t from, int32_t to,
                                       const AdamCoef* __restrict__ ring, int D, int vec) {
  for (int32_t u = from + 1; u <= to; ++u) {
    const AdamCoef c = ring[u & (D - 1)];
    if (coef_is_skip(c)) continue;
    replay_step(p, m, v, l2x2, c, vec);
  }
}

// ---- fil_embed_adam_catchup_runs: the forward's launch.  G lanes (a power of two, so a row never straddles a wave) per sorted
// position; the position that starts a run owns its row, brings it current through the completed steps and stamps it.
__global__ __launch_bounds__(256) void embed_adam_catchup_kernel(const int64_t* __restrict__ sorted_ids, long R, int K, int lgG,
                                                                 float* __restrict__ table, float* __restrict__ m, float* __restrict__ v,
                                                                 int32_t* __restrict__ stamp, const AdamCoef* __restrict__ ring, int D,
                                                                 int N, const int64_t* __restrict__ offsets,
                                                                 const float* __restrict__ field_l2, const unsigned char* __restrict__ frozen,
                                                                 int F, int64_t V, const int64_t* __restrict__ step, int vec) {
  __shared__ FieldTab s;
  load_field_tab(&s, offsets, field_l2, frozen, F);
  __syncthreads();
  const int32_t to = (int32_t)(uint32_t)(*step);
  const long total = R << lgG;
  const int kq = threadIdx.x & ((1 << lgG) - 1);
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const long j = q >> lgG;
    const int64_t row = sorted_ids[j];
    if (row < 0 || row >= V || (j > 0 && sorted_ids[j - 1] == row)) continue;
    const float l2x2 = field_l2x2(&s, F, row);
    if (l2x2 != l2x2) continue;                   // frozen
    const int32_t from = replay_from(stamp[row], to, N);
    if (from == to) continue;
    if (kq * 4 < K) {
      float p[4], mm[4], vv[4];
      row_load4(table, m, v, row, K, kq, p, mm, vv);
      replay(p, mm, vv, l2x2, from, to, ring, D, vec);
      row_store4<false>(table, m, v, row, K, kq, p, mm, vv);
    }
    if (kq == 0) stamp[row] = to;                 // (the row's other lanes read the stamp above: same wave, earlier instruction)
  }
}

// ---- the deferred runs update: embed_adam_runs_kernel's epilogue behind a catch-up of the row through the completed steps; the row
// is then stamped with step t.
template <typename GT>
__global__ __launch_bounds__(256) void embed_adam_runs_deferred_kernel(const GT* __restrict__ g, const int64_t* __restrict__ perm,
                                                                       const int64_t* __restrict__ sorted_ids, long R, int K, int F,
                                                                       const int64_t* __restrict__ offsets,
                                                                       const float* __restrict__ field_l2,
                                                                       const unsigned char* __restrict__ frozen, float* __restrict__ table,
                                                                       float* __restrict__ m, float* __restrict__ v,
                                                                       int32_t* __restrict__ stamp, const AdamCoef* __restrict__ ring,
                                                                       int D, int N, int64_t V, const int64_t* __restrict__ step,
                                                                       float lr, float b1, float b2, float eps, int vec,
                                                                       const float* __restrict__ lr_dev) {
  __shared__ FieldTab s;
  load_field_tab(&s, offsets, field_l2, frozen, F);
  __syncthreads();
  const FieldTab* sp = &s;
  const AdamCoef c = adam_coef(step, rate_of(lr, lr_dev), b1, b2, eps);
  const int32_t done = (int32_t)(uint32_t)(*step);
  embed_run_sums(g, perm, sorted_ids, R, K, [=](int64_t row, int kq, const float (&acc)[4], int64_t first) {
    if (row >= V) return;
    const float l2x2 = field_l2 ? 2.f * field_l2[first % F] : 0.f;      // step t's term, as embed_adam_runs_kernel
    const float r2 = field_l2x2(sp, F, row);                             // the replayed steps' term, as the sweep
    const int32_t from = r2 == r2 ? replay_from(stamp[row], done, N) : done;
    float p[4], mm[4], vv[4];
    row_load4(table, m, v, row, K, kq, p, mm, vv);
    replay(p, mm, vv, r2, from, done, ring, D, vec);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (kq * 4 + i < K) adam_touched(p[i], mm[i], vv[i], acc[i], l2x2, c);
    row_store4<false>(table, m, v, row, K, kq, p, mm, vv);
    if (kq == 0) stamp[row] = done + 1;
  });
}

// ---- the deferred merged update: embed_adam_merged_kernel with the owner catching its row up before the update
__global__ __launch_bounds__(256) void embed_adam_merged_deferred_kernel(const int64_t* __restrict__ ids, const float* __restrict__ values,
                                                                         const int64_t* __restrict__ counts, int W, long cap, int K,
                                                                         const int64_t* __restrict__ offsets,
                                                                         const float* __restrict__ field_l2,
                                                                         const unsigned char* __restrict__ frozen, int F,
                                                                         float* __restrict__ table, float* __restrict__ m,
                                                                         float* __restrict__ v, int32_t* __restrict__ stamp,
                                                                         const AdamCoef* __restrict__ ring, int D, int N, int64_t V,
                                                                         const int64_t* __restrict__ step, float lr, float b1, float b2,
                                                                         float eps, int vec, const float* __restrict__ lr_dev) {
  __shared__ FieldTab s;
  load_field_tab(&s, offsets, field_l2, frozen, F);
  __syncthreads();
  const FieldTab* sp = &s;
  const AdamCoef c = adam_coef(step, rate_of(lr, lr_dev), b1, b2, eps);
  const int32_t done = (int32_t)(uint32_t)(*step);
  const auto epi = [=](int64_t row, int f, float l2x2, int k0, const float (&acc)[kMergeChunk]) {
    const float r2 = f >= 0 ? sp->l2x2[f] : 0.f;
    const int32_t from = r2 == r2 ? replay_from(stamp[row], done, N) : done;     // (the stamp moves after the last chunk only)
    // (element by element: four at a time on the row helpers costs 33 registers and three waves of occupancy)
#pragma unroll
    for (int e = 0; e < kMergeChunk; ++e) {
      if (k0 + e < K) {
        const int64_t x = row * K + k0 + e;
        float p[1] = {table[x]}, mm[1] = {m[x]}, vv[1] = {v[x]};
        replay(p, mm, vv, r2, from, done, ring, D, vec);
        adam_touched(p[0], mm[0], vv[0], acc[e], l2x2, c);
        table[x] = p[0];
        m[x] = mm[0];
        v[x] = vv[0];
      }
    }
  };
  merged_row_sums((long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x, ids, values, counts, W, cap, K, V, s.off,
                  field_l2, F, epi, [=](int64_t row) { stamp[row] = done + 1; });
}

// ---- fil_embed_adam_roll: step t's ring entry (or the skip entry), then slice t mod N of ceil(V/N) rows brought current through
// step t; FLUSH: every row through the completed steps, no entry.  VALU-bound by design: the ring sits in LDS and a wave replays
// from its lowest stamp -- the rows of a slice almost all have the same gap N, so the loop is uniform and its second part runs
// unmasked.  16-byte accesses where K % 4 == 0 and the arrays allow it, non-temporal stores, as the sweep.
constexpr int kRollSkip = 1, kRollFlush = 2;

__global__ __launch_bounds__(256) void embed_adam_roll_kernel(float* __restrict__ table, float* __restrict__ m, float* __restrict__ v,
                                                              int32_t* __restrict__ stamp, AdamCoef* __restrict__ ring, int D, int N,
                                                              int64_t V, int K, int lgG, int vec, const int64_t* __restrict__ offsets,
                                                              const float* __restrict__ field_l2, const unsigned char* __restrict__ frozen,
                                                              int F, const int64_t* __restrict__ step, float lr, float b1, float b2,
                                                              float eps, int flags, const float* __restrict__ lr_dev) {
  __shared__ FieldTab s;
  __shared__ AdamCoef s_ring[kRingMax];
  const bool flush = (flags & kRollFlush) != 0;
  const int64_t done = *step;
  const int32_t to = (int32_t)(uint32_t)(flush ? done : done + 1);
  load_field_tab(&s, offsets, field_l2, frozen, F);
  for (int i = threadIdx.x; i < D; i += blockDim.x) s_ring[i] = ring[i];
  __syncthreads();
  int64_t lo = 0, hi = V;
  if (!flush) {
    // step t's entry: every workgroup holds its own copy (the global one is for later launches only)
    const AdamCoef ct = (flags & kRollSkip) ? coef_skip() : adam_coef(step, rate_of(lr, lr_dev), b1, b2, eps);
    if (threadIdx.x == 0) {
      s_ring[to & (D - 1)] = ct;
      if (blockIdx.x == 0) ring[to & (D - 1)] = ct;
    }
    __syncthreads();
    const int64_t S = (V + N - 1) / N;
    lo = ((done + 1) % N) * S;
    hi = lo + S < V ? lo + S : V;
    if (lo > hi) lo = hi;
  }
  const int64_t total = (hi - lo) << lgG;
  const int G = 1 << lgG;
  const int kq = threadIdx.x & (G - 1);
  // (a wave-uniform loop: every lane runs the same iterations, so the cross-lane minimum below sees all 64 lanes)
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < total; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = base + threadIdx.x;
    const int64_t row = lo + (q >> lgG);
    int32_t from = to;
    float l2x2 = 0.f;
    if (q < total) {
      l2x2 = field_l2x2(&s, F, row);
      if (l2x2 == l2x2) from = replay_from(stamp[row], to, N);
    }
    const bool act = from != to;
    int32_t wlo = from, whi = act ? from : INT32_MIN;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      wlo = min(wlo, __shfl_xor(wlo, o, 64));
      whi = max(whi, __shfl_xor(whi, o, 64));
    }
    wlo = __builtin_amdgcn_readfirstlane(wlo);
    whi = __builtin_amdgcn_readfirstlane(whi);
    if (wlo == to) continue;                      // the whole wave is current
    const bool mine = act && kq * 4 < K;
    const int64_t e0 = row * K + kq * 4;
    float p[4] = {0.f, 0.f, 0.f, 0.f}, mm[4] = {0.f, 0.f, 0.f, 0.f}, vv[4] = {0.f, 0.f, 0.f, 0.f};
    if (mine) {
      if (vec) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(table + e0);
        const f32x4 b = *reinterpret_cast<const f32x4*>(m + e0);
        const f32x4 c = *reinterpret_cast<const f32x4*>(v + e0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          p[i] = a[i];
          mm[i] = b[i];
          vv[i] = c[i];
        }
      } else {
        row_load4(table, m, v, row, K, kq, p, mm, vv);
      }
    }
    // steps the wave's rows disagree on (masked per lane), then the ones every row takes (lanes with nothing to do compute on
    // zeros they never store)
    int32_t u = wlo + 1;
    for (; u <= whi; ++u) {
      const AdamCoef c = s_ring[u & (D - 1)];
      if (coef_is_skip(c)) continue;
      if (u > from) replay_step(p, mm, vv, l2x2, c, vec);
    }
    for (; u <= to; ++u) {
      const AdamCoef c = s_ring[u & (D - 1)];
      if (coef_is_skip(c)) continue;
      replay_step(p, mm, vv, l2x2, c, vec);
    }
    if (mine) {
      if (vec) {
        __builtin_nontemporal_store(f32x4{p[0], p[1], p[2], p[3]}, reinterpret_cast<f32x4*>(table + e0));
        __builtin_nontemporal_store(f32x4{mm[0], mm[1], mm[2], mm[3]}, reinterpret_cast<f32x4*>(m + e0));
        __builtin_nontemporal_store(f32x4{vv[0], vv[1], vv[2], vv[3]}, reinterpret_cast<f32x4*>(v + e0));
      } else {
        row_store4<true>(table, m, v, row, K, kq, p, mm, vv);
      }
    }
    if (act && kq == 0) stamp[row] = to;
  }
}

// lanes per row of the deferred kernels: the power of two >= ceil(K / 4)
static int lanes_lg(int K) {
  int lg = 0;
  while ((1 << lg) < (K + 3) / 4) ++lg;
  return lg;
}

static int check_deferred(const char* who, int K, int F, int N, const float* ring) {
  if (int rc = check_table_shape(who, K, F)) return rc;
  if (ring_len(N) == 0) return fail(FIL_ERR_ARG, "%s: sweep_period %d (1 ... %d)", who, N, kRingMax - 1);
  if (((uintptr_t)ring & 15) != 0) return fail(FIL_ERR_ARG, "%s: the ring must be 16-byte aligned", who);
  return FIL_OK;
}

}  // namespace fil

using namespace fil;

// ---- the dense launch and the Keras / lazy mode table updates: the launchers of optim_adam.h without the amsgrad slot.  A _lrdev
// twin passes lr = 0 and its device rate.
extern "C" int fil_adam_multi(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, float lr, float beta_1,
                              float beta_2, float epsilon, int advance, void* stream) {
  return adam_multi_launch("fil_adam_multi", "adam_multi", 28.0, adam_multi_kernel, tensors, n, total_numel, step, lr, nullptr, beta_1,
                           beta_2, epsilon, advance, stream);
}

extern "C" int fil_adam_multi_lrdev(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, const float* lr_dev, float beta_1,
                              float beta_2, float epsilon, int advance, void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_adam_multi_lrdev: no device rate (lr_dev is NULL)");
  return adam_multi_launch("fil_adam_multi_lrdev", "adam_multi", 28.0, adam_multi_kernel, tensors, n, total_numel, step, 0.f, lr_dev,
                           beta_1, beta_2, epsilon, advance, stream);
}

extern "C" int fil_embed_adam_runs(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                   const float* field_l2, float* table, float* m, float* v, int32_t* stamp, const int64_t* step,
                                   float lr, float beta_1, float beta_2, float epsilon, int mode, void* stream) {
  return embed_adam_runs_launch<false>("fil_embed_adam_runs", g, perm, sorted_ids, R, K, g_dtype, F, field_l2, table, m, v, nullptr, stamp,
                                       step, lr, nullptr, beta_1, beta_2, epsilon, mode, stream);
}

extern "C" int fil_embed_adam_runs_lrdev(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                   const float* field_l2, float* table, float* m, float* v, int32_t* stamp, const int64_t* step,
                                   const float* lr_dev, float beta_1, float beta_2, float epsilon, int mode, void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_adam_runs_lrdev: no device rate (lr_dev is NULL)");
  return embed_adam_runs_launch<false>("fil_embed_adam_runs_lrdev", g, perm, sorted_ids, R, K, g_dtype, F, field_l2, table, m, v, nullptr,
                                       stamp, step, 0.f, lr_dev, beta_1, beta_2, epsilon, mode, stream);
}

extern "C" int fil_embed_adam_sweep(float* table, float* m, float* v, const int32_t* stamp, int64_t V, int K, const int64_t* offsets,
                                    const float* field_l2, const unsigned char* frozen, int F, const int64_t* step, float lr,
                                    float beta_1, float beta_2, float epsilon, void* stream) {
  return embed_adam_sweep_launch<false>("fil_embed_adam_sweep", table, m, v, nullptr, stamp, V, K, offsets, field_l2, frozen, F, step, lr,
                                        nullptr, beta_1, beta_2, epsilon, stream);
}

extern "C" int fil_embed_adam_sweep_lrdev(float* table, float* m, float* v, const int32_t* stamp, int64_t V, int K, const int64_t* offsets,
                                    const float* field_l2, const unsigned char* frozen, int F, const int64_t* step, const float* lr_dev,
                                    float beta_1, float beta_2, float epsilon, void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_adam_sweep_lrdev: no device rate (lr_dev is NULL)");
  return embed_adam_sweep_launch<false>("fil_embed_adam_sweep_lrdev", table, m, v, nullptr, stamp, V, K, offsets, field_l2, frozen, F, step,
                                        0.f, lr_dev, beta_1, beta_2, epsilon, stream);
}

extern "C" int fil_embed_adam_merged(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                     const int64_t* offsets, const float* field_l2, int F, float* table, float* m, float* v, int32_t* stamp,
                                     int64_t V, const int64_t* step, float lr, float beta_1, float beta_2, float epsilon, int mode,
                                     void* stream) {
  return embed_adam_merged_launch<false>("fil_embed_adam_merged", ids, values, counts, W, cap, K, offsets, field_l2, F, table, m, v, nullptr,
                                         stamp, V, step, lr, nullptr, beta_1, beta_2, epsilon, mode, stream);
}

extern "C" int fil_embed_adam_merged_lrdev(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                     const int64_t* offsets, const float* field_l2, int F, float* table, float* m, float* v, int32_t* stamp,
                                     int64_t V, const int64_t* step, const float* lr_dev, float beta_1, float beta_2, float epsilon, int mode,
                                     void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_adam_merged_lrdev: no device rate (lr_dev is NULL)");
  return embed_adam_merged_launch<false>("fil_embed_adam_merged_lrdev", ids, values, counts, W, cap, K, offsets, field_l2, F, table, m, v,
                                         nullptr, stamp, V, step, 0.f, lr_dev, beta_1, beta_2, epsilon, mode, stream);
}

extern "C" int fil_embed_adam_ring_len(int sweep_period) { return ring_len(sweep_period); }

extern "C" int fil_embed_adam_catchup_runs(const int64_t* sorted_ids, long R, int K, float* table, float* m, float* v, int32_t* stamp,
                                           const float* ring, int sweep_period, const int64_t* offsets, const float* field_l2,
                                           const unsigned char* frozen, int F, int64_t V, const int64_t* step, void* stream) {
  FIL_CHECK_ARG(R >= 0 && K >= 1 && F >= 1 && V >= 0);
  if (int rc = check_deferred("fil_embed_adam_catchup_runs", K, F, sweep_period, ring)) return rc;
  if (R == 0 || V == 0) return FIL_OK;
  FIL_CHECK_ARG(sorted_ids && table && m && v && stamp && ring && offsets && step);
  hipStream_t st = (hipStream_t)stream;
  const int lg = lanes_lg(K);
  const long total = R << lg;
  ProfScope ps("embed_adam_catchup", st, 8.0 * R);
  const dim3 grid = stride_grid(total);
  hipLaunchKernelGGL(embed_adam_catchup_kernel, grid, dim3(256), 0, st, sorted_ids, R, K, lg, table, m, v, stamp,
                     reinterpret_cast<const AdamCoef*>(ring), ring_len(sweep_period), sweep_period, offsets, field_l2, frozen, F, V, step,
                     sweep_vec(K, table, m, v));
  FIL_CHECK_LAUNCH();
  return FIL_OK;
}

static int embed_adam_runs_deferred_impl(const char* who, const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K,
                                         int g_dtype, int F, const int64_t* offsets, const float* field_l2, const unsigned char* frozen,
                                         float* table, float* m, float* v, int32_t* stamp, const float* ring, int sweep_period, int64_t V,
                                         const int64_t* step, float lr, float beta_1, float beta_2, float epsilon, void* stream,
                                         const float* lr_dev) {
  FIL_CHECK_ARG_W(who, R >= 0 && K >= 1 && F >= 1 && V >= 0);
  if (g_dtype != FIL_F32 && g_dtype != FIL_BF16) return fail(FIL_ERR_ARG, "%s: g_dtype %d (f32 or bf16)", who, g_dtype);
  if (int rc = check_deferred(who, K, F, sweep_period, ring)) return rc;
  if (int rc = check_hyper(who, lr, beta_1, beta_2, epsilon)) return rc;
  if (R == 0 || V == 0) return FIL_OK;
  FIL_CHECK_ARG_W(who, g && perm && sorted_ids && offsets && table && m && v && stamp && ring && step);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("embed_adam_runs_deferred", st, (double)R * K * (g_dtype == FIL_F32 ? 4 : 2) + 24.0 * R * K);
  const dim3 grid = run_sums_grid(R, K);
  const AdamCoef* rg = reinterpret_cast<const AdamCoef*>(ring);
  const int D = ring_len(sweep_period);
  if (g_dtype == FIL_F32)
    hipLaunchKernelGGL(embed_adam_runs_deferred_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(g), perm, sorted_ids, R,
                       K, F, offsets, field_l2, frozen, table, m, v, stamp, rg, D, sweep_period, V, step, lr, beta_1, beta_2, epsilon,
                       sweep_vec(K, table, m, v), lr_dev);
  else
    hipLaunchKernelGGL(embed_adam_runs_deferred_kernel<__hip_bfloat16>, grid, dim3(256), 0, st, static_cast<const __hip_bfloat16*>(g),
                       perm, sorted_ids, R, K, F, offsets, field_l2, frozen, table, m, v, stamp, rg, D, sweep_period, V, step, lr, beta_1,
                       beta_2, epsilon, sweep_vec(K, table, m, v), lr_dev);
  FIL_CHECK_LAUNCH_W(who);
  return FIL_OK;
}

extern "C" int fil_embed_adam_runs_deferred(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype,
                                            int F, const int64_t* offsets, const float* field_l2, const unsigned char* frozen, float* table,
                                            float* m, float* v, int32_t* stamp, const float* ring, int sweep_period, int64_t V,
                                            const int64_t* step, float lr, float beta_1, float beta_2, float epsilon, void* stream) {
  return embed_adam_runs_deferred_impl("fil_embed_adam_runs_deferred", g, perm, sorted_ids, R, K, g_dtype, F, offsets, field_l2, frozen,
                                       table, m, v, stamp, ring, sweep_period, V, step, lr, beta_1, beta_2, epsilon, stream, nullptr);
}

extern "C" int fil_embed_adam_runs_deferred_lrdev(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype,
                                            int F, const int64_t* offsets, const float* field_l2, const unsigned char* frozen, float* table,
                                            float* m, float* v, int32_t* stamp, const float* ring, int sweep_period, int64_t V,
                                            const int64_t* step, const float* lr_dev, float beta_1, float beta_2, float epsilon, void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_adam_runs_deferred_lrdev: no device rate (lr_dev is NULL)");
  return embed_adam_runs_deferred_impl("fil_embed_adam_runs_deferred_lrdev", g, perm, sorted_ids, R, K, g_dtype, F, offsets, field_l2,
                                       frozen, table, m, v, stamp, ring, sweep_period, V, step, 0.f, beta_1, beta_2, epsilon, stream,
                                       lr_dev);
}

static int embed_adam_merged_deferred_impl(const char* who, const int64_t* ids, const float* values, const int64_t* counts, int W, long cap,
                                           int K, const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F,
                                           float* table, float* m, float* v, int32_t* stamp, const float* ring, int sweep_period,
                                           int64_t V, const int64_t* step, float lr, float beta_1, float beta_2, float epsilon,
                                           void* stream, const float* lr_dev) {
  FIL_CHECK_ARG_W(who, W >= 1 && cap >= 0 && K >= 1 && F >= 1 && V >= 0);
  if (int rc = check_deferred(who, K, F, sweep_period, ring)) return rc;
  if (int rc = check_hyper(who, lr, beta_1, beta_2, epsilon)) return rc;
  if (cap == 0 || V == 0) return FIL_OK;
  FIL_CHECK_ARG_W(who, ids && values && counts && offsets && table && m && v && stamp && ring && step);
  hipStream_t st = (hipStream_t)stream;
  const long n = (long)W * cap;
  ProfScope ps("embed_adam_merged_deferred", st, 8.0 * n + 4.0 * (double)n * K + 24.0 * (double)cap * K);
  const dim3 grid = stride_grid(n);
  hipLaunchKernelGGL(embed_adam_merged_deferred_kernel, grid, dim3(256), 0, st, ids, values, counts, W, cap, K, offsets, field_l2, frozen,
                     F, table, m, v, stamp, reinterpret_cast<const AdamCoef*>(ring), ring_len(sweep_period), sweep_period, V, step, lr,
                     beta_1, beta_2, epsilon, sweep_vec(K, table, m, v), lr_dev);
  FIL_CHECK_LAUNCH_W(who);
  return FIL_OK;
}

extern "C" int fil_embed_adam_merged_deferred(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                              const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F,
                                              float* table, float* m, float* v, int32_t* stamp, const float* ring, int sweep_period,
                                              int64_t V, const int64_t* step, float lr, float beta_1, float beta_2, float epsilon,
                                              void* stream) {
  return embed_adam_merged_deferred_impl("fil_embed_adam_merged_deferred", ids, values, counts, W, cap, K, offsets, field_l2, frozen, F,
                                         table, m, v, stamp, ring, sweep_period, V, step, lr, beta_1, beta_2, epsilon, stream, nullptr);
}

extern "C" int fil_embed_adam_merged_deferred_lrdev(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                              const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F,
                                              float* table, float* m, float* v, int32_t* stamp, const float* ring, int sweep_period,
                                              int64_t V, const int64_t* step, const float* lr_dev, float beta_1, float beta_2, float epsilon,
                                              void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_adam_merged_deferred_lrdev: no device rate (lr_dev is NULL)");
  return embed_adam_merged_deferred_impl("fil_embed_adam_merged_deferred_lrdev", ids, values, counts, W, cap, K, offsets, field_l2, frozen,
                                         F, table, m, v, stamp, ring, sweep_period, V, step, 0.f, beta_1, beta_2, epsilon, stream, lr_dev);
}

static int embed_adam_roll_impl(const char* who, float* table, float* m, float* v, int32_t* stamp, float* ring, int sweep_period, int64_t V,
                                int K, const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F, const int64_t* step,
                                float lr, float beta_1, float beta_2, float epsilon, int flags, void* stream, const float* lr_dev) {
  FIL_CHECK_ARG_W(who, V >= 0 && K >= 1 && F >= 1);
  if (flags != FIL_ADAM_ROLL_STEP && flags != FIL_ADAM_ROLL_SKIP && flags != FIL_ADAM_ROLL_FLUSH)
    return fail(FIL_ERR_ARG, "%s: flags %d (FIL_ADAM_ROLL_STEP, _SKIP or _FLUSH)", who, flags);
  if (int rc = check_deferred(who, K, F, sweep_period, ring)) return rc;
  if (int rc = check_hyper(who, lr, beta_1, beta_2, epsilon)) return rc;
  if (V == 0) return FIL_OK;
  FIL_CHECK_ARG_W(who, table && m && v && stamp && ring && offsets && step);
  hipStream_t st = (hipStream_t)stream;
  const int lg = lanes_lg(K);
  const int64_t rows = flags == FIL_ADAM_ROLL_FLUSH ? V : (V + sweep_period - 1) / sweep_period;
  const int vec = sweep_vec(K, table, m, v);
  ProfScope ps(flags == FIL_ADAM_ROLL_FLUSH ? "embed_adam_flush" : "embed_adam_roll", st, 24.0 * (double)rows * K + 4.0 * (double)rows);
  const int64_t total = rows << lg;
  const dim3 grid = stride_grid(total);
  hipLaunchKernelGGL(embed_adam_roll_kernel, grid, dim3(256), 0, st, table, m, v, stamp, reinterpret_cast<AdamCoef*>(ring),
                     ring_len(sweep_period), sweep_period, V, K, lg, vec, offsets, field_l2, frozen, F, step, lr, beta_1, beta_2, epsilon,
                     flags == FIL_ADAM_ROLL_STEP ? 0 : (flags == FIL_ADAM_ROLL_SKIP ? kRollSkip : kRollFlush), lr_dev);
  FIL_CHECK_LAUNCH_W(who);
  return FIL_OK;
}

extern "C" int fil_embed_adam_roll(float* table, float* m, float* v, int32_t* stamp, float* ring, int sweep_period, int64_t V, int K,
                                   const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F, const int64_t* step,
                                   float lr, float beta_1, float beta_2, float epsilon, int flags, void* stream) {
  return embed_adam_roll_impl("fil_embed_adam_roll", table, m, v, stamp, ring, sweep_period, V, K, offsets, field_l2, frozen, F, step, lr,
                              beta_1, beta_2, epsilon, flags, stream, nullptr);
}

extern "C" int fil_embed_adam_roll_lrdev(float* table, float* m, float* v, int32_t* stamp, float* ring, int sweep_period, int64_t V, int K,
                                   const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F, const int64_t* step,
                                   const float* lr_dev, float beta_1, float beta_2, float epsilon, int flags, void* stream) {
  if (lr_dev == nullptr) return fail(FIL_ERR_ARG, "fil_embed_adam_roll_lrdev: no device rate (lr_dev is NULL)");
  return embed_adam_roll_impl("fil_embed_adam_roll_lrdev", table, m, v, stamp, ring, sweep_period, V, K, offsets, field_l2, frozen, F, step,
                              0.f, beta_1, beta_2, epsilon, flags, stream, lr_dev);
}
