// M2 (include/fil.h): Keras' Mean / MeanMetricWrapper state -- total, count and their quotient -- updated by one call.
//
// Summation.  Nothing here depends on scheduling: thread t of workgroup g takes the 16-byte vectors g * 1024 + t, + stride, ... of the
// body in that order (each vector folded as (x + y) + (z + w)), the wave folds its 64 sums by a fixed butterfly, thread 0 adds the 16
// waves' sums in wave order, and the workgroups' partials are stored to the workspace (plain stores, no initialisation needed) and
// folded the same way by the finishing launch: partial g goes to thread g of one 256-thread workgroup.  No atomics.  The state then
// takes ONE fp32 addition for total and one for count (Keras' assign_add), and result = div_no_nan(total, count) is written by the
// same launch.  Accuracy counts matches in integers (at most 2^24 per call) and converts the batch's count once.
//
// Launches.  n <= FIL_MEAN_ONE_LAUNCH_N: one workgroup does all of it (mean_one_kernel).  Larger n: up to kMeanMaxParts workgroups
// store one 4-byte partial each (mean_part_kernel), and one workgroup folds them and updates the state (mean_finish_kernel).
#include <algorithm>

#include "common.h"

namespace fil {

constexpr int kMeanThreads = 1024;            // 16 waves
constexpr int kMeanWaves = kMeanThreads / kWave;
constexpr int kMeanMaxParts = 256;            // one workgroup per CU
constexpr int kMeanPartElems = 8192;          // at least this many samples per workgroup of the partial launch

static inline int mean_parts(int n) { return std::min(kMeanMaxParts, cdiv(n, kMeanPartElems)); }

// The accumulator of a kind: matches are counted in integers, everything else is summed in fp32.
template <int KIND>
struct MeanAcc {
  typedef float type;
};
template <>
struct MeanAcc<FIL_MEAN_BINARY_ACC> {
  typedef unsigned type;
};

// v[i] of one sample.  No contraction into fma: the value is Keras' expression, operation by operation.
template <int KIND>
__device__ __forceinline__ typename MeanAcc<KIND>::type mean_value(float a, float y, float c0, float c1) {
#pragma clang fp contract(off)
  if constexpr (KIND == FIL_MEAN_VALUES) {
    return a;
  } else if constexpr (KIND == FIL_MEAN_BCE) {
    // TF 2.1 keras/losses.py binary_crossentropy (label smoothing) and keras/backend.py binary_crossentropy (the clip and the logs).
    // fmaxf / fminf return their other operand for a NaN: a NaN prediction must stay one, as clip_by_value leaves it.
    const float ys = c1 != 0.f ? y * (1.0f - c1) + 0.5f * c1 : y;
    const float pc = a != a ? a : fminf(fmaxf(a, c0), 1.0f - c0);
    const float u = pc + c0, w = 1.0f - pc + c0;
    const float s = ys * logf(u) + (1.0f - ys) * logf(w);
    return -s;
  } else {
    return y == (a > c0 ? 1.f : 0.f) ? 1u : 0u;
  }
}

template <typename T>
__device__ __forceinline__ T mean_wave_fold(T v) {
  v += __shfl_xor(v, 32);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 1);
  return v;
}

// Sum of `v` over the workgroup, valid in thread 0: a butterfly inside each wave, then the waves' sums in wave order.
// s_part: one word per wave.  Every thread calls.
template <typename T>
__device__ __forceinline__ T mean_block_fold(T v, T* s_part) {
  v = mean_wave_fold(v);
  if ((threadIdx.x & (kWave - 1)) == 0) s_part[threadIdx.x / kWave] = v;
  __syncthreads();
  T s = T(0);
  if (threadIdx.x == 0) {
    const int waves = blockDim.x / kWave;
    s = s_part[0];
    for (int w = 1; w < waves; ++w) s += s_part[w];
  }
  return s;
}

// This thread's share of a, y [n]: a scalar head up to a's first 16-byte boundary and a scalar tail (workgroup 0), a 16-byte body;
// y rides along with 16-byte loads when it shares a's alignment and with dword loads otherwise (a[1:], y[3:] of a torch tensor are
// legal inputs).
template <int KIND>
__device__ __forceinline__ typename MeanAcc<KIND>::type mean_thread_sum(const float* __restrict__ a, const float* __restrict__ y, int n,
                                                                         float c0, float c1, int block, int blocks) {
#pragma clang fp contract(off)
  typedef typename MeanAcc<KIND>::type acc_t;
  constexpr bool kUseY = KIND != FIL_MEAN_VALUES;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int head = min(n, (int)(((16u - (unsigned)((uintptr_t)a & 15u)) & 15u) >> 2));
  const int nvec = (n - head) >> 2;
  const int tail0 = head + 4 * nvec;
  acc_t acc = acc_t(0);
  if (block == 0) {
    if (tid < head) acc += mean_value<KIND>(a[tid], kUseY ? y[tid] : 0.f, c0, c1);
    if (tid < n - tail0) acc += mean_value<KIND>(a[tail0 + tid], kUseY ? y[tail0 + tid] : 0.f, c0, c1);
  }
  const f32x4* a4 = reinterpret_cast<const f32x4*>(a + head);
  const float* yb = kUseY ? y + head : nullptr;
  const bool y_vec = kUseY && ((uintptr_t)yb & 15u) == 0;
  auto load_y = [&](int v) {
    if (!kUseY) return f32x4{0.f, 0.f, 0.f, 0.f};
    if (y_vec) return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(yb) + v);
    return f32x4{yb[4 * v], yb[4 * v + 1], yb[4 * v + 2], yb[4 * v + 3]};
  };
  auto sum4 = [&](const f32x4& av, const f32x4& yv) {
    const acc_t s01 = mean_value<KIND>(av.x, yv.x, c0, c1) + mean_value<KIND>(av.y, yv.y, c0, c1);
    const acc_t s23 = mean_value<KIND>(av.z, yv.z, c0, c1) + mean_value<KIND>(av.w, yv.w, c0, c1);
    acc += s01 + s23;
  };
  // two vectors of each array in flight per lane
  const int stride = blocks * nt;
  for (int v = block * nt + tid; v < nvec; v += 2 * stride) {
    const int v1 = v + stride;
    const bool two = v1 < nvec;
    const f32x4 aa = __builtin_nontemporal_load(a4 + v);
    const f32x4 ya = load_y(v);
    f32x4 ab = aa, yc = ya;
    if (two) {
      ab = __builtin_nontemporal_load(a4 + v1);
      yc = load_y(v1);
    }
    sum4(aa, ya);
    if (two) sum4(ab, yc);
  }
  return acc;
}

// tf.math.div_no_nan
__device__ __forceinline__ float mean_dnn(float a, float b) { return b == 0.f ? 0.f : a / b; }

// state = total | count | result: one fp32 add each for total and count, then the quotient.  One thread calls, with the total and
// count it read when the kernel started (their load latency then lies under the summation, not behind it).
__device__ __forceinline__ void mean_state_add(float* __restrict__ state, float total0, float count0, float sum, int n) {
  const float total = total0 + sum;
  const float count = count0 + (float)n;
  state[0] = total;
  state[1] = count;
  state[2] = mean_dnn(total, count);
}

template <int KIND>
__global__ __launch_bounds__(kMeanThreads) void mean_one_kernel(const float* __restrict__ a, const float* __restrict__ y, int n, float c0,
                                                                 float c1, float* __restrict__ state) {
  typedef typename MeanAcc<KIND>::type acc_t;
  __shared__ acc_t s_part[kMeanWaves];
  float total0 = 0.f, count0 = 0.f;
  if (threadIdx.x == 0) {
    total0 = state[0];
    count0 = state[1];
  }
  const acc_t s = mean_block_fold(mean_thread_sum<KIND>(a, y, n, c0, c1, 0, 1), s_part);
  if (threadIdx.x == 0) mean_state_add(state, total0, count0, (float)s, n);
}

// parts [gridDim.x]: one fp32 sum (or, for accuracy, one integer count) per workgroup
template <int KIND>
__global__ __launch_bounds__(kMeanThreads) void mean_part_kernel(const float* __restrict__ a, const float* __restrict__ y, int n, float c0,
                                                                  float c1, typename MeanAcc<KIND>::type* __restrict__ parts) {
  typedef typename MeanAcc<KIND>::type acc_t;
  __shared__ acc_t s_part[kMeanWaves];
  const acc_t s = mean_block_fold(mean_thread_sum<KIND>(a, y, n, c0, c1, blockIdx.x, gridDim.x), s_part);
  if (threadIdx.x == 0) parts[blockIdx.x] = s;
}

// G <= kMeanMaxParts = blockDim.x: partial g is thread g's, the fold is the workgroup's fixed one
template <typename T>
__global__ __launch_bounds__(kMeanMaxParts) void mean_finish_kernel(const T* __restrict__ parts, int G, int n, float* __restrict__ state) {
  __shared__ T s_part[kMeanMaxParts / kWave];
  float total0 = 0.f, count0 = 0.f;
  if (threadIdx.x == 0) {
    total0 = state[0];
    count0 = state[1];
  }
  const T mine = (int)threadIdx.x < G ? parts[threadIdx.x] : T(0);
  const T s = mean_block_fold(mine, s_part);
  if (threadIdx.x == 0) mean_state_add(state, total0, count0, (float)s, n);
}

template <int KIND>
static void mean_launch(const float* a, const float* y, int n, float c0, float c1, float* state, void* workspace, hipStream_t st) {
  typedef typename MeanAcc<KIND>::type acc_t;
  if (n <= FIL_MEAN_ONE_LAUNCH_N) {
    hipLaunchKernelGGL(mean_one_kernel<KIND>, dim3(1), dim3(kMeanThreads), 0, st, a, y, n, c0, c1, state);
    return;
  }
  const int G = mean_parts(n);
  acc_t* parts = static_cast<acc_t*>(workspace);
  hipLaunchKernelGGL(mean_part_kernel<KIND>, dim3(G), dim3(kMeanThreads), 0, st, a, y, n, c0, c1, parts);
  hipLaunchKernelGGL(mean_finish_kernel<acc_t>, dim3(1), dim3(kMeanMaxParts), 0, st, parts, G, n, state);
}

}  // namespace fil

using namespace fil;

extern "C" size_t fil_mean_workspace_bytes(int n) {
  if (n <= FIL_MEAN_ONE_LAUNCH_N || n > (1 << 24)) return 0;
  return align_up((size_t)mean_parts(n) * 4, 256);
}

extern "C" int fil_mean_update(int kind, const float* a, const float* y, int n, float c0, float c1, float* state, void* workspace,
                               size_t workspace_bytes, void* stream) {
  if (kind != FIL_MEAN_VALUES && kind != FIL_MEAN_BCE && kind != FIL_MEAN_BINARY_ACC)
    return fail(FIL_ERR_ARG, "fil_mean_update: kind %d (0 values, 1 binary cross-entropy, 2 binary accuracy)", kind);
  FIL_CHECK_ARG(n >= 1);
  if (n > (1 << 24)) return fail(FIL_ERR_ARG, "fil_mean_update: n=%d > 2^24 samples in one call (feed larger inputs in slices)", n);
  FIL_CHECK_ARG(a && state);
  FIL_CHECK_ARG(y || kind == FIL_MEAN_VALUES);
  FIL_CHECK_ARG((((uintptr_t)a | (uintptr_t)y | (uintptr_t)state) & 3u) == 0);
  const size_t need = fil_mean_workspace_bytes(n);
  if (need > 0 && (workspace == nullptr || workspace_bytes < need))
    return fail(FIL_ERR_WORKSPACE, "fil_mean_update: workspace %zu < %zu bytes", workspace_bytes, need);
  if (need > 0) FIL_CHECK_ARG(((uintptr_t)workspace & 3u) == 0);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("mean_update", st, (kind == FIL_MEAN_VALUES ? 4.0 : 8.0) * n);
  if (kind == FIL_MEAN_VALUES) mean_launch<FIL_MEAN_VALUES>(a, y, n, c0, c1, state, workspace, st);
  else if (kind == FIL_MEAN_BCE) mean_launch<FIL_MEAN_BCE>(a, y, n, c0, c1, state, workspace, st);
  else mean_launch<FIL_MEAN_BINARY_ACC>(a, y, n, c0, c1, state, workspace, st);
  FIL_CHECK_LAUNCH();
  return FIL_OK;
}
