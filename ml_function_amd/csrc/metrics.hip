// M1 (include/fil.h): Keras' streaming AUC -- the confusion-matrix update and AUC.result().
//
// Counting.  A score's bucket is b(p) = #{i : thr[i] < p} in [0, T], found against the STORED fp32 thresholds (a copy in LDS): a
// guess from p * (T - 1) is accepted only when thr[b - 1] < p and !(thr[b] < p) hold, anything else (user thresholds, a guess off by
// one next to a threshold) takes a binary search over the same copy.  Every wave adds into its own pair of (T + 1)-bin histograms
// (positives | negatives) in LDS with integer atomics: CTR scores are skewed, and one shared histogram would serialise every wave of
// the workgroup on the same few addresses.  A suffix sum turns buckets into the four vectors (TP[i] = #{y != 0, b > i}), and each
// state entry takes one fp32 add.  Everything before that add is integer arithmetic, so the batch's counts are independent of
// scheduling and a repeated call gives the same bits.
//
// Launches.  n <= FIL_CONFUSION_ONE_LAUNCH_N: one workgroup does all of it (confusion_one_kernel).  Larger n: up to kMaxParts
// workgroups each store their histogram as an integer slab in the workspace (confusion_part_kernel, plain stores, no initialisation
// needed), and one workgroup sums the slabs, scans and adds (confusion_finish_kernel).
#include <algorithm>

#include "common.h"

namespace fil {

constexpr int kConfThreads = 1024;            // 16 waves
constexpr int kMaxParts = 256;                // one workgroup per CU
constexpr int kPartElems = 8192;              // at least this many samples per workgroup of the partial launch
constexpr int kHistBudget = 32768;            // bytes of LDS for the per-wave histograms

static inline int conf_bins(int T) { return 2 * (T + 1); }
// private histograms per workgroup: one per wave while they fit the budget (T = 200: 16; T = 1000: 4; T = 2048: 1)
static inline int conf_copies(int T) { return std::max(1, std::min(kConfThreads / kWave, kHistBudget / (conf_bins(T) * 4))); }
// LDS: thr [T] | hist [copies][2][T + 1] | scan buffer [2][T + 1]
static inline size_t conf_lds_bytes(int T) { return 4 * ((size_t)T + (size_t)(conf_copies(T) + 1) * conf_bins(T)); }
static inline int conf_parts(int n) { return std::min(kMaxParts, cdiv(n, kPartElems)); }

// b = #{i : thr[i] < p} for 0 <= p <= 1; thr ascending in LDS
__device__ __forceinline__ int bucket_of(float p, const float* thr, int T) {
  int b = (int)ceilf(p * (float)(T - 1));
  b = min(max(b, 0), T);
  const bool lo_ok = b == 0 || thr[b - 1] < p;
  const bool hi_ok = b == T || !(thr[b] < p);
  if (!(lo_ok && hi_ok)) {
    int lo = 0, hi = T;                       // first index whose threshold is not below p
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (thr[mid] < p) lo = mid + 1;
      else hi = mid;
    }
    b = lo;
  }
  return b;
}

// one sample into the wave's histograms; returns 1 for a sample Keras would refuse
__device__ __forceinline__ int count_one(float p, float y, const float* thr, int T, unsigned* hist) {
  if (!(p >= 0.f && p <= 1.f)) return 1;      // also NaN
  atomicAdd(&hist[(y != 0.f ? 0 : T + 1) + bucket_of(p, thr, T)], 1u);
  return 0;
}

// The workgroup's share of p, y [n] into its waves' histograms; the sum of the copies is left in copy 0.
// s_thr [T], hist [copies][2][T + 1]; returns this thread's invalid count.
__device__ __forceinline__ int histogram_block(const float* __restrict__ p, const float* __restrict__ y, int n, const float* __restrict__ thr,
                                               int T, int copies, float* s_thr, unsigned* hist, int block, int blocks) {
  const int tid = threadIdx.x, nt = blockDim.x, bins = 2 * (T + 1);
  for (int i = tid; i < T; i += nt) s_thr[i] = thr[i];
  for (int i = tid; i < copies * bins; i += nt) hist[i] = 0u;
  __syncthreads();
  unsigned* mine = hist + ((tid / kWave) % copies) * bins;
  int bad = 0;
  // scalar head up to p's first 16-byte boundary, 16-byte body, scalar tail; y rides along with 16-byte loads when it shares p's
  // alignment and with dword loads otherwise (p[1:], y[3:] of a torch tensor are legal inputs)
  const int head = min(n, (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2));
  const int nvec = (n - head) >> 2;
  const int tail0 = head + 4 * nvec;
  if (block == 0) {
    if (tid < head) bad += count_one(p[tid], y[tid], s_thr, T, mine);
    if (tid < n - tail0) bad += count_one(p[tail0 + tid], y[tail0 + tid], s_thr, T, mine);
  }
  const f32x4* p4 = reinterpret_cast<const f32x4*>(p + head);
  const float* yb = y + head;
  const bool y_vec = ((uintptr_t)yb & 15u) == 0;
  auto load_y = [&](int v) {
    if (y_vec) return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(yb) + v);
    return f32x4{yb[4 * v], yb[4 * v + 1], yb[4 * v + 2], yb[4 * v + 3]};
  };
  auto count4 = [&](const f32x4& pv, const f32x4& yv) {
    bad += count_one(pv.x, yv.x, s_thr, T, mine);
    bad += count_one(pv.y, yv.y, s_thr, T, mine);
    bad += count_one(pv.z, yv.z, s_thr, T, mine);
    bad += count_one(pv.w, yv.w, s_thr, T, mine);
  };
  // two vectors of each array in flight per lane before the first LDS atomic
  const int stride = blocks * nt;
  for (int v = block * nt + tid; v < nvec; v += 2 * stride) {
    const int v1 = v + stride;
    const bool two = v1 < nvec;
    const f32x4 pa = __builtin_nontemporal_load(p4 + v);
    const f32x4 ya = load_y(v);
    f32x4 pb = pa, yc = ya;
    if (two) {
      pb = __builtin_nontemporal_load(p4 + v1);
      yc = load_y(v1);
    }
    count4(pa, ya);
    if (two) count4(pb, yc);
  }
  __syncthreads();
  if (copies > 1) {
    for (int i = tid; i < bins; i += nt) {
      unsigned s = 0u;
      for (int c = 0; c < copies; ++c) s += hist[c * bins + i];
      hist[i] = s;                            // bin i of copy 0 is read and written by this thread only
    }
    __syncthreads();
  }
  return bad;
}

// Sum of `bad` over the workgroup (every thread calls), returned in thread 0; s_cnt: one LDS word.
__device__ __forceinline__ unsigned block_count(int bad, unsigned* s_cnt) {
  if (threadIdx.x == 0) *s_cnt = 0u;
  __syncthreads();
  if (bad) atomicAdd(s_cnt, (unsigned)bad);
  __syncthreads();
  return *s_cnt;
}

// h [2][T + 1] bucket counts (positives | negatives) in LDS, tmp the same size: inclusive suffix sums in place of the buckets, then
// the state's one fp32 add per entry.  Every thread of the workgroup calls; h and tmp are complete on entry.
__device__ __forceinline__ void suffix_and_add(unsigned* h, unsigned* tmp, int T, float* __restrict__ cm) {
  const int tid = threadIdx.x, nt = blockDim.x, L = T + 1, bins = 2 * L;
  unsigned* src = h;
  unsigned* dst = tmp;
  for (int off = 1; off < L; off <<= 1) {
    for (int i = tid; i < bins; i += nt) {
      const int j = i < L ? i : i - L;
      dst[i] = src[i] + (j + off < L ? src[i + off] : 0u);
    }
    __syncthreads();
    unsigned* t = src;
    src = dst;
    dst = t;
  }
  // src[j] = #{b >= j}: TP[i] = #{positive, b > i} = src[i + 1], and src[0] is the class total
  const unsigned n_pos = src[0], n_neg = src[L];
  for (int i = tid; i < T; i += nt) {
    const unsigned tp = src[i + 1], fp = src[L + i + 1];
    cm[i] += (float)tp;
    cm[T + i] += (float)fp;
    cm[2 * T + i] += (float)(n_neg - fp);
    cm[3 * T + i] += (float)(n_pos - tp);
  }
}

__global__ __launch_bounds__(kConfThreads) void confusion_one_kernel(const float* __restrict__ p, const float* __restrict__ y, int n,
                                                                      const float* __restrict__ thr, int T, int copies,
                                                                      float* __restrict__ cm, long long* __restrict__ invalid) {
  extern __shared__ unsigned s_mem[];
  __shared__ unsigned s_cnt;
  float* s_thr = reinterpret_cast<float*>(s_mem);
  unsigned* hist = s_mem + T;
  unsigned* tmp = hist + copies * 2 * (T + 1);
  const int bad = histogram_block(p, y, n, thr, T, copies, s_thr, hist, 0, 1);
  const unsigned total_bad = block_count(bad, &s_cnt);
  if (threadIdx.x == 0 && total_bad) *invalid += (long long)total_bad;
  suffix_and_add(hist, tmp, T, cm);
}

// parts [gridDim.x][2 (T + 1)] bucket counts, part_bad [gridDim.x]
__global__ __launch_bounds__(kConfThreads) void confusion_part_kernel(const float* __restrict__ p, const float* __restrict__ y, int n,
                                                                       const float* __restrict__ thr, int T, int copies,
                                                                       unsigned* __restrict__ parts, unsigned* __restrict__ part_bad) {
  extern __shared__ unsigned s_mem[];
  __shared__ unsigned s_cnt;
  float* s_thr = reinterpret_cast<float*>(s_mem);
  unsigned* hist = s_mem + T;
  const int bins = 2 * (T + 1);
  const int bad = histogram_block(p, y, n, thr, T, copies, s_thr, hist, blockIdx.x, gridDim.x);
  const unsigned total_bad = block_count(bad, &s_cnt);
  if (threadIdx.x == 0) part_bad[blockIdx.x] = total_bad;
  unsigned* out = parts + (size_t)blockIdx.x * bins;
  for (int i = threadIdx.x; i < bins; i += blockDim.x) out[i] = hist[i];
}

__global__ __launch_bounds__(kConfThreads) void confusion_finish_kernel(const unsigned* __restrict__ parts,
                                                                         const unsigned* __restrict__ part_bad, int G, int T,
                                                                         float* __restrict__ cm, long long* __restrict__ invalid) {
  extern __shared__ unsigned s_mem[];         // h [2][T + 1] | tmp [2][T + 1]
  __shared__ unsigned s_cnt;
  const int tid = threadIdx.x, nt = blockDim.x, bins = 2 * (T + 1);
  unsigned* h = s_mem;
  unsigned* tmp = s_mem + bins;
  for (int i = tid; i < bins; i += nt) h[i] = 0u;
  __syncthreads();
  // the slabs as one flat array: every load coalesced and every thread busy whatever T is; integer adds, so order-free
  // (eight loads in flight per lane before the first add: taken one at a time, each pays the whole memory latency)
  const int total = G * bins;
  constexpr int kInFlight = 8;
  for (int i0 = tid; i0 < total; i0 += kInFlight * nt) {
    unsigned v[kInFlight];
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      const int i = i0 + u * nt;
      v[u] = i < total ? parts[i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < kInFlight; ++u)
      if (v[u]) atomicAdd(&h[(i0 + u * nt) % bins], v[u]);
  }
  const unsigned total_bad = block_count(tid < G ? (int)part_bad[tid] : 0, &s_cnt);   // G <= kMaxParts <= blockDim.x; syncs
  if (tid == 0 && total_bad) *invalid += (long long)total_bad;
  suffix_and_add(h, tmp, T, cm);
}

// tf.math.div_no_nan
__device__ __forceinline__ float dnn(float a, float b) { return b == 0.f ? 0.f : a / b; }

// AUC.result() in fp32, term by term as Keras states it (no contraction into fma: the PR interpolation cancels)
__global__ __launch_bounds__(256) void auc_result_kernel(const float* __restrict__ cm, int T, int curve, int summation,
                                                          float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ float s_part[256 / kWave];
  const float* TP = cm;
  const float* FP = cm + T;
  const float* TN = cm + 2 * T;
  const float* FN = cm + 3 * T;
  float acc = 0.f;
  for (int i = threadIdx.x; i < T - 1; i += blockDim.x) {
    const float tp0 = TP[i], tp1 = TP[i + 1], fp0 = FP[i], fp1 = FP[i + 1], fn0 = FN[i], fn1 = FN[i + 1];
    float term;
    if (curve == 1 && summation == 0) {       // AUC.interpolate_pr_auc
      const float dtp = tp0 - tp1, p0 = tp0 + fp0, p1 = tp1 + fp1, dp = p0 - p1;
      const float slope = dnn(dtp, fmaxf(dp, 0.f));
      const float inter = tp1 - slope * p1;
      const float ratio = (p0 > 0.f && p1 > 0.f) ? dnn(p0, fmaxf(p1, 0.f)) : 1.f;
      term = dnn(slope * (dtp + inter * logf(ratio)), fmaxf(tp1 + fn1, 0.f));
    } else {
      const float rec0 = dnn(tp0, tp0 + fn0), rec1 = dnn(tp1, tp1 + fn1);
      float x0, x1, y0, y1;
      if (curve == 0) {
        x0 = dnn(fp0, fp0 + TN[i]);
        x1 = dnn(fp1, fp1 + TN[i + 1]);
        y0 = rec0;
        y1 = rec1;
      } else {
        x0 = rec0;
        x1 = rec1;
        y0 = dnn(tp0, tp0 + fp0);
        y1 = dnn(tp1, tp1 + fp1);
      }
      const float h = summation == 0 ? (y0 + y1) / 2.f : summation == 1 ? fminf(y0, y1) : fmaxf(y0, y1);
      term = (x0 - x1) * h;
    }
    acc += term;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & (kWave - 1)) == 0) s_part[threadIdx.x / kWave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < 256 / kWave; ++w) s += s_part[w];
    out[0] = s;
  }
}

static int check_T(const char* who, int T) {
  if (T < 2 || T > FIL_CONFUSION_MAX_T)
    return fail(FIL_ERR_UNSUPPORTED, "%s: T=%d thresholds (2 <= T <= FIL_CONFUSION_MAX_T = %d)", who, T, FIL_CONFUSION_MAX_T);
  return FIL_OK;
}

}  // namespace fil

using namespace fil;

extern "C" size_t fil_confusion_workspace_bytes(int n, int T) {
  if (n <= FIL_CONFUSION_ONE_LAUNCH_N || T < 2 || T > FIL_CONFUSION_MAX_T) return 0;
  const int G = conf_parts(n);
  return align_up((size_t)G * conf_bins(T) * sizeof(unsigned), 256) + align_up((size_t)G * sizeof(unsigned), 256);
}

extern "C" int fil_confusion_update(const float* p, const float* y, int n, const float* thr, int T, float* cm, long long* invalid,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  FIL_CHECK_ARG(n >= 1);
  if (n > (1 << 24)) return fail(FIL_ERR_ARG, "fil_confusion_update: n=%d > 2^24 samples in one call (feed larger inputs in slices)", n);
  if (int rc = check_T("fil_confusion_update", T)) return rc;
  FIL_CHECK_ARG(p && y && thr && cm && invalid);
  FIL_CHECK_ARG((((uintptr_t)p | (uintptr_t)y) & 3u) == 0);
  const size_t need = fil_confusion_workspace_bytes(n, T);
  if (need > 0 && (workspace == nullptr || workspace_bytes < need))
    return fail(FIL_ERR_WORKSPACE, "fil_confusion_update: workspace %zu < %zu bytes", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("confusion_update", st, 8.0 * n);
  const int copies = conf_copies(T);
  const size_t lds = conf_lds_bytes(T);
  if (n <= FIL_CONFUSION_ONE_LAUNCH_N) {
    hipLaunchKernelGGL(confusion_one_kernel, dim3(1), dim3(kConfThreads), lds, st, p, y, n, thr, T, copies, cm, invalid);
    FIL_CHECK_LAUNCH();
    return FIL_OK;
  }
  const int G = conf_parts(n);
  Carver cv(workspace);
  unsigned* parts = cv.take<unsigned>((size_t)G * conf_bins(T));
  unsigned* part_bad = cv.take<unsigned>(G);
  hipLaunchKernelGGL(confusion_part_kernel, dim3(G), dim3(kConfThreads), lds, st, p, y, n, thr, T, copies, parts, part_bad);
  FIL_CHECK_LAUNCH();
  hipLaunchKernelGGL(confusion_finish_kernel, dim3(1), dim3(kConfThreads), 2 * conf_bins(T) * sizeof(unsigned), st, parts, part_bad, G, T,
                     cm, invalid);
  FIL_CHECK_LAUNCH();
  return FIL_OK;
}

extern "C" int fil_auc_result(const float* cm, int T, int curve, int summation, float* out, void* stream) {
  if (int rc = check_T("fil_auc_result", T)) return rc;
  FIL_CHECK_ARG(cm && out);
  if (curve != 0 && curve != 1) return fail(FIL_ERR_ARG, "fil_auc_result: curve %d (0 ROC, 1 PR)", curve);
  if (summation < 0 || summation > 2)
    return fail(FIL_ERR_ARG, "fil_auc_result: summation %d (0 interpolation, 1 minoring, 2 majoring)", summation);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("auc_result", st, 16.0 * T);
  hipLaunchKernelGGL(auc_result_kernel, dim3(1), dim3(256), 0, st, cm, T, curve, summation, out);
  FIL_CHECK_LAUNCH();
  return FIL_OK;
}
