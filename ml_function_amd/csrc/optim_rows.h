// What the fused optimizers of optim.hip (Adam), optim_amsgrad.hip (Adam with amsgrad), optim_rowwise.hip (Adagrad, Ftrl) and
// optim_momentum.hip (SGD, RMSprop) share: the one walk of the dense descriptors, two-slot or with amsgrad's third slot (fil_adam_multi,
// fil_amsgrad_multi, fil_rowopt_multi, fil_momopt_multi), the field of a row, the walk of the gathered
// compact lists of fil_embed_runs_compact (runs_compact.hip; the merged updates), the regulariser's gradient, the sweeps' compacted
// field table, the workgroup sum and scan, and what every launcher computes the same way: the row tag of a step, the sweep's 16-byte
// predicate, the grid-stride grid and the table-shape check.
// Adam and its amsgrad form build their kernels on them in optim_adam.h and optim.hip (their coefficients depend on the step; lazy
// and deferred modes); the row-rule families get
// theirs, and their host launchers, from optim_rule.h, which sits on this header: there a rule supplies only its per-element update.
#pragma once
#include "common.h"

namespace fil {

constexpr int kSweepMaxF = 1024;

// the tag of the rows updated at the step in progress: the low 32 bits of its 1-based count
__device__ __forceinline__ int32_t step_tag(const int64_t* __restrict__ step) { return (int32_t)(uint32_t)(*step + 1); }

// does a sweep of these arrays take its 16-byte path (K % 4 == 0 and every array the rule has 16-byte aligned; NULL: not one of
// them).  Adam's 16-byte path rounds differently (adam_untouched, optim.hip), so its deferred kernels ask here too.
inline int sweep_vec(int K, const float* a, const float* b, const float* c) {
  return (K % 4 == 0 && ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0)) ? 1 : 0;
}

// the grid of a grid-stride kernel over `work` lanes' worth of items, 256 lanes a workgroup
inline dim3 stride_grid(int64_t work) { return dim3((int)std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, 256 * 8))); }

// a lane group of a wave holds a row (K <= 256) and the field table sits in LDS (F <= kSweepMaxF); K = 0 / F = 0: the caller's
// kernels have no such limit
inline int check_table_shape(const char* who, int K, int F) {
  if (K > 256) return fail(FIL_ERR_UNSUPPORTED, "%s: K=%d > 256", who, K);
  if (F > kSweepMaxF) return fail(FIL_ERR_UNSUPPORTED, "%s: F=%d > %d fields", who, F, kSweepMaxF);
  return FIL_OK;
}

// the last f with off[f] <= row, or -1
__device__ __forceinline__ int sweep_field(const int64_t* off, int F, int64_t row) {
  int lo = 0, hi = F;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= row) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

// the position of `row` in an ascending list of n distinct ids, or -1
__device__ __forceinline__ long find_row(const int64_t* __restrict__ list, long n, int64_t row) {
  long lo = 0, hi = n;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (list[mid] < row) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && list[lo] == row ? lo : -1;
}

// the number of valid entries of gathered list w (its count clipped to [0, cap])
__device__ __forceinline__ long list_count(const int64_t* counts, int w, long cap) {
  const int64_t c = counts[w];
  return c < 0 ? 0 : (c > cap ? cap : (long)c);
}

// the position of `row` in gathered list w2 (the lists of fil_embed_runs_compact, cap entries each, side by side in ids), or -1
__device__ __forceinline__ long find_in_list(const int64_t* __restrict__ ids, const int64_t* counts, int w2, long cap, int64_t row) {
  return find_row(ids + (long)w2 * cap, list_count(counts, w2, cap), row);
}

// ---- the dense launch: the descriptors' elements form one index space of kMultiChunk-element chunks (a workgroup's 256 lanes x 4),
// dealt round robin over the grid; a workgroup walks the descriptor list once and takes its chunks of each (grid-stride, balanced
// over tensors of any size).  16-byte accesses where the descriptor's arrays allow it (a slot only counts when the rule has it: kM,
// kV, kH -- a slot the rule does not have is neither read nor written and may be NULL), element-wise otherwise and in the tail.
// The one walk, multi_tensor_walk_desc, is over any descriptor type T with fil_adam_tensor's members; kH: T also has a third slot
// `vhat` (fil_amsgrad_tensor).  elem(p, m, v, h, g, l2x2) updates one element: g the gradient (0 without one), l2x2 = 2 l2 of the
// descriptor.
constexpr int kMultiChunk = 1024;

template <typename T, bool kM, bool kV, bool kH, typename Elem>
__device__ __forceinline__ void multi_tensor_walk_desc(const T* __restrict__ ts, int n, const Elem& elem) {
  const long G = gridDim.x;
  long base = 0;
  for (int d = 0; d < n; ++d) {
    float* __restrict__ P = ts[d].param;
    const float* __restrict__ Gr = ts[d].grad;
    float* __restrict__ M = ts[d].m;
    float* __restrict__ V = ts[d].v;
    float* __restrict__ H = nullptr;
    if constexpr (kH) H = ts[d].vhat;
    const long numel = ts[d].numel;
    const float l2x2 = 2.f * ts[d].l2;
    const long nc = (numel + kMultiChunk - 1) / kMultiChunk;
    const uintptr_t slots = (kM ? (uintptr_t)M : 0) | (kV ? (uintptr_t)V : 0) | (kH ? (uintptr_t)H : 0);
    const bool vec = ((((uintptr_t)P | (uintptr_t)Gr | slots) & 15) == 0);
    long r = ((long)blockIdx.x - base) % G;
    if (r < 0) r += G;
    for (long ch = r; ch < nc; ch += G) {
      const long e = ch * kMultiChunk + threadIdx.x * 4;
      if (vec && e + 4 <= numel) {
        float4 p = *reinterpret_cast<const float4*>(P + e);
        float4 g = Gr ? *reinterpret_cast<const float4*>(Gr + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 m = kM ? *reinterpret_cast<const float4*>(M + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 v = kV ? *reinterpret_cast<const float4*>(V + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 h = kH ? *reinterpret_cast<const float4*>(H + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        elem(p.x, m.x, v.x, h.x, g.x, l2x2);
        elem(p.y, m.y, v.y, h.y, g.y, l2x2);
        elem(p.z, m.z, v.z, h.z, g.z, l2x2);
        elem(p.w, m.w, v.w, h.w, g.w, l2x2);
        *reinterpret_cast<float4*>(P + e) = p;
        if (kM) *reinterpret_cast<float4*>(M + e) = m;
        if (kV) *reinterpret_cast<float4*>(V + e) = v;
        if (kH) *reinterpret_cast<float4*>(H + e) = h;
      } else {
        for (long i = e; i < e + 4 && i < numel; ++i) {
          float p = P[i], m = kM ? M[i] : 0.f, v = kV ? V[i] : 0.f, h = kH ? H[i] : 0.f;
          elem(p, m, v, h, Gr ? Gr[i] : 0.f, l2x2);
          P[i] = p;
          if (kM) M[i] = m;
          if (kV) V[i] = v;
          if (kH) H[i] = h;
        }
      }
    }
    base += nc;
  }
}

// the walk of the two-slot descriptor: elem(p, m, v, g, l2x2)
template <bool kM, bool kV, typename Elem>
__device__ __forceinline__ void multi_tensor_walk_slots(const fil_adam_tensor* __restrict__ ts, int n, const Elem& elem) {
  multi_tensor_walk_desc<fil_adam_tensor, kM, kV, false>(
      ts, n, [&](float& p, float& m, float& v, float&, float g, float l2x2) { elem(p, m, v, g, l2x2); });
}

// the walk of a rule that always has its first slot (Adam, Adagrad, Ftrl)
template <bool kV, typename Elem>
__device__ __forceinline__ void multi_tensor_walk(const fil_adam_tensor* __restrict__ ts, int n, const Elem& elem) {
  multi_tensor_walk_slots<true, kV>(ts, n, elem);
}

// launches the one-thread kernel that advances a device step counter behind the dense update (defined once, in optim.hip)
void launch_step_advance(int64_t* step, hipStream_t st);

// ---- the merged update of W gathered lists: one lane per gathered entry q = (w, i), q0 + k stride (the kernel's grid stride: read
// there, where blockDim folds to the launch bounds).  The lowest list holding a row owns it; rows outside [0, V) are skipped.  The
// owner adds the other lists' copies in list order (binary searches: each list is ascending and distinct), K in chunks of
// kMergeChunk elements (a later chunk repeats the searches), and hands each chunk to epi(row, f, l2x2, k0, acc): f the row's field
// (sweep_field of the offsets s_off, -1 before the first), l2x2 = 2 field_l2[f] (0 without), acc[e] element k0 + e of the summed
// row (0 past K).  fin(row) follows the row's last chunk.
constexpr int kMergeChunk = 16;

template <typename Epi, typename Fin>
__device__ __forceinline__ void merged_row_sums(long q0, long stride, const int64_t* __restrict__ ids, const float* __restrict__ values,
                                                const int64_t* __restrict__ counts, int W, long cap, int K, int64_t V,
                                                const int64_t* s_off, const float* __restrict__ field_l2, int F, const Epi& epi,
                                                const Fin& fin) {
  const long n = (long)W * cap;
  for (long q = q0; q < n; q += stride) {
    const int w = (int)(q / cap);
    const long i = q - (long)w * cap;
    if (i >= list_count(counts, w, cap)) continue;
    const int64_t row = ids[q];
    if (row < 0 || row >= V) continue;
    bool owner = true;
    for (int w2 = 0; w2 < w && owner; ++w2) owner = find_in_list(ids, counts, w2, cap, row) < 0;
    if (!owner) continue;
    const int f = sweep_field(s_off, F, row);
    const float l2x2 = (field_l2 && f >= 0) ? 2.f * field_l2[f] : 0.f;
    for (int k0 = 0; k0 < K; k0 += kMergeChunk) {
      float acc[kMergeChunk];
      const float* src = values + q * K + k0;
#pragma unroll
      for (int e = 0; e < kMergeChunk; ++e) acc[e] = k0 + e < K ? src[e] : 0.f;
      for (int w2 = w + 1; w2 < W; ++w2) {
        const long at = find_in_list(ids, counts, w2, cap, row);
        if (at < 0) continue;
        const float* o = values + ((long)w2 * cap + at) * K + k0;
#pragma unroll
        for (int e = 0; e < kMergeChunk; ++e)
          if (k0 + e < K) acc[e] += o[e];
      }
      epi(row, f, l2x2, k0, acc);
    }
    fin(row);
  }
}

// g = run sum + 2 l2 p of a field's regulariser (rounded as written)
__device__ __forceinline__ float with_l2(float acc, float l2x2, float p) {
#pragma clang fp contract(off)
  return acc + l2x2 * p;
}

// ---- the sweep's field table.  Only some fields' untouched rows move (the regularised, non-frozen ones; for a rule whose slot decays
// everywhere, every non-frozen one), so a sweep's grid walks those fields' rows only: every workgroup compacts the field table in LDS
// into "virtual" row ranges (an integer scan over F <= 1024 fields, a few hundred cycles) and strides over the virtual rows; a virtual
// row maps back to its table row by a binary search.
struct RegTab {
  int64_t vbeg[kSweepMaxF + 1];   // virtual row where compacted field c starts; vbeg[n] = all regularised rows
  int64_t rbeg[kSweepMaxF];       // its first table row
  float l2x2[kSweepMaxF];         // 2 field_l2
  int n;
};

// sum of x over a 256-lane workgroup (s: 4 longs of LDS); every lane gets the total
__device__ __forceinline__ long block_sum_256(long x, long* s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = x;
  __syncthreads();
  const long t = (s[0] + s[1]) + (s[2] + s[3]);
  __syncthreads();
  return t;
}

// exclusive scan of x over a 256-lane workgroup in lane order (s: 4 longs of LDS); *total = the sum over all lanes
__device__ __forceinline__ long block_scan_256(long x, long* s, long* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long incl = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  if (lane == 63) s[wave] = incl;
  __syncthreads();
  long before = incl - x;
  for (int w = 0; w < wave; ++w) before += s[w];
  *total = (s[0] + s[1]) + (s[2] + s[3]);
  __syncthreads();
  return before;
}

// kAll: every non-frozen field joins the table (2 field_l2 = 0 for an unregularised one, field_l2 may then be NULL), not only the
// regularised ones
template <bool kAll = false>
__device__ __forceinline__ void load_reg_tab(RegTab* t, const int64_t* __restrict__ offsets, const float* __restrict__ field_l2,
                                             const unsigned char* __restrict__ frozen, int F, int64_t V) {
  __shared__ long s[4];
  int64_t lo[4], rows[4];
  long cnt = 0, sum = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int f = threadIdx.x * 4 + i;
    lo[i] = 0;
    rows[i] = 0;
    if (f < F && !(frozen && frozen[f]) && (kAll || field_l2[f] > 0.f)) {
      int64_t a = offsets[f], b = f + 1 < F ? offsets[f + 1] : V;
      a = a < 0 ? 0 : (a > V ? V : a);
      b = b < a ? a : (b > V ? V : b);
      if (b > a) {
        lo[i] = a;
        rows[i] = b - a;
        ++cnt;
        sum += b - a;
      }
    }
  }
  long nf, total;
  long c = block_scan_256(cnt, s, &nf);
  long v = block_scan_256(sum, s, &total);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (rows[i] > 0) {
      t->vbeg[c] = v;
      t->rbeg[c] = lo[i];
      const float l2 = field_l2 ? field_l2[threadIdx.x * 4 + i] : 0.f;
      t->l2x2[c] = kAll && !(l2 > 0.f) ? 0.f : 2.f * l2;
      ++c;
      v += rows[i];
    }
  }
  if (threadIdx.x == 0) {
    t->n = (int)nf;
    t->vbeg[nf] = total;
  }
  __syncthreads();
}

// compacted field c holding virtual row vr (vbeg[c] <= vr < vbeg[c + 1])
__device__ __forceinline__ int reg_field(const RegTab* t, int64_t vr) {
  int lo = 0, hi = t->n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t->vbeg[mid] <= vr) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

}  // namespace fil
