// N3  Masked multi-head self-attention over a behaviour sequence for gfx950, forward and backward, fp32 (extension: the scaled
// dot-product layer of "Attention is all you need" as the Behaviour Sequence Transformer applies it to a user's history; NOT the
// reference's MultHeadAttentionLayer, which fil_attn_* / fil_pattn_* restate).
//
//     q = x Wq, k = x Wk, v = x Wv;  per head h (columns hD .. hD+D-1):  s_ij = q_i . k_j (* 1/sqrt(D))
//     p_ij = softmax of s_ij over the LIVE j;  out_i = sum_j p_ij v_j  for live i, 0 for masked i.
//
// The _v entry points add a structure mask (view) and a pooled output (the three views of the Sequence-Aware Factorization
// Machine).  The keys a row may see are one RANGE of positions -- FULL: [0,T); CAUSAL: [0,i]; CROSS with split S: [S,T) for a row
// i < S and [0,S) for a row i >= S -- so the key loops below keep their form and their ascending order and only get other bounds
// (sa_range; the column pass of the backward walks the transposed range).  A live row whose range holds no live key gives out_i = 0
// and sends no gradient (its 1/sum statistic is stored as 0 and the column pass skips it).  Pooled: the row pass leaves out_i in
// the LDS slot of q_i (which only its owner thread reads), and one more pass adds the live rows of a sample in position order and
// divides by their number; the backward builds its g rows as gpool[b] / n_b while staging them.  Each kernel has two instantiations
// per head width: GEN = false is the first form exactly (FULL view, rows out, g rows in: uniform loop bounds, no pooling code, the
// registers and occupancy it had), GEN = true takes the view and the pointers as run-time arguments (uniform branches).
//
// Structure (both directions).  A workgroup of 256 threads owns a tile of NS samples; everything of the tile sits in LDS (rows
// padded by 4 floats), nothing of size [T,T] exists anywhere: the scores are recomputed where they are needed.  The products run on
// FMAs (DESIGN 6t says why).  The weights are read through the caches, not staged: at K = H D = 64 they would take 48 KB that the
// T = 64 tile needs.
//   forward   1  x rows of the live positions -> LDS (a masked row is never read: zeros).
//             2  q, k, v: a thread owns four columns of one position, k ascending -> LDS (and `saved`).
//             3  a thread owns one (sample, head, row): the row's maximum over the live keys, then exp / sum / sum p v in key
//                order with q_i and the accumulators in registers and k_j, v_j broadcast from LDS.
//   backward  1  x, g, and q, k, v from `saved`, of the live positions -> LDS.
//             2  a thread owns one (sample, head, ROW i): maximum and top key; sum, and abar = sum_l p_il a_l with
//                a_l = g_i . v_l - g_i . v_top (exactly 0 at the top key); dq_i = scale sum_j ds_ij k_j with ds_ij = p_ij (a_j - abar).
//                The row's (max, 1/sum, abar, g_i . v_top, top) -> LDS.
//             3  a thread owns one (sample, head, COLUMN j): dk_j = scale sum_i ds_ij q_i, dv_j = sum_i p_ij g_i in row order,
//                from the rows' statistics; they replace k_j, v_j in LDS (only their owner reads those).
//             4  dx = dq Wq^T + dk Wk^T + dv Wv^T, a thread per (position, feature).
//             5  the tile's x^T [dq | dk | dv], position order, added to the workgroup's partial in `workspace`.
//             One partial per workgroup; param_reduce_kernel adds the partials in a fixed order.
// No atomics; every sum has a fixed order that does not depend on the tile or the batch for out / dx: repeats are bit-identical
// and a sample's out / dx rows do not depend on what else is in the batch.
#include "common.h"
#include "param_reduce.h"
#include "tiled_launch.h"
#include <algorithm>
#include <math.h>

namespace fil {

constexpr int kSaMaxK = 64, kSaMaxH = 8, kSaMaxHD = 64, kSaMaxT = 256;
constexpr int kSaGridCap = 1024;      // workgroups per launch
constexpr int kSaThreads = 256;
constexpr int kSaMaxNS = 256;         // samples per tile, at most
constexpr int kSaStat = 5;            // floats per (sample, head, row) in the backward: max, 1/sum, abar, g.v_top, top

// all LDS offsets in floats (multiples of 4)
struct SaLayout {
  int T, K, H, D, HD, KP, HDP, NS;
  int f_q, f_k, f_v, f_live, lds_fwd;                        // forward:  x [NS][T][KP] | q | k | v [NS][T][HDP] | live [NS][T]
  int b_g, b_q, b_k, b_v, b_dq, b_st, b_live, lds_bwd;       // backward: x | g | q | k (dk) | v (dv) | dq | stats [NS][H][T][5] | live
  int n_out;                                                 // one partial: dWq | dWk | dWv, each [K][HD]
  float scale;
  int view, split;                                           // FIL_SEQ_VIEW_*; set by the _v entry points (0, 0 otherwise)
};

static inline int sa_fwd_floats(int T, int K, int HD) { return T * ((K + 4) + 3 * (HD + 4) + 1); }
static inline int sa_bwd_floats(int T, int K, int H, int HD) { return T * ((K + 4) + 5 * (HD + 4) + kSaStat * H + 1); }
static inline int up4(int v) { return (v + 3) / 4 * 4; }

// samples per tile the LDS limit leaves room for (0: the shape does not fit)
static inline int sa_room(int per_sample_floats) { return (kTiledLdsLimit / 4 - 8) / per_sample_floats; }

static SaLayout sa_layout(int B, int T, int K, int H, int D, int use_scale) {
  SaLayout L;
  L.T = T; L.K = K; L.H = H; L.D = D; L.HD = H * D; L.KP = K + 4; L.HDP = L.HD + 4;
  const int room = std::min(sa_room(sa_fwd_floats(T, K, L.HD)), sa_room(sa_bwd_floats(T, K, H, L.HD)));
  // as many samples as give every thread at most ONE (head, row) pair.  The tile does not grow with B: the tile's LDS image is what
  // limits the workgroups a CU holds, so past the grid cap a workgroup walks several small tiles instead
  (void)B;
  L.NS = std::max(1, std::min(std::min(room, kSaMaxNS), kSaThreads / (H * T)));
  const int NT = L.NS * T;
  L.f_q = NT * L.KP;
  L.f_k = L.f_q + NT * L.HDP;
  L.f_v = L.f_k + NT * L.HDP;
  L.f_live = L.f_v + NT * L.HDP;
  L.lds_fwd = 4 * (L.f_live + up4(NT));
  L.b_g = NT * L.KP;
  L.b_q = L.b_g + NT * L.HDP;
  L.b_k = L.b_q + NT * L.HDP;
  L.b_v = L.b_k + NT * L.HDP;
  L.b_dq = L.b_v + NT * L.HDP;
  L.b_st = L.b_dq + NT * L.HDP;
  L.b_live = L.b_st + up4(NT * H * kSaStat);
  L.lds_bwd = 4 * (L.b_live + up4(NT));
  L.n_out = 3 * K * L.HD;
  L.scale = use_scale ? 1.0f / sqrtf((float)D) : 1.0f;
  L.view = FIL_SEQ_VIEW_FULL; L.split = 0;
  return L;
}

static inline int sa_grid(int B, int NS) { return tiled_grid(B, NS, kSaGridCap); }

// [lo, hi): the keys row `at` may see -- or, transposed, the rows that may see key `at`
__device__ __forceinline__ void sa_range(int view, int split, bool transposed, int at, int T, int& lo, int& hi) {
  lo = 0; hi = T;
  if (view == FIL_SEQ_VIEW_CAUSAL) {
    if (transposed) lo = at; else hi = at + 1;
  } else if (view == FIL_SEQ_VIEW_CROSS) {
    if (at < split) lo = split; else hi = split;
  }
}

// q . k over the head's D = 4 DQ columns, one fmaf chain in column order (a in registers, b in LDS)
template <int DQM>
__device__ __forceinline__ float sa_dot(const float4 (&a)[DQM], const float* b, int DQ) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < DQM; ++d)
    if (d < DQ) {
      const float4 v = *reinterpret_cast<const float4*>(b + 4 * d);
      s = fmaf(a[d].x, v.x, s); s = fmaf(a[d].y, v.y, s); s = fmaf(a[d].z, v.z, s); s = fmaf(a[d].w, v.w, s);
    }
  return s;
}

// the same chain with both operands in LDS
__device__ __forceinline__ float sa_dot_lds(const float* a, const float* b, int DQ) {
  float s = 0.f;
  for (int d = 0; d < DQ; ++d) {
    const float4 u = *reinterpret_cast<const float4*>(a + 4 * d);
    const float4 v = *reinterpret_cast<const float4*>(b + 4 * d);
    s = fmaf(u.x, v.x, s); s = fmaf(u.y, v.y, s); s = fmaf(u.z, v.z, s); s = fmaf(u.w, v.w, s);
  }
  return s;
}

template <int DQM>
__device__ __forceinline__ void sa_axpy(float4 (&acc)[DQM], float a, const float* b, int DQ) {
#pragma unroll
  for (int d = 0; d < DQM; ++d)
    if (d < DQ) {
      const float4 v = *reinterpret_cast<const float4*>(b + 4 * d);
      acc[d].x = fmaf(a, v.x, acc[d].x); acc[d].y = fmaf(a, v.y, acc[d].y);
      acc[d].z = fmaf(a, v.z, acc[d].z); acc[d].w = fmaf(a, v.w, acc[d].w);
    }
}

// rows of `width` floats (a multiple of 4) of the tile's LIVE positions: global [B,T,width] -> LDS [NS][T][pitch]; zeros elsewhere
__device__ __forceinline__ void sa_stage_rows(float* dst, int pitch, const float* __restrict__ src, int width, long src_pitch,
                                              const float* live, long b0, int NS, int T) {
  const int WQ = width / 4, n = NS * T * WQ;
  for (int idx = threadIdx.x; idx < n; idx += blockDim.x) {
    const int pos = idx / WQ, wq = idx - pos * WQ;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live[pos] != 0.f) v = *reinterpret_cast<const float4*>(src + (b0 * T + pos) * src_pitch + wq * 4);
    *reinterpret_cast<float4*>(dst + pos * pitch + wq * 4) = v;
  }
}

// live flags (1 / 0) of the tile's positions; a sample past B is all masked
__device__ __forceinline__ void sa_stage_live(float* live, const unsigned char* __restrict__ mask, long b0, int B, int NS, int T) {
  for (int idx = threadIdx.x; idx < NS * T; idx += blockDim.x) {
    const long bb = b0 + idx / T;
    live[idx] = (bb < B && (mask == nullptr || mask[b0 * T + idx] != 0)) ? 1.f : 0.f;
  }
}

template <int DQM, bool GEN>
__global__ __launch_bounds__(kSaThreads) void seqattn_fwd_kernel(const float* __restrict__ x, const unsigned char* __restrict__ mask,
                                                                const float* __restrict__ Wq, const float* __restrict__ Wk,
                                                                const float* __restrict__ Wv, float* __restrict__ out,
                                                                float* __restrict__ pooled, float* __restrict__ saved, int B,
                                                                SaLayout L) {
  extern __shared__ __attribute__((aligned(16))) float sa_smem[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int T = L.T, K = L.K, H = L.H, D = L.D, HD = L.HD, KP = L.KP, HDP = L.HDP, NS = L.NS, DQ = L.D / 4;
  float* xs = sa_smem;
  float* qs = sa_smem + L.f_q;
  float* ks = sa_smem + L.f_k;
  float* vs = sa_smem + L.f_v;
  float* live = sa_smem + L.f_live;
  const long n_tiles = ((long)B + NS - 1) / NS;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long b0 = tile * NS;
    __syncthreads();      // the previous tile's images are free
    sa_stage_live(live, mask, b0, B, NS, T);
    __syncthreads();
    sa_stage_rows(xs, KP, x, K, K, live, b0, NS, T);
    __syncthreads();
    // q, k, v of the live positions: four columns of one position per thread
    {
      const int CQ = HD / 4, n = NS * T * CQ;
      for (int idx = tid; idx < n; idx += nthr) {
        const int pos = idx / CQ, c = (idx - pos * CQ) * 4;
        if (live[pos] == 0.f) continue;
        float4 aq = make_float4(0.f, 0.f, 0.f, 0.f), ak = aq, av = aq;
        const float* xr = xs + pos * KP;
        for (int k4 = 0; k4 < K; k4 += 4) {
          const float4 xv = *reinterpret_cast<const float4*>(xr + k4);
          const float xe[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const long w = (long)(k4 + e) * HD + c;
            const float4 wq = *reinterpret_cast<const float4*>(Wq + w);
            const float4 wk = *reinterpret_cast<const float4*>(Wk + w);
            const float4 wv = *reinterpret_cast<const float4*>(Wv + w);
            aq.x = fmaf(xe[e], wq.x, aq.x); aq.y = fmaf(xe[e], wq.y, aq.y); aq.z = fmaf(xe[e], wq.z, aq.z); aq.w = fmaf(xe[e], wq.w, aq.w);
            ak.x = fmaf(xe[e], wk.x, ak.x); ak.y = fmaf(xe[e], wk.y, ak.y); ak.z = fmaf(xe[e], wk.z, ak.z); ak.w = fmaf(xe[e], wk.w, ak.w);
            av.x = fmaf(xe[e], wv.x, av.x); av.y = fmaf(xe[e], wv.y, av.y); av.z = fmaf(xe[e], wv.z, av.z); av.w = fmaf(xe[e], wv.w, av.w);
          }
        }
        *reinterpret_cast<float4*>(qs + pos * HDP + c) = aq;
        *reinterpret_cast<float4*>(ks + pos * HDP + c) = ak;
        *reinterpret_cast<float4*>(vs + pos * HDP + c) = av;
        if (saved != nullptr) {
          float* sv = saved + (b0 * T + pos) * 3 * HD + c;
          *reinterpret_cast<float4*>(sv) = aq;
          *reinterpret_cast<float4*>(sv + HD) = ak;
          *reinterpret_cast<float4*>(sv + 2 * HD) = av;
        }
      }
    }
    __syncthreads();
    // one (sample, head, row) per thread, rows fastest
    {
      const int n = NS * H * T;
      for (int idx = tid; idx < n; idx += nthr) {
        const int sh = idx / T, i = idx - sh * T;
        const int s = sh / H, h = sh - s * H;
        const long bb = b0 + s;
        if (bb >= B) continue;
        const float* lv = live + s * T;
        float4 acc[DQM];
#pragma unroll
        for (int d = 0; d < DQM; ++d) acc[d] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lv[i] != 0.f) {
          float4 qr[DQM];
#pragma unroll
          for (int d = 0; d < DQM; ++d)
            qr[d] = d < DQ ? *reinterpret_cast<const float4*>(qs + (s * T + i) * HDP + h * D + 4 * d) : make_float4(0.f, 0.f, 0.f, 0.f);
          const float* kh = ks + s * T * HDP + h * D;
          const float* vh = vs + s * T * HDP + h * D;
          int j0 = 0, j1 = T;
          if (GEN) sa_range(L.view, L.split, false, i, T, j0, j1);
          float m = -INFINITY;
          for (int j = j0; j < j1; ++j)
            if (lv[j] != 0.f) m = fmaxf(m, sa_dot<DQM>(qr, kh + j * HDP, DQ) * L.scale);
          float sum = 0.f;
          for (int j = j0; j < j1; ++j)
            if (lv[j] != 0.f) {
              const float e = expf(sa_dot<DQM>(qr, kh + j * HDP, DQ) * L.scale - m);
              sum += e;
              sa_axpy<DQM>(acc, e, vh + j * HDP, DQ);
            }
          const float inv = GEN && sum == 0.f ? 0.f : 1.f / sum;      // no live key in the range: the row is 0
#pragma unroll
          for (int d = 0; d < DQM; ++d) { acc[d].x *= inv; acc[d].y *= inv; acc[d].z *= inv; acc[d].w *= inv; }
          // out_i takes the place of q_i (which only this thread reads) for the pooling pass
          if (GEN && pooled != nullptr) {
#pragma unroll
            for (int d = 0; d < DQM; ++d)
              if (d < DQ) *reinterpret_cast<float4*>(qs + (s * T + i) * HDP + h * D + 4 * d) = acc[d];
          }
        }
        if (!GEN || out != nullptr) {
          float* o = out + (bb * T + i) * HD + h * D;
#pragma unroll
          for (int d = 0; d < DQM; ++d)
            if (d < DQ) *reinterpret_cast<float4*>(o + 4 * d) = acc[d];
        }
      }
    }
    // pooled[b] = (sum of out_i over the live i, in position order) / (their number); a thread per (sample, column)
    if (GEN && pooled != nullptr) {
      __syncthreads();
      const int n = NS * HD;
      for (int idx = tid; idx < n; idx += nthr) {
        const int s = idx / HD, c = idx - s * HD;
        const long bb = b0 + s;
        if (bb >= B) continue;
        const float* lv = live + s * T;
        const float* os = qs + s * T * HDP + c;
        float acc = 0.f;
        int cnt = 0;
        for (int i = 0; i < T; ++i)
          if (lv[i] != 0.f) { acc += os[i * HDP]; ++cnt; }
        pooled[bb * HD + c] = cnt > 0 ? acc / (float)cnt : 0.f;
      }
    }
  }
}

template <int DQM, bool GEN>
__global__ __launch_bounds__(kSaThreads) void seqattn_bwd_kernel(const float* __restrict__ x, const unsigned char* __restrict__ mask,
                                                                const float* __restrict__ Wq, const float* __restrict__ Wk,
                                                                const float* __restrict__ Wv, const float* __restrict__ saved,
                                                                const float* __restrict__ g, const float* __restrict__ gpool,
                                                                float* __restrict__ dx, float* __restrict__ partials, int B,
                                                                SaLayout L) {
  extern __shared__ __attribute__((aligned(16))) float sa_smem[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int T = L.T, K = L.K, H = L.H, D = L.D, HD = L.HD, KP = L.KP, HDP = L.HDP, NS = L.NS, DQ = L.D / 4;
  float* xs = sa_smem;
  float* gs = sa_smem + L.b_g;
  float* qs = sa_smem + L.b_q;
  float* ks = sa_smem + L.b_k;      // dk after phase 3
  float* vs = sa_smem + L.b_v;      // dv after phase 3
  float* dqs = sa_smem + L.b_dq;
  float* st = sa_smem + L.b_st;
  float* live = sa_smem + L.b_live;
  const bool want_params = partials != nullptr;
  const long n_tiles = ((long)B + NS - 1) / NS;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long b0 = tile * NS;
    __syncthreads();      // the previous tile's images are free
    sa_stage_live(live, mask, b0, B, NS, T);
    __syncthreads();
    if (want_params) sa_stage_rows(xs, KP, x, K, K, live, b0, NS, T);
    if (!GEN || g != nullptr) {
      sa_stage_rows(gs, HDP, g, HD, HD, live, b0, NS, T);
    } else {
      // the pooled form: g_i = gpool[b] / n_b at every live i.  n_b waits in the statistics' place, which the row pass writes later
      for (int s = tid; s < NS; s += nthr) {
        int cnt = 0;
        for (int i = 0; i < T; ++i) cnt += live[s * T + i] != 0.f;
        st[s] = (float)cnt;
      }
      __syncthreads();
      const int WQ = HD / 4, n = NS * T * WQ;
      for (int idx = tid; idx < n; idx += nthr) {
        const int pos = idx / WQ, wq = idx - pos * WQ, s = pos / T;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live[pos] != 0.f) {
          const float4 gp = *reinterpret_cast<const float4*>(gpool + (b0 + s) * HD + wq * 4);
          const float nb = st[s];
          v = make_float4(gp.x / nb, gp.y / nb, gp.z / nb, gp.w / nb);
        }
        *reinterpret_cast<float4*>(gs + pos * HDP + wq * 4) = v;
      }
    }
    sa_stage_rows(qs, HDP, saved, HD, 3L * HD, live, b0, NS, T);
    sa_stage_rows(ks, HDP, saved + HD, HD, 3L * HD, live, b0, NS, T);
    sa_stage_rows(vs, HDP, saved + 2 * HD, HD, 3L * HD, live, b0, NS, T);
    __syncthreads();
    // rows: the softmax statistics and dq
    {
      const int n = NS * H * T;
      for (int idx = tid; idx < n; idx += nthr) {
        const int sh = idx / T, i = idx - sh * T;
        const int s = sh / H, h = sh - s * H;
        const float* lv = live + s * T;
        float4 acc[DQM];
#pragma unroll
        for (int d = 0; d < DQM; ++d) acc[d] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lv[i] != 0.f) {
          float4 qr[DQM];
#pragma unroll
          for (int d = 0; d < DQM; ++d)
            qr[d] = d < DQ ? *reinterpret_cast<const float4*>(qs + (s * T + i) * HDP + h * D + 4 * d) : make_float4(0.f, 0.f, 0.f, 0.f);
          const float* kh = ks + s * T * HDP + h * D;
          const float* vh = vs + s * T * HDP + h * D;
          const float* gi = gs + (s * T + i) * HDP + h * D;
          int j0 = 0, j1 = T;
          if (GEN) sa_range(L.view, L.split, false, i, T, j0, j1);
          float m = -INFINITY;
          int top = GEN ? j0 : i;      // (every view but CROSS: row i is live, so key i is)
          for (int j = j0; j < j1; ++j)
            if (lv[j] != 0.f) {
              const float sc = sa_dot<DQM>(qr, kh + j * HDP, DQ) * L.scale;
              if (sc > m) { m = sc; top = j; }
            }
          // everything relative to the top key: a row with one live key gives ds = 0 exactly, a peaked row keeps its digits
          const float c = sa_dot_lds(gi, vh + top * HDP, DQ);
          float sum = 0.f, wsum = 0.f;
          for (int j = j0; j < j1; ++j)
            if (lv[j] != 0.f) {
              const float e = expf(sa_dot<DQM>(qr, kh + j * HDP, DQ) * L.scale - m);
              const float a = j == top ? 0.f : sa_dot_lds(gi, vh + j * HDP, DQ) - c;
              sum += e;
              wsum = fmaf(e, a, wsum);
            }
          const float inv = GEN && sum == 0.f ? 0.f : 1.f / sum;      // no live key in the range: the row sends nothing
          const float abar = wsum * inv;
          for (int j = j0; j < j1; ++j)
            if (lv[j] != 0.f) {
              const float e = expf(sa_dot<DQM>(qr, kh + j * HDP, DQ) * L.scale - m);
              const float a = j == top ? 0.f : sa_dot_lds(gi, vh + j * HDP, DQ) - c;
              const float ds = (e * inv) * (a - abar);
              sa_axpy<DQM>(acc, ds, kh + j * HDP, DQ);
            }
#pragma unroll
          for (int d = 0; d < DQM; ++d) { acc[d].x *= L.scale; acc[d].y *= L.scale; acc[d].z *= L.scale; acc[d].w *= L.scale; }
          float* sr = st + (long)idx * kSaStat;
          sr[0] = m; sr[1] = inv; sr[2] = abar; sr[3] = c; sr[4] = __int_as_float(top);
        }
#pragma unroll
        for (int d = 0; d < DQM; ++d)
          if (d < DQ) *reinterpret_cast<float4*>(dqs + (s * T + i) * HDP + h * D + 4 * d) = acc[d];
      }
    }
    __syncthreads();
    // columns: dk_j, dv_j in row order; they take the place of k_j, v_j (which only this thread reads)
    {
      const int n = NS * H * T;
      for (int idx = tid; idx < n; idx += nthr) {
        const int sh = idx / T, j = idx - sh * T;
        const int s = sh / H, h = sh - s * H;
        const float* lv = live + s * T;
        if (lv[j] == 0.f) continue;      // k_j, v_j were staged as zeros: dk_j = dv_j = 0 stands
        float* kj = ks + (s * T + j) * HDP + h * D;
        float* vj = vs + (s * T + j) * HDP + h * D;
        float4 kr[DQM], dk[DQM], dv[DQM];
#pragma unroll
        for (int d = 0; d < DQM; ++d) {
          kr[d] = d < DQ ? *reinterpret_cast<const float4*>(kj + 4 * d) : make_float4(0.f, 0.f, 0.f, 0.f);
          dk[d] = make_float4(0.f, 0.f, 0.f, 0.f);
          dv[d] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float* qh = qs + s * T * HDP + h * D;
        const float* gh = gs + s * T * HDP + h * D;
        const float* sth = st + (long)sh * T * kSaStat;
        int i0 = 0, i1 = T;
        if (GEN) sa_range(L.view, L.split, true, j, T, i0, i1);
        for (int i = i0; i < i1; ++i)
          if (lv[i] != 0.f) {
            const float* sr = sth + i * kSaStat;
            const float m = sr[0], inv = sr[1], abar = sr[2], c = sr[3];
            const int top = __float_as_int(sr[4]);
            if (GEN && inv == 0.f) continue;      // a row without keys
            // q_i . k_j with the operands' roles as in the row pass: the same bits
            float sc = 0.f;
#pragma unroll
            for (int d = 0; d < DQM; ++d)
              if (d < DQ) {
                const float4 u = *reinterpret_cast<const float4*>(qh + i * HDP + 4 * d);
                sc = fmaf(u.x, kr[d].x, sc); sc = fmaf(u.y, kr[d].y, sc); sc = fmaf(u.z, kr[d].z, sc); sc = fmaf(u.w, kr[d].w, sc);
              }
            const float p = expf(sc * L.scale - m) * inv;
            const float a = j == top ? 0.f : sa_dot_lds(gh + i * HDP, vj, DQ) - c;
            const float ds = p * (a - abar);
            sa_axpy<DQM>(dk, ds, qh + i * HDP, DQ);
            sa_axpy<DQM>(dv, p, gh + i * HDP, DQ);
          }
#pragma unroll
        for (int d = 0; d < DQM; ++d)
          if (d < DQ) {
            *reinterpret_cast<float4*>(kj + 4 * d) = make_float4(dk[d].x * L.scale, dk[d].y * L.scale, dk[d].z * L.scale, dk[d].w * L.scale);
            *reinterpret_cast<float4*>(vj + 4 * d) = dv[d];
          }
      }
    }
    __syncthreads();
    // dx = dq Wq^T + dk Wk^T + dv Wv^T; exactly 0 at a masked position
    if (dx != nullptr) {
      const int n = NS * T * K;
      for (int idx = tid; idx < n; idx += nthr) {
        const int pos = idx / K, kk = idx - pos * K;
        if (b0 + pos / T >= B) continue;
        float v = 0.f;
        if (live[pos] != 0.f) {
          const float* wq = Wq + (long)kk * HD;
          const float* wk = Wk + (long)kk * HD;
          const float* wv = Wv + (long)kk * HD;
          const float* a = dqs + pos * HDP;
          const float* b = ks + pos * HDP;
          const float* c = vs + pos * HDP;
          for (int c4 = 0; c4 < HD; c4 += 4) {
            const float4 da = *reinterpret_cast<const float4*>(a + c4), wa = *reinterpret_cast<const float4*>(wq + c4);
            const float4 db = *reinterpret_cast<const float4*>(b + c4), wb = *reinterpret_cast<const float4*>(wk + c4);
            const float4 dc = *reinterpret_cast<const float4*>(c + c4), wc = *reinterpret_cast<const float4*>(wv + c4);
            v = fmaf(da.x, wa.x, v); v = fmaf(da.y, wa.y, v); v = fmaf(da.z, wa.z, v); v = fmaf(da.w, wa.w, v);
            v = fmaf(db.x, wb.x, v); v = fmaf(db.y, wb.y, v); v = fmaf(db.z, wb.z, v); v = fmaf(db.w, wb.w, v);
            v = fmaf(dc.x, wc.x, v); v = fmaf(dc.y, wc.y, v); v = fmaf(dc.z, wc.z, v); v = fmaf(dc.w, wc.w, v);
          }
        }
        dx[(b0 * T + pos) * K + kk] = v;
      }
    }
    // the tile's x^T [dq | dk | dv] in position order -> the workgroup's partial (its first tile writes, the others add; an element
    // has the same owner thread in every tile)
    if (want_params) {
      float* part = partials + (long)blockIdx.x * L.n_out;
      const bool first = tile == (long)blockIdx.x;
      const int CQ = HD / 4, per = K * CQ, n = 3 * per;
      for (int idx = tid; idx < n; idx += nthr) {
        const int w = idx / per, r = idx - w * per;
        const int kk = r / CQ, c = (r - kk * CQ) * 4;
        const float* d = (w == 0 ? dqs : (w == 1 ? ks : vs)) + c;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int pos = 0; pos < NS * T; ++pos)
          if (live[pos] != 0.f) {
            const float xv = xs[pos * KP + kk];
            const float4 dv = *reinterpret_cast<const float4*>(d + pos * HDP);
            acc.x = fmaf(xv, dv.x, acc.x); acc.y = fmaf(xv, dv.y, acc.y); acc.z = fmaf(xv, dv.z, acc.z); acc.w = fmaf(xv, dv.w, acc.w);
          }
        float* o = part + (long)w * K * HD + (long)kk * HD + c;
        if (first) { o[0] = acc.x; o[1] = acc.y; o[2] = acc.z; o[3] = acc.w; }
        else { o[0] += acc.x; o[1] += acc.y; o[2] += acc.z; o[3] += acc.w; }
      }
    }
  }
}

// argument and menu checks shared by the entry points
static int sa_dims(const char* who, int B, int T, int K, int H, int D, int use_scale, SaLayout* L) {
  FIL_CHECK_ARG_W(who, B >= 0 && T >= 1 && K >= 1 && H >= 1 && D >= 1);
  if (K % 4 != 0 || K > kSaMaxK) return fail(FIL_ERR_UNSUPPORTED, "%s: K=%d needs K %% 4 == 0 and K <= %d", who, K, kSaMaxK);
  if (D % 4 != 0) return fail(FIL_ERR_UNSUPPORTED, "%s: D=%d needs D %% 4 == 0", who, D);
  if (H > kSaMaxH) return fail(FIL_ERR_UNSUPPORTED, "%s: H=%d needs H <= %d", who, H, kSaMaxH);
  if ((long)H * D > kSaMaxHD) return fail(FIL_ERR_UNSUPPORTED, "%s: H*D=%ld needs H*D <= %d", who, (long)H * D, kSaMaxHD);
  if (T > kSaMaxT) return fail(FIL_ERR_UNSUPPORTED, "%s: T=%d needs T <= %d", who, T, kSaMaxT);
  const int fb = 4 * (sa_fwd_floats(T, K, H * D) + 8), bb = 4 * (sa_bwd_floats(T, K, H, H * D) + 8);
  if (fb > kTiledLdsLimit || bb > kTiledLdsLimit)
    return fail(FIL_ERR_UNSUPPORTED, "%s: T=%d K=%d H=%d D=%d needs %d bytes of LDS (limit %d)", who, T, K, H, D, std::max(fb, bb), kTiledLdsLimit);
  *L = sa_layout(B, T, K, H, D, use_scale);
  return FIL_OK;
}

template <int DQM, bool GEN>
static int sa_launch_fwd(const char* who, const float* x, const unsigned char* mask, const float* Wq, const float* Wk, const float* Wv,
                         float* out, float* pooled, float* saved, int B, const SaLayout& L, hipStream_t st) {
  if (int rc = tiled_allow_lds(who, seqattn_fwd_kernel<DQM, GEN>, L.lds_fwd)) return rc;
  hipLaunchKernelGGL((seqattn_fwd_kernel<DQM, GEN>), dim3(sa_grid(B, L.NS)), dim3(kSaThreads), L.lds_fwd, st, x, mask, Wq, Wk, Wv, out,
                     pooled, saved, B, L);
  return FIL_OK;
}

template <int DQM, bool GEN>
static int sa_launch_bwd(const char* who, const float* x, const unsigned char* mask, const float* Wq, const float* Wk, const float* Wv,
                         const float* saved, const float* g, const float* gpool, float* dx, float* partials, int B, const SaLayout& L,
                         hipStream_t st) {
  if (int rc = tiled_allow_lds(who, seqattn_bwd_kernel<DQM, GEN>, L.lds_bwd)) return rc;
  hipLaunchKernelGGL((seqattn_bwd_kernel<DQM, GEN>), dim3(sa_grid(B, L.NS)), dim3(kSaThreads), L.lds_bwd, st, x, mask, Wq, Wk, Wv, saved,
                     g, gpool, dx, partials, B, L);
  return FIL_OK;
}

// the view's own argument rules (after sa_dims: T is known to be positive)
static int sa_view(const char* who, int T, int view, int split, SaLayout* L) {
  if (view != FIL_SEQ_VIEW_FULL && view != FIL_SEQ_VIEW_CAUSAL && view != FIL_SEQ_VIEW_CROSS)
    return fail(FIL_ERR_ARG, "%s: view=%d is none of FIL_SEQ_VIEW_FULL (0), _CAUSAL (1), _CROSS (2)", who, view);
  if (view != FIL_SEQ_VIEW_CROSS && split != 0)
    return fail(FIL_ERR_ARG, "%s: split=%d needs the cross view (view=%d takes split = 0)", who, split, view);
  if (view == FIL_SEQ_VIEW_CROSS && (split < 1 || split >= T))
    return fail(FIL_ERR_ARG, "%s: split=%d of the cross view needs 1 <= split <= T - 1 = %d", who, split, T - 1);
  L->view = view; L->split = split;
  return FIL_OK;
}

// the body of both forward entry points
static int sa_fwd(const char* who, const float* x, const unsigned char* mask, const float* Wq, const float* Wk, const float* Wv, float* out,
                  float* pooled, float* saved, int B, int T, int K, int H, int D, int use_scale, int view, int split, void* stream) {
  SaLayout L;
  if (int rc = sa_dims(who, B, T, K, H, D, use_scale, &L)) return rc;
  if (int rc = sa_view(who, T, view, split, &L)) return rc;
  if (B == 0) return FIL_OK;
  FIL_CHECK_ARG_W(who, x != nullptr && Wq != nullptr && Wk != nullptr && Wv != nullptr);
  if (out == nullptr && pooled == nullptr) return fail(FIL_ERR_ARG, "%s: out and pooled are both NULL: nothing to write", who);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("seqattn_fwd", st,
               4.0 * (double)B * (T * (K + (out != nullptr ? L.HD : 0) + (saved != nullptr ? 3.0 * L.HD : 0.0)) + (pooled != nullptr ? L.HD : 0)));
  const int DQ = D / 4;
#define SA_FWD(DQM, V) sa_launch_fwd<DQM, V>(who, x, mask, Wq, Wk, Wv, out, pooled, saved, B, L, st)
  const int rc = view == FIL_SEQ_VIEW_FULL && pooled == nullptr ? (DQ <= 2 ? SA_FWD(2, false) : DQ <= 4 ? SA_FWD(4, false) : DQ <= 8 ? SA_FWD(8, false) : SA_FWD(16, false))
                                                                : (DQ <= 2 ? SA_FWD(2, true) : DQ <= 4 ? SA_FWD(4, true) : DQ <= 8 ? SA_FWD(8, true) : SA_FWD(16, true));
#undef SA_FWD
  if (rc) return rc;
  FIL_CHECK_LAUNCH_W(who);
  return FIL_OK;
}

// the body of both backward entry points
static int sa_bwd(const char* who, const float* x, const unsigned char* mask, const float* Wq, const float* Wk, const float* Wv,
                  const float* saved, const float* g, const float* gpool, float* dx, float* dWq, float* dWk, float* dWv, void* workspace,
                  size_t workspace_bytes, int B, int T, int K, int H, int D, int use_scale, int view, int split, void* stream) {
  SaLayout L;
  if (int rc = sa_dims(who, B, T, K, H, D, use_scale, &L)) return rc;
  if (int rc = sa_view(who, T, view, split, &L)) return rc;
  if (B == 0) return FIL_OK;
  FIL_CHECK_ARG_W(who, x != nullptr && Wq != nullptr && Wk != nullptr && Wv != nullptr && saved != nullptr);
  if ((g != nullptr) == (gpool != nullptr))
    return fail(FIL_ERR_ARG, "%s: exactly one of g and gpool is given, got %s", who, g != nullptr ? "both" : "neither");
  const bool want_params = dWq != nullptr || dWk != nullptr || dWv != nullptr;
  FIL_CHECK_ARG_W(who, dx != nullptr || want_params);
  const int nparts = sa_grid(B, L.NS);
  if (want_params)
    if (int rc = tiled_check_workspace(who, workspace, workspace_bytes, nparts, L.n_out)) return rc;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("seqattn_bwd", st, 4.0 * (double)B * (T * (2.0 * K + 3.0 * L.HD) + (g != nullptr ? T : 1) * L.HD));
  float* partials = want_params ? static_cast<float*>(workspace) : nullptr;
  const int DQ = D / 4;
#define SA_BWD(DQM, V) sa_launch_bwd<DQM, V>(who, x, mask, Wq, Wk, Wv, saved, g, gpool, dx, partials, B, L, st)
  const int rc = view == FIL_SEQ_VIEW_FULL && gpool == nullptr ? (DQ <= 2 ? SA_BWD(2, false) : DQ <= 4 ? SA_BWD(4, false) : DQ <= 8 ? SA_BWD(8, false) : SA_BWD(16, false))
                                                               : (DQ <= 2 ? SA_BWD(2, true) : DQ <= 4 ? SA_BWD(4, true) : DQ <= 8 ? SA_BWD(8, true) : SA_BWD(16, true));
#undef SA_BWD
  if (rc) return rc;
  FIL_CHECK_LAUNCH_W(who);
  if (want_params) {
    const int off[4] = {0, K * L.HD, 2 * K * L.HD, L.n_out};
    float* outs[3] = {dWq, dWk, dWv};
    param_reduce_launch(partials, nparts, outs, off, 3, st);
    FIL_CHECK_LAUNCH_W(who);
  }
  return FIL_OK;
}

}  // namespace fil

using namespace fil;

extern "C" int fil_seqattn_plan(int B, int T, int K, int H, int D, int* plan) {
  SaLayout L;
  if (int rc = sa_dims(__func__, B, T, K, H, D, 1, &L)) return rc;
  FIL_CHECK_ARG(plan != nullptr);
  tiled_plan(plan, L.NS, sa_grid(B, L.NS), kSaGridCap, L.lds_fwd, L.lds_bwd);
  return FIL_OK;
}

extern "C" size_t fil_seqattn_saved_bytes(int B, int T, int K, int H, int D) {
  SaLayout L;
  if (sa_dims(__func__, B, T, K, H, D, 1, &L) != FIL_OK) return 0;
  return align_up((size_t)B * (size_t)T * 3 * (size_t)L.HD * sizeof(float), 256);
}

extern "C" size_t fil_seqattn_bwd_workspace_bytes(int B, int T, int K, int H, int D) {
  SaLayout L;
  if (sa_dims(__func__, B, T, K, H, D, 1, &L) != FIL_OK) return 0;
  return tiled_partial_bytes(sa_grid(B, L.NS), L.n_out);
}

extern "C" int fil_seqattn_fwd_v(const float* x, const unsigned char* mask, const float* Wq, const float* Wk, const float* Wv, float* out,
                                 float* pooled, float* saved, int B, int T, int K, int H, int D, int use_scale, int view, int split,
                                 void* stream) {
  return sa_fwd(__func__, x, mask, Wq, Wk, Wv, out, pooled, saved, B, T, K, H, D, use_scale, view, split, stream);
}

extern "C" int fil_seqattn_bwd_v(const float* x, const unsigned char* mask, const float* Wq, const float* Wk, const float* Wv,
                                 const float* saved, const float* g, const float* gpool, float* dx, float* dWq, float* dWk, float* dWv,
                                 void* workspace, size_t workspace_bytes, int B, int T, int K, int H, int D, int use_scale, int view,
                                 int split, void* stream) {
  return sa_bwd(__func__, x, mask, Wq, Wk, Wv, saved, g, gpool, dx, dWq, dWk, dWv, workspace, workspace_bytes, B, T, K, H, D, use_scale,
                view, split, stream);
}

// the first form: the FULL view, rows out, g rows in
extern "C" int fil_seqattn_fwd(const float* x, const unsigned char* mask, const float* Wq, const float* Wk, const float* Wv, float* out,
                               float* saved, int B, int T, int K, int H, int D, int use_scale, void* stream) {
  return sa_fwd(__func__, x, mask, Wq, Wk, Wv, out, nullptr, saved, B, T, K, H, D, use_scale, FIL_SEQ_VIEW_FULL, 0, stream);
}

extern "C" int fil_seqattn_bwd(const float* x, const unsigned char* mask, const float* Wq, const float* Wk, const float* Wv,
                               const float* out, const float* saved, const float* g, float* dx, float* dWq, float* dWk, float* dWv,
                               void* workspace, size_t workspace_bytes, int B, int T, int K, int H, int D, int use_scale, void* stream) {
  if (B > 0 && T >= 1 && K >= 1 && H >= 1 && D >= 1) FIL_CHECK_ARG(out != nullptr);      // (kept for a caller-side check; not read)
  return sa_bwd(__func__, x, mask, Wq, Wk, Wv, saved, g, nullptr, dx, dWq, dWk, dWv, workspace, workspace_bytes, B, T, K, H, D, use_scale,
                FIL_SEQ_VIEW_FULL, 0, stream);
}
