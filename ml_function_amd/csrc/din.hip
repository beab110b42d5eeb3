// N3  DIN attention pooling over a behaviour sequence for gfx950, forward and backward, fp32.
//
// The Deep Interest Network's activation unit (the paper's layer; offered as an extension): the candidate q [B,K] scores every item
// of the history keys [B,T,K] through a two-layer MLP on x_t = [q, k_t, q - k_t, q * k_t] and the history is pooled with the scores:
//     h1 = act(x_t W1 + b1),  h2 = act(h1 W2 + b2),  s_t = h2 . w3 + b3,
//     out = sum_t a_t k_t,    a_t = s_t (raw, the paper) or softmax over the LIVE slots (flag bit 0);  masked slots: a_t = 0.
// act = PReLU with a slope per unit, or the logistic sigmoid (flag bit 1).  Nothing of size B T n with n >= K leaves the chip in
// either direction other than keys and dkeys: per sample the kernels read q, the [T,K] keys (backward: also g and the T + 2 saved
// scores and softmax statistics) and write [K] and T + 2 statistics (backward: [K] and [T,K]).
//
// Structure (both directions, after afm.hip): a wave owns whole samples and has its own LDS region; W1, W2 (zero-padded to H1C rows
// of kDinCH units / H2T columns), the biases, slopes and w3 are staged ONCE per workgroup; the history is processed 64 slots at a
// time with lane = slot, its key rows in LDS at a stride of KP dwords with KP/4 odd.  A masked slot's key is never read: its LDS row
// is zero.
//   forward   pass 1: lane = slot: the score (layer 1 in chunks of kDinCH units straight into the H2T layer-2 accumulators held in
//             registers; the weights are broadcast LDS reads), scores -> LDS; wave max, exp, wave sum.  pass 2: lane = (k quad, slot
//             group): the weighted sum of the keys, group partials added in group order, ONE division by the softmax denominator.
//             NS <= 4 samples per workgroup (64 NS threads).
//   backward  always 256 threads; waves 0 .. NS-1 own the samples of a tile, ALL threads own the parameter gradients.  Per 64 slots:
//             0  softmax: g.out = sum_t a_t (g.k_t) from the saved scores, one pass over the keys; both relative to g.k of the slot
//                with the largest score, so that a weight of nearly 1 costs ds no digits.
//             A  lane = slot: the score again (same code, same bits), a_t, ds_t = a_t (g.k_t - g.out) [softmax] or g.k_t [raw],
//                u1 (PReLU) or h1 (sigmoid) -> LDS, du2 -> LDS and registers; db2, dalpha2, dw3, db3 by a butterfly over the lanes.
//             P2 (barrier) every thread: its 4 x 16 tile(s) of dW2 += h1^T du2 over the tile's samples, in registers.
//             B  lane = slot: du1 = (du2 W2^T) act'(u1) over the staged u1, in place; dalpha1.
//             C  lane = slot: dx = du1 W1^T, 16 inputs at a time; dkeys row -> global, the dq terms -> LDS.
//             P1 (barrier) every thread: its 4 x 16 tile(s) of dW1 += x^T du1; db1 by column.
//             4K H1 + H1 H2 <= 16384 bounds the tiles at two per thread (128 accumulators).  One partial per workgroup;
//             param_reduce_kernel adds the partials in a fixed order.
// No atomics; every sum has a fixed order for a given B, so repeats are bit-identical.
#include "common.h"
#include "param_reduce.h"
#include "tiled_launch.h"
#include <algorithm>
#include <math.h>

namespace fil {

constexpr int kDinMaxSamples = 4;      // samples in flight per workgroup
constexpr int kDinGridCap = 512;       // workgroups per launch
constexpr int kDinMaxK = 64, kDinMaxT = 256, kDinMaxH1 = 128, kDinMaxH2 = 64, kDinMaxParams = 16384;
constexpr int kDinCH = 8;              // layer-1 units per register chunk
constexpr int kDinBwdThreads = 256;
constexpr int kDinRedWave = 3 * 64 + 4;   // lane-held sums a sample wave hands over at the end: db2 | dw3 | dalpha2 | db3

// LDS layout, all offsets in floats (multiples of 4: every region is read in 16-byte pieces).
//   shared by the workgroup: W1 [4K][H1C] | b1 [H1C] | alpha1 [H1C] | W2 [H1C][H2T] | b2 | alpha2 | w3 [H2T] | b3 [4] | red [4][196]
//   per sample, forward:  keys [64][KP] | q [K] | scores [T] | group partials [64/KQ][K]
//   per sample, backward: keys [64][KP] | q [K] | g [K] | dq [K] | a [64] | dalpha1 [H1C] | u1/du1 [64][H1P] | du2 [64][H2P]
struct DinLayout {
  int T, K, H1, H2, H1C, H2T, N2, KP, KQ, H1P, H2P, NS;
  int o_b1, o_al1, o_W2, o_b2, o_al2, o_w3, o_b3, o_red, shared_f;
  int o_q, o_sc, o_part, samp_fwd;
  int o_g, o_dq, o_a, o_dal1, o_u1, o_du2, samp_bwd;
  int n_c1, n_t1, n_c2, n_t2;                                   // 4 x 16 tiles of dW1 (columns, count) and of dW2
  int p_b1, p_al1, p_W2, p_b2, p_al2, p_w3, p_b3, n_out;        // one partial: dW1 at 0, then these offsets
  int lds_fwd, lds_bwd;   // bytes
};

static inline int din_up(int v, int m) { return (v + m - 1) / m * m; }

static DinLayout din_layout(int T, int K, int H1, int H2, int NS) {
  DinLayout L;
  L.T = T; L.K = K; L.H1 = H1; L.H2 = H2; L.NS = NS;
  L.H1C = din_up(H1, kDinCH);
  L.H2T = din_up(H2, 16);
  L.N2 = L.H2T <= 16 ? 16 : (L.H2T <= 32 ? 32 : 64);
  L.KQ = K / 4;
  L.KP = (L.KQ % 2 == 0) ? K + 4 : K;
  L.H1P = din_up(H1, 16) + 4;
  L.H2P = L.H2T + 4;
  L.o_b1 = 4 * K * L.H1C;
  L.o_al1 = L.o_b1 + L.H1C;
  L.o_W2 = L.o_al1 + L.H1C;
  L.o_b2 = L.o_W2 + L.H1C * L.H2T;
  L.o_al2 = L.o_b2 + L.H2T;
  L.o_w3 = L.o_al2 + L.H2T;
  L.o_b3 = L.o_w3 + L.H2T;
  L.o_red = L.o_b3 + 4;
  L.shared_f = L.o_red + kDinMaxSamples * kDinRedWave;
  L.o_q = 64 * L.KP;
  L.o_sc = L.o_q + K;
  L.o_part = L.o_sc + din_up(T, 4);
  L.samp_fwd = L.o_part + (64 / L.KQ) * K;
  L.o_g = L.o_q + K;
  L.o_dq = L.o_g + K;
  L.o_a = L.o_dq + K;
  L.o_dal1 = L.o_a + 64;
  L.o_u1 = L.o_dal1 + L.H1C;
  L.o_du2 = L.o_u1 + 64 * L.H1P;
  L.samp_bwd = L.o_du2 + 64 * L.H2P;
  L.n_c1 = cdiv(H1, 16);
  L.n_t1 = K * L.n_c1;
  L.n_c2 = cdiv(H2, 16);
  L.n_t2 = cdiv(H1, 4) * L.n_c2;
  L.p_b1 = 4 * K * H1;
  L.p_al1 = L.p_b1 + H1;
  L.p_W2 = L.p_al1 + H1;
  L.p_b2 = L.p_W2 + H1 * H2;
  L.p_al2 = L.p_b2 + H2;
  L.p_w3 = L.p_al2 + H2;
  L.p_b3 = L.p_w3 + H2;
  L.n_out = L.p_b3 + 1;
  L.lds_fwd = 4 * (L.shared_f + NS * L.samp_fwd);
  L.lds_bwd = 4 * (L.shared_f + NS * L.samp_bwd);
  return L;
}

// the largest NS <= kDinMaxSamples whose footprints fit; NS = 0 in the result: not even one sample fits
static DinLayout din_pick(int T, int K, int H1, int H2) {
  for (int ns = kDinMaxSamples; ns >= 1; --ns) {
    const DinLayout L = din_layout(T, K, H1, H2, ns);
    if (L.lds_fwd <= kTiledLdsLimit && L.lds_bwd <= kTiledLdsLimit) return L;
  }
  DinLayout L = din_layout(T, K, H1, H2, 1);
  L.NS = 0;
  return L;
}

static inline int din_grid(int B, int NS) { return tiled_grid(B, NS, kDinGridCap); }

// Sums v[i] over the 64 lanes for every i < N (N a power of two <= 64) by a butterfly that halves the values at each step: N - 1 +
// (6 - log2 N) exchanges instead of 6 N.  The sum of element i = lane >> (6 - log2 N) is returned (the lanes that share i all hold
// it).  v is destroyed.  Fixed order.
template <int N>
__device__ __forceinline__ float din_lane_reduce(float (&v)[N], int lane) {
#pragma unroll
  for (int st = 0; st < 6; ++st) {
    const int o = 32 >> st;
    const int n = N >> st;
    if (n > 1) {
      const int half = n / 2;
      const bool up = (lane & o) != 0;
#pragma unroll
      for (int i = 0; i < half; ++i) {
        const float send = up ? v[i] : v[i + half];
        const float keep = up ? v[i + half] : v[i];
        v[i] = keep + __shfl_xor(send, o);
      }
    } else {
      v[0] += __shfl_xor(v[0], o);
    }
  }
  return v[0];
}

// a . b over 4 KQ elements, k ascending from +0 (g . out and g . k_t go through this one chain)
__device__ __forceinline__ float din_dot(const float* a, const float* b, int KQ) {
  float t = 0.f;
  for (int kq = 0; kq < KQ; ++kq) {
    const float4 av = *reinterpret_cast<const float4*>(a + kq * 4);
    const float4 bv = *reinterpret_cast<const float4*>(b + kq * 4);
    t = fmaf(av.x, bv.x, t);
    t = fmaf(av.y, bv.y, t);
    t = fmaf(av.z, bv.z, t);
    t = fmaf(av.w, bv.w, t);
  }
  return t;
}

template <bool SIG>
__device__ __forceinline__ float din_act(float u, float alpha) {
  if constexpr (SIG) return 1.f / (1.f + expf(-u));
  return u > 0.f ? u : alpha * u;
}

// the parameters -> LDS, once per workgroup (the caller synchronises)
__device__ __forceinline__ void din_stage_params(float* smem, const DinLayout& L, const float* __restrict__ W1, const float* __restrict__ b1,
                                                 const float* __restrict__ al1, const float* __restrict__ W2, const float* __restrict__ b2,
                                                 const float* __restrict__ al2, const float* __restrict__ w3, const float* __restrict__ b3) {
  const int H1 = L.H1, H2 = L.H2, H1C = L.H1C, H2T = L.H2T;
  for (int t = threadIdx.x; t < 4 * L.K * H1C; t += blockDim.x) {
    const int i = t / H1C, j = t - i * H1C;
    smem[t] = j < H1 ? W1[i * H1 + j] : 0.f;
  }
  for (int t = threadIdx.x; t < H1C; t += blockDim.x) {
    smem[L.o_b1 + t] = t < H1 ? b1[t] : 0.f;
    smem[L.o_al1 + t] = (t < H1 && al1 != nullptr) ? al1[t] : 0.f;
  }
  for (int t = threadIdx.x; t < H1C * H2T; t += blockDim.x) {
    const int j = t / H2T, m = t - j * H2T;
    smem[L.o_W2 + t] = (j < H1 && m < H2) ? W2[j * H2 + m] : 0.f;
  }
  for (int t = threadIdx.x; t < H2T; t += blockDim.x) {
    smem[L.o_b2 + t] = t < H2 ? b2[t] : 0.f;
    smem[L.o_al2 + t] = (t < H2 && al2 != nullptr) ? al2[t] : 0.f;
    smem[L.o_w3 + t] = t < H2 ? w3[t] : 0.f;
  }
  if (threadIdx.x < 4) smem[L.o_b3 + threadIdx.x] = threadIdx.x == 0 ? b3[0] : 0.f;
}

// 64 slots of one sample's keys, from slot c0 on -> LDS rows at stride KP; a masked slot and a slot past T give a zero row (a masked
// key is never read)
__device__ __forceinline__ void din_load_keys(float* kS, const float* __restrict__ keys_b, const unsigned char* __restrict__ mask_b,
                                              const DinLayout& L, int c0, int lane) {
  const int KQ = L.KQ, n = 64 * KQ;
  for (int idx = lane; idx < n; idx += 64) {
    const int r = idx / KQ, kq = idx - r * KQ, t = c0 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < L.T && (mask_b == nullptr || mask_b[t] != 0)) v = *reinterpret_cast<const float4*>(keys_b + (long)t * L.K + kq * 4);
    *reinterpret_cast<float4*>(kS + r * L.KP + kq * 4) = v;
  }
}

// The score of the slot whose key row is krow: layer 1 in chunks of kDinCH units (inputs in the order k quad, then q | k | q-k | q*k,
// then k), each chunk activated and added straight into the layer-2 pre-activations u2 (registers).  h2 = act(u2).  STORE: the
// chunk's pre-activations (PReLU) or activations (sigmoid) -> u1row.  The padded units hold zero weights and add +0.
template <int H2T, bool SIG, bool STORE>
__device__ __forceinline__ float din_score(const float* S, const DinLayout& L, const float* qS, const float* krow, float* u1row,
                                           float (&u2)[H2T], float (&h2)[H2T]) {
  const int K = L.K, H1C = L.H1C;
#pragma unroll
  for (int m = 0; m < H2T; m += 4) {
    const float4 b = *reinterpret_cast<const float4*>(S + L.o_b2 + m);
    u2[m] = b.x; u2[m + 1] = b.y; u2[m + 2] = b.z; u2[m + 3] = b.w;
  }
  for (int c = 0; c < H1C; c += kDinCH) {
    float u[kDinCH];
#pragma unroll
    for (int jj = 0; jj < kDinCH; ++jj) u[jj] = S[L.o_b1 + c + jj];
    for (int kq = 0; kq < L.KQ; ++kq) {
      const float4 qv = *reinterpret_cast<const float4*>(qS + kq * 4);
      const float4 kv = *reinterpret_cast<const float4*>(krow + kq * 4);
      const float x[16] = {qv.x, qv.y, qv.z, qv.w, kv.x, kv.y, kv.z, kv.w, qv.x - kv.x, qv.y - kv.y, qv.z - kv.z, qv.w - kv.w,
                           qv.x * kv.x, qv.y * kv.y, qv.z * kv.z, qv.w * kv.w};
#pragma unroll
      for (int sg = 0; sg < 4; ++sg) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float* w = S + (sg * K + kq * 4 + e) * H1C + c;
          const float4 w0 = *reinterpret_cast<const float4*>(w);
          const float4 w1 = *reinterpret_cast<const float4*>(w + 4);
          const float xv = x[sg * 4 + e];
          u[0] = fmaf(xv, w0.x, u[0]); u[1] = fmaf(xv, w0.y, u[1]); u[2] = fmaf(xv, w0.z, u[2]); u[3] = fmaf(xv, w0.w, u[3]);
          u[4] = fmaf(xv, w1.x, u[4]); u[5] = fmaf(xv, w1.y, u[5]); u[6] = fmaf(xv, w1.z, u[6]); u[7] = fmaf(xv, w1.w, u[7]);
        }
      }
    }
    float h[kDinCH];
#pragma unroll
    for (int jj = 0; jj < kDinCH; ++jj) h[jj] = din_act<SIG>(u[jj], S[L.o_al1 + c + jj]);
    if constexpr (STORE) {
      if constexpr (SIG) {
        *reinterpret_cast<float4*>(u1row + c) = make_float4(h[0], h[1], h[2], h[3]);
        *reinterpret_cast<float4*>(u1row + c + 4) = make_float4(h[4], h[5], h[6], h[7]);
      } else {
        *reinterpret_cast<float4*>(u1row + c) = make_float4(u[0], u[1], u[2], u[3]);
        *reinterpret_cast<float4*>(u1row + c + 4) = make_float4(u[4], u[5], u[6], u[7]);
      }
    }
#pragma unroll
    for (int jj = 0; jj < kDinCH; ++jj) {
      const float* w2 = S + L.o_W2 + (c + jj) * H2T;
#pragma unroll
      for (int m = 0; m < H2T; m += 4) {
        const float4 w = *reinterpret_cast<const float4*>(w2 + m);
        u2[m] = fmaf(h[jj], w.x, u2[m]);
        u2[m + 1] = fmaf(h[jj], w.y, u2[m + 1]);
        u2[m + 2] = fmaf(h[jj], w.z, u2[m + 2]);
        u2[m + 3] = fmaf(h[jj], w.w, u2[m + 3]);
      }
    }
  }
  float s = 0.f;
#pragma unroll
  for (int m = 0; m < H2T; ++m) {
    h2[m] = din_act<SIG>(u2[m], S[L.o_al2 + m]);
    s = fmaf(h2[m], S[L.o_w3 + m], s);
  }
  return s + S[L.o_b3];
}

template <int H2T, bool SIG>
__global__ __launch_bounds__(64 * kDinMaxSamples) void din_fwd_kernel(const float* __restrict__ q, const float* __restrict__ keys,
                                                                     const unsigned char* __restrict__ mask, const float* __restrict__ W1,
                                                                     const float* __restrict__ b1, const float* __restrict__ al1,
                                                                     const float* __restrict__ W2, const float* __restrict__ b2,
                                                                     const float* __restrict__ al2, const float* __restrict__ w3,
                                                                     const float* __restrict__ b3, float* __restrict__ out,
                                                                     float* __restrict__ stats, int B, int flags, DinLayout L) {
  extern __shared__ __attribute__((aligned(16))) float din_smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  din_stage_params(din_smem, L, W1, b1, al1, W2, b2, al2, w3, b3);
  __syncthreads();
  const float* S = din_smem;
  float* kS = din_smem + L.shared_f + wave * L.samp_fwd;
  float* qS = kS + L.o_q;
  float* scS = kS + L.o_sc;
  float* partS = kS + L.o_part;
  const bool softmax = (flags & 1) != 0;
  const int T = L.T, K = L.K, KQ = L.KQ, NG = 64 / KQ;
  const int kq = lane % KQ, pg = lane / KQ;
  for (long b = (long)blockIdx.x * L.NS + wave; b < B; b += (long)gridDim.x * L.NS) {
    const float* keys_b = keys + b * T * K;
    const unsigned char* mask_b = mask != nullptr ? mask + b * T : nullptr;
    if (lane < K) qS[lane] = q[b * K + lane];
    // pass 1: the scores of the live slots
    float mx = -INFINITY;
    for (int c0 = 0; c0 < T; c0 += 64) {
      din_load_keys(kS, keys_b, mask_b, L, c0, lane);
      wave_lds_sync();
      const int t = c0 + lane;
      float u2[H2T], h2[H2T];
      const float s = din_score<H2T, SIG, false>(S, L, qS, kS + lane * L.KP, nullptr, u2, h2);
      if (t < T) {
        const bool live = mask_b == nullptr || mask_b[t] != 0;
        scS[t] = live ? s : (softmax ? -INFINITY : 0.f);
        stats[b * (T + 2) + t] = live ? s : 0.f;
        if (live) mx = fmaxf(mx, s);
      }
      wave_lds_sync();    // (the next 64 slots overwrite the key rows)
    }
    float den = 1.f;
    if (softmax) {
      mx = wave_max(mx);
      den = 0.f;
      for (int t = lane; t < T; t += 64) {
        const float sc = scS[t];
        const float w = sc == -INFINITY ? 0.f : expf(sc - mx);
        scS[t] = w;
        den += w;
      }
      den = wave_sum(den);
      wave_lds_sync();
    }
    // pass 2: sum_t w_t k_t, lane = (4 consecutive k, slot group)
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < T; c0 += 64) {
      if (T > 64) {       // (one trip: the rows of pass 1 are still there)
        din_load_keys(kS, keys_b, mask_b, L, c0, lane);
        wave_lds_sync();
      }
      const int cnt = min(64, T - c0);
      if (pg < NG) {
#pragma unroll 4
        for (int r = pg; r < cnt; r += NG) {
          const float4 kv = *reinterpret_cast<const float4*>(kS + r * L.KP + kq * 4);
          const float w = scS[c0 + r];
          acc[0] = fmaf(w, kv.x, acc[0]);
          acc[1] = fmaf(w, kv.y, acc[1]);
          acc[2] = fmaf(w, kv.z, acc[2]);
          acc[3] = fmaf(w, kv.w, acc[3]);
        }
      }
      wave_lds_sync();
    }
    if (pg < NG) *reinterpret_cast<float4*>(partS + pg * K + kq * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    wave_lds_sync();
    if (lane < K) {
      float t = 0.f;
      for (int gq = 0; gq < NG; ++gq) t += partS[gq * K + lane];
      out[b * K + lane] = softmax ? (den > 0.f ? t / den : 0.f) : t;
    }
    if (lane == 0) {
      stats[b * (T + 2) + T] = (softmax && den > 0.f) ? mx : 0.f;      // (raw mode, or no live slot: the backward does not use it)
      stats[b * (T + 2) + T + 1] = den;
    }
    wave_lds_sync();    // the next sample overwrites this image
  }
}

// one thread's 4 x 16 tile of dW1 (rows i0 .. i0+3 of one input segment, columns j0 .. j0+15) += x^T du1 over the staged slots
__device__ __forceinline__ void din_tile_w1(float (&acc)[64], int id, const float* smem, const DinLayout& L, int nvalid, int cnt) {
  const int r = id / L.n_c1, c = id - r * L.n_c1;
  const int i0 = 4 * r, sg = i0 / L.K, kk = i0 - sg * L.K, j0 = 16 * c;
  for (int s = 0; s < nvalid; ++s) {
    const float* base = smem + L.shared_f + s * L.samp_bwd;
    const float4 qv = *reinterpret_cast<const float4*>(base + L.o_q + kk);
    for (int rr = 0; rr < cnt; ++rr) {
      const float4 kv = *reinterpret_cast<const float4*>(base + rr * L.KP + kk);
      float x[4];
      if (sg == 0) { x[0] = qv.x; x[1] = qv.y; x[2] = qv.z; x[3] = qv.w; }
      else if (sg == 1) { x[0] = kv.x; x[1] = kv.y; x[2] = kv.z; x[3] = kv.w; }
      else if (sg == 2) { x[0] = qv.x - kv.x; x[1] = qv.y - kv.y; x[2] = qv.z - kv.z; x[3] = qv.w - kv.w; }
      else { x[0] = qv.x * kv.x; x[1] = qv.y * kv.y; x[2] = qv.z * kv.z; x[3] = qv.w * kv.w; }
      const float* d = base + L.o_u1 + rr * L.H1P + j0;
#pragma unroll
      for (int bq = 0; bq < 4; ++bq) {
        const float4 dv = *reinterpret_cast<const float4*>(d + bq * 4);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          acc[a * 16 + bq * 4] = fmaf(x[a], dv.x, acc[a * 16 + bq * 4]);
          acc[a * 16 + bq * 4 + 1] = fmaf(x[a], dv.y, acc[a * 16 + bq * 4 + 1]);
          acc[a * 16 + bq * 4 + 2] = fmaf(x[a], dv.z, acc[a * 16 + bq * 4 + 2]);
          acc[a * 16 + bq * 4 + 3] = fmaf(x[a], dv.w, acc[a * 16 + bq * 4 + 3]);
        }
      }
    }
  }
}

// one thread's 4 x 16 tile of dW2 (units j0 .. j0+3, columns m0 .. m0+15) += h1^T du2 over the staged slots
template <bool SIG>
__device__ __forceinline__ void din_tile_w2(float (&acc)[64], int id2, const float* smem, const DinLayout& L, int nvalid, int cnt) {
  const int r = id2 / L.n_c2, c = id2 - r * L.n_c2;
  const int j0 = 4 * r, m0 = 16 * c;
  const float4 al = *reinterpret_cast<const float4*>(smem + L.o_al1 + j0);
  for (int s = 0; s < nvalid; ++s) {
    const float* base = smem + L.shared_f + s * L.samp_bwd;
    for (int rr = 0; rr < cnt; ++rr) {
      const float4 uv = *reinterpret_cast<const float4*>(base + L.o_u1 + rr * L.H1P + j0);
      float h[4] = {uv.x, uv.y, uv.z, uv.w};
      if constexpr (!SIG) {
        h[0] = din_act<false>(uv.x, al.x); h[1] = din_act<false>(uv.y, al.y); h[2] = din_act<false>(uv.z, al.z); h[3] = din_act<false>(uv.w, al.w);
      }
      const float* d = base + L.o_du2 + rr * L.H2P + m0;
#pragma unroll
      for (int bq = 0; bq < 4; ++bq) {
        const float4 dv = *reinterpret_cast<const float4*>(d + bq * 4);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          acc[a * 16 + bq * 4] = fmaf(h[a], dv.x, acc[a * 16 + bq * 4]);
          acc[a * 16 + bq * 4 + 1] = fmaf(h[a], dv.y, acc[a * 16 + bq * 4 + 1]);
          acc[a * 16 + bq * 4 + 2] = fmaf(h[a], dv.z, acc[a * 16 + bq * 4 + 2]);
          acc[a * 16 + bq * 4 + 3] = fmaf(h[a], dv.w, acc[a * 16 + bq * 4 + 3]);
        }
      }
    }
  }
}

// a finished tile -> the workgroup's partial
__device__ __forceinline__ void din_tile_out(const float (&acc)[64], int id, float* part, const DinLayout& L) {
  if (id < L.n_t1) {
    const int r = id / L.n_c1, c = id - r * L.n_c1;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int bb = 0; bb < 16; ++bb)
        if (16 * c + bb < L.H1) part[(4 * r + a) * L.H1 + 16 * c + bb] = acc[a * 16 + bb];
  } else if (id < L.n_t1 + L.n_t2) {
    const int id2 = id - L.n_t1, r = id2 / L.n_c2, c = id2 - r * L.n_c2;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int bb = 0; bb < 16; ++bb)
        if (4 * r + a < L.H1 && 16 * c + bb < L.H2) part[L.p_W2 + (4 * r + a) * L.H2 + 16 * c + bb] = acc[a * 16 + bb];
  }
}

// NT: 4 x 16 tiles of dW1 / dW2 per thread (1 where all of them fit 256 threads, else 2)
template <int H2T, bool SIG, int NT>
__global__ __launch_bounds__(kDinBwdThreads) void din_bwd_kernel(const float* __restrict__ q, const float* __restrict__ keys,
                                                                const unsigned char* __restrict__ mask, const float* __restrict__ W1,
                                                                const float* __restrict__ b1, const float* __restrict__ al1,
                                                                const float* __restrict__ W2, const float* __restrict__ b2,
                                                                const float* __restrict__ al2, const float* __restrict__ w3,
                                                                const float* __restrict__ b3, const float* __restrict__ out,
                                                                const float* __restrict__ stats, const float* __restrict__ g,
                                                                float* __restrict__ dq, float* __restrict__ dkeys,
                                                                float* __restrict__ partials, int B, int flags, DinLayout L) {
  extern __shared__ __attribute__((aligned(16))) float din_smem[];
  constexpr int N2 = H2T <= 16 ? 16 : (H2T <= 32 ? 32 : 64);
  constexpr int SH2 = N2 == 64 ? 0 : (N2 == 32 ? 1 : 2);       // the butterfly leaves unit m in the lanes m << SH2 ...
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  din_stage_params(din_smem, L, W1, b1, al1, W2, b2, al2, w3, b3);
  const bool owner = wave < L.NS;          // this wave owns a sample of every tile
  float* kS = din_smem + L.shared_f + (owner ? wave : 0) * L.samp_bwd;
  float* qS = kS + L.o_q;
  float* gS = kS + L.o_g;
  float* dqS = kS + L.o_dq;
  float* aS = kS + L.o_a;
  float* dal1S = kS + L.o_dal1;
  float* u1S = kS + L.o_u1;
  float* du2S = kS + L.o_du2;
  if (owner)
    for (int j = lane; j < L.H1C; j += 64) dal1S[j] = 0.f;
  __syncthreads();
  const float* S = din_smem;
  const bool softmax = (flags & 1) != 0;
  const bool want_params = partials != nullptr;
  const int T = L.T, K = L.K, KQ = L.KQ, H1C = L.H1C;
  const int n_tiles = L.n_t1 + L.n_t2;
  float acc[NT][64];
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int i = 0; i < 64; ++i) acc[n][i] = 0.f;
  float db1 = 0.f, db2 = 0.f, dw3 = 0.f, dal2 = 0.f, db3 = 0.f;
  const long n_samp_tiles = ((long)B + L.NS - 1) / L.NS;
  for (long tile = blockIdx.x; tile < n_samp_tiles; tile += gridDim.x) {
    const long b = tile * L.NS + wave;
    const bool have = owner && b < B;
    const long left = (long)B - tile * L.NS;
    const int nvalid = left < L.NS ? (int)left : L.NS;
    const float* keys_b = keys + (have ? b : 0) * T * K;
    const unsigned char* mask_b = (mask != nullptr && have) ? mask + b * T : nullptr;
    float mx = 0.f, den = 1.f, gp = 0.f, gc = 0.f;
    if (have) {
      if (lane < K) {
        qS[lane] = q[b * K + lane];
        gS[lane] = g[b * K + lane];
        dqS[lane] = 0.f;
      }
      mx = stats[b * (T + 2) + T];
      den = stats[b * (T + 2) + T + 1];
      wave_lds_sync();
      if (softmax) {
        // g . out as sum_t a_t (g . k_t) over the very a_t and g . k_t that ds_t = a_t (g . k_t - g . out) is made of (a_t from the
        // saved scores): the sum of ds over a sample then cancels to rounding, and with one live slot (a = 1) g . out IS that
        // slot's g . k and ds is exactly 0.  Where the slot with the largest score (the first one whose saved score is mx) holds
        // more than half of the weight (its weight is 1 / den), every g . k_t is taken relative to gc = its g . k (same chain, same
        // bits, so its own difference is exactly 0): with a weight of 1 - eps, g . k - g . out of that slot is eps-small, and formed
        // from the absolute values it carries their rounding, 2^-24 |g . k|, against a true value of eps |g . k| -- a relative
        // error of 2^-24 / eps in ds of every slot of the sample.  At or below one half nothing is lost and gc stays 0 (x - 0 = x).
        if (den < 2.f) {
          int tm = T;
          for (int t = lane; t < T; t += 64)
            if ((mask_b == nullptr || mask_b[t] != 0) && stats[b * (T + 2) + t] == mx) tm = min(tm, t);
#pragma unroll
          for (int o = 32; o >= 1; o >>= 1) tm = min(tm, __shfl_xor(tm, o));
          if (tm < T) gc = din_dot(gS, keys_b + (long)tm * K, KQ);
        }
        float part = 0.f;
        for (int c0 = 0; c0 < T; c0 += 64) {
          din_load_keys(kS, keys_b, mask_b, L, c0, lane);
          wave_lds_sync();
          const int t = c0 + lane;
          const bool live = t < T && (mask_b == nullptr || mask_b[t] != 0);
          const float a = live ? expf(stats[b * (T + 2) + t] - mx) / den : 0.f;
          part = fmaf(a, din_dot(gS, kS + lane * L.KP, KQ) - gc, part);
          wave_lds_sync();
        }
        gp = wave_sum(part);
      }
    }
    for (int c0 = 0; c0 < T; c0 += 64) {
      const int cnt = min(64, T - c0);
      const int t = c0 + lane;
      float* u1row = u1S + lane * L.H1P;
      const float* krow = kS + lane * L.KP;
      float a_t = 0.f;
      bool live = false;
      if (have) {
        // phase A
        din_load_keys(kS, keys_b, mask_b, L, c0, lane);
        wave_lds_sync();
        live = t < T && (mask_b == nullptr || mask_b[t] != 0);
        float u2[H2T], h2[H2T];
        const float s = din_score<H2T, SIG, true>(S, L, qS, krow, u1row, u2, h2);
        const float gk = din_dot(gS, krow, KQ);
        float ds;
        if (softmax) {
          a_t = live ? expf(stats[b * (T + 2) + t] - mx) / den : 0.f;      // (the saved score: the bits of s)
          ds = a_t * ((gk - gc) - gp);
        } else {
          a_t = live ? s : 0.f;
          ds = live ? gk : 0.f;
        }
        aS[lane] = a_t;
        // du2 = ds w3 act'(u2); h2 again from u2 (PReLU) so that only one of the two arrays stays live
        auto du2_of = [&](int m) {
          const float dh = ds * S[L.o_w3 + m];
          if constexpr (SIG) return dh * (h2[m] * (1.f - h2[m]));
          else return u2[m] > 0.f ? dh : dh * S[L.o_al2 + m];
        };
#pragma unroll
        for (int m = 0; m < H2T; m += 4)
          *reinterpret_cast<float4*>(du2S + lane * L.H2P + m) = make_float4(du2_of(m), du2_of(m + 1), du2_of(m + 2), du2_of(m + 3));
        if (want_params) {
          float tr[N2];
#pragma unroll
          for (int m = 0; m < N2; ++m) {
            if constexpr (SIG) tr[m] = m < H2T ? ds * h2[m < H2T ? m : 0] : 0.f;
            else tr[m] = m < H2T ? ds * din_act<false>(u2[m < H2T ? m : 0], S[L.o_al2 + (m < H2T ? m : 0)]) : 0.f;
          }
          dw3 += din_lane_reduce<N2>(tr, lane);
#pragma unroll
          for (int m = 0; m < N2; ++m) tr[m] = m < H2T ? du2_of(m < H2T ? m : 0) : 0.f;
          db2 += din_lane_reduce<N2>(tr, lane);
          if constexpr (!SIG) {
#pragma unroll
            for (int m = 0; m < N2; ++m) {
              const int mm = m < H2T ? m : 0;
              tr[m] = (m < H2T && !(u2[mm] > 0.f)) ? (ds * S[L.o_w3 + mm]) * u2[mm] : 0.f;
            }
            dal2 += din_lane_reduce<N2>(tr, lane);
          }
          db3 += wave_sum(ds);
        }
      }
      if (want_params) {
        __syncthreads();
        // P2: dW2 tiles
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          const int id = tid + n * kDinBwdThreads;
          if (id >= L.n_t1 && id < n_tiles) din_tile_w2<SIG>(acc[n], id - L.n_t1, din_smem, L, nvalid, cnt);
        }
        __syncthreads();
      }
      if (have) {
        // phase B: du1 = (du2 W2^T) act'(u1), in place over the staged row
        float du2[H2T];
#pragma unroll
        for (int m = 0; m < H2T; m += 4) {
          const float4 v = *reinterpret_cast<const float4*>(du2S + lane * L.H2P + m);
          du2[m] = v.x; du2[m + 1] = v.y; du2[m + 2] = v.z; du2[m + 3] = v.w;
        }
        for (int c = 0; c < H1C; c += kDinCH) {
          float dh[kDinCH];
#pragma unroll
          for (int jj = 0; jj < kDinCH; ++jj) {
            const float* w2 = S + L.o_W2 + (c + jj) * H2T;
            float acc = 0.f;
#pragma unroll
            for (int m = 0; m < H2T; m += 4) {
              const float4 w = *reinterpret_cast<const float4*>(w2 + m);
              acc = fmaf(du2[m], w.x, acc);
              acc = fmaf(du2[m + 1], w.y, acc);
              acc = fmaf(du2[m + 2], w.z, acc);
              acc = fmaf(du2[m + 3], w.w, acc);
            }
            dh[jj] = acc;
          }
          const float4 ua = *reinterpret_cast<const float4*>(u1row + c);
          const float4 ub = *reinterpret_cast<const float4*>(u1row + c + 4);
          const float uv[kDinCH] = {ua.x, ua.y, ua.z, ua.w, ub.x, ub.y, ub.z, ub.w};
          float d[kDinCH], tal[kDinCH];
#pragma unroll
          for (int jj = 0; jj < kDinCH; ++jj) {
            if constexpr (SIG) {
              d[jj] = dh[jj] * (uv[jj] * (1.f - uv[jj]));
              tal[jj] = 0.f;
            } else {
              d[jj] = uv[jj] > 0.f ? dh[jj] : dh[jj] * S[L.o_al1 + c + jj];
              tal[jj] = uv[jj] > 0.f ? 0.f : dh[jj] * uv[jj];
            }
          }
          *reinterpret_cast<float4*>(u1row + c) = make_float4(d[0], d[1], d[2], d[3]);
          *reinterpret_cast<float4*>(u1row + c + 4) = make_float4(d[4], d[5], d[6], d[7]);
          if constexpr (!SIG) {
            if (want_params) {
              const float r = din_lane_reduce<kDinCH>(tal, lane);      // unit c + (lane >> 3)
              if ((lane & 7) == 0) dal1S[c + (lane >> 3)] += r;
            }
          }
        }
        wave_lds_sync();
        // phase C: dx = du1 W1^T, the 16 inputs of a k quad at a time; dkeys row, dq terms
        for (int kq = 0; kq < KQ; ++kq) {
          float dx[16];
#pragma unroll
          for (int i = 0; i < 16; ++i) dx[i] = 0.f;
          for (int jq = 0; jq < H1C; jq += 4) {
            const float4 dv = *reinterpret_cast<const float4*>(u1row + jq);
#pragma unroll
            for (int sg = 0; sg < 4; ++sg) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float4 w = *reinterpret_cast<const float4*>(S + (sg * K + kq * 4 + e) * H1C + jq);
                float v = dx[sg * 4 + e];
                v = fmaf(dv.x, w.x, v);
                v = fmaf(dv.y, w.y, v);
                v = fmaf(dv.z, w.z, v);
                v = fmaf(dv.w, w.w, v);
                dx[sg * 4 + e] = v;
              }
            }
          }
          const float4 qv = *reinterpret_cast<const float4*>(qS + kq * 4);
          const float4 kv = *reinterpret_cast<const float4*>(krow + kq * 4);
          const float4 gv = *reinterpret_cast<const float4*>(gS + kq * 4);
          const float qa[4] = {qv.x, qv.y, qv.z, qv.w}, ka[4] = {kv.x, kv.y, kv.z, kv.w}, ga[4] = {gv.x, gv.y, gv.z, gv.w};
          float dk[4], dqt[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            dk[e] = fmaf(a_t, ga[e], fmaf(qa[e], dx[12 + e], dx[4 + e] - dx[8 + e]));
            dqt[e] = fmaf(ka[e], dx[12 + e], dx[e] + dx[8 + e]);
          }
          if (dkeys != nullptr && t < T) {
            const float4 o = live ? make_float4(dk[0], dk[1], dk[2], dk[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(dkeys + ((long)b * T + t) * K + kq * 4) = o;
          }
          if (dq != nullptr) {
            const float r = din_lane_reduce<4>(dqt, lane);             // element lane >> 4
            if ((lane & 15) == 0) dqS[kq * 4 + (lane >> 4)] += r;
          }
        }
      }
      if (want_params) {
        __syncthreads();
        // P1: dW1 tiles, db1 by column
#pragma unroll
        for (int n = 0; n < NT; ++n)
          if (tid + n * kDinBwdThreads < L.n_t1) din_tile_w1(acc[n], tid + n * kDinBwdThreads, din_smem, L, nvalid, cnt);
        if (tid < L.H1)
          for (int s = 0; s < nvalid; ++s) {
            const float* col = din_smem + L.shared_f + s * L.samp_bwd + L.o_u1 + tid;
            for (int rr = 0; rr < cnt; ++rr) db1 += col[rr * L.H1P];
          }
        __syncthreads();    // the next 64 slots overwrite the staged rows
      } else if (have) {
        wave_lds_sync();
      }
    }
    if (have && dq != nullptr) {
      wave_lds_sync();
      if (lane < K) dq[b * K + lane] = dqS[lane];
      wave_lds_sync();
    }
  }
  if (!want_params) return;
  // the workgroup's partial: tiles and db1 as they stand; the sample waves' lane-held sums in wave order
  float* part = partials + (long)blockIdx.x * L.n_out;
#pragma unroll
  for (int n = 0; n < NT; ++n) din_tile_out(acc[n], tid + n * kDinBwdThreads, part, L);
  if (tid < L.H1) part[L.p_b1 + tid] = db1;
  float* red = din_smem + L.o_red;
  if (owner) {
    if ((lane & ((1 << SH2) - 1)) == 0) {
      const int m = lane >> SH2;
      red[wave * kDinRedWave + m] = db2;
      red[wave * kDinRedWave + 64 + m] = dw3;
      red[wave * kDinRedWave + 128 + m] = dal2;
    }
    if (lane == 0) red[wave * kDinRedWave + 192] = db3;
  }
  __syncthreads();
  for (int o = tid; o < L.H1 + 3 * L.H2 + 1; o += blockDim.x) {
    // o: alpha1 [H1] | b2 [H2] | alpha2 [H2] | w3 [H2] | b3
    float t = 0.f;
    int dst;
    if (o < L.H1) {
      for (int s = 0; s < L.NS; ++s) t += din_smem[L.shared_f + s * L.samp_bwd + L.o_dal1 + o];
      dst = L.p_al1 + o;
    } else {
      const int r = o - L.H1;
      const int which = r < L.H2 ? 0 : (r < 2 * L.H2 ? 2 : (r < 3 * L.H2 ? 1 : 3));    // red slots: db2 0, dw3 1, dalpha2 2, db3 3
      const int m = which == 3 ? 0 : r - (which == 0 ? 0 : (which == 2 ? L.H2 : 2 * L.H2));
      for (int s = 0; s < L.NS; ++s) t += red[s * kDinRedWave + which * 64 + m];
      dst = which == 0 ? L.p_b2 + m : (which == 2 ? L.p_al2 + m : (which == 1 ? L.p_w3 + m : L.p_b3));
    }
    part[dst] = t;
  }
}

// argument and menu checks shared by the four entry points
static int din_dims(const char* who, int B, int T, int K, int H1, int H2, DinLayout* L) {
  FIL_CHECK_ARG_W(who, B >= 0 && T >= 1 && K >= 1 && H1 >= 1 && H2 >= 1);
  if (K % 4 != 0 || K > kDinMaxK) return fail(FIL_ERR_UNSUPPORTED, "%s: K=%d needs K %% 4 == 0 and K <= %d", who, K, kDinMaxK);
  if (T > kDinMaxT) return fail(FIL_ERR_UNSUPPORTED, "%s: T=%d > %d", who, T, kDinMaxT);
  if (H1 > kDinMaxH1) return fail(FIL_ERR_UNSUPPORTED, "%s: H1=%d > %d", who, H1, kDinMaxH1);
  if (H2 > kDinMaxH2) return fail(FIL_ERR_UNSUPPORTED, "%s: H2=%d > %d", who, H2, kDinMaxH2);
  if (4 * K * H1 + H1 * H2 > kDinMaxParams)
    return fail(FIL_ERR_UNSUPPORTED, "%s: 4 K H1 + H1 H2 = %d > %d (K=%d H1=%d H2=%d)", who, 4 * K * H1 + H1 * H2, kDinMaxParams, K, H1, H2);
  *L = din_pick(T, K, H1, H2);
  if (L->NS == 0)
    return fail(FIL_ERR_UNSUPPORTED, "%s: T=%d K=%d H1=%d H2=%d needs %d bytes of LDS (limit %d)", who, T, K, H1, H2,
                std::max(L->lds_fwd, L->lds_bwd), kTiledLdsLimit);
  return FIL_OK;
}

struct DinFwdArgs {
  const float *q, *keys;
  const unsigned char* mask;
  const float *W1, *b1, *al1, *W2, *b2, *al2, *w3, *b3;
  float *out, *stats;
};

template <int H2T, bool SIG>
static int din_launch_fwd(const char* who, const DinFwdArgs& a, int B, int flags, const DinLayout& L, hipStream_t st) {
  if (int rc = tiled_allow_lds(who, din_fwd_kernel<H2T, SIG>, L.lds_fwd)) return rc;
  hipLaunchKernelGGL((din_fwd_kernel<H2T, SIG>), dim3(din_grid(B, L.NS)), dim3(64 * L.NS), L.lds_fwd, st, a.q, a.keys, a.mask, a.W1, a.b1,
                     a.al1, a.W2, a.b2, a.al2, a.w3, a.b3, a.out, a.stats, B, flags, L);
  return FIL_OK;
}

struct DinBwdArgs {
  const float *q, *keys;
  const unsigned char* mask;
  const float *W1, *b1, *al1, *W2, *b2, *al2, *w3, *b3, *out, *stats, *g;
  float *dq, *dkeys, *partials;
};

template <int H2T, bool SIG, int NT>
static int din_launch_bwd_nt(const char* who, const DinBwdArgs& a, int B, int flags, const DinLayout& L, hipStream_t st) {
  if (int rc = tiled_allow_lds(who, din_bwd_kernel<H2T, SIG, NT>, L.lds_bwd)) return rc;
  hipLaunchKernelGGL((din_bwd_kernel<H2T, SIG, NT>), dim3(din_grid(B, L.NS)), dim3(kDinBwdThreads), L.lds_bwd, st, a.q, a.keys, a.mask, a.W1,
                     a.b1, a.al1, a.W2, a.b2, a.al2, a.w3, a.b3, a.out, a.stats, a.g, a.dq, a.dkeys, a.partials, B, flags, L);
  return FIL_OK;
}

template <int H2T, bool SIG>
static int din_launch_bwd(const char* who, const DinBwdArgs& a, int B, int flags, const DinLayout& L, hipStream_t st) {
  if (L.n_t1 + L.n_t2 <= kDinBwdThreads) return din_launch_bwd_nt<H2T, SIG, 1>(who, a, B, flags, L, st);
  return din_launch_bwd_nt<H2T, SIG, 2>(who, a, B, flags, L, st);
}

#define DIN_DISPATCH(fn, ...)                                                          \
  (sig ? (L.H2T == 16   ? fn<16, true>(__VA_ARGS__)                                    \
          : L.H2T == 32 ? fn<32, true>(__VA_ARGS__)                                    \
          : L.H2T == 48 ? fn<48, true>(__VA_ARGS__)                                    \
                        : fn<64, true>(__VA_ARGS__))                                   \
       : (L.H2T == 16   ? fn<16, false>(__VA_ARGS__)                                   \
          : L.H2T == 32 ? fn<32, false>(__VA_ARGS__)                                   \
          : L.H2T == 48 ? fn<48, false>(__VA_ARGS__)                                   \
                        : fn<64, false>(__VA_ARGS__)))

}  // namespace fil

using namespace fil;

extern "C" int fil_din_plan(int B, int T, int K, int H1, int H2, int* plan) {
  DinLayout L;
  if (int rc = din_dims(__func__, B, T, K, H1, H2, &L)) return rc;
  FIL_CHECK_ARG(plan != nullptr);
  tiled_plan(plan, L.NS, din_grid(B, L.NS), kDinGridCap, L.lds_fwd, L.lds_bwd);
  return FIL_OK;
}

extern "C" int fil_din_fwd(const float* q, const float* keys, const unsigned char* mask, const float* W1, const float* b1,
                           const float* alpha1, const float* W2, const float* b2, const float* alpha2, const float* w3, const float* b3,
                           float* out, float* stats, int B, int T, int K, int H1, int H2, int flags, void* stream) {
  DinLayout L;
  if (int rc = din_dims(__func__, B, T, K, H1, H2, &L)) return rc;
  FIL_CHECK_ARG((flags & ~(FIL_DIN_SOFTMAX | FIL_DIN_SIGMOID)) == 0);
  if (B == 0) return FIL_OK;
  const bool sig = (flags & FIL_DIN_SIGMOID) != 0;
  FIL_CHECK_ARG(q != nullptr && keys != nullptr && W1 != nullptr && b1 != nullptr && W2 != nullptr && b2 != nullptr && w3 != nullptr &&
                b3 != nullptr && out != nullptr && stats != nullptr);
  FIL_CHECK_ARG(sig || (alpha1 != nullptr && alpha2 != nullptr));
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("din_fwd", st, 4.0 * ((double)B * ((double)T * K + 2.0 * K + 2) + 4.0 * K * H1 + (double)H1 * H2));
  const DinFwdArgs a = {q, keys, mask, W1, b1, alpha1, W2, b2, alpha2, w3, b3, out, stats};
  if (int rc = DIN_DISPATCH(din_launch_fwd, __func__, a, B, flags, L, st)) return rc;
  FIL_CHECK_LAUNCH();
  return FIL_OK;
}

extern "C" size_t fil_din_bwd_workspace_bytes(int B, int T, int K, int H1, int H2) {
  DinLayout L;
  if (din_dims(__func__, B, T, K, H1, H2, &L) != FIL_OK) return 0;
  return tiled_partial_bytes(din_grid(B, L.NS), L.n_out);
}

extern "C" int fil_din_bwd(const float* q, const float* keys, const unsigned char* mask, const float* W1, const float* b1,
                           const float* alpha1, const float* W2, const float* b2, const float* alpha2, const float* w3, const float* b3,
                           const float* out, const float* stats, const float* g, float* dq, float* dkeys, float* dW1, float* db1,
                           float* dalpha1, float* dW2, float* db2, float* dalpha2, float* dw3, float* db3, void* workspace,
                           size_t workspace_bytes, int B, int T, int K, int H1, int H2, int flags, void* stream) {
  DinLayout L;
  if (int rc = din_dims(__func__, B, T, K, H1, H2, &L)) return rc;
  FIL_CHECK_ARG((flags & ~(FIL_DIN_SOFTMAX | FIL_DIN_SIGMOID)) == 0);
  if (B == 0) return FIL_OK;
  const bool sig = (flags & FIL_DIN_SIGMOID) != 0;
  FIL_CHECK_ARG(q != nullptr && keys != nullptr && W1 != nullptr && b1 != nullptr && W2 != nullptr && b2 != nullptr && w3 != nullptr &&
                b3 != nullptr && out != nullptr && stats != nullptr && g != nullptr);
  FIL_CHECK_ARG(sig || (alpha1 != nullptr && alpha2 != nullptr));
  const bool want_params = dW1 != nullptr || db1 != nullptr || dalpha1 != nullptr || dW2 != nullptr || db2 != nullptr ||
                           dalpha2 != nullptr || dw3 != nullptr || db3 != nullptr;
  FIL_CHECK_ARG(dq != nullptr || dkeys != nullptr || want_params);
  const int nparts = din_grid(B, L.NS);
  if (want_params)
    if (int rc = tiled_check_workspace(__func__, workspace, workspace_bytes, nparts, L.n_out)) return rc;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("din_bwd", st, 4.0 * ((double)B * (2.0 * T * K + 4.0 * K + 2) + 2.0 * (4.0 * K * H1 + (double)H1 * H2)));
  const DinBwdArgs a = {q, keys, mask, W1, b1, alpha1, W2, b2, alpha2, w3, b3, out, stats, g, dq, dkeys,
                        want_params ? static_cast<float*>(workspace) : nullptr};
  if (int rc = DIN_DISPATCH(din_launch_bwd, __func__, a, B, flags, L, st)) return rc;
  FIL_CHECK_LAUNCH();
  if (want_params) {
    float* const outs[8] = {dW1, db1, dalpha1, dW2, db2, dalpha2, dw3, db3};
    const int off[9] = {0, L.p_b1, L.p_al1, L.p_W2, L.p_b2, L.p_al2, L.p_w3, L.p_b3, L.n_out};
    param_reduce_launch(static_cast<const float*>(workspace), nparts, outs, off, 8, st);
    FIL_CHECK_LAUNCH();
  }
  return FIL_OK;
}
