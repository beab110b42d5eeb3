// N5  Time-stream GRU over a behaviour sequence with event gaps for gfx950, forward and backward, fp32 (extension: the core of the
// Deep Time-Stream model -- a GRU whose state moves between two events, and from the last event to the prediction time, under a
// learned ODE dh/dt = tanh(h Wf + bf), integrated by S explicit Euler substeps).
//
//     delta = dt[b,t] / (float)S;   S times:  f = tanh(bf + h Wf);  h = fma(delta, f, h)      (every unit reads the OLD h)
//     then gru.hip's step in the mode FIL_GRU_GRU on the evolved h;  a masked step carries h, its x row and its dt are never read.
//     z = the last state evolved once more by S substeps of dt_out[b] / S (every sample, also one without a live step).
//
// Structure (both directions): rnn_tile.h's sample-quad tiling and schedule, with gru.hip's three gates and two bias rows; dt takes
// the places of the scores.  Behind rnn_tile.h's sections the op keeps
//   forward   Wf [H][H] | bf [H] | E [2][H][NSP], the substep images: substep s reads the state of all units from the image of the
//             substep before (the first from the step's hT) and writes E[s & 1]; the GRU step reads the last one.  One barrier per
//             substep on top of the step's one.
//   backward  WfT [H][H] | I [2] x (hsT [H][NSP] | qT [H][NSP] | qS [NS][H]): per substep, in reverse, the pre-substep state and
//             q = delta dh (1 - f^2) of the thread's unit and samples -> the image; (barrier); dh += q Wf^T, dWf += h_s^T q over the
//             tile's samples in sample order (NR more accumulators beside the GRU's NR x 3), dbf += q.  The images alternate, so a
//             substep costs one barrier.  h_s and f come from `saved` (the next substep's are in flight during this one's
//             arithmetic); the GRU's previous state is fma(delta, f, h) of the last substep's pair: no product, no tanhf again.
// `saved` per live step: the GRU's four planes (z, r, c, hp_h), then (h_s, f_s) per substep: [B,T,4+2S,H]; behind them the final
// evolution's (h_s, f_s): [B,2S,H].  Masked steps are left unwritten.
// No atomics; every sum has a fixed order for a given shape: repeats are bit-identical.
#include "common.h"
#include "param_reduce.h"
#include "rnn_tile.h"
#include <math.h>

namespace fil {

constexpr int kTsGates = 3, kTsBiasRows = 2, kTsMaxSteps = 8;

// what the op appends behind rnn_tile.h's sections (offsets in floats) and its sizes
struct TsLayout {
  int S, planes;               // substeps; planes of H per saved step: 4 + 2 S
  int f_Wf, f_bf, f_E, lds_fwd;
  int b_WfT, b_img, img, lds_bwd;
  int n_out;                   // one partial: rnn_tile.h's dW | dU | db, then dWf [H][H] | dbf [H]
};

static inline TsLayout ts_layout(const RnnLayout& L, int S) {
  TsLayout X;
  X.S = S; X.planes = 4 + 2 * S;
  X.f_Wf = L.lds_fwd / 4;
  X.f_bf = X.f_Wf + L.H * L.H;
  X.f_E = X.f_bf + L.H;
  X.lds_fwd = 4 * (X.f_E + 2 * L.H * L.NSP);
  X.b_WfT = L.lds_bwd / 4;
  X.b_img = X.b_WfT + L.H * L.H;
  X.img = 2 * L.H * L.NSP + L.NS * L.H;
  X.lds_bwd = 4 * (X.b_img + 2 * X.img);
  X.n_out = L.n_out + L.H * L.H + L.H;
  return X;
}

// live flag (1 / 0) and gap of sample b0 + threadIdx.x at step t (threads below NS); a masked step's gap is never read
__device__ __forceinline__ void ts_load_step(float& lv, float& dv, const float* __restrict__ dt, const unsigned char* __restrict__ mask, long b0,
                                             int B, int t, const RnnLayout& L) {
  lv = 0.f; dv = 0.f;
  if ((int)threadIdx.x < L.NS) {
    const long bb = b0 + threadIdx.x;
    if (bb < B && (mask == nullptr || mask[bb * L.T + t] != 0)) {
      lv = 1.f;
      dv = dt[bb * L.T + t];
    }
  }
}

// f [e] = tanhf(bf_j + sum_k in [k][sample e of the quad] Wf [k][j]), k ascending, the chain started from bf_j
__device__ __forceinline__ void ts_ode_f(float (&f)[4], const float* in, const float* Wfs, float bfj, int j, const RnnLayout& L) {
  float acc[4] = {bfj, bfj, bfj, bfj};
#pragma unroll 4
  for (int k = 0; k < L.H; ++k) {
    const float4 v = *reinterpret_cast<const float4*>(in + k * L.NSP);
    const float w = Wfs[k * L.H + j];
    acc[0] = fmaf(v.x, w, acc[0]); acc[1] = fmaf(v.y, w, acc[1]); acc[2] = fmaf(v.z, w, acc[2]); acc[3] = fmaf(v.w, w, acc[3]);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) f[e] = tanhf(acc[e]);
}

__global__ __launch_bounds__(kRnnThreads) void tsgru_fwd_kernel(const float* __restrict__ x, const float* __restrict__ dt,
                                                               const float* __restrict__ dt_out, const unsigned char* __restrict__ mask,
                                                               const float* __restrict__ W, const float* __restrict__ U,
                                                               const float* __restrict__ bias, const float* __restrict__ Wf,
                                                               const float* __restrict__ bf, float* __restrict__ hs, float* __restrict__ zout,
                                                               float* __restrict__ saved, int B, RnnLayout L, TsLayout X) {
  extern __shared__ __attribute__((aligned(16))) float ts_smem[];
  const int tid = threadIdx.x;
  const int T = L.T, K = L.K, H = L.H, H3 = L.HG, NS = L.NS, NSP = L.NSP, S = X.S, PL = X.planes;
  rnn_stage(ts_smem, W, K * H3);
  rnn_stage(ts_smem + L.f_U, U, H * H3);
  rnn_stage(ts_smem + L.f_b, bias, kTsBiasRows * H3);
  rnn_stage(ts_smem + X.f_Wf, Wf, H * H);
  rnn_stage(ts_smem + X.f_bf, bf, H);
  const float* Ws = ts_smem;
  const float* Us = ts_smem + L.f_U;
  const float* bs = ts_smem + L.f_b;
  const float* Wfs = ts_smem + X.f_Wf;
  float* E = ts_smem + X.f_E;
  const bool active = tid < L.G * H;
  const int g = tid / H, j = tid - g * H;
  const float fS = (float)S;
  const long n_tiles = ((long)B + NS - 1) / NS;
  float* savedF = saved != nullptr ? saved + (long)B * T * PL * H : nullptr;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long b0 = tile * NS;
    float h[4] = {0.f, 0.f, 0.f, 0.f};
    float4 xr[kRnnXV];
    float lvn, dvn;
    __syncthreads();      // the weights are staged; the previous tile's images are free
    rnn_load_x(xr, x, mask, b0, B, 0, L);
    ts_load_step(lvn, dvn, dt, mask, b0, B, 0, L);
    rnn_store_x(xr, ts_smem + L.f_x, L);
    if (tid < NS) { ts_smem[L.f_live + tid] = lvn; ts_smem[L.f_a + tid] = dvn; }
    if (active) *reinterpret_cast<float4*>(ts_smem + L.f_h + j * NSP + 4 * g) = make_float4(0.f, 0.f, 0.f, 0.f);
    if (T > 1) {
      rnn_load_x(xr, x, mask, b0, B, 1, L);
      ts_load_step(lvn, dvn, dt, mask, b0, B, 1, L);
    }
    __syncthreads();
    const float bfj = active ? ts_smem[X.f_bf + j] : 0.f;
    // S substeps on the state whose image is `src`; plane 0 of the pairs of sample e of the quad is sv0 + e * es (sv0 = nullptr:
    // nothing is saved).  Leaves the evolved state in h and in E[(S - 1) & 1]; ends in a barrier.
    auto evolve = [&](const float* src, const float (&delta)[4], const bool (&lv)[4], float* sv0, long es) {
      for (int s = 0; s < S; ++s) {
        float* dst = E + (s & 1) * H * NSP;
        if (active) {
          float f[4];
          ts_ode_f(f, src + 4 * g, Wfs, bfj, j, L);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (lv[e]) {
              if (sv0 != nullptr) {
                float* sv = sv0 + e * es + 2 * s * H;
                sv[0] = h[e]; sv[H] = f[e];
              }
              h[e] = fmaf(delta[e], f[e], h[e]);
            }
          }
          *reinterpret_cast<float4*>(dst + j * NSP + 4 * g) = make_float4(h[0], h[1], h[2], h[3]);
        }
        __syncthreads();
        src = dst;
      }
    };
    // the order within a step: rnn_tile.h, Schedule
    for (int t = 0; t < T; ++t) {
      const int cur = t & 1, nxt = cur ^ 1;
      float zv[4], rv[4], cv[4], pv[4];
      bool lv[4] = {false, false, false, false};
      float delta[4] = {0.f, 0.f, 0.f, 0.f};
      if (active) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int s = 4 * g + e;
          lv[e] = ts_smem[L.f_live + cur * NS + s] != 0.f;
          delta[e] = ts_smem[L.f_a + cur * NS + s] / fS;      // one correctly rounded division
        }
      }
      float* sv0 = nullptr;
      if (active && saved != nullptr) sv0 = saved + (((b0 + 4 * g) * T + t) * PL + 4) * H + j;
      evolve(ts_smem + L.f_h + cur * H * NSP, delta, lv, sv0, (long)T * PL * H);
      if (active) {
        float ax[3][4], ah[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float bx = bs[c * H + j], bh = bs[H3 + c * H + j];
#pragma unroll
          for (int e = 0; e < 4; ++e) { ax[c][e] = bx; ah[c][e] = bh; }
        }
        const float* xc = ts_smem + L.f_x + cur * K * NSP + 4 * g;
        const float* hc = E + ((S - 1) & 1) * H * NSP + 4 * g;
        rnn_fwd_products(ax, xc, Ws, K, j, L);
        rnn_fwd_products(ah, hc, Us, H, j, L);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float z = rnn_sigmoid(ax[0][e] + ah[0][e]);
          const float r = rnn_sigmoid(ax[1][e] + ah[1][e]);
          const float c = tanhf(ax[2][e] + r * ah[2][e]);
          const float u = 1.f - z;
          const float hn = fmaf(u, c, (1.f - u) * h[e]);
          if (lv[e]) h[e] = hn;
          zv[e] = z; rv[e] = r; cv[e] = c; pv[e] = ah[2][e];
        }
        *reinterpret_cast<float4*>(ts_smem + L.f_h + nxt * H * NSP + j * NSP + 4 * g) = make_float4(h[0], h[1], h[2], h[3]);
      }
      if (t + 1 < T) {
        rnn_store_x(xr, ts_smem + L.f_x + nxt * K * NSP, L);
        if (tid < NS) { ts_smem[L.f_live + nxt * NS + tid] = lvn; ts_smem[L.f_a + nxt * NS + tid] = dvn; }
      }
      if (active) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long bb = b0 + 4 * g + e;
          if (lv[e] && saved != nullptr) {
            float* sv = saved + ((bb * T + t) * PL) * H + j;
            sv[0] = zv[e]; sv[H] = rv[e]; sv[2 * H] = cv[e]; sv[3 * H] = pv[e];
          }
          if (bb < B) hs[(bb * T + t) * H + j] = h[e];
        }
      }
      if (t + 2 < T) {
        rnn_load_x(xr, x, mask, b0, B, t + 2, L);
        ts_load_step(lvn, dvn, dt, mask, b0, B, t + 2, L);
      }
      __syncthreads();
    }
    if (dt_out != nullptr) {
      // the last state of every sample of the batch, to the prediction time (the state's image is hT[T & 1])
      bool lv[4] = {false, false, false, false};
      float delta[4] = {0.f, 0.f, 0.f, 0.f};
      if (active) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long bb = b0 + 4 * g + e;
          lv[e] = bb < B;
          if (lv[e]) delta[e] = dt_out[bb] / fS;
        }
      }
      float* sv0 = nullptr;
      if (active && savedF != nullptr) sv0 = savedF + ((b0 + 4 * g) * 2 * S) * H + j;
      evolve(ts_smem + L.f_h + (T & 1) * H * NSP, delta, lv, sv0, (long)2 * S * H);
      if (active) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long bb = b0 + 4 * g + e;
          if (bb < B) zout[bb * H + j] = h[e];
        }
      }
    }
  }
}

// dWf: the thread's column j of the rows g, g + G, ... of h_s^T q, summed over the tile's samples in sample order
template <int NR>
__device__ __forceinline__ void ts_bwd_accumulate(float (&acc)[NR], const float* hsT, const float* qS, int g, int j, const RnnLayout& L) {
  const int H = L.H;
  for (int s4 = 0; s4 < L.NS; s4 += 4) {
    float qe[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) qe[e] = qS[(s4 + e) * H + j];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int i = g + r * L.G;
      if (i < H) {
        const float4 v = *reinterpret_cast<const float4*>(hsT + i * L.NSP + s4);
        acc[r] = fmaf(v.x, qe[0], acc[r]); acc[r] = fmaf(v.y, qe[1], acc[r]); acc[r] = fmaf(v.z, qe[2], acc[r]); acc[r] = fmaf(v.w, qe[3], acc[r]);
      }
    }
  }
}

template <int NR>
__global__ __launch_bounds__(kRnnThreads) void tsgru_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dt,
                                                               const float* __restrict__ dt_out, const unsigned char* __restrict__ mask,
                                                               const float* __restrict__ W, const float* __restrict__ U,
                                                               const float* __restrict__ Wf, const float* __restrict__ saved,
                                                               const float* __restrict__ g_hs, const float* __restrict__ g_last,
                                                               const float* __restrict__ g_z, float* __restrict__ dx,
                                                               float* __restrict__ partials, int B, RnnLayout L, TsLayout X) {
  extern __shared__ __attribute__((aligned(16))) float ts_smem[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int T = L.T, K = L.K, H = L.H, H3 = L.HG, NS = L.NS, NSP = L.NSP, G = L.G, KH = L.K + L.H, S = X.S, PL = X.planes;
  rnn_stage_transposed(ts_smem, W, K, L);
  rnn_stage_transposed(ts_smem + L.b_UT, U, H, L);
  for (int i = tid; i < H * H; i += nthr) {      // WfT [m][k] = Wf [k][m]
    const int k = i / H, m = i - k * H;
    ts_smem[X.b_WfT + m * H + k] = Wf[i];
  }
  const float* WT = ts_smem;
  const float* UT = ts_smem + L.b_UT;
  const float* WfT = ts_smem + X.b_WfT;
  float* dT = ts_smem + L.b_dT;
  float* dS = ts_smem + L.b_dS;
  const bool active = tid < G * H;
  const int g = tid / H, j = tid - g * H;
  const bool want_params = partials != nullptr;
  const float fS = (float)S;
  const float* savedF = saved + (long)B * T * PL * H;
  float acc[NR][kTsGates], accF[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r][0] = acc[r][1] = acc[r][2] = accF[r] = 0.f;
  float dbs[4] = {0.f, 0.f, 0.f, 0.f};      // the thread's samples' dz, dr, dc (input side), dc r (recurrent side)
  float dbfs = 0.f;                         // ... and q
  int par = 0;                              // the substep image in turn
  const long n_tiles = ((long)B + NS - 1) / NS;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long b0 = tile * NS;
    float dh[4] = {0.f, 0.f, 0.f, 0.f};
    float svn[4][4] = {}, ohn[4] = {}, ofn[4] = {}, dln[4] = {}, ghn[4] = {}, lvn = 0.f;
    bool lqn[4] = {false, false, false, false};
    float4 xr[kRnnXV];
    // what step tt needs, of the thread's unit and samples -> registers
    auto prefetch = [&](int tt) {
      if (want_params) rnn_load_x(xr, x, mask, b0, B, tt, L);
      lvn = rnn_load_live(mask, b0, B, tt, L);
      if (active) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long bb = b0 + 4 * g + e;
          const bool valid = bb < B;
          const bool live = valid && (mask == nullptr || mask[bb * T + tt] != 0);
          const float* sv = saved + ((bb * T + tt) * PL) * H + j;
#pragma unroll
          for (int c = 0; c < 4; ++c) svn[e][c] = live ? sv[c * H] : 0.f;
          ohn[e] = live ? sv[(4 + 2 * (S - 1)) * H] : 0.f;
          ofn[e] = live ? sv[(5 + 2 * (S - 1)) * H] : 0.f;
          dln[e] = live ? dt[bb * T + tt] / fS : 0.f;
          lqn[e] = live;
          ghn[e] = (valid && g_hs != nullptr) ? g_hs[(bb * T + tt) * H + j] : 0.f;
        }
      }
    };
    float sv[4][4] = {}, oh[4] = {}, of[4] = {}, dl[4] = {}, hp[4] = {}, gh[4] = {};
    bool lq[4] = {false, false, false, false};
    // ... -> the LDS images of buffer `buf` and the registers of the current step; hp = the state the GRU step saw
    auto commit = [&](int buf) {
      float* inT = ts_smem + L.b_in + buf * KH * NSP;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int c = 0; c < 4; ++c) sv[e][c] = svn[e][c];
        oh[e] = ohn[e]; of[e] = ofn[e]; dl[e] = dln[e]; lq[e] = lqn[e];
        hp[e] = fmaf(dl[e], of[e], oh[e]);
        gh[e] = ghn[e];
      }
      if (want_params) {
        rnn_store_x(xr, inT, L);
        if (active) *reinterpret_cast<float4*>(inT + (K + j) * NSP + 4 * g) = make_float4(hp[0], hp[1], hp[2], hp[3]);
      }
      if (tid < NS) ts_smem[L.b_live + buf * NS + tid] = lvn;
    };
    // the S substeps behind d, the gradient of an evolved state, in reverse: d becomes the gradient of the state before them.
    // (ph, pf) = the last substep's pair, delta / lv per sample of the quad; plane 0 of the pairs of sample e is p0 + e * es.
    auto ode_bwd = [&](float (&d)[4], float (&ph)[4], float (&pf)[4], const float (&delta)[4], const bool (&lv)[4], const float* p0, long es) {
      for (int s = S - 1; s >= 0; --s) {
        float nh[4] = {0.f, 0.f, 0.f, 0.f}, nf[4] = {0.f, 0.f, 0.f, 0.f};
        if (s > 0 && active) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (lv[e]) {
              const float* p = p0 + e * es + 2 * (s - 1) * H;
              nh[e] = p[0]; nf[e] = p[H];
            }
          }
        }
        float* hsT = ts_smem + X.b_img + par * X.img;
        float* qT = hsT + H * NSP;
        float* qS = qT + H * NSP;
        if (active) {
          float q[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            q[e] = lv[e] ? (delta[e] * d[e]) * (1.f - pf[e] * pf[e]) : 0.f;
            dbfs += q[e];
            qS[(4 * g + e) * H + j] = q[e];
          }
          *reinterpret_cast<float4*>(qT + j * NSP + 4 * g) = make_float4(q[0], q[1], q[2], q[3]);
          if (want_params) *reinterpret_cast<float4*>(hsT + j * NSP + 4 * g) = make_float4(ph[0], ph[1], ph[2], ph[3]);
        }
        __syncthreads();
        if (active) {
          float v[4] = {0.f, 0.f, 0.f, 0.f};
          const float* qq = qT + 4 * g;
#pragma unroll 4
          for (int m = 0; m < H; ++m) {
            const float4 q4 = *reinterpret_cast<const float4*>(qq + m * NSP);
            const float w = WfT[m * H + j];
            v[0] = fmaf(q4.x, w, v[0]); v[1] = fmaf(q4.y, w, v[1]); v[2] = fmaf(q4.z, w, v[2]); v[3] = fmaf(q4.w, w, v[3]);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) d[e] += v[e];
          if (want_params) ts_bwd_accumulate(accF, hsT, qS, g, j, L);
        }
        par ^= 1;
#pragma unroll
        for (int e = 0; e < 4; ++e) { ph[e] = nh[e]; pf[e] = nf[e]; }
      }
    };
    if (active && g_last != nullptr) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long bb = b0 + 4 * g + e;
        if (bb < B) dh[e] = g_last[bb * H + j];
      }
    }
    __syncthreads();      // the weights are staged; the previous tile's images are free
    prefetch(T - 1);
    commit((T - 1) & 1);
    __syncthreads();
    if (g_z != nullptr) {
      // the final evolution of every sample of the batch
      float dz[4] = {0.f, 0.f, 0.f, 0.f}, ph[4] = {0.f, 0.f, 0.f, 0.f}, pf[4] = {0.f, 0.f, 0.f, 0.f}, delta[4] = {0.f, 0.f, 0.f, 0.f};
      bool lv[4] = {false, false, false, false};
      const float* p0 = savedF + ((b0 + 4 * g) * 2 * S) * H + j;
      if (active) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long bb = b0 + 4 * g + e;
          lv[e] = bb < B;
          if (lv[e]) {
            dz[e] = g_z[bb * H + j];
            delta[e] = dt_out[bb] / fS;
            const float* p = p0 + e * (long)2 * S * H + 2 * (S - 1) * H;
            ph[e] = p[0]; pf[e] = p[H];
          }
        }
      }
      ode_bwd(dz, ph, pf, delta, lv, p0, (long)2 * S * H);
#pragma unroll
      for (int e = 0; e < 4; ++e) dh[e] += dz[e];
    }
    for (int t = T - 1; t >= 0; --t) {
      const int cur = t & 1;
      if (t > 0) prefetch(t - 1);
      float keep[4] = {0.f, 0.f, 0.f, 0.f};
      if (active) {
        // phase 1: the gate gradients of (unit j, the quad's samples)
        float dz[4], dr[4], dcx[4], dch[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int s = 4 * g + e;
          const bool live = lq[e];
          if (g_hs != nullptr) dh[e] += gh[e];
          const float z = sv[e][0], r = sv[e][1], c = sv[e][2], hph = sv[e][3];
          const float u = 1.f - z;
          const float du = dh[e] * (c - hp[e]);
          const float dcp = (dh[e] * u) * (1.f - c * c);
          dz[e] = live ? -du * (z * (1.f - z)) : 0.f;
          dr[e] = live ? (dcp * hph) * (r * (1.f - r)) : 0.f;
          dcx[e] = live ? dcp : 0.f;
          dch[e] = live ? dcp * r : 0.f;
          keep[e] = live ? dh[e] * (1.f - u) : dh[e];
          dS[s * 4 * H + j] = dz[e];
          dS[s * 4 * H + H + j] = dr[e];
          dS[s * 4 * H + 2 * H + j] = dcx[e];
          dS[s * 4 * H + 3 * H + j] = dch[e];
          dbs[0] += dz[e]; dbs[1] += dr[e]; dbs[2] += dcx[e]; dbs[3] += dch[e];
        }
        *reinterpret_cast<float4*>(dT + j * NSP + 4 * g) = make_float4(dz[0], dz[1], dz[2], dz[3]);
        *reinterpret_cast<float4*>(dT + (H + j) * NSP + 4 * g) = make_float4(dr[0], dr[1], dr[2], dr[3]);
        *reinterpret_cast<float4*>(dT + (2 * H + j) * NSP + 4 * g) = make_float4(dcx[0], dcx[1], dcx[2], dcx[3]);
        *reinterpret_cast<float4*>(dT + (3 * H + j) * NSP + 4 * g) = make_float4(dch[0], dch[1], dch[2], dch[3]);
      }
      __syncthreads();
      // phase 2: the gradient of the evolved state, dh (1 - u) + d_hp U^T (at t = 0 too: the ODE moved the zero state), and dW / dU
      if (active) {
        float nh[4] = {0.f, 0.f, 0.f, 0.f};
        rnn_bwd_matvec<true>(nh, dT + 4 * g, UT, H, j, L);
#pragma unroll
        for (int e = 0; e < 4; ++e) dh[e] = keep[e] + nh[e];
        if (want_params) rnn_bwd_accumulate(acc, ts_smem + L.b_in + cur * KH * NSP, dS, g, j, L);
      }
      // phase 3: the substeps in front of the step.  Their images are their own: dT stays as it is for dx below.
      ode_bwd(dh, oh, of, dl, lq, saved + (((b0 + 4 * g) * T + t) * PL + 4) * H + j, (long)T * PL * H);
      // the registers loaded at the top of the step -> LDS BEFORE this step's stores are issued (rnn_tile.h, Schedule)
      const float* liveq = ts_smem + L.b_live + cur * NS + 4 * g;
      if (t > 0) commit((t - 1) & 1);
      if (active && dx != nullptr) rnn_bwd_dx(dx, dT + 4 * g, WT, liveq, b0 + 4 * g, B, t, j, L);
      __syncthreads();
    }
  }
  if (!want_params) return;
  // the workgroup's partial; db = the four sums on the two bias rows: dz, dr on both, dc on the input side's, dc r on the recurrent side's
  float* part = partials + (long)blockIdx.x * X.n_out;
  rnn_bwd_write_partial(part, acc, dbs, dS, active, g, j, L);
  for (int o = tid; o < 4 * H; o += nthr) {
    const int c = o / H, jj = o - c * H;
    const float sum = rnn_bwd_quad_sum(dS, o, L);
    float* db = part + KH * H3;
    if (c < 2) { db[c * H + jj] = sum; db[H3 + c * H + jj] = sum; }
    else if (c == 2) db[2 * H + jj] = sum;
    else db[H3 + 2 * H + jj] = sum;
  }
  // dWf as it stands; dbf = the quads' sums in quad order, through the first plane of dS [G][4][H]
  __syncthreads();
  if (active) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int i = g + r * G;
      if (i < H) part[L.n_out + i * H + j] = accF[r];
    }
    dS[g * 4 * H + j] = dbfs;
  }
  __syncthreads();
  for (int o = tid; o < H; o += nthr) part[L.n_out + H * H + o] = rnn_bwd_quad_sum(dS, o, L);
}

// argument and menu checks shared by the entry points: the signs, S below 1 (FIL_ERR_ARG); then the menu (FIL_ERR_UNSUPPORTED):
// S above kTsMaxSteps, rnn_tile.h's K and H, and the LDS of both passes with the op's own sections
static int tsgru_dims(const char* who, int B, int T, int K, int H, int S, RnnLayout* L, TsLayout* X) {
  FIL_CHECK_ARG_W(who, B >= 0 && T >= 1 && K >= 1 && H >= 1 && S >= 1);
  if (S > kTsMaxSteps) return fail(FIL_ERR_UNSUPPORTED, "%s: S=%d needs S <= %d", who, S, kTsMaxSteps);
  if (int rc = rnn_dims(who, B, T, K, H, kTsGates, kTsBiasRows, true, L)) return rc;
  *X = ts_layout(*L, S);
  if (X->lds_fwd > kTiledLdsLimit || X->lds_bwd > kTiledLdsLimit)
    return fail(FIL_ERR_UNSUPPORTED, "%s: K=%d H=%d needs %d bytes of LDS (limit %d)", who, K, H, std::max(X->lds_fwd, X->lds_bwd), kTiledLdsLimit);
  return FIL_OK;
}

}  // namespace fil

using namespace fil;

extern "C" int fil_tsgru_plan(int B, int T, int K, int H, int S, int* plan) {
  RnnLayout L;
  TsLayout X;
  if (int rc = tsgru_dims(__func__, B, T, K, H, S, &L, &X)) return rc;
  FIL_CHECK_ARG(plan != nullptr);
  tiled_plan(plan, L.NS, rnn_grid(B, L.NS), kRnnGridCap, X.lds_fwd, X.lds_bwd);
  return FIL_OK;
}

extern "C" size_t fil_tsgru_saved_bytes(int B, int T, int K, int H, int S) {
  RnnLayout L;
  TsLayout X;
  if (tsgru_dims(__func__, B, T, K, H, S, &L, &X) != FIL_OK) return 0;
  return align_up(((size_t)B * (size_t)T * (size_t)X.planes + (size_t)B * 2 * (size_t)S) * (size_t)H * sizeof(float), 256);
}

extern "C" int fil_tsgru_fwd(const float* x, const float* dt, const float* dt_out, const unsigned char* mask, const float* W, const float* U,
                             const float* b, const float* Wf, const float* bf, float* hs, float* z, float* saved, int B, int T, int K, int H,
                             int S, void* stream) {
  RnnLayout L;
  TsLayout X;
  if (int rc = tsgru_dims(__func__, B, T, K, H, S, &L, &X)) return rc;
  if (B == 0) return FIL_OK;
  FIL_CHECK_ARG(x != nullptr && dt != nullptr && W != nullptr && U != nullptr && b != nullptr && Wf != nullptr && bf != nullptr && hs != nullptr);
  FIL_CHECK_ARG((dt_out == nullptr) == (z == nullptr));
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("tsgru_fwd", st, 4.0 * (double)B * T * (K + 1 + H + (saved != nullptr ? (double)X.planes * H : 0.0)));
  if (int rc = tiled_allow_lds(__func__, tsgru_fwd_kernel, X.lds_fwd)) return rc;
  hipLaunchKernelGGL(tsgru_fwd_kernel, dim3(rnn_grid(B, L.NS)), dim3(L.threads), X.lds_fwd, st, x, dt, dt_out, mask, W, U, b, Wf, bf, hs, z, saved,
                     B, L, X);
  FIL_CHECK_LAUNCH();
  return FIL_OK;
}

extern "C" size_t fil_tsgru_bwd_workspace_bytes(int B, int T, int K, int H, int S) {
  RnnLayout L;
  TsLayout X;
  if (tsgru_dims(__func__, B, T, K, H, S, &L, &X) != FIL_OK) return 0;
  return tiled_partial_bytes(rnn_grid(B, L.NS), X.n_out);
}

extern "C" int fil_tsgru_bwd(const float* x, const float* dt, const float* dt_out, const unsigned char* mask, const float* W, const float* U,
                             const float* Wf, const float* saved, const float* g_hs, const float* g_last, const float* g_z, float* dx,
                             float* dW, float* dU, float* db, float* dWf, float* dbf, void* workspace, size_t workspace_bytes, int B, int T,
                             int K, int H, int S, void* stream) {
  RnnLayout L;
  TsLayout X;
  if (int rc = tsgru_dims(__func__, B, T, K, H, S, &L, &X)) return rc;
  if (B == 0) return FIL_OK;
  FIL_CHECK_ARG(x != nullptr && dt != nullptr && W != nullptr && U != nullptr && Wf != nullptr && saved != nullptr);
  FIL_CHECK_ARG(g_hs != nullptr || g_last != nullptr || g_z != nullptr);
  FIL_CHECK_ARG(g_z == nullptr || dt_out != nullptr);
  const bool want_params = dW != nullptr || dU != nullptr || db != nullptr || dWf != nullptr || dbf != nullptr;
  FIL_CHECK_ARG(dx != nullptr || want_params);
  const int nparts = rnn_grid(B, L.NS);
  if (want_params)
    if (int rc = tiled_check_workspace(__func__, workspace, workspace_bytes, nparts, X.n_out)) return rc;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("tsgru_bwd", st, 4.0 * (double)B * T * (2.0 * K + 1.0 + (2.0 + X.planes) * H));
  // (rnn_launch_bwd sizes the launch by the layout's lds_bwd: the op's own sections are behind it, so the NR switch is restated)
  auto launch = [&](auto nr) -> int {
    auto kernel = tsgru_bwd_kernel<decltype(nr)::value>;
    if (int rc = tiled_allow_lds(__func__, kernel, X.lds_bwd)) return rc;
    hipLaunchKernelGGL(kernel, dim3(nparts), dim3(L.threads), X.lds_bwd, st, x, dt, dt_out, mask, W, U, Wf, saved, g_hs, g_last, g_z, dx,
                       want_params ? static_cast<float*>(workspace) : nullptr, B, L, X);
    return FIL_OK;
  };
  if (int rc = L.NR == 8 ? launch(std::integral_constant<int, 8>())
                         : (L.NR == 16 ? launch(std::integral_constant<int, 16>()) : launch(std::integral_constant<int, 32>())))
    return rc;
  FIL_CHECK_LAUNCH();
  if (want_params) {
    float* const outs[5] = {dW, dU, db, dWf, dbf};
    const int off[6] = {0, K * L.HG, (K + H) * L.HG, L.n_out, L.n_out + H * H, X.n_out};
    param_reduce_launch(static_cast<const float*>(workspace), nparts, outs, off, 5, st);
    FIL_CHECK_LAUNCH();
  }
  return FIL_OK;
}
