// The sample-quad tiling of the recurrent ops (gru.hip: three gates, two bias rows, scores; lstm.hip: four gates, one bias row),
// defined once: the tile geometry, the LDS layout, the menu checks, the staging, the products of a step in both directions and the
// write of a workgroup's partial.  The step loops, the cell math and what only one op has stay with the op.
//
// Structure.  A workgroup owns a tile of NS = 4 G samples for all T steps; a thread owns ONE hidden unit j of FOUR samples (g = its
// sample quad), so that every weight read from LDS feeds four samples.  The weights are staged once per workgroup (forward: W, U as
// given, lanes = consecutive columns; backward: their transposes, and nothing else -- the backward recomputes no product, it reads
// the gates from `saved`).  x_t and the hidden state sit in LDS TRANSPOSED ([feature][sample], row stride NS + 4) so that one
// 16-byte read gives a feature of the thread's four samples; they are double buffered and the global loads of the next step are in
// flight during the arithmetic of this one (the step is a dependent chain: nothing else hides the load).  The backward leaves the
// gate gradients in LDS twice, dT [plane][sample] for the two transposed products and dS [sample][plane] for the weight gradients,
// FOUR planes of H in both ops: the GRU's fourth is the recurrent side's dc r.
//
// Schedule.  Forward, within a step: the arithmetic; the registers loaded a step ago -> LDS (the wait for them also covers the
// stores of the step before, long under way); this step's stores; the loads of the step after next.  A wait right behind fresh
// stores would put their latency on the chain.  Backward: the loads of the step before are issued at the top of the step, and their
// registers go to LDS BEFORE this step's stores are issued: the wait for those loads would otherwise also sit out the fresh stores,
// on the chain.
//
// Every fmaf chain below runs in one fixed order (k, m ascending; samples in sample order): the ops' bits depend on it.
#pragma once
#include "common.h"
#include "tiled_launch.h"
#include <algorithm>
#include <type_traits>

namespace fil {

constexpr int kRnnMaxK = 64, kRnnMaxH = 64;
constexpr int kRnnGridCap = 1024;      // workgroups per launch (and direction)
constexpr int kRnnThreads = 256;       // the most a workgroup has
constexpr int kRnnXV = 4;              // 16-byte pieces of x_t a thread stages per step, at most

// all LDS offsets in floats (multiples of 4); HG = gates * H; the sections in brackets exist with scores only
struct RnnLayout {
  int T, K, H, HG, G, NS, NSP, threads, NR;
  int f_U, f_b, f_x, f_h, f_live, f_a, lds_fwd;              // forward:  W | U | b [rows][HG] | xT [2][K][NSP] | hT [2][H][NSP] | live [2][NS] |
                                                             //           (a [2][NS])
  int b_UT, b_in, b_dT, b_dS, b_da, b_live, b_a, lds_bwd;    // backward: WT [HG][K] | UT [HG][H] | inT [2][K+H][NSP] | dT [4H][NSP] | dS [NS][4H] |
                                                             //           (da terms [H][NSP]) | live [2][NS] | (a [2][NS])
  int n_out;                                                 // one partial: dW [K][HG] | dU [H][HG] | db [rows][HG]
};

static inline RnnLayout rnn_layout(int B, int T, int K, int H, int gates, int bias_rows, bool scores) {
  RnnLayout L;
  L.T = T; L.K = K; L.H = H; L.HG = gates * H;
  const int P = std::max(H, K / 4);                         // threads per sample quad: a unit each, and enough to stage x_t in kRnnXV pieces
  const int Gmax = kRnnThreads / P;                         // >= 4
  const int Gmin = std::min(Gmax, cdiv(64, P));             // a full wave where the shape allows
  const int Glow = std::max(Gmin, cdiv(K + H, 32));         // at most 32 rows of [dW ; dU] per thread
  const long want = ((long)B + 4L * kRnnGridCap - 1) / (4L * kRnnGridCap);      // small batches: small tiles, more workgroups
  L.G = (int)std::min((long)Gmax, std::max((long)Glow, want));
  L.NS = 4 * L.G;
  L.NSP = L.NS + 4;
  L.threads = (L.G * P + 63) / 64 * 64;
  const int nr = cdiv(K + H, L.G);
  L.NR = nr <= 8 ? 8 : (nr <= 16 ? 16 : 32);
  const int a_floats = scores ? 2 * L.NS : 0;
  L.f_U = K * L.HG;
  L.f_b = L.f_U + H * L.HG;
  L.f_x = L.f_b + bias_rows * L.HG;
  L.f_h = L.f_x + 2 * K * L.NSP;
  L.f_live = L.f_h + 2 * H * L.NSP;
  L.f_a = L.f_live + 2 * L.NS;
  L.lds_fwd = 4 * (L.f_a + a_floats);
  L.b_UT = K * L.HG;
  L.b_in = L.b_UT + H * L.HG;
  L.b_dT = L.b_in + 2 * (K + H) * L.NSP;
  L.b_dS = L.b_dT + 4 * H * L.NSP;
  L.b_da = L.b_dS + L.NS * 4 * H;
  L.b_live = L.b_da + (scores ? H * L.NSP : 0);
  L.b_a = L.b_live + 2 * L.NS;
  L.lds_bwd = 4 * (L.b_a + a_floats);
  L.n_out = (K + H + bias_rows) * L.HG;
  return L;
}

static inline int rnn_grid(int B, int NS) { return tiled_grid(B, NS, kRnnGridCap); }

// the menu checks shared by the entry points of both ops, and the layout.  An op checks the signs of B, T, K, H and then its mode /
// its directions in front of this: a call wrong in several ways is answered for the first of them.
static inline int rnn_dims(const char* who, int B, int T, int K, int H, int gates, int bias_rows, bool scores, RnnLayout* L) {
  if (K % 4 != 0 || K > kRnnMaxK) return fail(FIL_ERR_UNSUPPORTED, "%s: K=%d needs K %% 4 == 0 and K <= %d", who, K, kRnnMaxK);
  if (H % 4 != 0 || H > kRnnMaxH) return fail(FIL_ERR_UNSUPPORTED, "%s: H=%d needs H %% 4 == 0 and H <= %d", who, H, kRnnMaxH);
  *L = rnn_layout(B, T, K, H, gates, bias_rows, scores);
  if (L->lds_fwd > kTiledLdsLimit || L->lds_bwd > kTiledLdsLimit)
    return fail(FIL_ERR_UNSUPPORTED, "%s: K=%d H=%d needs %d bytes of LDS (limit %d)", who, K, H, std::max(L->lds_fwd, L->lds_bwd), kTiledLdsLimit);
  return FIL_OK;
}

// Launches the instantiation of a backward kernel template that the layout's NR selects.  `kernel_of(nr)` returns it for
// nr = std::integral_constant<int, 8 | 16 | 32> (a generic lambda: a function template cannot be passed); `args` are the kernel's
// arguments in front of the layout.
template <typename KernelOf, typename... Args>
static int rnn_launch_bwd(const char* who, KernelOf kernel_of, const RnnLayout& L, dim3 grid, hipStream_t st, Args... args) {
  auto launch = [&](auto nr) -> int {
    auto kernel = kernel_of(nr);
    if (int rc = tiled_allow_lds(who, kernel, L.lds_bwd)) return rc;
    hipLaunchKernelGGL(kernel, grid, dim3(L.threads), L.lds_bwd, st, args..., L);
    return FIL_OK;
  };
  return L.NR == 8 ? launch(std::integral_constant<int, 8>())
                   : (L.NR == 16 ? launch(std::integral_constant<int, 16>()) : launch(std::integral_constant<int, 32>()));
}

__device__ __forceinline__ float rnn_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// 16-byte pieces of x_t of the tile's samples -> registers; a masked step's (and a sample past B's) row is never read: zeros
__device__ __forceinline__ void rnn_load_x(float4 (&xr)[kRnnXV], const float* __restrict__ x, const unsigned char* __restrict__ mask, long b0,
                                           int B, int t, const RnnLayout& L) {
  const int KQ = L.K / 4, n = L.NS * KQ;
#pragma unroll
  for (int i = 0; i < kRnnXV; ++i) {
    const int idx = threadIdx.x + i * blockDim.x;
    xr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (idx < n) {
      const int s = idx / KQ, kq = idx - s * KQ;
      const long bb = b0 + s;
      if (bb < B && (mask == nullptr || mask[bb * L.T + t] != 0))
        xr[i] = *reinterpret_cast<const float4*>(x + (bb * L.T + t) * L.K + kq * 4);
    }
  }
}

// ... -> the transposed LDS image xT [K][NSP]
__device__ __forceinline__ void rnn_store_x(const float4 (&xr)[kRnnXV], float* xT, const RnnLayout& L) {
  const int KQ = L.K / 4, n = L.NS * KQ;
#pragma unroll
  for (int i = 0; i < kRnnXV; ++i) {
    const int idx = threadIdx.x + i * blockDim.x;
    if (idx < n) {
      const int s = idx / KQ, kq = idx - s * KQ;
      float* d = xT + (kq * 4) * L.NSP + s;
      d[0] = xr[i].x; d[L.NSP] = xr[i].y; d[2 * L.NSP] = xr[i].z; d[3 * L.NSP] = xr[i].w;
    }
  }
}

// live flag (1 / 0) of sample b0 + threadIdx.x at time position t (threads below NS)
__device__ __forceinline__ float rnn_load_live(const unsigned char* __restrict__ mask, long b0, int B, int t, const RnnLayout& L) {
  if ((int)threadIdx.x < L.NS) {
    const long bb = b0 + threadIdx.x;
    if (bb < B && (mask == nullptr || mask[bb * L.T + t] != 0)) return 1.f;
  }
  return 0.f;
}

// n floats -> LDS as given.  The induction is a signed int on purpose: the compiler unrolls this loop by eight, eight loads in
// flight; stepping by blockDim.x itself (unsigned) keeps it from doing so, and every load then waits out its own round trip.
__device__ __forceinline__ void rnn_stage(float* dst, const float* __restrict__ src, int n) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  for (int i = tid; i < n; i += nthr) dst[i] = src[i];
}

// a weight [rows][HG] -> LDS transposed: dst [m][k] = src [k][m]
__device__ __forceinline__ void rnn_stage_transposed(float* dst, const float* __restrict__ src, int rows, const RnnLayout& L) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  for (int i = tid; i < rows * L.HG; i += nthr) {
    const int k = i / L.HG, m = i - k * L.HG;
    dst[m * rows + k] = src[i];
  }
}

// forward: acc [c][e] += in [k][sample e of the quad] * Ws [k][c H + j] over the n rows of a staged weight, k ascending;
// `in` = the quad's column of a transposed image [n][NSP].  The row's address is formed first and the gates are offsets from it:
// with one index expression per gate the compiler keeps a base per gate and gives the reads a wait apiece, on the chain.
// (gru_fwd_kernel's two loops; lstm_fwd_kernel keeps its own, see there.)
template <int GATES>
__device__ __forceinline__ void rnn_fwd_products(float (&acc)[GATES][4], const float* in, const float* Ws, int n, int j, const RnnLayout& L) {
#pragma unroll 4
  for (int k = 0; k < n; ++k) {
    const float4 v = *reinterpret_cast<const float4*>(in + k * L.NSP);
    const float ve[4] = {v.x, v.y, v.z, v.w};
    const float* wk = Ws + k * L.HG + j;
#pragma unroll
    for (int c = 0; c < GATES; ++c) {
      const float w = wk[c * L.H];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[c][e] = fmaf(ve[e], w, acc[c][e]);
    }
  }
}

// backward: v [e] += dT [row m][sample e of the quad] * WT [m][o] over the HG rows of a transposed weight [HG][n], m ascending;
// dTq = the quad's column of dT.  SKIP_THIRD (the GRU's recurrent side): the rows are the planes 0, 1 and 3 of dT.
template <bool SKIP_THIRD>
__device__ __forceinline__ void rnn_bwd_matvec(float (&v)[4], const float* dTq, const float* WT, int n, int o, const RnnLayout& L) {
#pragma unroll 4
  for (int m = 0; m < L.HG; ++m) {
    const float4 d = *reinterpret_cast<const float4*>(dTq + (SKIP_THIRD && m >= 2 * L.H ? m + L.H : m) * L.NSP);
    const float w = WT[m * n + o];
    v[0] = fmaf(d.x, w, v[0]); v[1] = fmaf(d.y, w, v[1]); v[2] = fmaf(d.z, w, v[2]); v[3] = fmaf(d.w, w, v[3]);
  }
}

// backward: dx_t = (the gate gradients of the input side) W^T of the quad's samples, outputs k = j, j + H, ...; a masked step's
// row is zero.  liveq = the quad's live flags of the step, b0q = its first sample.
__device__ __forceinline__ void rnn_bwd_dx(float* __restrict__ dx, const float* dTq, const float* WT, const float* liveq, long b0q, int B,
                                           int t, int j, const RnnLayout& L) {
  for (int k = j; k < L.K; k += L.H) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    rnn_bwd_matvec<false>(v, dTq, WT, L.K, k, L);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long bb = b0q + e;
      const bool live = liveq[e] != 0.f;
      if (bb < B) dx[(bb * L.T + t) * L.K + k] = live ? v[e] : 0.f;
    }
  }
}

// backward: dW / dU.  The thread's GATES columns (the gates of its unit j) of the rows g, g + G, ... of [x_t ; h_prev]^T d, summed
// over the tile's samples in sample order.  inT = the step's image [K+H][NSP], dS = the gate gradients [NS][4H].  With three gates
// the rows of h_prev take the fourth plane (the recurrent side's gradient) for their third column.
template <int NR, int GATES>
__device__ __forceinline__ void rnn_bwd_accumulate(float (&acc)[NR][GATES], const float* inT, const float* dS, int g, int j, const RnnLayout& L) {
  const int H = L.H, KH = L.K + L.H;
  for (int s4 = 0; s4 < L.NS; s4 += 4) {
    float ez[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float* d = dS + (s4 + e) * 4 * H + j;
      ez[0][e] = d[0]; ez[1][e] = d[H]; ez[2][e] = d[2 * H]; ez[3][e] = d[3 * H];
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int i = g + r * L.G;
      if (i < KH) {
        const float4 v = *reinterpret_cast<const float4*>(inT + i * L.NSP + s4);
        const float ve[4] = {v.x, v.y, v.z, v.w};
        const bool xrow = i < L.K;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
          for (int q = 0; q < GATES; ++q) acc[r][q] = fmaf(ve[e], (GATES == 3 && q == 2 && !xrow) ? ez[3][e] : ez[q][e], acc[r][q]);
        }
      }
    }
  }
}

// the workgroup's partial: the accumulators as they stand -> part (dW, dU), and the threads' four bias sums -> dS [G][4][H] (the last
// barrier of the step loop has passed: dS is free).  Ends in a barrier; rnn_bwd_quad_sum then reads dS.
template <int NR, int GATES>
__device__ __forceinline__ void rnn_bwd_write_partial(float* __restrict__ part, const float (&acc)[NR][GATES], const float (&dbs)[4], float* dS,
                                                      bool active, int g, int j, const RnnLayout& L) {
  if (active) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int i = g + r * L.G;
      if (i < L.K + L.H) {
#pragma unroll
        for (int q = 0; q < GATES; ++q) part[i * L.HG + q * L.H + j] = acc[r][q];
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) dS[(g * 4 + c) * L.H + j] = dbs[c];
  }
  __syncthreads();
}

// bias sum o = c H + unit of the four planes: the quads' sums in quad order
__device__ __forceinline__ float rnn_bwd_quad_sum(const float* dS, int o, const RnnLayout& L) {
  float sum = 0.f;
  for (int gg = 0; gg < L.G; ++gg) sum += dS[gg * 4 * L.H + o];
  return sum;
}

}  // namespace fil
