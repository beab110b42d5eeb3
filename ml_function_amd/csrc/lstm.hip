// N3  LSTM over a sequence for gfx950, one direction or both in one launch, forward and backward, fp32 (extension: TF 2 Keras' LSTM
// with its defaults, and Keras' Bidirectional(LSTM) as the session interest interacting layer of the Deep Session Interest Network).
//
//     z = x_t W + h U + b                                         (columns i | f | c | o)
//     i = sigmoid(z_i);  f = sigmoid(z_f);  g = tanh(z_c);  o = sigmoid(z_o);   c_new = f c + i g;   h_new = o tanh(c_new)
//     a masked step carries h and c.
//
// Structure: rnn_tile.h's sample-quad tiling and schedule, with four gates and one bias row.  A workgroup owns its tile for all T
// steps of ONE direction (blockIdx.y selects it: its weights are the only ones staged); a thread owns, with its unit of four
// samples, the cell: c (forward) and dc (backward) live in registers.  A direction walks its steps
// s = 0 .. T-1 at the time positions t = s (forward) or t = T-1-s (reverse) and leaves the state reached after step s at position t.
//   forward   per step: 4 (K + H) weight reads + (K + H) state reads for 16 (K + H) FMAs per thread; the gates; hs, saved -> global;
//             the new h -> LDS.  One barrier.  saved [B,T,5,H] per direction = (i, f, g, o) of the live steps and the cell c after
//             EVERY step: c_prev of a live step is the cell carried across the masked steps before it.
//   backward  s = T-1 .. 0, dh and dc in registers.  Per step:
//             1  the gate gradients dz of the thread's unit and samples from `saved` (tanh(c_new) is taken again: one tanhf per
//                element instead of a sixth saved plane) -> LDS, both [column][sample] and [sample][column].         (barrier)
//             2  dh_prev = dz U^T, dx_t = dz W^T (transposed weights, lanes = consecutive outputs);
//                dW / dU: the thread's four columns (the gates of its unit) of the rows g, g + G, ... of [x_t ; h_prev]^T dz, summed over
//                the tile's samples in sample order, in registers over all steps and tiles (NR x 4 accumulators, NR <= 32).  (barrier)
//             One partial per workgroup; param_reduce_kernel adds a direction's partials in a fixed order.  With both directions
//             in one launch the reverse direction's dx goes to the workspace and one more small launch adds it to dx.
// No atomics; every sum has a fixed order for a given shape: repeats are bit-identical.
#include "common.h"
#include "param_reduce.h"
#include "rnn_tile.h"
#include <algorithm>
#include <math.h>

namespace fil {

constexpr int kLstmGates = 4, kLstmBiasRows = 1;
constexpr int kLstmSaved = 5;           // planes of `saved` per step: i, f, g, o, c

static inline int lstm_ndir(int dirs) { return dirs == FIL_LSTM_BIDIR ? 2 : 1; }

// the workspace of a backward, in floats: the partials of every direction (rounded up to 256 bytes), then, with both directions in
// one launch, the reverse direction's dx [B,T,K]
static inline size_t lstm_workspace_floats(int B, int dirs, const RnnLayout& L) {
  const size_t parts = tiled_partial_bytes(lstm_ndir(dirs) * rnn_grid(B, L.NS), L.n_out) / sizeof(float);
  return parts + (dirs == FIL_LSTM_BIDIR ? (size_t)B * L.T * L.K : 0);
}

// blockIdx.y = the direction's index among those of the call (its weights, its columns of hs, its block of saved); dir0 = the first
// one's direction (FIL_LSTM_FORWARD or FIL_LSTM_REVERSE), ndir = how many the call runs
__global__ __launch_bounds__(kRnnThreads) void lstm_fwd_kernel(const float* __restrict__ x, const unsigned char* __restrict__ mask,
                                                               const float* __restrict__ W, const float* __restrict__ U,
                                                               const float* __restrict__ bias, float* __restrict__ hs, float* __restrict__ saved,
                                                               int B, int dir0, int ndir, RnnLayout L) {
  extern __shared__ __attribute__((aligned(16))) float lstm_smem[];
  const int tid = threadIdx.x;
  const int T = L.T, K = L.K, H = L.H, H4 = L.HG, NS = L.NS, NSP = L.NSP;
  const int d = blockIdx.y, HO = ndir * H;
  const bool rev = dir0 + d == FIL_LSTM_REVERSE;
  W += (long)d * K * H4;
  U += (long)d * H * H4;
  bias += (long)d * H4;
  hs += d * H;
  if (saved != nullptr) saved += (long)d * B * T * kLstmSaved * H;
  rnn_stage(lstm_smem, W, K * H4);
  rnn_stage(lstm_smem + L.f_U, U, H * H4);
  rnn_stage(lstm_smem + L.f_b, bias, kLstmBiasRows * H4);
  const float* Ws = lstm_smem;
  const float* Us = lstm_smem + L.f_U;
  const float* bs = lstm_smem + L.f_b;
  const bool active = tid < L.G * H;
  const int g = tid / H, j = tid - g * H;
  const long n_tiles = ((long)B + NS - 1) / NS;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long b0 = tile * NS;
    float h[4] = {0.f, 0.f, 0.f, 0.f}, c[4] = {0.f, 0.f, 0.f, 0.f};
    float4 xr[kRnnXV];
    float lvn;
    __syncthreads();      // the weights are staged; the previous tile's images are free
    rnn_load_x(xr, x, mask, b0, B, rev ? T - 1 : 0, L);
    lvn = rnn_load_live(mask, b0, B, rev ? T - 1 : 0, L);
    rnn_store_x(xr, lstm_smem + L.f_x, L);
    if (tid < NS) lstm_smem[L.f_live + tid] = lvn;
    if (active) *reinterpret_cast<float4*>(lstm_smem + L.f_h + j * NSP + 4 * g) = make_float4(0.f, 0.f, 0.f, 0.f);
    if (T > 1) {
      rnn_load_x(xr, x, mask, b0, B, rev ? T - 2 : 1, L);
      lvn = rnn_load_live(mask, b0, B, rev ? T - 2 : 1, L);
    }
    __syncthreads();
    // the order within a step: rnn_tile.h, Schedule
    for (int s = 0; s < T; ++s) {
      const int t = rev ? T - 1 - s : s;
      const int cur = s & 1, nxt = cur ^ 1;
      float gv[4][4];
      bool lv[4] = {false, false, false, false};
      if (active) {
        float az[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float bq = bs[q * H + j];
#pragma unroll
          for (int e = 0; e < 4; ++e) az[q][e] = bq;
        }
        const float* xc = lstm_smem + L.f_x + cur * K * NSP + 4 * g;
        const float* hc = lstm_smem + L.f_h + cur * H * NSP + 4 * g;
        // (written out, not rnn_fwd_products: from the helper the compiler orders these two blocks' instructions differently, and the
        // bare forward measured 0.3 to 0.8 % slower)
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
          const float4 v = *reinterpret_cast<const float4*>(xc + k * NSP);
          const float ve[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float w = Ws[k * H4 + q * H + j];
#pragma unroll
            for (int e = 0; e < 4; ++e) az[q][e] = fmaf(ve[e], w, az[q][e]);
          }
        }
#pragma unroll 4
        for (int k = 0; k < H; ++k) {
          const float4 v = *reinterpret_cast<const float4*>(hc + k * NSP);
          const float ve[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float w = Us[k * H4 + q * H + j];
#pragma unroll
            for (int e = 0; e < 4; ++e) az[q][e] = fmaf(ve[e], w, az[q][e]);
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          lv[e] = lstm_smem[L.f_live + cur * NS + 4 * g + e] != 0.f;
          const float iv = rnn_sigmoid(az[0][e]);
          const float fv = rnn_sigmoid(az[1][e]);
          const float gg = tanhf(az[2][e]);
          const float ov = rnn_sigmoid(az[3][e]);
          const float cn = fmaf(fv, c[e], iv * gg);
          const float hn = ov * tanhf(cn);
          if (lv[e]) { c[e] = cn; h[e] = hn; }
          gv[e][0] = iv; gv[e][1] = fv; gv[e][2] = gg; gv[e][3] = ov;
        }
        *reinterpret_cast<float4*>(lstm_smem + L.f_h + nxt * H * NSP + j * NSP + 4 * g) = make_float4(h[0], h[1], h[2], h[3]);
      }
      if (s + 1 < T) {
        rnn_store_x(xr, lstm_smem + L.f_x + nxt * K * NSP, L);
        if (tid < NS) lstm_smem[L.f_live + nxt * NS + tid] = lvn;
      }
      if (active) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long bb = b0 + 4 * g + e;
          if (bb < B) {
            if (saved != nullptr) {
              float* sv = saved + ((bb * T + t) * kLstmSaved) * H + j;
              if (lv[e]) { sv[0] = gv[e][0]; sv[H] = gv[e][1]; sv[2 * H] = gv[e][2]; sv[3 * H] = gv[e][3]; }
              sv[4 * H] = c[e];
            }
            hs[(bb * T + t) * HO + j] = h[e];
          }
        }
      }
      if (s + 2 < T) {
        rnn_load_x(xr, x, mask, b0, B, rev ? T - 3 - s : s + 2, L);
        lvn = rnn_load_live(mask, b0, B, rev ? T - 3 - s : s + 2, L);
      }
      __syncthreads();
    }
  }
}

template <int NR>
__global__ __launch_bounds__(kRnnThreads) void lstm_bwd_kernel(const float* __restrict__ x, const unsigned char* __restrict__ mask,
                                                               const float* __restrict__ W, const float* __restrict__ U,
                                                               const float* __restrict__ hs, const float* __restrict__ saved,
                                                               const float* __restrict__ g_hs, const float* __restrict__ g_last,
                                                               float* __restrict__ dx, float* __restrict__ dx_second,
                                                               float* __restrict__ partials, int B, int dir0, int ndir, RnnLayout L) {
  extern __shared__ __attribute__((aligned(16))) float lstm_smem[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int T = L.T, K = L.K, H = L.H, H4 = L.HG, NS = L.NS, NSP = L.NSP, G = L.G, KH = L.K + L.H;
  const int d = blockIdx.y, HO = ndir * H;
  const bool rev = dir0 + d == FIL_LSTM_REVERSE;
  W += (long)d * K * H4;
  U += (long)d * H * H4;
  hs += d * H;
  saved += (long)d * B * T * kLstmSaved * H;
  if (g_hs != nullptr) g_hs += d * H;
  if (g_last != nullptr) g_last += d * H;
  if (d == 1) dx = dx_second;            // (both null when dx is not wanted)
  rnn_stage_transposed(lstm_smem, W, K, L);
  rnn_stage_transposed(lstm_smem + L.b_UT, U, H, L);
  const float* WT = lstm_smem;
  const float* UT = lstm_smem + L.b_UT;
  float* dT = lstm_smem + L.b_dT;
  float* dS = lstm_smem + L.b_dS;
  const bool active = tid < G * H;
  const int g = tid / H, j = tid - g * H;
  const bool want_params = partials != nullptr;
  float acc[NR][kLstmGates];
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = 0.f;
  float dbs[4] = {0.f, 0.f, 0.f, 0.f};      // the thread's samples' dz_i, dz_f, dz_c, dz_o
  const long n_tiles = ((long)B + NS - 1) / NS;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long b0 = tile * NS;
    float dh[4] = {0.f, 0.f, 0.f, 0.f}, dc[4] = {0.f, 0.f, 0.f, 0.f};
    float svn[4][4], cnn[4], cpn[4], hpn[4], ghn[4], lvn;
    float4 xr[kRnnXV];
    // what step ss needs, of the thread's unit and samples -> registers
    auto prefetch = [&](int ss) {
      const int tt = rev ? T - 1 - ss : ss;           // the step's time position, and the one of the step before it
      const int tp = rev ? tt + 1 : tt - 1;
      if (want_params) rnn_load_x(xr, x, mask, b0, B, tt, L);
      lvn = rnn_load_live(mask, b0, B, tt, L);
      if (active) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long bb = b0 + 4 * g + e;
          const bool valid = bb < B;
          const bool live = valid && (mask == nullptr || mask[bb * T + tt] != 0);
          const float* sv = saved + ((bb * T + tt) * kLstmSaved) * H + j;
#pragma unroll
          for (int q = 0; q < 4; ++q) svn[e][q] = live ? sv[q * H] : 0.f;
          cnn[e] = live ? sv[4 * H] : 0.f;
          cpn[e] = (live && ss > 0) ? saved[((bb * T + tp) * kLstmSaved + 4) * H + j] : 0.f;
          hpn[e] = (live && ss > 0) ? hs[(bb * T + tp) * HO + j] : 0.f;
          ghn[e] = (valid && g_hs != nullptr) ? g_hs[(bb * T + tt) * HO + j] : 0.f;
        }
      }
    };
    float sv[4][4], cn[4], cp[4], gh[4];
    // ... -> the LDS images of buffer `buf` and the registers of the current step
    auto commit = [&](int buf) {
      float* inT = lstm_smem + L.b_in + buf * KH * NSP;
      if (want_params) {
        rnn_store_x(xr, inT, L);
        if (active) *reinterpret_cast<float4*>(inT + (K + j) * NSP + 4 * g) = make_float4(hpn[0], hpn[1], hpn[2], hpn[3]);
      }
      if (tid < NS) lstm_smem[L.b_live + buf * NS + tid] = lvn;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int q = 0; q < 4; ++q) sv[e][q] = svn[e][q];
        cn[e] = cnn[e];
        cp[e] = cpn[e];
        gh[e] = ghn[e];
      }
    };
    if (active && g_last != nullptr) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long bb = b0 + 4 * g + e;
        if (bb < B) dh[e] = g_last[bb * HO + j];
      }
    }
    __syncthreads();      // the weights are staged; the previous tile's images are free
    prefetch(T - 1);
    commit((T - 1) & 1);
    __syncthreads();
    for (int s = T - 1; s >= 0; --s) {
      const int t = rev ? T - 1 - s : s;
      const int cur = s & 1;
      if (s > 0) prefetch(s - 1);
      float keep[4] = {0.f, 0.f, 0.f, 0.f};
      if (active) {
        // phase 1: the gate gradients of (unit j, the quad's samples)
        float dz[4][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int sm = 4 * g + e;
          const bool live = lstm_smem[L.b_live + cur * NS + sm] != 0.f;
          if (g_hs != nullptr) dh[e] += gh[e];
          const float iv = sv[e][0], fv = sv[e][1], gg = sv[e][2], ov = sv[e][3];
          const float tc = tanhf(cn[e]);
          const float dcv = fmaf(dh[e] * ov, 1.f - tc * tc, dc[e]);
          dz[0][e] = live ? (dcv * gg) * (iv * (1.f - iv)) : 0.f;
          dz[1][e] = live ? (dcv * cp[e]) * (fv * (1.f - fv)) : 0.f;
          dz[2][e] = live ? (dcv * iv) * (1.f - gg * gg) : 0.f;
          dz[3][e] = live ? (dh[e] * tc) * (ov * (1.f - ov)) : 0.f;
          if (live) dc[e] = dcv * fv;
          keep[e] = live ? 0.f : dh[e];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            dS[sm * H4 + q * H + j] = dz[q][e];
            dbs[q] += dz[q][e];
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<float4*>(dT + (q * H + j) * NSP + 4 * g) = make_float4(dz[q][0], dz[q][1], dz[q][2], dz[q][3]);
      }
      __syncthreads();
      // phase 2
      if (active) {
        // dh_prev = dz U^T (a masked step: dz = 0, the gradient passes through)
        float nh[4] = {0.f, 0.f, 0.f, 0.f};
        if (s > 0) rnn_bwd_matvec<false>(nh, dT + 4 * g, UT, H, j, L);
#pragma unroll
        for (int e = 0; e < 4; ++e) dh[e] = keep[e] + nh[e];
        if (want_params) rnn_bwd_accumulate(acc, lstm_smem + L.b_in + cur * KH * NSP, dS, g, j, L);
      }
      // the registers loaded at the top of the step -> LDS BEFORE this step's stores are issued (rnn_tile.h, Schedule)
      if (s > 0) commit((s - 1) & 1);
      if (active && dx != nullptr) rnn_bwd_dx(dx, dT + 4 * g, WT, lstm_smem + L.b_live + cur * NS + 4 * g, b0 + 4 * g, B, t, j, L);
      __syncthreads();
    }
  }
  if (!want_params) return;
  // the workgroup's partial; db = the quads' sums in quad order
  float* part = partials + ((long)d * gridDim.x + blockIdx.x) * L.n_out;
  rnn_bwd_write_partial(part, acc, dbs, dS, active, g, j, L);
  for (int o = tid; o < H4; o += nthr) part[KH * H4 + o] = rnn_bwd_quad_sum(dS, o, L);
}

// dx += the reverse direction's dx (both directions in one launch)
__global__ __launch_bounds__(256) void lstm_dx_sum_kernel(float* __restrict__ dx, const float* __restrict__ second, long n4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4 a = reinterpret_cast<float4*>(dx)[i];
    const float4 b = reinterpret_cast<const float4*>(second)[i];
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    reinterpret_cast<float4*>(dx)[i] = a;
  }
}

// argument and menu checks shared by the entry points
static int lstm_dims(const char* who, int B, int T, int K, int H, int dirs, RnnLayout* L) {
  FIL_CHECK_ARG_W(who, B >= 0 && T >= 1 && K >= 1 && H >= 1);
  FIL_CHECK_ARG_W(who, dirs == FIL_LSTM_FORWARD || dirs == FIL_LSTM_REVERSE || dirs == FIL_LSTM_BIDIR);
  return rnn_dims(who, B, T, K, H, kLstmGates, kLstmBiasRows, false, L);
}

}  // namespace fil

using namespace fil;

extern "C" int fil_lstm_plan(int B, int T, int K, int H, int dirs, int* plan) {
  RnnLayout L;
  if (int rc = lstm_dims(__func__, B, T, K, H, dirs, &L)) return rc;
  FIL_CHECK_ARG(plan != nullptr);
  tiled_plan(plan, L.NS, rnn_grid(B, L.NS), kRnnGridCap, L.lds_fwd, L.lds_bwd);
  plan[5] *= lstm_ndir(dirs);      // grid and cap count the workgroups of ONE direction; every workgroup leaves a partial
  return FIL_OK;
}

extern "C" size_t fil_lstm_saved_bytes(int B, int T, int K, int H, int dirs) {
  RnnLayout L;
  if (lstm_dims(__func__, B, T, K, H, dirs, &L) != FIL_OK) return 0;
  return align_up((size_t)lstm_ndir(dirs) * (size_t)B * (size_t)T * kLstmSaved * (size_t)H * sizeof(float), 256);
}

extern "C" int fil_lstm_fwd(const float* x, const unsigned char* mask, const float* W, const float* U, const float* b, float* hs, float* saved,
                            int B, int T, int K, int H, int dirs, void* stream) {
  RnnLayout L;
  if (int rc = lstm_dims(__func__, B, T, K, H, dirs, &L)) return rc;
  if (B == 0) return FIL_OK;
  FIL_CHECK_ARG(x != nullptr && W != nullptr && U != nullptr && b != nullptr && hs != nullptr);
  hipStream_t st = (hipStream_t)stream;
  const int ndir = lstm_ndir(dirs);
  ProfScope ps("lstm_fwd", st, 4.0 * (double)B * T * (K + ndir * (H + (saved != nullptr ? (double)kLstmSaved * H : 0.0))));
  if (int rc = tiled_allow_lds(__func__, lstm_fwd_kernel, L.lds_fwd)) return rc;
  hipLaunchKernelGGL(lstm_fwd_kernel, dim3(rnn_grid(B, L.NS), ndir), dim3(L.threads), L.lds_fwd, st, x, mask, W, U, b, hs, saved, B,
                     dirs == FIL_LSTM_REVERSE ? 1 : 0, ndir, L);
  FIL_CHECK_LAUNCH();
  return FIL_OK;
}

extern "C" size_t fil_lstm_bwd_workspace_bytes(int B, int T, int K, int H, int dirs) {
  RnnLayout L;
  if (lstm_dims(__func__, B, T, K, H, dirs, &L) != FIL_OK) return 0;
  return tiled_partial_bytes(1, lstm_workspace_floats(B, dirs, L));
}

extern "C" int fil_lstm_bwd(const float* x, const unsigned char* mask, const float* W, const float* U, const float* hs, const float* saved,
                            const float* g_hs, const float* g_last, float* dx, float* dW, float* dU, float* db, void* workspace,
                            size_t workspace_bytes, int B, int T, int K, int H, int dirs, void* stream) {
  RnnLayout L;
  if (int rc = lstm_dims(__func__, B, T, K, H, dirs, &L)) return rc;
  if (B == 0) return FIL_OK;
  FIL_CHECK_ARG(x != nullptr && W != nullptr && U != nullptr && hs != nullptr && saved != nullptr);
  FIL_CHECK_ARG(g_hs != nullptr || g_last != nullptr);
  const bool want_params = dW != nullptr || dU != nullptr || db != nullptr;
  FIL_CHECK_ARG(dx != nullptr || want_params);
  const int ndir = lstm_ndir(dirs), grid = rnn_grid(B, L.NS);
  const bool second_dx = ndir == 2 && dx != nullptr;
  if (want_params || second_dx)
    if (int rc = tiled_check_workspace(__func__, workspace, workspace_bytes, 1, lstm_workspace_floats(B, dirs, L))) return rc;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("lstm_bwd", st, 4.0 * (double)B * T * (2.0 * K + ndir * 8.0 * H));
  float* const parts = static_cast<float*>(workspace);
  float* const dx_second = second_dx ? parts + tiled_partial_bytes(ndir * grid, L.n_out) / sizeof(float) : nullptr;
  if (int rc = rnn_launch_bwd(__func__, [](auto nr) { return lstm_bwd_kernel<decltype(nr)::value>; }, L, dim3(grid, ndir), st, x, mask, W, U, hs,
                              saved, g_hs, g_last, dx, dx_second, want_params ? parts : nullptr, B, dirs == FIL_LSTM_REVERSE ? 1 : 0, ndir))
    return rc;
  FIL_CHECK_LAUNCH();
  if (second_dx) {
    const long n4 = (long)B * T * K / 4;
    hipLaunchKernelGGL(lstm_dx_sum_kernel, dim3((int)std::min<long>((n4 + 255) / 256, 2048)), dim3(256), 0, st, dx, dx_second, n4);
    FIL_CHECK_LAUNCH();
  }
  if (want_params) {
    const int off[4] = {0, K * L.HG, (K + H) * L.HG, L.n_out};
    for (int d = 0; d < ndir; ++d) {
      float* const outs[3] = {dW != nullptr ? dW + (long)d * K * L.HG : nullptr, dU != nullptr ? dU + (long)d * H * L.HG : nullptr,
                              db != nullptr ? db + (long)d * L.HG : nullptr};
      param_reduce_launch(parts + (long)d * grid * L.n_out, grid, outs, off, 3, st);
      FIL_CHECK_LAUNCH();
    }
  }
  return FIL_OK;
}
