// N3  GRU / AUGRU / AGRU over a behaviour sequence for gfx950, forward and backward, fp32 (extension: the interest extraction and
// interest evolution layers of the Deep Interest Evolution Network; the GRU is TF 2 Keras' GRU with its defaults, reset_after=True).
//
//     xp = x_t W + b[0];  hp = h U + b[1]                        (columns z | r | h)
//     z = sigmoid(xp_z + hp_z);  r = sigmoid(xp_r + hp_r);  c = tanh(xp_h + r hp_h);  u = 1 - z
//     u' = u (GRU) | a_t u (AUGRU) | a_t (AGRU);   h_new = (1 - u') h + u' c;   a masked step carries h.
//
// Structure (both directions): rnn_tile.h's sample-quad tiling and schedule, with three gates, two bias rows and the scores.
//   forward   per step: 3 (K + H) weight reads + (K + H) state reads for 12 (K + H) FMAs per thread; the gates; hs, saved -> global;
//             the new state -> LDS.  One barrier.
//   backward  t = T-1 .. 0, dh (the gradient of the state) in registers.  Per step:
//             1  the gate gradients of the thread's unit and samples from `saved` -> LDS, both [column][sample] and [sample][column];
//                the da terms -> LDS.                                                                               (barrier)
//             2  dh_prev = dh (1 - u') + d_hp U^T, dx_t = d_xp W^T (transposed weights, lanes = consecutive outputs);
//                da[b,t] = the units' terms added in unit order;
//                dW / dU: the thread's three columns (the gates of its unit) of the rows g, g + G, ... of [x_t ; h_prev]^T [d_xp | d_hp],
//                summed over the tile's samples in sample order, in registers over all steps and tiles (NR x 3 accumulators, NR <= 32). (barrier)
//             One partial per workgroup; param_reduce_kernel adds the partials in a fixed order.
// No atomics; every sum has a fixed order for a given shape: repeats are bit-identical.
#include "common.h"
#include "param_reduce.h"
#include "rnn_tile.h"
#include <math.h>

namespace fil {

constexpr int kGruGates = 3, kGruBiasRows = 2;

// live flag (1 / 0) and score of sample b0 + threadIdx.x at step t (threads below NS)
__device__ __forceinline__ void gru_load_step(float& lv, float& av, const float* __restrict__ a, const unsigned char* __restrict__ mask, long b0,
                                              int B, int t, const RnnLayout& L) {
  lv = 0.f; av = 0.f;
  if ((int)threadIdx.x < L.NS) {
    const long bb = b0 + threadIdx.x;
    if (bb < B && (mask == nullptr || mask[bb * L.T + t] != 0)) {
      lv = 1.f;
      av = a != nullptr ? a[bb * L.T + t] : 1.f;
    }
  }
}

__global__ __launch_bounds__(kRnnThreads) void gru_fwd_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                             const unsigned char* __restrict__ mask, const float* __restrict__ W,
                                                             const float* __restrict__ U, const float* __restrict__ bias, float* __restrict__ hs,
                                                             float* __restrict__ saved, int B, int mode, RnnLayout L) {
  extern __shared__ __attribute__((aligned(16))) float gru_smem[];
  const int tid = threadIdx.x;
  const int T = L.T, K = L.K, H = L.H, H3 = L.HG, NS = L.NS, NSP = L.NSP;
  rnn_stage(gru_smem, W, K * H3);
  rnn_stage(gru_smem + L.f_U, U, H * H3);
  rnn_stage(gru_smem + L.f_b, bias, kGruBiasRows * H3);
  const float* Ws = gru_smem;
  const float* Us = gru_smem + L.f_U;
  const float* bs = gru_smem + L.f_b;
  const bool active = tid < L.G * H;
  const int g = tid / H, j = tid - g * H;
  const long n_tiles = ((long)B + NS - 1) / NS;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long b0 = tile * NS;
    float h[4] = {0.f, 0.f, 0.f, 0.f};
    float4 xr[kRnnXV];
    float lvn, avn;
    __syncthreads();      // the weights are staged; the previous tile's images are free
    rnn_load_x(xr, x, mask, b0, B, 0, L);
    gru_load_step(lvn, avn, a, mask, b0, B, 0, L);
    rnn_store_x(xr, gru_smem + L.f_x, L);
    if (tid < NS) { gru_smem[L.f_live + tid] = lvn; gru_smem[L.f_a + tid] = avn; }
    if (active) *reinterpret_cast<float4*>(gru_smem + L.f_h + j * NSP + 4 * g) = make_float4(0.f, 0.f, 0.f, 0.f);
    if (T > 1) {
      rnn_load_x(xr, x, mask, b0, B, 1, L);
      gru_load_step(lvn, avn, a, mask, b0, B, 1, L);
    }
    __syncthreads();
    // the order within a step: rnn_tile.h, Schedule
    for (int t = 0; t < T; ++t) {
      const int cur = t & 1, nxt = cur ^ 1;
      float zv[4], rv[4], cv[4], pv[4];
      bool lv[4] = {false, false, false, false};
      if (active) {
        float ax[3][4], ah[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float bx = bs[c * H + j], bh = bs[H3 + c * H + j];
#pragma unroll
          for (int e = 0; e < 4; ++e) { ax[c][e] = bx; ah[c][e] = bh; }
        }
        const float* xc = gru_smem + L.f_x + cur * K * NSP + 4 * g;
        const float* hc = gru_smem + L.f_h + cur * H * NSP + 4 * g;
        rnn_fwd_products(ax, xc, Ws, K, j, L);
        rnn_fwd_products(ah, hc, Us, H, j, L);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int s = 4 * g + e;
          lv[e] = gru_smem[L.f_live + cur * NS + s] != 0.f;
          const float at = gru_smem[L.f_a + cur * NS + s];
          const float z = rnn_sigmoid(ax[0][e] + ah[0][e]);
          const float r = rnn_sigmoid(ax[1][e] + ah[1][e]);
          const float c = tanhf(ax[2][e] + r * ah[2][e]);
          const float u = 1.f - z;
          const float up = mode == FIL_GRU_AGRU ? at : (mode == FIL_GRU_AUGRU ? at * u : u);
          const float hn = fmaf(up, c, (1.f - up) * h[e]);
          if (lv[e]) h[e] = hn;
          zv[e] = z; rv[e] = r; cv[e] = c; pv[e] = ah[2][e];
        }
        *reinterpret_cast<float4*>(gru_smem + L.f_h + nxt * H * NSP + j * NSP + 4 * g) = make_float4(h[0], h[1], h[2], h[3]);
      }
      if (t + 1 < T) {
        rnn_store_x(xr, gru_smem + L.f_x + nxt * K * NSP, L);
        if (tid < NS) { gru_smem[L.f_live + nxt * NS + tid] = lvn; gru_smem[L.f_a + nxt * NS + tid] = avn; }
      }
      if (active) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long bb = b0 + 4 * g + e;
          if (lv[e] && saved != nullptr) {
            float* sv = saved + ((bb * T + t) * 4) * H + j;
            sv[0] = zv[e]; sv[H] = rv[e]; sv[2 * H] = cv[e]; sv[3 * H] = pv[e];
          }
          if (bb < B) hs[(bb * T + t) * H + j] = h[e];
        }
      }
      if (t + 2 < T) {
        rnn_load_x(xr, x, mask, b0, B, t + 2, L);
        gru_load_step(lvn, avn, a, mask, b0, B, t + 2, L);
      }
      __syncthreads();
    }
  }
}

template <int NR>
__global__ __launch_bounds__(kRnnThreads) void gru_bwd_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                             const unsigned char* __restrict__ mask, const float* __restrict__ W,
                                                             const float* __restrict__ U, const float* __restrict__ hs,
                                                             const float* __restrict__ saved, const float* __restrict__ g_hs,
                                                             const float* __restrict__ g_last, float* __restrict__ dx, float* __restrict__ da,
                                                             float* __restrict__ partials, int B, int mode, RnnLayout L) {
  extern __shared__ __attribute__((aligned(16))) float gru_smem[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int T = L.T, K = L.K, H = L.H, H3 = L.HG, NS = L.NS, NSP = L.NSP, G = L.G, KH = L.K + L.H;
  rnn_stage_transposed(gru_smem, W, K, L);
  rnn_stage_transposed(gru_smem + L.b_UT, U, H, L);
  const float* WT = gru_smem;
  const float* UT = gru_smem + L.b_UT;
  float* dT = gru_smem + L.b_dT;
  float* dS = gru_smem + L.b_dS;
  float* daS = gru_smem + L.b_da;
  const bool active = tid < G * H;
  const int g = tid / H, j = tid - g * H;
  const bool want_params = partials != nullptr;
  float acc[NR][kGruGates];
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 0.f;
  float dbs[4] = {0.f, 0.f, 0.f, 0.f};      // the thread's samples' dz, dr, dc (input side), dc r (recurrent side)
  const long n_tiles = ((long)B + NS - 1) / NS;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long b0 = tile * NS;
    float dh[4] = {0.f, 0.f, 0.f, 0.f};
    float svn[4][4], hpn[4], ghn[4], lvn, avn;
    float4 xr[kRnnXV];
    // what step tt needs, of the thread's unit and samples -> registers
    auto prefetch = [&](int tt) {
      if (want_params) rnn_load_x(xr, x, mask, b0, B, tt, L);
      gru_load_step(lvn, avn, a, mask, b0, B, tt, L);
      if (active) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long bb = b0 + 4 * g + e;
          const bool valid = bb < B;
          const bool live = valid && (mask == nullptr || mask[bb * T + tt] != 0);
          const float* sv = saved + ((bb * T + tt) * 4) * H + j;
#pragma unroll
          for (int c = 0; c < 4; ++c) svn[e][c] = live ? sv[c * H] : 0.f;
          hpn[e] = (live && tt > 0) ? hs[(bb * T + tt - 1) * H + j] : 0.f;
          ghn[e] = (valid && g_hs != nullptr) ? g_hs[(bb * T + tt) * H + j] : 0.f;
        }
      }
    };
    float sv[4][4], hp[4], gh[4];
    // ... -> the LDS images of buffer `buf` and the registers of the current step
    auto commit = [&](int buf) {
      float* inT = gru_smem + L.b_in + buf * KH * NSP;
      if (want_params) {
        rnn_store_x(xr, inT, L);
        if (active) *reinterpret_cast<float4*>(inT + (K + j) * NSP + 4 * g) = make_float4(hpn[0], hpn[1], hpn[2], hpn[3]);
      }
      if (tid < NS) { gru_smem[L.b_live + buf * NS + tid] = lvn; gru_smem[L.b_a + buf * NS + tid] = avn; }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int c = 0; c < 4; ++c) sv[e][c] = svn[e][c];
        hp[e] = hpn[e];
        gh[e] = ghn[e];
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
    for (int t = T - 1; t >= 0; --t) {
      const int cur = t & 1;
      if (t > 0) prefetch(t - 1);
      float keep[4] = {0.f, 0.f, 0.f, 0.f};
      if (active) {
        // phase 1: the gate gradients of (unit j, the quad's samples)
        float dz[4], dr[4], dcx[4], dch[4], dat[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int s = 4 * g + e;
          const bool live = gru_smem[L.b_live + cur * NS + s] != 0.f;
          const float at = gru_smem[L.b_a + cur * NS + s];
          if (g_hs != nullptr) dh[e] += gh[e];
          const float z = sv[e][0], r = sv[e][1], c = sv[e][2], hph = sv[e][3];
          const float u = 1.f - z;
          const float up = mode == FIL_GRU_AGRU ? at : (mode == FIL_GRU_AUGRU ? at * u : u);
          const float dup = dh[e] * (c - hp[e]);
          const float du = mode == FIL_GRU_AGRU ? 0.f : (mode == FIL_GRU_AUGRU ? at * dup : dup);
          const float dcp = (dh[e] * up) * (1.f - c * c);
          dz[e] = live ? -du * (z * (1.f - z)) : 0.f;
          dr[e] = live ? (dcp * hph) * (r * (1.f - r)) : 0.f;
          dcx[e] = live ? dcp : 0.f;
          dch[e] = live ? dcp * r : 0.f;
          dat[e] = live ? (mode == FIL_GRU_AGRU ? dup : dup * u) : 0.f;
          keep[e] = live ? dh[e] * (1.f - up) : dh[e];
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
        if (da != nullptr) *reinterpret_cast<float4*>(daS + j * NSP + 4 * g) = make_float4(dat[0], dat[1], dat[2], dat[3]);
      }
      __syncthreads();
      // phase 2
      if (active) {
        // dh_prev = dh (1 - u') + d_hp U^T: rows z, r of dT, then the recurrent side's dc r
        float nh[4] = {0.f, 0.f, 0.f, 0.f};
        if (t > 0) rnn_bwd_matvec<true>(nh, dT + 4 * g, UT, H, j, L);
#pragma unroll
        for (int e = 0; e < 4; ++e) dh[e] = keep[e] + nh[e];
        if (want_params) rnn_bwd_accumulate(acc, gru_smem + L.b_in + cur * KH * NSP, dS, g, j, L);
      }
      // the registers loaded at the top of the step -> LDS BEFORE this step's stores are issued (rnn_tile.h, Schedule)
      if (t > 0) commit((t - 1) & 1);
      if (da != nullptr && tid < NS) {
        const long bb = b0 + tid;
        if (bb < B) {
          float sum = 0.f;
          for (int jj = 0; jj < H; ++jj) sum += daS[jj * NSP + tid];
          da[bb * T + t] = sum;
        }
      }
      if (active && dx != nullptr) rnn_bwd_dx(dx, dT + 4 * g, WT, gru_smem + L.b_live + cur * NS + 4 * g, b0 + 4 * g, B, t, j, L);
      __syncthreads();
    }
  }
  if (!want_params) return;
  // the workgroup's partial; db = the four sums on the two bias rows: dz, dr on both, dc on the input side's, dc r on the recurrent side's
  float* part = partials + (long)blockIdx.x * L.n_out;
  rnn_bwd_write_partial(part, acc, dbs, dS, active, g, j, L);
  for (int o = tid; o < 4 * H; o += nthr) {
    const int c = o / H, jj = o - c * H;
    const float sum = rnn_bwd_quad_sum(dS, o, L);
    float* db = part + KH * H3;
    if (c < 2) { db[c * H + jj] = sum; db[H3 + c * H + jj] = sum; }
    else if (c == 2) db[2 * H + jj] = sum;
    else db[H3 + 2 * H + jj] = sum;
  }
}

// argument and menu checks shared by the entry points
static int gru_dims(const char* who, int B, int T, int K, int H, int mode, RnnLayout* L) {
  FIL_CHECK_ARG_W(who, B >= 0 && T >= 1 && K >= 1 && H >= 1);
  FIL_CHECK_ARG_W(who, mode == FIL_GRU_GRU || mode == FIL_GRU_AUGRU || mode == FIL_GRU_AGRU);
  return rnn_dims(who, B, T, K, H, kGruGates, kGruBiasRows, true, L);
}

}  // namespace fil

using namespace fil;

extern "C" int fil_gru_plan(int B, int T, int K, int H, int mode, int* plan) {
  RnnLayout L;
  if (int rc = gru_dims(__func__, B, T, K, H, mode, &L)) return rc;
  FIL_CHECK_ARG(plan != nullptr);
  tiled_plan(plan, L.NS, rnn_grid(B, L.NS), kRnnGridCap, L.lds_fwd, L.lds_bwd);
  return FIL_OK;
}

extern "C" size_t fil_gru_saved_bytes(int B, int T, int K, int H) {
  RnnLayout L;
  if (gru_dims(__func__, B, T, K, H, FIL_GRU_GRU, &L) != FIL_OK) return 0;
  return align_up((size_t)B * (size_t)T * 4 * (size_t)H * sizeof(float), 256);
}

extern "C" int fil_gru_fwd(const float* x, const float* a, const unsigned char* mask, const float* W, const float* U, const float* b,
                           float* hs, float* saved, int B, int T, int K, int H, int mode, void* stream) {
  RnnLayout L;
  if (int rc = gru_dims(__func__, B, T, K, H, mode, &L)) return rc;
  if (B == 0) return FIL_OK;
  FIL_CHECK_ARG(x != nullptr && W != nullptr && U != nullptr && b != nullptr && hs != nullptr);
  FIL_CHECK_ARG((mode == FIL_GRU_GRU) == (a == nullptr));
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("gru_fwd", st, 4.0 * (double)B * T * (K + H + (saved != nullptr ? 4.0 * H : 0.0)));
  if (int rc = tiled_allow_lds(__func__, gru_fwd_kernel, L.lds_fwd)) return rc;
  hipLaunchKernelGGL(gru_fwd_kernel, dim3(rnn_grid(B, L.NS)), dim3(L.threads), L.lds_fwd, st, x, a, mask, W, U, b, hs, saved, B, mode, L);
  FIL_CHECK_LAUNCH();
  return FIL_OK;
}

extern "C" size_t fil_gru_bwd_workspace_bytes(int B, int T, int K, int H) {
  RnnLayout L;
  if (gru_dims(__func__, B, T, K, H, FIL_GRU_GRU, &L) != FIL_OK) return 0;
  return tiled_partial_bytes(rnn_grid(B, L.NS), L.n_out);
}

extern "C" int fil_gru_bwd(const float* x, const float* a, const unsigned char* mask, const float* W, const float* U, const float* hs,
                           const float* saved, const float* g_hs, const float* g_last, float* dx, float* da, float* dW, float* dU, float* db,
                           void* workspace, size_t workspace_bytes, int B, int T, int K, int H, int mode, void* stream) {
  RnnLayout L;
  if (int rc = gru_dims(__func__, B, T, K, H, mode, &L)) return rc;
  if (B == 0) return FIL_OK;
  FIL_CHECK_ARG(x != nullptr && W != nullptr && U != nullptr && hs != nullptr && saved != nullptr);
  FIL_CHECK_ARG((mode == FIL_GRU_GRU) == (a == nullptr));
  FIL_CHECK_ARG(g_hs != nullptr || g_last != nullptr);
  FIL_CHECK_ARG(da == nullptr || mode != FIL_GRU_GRU);
  const bool want_params = dW != nullptr || dU != nullptr || db != nullptr;
  FIL_CHECK_ARG(dx != nullptr || da != nullptr || want_params);
  const int nparts = rnn_grid(B, L.NS);
  if (want_params)
    if (int rc = tiled_check_workspace(__func__, workspace, workspace_bytes, nparts, L.n_out)) return rc;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("gru_bwd", st, 4.0 * (double)B * T * (2.0 * K + 6.0 * H));
  if (int rc = rnn_launch_bwd(__func__, [](auto nr) { return gru_bwd_kernel<decltype(nr)::value>; }, L, dim3(nparts), st, x, a, mask, W, U, hs,
                              saved, g_hs, g_last, dx, da, want_params ? static_cast<float*>(workspace) : nullptr, B, mode))
    return rc;
  FIL_CHECK_LAUNCH();
  if (want_params) {
    float* const outs[3] = {dW, dU, db};
    const int off[4] = {0, K * L.HG, (K + H) * L.HG, L.n_out};
    param_reduce_launch(static_cast<const float*>(workspace), nparts, outs, off, 3, st);
    FIL_CHECK_LAUNCH();
  }
  return FIL_OK;
}
