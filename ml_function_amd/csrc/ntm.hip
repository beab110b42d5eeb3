// N4  Neural Turing Machine memory read / write over a sequence for gfx950, forward and backward, fp32 (extension: the memory of the
// Multi-channel user Interest Memory Network, "Practice on Long Sequential User Behavior Modeling for CTR Prediction", 4.1: content
// addressing by cosine similarity, one read head, one erase / add write head; the controller sees the history only).
//
//     p = h_t Wp + bp   (columns kr | kw | e | a | br | bw);   kr, kw, a = tanh;  e = sigmoid;  beta = softplus + 1
//     c_i(k) = (M_i . k) / sqrt((|M_i|^2 + eps)(|k|^2 + eps));   wr = softmax_i(beta_r c_i(kr));   ww = softmax_i(beta_w c_i(kw))
//     r_t = sum_i wr_i M_i;   M_t[i] = M_i (1 - ww_i e) + ww_i a;   a masked step carries M and r.
//
// Structure (both directions).  A workgroup owns a tile of NS samples for all T steps; LP = D / 4 lanes own one sample, a lane FOUR
// consecutive columns d of it: its 4 columns of the m memory rows sit in registers (m float4) for the whole recurrence, and every
// weight read from LDS is a float4 that feeds four columns.  h_t sits in LDS as given ([sample][H], a lane reads its sample's row as
// a broadcast), double buffered, the global loads of the next step in flight during this one (rnn_tile.h's schedule; its loads, live
// flags and staging are used as they are -- its transposed x image is not: here the lanes of a sample share a row).  The sums over d
// (M_i . k, |M_i|^2, |k|^2, the two beta columns; backward: dwr_i, dww_i) are each lane's four columns in column order, then the LP
// lanes' partials through LDS in lane order -- every lane of the sample adds them itself, in the same order, so all of them hold the
// same bits and every slot is summed in the same order.
//   forward   per step: the projection (H rows x 4 float4 of Wp), the partials -> LDS (barrier), cosine, two softmaxes, read, write;
//             rs, saved -> global (barrier).
//   backward  t = T-1 .. 0, dM (the gradient of the memory) and dr in registers; the memory before the step, the activations, the
//             weights and the cosines come from `saved`: no product and no exp is taken again.  Per step: the partials of dwr, dww
//             (barrier); the softmax, cosine and activation chains; dp -> LDS (barrier); dh_t = dp Wp^T (transposed weights);
//             [dWp ; dbp] += [h_t ; 1]^T dp in 4 x 4 register blocks over the tile's samples in sample order, NB blocks per thread
//             (barrier).  The loads of step t - 1 from `saved` are issued in front of that last phase, into the registers it leaves free.
//             dM0: the tile's samples' dM in sample order, four slots per pass through LDS, added to the workgroup's sum.
//             One partial per workgroup; param_reduce_kernel adds the partials in a fixed order.
// No atomics; every sum has a fixed order for a given shape: repeats are bit-identical, and what one sample computes depends neither
// on its place in the batch nor on B.
#include "common.h"
#include "param_reduce.h"
#include "rnn_tile.h"
#include <math.h>

namespace fil {

constexpr int kNtmMaxH = 64, kNtmMaxD = 64, kNtmMaxM = 16;
constexpr int kNtmMaxNB = 5;          // 4 x 4 blocks of [dWp ; dbp] per thread, at most
constexpr float kNtmEps = 1e-6f;

// all LDS offsets in floats (multiples of 4)
struct NtmLayout {
  int H, m, D, LP, NS, threads, P, WS, HS, Q, NB, n_blocks;
  int S, s_act, s_tail;                       // one step of `saved`: M before the step [m][D] | kr kw e a [4D] | tail [6 + 5m, padded to 4]
  int f_b, f_h, f_live, f_red, lds_fwd;       // forward:  Wp [H][WS] | bp [WS] | h [2][NS][H] | live [2][NS] | red [NS][Q][LP]
  int b_h, b_live, b_dP, b_red, b_dM0, lds_bwd;   // backward: WpT [P][H] | [h 1 0 0 0] [2][NS][HS] | live [2][NS] | dp [NS][WS] | red [NS][2m][LP] | dM0 [m][D]
  int n_out;                                  // one partial: dWp [H][P] | dbp [P] | dM0 [m][D]
  RnnLayout R;                                // what rnn_tile.h's loads read: T, K = H, NS
};

static inline NtmLayout ntm_layout(int B, int T, int H, int m, int D) {
  NtmLayout L;
  L.H = H; L.m = m; L.D = D;
  L.LP = D / 4;
  L.P = 4 * D + 2;
  L.WS = 4 * D + 4;
  L.HS = H + 4;
  L.Q = 3 * m + 4;
  const int PT = std::max(L.LP, cdiv(H, 4 * kRnnXV));          // threads per sample: a lane per four columns, and enough to stage h_t in kRnnXV pieces
  const int NSmax = kRnnThreads / PT;                          // >= 16
  const int NSmin = std::min(NSmax, cdiv(64, PT));             // a full wave where the shape allows
  const long want = ((long)B + kRnnGridCap - 1) / kRnnGridCap; // small batches: small tiles, more workgroups
  L.NS = (int)std::min((long)NSmax, std::max((long)NSmin, want));
  L.threads = (L.NS * PT + 63) / 64 * 64;
  L.n_blocks = (H / 4 + 1) * (D + 1);
  while (cdiv(L.n_blocks, L.threads) > kNtmMaxNB) L.threads += 64;      // (17 x 65 blocks over 256 threads: 5)
  L.NB = cdiv(L.n_blocks, L.threads) <= 2 ? 2 : kNtmMaxNB;
  L.s_act = m * D;
  L.s_tail = L.s_act + 4 * D;
  L.S = L.s_tail + (6 + 5 * m + 3) / 4 * 4;
  L.f_b = H * L.WS;
  L.f_h = L.f_b + L.WS;
  L.f_live = L.f_h + 2 * L.NS * H;
  L.f_red = L.f_live + (2 * L.NS + 3) / 4 * 4;
  L.lds_fwd = 4 * (L.f_red + L.NS * L.Q * L.LP);
  L.b_h = (L.P * H + 3) / 4 * 4;
  L.b_live = L.b_h + 2 * L.NS * L.HS;
  L.b_dP = L.b_live + (2 * L.NS + 3) / 4 * 4;
  L.b_red = L.b_dP + L.NS * L.WS;
  L.b_dM0 = L.b_red + (L.NS * 2 * m * L.LP + 3) / 4 * 4;
  L.lds_bwd = 4 * (L.b_dM0 + m * D);
  L.n_out = H * L.P + L.P + m * D;
  L.R = RnnLayout();
  L.R.T = T; L.R.K = H; L.R.H = D; L.R.HG = L.P; L.R.NS = L.NS; L.R.NSP = L.NS + 4; L.R.threads = L.threads;
  return L;
}

static inline int ntm_grid(int B, int NS) { return tiled_grid(B, NS, kRnnGridCap); }

__device__ __forceinline__ float ntm_dot4(const float4& a, const float4& b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }
__device__ __forceinline__ float4 ntm_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void ntm_st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void ntm_fma4(float4& acc, float s, const float4& v) {
  acc.x = fmaf(s, v.x, acc.x); acc.y = fmaf(s, v.y, acc.y); acc.z = fmaf(s, v.z, acc.z); acc.w = fmaf(s, v.w, acc.w);
}
__device__ __forceinline__ float ntm_softplus(float v) { return fmaxf(v, 0.f) + log1pf(expf(-fabsf(v))); }

// the pieces of h_t that rnn_load_x brought -> the image [NS][stride] as given
__device__ __forceinline__ void ntm_store_h(const float4 (&xr)[kRnnXV], float* img, int stride, const NtmLayout& L) {
  const int HQ = L.H / 4, n = L.NS * HQ;
#pragma unroll
  for (int i = 0; i < kRnnXV; ++i) {
    const int idx = threadIdx.x + i * blockDim.x;
    if (idx < n) {
      const int s = idx / HQ, kq = idx - s * HQ;
      ntm_st4(img + s * stride + kq * 4, xr[i]);
    }
  }
}

// the sum of the sample's LP partials of quantity q, in lane order
__device__ __forceinline__ float ntm_lane_sum(const float* red_q, int LP) {
  float v = 0.f;
  for (int l = 0; l < LP; ++l) v += red_q[l];
  return v;
}

template <int MS>
__global__ __launch_bounds__(kRnnThreads) void ntm_fwd_kernel(const float* __restrict__ h, const unsigned char* __restrict__ mask,
                                                             const float* __restrict__ Wp, const float* __restrict__ bp,
                                                             const float* __restrict__ M0, float* __restrict__ rs, float* __restrict__ r_last,
                                                             float* __restrict__ MT, float* __restrict__ saved, int B, NtmLayout L) {
  extern __shared__ __attribute__((aligned(16))) float ntm_smem[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int T = L.R.T, H = L.H, m = L.m, D = L.D, LP = L.LP, NS = L.NS, WS = L.WS, Q = L.Q;
  for (int i = tid; i < H * L.P; i += nthr) {
    const int k = i / L.P, c = i - k * L.P;
    ntm_smem[k * WS + c] = Wp[i];
  }
  rnn_stage(ntm_smem + L.f_b, bp, L.P);
  const float* Ws = ntm_smem;
  const float* bs = ntm_smem + L.f_b;
  float* red = ntm_smem + L.f_red;
  const bool active = tid < NS * LP;
  const int s = active ? tid / LP : 0, c = tid - (tid / LP) * LP, d0 = 4 * c;
  const long n_tiles = ((long)B + NS - 1) / NS;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long b0 = tile * NS, bb = b0 + s;
    float4 M[MS];
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < MS; ++i) M[i] = (active && i < m) ? ntm_ld4(M0 + i * D + d0) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 xr[kRnnXV];
    float lvn;
    __syncthreads();      // the weights are staged; the previous tile's images are free
    rnn_load_x(xr, h, mask, b0, B, 0, L.R);
    lvn = rnn_load_live(mask, b0, B, 0, L.R);
    ntm_store_h(xr, ntm_smem + L.f_h, H, L);
    if (tid < NS) ntm_smem[L.f_live + tid] = lvn;
    if (T > 1) {
      rnn_load_x(xr, h, mask, b0, B, 1, L.R);
      lvn = rnn_load_live(mask, b0, B, 1, L.R);
    }
    __syncthreads();
    for (int t = 0; t < T; ++t) {
      const int cur = t & 1, nxt = cur ^ 1;
      float4 kr, kw, e, a;
      if (active) {
        kr = ntm_ld4(bs + d0); kw = ntm_ld4(bs + D + d0); e = ntm_ld4(bs + 2 * D + d0); a = ntm_ld4(bs + 3 * D + d0);
        const float* hrow = ntm_smem + L.f_h + (cur * NS + s) * H;
#pragma unroll 4
        for (int k = 0; k < H; ++k) {
          const float hv = hrow[k];
          const float* wk = Ws + k * WS + d0;
          ntm_fma4(kr, hv, ntm_ld4(wk));
          ntm_fma4(kw, hv, ntm_ld4(wk + D));
          ntm_fma4(e, hv, ntm_ld4(wk + 2 * D));
          ntm_fma4(a, hv, ntm_ld4(wk + 3 * D));
        }
        float pbr = 0.f, pbw = 0.f;      // the lane's rows of the two beta columns
        for (int k = c; k < H; k += LP) {
          pbr = fmaf(hrow[k], Ws[k * WS + 4 * D], pbr);
          pbw = fmaf(hrow[k], Ws[k * WS + 4 * D + 1], pbw);
        }
        kr = make_float4(tanhf(kr.x), tanhf(kr.y), tanhf(kr.z), tanhf(kr.w));
        kw = make_float4(tanhf(kw.x), tanhf(kw.y), tanhf(kw.z), tanhf(kw.w));
        e = make_float4(rnn_sigmoid(e.x), rnn_sigmoid(e.y), rnn_sigmoid(e.z), rnn_sigmoid(e.w));
        a = make_float4(tanhf(a.x), tanhf(a.y), tanhf(a.z), tanhf(a.w));
        float* rd = red + (s * Q) * LP + c;
#pragma unroll
        for (int i = 0; i < MS; ++i) {
          if (i < m) {
            rd[(3 * i) * LP] = ntm_dot4(M[i], kr);
            rd[(3 * i + 1) * LP] = ntm_dot4(M[i], kw);
            rd[(3 * i + 2) * LP] = ntm_dot4(M[i], M[i]);
          }
        }
        rd[(3 * m) * LP] = ntm_dot4(kr, kr);
        rd[(3 * m + 1) * LP] = ntm_dot4(kw, kw);
        rd[(3 * m + 2) * LP] = pbr;
        rd[(3 * m + 3) * LP] = pbw;
      }
      if (t + 1 < T) {
        ntm_store_h(xr, ntm_smem + L.f_h + nxt * NS * H, H, L);
        if (tid < NS) ntm_smem[L.f_live + nxt * NS + tid] = lvn;
      }
      __syncthreads();
      if (active) {
        const bool live = ntm_smem[L.f_live + cur * NS + s] != 0.f;
        const float* rq = red + (s * Q) * LP;
        const float nkr2 = ntm_lane_sum(rq + (3 * m) * LP, LP) + kNtmEps;
        const float nkw2 = ntm_lane_sum(rq + (3 * m + 1) * LP, LP) + kNtmEps;
        const float pr = ntm_lane_sum(rq + (3 * m + 2) * LP, LP) + bs[4 * D];
        const float pw = ntm_lane_sum(rq + (3 * m + 3) * LP, LP) + bs[4 * D + 1];
        const float br = ntm_softplus(pr) + 1.f, bw = ntm_softplus(pw) + 1.f;
        float cr[MS], cw[MS], n2[MS], wr[MS], ww[MS];
        float mxr = -INFINITY, mxw = -INFINITY;
#pragma unroll
        for (int i = 0; i < MS; ++i) {
          cr[i] = cw[i] = n2[i] = 0.f;
          if (i < m) {
            n2[i] = ntm_lane_sum(rq + (3 * i + 2) * LP, LP) + kNtmEps;
            cr[i] = ntm_lane_sum(rq + (3 * i) * LP, LP) / sqrtf(n2[i] * nkr2);
            cw[i] = ntm_lane_sum(rq + (3 * i + 1) * LP, LP) / sqrtf(n2[i] * nkw2);
            mxr = fmaxf(mxr, br * cr[i]);
            mxw = fmaxf(mxw, bw * cw[i]);
          }
        }
        float sr = 0.f, sw = 0.f;
#pragma unroll
        for (int i = 0; i < MS; ++i) {
          wr[i] = ww[i] = 0.f;
          if (i < m) {
            wr[i] = expf(br * cr[i] - mxr);
            ww[i] = expf(bw * cw[i] - mxw);
            sr += wr[i];
            sw += ww[i];
          }
        }
        float4 rn = make_float4(0.f, 0.f, 0.f, 0.f);
        float* sv = saved != nullptr ? saved + (bb * T + t) * L.S : nullptr;
        const bool keep = live && sv != nullptr;
#pragma unroll
        for (int i = 0; i < MS; ++i) {
          if (i < m) {
            wr[i] /= sr;
            ww[i] /= sw;
            ntm_fma4(rn, wr[i], M[i]);
            if (keep) {
              ntm_st4(sv + i * D + d0, M[i]);
              if (c == 0) {
                float* tl = sv + L.s_tail + 6 + 5 * i;
                tl[0] = wr[i]; tl[1] = ww[i]; tl[2] = cr[i]; tl[3] = cw[i]; tl[4] = n2[i];
              }
            }
            if (live) {
              const float w = ww[i];
              M[i].x = fmaf(w, a.x, M[i].x * (1.f - w * e.x));
              M[i].y = fmaf(w, a.y, M[i].y * (1.f - w * e.y));
              M[i].z = fmaf(w, a.z, M[i].z * (1.f - w * e.z));
              M[i].w = fmaf(w, a.w, M[i].w * (1.f - w * e.w));
            }
          }
        }
        if (keep) {
          float* av = sv + L.s_act + d0;
          ntm_st4(av, kr); ntm_st4(av + D, kw); ntm_st4(av + 2 * D, e); ntm_st4(av + 3 * D, a);
          if (c == 0) {
            float* tl = sv + L.s_tail;
            tl[0] = br; tl[1] = bw; tl[2] = rnn_sigmoid(pr); tl[3] = rnn_sigmoid(pw); tl[4] = nkr2; tl[5] = nkw2;
          }
        }
        if (live) r = rn;
        if (bb < B && rs != nullptr) ntm_st4(rs + (bb * T + t) * D + d0, r);
      }
      if (t + 2 < T) {
        rnn_load_x(xr, h, mask, b0, B, t + 2, L.R);
        lvn = rnn_load_live(mask, b0, B, t + 2, L.R);
      }
      __syncthreads();
    }
    if (active && bb < B) {
      if (r_last != nullptr) ntm_st4(r_last + bb * D + d0, r);
      if (MT != nullptr) {
#pragma unroll
        for (int i = 0; i < MS; ++i)
          if (i < m) ntm_st4(MT + (bb * m + i) * D + d0, M[i]);
      }
    }
  }
}

template <int MS, int NB>
__global__ __launch_bounds__(kRnnThreads) void ntm_bwd_kernel(const float* __restrict__ h, const unsigned char* __restrict__ mask,
                                                             const float* __restrict__ Wp, const float* __restrict__ saved,
                                                             const float* __restrict__ g_rs, const float* __restrict__ g_last,
                                                             const float* __restrict__ g_M, float* __restrict__ dh,
                                                             float* __restrict__ partials, int B, NtmLayout L) {
  extern __shared__ __attribute__((aligned(16))) float ntm_smem[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int T = L.R.T, H = L.H, m = L.m, D = L.D, LP = L.LP, NS = L.NS, WS = L.WS, HS = L.HS, P = L.P;
  rnn_stage_transposed(ntm_smem, Wp, H, L.R);      // WpT [P][H]
  const float* WT = ntm_smem;
  float* dP = ntm_smem + L.b_dP;
  float* red = ntm_smem + L.b_red;
  float* dM0s = ntm_smem + L.b_dM0;
  const bool want_params = partials != nullptr;
  if (want_params) {
    for (int i = tid; i < 2 * NS; i += nthr) ntm_st4(ntm_smem + L.b_h + i * HS + H, make_float4(1.f, 0.f, 0.f, 0.f));      // the bias row's ones
    for (int i = tid; i < m * D; i += nthr) dM0s[i] = 0.f;
  }
  const bool active = tid < NS * LP;
  const int s = active ? tid / LP : 0, c = tid - (tid / LP) * LP, d0 = 4 * c;
  const int RG = H / 4 + 1, CG = D + 1;      // row and column groups of the 4 x 4 blocks of [dWp ; dbp]
  float acc[NB][4][4];
#pragma unroll
  for (int n = 0; n < NB; ++n)
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[n][a][0] = acc[n][a][1] = acc[n][a][2] = acc[n][a][3] = 0.f;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const long n_tiles = ((long)B + NS - 1) / NS;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long b0 = tile * NS, bb = b0 + s;
    const bool valid = active && bb < B;
    float4 dM[MS], Mp[MS], kr, kw, e, a, gr;
    float4 dr = (valid && g_last != nullptr) ? ntm_ld4(g_last + bb * D + d0) : zero4;
    float tl[6], wr[MS], ww[MS], cr[MS], cw[MS], n2[MS];
#pragma unroll
    for (int i = 0; i < MS; ++i) dM[i] = (valid && g_M != nullptr && i < m) ? ntm_ld4(g_M + (bb * m + i) * D + d0) : zero4;
    float4 xr[kRnnXV];
    float lvn;
    // what step tt needs from `saved` and g_rs, of the thread's sample and columns -> registers.  A masked step's block was left
    // unwritten: it is loaded (the bytes are the caller's) and never used.
    auto load_saved = [&](int tt) __attribute__((always_inline)) {
      kr = kw = e = a = gr = zero4;
#pragma unroll
      for (int i = 0; i < MS; ++i) { Mp[i] = zero4; wr[i] = ww[i] = cr[i] = cw[i] = 0.f; n2[i] = 1.f; }
#pragma unroll
      for (int q = 0; q < 6; ++q) tl[q] = 1.f;
      if (valid) {
        const float* sv = saved + (bb * T + tt) * L.S;
        const float* av = sv + L.s_act + d0;
        kr = ntm_ld4(av); kw = ntm_ld4(av + D); e = ntm_ld4(av + 2 * D); a = ntm_ld4(av + 3 * D);
#pragma unroll
        for (int q = 0; q < 6; ++q) tl[q] = sv[L.s_tail + q];
#pragma unroll
        for (int i = 0; i < MS; ++i) {
          if (i < m) {
            Mp[i] = ntm_ld4(sv + i * D + d0);
            const float* ti = sv + L.s_tail + 6 + 5 * i;
            wr[i] = ti[0]; ww[i] = ti[1]; cr[i] = ti[2]; cw[i] = ti[3]; n2[i] = ti[4];
          }
        }
        if (g_rs != nullptr) gr = ntm_ld4(g_rs + (bb * T + tt) * D + d0);
      }
    };
    __syncthreads();      // the weights are staged; the previous tile's images are free
    if (want_params) {
      rnn_load_x(xr, h, mask, b0, B, T - 1, L.R);
      ntm_store_h(xr, ntm_smem + L.b_h + ((T - 1) & 1) * NS * HS, HS, L);
    }
    lvn = rnn_load_live(mask, b0, B, T - 1, L.R);
    if (tid < NS) ntm_smem[L.b_live + ((T - 1) & 1) * NS + tid] = lvn;
    load_saved(T - 1);
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
      const int cur = t & 1;
      if (t > 0) {
        if (want_params) rnn_load_x(xr, h, mask, b0, B, t - 1, L.R);
        lvn = rnn_load_live(mask, b0, B, t - 1, L.R);
      }
      const bool live = active && ntm_smem[L.b_live + cur * NS + s] != 0.f;
      if (active) {
        dr.x += gr.x; dr.y += gr.y; dr.z += gr.z; dr.w += gr.w;
        float* rd = red + (s * 2 * m) * LP + c;
#pragma unroll
        for (int i = 0; i < MS; ++i) {
          if (i < m) {
            const float4 u = make_float4(fmaf(-Mp[i].x, e.x, a.x), fmaf(-Mp[i].y, e.y, a.y), fmaf(-Mp[i].z, e.z, a.z), fmaf(-Mp[i].w, e.w, a.w));
            rd[(2 * i) * LP] = live ? ntm_dot4(Mp[i], dr) : 0.f;
            rd[(2 * i + 1) * LP] = live ? ntm_dot4(dM[i], u) : 0.f;
          }
        }
      }
      __syncthreads();
      if (active) {
        float4 pkr = zero4, pkw = zero4, pe = zero4, pa = zero4;
        float pbr = 0.f, pbw = 0.f;
        if (live) {
          const float* rq = red + (s * 2 * m) * LP;
          const float br = tl[0], bw = tl[1], nkr2 = tl[4], nkw2 = tl[5];
          float dwr[MS], dww[MS];
          float swr = 0.f, sww = 0.f;
#pragma unroll
          for (int i = 0; i < MS; ++i) {
            dwr[i] = dww[i] = 0.f;
            if (i < m) {
              dwr[i] = ntm_lane_sum(rq + (2 * i) * LP, LP);
              dww[i] = ntm_lane_sum(rq + (2 * i + 1) * LP, LP);
              swr = fmaf(wr[i], dwr[i], swr);
              sww = fmaf(ww[i], dww[i], sww);
            }
          }
          float dbr = 0.f, dbw = 0.f;
          float4 dkr = zero4, dkw = zero4, de = zero4, da = zero4;
          float skr = 0.f, skw = 0.f;      // sum_i dc_i c_i of the two heads: the keys' own terms
#pragma unroll
          for (int i = 0; i < MS; ++i) {
            if (i < m) {
              const float dsr = wr[i] * (dwr[i] - swr), dsw = ww[i] * (dww[i] - sww);
              dbr = fmaf(dsr, cr[i], dbr);
              dbw = fmaf(dsw, cw[i], dbw);
              const float dcr = br * dsr, dcw = bw * dsw;
              const float ir = 1.f / sqrtf(n2[i] * nkr2), iw = 1.f / sqrtf(n2[i] * nkw2);
              skr = fmaf(dcr, cr[i], skr);
              skw = fmaf(dcw, cw[i], skw);
              ntm_fma4(dkr, dcr * ir, Mp[i]);
              ntm_fma4(dkw, dcw * iw, Mp[i]);
              const float w = ww[i];
              ntm_fma4(da, w, dM[i]);
              de.x = fmaf(-w * Mp[i].x, dM[i].x, de.x); de.y = fmaf(-w * Mp[i].y, dM[i].y, de.y);
              de.z = fmaf(-w * Mp[i].z, dM[i].z, de.z); de.w = fmaf(-w * Mp[i].w, dM[i].w, de.w);
              // dM_i = dM'_i (1 - ww_i e) + wr_i dr + dcr_i (kr / (nM nkr) - cr_i M_i / nM^2) + the same of the write head
              const float back = -(dcr * cr[i] + dcw * cw[i]) / n2[i];
              float4 v = make_float4(dM[i].x * (1.f - w * e.x), dM[i].y * (1.f - w * e.y), dM[i].z * (1.f - w * e.z), dM[i].w * (1.f - w * e.w));
              ntm_fma4(v, wr[i], dr);
              ntm_fma4(v, dcr * ir, kr);
              ntm_fma4(v, dcw * iw, kw);
              ntm_fma4(v, back, Mp[i]);
              dM[i] = v;
            }
          }
          ntm_fma4(dkr, -skr / nkr2, kr);
          ntm_fma4(dkw, -skw / nkw2, kw);
          pkr = make_float4(dkr.x * (1.f - kr.x * kr.x), dkr.y * (1.f - kr.y * kr.y), dkr.z * (1.f - kr.z * kr.z), dkr.w * (1.f - kr.w * kr.w));
          pkw = make_float4(dkw.x * (1.f - kw.x * kw.x), dkw.y * (1.f - kw.y * kw.y), dkw.z * (1.f - kw.z * kw.z), dkw.w * (1.f - kw.w * kw.w));
          pe = make_float4(de.x * e.x * (1.f - e.x), de.y * e.y * (1.f - e.y), de.z * e.z * (1.f - e.z), de.w * e.w * (1.f - e.w));
          pa = make_float4(da.x * (1.f - a.x * a.x), da.y * (1.f - a.y * a.y), da.z * (1.f - a.z * a.z), da.w * (1.f - a.w * a.w));
          pbr = dbr * tl[2];
          pbw = dbw * tl[3];
          dr = zero4;      // the read is replaced at a live step: nothing of dr goes further back
        }
        float* dp = dP + s * WS + d0;
        ntm_st4(dp, pkr); ntm_st4(dp + D, pkw); ntm_st4(dp + 2 * D, pe); ntm_st4(dp + 3 * D, pa);
        if (c == 0) ntm_st4(dP + s * WS + 4 * D, make_float4(pbr, pbw, 0.f, 0.f));
      }
      __syncthreads();
      // the loads of the step before, into the registers this step is done with
      if (t > 0) load_saved(t - 1);
      if (active && dh != nullptr && bb < B) {
        const float* dps = dP + s * WS;
        for (int oc = c; oc < H / 4; oc += LP) {
          float4 v = zero4;
#pragma unroll 2
          for (int col = 0; col < 4 * D; col += 4) {
            const float4 d = ntm_ld4(dps + col);
            ntm_fma4(v, d.x, ntm_ld4(WT + col * H + 4 * oc));
            ntm_fma4(v, d.y, ntm_ld4(WT + (col + 1) * H + 4 * oc));
            ntm_fma4(v, d.z, ntm_ld4(WT + (col + 2) * H + 4 * oc));
            ntm_fma4(v, d.w, ntm_ld4(WT + (col + 3) * H + 4 * oc));
          }
          ntm_fma4(v, dps[4 * D], ntm_ld4(WT + (4 * D) * H + 4 * oc));
          ntm_fma4(v, dps[4 * D + 1], ntm_ld4(WT + (4 * D + 1) * H + 4 * oc));
          if (!live) v = zero4;
          ntm_st4(dh + (bb * T + t) * H + 4 * oc, v);
        }
      }
      if (want_params) {
        const float* hS = ntm_smem + L.b_h + cur * NS * HS;
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          const int blk = tid + n * nthr;
          if (blk < L.n_blocks) {
            const int rg = blk / CG, cg = blk - rg * CG;
            for (int ss = 0; ss < NS; ++ss) {
              const float4 hv = ntm_ld4(hS + ss * HS + 4 * rg);
              const float4 dv = ntm_ld4(dP + ss * WS + 4 * cg);
              const float he[4] = {hv.x, hv.y, hv.z, hv.w}, de4[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
              for (int a2 = 0; a2 < 4; ++a2)
#pragma unroll
                for (int c2 = 0; c2 < 4; ++c2) acc[n][a2][c2] = fmaf(he[a2], de4[c2], acc[n][a2][c2]);
            }
          }
        }
      }
      if (t > 0) {
        if (want_params) ntm_store_h(xr, ntm_smem + L.b_h + (cur ^ 1) * NS * HS, HS, L);
        if (tid < NS) ntm_smem[L.b_live + (cur ^ 1) * NS + tid] = lvn;
      }
      __syncthreads();
    }
    // dM0 += the tile's samples' dM, four slots per pass through the dp image (free now), in sample order
    if (want_params) {
      for (int i0 = 0; i0 < m; i0 += 4) {
#pragma unroll
        for (int i = 0; i < MS; ++i)
          if (active && i >= i0 && i < i0 + 4 && i < m) ntm_st4(dP + s * WS + (i - i0) * D + d0, dM[i]);
        __syncthreads();
        const int n = (m - i0 < 4 ? m - i0 : 4) * D;
        for (int o = tid; o < n; o += nthr) {
          float sum = 0.f;
          for (int ss = 0; ss < NS; ++ss) sum += dP[ss * WS + o];
          dM0s[i0 * D + o] += sum;
        }
        __syncthreads();
      }
    }
  }
  if (!want_params) return;
  float* part = partials + (long)blockIdx.x * L.n_out;
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int blk = tid + n * nthr;
    if (blk < L.n_blocks) {
      const int rg = blk / CG, cg = blk - rg * CG;
#pragma unroll
      for (int a2 = 0; a2 < 4; ++a2) {
        const int row = 4 * rg + a2;      // row H is dbp: it follows dWp in the partial
        if (row <= H) {
#pragma unroll
          for (int c2 = 0; c2 < 4; ++c2)
            if (4 * cg + c2 < P) part[row * P + 4 * cg + c2] = acc[n][a2][c2];
        }
      }
    }
  }
  for (int i = tid; i < m * D; i += nthr) part[(H + 1) * P + i] = dM0s[i];
}

// argument and menu checks shared by the entry points, and the layout
static int ntm_dims(const char* who, int B, int T, int H, int m, int D, NtmLayout* L) {
  FIL_CHECK_ARG_W(who, B >= 0 && T >= 1 && H >= 1 && m >= 1 && D >= 1);
  if (H % 4 != 0 || H > kNtmMaxH) return fail(FIL_ERR_UNSUPPORTED, "%s: H=%d needs H %% 4 == 0 and H <= %d", who, H, kNtmMaxH);
  if (D % 4 != 0 || D > kNtmMaxD) return fail(FIL_ERR_UNSUPPORTED, "%s: D=%d needs D %% 4 == 0 and D <= %d", who, D, kNtmMaxD);
  if (m > kNtmMaxM) return fail(FIL_ERR_UNSUPPORTED, "%s: m=%d needs m <= %d", who, m, kNtmMaxM);
  *L = ntm_layout(B, T, H, m, D);
  if (L->lds_fwd > kTiledLdsLimit || L->lds_bwd > kTiledLdsLimit)
    return fail(FIL_ERR_UNSUPPORTED, "%s: H=%d m=%d D=%d needs %d bytes of LDS (limit %d)", who, H, m, D, std::max(L->lds_fwd, L->lds_bwd),
                kTiledLdsLimit);
  return FIL_OK;
}

// launches the instantiation that the slot count (and the layout's NB) selects; `kernel_of(ms)` returns it for
// ms = std::integral_constant<int, 4 | 8 | 16>
template <typename KernelOf, typename... Args>
static int ntm_launch(const char* who, KernelOf kernel_of, const NtmLayout& L, int lds, dim3 grid, hipStream_t st, Args... args) {
  auto launch = [&](auto ms) -> int {
    auto kernel = kernel_of(ms);
    if (int rc = tiled_allow_lds(who, kernel, lds)) return rc;
    hipLaunchKernelGGL(kernel, grid, dim3(L.threads), lds, st, args..., L);
    return FIL_OK;
  };
  return L.m <= 4 ? launch(std::integral_constant<int, 4>())
                  : (L.m <= 8 ? launch(std::integral_constant<int, 8>()) : launch(std::integral_constant<int, 16>()));
}

}  // namespace fil

using namespace fil;

extern "C" int fil_ntm_plan(int B, int T, int H, int m, int D, int* plan) {
  NtmLayout L;
  if (int rc = ntm_dims(__func__, B, T, H, m, D, &L)) return rc;
  FIL_CHECK_ARG(plan != nullptr);
  tiled_plan(plan, L.NS, ntm_grid(B, L.NS), kRnnGridCap, L.lds_fwd, L.lds_bwd);
  return FIL_OK;
}

extern "C" size_t fil_ntm_saved_bytes(int B, int T, int H, int m, int D) {
  NtmLayout L;
  if (ntm_dims(__func__, B, T, H, m, D, &L) != FIL_OK) return 0;
  return align_up((size_t)B * (size_t)T * (size_t)L.S * sizeof(float), 256);
}

extern "C" int fil_ntm_fwd(const float* h, const unsigned char* mask, const float* Wp, const float* bp, const float* M0, float* rs,
                           float* r_last, float* MT, float* saved, int B, int T, int H, int m, int D, void* stream) {
  NtmLayout L;
  if (int rc = ntm_dims(__func__, B, T, H, m, D, &L)) return rc;
  if (B == 0) return FIL_OK;
  FIL_CHECK_ARG(h != nullptr && Wp != nullptr && bp != nullptr && M0 != nullptr);
  FIL_CHECK_ARG(rs != nullptr || r_last != nullptr || MT != nullptr);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("ntm_fwd", st, 4.0 * (double)B * T * (H + D + (saved != nullptr ? (double)L.S : 0.0)));
  if (int rc = ntm_launch(__func__, [](auto ms) { return ntm_fwd_kernel<decltype(ms)::value>; }, L, L.lds_fwd, dim3(ntm_grid(B, L.NS)), st, h,
                          mask, Wp, bp, M0, rs, r_last, MT, saved, B))
    return rc;
  FIL_CHECK_LAUNCH();
  return FIL_OK;
}

extern "C" size_t fil_ntm_bwd_workspace_bytes(int B, int T, int H, int m, int D) {
  NtmLayout L;
  if (ntm_dims(__func__, B, T, H, m, D, &L) != FIL_OK) return 0;
  return tiled_partial_bytes(ntm_grid(B, L.NS), L.n_out);
}

extern "C" int fil_ntm_bwd(const float* h, const unsigned char* mask, const float* Wp, const float* saved, const float* g_rs,
                           const float* g_last, const float* g_M, float* dh, float* dWp, float* dbp, float* dM0, void* workspace,
                           size_t workspace_bytes, int B, int T, int H, int m, int D, void* stream) {
  NtmLayout L;
  if (int rc = ntm_dims(__func__, B, T, H, m, D, &L)) return rc;
  if (B == 0) return FIL_OK;
  FIL_CHECK_ARG(h != nullptr && Wp != nullptr && saved != nullptr);
  FIL_CHECK_ARG(g_rs != nullptr || g_last != nullptr || g_M != nullptr);
  const bool want_params = dWp != nullptr || dbp != nullptr || dM0 != nullptr;
  FIL_CHECK_ARG(dh != nullptr || want_params);
  const int nparts = ntm_grid(B, L.NS);
  if (want_params)
    if (int rc = tiled_check_workspace(__func__, workspace, workspace_bytes, nparts, L.n_out)) return rc;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("ntm_bwd", st, 4.0 * (double)B * T * (2.0 * H + D + (double)L.S));
  float* parts = want_params ? static_cast<float*>(workspace) : nullptr;
  auto kernel_of = [&](auto ms) {
    constexpr int MS = decltype(ms)::value;
    return L.NB == 2 ? ntm_bwd_kernel<MS, 2> : ntm_bwd_kernel<MS, kNtmMaxNB>;
  };
  if (int rc = ntm_launch(__func__, kernel_of, L, L.lds_bwd, dim3(nparts), st, h, mask, Wp, saved, g_rs, g_last, g_M, dh, parts, B)) return rc;
  FIL_CHECK_LAUNCH();
  if (want_params) {
    float* const outs[3] = {dWp, dbp, dM0};
    const int off[4] = {0, H * L.P, (H + 1) * L.P, L.n_out};
    param_reduce_launch(static_cast<const float*>(workspace), nparts, outs, off, 3, st);
    FIL_CHECK_LAUNCH();
  }
  return FIL_OK;
}
