// N3  AFM pair-attention pooling (softmax over the PAIRS) for gfx950, forward and backward, fp32.
//
// The paper's attention pooling over the P = F(F-1)/2 pair products x_p = e_i * e_j of a sample's field embeddings (the reference's
// AttentionBaseLayer takes its softmax over a size-1 axis instead, interactive_layer.py:357-364; that quirk stays the default of the
// layers and is not computed here):
//     u_p = x_p W + b,   s_p = relu(u_p . h)  (reference op order)  or  relu(u_p) . h  (flag bit 0, the paper's form),
//     a = softmax_p(s),  pooled = sum_p a_p x_p.
// Nothing of size B P leaves the chip in either direction: per sample the kernels read the [F,K] slab (backward: also g, pooled and
// the two softmax statistics) and write [K] (backward: [F,K]).
//
// Structure (both directions): a workgroup is NW <= 4 waves, a wave owns whole samples (grid-stride over tiles of NW samples) and has
// its own LDS region; W (transposed, zero-padded to AT = 4 or 16 columns), b, h and the pair table (i, j of every p in
// itertools.combinations order) are staged ONCE per workgroup.  The slab's rows sit in LDS at a stride of KP dwords with KP/4 odd, so
// that lanes reading 16-byte pieces of consecutive rows fall on different bank groups.
//   forward   pass 1: lane = pair: u_p, s_p -> LDS, wave max, exp, wave sum.  pass 2: lane = (k quad, pair group): the weighted sum
//             of the pair products, group partials summed in group order, ONE division by the softmax denominator.
//   backward  phase A: lane = pair: s_p again (same code, same bits), a_p, ds_p = a_p (g.x_p - g.pooled), du_p -> LDS; db, dh in
//             registers.  phase B: lane = (field, k): de[f,k] = sum over the partners j of (a_p g_k + (W du_p)_k) e_j[k] in ascending
//             j -- no two lanes add into one de element.  phase C: lane = (k, pair group): dW[k,:] += x_p[k] du_p in registers.
//             The parameter gradients stay in registers over all samples of a wave, are summed over the workgroup's waves in a fixed
//             order and leave as ONE partial per workgroup; param_reduce_kernel then adds the partials in a fixed order.
// No atomics; every sum has a fixed order for a given B, so repeats are bit-identical.
#include "common.h"
#include "param_reduce.h"
#include "tiled_launch.h"
#include <algorithm>
#include <math.h>

namespace fil {

constexpr int kAfmMaxWaves = 4;        // waves (= samples in flight) per workgroup
constexpr int kAfmGridCap = 512;       // workgroups per launch: two per CU
constexpr int kAfmMaxF = 64, kAfmMaxK = 64, kAfmMaxA = 16;

// LDS layout, all offsets in floats (multiples of 4: every region is read in 16-byte pieces).
//   shared by the workgroup: Wt [AT][K] | b [AT] | h [AT] | pair table [P] (16-bit: i | j << 8)
//   per wave, forward:  e [F][KP] | scores [P] | group partials [64/KQ][K]
//   per wave, backward: e [F][KP] | g [K] | pooled [K] | a [P] | du [P][AT]
struct AfmLayout {
  int F, K, A, AT, P, KP, KQ, NW;
  int o_b, o_h, o_pair, shared_f;
  int o_sc, o_red, wave_fwd;
  int o_g, o_p, o_a, o_du, wave_bwd;
  int lds_fwd, lds_bwd;   // bytes
};

static inline int afm_al4(int v) { return (v + 3) / 4 * 4; }

static AfmLayout afm_layout(int F, int K, int A, int NW) {
  AfmLayout L;
  L.F = F; L.K = K; L.A = A;
  L.AT = A <= 4 ? 4 : 16;
  L.P = F * (F - 1) / 2;
  L.KQ = K / 4;
  L.KP = (L.KQ % 2 == 0) ? K + 4 : K;
  L.NW = NW;
  L.o_b = L.AT * K;
  L.o_h = L.o_b + L.AT;
  L.o_pair = L.o_h + L.AT;
  L.shared_f = L.o_pair + afm_al4((L.P + 1) / 2);
  const int e_f = F * L.KP;
  L.o_sc = e_f;
  L.o_red = L.o_sc + afm_al4(L.P);
  L.wave_fwd = L.o_red + (64 / L.KQ) * K;
  L.o_g = e_f;
  L.o_p = L.o_g + K;
  L.o_a = L.o_p + K;
  L.o_du = L.o_a + afm_al4(L.P);
  L.wave_bwd = L.o_du + L.P * L.AT;
  const int red_f = NW * (64 * L.AT + 2 * L.AT);    // the end-of-kernel sum over the waves overlays everything
  L.lds_fwd = 4 * (L.shared_f + NW * L.wave_fwd);
  L.lds_bwd = 4 * std::max(L.shared_f + NW * L.wave_bwd, red_f);
  return L;
}

// the largest NW <= kAfmMaxWaves whose footprints fit; NW = 0 in the result: not even one wave fits
static AfmLayout afm_pick(int F, int K, int A) {
  for (int nw = kAfmMaxWaves; nw >= 1; --nw) {
    const AfmLayout L = afm_layout(F, K, A, nw);
    if (L.lds_fwd <= kTiledLdsLimit && L.lds_bwd <= kTiledLdsLimit) return L;
  }
  AfmLayout L = afm_layout(F, K, A, 1);
  L.NW = 0;
  return L;
}

static inline int afm_grid(int B, int NW) { return tiled_grid(B, NW, kAfmGridCap); }

// W, b, h and the pair table -> LDS, once per workgroup (the caller synchronises)
template <int AT>
__device__ __forceinline__ void afm_stage_params(float* smem, const AfmLayout& L, const float* __restrict__ W,
                                                 const float* __restrict__ bias, const float* __restrict__ h) {
  const int K = L.K, A = L.A, F = L.F;
  for (int t = threadIdx.x; t < AT * K; t += blockDim.x) {
    const int a = t / K, k = t - a * K;
    smem[t] = a < A ? W[k * A + a] : 0.f;
  }
  for (int t = threadIdx.x; t < AT; t += blockDim.x) {
    smem[L.o_b + t] = t < A ? bias[t] : 0.f;
    smem[L.o_h + t] = t < A ? h[t] : 0.f;
  }
  unsigned short* pairS = reinterpret_cast<unsigned short*>(smem + L.o_pair);
  for (int i = threadIdx.x; i < F - 1; i += blockDim.x) {
    const int base = i * (2 * F - i - 1) / 2;
    for (int j = i + 1; j < F; ++j) pairS[base + j - i - 1] = (unsigned short)(i | (j << 8));
  }
}

// one sample's [F,K] slab -> LDS rows at stride KP
__device__ __forceinline__ void afm_load_slab(float* eS, const float* __restrict__ src, const AfmLayout& L, int lane) {
  const int KQ = L.KQ, n = L.F * KQ;
  for (int q = lane; q < n; q += 64) {
    const int f = q / KQ, kq = q - f * KQ;
    *reinterpret_cast<float4*>(eS + f * L.KP + kq * 4) = *reinterpret_cast<const float4*>(src + (long)q * 4);
  }
}

// u = b + x_p W for the pair (i, j), k ascending; WITH_G: also gx = g . x_p, k ascending from +0
template <int AT, bool WITH_G>
__device__ __forceinline__ void afm_pair_u(const float* eS, const float* WtS, const float* bS, const float* gS, const AfmLayout& L,
                                           int i, int j, float (&u)[AT], float& gx) {
#pragma unroll
  for (int a = 0; a < AT; ++a) u[a] = bS[a];
  gx = 0.f;
  const float* pi = eS + i * L.KP;
  const float* pj = eS + j * L.KP;
  for (int kq = 0; kq < L.KQ; ++kq) {
    const float4 ei = *reinterpret_cast<const float4*>(pi + kq * 4);
    const float4 ej = *reinterpret_cast<const float4*>(pj + kq * 4);
    const float x0 = ei.x * ej.x, x1 = ei.y * ej.y, x2 = ei.z * ej.z, x3 = ei.w * ej.w;
    if constexpr (WITH_G) {
      const float4 gv = *reinterpret_cast<const float4*>(gS + kq * 4);
      gx = fmaf(gv.x, x0, gx);
      gx = fmaf(gv.y, x1, gx);
      gx = fmaf(gv.z, x2, gx);
      gx = fmaf(gv.w, x3, gx);
    }
#pragma unroll
    for (int a = 0; a < AT; ++a) {
      const float4 w = *reinterpret_cast<const float4*>(WtS + a * L.K + kq * 4);
      u[a] = fmaf(x0, w.x, u[a]);
      u[a] = fmaf(x1, w.y, u[a]);
      u[a] = fmaf(x2, w.z, u[a]);
      u[a] = fmaf(x3, w.w, u[a]);
    }
  }
}

// the score of a pair; t = the pre-activation of the reference form (unused in the paper form).  The padded columns a >= A hold
// u = 0 and h = 0 and add +0.
template <int AT>
__device__ __forceinline__ float afm_score(const float (&u)[AT], const float* hS, bool hidden_relu, float& t) {
  t = 0.f;
  if (hidden_relu) {
#pragma unroll
    for (int a = 0; a < AT; ++a) t = fmaf(fmaxf(u[a], 0.f), hS[a], t);
    return t;
  }
#pragma unroll
  for (int a = 0; a < AT; ++a) t = fmaf(u[a], hS[a], t);
  return fmaxf(t, 0.f);
}

template <int AT>
__global__ __launch_bounds__(64 * kAfmMaxWaves) void afm_fwd_kernel(const float* __restrict__ emb, const float* __restrict__ W,
                                                                   const float* __restrict__ bias, const float* __restrict__ h,
                                                                   float* __restrict__ pooled, float* __restrict__ stats, int B,
                                                                   int flags, AfmLayout L) {
  extern __shared__ __attribute__((aligned(16))) float afm_smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  afm_stage_params<AT>(afm_smem, L, W, bias, h);
  __syncthreads();
  const float* WtS = afm_smem;
  const float* bS = afm_smem + L.o_b;
  const float* hS = afm_smem + L.o_h;
  const unsigned short* pairS = reinterpret_cast<const unsigned short*>(afm_smem + L.o_pair);
  float* eS = afm_smem + L.shared_f + wave * L.wave_fwd;
  float* scS = eS + L.o_sc;
  float* redS = eS + L.o_red;
  const bool hr = (flags & 1) != 0;
  const int K = L.K, KQ = L.KQ, P = L.P, NG = 64 / KQ;
  const int kq = lane % KQ, pg = lane / KQ;
  for (long b = (long)blockIdx.x * L.NW + wave; b < B; b += (long)gridDim.x * L.NW) {
    afm_load_slab(eS, emb + b * L.F * K, L, lane);
    wave_lds_sync();
    // pass 1: scores, their maximum, the exponentials and their sum
    float mx = -INFINITY;
    for (int p = lane; p < P; p += 64) {
      const int pr = pairS[p];
      float u[AT], gx, t;
      afm_pair_u<AT, false>(eS, WtS, bS, nullptr, L, pr & 255, pr >> 8, u, gx);
      const float s = afm_score<AT>(u, hS, hr, t);
      scS[p] = s;
      mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    float den = 0.f;
    for (int p = lane; p < P; p += 64) {
      const float w = expf(scS[p] - mx);
      scS[p] = w;
      den += w;
    }
    den = wave_sum(den);
    wave_lds_sync();
    // pass 2: sum_p w_p x_p, lane = (4 consecutive k, pair group)
    if (pg < NG) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int p = pg; p < P; p += NG) {
        const int pr = pairS[p];
        const float4 ei = *reinterpret_cast<const float4*>(eS + (pr & 255) * L.KP + kq * 4);
        const float4 ej = *reinterpret_cast<const float4*>(eS + (pr >> 8) * L.KP + kq * 4);
        const float w = scS[p];
        const float x0 = ei.x * ej.x, x1 = ei.y * ej.y, x2 = ei.z * ej.z, x3 = ei.w * ej.w;
        acc[0] = fmaf(w, x0, acc[0]);
        acc[1] = fmaf(w, x1, acc[1]);
        acc[2] = fmaf(w, x2, acc[2]);
        acc[3] = fmaf(w, x3, acc[3]);
      }
      *reinterpret_cast<float4*>(redS + pg * K + kq * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
    wave_lds_sync();
    if (lane < K) {
      float t = 0.f;
      for (int g = 0; g < NG; ++g) t += redS[g * K + lane];
      pooled[b * K + lane] = t / den;
    }
    if (lane == 0) {
      stats[2 * b] = mx;
      stats[2 * b + 1] = den;
    }
    wave_lds_sync();    // the next sample's slab overwrites this image
  }
}

template <int AT>
__global__ __launch_bounds__(64 * kAfmMaxWaves) void afm_bwd_kernel(const float* __restrict__ emb, const float* __restrict__ W,
                                                                   const float* __restrict__ bias, const float* __restrict__ h,
                                                                   const float* __restrict__ pooled, const float* __restrict__ stats,
                                                                   const float* __restrict__ g, float* __restrict__ demb,
                                                                   float* __restrict__ partials, int B, int flags, AfmLayout L) {
  extern __shared__ __attribute__((aligned(16))) float afm_smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  afm_stage_params<AT>(afm_smem, L, W, bias, h);
  __syncthreads();
  const float* WtS = afm_smem;
  const float* bS = afm_smem + L.o_b;
  const float* hS = afm_smem + L.o_h;
  const unsigned short* pairS = reinterpret_cast<const unsigned short*>(afm_smem + L.o_pair);
  float* eS = afm_smem + L.shared_f + wave * L.wave_bwd;
  float* gS = eS + L.o_g;
  float* pS = eS + L.o_p;
  float* aS = eS + L.o_a;
  float* duS = eS + L.o_du;
  const bool hr = (flags & 1) != 0;
  const bool want_params = partials != nullptr;
  const int F = L.F, K = L.K, P = L.P, KP = L.KP;
  const int NGK = 64 / K, ck = lane % K, cg = lane / K;     // phase C: lane = (k, pair group)
  float dW[AT], db[AT], dh[AT];
#pragma unroll
  for (int a = 0; a < AT; ++a) dW[a] = db[a] = dh[a] = 0.f;
  for (long b = (long)blockIdx.x * L.NW + wave; b < B; b += (long)gridDim.x * L.NW) {
    afm_load_slab(eS, emb + b * F * K, L, lane);
    if (lane < K) {
      gS[lane] = g[b * K + lane];
      pS[lane] = pooled[b * K + lane];
    }
    const float mx = stats[2 * b], den = stats[2 * b + 1];
    wave_lds_sync();
    float gp = 0.f;     // g . pooled in the order of g . x_p: for one pair (F = 2) the two are the same bits and ds is exactly 0
    for (int k = 0; k < K; ++k) gp = fmaf(gS[k], pS[k], gp);
    // phase A: per pair, the score again, a_p, ds_p, du_p
    for (int p = lane; p < P; p += 64) {
      const int pr = pairS[p];
      float u[AT], gx, t;
      afm_pair_u<AT, true>(eS, WtS, bS, gS, L, pr & 255, pr >> 8, u, gx);
      const float s = afm_score<AT>(u, hS, hr, t);
      const float a_p = expf(s - mx) / den;
      const float ds = a_p * (gx - gp);
      aS[p] = a_p;
      float du[AT];
      if (hr) {
#pragma unroll
        for (int a = 0; a < AT; ++a) {
          du[a] = u[a] > 0.f ? ds * hS[a] : 0.f;
          dh[a] = fmaf(ds, fmaxf(u[a], 0.f), dh[a]);
        }
      } else {
        const float dt = t > 0.f ? ds : 0.f;
#pragma unroll
        for (int a = 0; a < AT; ++a) {
          du[a] = dt * hS[a];
          dh[a] = fmaf(dt, u[a], dh[a]);
        }
      }
#pragma unroll
      for (int a = 0; a < AT; ++a) db[a] += du[a];
#pragma unroll
      for (int a = 0; a < AT; a += 4)
        *reinterpret_cast<float4*>(duS + p * AT + a) = make_float4(du[a], du[a + 1], du[a + 2], du[a + 3]);
    }
    wave_lds_sync();
    // phase B: de[f,k] = sum over the partners j (ascending) of dx_p[k] e_j[k], dx_p = a_p g + W du_p
    if (demb != nullptr) {
      float* dst = demb + b * F * K;
      for (int idx = lane; idx < F * K; idx += 64) {
        const int f = idx / K, k = idx - f * K;
        float wk[AT];
#pragma unroll
        for (int a = 0; a < AT; ++a) wk[a] = WtS[a * K + k];
        const float gk = gS[k];
        float acc = 0.f;
        auto partner = [&](int p, int j) {
          float wdu = 0.f;
#pragma unroll
          for (int a = 0; a < AT; a += 4) {
            const float4 d = *reinterpret_cast<const float4*>(duS + p * AT + a);
            wdu = fmaf(wk[a], d.x, wdu);
            wdu = fmaf(wk[a + 1], d.y, wdu);
            wdu = fmaf(wk[a + 2], d.z, wdu);
            wdu = fmaf(wk[a + 3], d.w, wdu);
          }
          const float dx = fmaf(aS[p], gk, wdu);
          acc = fmaf(dx, eS[j * KP + k], acc);
        };
        int p = f - 1;                              // the pair (0, f); (j + 1, f) sits F - j - 2 after (j, f)
#pragma unroll 4
        for (int j = 0; j < f; ++j) {
          partner(p, j);
          p += F - j - 2;
        }
        p = f * (2 * F - f - 1) / 2;                // the pair (f, f + 1); the pairs (f, j) follow each other
#pragma unroll 4
        for (int j = f + 1; j < F; ++j, ++p) partner(p, j);
        dst[idx] = acc;
      }
    }
    // phase C: dW[k,:] += x_p[k] du_p over this lane's pair group
    if (want_params && cg < NGK) {
#pragma unroll 4
      for (int p = cg; p < P; p += NGK) {
        const int pr = pairS[p];
        const float x = eS[(pr & 255) * KP + ck] * eS[(pr >> 8) * KP + ck];
#pragma unroll
        for (int a = 0; a < AT; a += 4) {
          const float4 d = *reinterpret_cast<const float4*>(duS + p * AT + a);
          dW[a] = fmaf(x, d.x, dW[a]);
          dW[a + 1] = fmaf(x, d.y, dW[a + 1]);
          dW[a + 2] = fmaf(x, d.z, dW[a + 2]);
          dW[a + 3] = fmaf(x, d.w, dW[a + 3]);
        }
      }
    }
    wave_lds_sync();    // the next sample overwrites this image
  }
  if (!want_params) return;
  // the workgroup's partial: waves and pair groups in index order.  The sums overlay the waves' regions: every wave is done first.
  __syncthreads();
  float* redW = afm_smem;                              // [NW][64 lanes][AT]
  float* redP = afm_smem + L.NW * 64 * AT;             // [NW][db AT | dh AT]
#pragma unroll
  for (int a = 0; a < AT; ++a) {
    redW[(wave * 64 + lane) * AT + a] = (cg < NGK) ? dW[a] : 0.f;
    const float sb = wave_sum(db[a]), sh = wave_sum(dh[a]);
    if (lane == 0) {
      redP[wave * 2 * AT + a] = sb;
      redP[wave * 2 * AT + AT + a] = sh;
    }
  }
  __syncthreads();
  const int A = L.A, KA = K * A;
  float* out = partials + (long)blockIdx.x * (KA + 2 * A);
  for (int o = threadIdx.x; o < KA + 2 * A; o += blockDim.x) {
    float t = 0.f;
    if (o < KA) {
      const int k = o / A, a = o - k * A;
      for (int w = 0; w < L.NW; ++w)
        for (int gq = 0; gq < NGK; ++gq) t += redW[(w * 64 + gq * K + k) * AT + a];
    } else {
      const int r = o - KA, which = r / A, a = r - which * A;
      for (int w = 0; w < L.NW; ++w) t += redP[w * 2 * AT + which * AT + a];
    }
    out[o] = t;
  }
}

// argument and menu checks shared by the four entry points
static int afm_dims(const char* who, int B, int F, int K, int A, AfmLayout* L) {
  FIL_CHECK_ARG_W(who, B >= 0 && F >= 1 && K >= 1 && A >= 1);
  if (F < 2 || F > kAfmMaxF) return fail(FIL_ERR_UNSUPPORTED, "%s: F=%d outside 2 <= F <= %d", who, F, kAfmMaxF);
  if (K % 4 != 0 || K > kAfmMaxK) return fail(FIL_ERR_UNSUPPORTED, "%s: K=%d needs K %% 4 == 0 and K <= %d", who, K, kAfmMaxK);
  if (A > kAfmMaxA) return fail(FIL_ERR_UNSUPPORTED, "%s: A=%d > %d", who, A, kAfmMaxA);
  *L = afm_pick(F, K, A);
  if (L->NW == 0)
    return fail(FIL_ERR_UNSUPPORTED, "%s: F=%d K=%d A=%d needs %d bytes of LDS (limit %d)", who, F, K, A, std::max(L->lds_fwd, L->lds_bwd),
                kTiledLdsLimit);
  return FIL_OK;
}

static size_t afm_partial_floats(int K, int A) { return (size_t)K * A + 2 * (size_t)A; }

}  // namespace fil

using namespace fil;

extern "C" int fil_afm_plan(int B, int F, int K, int A, int* plan) {
  AfmLayout L;
  if (int rc = afm_dims(__func__, B, F, K, A, &L)) return rc;
  FIL_CHECK_ARG(plan != nullptr);
  tiled_plan(plan, L.NW, afm_grid(B, L.NW), kAfmGridCap, L.lds_fwd, L.lds_bwd);
  return FIL_OK;
}

extern "C" int fil_afm_fwd(const float* emb, const float* W, const float* b, const float* h, float* pooled, float* stats, int B, int F,
                           int K, int A, int flags, void* stream) {
  AfmLayout L;
  if (int rc = afm_dims(__func__, B, F, K, A, &L)) return rc;
  FIL_CHECK_ARG((flags & ~1) == 0);
  if (B == 0) return FIL_OK;
  FIL_CHECK_ARG(emb != nullptr && W != nullptr && b != nullptr && h != nullptr && pooled != nullptr && stats != nullptr);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("afm_fwd", st, 4.0 * ((double)B * ((double)F * K + K + 2) + (double)K * A + 2.0 * A));
  const dim3 grid(afm_grid(B, L.NW)), block(64 * L.NW);
  if (L.AT == 4) {
    if (int rc = tiled_allow_lds(__func__, afm_fwd_kernel<4>, L.lds_fwd)) return rc;
    hipLaunchKernelGGL(afm_fwd_kernel<4>, grid, block, L.lds_fwd, st, emb, W, b, h, pooled, stats, B, flags, L);
  } else {
    if (int rc = tiled_allow_lds(__func__, afm_fwd_kernel<16>, L.lds_fwd)) return rc;
    hipLaunchKernelGGL(afm_fwd_kernel<16>, grid, block, L.lds_fwd, st, emb, W, b, h, pooled, stats, B, flags, L);
  }
  FIL_CHECK_LAUNCH();
  return FIL_OK;
}

extern "C" size_t fil_afm_bwd_workspace_bytes(int B, int F, int K, int A) {
  AfmLayout L;
  if (afm_dims(__func__, B, F, K, A, &L) != FIL_OK) return 0;
  return tiled_partial_bytes(afm_grid(B, L.NW), afm_partial_floats(K, A));
}

extern "C" int fil_afm_bwd(const float* emb, const float* W, const float* b, const float* h, const float* pooled, const float* stats,
                           const float* g, float* demb, float* dW, float* db, float* dh, void* workspace, size_t workspace_bytes, int B,
                           int F, int K, int A, int flags, void* stream) {
  AfmLayout L;
  if (int rc = afm_dims(__func__, B, F, K, A, &L)) return rc;
  FIL_CHECK_ARG((flags & ~1) == 0);
  if (B == 0) return FIL_OK;
  FIL_CHECK_ARG(emb != nullptr && W != nullptr && b != nullptr && h != nullptr && pooled != nullptr && stats != nullptr && g != nullptr);
  const bool want_params = dW != nullptr || db != nullptr || dh != nullptr;
  FIL_CHECK_ARG(demb != nullptr || want_params);
  const int nparts = afm_grid(B, L.NW);
  if (want_params)
    if (int rc = tiled_check_workspace(__func__, workspace, workspace_bytes, nparts, afm_partial_floats(K, A))) return rc;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("afm_bwd", st, 4.0 * ((double)B * (2.0 * F * K + 2.0 * K + 2) + 2.0 * ((double)K * A + 2.0 * A)));
  float* partials = want_params ? static_cast<float*>(workspace) : nullptr;
  const dim3 grid(nparts), block(64 * L.NW);
  if (L.AT == 4) {
    if (int rc = tiled_allow_lds(__func__, afm_bwd_kernel<4>, L.lds_bwd)) return rc;
    hipLaunchKernelGGL(afm_bwd_kernel<4>, grid, block, L.lds_bwd, st, emb, W, b, h, pooled, stats, g, demb, partials, B, flags, L);
  } else {
    if (int rc = tiled_allow_lds(__func__, afm_bwd_kernel<16>, L.lds_bwd)) return rc;
    hipLaunchKernelGGL(afm_bwd_kernel<16>, grid, block, L.lds_bwd, st, emb, W, b, h, pooled, stats, g, demb, partials, B, flags, L);
  }
  FIL_CHECK_LAUNCH();
  if (want_params) {
    float* const outs[3] = {dW, db, dh};
    const int off[4] = {0, K * A, K * A + A, K * A + 2 * A};
    param_reduce_launch(partials, nparts, outs, off, 3, st);
    FIL_CHECK_LAUNCH();
  }
  return FIL_OK;
}
