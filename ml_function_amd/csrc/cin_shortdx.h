// Data gradient of the pooled-weights shortcut on the merged quadratic tail, as a launch of its own (cin_shortdx_used, cin.hip):
//   dX[m,f] = dP[m] * sum_h x1[m,h] wsum[h,f]        x1 [M][xps] (Hp <= 128 maps, columns >= Hp zero), wsum [Hp][F], dxT [M][F]
// What cin_last_bwd2_kernel's phase u computes, up to summation order.  That body shares its prologue, registers and LDS with phase t;
// this kernel has one job, and is arranged so that memory is requested before anything waits:
//   1. every lane requests its words of the operand image of wsum (L2) and then the wave's whole 32 x 128 tile of x1 (sixteen
//      coalesced 16-byte loads per lane) before the first wait;
//   2. the image goes to LDS while the tile is in flight: wsum zero-padded to 128 x 16 NT and laid out so that the B operands of four
//      reduction steps are ONE unconditional 16-byte read per lane and column tile, 64 lanes on 1024 consecutive bytes;
//   3. the tile's first 64 columns are staged and contracted while its last 64 are still arriving.
// Fields are tiled 16 wide (v_mfma_f32_16x16x4_f32, the flop rate of the 32x32x2 form): NT = ceil(F / 16) tiles -- 48 columns at F = 39
// where two 32-wide blocks made 64 -- over two 16-row blocks.  Lane l = 16 g + c holds rows c and 16 + c of A and column c of B; the
// reduction order is permuted (free in a GEMM) so that k-group g takes h = 64 hh + 16 g + s, s = 0..15, in each 64-column half hh:
// sixteen consecutive floats of a staged row, four 16-byte reads.
#pragma once
#include "cin_kernels.h"

namespace fil {

constexpr int kSdxLd = 68;                 // floats between staged rows of x1 (64 columns + 4: 16-byte rows, conflict-free 16-byte row reads)
constexpr int kSdxStage = 32 * kSdxLd;     // per-wave staging floats: 32 rows x 64 columns
constexpr int sdx_image_floats(int NT) { return 2 * NT * 4 * 64 * 4; }   // [half hh][tile t][step quad s4][lane] x float4
inline size_t cin_shortdx_lds_bytes(int NT) { return (size_t)(sdx_image_floats(NT) + 4 * kSdxStage) * sizeof(float); }

template <int NT>
__global__ __launch_bounds__(256, 2) void cin_shortcut_dx_kernel(const float* __restrict__ xpT, int xps, const float* __restrict__ wsum,
                                                                const float* __restrict__ dP, int ldp, float* __restrict__ dxT, int M, int F,
                                                                int K, int Hp) {
  extern __shared__ __attribute__((aligned(16))) float smem[];   // image [2 NT 4 64] float4 | per wave: staging [kSdxStage]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int wrow0 = (blockIdx.x * 4 + wave) * 32;
  // ---- requests, all unconditional (clamped addresses; what lies outside is zeroed on the way to LDS / never stored).
  // lane r < 32 fetches the pooled gradient of row r (the other half the same words); the epilogue reads it across lanes
  const long mq = min(wrow0 + (lane & 31), M - 1);
  const int bq = (int)(mq / K);
  const float dpv = dP[(long)bq * ldp + (int)(mq - (long)bq * K)];
  // image word (hh, t, s4 = wave, lane, e) = wsum[64 hh + 16 g + 4 s4 + e][16 t + c], zero outside [Hp][F]
  float wv[2 * NT][4];
#pragma unroll
  for (int q = 0; q < 2 * NT; ++q) {
    const int hh = q / NT, t = q - hh * NT;
    const int h0 = 64 * hh + 16 * g + 4 * wave, f = min(16 * t + c, F - 1);
#pragma unroll
    for (int e = 0; e < 4; ++e) wv[q][e] = wsum[min(h0 + e, Hp - 1) * F + f];
  }
  // the wave's rows of x1, 64 columns per half: a quarter row per 16 lanes, four rows per load (xps >= 128: the launcher's condition)
  f32x4 v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int hh = i >> 3;
    const int row = (lane >> 4) + 4 * (i & 7), col = 64 * hh + 4 * (lane & 15);
    v[i] = *reinterpret_cast<const f32x4*>(xpT + (long)min(wrow0 + row, M - 1) * xps + col);
    if (i == 7) __builtin_amdgcn_sched_barrier(0);   // (the first half's eight first: its wait then leaves the second half in flight)
  }
  __builtin_amdgcn_sched_barrier(0);   // (nothing above is sunk below its first use: all of it is in flight here)
  // ---- the image
  f32x4* img = reinterpret_cast<f32x4*>(smem);
#pragma unroll
  for (int q = 0; q < 2 * NT; ++q) {
    const int hh = q / NT, t = q - hh * NT;
    const int h0 = 64 * hh + 16 * g + 4 * wave;
    const bool fin = 16 * t + c < F;
    img[q * 256 + tid] = f32x4{fin && h0 < Hp ? wv[q][0] : 0.f, fin && h0 + 1 < Hp ? wv[q][1] : 0.f, fin && h0 + 2 < Hp ? wv[q][2] : 0.f,
                               fin && h0 + 3 < Hp ? wv[q][3] : 0.f};
  }
  __syncthreads();
  // (No branch from here on, on purpose: a wave past the end works on row M - 1 and stores nothing, and with Hp <= 64 the second half
  // meets a zero image.  Behind a branch the compiler sinks the requests above to where their values are used.)
  float* stg = smem + sdx_image_floats(NT) + wave * kSdxStage;
  f32x4 acc[2][NT];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[rb][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    {   // (no `if (Hp > 64)` around the second half: see above)
      f32x4 a[2][4];
      __builtin_amdgcn_wave_barrier();   // (the previous half's reads of the staging area are done)
#pragma unroll
      for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(stg + ((lane >> 4) + 4 * i) * kSdxLd + 4 * (lane & 15)) = v[8 * hh + i];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int j = 0; j < 4; ++j) a[rb][j] = *reinterpret_cast<const f32x4*>(stg + (16 * rb + c) * kSdxLd + 16 * g + 4 * j);
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        f32x4 b[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) b[t] = img[((hh * NT + t) * 4 + s4) * 64 + lane];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[rb][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rb][s4][e], b[t][e], acc[rb][t], 0, 0, 0);
      }
    }
  }
  // ---- dX = dP u: register reg of tile (rb, t) is row 16 rb + 4 g + reg, field 16 t + c
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = 16 * rb + 4 * g + reg, m = wrow0 + row;
      const float dpr = __shfl(dpv, row);
      if (m < M) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
          if (16 * t + c < F) dxT[(long)m * F + 16 * t + c] = dpr * acc[rb][t][reg];
      }
    }
}

}  // namespace fil
