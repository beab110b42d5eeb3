// N3  The fixed-order sum of per-workgroup parameter-gradient partials for gfx950 (param_reduce.h says who uses it).
#include "param_reduce.h"

namespace fil {

struct ParamReduceOuts {
  float* p[kParamReduceMaxOuts];        // the outputs in ABI order; nullptr: not wanted
  int off[kParamReduceMaxOuts + 1];     // their offsets in a partial; every entry from the last output's end on holds n_out
};

// out[o] = sum over the partials in a fixed order: 16 slices of every 16th partial, then the slices in order
__global__ __launch_bounds__(256) void param_reduce_kernel(const float* __restrict__ partials, int nparts, ParamReduceOuts G) {
  __shared__ float red[16][17];
  const int ol = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int n_out = G.off[kParamReduceMaxOuts];
  const int o = blockIdx.x * 16 + ol;
  float t = 0.f;
  if (o < n_out)
    for (int pq = sl; pq < nparts; pq += 16) t += partials[(long)pq * n_out + o];
  red[sl][ol] = t;
  __syncthreads();
  if (sl == 0 && o < n_out) {
    float s = 0.f;
    for (int pq = 0; pq < 16; ++pq) s += red[pq][ol];
    int w = 0;
    while (o >= G.off[w + 1]) ++w;      // (o < n_out = off[n_outs]: the walk ends at an output)
    if (G.p[w] != nullptr) G.p[w][o - G.off[w]] = s;
  }
}

void param_reduce_launch(const float* partials, int nparts, float* const* outs, const int* off, int n_outs, hipStream_t st) {
  ParamReduceOuts G;
  for (int w = 0; w < kParamReduceMaxOuts; ++w) G.p[w] = w < n_outs ? outs[w] : nullptr;
  for (int w = 0; w <= kParamReduceMaxOuts; ++w) G.off[w] = off[w < n_outs ? w : n_outs];
  hipLaunchKernelGGL(param_reduce_kernel, dim3(cdiv(off[n_outs], 16)), dim3(256), 0, st, partials, nparts, G);
}

}  // namespace fil
