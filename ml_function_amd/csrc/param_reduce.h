// The fixed-order sum of per-workgroup parameter-gradient partials (param_reduce_kernel in param_reduce.hip), for every launcher
// that leaves its parameter gradients as one partial per workgroup: fil_afm_bwd, fil_din_bwd, fil_gru_bwd, fil_seqattn_bwd.
#pragma once
#include "common.h"

namespace fil {

constexpr int kParamReduceMaxOuts = 8;

// A partial is the outputs' elements back to back in ABI order (the order of the entry point's gradient arguments): off[n_outs]
// floats, output w at off[w] .. off[w + 1], n_outs <= kParamReduceMaxOuts.  outs[w] == nullptr: not wanted, nothing is written.
// out[o] = sum over the nparts partials: 16 slices of every 16th partial (each from 0.f, in increasing order), then the slices in
// order (from 0.f).  One launch of cdiv(off[n_outs], 16) workgroups of 256 threads on `st`.
void param_reduce_launch(const float* partials, int nparts, float* const* outs, const int* off, int n_outs, hipStream_t st);

}  // namespace fil
