// The fixed-order sum of per-workgroup parameter-gradient partials (gru_param_reduce_kernel in gru.hip), for every launcher that
// leaves its parameter gradients as one partial per workgroup.
#pragma once
#include "common.h"

namespace fil {

// A partial is off[3] floats: up to three outputs back to back, output w at off[w] .. off[w + 1].  outs[w] == nullptr: not wanted.
// out[o] = sum over the nparts partials: 16 slices of every 16th partial, then the slices in order.  One launch on `st`.
void param_reduce_launch(const float* partials, int nparts, float* const outs[3], const int off[4], hipStream_t st);

}  // namespace fil
