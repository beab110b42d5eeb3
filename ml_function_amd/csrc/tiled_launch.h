// The launch kit of the ops that give every workgroup tiles of samples and leave ONE parameter-gradient partial per workgroup
// (afm.hip, din.hip, gru.hip, lstm.hip, seq_attn.hip; param_reduce.h then adds the partials): the LDS limit and opt-in, the grid, the plan
// and the partial workspace, each defined once.  Host code only.
#pragma once
#include "common.h"
#include <algorithm>

namespace fil {

constexpr int kTiledLdsLimit = 163328;   // the launchers' dynamic LDS limit (include/fil.h)

// the opt-in a kernel needs above 48 KiB of dynamic LDS; `who` names the entry point that was called
template <typename KernelT>
static int tiled_allow_lds(const char* who, KernelT kernel, int bytes) {
  if (bytes > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return fail(FIL_ERR_HIP, "%s: %d bytes of dynamic LDS refused: %s", who, bytes, hipGetErrorString(e));
  }
  return FIL_OK;
}

// workgroups of a launch over B samples in tiles of `tile`: one per tile up to the op's cap, past it a workgroup walks several tiles
static inline int tiled_grid(int B, int tile, int cap) { return B <= 0 ? 0 : std::min(cdiv(B, tile), cap); }

// the eight ints of fil_*_plan
static inline void tiled_plan(int* plan, int tile, int grid, int cap, int lds_fwd, int lds_bwd) {
  plan[0] = 1;            // forward fits
  plan[1] = 1;            // backward fits
  plan[2] = tile;         // samples per workgroup tile
  plan[3] = grid;
  plan[4] = cap;
  plan[5] = grid;         // parameter-gradient partials: one per workgroup
  plan[6] = lds_fwd;
  plan[7] = lds_bwd;
}

// bytes of nparts partials of n_out floats each
static inline size_t tiled_partial_bytes(int nparts, size_t n_out) { return align_up((size_t)nparts * n_out * sizeof(float), 256); }

// the workspace a backward that wants parameter gradients has to be given; `who` is the fil_*_bwd entry point
static inline int tiled_check_workspace(const char* who, const void* workspace, size_t workspace_bytes, int nparts, size_t n_out) {
  const size_t need = tiled_partial_bytes(nparts, n_out);
  if (workspace == nullptr || workspace_bytes < need)
    return fail(FIL_ERR_ARG, "%s: workspace of %zu bytes, %zu needed (%s_workspace_bytes)", who, workspace_bytes, need, who);
  return FIL_OK;
}

}  // namespace fil
