// fil_embed_runs_compact: a rank's runs record as a compact list (distinct ids, their run sums) of fixed capacity, the unit of the
// data-parallel exchange; every fused optimizer's merged update (optim.hip, optim_rule.h) applies the gathered lists.
#include "common.h"
#include "embed_runs.h"
#include "optim_rows.h"
#include <hip/hip_bf16.h>

namespace fil {

// The run sums of embed_runs.h stored into compact slots.  Three launches, none sized by data:
//   count  one workgroup per kCompactTile sorted positions counts its run starts (id >= 0, != the id before);
//   write  every workgroup sums the counts of the tiles before it (and of all tiles: the total), scans its own starts in position
//          order and writes ids_out[u] = id and slot[perm of the start] = u; the slots [count, cap) get INT64_MAX, count_out the total;
//   sums   embed_run_sums with an epilogue that stores the row into values_out[slot[perm of the run's first element]].
// A one-id record's perm holds each position b*F + f exactly once (< R), so the slot map needs R entries and no two runs share one.
// A pooled field's record (embed_bag.hip) names the BAG in perm, once per slot: two runs that start with slots of one bag then write
// the same map entry.  The epilogue therefore checks ids_out[slot] against the run's row and, where another run's slot sits there,
// looks the row up in ids_out (ascending, padded with INT64_MAX: a binary search over all cap entries).  Integer scans: deterministic.
constexpr int kCompactPer = 8;
constexpr int kCompactTile = 256 * kCompactPer;

__device__ __forceinline__ bool run_start_at(const int64_t* __restrict__ sorted_ids, long j) {
  const int64_t id = sorted_ids[j];
  return id >= 0 && (j == 0 || sorted_ids[j - 1] != id);
}

__global__ __launch_bounds__(256) void runs_count_kernel(const int64_t* __restrict__ sorted_ids, long R, int64_t* __restrict__ tile_count) {
  __shared__ long s[4];
  const long base = (long)blockIdx.x * kCompactTile + (long)threadIdx.x * kCompactPer;
  long n = 0;
#pragma unroll
  for (int i = 0; i < kCompactPer; ++i)
    if (base + i < R && run_start_at(sorted_ids, base + i)) ++n;
  n = block_sum_256(n, s);
  if (threadIdx.x == 0) tile_count[blockIdx.x] = n;
}

__global__ __launch_bounds__(256) void runs_write_kernel(const int64_t* __restrict__ sorted_ids, const int64_t* __restrict__ perm, long R,
                                                         const int64_t* __restrict__ tile_count, int tiles, long cap,
                                                         int64_t* __restrict__ ids_out, int64_t* __restrict__ count_out,
                                                         int32_t* __restrict__ slot) {
  __shared__ long s[4];
  __shared__ long s_scan[4];
  long before = 0, all = 0;
  for (int b = threadIdx.x; b < tiles; b += 256) {
    const long c = tile_count[b];
    all += c;
    before += b < (int)blockIdx.x ? c : 0;
  }
  before = block_sum_256(before, s);
  all = block_sum_256(all, s);
  // this lane's starts, then an exclusive scan over the workgroup in lane order (= position order)
  const long base = (long)blockIdx.x * kCompactTile + (long)threadIdx.x * kCompactPer;
  unsigned flags = 0;
#pragma unroll
  for (int i = 0; i < kCompactPer; ++i)
    if (base + i < R && run_start_at(sorted_ids, base + i)) flags |= 1u << i;
  const long mine = __builtin_popcount(flags);
  long starts;                                   // (of this tile: tile_count has it already)
  long u = before + block_scan_256(mine, s_scan, &starts);
#pragma unroll
  for (int i = 0; i < kCompactPer; ++i) {
    if (flags & (1u << i)) {
      const long j = base + i;
      const int64_t pj = perm[j];
      if (u < cap) ids_out[u] = sorted_ids[j];
      if ((uint64_t)pj < (uint64_t)R) slot[pj] = (int32_t)u;
      ++u;
    }
  }
  for (long i = all + (long)blockIdx.x * 256 + threadIdx.x; i < cap; i += (long)gridDim.x * 256) ids_out[i] = INT64_MAX;
  if (blockIdx.x == 0 && threadIdx.x == 0) *count_out = all;
}

template <typename GT>
__global__ __launch_bounds__(256) void runs_compact_sums_kernel(const GT* __restrict__ g, const int64_t* __restrict__ perm,
                                                                const int64_t* __restrict__ sorted_ids, long R, int K,
                                                                const int32_t* __restrict__ slot, long cap,
                                                                const int64_t* __restrict__ ids_out, float* __restrict__ values_out) {
  embed_run_sums(g, perm, sorted_ids, R, K, [=](int64_t row, int kq, const float (&acc)[4], int64_t first) {
    if ((uint64_t)first >= (uint64_t)R) return;
    long u = slot[first];
    if (u < 0 || u >= cap) return;
    if (ids_out[u] != row) {       // (a perm entry shared by several runs: the map holds another run's slot)
      long lo = 0, hi = cap;
      while (lo < hi) {
        const long mid = lo + (hi - lo) / 2;
        if (ids_out[mid] < row) lo = mid + 1; else hi = mid;
      }
      if (lo >= cap || ids_out[lo] != row) return;
      u = lo;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (kq * 4 + i < K) values_out[u * K + kq * 4 + i] = acc[i];
  });
}

}  // namespace fil

using namespace fil;

extern "C" size_t fil_embed_runs_compact_workspace_bytes(long R) {
  if (R <= 0) return 0;
  const long tiles = (R + kCompactTile - 1) / kCompactTile;
  return align_up((size_t)tiles * sizeof(int64_t), 256) + align_up((size_t)R * sizeof(int32_t), 256);
}

extern "C" int fil_embed_runs_compact(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype,
                                      int64_t* ids_out, float* values_out, int64_t* count_out, long cap, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  FIL_CHECK_ARG(R >= 0 && K >= 1 && cap >= 0);
  if (g_dtype != FIL_F32 && g_dtype != FIL_BF16) return fail(FIL_ERR_ARG, "fil_embed_runs_compact: g_dtype %d (f32 or bf16)", g_dtype);
  if (int rc = check_table_shape("fil_embed_runs_compact", K, 0)) return rc;
  if (cap < R) return fail(FIL_ERR_ARG, "fil_embed_runs_compact: cap %ld < R %ld (a list must hold every run of the record)", cap, R);
  if (R > (long)INT32_MAX) return fail(FIL_ERR_UNSUPPORTED, "fil_embed_runs_compact: R=%ld > 2^31 - 1", R);
  FIL_CHECK_ARG(ids_out && count_out);
  if (workspace_bytes < fil_embed_runs_compact_workspace_bytes(R))
    return fail(FIL_ERR_ARG, "fil_embed_runs_compact: workspace of %zu bytes < %zu (fil_embed_runs_compact_workspace_bytes)", workspace_bytes,
                fil_embed_runs_compact_workspace_bytes(R));
  hipStream_t st = (hipStream_t)stream;
  if (R == 0) {         // an empty list: count 0, every slot padding (the write kernel with no tiles)
    hipLaunchKernelGGL(runs_write_kernel, dim3(1), dim3(256), 0, st, sorted_ids, perm, 0L, (const int64_t*)nullptr, 0, cap, ids_out,
                       count_out, (int32_t*)nullptr);
    FIL_CHECK_LAUNCH();
    return FIL_OK;
  }
  FIL_CHECK_ARG(g && perm && sorted_ids && values_out && workspace);
  Carver cv(workspace);
  const int tiles = (int)((R + kCompactTile - 1) / kCompactTile);
  int64_t* tile_count = cv.take<int64_t>(tiles);
  int32_t* slot = cv.take<int32_t>(R);
  ProfScope ps("embed_runs_compact", st, (double)R * K * (g_dtype == FIL_F32 ? 4 : 2) + 20.0 * R + 4.0 * (double)R * K);
  hipLaunchKernelGGL(runs_count_kernel, dim3(tiles), dim3(256), 0, st, sorted_ids, R, tile_count);
  FIL_CHECK_LAUNCH();
  hipLaunchKernelGGL(runs_write_kernel, dim3(tiles), dim3(256), 0, st, sorted_ids, perm, R, tile_count, tiles, cap, ids_out, count_out, slot);
  FIL_CHECK_LAUNCH();
  const dim3 grid = run_sums_grid(R, K);
  if (g_dtype == FIL_F32)
    hipLaunchKernelGGL(runs_compact_sums_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(g), perm, sorted_ids, R, K, slot,
                       cap, ids_out, values_out);
  else
    hipLaunchKernelGGL(runs_compact_sums_kernel<__hip_bfloat16>, grid, dim3(256), 0, st, static_cast<const __hip_bfloat16*>(g), perm,
                       sorted_ids, R, K, slot, cap, ids_out, values_out);
  FIL_CHECK_LAUNCH();
  return FIL_OK;
}
