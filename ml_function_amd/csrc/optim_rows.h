// Row helpers shared by the table optimizers of optim.hip (Adam) and optim_rowwise.hip (Adagrad, Ftrl): the field of a row, and the
// look-ups into the gathered compact lists of fil_embed_runs_compact.
#pragma once
#include "common.h"

namespace fil {

constexpr int kSweepMaxF = 1024;

// the last f with off[f] <= row, or -1
__device__ __forceinline__ int sweep_field(const int64_t* off, int F, int64_t row) {
  int lo = 0, hi = F;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= row) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

// the position of `row` in an ascending list of n distinct ids, or -1
__device__ __forceinline__ long find_row(const int64_t* __restrict__ list, long n, int64_t row) {
  long lo = 0, hi = n;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (list[mid] < row) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && list[lo] == row ? lo : -1;
}

// the number of valid entries of gathered list w (its count clipped to [0, cap])
__device__ __forceinline__ long list_count(const int64_t* counts, int w, long cap) {
  const int64_t c = counts[w];
  return c < 0 ? 0 : (c > cap ? cap : (long)c);
}

}  // namespace fil
