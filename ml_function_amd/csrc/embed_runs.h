// The run sums behind fil_embed_run_sum (embed.hip), fil_embed_runs_compact (runs_compact.hip) and the fused optimizers' runs
// updates (optim.hip, optim_rule.h): one definition, so a fused optimizer sums every row's gradient in exactly the order the dense
// gradient does; and the grid that walk is launched with.
#pragma once
#include "common.h"

namespace fil {

// Capture-safe form of the same sum (no data-dependent sizes anywhere).  A wave takes C = 64 / KQ consecutive SORTED POSITIONS
// per iteration, one per lane group (KQ lanes = one row of K floats).  A group whose position starts a run of equal row ids
//   * of at most kRunShort elements sums it by itself, in sorted order (the ids, the permutation entries and the gradient rows
//     of the whole run are three rounds of independent loads: Criteo-like batches are mostly runs of 1-3);
//   * of more elements hands it to the whole wave: lanes (c, kq) take elements c, c + C, ... and the C partial sums are folded
//     in lane order (hot ids with thousands of hits).
// Which form a run takes depends on its length only, so repeats are bit-identical.  Each finished row goes to the caller's
// epilogue epi(row, kq, acc[4], perm of the run's first element) from lane group 0 of the run (a short run's own group); id -1
// (out-of-range / frozen) is skipped.  (Round 2 first had one wave per position: 60 us for 160 k positions.)
constexpr int kRunShort = 8;

template <typename GT, typename Epi>
__device__ __forceinline__ void embed_run_sums(const GT* __restrict__ g, const int64_t* __restrict__ perm,
                                               const int64_t* __restrict__ sorted_ids, long R, int K, const Epi& epi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int KQ = (K + 3) / 4, C = 64 / KQ;
  const int c = lane / KQ, kq = lane - c * KQ;
  for (long j0 = ((long)blockIdx.x * 4 + wave) * C; j0 < R; j0 += (long)gridDim.x * 4 * C) {
    const long j = j0 + c;
    const bool have = c < C && j < R;
    const long jc = have ? j : R - 1;
    const int64_t row = sorted_ids[jc];
    const int64_t prev = jc > 0 ? sorted_ids[jc - 1] : -2;
    const bool start = have && row >= 0 && prev != row;
    // length of the run, counted up to kRunShort + 1 (all look-ahead ids are independent loads)
    int64_t nxt[kRunShort];
#pragma unroll
    for (int t = 0; t < kRunShort; ++t) nxt[t] = sorted_ids[jc + 1 + t < R ? jc + 1 + t : R - 1];
    int n = 1;
    bool same = true;
#pragma unroll
    for (int t = 0; t < kRunShort; ++t) {
      same = same && jc + 1 + t < R && nxt[t] == row;
      n += same ? 1 : 0;
    }
    const bool is_long = start && n > kRunShort;
    if (start && !is_long) {
      long pr[kRunShort];
#pragma unroll
      for (int t = 0; t < kRunShort; ++t) pr[t] = perm[t < n ? jc + t : jc];
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < kRunShort; ++t) {
        const GT* src = g + pr[t] * K + kq * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (t < n && kq * 4 + i < K) acc[i] += (float)src[i];
      }
      epi(row, kq, acc, pr[0]);
    }
    // long runs: one after the other, by the whole wave
    unsigned long long pending = __ballot(is_long && kq == 0);
    while (pending != 0) {
      const int ll = __builtin_ctzll(pending);          // first lane of the group that found the run
      pending &= pending - 1;
      const long js = j0 + ll / KQ;
      // the run's id from the lane that found it (a reload was one more L2 round trip per run)
      const int64_t rl = ((int64_t)__shfl((int)(row >> 32), ll, 64) << 32) | (unsigned)__shfl((int)(unsigned)row, ll, 64);
      // The end of the run, 64 ids per look (one ballot), and -- requested together with the first look, before its answer -- the
      // permutation entries of the first 4 C elements: a run of up to 4 C elements (most of the "long" ones: 9 ... 64) is then two
      // dependent round trips (ids | perm, rows) instead of four.  The sums run over a KNOWN range (a compare per element would
      // hang every load on an id: a field of 10 values in a batch of 4096 is ten runs of ~400).
      const long jj0 = js + c;
      long pr0[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long q = jj0 + (long)u * C;
        pr0[u] = perm[(c < C && q < R) ? q : js];
      }
      long je = js + 1;
      for (;;) {
        const long pp = je + lane;
        const unsigned long long same = __ballot(pp < R && sorted_ids[pp < R ? pp : R - 1] == rl);
        if (same == ~0ull) {
          je += 64;
          continue;
        }
        je += __builtin_ctzll(~same);
        break;
      }
      // lane group c takes elements js + c, + C, ...: four at a time into four accumulators (independent loads), folded as
      // (a0 + a1) + (a2 + a3) -- the order depends on the run's length only, so repeats stay bit-identical
      float acc4[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc4[u][i] = 0.f;
      if (c < C) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const GT* src = g + pr0[u] * K + kq * 4;
          const bool on = jj0 + (long)u * C < je;
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (on && kq * 4 + i < K) acc4[u][i] += (float)src[i];
        }
        // (the next batch's permutation entries requested in front of this batch's rows: 62 -> 90 registers, 20.9 -> 21.9 us)
        for (long jj = jj0 + 4L * C; jj < je; jj += 4L * C) {
          long pr[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) pr[u] = perm[jj + (long)u * C < je ? jj + (long)u * C : jj];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const GT* src = g + pr[u] * K + kq * 4;
            const bool on = jj + (long)u * C < je;
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (on && kq * 4 + i < K) acc4[u][i] += (float)src[i];
          }
        }
      }
      float acc[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = (acc4[0][i] + acc4[1][i]) + (acc4[2][i] + acc4[3][i]);
      // the C partial sums meet in a fixed tree of lane exchanges (group c takes group c + s, s = 1, 2, 4, ...): through LDS, lane
      // group 0 adding the others one by one, the fold was C - 1 dependent LDS reads per run
      for (int sft = 1; sft < C; sft <<= 1) {
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = __shfl(acc[i], (lane + sft * KQ) & 63, 64);
        if (c < C && (c & (2 * sft - 1)) == 0 && c + sft < C) {
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[i] += o[i];
        }
      }
      if (c == 0) epi(rl, kq, acc, pr0[0]);
    }
  }
}

// the grid of a kernel that walks R sorted positions with embed_run_sums: a workgroup's 4 waves take C positions each per iteration
inline dim3 run_sums_grid(long R, int K) {
  const int C = 64 / ((K + 3) / 4);
  return dim3((int)std::min<long>((R + 4 * C - 1) / (4 * C), 256 * 32));
}

}  // namespace fil
