// N3  Top-k retrieval over a long behaviour history for gfx950 (the General Search Unit of the Search-based Interest Model): score every
// live slot of a history straight from the embedding table, keep the k best, write them in time order.  Forward only, integer results.
//
// hist_idx [B,T] field-local ids.  A slot is LIVE iff id != pad_id, 0 <= id < size (size < 0: ids are trusted), mask is NULL or non-zero
// there, and attr is NULL or attr[b,t] == cand[b].  An id that is not pad_id and lies outside [0, size) is counted in *oob_count whatever
// mask and attr say.  A slot that is not live issues no table read.
//   score  s = +0; for j ascending: s = s + (row[j] * q[b,j])  -- one lane, every product and every sum rounded to fp32 on its own
//          (fp contract(off): hipcc would fuse a * b + c), so a sequential fp32 restatement gives the same bits.  Without the soft part
//          (table == NULL) the score is +0.
//   key    bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000): the unsigned order of the keys is the order of the scores, -0 < +0, +-inf are
//          ordinary values and a NaN is some key like any other -- the selection below is a matter of integers only.
//   select the n = min(k, live) largest slots by (key descending, position ascending -- descending with FIL_SEARCH_PREFER_LAST).
//   write  the selected slots in ascending position; the tail n..k-1 is -1 / pad_id / +0; count[b] = n.
//
// Geometry: one workgroup per sample (64 threads when T <= 64, 256 otherwise), at most kSearchCap workgroups, past that a workgroup walks
// samples blockIdx.x, + gridDim.x, ...  Phase 1: thread i of the workgroup owns slots i, i + threads, ...: it reads the id (coalesced), the
// whole row with 16-byte loads, and leaves the key in LDS; a wave's ballot of "live" is that 64-slot chunk's word of the live bitmap.
// Phase 2 (only when live > k and there are scores): a radix select on the keys, 4 passes of 8 bits from the top: an LDS histogram of the
// digit over the slots that match the prefix so far (integer LDS atomics), then wave 0 walks the bins from the top with a shuffle scan
// and fixes the digit of the k-th largest key.  It ends with the exact threshold key, the number `need` of slots equal to it that are
// still wanted and their total `ties`.  Phase 3: every wave owns a contiguous range of chunks; it counts its slots above and at the
// threshold (ballot + popcount), the counts of the waves before it give its bases, and a second walk over the same chunks turns
// (slots above before me, ties before me) into the output place: above + min(ties_before, need), or with PREFER_LAST
// above + max(0, ties_before - (ties - need)).  Nothing but the ids, the live rows, q and the [B,k] outputs touches global memory; no
// float atomics; every count is an integer, so repeats are bit-identical and a sample does not depend on its batch.
#include "common.h"
#include "tiled_launch.h"
#include <cstdint>

namespace fil {

constexpr int kSearchCap = 4096;       // grid cap (workgroups)
constexpr int kSearchMaxT = 16384;
constexpr int kSearchMaxK = 64;
constexpr int kSearchMaxSel = 256;     // what fil_din_* takes downstream
constexpr uint32_t kKeyZero = 0x80000000u;   // the key of +0

struct SearchArgs {
  const int64_t* hist;
  const unsigned char* mask;
  const float* table;
  const float* q;
  const int64_t* attr;
  const int64_t* cand;
  int* sel_pos;
  int64_t* sel_idx;
  int* count;
  float* sel_score;
  int* oob_count;
  int64_t offset, size, pad_id, hist_stride, attr_stride, q_stride;
  int B, T, K, k, prefer_last;
};

// LDS image: q [K] floats | keys [T rounded up to 4] | live bitmap [ceil(T/64)] 64-bit words | histogram [256] | 16 ints of hand-over
static inline int search_lds_bytes(int T, int K) { return 4 * (K + (T + 3) / 4 * 4) + 8 * ((T + 63) / 64) + 4 * 256 + 4 * 16; }
static inline int search_threads(int T) { return T <= 64 ? 64 : 256; }

#ifdef __HIPCC__
__device__ __forceinline__ uint32_t score_key(float s) {
  const uint32_t u = __float_as_uint(s);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key_score(uint32_t key) { return __uint_as_float((key >> 31) ? key ^ 0x80000000u : ~key); }

// four steps of the score.  HIP's __fmul_rn / __fadd_rn are plain * and +, which hipcc contracts into a fused multiply-add by default:
// the pragma is what keeps every product rounded on its own.
__device__ __forceinline__ float dot_step(float s, const float4 r, const float4 w) {
#pragma clang fp contract(off)
  s = s + r.x * w.x;
  s = s + r.y * w.y;
  s = s + r.z * w.z;
  s = s + r.w * w.w;
  return s;
}

// KQ = K / 4 when it is known at compile time (the whole row is then requested before the first product), 0 = read K at run time
template <int KQ>
__global__ __launch_bounds__(256) void seq_search_kernel(const SearchArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int T = a.T, K = a.K, k = a.k;
  const int C = (T + 63) >> 6;
  float* s_q = reinterpret_cast<float*>(smem);
  uint32_t* s_key = reinterpret_cast<uint32_t*>(s_q + K);
  unsigned long long* s_live = reinterpret_cast<unsigned long long*>(s_key + (T + 3) / 4 * 4);
  int* s_hist = reinterpret_cast<int*>(s_live + C);
  int* s_misc = s_hist + 256;   // [0..3] live per wave | [4..7] above per wave | [8] digit [9] need [10] ties | [12..15] ties per wave
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  const bool soft = a.table != nullptr;
  const unsigned long long below = (1ull << lane) - 1ull;

  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const int64_t* ids = a.hist + (long)b * a.hist_stride;
    const int64_t* at = a.attr != nullptr ? a.attr + (long)b * a.attr_stride : nullptr;
    const unsigned char* mk = a.mask != nullptr ? a.mask + (long)b * T : nullptr;
    const int64_t want = at != nullptr ? a.cand[b] : 0;
    if (soft)
      for (int j = tid; j < K; j += nt) s_q[j] = a.q[(long)b * a.q_stride + j];
    __syncthreads();   // q is staged; the previous sample's readers of the image are done

    // ---- phase 1: ids -> live, rows -> keys
    int nlive = 0, oob = 0;
    for (int base = 0; base < T; base += nt) {
      const int t = base + tid;
      bool live = false;
      int64_t id = 0;
      if (t < T) {
        id = ids[t];
        const bool slot = id != a.pad_id;
        const bool ok = a.size < 0 || (id >= 0 && id < a.size);
        oob += (slot && !ok) ? 1 : 0;
        live = slot && ok && (mk == nullptr || mk[t] != 0) && (at == nullptr || at[t] == want);
      }
      uint32_t key = kKeyZero;
      if (live && soft) {
        const float4* row = reinterpret_cast<const float4*>(a.table + (a.offset + id) * K);
        const float4* w = reinterpret_cast<const float4*>(s_q);
        float s = 0.f;
        if constexpr (KQ > 0) {
          float4 r[KQ];
#pragma unroll
          for (int c = 0; c < KQ; ++c) r[c] = row[c];
#pragma unroll
          for (int c = 0; c < KQ; ++c) s = dot_step(s, r[c], w[c]);
        } else {
          const int kq = K >> 2;
#pragma unroll 4
          for (int c = 0; c < kq; ++c) s = dot_step(s, row[c], w[c]);
        }
        key = score_key(s);
      }
      if (t < T) s_key[t] = key;
      const unsigned long long m = __ballot(live);
      if (lane == 0 && base + wave * 64 < T) s_live[(base >> 6) + wave] = m;
      nlive += __popcll(m);
    }
    if (lane == 0) s_misc[wave] = nlive;
    if (oob > 0 && a.oob_count != nullptr) atomicAdd(a.oob_count, oob);
    __syncthreads();
    int live_total = 0;
    for (int w = 0; w < nw; ++w) live_total += s_misc[w];
    const int n = live_total < k ? live_total : k;
    const bool take_all = live_total <= k;

    // ---- phase 2: the threshold key, how many of its slots are wanted, how many there are
    uint32_t thr = kKeyZero;
    int need = k, ties = live_total;   // no scores: every live slot ties at +0
    if (take_all) need = ties = 0;     // everything live is taken as "above": no slot counts as a tie
    if (!take_all && soft) {
      uint32_t prefix = 0;
      for (int p = 0; p < 4; ++p) {
        const int shift = 24 - 8 * p;
        for (int i = tid; i < 256; i += nt) s_hist[i] = 0;
        __syncthreads();
        for (int t = tid; t < T; t += nt) {
          const uint32_t key = s_key[t];
          const bool live = (s_live[t >> 6] >> (t & 63)) & 1ull;
          if (live && (p == 0 || (key >> (shift + 8)) == prefix)) atomicAdd(&s_hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        if (wave == 0) {   // lane l owns bins 4l .. 4l+3; `above` = the slots in the bins over them
          const int h0 = s_hist[4 * lane], h1 = s_hist[4 * lane + 1], h2 = s_hist[4 * lane + 2], h3 = s_hist[4 * lane + 3];
          const int own = h0 + h1 + h2 + h3;
          int v = own;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_down(v, o);
            if (lane + o < 64) v += u;
          }
          int above = v - own;
          const int hs[4] = {h3, h2, h1, h0};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (above < need && above + hs[j] >= need) {
              s_misc[8] = 4 * lane + 3 - j;
              s_misc[9] = need - above;
              s_misc[10] = hs[j];
            }
            above += hs[j];
          }
        }
        __syncthreads();
        prefix = (prefix << 8) | (uint32_t)s_misc[8];
        need = s_misc[9];
        ties = s_misc[10];
      }
      thr = prefix;
    }

    // ---- phase 3: ordered compaction, a contiguous range of chunks per wave
    const int c0 = wave * C / nw, c1 = (wave + 1) * C / nw;
    int n_above = 0, n_ties = 0;
    for (int c = c0; c < c1; ++c) {
      const int t = c * 64 + lane;
      const uint32_t key = t < T ? s_key[t] : 0u;
      const bool live = (s_live[c] >> lane) & 1ull;
      n_above += __popcll(__ballot(live && (take_all || key > thr)));
      n_ties += __popcll(__ballot(live && !take_all && key == thr));
    }
    if (lane == 0) {
      s_misc[4 + wave] = n_above;
      s_misc[12 + wave] = n_ties;
    }
    __syncthreads();
    int above_before = 0, ties_before = 0;
    for (int w = 0; w < wave; ++w) {
      above_before += s_misc[4 + w];
      ties_before += s_misc[12 + w];
    }
    const int skip = ties - need;   // PREFER_LAST: the first `skip` slots at the threshold are left out
    int* pos_out = a.sel_pos + (long)b * k;
    int64_t* idx_out = a.sel_idx + (long)b * k;
    float* score_out = a.sel_score != nullptr ? a.sel_score + (long)b * k : nullptr;
    for (int c = c0; c < c1; ++c) {
      const int t = c * 64 + lane;
      const uint32_t key = t < T ? s_key[t] : 0u;
      const bool live = (s_live[c] >> lane) & 1ull;
      const bool is_above = live && (take_all || key > thr);
      const bool is_tie = live && !take_all && key == thr;
      const unsigned long long ma = __ballot(is_above), me = __ballot(is_tie);
      const int my_above = above_before + __popcll(ma & below);
      const int my_tie = ties_before + __popcll(me & below);
      int tie_taken;   // the slots at the threshold before this one that are selected
      bool taken;
      if (a.prefer_last) {
        tie_taken = my_tie > skip ? my_tie - skip : 0;
        taken = is_above || (is_tie && my_tie >= skip);
      } else {
        tie_taken = my_tie < need ? my_tie : need;
        taken = is_above || (is_tie && my_tie < need);
      }
      const int place = my_above + tie_taken;
      if (taken && place < k) {
        pos_out[place] = t;
        idx_out[place] = ids[t];
        if (score_out != nullptr) score_out[place] = key_score(key);
      }
      above_before += __popcll(ma);
      ties_before += __popcll(me);
    }
    for (int j = n + tid; j < k; j += nt) {
      pos_out[j] = -1;
      idx_out[j] = a.pad_id;
      if (score_out != nullptr) score_out[j] = 0.f;
    }
    if (tid == 0) a.count[b] = n;
  }
}
#endif

// the dimensions and the menu, for the plan and the launch alike; *lds = the dynamic LDS of one workgroup
static int search_dims(const char* who, int B, int T, int K, int k, int* lds) {
  FIL_CHECK_ARG_W(who, B >= 0 && T >= 1 && K >= 1 && k >= 1);
  if (K % 4 != 0 || K > kSearchMaxK) return fail(FIL_ERR_UNSUPPORTED, "%s: K=%d (K %% 4 == 0 and K <= %d)", who, K, kSearchMaxK);
  if (k > kSearchMaxSel) return fail(FIL_ERR_UNSUPPORTED, "%s: k=%d > %d (k <= %d, what fil_din_* takes)", who, k, kSearchMaxSel, kSearchMaxSel);
  if (T > kSearchMaxT) return fail(FIL_ERR_UNSUPPORTED, "%s: T=%d > %d (T <= %d)", who, T, kSearchMaxT, kSearchMaxT);
  if ((long)B * T >= (1L << 31)) return fail(FIL_ERR_UNSUPPORTED, "%s: B*T = %ld slots >= 2^31", who, (long)B * T);
  *lds = search_lds_bytes(T, K);
  if (*lds > kTiledLdsLimit)
    return fail(FIL_ERR_UNSUPPORTED, "%s: %d bytes of dynamic LDS > %d", who, *lds, kTiledLdsLimit);
  return FIL_OK;
}

}  // namespace fil

using namespace fil;

extern "C" int fil_seq_search_plan(int B, int T, int K, int k, int* plan) {
  int lds;
  if (int rc = search_dims(__func__, B, T, K, k, &lds)) return rc;
  FIL_CHECK_ARG(plan != nullptr);
  tiled_plan(plan, 1, tiled_grid(B, 1, kSearchCap), kSearchCap, lds, 0);   // forward only: the backward fields are 1 / 0
  return FIL_OK;
}

extern "C" int fil_seq_search(const int64_t* hist_idx, int64_t hist_stride, int64_t offset, int64_t size, int64_t pad_id,
                              const unsigned char* mask, const float* table, const float* q, int64_t q_stride, const int64_t* attr,
                              int64_t attr_stride, const int64_t* cand, int* sel_pos, int64_t* sel_idx, int* count, float* sel_score,
                              int* oob_count, int B, int T, int K, int k, int flags, void* stream) {
  int lds;
  if (int rc = search_dims(__func__, B, T, K, k, &lds)) return rc;
  if (flags & ~FIL_SEARCH_PREFER_LAST) return fail(FIL_ERR_ARG, "fil_seq_search: unknown flags 0x%x (FIL_SEARCH_PREFER_LAST)", flags);
  if (B == 0) return FIL_OK;
  FIL_CHECK_ARG(hist_idx && sel_pos && sel_idx && count);
  FIL_CHECK_ARG((table != nullptr) == (q != nullptr));        // the soft part: both or neither
  FIL_CHECK_ARG((attr != nullptr) == (cand != nullptr));      // the hard part: both or neither
  FIL_CHECK_ARG(table != nullptr || attr != nullptr);         // at least one part
  FIL_CHECK_ARG(hist_stride >= T);
  FIL_CHECK_ARG(attr == nullptr || attr_stride >= T);
  FIL_CHECK_ARG(q == nullptr || q_stride >= K);
  FIL_CHECK_ARG(table == nullptr || offset >= 0);
  FIL_CHECK_ARG((reinterpret_cast<uintptr_t>(table) & 15) == 0);   // rows are read with 16-byte loads
  SearchArgs a;
  a.hist = hist_idx;
  a.mask = mask;
  a.table = table;
  a.q = q;
  a.attr = attr;
  a.cand = cand;
  a.sel_pos = sel_pos;
  a.sel_idx = sel_idx;
  a.count = count;
  a.sel_score = sel_score;
  a.oob_count = oob_count;
  a.offset = offset;
  a.size = size;
  a.pad_id = pad_id;
  a.hist_stride = hist_stride;
  a.attr_stride = attr_stride;
  a.q_stride = q_stride;
  a.B = B;
  a.T = T;
  a.K = K;
  a.k = k;
  a.prefer_last = (flags & FIL_SEARCH_PREFER_LAST) ? 1 : 0;
  const dim3 grid(tiled_grid(B, 1, kSearchCap)), block(search_threads(T));
  hipStream_t st = (hipStream_t)stream;
  // bytes: the ids, q, the outputs; the live rows are data-dependent and not counted
  ProfScope prof("seq_search", st, 8.0 * B * T + 4.0 * B * K + 16.0 * B * k);
#define FIL_SEARCH_LAUNCH(KQ)                                                                   \
  do {                                                                                          \
    if (int rc = tiled_allow_lds(__func__, seq_search_kernel<KQ>, lds)) return rc;              \
    hipLaunchKernelGGL(seq_search_kernel<KQ>, grid, block, lds, st, a);                         \
  } while (0)
  if (K == 16)
    FIL_SEARCH_LAUNCH(4);
  else if (K == 8)
    FIL_SEARCH_LAUNCH(2);
  else if (K == 32)
    FIL_SEARCH_LAUNCH(8);
  else
    FIL_SEARCH_LAUNCH(0);
#undef FIL_SEARCH_LAUNCH
  FIL_CHECK_LAUNCH();
  return FIL_OK;
}
