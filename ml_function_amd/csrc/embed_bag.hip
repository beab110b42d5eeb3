// N3  Pooled multi-valued sparse fields for gfx950: gather + sum / mean / sqrtn of a bag's rows in one launch, and the two small
// launches that turn its gradient into a runs record of the form the one-id consumers already take.
//
// idx [B,F,T]: T slots per sample and field.  A slot is padding iff id == pad_id, out of range iff it is not padding and
// id < 0 or id >= sizes[f]; the n remaining LIVE slots of a bag are summed in fp32 in ascending t and the sum is divided ONCE
// (mean: by (float)n, sqrtn: by sqrtf((float)n); n = 0: a zero row) -- tf.nn.safe_embedding_lookup_sparse without weights.  No
// reciprocal, no multiply feeding an add: the output is bit-equal to a sequential fp32 restatement.
//
// Geometry = the gather's (embed.hip): ceil(K/4) lanes own one bag, 16-byte row accesses when K % 4 == 0, grid-stride loop.  A bag's ids
// are read once, kBagSlots at a time; the rows of the live ones among them are requested together (independent loads), then added in
// slot order.  A padding or out-of-range slot issues no load: its addend is the constant +0, and x + (+0) == x bit for bit for every x
// this sum can hold (it starts at +0, so it is never -0).
//
// Gradient: fil_embed_bag_row_ids writes the global row id of every SLOT (-1: padding / out of range / frozen field), the caller
// sorts them stably (slot_perm), and fil_embed_bag_bwd_prep divides the incoming rows by the forward's divisor (gs = g / scale) and maps
// every sorted slot back to its bag (perm = slot_perm / T = b F + f).  (gs, perm, sorted_ids, R = B F T, F) is then a record that
// fil_embed_run_sum_dt, fil_embed_segment_sum, fil_embed_runs_compact and every fused optimizer read as it stands: they take the
// gradient row as g[perm[j]] and the field as perm[j] % F.
#include "common.h"
#include <cstdint>

namespace fil {

constexpr int kBagSlots = 8;   // slots whose rows are in flight before the first add
constexpr int kWaitVm0 = 0x0F70;   // s_waitcnt vmcnt(0) alone on gfx9: vmcnt = bits 15:14 | 3:0, expcnt (6:4) and lgkmcnt (11:8) at their maxima

template <bool VEC>
__global__ __launch_bounds__(256) void embed_bag_fwd_kernel(const float* __restrict__ table, const int64_t* __restrict__ offsets,
                                                            const int64_t* __restrict__ sizes, const int64_t* __restrict__ idx,
                                                            int64_t pad_id, float* __restrict__ out, int* __restrict__ count,
                                                            int* __restrict__ oob_count, long bags, int F, int T, int K, int combiner) {
  const int KQ = (K + 3) / 4;
  const long total = bags * KQ;
  const bool has_pad = pad_id != FIL_BAG_NO_PAD;
  for (long w = (long)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (long)gridDim.x * blockDim.x) {
    const long bag = w / KQ;
    const int kq = (int)(w - bag * KQ);
    const int f = (int)(bag % F);
    const int64_t off = offsets[f];
    const int64_t vf = sizes != nullptr ? sizes[f] : INT64_MAX;
    const int64_t* ids = idx + bag * T;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int n = 0, oob = 0;
    for (int t0 = 0; t0 < T; t0 += kBagSlots) {
      int64_t id[kBagSlots];
#pragma unroll
      for (int u = 0; u < kBagSlots; ++u) id[u] = ids[t0 + u < T ? t0 + u : T - 1];
      // every id has arrived before the first row is asked for (s_waitcnt vmcnt(0)): the row requests then follow each other with no
      // wait in between.  Left to the compiler, each request waits for its own id only, and since a request may be skipped it counts
      // the ones before it conservatively: the rows then come back in three dependent rounds instead of one.
      __builtin_amdgcn_s_waitcnt(kWaitVm0);
      bool live[kBagSlots];
#pragma unroll
      for (int u = 0; u < kBagSlots; ++u) {
        const bool slot = t0 + u < T && !(has_pad && id[u] == pad_id);
        const bool ok = id[u] >= 0 && id[u] < vf;
        live[u] = slot && ok;
        n += live[u] ? 1 : 0;
        oob += (slot && !ok) ? 1 : 0;
      }
      float v[kBagSlots][4];
#pragma unroll
      for (int u = 0; u < kBagSlots; ++u) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[u][i] = 0.f;
        if (live[u]) {
          const float* src = table + (off + id[u]) * K + kq * 4;
          if constexpr (VEC) {
            const float4 r = *reinterpret_cast<const float4*>(src);
            v[u][0] = r.x;
            v[u][1] = r.y;
            v[u][2] = r.z;
            v[u][3] = r.w;
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (kq * 4 + i < K) v[u][i] = src[i];
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < kBagSlots; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += v[u][i];
    }
    if (combiner != FIL_BAG_SUM && n > 0) {
      const float d = combiner == FIL_BAG_MEAN ? (float)n : sqrtf((float)n);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = acc[i] / d;
    }
    float* dst = out + bag * K + kq * 4;
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (kq * 4 + i < K) dst[i] = acc[i];
    }
    if (kq == 0) {
      count[bag] = n;
      if (oob > 0 && oob_count != nullptr) atomicAdd(oob_count, oob);
    }
  }
}

// global row id of every slot, in slot order (b F + f) T + t; -1 for a padding / out-of-range slot and for a frozen field
__global__ __launch_bounds__(256) void embed_bag_row_ids_kernel(const int64_t* __restrict__ offsets, const int64_t* __restrict__ sizes,
                                                                const unsigned char* __restrict__ frozen, const int64_t* __restrict__ idx,
                                                                int64_t pad_id, int64_t* __restrict__ row_ids, long R, int F, int T) {
  const bool has_pad = pad_id != FIL_BAG_NO_PAD;
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (long)gridDim.x * blockDim.x) {
    const int f = (int)((r / T) % F);
    const int64_t id = idx[r];
    const bool ok = !(has_pad && id == pad_id) && (sizes == nullptr || (id >= 0 && id < sizes[f])) && (frozen == nullptr || !frozen[f]);
    row_ids[r] = ok ? offsets[f] + id : -1;
  }
}

// gs[bag,:] = g[bag,:] / the forward's divisor of the bag (n = 0: zeros, never read -- such a bag has no slot with a row id), and
// perm[j] = slot_perm[j] / T (elementwise: perm may be slot_perm itself).  gs == nullptr (sum): only the permutation.
__global__ __launch_bounds__(256) void embed_bag_bwd_prep_kernel(const float* __restrict__ g, const int* __restrict__ count,
                                                                 const int64_t* slot_perm, float* __restrict__ gs, int64_t* perm,
                                                                 long bags, int T, int K, int combiner, long R) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nt = (long)gridDim.x * blockDim.x;
  if (gs != nullptr) {
    const long total = bags * K;
    for (long e = tid; e < total; e += nt) {
      const int n = count[e / K];
      const float d = combiner == FIL_BAG_MEAN ? (float)n : sqrtf((float)n);
      gs[e] = n > 0 ? g[e] / d : 0.f;
    }
  }
  for (long j = tid; j < R; j += nt) perm[j] = (int64_t)((unsigned)slot_perm[j] / (unsigned)T);   // (R < 2^31)
}

static int bag_dims(const char* who, int B, int F, int T, int K, long* R) {
  FIL_CHECK_ARG_W(who, B >= 0 && F >= 1 && T >= 1 && K >= 1);
  if (K > 256) return fail(FIL_ERR_UNSUPPORTED, "%s: K=%d > 256 (the run sums' limit)", who, K);
  *R = (long)B * F * T;
  if (*R >= (1L << 31)) return fail(FIL_ERR_UNSUPPORTED, "%s: B*F*T = %ld slots >= 2^31", who, *R);
  return FIL_OK;
}

static bool bag_combiner(int c) { return c == FIL_BAG_SUM || c == FIL_BAG_MEAN || c == FIL_BAG_SQRTN; }

}  // namespace fil

using namespace fil;

extern "C" int fil_embed_bag_fwd(const float* table, const int64_t* offsets, const int64_t* sizes, const int64_t* idx, int64_t pad_id,
                                 float* out, int* count, int* oob_count, int B, int F, int T, int K, int combiner, void* stream) {
  long R;
  if (int rc = bag_dims(__func__, B, F, T, K, &R)) return rc;
  if (!bag_combiner(combiner)) return fail(FIL_ERR_ARG, "fil_embed_bag_fwd: combiner %d (FIL_BAG_SUM, _MEAN or _SQRTN)", combiner);
  if (B == 0) return FIL_OK;
  FIL_CHECK_ARG(table && offsets && idx && out && count);
  const long bags = (long)B * F;
  const long total = bags * ((K + 3) / 4);
  const dim3 grid((int)std::min<long>((total + 255) / 256, FIL_BAG_MAX_BLOCKS));
  if (K % 4 == 0)
    hipLaunchKernelGGL(embed_bag_fwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, table, offsets, sizes, idx, pad_id, out, count,
                       oob_count, bags, F, T, K, combiner);
  else
    hipLaunchKernelGGL(embed_bag_fwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, table, offsets, sizes, idx, pad_id, out, count,
                       oob_count, bags, F, T, K, combiner);
  FIL_CHECK_LAUNCH();
  return FIL_OK;
}

extern "C" int fil_embed_bag_row_ids(const int64_t* offsets, const int64_t* sizes, const unsigned char* frozen, const int64_t* idx,
                                     int64_t pad_id, int64_t* row_ids, int B, int F, int T, void* stream) {
  long R;
  if (int rc = bag_dims(__func__, B, F, T, 1, &R)) return rc;
  if (B == 0) return FIL_OK;
  FIL_CHECK_ARG(offsets && idx && row_ids);
  hipLaunchKernelGGL(embed_bag_row_ids_kernel, dim3((int)std::min<long>((R + 255) / 256, FIL_BAG_MAX_BLOCKS)), dim3(256), 0,
                     (hipStream_t)stream, offsets, sizes, frozen, idx, pad_id, row_ids, R, F, T);
  FIL_CHECK_LAUNCH();
  return FIL_OK;
}

extern "C" int fil_embed_bag_bwd_prep(const float* g, const int* count, const int64_t* slot_perm, float* gs, int64_t* perm, int B, int F,
                                      int T, int K, int combiner, void* stream) {
  long R;
  if (int rc = bag_dims(__func__, B, F, T, K, &R)) return rc;
  if (!bag_combiner(combiner)) return fail(FIL_ERR_ARG, "fil_embed_bag_bwd_prep: combiner %d (FIL_BAG_SUM, _MEAN or _SQRTN)", combiner);
  if (B == 0) return FIL_OK;
  FIL_CHECK_ARG(slot_perm && perm);
  if (combiner == FIL_BAG_SUM) {
    FIL_CHECK_ARG(gs == nullptr);          // sum: the incoming rows are the record's rows as they are
  } else {
    FIL_CHECK_ARG(g && count && gs);
  }
  const long bags = (long)B * F;
  const long work = std::max<long>(gs != nullptr ? bags * K : 0, R);
  hipLaunchKernelGGL(embed_bag_bwd_prep_kernel, dim3((int)std::min<long>((work + 255) / 256, FIL_BAG_MAX_BLOCKS)), dim3(256), 0,
                     (hipStream_t)stream, g, count, slot_perm, gs, perm, bags, T, K, combiner, R);
  FIL_CHECK_LAUNCH();
  return FIL_OK;
}
