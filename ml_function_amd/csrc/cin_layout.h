// A3  xDeepFM CIN, host side: what a call's shape decides before anything is launched -- the shape and its limits, the tuning knobs,
// the launch plans that size buffers, the fused tail's geometry, and the LAYOUT of the three buffers a caller allocates (`saved`, the
// forward workspace, the backward workspace).  Each buffer is declared once, by the lay_out walk of its struct; the sizes
// fil_cin_*_bytes report and the pointers the launchers of cin.hip use both come from that walk.
#pragma once
#include "cin_kernels.h"
#include "cin_tail.h"
#include "cin_launch.h"
#include "cin_qtail.h"
#include "cin_qsplit.h"
#include "cin_qmerge.h"

#include <stdlib.h>

namespace fil {

struct CinShape {
  int B, F, K, L;
  int H[kCinMaxL];
  int Hp(int l) const { return l == 0 ? F : H[l - 1]; }
  int HS(int l) const { return 128 * cdiv(H[l], 128); }   // row stride of layer l's feature map / gradient
  int xps(int l) const { return l == 0 ? F : HS(l - 1); } // row stride of x^{l-1}
  long M() const { return (long)B * K; }
  int JT() const { return cin_jt_of(F); }
  int HSmax() const {
    int h = 0;
    for (int l = 0; l < L; ++l) h = std::max(h, HS(l));
    return h;
  }
};

static int check_shape(const char* fn, int B, int F, int K, int L, const int* H, CinShape& s) {
  if (B < 0 || F < 1 || K < 1 || L < 1 || H == nullptr) return fail(FIL_ERR_ARG, "%s: bad shape B=%d F=%d K=%d L=%d", fn, B, F, K, L);
  if (L > kCinMaxL) return fail(FIL_ERR_UNSUPPORTED, "%s: L=%d > %d", fn, L, kCinMaxL);
  if (F > kCinMaxFields) return fail(FIL_ERR_UNSUPPORTED, "%s: F=%d > %d fields", fn, F, kCinMaxFields);
  if ((long)B * K > (1L << 28)) return fail(FIL_ERR_UNSUPPORTED, "%s: B*K = %ld rows > 2^28 (row-split byte offsets of the dW kernel are 32-bit)", fn, (long)B * K);
  s.B = B; s.F = F; s.K = K; s.L = L;
  for (int l = 0; l < L; ++l) {
    if (H[l] < 1) return fail(FIL_ERR_ARG, "%s: H[%d]=%d", fn, l, H[l]);
    if (H[l] > kCinMaxH) return fail(FIL_ERR_UNSUPPORTED, "%s: H[%d]=%d > %d feature maps", fn, l, H[l], kCinMaxH);
    s.H[l] = H[l];
  }
  return FIL_OK;
}

static int chunks_of(int H) { return cdiv(H, 128); }
// rows per wave of the row-parallel kernels: 64 when that still yields about one wave per SIMD (1024 SIMDs)
static int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v != nullptr && *v != 0 ? atoi(v) : dflt;
}
// Process-level tuning knobs, read from the environment ONCE (first call into the library), never on the launch path:
//   FIL_CIN_MB=1|2        rows per wave (x32) of the row-parallel kernels (default: by M)
//   FIL_CIN_SYM=0         symmetric first-layer kernels off
//   FIL_CIN_DW_MB, FIL_CIN_DW_SPLITS, FIL_CIN_DZ_MB   launch shape of the dW / dZ kernels
//   FIL_CIN_TAIL_SPLITS   row splits of the fused tail's weight-gradient kernel
//   FIL_CIN_KSPLIT=0|4    reduction split of the row-parallel kernels over the 4 waves of a workgroup (default: by M)
//   FIL_CIN_QMERGE=0      quadratic tail: two weight-gradient launches (first layer, quadratic form) instead of the merged one
//   FIL_CIN_DZ2=0         ... its two data-gradient passes as two launches of the pair-symmetric dZ kernel instead of one two-pass launch
//   FIL_CIN_FWDQ=0        ... its forward as two 128-column launches + the pool kernel instead of the 256-column launch with fused pools
//   FIL_CIN_HEADFOLD=0    ... the pooled relayout + Dense(1) head as their own launch instead of the 256-column launch's epilogue
//   FIL_CIN_PACKFOLD=0    ... T's two operand layouts by a pack launch instead of by the T workgroups themselves (exact mode)
//   FIL_CIN_DWFOLD4=0     ... the merged weight-gradient launch folds PAIRS of row splits (4 tiles x 2 splits per workgroup) instead of quads
//   FIL_CIN_GHAT=0        ... the forward saves R itself and cin_last_bwd2_kernel builds G1 from it, instead of the forward saving the
//                         g-free G1 in R's place (cin_ghat_used, cin.hip)
//   FIL_CIN_SHORTDX=0     ... the shortcut's data gradient by cin_last_bwd2_kernel's phase u instead of cin_shortcut_dx_kernel (cin_shortdx_used,
//                         cin.hip)
// Results are identical up to summation order whatever they say.  Per-call overrides for tests travel in `mode`
// (FIL_CIN_MB2, FIL_CIN_NOSYM), not through the environment.
struct Knobs {
  int mb, sym, dw_mb, dw_splits, dz_mb, tail_splits, tail_settle, tail_dz_mode, ksplit, dzs_mb, qtail, qmerge, dz2, fwdq, headfold, packfold, dwfold4, ghat, shortdx;
};
static const Knobs& knobs() {
  static const Knobs k = {env_int("FIL_CIN_MB", 0), env_int("FIL_CIN_SYM", 1), env_int("FIL_CIN_DW_MB", 1), env_int("FIL_CIN_DW_SPLITS", 0),
                          env_int("FIL_CIN_DZ_MB", 1), env_int("FIL_CIN_TAIL_SPLITS", 0), env_int("FIL_CIN_TAIL_SETTLE", 0), env_int("FIL_CIN_TAIL_DZ_MODE", 0), env_int("FIL_CIN_KSPLIT", -1), env_int("FIL_CIN_DZS_MB", 0), env_int("FIL_CIN_QTAIL", 1), env_int("FIL_CIN_QMERGE", 1), env_int("FIL_CIN_DZ2", 1), env_int("FIL_CIN_FWDQ", 1), env_int("FIL_CIN_HEADFOLD", 1), env_int("FIL_CIN_PACKFOLD", 1), env_int("FIL_CIN_DWFOLD4", 1), env_int("FIL_CIN_GHAT", 1), env_int("FIL_CIN_SHORTDX", 1)};
  return k;
}
// per-call view of the knobs: the process defaults with the call's mode bits applied
struct CinTune {
  int mb_forced;
  bool sym, no_ksplit;
  CinTune() : CinTune(0) {}
  explicit CinTune(int mode)
      : mb_forced((mode & FIL_CIN_MB2) ? 2 : knobs().mb), sym(knobs().sym != 0 && !(mode & FIL_CIN_NOSYM)), no_ksplit((mode & FIL_CIN_NOKSPLIT) != 0) {}
  int mb_rows(long M) const {
    if (mb_forced == 1 || mb_forced == 2) return mb_forced;
    return cdiv((int)std::min<long>(M, 1L << 30), 64) >= 768 ? 2 : 1;
  }
  // Small M (a strong-scaling shard: 512 samples x K = 16 is 256 blocks of 32 rows for 1024 SIMDs): a wave reduces over ALL
  // channels of its rows, so below one row block per SIMD the row-parallel kernels stop getting faster.  ks = 4 gives a row
  // block to the four waves of a workgroup, which split the reduction (h range / periods) and fold their partial sums through
  // LDS.  Used when that still leaves at most two waves per SIMD; exact kernels with 32-row blocks only.
  int ksplit(long M) const {
    if (knobs().ksplit == 0 || no_ksplit) return 1;
    if (mb_rows(M) != 1) return 1;
    if (knobs().ksplit == 4) return 4;
    return cdiv((int)std::min<long>(M, 1L << 30), 32) <= 512 ? 4 : 1;
  }
};

// ---- weight-gradient launch plan: waves over channel tiles x splits of the m range ~ one wave per SIMD
struct DwPlan {
  int MB, blocks_x, splits, rows_per_split, chunks;
};
static int cu_count() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    return v;
  }();
  return n;
}

// Row splits of the dW GEMM, from a launch-time model fitted on MI355X (profiles/r01_dw_split_sweep.txt).
// Workgroups are dealt evenly over the CUs, at most 3 resident per CU, in rounds of 3*CUs; a round with r resident
// workgroups per CU spends t(r) = {1.05, 1.39, 1.96} * 1e-4 ms per row of its split (two resident waves per SIMD
// already cover the MFMA pipe, so a third adds its full share of time); each split also costs one partial [C,H]
// write + re-read in the reduction (served from the Infinity Cache, about 6 TB/s).  Pick the cheapest split count.
static DwPlan dw_plan(long M, int C, int H) {
  DwPlan p;
  p.chunks = chunks_of(H);
  p.MB = knobs().dw_mb == 2 ? 2 : 1;   // 64 rows per wave measured slower (67 vs 122 TFLOP/s)
  const int waves_c = cdiv(C, 32 * p.MB);
  p.blocks_x = cdiv(waves_c, 4);
  const long tiles = (long)p.blocks_x * p.chunks;
  const long ncu = cu_count();
  const long unit = 2 * kDwDepth;
  auto rows_of = [&](int splits) { return std::max<long>(unit, ((M + splits - 1) / splits + unit - 1) / unit * unit); };
  int best = knobs().dw_splits;
  if (best <= 0) {
    static const double t_of[4] = {0.0, 1.05e-4, 1.39e-4, 1.96e-4};
    double best_ms = -1.0;
    // a split's byte offsets (rows * up to 1 KiB) must stay below 2^31: at most 2^20 rows per split
    for (int sp = (int)std::max<long>(1, (M + (1L << 20) - 1) >> 20); sp <= 256; ++sp) {
      const long rps = rows_of(sp);
      const long real = (M + rps - 1) / rps;           // splits that actually get rows
      if (real != sp && sp > 1) continue;              // same plan as a smaller sp
      long wgs = tiles * real;
      double per_row = 0.0;
      while (wgs > 0) {
        const long round = std::min(wgs, 3 * ncu);
        per_row += t_of[std::min<long>(3, (round + ncu - 1) / ncu)];
        wgs -= round;
      }
      const double ms = (double)rps * per_row * p.MB + (double)real * C * H * 4.0 / 6e9;
      if (best_ms < 0 || ms < best_ms) best = sp, best_ms = ms;
      if (rps == unit) break;
    }
  }
  best = std::min(std::max(best, 1), 256);
  const long rps = rows_of(best);
  p.rows_per_split = (int)rps;
  p.splits = (int)std::max<long>(1, (M + rps - 1) / rps);
  return p;
}

// ---- fused tail (cin_tail.h): geometry of the last two layers handled as one implicit GEMM with F+2 columns
struct TailGeom {
  bool on = false;
  int p = 0;                       // index of the lower tail layer (L-2); the upper one is L-1
  int NCB = 0, JP = 0, JT4 = 0, NQ = 0, JHp = 0;
  int Hpp = 0, Hq = 0, HL = 0, Cp = 0, C1 = 0;
  int periods = 0, tiles = 0;      // dZ stream (slot order of cin_pack_wz_kernel, one tile past the end)
  size_t uf_floats = 0, uz_floats = 0;
};
static TailGeom tail_geom(const CinShape& s) {   // what the tail WOULD look like (independent of mode: buffer sizes use it)
  TailGeom g;
  if (s.L < 3 || !cin_tail_supported(s.F)) return g;
  g.on = true;
  g.p = s.L - 2;
  g.NCB = cin_tail_ncb(s.F);
  g.JP = 16 * g.NCB;
  g.JT4 = cin_tail_jt4(s.F);
  g.NQ = cin_tail_nq(s.F);
  g.JHp = 4 * g.NQ;
  g.Hpp = s.H[g.p - 1];
  g.Hq = s.H[g.p];
  g.HL = s.H[s.L - 1];
  g.Cp = g.Hpp * s.F;
  g.C1 = g.Cp + 1;
  const int JT = s.JT();
  g.periods = cin_dz_periods(g.Hpp, JT);
  g.tiles = cin_slot_tiles(g.Hpp, JT);
  g.uf_floats = (size_t)g.Hpp * g.JT4 * 64 * g.NCB + (size_t)align_up(g.JP + 1, 64);   // Uf | consts (beff[JP], sum bias_L)
  g.uz_floats = (size_t)g.tiles * 64 * g.JHp;
  return g;
}
struct TailDwPlan {
  int blocks_x, splits, rows_per_split;
};
static TailDwPlan tail_dw_plan(long M, int C1) {
  TailDwPlan p;
  p.blocks_x = cdiv(C1, 16 * kTailCbw);           // one workgroup per channel block and row split (its 4 waves quarter the split)
  const long unit = 4L * 4 * kTailDwDepth;        // a quarter of a split is a whole number of DEPTH-step groups
  // two workgroups per CU (two waves per SIMD: the second covers the first one's operand waits), all resident at once
  long want = knobs().tail_splits > 0 ? knobs().tail_splits : std::max<long>(1, 2L * cu_count() / p.blocks_x);
  want = std::max<long>(want, (M + (1L << 22) - 1) >> 22);   // byte offsets inside a split (rows * 256) stay below 2^31
  const long rows = std::max(unit, ((M + want - 1) / want + unit - 1) / unit * unit);
  p.rows_per_split = (int)rows;
  p.splits = (int)std::max<long>(1, (M + rows - 1) / rows);
  return p;
}

constexpr int kHeadChunk = 16;    // samples per block in the head partial reductions
constexpr int kColRows = 128;     // rows per block in the dbias (column-sum) partial reductions

static size_t wf_floats(const CinShape& s) {
  size_t w = 0;
  for (int l = 0; l < s.L; ++l) {
    w = std::max(w, (size_t)chunks_of(s.H[l]) * s.Hp(l) * 2 * s.JT() * 128);
  }
  w = std::max(w, (size_t)chunks_of(s.H[0]) * s.F * 2 * cin_jt_sym(s.F) * 128);   // the pair-symmetric first layer
  w += (size_t)2 * 2 * s.JT() * 128;   // + the packed pooled weights of a fused last layer (<= 2 chunks)
  return w;
}
static size_t wz_floats(const CinShape& s) {
  // symmetric first layer: its tile count and the pair-indexed dW sum both fit below
  size_t w = (size_t)cin_slot_tiles(s.F, cin_jt_sym(s.F)) * 32 * s.HS(0);
  w = std::max(w, (size_t)s.F * (s.F / 2 + 1) * s.H[0]);
  for (int l = 0; l < s.L; ++l) w = std::max(w, (size_t)cin_slot_tiles(s.Hp(l), s.JT()) * 32 * s.HS(l));
  return w;
}
// column chunks a layer's pooled partials may come in: its own, or (last layer pooled by the epilogue of the layer
// below) that layer's
static int pool_chunks(const CinShape& s, int l) { return std::max(chunks_of(s.H[l]), l > 0 ? chunks_of(s.H[l - 1]) : 1); }
// floats of the dW partial-sum buffer: the largest splits * C * H over the layers (both first-layer forms, so the
// size does not depend on the FIL_CIN_SYM knob) and the last layer's rank-one dW (C' = Hp, H' = F)
static size_t dw_part_floats(const CinShape& s) {
  size_t pmax = 0;
  for (int l = 0; l < s.L; ++l) pmax = std::max(pmax, (size_t)dw_plan(s.M(), s.Hp(l) * s.F, s.H[l]).splits * s.Hp(l) * s.F * s.H[l]);
  const int csym = s.F * (s.F / 2 + 1);
  pmax = std::max(pmax, (size_t)dw_plan(s.M(), csym, s.H[0]).splits * csym * s.H[0]);
  pmax = std::max(pmax, (size_t)dw_plan(s.M(), csym + s.F, s.H[0]).splits * (csym + s.F) * s.H[0]);   // quadratic tail: pairs + F single-field rows
  if (s.L == 3) pmax = std::max(pmax, (size_t)cin_dwq_plan(s.M(), csym + s.F + 1, cu_count()).pairs * (csym + s.F + 1) * 256);   // ... merged: 256 columns (+ the dbias_1 row)
  if (s.L == 3) pmax = std::max(pmax, (size_t)cin_dwqb_plan(s.M(), csym + s.F, cu_count()).splits * (csym + s.F) * 256);  // ... split-bf16: a partial per row split
  pmax = std::max(pmax, (size_t)dw_plan(s.M(), s.Hp(s.L - 1), s.F).splits * s.Hp(s.L - 1) * s.F);
  pmax = std::max(pmax, (size_t)dw_plan(s.M(), s.F, s.Hp(s.L - 1)).splits * s.Hp(s.L - 1) * s.F);   // (its swapped form)
  const TailGeom g = tail_geom(s);
  if (g.on) {   // fused tail: Q partials, then the dwsum_L partials of cin_tail_params_kernel
    pmax = std::max(pmax, (size_t)tail_dw_plan(s.M(), g.C1).splits * g.C1 * g.JP + (size_t)cdiv(g.Cp, kTailPc) * g.Hq * s.F);
  }
  return pmax;
}

// ---- Buffer layouts.  `saved` and the two workspaces are each declared ONCE, by the lay_out walk of their struct: one line per slice
// (pointer, element count), in the order they lie in the buffer.  A walk runs with a LayoutSizer (the size the caller is told:
// saved_bytes, fwd_ws_bytes, bwd_ws_bytes) or a LayoutCarver (the pointers the launchers use).  take = a slice that starts and ends on
// a 256-byte boundary; sub ... seal = several arrays packed into one such slice.  To add a buffer, add its line to the walk.
struct LayoutSizer {
  size_t off = 0;
  template <typename T> void sub(T*&, size_t n) { off += n * sizeof(T); }
  void seal() { off = align_up(off, 256); }
  template <typename T> void take(T*& p, size_t n) { sub(p, n), seal(); }
};
struct LayoutCarver {
  char* base;
  size_t off = 0;
  explicit LayoutCarver(const void* p) : base(static_cast<char*>(const_cast<void*>(p))) {}
  template <typename T> void sub(T*& p, size_t n) { p = reinterpret_cast<T*>(base + off), off += n * sizeof(T); }
  void seal() { off = align_up(off, 256); }
  template <typename T> void take(T*& p, size_t n) { sub(p, n), seal(); }
};

enum class SavedForm { plain, tail, qtail };   // what lies behind xT and the maps of the layers below the tail
struct CinSaved {
  float* xT;                 // [M][F] (unused when x arrives transposed; the layout stays the same)
  float* maps[kCinMaxL];     // x^{l+1} [M][HS_l] of every layer that runs as a layer of its own and has one above it
  float *Y, *Uz, *Uf, *consts, *bmT;                     // fused tail (Uz | Uf | consts: one slice, one clear; bmT = wsum_L as [f][n])
  float *R, *T, *wsumL, *cvec, *wsumP, *wsnP, *WzT;      // quadratic tail: one packed slice (WzT = T in the dZ kernel's slot order)
  template <class Taker>
  void lay_out(Taker& t, const CinShape& s, const TailGeom& g, SavedForm form) {
    const size_t M = (size_t)s.M();
    t.take(xT, M * s.F);
    const int nmaps = form == SavedForm::qtail ? 1 : (form == SavedForm::tail ? g.p : s.L - 1);
    for (int l = 0; l < nmaps; ++l) t.take(maps[l], M * s.HS(l));
    if (form == SavedForm::qtail) {
      t.sub(R, M * s.HS(0));
      t.sub(T, (size_t)s.F * s.F * s.H[0]);
      t.sub(wsumL, (size_t)s.H[1] * s.F);
      t.sub(cvec, (size_t)128);
      t.sub(wsumP, (size_t)s.H[0] * s.F);
      t.sub(wsnP, (size_t)chunks_of(s.H[0]) * 2 * s.JT() * 128);
      t.sub(WzT, (size_t)cin_slot_tiles(s.F, cin_jt_sym(s.F)) * 32 * s.HS(0));
      t.seal();
    } else if (form == SavedForm::tail) {
      t.take(Y, M * g.JP);
      t.sub(Uz, g.uz_floats);
      t.sub(Uf, g.uf_floats - (size_t)align_up(g.JP + 1, 64));
      t.sub(consts, (size_t)align_up(g.JP + 1, 64));   // beff[JP], sum bias_L
      t.seal();
      t.take(bmT, (size_t)g.Hq * s.F);
    }
  }
};
// (whichever form the call's mode picks must fit: the largest of those the shape allows)
static size_t saved_bytes(const CinShape& s) {
  const TailGeom g = tail_geom(s);
  size_t t = 0;
  for (SavedForm form : {SavedForm::plain, SavedForm::tail, SavedForm::qtail}) {
    if ((form != SavedForm::plain && !g.on) || (form == SavedForm::qtail && s.L != 3)) continue;
    LayoutSizer z;
    CinSaved().lay_out(z, s, g, form);
    t = std::max(t, z.off);
  }
  return t;
}

struct CinFwdWs {
  float *pool[kCinMaxL], *wsum, *Wf, *zbias, *x2T, *WfT;
  u32x4* Wb;
  template <class Taker>
  void lay_out(Taker& t, const CinShape& s) {
    const size_t M = (size_t)s.M();
    const int jts = cin_jt_sym(s.F);
    for (int l = 0; l < s.L; ++l) t.take(pool[l], (size_t)pool_chunks(s, l) * M);        // pool partials [chunks][M] per layer
    t.take(wsum, (size_t)s.Hp(s.L - 1) * s.F);                                           // wsum of the last layer
    t.take(Wf, wf_floats(s));                                                            // packed W
    t.take(zbias, (size_t)kCinMaxH);                                                     // quadratic tail: zero bias of the R GEMM
    t.take(x2T, cin_x2_floats(s.M(), cin_x2_len(s.F)));                                  // wrapped rows of x (pair-symmetric forward)
    t.take(WfT, (size_t)chunks_of(s.H[0]) * s.F * 2 * jts * 128);                        // merged quadratic-tail forward: T's packed operand beside W1's
    t.take(Wb, (size_t)cin_qs_steps(s.F, jts) * kQsStageBytes / sizeof(u32x4));          // ... its split-bf16 planes (three; the one-plane mode uses the first third)
  }
};
static size_t fwd_ws_bytes(const CinShape& s) {
  LayoutSizer z;
  CinFwdWs().lay_out(z, s);
  return z.off;
}

struct CinBwdWs {
  float *dP, *G[2], *part, *small, *wsum, *vlast, *Wz, *dxT, *gx0T, *dT, *dcpart, *hpart;
  u32x4 *Wzb1, *Wzb2;
  template <class Taker>
  void lay_out(Taker& t, const CinShape& s) {
    const size_t M = (size_t)s.M(), LK = (size_t)s.L * s.K, HSmax = (size_t)s.HSmax();
    t.take(dP, (size_t)s.B * LK);
    t.take(G[0], M * HSmax);                                                 // G ping-pong (also the last layer's x*dP rows,
    t.take(G[1], M * HSmax);                                                 // and the tails' scratch: Apk, scratch())
    t.take(part, dw_part_floats(s));                                         // dW partials
    t.take(small, std::max(ncol(s) * HSmax, (size_t)nblk(s) * (LK + 1)));    // colsum / head partials
    const size_t cl = (size_t)std::max(s.Hp(s.L - 1), s.L == 3 ? s.H[0] : 0) * s.F;   // (quadratic tail: the shortcut runs on layer L-2)
    t.take(wsum, cl);                                                        // wsum, v of the last layer
    t.take(vlast, cl);
    t.take(Wz, wz_floats(s));                                                // packed W (slot order)
    t.take(dxT, M * s.F);
    t.take(gx0T, M * s.F);                                                   // Gx^0
    t.take(dT, (size_t)s.F * s.F * kCinMaxH);                                // quadratic tail: dT
    t.take(dcpart, (ndc(s) + 1) * kQtConst);                                 //                 column-sum partials of dP_L x | their sum
    t.take(hpart, ndc(s) * (LK + 1));                                        //                 the dense head's block partials (merged launches)
    const size_t wzb = (size_t)cin_slot_tiles(s.F, cin_jt_sym(s.F)) * 8 * 3072 / sizeof(u32x4);
    t.take(Wzb1, wzb);                                                       // split-bf16 modes: W1s and Ts in slot order as split planes
    t.take(Wzb2, wzb);                                                       // (tiles x 8 steps x 3 KiB each)
  }
  static int nblk(const CinShape& s) { return cdiv(std::max(1, s.B), kHeadChunk); }                  // blocks of the head's partial sums
  static size_t ncol(const CinShape& s) { return ((size_t)s.M() + kColRows - 1) / kColRows; }        // ... of the column sums
  static size_t ndc(const CinShape& s) { return ((size_t)s.M() + 255) / 256; }                       // ... of the quadratic tail's 256-row blocks
  // the quadratic tail's views of G[1], free while no general layer runs: xr | gxR | dxR.  xr is [M][XS]: the merged path's xe
  // (x | 1 | dP_L | dP_p, XS = F + 3; | g, XS = F + 4, where the forward saved the g-free G1: gxR and dxR are not used then), the
  // two-launch path's xs (dP_L x | dP_p, XS = F + 1)
  struct Scratch {
    float *xr, *gxR, *dxR;
    int XS;
  };
  Scratch scratch(const CinShape& s, bool qmerge, bool ghat = false) const {
    const int XS = s.F + (qmerge ? (ghat ? 4 : 3) : 1);
    float* gxR = G[1] + (size_t)s.M() * XS;
    return Scratch{G[1], gxR, gxR + (size_t)s.M() * s.F, XS};
  }
};
static size_t bwd_ws_bytes(const CinShape& s) {
  LayoutSizer z;
  CinBwdWs().lay_out(z, s);
  return z.off;
}

}  // namespace fil
