// A3  xDeepFM CIN: host-side drivers of the C ABI (fil_cin_*).  Device kernels: cin_kernels.h.
//
// Data flow (all internal tensors m-major, m = b*K + k; see cin_kernels.h):
//   fwd:  x [B,F,K] --transpose--> xT [M][F]  (kept in `saved` for the backward)
//         per layer l < L-1 (and the last one in mode 1): pack W_l -> Wf, cin_fwd3 -> x^l [M][HS_l] (saved) + pool partials
//         last layer (mode 0): wsum_L, cin_last_fwd -> pool;   head: pooled [B, L*K], out [B]
//   bwd:  head backward -> dP [B, L*K];  last layer (mode 0): rank-one dW_L, dbias_L, cin_last_bwd -> G^{L-1}, dX
//         per remaining layer: dbias (column sums of G), cin_dw3 (+ fixed-order reduce) -> dW_l,
//         pack W_l -> Wz, cin_dz3 -> G^{l-1}, dX;   finally dxT (+ Gx^0) --transpose--> dx [B,F,K]
// The shape, knobs, launch plans and the layouts of `saved` and the two workspaces (CinSaved, CinFwdWs, CinBwdWs: each declared once, by
// its lay_out walk) are in cin_layout.h.  Here: the path of a call (CinPath: which kernels a mode, precision and shape select), then the
// forward and the backward, each as check, plan, lay out, dispatch over one static function per path (cin_fwd_*, cin_bwd_*).
#include "cin_layout.h"

namespace fil {

static const char* kFwdNames[kCinMaxL] = {"cin_fwd_l1", "cin_fwd_l2", "cin_fwd_l3", "cin_fwd_l4", "cin_fwd_l5", "cin_fwd_l6", "cin_fwd_l7", "cin_fwd_l8"};
static const char* kDwNames[kCinMaxL] = {"cin_bwd_dw_l1", "cin_bwd_dw_l2", "cin_bwd_dw_l3", "cin_bwd_dw_l4", "cin_bwd_dw_l5", "cin_bwd_dw_l6", "cin_bwd_dw_l7", "cin_bwd_dw_l8"};
static const char* kDzNames[kCinMaxL] = {"cin_bwd_dz_l1", "cin_bwd_dz_l2", "cin_bwd_dz_l3", "cin_bwd_dz_l4", "cin_bwd_dz_l5", "cin_bwd_dz_l6", "cin_bwd_dz_l7", "cin_bwd_dz_l8"};
// algorithmic flops of one layer GEMM: 2 * M * C * H
static double gemm_flops(long M, int Hp, int F, int H) { return 2.0 * (double)M * Hp * F * H; }

static int launch_dw3(hipStream_t st, const DwPlan& p, const float* gT, int HS, const float* xT, const float* xpT, int xps, float* part,
                      long M, int F, int Hp, int H, int symD = 0, int xtra = 0) {
  const int items = p.blocks_x * p.splits * p.chunks;
  const dim3 grid((items + 7) / 8 * 8);
#define FIL_DW3(MBV, ONES) \
  hipLaunchKernelGGL((cin_dw3_kernel<MBV, ONES>), grid, dim3(kCinThreads), 0, st, gT, HS, xT, xpT, xps, part, (int)M, F, Hp, H, p.rows_per_split, \
                     p.blocks_x, p.chunks, items, symD, xtra)
  if (xT == nullptr) {
    if (p.MB == 2) FIL_DW3(2, true); else FIL_DW3(1, true);
  } else {
    if (p.MB == 2) FIL_DW3(2, false); else FIL_DW3(1, false);
  }
#undef FIL_DW3
  return p.splits;
}

constexpr int kCinRetiredBits = 0;   // mode bits that no longer select anything: FIL_ERR_UNSUPPORTED (none at present)
// is the tail used by a call with these mode bits?
static bool tail_used(const CinShape& s, int mode) {
  if ((mode & (FIL_CIN_GENERAL | FIL_CIN_NOTAIL)) != 0) return false;
  const TailGeom g = tail_geom(s);
  if (!g.on) return false;
  return (mode & FIL_CIN_TAIL_ALWAYS) != 0 || 4 * g.JP <= 3 * g.Hq;
}
// Quadratic tail (cin_qtail.h): three layers, pair-symmetric first-layer kernels available, one 128-column chunk below the tail.
// The top two layers then cost F(F+1)/2 x H_1 products per row -- half of the fused tail's H_1 F (F+1), and no column padding.
// It takes ~10 more small launches than the fused tail: below ~16 K rows (a strong-scaling shard: the step is launch-latency bound
// there, B=512: 0.40 ms against 0.33) the fused tail stays the default; FIL_CIN_TAIL_ALWAYS lifts the size rule (tests).
static bool qtail_used(const CinShape& s, int mode, const CinTune& tune) {
  if (s.M() <= 16384 && (mode & FIL_CIN_TAIL_ALWAYS) == 0) return false;
  return tail_used(s, mode) && s.L == 3 && tune.sym && s.F >= 2 && s.F + 2 <= kQtConst && s.H[0] <= 128 && 3 * s.F + 1 <= s.HSmax() && (mode & FIL_CIN_NOQTAIL) == 0 &&
         knobs().qtail != 0;   // (3 F: its three [M][F] scratch arrays share one gradient buffer)
}
// ... with ONE weight-gradient and ONE data-gradient GEMM for the first layer and the quadratic form together (cin_qmerge.h)
static bool qmerge_used(const CinShape& s, int mode, const CinTune& tune) {
  return qtail_used(s, mode, tune) && 3 * s.F + 3 <= s.HSmax() && (mode & FIL_CIN_NOQMERGE) == 0 && knobs().qmerge != 0;   // (xe | gxR | dxR share one gradient buffer)
}
// ... on split-bf16 operands (cin_qsplit.h, FIL_CIN_BF16X3): where the merged kernels run in their full form and a split kernel exists
// ... or on one bf16 plane per operand (FIL_CIN_PREC_BF16 of the _p entry points): the same places, the same kernels with NP = 1.  The
// precision travels inside the library as a mode bit that the public entry points never accept (their modes stop at 1023).
constexpr int kCinPrecBf16 = 1 << 20;
static bool qsplit_fwd_menu(int JT) { return JT >= 2 && JT <= 12 && JT % 2 == 0; }   // (F <= 41 on the merged tail: JT <= 12)
static bool qsplit_used(const CinShape& s, int mode, const CinTune& tune) {
  return (mode & (FIL_CIN_BF16X3 | kCinPrecBf16)) != 0 && qmerge_used(s, mode, tune) && knobs().fwdq != 0 && knobs().dz2 != 0 && s.HS(0) == 128 &&
         qsplit_fwd_menu(cin_jt_sym(s.F));
}

// ---- the path of one call: every decision the mode bits, the precision and the shape make, taken once (cin_path_of) and read by the
// forward, the backward, fil_cin_grad_ready_points and fil_cin_precision_used
struct CinPath {
  bool xt_in;      // x is already [B*K][F] (fil_embed_gather_xt): no input transpose
  bool general;    // mode bit 1: the general GEMM kernels for every layer, no last-layer shortcut
  bool tail;       // last two layers as one implicit GEMM (cin_tail.h)
  bool qtail;      // ... as a quadratic form over field pairs (cin_qtail.h)
  bool qmerge;     // ... with merged launches (cin_qmerge.h)
  bool qsplit;     // ... on split-bf16 operands (cin_qsplit.h)
  int qnp;         //     of three planes each (BF16X3) or one (PREC_BF16)
  CinTune tune;
  TailGeom tg;
  // merged quadratic tail, forward: the 256-column launch with the pools in its epilogue
  bool fwdq(const CinShape& s) const { return qmerge && knobs().fwdq != 0 && s.HS(0) == 128; }
};
static CinPath cin_path_of(const CinShape& s, int mode) {   // mode: the public bits | kCinPrecBf16
  const CinTune tune(mode);
  return CinPath{(mode & FIL_CIN_X_TRANSPOSED) != 0, (mode & FIL_CIN_GENERAL) != 0, tail_used(s, mode), qtail_used(s, mode, tune), qmerge_used(s, mode, tune),
                 qsplit_used(s, mode, tune), (mode & kCinPrecBf16) != 0 ? 1 : 3, tune, tail_geom(s)};
}
// Which form saved.R holds after a forward on the merged quadratic tail (exact mode).  True: the g-free gradient of x1,
//   Ghat[m,:] = dw_L[k] R[m,:] + dw_p[k] S[m,:] + dw_1[k]     (dw_j[k] = dense_w[j K + k], k = m mod K, S = x wsum_p^T),
// which the forward's epilogue holds in registers anyway; the backward's two GEMMs apply g[b] (G1 = g[b] Ghat) where they already apply a
// per-row scale, and cin_last_bwd2_kernel's pass over R, x and G1 is gone.  False: R itself, G1 built by cin_last_bwd2_kernel.
// It needs the Dense(1) head folded into the forward's epilogue (dense_w at hand there, dP_j = g dw_j) and the two-pass data-gradient
// launch (its first pass scales its rows on load).  The forward and the backward both ask this function and nothing else.
static bool cin_ghat_used(const CinShape& s, const CinPath& p, int output_dim) {
  const bool headfold = output_dim == 1 && s.K <= 32 && (s.K & (s.K - 1)) == 0 && knobs().headfold != 0;
  const bool dz2 = knobs().dz2 != 0 && s.HS(0) / 2 == 64;
  return p.qmerge && p.fwdq(s) && !p.qsplit && headfold && dz2 && knobs().ghat != 0;
}
// Merged quadratic tail, backward: where the forward saved the g-free G1 (cin_ghat_used) the only work left for the cin_last_bwd launch is
// the shortcut's data gradient, and cin_shortcut_dx_kernel (cin_shortdx.h) does it.  False: cin_last_bwd2_kernel, as everywhere else.
// (ghat implies Hp = H[0] <= 128 and F <= 64, the kernel's limits; the split-bf16 and one-plane bf16 modes never have ghat where their
// own kernels run -- they keep cin_last_bwd2_kernel -- and take this kernel where they fall back to the exact ones.)
static bool cin_shortdx_used(const CinShape& s, const CinPath& p, int output_dim) { return cin_ghat_used(s, p, output_dim) && knobs().shortdx != 0; }
// precision code of the _p entry points -> the internal mode bit (FIL_OK), or FIL_ERR_ARG
static int cin_precision_bits(const char* who, int mode, int precision, int* bits) {
  if (precision != FIL_CIN_PREC_DEFAULT && precision != FIL_CIN_PREC_BF16)
    return fail(FIL_ERR_ARG, "%s: precision %d (0 DEFAULT, 1 BF16)", who, precision);
  if (precision == FIL_CIN_PREC_BF16 && (mode & FIL_CIN_BF16X3) != 0)
    return fail(FIL_ERR_ARG, "%s: precision BF16 with mode bit BF16X3 (mode %d): two operand precisions", who, mode);
  *bits = precision == FIL_CIN_PREC_BF16 ? kCinPrecBf16 : 0;
  return FIL_OK;
}
// the mode / precision checks of the fwd / bwd entry points, then the path
static int cin_path(const char* who, const CinShape& s, int mode, int precision, CinPath* path) {
  if (mode < 0 || mode > 1023 || (mode & kCinRetiredBits) != 0)
    return fail(FIL_ERR_UNSUPPORTED, "%s: mode %d (bits: 1 general kernels, 2 BF16X3, 4 MB2, 8 NOSYM, 16 X_TRANSPOSED, 32 NOTAIL, 64 TAIL_ALWAYS, 128 NOKSPLIT, 256 NOQTAIL, 512 NOQMERGE)", who, mode);
  int bits = 0;
  if (int rc = cin_precision_bits(who, mode, precision, &bits)) return rc;
  *path = cin_path_of(s, mode | bits);
  return FIL_OK;
}
// The order in which the backward records its grad_ready slots ([l]: layer l, [L]: the dense head), and the ordinal of each: slots
// with one ordinal become final in one group of launches.  cin_bwd_impl records slot[0], slot[1], ... (ready_next);
// fil_cin_grad_ready_points reports point[].  Returns the number of ordinals.
static int cin_ready_order(int L, const CinPath& p, int* slot, int* point) {
  int n = 0, pt = 0;
  slot[n] = L, point[n++] = pt;
  if (p.qmerge) slot[n] = 0, point[n++] = pt;   // merged weight gradients: the first layer's come out first, the dense head's with them
  ++pt;
  int l = L - 1;
  if (p.tail) {                                 // the two top layers' gradients come out of one group of launches
    slot[n] = L - 1, point[n++] = pt;
    slot[n] = L - 2, point[n++] = pt++;
    l = L - 3;
  }
  for (; l >= (p.qmerge ? 1 : 0); --l) slot[n] = l, point[n++] = pt++;
  return pt;
}
static SavedForm saved_form(const CinPath& p) { return p.qtail ? SavedForm::qtail : (p.tail ? SavedForm::tail : SavedForm::plain); }

template <typename KernelT>
static void allow_lds(KernelT kernel, size_t sh) {
  if (sh > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
}

// the pair-symmetric dZ kernel's launch shape.  Exact kernel, H <= 128: 32 rows per wave at TWO waves per SIMD where the instantiation
// fits 256 registers (the second wave covers the first one's prologue, epilogue and contraction issue: c4 0.154 -> 0.136 ms);
// FIL_CIN_MB2 / FIL_CIN_MB=2 / FIL_CIN_DZS_MB=2 keep 64 rows per wave (measured best otherwise)
struct DzsShape {
  int MBs, ks;
  dim3 grid;
};
static DzsShape dzs_launch_shape(const CinTune& tune, long M, int JTs, int NHMAX) {
  const bool two_waves = NHMAX == 64 && cin_dzs_two_waves(JTs) && tune.mb_forced != 2 && knobs().dzs_mb != 2;
  const int MBs = (two_waves || NHMAX == 128) ? 1 : tune.mb_rows(M);
  const int ks = (NHMAX != 64 || MBs != 1) ? 1 : tune.ksplit(M);
  return DzsShape{MBs, ks, dim3(ks == 4 ? cdiv((int)M, 32) : cdiv((int)M, 128 * MBs))};
}

}  // namespace fil

using namespace fil;

extern "C" size_t fil_cin_saved_bytes(int B, int F, int K, int L, const int* H) {
  CinShape s;
  if (check_shape("fil_cin_saved_bytes", B, F, K, L, H, s) != FIL_OK || B == 0) return 0;
  return saved_bytes(s);
}

extern "C" size_t fil_cin_fwd_workspace_bytes(int B, int F, int K, int L, const int* H) {
  CinShape s;
  if (check_shape("fil_cin_fwd_workspace_bytes", B, F, K, L, H, s) != FIL_OK || B == 0) return 0;
  return fwd_ws_bytes(s);
}

extern "C" size_t fil_cin_bwd_workspace_bytes(int B, int F, int K, int L, const int* H) {
  CinShape s;
  if (check_shape("fil_cin_bwd_workspace_bytes", B, F, K, L, H, s) != FIL_OK || B == 0) return 0;
  return bwd_ws_bytes(s);
}

extern "C" int fil_cin_grad_ready_points(int B, int F, int K, int L, const int* H, int mode, int* point) {
  CinShape s;
  if (int rc = check_shape("fil_cin_grad_ready_points", B, F, K, L, H, s)) return rc;
  if (point == nullptr || mode < 0 || mode > 1023) return fail(FIL_ERR_ARG, "fil_cin_grad_ready_points: point == NULL or mode %d out of range", mode);
  if ((mode & kCinRetiredBits) != 0) return fail(FIL_ERR_UNSUPPORTED, "fil_cin_grad_ready_points: mode %d holds a retired bit (2: the split-bf16 experiment)", mode);
  if (B == 0) {                                         // empty batch: zero gradients, every slot at once
    for (int i = 0; i <= L; ++i) point[i] = 0;
    return 1;
  }
  int slot[kCinMaxL + 1], pt[kCinMaxL + 1];
  const int n = cin_ready_order(L, cin_path_of(s, mode), slot, pt);
  for (int i = 0; i <= L; ++i) point[slot[i]] = pt[i];
  return n;
}

extern "C" int fil_cin_shortdx_used(int B, int F, int K, int L, const int* H, int output_dim, int mode, int precision) {
  CinShape s;
  if (int rc = check_shape("fil_cin_shortdx_used", B, F, K, L, H, s)) return rc;
  CinPath p;
  if (int rc = cin_path("fil_cin_shortdx_used", s, mode, precision, &p)) return rc;
  return B > 0 && cin_shortdx_used(s, p, output_dim) ? 1 : 0;
}

extern "C" int fil_cin_precision_used(int B, int F, int K, int L, const int* H, int mode, int precision) {
  CinShape s;
  if (int rc = check_shape("fil_cin_precision_used", B, F, K, L, H, s)) return rc;
  if (mode < 0 || mode > 1023 || (mode & kCinRetiredBits) != 0) return fail(FIL_ERR_UNSUPPORTED, "fil_cin_precision_used: mode %d", mode);
  int bits = 0;
  if (int rc = cin_precision_bits("fil_cin_precision_used", mode, precision, &bits)) return rc;
  if (bits == 0 || B == 0) return FIL_CIN_PREC_DEFAULT;
  return cin_path_of(s, mode | bits).qsplit ? FIL_CIN_PREC_BF16 : FIL_CIN_PREC_DEFAULT;
}

// FIL_CHECK_ARG / FIL_CHECK_LAUNCH inside the pieces of the fwd / bwd bodies: the message names the entry point called (c.who) /
// the body the piece belongs to
#define FIL_CIN_CHECK_ARG(cond)                                                          \
  do {                                                                                   \
    if (!(cond)) return ::fil::fail(FIL_ERR_ARG, "%s: bad argument: %s", c.who, #cond); \
  } while (0)
#define FIL_CIN_FWD_LAUNCHED() FIL_CHECK_LAUNCH_W("cin_fwd_impl")
#define FIL_CIN_BWD_LAUNCHED() FIL_CHECK_LAUNCH_W("cin_bwd_impl")

// one call: the shape, its path, the stream, the caller's tensors, `saved` carved
struct CinCall {
  const char* who;
  CinShape s;
  CinPath p;
  hipStream_t st;
  const float* x;
  const float* xT;             // [M][F]: x itself (X_TRANSPOSED) or saved's copy
  const float* const* W;
  const float* const* bias;
  const float* dense_w;
  int output_dim;
  CinSaved sv;
};
struct CinFwd : CinCall {
  const float* dense_b;
  float *out, *pooled;
  CinFwdWs ws;
  PoolArgs pa;
  const float* xpT;            // x^{l-1} of the layer that runs next
  bool fused_last = false;     // the last layer's sum-pool was produced by the epilogue of the layer below
  bool head_done = false;      // merged forward: pooled and out came out of cin_fwdq_kernel's epilogue
};

// Every preparation job that depends on the inputs alone.  Exact pair-symmetric first layer + a tail (the north-star path): x transpose,
// first-layer weight pack, pooled weights of the last layer, clearing the fused tail's operand buffers -- in ONE launch instead of four
static int cin_fwd_prepare(CinFwd& c) {
  const CinShape& s = c.s;
  const TailGeom& tg = c.p.tg;
  const int B = s.B, F = s.F, K = s.K, L = s.L, JT = s.JT(), XL = cin_x2_len(F);
  const long M = s.M();
  const bool xt_in = c.p.xt_in, need_x2 = c.p.tune.sym;   // (the pair-symmetric forward kernel reads the wrapped rows)
  hipStream_t st = c.st;
  if (c.p.qtail) {
    FIL_CIN_CHECK_ARG(c.W[0] && c.W[L - 1] && c.W[L - 2]);
    ProfScope ps("cin_fwd_prep", st, 2.0 * M * F * sizeof(float));
    const int JTs = cin_jt_sym(F), chunks0 = chunks_of(s.H[0]);
    const long npack = (long)chunks0 * F * 2 * JTs * 128;
    // (merged forward: the x transposes ride in the NEXT launch, behind the T workgroups, whose latency chain is the longer one -- this
    // launch is the weight work alone.  Measured the other way round, transposes here and T alone there: 9.8 + 11.4 us against
    // 4.2 + 12.5)
    const bool fq = c.p.fwdq(s);
    const int nt = fq ? 0 : B, npk = (int)std::min<long>((npack + 255) / 256, 1024), nwl = cdiv(tg.Hq * F, 8), nwp = cdiv(tg.Hpp * F, 8);
    const size_t sh = (xt_in || fq) ? 0 : (size_t)F * (K + 1) * sizeof(float);
    allow_lds(cin_qtail_prep_kernel, sh);
    hipLaunchKernelGGL(cin_qtail_prep_kernel, dim3(nt + npk + nwl + nwp), dim3(256), sh, st, c.x, c.sv.xT, F, K, nt, c.W[0], c.ws.Wf, s.H[0], 2 * JTs, chunks0, npk,
                       c.W[L - 1], c.sv.wsumL, tg.Hq, tg.HL, nwl, c.W[L - 2], c.sv.wsumP, c.sv.wsnP, tg.Hpp, 2 * JT, chunks_of(tg.Hpp), c.ws.x2T, XL, xt_in ? 1 : 0);
  } else if (c.p.tail && c.p.tune.sym) {
    FIL_CIN_CHECK_ARG(c.W[0] && c.W[L - 1]);
    ProfScope ps("cin_fwd_prep", st, 2.0 * M * F * sizeof(float));
    const int JTs = cin_jt_sym(F), chunks0 = chunks_of(s.H[0]);
    const long npack = (long)chunks0 * F * 2 * JTs * 128;
    const int nt = B, npk = (int)std::min<long>((npack + 255) / 256, 1024), nws = cdiv(tg.Hq * F, 8), nz = 64;
    const size_t sh = xt_in ? 0 : (size_t)F * (K + 1) * sizeof(float);
    allow_lds(cin_fwd_prep_kernel, sh);
    hipLaunchKernelGGL(cin_fwd_prep_kernel, dim3(nt + npk + nws + nz), dim3(256), sh, st, c.x, c.sv.xT, F, K, nt, c.W[0], c.ws.Wf, s.H[0], 2 * JTs, chunks0,
                       npk, c.W[L - 1], c.sv.bmT, tg.Hq, tg.HL, nws, reinterpret_cast<float4*>(c.sv.Uz), (long)((tg.uz_floats + tg.uf_floats) / 4), c.ws.x2T, XL,
                       xt_in ? 1 : 0);
  } else if (!xt_in || need_x2) {
    ProfScope ps("cin_transpose_in", st, 2.0 * M * F * sizeof(float));
    hipLaunchKernelGGL(cin_transpose_in_kernel, dim3(B), dim3(256), xt_in ? 0 : (size_t)F * (K + 1) * sizeof(float), st, c.x, c.sv.xT, F, K,
                       need_x2 ? c.ws.x2T : nullptr, XL, xt_in ? 1 : 0);
  }
  FIL_CIN_FWD_LAUNCHED();
  return FIL_OK;
}

// ---- merged quadratic tail, forward (cin_qmerge.h): [x1 | R] = pairs(x) [W1s | Ts] in ONE launch of 256 columns, all three
// sum-pools in its epilogue.  T (and its packed operand copies) depend on the weights alone: they come first.
static int cin_fwd_merged_q(CinFwd& c) {
  const CinShape& s = c.s;
  const TailGeom& tg = c.p.tg;
  const CinSaved& sv = c.sv;
  const CinFwdWs& ws = c.ws;
  const int B = s.B, F = s.F, K = s.K, L = s.L, JT = s.JT(), XL = cin_x2_len(F), *H = s.H;
  const long M = s.M();
  const bool xt_in = c.p.xt_in, qsplit = c.p.qsplit;
  const float* x = c.x;
  hipStream_t st = c.st;
  const int p = tg.p, lL = L - 1, Hpp = tg.Hpp, Hq = tg.Hq, HS0 = s.HS(0);
  FIL_CIN_CHECK_ARG(c.W[p] && c.W[lL] && c.bias[p] && c.bias[lL]);
  const int JTs = cin_jt_sym(F), chunks = chunks_of(Hpp);
  float* x1T = sv.maps[0];
  {
    ProfScope ps("cin_tail_prep", st);
    // T / cvec (weights only) and, beside them, the x -> xT / wrapped-row transposes (x only)
    // (x as given and K a power of two <= 64: the transposes go by 64-row blocks of whole samples, cin_transpose_block_body)
    int ks = -1;
    if (!xt_in && K <= 64 && (K & (K - 1)) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0)
      for (ks = 0; (1 << ks) < K;) ++ks;
    const size_t sh_x = ks >= 0 ? (size_t)(64 >> ks) * F * (K + 1) : (xt_in ? (size_t)64 * (F | 1) : (size_t)F * (K + 1));
    const int tiles = cin_slot_tiles(F, JTs);
    // exact mode: every T workgroup writes its column of both operand layouts itself (one workgroup per column) -- no pack launch;
    // split-bf16 mode: the planes of [W1s | Ts] need whole rows of T, the pack launch stays
    const bool fold = !qsplit && knobs().packfold != 0;
    const QtPackFold pf = fold ? QtPackFold{ws.WfT, sv.WzT, JTs, chunks, HS0, tiles} : QtPackFold{nullptr, nullptr, 0, 0, 0, 0};
    const size_t sh = std::max(cin_qtail_t_lds_floats(F, Hq, fold), sh_x) * sizeof(float);
    allow_lds(cin_qtail_t_x_kernel, sh);
    const int nx = (ks >= 0 || xt_in) ? (int)((M + 63) / 64) : B, nT = cin_qtail_t_wgs(Hpp);
    hipLaunchKernelGGL(cin_qtail_t_x_kernel, dim3(nT + nx), dim3(256), sh, st, c.W[p], sv.wsumL, c.bias[p], c.bias[lL], tg.HL, sv.T, sv.cvec, ws.zbias, Hpp, F, Hq,
                       nT, x, sv.xT, K, ws.x2T, XL, xt_in ? 1 : 0, ks, (ks >= 0 || xt_in) ? (long)M : 0L, pf);
    if (!fold) {
      const long npack = (long)chunks * F * 2 * JTs * 128;
      const int nbf = (int)std::min<long>((npack + 255) / 256, 1024), nbz = (int)std::min<long>(((long)tiles * 32 * HS0 + 255) / 256, 1024);
      // (split-bf16 mode: + the forward's planes of [W1s | Ts], from W1 and T themselves)
      const int NTq = qsplit ? cin_qs_steps(F, JTs) : 0, nbq = qsplit ? std::min(cdiv(NTq * 512, 256), 512) : 0;
      if (c.p.qnp == 1)
        hipLaunchKernelGGL(cin_qtail_pack_kernel<1>, dim3(nbf + nbz + nbq), dim3(256), 0, st, sv.T, ws.WfT, sv.WzT, F, Hpp, JTs, chunks, nbf, HS0, tiles, nbz,
                           c.W[0], H[0], ws.Wb, NTq);
      else
        hipLaunchKernelGGL(cin_qtail_pack_kernel<3>, dim3(nbf + nbz + nbq), dim3(256), 0, st, sv.T, ws.WfT, sv.WzT, F, Hpp, JTs, chunks, nbf, HS0, tiles, nbz,
                           c.W[0], H[0], ws.Wb, NTq);
    }
  }
  FIL_CIN_FWD_LAUNCHED();
  {
    const double algo = gemm_flops(M, F, F, H[0]) + gemm_flops(M, Hpp, F, Hq) + gemm_flops(M, Hq, F, tg.HL);   // all three layers of the reference graph
    ProfScope ps("cin_fwd_q", st, algo, gemm_flops(M, 1, F * (F / 2 + 1), H[0]) + gemm_flops(M, 1, F * (F / 2 + 1), Hpp));
    // (K a power of two <= 32: a wave's rows are whole samples, and the pooled relayout + Dense(1) head ride in the epilogue)
    CinHeadFold hf{};
    if (K <= 32 && (K & (K - 1)) == 0 && knobs().headfold != 0) {
      int ks = 0;
      while ((1 << ks) < K) ++ks;
      hf = CinHeadFold{c.pooled, c.output_dim == 1 ? c.out : nullptr, c.dense_w, c.dense_b, ks, (int)(L * K), p * K, lL * K};
      c.head_done = true;
    }
    if (qsplit) {
      // split-bf16 operands (their planes came out of the pack launch above): the same GEMM on the bf16 pipe
      const int NT = cin_qs_steps(F, JTs);
      if (!cin_launch_fwdq_b(st, c.p.qnp, JTs, ws.x2T, XL, ws.Wb, NT, c.bias[0], sv.wsnP, JT, sv.cvec, x1T, sv.R, HS0, ws.pool[0], ws.pool[p], ws.pool[lL], (int)M, F,
                             H[0], hf))
        return fail(FIL_ERR_UNSUPPORTED, "fil_cin_fwd: no split-bf16 forward kernel for JT=%d (F=%d)", JTs, F);
    } else if (!cin_launch_fwdq(st, JTs, ws.x2T, XL, ws.Wf, ws.WfT, c.bias[0], sv.wsnP, JT, sv.cvec, x1T, sv.R, HS0, ws.pool[0], ws.pool[p], ws.pool[lL], (int)M, F,
                                H[0], hf, cin_ghat_used(s, c.p, c.output_dim)))   // (true: the g-free G1 in R's place)
      return fail(FIL_ERR_UNSUPPORTED, "fil_cin_fwd: no merged forward kernel for JT=%d (F=%d)", JTs, F);
    c.pa.chunks[0] = c.pa.chunks[p] = c.pa.chunks[lL] = 1;
  }
  FIL_CIN_FWD_LAUNCHED();
  return FIL_OK;
}

// ---- quadratic tail (cin_qtail.h), layers l = L-2 and L-1: R = (pairs of x) T through the first layer's pair-symmetric forward kernel,
// pool_L = <x1, R> + <x, c> + const, pool_p through the pooled-weights shortcut
static int cin_fwd_qtail(CinFwd& c, int l) {
  const CinShape& s = c.s;
  const TailGeom& tg = c.p.tg;
  const CinSaved& sv = c.sv;
  const CinFwdWs& ws = c.ws;
  const int F = s.F, L = s.L, JT = s.JT(), XL = cin_x2_len(F), MB = c.p.tune.mb_rows(s.M());
  const long M = s.M();
  const float *xT = c.xT, *xpT = c.xpT;
  hipStream_t st = c.st;
  const int lL = L - 1, Hpp = tg.Hpp, Hq = tg.Hq, HS0 = s.HS(0);
  FIL_CIN_CHECK_ARG(c.W[lL] && c.bias[lL]);
  const int JTs = cin_jt_sym(F), chunks = chunks_of(Hpp);
  {
    ProfScope ps("cin_tail_prep", st);
    // (wsum_L, wsum_p and its MFMA operand copy came out of the preparation launch)
    const size_t sh = cin_qtail_t_lds_floats(F, Hq, false) * sizeof(float);
    allow_lds(cin_qtail_t_kernel, sh);
    hipLaunchKernelGGL(cin_qtail_t_kernel, dim3(cin_qtail_t_wgs(Hpp)), dim3(256), sh, st, c.W[l], sv.wsumL, c.bias[l], c.bias[lL], tg.HL, sv.T, sv.cvec, ws.zbias, Hpp, F, Hq);
    // T in the forward kernel's operand layout (workspace) and in the dZ kernel's slot order (saved for the backward): one launch
    const long npack = (long)chunks * F * 2 * JTs * 128;
    const int tiles = cin_slot_tiles(F, JTs);
    const int nbf = (int)std::min<long>((npack + 255) / 256, 1024), nbz = (int)std::min<long>(((long)tiles * 32 * HS0 + 255) / 256, 1024);
    hipLaunchKernelGGL(cin_qtail_pack_kernel<3>, dim3(nbf + nbz), dim3(256), 0, st, sv.T, ws.Wf, sv.WzT, F, Hpp, JTs, chunks, nbf, HS0, tiles);
  }
  FIL_CIN_FWD_LAUNCHED();
  {
    const double algo = gemm_flops(M, Hpp, F, Hq) + gemm_flops(M, Hq, F, tg.HL);   // the two layers of the reference graph
    ProfScope ps("cin_fwd_tail", st, algo, gemm_flops(M, 1, F * (F / 2 + 1), Hpp));
    const int ks = c.p.tune.ksplit(M);
    // (the kernel's own sum-pool output is not used: it goes to the last layer's slot, which the pool kernel below overwrites)
    cin_launch_fwd3_sym(st, MB, JTs, dim3(ks == 4 ? cdiv((int)M, 32) : cdiv((int)M, 128 * MB), chunks), xT, ws.x2T, XL, ws.Wf, ws.zbias, sv.R, HS0, ws.pool[lL],
                        (int)M, F, Hpp, ks);
  }
  FIL_CIN_FWD_LAUNCHED();
  {
    ProfScope ps("cin_tail_pool", st);
    const float* wsn = sv.wsnP;
    float *pp = ws.pool[l], *pL = ws.pool[lL];
    const dim3 grid((int)((M + 127) / 128));
#define FIL_QP(JTV) \
  case JTV: hipLaunchKernelGGL((cin_qtail_pool2_kernel<JTV>), grid, dim3(256), 0, st, xT, xpT, s.xps(l), wsn, sv.R, HS0, sv.cvec, pp, pL, (int)M, F, Hpp); break;
    switch (JT) { FIL_QP(4) FIL_QP(8) FIL_QP(12) FIL_QP(16) FIL_QP(20) FIL_QP(24) FIL_QP(28) FIL_QP(32) }
#undef FIL_QP
    c.pa.chunks[l] = c.pa.chunks[lL] = 1;
  }
  FIL_CIN_FWD_LAUNCHED();
  return FIL_OK;
}

// ---- fused tail: layers l = L-2 and L-1 through Ueff = W_p [1 | wsum_L]: F+1 output columns instead of H_p
static int cin_fwd_fused_tail(CinFwd& c, int l) {
  const CinShape& s = c.s;
  const TailGeom& tg = c.p.tg;
  const CinSaved& sv = c.sv;
  const int F = s.F, lL = s.L - 1, JT = s.JT();
  const long M = s.M();
  hipStream_t st = c.st;
  FIL_CIN_CHECK_ARG(c.W[lL] && c.bias[lL]);
  {
    ProfScope ps("cin_tail_prep", st);
    if (!c.p.tune.sym) {   // (else the preparation launch did both)
      hipLaunchKernelGGL(cin_tail_wsum_kernel, dim3(cdiv(tg.Hq * F, 8)), dim3(256), 0, st, c.W[lL], sv.bmT, tg.Hq, F, tg.HL);
      // (padding of the operand layouts -- f >= F, j > F, spare slots -- must be zero)
      (void)hipMemsetAsync(sv.Uz, 0, (tg.uz_floats + tg.uf_floats) * sizeof(float), st);
    }
    const size_t sh = (size_t)(F + 1) * (((tg.Hq + 3) & ~3) + 4) * sizeof(float);
    allow_lds(cin_tail_ueff_kernel, sh);
    hipLaunchKernelGGL(cin_tail_ueff_kernel, dim3(cdiv(tg.C1, kTailUc)), dim3(256), sh, st, c.W[l], c.bias[l], sv.bmT, c.bias[lL], tg.HL, sv.Uf, sv.Uz, sv.consts,
                       tg.Hpp, F, tg.Hq, tg.JT4, tg.JP, JT, tg.JHp);
  }
  FIL_CIN_FWD_LAUNCHED();
  {
    const double algo = gemm_flops(M, tg.Hpp, F, tg.Hq) + gemm_flops(M, tg.Hq, F, tg.HL);   // the two layers of the reference graph
    ProfScope ps("cin_fwd_tail", st, algo, 2.0 * (double)M * tg.Cp * (F + 1));
    const int RB = c.p.tune.mb_rows(M) == 2 ? 4 : 2;
    TailFwdArgs a{c.xT, c.xpT, s.xps(l), sv.Uf, sv.consts, sv.Y, tg.JP, c.ws.pool[l], c.ws.pool[lL], (int)M, F, tg.Hpp, c.p.tune.ksplit(M)};
    cin_launch_tail_fwd(st, RB, tg.JT4, tg.NCB, a);
    c.pa.chunks[l] = c.pa.chunks[lL] = 1;
  }
  FIL_CIN_FWD_LAUNCHED();
  return FIL_OK;
}

// ---- layer l as a layer of its own: pack W_l, GEMM -> x^{l+1} (saved) + pool partials; the last layer in mode 0 through wsum alone
static int cin_fwd_general_layer(CinFwd& c, int l) {
  const CinShape& s = c.s;
  const CinTune& tune = c.p.tune;
  const CinFwdWs& ws = c.ws;
  const int F = s.F, L = s.L, JT = s.JT(), XL = cin_x2_len(F), MB = tune.mb_rows(s.M()), *H = s.H;
  const long M = s.M();
  const float *xT = c.xT, *xpT = c.xpT;
  hipStream_t st = c.st;
  const int Hp = s.Hp(l), Hl = H[l], xps = s.xps(l);
  float* xoutT = l + 1 < L ? c.sv.maps[l] : nullptr;
  float* part = ws.pool[l];
  // mode 0, last layer: only its sum-pool is observable -> contract with wsum[c] = sum_n W[c,n].  When the layer
  // below it runs the general (non pair-symmetric) forward kernel, that kernel's epilogue does it (fused_last).
  const bool fuse_next = !c.p.general && l == L - 2 && !(l == 0 && tune.sym);
  if (l == L - 1 && !c.p.general) {
    if (!c.fused_last) {
      const size_t sh = (size_t)Hp * ((F + 3) & ~3) * sizeof(float);
      ProfScope ps("cin_last_fwd", st, 2.0 * (double)M * Hp * F);
      hipLaunchKernelGGL(cin_wsum_kernel, dim3(cdiv(Hp * F, 8)), dim3(256), 0, st, c.W[l], ws.wsum, Hp * F, Hl);
      allow_lds(cin_last_fwd_kernel, sh);
      hipLaunchKernelGGL(cin_last_fwd_kernel, dim3(cdiv((int)M, kLastRows)), dim3(256), sh, st, xT, xpT, xps, ws.wsum, c.bias[l], part, (int)M, F, Hp, Hl);
      c.pa.chunks[l] = 1;
    }
  } else {
    const int chunks = chunks_of(Hl);
    if (l == 0 && tune.sym) {
      // first layer: x^{l-1} = x, reduce over unordered field pairs (half the steps)
      const int JTs = cin_jt_sym(F);
      const long npack = (long)chunks * F * 2 * JTs * 128;
      if (!c.p.tail)   // (else the preparation launch packed them)
        hipLaunchKernelGGL(cin_pack_wf_sym_kernel, dim3((int)std::min<long>((npack + 255) / 256, 2048)), dim3(256), 0, st, c.W[l], ws.Wf, F, Hl, 2 * JTs, chunks);
      ProfScope ps(kFwdNames[l], st, gemm_flops(M, Hp, F, Hl), gemm_flops(M, 1, F * (F / 2 + 1), Hl));   // (executed: unordered pairs)
      const int ks = tune.ksplit(M);
      cin_launch_fwd3_sym(st, MB, JTs, dim3(ks == 4 ? cdiv((int)M, 32) : cdiv((int)M, 128 * MB), chunks), xT, ws.x2T, XL, ws.Wf, c.bias[l], xoutT, s.HS(l), part,
                          (int)M, F, Hl, ks);
    } else {
      const long npack = (long)chunks * Hp * 2 * JT * 128;
      hipLaunchKernelGGL(cin_pack_wf_kernel, dim3((int)std::min<long>((npack + 255) / 256, 2048)), dim3(256), 0, st, c.W[l], ws.Wf, Hp, F, Hl, 2 * JT, chunks);
      const float* wsn = nullptr;
      if (fuse_next) {
        FIL_CIN_CHECK_ARG(c.W[l + 1] && c.bias[l + 1]);
        float* wsn_buf = ws.Wf + (size_t)npack;   // behind this layer's packed weights
        hipLaunchKernelGGL(cin_wsum_wsn_kernel, dim3(cdiv(Hl * F, 8)), dim3(256), 0, st, c.W[l + 1], ws.wsum, Hl * F, H[l + 1], wsn_buf, Hl, F, 2 * JT,
                           chunks);
        wsn = wsn_buf;
        c.pa.chunks[l + 1] = chunks;
        c.fused_last = true;
      }
      ProfScope ps(kFwdNames[l], st, gemm_flops(M, Hp, F, Hl) + (fuse_next ? 2.0 * (double)M * Hl * F : 0.0));
      cin_launch_fwd3(st, MB, JT, dim3(cdiv((int)M, 128 * MB), chunks), xT, xpT, xps, ws.Wf, c.bias[l], xoutT, s.HS(l), part, (int)M, F, Hp, Hl,
                      wsn, fuse_next ? c.bias[l + 1] : nullptr, fuse_next ? H[l + 1] : 0, fuse_next ? ws.pool[l + 1] : nullptr);
    }
  }
  FIL_CIN_FWD_LAUNCHED();
  c.xpT = xoutT;
  return FIL_OK;
}

static int cin_fwd_head(CinFwd& c) {
  const int B = c.s.B, K = c.s.K, L = c.s.L;
  if (!c.head_done) {
    ProfScope ps("cin_head_fwd", c.st);
    hipLaunchKernelGGL(cin_head_fwd_kernel, dim3(cdiv(B, kHeadSamples)), dim3(256), (size_t)kHeadSamples * L * K * sizeof(float), c.st, c.pa, c.dense_w, c.dense_b,
                       c.pooled, c.output_dim == 1 ? c.out : nullptr, B, K, L);
  }
  FIL_CIN_FWD_LAUNCHED();
  return FIL_OK;
}

static int cin_fwd_impl(const char* who, const float* x, const float* const* W, const float* const* bias, const float* dense_w,
                        const float* dense_b, float* out, float* pooled, float* saved, int B, int F, int K, int L,
                        const int* H, int output_dim, int mode, int precision, void* workspace, size_t workspace_bytes, void* stream) {
  CinFwd c{};
  c.who = who;
  int rc = check_shape(who, B, F, K, L, H, c.s);
  if (rc != FIL_OK) return rc;
  if ((rc = cin_path(who, c.s, mode, precision, &c.p)) != FIL_OK) return rc;
  if (B == 0) return FIL_OK;
  FIL_CIN_CHECK_ARG(x && W && bias && pooled && saved);
  FIL_CIN_CHECK_ARG(output_dim != 1 || (dense_w && dense_b && out));
  const size_t need = fwd_ws_bytes(c.s);
  if (workspace == nullptr || workspace_bytes < need) return fail(FIL_ERR_WORKSPACE, "fil_cin_fwd: workspace %zu < %zu bytes", workspace_bytes, need);
  c.st = (hipStream_t)stream;
  c.x = x, c.W = W, c.bias = bias, c.dense_w = dense_w, c.dense_b = dense_b, c.out = out, c.pooled = pooled, c.output_dim = output_dim;
  LayoutCarver wsc(workspace), svc(saved);
  c.ws.lay_out(wsc, c.s);
  c.sv.lay_out(svc, c.s, c.p.tg, saved_form(c.p));
  for (int l = 0; l < L; ++l) c.pa.part[l] = c.ws.pool[l], c.pa.chunks[l] = chunks_of(H[l]);
  c.xT = c.xpT = c.p.xt_in ? x : c.sv.xT;
  if ((rc = cin_fwd_prepare(c)) != FIL_OK) return rc;
  const int ltail = !c.p.tail ? L : (c.p.fwdq(c.s) ? 0 : c.p.tg.p);   // the tail takes every layer from here up
  for (int l = 0; l < L && rc == FIL_OK; ++l) {
    FIL_CIN_CHECK_ARG(W[l] && bias[l]);
    if (l < ltail) rc = cin_fwd_general_layer(c, l);
    else rc = c.p.fwdq(c.s) ? cin_fwd_merged_q(c) : (c.p.qtail ? cin_fwd_qtail(c, l) : cin_fwd_fused_tail(c, l));
    if (l == ltail) break;
  }
  return rc != FIL_OK ? rc : cin_fwd_head(c);
}

extern "C" int fil_cin_fwd(const float* x, const float* const* W, const float* const* bias, const float* dense_w,
                           const float* dense_b, float* out, float* pooled, float* saved, int B, int F, int K, int L,
                           const int* H, int output_dim, int mode, void* workspace, size_t workspace_bytes, void* stream) {
  return cin_fwd_impl("fil_cin_fwd", x, W, bias, dense_w, dense_b, out, pooled, saved, B, F, K, L, H, output_dim, mode, FIL_CIN_PREC_DEFAULT, workspace,
                      workspace_bytes, stream);
}

extern "C" int fil_cin_fwd_p(const float* x, const float* const* W, const float* const* bias, const float* dense_w,
                             const float* dense_b, float* out, float* pooled, float* saved, int B, int F, int K, int L,
                             const int* H, int output_dim, int mode, int precision, void* workspace, size_t workspace_bytes, void* stream) {
  return cin_fwd_impl("fil_cin_fwd_p", x, W, bias, dense_w, dense_b, out, pooled, saved, B, F, K, L, H, output_dim, mode, precision, workspace,
                      workspace_bytes, stream);
}

struct CinBwd : CinCall {
  const float *pooled, *g;
  float* dx;
  float* const* dW;
  float* const* dbias;
  float *ddense_w, *ddense_b;
  void* const* events;
  CinBwdWs ws;
  const float* dPsrc;          // dL/dpooled [B][L*K]: g itself (output_dim != 1) or ws.dP
  int nblk, ncol, ndc;         // blocks of the head's partial sums / of the column sums / of the quadratic tail's 256-row blocks
  int ready_slot[kCinMaxL + 1];   // cin_ready_order
  // running state
  int nready = 0;              // slots recorded so far
  int cur = 0;                 // ws.G[cur] holds the gradient of the map the next layer down reads
  int ltop;                    // first layer handled by the general kernels
  bool dx_started = false;     // has dxT been initialised yet
  bool have_gx0 = false;       // did a general layer-1 kernel produce Gx^0
  bool wz_prepacked = false;   // a tail with L == 3: layer 0's dZ weights were packed by the tail's first launch
  bool qm_joined = false;      // merged quadratic tail: the two-pass dZ launch left nothing for the final transpose
};

// grad_ready_events[l] (l < L): recorded once dW[l] and dbias[l] are final; [L]: the dense head's gradients.  The
// data-parallel caller makes a side stream wait on them and starts each layer's all-reduce while the rest of the
// backward is still running (gradients become final from the top layer down, in cin_ready_order's order).
static void cin_record_ready(const CinBwd& c, int slot) {
  if (c.events != nullptr && c.events[slot] != nullptr) (void)hipEventRecord((hipEvent_t)c.events[slot], c.st);
}
static void ready_next(CinBwd& c) { cin_record_ready(c, c.ready_slot[c.nready++]); }

// ---- head backward: dP, ddense_w, ddense_b
static int cin_bwd_head(CinBwd& c) {
  const int B = c.s.B, LK = c.s.L * c.s.K;
  hipStream_t st = c.st;
  c.dPsrc = c.g;  // output_dim != 1: g is already dL/dpooled
  if (c.output_dim == 1 && c.p.qmerge) {
    c.dPsrc = c.ws.dP;   // (merged launches: the head's backward rides in cin_qtail_xe_kernel / cin_reduce_expand_q_kernel)
  } else if (c.output_dim == 1) {
    ProfScope ps("cin_head_bwd", st);
    hipLaunchKernelGGL(cin_head_bwd_kernel, dim3(c.nblk), dim3(256), 0, st, c.g, c.dense_w, c.pooled, c.ws.dP, c.ws.small, B, LK, kHeadChunk);
    // (fused / quadratic tail: the fixed-order sum of the head's partials rides in the tail's first launch)
    if (!c.p.tail)
      hipLaunchKernelGGL(cin_reduce_kernel, dim3(cdiv(LK + 1, 64)), dim3(256), 0, st, c.ws.small, c.ddense_w, (long)(LK + 1), c.nblk, c.ddense_b, (long)LK);
    FIL_CIN_BWD_LAUNCHED();
    c.dPsrc = c.ws.dP;
  }
  if (!c.p.tail) ready_next(c);   // the dense head
  return FIL_OK;
}

// the quadratic tail's parameter gradients from dT, v and the dc partials: dW_p, then dW_L, dbias_p, dbias_L
static void cin_qtail_params_fill(const CinBwd& c) {
  const TailGeom& tg = c.p.tg;
  const CinBwdWs& ws = c.ws;
  const int F = c.s.F, p = tg.p, lL = c.s.L - 1, Hpp = tg.Hpp, Hq = tg.Hq;
  ProfScope ps("cin_tail_params", c.st);
  const size_t sh = cin_qtail_params_lds(F, Hq);   // (at least the 4 x 64 floats the extra workgroup folds the dc partials through)
  allow_lds(cin_qtail_params_kernel, sh);
  float* dcfin = ws.dcpart + (size_t)c.ndc * kQtConst;
  hipLaunchKernelGGL(cin_qtail_params_kernel, dim3(2 * Hpp + 1), dim3(256), sh, c.st, c.W[p], c.sv.wsumL, ws.dT, ws.vlast, c.dW[p], ws.part, Hpp, F, Hq, ws.dcpart, c.ndc,
                     dcfin);
  hipLaunchKernelGGL(cin_qtail_fill_kernel, dim3(cdiv(Hq * F, kQtFillCols)), dim3(kQtFillThreads), 0, c.st, ws.part, Hpp, dcfin, c.bias[p], c.sv.wsumL, c.dW[lL], c.dbias[p],
                     c.dbias[lL], F, Hq, tg.HL);
}

// ---- quadratic tail with merged weight gradients (cin_qmerge.h): [dW1 | dT] = pairs(x)^T [G1 | dP_L x1] in ONE launch; the data
// gradients are one two-pass launch of the pair-symmetric dZ kernel (G1 with W1, then the unscaled x1 with T, scaled by dP_L), or two
// launches of it.  G1 = dP_p S + dP_1 + dP_L R and the shortcut's dX part come out of cin_last_bwd2_kernel -- or, where the forward
// saved the g-free G1 in R's place (cin_ghat_used), G1 = g Ghat is formed inside the two GEMMs and only the dX part is left: for
// cin_shortcut_dx_kernel (cin_shortdx_used), or for that kernel's second phase.
static int cin_bwd_top_merged_q(CinBwd& c) {
  const CinShape& s = c.s;
  const TailGeom& tg = c.p.tg;
  const CinSaved& sv = c.sv;
  const CinBwdWs& ws = c.ws;
  const int F = s.F, K = s.K, L = s.L, JT = s.JT(), LK = s.L * s.K, *H = s.H;
  const long M = s.M();
  const bool qsplit = c.p.qsplit;
  const float* xT = c.xT;
  hipStream_t st = c.st;
  const int p = tg.p, lL = L - 1, Hpp = tg.Hpp, Hq = tg.Hq, HS0 = s.HS(0);
  FIL_CIN_CHECK_ARG(c.bias && c.W[0] && c.W[p] && c.W[lL] && c.bias[p] && c.dW[0] && c.dW[p] && c.dW[lL] && c.dbias[0] && c.dbias[p] && c.dbias[lL]);
  const float* xpT = sv.maps[p - 1];
  const int xps = s.xps(p);
  const float* dPp = c.dPsrc + (size_t)p * K;
  const float* dPL = c.dPsrc + (size_t)lL * K;
  const float* dPprev = c.dPsrc + (size_t)(p - 1) * K;
  const double algo_tail = gemm_flops(M, Hpp, F, Hq) + gemm_flops(M, Hq, F, tg.HL);   // the top two layers of the reference graph
  const double algo1 = gemm_flops(M, F, F, H[0]);
  const int symD = F / 2 + 1, Cl = F * symD;
  const int JTs = cin_jt_sym(F);
  const int periods = cin_dz_periods(F, JTs), tiles0 = cin_slot_tiles(F, JTs);
  const bool ghat = cin_ghat_used(s, c.p, c.output_dim);   // saved.R holds the g-free G1: G1 = g[b] Ghat is applied by the GEMMs, ws.G stays untouched
  const CinBwdWs::Scratch v = ws.scratch(s, true, ghat);   // xe [M][F+3]: x | 1 | dP_L | dP_p   (ghat: [M][F+4], | g)
  const float* G = ghat ? sv.R : ws.G[c.cur];
  const float* gsc = ghat ? c.g : nullptr;
  {
    ProfScope ps("cin_tail_a", st, (double)M * (2 * F + 3) * sizeof(float));
    const size_t sh = (size_t)256 * (F + 3 + (c.output_dim == 1 ? L : 0) + (ghat ? 1 : 0)) * sizeof(float);
    allow_lds(cin_qtail_xe_kernel<3>, sh);
    allow_lds(cin_qtail_xe_kernel<1>, sh);
    const int np = (int)std::min<long>(((long)tiles0 * 32 * HS0 + 255) / 256, 1024);   // + W1 in the dZ kernel's slot order
    const int nq2 = qsplit ? 2 * std::min(cdiv(tiles0 * 512, 256), 256) : 0;           // + (split-bf16 mode) W1s and Ts in slot order as planes
    // (output_dim == 1: + the dense head's backward -- dP and the block partials of ddense_w | ddense_b)
    if (c.p.qnp == 1)
      hipLaunchKernelGGL(cin_qtail_xe_kernel<1>, dim3(c.ndc + np + nq2), dim3(kXeThreads), sh, st, xT, dPL, dPp, LK, K, v.xr, ws.dcpart, (int)M, F,
                         c.ndc, c.output_dim == 1 ? c.g : nullptr, c.dense_w, c.pooled, ws.dP, ws.hpart, LK, lL, p, c.W[0], ws.Wz, H[0], JTs, HS0, tiles0, np, sv.T,
                         Hpp, ws.Wzb1, ws.Wzb2, ghat ? 1 : 0);
    else
      hipLaunchKernelGGL(cin_qtail_xe_kernel<3>, dim3(c.ndc + np + nq2), dim3(kXeThreads), sh, st, xT, dPL, dPp, LK, K, v.xr, ws.dcpart, (int)M, F,
                         c.ndc, c.output_dim == 1 ? c.g : nullptr, c.dense_w, c.pooled, ws.dP, ws.hpart, LK, lL, p, c.W[0], ws.Wz, H[0], JTs, HS0, tiles0, np, sv.T,
                         Hpp, ws.Wzb1, ws.Wzb2, ghat ? 1 : 0);
  }
  FIL_CIN_BWD_LAUNCHED();
  {
    ProfScope ps("cin_last_bwd", st, 6.0 * (double)M * Hpp * F);
    if (cin_shortdx_used(s, c.p, c.output_dim))   // the shortcut's dX part alone (G1 = g Ghat needs no pass of its own), by its own kernel
      cin_launch_shortcut_dx(st, xpT, xps, sv.wsumP, dPp, LK, ws.dxT, (int)M, F, K, Hpp);
    else if (ghat)
      cin_launch_last_bwd2(st, JT, xT, xpT, xps, sv.wsumP, sv.wsnP, dPp, LK, nullptr, nullptr, HS0, ws.dxT, (int)M, F, K, Hpp);
    else
      cin_launch_last_bwd2(st, JT, xT, xpT, xps, sv.wsumP, sv.wsnP, dPp, LK, dPprev, ws.G[c.cur], HS0, ws.dxT, (int)M, F, K, Hpp, sv.R, HS0, dPL, ws.small);
  }
  FIL_CIN_BWD_LAUNCHED();
  int dw_parts = 0;   // partials [C][256] the weight-gradient launch leaves
  {
    ProfScope ps("cin_bwd_dw_q", st, algo1 + algo_tail, gemm_flops(M, 1, Cl, H[0]) + gemm_flops(M, 1, Cl, Hpp));
    if (qsplit) {   // split-bf16 operands (cin_qsplit.h): one partial per row split
      const DwqbPlan bp = cin_dwqb_plan(M, Cl + F, cu_count());
      cin_launch_dwq_b(st, c.p.qnp, bp, G, xpT, HS0, v.xr, v.XS, ws.part, (int)M, F, symD);
      dw_parts = bp.splits;
    } else {
      const bool f4 = knobs().dwfold4 != 0;
      const int Cw = Cl + F + (ghat ? 1 : 0);   // (ghat: + the ones row whose first 128 columns are dbias_1 = sum_m g Ghat[m,:])
      const DwqPlan dp = f4 ? cin_dwq_plan4(M, Cw, cu_count()) : cin_dwq_plan(M, Cw, cu_count());
#define FIL_DWQ(FOLDV, GHV) \
  hipLaunchKernelGGL((cin_dwq_kernel<kDwqDepth, FOLDV, GHV>), dim3((dp.wgs + 7) / 8 * 8), dim3(kDwqThreads), 0, st, G, xpT, HS0, v.xr, v.XS, ws.part, (int)M, F, \
                     symD, dp.rows_per_split, dp.splits, dp.ncol_full, dp.rem, dp.wgs_full, dp.wgs)
      if (ghat) {
        if (f4) FIL_DWQ(4, true); else FIL_DWQ(2, true);
      } else {
        if (f4) FIL_DWQ(4, false); else FIL_DWQ(2, false);
      }
#undef FIL_DWQ
      dw_parts = dp.pairs;
    }
  }
  FIL_CIN_BWD_LAUNCHED();
  {
    // fixed-order sums of the partials -> dW1 (both rows of a pair), dT, v^T; + dbias1 from the column sums cin_last_bwd2_kernel left
    // (ghat: from the ones row of the partials)
    ProfScope ps("cin_reduce_dw", st);
    const int nb1 = ghat ? 0 : cdiv(H[0], 64);
    const int nh = c.output_dim == 1 ? cdiv(LK + 1, 64) : 0;   // + ddense_w | ddense_b from the head's block partials
    if (ghat)
      hipLaunchKernelGGL(cin_reduce_expand_q_kernel<true>, dim3((Cl + F + 1 + 3) / 4 + nh), dim3(256), 0, st, ws.part, dw_parts, F, symD, H[0], Hpp, c.dW[0], ws.dT,
                         ws.vlast, ws.small, c.ncol, c.dbias[0], nb1, ws.hpart, c.ndc, LK, c.ddense_w, c.ddense_b);
    else
      hipLaunchKernelGGL(cin_reduce_expand_q_kernel<false>, dim3((Cl + F + 3) / 4 + nb1 + nh), dim3(256), 0, st, ws.part, dw_parts, F, symD, H[0], Hpp, c.dW[0], ws.dT,
                         ws.vlast, ws.small, c.ncol, c.dbias[0], nb1, ws.hpart, c.ndc, LK, c.ddense_w, c.ddense_b);
  }
  FIL_CIN_BWD_LAUNCHED();
  ready_next(c);   // the dense head
  ready_next(c);   // layer 0
  cin_qtail_params_fill(c);
  FIL_CIN_BWD_LAUNCHED();
  ready_next(c);   // layer L-1
  ready_next(c);   // layer L-2
  const int NHMAX = HS0 / 2;
  if (NHMAX == 64 && knobs().dz2 != 0) {
    // both data-gradient passes in one launch (cin_dz2_kernel): G1 with W1, then dP_L x1 with T, into one dX image
    ProfScope ps("cin_bwd_dz_q", st, algo1 + algo_tail, gemm_flops(M, 1, Cl, H[0]) + gemm_flops(M, 1, Cl, Hpp));
    // (the kernel also finishes dx: + the shortcut's part in dxT, + dP_L c, transposed to [B,F,K] on the way out)
    bool split_done = false;
    if (qsplit) {   // split-bf16 operands (the planes of both layers' slot-ordered weights came out of the operand-row launch)
      split_done = cin_launch_dz2_b(st, c.p.qnp, JTs, G, xpT, HS0, dPL, LK, K, ws.Wzb1, ws.Wzb2, xT, ws.dxT, /*accumulate=*/1, (int)M, F, H[0], Hpp, periods, c.dx, sv.cvec);
    }
    if (!split_done &&
        !cin_launch_dz2(st, JTs, G, xpT, HS0, dPL, LK, K, ws.Wz, sv.WzT, xT, ws.dxT, /*accumulate=*/1, (int)M, F, H[0], Hpp, periods, c.dx, sv.cvec, gsc))
      return fail(FIL_ERR_UNSUPPORTED, "fil_cin_bwd: no two-pass data-gradient kernel for JT=%d (F=%d)", JTs, F);
    c.qm_joined = true;
  } else {
    const DzsShape z = dzs_launch_shape(c.p.tune, M, JTs, NHMAX);
    {
      ProfScope ps("cin_bwd_dz_tail", st, algo_tail, gemm_flops(M, 1, Cl, Hpp));   // (T in slot order: packed and saved by the forward)
      cin_launch_dz3_sym(st, z.MBs, JTs, NHMAX, z.grid, xpT, HS0, sv.WzT, xT, v.gxR, v.dxR, 0, (int)M, F, Hpp, periods, z.ks);
      // (gxR + dxR, scaled by dP_L, and the linear term join dX in the final transpose)
    }
    FIL_CIN_BWD_LAUNCHED();
    {
      ProfScope ps("cin_bwd_dz_l1", st, algo1, gemm_flops(M, 1, Cl, H[0]));
      cin_launch_dz3_sym(st, z.MBs, JTs, NHMAX, z.grid, G, HS0, ws.Wz, xT, ws.gx0T, ws.dxT, 1, (int)M, F, H[0], periods, z.ks);
    }
    c.have_gx0 = true;
  }
  FIL_CIN_BWD_LAUNCHED();
  c.dx_started = true;
  c.ltop = -1;
  return FIL_OK;
}

// ---- quadratic tail (cin_qtail.h).  pool_p goes back through the pooled-weights shortcut of layer p; pool_L = <x1, R> through the
// first layer's pair-symmetric dW / dZ kernels with x1 (unscaled) as their "gradient" operand: dT = (pairs of x, one factor scaled
// by dP_L)^T x1, the two halves of d<x1,R>/dx come out per row and are scaled by dP_L afterwards; G^{p-1} += dP_L R is elementwise.
static int cin_bwd_top_qtail(CinBwd& c) {
  const CinShape& s = c.s;
  const TailGeom& tg = c.p.tg;
  const CinSaved& sv = c.sv;
  const CinBwdWs& ws = c.ws;
  const int F = s.F, K = s.K, L = s.L, JT = s.JT(), LK = s.L * s.K, *H = s.H;
  const long M = s.M();
  const float* xT = c.xT;
  hipStream_t st = c.st;
  const int p = tg.p, lL = L - 1, Hpp = tg.Hpp, Hq = tg.Hq, HS0 = s.HS(0);
  FIL_CIN_CHECK_ARG(c.bias && c.W[p] && c.W[lL] && c.bias[p] && c.dW[p] && c.dW[lL] && c.dbias[p] && c.dbias[lL]);
  const float* xpT = sv.maps[p - 1];
  const int xps = s.xps(p);
  const float* dPp = c.dPsrc + (size_t)p * K;
  const float* dPL = c.dPsrc + (size_t)lL * K;
  const float* dPprev = c.dPsrc + (size_t)(p - 1) * K;
  const double algo = gemm_flops(M, Hpp, F, Hq) + gemm_flops(M, Hq, F, tg.HL);
  const int symD = F / 2 + 1, Cl = F * symD;
  const int JTs = cin_jt_sym(F);
  const CinBwdWs::Scratch v = ws.scratch(s, false);   // xs [M][F+1]: dP_L x | dP_p  (L == 3: the layer loop runs layer 0 only)
  {
    ProfScope ps("cin_tail_a", st, (double)M * (F + 64) * sizeof(float));
    const size_t sh = (size_t)256 * (F + 3) * sizeof(float);
    allow_lds(cin_qtail_scale_kernel, sh);
    const int nh = c.output_dim == 1 ? cdiv(LK + 1, 64) : 0;   // + the head's partial sums (as in the fused tail's first launch)
    // ... and the first layer's dZ weights in slot order (the packed-W buffer is idle until that layer's dZ kernel)
    FIL_CIN_CHECK_ARG(c.W[0]);
    const int tiles0 = cin_slot_tiles(F, JTs);
    const int np = (int)std::min<long>(((long)tiles0 * 32 * HS0 + 255) / 256, 1024);
    hipLaunchKernelGGL(cin_qtail_scale_kernel, dim3(c.ndc + nh + np), dim3(256), sh, st, xT, dPL, dPp, LK, K, v.xr, ws.dcpart, (int)M, F, c.ndc, ws.small,
                       c.ddense_w, c.ddense_b, LK, c.nblk, nh, c.W[0], ws.Wz, H[0], JTs, HS0, tiles0);
    c.wz_prepacked = true;
  }
  FIL_CIN_BWD_LAUNCHED();
  ready_next(c);   // the dense head
  {
    // pooled-weights shortcut of layer p: G^{p-1} = dP_p S + dP_{p-1} (+ dP_L R), dX = dP_p x1 wsum_p
    ProfScope ps("cin_last_bwd", st, 6.0 * (double)M * Hpp * F);
    // (wsum_p and its operand copy were saved by the forward; + dP_L R on the way out: the pool_L part of G^{p-1})
    // (... and the partial column sums of G^{p-1} for dbias_{p-1}: `small` is free again, the head's partials were reduced above)
    cin_launch_last_bwd2(st, JT, xT, xpT, xps, sv.wsumP, sv.wsnP, dPp, LK, dPprev, ws.G[c.cur], HS0, ws.dxT, (int)M, F, K, Hpp, sv.R, HS0, dPL, ws.small);
  }
  FIL_CIN_BWD_LAUNCHED();
  {
    ProfScope ps("cin_bwd_dw_tail", st, algo, gemm_flops(M, 1, Cl, Hpp));
    // F extra channel rows behind the pairs: v^T[f][h] = sum_m dP_p[m] x[m,f] x1[m,h], the rank-one part of dW_p (column F of xs)
    const int parts = launch_dw3(st, dw_plan(M, Cl + F, Hpp), xpT, HS0, xT, v.xr, v.XS, ws.part, M, F, F, Hpp, symD, /*xtra=*/F);
    const long nW = (long)Cl * Hpp, pstride = (long)(Cl + F) * Hpp;
    hipLaunchKernelGGL(cin_reduce_expand_sym_kernel, dim3((int)((nW + 63) / 64) + cdiv(F * Hpp, 64)), dim3(256), 0, st, ws.part, ws.dT, F, symD, Hpp, parts,
                       pstride, ws.vlast, (long)F * Hpp);
  }
  FIL_CIN_BWD_LAUNCHED();
  cin_qtail_params_fill(c);
  FIL_CIN_BWD_LAUNCHED();
  ready_next(c);   // layer L-1
  ready_next(c);   // layer L-2
  {
    ProfScope ps("cin_bwd_dz_tail", st, algo, gemm_flops(M, 1, Cl, Hpp));   // (T in slot order: packed and saved by the forward)
    const int NHMAX = HS0 / 2;
    const DzsShape z = dzs_launch_shape(c.p.tune, M, JTs, NHMAX);
    cin_launch_dz3_sym(st, z.MBs, JTs, NHMAX, z.grid, xpT, HS0, sv.WzT, xT, v.gxR, v.dxR, 0, (int)M, F, Hpp, cin_dz_periods(F, JTs), z.ks);
    // (gxR + dxR, scaled by dP_L, and the linear term join dX in the final transpose)
  }
  FIL_CIN_BWD_LAUNCHED();
  c.dx_started = true;
  c.ltop = p - 1;
  return FIL_OK;
}

// ---- fused tail: both top layers' parameter gradients from Q = Z_p^T A (F+2 columns), data gradients from A Ueff^T
static int cin_bwd_top_fused_tail(CinBwd& c) {
  const CinShape& s = c.s;
  const TailGeom& tg = c.p.tg;
  const CinSaved& sv = c.sv;
  const CinBwdWs& ws = c.ws;
  const int F = s.F, K = s.K, L = s.L, JT = s.JT(), LK = s.L * s.K, *H = s.H;
  const long M = s.M();
  const float* xT = c.xT;
  hipStream_t st = c.st;
  const int p = tg.p, lL = L - 1;
  FIL_CIN_CHECK_ARG(c.bias && c.W[p] && c.W[lL] && c.bias[p] && c.dW[p] && c.dW[lL] && c.dbias[p] && c.dbias[lL]);
  const float* xpT = sv.maps[p - 1];
  const int xps = s.xps(p);
  const double algo = gemm_flops(M, tg.Hpp, F, tg.Hq) + gemm_flops(M, tg.Hq, F, tg.HL);   // the two layers of the reference graph
  float* Apk = ws.G[1];
  // the first general layer below the tail is the pair-symmetric layer 0 (L == 3): its slot-ordered weights can be packed now
  // (nothing else uses the packed-W buffer any more), together with A and the head's partial sums -- one launch for the three
  c.wz_prepacked = p == 1 && c.p.tune.sym && F >= 2;
  {
    ProfScope ps("cin_tail_a", st, (double)M * (F + 64) * sizeof(float));
    const int na = (int)std::min<long>((M * 16 * tg.NCB + 255) / 256, 4096);
    const int nh = c.output_dim == 1 ? cdiv(LK + 1, 64) : 0;
    int np = 0, JTs = 0, tiles0 = 0;
    if (c.wz_prepacked) {
      FIL_CIN_CHECK_ARG(c.W[0]);
      JTs = cin_jt_sym(F);
      tiles0 = cin_slot_tiles(F, JTs);
      np = (int)std::min<long>(((long)tiles0 * 32 * s.HS(0) + 255) / 256, 1024);
    }
    hipLaunchKernelGGL(cin_tail_pre_kernel, dim3(na + nh + np), dim3(256), 0, st, xT, c.dPsrc, LK, K, p, lL, Apk, (int)M, F, tg.NCB, na, ws.small,
                       c.ddense_w, c.ddense_b, LK, c.nblk, nh, c.W[0], ws.Wz, H[0], JTs, s.HS(0), tiles0);
  }
  FIL_CIN_BWD_LAUNCHED();
  ready_next(c);   // the dense head
  const TailDwPlan tp = tail_dw_plan(M, tg.C1);
  {
    ProfScope ps("cin_bwd_dw_tail", st, algo, 2.0 * (double)M * tg.C1 * (F + 2));
    TailDwArgs a{Apk, xT, xpT, xps, ws.part, (int)M, F, tg.Hpp, tg.JP, tp.rows_per_split, tp.blocks_x, tp.blocks_x * tp.splits, knobs().tail_settle != 0};
    cin_launch_tail_dw(st, tg.NCB, a);
  }
  FIL_CIN_BWD_LAUNCHED();
  {
    ProfScope ps("cin_tail_params", st);
    const int nblk_p = cdiv(tg.Cp, kTailPc);
    const int ldb = (tg.Hq + 3) & ~3;
    const size_t sh = ((size_t)(F + 1) * ldb + (size_t)tg.JP * (kTailPc + 4) + (size_t)kTailPc * ldb) * sizeof(float);
    allow_lds(cin_tail_params_kernel, sh);
    // the dwsum_L partials go behind the Q partials in `part`; the reduced ones row of Q into the (idle) v buffer of the last-layer shortcut
    float* partB = ws.part + (size_t)tp.splits * tg.C1 * tg.JP;
    float* qones = ws.vlast;
    hipLaunchKernelGGL(cin_tail_params_kernel, dim3(2 * nblk_p), dim3(256), sh, st, ws.part, tp.splits, c.W[p], sv.bmT, c.dW[p], c.dbias[p], partB, qones,
                       tg.Cp, F, tg.Hq, tg.JP);
    hipLaunchKernelGGL(cin_tail_fill_kernel, dim3(cdiv(tg.Hq * F, 64)), dim3(256), 0, st, partB, nblk_p, qones, c.bias[p], c.dW[lL], c.dbias[lL], F,
                       tg.Hq, tg.HL);
  }
  FIL_CIN_BWD_LAUNCHED();
  ready_next(c);   // layer L-1
  ready_next(c);   // layer L-2
  {
    ProfScope ps("cin_bwd_dz_tail", st, algo, 2.0 * (double)M * tg.Cp * (F + 1));
    TailDzArgs a{sv.Uz, xT, xpT, xps, sv.Y, tg.JP, c.dPsrc, LK, K, p, lL, ws.G[c.cur], s.HS(p - 1), ws.dxT, (int)M, F, tg.Hpp, tg.periods, knobs().tail_dz_mode,
                 c.p.tune.ksplit(M)};
    cin_launch_tail_dz(st, JT, tg.NQ, a);
  }
  FIL_CIN_BWD_LAUNCHED();
  c.dx_started = true;
  c.ltop = p - 1;
  return FIL_OK;
}

// ---- last layer through the pooled-weights shortcut (see cin_last_* kernels)
static int cin_bwd_top_shortcut(CinBwd& c) {
  const CinShape& s = c.s;
  const CinBwdWs& ws = c.ws;
  const int B = s.B, F = s.F, K = s.K, L = s.L, JT = s.JT(), LK = s.L * s.K, nblk = c.nblk;
  const long M = s.M();
  const float* xT = c.xT;
  hipStream_t st = c.st;
  const int l = L - 1;
  FIL_CIN_CHECK_ARG(c.W[l] && c.dW[l] && c.dbias[l]);
  const int Hp = s.Hp(l), Hl = s.H[l], xps = s.xps(l);
  const size_t cl = (size_t)Hp * F;
  const float* xpT = l == 0 ? xT : c.sv.maps[l - 1];
  const float* dPl = c.dPsrc + (size_t)l * K;
  const float* dPprev = l > 0 ? c.dPsrc + (size_t)(l - 1) * K : nullptr;
  const size_t shw = (size_t)Hp * ((F + 3) & ~3) * sizeof(float);
  ProfScope ps("cin_last_bwd", st, 6.0 * (double)M * Hp * F);
  // (l > 0: wsum also in the MFMA operand layout of cin_last_bwd2_kernel -- the dZ kernels' packed-W buffer is idle until
  // the first general layer packs into it, and nothing between here and that kernel touches it)
  hipLaunchKernelGGL(cin_wsum_wsn_kernel, dim3(cdiv(Hp * F, 8)), dim3(256), 0, st, c.W[l], ws.wsum, Hp * F, Hl, l > 0 ? ws.Wz : nullptr, Hp, F, 2 * JT,
                     chunks_of(Hp));
  hipLaunchKernelGGL(cin_slice_sum_kernel, dim3(nblk), dim3(256), 0, st, dPl, LK, ws.small, B, K, kHeadChunk);
  // dW_L[c,:] = v[c],  v[h,f] = sum_m x^{L-1}[m,h] * (x[m,f] dP[m]): the weight-gradient kernel with a single
  // all-ones field (F' = 1, so c = h) and G' = x * dP ([M][128], zero padded) as its right-hand side
  {
    float* yT = ws.G[1];
    const int YS = (F + 3) & ~3;
    const long tot = M * YS;
    hipLaunchKernelGGL(cin_scale_rows3_kernel, dim3((int)std::min<long>((tot + 255) / 256, 4096)), dim3(256), 0, st, xT, dPl, LK, K, yT, (int)M, F, YS);
    // l > 0: the roles are swapped -- the F fields of G' are the channel rows and x^{L-1} ([M][HS], 128-aligned rows) is the
    // streamed right-hand side, so the kernel computes v^T [F][Hp]: 2 channel blocks x a full 128-column chunk instead of
    // 4 blocks x a chunk that is 70 % padding (27 -> 14 us at c4); the fill kernel reads it transposed
    const bool swap = l > 0;
    int nb;
    if (swap) nb = launch_dw3(st, dw_plan(M, F, Hp), xpT, xps, nullptr, yT, YS, ws.part, M, /*F=*/1, /*Hp=*/F, /*H=*/Hp);
    else nb = launch_dw3(st, dw_plan(M, Hp, F), yT, YS, nullptr, xpT, xps, ws.part, M, /*F=*/1, Hp, /*H=*/F);
    hipLaunchKernelGGL(cin_reduce_kernel, dim3(cdiv((int)cl, 64)), dim3(256), 0, st, ws.part, ws.vlast, (long)cl, nb);
    // (the same launch finishes dbias_L from the slice sums above)
    hipLaunchKernelGGL(cin_fill_rows_kernel, dim3((int)std::min<long>(((long)cl * Hl + 255) / 256, 2048)), dim3(256), 0, st, ws.vlast, c.dW[l], (long)cl, Hl,
                       swap ? F : 0, Hp, ws.small, nblk, c.dbias[l]);
  }
  ready_next(c);   // layer L-1
  // G^{L-1} and dX
  if (l > 0) {
    cin_launch_last_bwd2(st, JT, xT, xpT, xps, ws.wsum, ws.Wz, dPl, LK, dPprev, ws.G[c.cur], s.HS(l - 1), ws.dxT, (int)M, F, K, Hp);
  } else {
    const size_t shb = shw + (size_t)kLastRows * (kLastFMax + 1) * sizeof(float);
    allow_lds(cin_last_bwd_kernel, shb);
    hipLaunchKernelGGL(cin_last_bwd_kernel, dim3(cdiv((int)M, kLastRows)), dim3(256), shb, st, xT, xpT, xps, ws.wsum, dPl, LK, dPprev,
                       nullptr, 0, ws.dxT, /*layer1=*/1, (int)M, F, K, Hp);
  }
  FIL_CIN_BWD_LAUNCHED();
  c.dx_started = true;
  c.ltop = L - 2;
  return FIL_OK;
}

// ---- top layer gradient: broadcast of its pooled gradient
static int cin_bwd_top_bcast(CinBwd& c) {
  const CinShape& s = c.s;
  const int L = s.L, LK = s.L * s.K;
  const long total = s.M() * s.HS(L - 1);
  ProfScope ps("cin_bcast_g", c.st, (double)total * sizeof(float));
  hipLaunchKernelGGL(cin_bcast3_kernel, dim3((int)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, c.st, c.dPsrc + (size_t)(L - 1) * s.K, LK,
                     s.K, c.ws.G[c.cur], s.HS(L - 1), (int)s.M(), s.H[L - 1]);
  FIL_CIN_BWD_LAUNCHED();
  c.ltop = L - 1;
  return FIL_OK;
}

// ---- layer l as a layer of its own: dbias (column sums of G), dW (+ fixed-order reduce), pack W_l -> Wz, dZ -> G^{l-1}, dX
static int cin_bwd_general_layer(CinBwd& c, int l) {
  const CinShape& s = c.s;
  const CinTune& tune = c.p.tune;
  const CinBwdWs& ws = c.ws;
  const int F = s.F, K = s.K, JT = s.JT(), LK = s.L * s.K, ncol = c.ncol;
  const long M = s.M();
  const float* xT = c.xT;
  hipStream_t st = c.st;
  FIL_CIN_CHECK_ARG(c.W[l] && c.dW[l] && c.dbias[l]);
  const int Hp = s.Hp(l), Hl = s.H[l], HSl = s.HS(l), xps = s.xps(l);
  const float* xpT = l == 0 ? xT : c.sv.maps[l - 1];
  const float* G = ws.G[c.cur];
  // dbias
  {
    ProfScope ps("cin_dbias", st, (double)M * Hl * sizeof(float));
    // (quadratic tail: the kernel that wrote G left its per-128-row column sums in `small` already)
    if (!(c.p.qtail && l == c.ltop)) hipLaunchKernelGGL(cin_colsum3_kernel, dim3(ncol), dim3(256), 0, st, G, HSl, ws.small, (int)M, Hl, kColRows);
    hipLaunchKernelGGL(cin_reduce_kernel, dim3(cdiv(Hl, 64)), dim3(256), 0, st, ws.small, c.dbias[l], (long)Hl, ncol);
  }
  FIL_CIN_BWD_LAUNCHED();
  // dW
  int parts;
  const int symD = (l == 0 && tune.sym) ? F / 2 + 1 : 0;   // unordered field pairs: half the channels
  const int Cl = symD > 0 ? F * symD : Hp * F;
  {
    ProfScope ps(kDwNames[l], st, gemm_flops(M, Hp, F, Hl), gemm_flops(M, 1, Cl, Hl));
    parts = launch_dw3(st, dw_plan(M, Cl, Hl), G, HSl, xT, xpT, xps, ws.part, M, F, Hp, Hl, symD);
  }
  FIL_CIN_BWD_LAUNCHED();
  const long nW = (long)Cl * Hl;
  {
    ProfScope ps("cin_reduce_dw", st, (double)(parts + 1) * nW * sizeof(float));
    // (pair-indexed first layer: the fixed-order sum is written straight to both dW rows of each pair)
    if (symD > 0) hipLaunchKernelGGL(cin_reduce_expand_sym_kernel, dim3((int)((nW + 63) / 64)), dim3(256), 0, st, ws.part, c.dW[l], F, symD, Hl, parts);
    else hipLaunchKernelGGL(cin_reduce_kernel, dim3((int)((nW + 63) / 64)), dim3(256), 0, st, ws.part, c.dW[l], nW, parts);
  }
  FIL_CIN_BWD_LAUNCHED();
  ready_next(c);   // dW[l], dbias[l] final: the dZ kernel of this layer and everything below can overlap their all-reduce
  // dZ -> G^{l-1}, dX
  {
    const int NHMAX = HSl / 2;                  // 64 (H <= 128) or 128
    // general dZ kernel: 32 rows per wave, two waves per SIMD -- the second wave covers the issue time of the first
    // one's register contraction (c4: 0.715 -> 0.687 ms); FIL_CIN_DZ_MB overrides
    const int MBg = NHMAX == 128 ? 1 : ((knobs().dz_mb == 2 && JT <= 28) ? 2 : 1);   // (JT = 32 at 64 rows: scratch + line buffers > 160 KB of LDS)
    const float* dPprev = l > 0 ? c.dPsrc + (size_t)(l - 1) * K : nullptr;
    if (l == 0 && tune.sym && F >= 2) {
      // first layer over unordered field pairs (half the tiles); F = 1 would make both lane halves hit one word
      const int JTs = cin_jt_sym(F);
      const int tiles = cin_slot_tiles(F, JTs);
      const long npack = (long)tiles * 32 * HSl;
      if (!c.wz_prepacked) {
        hipLaunchKernelGGL(cin_pack_wz_sym_kernel, dim3((int)std::min<long>((npack + 255) / 256, 2048)), dim3(256), 0, st, c.W[l], ws.Wz, F, Hl, JTs, HSl, tiles);
      }
      ProfScope ps(kDzNames[l], st, gemm_flops(M, Hp, F, Hl), gemm_flops(M, 1, F * (F / 2 + 1), Hl));
      const DzsShape z = dzs_launch_shape(tune, M, JTs, NHMAX);
      cin_launch_dz3_sym(st, z.MBs, JTs, NHMAX, z.grid, G, HSl, ws.Wz, xT, ws.gx0T, ws.dxT, c.dx_started ? 1 : 0, (int)M, F, Hl, cin_dz_periods(F, JTs), z.ks);
    } else {
      const int periods = cin_dz_periods(Hp, JT), tiles = cin_slot_tiles(Hp, JT);
      const long npack = (long)tiles * 32 * HSl;
      hipLaunchKernelGGL(cin_pack_wz_kernel, dim3((int)std::min<long>((npack + 255) / 256, 2048)), dim3(256), 0, st, c.W[l], ws.Wz, Hp, F, Hl, JT, HSl, tiles);
      ProfScope ps(kDzNames[l], st, gemm_flops(M, Hp, F, Hl));
      cin_launch_dz3(st, MBg, JT, NHMAX, dim3(cdiv((int)M, 128 * MBg)), G, HSl, ws.Wz, xT, xpT, xps, dPprev, LK, K,
                     l > 0 ? ws.G[c.cur ^ 1] : nullptr, l > 0 ? s.HS(l - 1) : 0, l == 0 ? ws.gx0T : nullptr, ws.dxT, c.dx_started ? 1 : 0,
                     (int)M, F, Hp, Hl, periods);
    }
    c.dx_started = true;
    if (l == 0) c.have_gx0 = true;
  }
  FIL_CIN_BWD_LAUNCHED();
  c.cur ^= 1;
  return FIL_OK;
}

// dxT (+ Gx^0, + the quadratic tail's gxR + dxR scaled by dP_L and its linear term) --transpose--> dx [B,F,K]
static int cin_bwd_finish_dx(CinBwd& c) {
  const CinShape& s = c.s;
  const int F = s.F, K = s.K, LK = s.L * s.K;
  if (!c.qm_joined) {   // (merged quadratic tail: cin_dz2_kernel wrote dx itself)
    ProfScope ps("cin_transpose_out", c.st, 2.0 * s.M() * F * sizeof(float));
    const float* gx0T = c.have_gx0 ? c.ws.gx0T : nullptr;
    if (c.p.qtail) {
      const CinBwdWs::Scratch v = c.ws.scratch(s, c.p.qmerge);
      hipLaunchKernelGGL(cin_transpose_out_kernel, dim3(s.B), dim3(256), (size_t)K * (F + 1) * sizeof(float), c.st, c.ws.dxT, gx0T, c.dx, F, K, v.gxR, v.dxR,
                         c.sv.cvec, c.dPsrc + (size_t)(s.L - 1) * K, LK);
    } else {
      hipLaunchKernelGGL(cin_transpose_out_kernel, dim3(s.B), dim3(256), (size_t)K * (F + 1) * sizeof(float), c.st, c.ws.dxT, gx0T, c.dx, F, K);
    }
  }
  FIL_CIN_BWD_LAUNCHED();
  return FIL_OK;
}

static int cin_bwd_impl(const char* who, const float* x, const float* const* W, const float* const* bias, const float* dense_w,
                        const float* pooled, const float* saved, const float* g, float* dx, float* const* dW,
                        float* const* dbias, float* ddense_w, float* ddense_b, int B, int F, int K, int L, const int* H,
                        int output_dim, int mode, int precision, void* const* grad_ready_events, void* workspace, size_t workspace_bytes,
                        void* stream) {
  CinBwd c{};
  c.who = who;
  int rc = check_shape(who, B, F, K, L, H, c.s);
  if (rc != FIL_OK) return rc;
  if ((rc = cin_path(who, c.s, mode, precision, &c.p)) != FIL_OK) return rc;
  FIL_CIN_CHECK_ARG(W && dW && dbias);
  c.st = (hipStream_t)stream;
  c.events = grad_ready_events;
  if (B == 0) {  // empty batch: parameter gradients are zero
    for (int l = 0; l < L; ++l) {
      (void)hipMemsetAsync(dW[l], 0, (size_t)c.s.Hp(l) * F * H[l] * sizeof(float), c.st);
      (void)hipMemsetAsync(dbias[l], 0, (size_t)H[l] * sizeof(float), c.st);
    }
    if (output_dim == 1) {
      (void)hipMemsetAsync(ddense_w, 0, (size_t)L * K * sizeof(float), c.st);
      (void)hipMemsetAsync(ddense_b, 0, sizeof(float), c.st);
    }
    for (int l = 0; l <= L; ++l) cin_record_ready(c, l);
    return FIL_OK;
  }
  FIL_CIN_CHECK_ARG(g && dx && saved && (x || !c.p.xt_in));
  FIL_CIN_CHECK_ARG(output_dim != 1 || (dense_w && pooled && ddense_w && ddense_b));
  const size_t need = bwd_ws_bytes(c.s);
  if (workspace == nullptr || workspace_bytes < need) return fail(FIL_ERR_WORKSPACE, "fil_cin_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
  c.x = x, c.W = W, c.bias = bias, c.dense_w = dense_w, c.pooled = pooled, c.g = g, c.output_dim = output_dim;
  c.dx = dx, c.dW = dW, c.dbias = dbias, c.ddense_w = ddense_w, c.ddense_b = ddense_b;
  LayoutCarver wsc(workspace), svc(saved);
  c.ws.lay_out(wsc, c.s);
  c.sv.lay_out(svc, c.s, c.p.tg, saved_form(c.p));
  c.xT = c.p.xt_in ? x : c.sv.xT;   // (X_TRANSPOSED: the caller's [B*K][F] copy; the forward left saved's own area unused)
  c.nblk = CinBwdWs::nblk(c.s), c.ncol = (int)CinBwdWs::ncol(c.s), c.ndc = (int)CinBwdWs::ndc(c.s);
  int point[kCinMaxL + 1];
  (void)cin_ready_order(L, c.p, c.ready_slot, point);
  if ((rc = cin_bwd_head(c)) != FIL_OK) return rc;
  if (c.p.qmerge) rc = cin_bwd_top_merged_q(c);
  else if (c.p.qtail) rc = cin_bwd_top_qtail(c);
  else if (c.p.tail) rc = cin_bwd_top_fused_tail(c);
  else if (!c.p.general) rc = cin_bwd_top_shortcut(c);
  else rc = cin_bwd_top_bcast(c);
  for (int l = c.ltop; l >= 0 && rc == FIL_OK; --l) rc = cin_bwd_general_layer(c, l);
  return rc != FIL_OK ? rc : cin_bwd_finish_dx(c);
}

extern "C" int fil_cin_bwd(const float* x, const float* const* W, const float* const* bias, const float* dense_w,
                           const float* pooled, const float* saved, const float* g, float* dx, float* const* dW,
                           float* const* dbias, float* ddense_w, float* ddense_b, int B, int F, int K, int L, const int* H,
                           int output_dim, int mode, void* const* grad_ready_events, void* workspace, size_t workspace_bytes,
                           void* stream) {
  return cin_bwd_impl("fil_cin_bwd", x, W, bias, dense_w, pooled, saved, g, dx, dW, dbias, ddense_w, ddense_b, B, F, K, L, H, output_dim, mode,
                      FIL_CIN_PREC_DEFAULT, grad_ready_events, workspace, workspace_bytes, stream);
}

extern "C" int fil_cin_bwd_p(const float* x, const float* const* W, const float* const* bias, const float* dense_w,
                             const float* pooled, const float* saved, const float* g, float* dx, float* const* dW,
                             float* const* dbias, float* ddense_w, float* ddense_b, int B, int F, int K, int L, const int* H,
                             int output_dim, int mode, int precision, void* const* grad_ready_events, void* workspace, size_t workspace_bytes,
                             void* stream) {
  return cin_bwd_impl("fil_cin_bwd_p", x, W, bias, dense_w, pooled, saved, g, dx, dW, dbias, ddense_w, ddense_b, B, F, K, L, H, output_dim, mode,
                      precision, grad_ready_events, workspace, workspace_bytes, stream);
}
