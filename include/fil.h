/*
 * fil.h -- C ABI of libfil_hip.so: the MI355X (gfx950) feature-interaction hot path.
 *
 * The reference (TIXhjq/ML_Function) is 100% Python/TF2 and has NO native code, so there is no
 * existing FFI to mirror; each entry point below replaces the TF op group that the cited reference
 * lines execute per batch (paths relative to /root/reference/kon/model/ctr_model/layer/).  The
 * Python layer classes in ml_function_amd/layers bind these through ctypes; INTEGRATION.md shows
 * the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch.cuda storage), row-major contiguous;
 *   - the caller allocates and owns every buffer, including workspaces (sizes from *_workspace_bytes);
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *     no entry point synchronises, allocates or frees (graph-capture safe);
 *   - reductions use a fixed two-stage order: repeated calls on the same inputs are bit-identical;
 *   - return value: 0 on success, negative fil_status on error; fil_last_error() gives the message
 *     of the last failing call on the calling thread.
 */
#ifndef FIL_H_
#define FIL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  FIL_OK = 0,
  FIL_ERR_ARG = -1,         /* NULL pointer / non-positive dim / inconsistent arguments */
  FIL_ERR_HIP = -2,         /* a HIP runtime call or kernel launch failed */
  FIL_ERR_WORKSPACE = -3,   /* workspace smaller than *_workspace_bytes() */
  FIL_ERR_UNSUPPORTED = -4  /* shape outside the compiled kernel menu (message says which limit) */
} fil_status;

typedef enum { FIL_F32 = 0, FIL_BF16 = 1 } fil_dtype;

/* ABI version: bumped on EVERY change of an entry point's argument list or semantics.  fil_version() returns the value the
 * library was compiled with; the ctypes binding (ml_function_amd/_lib.py) refuses a library whose value differs from this
 * header's, so a stale prebuilt .so can never be called with shifted arguments.  Entry points that are only ADDED leave it as it
 * is (O1, the Adam entry points, kept 216): the binding already refuses a library that lacks any symbol of its table. */
#define FIL_ABI_VERSION 216
int fil_version(void);                 /* == FIL_ABI_VERSION of the header the library was built from */
const char* fil_last_error(void);      /* thread-local, never NULL */

/* Opt-in per-kernel timing for bench.py's roofline line (off by default).  Between begin and end every major
 * kernel launch made through this library is bracketed by HIP events recorded ON THE LAUNCH STREAM.
 * fil_profile_end synchronises those events and writes one text line per kernel name into buf:
 *   "<name> <launches> <total_ms> <algorithmic work per launch: flops for MFMA kernels, bytes for streaming> <executed work>\n"
 * (algorithmic = what the reference graph spends on that step; executed = what the kernels really compute -- smaller where an
 * exact algebraic restructuring removes products, e.g. the pair-symmetric first CIN layer; equal otherwise)
 * and returns the number of bytes needed (including the NUL).  Not for use under graph capture. */
int fil_profile_begin(const char* filter);   /* filter: "substr[,substr...]" of kernel names to time, NULL = all */
size_t fil_profile_end(char* buf, size_t cap);

/* ---------------------------------------------------------------------------------------------
 * A1  FM second order -- replaces InnerLayer.call + FmLayer.call
 *     interactive_layer/interactive_layer.py:59-66,161-170 (C(F,2) tf.multiply + Add + Add).
 *   emb [B,F,K], lin [B,F] or NULL, out [B,K]:  out[b,k] = sum_{i<j} e_i e_j + sum_f lin[b,f].
 *   dtype selects the storage type of emb/out/g/demb (accumulation is always fp32); lin/dlin are fp32.
 *   bwd: demb[b,f,k] = g[b,k] (S[b,k] - e[b,f,k]);  dlin[b,f] = sum_k g[b,k]  (dlin may be NULL).
 */
int fil_fm_fwd(const void* emb, const float* lin, void* out, int B, int F, int K, int dtype, void* stream);
int fil_fm_bwd(const void* emb, const void* g, void* demb, float* dlin, int B, int F, int K, int dtype, void* stream);

/* N3  InnerLayer(use_add=False) pair list (PNN/AFM input), interactive_layer.py:61:
 *   pairs [B, F(F-1)/2, K] in itertools.combinations order; bwd: demb from gpairs. fp32 only. */
int fil_fm_pairs_fwd(const float* emb, float* pairs, int B, int F, int K, void* stream);
int fil_fm_pairs_bwd(const float* emb, const float* gpairs, float* demb, int B, int F, int K, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A2  DCN cross network -- replaces CrossLayer.call, interactive_layer.py:275-282, all L layers fused.
 *   x [B,D], w [L,D], b [L,D] (the reference's L tensors [D,1] stacked), y [B,D], s [B,L] (saved dots).
 *   bwd: g [B,D] -> dx [B,D], dw [L,D], db [L,D].
 *   Limit: L <= 16.  D <= 4096 with L <= 6 and 2 L D 4 bytes <= 160 KiB run the register-resident kernels (a sample's row in one
 *   wave's registers, every parameter in LDS, all layers fused); anything else takes the generic two-pass kernels (any D): the closed
 *   form of the recurrence -- L dot products per sample in one pass over its row, then y = c_L x0 + sum_t b_t column by column.
 */
int fil_dcn_fwd(const float* x, const float* w, const float* b, float* y, float* s, int B, int D, int L, void* stream);
size_t fil_dcn_bwd_workspace_bytes(int B, int D, int L);
int fil_dcn_bwd(const float* x, const float* w, const float* b, const float* s, const float* g, float* dx, float* dw,
                float* db, int B, int D, int L, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A3  xDeepFM CIN (north star) -- replaces CIN.call, interactive_layer.py:310-327
 *     (BatchMatMul outer product, 2 transposes, Conv1D 1x1, reduce_sum pooling, Concat, Dense(1)).
 *   x [B,F,K]; W[l] [H_{l-1}*F, H_l] with channel c = h*F+f (H_0 = F); bias[l] [H_l];
 *   dense_w [L*K], dense_b [1] (ignored when output_dim != 1).
 *   fwd outputs: out [B] (output_dim==1; may be NULL otherwise), pooled [B, L*K] (always written),
 *                saved = opaque buffer of fil_cin_saved_bytes bytes that bwd needs (internally: x transposed to
 *                [B*K][F], the feature maps of the layers BELOW the top two as [B*K][128*ceil(H_l/128)], and what the
 *                mode's form of the top two layers keeps: their maps, or the fused tail's [B*K][F+1 columns] and operand
 *                copies, or the quadratic tail's R [B*K][128], T and packed operands; the last layer's map is never
 *                materialised).  Forward and backward must be called with the same shape and mode bits, and fil_cin_bwd must
 *                be given the dense_w its forward was given (as `pooled` and `saved` are that forward's: with output_dim == 1 the
 *                merged quadratic tail keeps the dense_w-weighted gradient of x^1 in R's place).
 *   bwd: g = dL/dout [B] (output_dim==1) or dL/dpooled [B,L*K];
 *        writes dx [B,F,K], dW[l], dbias[l], ddense_w [L*K], ddense_b [1] (dense grads only if output_dim==1).
 *   mode: 0 = fp32 MFMA (v_mfma_f32_32x32x2_f32 / 16x16x4_f32, exact fp32 products) with the last layer contracted against
 *             wsum_L[c] = sum_n W_L[c,n] (its feature map is only ever sum-pooled, so this is the same function at 1/H_L of
 *             the flops) and, for L >= 3, the layer below it contracted against [1 | wsum_L] (its map is only ever sum-pooled
 *             or fed to the last layer: F+1 observable columns instead of H_{L-1}; the "fused tail", csrc/cin_tail.h);
 *         1 = fp32 MFMA with every layer through the general GEMM kernels (validation / comparison).
 *         + FIL_CIN_BF16X3 (2; ABI 214): the LABELLED reduced-operand mode ("bf16 operands + fp32 accumulate").  The three
 *           GEMM launches of the merged quadratic tail run on split-bf16 operands (csrc/cin_qsplit.h): every fp32 operand as three bf16
 *           pieces (an exact cut), every product as six v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- the fp32-equivalent chain
 *           a1b1 + a1b2 + a2b1 + a2b2 + a1b3 + a3b1 (dropped terms < 2^-24 relative) on the bf16 matrix pipe.  Holds the parity bars
 *           of mode 0 (tests run both side by side); not bit-identical to it (other summation order), and an infinite input gives
 *           NaN where the exact chain gives inf.  Selects something only where those kernels exist (three layers on the merged
 *           quadratic tail, F in the kernels' menu, H_1 <= 128): elsewhere the call runs the exact kernels.  Never the default;
 *           bench.py reports it beside the exact-fp32 headline, not as it.  (Bit 2 of ABI <= 209 was the same idea on the round-2
 *           layer structure; ABI 210-213 answered it with FIL_ERR_UNSUPPORTED.)
 *         + FIL_CIN_X_TRANSPOSED (16), forward and backward alike: `x` is given transposed, [B*K][F] row-major (x_t[(b*K+k)*F+f]
 *           = x[b,f,k], as written by fil_embed_gather_xt): no input transpose, saved's own copy of it stays unused.  dx is
 *           still returned as [B,F,K].
 *         + FIL_CIN_NOTAIL (32): mode 0 without the fused tail (last layer through wsum_L only: the round-2 path);
 *           FIL_CIN_TAIL_ALWAYS (64): the fused tail whenever it is defined (L >= 3, F <= 62), also where it saves nothing
 *           (by default it is used when F+2 columns padded to 16 are at most 3/4 of H_{L-1}); both exist for tests / comparison.
 *         + FIL_CIN_NOQTAIL (256): for THREE layers (and F + 2 <= 64, H_1 <= 128, 3F + 1 <= the widest feature-map row) mode 0 goes one
 *           step further than the fused tail: pool_L = sum_h x^1[h] (x^T T_h x) + <x, c> + const is a quadratic form in x for every
 *           feature map h of the FIRST layer, so the top two layers run as a product over UNORDERED field pairs with the first layer's
 *           pair-symmetric GEMM kernels -- F(F+1)/2 x H_1 products per row, half of the fused tail's, no column padding
 *           (csrc/cin_qtail.h).  Used above 16,384 rows (B*K; smaller batches are launch-latency bound and keep the fused tail,
 *           FIL_CIN_TAIL_ALWAYS lifts that rule).  This bit keeps three-layer nets on the F+1-column fused tail (tests / comparison).
 *         + FIL_CIN_NOQMERGE (512): the quadratic tail normally runs THREE GEMM launches (csrc/cin_qmerge.h): the forward
 *           [x^1 | R] = pairs(x) [W_1 | T] with 256 output columns and all three sum-pools in its epilogue, the weight gradients
 *           pairs(x)^T [G^1 | dP_L x^1] with 256 output columns, and the data gradients as two passes of one launch over one dX image.
 *           This bit keeps round 3's two launches per direction (tests / comparison).  Same function up to summation order.
 *         + FIL_CIN_NOKSPLIT (128): small batches (B*K <= 16,384 rows) give each block of 32 rows to the FOUR waves of a workgroup,
 *           which split the reduction between them (strong-scaling shards: without it the row-parallel kernels stop getting faster
 *           below one row block per SIMD); this bit keeps one wave per row block.  Same function up to summation order.
 *         + FIL_CIN_MB2 (4) / FIL_CIN_NOSYM (8): per-call launch-shape overrides (64-row waves in the row-parallel kernels,
 *             i.e. the launch configuration large batches get by themselves; symmetric first-layer kernels off).  Same
 *             function up to summation order; they exist so that tests can reach every instantiation at small sizes.
 *   grad_ready_events (bwd; may be NULL): L+1 hipEvent_t handles (entries may be NULL).  [l] is recorded on `stream` once
 *       dW[l] and dbias[l] are final, [L] once the dense head's gradients are -- from the top layer down, each before the
 *       data-gradient kernel of its layer starts -- so a data-parallel caller can start the all-reduce of a layer's
 *       gradients on another stream while the rest of the backward is still running.
 *       fil_cin_grad_ready_points(.., mode, point) tells WHERE in the backward each slot is recorded: point[l] (l = 0..L) = ordinal of
 *       the recording point, 0 first; slots with the same ordinal are recorded together (fused tail: the two top layers), so a
 *       caller reduces them with ONE collective.  Returns the number of distinct points, or a (negative) error code.
 *   Limits: F <= 64, H_l <= 256, L <= 8, B*K <= 2^28.
 */
size_t fil_cin_saved_bytes(int B, int F, int K, int L, const int* H);
size_t fil_cin_fwd_workspace_bytes(int B, int F, int K, int L, const int* H);
size_t fil_cin_bwd_workspace_bytes(int B, int F, int K, int L, const int* H);
int fil_cin_grad_ready_points(int B, int F, int K, int L, const int* H, int mode, int* point);
int fil_cin_fwd(const float* x, const float* const* W, const float* const* bias, const float* dense_w,
                const float* dense_b, float* out, float* pooled, float* saved, int B, int F, int K, int L,
                const int* H, int output_dim, int mode, void* workspace, size_t workspace_bytes, void* stream);
int fil_cin_bwd(const float* x, const float* const* W, const float* const* bias, const float* dense_w,
                const float* pooled, const float* saved, const float* g, float* dx, float* const* dW,
                float* const* dbias, float* ddense_w, float* ddense_b, int B, int F, int K, int L, const int* H,
                int output_dim, int mode, void* const* grad_ready_events, void* workspace, size_t workspace_bytes,
                void* stream);
/* fil_cin_fwd_p / fil_cin_bwd_p (ABI 216): fil_cin_fwd / fil_cin_bwd with an operand precision beside `mode`.
 *   precision FIL_CIN_PREC_DEFAULT (0): exactly what `mode` selects (the same call as fil_cin_fwd / fil_cin_bwd).
 *   precision FIL_CIN_PREC_BF16 (1): the LABELLED bf16 training mode.  Wherever the merged quadratic tail runs (the places
 *       FIL_CIN_BF16X3 can run: three layers, H_1 == 128 column chunk, F in the split kernels' menu, above 16,384 rows unless
 *       FIL_CIN_TAIL_ALWAYS) its three GEMM launches round every operand ONCE to bf16 (nearest even) and take ONE
 *       v_mfma_f32_32x32x16_bf16 per product with fp32 accumulation (csrc/cin_qsplit.h, NP = 1); everything else stays exact fp32.
 *       Error ~1e-3 relative (one bf16 rounding per operand over an F(F+1)/2-long reduction): a mode of its own, never the default.
 *       Elsewhere the call runs the exact kernels; fil_cin_precision_used says which.  (At the few F where no one-plane dZ kernel
 *       exists -- those the two-pass BF16X3 dZ kernel refuses -- the data gradient runs exact.)
 *       Combined with mode bit FIL_CIN_BF16X3: FIL_ERR_ARG.  Any other precision code: FIL_ERR_ARG.
 *   saved / workspace sizes: fil_cin_saved_bytes / fil_cin_*_workspace_bytes cover every precision.  Allocates nothing, never
 *   synchronises, graph-capturable, bit-identical for identical inputs, like the exact path.
 *   grad_ready_events: recorded at the same points as FIL_CIN_BF16X3's (fil_cin_grad_ready_points(.., mode, ..) holds for either
 *   precision: they do not depend on it).
 * fil_cin_precision_used: the precision a call with these arguments actually runs (FIL_CIN_PREC_BF16 or FIL_CIN_PREC_DEFAULT; B = 0:
 *   DEFAULT, nothing runs), or a (negative) error code for arguments the _p entry points refuse. */
enum fil_cin_precision { FIL_CIN_PREC_DEFAULT = 0, FIL_CIN_PREC_BF16 = 1 };
int fil_cin_precision_used(int B, int F, int K, int L, const int* H, int mode, int precision);
/* fil_cin_shortdx_used: 1 where a backward with these arguments computes the shortcut's data gradient with cin_shortcut_dx_kernel (merged
 *   quadratic tail whose forward saved the g-free gradient of x1, exact kernels; FIL_CIN_SHORTDX=0 in the environment turns it off), 0 where
 *   cin_last_bwd2_kernel or another path does (B = 0: 0, nothing runs), or a (negative) error code for arguments fil_cin_bwd_p refuses.
 *   For tests and tools.  Entry point added only: the ABI version stays. */
int fil_cin_shortdx_used(int B, int F, int K, int L, const int* H, int output_dim, int mode, int precision);
int fil_cin_fwd_p(const float* x, const float* const* W, const float* const* bias, const float* dense_w,
                  const float* dense_b, float* out, float* pooled, float* saved, int B, int F, int K, int L,
                  const int* H, int output_dim, int mode, int precision, void* workspace, size_t workspace_bytes, void* stream);
int fil_cin_bwd_p(const float* x, const float* const* W, const float* const* bias, const float* dense_w,
                  const float* pooled, const float* saved, const float* g, float* dx, float* const* dW,
                  float* const* dbias, float* ddense_w, float* ddense_b, int B, int F, int K, int L, const int* H,
                  int output_dim, int mode, int precision, void* const* grad_ready_events, void* workspace, size_t workspace_bytes,
                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * A4  AutoInt interacting layer -- replaces MultHeadAttentionLayer.call + ProductAttentionLayer.call
 *     (behavior_layer/behavior_layer.py:292-311,356-377) and DnnLayer's Add + ReLU
 *     (core_layer/core_layer.py:204-216), fused; the [H,B,F,F] score tensor is never materialised.
 *   x [B,F,K]; Wq, Wk, Wr [K,H,A] (V is projected with Wk, as the reference does; Wr may be NULL = use_res off);
 *   gamma, beta [A] (NULL = use_ln off); eps = 1e-3 for Keras parity; scale = 1/sqrt(A) (use_scale) or 1.
 *   fuse_relu != 0 (the DnnLayer(res_unit=1, other_dense=[layer]) wrapper AutoInt uses):
 *       y [H,B,F,A] = relu(x Wr + LN(sigmoid(scale * q k^T) k)),  res_out ignored.
 *   fuse_relu == 0 (MultHeadAttentionLayer.call as a stand-alone layer, which returns [atten_v, res]):
 *       y = LN(sigmoid(scale * q k^T) k),  res_out [H,B,F,A] = x Wr (may be NULL).
 *   bwd: dy [H,B,F,A] (and, when fuse_relu == 0 and Wr != NULL, dres_in [H,B,F,A] = gradient of res_out)
 *        -> dx [B,F,K], dWq, dWk, dWr [K,H,A], dgamma, dbeta [A].
 *   av_out [H,B,F,A] + rstd_out [H,B,F] (fwd, optional, both or neither; used with gamma): the LayerNorm input saved for the
 *       backward, NORMALISED -- (av - mean) / sqrt(var + eps) -- with the rows' 1 / sqrt(var + eps) beside it, so that the
 *       backward's LayerNorm gradient does not derive the statistics of every row again (av_saved + rstd_saved).  The fused
 *       ReLU mask is y > 0: pass the forward's y back as y_saved.  If any of them is NULL the backward first re-runs the
 *       forward into its workspace (fil_attn_bwd_workspace_bytes(.., have_saved = 0)); same gradients bit for bit.
 *   x_chunk: 0 = x (and dx) are [B,F,K].  c > 0 = head-major [K/c][B][F][c], i.e. the [H',B,F,A'] output of a previous
 *       interacting layer read in place as its head-concat [B,F,H'*A'] (ESULayer's convention, behavior_layer.py:973):
 *       a stack of interacting layers (BASELINE config 5: 3 layers) needs no transposes, and dx IS the dy of the layer below.
 *   The backward is one kernel (one pass over the F x F scores): per-workgroup partial sums of dW* / dgamma / dbeta are
 *   reduced afterwards in a fixed order (bit-identical repeats).
 *   precision: FIL_PREC_F32 = every matrix product on the exact fp32 MFMA (1e-5 parity with the reference);
 *       FIL_PREC_F16_MFMA = BASELINE config 5 ("fp16 MFMA QK^T V"): the operands of every matrix product (projections,
 *       scores, weighted sums and their gradients) are rounded to fp16 and multiplied on v_mfma_f32_16x16x16_f16 with
 *       fp32 accumulation; sigmoid, LayerNorm, residual, ReLU, all tensors in memory and all reductions stay fp32.
 *       Parity of that mode is ~1e-3 (tests state 5e-3 / 2e-2); values beyond the fp16 range (65504) overflow.
 *   Limits: K <= 64, A <= 16, H <= 8, F <= 512, AND the kernel's dynamic LDS footprint <= 163,328 bytes (the CU's 160 KiB less the
 *       kernels' static arrays, rounded to the allocation granule).  The footprint grows with H and F (f16: also with K), and the
 *       backward's is the larger one: in FIL_PREC_F32 with H = 8 the forward runs up to F = 240 and the backward up to F = 128; with
 *       H = 4 up to F = 496 / 384.  FIL_PREC_F16_MFMA, K = 64: the backward runs up to F = 208 at H = 8 and F = 480 at H = 4.  A shape
 *       past the limit returns FIL_ERR_UNSUPPORTED before anything is launched or written.
 *   fil_attn_plan: which instantiation fil_attn_fwd / fil_attn_bwd launch for a shape, from the same host function the launchers
 *       use (no GPU call, no allocation; the environment knobs FIL_ATTN_KREG / FIL_ATTN_WPH / FIL_ATTN_DX_LDS apply as they do to the
 *       launch).  plan[10] = {fwd_ok, fwd_kreg (k fragments in registers), fwd_a16 (A == 16 form), fwd_lds_bytes,
 *       bwd_ok, bwd_nb (key-block menu entry 4 / 8 / 13 / 32), bwd_wph (waves per head), bwd_dx_lds (dx image in LDS),
 *       bwd_a16, bwd_lds_bytes}; *_ok = 0 where the LDS footprint (then of the smallest configuration) exceeds the limit.  Returns
 *       FIL_OK, or the argument / menu error the launch would give.  Entry point added only: the ABI version stays.
 */
enum fil_cin_mode_bits { FIL_CIN_GENERAL = 1, FIL_CIN_BF16X3 = 2, FIL_CIN_MB2 = 4, FIL_CIN_NOSYM = 8, FIL_CIN_X_TRANSPOSED = 16,
                         FIL_CIN_NOTAIL = 32, FIL_CIN_TAIL_ALWAYS = 64, FIL_CIN_NOKSPLIT = 128, FIL_CIN_NOQTAIL = 256, FIL_CIN_NOQMERGE = 512 };
enum fil_precision { FIL_PREC_F32 = 0, FIL_PREC_F16_MFMA = 1 };
int fil_attn_plan(int F, int K, int H, int A, int precision, int* plan /* [10] */);
size_t fil_attn_fwd_workspace_bytes(int B, int F, int K, int H, int A);
size_t fil_attn_bwd_workspace_bytes(int B, int F, int K, int H, int A, int have_saved);
int fil_attn_fwd(const float* x, const float* Wq, const float* Wk, const float* Wr, const float* gamma,
                 const float* beta, float* y, float* res_out, float* av_out, float* rstd_out, int B, int F, int K, int H,
                 int A, float scale, float eps, int fuse_relu, int precision, int x_chunk, void* workspace,
                 size_t workspace_bytes, void* stream);
int fil_attn_bwd(const float* x, const float* Wq, const float* Wk, const float* Wr, const float* gamma,
                 const float* beta, const float* dy, const float* dres_in, const float* y_saved, const float* av_saved,
                 const float* rstd_saved, float* dx, float* dWq, float* dWk, float* dWr, float* dgamma, float* dbeta, int B, int F, int K, int H,
                 int A, float scale, float eps, int fuse_relu, int precision, int x_chunk, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ProductAttentionLayer.call([q, k, v], mask) as a stand-alone layer (behavior_layer.py:292-311): separate q / k / v, any
 * mask.  (AutoInt's own path is fil_attn_*: projections, attention, LayerNorm and residual fused.)
 *   q [N,Fq,A], k [N,Fk,A], v [N,Fk,Av] -> out [N,Fq,Av] = sigmoid(scale * q k^T + mask * (-1e5)) v     (fp32 MFMA)
 *   N = the flattened leading axes (e.g. heads x batch); scale = 1/sqrt(A) for use_scale, else 1.
 *   mask (may be NULL) [mask_period, Fq, Fk], item n uses mask[n % mask_period]: the additive mask of mask_mod == 2
 *   (:303-306).  mask_mod == 1 (:300-302, the scores right-multiplied by a mask matrix M) is (q k^T) M = q (M^T k)^T:
 *   the caller passes k' = M^T k and no mask.
 *   bwd: dout [N,Fq,Av] -> dq, dk, dv.  Limits: A, Av <= 64; LDS footprint 80*(ceil(A/16)+ceil(Av/16))*max(Fq,Fk) bytes <= 160 KiB.
 */
int fil_pattn_fwd(const float* q, const float* k, const float* v, const float* mask, float* out, int N, int Fq, int Fk, int A,
                  int Av, float scale, int mask_period, void* stream);
int fil_pattn_bwd(const float* q, const float* k, const float* v, const float* mask, const float* dout, float* dq, float* dk,
                  float* dv, int N, int Fq, int Fk, int A, int Av, float scale, int mask_period, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N1  SparseEmbed field-index work -- replaces the F Embedding lookups of SparseEmbed.call,
 *     interactive_layer.py:225-242, emitting the packed [B,F,K] layout directly (bit-exact row copies).
 *   table: all F tables concatenated [sum_f V_f, K]; offsets [F] = first row of field f (int64);
 *   sizes [F] = V_f (int64; NULL = ids are trusted); idx [B,F] (int64, per-field local ids).  out [B,F,K].
 *   An id outside [0, V_f) gives a ZERO output row (Keras' Embedding on a GPU) and is counted in *oob_count (device int,
 *   may be NULL; the caller zeroes it) -- never a read of the neighbouring field's table; its gradient is dropped.
 *   Gradient, deterministic (default in the Python layer):
 *     fil_embed_row_ids      row_ids[b*F+f] = offsets[f] + idx[b,f], or -1 for out-of-range ids and frozen fields
 *                            (frozen [F] bytes, may be NULL: sparseFea.is_trainable = False);
 *     (the caller sorts row_ids stably -> perm, and takes the run starts of the sorted ids -> rows_out [U], starts [U+1])
 *     fil_embed_segment_sum  values[u,:] = sum_{j in [starts[u], starts[u+1])} g[perm[j], :] in sorted order with a fixed
 *                            lane tree; rows_out[u] < 0 is skipped; dtable != NULL additionally stores the row sums into
 *                            dtable[rows_out[u], :] (unique rows: plain stores).  values / dtable: either may be NULL.
 *   fil_embed_scatter_add: the fp32-atomic alternative, dtable[offsets[f]+idx[b,f], :] += g[b,f,:] (dtable pre-zeroed;
 *                            the order of additions into a row hit several times is NOT fixed).
 */
int fil_embed_gather(const float* table, const int64_t* offsets, const int64_t* sizes, const int64_t* idx, float* out,
                     int* oob_count, int B, int F, int K, void* stream);
/* the same with the block's storage type chosen (out_dtype FIL_F32 / FIL_BF16: the rows leave rounded to bf16 -- what a bf16 model
 * would otherwise do to the block in a cast launch of its own; the table stays fp32) */
int fil_embed_gather_dt(const float* table, const int64_t* offsets, const int64_t* sizes, const int64_t* idx, void* out,
                        int* oob_count, int B, int F, int K, int out_dtype, void* stream);
/* the same gather emitting BOTH the packed block out [B,F,K] and its transposed rows out_t [B*K][F] (out_t[(b*K+k)*F+f] =
 * out[b,f,k]) -- the layout the CIN kernels read: hand out_t to fil_cin_fwd / fil_cin_bwd as `x` with FIL_CIN_X_TRANSPOSED and
 * the consumer's input transpose is gone (gather fused into the consumer). */
int fil_embed_gather_xt(const float* table, const int64_t* offsets, const int64_t* sizes, const int64_t* idx, float* out,
                        float* out_t, int* oob_count, int B, int F, int K, void* stream);
int fil_embed_scatter_add(const int64_t* offsets, const int64_t* sizes, const int64_t* idx, const float* g, float* dtable,
                          int B, int F, int K, void* stream);
int fil_embed_row_ids(const int64_t* offsets, const int64_t* sizes, const unsigned char* frozen, const int64_t* idx,
                      int64_t* row_ids, int B, int F, void* stream);
int fil_embed_segment_sum(const float* g, const int64_t* perm, const int64_t* starts, const int64_t* rows_out, float* values,
                          float* dtable, long U, int K, void* stream);
/* row ids AND their sort in one launch, for fil_embed_run_sum: field f's B entries sorted by (row id, position) -- a stable sort
 * within the field -- land in sorted_ids / perm [f*B, (f+1)*B) (perm[j] = b*F + f); skipped entries (-1) lead each field's segment.
 * Equal row ids are adjacent and in position order, which is all the run sum needs (rows of different fields cannot be equal), but
 * the list as a whole is sorted only if offsets[] ascends.  B <= 8192 (one workgroup sorts a field in LDS), ids < 2^32 - 1.
 * max_vocab: an upper bound of every field's vocabulary (the concatenated table's row count will do), 0 = unknown: when
 * (max_vocab + 1) * 2^ceil(log2 B) fits 32 bits the sort runs on 32-bit composites (half the LDS traffic). */
int fil_embed_sort_fields(const int64_t* offsets, const int64_t* sizes, const unsigned char* frozen, const int64_t* idx,
                          int64_t* sorted_ids, int64_t* perm, int B, int F, int64_t max_vocab, void* stream);
/* the same sums without any data-dependent size (HIP-graph capturable): sorted_ids [R] = the stably sorted row ids, perm [R]
 * the sorting permutation; the run of every distinct id >= 0 is summed in sorted order into the (pre-zeroed) dense dtable. */
int fil_embed_run_sum(const float* g, const int64_t* perm, const int64_t* sorted_ids, float* dtable, long R, int K, void* stream);
/* the same for a gradient block stored as g_dtype (FIL_F32 / FIL_BF16: converted on load, summed in fp32 into the fp32 dtable) */
int fil_embed_run_sum_dt(const void* g, const int64_t* perm, const int64_t* sorted_ids, float* dtable, long R, int K, int g_dtype,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * N3  Pooled multi-valued sparse fields -- tf.feature_column.embedding_column(combiner=...) / tf.nn.safe_embedding_lookup_sparse
 *     without weights, or Embedding(mask_zero=True) + a masked average (the reference's sparseFea.mask_zero / input_length,
 *     InputFeature.seq_info / seq_inputs).  Entry points added only: the ABI version stays.
 *   table, offsets, sizes: as N1.  idx [B,F,T] int64: T slots per sample and field.  A slot is PADDING iff id == pad_id
 *   (FIL_BAG_NO_PAD: no id is padding; 0 = Keras' mask_zero, row 0 of every field is then never read), OUT OF RANGE iff it is not
 *   padding and id < 0 or id >= sizes[f] (sizes NULL = ids are trusted): it contributes nothing and is counted in *oob_count (device
 *   int, may be NULL; the caller zeroes it; padding is not counted).  Every other slot is LIVE; n(b,f) = their number (an id repeated
 *   in a bag counts once per occurrence; padding may sit anywhere in the row).
 *   fil_embed_bag_fwd: out[b,f,:] = (sum over the live t, ascending, of table[offsets[f] + idx[b,f,t], :]) / d, fp32 additions in that
 *     order, then ONE correctly rounded division: FIL_BAG_SUM none, FIL_BAG_MEAN d = (float)n, FIL_BAG_SQRTN d = sqrtf((float)n);
 *     n = 0 gives a zero row.  No reciprocal, no fused multiply-add: bit-equal to the sequential fp32 restatement.  count [B,F]
 *     (int32) receives n.  A padding or out-of-range slot issues no table read.  One launch; ceil(K/4) lanes per bag, 16-byte row
 *     accesses when K % 4 == 0, at most FIL_BAG_MAX_BLOCKS workgroups of 256 threads walking the bags in a grid-stride loop.
 *   Gradient (deterministic, no atomics, no data-dependent sizes):
 *     fil_embed_bag_row_ids   row_ids[(b F + f) T + t] = offsets[f] + idx[b,f,t], or -1 for a padding / out-of-range slot and for
 *                             a frozen field (frozen [F] bytes, may be NULL);
 *     (the caller sorts row_ids stably -> sorted_ids [R], slot_perm [R], R = B F T)
 *     fil_embed_bag_bwd_prep  gs[b,f,:] = g[b,f,:] / d with the forward's d (count = the forward's; n = 0: zeros) and
 *                             perm[j] = slot_perm[j] / T = the bag b F + f of sorted slot j (perm may be slot_perm itself), in one
 *                             launch.  FIL_BAG_SUM: gs must be NULL (g and count are not read): the incoming rows are used as they are.
 *     (g = gs [B F][K] fp32, perm, sorted_ids, R, F) is then a record of exactly the form fil_embed_run_sum_dt,
 *     fil_embed_segment_sum, fil_embed_runs_compact and every fil_embed_*_runs / _merged optimizer entry point take: they read the
 *     gradient row as g[perm[j]] and the field as perm[j] % F, and b F + f satisfies both.
 *   B == 0 returns FIL_OK before any pointer is looked at; K <= 256 (the run sums' limit) and B F T < 2^31 (FIL_ERR_UNSUPPORTED).
 */
#define FIL_BAG_SUM 0
#define FIL_BAG_MEAN 1
#define FIL_BAG_SQRTN 2
#define FIL_BAG_NO_PAD INT64_MIN
#define FIL_BAG_MAX_BLOCKS 2048
int fil_embed_bag_fwd(const float* table, const int64_t* offsets, const int64_t* sizes, const int64_t* idx, int64_t pad_id, float* out,
                      int* count, int* oob_count, int B, int F, int T, int K, int combiner, void* stream);
int fil_embed_bag_row_ids(const int64_t* offsets, const int64_t* sizes, const unsigned char* frozen, const int64_t* idx,
                          int64_t pad_id, int64_t* row_ids, int B, int F, int T, void* stream);
int fil_embed_bag_bwd_prep(const float* g, const int* count, const int64_t* slot_perm, float* gs, int64_t* perm, int B, int F, int T,
                           int K, int combiner, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N3  AFM pair-attention pooling with the softmax over the PAIRS (extension: the reference's AttentionBaseLayer,
 *     interactive_layer.py:357-364, normalises over a size-1 axis, so all of its weights are 1; that stays the layers' default and is
 *     not computed here).  All tensors fp32.  Entry points added only: the ABI version stays.
 *   emb [B,F,K]; W [K,A], b [A], h [A] (single_score_w, single_score_b, single_mlp_kernel [A,1]).  Pairs p = (i, j), i < j, in
 *   itertools.combinations order, P = F(F-1)/2; x_p = e_i * e_j, u_p = x_p W + b;
 *     flags bit 0 clear (reference op order): s_p = relu(u_p . h);   set (FIL_AFM_HIDDEN_RELU, the paper's form): s_p = relu(u_p) . h;
 *     a = softmax_p(s) with the maximum subtracted;  pooled[b,:] = sum_p a_p x_p   [B,K].
 *   fil_afm_fwd: pooled, and stats [B,2] = (maximum score, softmax denominator) for the backward (opaque to the caller).
 *   fil_afm_bwd: g = d pooled [B,K] -> demb [B,F,K], dW [K,A], db [A], dh [A]; the scores are recomputed (same code, same bits).
 *     ds_p = a_p (g.x_p - g.pooled); du_p through the ReLU of the chosen form (derivative 0 at 0); dW = sum x_p^T du_p, db = sum du_p,
 *     dh = sum dt_p u_p (reference form) or sum ds_p relu(u_p) (paper form); dx_p = a_p g + W du_p; de_i += dx_p * e_j, de_j += dx_p * e_i.
 *     demb may be NULL, and dW / db / dh may each be NULL (all three NULL: no parameter pass, no workspace; everything NULL: FIL_ERR_ARG).
 *     The parameter gradients leave the main launch as one partial per workgroup in `workspace` (fil_afm_bwd_workspace_bytes; every
 *     byte that is read was written by that launch) and a second small launch adds the partials in a fixed order.
 *   Nothing of size B P touches global memory in either direction.  No atomics; every sum has a fixed order for a given shape: the
 *   same inputs give the same bits on every call.  A wave owns whole samples out of an LDS-resident [F,K] slab; W, b, h and the pair
 *   table are staged once per workgroup.  F = 2 (one pair): pooled == e_0 * e_1 and demb == g * e_other bit for bit, dW = db = dh = 0.
 *   Menu: 2 <= F <= 64, K % 4 == 0, K <= 64, A <= 16 (FIL_ERR_UNSUPPORTED otherwise, the limit in the message); the dynamic LDS stays
 *   within 163,328 bytes over the whole menu (the workgroup shrinks from 4 waves to 1 as the footprint grows).
 *   B == 0 returns FIL_OK before any pointer is looked at.  A workspace smaller than needed: FIL_ERR_ARG, the needed size in the message.
 *   fil_afm_plan: the launchers' own arithmetic (no GPU call): plan[8] = {fwd_ok, bwd_ok, samples per workgroup tile (= waves per
 *     workgroup), grid, grid cap, parameter-gradient partials (= grid), forward LDS bytes, backward LDS bytes}.  Returns FIL_OK, or
 *     the argument / menu error the launch would give.
 */
#define FIL_AFM_HIDDEN_RELU 1
int fil_afm_plan(int B, int F, int K, int A, int* plan /* [8] */);
int fil_afm_fwd(const float* emb, const float* W, const float* b, const float* h, float* pooled, float* stats, int B, int F, int K,
                int A, int flags, void* stream);
size_t fil_afm_bwd_workspace_bytes(int B, int F, int K, int A);
int fil_afm_bwd(const float* emb, const float* W, const float* b, const float* h, const float* pooled, const float* stats,
                const float* g, float* demb, float* dW, float* db, float* dh, void* workspace, size_t workspace_bytes, int B, int F,
                int K, int A, int flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N3  DIN attention pooling over a behaviour sequence (extension: the Deep Interest Network paper's activation unit; the
 *     reference's AttentionUnitLayer / ActivationUnitLayer are not restated -- their source was not available).  All tensors fp32
 *     except mask.  Entry points added only: the ABI version stays.
 *   q [B,K] the candidate; keys [B,T,K] the history; mask [B,T] uint8, non-zero = live, NULL = all live (live slots may sit anywhere);
 *   W1 [4K,H1], b1 [H1], alpha1 [H1], W2 [H1,H2], b2 [H2], alpha2 [H2], w3 [H2], b3 [1].
 *     x_t = [q, k_t, q - k_t, q * k_t];  h1 = act(x_t W1 + b1);  h2 = act(h1 W2 + b2);  s_t = h2 . w3 + b3  (not scaled by sqrt(K));
 *     flags bit 0 clear (raw, the paper): a_t = s_t for live t, 0 for masked t;  set (FIL_DIN_SOFTMAX): a = softmax of s over the LIVE t;
 *     out[b,:] = sum_t a_t k_t  [B,K]  (a sample with no live slot: the zero row).
 *     act = PReLU, u > 0 ? u : alpha u, a slope per unit (derivative at 0: alpha); flags bit 1 (FIL_DIN_SIGMOID): the logistic
 *     sigmoid, alpha1 / alpha2 are then ignored and may be NULL.  ReLU = PReLU with alpha = 0 and no gradient asked for alpha.
 *   fil_din_fwd: out, and stats [B, T+2] = (the T scores, maximum live score, softmax denominator) for the backward (opaque to the
 *     caller).
 *   fil_din_bwd: g = d out [B,K] -> dq [B,K], dkeys [B,T,K], dW1, db1, dalpha1, dW2, db2, dalpha2, dw3, db3; the hidden layers are
 *     recomputed (same code, same bits).  ds_t = a_t (g.k_t - g.out) (softmax) or g.k_t (raw), 0 at masked t, with g.out summed as
 *     sum_t a_t (g.k_t) from the saved scores (`out` itself is not read); dkeys is exactly 0 at masked slots.
 *     Each of the ten outputs may be NULL and is then not computed (all eight parameter gradients NULL: no parameter pass, no
 *     workspace; everything NULL: FIL_ERR_ARG).  With FIL_DIN_SIGMOID dalpha1 / dalpha2 receive zeros.  The parameter gradients leave
 *     the main launch as one partial per workgroup in `workspace` (fil_din_bwd_workspace_bytes; every byte that is read was written
 *     by that launch) and a second small launch adds the partials in a fixed order.
 *   Nothing of size B T n, n >= K, other than keys and dkeys touches global memory.  No atomics; every sum has a fixed order for a
 *   given shape: the same inputs give the same bits on every call.  A masked slot's key is never read.  Softmax with ONE live slot:
 *   its weight is exactly 1, out is that key bit for bit, ds is exactly 0 (g.out is then that slot's g.k_t, the same bits).
 *   Menu: K % 4 == 0, K <= 64, T <= 256, H1 <= 128, H2 <= 64, 4 K H1 + H1 H2 <= 16384 (FIL_ERR_UNSUPPORTED otherwise, the limit in
 *   the message); the dynamic LDS stays within 163,328 bytes over the whole menu (a workgroup holds 4 samples down to 1 as the
 *   footprint grows; a shape that still did not fit would return FIL_ERR_UNSUPPORTED with the byte count).
 *   B == 0 returns FIL_OK before any pointer is looked at.  A workspace smaller than needed: FIL_ERR_ARG, the needed size in the message.
 *   fil_din_plan: the launchers' own arithmetic (no GPU call): plan[8] = {fwd_ok, bwd_ok, samples per workgroup tile, grid, grid cap,
 *     parameter-gradient partials (= grid), forward LDS bytes, backward LDS bytes}.  Returns FIL_OK, or the argument / menu error the
 *     launch would give.
 */
#define FIL_DIN_SOFTMAX 1
#define FIL_DIN_SIGMOID 2
int fil_din_plan(int B, int T, int K, int H1, int H2, int* plan /* [8] */);
int fil_din_fwd(const float* q, const float* keys, const unsigned char* mask, const float* W1, const float* b1, const float* alpha1,
                const float* W2, const float* b2, const float* alpha2, const float* w3, const float* b3, float* out, float* stats, int B,
                int T, int K, int H1, int H2, int flags, void* stream);
size_t fil_din_bwd_workspace_bytes(int B, int T, int K, int H1, int H2);
int fil_din_bwd(const float* q, const float* keys, const unsigned char* mask, const float* W1, const float* b1, const float* alpha1,
                const float* W2, const float* b2, const float* alpha2, const float* w3, const float* b3, const float* out,
                const float* stats, const float* g, float* dq, float* dkeys, float* dW1, float* db1, float* dalpha1, float* dW2,
                float* db2, float* dalpha2, float* dw3, float* db3, void* workspace, size_t workspace_bytes, int B, int T, int K, int H1,
                int H2, int flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N3  GRU / AUGRU / AGRU over a behaviour sequence (extension: the interest extraction and interest evolution layers of the Deep
 *     Interest Evolution Network paper; the GRU is TF 2 Keras' GRU with its defaults -- reset_after=True, sigmoid / tanh -- and the
 *     attention-gated variants are the paper's eq. 15-16; the reference's rnn_demo.py is not restated, its source was not
 *     available).  All tensors fp32 except mask.  Entry points added only: the ABI version stays.
 *   x [B,T,K] the sequence; a [B,T] the attention scores (NULL in FIL_GRU_GRU mode, required otherwise); mask [B,T] uint8, non-zero =
 *   live, NULL = all live (live slots may sit anywhere); W [K,3H] and U [H,3H] in Keras' column order z | r | h; b [2,3H]: row 0 the
 *   input bias, row 1 the recurrent bias; hs [B,T,H] the output.  One live step, h = the previous state, h_0 = 0:
 *     xp = x_t W + b[0];  hp = h U + b[1];  z = sigmoid(xp_z + hp_z);  r = sigmoid(xp_r + hp_r);  c = tanh(xp_h + r * hp_h);
 *     u = 1 - z  (z is Keras' keep gate, u the paper's update gate);
 *     u' = u (FIL_GRU_GRU) | a_t * u (FIL_GRU_AUGRU) | a_t for every unit (FIL_GRU_AGRU: z is unused and gets no gradient);
 *     h_new = fma(u', c, (1 - u') * h) -- one expression for the three modes: GRU and AUGRU with a = 1 return the same bits, and
 *     a_t = 0 repeats the state.
 *   A masked step carries the state: hs[b,t] = h bit for bit (zeros before the first live step); its x_t and a_t are never read.
 *   fil_gru_fwd: hs, and `saved` [B,T,4,H] = (z, r, c, hp_h) of the live steps for the backward (fil_gru_saved_bytes; opaque to the
 *     caller; masked steps are left unwritten; NULL: nothing is saved, for inference).  x_t W is fused into the step: nothing else of
 *     size B T n touches global memory.
 *   fil_gru_bwd: g_hs [B,T,H] and / or g_last [B,H] (the gradient of hs[:,T-1], for return_sequences=False; either may be NULL, not
 *     both) -> dx [B,T,K], da [B,T] (not in FIL_GRU_GRU mode), dW, dU, db [2,3H].  No product is recomputed: the gates come from
 *     `saved`, the previous state from hs.  Each output may be NULL and is then not computed (dW, dU, db all NULL: no parameter pass,
 *     no workspace; everything NULL: FIL_ERR_ARG).  dx and da are exactly 0 at masked steps.  The parameter gradients leave the main
 *     launch as one partial per workgroup in `workspace` (fil_gru_bwd_workspace_bytes; every byte that is read was written by that
 *     launch) and a second small launch adds the partials in a fixed order.
 *   One launch per direction (plus the partial sum).  No atomics; every sum has a fixed order for a given shape: the same inputs give
 *   the same bits on every call.
 *   Menu: any T >= 1; K % 4 == 0, H % 4 == 0, K <= 64, H <= 64 in both directions (FIL_ERR_UNSUPPORTED otherwise, the limit in the
 *   message); the dynamic LDS stays within 163,328 bytes over the whole menu (161,024 in the backward at K = H = 64).
 *   B == 0 returns FIL_OK before any pointer is looked at.  A workspace smaller than needed: FIL_ERR_ARG, the needed size in the message.
 *   fil_gru_plan: the launchers' own arithmetic (no GPU call): plan[8] = {fwd_ok, bwd_ok, samples per workgroup tile, grid, grid cap,
 *     parameter-gradient partials (= grid), forward LDS bytes, backward LDS bytes}.  The tile grows with B (small batches take small
 *     tiles and more workgroups).  Returns FIL_OK, or the argument / menu error the launch would give.
 */
#define FIL_GRU_GRU 0
#define FIL_GRU_AUGRU 1
#define FIL_GRU_AGRU 2
int fil_gru_plan(int B, int T, int K, int H, int mode, int* plan /* [8] */);
size_t fil_gru_saved_bytes(int B, int T, int K, int H);
int fil_gru_fwd(const float* x, const float* a, const unsigned char* mask, const float* W, const float* U, const float* b, float* hs,
                float* saved, int B, int T, int K, int H, int mode, void* stream);
size_t fil_gru_bwd_workspace_bytes(int B, int T, int K, int H);
int fil_gru_bwd(const float* x, const float* a, const unsigned char* mask, const float* W, const float* U, const float* hs,
                const float* saved, const float* g_hs, const float* g_last, float* dx, float* da, float* dW, float* dU, float* db,
                void* workspace, size_t workspace_bytes, int B, int T, int K, int H, int mode, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N3  LSTM over a sequence, one direction or both in one launch (extension: TF 2 Keras' LSTM with its defaults -- sigmoid / tanh,
 *     one bias, no dropout -- and Keras' Bidirectional(LSTM), the session interest interacting layer of the Deep Session Interest
 *     Network paper; the reference's rnn_demo.py is not restated, its source was not available).  All tensors fp32 except mask.
 *     Entry points added only: the ABI version stays.
 *   dirs: FIL_LSTM_FORWARD, FIL_LSTM_REVERSE or FIL_LSTM_BIDIR; ndir = 2 for FIL_LSTM_BIDIR, else 1.
 *   x [B,T,K] the sequence; mask [B,T] uint8, non-zero = live, NULL = all live (live slots may sit anywhere); per direction W [K,4H],
 *   U [H,4H] in Keras' column order i | f | c | o and ONE bias b [4H]: W [ndir,K,4H], U [ndir,H,4H], b [ndir,4H], the forward
 *   direction first; hs [B,T,ndir*H] the output, the forward direction in the columns 0 .. H-1 and the reverse in H .. 2H-1 (the
 *   concatenation is fused).  One live step, h and c = the previous states, h_0 = c_0 = 0:
 *     z = x_t W + h U + b;  i = sigmoid(z_i);  f = sigmoid(z_f);  g = tanh(z_c);  o = sigmoid(z_o);
 *     c_new = fma(f, c, i * g);  h_new = o * tanh(c_new).
 *   A masked step carries BOTH states: hs[b,t] = h bit for bit (zeros before the first live step); its x_t is never read.
 *   The forward direction walks t = 0 .. T-1, the reverse t = T-1 .. 0 and stores the state reached after step t at position t (Keras'
 *   go_backwards with the output turned back): its last state is hs[:,0].  REVERSE on the time-reversed inputs returns FORWARD's bits,
 *   time-reversed, and one BIDIR call returns the bits of a FORWARD and a REVERSE call on the two halves of the weights.
 *   fil_lstm_fwd: hs, and `saved` [ndir,B,T,5,H] = (i, f, g, o) of the live steps and the cell c after EVERY step (c_prev of a live step
 *     is the cell carried across masked steps) for the backward (fil_lstm_saved_bytes; opaque to the caller; the gates of masked steps
 *     are left unwritten; NULL: nothing is saved, for inference).  x_t W is fused into the step.
 *   fil_lstm_bwd: g_hs [B,T,ndir*H] and / or g_last [B,ndir*H] (the gradient of the directions' last states, the forward hs[:,T-1,:H]
 *     and the reverse hs[:,0,H:], for return_sequences=False; either may be NULL, not both) -> dx [B,T,K], dW, dU, db in the shapes of
 *     W, U, b.  No product is recomputed: the gates come from `saved`, the previous h from hs; tanh(c_new) is taken again from the
 *     saved cell.  A masked step passes both state gradients through unchanged; dx is exactly 0 there (in BIDIR: the sum of two
 *     zeros).  Each output may be NULL and is then not computed, the others keep the bits of the full call (dW, dU, db all NULL: no
 *     parameter pass; all four NULL: FIL_ERR_ARG).  The parameter gradients leave the main launch as one partial per workgroup in
 *     `workspace` and a small launch per direction adds that direction's partials in a fixed order; in BIDIR the reverse direction's
 *     dx goes to the workspace as well and one more small launch adds it to dx.  The workspace (fil_lstm_bwd_workspace_bytes; every
 *     byte that is read was written by the main launch) is needed for a parameter gradient, and in BIDIR for dx.
 *   One main launch per pass, both directions of BIDIR in it (a grid dimension selects the direction; a workgroup stages only its
 *   own direction's weights).  No atomics; every sum has a fixed order for a given shape: the same inputs give the same bits on
 *   every call.
 *   Menu: any T >= 1; K % 4 == 0, H % 4 == 0, K <= 64, H <= 64, and both passes within 163,328 bytes of dynamic LDS: every such
 *   shape with H <= 56, H = 60 with K <= 52, H = 64 with K <= 40 (the backward's 4 ((K + H) 4H + (2 (K + H) + 4H) (NS + 4) + NS 4H +
 *   2 NS) bytes with NS = 16 there decide it: 159,104 at K = 64, H = 56; 188,544 at K = H = 64).  FIL_ERR_UNSUPPORTED otherwise, the
 *   needed and the allowed bytes in the message.
 *   B == 0 returns FIL_OK before any pointer is looked at.  A workspace smaller than needed: FIL_ERR_ARG, the needed size in the message.
 *   fil_lstm_plan: the launchers' own arithmetic (no GPU call): plan[8] = {fwd_ok, bwd_ok, samples per workgroup tile, workgroups per
 *     direction, their cap, parameter-gradient partials (= ndir * workgroups per direction), forward LDS bytes, backward LDS bytes}.
 *     The tile grows with B (small batches take small tiles and more workgroups).  Returns FIL_OK, or the argument / menu error the
 *     launch would give.
 */
#define FIL_LSTM_FORWARD 0
#define FIL_LSTM_REVERSE 1
#define FIL_LSTM_BIDIR 2
int fil_lstm_plan(int B, int T, int K, int H, int dirs, int* plan /* [8] */);
size_t fil_lstm_saved_bytes(int B, int T, int K, int H, int dirs);
int fil_lstm_fwd(const float* x, const unsigned char* mask, const float* W, const float* U, const float* b, float* hs, float* saved,
                 int B, int T, int K, int H, int dirs, void* stream);
size_t fil_lstm_bwd_workspace_bytes(int B, int T, int K, int H, int dirs);
int fil_lstm_bwd(const float* x, const unsigned char* mask, const float* W, const float* U, const float* hs, const float* saved,
                 const float* g_hs, const float* g_last, float* dx, float* dW, float* dU, float* db, void* workspace,
                 size_t workspace_bytes, int B, int T, int K, int H, int dirs, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N3  Masked multi-head self-attention over a behaviour sequence (extension: the scaled dot-product layer of "Attention is all you
 *     need" as the Behaviour Sequence Transformer applies it to a history; NOT the reference's MultHeadAttentionLayer, which
 *     fil_attn_* / fil_pattn_* restate and which stays as it is).  All tensors fp32 except mask.  Entry points added only: the ABI
 *     version stays.
 *   x [B,T,K] the sequence; mask [B,T] uint8, non-zero = live, NULL = all live (live slots may sit anywhere); Wq, Wk, Wv [K, H*D],
 *   H heads of width D; out [B,T,H*D], position-major, heads concatenated.  With q = x Wq, k = x Wk, v = x Wv, per sample and head h
 *   (columns hD .. hD+D-1):
 *     s_ij = q_i . k_j (* 1/sqrt(D) when use_scale != 0);  p_ij = softmax of s_ij over the LIVE j (max-subtracted);
 *     out_i = sum_j p_ij v_j for a live i;  out_i = 0 for a masked i (a sample with no live slot: zeros).
 *   No biases, no output projection, no dropout.  A masked position's x row is never read.
 *   fil_seqattn_fwd: out, and `saved` [B,T,3,H*D] = (q, k, v) of the live positions for the backward (fil_seqattn_saved_bytes; opaque
 *     to the caller; masked positions are left unwritten; NULL: nothing is saved, for inference).
 *   fil_seqattn_bwd: g [B,T,H*D] -> dx [B,T,K], dWq, dWk, dWv [K, H*D].  A masked position's g row is never read; dx is exactly 0
 *     there.  The scores and probabilities are recomputed from `saved`; the softmax gradient is taken relative to the row's top key
 *     (a row with one live key gives exactly 0, a peaked row keeps its digits).  Each output may be NULL and is then not
 *     written, the others keep the bits of the full call (dWq, dWk, dWv all NULL: no parameter pass, no workspace; all four NULL:
 *     FIL_ERR_ARG).  The parameter gradients leave the main launch as one partial per workgroup in `workspace`
 *     (fil_seqattn_bwd_workspace_bytes; every byte that is read was written by that launch) and a second small launch adds the
 *     partials in a fixed order.  `out` is the forward's output (kept in the signature for a caller-side check; not read).
 *   One launch per direction (plus the partial sum).  Nothing of size [T,T] or [B,T,3HD] beyond `saved` touches global memory.  No
 *   atomics; every sum has a fixed order: the same inputs give the same bits on every call, and a sample's out / dx rows do not
 *   depend on the rest of the batch.
 *   Menu: K % 4 == 0, D % 4 == 0, K <= 64, H <= 8, H*D <= 64, 1 <= T <= 256, and a one-sample tile within 163,328 bytes of dynamic
 *   LDS in both directions: 4 (T (K + 5 H D + 5 H + 25) + 8) bytes in the backward, the larger (every menu shape at T <= 64 fits,
 *   and T <= 256 at K, H*D <= 16).  FIL_ERR_UNSUPPORTED otherwise, the limit in the message.
 *   B == 0 returns FIL_OK before any pointer is looked at.  A workspace smaller than needed: FIL_ERR_ARG, the needed size in the message.
 *   fil_seqattn_plan: the launchers' own arithmetic (no GPU call): plan[8] = {fwd_ok, bwd_ok, samples per workgroup tile, grid, grid
 *     cap, parameter-gradient partials (= grid), forward LDS bytes, backward LDS bytes}.  The tile is the most samples that give each of a
 *     workgroup's 256 threads at most one (head, row) pair, floor(256 / (H T)), at least 1 and at most what LDS holds; it does not
 *     grow with B (a small LDS image keeps several workgroups on a CU): past grid cap tiles a workgroup walks several.  Returns
 *     FIL_OK, or the argument / menu error the launch would give.
 */
int fil_seqattn_plan(int B, int T, int K, int H, int D, int* plan /* [8] */);
size_t fil_seqattn_saved_bytes(int B, int T, int K, int H, int D);
int fil_seqattn_fwd(const float* x, const unsigned char* mask, const float* Wq, const float* Wk, const float* Wv, float* out,
                    float* saved, int B, int T, int K, int H, int D, int use_scale, void* stream);
size_t fil_seqattn_bwd_workspace_bytes(int B, int T, int K, int H, int D);
int fil_seqattn_bwd(const float* x, const unsigned char* mask, const float* Wq, const float* Wk, const float* Wv, const float* out,
                    const float* saved, const float* g, float* dx, float* dWq, float* dWk, float* dWv, void* workspace,
                    size_t workspace_bytes, int B, int T, int K, int H, int D, int use_scale, void* stream);

/* The same operator under a structure mask (view) and with a pooled output (extension: the three views of the Sequence-Aware
 * Factorization Machine and its intra-view mean pooling).  The same kernels: fil_seqattn_fwd / _bwd are these calls with
 * FIL_SEQ_VIEW_FULL, split 0, rows out and g.  fil_seqattn_plan, _saved_bytes and _bwd_workspace_bytes serve both families; the menu
 * and both LDS images are the same.  Entry points added only: the ABI version stays.
 *   The keys row i may see are A_i = { j : j live and allowed(i, j) }:
 *     FIL_SEQ_VIEW_FULL    every j                     (split must be 0)
 *     FIL_SEQ_VIEW_CAUSAL  j <= i                      (split must be 0)
 *     FIL_SEQ_VIEW_CROSS   (i < split) != (j < split), 1 <= split <= T - 1: the first `split` rows see only the others and the
 *                          others see only them
 *   p_ij = max-subtracted softmax of s_ij over A_i, out_i = sum over A_i of p_ij v_j in ascending j.  A masked i, and a live i with an
 *   empty A_i (a static row of a sample whose history is all padding), gives out_i = 0 and sends no gradient anywhere.  Keys outside
 *   A_i are not visited.  The softmax gradient is relative to the row's first maximal key of A_i (one allowed key: ds = 0 exactly).
 *   fil_seqattn_fwd_v: out [B,T,H*D] or NULL; pooled [B,H*D] or NULL: pooled[b] = (sum of out_i over the live i, ascending, fp32) /
 *     n_b with n_b the number of live rows, one division; n_b = 0 gives zeros.  At least one of the two; both given: both written.
 *     With out = NULL nothing of size [B,T,H*D] but `saved` is written.
 *   fil_seqattn_bwd_v: exactly one of g [B,T,H*D] and gpool [B,H*D]; with gpool every live row takes g_i = gpool[b] / n_b (one fp32
 *     division per element).  No `out` argument (the first form does not read its own).  Outputs, NULL subsets, workspace, B == 0 and
 *     the fixed summation order are those of fil_seqattn_bwd.
 *   FIL_ERR_ARG, the entry point and the offending value in the message: a view outside 0 .. 2; split != 0 with FULL or CAUSAL; CROSS
 *     with split < 1 or split >= T; out and pooled both NULL; g and gpool both or neither given.  Menu errors as above.
 */
#define FIL_SEQ_VIEW_FULL 0
#define FIL_SEQ_VIEW_CAUSAL 1
#define FIL_SEQ_VIEW_CROSS 2
int fil_seqattn_fwd_v(const float* x, const unsigned char* mask, const float* Wq, const float* Wk, const float* Wv, float* out,
                      float* pooled, float* saved, int B, int T, int K, int H, int D, int use_scale, int view, int split, void* stream);
int fil_seqattn_bwd_v(const float* x, const unsigned char* mask, const float* Wq, const float* Wk, const float* Wv, const float* saved,
                      const float* g, const float* gpool, float* dx, float* dWq, float* dWk, float* dWv, void* workspace,
                      size_t workspace_bytes, int B, int T, int K, int H, int D, int use_scale, int view, int split, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N3  Top-k retrieval over a LONG behaviour history (extension: the General Search Unit of the Search-based Interest Model): score
 *     every live slot of a history straight from the embedding table, keep the k best, return them in time order.  Forward only,
 *     integer results, nothing to differentiate: fil_embed_gather on the selected ids and fil_din_* then run over k slots instead
 *     of T.  Entry points added only: the ABI version stays.
 *   hist_idx: B rows of T field-local ids (int64), row b at hist_idx + b * hist_stride (hist_stride >= T, in elements);
 *   offset, size: the field's first row in the concatenated table and its vocabulary (size < 0: ids are trusted); pad_id;
 *   mask [B,T] uint8, non-zero = live, NULL = all live.
 *   Soft part (both or neither): table [V,K] fp32, 16-byte aligned; q: B rows of K fp32, row b at q + b * q_stride (>= K).
 *   Hard part (both or neither): attr: B rows of T int64, row b at attr + b * attr_stride (>= T); cand [B] int64.
 *   At least one part must be given (FIL_ERR_ARG otherwise); both may be.
 *   A slot is LIVE iff id != pad_id, 0 <= id < size, mask is NULL or non-zero there, and attr is NULL or attr[b,t] == cand[b].  An id
 *   that is not pad_id and lies outside [0, size) is not live and is counted in *oob_count (device int, may be NULL; the caller zeroes
 *   it), whatever mask and attr say -- as the gather counts it.  A slot that is not live issues NO table read.
 *   Score of a live slot: s = +0; for j = 0 .. K-1: s = s + (table[offset + id, j] * q[b, j]), every multiply and every add rounded
 *     to fp32 on its own, in ascending j, by one lane: no fused multiply-add, no tree.  Without the soft part the score is +0.
 *   Order of scores: by the key bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000) of their fp32 bits, compared as unsigned integers:
 *     -0 < +0, +-inf are ordinary values.  NaN scores give an unspecified but valid selection (distinct live slots, ascending, n of them).
 *   Selection: the n = min(k, live slots) largest by (key descending, position ascending); with FIL_SEARCH_PREFER_LAST the second
 *     criterion is position descending.  The hard part alone therefore returns the first k matches, with PREFER_LAST the last k.
 *   Output, the selected slots in ASCENDING position (time order): sel_pos [B,k] int32 the positions, sel_idx [B,k] int64 the ids,
 *     sel_score [B,k] fp32 the scores (NULL: not written); the tail n .. k-1 is -1 / pad_id / +0; count [B] int32 = n.
 *   One launch.  One workgroup per sample (64 threads for T <= 64, 256 otherwise), at most 4096 workgroups, past that a workgroup walks
 *   several samples.  The keys stay in LDS: a radix select (four 8-bit passes, integer LDS histograms) finds the k-th key, ballots and
 *   popcounts order the ties and compact the result.  No float atomics, no [B,T] or [B,T,K] block in global memory, no host
 *   synchronisation, no data-dependent size (graph-capture safe); repeats are bit-identical and a sample's result does not depend on
 *   the rest of the batch.
 *   Menu: K % 4 == 0, K <= 64 (also without the soft part, where K is otherwise unused), 1 <= k <= 256 (what fil_din_* takes),
 *   1 <= T <= 16384, B T < 2^31, dynamic LDS 4 (K + T rounded up to 4) + 8 ceil(T / 64) + 1088 bytes within 163,328
 *   (FIL_ERR_UNSUPPORTED otherwise, the limit in the message).  k may exceed T.  Unknown flag bits: FIL_ERR_ARG.
 *   B == 0 returns FIL_OK before any pointer is looked at.
 *   fil_seq_search_plan: the launcher's own arithmetic (no GPU call): plan[8] = {1, 1, samples per workgroup tile (= 1), grid, grid cap,
 *     grid, LDS bytes, 0} -- the layout of the other fil_*_plan entry points; there is no backward, its fields are 1 / 0.  Returns
 *     FIL_OK, or the argument / menu error the launch would give.
 */
#define FIL_SEARCH_PREFER_LAST 1
int fil_seq_search_plan(int B, int T, int K, int k, int* plan /* [8] */);
int fil_seq_search(const int64_t* hist_idx, int64_t hist_stride, int64_t offset, int64_t size, int64_t pad_id,
                   const unsigned char* mask, const float* table, const float* q, int64_t q_stride, const int64_t* attr,
                   int64_t attr_stride, const int64_t* cand, int* sel_pos, int64_t* sel_idx, int* count, float* sel_score,
                   int* oob_count, int B, int T, int K, int k, int flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N4  Neural Turing Machine memory read / write over a sequence (extension: the memory of the Multi-channel user Interest Memory
 *     Network, "Practice on Long Sequential User Behavior Modeling for CTR Prediction", section 4.1 -- content addressing by cosine
 *     similarity, one read head, one erase / add write head; the reference's ReadLayer / WriteLayer / AddressCalLayer /
 *     ControlWrapLayer are not restated, their source was not available).  All tensors fp32 except mask.  Entry points added only:
 *     the ABI version stays.
 *   h [B,T,H] the controller's states; mask [B,T] uint8, non-zero = live, NULL = all live (live slots may sit anywhere); Wp [H,4D+2]
 *   and bp [4D+2] in the column order kr (D) | kw (D) | e (D) | a (D) | beta_r | beta_w; M0 [m,D] the initial memory, shared by all
 *   samples.  The state is M [m,D] (M0 before the first live step) and r [D] (zeros).  One live step, M = the previous memory:
 *     p = h_t Wp + bp;  kr = tanh(p_kr);  kw = tanh(p_kw);  e = sigmoid(p_e);  a = tanh(p_a);
 *     beta = softplus(p_beta) + 1 for both heads, softplus(v) = max(v, 0) + log1p(exp(-|v|));
 *     c_i(k) = (M_i . k) / sqrt((|M_i|^2 + eps) (|k|^2 + eps)), eps = 1e-6: one square root of the product, smooth at M_i = 0 and k = 0;
 *     wr = softmax_i(beta_r c_i(kr));  ww = softmax_i(beta_w c_i(kw)): both on the PREVIOUS M, the row maximum subtracted;
 *     r_t = sum_i wr_i M_i (the read comes before the write);  M_t[i] = M_i (1 - ww_i e) + ww_i a (erase, then add).
 *   A masked step carries M and r bit for bit (rs[b,t] = zeros before the first live step); its h_t is never read.
 *   fil_ntm_fwd: rs [B,T,D] the reads, r_last [B,D] = rs[:,T-1], MT [B,m,D] the final memory (each may be NULL and is then not
 *     written; all three NULL: FIL_ERR_ARG), and `saved` for the backward (fil_ntm_saved_bytes; opaque to the caller; per live step
 *     the memory BEFORE the step [m,D], the activations [4D] and 6 + 5m scalars: the betas and their sigmoids, the key norms, and per
 *     slot both weights, both cosines and the row norm; masked steps are left unwritten; NULL: nothing is saved, for inference).
 *     h_t Wp is fused into the step: besides h, rs and saved nothing of size B T n touches global memory.
 *   fil_ntm_bwd: g_rs [B,T,D] or g_last [B,D] (the gradient of rs[:,T-1]) and / or g_M [B,m,D] (any may be NULL, not all) ->
 *     dh [B,T,H], dWp, dbp, dM0.  No product and no exponential is taken again: everything comes from `saved`.  A masked step passes
 *     the gradients of M and r through unchanged; dh is exactly 0 there.  A sample without a live step sends g_M[b] to dM0.  Each
 *     output may be NULL and is then not computed, the others keep the bits of the full call (dWp, dbp, dM0 all NULL: no parameter
 *     pass, no workspace; all four NULL: FIL_ERR_ARG).  The parameter gradients leave the main launch as one partial per workgroup in
 *     `workspace` (fil_ntm_bwd_workspace_bytes; every byte that is read was written by that launch) and a second small launch adds
 *     the partials in a fixed order.
 *   One launch per direction (plus the partial sum).  No atomics; every sum has a fixed order for a given shape: the same inputs give
 *   the same bits on every call, a sample's bits depend neither on its place in the batch nor on B, and the sums over d behind
 *   M_i . k, |M_i|^2 and |k|^2 run in one order for every slot: slots with identical rows get identical bits.
 *   Menu: any T >= 1; H % 4 == 0, H <= 64; D % 4 == 0, D <= 64; 1 <= m <= 16; both passes within 163,328 bytes of dynamic LDS, which
 *   every such shape is (129,168 in the forward and 128,384 in the backward at H = 64, m = 16, D = 64 with tiles of 16 samples).  FIL_ERR_UNSUPPORTED
 *   otherwise, the limit in the message.
 *   B == 0 returns FIL_OK before any pointer is looked at.  A workspace smaller than needed: FIL_ERR_ARG, the needed size in the message.
 *   fil_ntm_plan: the launchers' own arithmetic (no GPU call): plan[8] = {fwd_ok, bwd_ok, samples per workgroup tile, grid, grid cap,
 *     parameter-gradient partials (= grid), forward LDS bytes, backward LDS bytes}.  The tile grows with B (small batches take small
 *     tiles and more workgroups).  Returns FIL_OK, or the argument / menu error the launch would give.
 */
int fil_ntm_plan(int B, int T, int H, int m, int D, int* plan /* [8] */);
size_t fil_ntm_saved_bytes(int B, int T, int H, int m, int D);
int fil_ntm_fwd(const float* h, const unsigned char* mask, const float* Wp, const float* bp, const float* M0, float* rs, float* r_last,
                float* MT, float* saved, int B, int T, int H, int m, int D, void* stream);
size_t fil_ntm_bwd_workspace_bytes(int B, int T, int H, int m, int D);
int fil_ntm_bwd(const float* h, const unsigned char* mask, const float* Wp, const float* saved, const float* g_rs, const float* g_last,
                const float* g_M, float* dh, float* dWp, float* dbp, float* dM0, void* workspace, size_t workspace_bytes, int B, int T,
                int H, int m, int D, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N5  Time-stream GRU over a behaviour sequence with event gaps (extension: the core of the Deep Time-Stream model -- a GRU whose
 *     state moves between two events, and from the last event to the prediction time, under a learned ODE dh/dt = tanh(h Wf + bf),
 *     integrated by S explicit Euler substeps; the reference's layer was not available, this is the project's own statement).  All
 *     tensors fp32 except mask.  Entry points added only: the ABI version stays.
 *   x [B,T,K]; dt [B,T] the time from the previous live event to this one, in the caller's units (documented as >= 0; any finite
 *   value runs, nothing is checked on the device); dt_out [B] the time from the last event to the prediction, or NULL; mask [B,T]
 *   uint8, non-zero = live, NULL = all live; W [K,3H], U [H,3H], b [2,3H]: fil_gru_*'s in the mode FIL_GRU_GRU; Wf [H,H], bf [H] the
 *   ODE's; S the substeps.  One live step on the carried state h (zeros at first):
 *     delta = dt[b,t] / (float)S                                  (one correctly rounded fp32 division)
 *     S times:  f_j = tanhf(bf_j + sum_k h_k Wf[k,j])             (one fmaf chain, k ascending, started from bf_j)
 *               h_j = fmaf(delta, f_j, h_j)                       (explicit Euler; every unit reads the OLD h)
 *     then fil_gru_fwd's step (reset_after, columns z | r | h, h_new = fma(u, c, (1 - u) h)) on the evolved h.
 *   A masked step carries h bit for bit; its x row and its dt are never read.
 *   fil_tsgru_fwd: hs [B,T,H] the states after each step; with dt_out, z [B,H] = the last state of EVERY sample (zeros for one
 *     without a live step) evolved by S more substeps of dt_out[b] / S (dt_out and z are both given or both NULL); and `saved` for
 *     the backward (fil_tsgru_saved_bytes; opaque to the caller: per live step fil_gru_fwd's four planes and, per substep, the state
 *     before it and f, [B,T,4+2S,H]; behind them the final evolution's pairs [B,2S,H]; masked steps are left unwritten; NULL: nothing
 *     is saved, for inference).
 *   fil_tsgru_bwd: g_hs [B,T,H], g_last [B,H] (the gradient of hs[:,T-1]) and g_z [B,H] (needs dt_out): any non-empty subset, the
 *     others NULL -> dx, dW, dU, db, dWf, dbf.  dt and dt_out are data: they get no gradient.  Per substep, in reverse:
 *     q = delta dh (1 - f^2); dh += q Wf^T; dWf += h_s^T q; dbf += q.  No product and no tanhf is taken again: the GRU step's previous
 *     state is fma(delta, f, h) of the last saved pair.  Each output may be NULL and is then not computed, the others keep the bits
 *     of the full call (all five parameter gradients NULL: no parameter pass, no workspace; all six NULL: FIL_ERR_ARG).  The
 *     parameter gradients leave the main launch as one partial per workgroup in `workspace` (fil_tsgru_bwd_workspace_bytes; every
 *     byte that is read was written by that launch) and a second small launch adds the partials in a fixed order.
 *   One launch per direction for all T steps and all substeps (plus the partial sum).  No atomics; every sum has a fixed order for a
 *   given shape: the same inputs give the same bits on every call, and a sample's hs, z and dx depend neither on its place in the
 *   batch nor on B.  With dt = 0 and dt_out = 0, or with Wf = 0 and bf = 0, hs has fil_gru_fwd's bits and z those of hs[:,T-1].
 *   Menu: any T >= 1; K % 4 == 0, H % 4 == 0, K <= 64, H <= 64; 1 <= S <= 8; both passes within 163,328 bytes of dynamic LDS: the
 *   weights, Wf (forward) or its transpose (backward) and the substep images sit beside fil_gru_*'s sections, which leaves out the
 *   largest shapes (every H <= 52 is in; H = 56: K >= 52 is out, H = 60: K >= 40, H = 64: K >= 36, and at the tiles of 16 samples
 *   that large batches take H = 60: K >= 36, H = 64: K >= 20; fil_tsgru_plan decides, and S does not enter).  FIL_ERR_UNSUPPORTED
 *   otherwise (also for S > 8), the limit in the message; S < 1 is FIL_ERR_ARG.
 *   B == 0 returns FIL_OK before any pointer is looked at.  A workspace smaller than needed: FIL_ERR_ARG, the needed size in the message.
 *   fil_tsgru_plan: the launchers' own arithmetic (no GPU call): plan[8] = {fwd_ok, bwd_ok, samples per workgroup tile, grid, grid cap,
 *     parameter-gradient partials (= grid), forward LDS bytes, backward LDS bytes}, as fil_gru_plan's.
 */
int fil_tsgru_plan(int B, int T, int K, int H, int S, int* plan /* [8] */);
size_t fil_tsgru_saved_bytes(int B, int T, int K, int H, int S);
int fil_tsgru_fwd(const float* x, const float* dt, const float* dt_out, const unsigned char* mask, const float* W, const float* U,
                  const float* b, const float* Wf, const float* bf, float* hs, float* z, float* saved, int B, int T, int K, int H, int S,
                  void* stream);
size_t fil_tsgru_bwd_workspace_bytes(int B, int T, int K, int H, int S);
int fil_tsgru_bwd(const float* x, const float* dt, const float* dt_out, const unsigned char* mask, const float* W, const float* U,
                  const float* Wf, const float* saved, const float* g_hs, const float* g_last, const float* g_z, float* dx, float* dW,
                  float* dU, float* db, float* dWf, float* dbf, void* workspace, size_t workspace_bytes, int B, int T, int K, int H, int S,
                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * N2  The score head and the loss behind the interaction layers (all tensors fp32, n = batch rows).
 *   ScoreLayer(use_add=True).call (kon/model/ctr_model/layer/core_layer/core_layer.py:58-84): keras Add over the [B,1] parts,
 *   then sigmoid.  fil_score_add_sigmoid_fwd: out[i] = sigmoid(((a[i] + b[i]) + c[i]) + d[i]) -- left to right like the
 *   reference's Add; b, c, d may be NULL.  _bwd: dsum[i] = dout[i] * out[i] * (1 - out[i]), the gradient of EVERY part.
 *   fil_bce_mean_fwd: binary cross-entropy on probabilities as the reference compiles it (example/ctr_example/un_seq.py:61,
 *   model.compile(loss=tf.losses.binary_crossentropy); TensorFlow 2.1 keras/backend.py): pc = clip(p, eps, 1 - eps),
 *   loss[0] = mean(-(y log(pc + eps) + (1 - y) log(1 - pc + eps))); dp (may be NULL) [n] = d loss / d p (0 where the clip is
 *   active).  Keras' eps is 1e-7.  One workgroup, fixed summation order: repeats are
 *   bit-identical.  Meant for training batches (n up to ~1e5); n >= 1.
 */
int fil_score_add_sigmoid_fwd(const float* a, const float* b, const float* c, const float* d, float* out, int n, void* stream);
int fil_score_add_sigmoid_bwd(const float* out, const float* dout, float* dsum, int n, void* stream);
int fil_bce_mean_fwd(const float* p, const float* y, float eps, float* loss, float* dp, int n, void* stream);

/* MergeScoreLayer.call (core_layer/core_layer.py:86-100): StackLayer concat of the n_parts (1..4) tensors parts[i] [B, widths[i]] ->
 * Dense(O <= 8 units, softmax): out [B, O] = softmax(concat(parts) W + bias), W [D = sum widths, O] row-major (the Keras Dense kernel),
 * bias [O].  DeepFM / DCN / Wide&Deep end in it (model/models.py:87,104).  One launch forward, two backward, the parts read where they lie (no
 * concatenated copy).  dtypes[i] = storage type of parts[i] and of dparts[i] (FIL_F32 or FIL_BF16: a model under bf16 autocast hands
 * a bf16 FM output next to an fp32 MLP output); W, bias, out, dout, dW, db are fp32 and so is the arithmetic.
 *   bwd: dz = out (dout - <dout, out>); dparts[i] [B, widths[i]] = dz W_i^T (entries / the array may be NULL: not wanted);
 *        dW [D, O] = concat(parts)^T dz, db [O] = column sums of dz -- block partials summed in block order by a second, tiny launch:
 *        deterministic.  workspace: fil_merge_softmax_bwd_workspace_bytes(B, D, O) bytes. */
/* The dense layers of the zoo's MLPs (DnnLayer / HiddenLayer / Dense, core_layer/core_layer.py:102-118,201-226) at batch-sized M and a
 * few hundred columns: C [M][N] = op(A) [M][K] . op(B) [K][N] (+ bias[n] (epilogue 1), then ReLU (2)), fp32, exact
 * v_mfma_f32_32x32x2_f32 chains, deterministic (a small output with a long reduction -- dW = x^T dz -- is split over k and the slices
 * are summed in order by a second launch: that is what the workspace is for; a call with an epilogue is never split).
 *   trans_a = 0: A is [M][K] row-major, leading dimension lda >= K;  1: A is [K][M], lda >= M   (dW = x^T dz: A = x, trans_a = 1)
 *   trans_b = 0: B is [K][N] row-major, ldb >= N;                    1: B is [N][K], ldb >= K   (dx = dz W^T: B = W [in][out], trans_b = 1)
 * Any M, N, K; 16-byte operand loads where base and leading dimension allow, element-wise otherwise.  Leading dimensions may be padded
 * (the padding is neither used nor written) and A, B, C need dword alignment only.  K = 0: C = 0 (+ bias, ReLU) and A, B are not
 * dereferenced, whatever lda and ldb are (they may be NULL). */
size_t fil_gemm_f32_workspace_bytes(int M, int N, int K);
int fil_gemm_f32(const float* A, const float* B, float* C, const float* bias, int M, int N, int K, int lda, int ldb, int ldc, int trans_a,
                 int trans_b, int epilogue, void* workspace, size_t workspace_bytes, void* stream);

/* Backward half of Dense + bias + ReLU (the zoo's MLP layers, DnnLayer core_layer/core_layer.py:102-118,201-226; the layer's GEMMs stay
 * library GEMMs): dz[b,n] = y[b,n] > 0 ? dy[b,n] : 0 (y = the layer's OUTPUT) and dbias[n] = sum_b dz[b,n] in ONE pass over [B, N]
 * (torch: threshold_backward, then a column reduce).  y, dy, dz in `dtype` storage (FIL_F32 / FIL_BF16), dbias fp32; deterministic (block
 * partials summed in block order by a second, tiny launch). */
size_t fil_relu_bias_bwd_workspace_bytes(int B, int N);
int fil_relu_bias_bwd(const void* y, const void* dy, void* dz, float* dbias, int B, int N, int dtype, void* workspace, size_t workspace_bytes,
                      void* stream);
size_t fil_merge_softmax_bwd_workspace_bytes(int B, int D, int O);
int fil_merge_softmax_fwd(const void* const* parts, const int* widths, const int* dtypes, int n_parts, const float* W, const float* bias,
                          float* out, int B, int O, void* stream);
int fil_merge_softmax_bwd(const void* const* parts, const int* widths, const int* dtypes, int n_parts, const float* W, const float* out,
                          const float* dout, void* const* dparts, float* dW, float* db, int B, int O, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ---------------------------------------------------------------------------------------------
 * O1  Keras-exact Adam -- replaces optimizer='adam' of model.compile (example/ctr_example/un_seq.py:61; TF 2.1 Keras Adam ->
 *     the ApplyAdam kernel), every tensor fp32:
 *       t = *step + 1;  b1^t, b2^t = powf(beta_1, (float)t), powf(beta_2, (float)t)   (on the device: Keras' iterations + 1)
 *       alpha = lr * sqrt(1 - b2^t) / (1 - b1^t)
 *       m += (g - m) * (1 - beta_1);  v += (g*g - v) * (1 - beta_2);  p -= (m * alpha) / (sqrt(v) + epsilon)
 *     epsilon is added to the UNCORRECTED sqrt(v) (torch.optim.Adam adds it to sqrt(v / (1 - b2^t)): at t = 1 its epsilon is in
 *     effect 1/sqrt(1 - beta_2) times Keras').  Keras' defaults: lr 1e-3, beta_1 0.9, beta_2 0.999, epsilon 1e-7.
 *   step: ONE int64 device counter per optimizer = the number of completed steps (Keras' `iterations`).  Every entry point below
 *     only reads it; fil_adam_multi(advance = 1) increments it in a one-thread launch queued behind its update, so the last call of
 *     an optimizer step passes advance = 1 (a captured graph then advances the counter on every replay).
 *
 *   fil_adam_multi: every descriptor of `tensors` (a DEVICE array of n entries) in one launch.  grad NULL = a zero gradient;
 *     l2 != 0 adds 2 * l2 * p to the gradient (Keras' l2(l2) regulariser, applied inside the update: split a tensor into several
 *     descriptors to give its row ranges different coefficients).  Any numel (>= 0); 16-byte accesses where all four arrays of a
 *     descriptor are 16-byte aligned, element-wise otherwise and in the tail.  total_numel = the sum of the descriptors' numel (it
 *     sizes the grid: a wrong value costs speed, never correctness).  n = 0 with advance = 1 only advances the counter.
 *
 *   fil_embed_adam_runs: the gradient of an embedding table as fil_embed_run_sum_dt would build it -- (g [R/F rows of F fields][K]
 *     in g_dtype, perm, sorted_ids) of fil_embed_sort_fields -- applied to table / m / v [V, K] IN PLACE, never materialised: each run
 *     of equal ids >= 0 is summed in the same order as fil_embed_run_sum (so the row gradient is bit-identical to the dense one),
 *     gets + 2 * field_l2[f] * p (f = perm % F, the field of the run; field_l2 [F] may be NULL = no l2) and its row takes the update
 *     above.  Ids -1 (out-of-range ids, frozen fields) are skipped.  No data-dependent size: graph-capturable.  mode:
 *       FIL_ADAM_KERAS  Keras' dense semantics: the rows it updates are stamped (stamp[row] = low 32 bits of t; stamp [V] int32,
 *                       caller-owned, zero-initialised once), and fil_embed_adam_sweep then updates every OTHER row of the table.
 *       FIL_ADAM_LAZY   LABELLED deviation from the reference (TF-Addons LazyAdam): only the touched rows change (bias correction
 *                       with the global t); no stamps, no sweep.  Never the default.
 *   fil_embed_adam_sweep: the FIL_ADAM_KERAS rows of the table that are not stamped with the current t take the update with
 *     g = 2 * field_l2[f] * p (0 without l2): m and v decay and the row moves, as Keras' dense Adam moves every row.  Row r belongs to
 *     the last field f with offsets[f] <= r (none: no l2); rows of fields with frozen[f] != 0 (frozen [F] may be NULL) are left alone
 *     (a non-trainable Keras Embedding is not in the optimizer's variable list).  One read and one non-temporal write of p, m, v and a
 *     read of stamp per row; F <= 1024. *
 *   Data parallelism (every rank holds the whole table; each rank's batch shard leaves its own runs record):
 *   fil_embed_runs_compact: one record -> a compact list.  ids_out [cap] = the distinct row ids >= 0 of sorted_ids in ascending order
 *     (ids -1 dropped; ascending because offsets[] ascends, as fil_embed_sort_fields requires of a sorted list), values_out [cap, K]
 *     fp32 = each run's sum in fil_embed_run_sum's order (bit-identical to the dense gradient's row), *count_out (device int64) = the
 *     number of ids; slots [count, cap) get ids INT64_MAX (a binary search over all cap entries stays valid; their values are left
 *     as they were).  cap >= R; R < 2^31.  Workspace: fil_embed_runs_compact_workspace_bytes(R).  Three launches, none sized by data
 *     (capturable); the compaction scan is integer, hence deterministic.  perm may name a position more than once (a pooled
 *     field's record, N3: every slot of a bag names the bag); sorted_ids must then ascend over the whole record.
 *   fil_embed_adam_merged: W such lists gathered back to back -- ids [W][cap], values [W][cap][K], counts [W] (device) -- applied to
 *     table / m / v [V, K] in place: every row of the union is updated once, by its owner (the lowest list holding it), with
 *     g = the row's sums added in list order 0 .. W-1 + 2 * field_l2[f] * p (f = the last field with offsets[f] <= row, as in the
 *     sweep; field_l2 may be NULL) and the update above; FIL_ADAM_KERAS stamps it (then fil_embed_adam_sweep, unchanged).  Every
 *     replica that applies the same gathered lists computes the same bits; W = 1 is bit-identical to fil_embed_adam_runs on the same
 *     record.  Rows outside [0, V) are skipped.  F <= 1024, K <= 256.
 */
size_t fil_embed_runs_compact_workspace_bytes(long R);
int fil_embed_runs_compact(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int64_t* ids_out,
                           float* values_out, int64_t* count_out, long cap, void* workspace, size_t workspace_bytes, void* stream);
int fil_embed_adam_merged(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K, const int64_t* offsets,
                          const float* field_l2, int F, float* table, float* m, float* v, int32_t* stamp, int64_t V, const int64_t* step,
                          float lr, float beta_1, float beta_2, float epsilon, int mode, void* stream);
/*   Deferred mode (optim.Adam(sweep_period=N)): instead of fil_embed_adam_sweep at every step, a table's untouched rows
 *   catch up lazily, bit-identical to the per-step sweep (the update of an untouched row, g = 2 l2[f] p, depends on the row's own
 *   p, m, v, its field's l2 and the step's coefficients only).  State per table, caller-owned:
 *     stamp [V] int32   stamp[r] = s: row r is current through completed step s (low 32 bits); all = the step count to begin with.
 *     ring  [D][4] fp32 (16-byte aligned; D = fil_embed_adam_ring_len(N), the power of two >= N + 1): entry t mod D = the
 *                       coefficients of step t (1-based), or a "skip" entry for a step at which the table had no record (Keras mode
 *                       leaves such a table alone).  Written by fil_embed_adam_roll of step t only.
 *   Replayed steps take the sweep's field view (offsets / field_l2 / frozen: frozen fields never move).  No entry point allocates,
 *   synchronises or sizes a launch by data: a deferred step captures like Keras mode.  1 <= N <= 1023; K <= 256; F <= 1024.
 *   fil_embed_adam_catchup_runs: the forward's launch.  Every distinct row >= 0 (< V) of a sorted record (sorted_ids of
 *     fil_embed_sort_fields, R entries) is brought current through the completed steps (*step) in place and stamped; the gather that
 *     follows reads exactly the values the per-step sweep would have left.
 *   fil_embed_adam_runs_deferred: fil_embed_adam_runs in FIL_ADAM_KERAS mode, each run's row first caught up through the completed
 *     steps, then updated with step t = *step + 1 and stamped t.
 *   fil_embed_adam_merged_deferred: fil_embed_adam_merged in FIL_ADAM_KERAS mode with the same catch-up before each row's update (a
 *     row another rank touched may be stale on this replica: replicas differ in how stale their memory is, never in what they compute).
 *   fil_embed_adam_roll: flags FIL_ADAM_ROLL_STEP writes step t's ring entry (FIL_ADAM_ROLL_SKIP: the skip entry) and brings slice
 *     t mod N (rows [j ceil(V/N), (j + 1) ceil(V/N)) clipped to V) current through step t -- every row at least every N steps; called
 *     once per step and table, after the runs update and before the counter advances.  FIL_ADAM_ROLL_FLUSH brings EVERY row current
 *     through the completed steps and writes no entry (a checkpoint, a regulariser value).
 */
int fil_embed_adam_ring_len(int sweep_period);       /* D, or 0 when sweep_period is outside 1 ... 1023 */
enum { FIL_ADAM_ROLL_STEP = 0, FIL_ADAM_ROLL_SKIP = 1, FIL_ADAM_ROLL_FLUSH = 2 };
int fil_embed_adam_catchup_runs(const int64_t* sorted_ids, long R, int K, float* table, float* m, float* v, int32_t* stamp,
                                const float* ring, int sweep_period, const int64_t* offsets, const float* field_l2,
                                const unsigned char* frozen, int F, int64_t V, const int64_t* step, void* stream);
int fil_embed_adam_runs_deferred(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                 const int64_t* offsets, const float* field_l2, const unsigned char* frozen, float* table, float* m, float* v,
                                 int32_t* stamp, const float* ring, int sweep_period, int64_t V, const int64_t* step, float lr, float beta_1,
                                 float beta_2, float epsilon, void* stream);
int fil_embed_adam_merged_deferred(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                   const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F, float* table, float* m,
                                   float* v, int32_t* stamp, const float* ring, int sweep_period, int64_t V, const int64_t* step, float lr,
                                   float beta_1, float beta_2, float epsilon, void* stream);
int fil_embed_adam_roll(float* table, float* m, float* v, int32_t* stamp, float* ring, int sweep_period, int64_t V, int K,
                        const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F, const int64_t* step, float lr,
                        float beta_1, float beta_2, float epsilon, int flags, void* stream);
typedef struct {
  float* param;
  const float* grad;   /* NULL = zero gradient */
  float* m;
  float* v;
  int64_t numel;
  float l2;            /* g += 2 * l2 * param; 0 = none */
  int32_t reserved;    /* 0 */
} fil_adam_tensor;     /* 48 bytes */
enum { FIL_ADAM_KERAS = 0, FIL_ADAM_LAZY = 1 };
int fil_adam_multi(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, float lr, float beta_1, float beta_2,
                   float epsilon, int advance, void* stream);
int fil_embed_adam_runs(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                        const float* field_l2, float* table, float* m, float* v, int32_t* stamp, const int64_t* step, float lr,
                        float beta_1, float beta_2, float epsilon, int mode, void* stream);
int fil_embed_adam_sweep(float* table, float* m, float* v, const int32_t* stamp, int64_t V, int K, const int64_t* offsets,
                         const float* field_l2, const unsigned char* frozen, int F, const int64_t* step, float lr, float beta_1,
                         float beta_2, float epsilon, void* stream);

/* ---------------------------------------------------------------------------------------------
 * O2  Keras-exact Adagrad and Ftrl (TF 2.1 Keras -> ApplyAdagradV2 / ApplyFtrl, ApplyFtrlV2 when l2_shrinkage > 0), every tensor fp32,
 *     `rule` FIL_OPT_ADAGRAD or FIL_OPT_FTRL, hyper-parameters in a fil_rowopt_hyper read ON THE HOST at the call (a captured graph
 *     keeps the values it was captured with):
 *       Adagrad  acc += g*g;  p -= g*lr / (sqrt(acc) + epsilon)                     (Keras: accumulator starts at 0.1, epsilon 1e-7)
 *       Ftrl     gs = g + 2*l2_shrinkage*p;  n' = n + g*g (the raw g);  a(x) = sqrt(x) if lr_power == -0.5 else pow(x, -lr_power)
 *                z += gs - (a(n') - a(n))/lr * p;  q = a(n')/lr + 2*l2;  p = |z| > l1 ? (sign(z)*l1 - z)/q : 0;  n = n'
 *     The accumulator (n) lives in the `m` array of fil_adam_tensor / the `accum` argument, Ftrl's linear slot (z) in `v` / `linear`
 *     (NULL for Adagrad).  Neither rule reads the step counter; it is kept (Keras' iterations) and used for the row stamps only.
 *     Requires lr >= 0; Adagrad epsilon >= 0; Ftrl lr_power <= 0, l1, l2, l2_shrinkage >= 0 (FIL_ERR_ARG otherwise).
 *   Which rows Keras updates (each field a Keras Embedding with l2(emb_reg)): a field with emb_reg > 0 has a dense regulariser
 *     gradient, so EVERY row moves -- a touched row with g = run sum + 2 emb_reg p, an untouched one with g = 2 emb_reg p; a field
 *     with emb_reg = 0 gets IndexedSlices, so only the batch's rows change and every other row and its slots keep their bits (for
 *     Ftrl this is NOT a dense apply with g = 0, which recomputes p from z); a frozen field never changes.  Keras' quirk, reproduced:
 *     under Ftrl the first step takes every untouched row of a regularised field to about -lr*2*emb_reg*p/sqrt(n), in effect 0 (its
 *     initial weights are gone) -- the common case, since make_sparse_info's default emb_reg is 1e-8.
 *   fil_rowopt_multi: fil_adam_multi's contract with the rule: every descriptor in one launch, grad NULL = a zero gradient, l2 adds
 *     2*l2*p to the gradient, 16-byte accesses where the descriptor's arrays are aligned, advance = 1 increments *step.
 *   fil_embed_rowopt_runs: fil_embed_adam_runs' contract with the rule: each run of ids >= 0 summed in fil_embed_run_sum's order,
 *     g = run sum + 2*field_l2[perm % F]*p, the row updated in place; stamp[row] = low 32 bits of *step + 1 when stamp != NULL
 *     (needed when a sweep follows, i.e. when field_l2 has an entry > 0).  f32 / bf16 g_dtype, K <= 256, capturable.
 *   fil_embed_rowopt_sweep: the rows of non-frozen fields with field_l2[f] > 0 (f = the last field with offsets[f] <= row) not stamped
 *     with the current t take the rule with g = 2*field_l2[f]*p; the grid walks those fields' rows only (field_l2 NULL: nothing to
 *     do, no launch).  Non-temporal stores; F <= 1024.
 *   fil_embed_rowopt_merged: fil_embed_adam_merged's contract with the rule on W gathered fil_embed_runs_compact lists: each row of
 *     the union updated once, by its owner (the lowest list holding it), summed in list order; W = 1 is bit-identical to
 *     fil_embed_rowopt_runs on the same record.  Stamps when stamp != NULL.  F <= 1024, K <= 256.
 */
enum { FIL_OPT_ADAGRAD = 1, FIL_OPT_FTRL = 2 };
typedef struct {
  float lr;
  float epsilon;        /* Adagrad */
  float lr_power;       /* Ftrl: learning_rate_power (<= 0) */
  float l1;             /* Ftrl: l1_regularization_strength */
  float l2;             /* Ftrl: l2_regularization_strength */
  float l2_shrinkage;   /* Ftrl: l2_shrinkage_regularization_strength */
} fil_rowopt_hyper;     /* 24 bytes */
int fil_rowopt_multi(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule, const fil_rowopt_hyper* hyper,
                     int advance, void* stream);
int fil_embed_rowopt_runs(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                          const float* field_l2, float* table, float* accum, float* linear, int32_t* stamp, const int64_t* step, int rule,
                          const fil_rowopt_hyper* hyper, void* stream);
int fil_embed_rowopt_sweep(float* table, float* accum, float* linear, const int32_t* stamp, int64_t V, int K, const int64_t* offsets,
                           const float* field_l2, const unsigned char* frozen, int F, const int64_t* step, int rule,
                           const fil_rowopt_hyper* hyper, void* stream);
int fil_embed_rowopt_merged(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K, const int64_t* offsets,
                            const float* field_l2, int F, float* table, float* accum, float* linear, int32_t* stamp, int64_t V,
                            const int64_t* step, int rule, const fil_rowopt_hyper* hyper, void* stream);

/* ---------------------------------------------------------------------------------------------
 * O3  Keras' learning-rate schedules (tf.keras.optimizers.schedules, TF 2.1) and the legacy `decay` of OptimizerV2._decayed_lr,
 *     evaluated ON THE DEVICE from the step counter, so a captured step changes its rate on every replay.  Entry points added only:
 *     the ABI version stays.
 *   fil_lr_schedule: a POD descriptor.  step = *step (Keras' iterations: completed steps, 0 at the first step), s = (float)step;
 *     every constant is fp32 and every operation rounds to fp32 as written (no fused multiply-add), except the two powers, which
 *     are pow((double)base, (double)p) rounded once to fp32:
 *       FIL_LR_CONSTANT      lr = initial_lr
 *       FIL_LR_EXPONENTIAL   p = s / decay_steps (floor(p) when flag);  lr = initial_lr * pow(decay_rate, p)
 *       FIL_LR_INVERSE_TIME  p as above;  lr = initial_lr / (1 + decay_rate * p)
 *       FIL_LR_POLYNOMIAL    flag (cycle): d = decay_steps * (s == 0 ? 1 : ceil(s / decay_steps)), else s = min(s, decay_steps),
 *                            d = decay_steps;  p = s / d;  lr = (initial_lr - end_lr) * pow(1 - p, power) + end_lr
 *                            (power == 1: the base itself, x ** 1.0 == x)
 *       FIL_LR_PIECEWISE     lr = values[i] for the first i < n_boundaries with step <= boundaries[i] (int64 comparisons),
 *                            values[n_boundaries] beyond the last; boundaries non-decreasing, n_boundaries <= 32
 *     then, when decay > 0:  lr = lr / (1 + decay * s).
 *   fil_lr_schedule_check: validates a descriptor in HOST memory (kind, decay_steps > 0, n_boundaries, their order, decay >= 0);
 *     the caller then copies it to the device once.
 *   fil_lr_schedule_eval: one one-thread launch, lr_out[0] = the rate of the step about to run.  sched, step, lr_out: device memory.
 *     Queued once per (step, device) before the first update launch; every update launch of the step then reads the same bits.
 *   The *_lrdev variants are the update entry points of O1 / O2 with the rate read from device memory (lr_dev, one fp32, not
 *     NULL) in place of the by-value `lr` (fil_rowopt_hyper.lr is ignored); everything else, the kernels included, is unchanged.
 *     fil_embed_adam_roll_lrdev writes the step's ring entry from *lr_dev: a replayed step takes the rate of the step it replays
 *     (FIL_ADAM_ROLL_FLUSH and _SKIP read no rate, but lr_dev must still be valid device memory).
 */
#define FIL_LR_MAX_BOUNDARIES 32
enum { FIL_LR_CONSTANT = 0, FIL_LR_EXPONENTIAL = 1, FIL_LR_INVERSE_TIME = 2, FIL_LR_POLYNOMIAL = 3, FIL_LR_PIECEWISE = 4 };
typedef struct {
  int32_t kind;
  int32_t flag;           /* exponential / inverse time: staircase; polynomial: cycle */
  float initial_lr;
  float decay_steps;
  float decay_rate;
  float end_lr;           /* polynomial */
  float power;            /* polynomial */
  float decay;            /* the legacy keyword; 0 = none */
  int32_t n_boundaries;   /* piecewise */
  int32_t reserved;       /* 0 */
  int64_t boundaries[FIL_LR_MAX_BOUNDARIES];
  float values[FIL_LR_MAX_BOUNDARIES + 1];
  int32_t reserved2;      /* 0 */
} fil_lr_schedule;        /* 432 bytes */
int fil_lr_schedule_check(const fil_lr_schedule* host_sched);
int fil_lr_schedule_eval(const fil_lr_schedule* sched, const int64_t* step, float* lr_out, void* stream);
int fil_adam_multi_lrdev(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, const float* lr_dev, float beta_1,
                         float beta_2, float epsilon, int advance, void* stream);
int fil_embed_adam_runs_lrdev(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                              const float* field_l2, float* table, float* m, float* v, int32_t* stamp, const int64_t* step,
                              const float* lr_dev, float beta_1, float beta_2, float epsilon, int mode, void* stream);
int fil_embed_adam_sweep_lrdev(float* table, float* m, float* v, const int32_t* stamp, int64_t V, int K, const int64_t* offsets,
                               const float* field_l2, const unsigned char* frozen, int F, const int64_t* step, const float* lr_dev,
                               float beta_1, float beta_2, float epsilon, void* stream);
int fil_embed_adam_merged_lrdev(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                const int64_t* offsets, const float* field_l2, int F, float* table, float* m, float* v, int32_t* stamp,
                                int64_t V, const int64_t* step, const float* lr_dev, float beta_1, float beta_2, float epsilon, int mode,
                                void* stream);
int fil_embed_adam_runs_deferred_lrdev(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                       const int64_t* offsets, const float* field_l2, const unsigned char* frozen, float* table, float* m,
                                       float* v, int32_t* stamp, const float* ring, int sweep_period, int64_t V, const int64_t* step,
                                       const float* lr_dev, float beta_1, float beta_2, float epsilon, void* stream);
int fil_embed_adam_merged_deferred_lrdev(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                         const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F, float* table,
                                         float* m, float* v, int32_t* stamp, const float* ring, int sweep_period, int64_t V,
                                         const int64_t* step, const float* lr_dev, float beta_1, float beta_2, float epsilon, void* stream);
int fil_embed_adam_roll_lrdev(float* table, float* m, float* v, int32_t* stamp, float* ring, int sweep_period, int64_t V, int K,
                              const int64_t* offsets, const float* field_l2, const unsigned char* frozen, int F, const int64_t* step,
                              const float* lr_dev, float beta_1, float beta_2, float epsilon, int flags, void* stream);
int fil_rowopt_multi_lrdev(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule,
                           const fil_rowopt_hyper* hyper, const float* lr_dev, int advance, void* stream);
int fil_embed_rowopt_runs_lrdev(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                const float* field_l2, float* table, float* accum, float* linear, int32_t* stamp, const int64_t* step,
                                int rule, const fil_rowopt_hyper* hyper, const float* lr_dev, void* stream);
int fil_embed_rowopt_sweep_lrdev(float* table, float* accum, float* linear, const int32_t* stamp, int64_t V, int K, const int64_t* offsets,
                                 const float* field_l2, const unsigned char* frozen, int F, const int64_t* step, int rule,
                                 const fil_rowopt_hyper* hyper, const float* lr_dev, void* stream);
int fil_embed_rowopt_merged_lrdev(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                  const int64_t* offsets, const float* field_l2, int F, float* table, float* accum, float* linear,
                                  int32_t* stamp, int64_t V, const int64_t* step, int rule, const fil_rowopt_hyper* hyper,
                                  const float* lr_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * O4  Keras-exact SGD and RMSprop (TF 2.1 keras/optimizer_v2/gradient_descent.py, rmsprop.py -> ApplyKerasMomentum, ApplyRMSProp and
 *     their Sparse twins), every tensor fp32, `rule` FIL_OPT_SGD or FIL_OPT_RMSPROP, hyper-parameters in a fil_momopt_hyper read ON THE
 *     HOST at the call (a captured graph keeps the values it was captured with).  Entry points added only: the ABI version stays.
 *     Every operation rounds to fp32 in the order written (no fused multiply-add; correctly rounded division and square root):
 *       SGD      momentum == 0   p -= g*lr                                              no slot: slot0 / slot1 (m / v) may be NULL
 *       SGD      momentum  > 0   a = a*momentum - g*lr;  p += a     (FIL_MOMOPT_NESTEROV: p += a*momentum - g*lr)     a in slot0
 *       RMSprop  momentum == 0   rms = rho*rms + (1 - rho)*(g*g);  p -= lr*g / (sqrt(rms) + epsilon)                 rms in slot0
 *                                (Keras computes this variant in Python ops: epsilon OUTSIDE the root; 1 - rho formed once in fp32)
 *       RMSprop  momentum  > 0   the fused ops, epsilon INSIDE the root, rms in slot0, mom in slot1:
 *                  dense rows    rms += (g*g - rms)*(1 - rho);  mom = mom*momentum + (g*lr) / sqrt(rms + epsilon);  p -= mom
 *                  touched rows  rms = rms*rho + (g*g)*(1 - rho);  mom = mom*momentum + ((1 / sqrt(rms + epsilon))*lr)*g;  p -= mom
 *     slot0 lives in the `m` array of fil_adam_tensor, slot1 in `v`; a slot the variant does not have is never read or written.
 *     Requires lr >= 0, momentum in [0, 1]; RMSprop epsilon >= 0, rho in [0, 1], no Nesterov flag (FIL_ERR_ARG otherwise).  None of the
 *     rules reads the step counter; it is kept (Keras' iterations) and used for the row stamps only.
 *   Which rows Keras updates.  All variants but RMSprop with momentum == 0 are row-local, exactly as O2: a touched row takes the touched
 *     form with g = run sum + 2 emb_reg p; an untouched row of a field with emb_reg > 0 takes the DENSE form with g = 2 emb_reg p (the
 *     regulariser's gradient is dense: its momentum decays and it moves); every other row and its slots keep their bits; a frozen field
 *     never changes.  RMSprop with momentum == 0 is not row-local: for IndexedSlices Keras first assigns rms = rms*rho over the WHOLE
 *     variable, then scatters (g*g)*(1 - rho) at the batch's rows and moves only those.  So there an untouched row of an unregularised,
 *     non-frozen field takes rms = rms*rho and its p keeps its bits.  (SGD with momentum == 0: Keras scatter-adds each duplicate id on
 *     its own in an unspecified order; here the run is summed first, in fil_embed_run_sum's order, like every other rule.)
 *   fil_momopt_multi: fil_rowopt_multi's contract with these rules (dense form).
 *   fil_embed_momopt_runs: fil_embed_rowopt_runs' contract (touched form); stamps when stamp != NULL -- needed when a sweep follows:
 *     a regularised field, or RMSprop with momentum == 0 on any table.
 *   fil_embed_momopt_sweep: the unstamped rows.  Row-local variants: fil_embed_rowopt_sweep's shape, the rows of the regularised,
 *     non-frozen fields only (field_l2 NULL: nothing to do, no launch).  RMSprop with momentum == 0: one launch over every non-frozen
 *     field (field_l2 may be NULL) -- an unregularised field's row reads and writes rms alone (8 bytes per element; p, and anything
 *     else, is not touched), a regularised one takes the full rule (16 bytes per element).  16-byte accesses when K % 4 == 0 and the
 *     arrays are 16-byte aligned, non-temporal stores, F <= 1024.
 *   fil_embed_momopt_merged: fil_embed_rowopt_merged's contract (touched form); W = 1 is bit-identical to fil_embed_momopt_runs on the
 *     same record.  F <= 1024, K <= 256.
 *   The *_lrdev twins read the rate from device memory (lr_dev, one fp32, not NULL), as in O3; fil_momopt_hyper.lr is then ignored.
 */
enum { FIL_OPT_SGD = 3, FIL_OPT_RMSPROP = 4 };
enum { FIL_MOMOPT_NESTEROV = 1 };
typedef struct {
  float lr;
  float epsilon;        /* RMSprop */
  float rho;            /* RMSprop */
  float momentum;       /* 0 = none (no momentum slot) */
  int32_t flags;        /* SGD: FIL_MOMOPT_NESTEROV */
  int32_t reserved;     /* 0 */
} fil_momopt_hyper;     /* 24 bytes */
int fil_momopt_multi(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule, const fil_momopt_hyper* hyper,
                     int advance, void* stream);
int fil_embed_momopt_runs(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                          const float* field_l2, float* table, float* slot0, float* slot1, int32_t* stamp, const int64_t* step, int rule,
                          const fil_momopt_hyper* hyper, void* stream);
int fil_embed_momopt_sweep(float* table, float* slot0, float* slot1, const int32_t* stamp, int64_t V, int K, const int64_t* offsets,
                           const float* field_l2, const unsigned char* frozen, int F, const int64_t* step, int rule,
                           const fil_momopt_hyper* hyper, void* stream);
int fil_embed_momopt_merged(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K, const int64_t* offsets,
                            const float* field_l2, int F, float* table, float* slot0, float* slot1, int32_t* stamp, int64_t V,
                            const int64_t* step, int rule, const fil_momopt_hyper* hyper, void* stream);
int fil_momopt_multi_lrdev(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule,
                           const fil_momopt_hyper* hyper, const float* lr_dev, int advance, void* stream);
int fil_embed_momopt_runs_lrdev(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                const float* field_l2, float* table, float* slot0, float* slot1, int32_t* stamp, const int64_t* step,
                                int rule, const fil_momopt_hyper* hyper, const float* lr_dev, void* stream);
int fil_embed_momopt_sweep_lrdev(float* table, float* slot0, float* slot1, const int32_t* stamp, int64_t V, int K, const int64_t* offsets,
                                 const float* field_l2, const unsigned char* frozen, int F, const int64_t* step, int rule,
                                 const fil_momopt_hyper* hyper, const float* lr_dev, void* stream);
int fil_embed_momopt_merged_lrdev(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                  const int64_t* offsets, const float* field_l2, int F, float* table, float* slot0, float* slot1,
                                  int32_t* stamp, int64_t V, const int64_t* step, int rule, const fil_momopt_hyper* hyper,
                                  const float* lr_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * O5  Keras-exact Adadelta and Adamax (TF 2.1 keras/optimizer_v2/adadelta.py, adamax.py -> ApplyAdadelta / SparseApplyAdadelta,
 *     ApplyAdaMax and adamax.py's Python for IndexedSlices), every tensor fp32, `rule` FIL_OPT_ADADELTA or FIL_OPT_ADAMAX,
 *     hyper-parameters in a fil_adaopt_hyper read ON THE HOST at the call (a captured graph keeps the values it was captured with).
 *     Entry points added only: the ABI version stays.  Every operation rounds to fp32 in the order written (no fused multiply-add;
 *     correctly rounded division and square root; 1 - rho and 1 - beta_1 formed once in fp32):
 *       Adadelta  dense and touched rows   ag = ag*rho + (g*g)*(1 - rho);  upd = (sqrt(av + epsilon)*(1 / sqrt(ag + epsilon)))*g;
 *                                          p = p - upd*lr;  av = av*rho + (upd*upd)*(1 - rho)       accum_grad in slot0, accum_var in slot1
 *       Adamax    dense rows      m += (g - m)*(1 - beta_1);  v = max(beta_2*v, |g|);  p -= c*(m / (v + epsilon))       m in slot0, v in slot1
 *                 touched rows    m = m*beta_1 + g*(1 - beta_1);  v = max(v*beta_2, |g|);  p += (-c)*(m / (v + epsilon))
 *                 c = lr / (1 - powf(beta_1, (float)(*step + 1))), computed ON THE DEVICE once per kernel from the step counter and the
 *                 step's rate (lr, or *lr_dev in the _lrdev twins): a captured step takes each replay's coefficient.  powf is the
 *                 device's, so Adamax is Keras-exact within optim.Adam's bars, not bit-exact; Adadelta reads no step and is bit-exact.
 *     slot0 lives in the `m` array of fil_adam_tensor, slot1 in `v`; both rules need both (FIL_ERR_ARG for a NULL one).
 *     Requires lr, epsilon >= 0; Adadelta rho in [0, 1]; Adamax beta_1, beta_2 in [0, 1) (FIL_ERR_ARG otherwise).
 *   Which rows Keras updates: both rules are row-local, exactly as O2 -- a touched row takes the touched form with g = run sum +
 *     2 emb_reg p; an untouched row of a field with emb_reg > 0 takes the DENSE form with g = 2 emb_reg p; every other row and its slots
 *     keep their bits; a frozen field never changes.
 *   fil_adaopt_multi / fil_embed_adaopt_runs / fil_embed_adaopt_sweep / fil_embed_adaopt_merged: the contracts, argument lists and
 *     errors of their fil_momopt_* counterparts (O4) with these rules: the sweep walks the regularised, non-frozen fields only
 *     (field_l2 NULL: nothing to do, no launch); W = 1 merged is bit-identical to runs on the same record; F <= 1024, K <= 256
 *     (FIL_ERR_UNSUPPORTED otherwise); R = 0, V = 0 or cap = 0 return FIL_OK before any pointer is looked at.
 *   The *_lrdev twins read the rate from device memory (lr_dev, one fp32, not NULL), as in O3; fil_adaopt_hyper.lr is then ignored.
 */
enum { FIL_OPT_ADADELTA = 5, FIL_OPT_ADAMAX = 6 };
typedef struct {
  float lr;
  float rho;            /* Adadelta */
  float beta_1;         /* Adamax */
  float beta_2;         /* Adamax */
  float epsilon;
} fil_adaopt_hyper;     /* 20 bytes */
int fil_adaopt_multi(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule, const fil_adaopt_hyper* hyper,
                     int advance, void* stream);
int fil_embed_adaopt_runs(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                          const float* field_l2, float* table, float* slot0, float* slot1, int32_t* stamp, const int64_t* step, int rule,
                          const fil_adaopt_hyper* hyper, void* stream);
int fil_embed_adaopt_sweep(float* table, float* slot0, float* slot1, const int32_t* stamp, int64_t V, int K, const int64_t* offsets,
                           const float* field_l2, const unsigned char* frozen, int F, const int64_t* step, int rule,
                           const fil_adaopt_hyper* hyper, void* stream);
int fil_embed_adaopt_merged(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K, const int64_t* offsets,
                            const float* field_l2, int F, float* table, float* slot0, float* slot1, int32_t* stamp, int64_t V,
                            const int64_t* step, int rule, const fil_adaopt_hyper* hyper, void* stream);
int fil_adaopt_multi_lrdev(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule,
                           const fil_adaopt_hyper* hyper, const float* lr_dev, int advance, void* stream);
int fil_embed_adaopt_runs_lrdev(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                                const float* field_l2, float* table, float* slot0, float* slot1, int32_t* stamp, const int64_t* step,
                                int rule, const fil_adaopt_hyper* hyper, const float* lr_dev, void* stream);
int fil_embed_adaopt_sweep_lrdev(float* table, float* slot0, float* slot1, const int32_t* stamp, int64_t V, int K, const int64_t* offsets,
                                 const float* field_l2, const unsigned char* frozen, int F, const int64_t* step, int rule,
                                 const fil_adaopt_hyper* hyper, const float* lr_dev, void* stream);
int fil_embed_adaopt_merged_lrdev(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                                  const int64_t* offsets, const float* field_l2, int F, float* table, float* slot0, float* slot1,
                                  int32_t* stamp, int64_t V, const int64_t* step, int rule, const fil_adaopt_hyper* hyper,
                                  const float* lr_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * O6  Keras-exact Nadam (TF 2.1 keras/optimizer_v2/nadam.py), every tensor fp32, `rule` FIL_OPT_NADAM, hyper-parameters in a
 *     fil_nadam_hyper read ON THE HOST at the call (a captured graph keeps the values it was captured with, the m_cache pointer too).
 *     Entry points added only: the ABI version stays.  Every operation rounds to fp32 in the order written (no fused multiply-add;
 *     correctly rounded division and square root).  Per step, computed ON THE DEVICE once per kernel from the step counter and the
 *     momentum cache, with it = *step, t = (float)(it + 1), n = (float)(it + 2), sd = schedule_decay, cache = *m_cache (one fp32 word on
 *     the device, 1.0 before the first step):
 *       mt   = beta_1*(1 - 0.5*powf(0.96f, sd*t))       mt1 = beta_1*(1 - 0.5*powf(0.96f, sd*n))       msn = cache*mt      msx = msn*mt1
 *       omm  = 1 - mt;  omsn = 1 - msn;  omsx = 1 - msx;  vden = 1 - powf(beta_2, t);  omb1 = 1 - beta_1;  omb2 = 1 - beta_2
 *     and per element, with gradient g:
 *       gp = g / omsn;  m = beta_1*m + omb1*g;  mp = m / omsx;  v = beta_2*v + omb2*(g*g);  vp = v / vden        m in slot0, v in slot1
 *       mbar = omm*gp + mt1*mp;  p = p - (lr*mbar) / (sqrt(vp) + epsilon)
 *     Keras' dense form and its IndexedSlices form round to the same bits (the products commute, and p + (-lr*mbar)/d == p -
 *     (lr*mbar)/d), so there is ONE form.  powf is the device's: Keras-exact within optim.Adam's bars, bit-exact in m and v, and
 *     fully bit-exact once both powers have left the coefficients (large t).  lr is the plain hyper-parameter: Keras' Nadam applies no
 *     decay and takes no schedule, so there are no _lrdev twins.
 *     Requires m_cache != NULL, reserved == 0, lr, epsilon, schedule_decay >= 0, beta_1 and beta_2 in [0, 1), both slots
 *     (FIL_ERR_ARG otherwise, a NaN included).
 *   Which rows Keras updates: m = m*beta_1 and v = v*beta_2 are assigned over the WHOLE variable, the batch's rows are scattered, so
 *     (as RMSprop with momentum == 0, O4) a touched row takes the rule with g = run sum + 2 emb_reg p; an untouched row of a field
 *     with emb_reg > 0 takes it with g = 2 emb_reg p; an untouched row of an unregularised field gets m *= beta_1, v *= beta_2 and
 *     keeps the bits of p; a frozen field never changes.
 *   fil_nadam_multi / fil_embed_nadam_runs / fil_embed_nadam_sweep / fil_embed_nadam_merged: the contracts, argument lists and errors
 *     of their fil_momopt_* counterparts (O4): the sweep walks every non-frozen field and launches even when field_l2 is NULL; W = 1
 *     merged is bit-identical to runs on the same record; F <= 1024, K <= 256 (FIL_ERR_UNSUPPORTED otherwise); R = 0, V = 0 or cap = 0
 *     return FIL_OK before any pointer is looked at.  Every launch reads *m_cache and *step; fil_nadam_multi(advance = 1) ends with
 *     ONE one-thread launch that writes *m_cache = *m_cache * mt(it) and then *step = it + 1 (with n = 0 it is the only launch).
 */
enum { FIL_OPT_NADAM = 7 };
typedef struct {
  float lr;
  float beta_1;
  float beta_2;
  float epsilon;
  float schedule_decay;
  int32_t reserved;     /* 0 */
  float* m_cache;       /* device, one fp32: the momentum cache (the product of the completed steps' mt) */
} fil_nadam_hyper;      /* 32 bytes */
int fil_nadam_multi(const fil_adam_tensor* tensors, int n, int64_t total_numel, int64_t* step, int rule, const fil_nadam_hyper* hyper,
                    int advance, void* stream);
int fil_embed_nadam_runs(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                         const float* field_l2, float* table, float* slot0, float* slot1, int32_t* stamp, const int64_t* step, int rule,
                         const fil_nadam_hyper* hyper, void* stream);
int fil_embed_nadam_sweep(float* table, float* slot0, float* slot1, const int32_t* stamp, int64_t V, int K, const int64_t* offsets,
                          const float* field_l2, const unsigned char* frozen, int F, const int64_t* step, int rule,
                          const fil_nadam_hyper* hyper, void* stream);
int fil_embed_nadam_merged(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K, const int64_t* offsets,
                           const float* field_l2, int F, float* table, float* slot0, float* slot1, int32_t* stamp, int64_t V,
                           const int64_t* step, int rule, const fil_nadam_hyper* hyper, void* stream);

/* ---------------------------------------------------------------------------------------------
 * O7  Keras' Adam(amsgrad=True) (TF 2.1 keras/optimizer_v2/adam.py with amsgrad -> ApplyAdamWithAmsgrad; restated, parity with
 *     TensorFlow unpinned), every tensor fp32.  Entry points added only: the ABI version stays.  O1's rule with a third slot `vhat`
 *     (zeros to begin with), the running maximum of v, in the denominator:
 *       t = *step + 1;  alpha = lr * sqrt(1 - b2^t) / (1 - b1^t)                    (as O1: powf on the device from the counter)
 *       m += (g - m) * (1 - beta_1);  v += (g*g - v) * (1 - beta_2)
 *       vhat = (vhat < v) ? v : vhat                                                (Eigen's cwiseMax order: a NaN v leaves vhat)
 *       p -= (m * alpha) / (sqrt(vhat) + epsilon)
 *   The rate: every entry point takes `lr` by value AND `const float* lr_dev`; lr_dev != NULL is the device word of
 *     fil_lr_schedule_eval (O3), read by the launch, and lr is then ignored; lr_dev == NULL takes lr.  There are no _lrdev twins.
 *     Requires lr (when used), epsilon >= 0 and betas in [0, 1) (FIL_ERR_ARG otherwise, a NaN included).  step: O1's counter; only
 *     fil_amsgrad_multi(advance = 1) moves it, in a one-thread launch behind its update.
 *   Which rows Keras updates: its sparse apply decays m and v over the WHOLE variable, takes the maximum over the whole variable and
 *     moves every row (as O1's FIL_ADAM_KERAS): a touched row takes g = run sum + 2 field_l2[f] p, an untouched row g = 2 field_l2[f] p
 *     (0 without l2: m and v decay, vhat keeps its bits, p still moves by m alpha / (sqrt(vhat) + epsilon)), a frozen field never
 *     changes.  There is no lazy and no deferred mode.  The table kernels form m and v through the helpers of O1's table kernels, so
 *     the table m and v are bit-identical to O1's on the same gradients.
 *   fil_amsgrad_multi: fil_adam_multi's contract over fil_amsgrad_tensor descriptors (a DEVICE array of n entries): grad NULL = a
 *     zero gradient; l2 != 0 adds 2 * l2 * p; 16-byte accesses where all FIVE arrays of a descriptor are 16-byte aligned, element-wise
 *     otherwise and in the tail; n = 0 with advance = 1 only advances the counter.
 *   fil_embed_amsgrad_runs: fil_embed_adam_runs in FIL_ADAM_KERAS mode with vhat [V, K]: the same run sums, every updated row stamped
 *     (stamp [V] int32 is required).  R = 0 returns FIL_OK before any pointer is looked at; a NULL table, m, v, vhat, stamp or step is
 *     FIL_ERR_ARG before any launch.  K <= 256.
 *   fil_embed_amsgrad_sweep: every row not stamped with the current t, of every non-frozen field, takes the update with
 *     g = 2 * field_l2[f] * p (field_l2 may be NULL; the sweep always runs: v decays on every row).  One read and one non-temporal
 *     write of p, m, v, vhat and a read of stamp per row: 32 bytes per element; the write of vhat is skipped where it would store the
 *     bits that were read (every untouched row of an unregularised field: 28 bytes per element).  16-byte accesses when K % 4 == 0
 *     and the four arrays are 16-byte aligned, element-wise otherwise.  F <= 1024; V = 0 returns FIL_OK.
 *   fil_embed_amsgrad_merged: fil_embed_adam_merged in FIL_ADAM_KERAS mode with vhat: every row of the union of the W gathered lists
 *     of fil_embed_runs_compact updated once, by its owner, contributions summed in list order; W = 1 is bit-identical to
 *     fil_embed_amsgrad_runs on the same record.  F <= 1024, K <= 256; cap = 0 or V = 0 returns FIL_OK.
 *   Nothing allocates, synchronises or sizes a launch by data: the step captures.
 */
typedef struct {
  float* param;
  const float* grad;   /* NULL = zero gradient */
  float* m;
  float* v;
  float* vhat;
  int64_t numel;
  float l2;            /* g += 2 * l2 * param; 0 = none */
  int32_t reserved;    /* 0 */
} fil_amsgrad_tensor;  /* 56 bytes */
int fil_amsgrad_multi(const fil_amsgrad_tensor* tensors, int n, int64_t total_numel, int64_t* step, float lr, const float* lr_dev,
                      float beta_1, float beta_2, float epsilon, int advance, void* stream);
int fil_embed_amsgrad_runs(const void* g, const int64_t* perm, const int64_t* sorted_ids, long R, int K, int g_dtype, int F,
                           const float* field_l2, float* table, float* m, float* v, float* vhat, int32_t* stamp, const int64_t* step,
                           float lr, const float* lr_dev, float beta_1, float beta_2, float epsilon, void* stream);
int fil_embed_amsgrad_sweep(float* table, float* m, float* v, float* vhat, const int32_t* stamp, int64_t V, int K, const int64_t* offsets,
                            const float* field_l2, const unsigned char* frozen, int F, const int64_t* step, float lr, const float* lr_dev,
                            float beta_1, float beta_2, float epsilon, void* stream);
int fil_embed_amsgrad_merged(const int64_t* ids, const float* values, const int64_t* counts, int W, long cap, int K,
                             const int64_t* offsets, const float* field_l2, int F, float* table, float* m, float* v, float* vhat,
                             int32_t* stamp, int64_t V, const int64_t* step, float lr, const float* lr_dev, float beta_1, float beta_2,
                             float epsilon, void* stream);

/* ---------------------------------------------------------------------------------------------
 * M1 Keras' streaming AUC (TF 2.1 keras/metrics.py: AUC; keras/utils/metrics_utils.py: update_confusion_matrix_variables) --
 *     replaces metrics=[tf.keras.metrics.AUC()] of example/ctr_example/un_seq.py:61.  Entry points added only: the ABI version stays.
 *   State: cm [4][T] fp32 = TP | FP | TN | FN per threshold, as Keras keeps them, and one int64 `invalid`.
 *   fil_confusion_update: p, y [n] fp32 (y != 0 is a positive label); thr [T] fp32 ascending (duplicates allowed); for every i
 *     cm[0][i] += #{y != 0, p > thr[i]}, cm[1][i] += #{y == 0, p > thr[i]}, cm[2][i] += #{y == 0, p <= thr[i]},
 *     cm[3][i] += #{y != 0, p <= thr[i]}: the comparison is fp32 p against the STORED fp32 thr[i]; the batch's counts are integers
 *     (per-bucket histograms, integer atomics, a suffix sum), so they do not depend on scheduling, and each state entry then takes
 *     exactly ONE fp32 addition per call (Keras' assign_add: integer-exact below 2^24, an fp32 rounding past it).  Samples with p < 0,
 *     p > 1 or NaN touch no entry and are counted in *invalid (TF fails an assertion there; a captured step cannot raise).
 *     n <= FIL_CONFUSION_ONE_LAUNCH_N is one kernel launch and needs no workspace (workspace may be NULL); larger n is a
 *     partial-histogram launch and a finishing launch with integer partials in the workspace, which needs no initialisation.
 *     2 <= T <= FIL_CONFUSION_MAX_T (FIL_ERR_UNSUPPORTED otherwise), 1 <= n <= 2^24 (so a call's count is exact in fp32; larger inputs
 *     are the caller's loop).  p and y need 4-byte alignment only (16-byte loads where the addresses allow).  Repeats from the same
 *     state on the same inputs are bit-identical.
 *   fil_auc_result: out[0] = AUC.result() of cm in fp32.  curve 0 ROC, 1 PR; summation 0 interpolation, 1 minoring, 2 majoring
 *     (PR + interpolation is Keras' interpolate_pr_auc).  Every division is div_no_nan: an empty or one-class state gives 0.
 *     One small launch, no host round trip.
 */
#define FIL_CONFUSION_MAX_T 2048
#define FIL_CONFUSION_ONE_LAUNCH_N 16384
size_t fil_confusion_workspace_bytes(int n, int T);
int fil_confusion_update(const float* p, const float* y, int n, const float* thr, int T, float* cm, long long* invalid,
                         void* workspace, size_t workspace_bytes, void* stream);
int fil_auc_result(const float* cm, int T, int curve, int summation, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * M2 Keras' Mean and the metrics that are a Mean of a per-sample value (TF 2.1 keras/metrics.py: Reduce / Mean / MeanMetricWrapper;
 *     BinaryCrossentropy, BinaryAccuracy) -- the rest of what model.compile(loss=binary_crossentropy, metrics=[...]) reports per batch.
 *     Entry points added only: the ABI version stays.  (Precision and Recall are fil_confusion_update with their own thresholds.)
 *   State: state [3] fp32 = total | count | result.
 *   fil_mean_update: a [n] fp32 and, except for FIL_MEAN_VALUES, y [n] fp32.  With v[i] as the kind defines it below,
 *     state[0] += sum_i v[i] and state[1] += (float)n, each ONE fp32 addition (Keras' assign_add: the count is integer-exact below
 *     2^24 and rounds past it), and state[2] = div_no_nan(state[0], state[1]) (the correctly rounded quotient, 0 for a zero count) is
 *     written by the same launch: reading the result costs nothing.
 *       FIL_MEAN_VALUES      v[i] = a[i]                                         (y may be NULL; c0, c1 unused)
 *       FIL_MEAN_BCE         ys = c1 != 0 ? y[i] (1 - c1) + 0.5 c1 : y[i],  pc = clip(a[i], c0, 1 - c0),
 *                            v[i] = -(ys log(pc + c0) + (1 - ys) log(1 - pc + c0))    c0 = epsilon (Keras: 1e-7), c1 = label_smoothing;
 *                            every operation fp32, in this order, none fused (fil_bce_mean_fwd's per-sample expression)
 *       FIL_MEAN_BINARY_ACC  v[i] = (y[i] == (a[i] > c0 ? 1.f : 0.f)) ? 1 : 0      c0 = threshold; a strict >, and a label that is
 *                            neither 0 nor 1 never matches; counted in integers, converted once
 *     NaN and infinity are not filtered: a NaN value makes total and result NaN, and they stay NaN (Keras asserts no range here).
 *     The sum's order is fixed by n and the addresses' alignment alone -- per-thread sums, a fixed fold inside each wave, the waves in
 *     wave order, the workgroups' partials by the same fold; no floating-point atomics -- so repeats from the same state on the same
 *     inputs are bit-identical.  n <= FIL_MEAN_ONE_LAUNCH_N is one kernel launch and needs no workspace (workspace may be NULL);
 *     larger n is a partial launch of at most 256 workgroups and a one-workgroup finishing launch, with one 4-byte partial per
 *     workgroup in the workspace, which needs no initialisation.  1 <= n <= 2^24 (larger inputs are the caller's loop).  a, y and
 *     state need 4-byte alignment only (16-byte loads where the addresses allow).
 */
#define FIL_MEAN_VALUES 0
#define FIL_MEAN_BCE 1
#define FIL_MEAN_BINARY_ACC 2
#define FIL_MEAN_ONE_LAUNCH_N 16384
size_t fil_mean_workspace_bytes(int n);
int fil_mean_update(int kind, const float* a, const float* y, int n, float c0, float c1, float* state, void* workspace,
                    size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FIL_H_ */
