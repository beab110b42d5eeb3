"""The dense layers' two hand-written pieces at CONSTRUCTED edges: fil_gemm_f32 (csrc/gemm.hip: gemm_f32_kernel<TA, TB, BN, KW>, 16
instantiations, and gemm_splitk_sum_kernel) and fil_relu_bias_bwd (csrc/head.hip: relu_bias_bwd_kernel<T, VEC>, 4 instantiations, and
block_partials_sum_kernel), called through the C ABI with padded leading dimensions, poisoned padding and guarded outputs.

Sections 1, 3 and 4 need no tolerance.  GEMM operands are integers in [-8, 8] \\ {0} and the bias an integer in [-64, 64]: a product is at
most 64 and with K <= 4096 every partial sum stays below 2^24, so fp32 MFMA accumulation is exact in ANY order -- with or without the
split over k and the join of the two k halves (KW = 2) -- and C must equal the int64 product (+ bias, ReLU) bit for bit; a dropped,
doubled or misplaced k term, row or column moves an element by at least 1.  (The int64 product is evaluated as a float64 BLAS product of
the same integers: every partial sum is an integer below 2^53, so that is the int64 product, and one case checks it against numpy's
int64 matmul.)  dy of the ReLU backward holds integers in [-64, 64] \\ {0}, exact in bf16 and fp32, and B * 64 < 2^24.  The only inexact
comparisons are the textbook gamma(n) bounds of fp32 summation in section 2 and at the end of section 3, asserted per element.

Every operand lives inside a larger allocation: ld = the tight value + a pad from {0, 1, 3, 4, 5}, all padding (the last row's too, and
8 words behind it) holds the payload NaN 0x7FC12345, C is sentinel-filled with two guard rows of ldc words in front and behind, and
after the call every word of the C allocation outside C[:M, :N] must still hold the sentinel's bits.  The workspace is exactly
fil_gemm_f32_workspace_bytes long, in front of a guard that must be unchanged.

Which path a case reaches (restated from gemm_bn / gemm_splits):
    tiles64 = cdiv(M, 64) cdiv(N, 64);   BN = 64 if tiles64 >= 192 else 32;   tiles = cdiv(M, 64) cdiv(N, BN)
    split over k  <=>  epilogue == 0 and K >= 512 and tiles < 192:  want = min(16, max(1, 768 // tiles)),
                       kchunk = 32 cdiv(cdiv(K, want), 32), slices = cdiv(K, kchunk)     (observable: workspace_bytes > 0)
    a launch has 8 cdiv(tiles, 8) workgroups; those whose tile index is >= tiles return at once
    KW = 2 unless FIL_GEMM_KW=1 (read once per process): tests/test_gpu_knobs.py::test_gemm_edges_with_one_wave_per_tile runs the
    tests named *gemm_bn64*, *gemm_splitk* and the `kw1` slice of *gemm_bn32* in a child with that setting

    kernel instantiation                              case
    gemm_f32_kernel<ta, tb, 64, 2>  (4 of them)       test_gemm_bn64_equals_the_int64_product[ta-tb-*]  (769 x 899: 195 tiles, ragged M and
                                                      N, N % 4 = 3, 5 idle workgroups;  832 x 1024: 208 tiles, no edge, none idle)
    gemm_f32_kernel<ta, tb, 32, 2>  (4)               test_gemm_bn32_equals_the_int64_product[ta-tb-*], test_gemm_splitk_...[ta-tb-*]
    gemm_f32_kernel<ta, tb, 64, 1>  (4)               the same bn64 tests in the FIL_GEMM_KW=1 child
    gemm_f32_kernel<ta, tb, 32, 1>  (4)               the same splitk tests and the kw1 slice of the bn32 tests in that child
    gemm_splitk_sum_kernel                            test_gemm_splitk_equals_the_int64_product (1, 9, 100 tiles: want 16, 16, 7)
    relu_bias_bwd_kernel<float, true>                 test_relu_bias_bwd_equals_the_int64_sums[f32-N], N in VEC_N (N % 4 == 0, N <= 1024)
    relu_bias_bwd_kernel<float, false>                ...[f32-N], N in COL_N
    relu_bias_bwd_kernel<__hip_bfloat16, true>        ...[bf16-N], N in VEC_N
    relu_bias_bwd_kernel<__hip_bfloat16, false>       ...[bf16-N], N in COL_N
    block_partials_sum_kernel                         every B of RELU_B: 1, 1, 1, 1, 2, 7, 8, 9, 16, 17 block partials (unrolled by 8 + tail)
"""
import functools

import numpy as np
import pytest
import torch

from ml_function_amd import _lib
from ml_function_amd import functional as Fn
from ml_function_amd._lib import FIL_BF16, FIL_F32, check, ptr, stream_ptr

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC12345                      # a quiet NaN with a payload: compared as bits (operand padding and untouched outputs)
GUARD_ROWS = 2
TAIL = 8                                   # words behind the last row's padding
WS_GUARD = 256                             # bytes behind the workspace
WS_FILL = 0xA5
TRANS = [(0, 0), (0, 1), (1, 0), (1, 1)]
TRANS_IDS = ["nn", "nt", "tn", "tt"]
PADS = [0, 1, 3, 4, 5]
U24 = 2.0 ** -24


def gamma(m):
    return m * U24 / (1.0 - m * U24)


def cdiv(a, b):
    return (a + b - 1) // b


def gemm_path(M, N, K, epi):
    """(BN, tiles, slices) as gemm_bn / gemm_splits / fil_gemm_f32 choose them."""
    bn = 64 if cdiv(M, 64) * cdiv(N, 64) >= 192 else 32
    tiles = cdiv(M, 64) * cdiv(N, bn)
    if epi != 0 or tiles >= 192 or K < 512:
        return bn, tiles, 1
    want = min(16, max(1, 768 // tiles))
    kchunk = cdiv(cdiv(K, want), 32) * 32
    return bn, tiles, cdiv(K, kchunk)


def nonzero_ints(rng, shape, hi):
    return (rng.integers(1, hi + 1, size=shape) * rng.choice(np.array([-1, 1]), size=shape)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def int_case(M, N, K):
    """Logical A [M, K], B [K, N] (int8, in [-8, 8] \\ {0}), bias [N] (in [-64, 64]) and the product A B (int32); shared by every
    transposition and epilogue of the shape and read-only."""
    rng = np.random.default_rng(1000003 * M + 1009 * N + K)
    A, B = nonzero_ints(rng, (M, K), 8), nonzero_ints(rng, (K, N), 8)
    bias = rng.integers(-64, 65, size=N).astype(np.int64)
    AB = np.rint(A.astype(np.float64) @ B.astype(np.float64)).astype(np.int64)      # integers below 2^53: exact in any order
    assert K * 64 < 2 ** 24 and np.abs(AB).max(initial=0) + 64 < 2 ** 24
    out = (A.astype(np.int8), B.astype(np.int8), bias, AB.astype(np.int32))
    for a in out:
        a.setflags(write=False)
    return out


def epilogue(AB, bias, epi):
    want = AB.astype(np.int64) + (bias[None, :] if epi >= 1 else 0)
    return np.maximum(want, 0) if epi == 2 else want


def padded_operand(stored, pad, off):
    """stored [R, C] fp32 at `off` words into an allocation, row stride C + pad; everything that is not an element is the payload NaN.
    -> (tensor that owns the memory, device address of element [0][0], ld)"""
    R, C = stored.shape
    ld = C + pad
    buf = np.full(off + R * ld + TAIL, SENTINEL, np.uint32)
    if R and C:
        buf[off:off + R * ld].reshape(R, ld)[:, :C] = np.ascontiguousarray(stored, dtype=np.float32).view(np.uint32)
    t = torch.from_numpy(buf.view(np.int32)).cuda()
    return t, t.data_ptr() + 4 * off, ld


def launch_gemm(A, B, bias, epi, ta, tb, pads=(0, 0, 0), offs=(0, 0, 0), operands="allocated", ld_null=(0, 0), expect_split=None):
    """fil_gemm_f32 on logical A [M, K], B [K, N] (fp32 arrays) -> the bits of C[:M, :N].  Checked here: the return code, whether the
    shape splits (workspace_bytes > 0), every word of the C allocation outside C[:M, :N], the workspace's guard.
    operands = "null": A = B = NULL with leading dimensions ld_null = (lda, ldb) (K must be 0)."""
    lib = _lib.load()
    (M, K), N = A.shape, B.shape[1]
    assert B.shape[0] == K
    if operands == "null":
        assert K == 0
        ta_t = tb_t = None
        pa = pb = None
        lda, ldb = ld_null
    else:
        ta_t, pa, lda = padded_operand(A.T if ta else A, pads[0], offs[0])
        tb_t, pb, ldb = padded_operand(B.T if tb else B, pads[1], offs[1])
    ldc = N + pads[2]
    c0 = offs[2] + GUARD_ROWS * ldc
    cbuf = torch.full((offs[2] + (M + 2 * GUARD_ROWS) * ldc + TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
    bias_t = torch.tensor(np.asarray(bias, np.float32), device="cuda") if epi >= 1 else None
    nws = lib.fil_gemm_f32_workspace_bytes(M, N, K)
    slices = gemm_path(M, N, K, 0)[2]
    assert (nws > 0) == (slices > 1) and (slices == 1 or nws >= slices * M * N * 4), (M, N, K, nws, slices)
    if expect_split is not None:
        assert (nws > 0) == expect_split, "M=%d N=%d K=%d: workspace_bytes = %d" % (M, N, K, nws)
    # a call with an epilogue never splits: it gets NO workspace, and has to succeed without one
    ws = torch.full((nws + WS_GUARD,), WS_FILL, dtype=torch.uint8, device="cuda") if nws and epi == 0 else None
    rc = lib.fil_gemm_f32(pa, pb, cbuf.data_ptr() + 4 * c0, ptr(bias_t), M, N, K, lda, ldb, ldc, ta, tb, epi, ptr(ws), nws if ws is not None else 0,
                          stream_ptr())
    assert rc == 0, (rc, lib.fil_last_error())
    bits = cbuf.cpu().numpy().view(np.uint32)
    if ws is not None:
        assert (ws[nws:].cpu().numpy() == WS_FILL).all(), "M=%d N=%d K=%d: a store behind the workspace's %d bytes" % (M, N, K, nws)
    body = bits[c0:c0 + M * ldc].reshape(M, ldc)
    got = body[:, :N].copy()
    outside = bits != SENTINEL
    outside[c0:c0 + M * ldc].reshape(M, ldc)[:, :N] = False
    stray = np.nonzero(outside)[0]
    assert stray.size == 0, "M=%d N=%d K=%d ldc=%d ta=%d tb=%d epi=%d: %d words outside C[:M, :N] were written, first (row, col) %s" % (
        M, N, K, ldc, ta, tb, epi, stray.size, [divmod(int(w) - c0, ldc) for w in stray[:6]])
    del ta_t, tb_t
    return got


def assert_bits(got, want_int, what):
    want = want_int.astype(np.float32).view(np.uint32)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d of %d elements differ, first (row, col) %s: got %s want %s" % (
        what, len(bad), got.size, bad[:6].tolist(), got.view(np.float32)[tuple(bad[:6].T)], want_int[tuple(bad[:6].T)])


def check_int_gemm(M, N, K, ta, tb, epi, pads, offs=(0, 0, 0), bn=None, split=None):
    A, B, bias, AB = int_case(M, N, K)
    got_bn, _, slices = gemm_path(M, N, K, epi)
    assert bn is None or got_bn == bn
    got = launch_gemm(A.astype(np.float32), B.astype(np.float32), bias, epi, ta, tb, pads, offs,
                      expect_split=None if split is None else (split if epi == 0 else gemm_path(M, N, K, 0)[2] > 1))
    assert split is None or (slices > 1) == split
    assert_bits(got, epilogue(AB, bias, epi), "M=%d N=%d K=%d ta=%d tb=%d epi=%d pads=%s offs=%s (BN=%d, %d slices)" % (
        M, N, K, ta, tb, epi, pads, offs, got_bn, slices))


def pads_of(i):
    """Three pads for case number i: every pad of PADS turns up for every operand, strides that are no multiple of 4 among them."""
    return PADS[i % 5], PADS[(i // 5 + i + 1) % 5], PADS[(i // 25 + 2 * i + 3) % 5]


# ------------------------------------------------------------------------------------------------ 1. fil_gemm_f32, exact
def test_the_float64_product_of_the_integers_is_the_int64_product():
    A, B, _, AB = int_case(65, 33, 129)
    assert np.array_equal(A.astype(np.int64) @ B.astype(np.int64), AB)


BN64_K = [1, 31, 32, 33, 64, 65, 97]       # one stage; an odd and an even stage count (the s + 1 >= nst break); a last stage of one k


@pytest.mark.parametrize("M,N", [(769, 899), (832, 1024)])
@pytest.mark.parametrize("ta,tb", TRANS, ids=TRANS_IDS)
def test_gemm_bn64_equals_the_int64_product(ta, tb, M, N):
    """1a.  BN = 64 (>= 192 tiles of 64 x 64), every epilogue.  769 x 899: 13 x 15 = 195 tiles in 200 workgroups (5 return early), both
    edges ragged, N % 4 = 3;  832 x 1024: 13 x 16 = 208 tiles, no edge, no idle workgroup.  Never split (K < 512)."""
    tiles = cdiv(M, 64) * cdiv(N, 64)
    assert tiles == (195 if M == 769 else 208) and (8 * cdiv(tiles, 8) - tiles) == (5 if M == 769 else 0)
    for i, K in enumerate(BN64_K):
        for epi in (0, 1, 2):
            check_int_gemm(M, N, K, ta, tb, epi, pads_of(3 * i + epi + 2 * ta + tb), bn=64, split=False)


BN32_SIZES = [1, 31, 32, 33, 63, 64, 65, 129]
BN32_K = [1, 3, 31, 32, 33, 63, 64, 65, 96, 97, 129]
BN32_MN = [(BN32_SIZES[i], BN32_SIZES[(i + s) % 8]) for s in (0, 3) for i in range(8)]      # M and N each take every size, twice


@pytest.mark.parametrize("M,N", BN32_MN, ids=["%dx%d%s" % (m, n, "-kw1" if j % 3 == 0 else "") for j, (m, n) in enumerate(BN32_MN)])
@pytest.mark.parametrize("ta,tb", TRANS, ids=TRANS_IDS)
def test_gemm_bn32_equals_the_int64_product(ta, tb, M, N):
    """1b.  BN = 32 (64 x 32 tiles, 2 waves per k half): one to nine tiles, ragged in M, in N, in both or in neither; K of one to five
    stages with a last stage of 1, 3, 31, 32 k.  The epilogue rotates with K.  Never split."""
    j = BN32_MN.index((M, N))
    for i, K in enumerate(BN32_K):
        check_int_gemm(M, N, K, ta, tb, (i + j) % 3, pads_of(11 * j + i + 2 * ta + tb), bn=32, split=False)


SPLIT_MN = [(33, 31), (129, 95), (601, 299)]        # 1, 9, 100 tiles of 64 x 32: want = 16, 16, 7
SPLIT_K = [512, 513, 545, 1000, 4096]


@pytest.mark.parametrize("M,N", SPLIT_MN)
@pytest.mark.parametrize("ta,tb", TRANS, ids=TRANS_IDS)
def test_gemm_splitk_equals_the_int64_product(ta, tb, M, N):
    """1c.  Split over k (epilogue 0, K >= 512, < 192 tiles): K = 512 -> 16 slices of one stage; 513 -> 9 slices, the last one k wide;
    545 -> a last slice of 33 = two stages, the second one k wide (at 1 and 9 tiles).  The same shapes with epilogue 1 get no workspace:
    they must not split and give the same integers + bias.  K = 511 does not split."""
    tiles = gemm_path(M, N, 512, 0)[1]
    assert tiles == {33: 1, 129: 9, 601: 100}[M] and min(16, 768 // tiles) == (7 if M == 601 else 16)
    if tiles < 100:
        assert [gemm_path(M, N, K, 0)[2] for K in (512, 513, 545)] == [16, 9, 9]
    for i, K in enumerate(SPLIT_K):
        check_int_gemm(M, N, K, ta, tb, 0, pads_of(i + M + 2 * ta + tb), bn=32, split=True)
        check_int_gemm(M, N, K, ta, tb, 1, pads_of(i + M + 2 * ta + tb + 7), bn=32, split=False)
    check_int_gemm(M, N, 511, ta, tb, 0, pads_of(M + ta), bn=32, split=False)


@pytest.mark.parametrize("ta,tb", TRANS, ids=TRANS_IDS)
def test_gemm_misaligned_bases(ta, tb):
    """1d.  A, B and C start 1, 2 and 3 floats (in every rotation) into their allocations -- dword-aligned, not 16-byte-aligned -- with
    padded strides on top: a BN = 64 shape, a BN = 32 shape and a split one."""
    for r, offs in enumerate([(1, 2, 3), (2, 3, 1), (3, 1, 2)]):
        for epi in (0, 2):
            check_int_gemm(769, 899, 33 if r else 97, ta, tb, epi, pads_of(r + epi), offs, bn=64, split=False)
            check_int_gemm(65, 33, 129, ta, tb, epi, pads_of(r + epi + 1), offs, bn=32, split=False)
            check_int_gemm(129, 95, 545, ta, tb, epi, pads_of(r + epi + 2), offs, bn=32, split=(epi == 0))


@pytest.mark.parametrize("ta,tb", TRANS, ids=TRANS_IDS)
def test_gemm_f32_of_a_row_slice_of_an_odd_width_tensor(ta, tb):
    """1d.  functional.gemm_f32 on big[1:] of tensors with an odd row width: contiguous, and its base is an odd number of floats into the
    allocation -- the form a caller would pass."""
    M, N, K = 65, 33, 129
    A, B, bias, AB = int_case(M, N, K)
    sa, sb = (A.T if ta else A), (B.T if tb else B)
    assert sa.shape[1] % 2 == 1 and sb.shape[1] % 2 == 1
    big_a = torch.full((sa.shape[0] + 1, sa.shape[1]), float("nan"), device="cuda")
    big_b = torch.full((sb.shape[0] + 1, sb.shape[1]), float("nan"), device="cuda")
    big_a[1:] = torch.tensor(sa.astype(np.float32))
    big_b[1:] = torch.tensor(sb.astype(np.float32))
    a, b = big_a[1:], big_b[1:]
    assert a.is_contiguous() and b.is_contiguous() and a.data_ptr() % 16 == 4 and b.data_ptr() % 16 == 4
    for epi in (0, 1, 2):
        c = Fn.gemm_f32(a, b, trans_a=bool(ta), trans_b=bool(tb), bias=torch.tensor(bias.astype(np.float32), device="cuda") if epi else None,
                        relu=epi == 2)
        assert_bits(c.cpu().numpy().view(np.uint32), epilogue(AB, bias, epi), "gemm_f32(big[1:]) ta=%d tb=%d epi=%d" % (ta, tb, epi))


@pytest.mark.parametrize("operands", ["allocated-ld>0", "null-ld=tight", "null-ld>0"])
@pytest.mark.parametrize("ta,tb", TRANS, ids=TRANS_IDS)
def test_gemm_k_zero_is_the_epilogue_alone(ta, tb, operands):
    """1g.  K = 0: C = 0, bias or ReLU(bias), its padding untouched -- with allocated operands behind ld > 0 (all of them the payload
    NaN), with NULL operands and the tight ld (what functional.gemm_f32 passes: 0 for an operand that is contiguous along k, M or N for one
    that is not), and with NULL operands behind ld = tight + 3 > 0, which the launcher has to keep every load away from (it gives both
    operands zero-byte resources)."""
    for j, (M, N) in enumerate([(65, 33), (769, 899), (1, 1)]):
        A, B = np.zeros((M, 0), np.float32), np.zeros((0, N), np.float32)
        bias = np.random.default_rng(M).integers(-64, 65, size=N).astype(np.int64)
        for epi in (0, 1, 2):
            pads = tuple(max(p, 1) for p in pads_of(j + epi))
            if operands == "allocated-ld>0":
                got = launch_gemm(A, B, bias, epi, ta, tb, pads, expect_split=False)
            else:
                got = launch_gemm(A, B, bias, epi, ta, tb, pads, operands="null", expect_split=False,
                                  ld_null=tuple(ld + (3 if operands == "null-ld>0" else 0) for ld in (M if ta else 0, 0 if tb else N)))
            assert_bits(got, epilogue(np.zeros((M, N), np.int64), bias, epi), "K=0 M=%d N=%d ta=%d tb=%d epi=%d %s" % (M, N, ta, tb, epi, operands))


# ------------------------------------------------------------------------------------------------ 2. fil_gemm_f32, real-valued
REAL_SHAPES = [(769, 899, 97), (832, 1024, 33), (65, 33, 129), (129, 95, 545), (601, 299, 1000), (33, 31, 4096)]


@functools.lru_cache(maxsize=None)
def real_case(M, N, K):
    """Standard-normal A [M, K], B [K, N], bias [N] (fp32) with A B and |A| |B| in float64; shared by the transpositions, read-only."""
    rng = np.random.default_rng(2000003 * M + 2003 * N + K)
    A, B = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    out = (A, B, bias, A64 @ B64, np.abs(A64) @ np.abs(B64))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("M,N,K", REAL_SHAPES)
@pytest.mark.parametrize("ta,tb", TRANS, ids=TRANS_IDS)
def test_gemm_real_values_stay_inside_the_fp32_bound_per_element(ta, tb, M, N, K):
    """Standard-normal operands and bias.  For EVERY element |got - want64| <= gamma(K + 20) (|A| |B| + |bias|), gamma(n) = n u / (1 - n u),
    u = 2^-24, |A| |B| in float64: the bound of an fp32 dot product summed in any order (Higham, Accuracy and Stability, section 3.1), the
    + 20 for the slice sum (<= 16 slices), the join of the k halves, the bias add and the final rounding.  ReLU is 1-Lipschitz: the same
    bound.  1e.  A second call into a fresh sentinel buffer gives the same bits (split sums included: slice order is fixed)."""
    A, B, bias, AB, mag = real_case(M, N, K)
    for epi in (0, 1, 2):
        pads = pads_of(M + K + epi + 2 * ta + tb)
        got = launch_gemm(A, B, bias, epi, ta, tb, pads, expect_split=(K >= 512))
        again = launch_gemm(A, B, bias, epi, ta, tb, pads)
        assert np.array_equal(got, again), "M=%d N=%d K=%d epi=%d: a second call changed %d elements" % (M, N, K, epi, (got != again).sum())
        want = AB + (bias.astype(np.float64)[None, :] if epi else 0.0)
        want = np.maximum(want, 0.0) if epi == 2 else want
        bound = gamma(K + 20.0) * (mag + (np.abs(bias.astype(np.float64))[None, :] if epi else 0.0))
        err = np.abs(got.view(np.float32).astype(np.float64) - want)        # (a NaN fails the comparison below)
        print("M=%d N=%d K=%d ta=%d tb=%d epi=%d: max (err / bound) = %.4f" % (M, N, K, ta, tb, epi, np.nanmax(err / bound)))
        bad = np.argwhere(~(err <= bound))
        assert bad.size == 0, "M=%d N=%d K=%d epi=%d: %d elements outside gamma(K + 20) (|A||B| + |bias|), first (row, col) %s" % (
            M, N, K, epi, len(bad), bad[:6].tolist())


# ------------------------------------------------------------------------------------------------ 3. fil_relu_bias_bwd, exact
VEC_N = [4, 8, 12, 200, 256, 260, 512, 516, 1020, 1024]     # N % 4 == 0 and N <= 1024: Q = N / 4 threads per row, 256 % Q idle ones
COL_N = [1, 3, 255, 257, 1026, 1028, 2050]                  # a thread per column: one to nine trips of n += 256
RELU_B = [1, 2, 63, 64, 65, 448, 512, 513, 1024, 1025]      # 1 row; a short last block; 7, 8, 9, 16, 17 block partials
DTYPES = [FIL_F32, FIL_BF16]
DT_IDS = ["f32", "bf16"]
# +0, -0, NaN, -NaN with a payload, -inf, +inf, the smallest positive subnormal, the smallest normal, -1.5, the smallest negative subnormal
SPECIAL = {FIL_F32: [0x00000000, 0x80000000, 0x7FC00000, 0xFFC00001, 0xFF800000, 0x7F800000, 0x00000001, 0x00800000, 0xBFC00000, 0x80000001],
           FIL_BF16: [0x0000, 0x8000, 0x7FC0, 0xFFC1, 0xFF80, 0x7F80, 0x0001, 0x0080, 0xBFC0, 0x8001]}
SPECIAL_POSITIVE = [False, False, False, False, False, True, True, True, False, False]
POOL_ROWS, POOL_COLS = 1025 + 16, 2050 + 32


def storage(dt):
    """(numpy word type, torch word type, torch float type, the sentinel in that width)"""
    return (np.uint32, torch.int32, torch.float32, SENTINEL) if dt == FIL_F32 else (np.uint16, torch.int16, torch.bfloat16, SENTINEL >> 16)


def to_f32(words, dt):
    """The stored words as the fp32 values they stand for."""
    return words.view(np.float32) if dt == FIL_F32 else (words.astype(np.uint32) << 16).view(np.float32)


def to_words(values, dt):
    """fp32 values that are exact in the storage type -> its words."""
    w = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32)
    if dt == FIL_F32:
        return w
    assert not (w & 0xFFFF).any()
    return (w >> 16).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def relu_pool(dt, real=False):
    """One block of y words (random normals, a quarter of them one of SPECIAL) and dy (integers in [-64, 64] \\ {0}; real: normals
    rounded to the storage type) that every case cuts its [B, N] window from; read-only."""
    rng = np.random.default_rng(31 + dt + 2 * real)
    npw = storage(dt)[0]

    def stored_normals():
        t = torch.tensor(rng.standard_normal((POOL_ROWS, POOL_COLS)).astype(np.float32))
        return t.view(torch.int32).numpy().view(np.uint32).copy() if dt == FIL_F32 else t.bfloat16().view(torch.int16).numpy().view(np.uint16).copy()

    y = stored_normals()
    plant = rng.random(y.shape) < 0.25
    y[plant] = np.array(SPECIAL[dt], npw)[rng.integers(0, len(SPECIAL[dt]), size=int(plant.sum()))]
    dy = stored_normals() if real else to_words(nonzero_ints(rng, y.shape, 64).astype(np.float32), dt)
    # the reference's own comparison: a subnormal counts as positive, a NaN and either zero do not
    assert ((to_f32(np.array(SPECIAL[dt], npw), dt) > 0) == np.array(SPECIAL_POSITIVE)).all()
    y.setflags(write=False)
    dy.setflags(write=False)
    return y, dy


def launch_relu_bwd(yw, dyw, dt):
    """fil_relu_bias_bwd on y, dy words [B, N] -> (dz words [B, N], dbias bits [N]); the guards of dz, dbias and the workspace are
    checked here."""
    lib = _lib.load()
    B, N = yw.shape
    npw, tw, _, sent = storage(dt)
    y_t, dy_t = (torch.from_numpy(np.array(a).view(np.int32 if dt == FIL_F32 else np.int16)).cuda() for a in (yw, dyw))
    dz = torch.full(((B + 2 * GUARD_ROWS) * N + TAIL,), sent, dtype=tw, device="cuda")       # (guard rows of N words keep dz's alignment)
    db = torch.full((N + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    nws = lib.fil_relu_bias_bwd_workspace_bytes(B, N)
    assert nws == 256 + cdiv(max(B, 1), 64) * N * 4
    ws = torch.full((nws + WS_GUARD,), WS_FILL, dtype=torch.uint8, device="cuda")
    esz = 4 if dt == FIL_F32 else 2
    check(lib.fil_relu_bias_bwd(ptr(y_t), ptr(dy_t), dz.data_ptr() + GUARD_ROWS * N * esz, db.data_ptr() + 16, B, N, dt, ptr(ws), nws, stream_ptr()),
          "fil_relu_bias_bwd")
    dzw, dbw, wsb = dz.cpu().numpy().view(npw), db.cpu().numpy().view(np.uint32), ws.cpu().numpy()
    what = "B=%d N=%d %s" % (B, N, DT_IDS[dt])
    assert (dzw[:GUARD_ROWS * N] == sent).all() and (dzw[(GUARD_ROWS + B) * N:] == sent).all(), what + ": a store outside dz"
    assert (dbw[:4] == SENTINEL).all() and (dbw[4 + N:] == SENTINEL).all(), what + ": a store outside dbias"
    assert (wsb[nws:] == WS_FILL).all(), what + ": a store behind the workspace"
    if B == 0:
        assert (wsb == WS_FILL).all(), what + ": B = 0 wrote to the workspace"
    return dzw[GUARD_ROWS * N:(GUARD_ROWS + B) * N].reshape(B, N).copy(), dbw[4:4 + N].copy()


def relu_window(dt, B, N, real=False):
    y, dy = relu_pool(dt, real)
    r0, c0 = (7 * B + N) % 16, (3 * B + 5 * N) % 32
    return y[r0:r0 + B, c0:c0 + N], dy[r0:r0 + B, c0:c0 + N]


@pytest.mark.parametrize("N", VEC_N + COL_N)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_relu_bias_bwd_equals_the_int64_sums(dt, N):
    """dz = where(y > 0, dy, +0.0) as bits -- y > 0 evaluated by numpy on the stored values: subnormals are positive, NaN, -0.0 and +0.0 are
    not -- and dbias = the int64 column sums as bits, at every B of RELU_B and B = 0; a second call gives the same bits."""
    assert ((N % 4 == 0) and N <= 1024) == (N in VEC_N)
    npw = storage(dt)[0]
    for B in RELU_B:
        yw, dyw = relu_window(dt, B, N)
        pos = to_f32(np.ascontiguousarray(yw), dt) > 0
        assert B * N < 64 or (pos.any() and not pos.all())
        want_dz = np.where(pos, dyw, npw(0))
        want_db = np.where(pos, to_f32(np.ascontiguousarray(dyw), dt).astype(np.int64), 0).sum(0)
        assert B * 64 < 2 ** 24
        dz, db = launch_relu_bwd(yw, dyw, dt)
        bad = np.argwhere(dz != want_dz)
        assert bad.size == 0, "B=%d N=%d: %d dz words differ, first (row, col) %s, y words %s" % (
            B, N, len(bad), bad[:6].tolist(), [hex(int(v)) for v in np.ascontiguousarray(yw)[tuple(bad[:6].T)]])
        badb = np.nonzero(db != want_db.astype(np.float32).view(np.uint32))[0]
        assert badb.size == 0, "B=%d N=%d: dbias differs at columns %s: got %s want %s" % (
            B, N, badb[:6], db.view(np.float32)[badb[:6]], want_db[badb[:6]])
        if B in (65, 1025):
            dz2, db2 = launch_relu_bwd(yw, dyw, dt)
            assert np.array_equal(dz, dz2) and np.array_equal(db, db2)
    yw, dyw = relu_window(dt, 0, N)
    dz, db = launch_relu_bwd(yw, dyw, dt)                 # B = 0: dbias = 0, nothing else is touched (checked in launch_relu_bwd)
    assert dz.size == 0 and (db == 0).all()


@pytest.mark.parametrize("N", [260, 257])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_relu_bias_bwd_real_sums_stay_inside_the_fp32_bound(dt, N):
    """Real-valued dy (normals, rounded to the storage type), one case per type and path, B = 1025: dz is still dy or +0.0 bit for bit, and
    every dbias[n] lies within gamma(B) sum_b |dz[b, n]| of the float64 column sum (fp32 summation of B terms in any order, the adds to
    the accumulators' zeros included)."""
    B = 1025
    yw, dyw = relu_window(dt, B, N, real=True)
    pos = to_f32(np.ascontiguousarray(yw), dt) > 0
    want_dz = np.where(pos, dyw, storage(dt)[0](0))
    dz, db = launch_relu_bwd(yw, dyw, dt)
    assert np.array_equal(dz, want_dz)
    dz64 = to_f32(want_dz, dt).astype(np.float64)
    err = np.abs(db.view(np.float32).astype(np.float64) - dz64.sum(0))
    bound = gamma(float(B)) * np.abs(dz64).sum(0)
    print("N=%d %s: max (err / bound) = %.4f" % (N, DT_IDS[dt], np.nanmax(err / bound)))
    assert (err <= bound).all(), "N=%d: columns %s outside gamma(B) sum|dz|" % (N, np.nonzero(~(err <= bound))[0][:8])


# ------------------------------------------------------------------------------------------------ 4. through the layer
@pytest.mark.parametrize("B,I,N", [(65, 33, 12), (130, 97, 257)])
@pytest.mark.parametrize("layer", ["dense_relu", "dense"])
def test_dense_layers_equal_the_int64_results(layer, B, I, N):
    """functional.dense_relu / functional.dense in fp32 on integer data: y, dx, dW and db bit-equal to the int64 results (the Python glue
    around the kernels above: leading dimensions, transposes, workspaces)."""
    rng = np.random.default_rng(B + I + N)
    x, W = nonzero_ints(rng, (B, I), 8), nonzero_ints(rng, (I, N), 8)
    b, dy = rng.integers(-64, 65, size=N).astype(np.int64), nonzero_ints(rng, (B, N), 64)
    z = x @ W + b
    y = np.maximum(z, 0) if layer == "dense_relu" else z
    dz = np.where(z > 0, dy, 0) if layer == "dense_relu" else dy
    want = dict(y=y, dx=dz @ W.T, dW=x.T @ dz, db=dz.sum(0))
    assert max(np.abs(v).max() for v in want.values()) < 2 ** 24 and (layer == "dense" or ((z > 0).any() and (z <= 0).any()))
    xt, Wt, bt = (torch.tensor(a.astype(np.float32), device="cuda", requires_grad=True) for a in (x, W, b))
    out = getattr(Fn, layer)(xt, Wt, bt)
    out.backward(torch.tensor(dy.astype(np.float32), device="cuda"))
    got = dict(y=out.detach(), dx=xt.grad, dW=Wt.grad, db=bt.grad)
    for k, w in want.items():
        g = got[k].cpu().numpy()
        assert g.dtype == np.float32 and g.shape == w.shape
        assert_bits(np.ascontiguousarray(g).view(np.uint32), w, "%s (%d, %d, %d): %s" % (layer, B, I, N, k))
