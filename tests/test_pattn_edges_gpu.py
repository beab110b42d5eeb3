"""The stand-alone product attention (csrc/pattn.hip: fil_pattn_fwd = pattn_q_kernel<0>, fil_pattn_bwd = pattn_q_kernel<1> for dq followed by
pattn_bwd_kv_kernel for dk and dv) at CONSTRUCTED shape, LDS, mask and value edges, called through the C ABI with 64 words of the payload NaN
0x7FC12345 behind q, k, v, mask and dout and 256 guarded bytes in front of and behind out, dq, dk and dv (tests/guarded.py).

Which path a case reaches (restated from pdims / pallow / the launchers):
    nq = cdiv(Fq, 16), nk = cdiv(Fk, 16), QP = 16 nq, KP = 16 nk, NA = cdiv(A, 16), NV = cdiv(Av, 16);  A, Av <= 64 or FIL_ERR_UNSUPPORTED
    one workgroup of four waves per item n;  pattn_q_kernel: wave w takes the query blocks i = w, w + 4, w + 8, ... < nq and walks all nk key
    blocks;  pattn_bwd_kv_kernel: wave w takes the key blocks j = w, w + 4, ... < nk and walks all nq query blocks
    dynamic LDS  sh(F) = (NA + NV) * 16 cdiv(F, 16) * 80 bytes:  the forward and pattn_q_kernel<1> stage k and v: sh(Fk);  pattn_bwd_kv_kernel stages
    q and dout: sh(Fq).  sh > 48 KiB: the launcher opts the kernel in (hipFuncSetAttribute);  sh > 160 KiB: FIL_ERR_UNSUPPORTED
    rows and columns beyond Fq, Fk, A, Av are ZEROS in LDS and registers (not masked): a padded key scores sigmoid(0) = 0.5 against every query
    and contributes 0.5 * 0 because its v and the padded dout rows are zero.  (Known, not asserted: with Fk % 16 != 0 an inf in an item's q or
    dout meets those zeros as 0 * inf = NaN inside that item.)
    mask (additive, -1e5 per unit): item n reads mask[n % mask_period] of [mask_period, Fq, Fk];  mask_period must be >= 1 and divide N

    kernel / launch                          test
    pattn_q_kernel<0>                        test_pattn_shape_edges[*] (18 pairwise shapes), every other test's forward
    pattn_q_kernel<1>, pattn_bwd_kv_kernel   the same tests' backward
    forward          sh <= 48 KiB            test_pattn_lds_opt_in[77-5]  (10 KiB);          > 48 KiB: [5-77], [77-77] (50 KiB), test_pattn_at_160_kib
    pattn_q_kernel<1> sh <= 48 KiB           test_pattn_lds_opt_in[77-5];                    > 48 KiB: [5-77], [77-77], test_pattn_at_160_kib
    pattn_bwd_kv_kernel sh <= 48 KiB         test_pattn_lds_opt_in[5-77];                    > 48 KiB: [77-5], [77-77], test_pattn_at_160_kib
ProductAttentionLayer documents no composed path for shapes outside the menu (it raises the library's error), so there is no such case.

Reference and bounds.  The reference is oracle.graph.product_attention in float64 on the same fp32 inputs, gradients by autograd.  Per element,
with u = 2^-24, gamma(m) = m u / (1 - m u), s = scale q.k the score and S = sigmoid(s - 1e5 mask):
    the kernel holds t = -log2(e) (scale q.k - 1e5 mask) and evaluates S = rcp(1 + exp2(t)).  t carries gamma(A + 3) on sum_a |q_a k_a| scale log2(e)
    (the roundings of scale, of log2(e) scale, of q times that, and A fused multiply-adds); dS/dt = -ln(2) S (1 - S), at most ln(2) / 4 in size:
        delta = gamma(A + 3) scale sum_a |q_a k_a| / 4                                        absolute, on every S
    v_exp_f32, the rounding of 1 + x and v_rcp_f32 add a relative error E_S; the ISA and micro-architecture guides at hand do not state the two
    instructions' accuracy, so it is MEASURED: PSIGMOID_MEASURED_U = the worst relative error of S against float64 in units of u on the 4096
    scores linspace(-1, 1) (A = 1, k = 1, scale = 1, v = the 64 x 64 identity so that out IS S, N = 16, Fq = 256, Fk = 64; it CONTAINS the score's own
    roundings there, |t| <= 1.45), and E_S = 2 PSIGMOID_MEASURED_U u:
        b_S = delta + E_S S
    out = S v, dS = dout v^T, dP = dS S (1 - S) scale, dq = dP k, dk = dP^T q, dv = S^T dout, every sum an fp32 MFMA accumulation:
        b_out = sum_k |v| (b_S + gamma(Fk) S)
        b_dS  = gamma(Av) sum |dout| |v|
        b_dP  = 1.01 scale (b_dS S (1 - S) + |dS| (b_S |1 - 2 S| + b_S^2) + gamma(6) |dS| S (1 - S))
        b_dq  = sum_k |k| (b_dP + gamma(Fk) |dP|),   b_dk = sum_q |q| (b_dP + gamma(Fq) |dP|),   b_dv = sum_q |dout| (b_S + gamma(Fq) S)
Every comparison asserts error <= bound per element and reports the worst ratio.  Measured on an MI355X: PSIGMOID_MEASURED_U = 2.0901 u; with
it the worst error-to-bound ratios over this file were out 0.24, dq 0.32, dk 0.39, dv 0.37.
"""
import functools

import numpy as np
import pytest
import torch

from ml_function_amd import _lib
from ml_function_amd import functional as Fn
from ml_function_amd._lib import check, ptr, stream_ptr
from ml_function_amd.layers.behavior_layer import ProductAttentionLayer
from oracle import graph as G
from tests.guarded import GuardedOutput, f32_words, poisoned_input, sentinel

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PSIGMOID_MEASURED_U = 2.0901
E_S = 2.0 * PSIGMOID_MEASURED_U * U
ERR_ARG, ERR_UNSUPPORTED = -1, -4
KEYS = ("out", "dq", "dk", "dv")


def gamma(m):
    return m * U / (1.0 - m * U)


def cdiv(a, b):
    return (a + b - 1) // b


def lds_bytes(F, A, Av):
    return (cdiv(A, 16) + cdiv(Av, 16)) * 16 * cdiv(F, 16) * 80


def untouched(g):
    return (g.t.cpu().numpy().view(g.npw) == sentinel(g.npw)).all()


def scale_of(A, use_scale):
    return float(np.float32(1.0 / np.sqrt(A))) if use_scale else 1.0


def run_pattn(q, k, v, mask, dout, scale, period, expect=(0, 0), N=None):
    """fil_pattn_fwd and fil_pattn_bwd on fp32 arrays q [N, Fq, A], k [N, Fk, A], v [N, Fk, Av], mask [period, Fq, Fk] or None, dout [N, Fq, Av]
    -> dict of out, dq, dk, dv (fp32).  Return codes (expect = (forward, backward)) and every guard are checked here; a rejected call must leave
    its outputs' payloads untouched as well.  N: the item count passed, when it is not q's."""
    lib = _lib.load()
    n_alloc, Fq, A = q.shape
    Fk, Av = v.shape[1:]
    N = n_alloc if N is None else N
    what = "N=%d Fq=%d Fk=%d A=%d Av=%d scale=%.4g period=%d" % (N, Fq, Fk, A, Av, scale, period)
    qt, kt, vt, gt = (poisoned_input(f32_words(a)) for a in (q, k, v, dout))
    mt = None if mask is None else poisoned_input(f32_words(mask))
    out, dq = GuardedOutput((n_alloc, Fq, Av), np.uint32, "out"), GuardedOutput((n_alloc, Fq, A), np.uint32, "dq")
    dk, dv = GuardedOutput((n_alloc, Fk, A), np.uint32, "dk"), GuardedOutput((n_alloc, Fk, Av), np.uint32, "dv")
    rc = lib.fil_pattn_fwd(ptr(qt), ptr(kt), ptr(vt), ptr(mt), out.ptr, N, Fq, Fk, A, Av, float(scale), int(period), stream_ptr())
    assert rc == expect[0], (what, rc, lib.fil_last_error())
    check(rc if expect[0] == 0 else 0, "fil_pattn_fwd")
    rc = lib.fil_pattn_bwd(ptr(qt), ptr(kt), ptr(vt), ptr(mt), ptr(gt), dq.ptr, dk.ptr, dv.ptr, N, Fq, Fk, A, Av, float(scale), int(period), stream_ptr())
    assert rc == expect[1], (what, rc, lib.fil_last_error())
    got = dict(out=out.read(what), dq=dq.read(what), dk=dk.read(what), dv=dv.read(what))
    if expect[0] != 0 or N == 0:
        assert untouched(out), what + ": out was written"
    if expect[1] != 0 or N == 0:
        assert untouched(dq) and untouched(dk) and untouched(dv), what + ": a gradient was written"
    return {key: a.view(np.float32) for key, a in got.items()}


def reference(q, k, v, mask, dout, use_scale):
    """mask: None or broadcastable to [N, Fq, Fk].  -> (want, bound): the float64 oracle's out, dq, dk, dv and the per-element bounds of the
    module docstring."""
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    qt, kt, vt = t64(q), t64(k), t64(v)
    m = None if mask is None else torch.tensor(np.asarray(mask, np.float64))
    out = G.product_attention(qt, kt, vt, use_scale=use_scale, mask=m, mask_mod=2)
    out.backward(torch.tensor(dout.astype(np.float64)))
    want = dict(out=out.detach().numpy(), dq=qt.grad.numpy(), dk=kt.grad.numpy(), dv=vt.grad.numpy())
    q, k, v, g = (np.asarray(a, np.float64) for a in (q, k, v, dout))
    N, Fq, A = q.shape
    Fk, Av = v.shape[1:]
    sc = 1.0 / np.sqrt(A) if use_scale else 1.0
    s = np.einsum("nqa,nka->nqk", q, k) * sc
    if mask is not None:
        s = s - 1e5 * np.broadcast_to(np.asarray(mask, np.float64), s.shape)
    with np.errstate(over="ignore"):
        S = 1.0 / (1.0 + np.exp(-s))
    delta = gamma(A + 3.0) * sc * np.einsum("nqa,nka->nqk", np.abs(q), np.abs(k)) / 4.0
    bS = delta + E_S * S
    SS = S * (1.0 - S)
    dS = np.einsum("nqv,nkv->nqk", g, v)
    bdS = gamma(float(Av)) * np.einsum("nqv,nkv->nqk", np.abs(g), np.abs(v))
    dP = dS * SS * sc
    bdP = 1.01 * sc * (bdS * SS + np.abs(dS) * (bS * np.abs(1.0 - 2.0 * S) + bS * bS) + gamma(6.0) * np.abs(dS) * SS)
    bound = dict(out=np.einsum("nqk,nkv->nqv", bS + gamma(float(Fk)) * S, np.abs(v)),
                 dq=np.einsum("nqk,nka->nqa", bdP + gamma(float(Fk)) * np.abs(dP), np.abs(k)),
                 dk=np.einsum("nqk,nqa->nka", bdP + gamma(float(Fq)) * np.abs(dP), np.abs(q)),
                 dv=np.einsum("nqk,nqv->nkv", bS + gamma(float(Fq)) * S, np.abs(g)))
    return want, bound


def assert_within(got, want, bound, what, keys=KEYS):
    """error <= bound per element (a NaN fails); -> the worst ratio per output."""
    worst = {}
    for key in keys:
        err = np.abs(got[key].astype(np.float64) - want[key])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound[key])
        worst[key] = float(np.max(ratio)) if ratio.size else 0.0
    print("%s: worst error / bound %s" % (what, {k: "%.4f" % r for k, r in worst.items()}))
    for key in keys:
        assert worst[key] <= 1.0, "%s: %s: worst error / bound = %.4f at %s" % (
            what, key, worst[key], np.unravel_index(np.nanargmax(np.abs(got[key].astype(np.float64) - want[key]) / bound[key]), want[key].shape))
    return worst


def make_case(N, Fq, Fk, A, Av, seed=0):
    """q, k ~ N(0, 1) A^-1/4 (scores of unit deviation at scale 1), v, dout ~ N(0, 1)."""
    rng = np.random.default_rng(1000003 * Fq + 10007 * Fk + 101 * A + Av + 7 * N + seed)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    a4 = np.float32(A ** -0.25)
    return f(N, Fq, A) * a4, f(N, Fk, A) * a4, f(N, Fk, Av), f(N, Fq, Av)


def check_case(N, Fq, Fk, A, Av, use_scale, mask=None, period=0, seed=0, data=None):
    q, k, v, dout = make_case(N, Fq, Fk, A, Av, seed) if data is None else data
    got = run_pattn(q, k, v, mask, dout, scale_of(A, use_scale), period)
    full_mask = None if mask is None else mask[np.arange(N) % period]
    want, bound = reference(q, k, v, full_mask, dout, use_scale)
    worst = assert_within(got, want, bound, "N=%d Fq=%d Fk=%d A=%d Av=%d use_scale=%s period=%d" % (N, Fq, Fk, A, Av, use_scale, period))
    return got, want, bound, worst


# ------------------------------------------------------------------------------------------------ 1. shape edges
F_EDGES = [1, 15, 16, 17, 33, 65, 80, 81, 129]           # nq / nk = 1, 1, 1, 2, 3, 5, 5, 6, 9: no round, ragged rounds and full rounds of four waves
A_EDGES = [1, 3, 5, 15, 16, 17, 33, 63, 64]              # ragged 4-groups (1, 3, 5, 15, 17, 33, 63), the chunk edge, the menu's end
SHAPES = [(F_EDGES[i], F_EDGES[(i + 4) % 9], A_EDGES[i], A_EDGES[(i + 5) % 9], 1 + 2 * (i % 2), bool(i % 2)) for i in range(9)] + \
         [(F_EDGES[i], F_EDGES[(i + 7) % 9], A_EDGES[(i + 3) % 9], A_EDGES[(i + 1) % 9], 3 - 2 * (i % 2), not bool(i % 2)) for i in range(9)]


def test_the_shape_list_covers_every_edge_in_every_role():
    for col, edges in ((0, F_EDGES), (1, F_EDGES), (2, A_EDGES), (3, A_EDGES)):
        assert sorted({s[col] for s in SHAPES}) == edges
    assert all(s[0] != s[1] and s[2] != s[3] for s in SHAPES) and {s[4] for s in SHAPES} == {1, 3} and {s[5] for s in SHAPES} == {False, True}
    assert sorted({cdiv(F, 16) for F in F_EDGES}) == [1, 2, 3, 5, 6, 9]
    assert max(lds_bytes(max(s[0], s[1]), s[2], s[3]) for s in SHAPES) <= 160 * 1024


@pytest.mark.parametrize("Fq,Fk,A,Av,N,use_scale", SHAPES, ids=["%d-%d-%d-%d-N%d-%s" % (s[:5] + ("scaled" if s[5] else "unscaled",)) for s in SHAPES])
def test_pattn_shape_edges(Fq, Fk, A, Av, N, use_scale):
    """Forward and all three gradients against the float64 oracle, per element, at every extent edge in every role; the element at the last
    valid query / key row and last valid column is under the same bound as any other."""
    got, want, bound, _ = check_case(N, Fq, Fk, A, Av, use_scale)
    for key in KEYS:
        last = (N - 1, want[key].shape[1] - 1, want[key].shape[2] - 1)
        assert abs(float(got[key][last]) - want[key][last]) <= bound[key][last], (key, last)


def test_pattn_sigmoid_on_the_measured_grid():
    """The inputs PSIGMOID_MEASURED_U was measured on (module docstring): out IS S.  Prints the figure; asserts the general bounds."""
    s = np.linspace(-1.0, 1.0, 4096).astype(np.float32).reshape(16, 256, 1)
    k = np.ones((16, 64, 1), np.float32)
    v = np.broadcast_to(np.eye(64, dtype=np.float32), (16, 64, 64)).copy()
    dout = np.ones((16, 256, 64), np.float32)
    got, want, _, _ = check_case(16, 256, 64, 1, 64, False, data=(s, k, v, dout))
    rel = np.abs(got["out"].astype(np.float64) - want["out"]) / want["out"]
    print("S on linspace(-1, 1, 4096): worst relative error %.4f u" % (rel.max() / U))


# ------------------------------------------------------------------------------------------------ 2. the LDS opt-in
@pytest.mark.parametrize("Fq,Fk", [(5, 77), (77, 5), (77, 77)])
def test_pattn_lds_opt_in(Fq, Fk):
    """A = Av = 64: sh(77) = 51200 > 48 KiB, sh(5) = 10240.  (5, 77): the forward and pattn_q_kernel<1> opt in, pattn_bwd_kv_kernel does not;
    (77, 5): the other way round; (77, 77): all three.  (These cases pin the RESULTS on both sides of the threshold.  The HIP runtime this was
    written against also launches above 48 KiB, and at 160 KiB, when the opt-in is left out, so no test of results can notice a missing call;
    the launcher reports a refused opt-in as FIL_ERR_HIP.)"""
    assert lds_bytes(77, 64, 64) == 51200 > 48 * 1024 > lds_bytes(5, 64, 64) == 10240
    assert (lds_bytes(Fk, 64, 64) > 48 * 1024) == (Fk == 77) and (lds_bytes(Fq, 64, 64) > 48 * 1024) == (Fq == 77)
    check_case(2, Fq, Fk, 64, 64, True)


def test_pattn_at_160_kib():
    """Fq = Fk = 256, A = Av = 64, N = 1: exactly 160 KiB for each of the three launches, the documented ceiling.  Both calls return OK and
    match the oracle."""
    assert lds_bytes(256, 64, 64) == 160 * 1024
    check_case(1, 256, 256, 64, 64, True)


def test_pattn_rejects_shapes_outside_the_menu():
    """Fk = 257 (forward and backward: sh(Fk) > 160 KiB), Fq = 257 (backward only: the forward stages k and v and runs), A = 65, Av = 65:
    FIL_ERR_UNSUPPORTED and not one word written."""
    assert lds_bytes(257, 64, 64) > 160 * 1024
    q, k, v, dout = make_case(1, 3, 257, 64, 64)
    run_pattn(q, k, v, None, dout, 1.0, 0, expect=(ERR_UNSUPPORTED, ERR_UNSUPPORTED))
    q, k, v, dout = make_case(1, 257, 3, 64, 64)
    got = run_pattn(q, k, v, None, dout, 1.0, 0, expect=(0, ERR_UNSUPPORTED))
    want, bound = reference(q, k, v, None, dout, False)
    assert_within(got, want, bound, "Fq=257 forward", keys=("out",))
    for A, Av in [(65, 4), (4, 65)]:
        q, k, v, dout = make_case(1, 3, 5, A, Av)
        run_pattn(q, k, v, None, dout, 1.0, 0, expect=(ERR_UNSUPPORTED, ERR_UNSUPPORTED))
    q, k, v, dout = (torch.tensor(a, device="cuda") for a in make_case(1, 3, 5, 65, 4))
    with pytest.raises(_lib.FilError):
        ProductAttentionLayer().call([q, k, v])


# ------------------------------------------------------------------------------------------------ 3. masks through the C ABI
MASK_N, MASK_FQ, MASK_FK, DEAD_KEY = 6, 17, 33, 5


@functools.lru_cache(maxsize=None)
def mask_of(period):
    """[period, Fq, Fk] of 0 / 1, different per item and per query row; key DEAD_KEY is masked for every query of every item."""
    m = (np.random.default_rng(40 + period).random((period, MASK_FQ, MASK_FK)) < 0.3).astype(np.float32)
    m[:, :, DEAD_KEY] = 1
    m[:, :, DEAD_KEY + 1] = 0
    assert all(not np.array_equal(m[i], m[j]) for i in range(period) for j in range(i)) and not np.array_equal(m[0, 0], m[0, 1])
    m.setflags(write=False)
    return m


@pytest.mark.parametrize("period", [1, 2, 3, 6])
def test_pattn_mask_periods(period):
    """N = 6 items read mask[n % period].  With v = the identity (Av = Fk = 33) out IS S: exactly 0 at every masked (query, key) pair and
    non-zero elsewhere; dv and dk of the key that every query masks are exactly 0.  With random v (Av = 3) everything is compared with the
    oracle given mask[n % period].  The mask buffer is N items long, the items behind the period holding the complements of the masks."""
    m = mask_of(period)
    full = m[np.arange(MASK_N) % period]
    # the buffer holds N items: behind the period's masks their complements, which an index n in place of n % period would read
    m = np.concatenate([m, 1.0 - m[np.arange(MASK_N - period) % period]]).astype(np.float32)
    q, k, _, _ = make_case(MASK_N, MASK_FQ, MASK_FK, 5, 3)
    eye = np.broadcast_to(np.eye(MASK_FK, dtype=np.float32), (MASK_N, MASK_FK, MASK_FK)).copy()
    dout = np.random.default_rng(period).standard_normal((MASK_N, MASK_FQ, MASK_FK)).astype(np.float32)
    got, _, _, _ = check_case(MASK_N, MASK_FQ, MASK_FK, 5, MASK_FK, False, mask=m, period=period, data=(q, k, eye, dout))
    assert (got["out"][full == 1] == 0).all() and (got["out"][full == 0] > 0).all()
    assert (got["dv"][:, DEAD_KEY] == 0).all() and (got["dk"][:, DEAD_KEY] == 0).all() and (got["dk"][:, DEAD_KEY + 1] != 0).all()
    got, _, _, _ = check_case(MASK_N, MASK_FQ, MASK_FK, 5, 3, True, mask=m, period=period)
    assert (got["dv"][:, DEAD_KEY] == 0).all() and (got["dk"][:, DEAD_KEY] == 0).all()


def test_pattn_mask_period_must_divide_the_item_count():
    """period = 4 (6 % 4 != 0) and period = 0 with a mask: the argument error, nothing written.  Without a mask the period is ignored: the
    same bits as the plain run."""
    q, k, v, dout = make_case(MASK_N, MASK_FQ, MASK_FK, 5, 3)
    m = np.zeros((6, MASK_FQ, MASK_FK), np.float32)
    for period in (4, 0, -1):
        run_pattn(q, k, v, m, dout, 1.0, period, expect=(ERR_ARG, ERR_ARG))
    plain = run_pattn(q, k, v, None, dout, 1.0, 0)
    for period in (4, 7, -3):
        other = run_pattn(q, k, v, None, dout, 1.0, period)
        for key in KEYS:
            assert np.array_equal(plain[key].view(np.uint32), other[key].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 4. masks through functional.product_attention
LEAD, W_FQ, W_FK, W_A, W_AV = (3, 2), 17, 33, 5, 3


def wrapper_case(Fk=W_FK, k_eighths=False):
    rng = np.random.default_rng(50 + Fk)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    k = (rng.integers(-8, 9, size=LEAD + (Fk, W_A)) / 8.0).astype(np.float32) if k_eighths else f(*LEAD, Fk, W_A) * 0.7
    return f(*LEAD, W_FQ, W_A) * 0.7, k


def through_the_wrapper(q, k, v, mask, dout, mask_mod, use_scale):
    ts = [torch.tensor(a, device="cuda", requires_grad=True) for a in (q, k, v)]
    out = Fn.product_attention(*ts, use_scale=use_scale, mask=torch.tensor(mask, device="cuda"), mask_mod=mask_mod)
    out.backward(torch.tensor(dout, device="cuda"))
    return dict(out=out.detach().cpu().numpy(), dq=ts[0].grad.cpu().numpy(), dk=ts[1].grad.cpu().numpy(), dv=ts[2].grad.cpu().numpy())


@pytest.mark.parametrize("shape", [(W_FK,), (1, W_FK), (W_FQ, W_FK), (2, W_FQ, W_FK), (3, 1, W_FQ, W_FK), (1, 1, 1, W_FK), (3, 2, W_FQ, W_FK)],
                         ids=["Fk", "1-Fk", "Fq-Fk", "2-Fq-Fk", "3-1-Fq-Fk", "1-1-1-Fk", "3-2-Fq-Fk"])
def test_pattn_mask_shapes_through_the_layer(shape):
    """mask_mod = 2 with q of leading axes (3, 2).  A mask whose leading axes are a suffix of q's goes to the kernel as [period, Fq, Fk]:
    [Fk], [1, Fk], [Fq, Fk] with period 1, [2, Fq, Fk] with period 2, [3, 2, Fq, Fk] with period 6.  [3, 1, Fq, Fk] and [1, 1, 1, Fk] are no
    suffix and are expanded to one mask per item (period 6).  All must match the oracle's broadcasting."""
    rng = np.random.default_rng(len(shape) + shape[0])
    q, k = wrapper_case()
    v, dout = rng.standard_normal(LEAD + (W_FK, W_AV)).astype(np.float32), rng.standard_normal(LEAD + (W_FQ, W_AV)).astype(np.float32)
    mask = (rng.random(shape) < 0.3).astype(np.float32)
    got = through_the_wrapper(q, k, v, mask, dout, 2, True)
    flat = lambda a: a.reshape((-1,) + a.shape[-2:])
    full = np.broadcast_to(mask, LEAD + (W_FQ, W_FK)).reshape(-1, W_FQ, W_FK)
    want, bound = reference(flat(q), flat(k), flat(v), full, flat(dout), True)
    assert_within({key: flat(a) for key, a in got.items()}, want, bound, "mask %s through the layer" % (shape,))


def test_pattn_right_multiplied_mask_through_the_layer():
    """mask_mod = 1 with a non-square 0 / 1 mask [Fk, Fk'] = [33, 20] and v of Fk' rows: (q k^T) M = q (M^T k)^T.  k holds multiples of 1/8, so
    M^T k is exact in fp32 and the kernel's bounds hold for out, dq and dv with k' = M^T k; dk = M dk' is one more fp32 matrix product:
    M b_dk' + gamma(Fk' + 2) M |dk'|."""
    Fk2 = 20
    rng = np.random.default_rng(60)
    q, k = wrapper_case(k_eighths=True)
    v, dout = rng.standard_normal(LEAD + (Fk2, W_AV)).astype(np.float32), rng.standard_normal(LEAD + (W_FQ, W_AV)).astype(np.float32)
    M = (rng.random((W_FK, Fk2)) < 0.4).astype(np.float32)
    got = through_the_wrapper(q, k, v, M, dout, 1, False)
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    qt, kt, vt = t64(q), t64(k), t64(v)
    out = G.product_attention(qt, kt, vt, use_scale=False, mask=torch.tensor(M.astype(np.float64)), mask_mod=1)
    out.backward(torch.tensor(dout.astype(np.float64)))
    flat = lambda a: a.reshape((-1,) + a.shape[-2:])
    k2 = np.einsum("kj,nka->nja", M.astype(np.float64), flat(k).astype(np.float64))
    assert np.array_equal(k2, k2.astype(np.float32).astype(np.float64))
    want2, bound = reference(flat(q), k2, flat(v), None, flat(dout), False)
    want = dict(out=flat(out.detach().numpy()), dq=flat(qt.grad.numpy()), dk=flat(kt.grad.numpy()), dv=flat(vt.grad.numpy()))
    for key in ("out", "dq", "dv"):
        assert np.allclose(want[key], want2[key], rtol=1e-12, atol=1e-12)
    M64 = M.astype(np.float64)
    bound["dk"] = np.einsum("kj,nja->nka", M64, bound["dk"] + gamma(Fk2 + 2.0) * np.abs(want2["dk"]))
    assert_within({key: flat(a) for key, a in got.items()}, want, bound, "mask_mod = 1 through the layer")


# ------------------------------------------------------------------------------------------------ 5. padding is inert
def bits_equal(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_pattn_items_do_not_depend_on_their_neighbours():
    """Fq = Fk = 17, A = 5, Av = 3 (15 padded rows and 11 / 13 padded columns): items 0 and 1 of a run of N = 5 whose other items hold values a
    thousand times larger equal, bit for bit and in all four outputs, the run of that item alone (N = 1); each single run is inside the oracle's
    bounds, its element at the last valid row and column included."""
    q, k, v, dout = make_case(5, 17, 17, 5, 3)
    for a in (q, k, v, dout):
        a[2:] *= 1000.0
    both = run_pattn(q, k, v, None, dout, scale_of(5, True), 0)
    for n in (0, 1):
        data = tuple(a[n:n + 1].copy() for a in (q, k, v, dout))
        alone, want, bound, _ = check_case(1, 17, 17, 5, 3, True, data=data)
        for key in KEYS:
            assert bits_equal(alone[key][0], both[key][n]), "%s of item %d depends on the other items" % (key, n)
            assert abs(float(alone[key][0, -1, -1]) - want[key][0, -1, -1]) <= bound[key][0, -1, -1]
    assert all(np.isfinite(both[key]).all() for key in KEYS)


def test_pattn_saturated_scores():
    """Scores of +-200 ... +-260 (q = c k along one direction), v = the identity so that out IS S: S is exactly 1 or 0 by the score's sign,
    nothing is NaN, and dq and dk -- every S of every row is saturated -- are exactly 0."""
    N, F, A = 2, 17, 5
    rng = np.random.default_rng(70)
    w = rng.standard_normal(A)
    sk, sq = rng.choice([-1.0, 1.0], size=(N, F)), rng.choice([-1.0, 1.0], size=(N, F))
    k = (sk[:, :, None] * w).astype(np.float32)
    q = (sq[:, :, None] * rng.uniform(200, 260, size=(N, F, 1)) * w / (w @ w)).astype(np.float32)
    score = np.einsum("nqa,nka->nqk", q.astype(np.float64), k.astype(np.float64))
    assert (np.abs(score) > 195).all() and (score > 0).any() and (score < 0).any()
    v = np.broadcast_to(np.eye(F, dtype=np.float32), (N, F, F)).copy()
    dout = rng.standard_normal((N, F, F)).astype(np.float32)
    got = run_pattn(q, k, v, None, dout, 1.0, 0)
    assert np.array_equal(got["out"], (score > 0).astype(np.float32))
    assert all(not np.isnan(got[key]).any() for key in KEYS)
    assert (got["dq"] == 0).all() and (got["dk"] == 0).all()
    want, bound = reference(q, k, v, None, dout, False)
    assert_within(got, want, bound, "saturated scores")


# ------------------------------------------------------------------------------------------------ 6. non-finite values stay in their item
@pytest.mark.parametrize("which", ["q", "v"])
def test_pattn_a_nan_stays_in_its_item(which):
    """A NaN in one element of item 2's q, then of its v (N = 4, Fq = 17, Fk = 33: padded keys): every other item's out, dq, dk, dv are
    bit-identical to the clean run, and item 2's outputs that depend on the element contain NaN (dv does not depend on v)."""
    q, k, v, dout = make_case(4, 17, 33, 5, 3, seed=1)
    clean = run_pattn(q, k, v, None, dout, 1.0, 0)
    if which == "q":
        q[2, 3, 1] = np.nan
    else:
        v[2, 5, 0] = np.nan
    got = run_pattn(q, k, v, None, dout, 1.0, 0)
    others = [0, 1, 3]
    for key in KEYS:
        assert bits_equal(got[key][others], clean[key][others]), "%s: the NaN left item 2" % key
    if which == "q":
        assert np.isnan(got["out"][2, 3]).all() and np.isnan(got["dq"][2, 3]).all() and np.isnan(got["dk"][2]).all() and np.isnan(got["dv"][2]).all()
    else:
        assert np.isnan(got["out"][2, :, 0]).all() and np.isnan(got["dq"][2]).all() and np.isnan(got["dk"][2, 5]).all()
        assert bits_equal(got["dv"][2], clean["dv"][2])


# ------------------------------------------------------------------------------------------------ 7. housekeeping
def test_pattn_empty_batch_and_repeats():
    """N = 0: both calls return OK and write nothing.  A repeat gives the same bits (masked, two rounds of the wave loop, above 48 KiB)."""
    q, k, v, dout = make_case(1, 17, 33, 5, 3)
    run_pattn(q, k, v, None, dout, 1.0, 0, N=0)
    q, k, v, dout = make_case(3, 81, 129, 17, 33)
    m = (np.random.default_rng(80).random((3, 81, 129)) < 0.2).astype(np.float32)
    a, b = run_pattn(q, k, v, m, dout, 0.25, 3), run_pattn(q, k, v, m, dout, 0.25, 3)
    for key in KEYS:
        assert bits_equal(a[key], b[key])
