"""The AutoInt interacting layer (csrc/attn_impl.h: fil_attn_fwd = attn_fwd_kernel<NC, F16, A16, KREG>, fil_attn_bwd = attn_bwd_kernel<NC, F16, NB,
WPH, DX, A16> followed by attn_reduce_kernel) at CONSTRUCTED dispatch, grid, option and value edges, called through the C ABI with 64 words of the
payload NaN 0x7FC12345 behind every input (the head-major x included), 256 guarded bytes in front of and behind y, res, av, rstd, dx, dWq, dWk, dWr,
dgamma and dbeta, and a workspace of exactly fil_attn_bwd_workspace_bytes in front of a guard (tests/guarded.py).

Which instantiation a case reaches is restated in tests/attn_edge_cases.py (held to fil_attn_plan over the whole menu by tests/test_host.py without a
GPU); every case here asserts fil_attn_plan == that restatement, and without knobs == the tuple its table row was built for, BEFORE it launches.

    kernel form (backward NB, wph, dx image; f32 / f16)                     case (F, K, H, A)      built for
    NB=4                                                                    (1, 1, 1, 1)           smallest legal shape
    NB=4                                                                    (16, 16, 1, 16)        one full tile, no masks
    NB=4, NC=2                                                              (17, 17, 1, 16)        one row into block 2, one column into chunk 2
    NB=4                                                                    (64, 16, 2, 16)        top of NB=4
    [8,1,1] / [8,1,1]      NC=3                                             (65, 33, 2, 8)         bottom of NB=8, one live column in chunk 3
    [8,1,1] / [8,1,0]                                                       (112, 33, 5, 3)        H=5, A=3
    [8,1,0] / [8,1,1]                                                       (128, 48, 8, 16)       top of NB=8, H=8
    [13,2,1] / [13,2,0]    general form                                     (129, 48, 4, 7)        bottom of NB=13
    [13,2,0] / [13,2,1]    A16 form; f16 forward KREG=13                    (208, 64, 4, 16)       top of NB=13
    [32,2,0] / [32,2,0]    A16 form; f16 forward k image in LDS             (209, 64, 4, 16)       first NB=32 shape
    [32,1,0] / [32,2,0]                                                     (300, 48, 4, 16)       NC=3 at NB=32
    [32,1,0] / [32,2,1]    158,720 B / 161,792 B                            (384, 32, 4, 16)       last f32-supported F at H=4
    [32,2,0] / [32,1,1]                                                     (512, 16, 1, 16)       menu end, one head
    [32,2,1] / [32,2,0]                                                     (512, 16, 2, 16)       menu end, two heads
    f16 [32,2,1] at 163,328 B = the limit exactly                           (400, 48, 2, 16)       the launch must succeed
    f16 [13,1,0]                                                            (208, 64, 8, 16)       last supported F at H=8, K=64
    f16 [32,1,0]           general form                                     (400, 16, 8, 1)        H=8, A=1 at NB=32
    (NB, NC) pairs no edge lands on: (40,40,2,16) 4x3, (33,64,2,4) 4x4, (80,16,3,16) 8x1, (100,32,2,5) 8x2, (97,64,1,16) 8x4, (130,16,2,9) 13x1,
    (150,32,3,16) 13x2
    refused (FIL_ERR_UNSUPPORTED, nothing written): (129,16,8,16) f32 backward; (209,64,8,16) f16 backward; (400,16,8,1) f32 both; (512,64,4,16) f32 both
    several samples per workgroup (B = 1025, 1030)                          test_attn_several_samples_per_workgroup, test_attn_a_nan_stays_in_its_sample
    attn_reduce_kernel: unrolled loop and its tail, 64-column blocks        test_attn_reduce_partial_counts, test_attn_reduce_column_blocks;  the
                        dgamma / dbeta loop past 1024 partial blocks        (17, 8, 8, 4) row of test_attn_several_samples_per_workgroup

Reference and bars.  The reference is oracle.closed.attn_fwd / attn_bwd in float64 on synth.attn_case(dist="normal") (unfused mode: float64 autograd
over oracle.graph.mult_head_attention with the loss <av, dy> + <res, dres>).  Bars are the project's own, norm-relative max|a - b| / max|b|:
f32 1e-5 on outputs and 2e-5 on gradients; f16_mfma 5e-3 / 2e-2 on kink-free inputs (beta + 6: no output near the ReLU kink, as
test_gpu_parity.py::test_attn_two_waves_per_head does).  The saved LayerNorm input (av, NORMALISED) and rstd are outputs of the forward too: the f32 mode
holds them at the output bar; in the f16 mode they are printed only -- the normalisation divides the f16 products' error (5e-4 of max|av|) by the ROW's
deviation, so a row whose elements nearly agree (A = 3: one row in a few hundred) carries any multiple of it, up to 1 / sqrt(eps) = 31.6 -- while y,
which adds the normalised row to the residual, and every gradient, which consumes av and rstd, are held.  Where the reference gradient is identically zero the check is absolute:
|got| <= 1e-6 max|dWr|.  Bit-for-bit properties carry no tolerance.  Every comparison prints its measured errors.

Measured on an MI355X, the worst norm-relative error over this file and the case it belongs to:
                 f32 (bars 1e-5 / 2e-5)                                  f16_mfma (bars 5e-3 / 2e-2)
    y            4.4e-6   (112, 33, 5, 3)                                1.9e-3   (112, 33, 5, 3)
    res          2.3e-7   unfused (129, 48, 4, 7)                        3.2e-4   unfused (129, 48, 4, 7)
    av, rstd     9.3e-6, 4.1e-6   (112, 33, 5, 3)                        1.1e-2, 7.4e-3   (112, 33, 5, 3): printed, not held (above)
    dx           9.4e-6   saturated (129, 48, 4, 7)                      1.7e-2   (112, 33, 5, 3)
    dWq, dWk     1.6e-5, 1.5e-5   saturated (129, 48, 4, 7)              1.1e-2, 7.9e-3   (112, 33, 5, 3)
    dWr          5.1e-7   (384, 32, 4, 16)                               4.4e-4   (33, 64, 2, 4)
    dgamma       1.3e-6   (512, 16, 2, 16)                               9.6e-4   (112, 33, 5, 3)
    dbeta        1.4e-6   reduce n = 65                                  2.1e-7   zero sample (39, 16, 3, 8)
    zero references (A = 1: av, dWq, dWk, dgamma): exactly 0 in both precisions
(112, 33, 5, 3) is the ill-conditioned one in either precision: a LayerNorm over three elements.  Everywhere else f32 stays below 2e-6 outside the
saturated cases.  At F = 512 the f32 kernels measure y 5.4e-7 / 6.9e-7, dx 5.3e-7 / 6.5e-7, dWq 7.3e-7 / 4.9e-7, dgamma 3.1e-7 / 1.3e-6 (one / two heads) --
the same closed forms in float32 numpy measure y 6.2e-7 / 5.7e-7, dx 5.8e-7 / 8.1e-7, dWq 7.5e-7 / 7.5e-7, dgamma 2.8e-7 / 1.1e-6 against float64 (printed by
the F = 512 cases) -- so the project's bars hold there with a factor of ten to spare and no restated bar is used.
Saturated scores in the f16 mode (printed only): y 3.3e-4, dx 1.8e-2, dWq 5.8e-2, dWk 3.7e-2.

What these cases found: (1) the layer's forward succeeding and its backward raising past the backward's LDS limit (now the composed path:
test_gpu_parity.py::test_autoint_layer_past_the_lds_limit_takes_the_composed_path); (2) NaN in the whole dx of a sample with ONE score below -88.7:
the backward formed S (1-S) as e S^2 with e = exp(-score) = inf and S = 0 (test_attn_saturated_scores; now S - S^2); (3) A = 1: dWq and dWk of
2.4e-6 .. 1.8e-5 max|dWr| where they are zero -- the LayerNorm backward's dz gamma was contracted into an fma on one side of dxh - mean(dxh) and rounded on
the other, leaving rstd = 31.6 times the product's rounding error (test_attn_layer_norm_of_one_element; now rounded once: exactly zero).
"""
import ctypes

import numpy as np
import pytest
import torch

from ml_function_amd import _lib, synth
from ml_function_amd._lib import ptr, stream_ptr
from oracle import closed
from oracle import graph as G
from tests import attn_edge_cases as ac
from tests.guarded import GuardedOutput, assert_workspace_guard, f32_words, poisoned_input, sentinel, workspace

pytestmark = pytest.mark.gpu

BARS = {"f32": (1e-5, 2e-5), "f16_mfma": (5e-3, 2e-2)}
OUT_KEYS = ("y", "res", "av", "rstd")
GRAD_KEYS = ("dx", "dWq", "dWk", "dWr", "dgamma", "dbeta")
EPS = 1e-3


def untouched(g):
    return g is None or bool((g.t.cpu().numpy().view(g.npw) == sentinel(g.npw)).all())


def c_plan(shape, precision):
    """fil_attn_plan for (F, K, H, A) -> ac.Plan; equal to the restatement (which follows the knobs of this process), and without knobs to the
    tuple the case's table row was built for."""
    out = (ctypes.c_int * 10)()
    rc = _lib.load().fil_attn_plan(*shape, ac.PRECISIONS[precision], out)
    assert rc == 0, (shape, precision, rc, _lib.load().fil_last_error())
    p = ac.Plan(*out)
    assert p == ac.plan(*shape, ac.PRECISIONS[precision]), (shape, precision, p)
    return p


def assert_built_for(shape, precision):
    p = c_plan(shape, precision)
    if not ac.knobs_set():
        want = ac.expected_tuple(shape, precision)
        assert want is None or want == (p.bwd_nb, p.bwd_wph, p.bwd_dx_lds), (shape, precision, p)
        nbytes = ac.BWD_LDS_BYTES.get((shape, ac.PRECISIONS[precision]))
        assert nbytes is None or nbytes == p.bwd_lds, (shape, precision, p)
    return p


def run_attn(x, Wq, Wk, Wr, gamma, beta, dy, precision, dres=None, fuse_relu=1, saved=True, x_chunk=0, B=None, expect=(0, 0), use_scale=True):
    """fil_attn_fwd and fil_attn_bwd on fp32 arrays: x [B, F, K] (x_chunk = c > 0: head-major [K / c, B, F, c]), Wq, Wk, Wr [K, H, A] (Wr None = no
    residual), gamma, beta [A] (None = no LayerNorm), dy and dres [H, B, F, A] -> dict of uint32 words of y, res, av, rstd, dx (x's layout), dWq, dWk,
    dWr, dgamma, dbeta (None where the mode has no such tensor).  saved: the backward gets the forward's y / av / rstd; otherwise NULL for all three
    and the have_saved = 0 workspace.  B: the batch size passed, when it is not the arrays'.  Return codes (expect = (forward, backward)), every guard
    and the workspace guard are checked here; a refused call must leave its outputs' payloads untouched as well and name its reason."""
    lib = _lib.load()
    K, H, A = Wq.shape
    if x_chunk:
        Kc, Ba, F, c = x.shape
        assert c == x_chunk and Kc * c == K
    else:
        Ba, F, Kx = x.shape
        assert Kx == K
    B = Ba if B is None else B
    prec = ac.PRECISIONS[precision]
    what = "B=%d F=%d K=%d H=%d A=%d %s fuse_relu=%d saved=%s x_chunk=%d" % (B, F, K, H, A, precision, fuse_relu, saved, x_chunk)
    scale = float(np.float32(1.0 / np.sqrt(A))) if use_scale else 1.0
    dev = lambda a: None if a is None else poisoned_input(f32_words(a))
    xt, qt, kt, rt, gt, bt, dyt, drt = (dev(a) for a in (x, Wq, Wk, Wr, gamma, beta, dy, dres))
    act = (H, Ba, F, A)
    out = lambda shape, name, on=True: GuardedOutput(shape, np.uint32, name) if on else None
    o = dict(y=out(act, "y"), res=out(act, "res", not fuse_relu and Wr is not None), av=out(act, "av", gamma is not None),
             rstd=out((H, Ba, F), "rstd", gamma is not None), dx=out(x.shape, "dx"), dWq=out(Wq.shape, "dWq"), dWk=out(Wq.shape, "dWk"),
             dWr=out(Wq.shape, "dWr", Wr is not None), dgamma=out((A,), "dgamma", gamma is not None), dbeta=out((A,), "dbeta", gamma is not None))
    gp = lambda key: None if o[key] is None else o[key].ptr
    rc = lib.fil_attn_fwd(ptr(xt), ptr(qt), ptr(kt), ptr(rt), ptr(gt), ptr(bt), gp("y"), gp("res"), gp("av"), gp("rstd"), B, F, K, H, A, scale, EPS,
                          fuse_relu, prec, x_chunk, None, 0, stream_ptr())
    assert rc == expect[0], (what, "forward", rc, lib.fil_last_error())
    if rc != 0:
        assert len(lib.fil_last_error()) > 20 and (rc != ac.ERR_UNSUPPORTED or b"LDS" in lib.fil_last_error()), lib.fil_last_error()
    if expect[0] != 0 or B == 0:
        assert all(untouched(o[key]) for key in OUT_KEYS), what + ": a refused / empty forward wrote an output"
    have_saved = int(saved)
    nws = lib.fil_attn_bwd_workspace_bytes(B, F, K, H, A, have_saved)
    assert (nws > 0) == (B > 0)
    ws = workspace(nws)
    sv = (lambda key: gp(key)) if saved else (lambda key: None)
    rc = lib.fil_attn_bwd(ptr(xt), ptr(qt), ptr(kt), ptr(rt), ptr(gt), ptr(bt), ptr(dyt), ptr(drt), sv("y") if fuse_relu else None, sv("av"),
                          sv("rstd"), gp("dx"), gp("dWq"), gp("dWk"), gp("dWr"), gp("dgamma"), gp("dbeta"), B, F, K, H, A, scale, EPS, fuse_relu,
                          prec, x_chunk, ptr(ws), nws, stream_ptr())
    assert rc == expect[1], (what, "backward", rc, lib.fil_last_error())
    if rc != 0:
        assert len(lib.fil_last_error()) > 20 and (rc != ac.ERR_UNSUPPORTED or b"LDS" in lib.fil_last_error()), lib.fil_last_error()
    torch.cuda.synchronize()
    assert_workspace_guard(ws, nws, what)
    if expect[1] != 0:
        assert all(untouched(o[key]) for key in GRAD_KEYS), what + ": a refused backward wrote a gradient"
    if B == 0:
        assert untouched(o["dx"]), what + ": an empty backward wrote dx"
    return {key: None if g is None else g.read(what + " " + key) for key, g in o.items()}


def f32(words):
    return None if words is None else words.view(np.float32)


def rel(got, want):
    want = np.asarray(want, np.float64)
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def compare(what, got, want, precision, keys=None, bars=None):
    """got: run_attn's dict (words); want: dict of float64 references.  Norm-relative error of every key against its bar (outputs / gradients of the
    precision); a reference that is identically zero is held absolutely: |got| <= 1e-6 max|dWr| (of the reference).  Prints every figure."""
    by, bg = bars or BARS[precision]
    errs, bad = [], []
    for key in keys or [k for k in OUT_KEYS + GRAD_KEYS if want.get(k) is not None]:
        g, w = f32(got[key]).astype(np.float64), np.asarray(want[key], np.float64)
        assert np.isfinite(g).all(), "%s: %s is not finite" % (what, key)
        if not np.any(w):
            e, bar, kind = float(np.abs(g).max()) if g.size else 0.0, 1e-6 * float(np.abs(want["dWr"]).max()), "abs"
        else:
            e, bar, kind = rel(g, w), (by if key in OUT_KEYS else bg), "rel"
        errs.append("%s %.1e%s" % (key, e, "" if kind == "rel" else " (abs, bar %.1e)" % bar))
        if precision != "f32" and key in ("av", "rstd") and kind == "rel":
            continue                # printed, not held: see the module docstring
        if not e <= bar:
            bad.append("%s %s err %.3e > %.1e" % (key, kind, e, bar))
    print("%s [%s, bars %.0e / %.0e]: %s" % (what, precision, by, bg, ", ".join(errs)))
    assert not bad, "%s: %s" % (what, "; ".join(bad))


def make_case(B, shape, precision, seed=0):
    """synth.attn_case(dist="normal"); f16: beta + 6 (kink-free)."""
    F, K, H, A = shape
    c = synth.attn_case(B, F, K, H, A, seed=synth.SEED + seed, dist="normal")
    if precision != "f32":
        c["beta"] = (c["beta"] + 6.0).astype(np.float32)
    return c


def reference(c, use_res=True, use_ln=True):
    """float64 closed forms of the fused layer -> dict (rstd and av: the saved LayerNorm input, normalised, and 1 / sigma)."""
    y, sv = closed.attn_fwd(c["x"], c["Wq"], c["Wk"], c["Wr"], c["gamma"], c["beta"], use_res=use_res, use_ln=use_ln, eps=EPS, return_saved=True)
    dx, dWq, dWk, dWr, dg, db = closed.attn_bwd(c["x"], c["Wq"], c["Wk"], c["Wr"], c["gamma"], c["beta"], c["dy"], use_res=use_res, use_ln=use_ln,
                                                eps=EPS)
    return dict(y=y, av=sv["xhat"] if use_ln else None, rstd=sv["rstd"][..., 0] if use_ln else None, dx=dx, dWq=dWq, dWk=dWk, dWr=dWr, dgamma=dg,
                dbeta=db)


def run_case(c, precision, **kw):
    return run_attn(c["x"], c["Wq"], c["Wk"], c["Wr"], c["gamma"], c["beta"], c["dy"], precision, **kw)


def assert_same_bits(what, a, b, keys):
    for key in keys:
        if a[key] is None and b[key] is None:
            continue
        assert np.array_equal(a[key], b[key]), "%s: %s differs in %d words" % (what, key, int((a[key] != b[key]).sum()))


def closed_form_in(dtype, c):
    """The same closed forms (residual, LayerNorm, fused ReLU) evaluated in `dtype` with numpy: float32 = an equally valid summation order in the
    kernels' own arithmetic; its error against float64 says how much such an order may differ.  -> dict like reference()."""
    x, Wq, Wk, Wr, gamma, beta, dy = (np.asarray(c[n], dtype) for n in ("x", "Wq", "Wk", "Wr", "gamma", "beta", "dy"))
    A = Wq.shape[-1]
    one, sc, eps = dtype(1.0), dtype(1.0 / np.sqrt(A)), dtype(EPS)
    q, k, r = (np.einsum("bfk,kma->mbfa", x, W) for W in (Wq, Wk, Wr))
    S = one / (one + np.exp(-(np.einsum("mbfa,mbga->mbfg", q, k) * sc)))
    av = np.einsum("mbfg,mbga->mbfa", S, k)
    mu = av.mean(-1, keepdims=True)
    rstd = one / np.sqrt(((av - mu) ** 2).mean(-1, keepdims=True) + eps)
    xhat = (av - mu) * rstd
    z = r + xhat * gamma + beta
    dz = dy * (z > 0)
    dxhat = dz * gamma
    dav = rstd * (dxhat - dxhat.mean(-1, keepdims=True) - xhat * (dxhat * xhat).mean(-1, keepdims=True))
    dpre = np.einsum("mbfa,mbga->mbfg", dav, k) * S * (one - S) * sc
    dq = np.einsum("mbfg,mbga->mbfa", dpre, k)
    dk = np.einsum("mbfg,mbfa->mbga", dpre, q) + np.einsum("mbfg,mbfa->mbga", S, dav)
    dx = np.einsum("mbfa,kma->bfk", dq, Wq) + np.einsum("mbfa,kma->bfk", dk, Wk) + np.einsum("mbfa,kma->bfk", dz, Wr)
    return dict(y=np.maximum(z, 0), av=xhat, rstd=rstd[..., 0], dx=dx, dWq=np.einsum("bfk,mbfa->kma", x, dq), dWk=np.einsum("bfk,mbfa->kma", x, dk),
                dWr=np.einsum("bfk,mbfa->kma", x, dz), dgamma=(dz * xhat).sum((0, 1, 2)), dbeta=dz.sum((0, 1, 2)))


# ------------------------------------------------------------------------------------------------ 1. shape cases
def shape_id(shape, precision):
    return "%sF%d-K%d-H%d-A%d-%s" % (("big-" if shape[0] >= ac.KNOB_MIN_F else "",) + tuple(shape) + (precision,))


SHAPE_PAIRS = ac.shape_case_list()


@pytest.mark.parametrize("shape,precision", SHAPE_PAIRS, ids=[shape_id(s, p) for s, p in SHAPE_PAIRS])
def test_attn_shape_edges(shape, precision):
    """Residual and LayerNorm on, fused ReLU, B = 2 or 3: every output (y, the saved normalised av, rstd) and every gradient against the float64
    closed forms at the project's bars; then, with no tolerance, the backward without saved tensors (the forward re-run into the have_saved = 0
    workspace at its exact size) and a repeated call, bit for bit."""
    assert_built_for(shape, precision)
    B = 2 if shape[0] >= 200 else 3
    c = make_case(B, shape, precision)
    want = reference(c)
    got = run_case(c, precision)
    what = "shape %s B=%d" % (shape, B)
    if shape[0] == 512 and precision == "f32":
        r32, r64 = closed_form_in(np.float32, c), closed_form_in(np.float64, c)
        assert all(rel(r64[key], want[key]) < 1e-11 for key in want)
        print("%s: float32 numpy restatement against float64: %s" % (what, ", ".join("%s %.1e" % (key, rel(r32[key], want[key])) for key in want)))
    compare(what, got, want, precision)
    again = run_case(c, precision)
    assert_same_bits(what + ": repeated call", got, again, OUT_KEYS + GRAD_KEYS)
    unsaved = run_case(c, precision, saved=False)
    assert_same_bits(what + ": without saved tensors", got, unsaved, OUT_KEYS + GRAD_KEYS)


REFUSED_PAIRS = [(s, {v: k for k, v in ac.PRECISIONS.items()}[p]) for s, p in ac.REFUSED]


@pytest.mark.parametrize("shape,precision", REFUSED_PAIRS, ids=[shape_id(s, p) for s, p in REFUSED_PAIRS])
def test_attn_refuses_past_the_lds_limit(shape, precision):
    """The pairs past the LDS limit: FIL_ERR_UNSUPPORTED with a text that names the LDS, every guarded output of the refused direction still its
    sentinel (run_attn asserts both); a forward that does run is held to its bar."""
    p = c_plan(shape, precision)
    fwd_refused, bwd_refused = ac.REFUSED[(shape, ac.PRECISIONS[precision])]
    assert (not p.fwd_ok, not p.bwd_ok) == (fwd_refused, bwd_refused), p
    c = make_case(2, shape, precision)
    got = run_case(c, precision, expect=(ac.ERR_UNSUPPORTED if fwd_refused else 0, ac.ERR_UNSUPPORTED if bwd_refused else 0))
    if not fwd_refused:
        compare("refused backward %s: the forward" % (shape,), got, reference(c), precision, keys=("y", "av", "rstd"))
    # the backward without saved tensors is refused the same way (its forward re-run must not start)
    run_case(c, precision, saved=False, expect=(ac.ERR_UNSUPPORTED if fwd_refused else 0, ac.ERR_UNSUPPORTED))


# ------------------------------------------------------------------------------------------------ 2. options
def unfused_reference(c, use_ln=True):
    """float64 autograd over oracle.graph.mult_head_attention, loss <av, dy> + <res, dres>."""
    t = {n: torch.tensor(np.asarray(c[n], np.float64), requires_grad=True) for n in ("x", "Wq", "Wk", "Wr", "gamma", "beta")}
    av, res = G.mult_head_attention(t["x"], t["Wq"], t["Wk"], t["Wr"], t["gamma"], t["beta"], use_ln=use_ln)
    ((av * torch.tensor(c["dy"], dtype=torch.float64)).sum() + (res * torch.tensor(c["dres"], dtype=torch.float64)).sum()).backward()
    g = lambda n: t[n].grad.numpy() if t[n].grad is not None else None
    return dict(y=av.detach().numpy(), res=res.detach().numpy(), dx=g("x"), dWq=g("Wq"), dWk=g("Wk"), dWr=g("Wr"), dgamma=g("gamma"), dbeta=g("beta"))


@pytest.mark.parametrize("precision", list(ac.PRECISIONS))
@pytest.mark.parametrize("shape", ac.OPTION_SHAPES, ids=["F%d-K%d-H%d-A%d" % s for s in ac.OPTION_SHAPES])
def test_attn_options(shape, precision):
    """Wr = NULL; gamma = beta = NULL; the unfused mode (y = LN(av), res_out = x Wr, gradients of both arriving) against autograd over the oracle
    graph; the unfused mode with Wr but without dres_in is FIL_ERR_ARG and writes nothing."""
    assert_built_for(shape, precision)
    B = 3
    c = make_case(B, shape, precision)
    what = "options %s" % (shape,)
    got = run_attn(c["x"], c["Wq"], c["Wk"], None, c["gamma"], c["beta"], c["dy"], precision)
    want = reference(c, use_res=False)
    # (no residual: |got| of a zero reference has no dWr to be measured against; there is none here)
    compare(what + " Wr=NULL", got, want, precision)
    # without the LayerNorm there is no beta to lift the f16 mode's outputs off the ReLU kink: there, the pre-activations within twice the output
    # bar (2 x 5e-3 max|z|: a forward that holds its bar cannot move any other across zero) carry no gradient
    cn = dict(c)
    if precision != "f32":
        _, sv = closed.attn_fwd(c["x"], c["Wq"], c["Wk"], c["Wr"], None, None, use_ln=False, eps=EPS, return_saved=True)
        off_kink = np.abs(sv["z"]) > 2 * BARS[precision][0] * np.abs(sv["z"]).max()
        assert float(off_kink.mean()) > 0.5
        cn["dy"] = (c["dy"] * off_kink).astype(np.float32)
    got = run_attn(cn["x"], cn["Wq"], cn["Wk"], cn["Wr"], None, None, cn["dy"], precision)
    compare(what + " gamma=beta=NULL", got, reference(cn, use_ln=False), precision)
    cu = dict(c, dres=np.random.default_rng(5).standard_normal(c["dy"].shape).astype(np.float32))
    got = run_attn(cu["x"], cu["Wq"], cu["Wk"], cu["Wr"], cu["gamma"], cu["beta"], cu["dy"], precision, dres=cu["dres"], fuse_relu=0)
    compare(what + " unfused", got, unfused_reference(cu), precision)
    unsaved = run_attn(cu["x"], cu["Wq"], cu["Wk"], cu["Wr"], cu["gamma"], cu["beta"], cu["dy"], precision, dres=cu["dres"], fuse_relu=0, saved=False)
    assert_same_bits(what + " unfused without saved tensors", got, unsaved, GRAD_KEYS)
    run_attn(cu["x"], cu["Wq"], cu["Wk"], cu["Wr"], cu["gamma"], cu["beta"], cu["dy"], precision, dres=None, fuse_relu=0, expect=(0, ac.ERR_ARG))


# ------------------------------------------------------------------------------------------------ 3. head-major input
HEAD_MAJOR_SHAPES = {(1, 8): (21, 2, 5), (3, 12): (39, 3, 8), (5, 10): (70, 2, 16), (16, 48): (39, 2, 16)}      # (x_chunk, K) -> (F, H, A)


@pytest.mark.parametrize("precision", list(ac.PRECISIONS))
@pytest.mark.parametrize("x_chunk,K", ac.HEAD_MAJOR)
def test_attn_head_major_input(x_chunk, K, precision):
    """x as a previous layer's [K / c, B, F, c] output (c = x_chunk) == the same call on the materialised head-concat [B, F, K], bit for bit,
    forward and backward, dx coming back head-major: c = 1, 3 and 5 take the scalar load path (c = 3 with K % 4 == 0), c = 16 the vector one."""
    F, H, A = HEAD_MAJOR_SHAPES[(x_chunk, K)]
    assert_built_for((F, K, H, A), precision)
    B = 3
    c = make_case(B, (F, K, H, A), precision)
    xh = np.ascontiguousarray(np.transpose(c["x"].reshape(B, F, K // x_chunk, x_chunk), (2, 0, 1, 3)))
    assert np.array_equal(closed.head_concat(xh), c["x"])
    flat = run_case(c, precision)
    hm = run_attn(xh, c["Wq"], c["Wk"], c["Wr"], c["gamma"], c["beta"], c["dy"], precision, x_chunk=x_chunk)
    hm["dx"] = np.ascontiguousarray(np.transpose(hm["dx"], (1, 2, 0, 3)).reshape(B, F, K))
    assert_same_bits("head-major c=%d K=%d" % (x_chunk, K), flat, hm, OUT_KEYS + GRAD_KEYS)
    compare("head-major c=%d K=%d" % (x_chunk, K), hm, reference(c), precision)


# ------------------------------------------------------------------------------------------------ 4. several samples per workgroup
def periodic(c5, B):
    idx = np.arange(B) % ac.MULTI_PERIOD
    return dict(c5, x=np.ascontiguousarray(c5["x"][idx]), dy=np.ascontiguousarray(c5["dy"][:, idx]))


@pytest.mark.parametrize("precision", list(ac.PRECISIONS))
@pytest.mark.parametrize("shape", list(ac.MULTI_CASES), ids=["NB%d-F%d-K%d-H%d-A%d" % ((nb,) + s) for s, nb in ac.MULTI_CASES.items()])
def test_attn_several_samples_per_workgroup(shape, precision):
    """B = 1025 = five distinct samples 205 times over: more samples than the 1024 / wph persistent workgroups, so some workgroup accumulates dW*
    over two or more samples in registers, prefetches the x of its next sample and reuses its LDS dx tile -- one case per NB, and (17, 8, 8, 4) for
    more than 1024 dgamma / dbeta partial blocks in attn_reduce_kernel.  y and dx of every copy equal the bits of the B = 5 run; the parameter
    gradients are held to 205 x the float64 gradients of the five samples."""
    p = assert_built_for(shape, precision)
    assert p.bwd_nb == ac.MULTI_CASES[shape]
    B, P = ac.MULTI_B, ac.MULTI_PERIOD
    assert B % P == 0 and ac.bwd_grid_bounds(B, p.bwd_wph)[1] < B
    if shape == (17, 8, 8, 4):
        assert ac.bwd_grid_bounds(B, p.bwd_wph)[0] * p.bwd_wph * shape[2] > 1024
    c5 = make_case(P, shape, precision)
    five = run_case(c5, precision)
    want = reference(c5)
    compare("B=5 of %s" % (shape,), five, want, precision)
    got = run_case(periodic(c5, B), precision)
    idx = np.arange(B) % P
    for key in ("y", "av", "rstd"):
        assert np.array_equal(got[key], five[key][:, idx]), "%s of a copy differs from the B = 5 run" % key
    assert np.array_equal(got["dx"], five["dx"][idx]), "dx of a copy differs from the B = 5 run"
    many = {key: want[key] * (B // P) for key in ("dWq", "dWk", "dWr", "dgamma", "dbeta")}
    compare("B=%d of %s" % (B, shape), got, many, precision)


# ------------------------------------------------------------------------------------------------ 5. the reduce kernel
@pytest.mark.parametrize("B", ac.REDUCE_B)
def test_attn_reduce_partial_counts(B):
    """(5, 4, 2, 4): one workgroup per sample and one wave per head, so attn_reduce_kernel sums B partial sets -- around every edge of its four-way
    unrolled loop (wave w adds sets w, w + 16, w + 32, w + 48 while p + 48 < parts, then steps of 16)."""
    p = assert_built_for(ac.REDUCE_SHAPE, "f32")
    assert p.bwd_wph == 1 and ac.bwd_grid_bounds(B, 1) == (B, B)
    c = make_case(B, ac.REDUCE_SHAPE, "f32", seed=B)
    compare("reduce over %d partial sets" % B, run_case(c, "f32"), reference(c), "f32")


@pytest.mark.parametrize("K,H,A", list(ac.REDUCE_N), ids=["n%d" % n for n in ac.REDUCE_N.values()])
def test_attn_reduce_column_blocks(K, H, A):
    """n = K H A = 32, 64 and 65 columns: half a 64-column block, one exactly, one and a single column."""
    assert K * H * A == ac.REDUCE_N[(K, H, A)]
    shape = (5, K, H, A)
    assert_built_for(shape, "f32")
    c = make_case(3, shape, "f32")
    compare("reduce n=%d" % (K * H * A), run_case(c, "f32"), reference(c), "f32")


# ------------------------------------------------------------------------------------------------ 6. value edges
VALUE_IDS = ["F%d-K%d-H%d-A%d" % s for s in ac.VALUE_SHAPES]


@pytest.mark.parametrize("precision", list(ac.PRECISIONS))
@pytest.mark.parametrize("shape", ac.VALUE_SHAPES, ids=VALUE_IDS)
def test_attn_saturated_scores(shape, precision):
    """x scaled until a quarter of |scale q.k| exceeds 200: the sigmoid is exactly 0 or 1 there (exp2 overflows to inf or flushes to 0).  Everything
    stays finite in both precisions (|q|, |k| < 6e4: representable in fp16).  The f32 mode is held to its bars.  The f16 mode is not: a score that
    cancels to O(1) out of terms in the hundreds carries the operands' fp16 rounding, 4.9e-4 sum|q_a k_a| = O(0.1), so its sigmoid is not
    determined by the inputs in that mode; its errors are printed."""
    assert_built_for(shape, precision)
    c = make_case(3, shape, precision)
    _, sv = closed.attn_fwd(c["x"], c["Wq"], c["Wk"], c["Wr"], c["gamma"], c["beta"], eps=EPS, return_saved=True)
    pre = np.abs(np.einsum("mbfa,mbga->mbfg", sv["q"], sv["kk"]) * sv["scale"])
    c["x"] = (c["x"] * np.float32(np.sqrt(200.0 / np.percentile(pre, 75)))).astype(np.float32)
    with np.errstate(over="ignore"):
        _, sv = closed.attn_fwd(c["x"], c["Wq"], c["Wk"], c["Wr"], c["gamma"], c["beta"], eps=EPS, return_saved=True)
    pre = np.abs(np.einsum("mbfa,mbga->mbfg", sv["q"], sv["kk"]) * sv["scale"])
    share = float((pre > 100).mean())
    assert 0.25 < share < 0.9 and max(np.abs(sv["q"]).max(), np.abs(sv["kk"]).max()) < 6e4, share
    got = run_case(c, precision)
    with np.errstate(over="ignore"):          # exp(-score) of the float64 reference overflows to inf beyond 709: its sigmoid is 0 there, as it should be
        want = reference(c)
    what = "saturated %s (%.0f %% of |scores| > 100)" % (shape, 100 * share)
    compare(what, got, want, precision, bars=None if precision == "f32" else (np.inf, np.inf))


@pytest.mark.parametrize("precision", list(ac.PRECISIONS))
@pytest.mark.parametrize("shape", ac.VALUE_SHAPES, ids=VALUE_IDS)
def test_attn_layer_norm_of_one_element(shape, precision):
    """A = 1: the LayerNorm of one element is zero, so y = relu(res + beta); dgamma, dWq and dWk are zero (absolutely: <= 1e-6 max|dWr|) and dx
    comes from the residual alone."""
    F, K, H, _ = shape
    shape = (F, K, H, 1)
    c_plan(shape, precision)
    c = make_case(3, shape, precision)
    want = reference(c)
    assert not np.any(want["dWq"]) and not np.any(want["dWk"]) and not np.any(want["dgamma"]) and not np.any(want["av"])
    res = np.einsum("bfk,kma->mbfa", c["x"].astype(np.float64), c["Wr"].astype(np.float64))
    assert np.allclose(want["y"], np.maximum(res + c["beta"].astype(np.float64), 0), rtol=0, atol=1e-12)
    compare("A=1 %s" % (shape,), run_case(c, precision), want, precision)


@pytest.mark.parametrize("precision", list(ac.PRECISIONS))
@pytest.mark.parametrize("shape", ac.VALUE_SHAPES, ids=VALUE_IDS)
def test_attn_zero_sample_and_zero_gradient_sample(shape, precision):
    """An all-zero sample (its LayerNorm input is a zero row: variance 0) and a sample with dy = 0 inside a batch of four: the bars hold, and the
    sample without a gradient gets dx = 0 exactly (every term of its dx carries a factor of its dz = 0)."""
    assert_built_for(shape, precision)
    c = make_case(4, shape, precision)
    c["x"][1] = 0
    c["dy"][:, 2] = 0
    got = run_case(c, precision)
    compare("zero sample, zero-gradient sample %s" % (shape,), got, reference(c), precision)
    assert not np.any(f32(got["dx"])[2]), "dx of the sample with dy = 0"


@pytest.mark.parametrize("precision", list(ac.PRECISIONS))
@pytest.mark.parametrize("shape", ac.VALUE_SHAPES, ids=VALUE_IDS)
def test_attn_a_nan_stays_in_its_sample(shape, precision):
    """B = 1030 (five distinct samples repeated; every workgroup takes two samples, some three): one sample carries NaN, +Inf and -Inf in x and dy.
    The y, av, rstd and dx rows of EVERY other sample -- the ones the same workgroup takes next, whose x it prefetched beside the bad one and whose
    dx tile reuses the same LDS, included -- equal the bits of the run in which that sample is clean.  (The parameter gradients are legitimately
    NaN and are not compared.)"""
    p = assert_built_for(shape, precision)
    B = ac.NAN_B
    assert ac.bwd_grid_bounds(B, p.bwd_wph)[1] <= B // 2
    c = periodic(make_case(ac.MULTI_PERIOD, shape, precision), B)
    clean = run_case(c, precision)
    bad = 3          # workgroup 3's first sample in every possible grid: its later samples follow the NaN through the same registers and LDS
    c["x"][bad, 0, 0], c["x"][bad, -1, -1], c["x"][bad, shape[0] // 2, 1] = np.nan, np.inf, -np.inf
    c["dy"][0, bad, 0, 0], c["dy"][-1, bad, -1, -1] = np.nan, -np.inf
    got = run_case(c, precision)
    others = np.arange(B) != bad
    for key in ("y", "av", "rstd"):
        assert np.array_equal(got[key][:, others], clean[key][:, others]), "%s of a clean sample changed" % key
    assert np.array_equal(got["dx"][others], clean["dx"][others]), "dx of a clean sample changed"
    assert not np.array_equal(got["av"][:, bad], clean["av"][:, bad]), "the bad sample was not processed"


@pytest.mark.parametrize("precision", list(ac.PRECISIONS))
def test_attn_empty_batch(precision):
    """B = 0: FIL_OK, dWq / dWk / dWr / dgamma / dbeta zeroed, no other store (run_attn asserts y, av, rstd and dx untouched and every guard)."""
    shape = ac.VALUE_SHAPES[0]
    c = make_case(2, shape, precision)
    got = run_case(c, precision, B=0)
    for key in ("dWq", "dWk", "dWr", "dgamma", "dbeta"):
        assert not np.any(got[key]), key + " is not zeroed (bits)"


# ------------------------------------------------------------------------------------------------ 7. the table itself
def test_the_tables_cover_what_they_claim():
    """Without a launch: every (case, precision) pair of the issue's table either runs or is refused, none both; the cases reach every NB x NC of the
    backward menu in both precisions and every (wph, dx image) at NB >= 13."""
    ran = set(SHAPE_PAIRS)
    refused = set(REFUSED_PAIRS)
    assert not ran & refused
    seen, forms = set(), set()
    for shape, precision in SHAPE_PAIRS:
        p = c_plan(shape, precision)
        assert p.fwd_ok and p.bwd_ok
        seen.add((p.bwd_nb, ac.cdiv(shape[1], 16), precision))
        if p.bwd_nb >= 13:
            forms.add((p.bwd_wph, p.bwd_dx_lds))
    if not ac.knobs_set():
        assert len(seen) == 4 * 4 * 2 and len(forms) == 4, (sorted(seen), sorted(forms))
