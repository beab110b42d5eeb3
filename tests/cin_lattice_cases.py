"""CIN inputs on an integer lattice, the conditions they guarantee and the table of cases (TEST INFRASTRUCTURE: numpy only, no GPU, no
library).  tests/test_cin_lattice_host.py checks every condition stated here for every case of the table; tests/test_cin_lattice_gpu.py
relies on them to hold every CIN path to the fp64 oracle bit for bit, element for element.

The construction.  x is in {-1, 0, 1}, every weight is 0 or +-1 at sparse positions, the biases are integers in [-2, 2], dense_w is +-1,
g is +-1 or +-2.  Then
  * every product and every partial sum of every kernel is an integer (a multiple of 1/2 in the pair-symmetric kernels, whose weight
    W[(h,f)] + W[(f,h)] is halved where an even F meets a pair from both ends, 2d == F), so an fp32 sum whose terms' absolute values
    add up to less than 2^24 (2^23 for the halves) is exact in ANY order: abs_bound() evaluates the net on the absolute values of
    every input, which bounds every partial sum of every summation order;
  * every value the one-plane bf16 kernels (csrc/cin_qsplit.h, NP = 1) round -- operands() lists them -- is already a bf16 number, so
    their single MFMA per product computes the same products as the exact kernels, and the split mode's five further MFMAs add
    products of zero pieces.
Every path must then return the fp64 oracle's value in every element.

The densities follow from the shape (lattice_case): W_1 has about c1 = 8 entries per column; the deeper W_l have e_l expected entries
per ROW (e = 1, the last layer's from e_last()), because the magnitude of G1 = dP_1 + dP_2 S + dP_3 R does not depend on the widths:
var R = 0.72 F^2 e_2 e_3, var S = 0.85 F e_2, and G1 has to stay within the 8 significant bits of bf16 (|G1| <= 256 or even).  Narrow
nets are then dense and wide ones sparse.  Fix-ups after the draw (they add entries, never values off the lattice): every pair slot of
W1s and of Ts nonzero in some column, no empty column, every field nonzero in every block of 32 rows.
"""
import collections

import numpy as np

F32, F64 = np.float32, np.float64
TAIL_ALWAYS = 64          # fil.h FIL_CIN_TAIL_ALWAYS
EXACT_BELOW = 2.0 ** 24   # |partial sums| of integers below this are exact in fp32
HALF_BELOW = 2.0 ** 23    # ... of multiples of 1/2
HEAD_TENSORS = ("out", "ddw", "ddb")   # the only tensors a case may exempt from bit equality, and only with output_dim = 1


def is_bf16(v):
    """True where every value is a bf16 number: it is an fp32 number and the low 16 bits of its fp32 pattern are zero."""
    v = np.asarray(v, F64)
    f = v.astype(F32)
    if not np.array_equal(f.astype(F64), v):
        return False
    return not np.any(f.view(np.uint32) & np.uint32(0xFFFF))


def to_bf16(v):
    """float32 values rounded to the nearest bf16 number, ties to even (what v_cvt_pk_bf16_f32 does), returned as float32."""
    u = np.ascontiguousarray(v, dtype=F32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(F32)


def rows_of(x):
    """x [B,F,K] -> the kernels' rows [M = B*K, F], m = b*K + k."""
    x = np.asarray(x, F64)
    return x.transpose(0, 2, 1).reshape(-1, x.shape[1])


def sym_weight(W, F):
    """cin_sym_weight (csrc/cin_split.h) for every slot: W [F*F, H] -> [F, F//2 + 1, H], slot (h, d) = W[(h,f)] + W[(f,h)] with
    f = (h + d) mod F; the diagonal (d = 0) once; half the sum where 2d == F."""
    W3 = np.asarray(W, F64).reshape(F, F, -1)
    h = np.arange(F)[:, None]
    d = np.arange(F // 2 + 1)[None, :]
    f = (h + d) % F
    out = W3[h, f] + W3[f, h]
    out[:, 0] = W3[h[:, 0], h[:, 0]]
    if F % 2 == 0:
        out[:, F // 2] *= 0.5
    return out


def quad_T(W2, W3, F):
    """T[(f',f),h] = sum_n W_2[(h,f'),n] wsum_3[(n,f)], wsum_3[c] = sum_n W_3[c,n] (csrc/cin_qtail.h) -> [F*F, H_1]."""
    W2 = np.asarray(W2, F64)
    H2 = W2.shape[1]
    ws3 = np.asarray(W3, F64).sum(1).reshape(H2, F)
    T = np.einsum("hpn,nf->pfh", W2.reshape(-1, F, H2), ws3)
    return T.reshape(F * F, -1)


def dP_of(case, output_dim):
    """dP [B, L*K]: g[b] dense_w[jK+k] with the Dense(1) head, g itself without."""
    g = np.asarray(case["g"], F64)
    return g @ np.asarray(case["dense_w"], F64).T if output_dim == 1 else g


def operands(case, output_dim):
    """Three-layer case -> the fp64 values of every operand family the one-plane kernels round (split_planes<1>):
    P      [M, F, F//2+1]  x[m,h] x[m,(h+d) mod F], the forward's and the weight gradients' generated operand
    W1s Ts [F, F//2+1, H1] the pair weights (sym_weight) of W_1 and of T
    x1     [M, H1]         the first map
    G1     [M, H1]         dP_1 + dP_2 S + dP_3 R
    dPLx1  [M, H1]         dP_3[m] x1[m,:]
    xe     [M, F]          xe[h] xe[f] with the ones column as one factor (the single-field rows)
    PdPL PdPp xedPp        the generated operand times dP_3[m] or dP_2[m]
    """
    assert len(case["Ws"]) == 3
    x = np.asarray(case["x"], F64)
    B, F, K = x.shape
    xr = rows_of(x)
    W1, W2, W3 = (np.asarray(w, F64) for w in case["Ws"])
    H1 = W1.shape[1]
    T = quad_T(W2, W3, F)
    idx = (np.arange(F)[:, None] + np.arange(F // 2 + 1)[None, :]) % F
    P = xr[:, :, None] * xr[:, idx]
    Z = (xr[:, :, None] * xr[:, None, :]).reshape(-1, F * F)
    x1 = Z @ W1 + np.asarray(case["bs"][0], F64)
    R = Z @ T
    S = xr @ W2.sum(1).reshape(H1, F).T
    dP = dP_of(case, output_dim).reshape(B, 3, K).transpose(0, 2, 1).reshape(-1, 3)   # [M, 3]
    G1 = dP[:, 0:1] + dP[:, 1:2] * S + dP[:, 2:3] * R
    return dict(P=P, W1s=sym_weight(W1, F), Ts=sym_weight(T, F), x1=x1, G1=G1, dPLx1=dP[:, 2:3] * x1, xe=xr,
                PdPL=P * dP[:, 2:3, None], PdPp=P * dP[:, 1:2, None], xedPp=xr * dP[:, 1:2], T=T.reshape(F, F, H1), R=R, S=S)


OPERAND_FAMILIES = ("P", "W1s", "Ts", "x1", "G1", "dPLx1", "xe", "PdPL", "PdPp", "xedPp")


def rows_oracle(case, output_dim):
    """The fp64 oracle as plain matrix products over the rows m (the "einsum restatement": Z_l = x^{l-1} (x) x materialised per layer,
    as oracle/graph.py does): dict(out, dx, dW, db, ddw, ddb), the layout of tests.test_gpu_parity._graph_oracle_cin.  It follows
    oracle/closed.py's recurrences line by line and the host test holds it equal to closed.cin_fwd / cin_bwd; it exists because BLAS
    runs M = 3072 rows in a second where the closed form's batched einsum takes a minute."""
    x = np.asarray(case["x"], F64)
    B, F, K = x.shape
    xr = rows_of(x)
    M = xr.shape[0]
    Ws = [np.asarray(w, F64) for w in case["Ws"]]
    L = len(Ws)
    pres, Zs, pools = [xr], [], []
    for W, b in zip(Ws, case["bs"]):
        Z = (pres[-1][:, :, None] * xr[:, None, :]).reshape(M, -1)
        Zs.append(Z)
        pres.append(Z @ W + np.asarray(b, F64))
        pools.append(pres[-1].sum(1).reshape(B, K))
    P = np.concatenate(pools, -1)
    g = np.asarray(case["g"], F64)
    if output_dim == 1:
        out = P @ np.asarray(case["dense_w"], F64) + np.asarray(case["dense_b"], F64)
        ddw, ddb = P.T @ g, g.sum(0)
    else:
        out, ddw, ddb = P, None, None
    dP = dP_of(case, output_dim).reshape(B, L, K).transpose(0, 2, 1).reshape(M, L)
    dxr = np.zeros_like(xr)
    dW, db = [None] * L, [None] * L
    Gx = None
    for l in range(L - 1, -1, -1):
        G = np.repeat(dP[:, l:l + 1], Ws[l].shape[1], 1)
        if Gx is not None:
            G = G + Gx
        db[l] = G.sum(0)
        dW[l] = Zs[l].T @ G
        dZ = (G @ Ws[l].T).reshape(M, -1, F)
        Gx = np.einsum("mhf,mf->mh", dZ, xr)
        dxr += np.einsum("mhf,mh->mf", dZ, pres[l])
    dxr += Gx
    return dict(out=out, dx=dxr.reshape(B, K, F).transpose(0, 2, 1).copy(), dW=dW, db=db, ddw=ddw, ddb=ddb)


def abs_case(case):
    """The case with every input replaced by its absolute value."""
    a = lambda v: np.abs(np.asarray(v))
    return dict(x=a(case["x"]), Ws=[a(w) for w in case["Ws"]], bs=[a(b) for b in case["bs"]], dense_w=a(case["dense_w"]),
                dense_b=a(case["dense_b"]), g=a(case["g"]))


def abs_bound(case, output_dim):
    """The oracle's outputs and gradients on abs_case(case): every partial sum of every summation order of the real case is at most the
    matching entry in absolute value."""
    return rows_oracle(abs_case(case), output_dim)


def flat(res):
    """dict of an oracle / a run -> [(name, array)] over every tensor that is there."""
    out = [("out", res["out"]), ("dx", res["dx"])]
    out += [("dW%d" % l, w) for l, w in enumerate(res["dW"])] + [("db%d" % l, b) for l, b in enumerate(res["db"])]
    if res.get("ddw") is not None:
        out += [("ddw", res["ddw"]), ("ddb", res["ddb"])]
    return out


def over_the_bound(case, output_dim):
    """Names of the tensors whose abs_bound reaches 2^24: they cannot be promised bit for bit."""
    return tuple(n for n, v in flat(abs_bound(case, output_dim)) if float(np.max(v, initial=0.0)) >= EXACT_BELOW)


# ---------------------------------------------------------------------------------------------------------------- the builder
def e_last(F):
    """Expected entries per row of the last layer's weights: 0.8, less where F is large, so that sigma(G1 / dP) stays near 19
    (0.85 F e_2 + 0.72 F^2 e_2 e_3 <= 350 at e_2 = 1) and |G1| <= 2 * 5.5 sigma stays inside bf16's 8 bits."""
    return min(0.8, (350.0 - 0.85 * F) / (0.72 * F * F))


def _sparse_pm1(rng, shape, density):
    return np.where(rng.random(shape) < density, rng.choice([-1.0, 1.0], shape), 0.0)


def _no_empty_column(rng, W):
    for n in np.flatnonzero(~W.any(0)):
        W[rng.integers(W.shape[0]), n] = rng.choice([-1.0, 1.0])


def _cover_w1s(rng, W1, F):
    """Every pair slot (h, d) of sym_weight(W1) nonzero in some column: an uncovered pair gets one entry, in one orientation, in a
    column where it has none."""
    for _ in range(8):
        s = sym_weight(W1, F)
        miss = np.argwhere(~s.any(2))
        if len(miss) == 0:
            return
        for h, d in miss:
            f = (h + d) % F
            a, b = ((h, f), (f, h))[rng.integers(2)]
            free = np.flatnonzero((W1[h * F + f] == 0) & (W1[f * F + h] == 0))
            n = rng.choice(free) if len(free) else rng.integers(W1.shape[1])
            W1[a * F + b, n] = rng.choice([-1.0, 1.0])
    raise AssertionError("W1s: pair slots left uncovered")


def _cover_ts(rng, W2, W3, F):
    """Every pair slot of sym_weight(T) nonzero in some column h: first every field f gets a nonzero wsum_3[(n,f)] for some n, then an
    uncovered pair (f', f) gets one entry W_2[(h,f'),n] at such an n."""
    H2 = W2.shape[1]
    H1 = W2.shape[0] // F
    for f in range(F):
        if not W3.sum(1).reshape(H2, F)[:, f].any():
            c = rng.integers(H2) * F + f
            W3[c] = 0.0
            W3[c, rng.integers(W3.shape[1])] = rng.choice([-1.0, 1.0])
    ws3 = W3.sum(1).reshape(H2, F)
    missing = lambda: np.argwhere(~sym_weight(quad_T(W2, W3, F), F).any(2))
    miss = missing()
    for _ in range(64 * F * F):
        if len(miss) == 0:
            return
        h0, d = miss[rng.integers(len(miss))]
        fp, f = ((h0, (h0 + d) % F), ((h0 + d) % F, h0))[rng.integers(2)]
        at = (rng.integers(H1) * F + fp, rng.choice(np.flatnonzero(ws3[:, f])))
        old = W2[at]
        W2[at] = rng.choice([-1.0, 1.0])
        now = missing()
        if len(now) < len(miss):      # (an entry of W_2 feeds a whole row of T: keep it only if it uncovers no more than it covers)
            miss = now
        else:
            W2[at] = old
    raise AssertionError("Ts: pair slots left uncovered")


def lattice_case(B, F, K, H, output_dim=2, seed=0, zeros=0.15, c1=8.0, e_mid=1.0, e_end=None):
    """A CIN case on the lattice: the dict of ml_function_amd.synth.cin_case (x [B,F,K], Ws, bs, dense_w [L*K,1], dense_b [1], g: [B,1]
    with the Dense(1) head, [B, L*K] without), float32, for any L = len(H) >= 1.
    zeros  fraction of x that is 0 (the rest +-1)           c1     expected entries per column of W_1
    e_mid  expected entries per row of W_2 .. W_{L-1}       e_end  ... of W_L (default e_last(F)); densities stop at 1/2."""
    H = list(H)
    L = len(H)
    rng = np.random.default_rng([seed, B, F, K, output_dim] + H)
    x = np.where(rng.random((B, F, K)) < zeros, 0.0, rng.choice([-1.0, 1.0], (B, F, K)))
    xr = x.transpose(0, 2, 1).reshape(-1, F)          # a view: the fix-up below writes x
    for lo in range(0, B * K, 32):                    # every field nonzero in every block of 32 rows
        for f in np.flatnonzero(~xr[lo:lo + 32].any(0)):
            m = lo + rng.integers(min(32, B * K - lo))
            x[m // K, f, m % K] = rng.choice([-1.0, 1.0])
    Ws, bs, hp = [], [], F
    for l, h in enumerate(H):
        if l == 0:
            dens = c1 / (F * F)
        else:
            dens = (e_mid if l < L - 1 else (e_last(F) if e_end is None else e_end)) / h
        Ws.append(_sparse_pm1(rng, (hp * F, h), min(0.5, dens)))
        bs.append(rng.integers(-2, 3, h).astype(F64))
        hp = h
    _cover_w1s(rng, Ws[0], F)
    if L == 3:
        _cover_ts(rng, Ws[1], Ws[2], F)
    for W in Ws:
        _no_empty_column(rng, W)
    dense_w = rng.choice([-1.0, 1.0], (L * K, 1))
    dense_b = rng.integers(-2, 3, 1).astype(F64)
    g = rng.choice([-2.0, -1.0, 1.0, 2.0], (B, 1) if output_dim == 1 else (B, L * K))
    f = lambda a: np.ascontiguousarray(a, dtype=F32)
    return dict(x=f(x), Ws=[f(w) for w in Ws], bs=[f(b) for b in bs], dense_w=f(dense_w), dense_b=f(dense_b), g=f(g))


# ---------------------------------------------------------------------------------------------------------------- the case table
def jt_sym(F):
    """cin_jt_sym (csrc/cin_launch.h): steps per h of the pair-symmetric kernels."""
    return ((F // 2 + 2) // 2 + 1) // 2 * 2


def dz2_b_accepts(F):
    """cin_launch_dz2_b's rule (csrc/cin_qsplit.hip): the two-pass data-gradient kernel on bf16 planes takes JT >= 4 and
    F >= cin_dz_h_per_period(JT) + 2 JT (blocks of four slots); every other shape keeps the exact dZ kernel inside the bf16 modes.
    cin_dz_h_per_period(JT) = 16 (JT / gcd(16, JT)) / JT (csrc/cin_launch.h).  The edges are F = 11|12 (JT 4) and 19|20 (JT 6)."""
    JT = jt_sym(F)
    hpp = 16 * (JT // np.gcd(16, JT)) // JT
    return bool(JT >= 4 and F >= hpp + 2 * JT)


Case = collections.namedtuple("Case", "group B F K H output_dim seeds prec exempt opts")
Case.id = property(lambda c: "%s-B%d-F%d-K%d-H%s-od%d" % (c.group, c.B, c.F, c.K, "x".join(map(str, c.H)), c.output_dim))
Case.L = property(lambda c: len(c.H))
Case.M = property(lambda c: c.B * c.K)
Case.dz2_b = property(lambda c: c.L == 3 and c.prec == "bf16" and dz2_b_accepts(c.F))


def _case(group, B, F, K, H, output_dim=2, prec="bf16", seeds=(0, 1), exempt=(), **opts):
    """prec: what cin_precision_used(B, F, K, H, mode=TAIL_ALWAYS, precision="bf16") must say; exempt: the head tensors of an
    output_dim = 1 case whose abs_bound reaches 2^24 (compared at the project's 1e-5 bar instead of bit for bit)."""
    return Case(group, B, F, K, tuple(H), output_dim, tuple(seeds), prec, tuple(exempt), opts)


H3 = (128, 128, 128)
WIDE = (128, 130, 8)      # a layer wider than 128: HSmax = 256, so 3F + 3 <= HSmax holds up to F = 47
TINY = dict(zeros=0.0)    # fewer rows than a block of 32: no zeros in x, or too many gradient entries are structurally zero
CASES = []
# F sweep (K = 8, M = 136 rows, pooled output): JT 2, 4, 6, 8, 10, 12 and both sides of cin_launch_dz2_b's rule
for _F in (2, 7, 8, 11, 12, 15, 16, 19, 20, 23, 24, 31, 32, 39, 40, 41):
    CASES.append(_case("F", 17, _F, 8, H3))
CASES += [_case("F", 17, 42, 8, WIDE), _case("F", 17, 47, 8, WIDE),        # JT 12 past F = 41: the split and bf16 kernels run
          _case("F", 17, 42, 8, H3, prec="f32"),                           # 3F + 3 > 128: no merged launches
          _case("F", 17, 48, 8, WIDE, prec="f32")]                         # JT 14: off the split menu
# width sweep
for _F in (12, 39):
    for _H in ((100, 37, 9), (3, 2, 2), (128, 200, 12), (64, 48, 8)):
        CASES.append(_case("width", 17, _F, 8, _H))
# row sweep: one row, both sides of the 32-row wave and the 128-row workgroup, odd K, K of two waves, several 16-row steps per split
# of cin_dwqb_plan (M = 3072) and a short last split (M = 3088)
for _F in (12, 39):
    for _B, _K in ((1, 1), (31, 1), (33, 1), (127, 1), (129, 1), (7, 5), (3, 64), (17, 8), (192, 16), (193, 16)):
        if _B * _K < 32:
            CASES.append(_case("rows", _B, _F, _K, H3, seeds=(0, 1, 2, 3), **TINY))
        else:
            CASES.append(_case("rows", _B, _F, _K, H3, seeds=(0,) if _B * _K > 1024 else (0, 1)))
# Dense(1) head: folded into the forward's epilogue (K a power of two <= 32) or its own kernel
for _F in (12, 39):
    for _K in (8, 16, 32, 5, 64):
        # (F = 39, K = 64: 192 pooled columns of up to 1.1e5 each reach 2^24 in `out`; every other head case is exact in full)
        CASES.append(_case("head", 6, _F, _K, H3, output_dim=1, exempt=("out",) if (_F, _K) == (39, 64) else ()))
# other depths (exact modes only): general kernels, the last-layer shortcut, the fused tail under two general layers
for _F in (5, 13, 39):
    for _H in ((12,), (10, 7), (9, 8, 7, 6)):
        CASES.append(_case("depth", 9, _F, 8, _H, prec="f32"))
del _F, _H, _B, _K

_BUILT = {}


def build(case, seed):
    """The inputs of one (case, seed), built once."""
    key = (case.id, seed)
    if key not in _BUILT:
        _BUILT[key] = lattice_case(case.B, case.F, case.K, case.H, case.output_dim, seed, **case.opts)
    return _BUILT[key]
